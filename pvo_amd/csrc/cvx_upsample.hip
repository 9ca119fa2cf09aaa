// cvx_upsample.hip — convex 8x upsampling (droid_net.py:23-37, `cvx_upsample`) and its vector-Jacobian product.
//
//   out[b][8y+dy][8x+dx][d] = sum_k softmax_k(mask[b][64k + 8dy + dx][y][x]) * data[b][y+ky-1][x+kx-1][d],   k = 3 ky + kx,
// neighbours outside the map are zero (F.unfold(padding = 1)) and the weights are not renormalised there.
//
// An HBM-bound gather: per coarse pixel 576 logits and 9 neighbours in, 64 D values out.  Two mask layouts:
//   channels-last [B,H,W,576] (what pvo_update_operator writes): a lane owns (pixel, dy); per tap it reads ONE 16-byte piece -
//     dx = 0..7 of a 16-bit mask, 4 resp. 2 values of an fp32 / fp64 one - and writes the matching contiguous piece of one output
//     row; the 8 x 8 lanes of a wave are 8 neighbouring pixels x 8 dy, so a wave reads 8 x 128 contiguous bytes per tap and fills
//     eight 256-byte runs of output rows (fp16 mask, D = 1);
//   planar [B,576,H,W] (the PyTorch module's): a lane owns a pixel, the 64 lanes of a wave are 64 consecutive pixels of the
//     flattened plane, so every logit load is one contiguous run per wave; a wave takes dy = w and w + 4 and writes 8 D contiguous
//     values per lane, the lanes of a map row side by side: runs of 32 D W bytes.
// Arithmetic (A = fp32, or fp64 for fp64 operands): logits converted exactly, m = max_k, e_k = exp(l_k - m), s = sum e_k and
// acc_d = sum e_k nbr_k,d in tap order 0..8, out_d = acc_d / s: one division, one rounding on store.  No atomics anywhere: the same
// operands give the same bits.
//
// Backward (weights recomputed from the logits, nothing of the forward is kept):
//   gmask_k   = w_k * sum_d gout_d (nbr_k,d - out_d)                            same lanes as the forward
//   gdata[y][x][d] = sum over the nine coarse pixels q whose tap k lands on (y, x) of P[q][k][d],
//   P[q][k][d] = sum over the 64 fine pixels of q of w_k gout_d                 per lane over dx, then over dy through LDS in index order
// P goes through the caller's scratch ([B,H,W,9,D], 1.6 % of the mask) and a second launch GATHERS it: every gdata element is owned by one
// lane and summed in tap order.
#include "common.h"
#include <math.h>

namespace {

template <typename M> struct MaskElem { using store_t = typename Elem<M>::store_t; };
template <> struct MaskElem<double> { using store_t = double; };

template <typename A, typename M>
__device__ __forceinline__ A logit(typename MaskElem<M>::store_t v) {
  if constexpr (sizeof(M) == 8) return static_cast<A>(v);
  else return static_cast<A>(Elem<M>::to_f32(v));
}

__device__ __forceinline__ float cvx_exp(float x) { return expf(x); }
__device__ __forceinline__ double cvx_exp(double x) { return exp(x); }

// one lane's place: the coarse pixel it owns and the fine rows (dy = dy0, dy0 + dystep, ... < 8) it computes
struct Place { long long P; int b, y, x, dy0, dystep; bool valid; };

template <bool PLANAR>
__device__ __forceinline__ Place place(long long npix, int HW, int W) {
  Place p;
  if constexpr (PLANAR) {
    p.P = static_cast<long long>(blockIdx.x) * 64 + (threadIdx.x & 63);
    p.dy0 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); p.dystep = 4;      // (uniform over the wave, and known to be)
  } else {
    p.P = (static_cast<long long>(blockIdx.x) * 32 + (threadIdx.x >> 6) * 8) + (threadIdx.x & 7);
    p.dy0 = (threadIdx.x >> 3) & 7; p.dystep = 8;
  }
  p.valid = p.P < npix;
  const long long Pc = p.valid ? p.P : 0;
  p.b = static_cast<int>(Pc / HW);
  const int r = static_cast<int>(Pc - static_cast<long long>(p.b) * HW);
  p.y = r / W; p.x = r - p.y * W;
  return p;
}

// the nine zero-padded neighbours of (y, x) in image `img` of data [.,H,W,D]
template <typename R, typename A, int D>
__device__ __forceinline__ void load_nbrs(const R* __restrict__ img, int y, int x, int H, int W, A (&nbr)[9][D]) {
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
    const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
#pragma unroll
    for (int d = 0; d < D; ++d)
      nbr[k][d] = in ? static_cast<A>(img[(static_cast<size_t>(yy) * W + xx) * D + d]) : A(0);
  }
}

// planar masks: element offset of the lane's pixel inside plane 0 of its image, from the start of the mask
__device__ __forceinline__ unsigned planar_lane_offset(const Place& p, int HW) {
  return static_cast<unsigned>(p.b) * 576u * static_cast<unsigned>(HW) + static_cast<unsigned>(p.P - static_cast<long long>(p.b) * HW);
}

// logits of taps 0..8 for dx = c0 .. c0 + CH - 1 of fine row dy.  Channels-last: CH elements are one 16-byte piece.
template <typename M, typename A, int CH, bool PLANAR>
__device__ __forceinline__ void load_logits(const typename MaskElem<M>::store_t* __restrict__ mask, const Place& p, int HW, int dy, int c0,
                                            A (&lg)[9][CH]) {
  using S = typename MaskElem<M>::store_t;
  if constexpr (PLANAR) {
    // plane pointers are uniform over the wave (dy is: place()), the lane adds its 32-bit pixel offset (the host checks the range)
    const unsigned lane = planar_lane_offset(p, HW);
    const S* planes = mask + static_cast<size_t>(8 * dy + c0) * HW;
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
      for (int j = 0; j < CH; ++j)
        lg[k][j] = logit<A, M>((planes + static_cast<size_t>(64 * k + j) * HW)[lane]);
  } else {
    static_assert(CH * sizeof(S) == 16, "a channels-last piece is 16 bytes");
    const S* base = mask + static_cast<size_t>(p.P) * 576 + 8 * dy + c0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      union { uint4 q; S e[CH]; } u;
      u.q = *reinterpret_cast<const uint4*>(base + 64 * k);
#pragma unroll
      for (int j = 0; j < CH; ++j) lg[k][j] = logit<A, M>(u.e[j]);
    }
  }
}

// N contiguous values, 16-byte aligned, as 16-byte pieces
template <typename R, int N>
__device__ __forceinline__ void store_run(R* __restrict__ dst, const R (&v)[N]) {
  constexpr int PER = 16 / sizeof(R);
  static_assert(N % PER == 0, "whole 16-byte pieces");
#pragma unroll
  for (int i = 0; i < N / PER; ++i) {
    union { uint4 q; R e[PER]; } u;
#pragma unroll
    for (int j = 0; j < PER; ++j) u.e[j] = v[i * PER + j];
    reinterpret_cast<uint4*>(dst)[i] = u.q;
  }
}
template <typename R, int N>
__device__ __forceinline__ void load_run(const R* __restrict__ src, R (&v)[N]) {
  constexpr int PER = 16 / sizeof(R);
  static_assert(N % PER == 0, "whole 16-byte pieces");
#pragma unroll
  for (int i = 0; i < N / PER; ++i) {
    union { uint4 q; R e[PER]; } u;
    u.q = reinterpret_cast<const uint4*>(src)[i];
#pragma unroll
    for (int j = 0; j < PER; ++j) v[i * PER + j] = u.e[j];
  }
}

// dx values per step: channels-last one 16-byte piece of the mask; planar all eight in fp32 (whole 32 D-byte runs per lane), two in fp64
template <typename M, typename A, bool PLANAR>
constexpr int chunk_fwd() { return PLANAR ? (sizeof(A) == 4 ? 8 : 2) : static_cast<int>(16 / sizeof(typename MaskElem<M>::store_t)); }

template <typename M, typename R, int D, bool PLANAR>
__global__ __launch_bounds__(256) void pvo_cvx_upsample_fwd_kernel(const typename MaskElem<M>::store_t* __restrict__ mask,
                                                                   const R* __restrict__ data, R* __restrict__ out,
                                                                   const int64_t* __restrict__ in_rows, const int64_t* __restrict__ out_rows,
                                                                   int n_in, int n_out, long long npix, int H, int W) {
  using A = R;
  constexpr int CH = chunk_fwd<M, A, PLANAR>();
  const int HW = H * W;
  const Place p = place<PLANAR>(npix, HW, W);
  if (!p.valid) return;
  const long long rin = in_rows ? in_rows[p.b] : p.b, rout = out_rows ? out_rows[p.b] : p.b;
  if (rin < 0 || rin >= n_in || rout < 0 || rout >= n_out) return;      // a row table that points outside the buffers writes nothing
  A nbr[9][D];
  load_nbrs<R, A, D>(data + static_cast<size_t>(rin) * HW * D, p.y, p.x, H, W, nbr);
  for (int dy = p.dy0; dy < 8; dy += p.dystep) {
    R* orow = out + ((static_cast<size_t>(rout) * 8 * H + 8 * p.y + dy) * 8 * W + 8 * p.x) * D;
#pragma unroll
    for (int c0 = 0; c0 < 8; c0 += CH) {
      A lg[9][CH];
      load_logits<M, A, CH, PLANAR>(mask, p, HW, dy, c0, lg);
      R o[CH * D];
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        A m = lg[0][j];
#pragma unroll
        for (int k = 1; k < 9; ++k) m = lg[k][j] > m ? lg[k][j] : m;
        A s = 0, acc[D];
#pragma unroll
        for (int d = 0; d < D; ++d) acc[d] = 0;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          const A e = cvx_exp(lg[k][j] - m);
          s += e;
#pragma unroll
          for (int d = 0; d < D; ++d) acc[d] += e * nbr[k][d];
        }
#pragma unroll
        for (int d = 0; d < D; ++d) o[j * D + d] = acc[d] / s;
      }
      store_run<R, CH * D>(orow + c0 * D, o);
    }
  }
}

// backward, first launch: gmask, and P[q][k][d] = sum over q's 64 fine pixels of w_k gout_d into `part` [npix, 9, D]
template <typename R, int D, bool PLANAR>
__global__ __launch_bounds__(256) void pvo_cvx_upsample_bwd_mask_kernel(const R* __restrict__ mask, const R* __restrict__ data,
                                                                        const R* __restrict__ gout, R* __restrict__ gmask,
                                                                        R* __restrict__ part, long long npix, int H, int W) {
  using A = R;
  constexpr int CH = 16 / sizeof(R);
  constexpr int NPL = PLANAR ? 64 : 32, NSLOT = PLANAR ? 4 : 8, J = 9 * D;
  __shared__ A red[NSLOT * J * NPL];
  const int HW = H * W;
  const Place p = place<PLANAR>(npix, HW, W);
  A ps[9][D];
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int d = 0; d < D; ++d) ps[k][d] = 0;
  if (p.valid) {
    A nbr[9][D];
    load_nbrs<R, A, D>(data + static_cast<size_t>(p.b) * HW * D, p.y, p.x, H, W, nbr);
#pragma unroll 1
    for (int dy = p.dy0; dy < 8; dy += p.dystep) {
      const R* grow = gout + ((static_cast<size_t>(p.b) * 8 * H + 8 * p.y + dy) * 8 * W + 8 * p.x) * D;
#pragma unroll
      for (int c0 = 0; c0 < 8; c0 += CH) {
        A lg[9][CH];
        load_logits<R, A, CH, PLANAR>(mask, p, HW, dy, c0, lg);
        R g[CH * D];
        load_run<R, CH * D>(grow + c0 * D, g);
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          A m = lg[0][j];
#pragma unroll
          for (int k = 1; k < 9; ++k) m = lg[k][j] > m ? lg[k][j] : m;
          A s = 0;
#pragma unroll
          for (int k = 0; k < 9; ++k) { lg[k][j] = cvx_exp(lg[k][j] - m); s += lg[k][j]; }
          const A inv = A(1) / s;
          A o[D];
#pragma unroll
          for (int d = 0; d < D; ++d) o[d] = 0;
#pragma unroll
          for (int k = 0; k < 9; ++k) {
            lg[k][j] *= inv;                                           // w_k
#pragma unroll
            for (int d = 0; d < D; ++d) o[d] += lg[k][j] * nbr[k][d];
          }
#pragma unroll
          for (int k = 0; k < 9; ++k) {
            A t = 0;
#pragma unroll
            for (int d = 0; d < D; ++d) {
              t += g[j * D + d] * (nbr[k][d] - o[d]);
              ps[k][d] += lg[k][j] * g[j * D + d];
            }
            lg[k][j] *= t;                                             // gmask_k
          }
        }
        // the gradient goes where the logits came from
        if constexpr (PLANAR) {
          const unsigned lane = planar_lane_offset(p, HW);
          R* planes = gmask + static_cast<size_t>(8 * dy + c0) * HW;
#pragma unroll
          for (int k = 0; k < 9; ++k)
#pragma unroll
            for (int j = 0; j < CH; ++j) (planes + static_cast<size_t>(64 * k + j) * HW)[lane] = lg[k][j];
        } else {
          R* base = gmask + static_cast<size_t>(p.P) * 576 + 8 * dy + c0;
#pragma unroll
          for (int k = 0; k < 9; ++k) store_run<R, CH>(base + 64 * k, lg[k]);
        }
      }
    }
  }
  // P: the lanes of one pixel (its dy slots) summed in slot order
  const int slot = PLANAR ? (threadIdx.x >> 6) : ((threadIdx.x >> 3) & 7);
  const int pl = PLANAR ? (threadIdx.x & 63) : ((threadIdx.x >> 6) * 8 + (threadIdx.x & 7));
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int d = 0; d < D; ++d) red[(slot * J + k * D + d) * NPL + pl] = ps[k][d];
  __syncthreads();
  const long long P0 = static_cast<long long>(blockIdx.x) * NPL;
  for (int i = threadIdx.x; i < NPL * J; i += 256) {
    const int q = i / J, j = i - q * J;
    if (P0 + q >= npix) break;
    A s = red[j * NPL + q];
#pragma unroll
    for (int sl = 1; sl < NSLOT; ++sl) s += red[(sl * J + j) * NPL + q];
    part[static_cast<size_t>(P0 + q) * J + j] = s;
  }
}

// backward, second launch: every gdata element gathers its nine P terms in tap order
template <typename R, int D>
__global__ __launch_bounds__(256) void pvo_cvx_upsample_bwd_data_kernel(const R* __restrict__ part, R* __restrict__ gdata, long long n,
                                                                        int H, int W) {
  const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  const int d = static_cast<int>(i % D);
  const long long P = i / D;
  const int HW = H * W;
  const long long b = P / HW;
  const int r = static_cast<int>(P - b * HW), y = r / W, x = r - y * W;
  R s = 0;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int qy = y - (k / 3 - 1), qx = x - (k % 3 - 1);
    if (qy >= 0 && qy < H && qx >= 0 && qx < W)
      s += part[((static_cast<size_t>(b) * HW + static_cast<size_t>(qy) * W + qx) * 9 + k) * D + d];
  }
  gdata[i] = s;
}

constexpr long long kMaxPixels = 1LL << 27;      // B * H * W: the grids and the 32-bit in-image offsets are sized for this

int check_shape(int B, int H, int W, int D, int mask_channels, int planar) {
  if (B < 0 || H < 0 || W < 0) return PVO_EINVAL;
  if (D != 1 && D != 2) return PVO_EINVAL;
  if (mask_channels != 576) return PVO_EINVAL;
  if (static_cast<long long>(B) * H * W > kMaxPixels) return PVO_EUNSUPPORTED;
  if (planar && static_cast<long long>(B) * H * W * 576 >= (1LL << 31)) return PVO_EUNSUPPORTED;      // 32-bit lane offsets
  return PVO_OK;
}

template <typename M, typename R>
int launch_fwd(const void* data, const void* mask, void* out, const int64_t* in_rows, const int64_t* out_rows, int n_in, int n_out,
               int B, int H, int W, int D, int planar, hipStream_t st) {
  using S = typename MaskElem<M>::store_t;
  const long long npix = static_cast<long long>(B) * H * W;
  const unsigned blocks = static_cast<unsigned>(planar ? (npix + 63) / 64 : (npix + 31) / 32);
  const S* m = static_cast<const S*>(mask);
  const R* x = static_cast<const R*>(data);
  R* o = static_cast<R*>(out);
#define PVO_CVX_FWD(DD, PL) \
  hipLaunchKernelGGL((pvo_cvx_upsample_fwd_kernel<M, R, DD, PL>), dim3(blocks), dim3(256), 0, st, m, x, o, in_rows, out_rows, n_in, n_out, npix, H, W)
  if (D == 1 && planar) PVO_CVX_FWD(1, true);
  else if (D == 1) PVO_CVX_FWD(1, false);
  else if (planar) PVO_CVX_FWD(2, true);
  else PVO_CVX_FWD(2, false);
#undef PVO_CVX_FWD
  PVO_CHECK_LAUNCH();
  return PVO_OK;
}

}  // namespace

// update_exec.hip calls this with the operator's own mask
extern "C" int pvo_cvx_upsample(const void* data, const void* mask, void* out, const int64_t* in_rows, const int64_t* out_rows,
                                int n_in, int n_out, int B, int H, int W, int D, int mask_channels, int mask_planar,
                                int data_dtype, int mask_dtype, void* stream) {
  const int rc = check_shape(B, H, W, D, mask_channels, mask_planar);
  if (rc != PVO_OK) return rc;
  if (B == 0 || H == 0 || W == 0) return PVO_OK;
  if (!data || !mask || !out) return PVO_EINVAL;
  if ((in_rows ? n_in < 0 : n_in < B) || (out_rows ? n_out < 0 : n_out < B)) return PVO_EINVAL;
  if (pvo_misaligned16(mask, out)) return PVO_EINVAL;
  hipStream_t st = pvo_stream(stream);
  if (data_dtype == PVO_F64) {
    if (mask_dtype != PVO_F64) return PVO_EUNSUPPORTED;
    return launch_fwd<double, double>(data, mask, out, in_rows, out_rows, n_in, n_out, B, H, W, D, mask_planar, st);
  }
  if (data_dtype != PVO_F32) return PVO_EUNSUPPORTED;
  return pvo_dispatch<pvo_half, pvo_bf16, float>(mask_dtype, [&](auto tag) -> int {
    using M = decltype(tag);
    return launch_fwd<M, float>(data, mask, out, in_rows, out_rows, n_in, n_out, B, H, W, D, mask_planar, st);
  });
}

extern "C" size_t pvo_cvx_upsample_vjp_scratch_bytes(int B, int H, int W, int D, int dtype) {
  if (B < 0 || H < 0 || W < 0 || (D != 1 && D != 2)) return 0;
  return static_cast<size_t>(B) * H * W * 9 * D * (dtype == PVO_F64 ? 8 : 4) + 16;
}

extern "C" int pvo_cvx_upsample_vjp(const void* data, const void* mask, const void* gout, void* gmask, void* gdata,
                                    int B, int H, int W, int D, int mask_channels, int mask_planar, int dtype,
                                    void* scratch, size_t scratch_bytes, void* stream) {
  const int rc = check_shape(B, H, W, D, mask_channels, mask_planar);
  if (rc != PVO_OK) return rc;
  if (B == 0 || H == 0 || W == 0) return PVO_OK;
  if (!data || !mask || !gout || !gmask || !gdata) return PVO_EINVAL;
  if (pvo_misaligned16(mask, gout, gmask, scratch)) return PVO_EINVAL;
  if (!scratch || scratch_bytes < pvo_cvx_upsample_vjp_scratch_bytes(B, H, W, D, dtype)) return PVO_EWORKSPACE;
  hipStream_t st = pvo_stream(stream);
  return pvo_dispatch<float, double>(dtype, [&](auto tag) -> int {
    using R = decltype(tag);
    const long long npix = static_cast<long long>(B) * H * W;
    const unsigned blocks = static_cast<unsigned>(mask_planar ? (npix + 63) / 64 : (npix + 31) / 32);
    const R *m = static_cast<const R*>(mask), *x = static_cast<const R*>(data), *g = static_cast<const R*>(gout);
    R *gm = static_cast<R*>(gmask), *gd = static_cast<R*>(gdata), *part = static_cast<R*>(scratch);
#define PVO_CVX_BWD(DD, PL) \
  hipLaunchKernelGGL((pvo_cvx_upsample_bwd_mask_kernel<R, DD, PL>), dim3(blocks), dim3(256), 0, st, m, x, g, gm, part, npix, H, W)
    if (D == 1 && mask_planar) PVO_CVX_BWD(1, true);
    else if (D == 1) PVO_CVX_BWD(1, false);
    else if (mask_planar) PVO_CVX_BWD(2, true);
    else PVO_CVX_BWD(2, false);
#undef PVO_CVX_BWD
    PVO_CHECK_LAUNCH();
    const long long n = npix * D;
    const unsigned b2 = static_cast<unsigned>((n + 255) / 256);
    if (D == 1) hipLaunchKernelGGL((pvo_cvx_upsample_bwd_data_kernel<R, 1>), dim3(b2), dim3(256), 0, st, part, gd, n, H, W);
    else hipLaunchKernelGGL((pvo_cvx_upsample_bwd_data_kernel<R, 2>), dim3(b2), dim3(256), 0, st, part, gd, n, H, W);
    PVO_CHECK_LAUNCH();
    return PVO_OK;
  });
}
