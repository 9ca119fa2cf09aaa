// encoder_conv.hip — the per-frame encoders' 3 x 3 and 7 x 7 convolutions on their own tensor layout (contiguous 16-bit NCHW planes),
// on the matrix cores, DETERMINISTIC BY CONSTRUCTION.
//
// The reference's BasicEncoder (VO_Module/droid_slam/modules/extractor.py:116-201) has thirteen of them per network: the 7 x 7 stride-2
// stem (3 -> 32) and twelve 3 x 3 layers at 32, 64 and 128 channels, stride 1 and 2.  The vendor library chooses a kernel per shape from
// timings taken on the box, and some candidates add split-K partial sums with atomics (profiles/r06_encoder_determinism.txt).  Here
//     y[n][co][oy][ox] = epilogue( sum_{ci,ky,kx} w[co][ci][ky][kx] x[n][ci][oy s + ky - p][ox s + kx - p] ),   zero padding,
// 16-bit products accumulated in fp32 on v_mfma_f32_16x16x32_{f16,bf16}; every output element belongs to ONE wave, which adds its K
// products in an order the shape alone fixes (32-channel chunk by chunk, tap by tap): no atomics, no split of K across workgroups or
// waves, nothing that depends on N, on the tile a pixel falls into or on what else runs.
//
// Roles on the MFMA (D[16 x 16] += A[16 x 32] B[32 x 16]): A = FILTER (rows = 16 output channels), B = ACTIVATIONS (columns = 16
// consecutive output pixels of one row).  A lane then holds, of D, one pixel (lane & 15) and four channels (4 (lane >> 4) + r): the 16
// lanes of a channel store 32 contiguous bytes of its plane - the NCHW output needs no transpose through LDS.
//
// K order (A and B agree on it, nothing else matters): a k-step of 32 is ONE TAP x 32 INPUT CHANNELS; lane group kg = lane >> 4 holds
// the 8 channels 8 kg .. 8 kg + 7 of the chunk.
//   filter      pvo_conv_planes_pack re-arranges w once into fragment order, [k-step][Cout / 16][64 lanes][8]: a wave's A fragment is one
//               coalesced 16-byte load per lane (1 KB per wave), straight from global memory / L2 - no LDS for the filter.
//   activations a workgroup stages the halo of its pixel tile, one 32-channel chunk at a time, as tile[kg][halo row][halo column][8
//               channels]: 16 bytes per position, so a B fragment is ONE ds_read_b128.  Staging transposes from planes: a thread reads
//               the 8 channels of one position (8 two-byte loads, each coalesced along W across the threads) and parks them with one
//               ds_write_b128.  For stride 2 the halo columns are stored even columns first, then odd ones, so the 16 pixels of a fragment
//               read 16 CONSECUTIVE positions for every tap, as for stride 1.
//               Bank conflicts: a ds_read_b128 is served in four groups of 16 lanes that mix two kg values ({0-3, 12-15, 20-27}, ...);
//               with the kg blocks a multiple of 256 bytes apart and the 16 positions of a kg contiguous, every group covers the 64 banks
//               exactly once.
//   stem        Cin = 3, 7 x 7, stride 2: K = 147.  A k-group of 8 is one (channel, filter row) and its 7 taps + one zero: 21 groups,
//               padded with zero groups to 24 = 6 k-steps (K = 192).  The staged tile holds, per (channel, halo row, output column), the 8
//               input pixels 2 ox - 3 .. 2 ox + 4 (the eighth as zero): again one ds_read_b128 per fragment.  The padding groups read
//               a zero fragment, not memory.
//
// Tiles.  256 threads = 4 waves; a workgroup owns 16 output columns x 4 RPW output rows x 32 output channels, wave w the rows
// RPW w .. RPW w + RPW - 1: RPW x 2 accumulator tiles (8 or 16 VGPRs).  Per k-step a wave issues 2 filter loads, RPW LDS reads and
// 2 RPW MFMAs.
//   RPW = 2 (8 x 16 pixels)   maps of >= 32768 output pixels over the batch: the stem and the 32-channel layers at 120 x 404 (390
//                             workgroups per image); bandwidth / launch bound, the larger tile reads a halo of 1.4 x instead of 1.7 x.
//   RPW = 1 (4 x 16 pixels)   everything smaller: 60 x 202 x 64 -> 390, 30 x 101 x 128 -> 224 workgroups.  The 1/8-resolution layers
//                             stay parallelism bound (under one workgroup per compute unit); splitting K over the waves of a workgroup
//                             with a fixed-order LDS reduction is the next step there and is NOT done here.
// Resources (hipcc, gfx950, -O3, per instantiation in DESIGN.md section 4, *The encoders' own convolutions*): no scratch, at most
// 49 VGPRs + 24 AGPRs, 7-37 KB of LDS per workgroup.
//
// Epilogue, the operations, order and roundings of pvo_bias_norm_act with norm = 0, every step optional:
//     t = round16(acc);  t = round16(t + bias[co]);  relu_inner;  t = round16(residual + t);  relu_outer.
#include "operand16.h"

namespace {

constexpr int kCoBlock = 32;                                       // output channels per workgroup (2 M-tiles)
constexpr int kStemGroups = 21, kStemSteps = 6;                    // 3 channels x 7 filter rows; ceil(21 / 4) k-steps

template <typename T>
__device__ __forceinline__ void conv_epilogue(const v4f (&acc)[2], const uint16_t* __restrict__ bias, const uint16_t* __restrict__ residual,
                                              uint16_t* __restrict__ y, size_t n, int Cout, int co0, int kg, size_t HWo, size_t pix,
                                              int relu_inner, int relu_outer) {
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = co0 + mt * 16 + 4 * kg + r;
      const size_t o = (n * Cout + co) * HWo + pix;
      float t = pvo_round<T>(acc[mt][r]);
      if (bias) t = pvo_round<T>(t + pvo_val<T>(bias[co]));
      if (relu_inner) t = fmaxf(t, 0.0f);
      if (residual) t = pvo_round<T>(pvo_val<T>(residual[o]) + t);
      if (relu_outer) t = fmaxf(t, 0.0f);
      y[o] = static_cast<uint16_t>(pvo_bits<T>(t));
    }
}

// 3 x 3, padding 1, stride STRIDE; grid (N * tiles_y * tiles_x, Cout / 32)
template <typename T, int STRIDE, int RPW>
__global__ __launch_bounds__(256) void conv3x3_planes_kernel(const uint16_t* __restrict__ x, const u32x4* __restrict__ wf, const uint16_t* __restrict__ bias,
                                                             const uint16_t* __restrict__ residual, uint16_t* __restrict__ y, int Cin, int Cout,
                                                             int H, int W, int Ho, int Wo, int tiles_x, int tiles_y, int relu_inner, int relu_outer) {
  constexpr int TH = 4 * RPW;
  constexpr int HR = (TH - 1) * STRIDE + 3, HC = 15 * STRIDE + 3;   // halo rows / columns (18 or 33 columns)
  constexpr int ODD0 = (HC + 1) / 2;                                // stride 2: first slot of the odd columns
  constexpr int KGP = (HR * HC + 15) & ~15;                         // positions per kg block: a multiple of 16 (256 bytes)
  __shared__ u32x4 tile[4 * KGP];
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, kg = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y;
  const size_t n = blockIdx.x / (tiles_x * tiles_y);
  const int ox0 = tx * 16, oy0 = ty * TH;
  const int cb = blockIdx.y, mtiles = Cout >> 4;
  const size_t HW = static_cast<size_t>(H) * W;
  const uint16_t* xn = x + n * Cin * HW;
  const int nC = Cin >> 5;
  v4f acc[RPW][2];
#pragma unroll
  for (int nt = 0; nt < RPW; ++nt)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) acc[nt][mt] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
  const u32x4* wl = wf + static_cast<size_t>(cb * 2) * 64 + lane;   // + (s * mtiles + mt) * 64
#pragma unroll 1
  for (int cc = 0; cc < nC; ++cc) {
    __syncthreads();                                                // (the previous chunk's fragments have been read)
    for (int i = tid; i < 4 * HR * HC; i += 256) {
      const int g = i / (HR * HC), rem = i - g * (HR * HC);
      const int hr = rem / HC, hc = rem - hr * HC;
      const int iy = oy0 * STRIDE - 1 + hr, ix = ox0 * STRIDE - 1 + hc;
      u32x4 v = u32x4{0u, 0u, 0u, 0u};
      if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
        const uint16_t* p = xn + static_cast<size_t>(cc * 32 + g * 8) * HW + static_cast<size_t>(iy) * W + ix;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = static_cast<uint32_t>(p[(2 * k) * HW]) | (static_cast<uint32_t>(p[(2 * k + 1) * HW]) << 16);
      }
      const int slot = STRIDE == 2 ? ((hc & 1) ? ODD0 + (hc >> 1) : (hc >> 1)) : hc;
      tile[g * KGP + hr * HC + slot] = v;
    }
    __syncthreads();
    const u32x4* ws = wl + static_cast<size_t>(cc) * 9 * mtiles * 64;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int ky = t / 3, kx = t % 3;
      const int slot0 = STRIDE == 2 ? ((kx & 1) ? ODD0 : 0) + (kx >> 1) : kx;
      const u32x4 a0 = ws[(t * mtiles) * 64], a1 = ws[(t * mtiles + 1) * 64];
#pragma unroll
      for (int nt = 0; nt < RPW; ++nt) {
        const int hr = (wave * RPW + nt) * STRIDE + ky;
        const u32x4 b = tile[kg * KGP + hr * HC + slot0 + li];
        acc[nt][0] = pvo_mfma<T>(a0, b, acc[nt][0]);
        acc[nt][1] = pvo_mfma<T>(a1, b, acc[nt][1]);
      }
    }
  }
  const int ox = ox0 + li;
#pragma unroll
  for (int nt = 0; nt < RPW; ++nt) {
    const int oy = oy0 + wave * RPW + nt;
    if (oy < Ho && ox < Wo)
      conv_epilogue<T>(acc[nt], bias, residual, y, n, Cout, cb * kCoBlock, kg, static_cast<size_t>(Ho) * Wo, static_cast<size_t>(oy) * Wo + ox,
                       relu_inner, relu_outer);
  }
}

// the stem: 7 x 7, padding 3, stride 2, Cin = 3
template <typename T, int RPW>
__global__ __launch_bounds__(256) void conv7x7_stem_kernel(const uint16_t* __restrict__ x, const u32x4* __restrict__ wf, const uint16_t* __restrict__ bias,
                                                           const uint16_t* __restrict__ residual, uint16_t* __restrict__ y, int Cout,
                                                           int H, int W, int Ho, int Wo, int tiles_x, int tiles_y, int relu_inner, int relu_outer) {
  constexpr int TH = 4 * RPW, HR = (TH - 1) * 2 + 7;
  __shared__ u32x4 tile[3 * HR * 16];                               // [channel][halo row][output column] x 8 input pixels
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, kg = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y;
  const size_t n = blockIdx.x / (tiles_x * tiles_y);
  const int ox0 = tx * 16, oy0 = ty * TH;
  const int cb = blockIdx.y, mtiles = Cout >> 4;
  const size_t HW = static_cast<size_t>(H) * W;
  const uint16_t* xn = x + n * 3 * HW;
  for (int i = tid; i < 3 * HR * 16; i += 256) {
    const int c = i / (HR * 16), rem = i - c * (HR * 16);
    const int hr = rem >> 4, oc = rem & 15;
    const int iy = oy0 * 2 - 3 + hr, ix0 = (ox0 + oc) * 2 - 3;
    uint32_t e[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int ix = ix0 + j;
      e[j] = (j < 7 && iy >= 0 && iy < H && ix >= 0 && ix < W) ? xn[c * HW + static_cast<size_t>(iy) * W + ix] : 0u;
    }
    tile[i] = u32x4{e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16)};
  }
  __syncthreads();
  v4f acc[RPW][2];
#pragma unroll
  for (int nt = 0; nt < RPW; ++nt)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) acc[nt][mt] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
  const u32x4* wl = wf + static_cast<size_t>(cb * 2) * 64 + lane;
#pragma unroll
  for (int s = 0; s < kStemSteps; ++s) {
    const int g = 4 * s + kg;                                       // this lane's k-group: (channel, filter row), >= 21: zero padding
    const int gc = min(g, kStemGroups - 1);
    const int c = gc / 7, ky = gc - 7 * c;
    const u32x4 a0 = wl[(s * mtiles) * 64], a1 = wl[(s * mtiles + 1) * 64];
#pragma unroll
    for (int nt = 0; nt < RPW; ++nt) {
      const int hr = (wave * RPW + nt) * 2 + ky;
      u32x4 b = tile[(c * HR + hr) * 16 + li];
      if (g >= kStemGroups) b = u32x4{0u, 0u, 0u, 0u};              // (0 x a NaN of a real group would be a NaN)
      acc[nt][0] = pvo_mfma<T>(a0, b, acc[nt][0]);
      acc[nt][1] = pvo_mfma<T>(a1, b, acc[nt][1]);
    }
  }
  const int ox = ox0 + li;
#pragma unroll
  for (int nt = 0; nt < RPW; ++nt) {
    const int oy = oy0 + wave * RPW + nt;
    if (oy < Ho && ox < Wo)
      conv_epilogue<T>(acc[nt], bias, residual, y, n, Cout, cb * kCoBlock, kg, static_cast<size_t>(Ho) * Wo, static_cast<size_t>(oy) * Wo + ox,
                       relu_inner, relu_outer);
  }
}

// w [Cout][Cin][k][k] -> fragment order [k-step][Cout / 16][64 lanes][8]; one thread per packed element
template <int KSIZE>
__global__ void conv_planes_pack_kernel(const uint16_t* __restrict__ w, uint16_t* __restrict__ wf, int Cin, int Cout, long long total) {
  const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int j = static_cast<int>(i & 7), lane = static_cast<int>((i >> 3) & 63);
  const long long f = i >> 9;
  const int mtiles = Cout >> 4;
  const int mt = static_cast<int>(f % mtiles), s = static_cast<int>(f / mtiles);
  const int co = mt * 16 + (lane & 15), kg = lane >> 4;
  uint16_t v = 0;
  if (KSIZE == 3) {
    const int cc = s / 9, t = s - 9 * cc;
    v = w[(static_cast<size_t>(co) * Cin + cc * 32 + kg * 8 + j) * 9 + t];
  } else {
    const int g = 4 * s + kg;
    if (g < kStemGroups && j < 7) v = w[(static_cast<size_t>(co) * 3 + g / 7) * 49 + (g % 7) * 7 + j];
  }
  wf[i] = v;
}

// k-steps of the packed filter
int conv_planes_steps(int ksize, int Cin) { return ksize == 3 ? (Cin / 32) * 9 : kStemSteps; }

}  // namespace

extern "C" int pvo_conv_planes_supported(int ksize, int stride, int Cin, int Cout) {
  if (Cout <= 0 || (Cout % kCoBlock) != 0) return 0;
  if (ksize == 3) return (stride == 1 || stride == 2) && Cin > 0 && (Cin % 32) == 0;
  if (ksize == 7) return stride == 2 && Cin == 3;
  return 0;
}

extern "C" size_t pvo_conv_planes_filter_bytes(int ksize, int Cin, int Cout) {
  if (!pvo_conv_planes_supported(ksize, ksize == 7 ? 2 : 1, Cin, Cout)) return 0;
  return static_cast<size_t>(conv_planes_steps(ksize, Cin)) * 32 * Cout * sizeof(uint16_t);
}

extern "C" int pvo_conv_planes_pack(const void* w, void* w_frag, int ksize, int Cin, int Cout, int dtype, void* stream) {
  if (!pvo_conv_planes_supported(ksize, ksize == 7 ? 2 : 1, Cin, Cout)) return PVO_EUNSUPPORTED;
  if (dtype != PVO_F16 && dtype != PVO_BF16) return PVO_EUNSUPPORTED;
  if (!w || !w_frag || pvo_misaligned16(w_frag)) return PVO_EINVAL;
  const long long total = static_cast<long long>(conv_planes_steps(ksize, Cin)) * 32 * Cout;
  const dim3 grid(static_cast<unsigned>((total + 255) / 256));
  hipStream_t st = pvo_stream(stream);
  if (ksize == 3)
    hipLaunchKernelGGL(conv_planes_pack_kernel<3>, grid, dim3(256), 0, st, static_cast<const uint16_t*>(w), static_cast<uint16_t*>(w_frag), Cin, Cout, total);
  else
    hipLaunchKernelGGL(conv_planes_pack_kernel<7>, grid, dim3(256), 0, st, static_cast<const uint16_t*>(w), static_cast<uint16_t*>(w_frag), Cin, Cout, total);
  PVO_CHECK_LAUNCH();
  return PVO_OK;
}

extern "C" int pvo_conv_planes(const void* x, const void* w_frag, const void* bias, const void* residual, void* y, int N, int Cin, int Cout,
                               int H, int W, int ksize, int stride, int relu_inner, int relu_outer, int dtype, void* stream) {
  if (N < 0 || H < 0 || W < 0 || Cin <= 0 || Cout <= 0) return PVO_EINVAL;
  if (!pvo_conv_planes_supported(ksize, stride, Cin, Cout)) return PVO_EUNSUPPORTED;
  if (N == 0 || H == 0 || W == 0) return PVO_OK;
  if (!x || !w_frag || !y || pvo_misaligned16(x, w_frag, y)) return PVO_EINVAL;
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  {
    // y must not overlap x: other workgroups read the halo of pixels this one writes
    const uintptr_t xa = reinterpret_cast<uintptr_t>(x), ya = reinterpret_cast<uintptr_t>(y);
    const uintptr_t xb = xa + static_cast<uintptr_t>(N) * Cin * H * W * 2, yb = ya + static_cast<uintptr_t>(N) * Cout * Ho * Wo * 2;
    if (xa < yb && ya < xb) return PVO_EINVAL;
  }
  const int rpw = static_cast<long long>(N) * Ho * Wo >= 32768 ? 2 : 1;
  const int tiles_x = (Wo + 15) / 16, tiles_y = (Ho + 4 * rpw - 1) / (4 * rpw);
  const long long wgs = static_cast<long long>(N) * tiles_x * tiles_y;
  if (wgs > 0x7fffffffLL) return PVO_EUNSUPPORTED;
  const dim3 grid(static_cast<unsigned>(wgs), Cout / kCoBlock);
  hipStream_t st = pvo_stream(stream);
  const uint16_t* xp = static_cast<const uint16_t*>(x);
  const u32x4* wp = static_cast<const u32x4*>(w_frag);
  const uint16_t* bp = static_cast<const uint16_t*>(bias);
  const uint16_t* rp = static_cast<const uint16_t*>(residual);
  uint16_t* yp = static_cast<uint16_t*>(y);
  return pvo_dispatch16(dtype, [&](auto tag) -> int {
    using T = decltype(tag);
    auto launch3 = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, xp, wp, bp, rp, yp, Cin, Cout, H, W, Ho, Wo, tiles_x, tiles_y, relu_inner, relu_outer);
    };
    auto launch7 = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, xp, wp, bp, rp, yp, Cout, H, W, Ho, Wo, tiles_x, tiles_y, relu_inner, relu_outer);
    };
    if (ksize == 7) { if (rpw == 2) launch7(conv7x7_stem_kernel<T, 2>); else launch7(conv7x7_stem_kernel<T, 1>); }
    else if (stride == 1) { if (rpw == 2) launch3(conv3x3_planes_kernel<T, 1, 2>); else launch3(conv3x3_planes_kernel<T, 1, 1>); }
    else { if (rpw == 2) launch3(conv3x3_planes_kernel<T, 2, 2>); else launch3(conv3x3_planes_kernel<T, 2, 1>); }
    PVO_CHECK_LAUNCH();
    return PVO_OK;
  });
}
