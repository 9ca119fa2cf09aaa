// segment_assoc.hip — segments associated across keyframes: per graph edge i -> j the segments of frame i carried along the flow into
// frame j, the contingency table of (label in i, label in j), and the mutual best match by IoU.  Contract: include/pvo_hip.h
// (pvo_segment_associate); yardstick: tests/segment_assoc_reference.py.  Everything is an integer or an exactly stated fp32 operation.
//
//   (a) assoc_fill_kernel     overlap, area_i and area_j cleared on the stream (the caller never clears them)
//   (b) assoc_count_kernel    workgroups of 256 over (edge, pixel chunk), the grid sized per edge so that no workgroup and no wave holds
//                             pixels of two edges.  Global form (the one the call picks): one atomic per (wave, distinct pair) by
//                             segment_hist_kernel's ballot loop - a wave's 64 consecutive pixels touch a few pairs.  LDS form (form = 1,
//                             S <= 128: the S x S table fits 64 KB of static LDS): the workgroup counts into its own table and hands
//                             in its nonzero cells with one global atomic each.  area_j from the same chunk of frame jj[e]'s own
//                             pixels, by the ballot loop in both forms
//   (c) assoc_match_kernel    one workgroup of sixteen waves per edge: by rows (a wave per row, the lanes across the columns) area_i
//                             and the row maxima, by columns (groups of threads share a column's rows, joined through LDS) the column
//                             maxima, then the mutual test and the threshold.  The maxima hold (n, d) and compare n1 d2 against
//                             n2 d1 in int64: no float takes part
//
// Integer atomics: the table is the same in whatever order the adds arrive.  No allocation, no host synchronisation; capturable.
#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kLdsS = 128;            // the widest table the LDS form holds: 128 * 128 * 4 bytes = 64 KB

__global__ __launch_bounds__(kBlock) void assoc_fill_kernel(int* __restrict__ overlap, int* __restrict__ area_i, int* __restrict__ area_j,
                                                            long long cells, long long rows) {
  const long long stride = static_cast<long long>(gridDim.x) * kBlock;
  for (long long k = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; k < cells + 2 * rows; k += stride) {
    if (k < cells) overlap[k] = 0;
    else if (k < cells + rows) area_i[k - cells] = 0;
    else area_j[k - cells - rows] = 0;
  }
}

struct Count {
  const int32_t* labels; const int64_t* ii; const int64_t* jj; const float* target; const uint8_t* valid;
  int* overlap; int* area_j;
  int nframes, ht, wd, S, chunks, per;       // chunks: workgroups per edge; per: pixels per thread
};

// one add per (wave, distinct key): key < 0 = nothing to add.  Every lane of the wave must arrive.
__device__ __forceinline__ void wave_count(int* __restrict__ table, int key) {
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(key >= 0);
  while (todo) {
    const int leader = __ffsll(static_cast<long long>(todo)) - 1;
    const int k = __shfl(key, leader);
    const unsigned long long same = __ballot(key == k);
    if (lane == leader) atomicAdd(table + k, __popcll(same));
    todo &= ~same;
  }
}

// TABLE: ints of LDS for the S x S table (0: the global form)
template <int TABLE>
__global__ __launch_bounds__(kBlock) void assoc_count_kernel(const Count in) {
  __shared__ int tab[TABLE > 0 ? TABLE : 1];
  const int e = blockIdx.x / in.chunks, chunk = blockIdx.x - e * in.chunks;
  const long long i = in.ii[e], j = in.jj[e];
  if (i < 0 || i >= in.nframes || j < 0 || j >= in.nframes) return;        // (uniform over the workgroup) nothing of the edge is read
  const int S = in.S, P = in.ht * in.wd;
  if (TABLE > 0) {
    for (int c = threadIdx.x; c < S * S; c += kBlock) tab[c] = 0;
    __syncthreads();
  }
  const int32_t* li = in.labels + i * P;
  const int32_t* lj = in.labels + j * P;
  const float wmax = static_cast<float>(in.wd - 1), hmax = static_cast<float>(in.ht - 1);
  int* ov = in.overlap + static_cast<size_t>(e) * S * S;
  int* aj = in.area_j + static_cast<size_t>(e) * S;
  const int base = chunk * in.per * kBlock;
  for (int k = 0; k < in.per; ++k) {                                        // (the trip count is the same for every lane)
    const int p = base + k * kBlock + threadIdx.x;
    int key = -1, own = -1;
    if (p < P) {
      const int bj = lj[p];
      own = static_cast<unsigned>(bj) < static_cast<unsigned>(S) ? bj : 0;
      const size_t q = static_cast<size_t>(e) * P + p;
      if (!in.valid || in.valid[q]) {
        const float tx = in.target[2 * q], ty = in.target[2 * q + 1];
        const float rx = floorf(tx + 0.5f), ry = floorf(ty + 0.5f);
        // compared as floats: a NaN fails every comparison, an infinity or 1e30 the upper one
        if (tx - tx == 0.0f && ty - ty == 0.0f && rx >= 0.0f && rx <= wmax && ry >= 0.0f && ry <= hmax) {
          int a = li[p], b = lj[static_cast<int>(ry) * in.wd + static_cast<int>(rx)];
          a = static_cast<unsigned>(a) < static_cast<unsigned>(S) ? a : 0;
          b = static_cast<unsigned>(b) < static_cast<unsigned>(S) ? b : 0;
          key = a * S + b;
        }
      }
    }
    wave_count(aj, own);
    if (TABLE > 0) {
      if (key >= 0) atomicAdd(tab + key, 1);
    } else {
      wave_count(ov, key);
    }
  }
  if (TABLE > 0) {
    __syncthreads();
    for (int c = threadIdx.x; c < S * S; c += kBlock) {
      const int v = tab[c];
      if (v) atomicAdd(ov + c, v);
    }
  }
}

struct Match {
  const int* overlap; int* area_i; const int* area_j; const int32_t* cls; const int64_t* ii; const int64_t* jj;
  int* match; int* match_n; int* match_d;
  int nframes, S;
  float min_iou;
};

constexpr int kMaxS = PVO_SEGMENT_ASSOC_MAX_S;

// is (n1, d1, index k1) ahead of (n2, d2, k2)?  n = 0: no candidate.  Larger n / d first, then the lower index.
__device__ __forceinline__ bool ahead(int n1, int d1, int k1, int n2, int d2, int k2) {
  if (n1 <= 0) return false;
  if (n2 <= 0) return true;
  const long long l = static_cast<long long>(n1) * d2, r = static_cast<long long>(n2) * d1;
  return l > r || (l == r && k1 < k2);
}

constexpr int kMatchBlock = 1024;     // sixteen waves: the table is walked once by rows and once by columns, a few cells deep per thread

__global__ __launch_bounds__(kMatchBlock) void assoc_match_kernel(const Match in) {
  __shared__ int ai[kMaxS], aj[kMaxS], ci[kMaxS], cj[kMaxS], best_j[kMaxS], best_i[kMaxS];
  __shared__ int part_n[kMatchBlock], part_d[kMatchBlock], part_k[kMatchBlock];
  const int e = blockIdx.x, S = in.S, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long i = in.ii[e], j = in.jj[e];
  const bool frames = i >= 0 && i < in.nframes && j >= 0 && j < in.nframes;
  const int* ov = in.overlap + static_cast<size_t>(e) * S * S;
  const bool veto = in.cls != nullptr && frames;
  for (int s = tid; s < S; s += kMatchBlock) {
    aj[s] = in.area_j[static_cast<size_t>(e) * S + s];
    ci[s] = veto ? in.cls[i * S + s] : 0;
    cj[s] = veto ? in.cls[j * S + s] : 0;
  }
  __syncthreads();
  // by rows, a wave per row and the lanes across its columns: area_i (the row's sum), then best_j(a), ties to the lowest b
  for (int a = wave; a < S; a += kMatchBlock / 64) {
    const int* row = ov + a * S;
    const int first = lane < S ? row[lane] : 0;                              // (a row of up to 64 cells is read once)
    int sum = first;
    for (int b = lane + 64; b < S; b += 64) sum += row[b];
#pragma unroll
    for (int m = 32; m; m >>= 1) sum += __shfl_xor(sum, m);
    if (lane == 0) { ai[a] = sum; in.area_i[static_cast<size_t>(e) * S + a] = sum; }
    int n = 0, d = 1, k = 0;
    if (a >= 1)
      for (int b = lane; b < S; b += 64) {
        const int m = b == lane ? first : row[b];
        if (b >= 1 && m > 0 && ci[a] == cj[b]) {
          const int dd = sum + aj[b] - m;
          if (ahead(m, dd, b, n, d, k)) { n = m; d = dd; k = b; }
        }
      }
#pragma unroll
    for (int m = 32; m; m >>= 1) {
      const int n2 = __shfl_xor(n, m), d2 = __shfl_xor(d, m), k2 = __shfl_xor(k, m);
      if (ahead(n2, d2, k2, n, d, k)) { n = n2; d = d2; k = k2; }
    }
    if (lane == 0) best_j[a] = n > 0 ? k : 0;
  }
  __syncthreads();
  // by columns: the block is G groups of Sp >= S threads, thread (g, b) walks the rows 1 + g, 1 + g + G, ... of column b (a wave reads
  // consecutive cells of one row), then group 0 joins the G partial maxima: best_i(b), ties to the lowest a
  int Sp = 1;
  while (Sp < S) Sp *= 2;
  const int G = kMatchBlock / Sp, g = tid / Sp, b = tid - g * Sp;
  {
    int n = 0, d = 1, k = 0;
    if (b >= 1 && b < S)
#pragma unroll 4
      for (int a = 1 + g; a < S; a += G) {
        const int m = ov[a * S + b];
        if (m > 0 && ci[a] == cj[b]) {
          const int dd = ai[a] + aj[b] - m;
          if (ahead(m, dd, a, n, d, k)) { n = m; d = dd; k = a; }
        }
      }
    part_n[tid] = n; part_d[tid] = d; part_k[tid] = k;
  }
  __syncthreads();
  if (g == 0 && b < S) {
    int n = part_n[b], d = part_d[b], k = part_k[b];
    for (int q = 1; q < G; ++q) {
      const int n2 = part_n[q * Sp + b], d2 = part_d[q * Sp + b], k2 = part_k[q * Sp + b];
      if (ahead(n2, d2, k2, n, d, k)) { n = n2; d = d2; k = k2; }
    }
    best_i[b] = n > 0 ? k : 0;
  }
  __syncthreads();
  for (int a = tid; a < S; a += kMatchBlock) {
    int to = -1, n = 0, d = 0;
    const int bb = best_j[a];
    if (a >= 1 && bb >= 1 && best_i[bb] == a) {
      const int m = ov[a * S + bb], dd = ai[a] + aj[bb] - m;
      if (static_cast<double>(m) >= static_cast<double>(in.min_iou) * static_cast<double>(dd)) { to = bb; n = m; d = dd; }
    }
    const size_t o = static_cast<size_t>(e) * S + a;
    in.match[o] = to; in.match_n[o] = n; in.match_d[o] = d;
  }
}

}  // namespace

#define PVO_REQ(c) do { if (!(c)) return PVO_EINVAL; } while (0)

extern "C" size_t pvo_segment_assoc_args_size(void) { return sizeof(pvo_segment_assoc_args); }

extern "C" int pvo_segment_associate(const pvo_segment_assoc_args* a, void* stream) {
  PVO_REQ(a);
  PVO_REQ(a->E >= 0 && a->nframes >= 0 && a->ht >= 0 && a->wd >= 0 && static_cast<long long>(a->ht) * a->wd < (1ll << 24));
  PVO_REQ(a->S >= 1 && a->S <= PVO_SEGMENT_ASSOC_MAX_S && a->min_iou >= 0.0f && a->min_iou - a->min_iou == 0.0f);
  PVO_REQ(a->form == 0 || (a->form == 1 && a->S <= kLdsS));
  if (a->E == 0) return PVO_OK;
  PVO_REQ(a->ii && a->jj && a->overlap && a->area_i && a->area_j && a->match && a->match_n && a->match_d);
  const int P = a->ht * a->wd, S = a->S;
  PVO_REQ(P == 0 || (a->target && (a->nframes == 0 || a->labels)));
  hipStream_t s = pvo_stream(stream);
  const long long rows = static_cast<long long>(a->E) * S, cells = rows * S;
  const long long fill = (cells + 2 * rows + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(assoc_fill_kernel, dim3(static_cast<unsigned>(fill < 4096 ? fill : 4096)), dim3(kBlock), 0, s, a->overlap, a->area_i,
                     a->area_j, cells, rows);
  PVO_CHECK_LAUNCH();
  if (P > 0 && a->nframes > 0) {
    // the global form at every S unless the caller asks for the table in LDS: on the window measured
    // (profiles/r30_segment_assoc_kernels.txt) the two count equally fast at S = 16 and 64, and at S = 128 the global form is the faster
    // one even where every lane of a wave meets a pair of its own (the LDS form clears and scans S * S cells per workgroup)
    const bool lds = a->form == 1;
    // pixels per thread: as many as leave two workgroups for each of the 256 compute units, 16 at most (a chunk is read by one
    // workgroup front to back: with one workgroup per edge the LDS form at S = 64 took 18.9 us on 48 edges of 30 x 101, with twelve 5.2)
    int per = 16;
    while (per > 1 && static_cast<long long>(a->E) * ((P + per * kBlock - 1) / (per * kBlock)) < 512) per /= 2;
    const int chunks = (P + per * kBlock - 1) / (per * kBlock);
    PVO_REQ(static_cast<long long>(a->E) * chunks < (1ll << 31));
    const Count c = {a->labels, a->ii, a->jj, a->target, a->valid, a->overlap, a->area_j, a->nframes, a->ht, a->wd, S, chunks, per};
    const dim3 grid(static_cast<unsigned>(a->E * chunks));
    if (!lds) hipLaunchKernelGGL(assoc_count_kernel<0>, grid, dim3(kBlock), 0, s, c);
    else if (S <= 32) hipLaunchKernelGGL(assoc_count_kernel<32 * 32>, grid, dim3(kBlock), 0, s, c);
    else if (S <= 64) hipLaunchKernelGGL(assoc_count_kernel<64 * 64>, grid, dim3(kBlock), 0, s, c);
    else hipLaunchKernelGGL(assoc_count_kernel<kLdsS * kLdsS>, grid, dim3(kBlock), 0, s, c);
    PVO_CHECK_LAUNCH();
  }
  const Match m = {a->overlap, a->area_i, a->area_j, a->cls, a->ii, a->jj, a->match, a->match_n, a->match_d, a->nframes, S, a->min_iou};
  hipLaunchKernelGGL(assoc_match_kernel, dim3(a->E), dim3(kMatchBlock), 0, s, m);
  PVO_CHECK_LAUNCH();
  return PVO_OK;
}
