// ---------------------------------------------------------------------------
// solve: damping + fp64 Cholesky + substitution + pose retraction, one workgroup
// ---------------------------------------------------------------------------
#pragma once
#include "se3.h"
#include "conv1x1_tile.h"
#include "glo_tile.h"
#include <type_traits>
#include "ba_workspace.h"

namespace {
// Blocked LL^T (6x6 blocks: the natural granularity of the pose system) of the SPD matrix in A, rhs carried as
// row n of A (so the forward substitution is just one more row of every panel / trailing update).
//   per block column kb:  (a) every thread factors the 6x6 diagonal block redundantly in registers (21 broadcast LDS reads,
//                             no communication);  (b) one thread per remaining row solves its 1x6 panel in place;
//                         barrier;  (c) rank-6 trailing update over a 16x16 thread grid;  barrier.
// 2 barriers per 6 columns (the column-at-a-time version needed 6, and a serial fp64 sqrt/div in front of each).
// Ld[kb][27] keeps the factored diagonal blocks (row-major lower, 21) and their reciprocal diagonals (6) for the back substitution.
// 1/sqrt(d) in fp64: hardware estimate (v_rsq_f64) + two Newton steps; the library sqrt and divide are ~30-instruction
// software sequences each and sit on the serial critical path of the factorisation
// tools/ba_solve_timeline.py builds this file with -DPVO_BA_PROBE: clock stamps of the solve kernel's phases
#ifdef PVO_BA_PROBE
__device__ unsigned long long* g_ba_probe = nullptr;
#define BA_PROBE(slot) do { if (g_ba_probe && threadIdx.x == 0) g_ba_probe[slot] = __builtin_readcyclecounter(); } while (0)
#else
#define BA_PROBE(slot)
#endif
// ... and (-DPVO_BA_PROBE=2) of one block column (P / 2) of the pipelined factorisation's wave 0, slots 8..: every stamp is a
// scalar load + s_waitcnt lgkmcnt(0), which drains the LDS queue - the split it shows is of a step ~30 % longer than the real one
#if defined(PVO_BA_PROBE) && PVO_BA_PROBE == 2
#define BA_PROBE_STEP(slot) do { if (g_ba_probe && lane == 0 && kb == P / 2) g_ba_probe[slot] = __builtin_readcyclecounter(); } while (0)
#else
#define BA_PROBE_STEP(slot)
#endif

__device__ __forceinline__ double rsqrt_nr(double d) {
  double y = __builtin_amdgcn_rsq(d);
  y = y * (1.5 - 0.5 * d * y * y);
  y = y * (1.5 - 0.5 * d * y * y);
  return y;
}

__device__ __forceinline__ bool chol6(const double D[21], double L[21], double rdiag[6]) {
  // index (r,c), r >= c:  r*(r+1)/2 + c
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = D[j * (j + 1) / 2 + j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j * (j + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
    ok = ok && (d > 0.0);
    const double rs = ok ? rsqrt_nr(d) : 0.0;
    rdiag[j] = rs;
    L[j * (j + 1) / 2 + j] = d * rs;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double v = D[i * (i + 1) / 2 + j];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= L[i * (i + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
      L[i * (i + 1) / 2 + j] = v * rs;
    }
  }
  return ok;
}

// ENVELOPE (skyline) form: first[ib] = first block column of block row ib that holds a non-zero.  Cholesky creates no
// fill outside the envelope, so every panel / trailing-update / back-substitution term that lies outside it is an exact
// zero and is skipped - same bits as the dense factorisation, O(P * band^2) block operations instead of O(P^3).  The
// reduced pose system of a keyframe graph is block-banded up to its loop closures (two poses couple only through a depth
// frame both observe): at 63 free poses and temporal radius 3 the envelope holds 12 % of the matrix.  (The reference
// uses a sparse LLT for the same reason, droid_kernels.cu:1178-1184.)
// The matrix behind an accessor A(i, c): (n+1) x n, row n = rhs.  Two storages:
//   DenseMat  row-major in global memory: an envelope too large for LDS (slow: every access an L2 round trip);
//   EnvMat    only the blocks inside the envelope, block row b = blocks first[b] .. b of 36 doubles each at rowbase[b], + the
//             rhs - what lets a 63-pose system of a radius-3 graph (envelope 12 % of the matrix: 121 KB) live in LDS.
struct MatRow {            // one row of either storage: element c at base[c + k * (c / 6)]
  double* base; int k;
  __device__ __forceinline__ double& operator()(int c) const { return base[c + k * (c / 6)]; }
};
struct DenseMat {
  double* p; long long n;
  __device__ __forceinline__ MatRow row(int i) const { return MatRow{p + i * n, 0}; }
  __device__ __forceinline__ long long rowstep() const { return n; }  // distance between the same column of rows i and i + 1
  __device__ __forceinline__ int blockstep() const { return 6; }       // ... between the same entry of blocks (ib, cb) and (ib, cb + 1)
  // six contiguous (16-byte aligned) entries: row r of 6 x 6 block (ib, cb); the rhs entries of block cb
  __device__ __forceinline__ double* brow(int ib, int r, int cb) const { return p + static_cast<long long>(6 * ib + r) * n + 6 * cb; }
  __device__ __forceinline__ double* yrow(int cb) const { return p + n * n + 6 * cb; }
};
struct EnvMat {
  double* blk; double* rhs; const int* rowoff; int n;      // rowoff[ib] = rowbase[ib] - 36 first[ib]: block (ib, cb) at rowoff[ib] + 36 cb
  __device__ __forceinline__ MatRow row(int i) const {
    if (i == n) return MatRow{rhs, 0};
    const int ib = i / 6;                                  // 6 x 6 blocks, row-major inside
    return MatRow{blk + rowoff[ib] + (i - 6 * ib) * 6, 30};
  }
  __device__ __forceinline__ int rowstep() const { return 6; }         // ... inside one block row
  __device__ __forceinline__ int blockstep() const { return 36; }
  __device__ __forceinline__ double* brow(int ib, int r, int cb) const { return blk + rowoff[ib] + 36 * cb + 6 * r; }
  __device__ __forceinline__ double* yrow(int cb) const { return rhs + 6 * cb; }
};

// Inclusive scan (sum or max) of v[0..P) in place by the whole workgroup, 256 entries at a time with a carry: the serial
// thread-0 loops this replaces were 50 k cycles of LDS round trips per 63-pose solve.
__device__ __forceinline__ int* scan_scratch() {             // one copy for both instantiations of block_scan (LDS is scarce in the solve)
  __shared__ int scratch[2 * 256 + 1];
  return scratch;
}
template <bool MAX>
__device__ __forceinline__ void block_scan(int* v, int P) {
  int (*buf)[256] = reinterpret_cast<int (*)[256]>(scan_scratch());
  int& carry_s = scan_scratch()[512];
  const int tid = threadIdx.x;
  if (tid == 0) carry_s = MAX ? -0x7fffffff : 0;
  __syncthreads();
  for (int base = 0; base < P; base += 256) {
    const int i = base + tid;
    int x = i < P ? v[i] : (MAX ? -0x7fffffff : 0);
    int cur = 0;
    buf[0][tid] = x;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      int y = buf[cur][tid];
      if (tid >= d) { const int z = buf[cur][tid - d]; y = MAX ? (z > y ? z : y) : y + z; }
      buf[cur ^ 1][tid] = y;
      cur ^= 1;
      __syncthreads();
    }
    const int c = carry_s;
    const int r = MAX ? (c > buf[cur][tid] ? c : buf[cur][tid]) : c + buf[cur][tid];
    if (i < P) v[i] = r;
    __syncthreads();
    if (tid == 255) carry_s = r;
    __syncthreads();
  }
}

// reach[kb] = last block row whose envelope reaches block column kb: the rows below it (except the rhs) take no part in
// step kb, and scanning them - 23 loop trips per thread and step at 63 poses, each an LDS lookup to find out - cost more than
// the arithmetic (tools/ba_solve_timeline.py: 14 k cycles per block column against 4.5 k at 7 poses)
__device__ __forceinline__ void envelope_reach(const int* first, int* reach, int P) {
  if (P <= 12) {                                           // (nothing to skip in a window-sized system)
    for (int b = threadIdx.x; b < P; b += blockDim.x) reach[b] = P - 1;
    __syncthreads();
    return;
  }
  for (int b = threadIdx.x; b < P; b += blockDim.x) reach[b] = b;
  __syncthreads();
  for (int b = threadIdx.x; b < P; b += blockDim.x) atomicMax(&reach[first[b]], b);
  __syncthreads();
  block_scan<true>(reach, P);
}

template <class Mat>
__device__ __forceinline__ void chol_solve_blocked(Mat A, double* Ld, int n, int* fail_flag, const int* first, const int* reach) {
  // On return row n holds the solution x.
  const int tid = threadIdx.x, nt = blockDim.x;
  const int tx = tid & 15, ty = tid >> 4, nty = nt >> 4;
  const int P = n / 6;
  const MatRow Y = A.row(n);
  for (int kb = 0; kb < P; ++kb) {
    const int j0 = 6 * kb;
    const int iend = 6 * reach[kb] + 5;                    // last matrix row active in this step
    double D[21], L[21], rd[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const double* rp = &A.row(j0 + r)(j0);               // (six entries of one block row are contiguous in either storage)
#pragma unroll
      for (int c = 0; c <= r; ++c) D[r * (r + 1) / 2 + c] = rp[c];
    }
    const bool ok = chol6(D, L, rd);
    if (!ok) { if (tid == 0) *fail_flag = 1; __syncthreads(); return; }      // uniform: every thread saw the same block
    if (tid == 0) {
#pragma unroll
      for (int q = 0; q < 21; ++q) Ld[kb * 27 + q] = L[q];
#pragma unroll
      for (int q = 0; q < 6; ++q) Ld[kb * 27 + 21 + q] = rd[q];
    }
    // (b) panel rows j0+6 .. iend and the rhs row n, those whose envelope reaches this block column
    for (int ii = j0 + 6 + tid; ii <= iend + 1; ii += nt) {
      const int i = ii <= iend ? ii : n;
      if (i < n && first[i / 6] > kb) continue;
      double* rp = &A.row(i)(j0);
      double x[6];
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        double v = rp[c];
#pragma unroll
        for (int k = 0; k < c; ++k) v = fma(-x[k], L[c * (c + 1) / 2 + k], v);
        x[c] = v * rd[c];
      }
#pragma unroll
      for (int c = 0; c < 6; ++c) rp[c] = x[c];
    }
    __syncthreads();
    // (c) trailing update, rows i in (j0+6 .. iend] and n, columns c in (j0+6 .. min(i, iend)]
    for (int ii = j0 + 6 + ty; ii <= iend + 1; ii += nty) {
      const int i = ii <= iend ? ii : n;
      if (i < n && first[i / 6] > kb) continue;
      const MatRow R = A.row(i);
      double li[6];
      {
        const double* rp = &R(j0);
#pragma unroll
        for (int t = 0; t < 6; ++t) li[t] = rp[t];
      }
      const int cmax = (i < n) ? i : iend;
      for (int c = j0 + 6 + tx; c <= cmax; c += 16) {
        if (first[c / 6] > kb) continue;
        const double* cp = &A.row(c)(j0);
        double& dst = R(c);
        double acc = dst;
#pragma unroll
        for (int t = 0; t < 6; ++t) acc = fma(-li[t], cp[t], acc);
        dst = acc;
      }
    }
    __syncthreads();
  }
  BA_PROBE(2);
  // back substitution L^T x = y (y in row n), block rows from the bottom; x overwrites y.  Right-looking: once the six
  // unknowns of block kb are known, every earlier entry takes its update y[i] -= sum_c L[j0+c][i] x[c] independently, so
  // a block step is one redundant 6x6 triangular solve per thread (registers, reciprocal diagonals, no division), one
  // parallel update and ONE barrier.  (The left-looking form - dot products over the rows below, 36 wave shuffles of
  // doubles, a serial thread-0 solve with six fp64 divisions, two barriers - cost 20 of the solve's 37 us at P = 7:
  // measured with ablation builds.)
  for (int kb = P - 1; kb >= 0; --kb) {
    const int j0 = 6 * kb;
    const double* L = Ld + kb * 27;
    double x[6];
#pragma unroll
    for (int c = 5; c >= 0; --c) {
      double v = Y(j0 + c);
#pragma unroll
      for (int k = c + 1; k < 6; ++k) v = fma(-L[k * (k + 1) / 2 + c], x[k], v);
      x[c] = v * L[21 + c];                                  // reciprocal diagonal
    }
    __syncthreads();                                         // everyone has read y[j0..j0+6) before it is overwritten
    if (tid < 6) Y(j0 + tid) = x[tid];
    const MatRow R0 = A.row(j0);                             // rows j0 .. j0+5 of one block row: 6 entries apart
    for (int i = 6 * first[kb] + tid; i < j0; i += nt) {     // row block kb of L is zero left of its envelope
      const double* lp = &R0(i);
      double v = Y(i);
#pragma unroll
      for (int c = 0; c < 6; ++c) v = fma(-lp[c * A.rowstep()], x[c], v);
      Y(i) = v;
    }
    __syncthreads();
  }
}

// ---- the same factorisation by ONE wave, without workgroup barriers (matrices that live in LDS) ------------------------------
// The block steps of a Cholesky factorisation are a serial chain; with four waves every step paid two s_barriers, a scan of
// the candidate rows by 256 threads and element-wise LDS traffic through the row accessor (tools/ba_solve_timeline.py: 3.8 k
// cycles per block column at 7 poses, 7.6 k at 63).  One wave needs no barrier - LDS operations of a wave are performed in
// program order, only the COMPILER has to be kept from reordering them (wave_lds_sync) - and the step's work is small: at
// most a few hundred 6-element row tasks.  Per block column kb:
//   (a) every lane factors the 6 x 6 diagonal block redundantly in registers (as before);
//   (b) the active block rows (envelope reaches column kb) are compacted into a list by ballot;
//   (c) panel: one lane per row of the active blocks and the rhs row;
//   (d) trailing update: one lane per (block pair, row): six entries of the pair's block, 36 FMAs, operands as 16-byte reads.
// Every entry sees exactly the operations of chol_solve_blocked in the same order (t = 0..5 within a step, steps ascending),
// so the result is bit-identical to it - and to the dense factorisation, for the reason given at EnvMat.
constexpr int kMaxEnvBlocks = 2048;      // poses the envelope table covers (beyond: dense, first = 0)
constexpr int kMaxActiveRows = 512;      // active block rows of one step (each owns a stored block: the LDS budget holds < 490)

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ void ld6(const double* p, double (&v)[6]) {
  const double2 a = reinterpret_cast<const double2*>(p)[0], b = reinterpret_cast<const double2*>(p)[1], c = reinterpret_cast<const double2*>(p)[2];
  v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y; v[4] = c.x; v[5] = c.y;
}
__device__ __forceinline__ void st6(double* p, const double (&v)[6]) {
  reinterpret_cast<double2*>(p)[0] = double2{v[0], v[1]};
  reinterpret_cast<double2*>(p)[1] = double2{v[2], v[3]};
  reinterpret_cast<double2*>(p)[2] = double2{v[4], v[5]};
}

template <class Mat>
__device__ __forceinline__ void chol_solve_wave(Mat A, double* Ld, int n, int* fail_flag, const int* first, const int* reach, unsigned short* rows) {
  // executed by the 64 lanes of ONE wave; on return the rhs holds the solution x
  const int lane = threadIdx.x & 63;
  const int P = n / 6;
  for (int kb = 0; kb < P; ++kb) {
    double D[21], L[21], rd[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const double* rp = A.brow(kb, r, kb);
#pragma unroll
      for (int c = 0; c <= r; ++c) D[r * (r + 1) / 2 + c] = rp[c];
    }
    const bool ok = chol6(D, L, rd);
    if (!ok) { if (lane == 0) *fail_flag = 1; return; }                // uniform: every lane saw the same block
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < 21; ++q) Ld[kb * 27 + q] = L[q];
#pragma unroll
      for (int q = 0; q < 6; ++q) Ld[kb * 27 + 21 + q] = rd[q];
    }
    // (b) the block rows below kb whose envelope reaches this block column
    const int lo = kb + 1, hi = reach[kb];
    int m = 0;
    for (int base = lo; base <= hi; base += 64) {
      const int ib = base + lane;
      const bool act = ib <= hi && first[ib] <= kb;
      const unsigned long long mask = __ballot(act);
      const int at = m + __popcll(mask & ((1ull << lane) - 1ull));
      if (act && at < kMaxActiveRows) rows[at] = static_cast<unsigned short>(ib);
      m += __popcll(mask);
    }
    if (m > kMaxActiveRows) { if (lane == 0) *fail_flag = 1; return; }   // (cannot happen for a matrix that fits the LDS budget: every active row owns a stored block)
    wave_lds_sync();
    // (c) panel: x = row L^-T, in place; task 6 m is the rhs row
    for (int t = lane; t <= 6 * m; t += 64) {
      const int q = t / 6;
      double* rp = (t < 6 * m) ? A.brow(rows[q], t - 6 * q, kb) : A.yrow(kb);
      double v[6], x[6];
      ld6(rp, v);
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        double u = v[c];
#pragma unroll
        for (int k = 0; k < c; ++k) u = fma(-x[k], L[c * (c + 1) / 2 + k], u);
        x[c] = u * rd[c];
      }
      st6(rp, x);
    }
    wave_lds_sync();
    // (d) trailing update: block (a, b) of the active list, a >= b, row r: A(a,b)[r][:] -= L(a,kb)[r][:] L(b,kb)^T; then
    // one task per active block for the rhs row
    const int npair = m * (m + 1) / 2;
    const int ntask = 6 * npair + m;
    for (int t = lane; t < ntask; t += 64) {
      double li[6];
      double* dst;
      int cb, cmax = 5;
      if (t < 6 * npair) {
        const int pr = t / 6, r = t - 6 * pr;
        int a = static_cast<int>((sqrtf(8.0f * static_cast<float>(pr) + 1.0f) - 1.0f) * 0.5f);
        while ((a + 1) * (a + 2) / 2 <= pr) ++a;
        while (a * (a + 1) / 2 > pr) --a;
        const int b = pr - a * (a + 1) / 2;
        const int ib = rows[a];
        cb = rows[b];
        ld6(A.brow(ib, r, kb), li);
        dst = A.brow(ib, r, cb);
        if (a == b) cmax = r;                                          // lower triangle of a diagonal block
      } else {
        cb = rows[t - 6 * npair];
        ld6(A.yrow(kb), li);
        dst = A.yrow(cb);
      }
      double acc[6];
      ld6(dst, acc);
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        double cp[6];
        ld6(A.brow(cb, c, kb), cp);
        double u = acc[c];
#pragma unroll
        for (int q = 0; q < 6; ++q) u = fma(-li[q], cp[q], u);
        acc[c] = (c <= cmax) ? u : acc[c];
      }
      st6(dst, acc);
    }
    wave_lds_sync();
  }
  BA_PROBE(2);
  // back substitution L^T x = y, block rows from the bottom (right-looking, as in chol_solve_blocked)
  for (int kb = P - 1; kb >= 0; --kb) {
    const double* L = Ld + kb * 27;
    double* y = A.yrow(kb);
    double x[6];
#pragma unroll
    for (int c = 5; c >= 0; --c) {
      double v = y[c];
#pragma unroll
      for (int k = c + 1; k < 6; ++k) v = fma(-L[k * (k + 1) / 2 + c], x[k], v);
      x[c] = v * L[21 + c];                                            // reciprocal diagonal
    }
    wave_lds_sync();                                                   // every lane has read y before it is overwritten
    if (lane < 6) y[lane] = x[lane];
    for (int i = 6 * first[kb] + lane; i < 6 * kb; i += 64) {          // row block kb of L is zero left of its envelope
      const int cbk = i / 6, c2 = i - 6 * cbk;
      double* yp = A.yrow(cbk) + c2;
      double v = *yp;
#pragma unroll
      for (int c = 0; c < 6; ++c) v = fma(-A.brow(kb, c, cbk)[c2], x[c], v);
      *yp = v;
    }
    wave_lds_sync();
  }
}

// ---- ... and by FOUR waves in a look-ahead pipeline --------------------------------------------------------------------------
// What bounds the two forms above is the serial chain  6 x 6 Cholesky of block (kb, kb) -> panel -> update of block column
// kb + 1 -> next 6 x 6 Cholesky; the rest of a step's trailing update (all block columns beyond kb + 1) and the whole forward
// substitution of the right-hand side are not on it.  Here wave 0 walks the chain and nothing else:
//   wave 0    step kb: factor the diagonal block, panel; make sure the workers have finished step kb - 1; publish
//             (`panel` = kb); update block column kb + 1 (the look-ahead); next step.
//   wave 1    the right-hand side (its panel solve and its updates, all steps in order), then pair tasks
//   waves 2-3 pair tasks of step kb for the block columns beyond kb + 1, as soon as `panel` >= kb; publish `done[w]` = kb.
// Order of the operations an entry sees (= bit-identity with chol_solve_blocked): a worker starts step kb when `panel` >= kb,
// which wave 0 publishes only after EVERY worker has finished step kb - 1 (two steps' updates of one entry may belong to two
// different waves); wave 0's look-ahead of step kb comes after the same wait.  Waves of one workgroup are resident together,
// so waiting on a flag in LDS cannot deadlock; LDS operations of a wave are performed in order, so data written before a flag
// are visible to whoever sees the flag (the fences only pin the compiler and the wait counters).  Waits are bounded: a wave
// that gives up sets `abort` and the solve reports failure instead of hanging the device.
// Wave 0's step: the active rows of every step are listed ONCE, before the factorisation, by the whole workgroup (pipe_lists:
// they depend on the envelope only); a step's lookups (list, row offsets) are made during the step before; the panel's
// operand rows and the workers' flags are loaded BEFORE the 6 x 6 Cholesky; a lane keeps its panel row in registers for the
// look-ahead update (it is that update's left operand).
// Measured (tools/ba_solve_timeline.py, 63 free poses): 4.1 k cycles per block column against 6.7 k for one wave doing
// everything.  A lone wave pays ~10-16 cycles of issue per LDS instruction and ~8 per fp64 operation, and ~150-200 per
// dependent LDS round trip, so what is left is the 6 x 6 Cholesky (~1.0 k), the look-ahead (~1.5 k: 24 16-byte loads, 36
// FMAs, 3 stores per lane) and the panel.  Tried on top of this and slower: the next diagonal block handed over through 42
// v_readlane instead of LDS, and the factored block stored by six panel lanes instead of 27 stores of lane 0 (+5 %); the
// look-ahead split into wave 0 (diagonal block, one entry per lane) and a worker (rest of the column, own flag) (+17 %: two
// flag hand-overs on the chain cost more than the arithmetic they take off it).
constexpr int kPipeSpinLimit = 1 << 20;
constexpr int kPipeListMax = 2 * kMaxActiveRows;      // sub-diagonal blocks inside the envelope (every one is a stored block: < 494 in LDS)
struct __attribute__((aligned(16))) PipeCtl { int panel; int done[3]; int abort; int total; };

__device__ __forceinline__ int lds_peek(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void pipe_post(int* flag, int v) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __hip_atomic_store(flag, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ bool pipe_wait_panel(PipeCtl* ctl, int v) {
  int spins = 0;
  while (lds_peek(&ctl->panel) < v) {
    if (lds_peek(&ctl->abort) || ++spins > kPipeSpinLimit) return false;
    __builtin_amdgcn_s_sleep(1);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  return true;
}
__device__ __forceinline__ int pipe_done_min(PipeCtl* ctl) {            // three reads in flight, one round trip
  const int a = lds_peek(&ctl->done[0]), b = lds_peek(&ctl->done[1]), c = lds_peek(&ctl->done[2]);
  return min(a, min(b, c));
}
__device__ __forceinline__ bool pipe_wait_done(PipeCtl* ctl, int seen, int v) {
  int spins = 0;
  while (seen < v) {
    if (lds_peek(&ctl->abort) || ++spins > kPipeSpinLimit) return false;
    __builtin_amdgcn_s_sleep(1);
    seen = pipe_done_min(ctl);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  return true;
}

// Lists of every step's active block rows (ib > kb with first[ib] <= kb), ascending, in compressed-column form:
// rowlist[colptr[kb] .. colptr[kb + 1]).  `reach` is consumed: on return it holds colptr (P + 1 entries; P < kMaxEnvBlocks).
// Whole workgroup; returns false (everything untouched) when the lists do not fit.
__device__ __forceinline__ bool pipe_lists(const int* first, int* reach, int P, unsigned short* rowlist, PipeCtl* ctl) {
  int hi_keep[kMaxEnvBlocks / 256], cnt_keep[kMaxEnvBlocks / 256];
  int mine = 0;
#pragma unroll
  for (int q = 0; q < kMaxEnvBlocks / 256; ++q) {
    const int kb = q * 256 + threadIdx.x;
    int cnt = 0, hi = -1;
    if (kb < P) {
      hi = reach[kb];
      for (int ib = kb + 1; ib <= hi; ++ib) cnt += first[ib] <= kb ? 1 : 0;
    }
    hi_keep[q] = hi; cnt_keep[q] = cnt; mine += cnt;
  }
  if (threadIdx.x == 0) ctl->total = 0;
  __syncthreads();
  if (mine) atomicAdd(&ctl->total, mine);
  __syncthreads();
  if (ctl->total > kPipeListMax || P + 1 > kMaxEnvBlocks) return false;
#pragma unroll
  for (int q = 0; q < kMaxEnvBlocks / 256; ++q) {
    const int kb = q * 256 + threadIdx.x;
    if (kb < P) reach[kb] = cnt_keep[q];
  }
  __syncthreads();
  block_scan<false>(reach, P);                                            // inclusive
#pragma unroll
  for (int q = 0; q < kMaxEnvBlocks / 256; ++q) {
    const int kb = q * 256 + threadIdx.x;
    if (kb >= P) continue;
    int at = reach[kb] - cnt_keep[q];
    for (int ib = kb + 1; ib <= hi_keep[q]; ++ib)
      if (first[ib] <= kb) rowlist[at++] = static_cast<unsigned short>(ib);
  }
  __syncthreads();
  // inclusive -> colptr: shift by one entry (through registers: in place)
  int incl[kMaxEnvBlocks / 256];
#pragma unroll
  for (int q = 0; q < kMaxEnvBlocks / 256; ++q) {
    const int kb = q * 256 + threadIdx.x;
    incl[q] = kb < P ? reach[kb] : 0;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < kMaxEnvBlocks / 256; ++q) {
    const int kb = q * 256 + threadIdx.x;
    if (kb < P) reach[kb + 1] = incl[q];
  }
  if (threadIdx.x == 0) reach[0] = 0;
  __syncthreads();
  return true;
}

// acc (row r of block (ib, cb)) -= li (row r of L(ib, kb)) times L(cb, kb)^T, whose rows start at cprow0 and lie rstep apart;
// entries beyond column cmax stay (diagonal blocks: lower triangle)
__device__ __forceinline__ void pair_update(const double* cprow0, int rstep, const double (&li)[6], int cmax, double (&acc)[6]) {
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    double cp[6];
    ld6(cprow0 + c * rstep, cp);
    double u = acc[c];
#pragma unroll
    for (int q = 0; q < 6; ++q) u = fma(-li[q], cp[q], u);
    acc[c] = (c <= cmax) ? u : acc[c];
  }
}
template <class Mat>
__device__ __forceinline__ void pair_task(const Mat& A, int kb, int ib, int r, int cb, int cmax) {
  double li[6], acc[6];
  ld6(A.brow(ib, r, kb), li);
  double* dst = A.brow(ib, r, cb);
  ld6(dst, acc);
  pair_update(A.brow(cb, 0, kb), static_cast<int>(A.rowstep()), li, cmax, acc);
  st6(dst, acc);
}
__device__ __forceinline__ void panel_row(const double (&v)[6], const double (&L)[21], const double (&rd)[6], double (&x)[6]) {
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    double u = v[c];
#pragma unroll
    for (int k = 0; k < c; ++k) u = fma(-x[k], L[c * (c + 1) / 2 + k], u);
    x[c] = u * rd[c];
  }
}

// Block columns [kb0, kb1) of the factorisation (and of the right-hand side's forward substitution): the whole of it is
// (0, P); the partitioned solve (ba_solve_twin_kernel) stops in between, and continues with the flags where they stand -
// `panel` and `done[]` hold kb0 - 1 when a range ends at kb0.  Executed by the four waves of the workgroup, after pipe_lists;
// the caller puts a barrier behind it.
template <class Mat>
__device__ __forceinline__ void chol_pipe_range(Mat A, double* Ld, int P, int* fail_flag, const int* colptr,
                                const unsigned short* rowlist, PipeCtl* ctl, int kb0, int kb1) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rstep = static_cast<int>(A.rowstep()), bstep = A.blockstep();
#define PIPE_GIVE_UP() do { if (lane == 0) { *fail_flag = 1; __hip_atomic_store(&ctl->abort, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); } return; } while (0)
  if (kb0 >= kb1) return;
  if (wave == 0) {
    const int q0 = lane / 6, r0 = lane - 6 * q0;
    int m = colptr[kb0 + 1] - colptr[kb0];
    const unsigned short* rows = rowlist + colptr[kb0];
    bool one_trip = 6 * m <= 64, mine = one_trip && lane < 6 * m;
    double* rp0 = A.brow(mine ? rows[q0] : kb0, r0, kb0);
    double* dptr = A.brow(kb0, 0, kb0);
    bool ahead = m > 0 && rows[0] == kb0 + 1;
    for (int kb = kb0; kb < kb1; ++kb) {
      const bool more = kb + 1 < P;
      BA_PROBE_STEP(8);
      double D[21], L[21], rd[6], v0[6], x0[6];
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        double v[6];
        ld6(dptr + r * rstep, v);
#pragma unroll
        for (int c = 0; c <= r; ++c) D[r * (r + 1) / 2 + c] = v[c];
      }
      if (one_trip) ld6(rp0, v0);                                          // (idle lanes read some valid row)
      const int seen = kb >= 1 ? pipe_done_min(ctl) : 0;                   // the workers' progress, read early
      const int nbeg = more ? colptr[kb + 1] : 0;                          // next step, first lookup
      const int nm = more ? colptr[kb + 2] - nbeg : 0;
      BA_PROBE_STEP(9);
      const bool ok = chol6(D, L, rd);
      if (!ok) PIPE_GIVE_UP();                                             // uniform: every lane saw the same block
      BA_PROBE_STEP(10);
      const unsigned short* nrows = rowlist + nbeg;                        // next step, second lookup
      const bool n_one = 6 * nm <= 64, n_mine = n_one && lane < 6 * nm;
      const int nib0 = n_mine ? nrows[q0] : (more ? kb + 1 : kb);
      const bool nahead = nm > 0 && nrows[0] == kb + 2;
      if (one_trip) {
        panel_row(v0, L, rd, x0);
        if (mine) st6(rp0, x0);
      } else {
        for (int t = lane; t < 6 * m; t += 64) {
          const int q = t / 6;
          double* rp = A.brow(rows[q], t - 6 * q, kb);
          double v[6], x[6];
          ld6(rp, v);
          panel_row(v, L, rd, x);
          st6(rp, x);
        }
      }
      if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 21; ++q) Ld[kb * 27 + q] = L[q];
#pragma unroll
        for (int q = 0; q < 6; ++q) Ld[kb * 27 + 21 + q] = rd[q];
      }
      BA_PROBE_STEP(11);
      double* nrp0 = A.brow(nib0, r0, more ? kb + 1 : kb);                 // next step, third lookup (the rows' offsets)
      double* ndptr = more ? A.brow(kb + 1, 0, kb + 1) : dptr;
      // nobody may start step kb before every worker has finished step kb - 1; the same wait covers the look-ahead below
      // (block column kb + 1 must have seen the workers' step kb - 1 before this step's update and the next Cholesky)
      if (kb >= 1 && !pipe_wait_done(ctl, seen, kb - 1)) PIPE_GIVE_UP();
      BA_PROBE_STEP(12);
      pipe_post(&ctl->panel, kb);
      BA_PROBE_STEP(13);
      if (ahead) {                                                         // look-ahead: pairs (a, 0) of the list; L(kb + 1, kb) sits left of the next diagonal block
        if (one_trip) {
          if (mine) {
            double* dst = rp0 + bstep;
            double acc[6];
            ld6(dst, acc);
            pair_update(ndptr - bstep, rstep, x0, q0 == 0 ? r0 : 5, acc);
            st6(dst, acc);
          }
        } else {
          for (int t = lane; t < 6 * m; t += 64) {
            const int a = t / 6, r = t - 6 * a;
            pair_task(A, kb, rows[a], r, kb + 1, a == 0 ? r : 5);
          }
        }
      }
      wave_lds_sync();
      BA_PROBE_STEP(14);
      m = nm; rows = nrows; one_trip = n_one; mine = n_mine; rp0 = nrp0; dptr = ndptr; ahead = nahead;
    }
    // the right-hand side's forward substitution is wave 1's: wait for its last step
    if (!pipe_wait_done(ctl, pipe_done_min(ctl), kb1 - 1)) PIPE_GIVE_UP();
    wave_lds_sync();
    return;
  }
  // ---- workers
  const int slot = wave == 1 ? 2 : wave - 2;                               // pair tasks go to waves 2, 3 first: wave 1 has the rhs
  for (int kb = kb0; kb < kb1; ++kb) {
    const int beg = colptr[kb], m = colptr[kb + 1] - beg;
    const unsigned short* rows = rowlist + beg;
    if (!pipe_wait_panel(ctl, kb)) PIPE_GIVE_UP();
    if (wave == 1) {
      // rhs: y(kb) <- L(kb,kb)^-1 y(kb) (every lane redundantly, lane 0 stores), then y(cb) -= L(cb, kb) y(kb) per active row
      const double* Lp = Ld + kb * 27;
      double L[21], rd[6];
#pragma unroll
      for (int q = 0; q < 21; ++q) L[q] = Lp[q];
#pragma unroll
      for (int q = 0; q < 6; ++q) rd[q] = Lp[21 + q];
      double* y = A.yrow(kb);
      double v[6], x[6];
      ld6(y, v);
      panel_row(v, L, rd, x);
      if (lane == 0) st6(y, x);
      for (int a = lane; a < m; a += 64) {
        const int cb = rows[a];
        double* dst = A.yrow(cb);
        double acc[6];
        ld6(dst, acc);
        pair_update(A.brow(cb, 0, kb), rstep, x, 5, acc);
        st6(dst, acc);
      }
    }
    const int b0 = (m > 0 && rows[0] == kb + 1) ? 1 : 0;                   // block column kb + 1 is wave 0's
    const int mm = m - b0;
    const int ntask = 6 * (mm * (mm + 1) / 2);
    for (int t = slot * 64 + lane; t < ntask; t += 192) {
      const int pr = t / 6, r = t - 6 * pr;
      int a = static_cast<int>((sqrtf(8.0f * static_cast<float>(pr) + 1.0f) - 1.0f) * 0.5f);
      while ((a + 1) * (a + 2) / 2 <= pr) ++a;
      while (a * (a + 1) / 2 > pr) --a;
      const int b = pr - a * (a + 1) / 2;
      pair_task(A, kb, rows[a + b0], r, rows[b + b0], a == b ? r : 5);
    }
    pipe_post(&ctl->done[wave - 1], kb);
  }
#undef PIPE_GIVE_UP
}

// Back substitution L^T x = y by wave 0, block rows kb_top .. 0, the arithmetic of chol_solve_blocked.  One wave, LDS
// operations in program order, so no fence inside: a step's operands that do not depend on x (this lane's column of
// L and its y entry, the next step's factored diagonal block) are in flight while the 6 x 6 triangular solve runs.
// Block rows >= given_from hold their solution already (the partitioned solve: the separator's unknowns arrive from the
// other workgroup); they only update the rows below given_from.  given_from > kb_top: the ordinary substitution.
// Stops after block row kb_bot (every row above it has then received all its updates from the rows processed).
template <class Mat>
__device__ __forceinline__ void pipe_backsub(Mat A, const double* Ld, const int* first, int kb_top, int given_from, int kb_bot = 0) {
  if (threadIdx.x >= 64 || kb_top < kb_bot) return;
  const int lane = threadIdx.x & 63;
  const int rstep = static_cast<int>(A.rowstep());
  double Lc[27];
#pragma unroll
  for (int q = 0; q < 27; ++q) Lc[q] = Ld[kb_top * 27 + q];
  for (int kb = kb_top; kb >= kb_bot; --kb) {
    double* y = A.yrow(kb);
    double yv[6], x[6], Ln[27];
    ld6(y, yv);
    const int ibeg = 6 * first[kb];
    const bool given = kb >= given_from;
    const int iend = 6 * (given ? given_from : kb);
    if (kb > 0) {
#pragma unroll
      for (int q = 0; q < 27; ++q) Ln[q] = Ld[(kb - 1) * 27 + q];
    }
#pragma unroll
    for (int c = 5; c >= 0; --c) {
      double v = yv[c];
#pragma unroll
      for (int k = c + 1; k < 6; ++k) v = fma(-Lc[k * (k + 1) / 2 + c], x[k], v);
      x[c] = given ? yv[c] : v * Lc[21 + c];                               // reciprocal diagonal
    }
    asm volatile("" ::: "memory");
    if (lane < 6 && !given) y[lane] = x[lane];
    asm volatile("" ::: "memory");
    for (int i = ibeg + lane; i < iend; i += 64) {                         // row block kb of L is zero left of its envelope
      const int cbk = i / 6, c2 = i - 6 * cbk;
      double* yp = A.yrow(cbk) + c2;
      const double* lp = A.brow(kb, 0, cbk) + c2;
      double v = *yp;
#pragma unroll
      for (int c = 0; c < 6; ++c) v = fma(-lp[c * rstep], x[c], v);
      *yp = v;
    }
    asm volatile("" ::: "memory");                                         // (compiler only: the next step reads what other lanes wrote)
    if (kb > 0) {
#pragma unroll
      for (int q = 0; q < 27; ++q) Lc[q] = Ln[q];
    }
  }
  wave_lds_sync();
}

template <class Mat>
__device__ __forceinline__ void chol_solve_pipe(Mat A, double* Ld, int n, int* fail_flag, const int* first, const int* colptr,
                                const unsigned short* rowlist, PipeCtl* ctl) {
  // executed by the four waves of the workgroup, after pipe_lists; on return (and after the caller's barrier) the rhs holds x
  const int P = n / 6;
  chol_pipe_range(A, Ld, P, fail_flag, colptr, rowlist, ctl, 0, P);
  if (threadIdx.x < 64 && !lds_peek(&ctl->abort)) {
    BA_PROBE(2);
    pipe_backsub(A, Ld, first, P - 1, P);
  }
}


// ---- the ENVELOPE form (systems beyond the dense matrix-core solve: the global bundle adjustment) ------------------------
// Two multi-workgroup kernels prepare the envelope solve (inside it, reading 1.1 MB of fixed point through a single CU
// was 429 k of its 1479 k cycles at 63 poses - tools/ba_solve_timeline.py):
//   ba_env_kernel      numeric envelope: env[b] = first block column with a non-zero in block row b (atomicMin; the table is
//                      INT_MAX between solves).  Numeric, not structural: in an edge-sharded BA the system is the all-reduced
//                      one, whose couplings this rank's edge list does not know.
//   ba_prepare_kernel  fixed point -> fp64 with the damping, `sys` zeroed, into the layout the solve will use: compact
//                      envelope blocks if they fit the LDS budget, else dense.
// env_layout: offsets of the compact layout (block row b = blocks first[b] .. b); returns the number of doubles of all
// blocks.  Executed by one thread.
// first[] from the numeric envelope and the offsets of the compact layout (block row b = blocks first[b] .. b); returns the
// number of doubles of all blocks, or INT_MAX when that does not fit an int.  Whole workgroup; valid after it returns.
__device__ __forceinline__ int env_layout(const int* __restrict__ env, int P, int* first, int* rowbase, int* total_s) {
  for (int b = threadIdx.x; b < P; b += blockDim.x) {
    const int e = env[b];
    const int f = e < b ? (e < 0 ? 0 : e) : b;             // clamped to [0, b] on BOTH sides, as pvo_ba_packed_elems sizes the message
    first[b] = f;
    rowbase[b] = (b - f + 1) * 36;                         // sizes, scanned below
  }
  __syncthreads();
  // (sizes up to 36 * 2048 per row: the running sum can overflow an int only far beyond any LDS budget - clamp)
  block_scan<false>(rowbase, P);
  if (threadIdx.x == 0) *total_s = (P > 0 && rowbase[P - 1] >= 0) ? rowbase[P - 1] : 0x7fffffff;
  __syncthreads();
  for (int b = threadIdx.x; b < P; b += blockDim.x) {      // inclusive -> exclusive
    const int sz = (b - first[b] + 1) * 36;
    rowbase[b] -= sz;
  }
  __syncthreads();
  return *total_s;
}
// doubles of LDS the compact path needs: blocks + rhs + Ld (27 per pose) + slack, and (as ints) the offset table
__device__ __host__ __forceinline__ long long env_lds_bytes(long long blocks, int n, int P) {
  return 16 + 8 * (blocks + n + 27LL * P + 24) + 4LL * (P + 2);
}

__global__ __launch_bounds__(256) void ba_env_kernel(const long long* __restrict__ sys, int* __restrict__ env, int n) {
  // the minima of the few block rows a workgroup's 2048 entries span are formed in LDS first: one atomic per entry on ~P
  // global addresses was 69 us of a 64-keyframe step (15 k non-zeros below the diagonal, ~250 per address)
  constexpr int kSlots = 64;
  __shared__ int smin[kSlots];
  const int NN = n * n;
  const int base = blockIdx.x * 2048;
  const int br0 = (base / n) / 6;
  if (threadIdx.x < kSlots) smin[threadIdx.x] = 0x7fffffff;
  __syncthreads();
  long long raw[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int idx = base + u * 256 + threadIdx.x;
    raw[u] = idx < NN ? sys[idx] : 0;
  }
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int idx = base + u * 256 + threadIdx.x;
    if (idx >= NN || raw[u] == 0) continue;
    const int r = idx / n, c = idx - r * n;
    if (c >= r) continue;
    const int slot = r / 6 - br0, cb = c / 6;
    if (slot < kSlots) { if (cb < smin[slot]) atomicMin(&smin[slot], cb); }      // (the plain read only skips atomics that cannot lower the minimum)
    else atomicMin(&env[r / 6], cb);
  }
  __syncthreads();
  if (threadIdx.x < kSlots && smin[threadIdx.x] != 0x7fffffff) atomicMin(&env[br0 + threadIdx.x], smin[threadIdx.x]);
}

// The partition of the pose chain (ba_solve_twin_kernel): poses [0, m) are eliminated by one workgroup, poses [s, P) - in
// reverse order - by another, at the same time; the separator [m, s) = every pose that couples with one below m (s =
// reach[m - 1] + 1) comes last.  Chosen to make the longer chain + the separator shortest; 0 / 0 = not partitioned: separator
// wider than kMaxSep (loop closures), a chain less than a quarter shorter, or an image that does not fit the LDS budget.
// One workgroup, after env_layout (first, exclusive row offsets) and envelope_reach.
__device__ __forceinline__ void choose_partition(const int* first, const int* reach, const int* rowbase, int P, int blocks,
                                                 long long lds_budget, int* xchg_i) {
  __shared__ int best_s, colsum_s;
  if (threadIdx.x == 0) { best_s = 0x7fffffff; colsum_s = 0; }
  __syncthreads();
  for (int m = 1 + threadIdx.x; m < P; m += blockDim.x) {
    const int sp = reach[m - 1] + 1, w = sp - m;
    if (w < 1 || w > kMaxSep || P - sp < 2 || m < 2) continue;
    const int cost = (m > P - sp ? m : P - sp) + w;
    atomicMin(&best_s, cost * 4096 + m);
  }
  __syncthreads();
  int m = 0, sp = 0;
  if (best_s != 0x7fffffff && P < 4096) {
    m = best_s & 4095; sp = reach[m - 1] + 1;
    if (4 * (best_s >> 12) > 3 * P) m = 0;
  }
  if (m) {                                                 // sizes of the two images (bounds: the separator rows are stored dense)
    int mine = 0;
    for (int g = m + threadIdx.x; g < P; g += blockDim.x) mine += reach[g] - g + 1;
    if (mine) atomicAdd(&colsum_s, mine);
    __syncthreads();
    const int w = sp - m;
    const long long b0 = rowbase[sp] + 36LL * w * w, b1 = 36LL * (colsum_s + w * w);
    const long long tail = 16LL * (P + 2);                 // the global tables the loaders keep beside the image
    const bool fits = env_lds_bytes(b0, 6 * sp, sp) + tail <= lds_budget && env_lds_bytes(b1, 6 * (P - m), P - m) + tail <= lds_budget &&
                      b0 / 36 - sp <= kPipeListMax && b1 / 36 - (P - m) <= kPipeListMax && blocks > 0;
    if (!fits) m = 0;
  }
  if (threadIdx.x == 0) { xchg_i[0] = 0; xchg_i[1] = 0; xchg_i[2] = m; xchg_i[3] = m ? sp : 0; }
}

__global__ __launch_bounds__(256) void ba_prepare_kernel(long long* __restrict__ sys, double* __restrict__ out, const int* __restrict__ env,
                                                         int n, float lm, float ep, long long lds_budget, int* __restrict__ xchg_i) {
  __shared__ int first[kMaxEnvBlocks], rowbase[kMaxEnvBlocks + 1];
  __shared__ int blocks_s;
  const int P = n / 6;
  const int blocks = env_layout(env, P, first, rowbase, &blocks_s);
  const bool compact = env_lds_bytes(blocks, n, P) <= lds_budget;
  if (xchg_i && blockIdx.x == 0) {                         // (block-uniform)
    __shared__ int reach[kMaxEnvBlocks];
    if (compact && P > 12) {
      envelope_reach(first, reach, P);
      choose_partition(first, reach, rowbase, P, blocks, lds_budget, xchg_i);
    } else if (threadIdx.x == 0) {
      xchg_i[0] = 0; xchg_i[1] = 0; xchg_i[2] = 0; xchg_i[3] = 0;
    }
  }
  const int N = n * n + n;
  const int base = blockIdx.x * 2048;
  long long raw[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int idx = base + u * 256 + threadIdx.x;
    raw[u] = idx < N ? sys[idx] : 0;
  }
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int idx = base + u * 256 + threadIdx.x;
    if (idx >= N) continue;
    double v = static_cast<double>(raw[u]) * kInvFix;       // fixed point -> fp64
    sys[idx] = 0;                                           // ready for the next Gauss-Newton step's accumulation
    if (idx >= n * n) {                                     // rhs
      out[compact ? blocks + (idx - n * n) : idx] = v;
      continue;
    }
    const int r = idx / n, c = idx - r * n;
    if (r == c) v += static_cast<double>(ep) + static_cast<double>(lm) * v;   // droid_kernels.cu:1176
    if (!compact) { out[idx] = v; continue; }
    const int rb = r / 6, cb = c / 6;
    if (cb > rb || cb < first[rb]) continue;                // upper triangle / outside the envelope (exact zeros)
    out[rowbase[rb] + (cb - first[rb]) * 36 + (r - 6 * rb) * 6 + (c - 6 * cb)] = v;
  }
}

// ---- the edge-sharded step's message: the STRUCTURAL envelope of the pose system, packed -----------------------------------
// Between pvo_ba_local and pvo_ba_finish an edge-sharded run all-reduces the lower-triangle blocks (b, first_s[b] .. b) and the
// right-hand side (parallel.py: envelope_structure - derived from the whole graph's edge list, the same table on every rank).
// ba_pack_kernel gathers exactly those entries of the dense fixed-point system into one contiguous int64 message, in the
// compact layout of env_layout(first_s) - block row b = blocks first_s[b] .. b of 36 entries, then the 6P right-hand side - and
// leaves `sys` zeroed; after the all-reduce ba_env_packed_kernel / ba_prepare_packed_kernel read the MESSAGE (124 KB at 63
// poses) instead of the dense system (1.15 MB): numeric envelope, fp64 + damping into the solve's layout, partition.  No
// index tensors, no scatter back, nothing of torch's between the two library calls and the collective.
__global__ __launch_bounds__(256) void ba_pack_kernel(long long* __restrict__ sys, const int* __restrict__ first_s, long long* __restrict__ msg, int n) {
  __shared__ int first[kMaxEnvBlocks], rowbase[kMaxEnvBlocks + 1];
  __shared__ int blocks_s;
  const int P = n / 6;
  const int blocks = env_layout(first_s, P, first, rowbase, &blocks_s);
  const int N = n * n + n;
  const int base = blockIdx.x * 2048;
  long long raw[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int idx = base + u * 256 + threadIdx.x;
    raw[u] = idx < N ? sys[idx] : 0;
  }
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int idx = base + u * 256 + threadIdx.x;
    if (idx >= N) continue;
    sys[idx] = 0;
    if (idx >= n * n) { msg[blocks + (idx - n * n)] = raw[u]; continue; }
    const int r = idx / n, c = idx - r * n;
    const int rb = r / 6, cb = c / 6;
    if (cb > rb || cb < first[rb]) continue;                // upper triangle (never written) / structural zeros
    msg[rowbase[rb] + (cb - first[rb]) * 36 + (r - 6 * rb) * 6 + (c - 6 * cb)] = raw[u];
  }
}

// One workgroup per BLOCK ROW of the message (its blocks are contiguous: no search for the row of an entry; a flat split of the
// message with a binary search per entry made these two kernels twice as long as their dense counterparts).
__global__ __launch_bounds__(256) void ba_env_packed_kernel(const long long* __restrict__ msg, const int* __restrict__ first_s, int* __restrict__ env, int n) {
  __shared__ int first[kMaxEnvBlocks], rowbase[kMaxEnvBlocks + 1];
  __shared__ int blocks_s, smin;
  const int P = n / 6;
  env_layout(first_s, P, first, rowbase, &blocks_s);
  const int rb = blockIdx.x;
  if (threadIdx.x == 0) smin = 0x7fffffff;
  __syncthreads();
  const int f = first[rb], nsub = (rb - f) * 36;                         // entries left of the diagonal block
  const long long* row = msg + rowbase[rb];
  for (int base = 0; base < nsub; base += 8 * 256) {
    long long raw[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { const int k = base + u * 256 + threadIdx.x; raw[u] = k < nsub ? row[k] : 0; }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = base + u * 256 + threadIdx.x;
      if (k < nsub && raw[u] != 0) { const int cb = f + k / 36; if (cb < smin) atomicMin(&smin, cb); }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && smin != 0x7fffffff) env[rb] = smin;             // (this workgroup alone writes env[rb]; INT_MAX between solves)
}

// grid: P block rows + one workgroup for the right-hand side
__global__ __launch_bounds__(256) void ba_prepare_packed_kernel(const long long* __restrict__ msg, const int* __restrict__ first_s, double* __restrict__ out,
                                                                const int* __restrict__ env, int n, float lm, float ep, long long lds_budget,
                                                                int* __restrict__ xchg_i) {
  __shared__ int sfirst[kMaxEnvBlocks], srow[kMaxEnvBlocks + 1];       // the message's (structural) layout
  __shared__ int first[kMaxEnvBlocks], rowbase[kMaxEnvBlocks + 1];     // the solve's (numeric) layout
  __shared__ int sblocks_s, blocks_s;
  const int P = n / 6;
  const int sblocks = env_layout(first_s, P, sfirst, srow, &sblocks_s);
  const int blocks = env_layout(env, P, first, rowbase, &blocks_s);
  const bool compact = env_lds_bytes(blocks, n, P) <= lds_budget;
  if (xchg_i && blockIdx.x == 0) {                         // (block-uniform)
    __shared__ int reach[kMaxEnvBlocks];
    if (compact && P > 12) {
      envelope_reach(first, reach, P);
      choose_partition(first, reach, rowbase, P, blocks, lds_budget, xchg_i);
    } else if (threadIdx.x == 0) {
      xchg_i[0] = 0; xchg_i[1] = 0; xchg_i[2] = 0; xchg_i[3] = 0;
    }
  }
  const int rb = blockIdx.x;
  if (rb == P) {                                            // rhs
    for (int i = threadIdx.x; i < n; i += 256)
      out[compact ? blocks + i : static_cast<long long>(n) * n + i] = static_cast<double>(msg[sblocks + i]) * kInvFix;
    return;
  }
  const int sf = sfirst[rb], f = first[rb], nrow = (rb - sf + 1) * 36;
  const long long* row = msg + srow[rb];
  for (int base = 0; base < nrow; base += 8 * 256) {
    long long raw[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { const int k = base + u * 256 + threadIdx.x; raw[u] = k < nrow ? row[k] : 0; }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = base + u * 256 + threadIdx.x;
      if (k >= nrow) continue;
      double v = static_cast<double>(raw[u]) * kInvFix;
      const int q = k / 36, cb = sf + q, e = k - 36 * q, ri = e / 6, ci = e - 6 * ri;
      if (rb == cb && ri == ci) v += static_cast<double>(ep) + static_cast<double>(lm) * v;   // droid_kernels.cu:1176
      if (!compact) { out[static_cast<long long>(6 * rb + ri) * n + 6 * cb + ci] = v; continue; }
      if (cb < f) continue;                                 // inside the structural envelope, outside the numeric one: an exact zero
      out[rowbase[rb] + (cb - f) * 36 + e] = v;
    }
  }
}

// The pose solve is ONE workgroup for ~20 us (a window) to ~170 us (63 free poses) while the rest of the chip idles - and
// nothing else may run beside the bundle adjustment on another queue.  Work that is independent of it can ride in
// the SAME dispatch instead: workgroups 1 .. of this launch run up to three jobs that share no buffer with the solve -
//   a 1x1 convolution of a 128-channel tensor (conv1x1_tile.h): GraphAgg's upsampling mask in pvo_graph_update, 17 us on the
//   launch stream otherwise;
//   the two halves of the ConvGRU's global context (glo_tile.h) of the NEXT update, which depend on the hidden state only:
//   the partial means in the first solve's dispatch, the gate context in the second's (it reads what the first wrote - a
//   kernel boundary in between, no fence inside a dispatch).
struct Riders {
  const uint16_t *cx, *cw; const float* cbias; uint16_t* cy; long long crows; int cCout, cdtype, crow_blocks, cblocks;
  const uint16_t *gnet, *gw; const float* gbias; float* gpart; int gHW, gchunks, gdtype, gblocks;
  const float *xpart, *xwt, *xbias; float* xg; int xchunks, xblocks;
};

__device__ __forceinline__ void ride(unsigned char* smem, const Riders r, int b) {
  if (b < r.cblocks) {
    const int cb = b / r.crow_blocks;
    const long long rb = b - cb * r.crow_blocks;
    if (r.cdtype == PVO_F16) c1t::conv1x1_c128_tile<pvo_half>(smem, r.cx, r.cw, r.cbias, r.cy, r.crows, r.cCout, 0, rb, cb);
    else c1t::conv1x1_c128_tile<pvo_bf16>(smem, r.cx, r.cw, r.cbias, r.cy, r.crows, r.cCout, 0, rb, cb);
    return;
  }
  b -= r.cblocks;
  if (b < r.gblocks) {
    const int e = b / r.gchunks, ci = b - e * r.gchunks;
    if (r.gdtype == PVO_F16) glt::glo_partial_means<pvo_half>(smem, r.gnet, r.gw, r.gbias, r.gpart, r.gHW, 256, e, ci, r.gchunks);
    else glt::glo_partial_means<pvo_bf16>(smem, r.gnet, r.gw, r.gbias, r.gpart, r.gHW, 256, e, ci, r.gchunks);
    return;
  }
  b -= r.gblocks;
  if (b < r.xblocks) glt::gate_context_256(reinterpret_cast<float*>(smem), r.xpart, r.xwt, r.xbias, r.xg, r.xchunks, b);
}

// The end of every pose solve: dx out (the workspace copy the depth back-substitution reads, and the caller's), retraction of the
// poses [g0, g1) this workgroup owns, then - with `status` - thread 0's status words.  x(idx) = entry idx of the solution; a failed
// solve gives zeros (:1186-1189), and with nan_to_zero (the dense forms) so does a NaN entry.  `retracted` stamps a probe.  A
// workgroup of 256 threads (every solve kernel's; the constant stride keeps the dense solves' register allocation as it was).
template <class X, class Stamp>
__device__ __forceinline__ void solve_epilogue(X x, int failed, bool nan_to_zero, int g0, int g1, int t0, float* __restrict__ poses,
                                               float* __restrict__ dx_ws, float* __restrict__ dx_out, int* __restrict__ meta,
                                               int* __restrict__ status_out, bool status, Stamp retracted) {
  for (int idx = 6 * g0 + threadIdx.x; idx < 6 * g1; idx += 256) {
    float v = 0.0f;
    if (!failed) { const double xv = x(idx); v = (nan_to_zero && !(xv == xv)) ? 0.0f : static_cast<float>(xv); }
    dx_ws[idx] = v;
    if (dx_out) dx_out[idx] = v;
  }
  __syncthreads();
  for (int p = g0 + threadIdx.x; p < g1; p += 256) {                     // pose_retr_kernel (:877-910)
    float xi[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) xi[c] = dx_ws[6 * p + c];
    float* ps = poses + 7 * static_cast<long long>(t0 + p);
    const Pose T = retract(xi, load_pose(ps));
    ps[0] = T.t.x; ps[1] = T.t.y; ps[2] = T.t.z;
    ps[3] = T.q.x; ps[4] = T.q.y; ps[5] = T.q.z; ps[6] = T.q.w;
  }
  __syncthreads();
  retracted();
  if (threadIdx.x == 0 && status) {
    meta[4] = 0;
    if (failed) meta[1] = 1;
    if (status_out) { status_out[0] = meta[1]; status_out[1] = meta[0]; status_out[2] = meta[2]; status_out[3] = meta[3]; }
  }
}

// ---- the ENVELOPE pose solve: one chain, or PARTITIONED (systems beyond the dense matrix-core solve: the global BA) ---------
// Reads what ba_prepare_kernel / ba_prepare_packed_kernel left: the damped fp64 system in the compact envelope layout (dense in
// global memory when that does not fit the LDS budget) and in `xchg` the partition, m = s = 0 for none.
// ONE CHAIN (m = 0): workgroup 0 factorises the whole system with the bit-identical form `chol` names - 0 chol_solve_blocked,
// 1 chol_solve_wave, 2 chol_solve_pipe (the shipped one; the wave form when its active-row lists do not fit).  tools/
// ba_solve_timeline.py: cycles of the whole solve at 7 free poses 44.8 k blocked / 48.0 k wave / 52.1 k pipe, 12: 87.5 k blocked /
// 86.0 k pipe, 21: 168 k / 157 k, 63: 578 k blocked / 485 k wave / 364 k pipe - the pipeline wins once the envelope makes most of a
// step's candidate rows inactive.
// PARTITIONED: the factorisation is a serial chain of P block columns (chol_solve_pipe: ~4 k cycles each), replicated on every rank
// of an edge-sharded run.  A keyframe graph's pose system is block-banded away from its loop closures, and a banded chain can be
// eliminated from BOTH ends at once (a "twisted" factorisation, the two-way case of nested dissection): ba_prepare_kernel
// picks poses m <= s (choose_partition) such that nothing below m couples with anything from s on; then
//   workgroup 0   loads block rows [0, s), eliminates [0, m), waits for workgroup 1's terms on the separator [m, s), adds them,
//                 eliminates the separator, substitutes back, hands the separator's solution over, retracts poses [0, s);
//   workgroup 1   loads block rows [m, P) REVERSED (local row l = pose P - 1 - l, blocks transposed: eliminating from the far
//                 end is the ordinary factorisation of the reversed matrix, whose envelope is the column envelope `reach`),
//                 with the separator x separator blocks and the separator's right-hand side ZERO, eliminates its interior
//                 [s, P) - what is left in the separator's blocks is exactly its Schur-complement term -, writes that to
//                 global memory, waits for the separator's solution, substitutes back, retracts poses [s, P).
// Both run chol_pipe_range / pipe_backsub, i.e. the pipelined factorisation of the whole chain on their part; the order
// of elimination differs from the one-chain solve, so the result agrees with it to fp64 rounding, not bit for bit - and it
// is the same on every rank, because every rank factorises the same (all-reduced, integer) system with the same partition.
// Hand-over through global memory: data, agent-scope release fence, flag; the reader spins on the flag (bounded), acquires.
// Workgroups 0 and 1 of a dispatch are resident together (the first two to be placed), so the wait cannot deadlock; if a
// limit is hit anyway the solve reports failure (zero update) instead of hanging.
// (-DPVO_BA_PROBE, tools/ba_solve_timeline.py: the constant-rate 100 MHz clock - the two workgroups sit on different CUs -
// at the phases of either part, slots 32 + 16 * part + k)
#ifdef PVO_BA_PROBE
#define TWIN_PROBE(k) do { if (g_ba_probe && threadIdx.x == 0) g_ba_probe[32 + 16 * blockIdx.x + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define TWIN_PROBE(k)
#endif
constexpr int kTwinSpinLimit = 1 << 18;
__device__ __forceinline__ int twin_wait(int* flag) {                      // thread 0: 1 = data ready, 2 = the other side failed / timeout
  int v = 0, spins = 0;
  while ((v = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0) {
    if (++spins > kTwinSpinLimit) return 2;
    __builtin_amdgcn_s_sleep(8);
  }
  return v;
}

__global__ __launch_bounds__(256) void ba_solve_twin_kernel(
    double* __restrict__ chol_global, float* __restrict__ poses, float* __restrict__ dx_ws, float* __restrict__ dx_out,
    int* __restrict__ meta, int* __restrict__ status_out, int P, int t0, int* __restrict__ env, long long lds_budget,
    double* __restrict__ xchg, int chol, Riders riders) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  if (blockIdx.x > 1) {
    ride(smem, riders, blockIdx.x - 2);
    return;
  }
  int* xi = reinterpret_cast<int*>(xchg);                                  // 0: terms ready  1: solution ready  2: m  3: s
  const int m = xi[2], s = xi[3];
  const bool split = m > 0, bottom = blockIdx.x == 1;
  if (bottom && !split) return;
  int& fail = *reinterpret_cast<int*>(smem);
  __shared__ int first[kMaxEnvBlocks];
  __shared__ int reach[kMaxEnvBlocks];
  __shared__ unsigned short act_rows[2][kMaxActiveRows];
  __shared__ PipeCtl pipe_ctl;
  __shared__ int blocks_s, got_s;
  const int meta4 = meta[4] | meta[2];      // (meta[2]: eta's row count != K - the whole step is a no-op)
  if (threadIdx.x == 0) {
    fail = 0;
    pipe_ctl.panel = -1; pipe_ctl.done[0] = pipe_ctl.done[1] = pipe_ctl.done[2] = -1; pipe_ctl.abort = 0; pipe_ctl.total = 0;
  }
  const int n = 6 * P;
  TWIN_PROBE(0);
  // the global tables: first[] and the offsets of the compact layout ba_prepare_kernel wrote, the column envelope
  int* tmp = reinterpret_cast<int*>(smem + 16);
  env_layout(env, P, first, tmp, &blocks_s);
  const int blocks = blocks_s;
  if (!split) {
    BA_PROBE(0);
    double* blk = reinterpret_cast<double*>(smem + 16);
    double* rhs = blk + blocks;
    double* Ld = rhs + n;
    int* rowbase = reinterpret_cast<int*>(Ld + 27 * P + 24);
    const bool compact = env_lds_bytes(blocks, n, P) <= lds_budget;
    double* xrow;
    if (compact) {
      // (the offsets env_layout computed into the scratch copy move to their place behind the doubles; the scratch is about to be
      // overwritten by the matrix, so they travel through registers)
      int rb_keep[kMaxEnvBlocks / 256];
#pragma unroll
      for (int q = 0; q < kMaxEnvBlocks / 256; ++q) {
        const int b = q * 256 + threadIdx.x;
        rb_keep[q] = b < P ? tmp[b] : 0;
      }
      __syncthreads();
      // 124 KB at 63 poses through one workgroup: sixteen 16-byte loads in flight per thread, every one unconditional on a clamped
      // index (one 8-byte load at a time was 57 k cycles of latency; a guarded `v[u] = src[i]` sends the array to scratch)
      const int nd2 = (blocks + n) >> 1;
      const double2* src = reinterpret_cast<const double2*>(chol_global);
      double2* dst = reinterpret_cast<double2*>(blk);
      for (int base = 0; base < nd2; base += 16 * blockDim.x) {
        double2 v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) { const int i = base + u * blockDim.x + threadIdx.x; v[u] = src[i < nd2 ? i : nd2 - 1]; }
#pragma unroll
        for (int u = 0; u < 16; ++u) { const int i = base + u * blockDim.x + threadIdx.x; if (i < nd2) dst[i] = v[u]; }
      }
      if (((blocks + n) & 1) && threadIdx.x == 0) blk[blocks + n - 1] = chol_global[blocks + n - 1];
#pragma unroll
      for (int q = 0; q < kMaxEnvBlocks / 256; ++q) {
        const int b = q * 256 + threadIdx.x;
        if (b < P) rowbase[b] = rb_keep[q] - 36 * first[b];                  // (as EnvMat::rowoff)
      }
      for (int b = threadIdx.x; b < P; b += blockDim.x) env[b] = 0x7fffffff;
      __syncthreads();
      envelope_reach(first, reach, P);
      BA_PROBE(1);
      const EnvMat A{blk, rhs, rowbase, n};
      if (chol == 2 && pipe_lists(first, reach, P, act_rows[0], &pipe_ctl)) chol_solve_pipe(A, Ld, n, &fail, first, reach, act_rows[0], &pipe_ctl);
      else if (chol >= 1) { if (threadIdx.x < 64) chol_solve_wave(A, Ld, n, &fail, first, reach, act_rows[0]); }
      else chol_solve_blocked(A, Ld, n, &fail, first, reach);
      xrow = rhs;
    } else {
      for (int b = threadIdx.x; b < P; b += blockDim.x) env[b] = 0x7fffffff;
      double* A = chol_global;
      __syncthreads();
      envelope_reach(first, reach, P);
      BA_PROBE(1);
      chol_solve_blocked(DenseMat{A, n}, A + static_cast<long long>(n) * n + n, n, &fail, first, reach);
      xrow = A + static_cast<long long>(n) * n;
    }
    __syncthreads();
    BA_PROBE(4);
    solve_epilogue([&](int i) { return xrow[i]; }, fail | meta4, false, 0, P, t0, poses, dx_ws, dx_out, meta, status_out, true, [] { BA_PROBE(5); });
    return;
  }

  // ---- partitioned
  envelope_reach(first, reach, P);                                         // column envelope of the whole system
  const int w = s - m, Pl = bottom ? P - m : s, nl = 6 * Pl;
  // the global tables move to the end of the dynamic segment (the image grows from its start; choose_partition left room)
  int* tail = reinterpret_cast<int*>(smem + ((lds_budget - 16LL * (P + 2)) & ~15LL));
  int* gfirst = tail, *grow = tail + (P + 2), *lrow = tail + 2 * (P + 2), *greach = tail + 3 * (P + 2);
  {
    int keep[4][kMaxEnvBlocks / 256];
#pragma unroll
    for (int q = 0; q < kMaxEnvBlocks / 256; ++q) {
      const int b = q * 256 + threadIdx.x;
      keep[0][q] = b < P ? first[b] : 0; keep[1][q] = b < P ? tmp[b] : 0; keep[2][q] = b < P ? reach[b] : 0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kMaxEnvBlocks / 256; ++q) {
      const int b = q * 256 + threadIdx.x;
      if (b < P) { gfirst[b] = keep[0][q]; grow[b] = keep[1][q]; greach[b] = keep[2][q]; }
    }
    if (threadIdx.x == 0) grow[P] = blocks;
    __syncthreads();
  }
  // this part's envelope: the separator's rows are dense inside the separator (the other part's elimination fills them)
  for (int l = threadIdx.x; l < Pl; l += blockDim.x) {
    int f;
    if (!bottom) f = l < m ? gfirst[l] : min(gfirst[l], m);
    else { const int g = P - 1 - l; f = P - 1 - greach[g]; if (l >= P - s) f = min(f, P - s); }
    first[l] = f;
  }
  __syncthreads();
  const int lblocks = env_layout(first, Pl, first, lrow, &blocks_s);       // (reads first[b] as the envelope, writes min(first[b], b) back)
  double* blk = reinterpret_cast<double*>(smem + 16);
  double* rhs = blk + lblocks;
  double* Ld = rhs + nl;
  int* rowoff = reinterpret_cast<int*>(Ld + 27 * Pl + 24);
  const bool room = reinterpret_cast<unsigned char*>(rowoff + Pl + 2) <= reinterpret_cast<unsigned char*>(tail);
  if (!room) {                                                             // (choose_partition checked a bound of this: not reached)
    if (threadIdx.x == 0) fail = 1;
  } else {
    for (int i = threadIdx.x; i < lblocks + nl; i += blockDim.x) blk[i] = 0.0;
    for (int l = threadIdx.x; l < Pl; l += blockDim.x) rowoff[l] = lrow[l] - 36 * first[l];
  }
  __syncthreads();
  TWIN_PROBE(1);
  if (room) {
    // source: whole block rows of the compact image, [0, s) for the top part, [s, P) for the bottom part.  Rows [0, m) keep
    // their layout: a straight copy.  Everything else is placed pair by pair (offsets are multiples of 36, so a 16-byte pair
    // never straddles a block): sixteen loads in flight per thread, the row search and the index arithmetic behind them.
    const double2* src2 = reinterpret_cast<const double2*>(chol_global);
    if (!bottom) {
      const int nd2 = grow[m] >> 1;
      double2* dst2 = reinterpret_cast<double2*>(blk);
      for (int base = 0; base < nd2; base += 16 * blockDim.x) {
        double2 v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) { const int i = base + u * blockDim.x + threadIdx.x; v[u] = src2[i < nd2 ? i : nd2 - 1]; }
#pragma unroll
        for (int u = 0; u < 16; ++u) { const int i = base + u * blockDim.x + threadIdx.x; if (i < nd2) dst2[i] = v[u]; }
      }
    }
    const int p0 = (bottom ? grow[s] : grow[m]) >> 1, p1 = (bottom ? blocks : grow[s]) >> 1;
    for (int base = p0; base < p1; base += 16 * blockDim.x) {
      double2 v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) { const int i = base + u * blockDim.x + threadIdx.x; v[u] = src2[i < p1 ? i : p1 - 1]; }
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int i2 = base + u * blockDim.x + threadIdx.x;
        if (i2 >= p1) continue;
        const int i = 2 * i2;
        int lo = bottom ? s : m, hi = bottom ? P : s;                      // row rb with grow[rb] <= i < grow[rb + 1]
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (grow[mid] <= i) lo = mid; else hi = mid; }
        const int rb = lo, k = i - grow[rb], kb36 = k / 36, e = k - 36 * kb36, cb = gfirst[rb] + kb36;
        if (!bottom) {
          *reinterpret_cast<double2*>(blk + rowoff[rb] + 36 * cb + e) = v[u];
        } else {
          const int ri = e / 6, ci = e - 6 * ri;                           // (e even: ci and ci + 1 lie in one row)
          const int l = P - 1 - cb, lp = P - 1 - rb;                       // block (rb, cb) -> block (l, lp), transposed
          double* dst = blk + rowoff[l] + 36 * lp + 6 * ci + ri;
          dst[0] = v[u].x; dst[6] = v[u].y;
        }
      }
    }
    if (!bottom) { for (int i = threadIdx.x; i < 6 * s; i += blockDim.x) rhs[i] = chol_global[blocks + i]; }
    else { for (int i = threadIdx.x; i < 6 * (P - s); i += blockDim.x) { const int l = i / 6; rhs[i] = chol_global[blocks + 6 * (P - 1 - l) + (i - 6 * l)]; } }
  }
  __syncthreads();
  TWIN_PROBE(2);
  bool lists = false;
  if (room) {
    envelope_reach(first, reach, Pl);
    lists = pipe_lists(first, reach, Pl, act_rows[0], &pipe_ctl);
    if (!lists && threadIdx.x == 0) fail = 1;
  }
  __syncthreads();
  const EnvMat A{blk, rhs, rowoff, nl};
  TWIN_PROBE(3);
  double* cterm = xchg + 2;                                                // [w][w][36] rows a >= c, then the rhs [6 w], then x [6 w]
  double* crhs = cterm + 36 * kMaxSep * kMaxSep;
  double* xsep = crhs + 6 * kMaxSep;
  if (!bottom) {
    if (!fail) chol_pipe_range(A, Ld, Pl, &fail, reach, act_rows[0], &pipe_ctl, 0, m);
    __syncthreads();
    TWIN_PROBE(4);
    if (threadIdx.x == 0) got_s = twin_wait(&xi[0]);                       // (always: workgroup 1 reads `env`, reset below)
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (got_s != 1 && threadIdx.x == 0) fail = 1;
    TWIN_PROBE(5);
    for (int b = threadIdx.x; b < P; b += blockDim.x) env[b] = 0x7fffffff;
    __syncthreads();
    if (!fail) {
      for (int t = threadIdx.x; t < 36 * w * w; t += blockDim.x) {
        const int pr = t / 36, e = t - 36 * pr, a = pr / w, c = pr - a * w;
        if (c > a) continue;
        blk[rowoff[m + a] + 36 * (m + c) + e] += cterm[(a * kMaxSep + c) * 36 + e];
      }
      for (int t = threadIdx.x; t < 6 * w; t += blockDim.x) rhs[6 * m + t] += crhs[t];
    }
    __syncthreads();
    TWIN_PROBE(6);
    if (!fail) chol_pipe_range(A, Ld, Pl, &fail, reach, act_rows[0], &pipe_ctl, m, s);
    __syncthreads();
    TWIN_PROBE(7);
    if (!fail) pipe_backsub(A, Ld, first, Pl - 1, Pl, m);                   // the separator's unknowns first: the other part waits for them
    __syncthreads();
    TWIN_PROBE(8);
    if (threadIdx.x < 6 * w) xsep[threadIdx.x] = fail ? 0.0 : rhs[6 * m + threadIdx.x];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(&xi[1], fail ? 2 : 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    TWIN_PROBE(9);
    if (!fail) pipe_backsub(A, Ld, first, m - 1, Pl);
  } else {
    if (!fail) chol_pipe_range(A, Ld, Pl, &fail, reach, act_rows[0], &pipe_ctl, 0, P - s);
    __syncthreads();
    TWIN_PROBE(4);
    if (!fail) {
      for (int t = threadIdx.x; t < 36 * w * w; t += blockDim.x) {
        const int pr = t / 36, e = t - 36 * pr, a = pr / w, c = pr - a * w;
        if (c > a) continue;
        const int ri = e / 6, ci = e - 6 * ri;
        const int l = P - 1 - (m + c), lp = P - 1 - (m + a);               // global block (m + a, m + c), a >= c  <-  local (l, lp), l >= lp
        cterm[(a * kMaxSep + c) * 36 + e] = blk[rowoff[l] + 36 * lp + (a == c ? 6 * ri + ci : 6 * ci + ri)];
      }
      for (int t = threadIdx.x; t < 6 * w; t += blockDim.x) { const int a = t / 6; crhs[t] = rhs[6 * (P - 1 - (m + a)) + (t - 6 * a)]; }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    if (threadIdx.x == 0) {
      __hip_atomic_store(&xi[0], fail ? 2 : 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      TWIN_PROBE(5);
      got_s = twin_wait(&xi[1]);
    }
    __syncthreads();
    TWIN_PROBE(6);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (got_s != 1 && threadIdx.x == 0) fail = 1;
    __syncthreads();
    if (!fail) {
      for (int t = threadIdx.x; t < 6 * w; t += blockDim.x) { const int a = t / 6; rhs[6 * (P - 1 - (m + a)) + (t - 6 * a)] = xsep[t]; }
    }
    __syncthreads();
    if (!fail) pipe_backsub(A, Ld, first, Pl - 1, P - s);
  }
  __syncthreads();
  TWIN_PROBE(10);
  // the poses this part owns; the bottom part's right-hand side is reversed
  auto x = [&](int i) { const int g = i / 6; return rhs[bottom ? 6 * (P - 1 - g) + (i - 6 * g) : i]; };
  solve_epilogue(x, fail | meta4, false, bottom ? s : 0, bottom ? P : s, t0, poses, dx_ws, dx_out, meta, status_out, !bottom,
                 [] { TWIN_PROBE(11); });
}

// ---- the DENSE pose solve on the fp64 matrix cores (round 6): windows up to kDenseMaxPoses free poses, one launch ---------------
// A frontend window's pose system is DENSE: 21-25 free poses whose ~400 inactive edges couple almost every pair
// (factor_graph.py:281-291; bench.py `sequence.ba_windows_sampled`).  The envelope forms above gain nothing there and paid for it:
// beyond 21 poses env + prepare + partitioned solve = three launches, 16 + 100 us per Gauss-Newton step, the partition finding no
// separator and one workgroup walking a 25-column chain at ~9 k cycles per block column - most of them the rank-6 trailing update
// read and written through LDS (27 LDS operations per 36 multiply-adds).
// Here the whole lower triangle lives in the REGISTERS of one workgroup, as 16 x 16 accumulator tiles of
// v_mfma_f64_16x16x4_f64 dealt round-robin over the four waves (a 26-pose system: 55 tiles, 14 per wave, 112 VGPRs):
//   per step of EIGHT columns (20 steps for 156 rows; a panel never straddles a tile column):
//     1. the tiles of the panel's tile column write its eight columns to the panel's place in LDS (+ the 8 x 8 diagonal block apart)
//     2. one lane per row: the 8 x 8 Cholesky redundantly in registers, then its own row of the panel (forward substitution
//        against the diagonal block) - in place; the finished panels ARE the factor L, kept for the back-substitution
//     3. every tile right of / below the panel: C -= L_rows(i) L_rows(j)^T, two MFMAs (K = 8), operands straight from the panel
//   two barriers per step; the trailing matrix never touches LDS.  The right-hand side rides as row n of the matrix (as in the
//   forms above), so the forward substitution is part of step 2; the back-substitution is wave 0's: one lane per column, the
//   panel's eight unknowns by v_readlane, no LDS exchange of the vector.
// Loads the fixed-point system itself (lower block triangle + right-hand side; zeroes ALL of it for the next step), damping as
// droid_kernels.cu:1176, failure -> zero update (:1186-1189).  Deterministic: a fixed order of fp64 operations on an integer
// system, so every rank of an edge-sharded run that takes this path gets the same bits; against the envelope forms the order of
// the additions differs: equal to fp64 rounding, not bit for bit (tests: oracle parity at 1e-4 in fp32 outputs, and agreement
// with the pipelined form to 4e-7 relative).
constexpr int kDenseMaxPoses = 29;      // N = 16 ceil((6 P + 1) / 16) <= 176: 66 tiles (17 per wave), 129.5 KB of panels in LDS
typedef double pvo_d4 __attribute__((ext_vector_type(4)));

__host__ __device__ __forceinline__ int dense_N(int n) { return ((n + 1 + 15) / 16) * 16; }
__host__ __device__ __forceinline__ int dense_panel_off(int kb8, int N) { return kb8 * N - 4 * kb8 * (kb8 - 1); }      // rows in front of panel kb8
__host__ __forceinline__ size_t dense_lds_bytes(int n) {
  const int N = dense_N(n), nb = N / 8;
  return 16 + sizeof(double) * (8 * static_cast<size_t>(dense_panel_off(nb, N)) + 64 + 2 * static_cast<size_t>(N));
}

#ifdef PVO_BA_PROBE
#define DENSE_STEP_PROBE(slot) do { if (g_ba_probe && threadIdx.x == 0 && kb8 == nb / 2) g_ba_probe[slot] = __builtin_readcyclecounter(); } while (0)
#else
#define DENSE_STEP_PROBE(slot)
#endif
// element (row t of a panel, column k of its eight) sits at t * 8 + (k ^ ((t >> 1) & 7)): the matrix-core operand reads take ONE
// column of 16 consecutive rows per 16 lanes - at a plain 64-byte row pitch that is an 8-way bank conflict on every read
__device__ __forceinline__ int dense_swz(int t, int k) { return t * 8 + (k ^ ((t >> 1) & 7)); }
// 1 / sqrt(d): hardware estimate + ONE Newton step (the estimate carries ~26 bits: ~1.5 ulp after the step; the outputs are fp32).
// The second step of rsqrt_nr was 4 of the ~12 dependent fp64 operations per column on this kernel's critical chain.
__device__ __forceinline__ double rsqrt_nr1(double d) {
  const double y = __builtin_amdgcn_rsq(d);
  return y * (1.5 - 0.5 * d * y * y);
}

template <int SLOTS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void ba_solve_dense_kernel(
    long long* __restrict__ sys, const long long* __restrict__ msg, const int* __restrict__ first_s,
    float* __restrict__ poses, float* __restrict__ dx_ws, float* __restrict__ dx_out,
    int* __restrict__ meta, int* __restrict__ status_out, int P, int t0, float lm, float ep, Riders riders) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // [16 B flags | panels | diagonal block | 1 / L_jj | x]
  if (blockIdx.x > 0) {                                                  // rider workgroups (launched only with riders)
    ride(smem, riders, blockIdx.x - 1);
    return;
  }
  // msg != NULL: the system arrives as the packed envelope message of an edge-sharded step (ba_pack_kernel's layout: block row b =
  // blocks first[b] .. b of 36, then the right-hand side) instead of the dense image - same values into the same tiles, so a
  // sharded run gets the bits of the whole graph on one GPU at these sizes too
  __shared__ int mfirst[kDenseMaxPoses + 1], mbase[kDenseMaxPoses + 2];
  if (msg) {
    if (threadIdx.x == 0) {
      int run = 0;
      for (int b = 0; b < P; ++b) {
        const int e = first_s[b];
        const int f = e < b ? (e < 0 ? 0 : e) : b;                       // (clamped as env_layout does)
        mfirst[b] = f; mbase[b] = run; run += (b - f + 1) * 36;
      }
      mbase[P] = run;
    }
    __syncthreads();
  }
  int& fail = *reinterpret_cast<int*>(smem);
  const int n = 6 * P, N = dense_N(n), T = N / 16, nb = (n + 7) / 8;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // (uniform: the tile tables below live in scalar registers)
  const int lr = lane >> 4, lc = lane & 15;                              // C / D: row lr + 4 r, column lc; A / B: index lc, k = lr
  double* Lp = reinterpret_cast<double*>(smem + 16);
  double* Dg = Lp + 8 * dense_panel_off(N / 8, N);
  double* rdg = Dg + 64;
  double* xs = rdg + N;
  if (tid == 0) fail = 0;
  BA_PROBE(0);
#ifdef PVO_BA_PROBE
  if (g_ba_probe && tid == 0) g_ba_probe[15] = 0xD15E;                    // (tools/ba_solve_timeline.py: the step stamps below are this kernel's)
#endif

  // ---- this wave's tiles: the lower triangle's tiles in COLUMN-major order (tile column 0 top to bottom, then column 1, ...),
  // q = 4 slot + wave.  The tiles a step still has to update are then a SUFFIX of every wave's slots and the tiles of one tile
  // column a short run of them: the unrolled slot code is entered through one jump instead of one branch per slot
  int tti[SLOTS], ttj[SLOTS];
  const int ntiles = T * (T + 1) / 2;
  auto colstart = [&](int c) { return c * T - c * (c - 1) / 2; };         // index of tile (c, c)
  auto first_slot = [&](int c) { const int q0 = colstart(c) - wave; return q0 > 0 ? (q0 + 3) >> 2 : 0; };      // this wave's first slot with tj >= c
#pragma unroll
  for (int sl = 0; sl < SLOTS; ++sl) {
    const int q = 4 * sl + wave;
    int tj = 0;
    while (tj + 1 < T && colstart(tj + 1) <= q) ++tj;
    tti[sl] = q < ntiles ? tj + (q - colstart(tj)) : -1;
    ttj[sl] = tj;
  }
  const int nsl = ntiles > wave ? (ntiles - wave + 3) >> 2 : 0;           // this wave's slots in use
  // ---- load: fixed point -> fp64 (+ damping on the diagonal, droid_kernels.cu:1176) straight into the accumulator tiles.  Every
  // load unconditional on a clamped index (a guarded load is a branch of its own; these are 32 in flight per lane)
  pvo_d4 C[SLOTS];
  auto load_tiles = [&](auto from_message) {
    constexpr bool MSG = decltype(from_message)::value;
    const long long* __restrict__ src = MSG ? msg : sys;
    constexpr int B = MSG ? 4 : SLOTS;       // slots per batch of loads: the dense image's addresses are cheap - all 4 SLOTS loads in flight at once (a round trip to the
                                             // memory side, where the atomics left the system, is ~3 us: four batches were 14 us of this kernel)
#pragma unroll
    for (int s0 = 0; s0 < SLOTS; s0 += B) {
      long long raw[B][4];
#pragma unroll
      for (int u = 0; u < B; ++u) {
        const int sl = s0 + u < SLOTS ? s0 + u : SLOTS - 1;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * tti[sl] + lr + 4 * r, col = 16 * ttj[sl] + lc;
          int idx = -1;
          const bool in = tti[sl] >= 0 && col < n;
          if (MSG) {
            const int rw = row < n ? row : 0;
            const int rb = rw / 6, cb = col / 6;
            const int body = mbase[rb] + (cb - mfirst[rb]) * 36 + (rw - 6 * rb) * 6 + (col - 6 * cb);
            idx = (in && row < n && col <= row && cb >= mfirst[rb]) ? body : ((in && row == n) ? mbase[P] + col : -1);
          } else {
            idx = (in && row < n && col <= row) ? row * n + col : ((in && row == n) ? n * n + col : -1);
          }
          const long long v = src[idx < 0 ? 0 : idx];
          raw[u][r] = idx < 0 ? 0LL : v;
        }
      }
#pragma unroll
      for (int u = 0; u < B; ++u) {
        if (s0 + u >= SLOTS) continue;
        const int sl = s0 + u;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * tti[sl] + lr + 4 * r, col = 16 * ttj[sl] + lc;
          double v = static_cast<double>(raw[u][r]) * kInvFix;
          if (row == col && row < n) v += static_cast<double>(ep) + static_cast<double>(lm) * v;
          C[sl][r] = v;
        }
      }
    }
  };
  if (msg) load_tiles(std::true_type{}); else load_tiles(std::false_type{});
  // the first panel's columns out of the accumulators (afterwards every step extracts the NEXT panel behind its own update)
  auto extract = [&](int kb8x) {
    const int tcx = kb8x >> 1, hx = kb8x & 1, c0x = 8 * kb8x;
    double* panx = Lp + 8 * dense_panel_off(kb8x, N);
    const int e0 = first_slot(tcx), e1x = first_slot(tcx + 1), e1 = e1x < nsl ? e1x : nsl;
    auto one = [&](const pvo_d4& Cs, int ti) {
      if ((lc >> 3) == hx) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * ti + lr + 4 * r;
          if (row >= c0x) {
            panx[dense_swz(row - c0x, lc & 7)] = Cs[r];
            if (row < c0x + 8) Dg[(row - c0x) * 8 + (lc & 7)] = Cs[r];
          }
        }
      }
    };
    switch (e0) {                                                         // (the column's slots are consecutive: one jump, then straight down)
#define PVO_DENSE_CASE(K) case K: if (K < SLOTS) { if (K >= e1) break; one(C[K < SLOTS ? K : 0], tti[K < SLOTS ? K : 0]); } [[fallthrough]];
      PVO_DENSE_CASE(0) PVO_DENSE_CASE(1) PVO_DENSE_CASE(2) PVO_DENSE_CASE(3) PVO_DENSE_CASE(4) PVO_DENSE_CASE(5)
      PVO_DENSE_CASE(6) PVO_DENSE_CASE(7) PVO_DENSE_CASE(8) PVO_DENSE_CASE(9) PVO_DENSE_CASE(10) PVO_DENSE_CASE(11)
      PVO_DENSE_CASE(12) PVO_DENSE_CASE(13) PVO_DENSE_CASE(14) PVO_DENSE_CASE(15) PVO_DENSE_CASE(16)
#undef PVO_DENSE_CASE
      default: break;
    }
  };
  extract(0);
  // (every entry the assembly / Schur kernels or an all-reduce may have written: ready for the next step's accumulation.  Behind a
  // barrier: a wave with few tiles would otherwise zero entries another wave has not loaded yet)
  __syncthreads();
  if (!msg) for (int idx = tid; idx < n * n + n; idx += 256) sys[idx] = 0LL;      // (ba_pack_kernel has zeroed the image a message came from)
  BA_PROBE(1);

  // ---- factorisation, eight columns per step.  At the head of a step the panel's columns (as the updates so far left them) and
  // its diagonal block are in LDS.
  for (int kb8 = 0; kb8 < nb; ++kb8) {
    const int tc = kb8 >> 1, h = kb8 & 1, c0 = 8 * kb8;
    double* pan = Lp + 8 * dense_panel_off(kb8, N);                      // rows c0 .. N-1 of columns c0 .. c0+7, 8 doubles per row (swizzled)
    DENSE_STEP_PROBE(8);
    // 2. one lane per row of the panel
    const int nv = (n - c0 < 8) ? n - c0 : 8;                           // columns of this panel that belong to the system (the rest: padding)
    if (tid < N - c0) {
      // the 8 x 8 Cholesky IN PLACE on the block's lower triangle; a diagonal slot ends up holding 1 / L_jj (L_jj itself is never
      // needed: the diagonal rows leave as d * rs through the row formula below) - registers are what bounds this kernel's occupancy
      double L[36], a[8];
      const int sw = (tid >> 1) & 7;
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = pan[tid * 8 + (j ^ sw)];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) L[i * (i + 1) / 2 + j] = Dg[i * 8 + j];
      }
      bool ok = true;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        double d = L[j * (j + 1) / 2 + j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[j * (j + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
        const bool real = j < nv;
        ok = ok && (!real || d > 0.0);
        const double rs = (real && ok) ? rsqrt_nr1(d) : 0.0;
        L[j * (j + 1) / 2 + j] = rs;
#pragma unroll
        for (int i = j + 1; i < 8; ++i) {
          double v = L[i * (i + 1) / 2 + j];
#pragma unroll
          for (int k = 0; k < j; ++k) v -= L[i * (i + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
          L[i * (i + 1) / 2 + j] = v * rs;
        }
        // this row's entry of column j as soon as the column's reciprocal pivot exists (the row's chain runs beside the block's)
        double v = a[j];
#pragma unroll
        for (int k = 0; k < j; ++k) v -= a[k] * L[j * (j + 1) / 2 + k];
        v *= rs;
        if (tid < 8 && j > tid) v = 0.0;                                 // (the diagonal block's rows: L is lower triangular)
        a[j] = v;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) pan[tid * 8 + (j ^ sw)] = a[j];
      if (tid < 8) {
        double r = L[0];
#pragma unroll
        for (int j = 1; j < 8; ++j) r = (tid == j) ? L[j * (j + 1) / 2 + j] : r;
        rdg[c0 + tid] = r;
      }
      if (tid == 0 && !ok) fail = 1;
    }
    DENSE_STEP_PROBE(9);
    __syncthreads();
    DENSE_STEP_PROBE(10);
    // 3. trailing update C -= L_rows(i) L_rows(j)^T of every tile with a column beyond the panel: this wave's slots from `u0` on,
    // two slots per block of straight-line code (eight operand reads in flight, the two tiles' MFMA pairs interleaved), entered
    // through one jump
    {
      const int u0 = first_slot(h == 0 ? tc : tc + 1);
      auto pair = [&](auto kc) {
        constexpr int K = decltype(kc)::value;
        constexpr int K1 = K + 1 < SLOTS ? K + 1 : K;
        const bool on0 = K >= u0 && K < nsl, on1 = K + 1 < SLOTS && K + 1 >= u0 && K + 1 < nsl;
        const int ta0 = on0 ? 16 * tti[K] + lc - c0 : 0, tb0 = on0 ? 16 * ttj[K] + lc - c0 : 0;
        const int ta1 = on1 ? 16 * tti[K1] + lc - c0 : 0, tb1 = on1 ? 16 * ttj[K1] + lc - c0 : 0;
        double a00 = pan[dense_swz(ta0, lr)], b00 = pan[dense_swz(tb0, lr)], a01 = pan[dense_swz(ta0, 4 + lr)], b01 = pan[dense_swz(tb0, 4 + lr)];
        double a10 = pan[dense_swz(ta1, lr)], b10 = pan[dense_swz(tb1, lr)], a11 = pan[dense_swz(ta1, 4 + lr)], b11 = pan[dense_swz(tb1, 4 + lr)];
        if (!on0) { a00 = 0.0; a01 = 0.0; }                              // (a slot below u0 in its pair / beyond this wave's tiles: C += 0)
        if (!on1) { a10 = 0.0; a11 = 0.0; }
        C[K] = __builtin_amdgcn_mfma_f64_16x16x4f64(-a00, b00, C[K], 0, 0, 0);
        if (K + 1 < SLOTS) C[K1] = __builtin_amdgcn_mfma_f64_16x16x4f64(-a10, b10, C[K1], 0, 0, 0);
        C[K] = __builtin_amdgcn_mfma_f64_16x16x4f64(-a01, b01, C[K], 0, 0, 0);
        if (K + 1 < SLOTS) C[K1] = __builtin_amdgcn_mfma_f64_16x16x4f64(-a11, b11, C[K1], 0, 0, 0);
      };
      switch (u0 >> 1) {
#define PVO_DENSE_PAIR(K) case K / 2: if (K < SLOTS) { if (K >= nsl) break; pair(std::integral_constant<int, (K < SLOTS ? K : 0)>{}); } [[fallthrough]];
        PVO_DENSE_PAIR(0) PVO_DENSE_PAIR(2) PVO_DENSE_PAIR(4) PVO_DENSE_PAIR(6) PVO_DENSE_PAIR(8) PVO_DENSE_PAIR(10) PVO_DENSE_PAIR(12)
        PVO_DENSE_PAIR(14) PVO_DENSE_PAIR(16)
#undef PVO_DENSE_PAIR
        default: break;
      }
    }
    DENSE_STEP_PROBE(11);
    if (kb8 + 1 < nb) extract(kb8 + 1);
    DENSE_STEP_PROBE(12);
    DENSE_STEP_PROBE(13);
    __syncthreads();
    DENSE_STEP_PROBE(14);
  }
  BA_PROBE(2);

  // ---- back-substitution L^T x = y (y = row n of L), wave 0: lane holds columns lane, lane + 64, lane + 128
  if (wave == 0) {
    double z[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      const int c = lane + 64 * m;
      z[m] = c < n ? Lp[8 * dense_panel_off(c >> 3, N) + dense_swz(n - 8 * (c >> 3), c & 7)] : 0.0;
    }
    for (int kb8 = nb - 1; kb8 >= 0; --kb8) {
      const int c0 = 8 * kb8, m0 = c0 >> 6, l0 = c0 & 63;
      const int nv = (n - c0 < 8) ? n - c0 : 8;
      const double* pan = Lp + 8 * dense_panel_off(kb8, N);
      // everything this step reads from LDS is independent of the unknowns: requested up front
      double Lk[28], rdv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        rdv[j] = rdg[c0 + j];
#pragma unroll
        for (int i = j + 1; i < 8; ++i) Lk[i * (i - 1) / 2 + j] = pan[dense_swz(i, j)];      // L[c0 + i][c0 + j]
      }
      const double zsel = m0 == 0 ? z[0] : (m0 == 1 ? z[1] : z[2]);
      double x[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int lo = __builtin_amdgcn_readlane(static_cast<int>(__double_as_longlong(zsel) & 0xffffffffLL), l0 + j);
        const int hi = __builtin_amdgcn_readlane(static_cast<int>(__double_as_longlong(zsel) >> 32), l0 + j);
        x[j] = __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned int>(lo));
      }
#pragma unroll
      for (int j = 7; j >= 0; --j) {
        double v = x[j];
#pragma unroll
        for (int i = 7; i > j; --i) v -= Lk[i * (i - 1) / 2 + j] * x[i];
        x[j] = (j < nv) ? v * rdv[j] : 0.0;
      }
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        const int c = lane + 64 * m;
        if (c < c0) {
          const double* pc = Lp + 8 * dense_panel_off(c >> 3, N);
          double v = z[m];
#pragma unroll
          for (int i = 0; i < 8; ++i) v -= pc[dense_swz(c0 + i - 8 * (c >> 3), c & 7)] * x[i];          // L[c0 + i][c]
          z[m] = v;
        } else if (c < c0 + 8) {
          double v = x[0];
#pragma unroll
          for (int j = 1; j < 8; ++j) v = (c - c0 == j) ? x[j] : v;
          z[m] = v;
        }
      }
    }
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      const int c = lane + 64 * m;
      if (c < n) xs[c] = z[m];
    }
  }
  __syncthreads();
  BA_PROBE(4);
  // (meta[2]: eta's row count != K - the whole step is a no-op, see ba_plan_kernel)
  solve_epilogue([&](int i) { return xs[i]; }, fail | meta[4] | meta[2], true, 0, P, t0, poses, dx_ws, dx_out, meta, status_out, true,
                 [] { BA_PROBE(5); });
}

// ---- BLOCKED pose solve over MANY workgroups (round 6): big systems that are not narrow-banded - the backend's global graph ---------
// A global bundle adjustment over ~85 keyframes connected by proximity (10-15 edges per frame) has an envelope of several hundred KB:
// it fits no compute unit's LDS, the partition finds no separator, and the one-workgroup factorisation then ran out of global memory
// - 1.8 ms per Gauss-Newton step, 38 of them in Droid.terminate (bench.py `sequence`, profiles/r06_sequence_timeline.txt).  At that
// point sparsity is not worth a CU's patience: the DENSE right-looking factorisation in 48 x 48 blocks, three launches per block column,
//   dense_panel_kernel   every workgroup factors the 48 x 48 diagonal block redundantly (one wave, rows in registers) and solves its own
//                        row block of the panel against it (one thread per row; the right-hand side rides as row n, so this is the
//                        forward substitution too); the diagonal block's workgroup stores the factor + reciprocal pivots apart
//   dense_update_kernel  A_ij -= L_ik L_jk^T, one workgroup per block pair of the trailing lower triangle (3 x 3 outputs per thread)
//   dense_back_kernel    back-substitution, block column by block column from the end: x_k from the stored diagonal factor (redundantly
//                        per workgroup), y_j -= L_kj^T x_k by the workgroup of column block j
// and dense_finish_kernel (dx, retraction, status; the riders ride here).  ~3 n / 48 + 3 launches, no host synchronisation; 85 poses:
// ~35 launches.  Same damping, failure -> zero update, fixed order of operations (bitwise reproducible); agrees with the other forms
// to fp64 rounding.  Chosen on the host by size and edge density (ba_finish_impl); never for a packed message.
constexpr int kNB = 48;
__global__ __launch_bounds__(256) void dense_panel_kernel(double* __restrict__ A, double* __restrict__ Ldiag, int n, int kb, int* __restrict__ meta) {
  // (everything in LDS, runtime loops: the first version kept a row per lane in 48 registers with every loop unrolled - 512 registers
  // and 8 KB of scratch per thread, 131 us per launch)
  __shared__ double Lk[kNB][kNB + 1];       // the diagonal block: lower triangle, factored in place (the diagonal itself stays, sqrt in ldg)
  __shared__ double Xs[kNB][kNB + 1];       // this workgroup's rows of the panel
  __shared__ double rinv[kNB], ldg[kNB];
  const int tid = threadIdx.x;
  const int c0 = kNB * kb, nc = (n - c0 < kNB) ? n - c0 : kNB;         // valid columns of this block column
  const int rb = kb + blockIdx.x, r0 = kNB * rb;                        // this workgroup's row block
  for (int t = tid; t < kNB * kNB; t += 256) {
    const int r = t / kNB, c = t - r * kNB;
    Lk[r][c] = (r < nc && c <= r) ? A[static_cast<size_t>(c0 + r) * n + c0 + c] : 0.0;
    const int rr = r0 + r;
    Xs[r][c] = (rr <= n && c < nc) ? A[static_cast<size_t>(rr) * n + c0 + c] : 0.0;
  }
  __syncthreads();
  // ---- factorisation of the diagonal block AND substitution of this workgroup's panel rows together, EIGHT columns per step (two
  // barriers per step; one column per step with a thread per entry was 48 x 2 barriers + a 48-step substitution: 53 us per launch):
  //   (a) one thread per row - rows of the diagonal block from the step's first column on, and the 48 panel rows -: the 8 x 8 Cholesky of
  //       the step's diagonal sub-block redundantly in registers, then the row's eight entries by forward substitution against it;
  //   (b) every entry right of the step's columns: E[r][c] -= sum_k row_r[k] L_c[k], a thread per (row, column stripe).
  // (The diagonal block's workgroup and every panel workgroup do the same arithmetic on the diagonal block: redundant, and identical.)
  bool ok = true;
  for (int j0 = 0; j0 < nc; j0 += 8) {
    const int nv = (nc - j0 < 8) ? nc - j0 : 8;
    double L[36], av[8];
    if (tid < 2 * kNB) {
      const bool isx = tid >= kNB;
      const int t = isx ? tid - kNB : tid;
      if (isx || (t >= j0 && t < nc)) {
        double (*Row)[kNB + 1] = isx ? Xs : Lk;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
#pragma unroll
          for (int j = 0; j <= i; ++j) L[i * (i + 1) / 2 + j] = Lk[j0 + i][j0 + j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) av[j] = Row[t][j0 + j];
      }
    }
    __syncthreads();                       // (the sub-block's own rows are rewritten below by their threads: everybody has read them)
    if (tid < 2 * kNB) {
      const bool isx = tid >= kNB;
      const int t = isx ? tid - kNB : tid;
      if (isx || (t >= j0 && t < nc)) {
        double (*Row)[kNB + 1] = isx ? Xs : Lk;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          double d = L[j * (j + 1) / 2 + j];
#pragma unroll
          for (int k = 0; k < j; ++k) d -= L[j * (j + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
          const bool real = j < nv;
          ok = ok && (!real || d > 0.0);
          const double rs = (real && ok) ? rsqrt_nr(d) : 0.0;
          if (!isx && t == j0 + j) { rinv[j0 + j] = rs; ldg[j0 + j] = d * rs; }
          L[j * (j + 1) / 2 + j] = rs;
#pragma unroll
          for (int i = j + 1; i < 8; ++i) {
            double v = L[i * (i + 1) / 2 + j];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= L[i * (i + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
            L[i * (i + 1) / 2 + j] = v * rs;
          }
          double v = av[j];
#pragma unroll
          for (int k = 0; k < j; ++k) v -= av[k] * L[j * (j + 1) / 2 + k];
          av[j] = v * rs;
        }
        // (a row of the diagonal sub-block itself: entry j == its own column is d * rs = the pivot's square root through the same formula;
        // entries right of its diagonal are not part of L - they are never read again)
#pragma unroll
        for (int j = 0; j < 8; ++j) if (j < nv && (isx || j0 + j <= t)) Row[t][j0 + j] = av[j];
      }
    }
    __syncthreads();
    const int c1 = j0 + 8;
    if (c1 < nc) {
      // rows: the diagonal block's rows r >= c1 (columns c1 .. r), then the 48 panel rows (columns c1 .. nc - 1); 16 column stripes
      const int ty = tid >> 4, tx = tid & 15;
      for (int r = c1 + ty; r < nc + kNB; r += 16) {
        const bool isx = r >= nc;
        double (*Row)[kNB + 1] = isx ? Xs : Lk;
        const int rr = isx ? r - nc : r;
        double a8[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) a8[k] = Row[rr][j0 + k];
        const int cend = isx ? nc - 1 : rr;
        for (int c = c1 + tx; c <= cend; c += 16) {
          double v = Row[rr][c];
#pragma unroll
          for (int k = 0; k < 8; ++k) v -= a8[k] * Lk[c][j0 + k];
          Row[rr][c] = v;
        }
      }
    }
    __syncthreads();
  }
  if (tid == kNB && !ok) meta[4] = 1;      // non-SPD (the first panel-row thread factors every sub-block): the finish kernel writes the zero update
  if (tid >= nc && tid < kNB) { rinv[tid] = 0.0; ldg[tid] = 0.0; }
  __syncthreads();
  for (int t = tid; t < kNB * kNB; t += 256) {
    const int r = t / kNB, c = t - r * kNB;
    const int rr = r0 + r;
    if (rr <= n && c < nc && (rb > kb || r >= nc)) A[static_cast<size_t>(rr) * n + c0 + c] = Xs[r][c];
  }
  if (blockIdx.x == 0) {                                                 // the diagonal block's workgroup keeps the factor for the back-substitution
    double* Ld = Ldiag + static_cast<size_t>(kb) * (kNB * kNB + kNB);
    for (int t = tid; t < kNB * kNB; t += 256) {
      const int r = t / kNB, c = t - r * kNB;
      Ld[t] = (r < nc && c < r) ? Lk[r][c] : ((r == c && r < nc) ? ldg[r] : 0.0);
    }
    if (tid < kNB) Ld[kNB * kNB + tid] = rinv[tid];
  }
}

__global__ __launch_bounds__(256) void dense_update_kernel(double* __restrict__ A, int n, int kb, int nrb) {
  __shared__ double Li[kNB][kNB + 1], Lj[kNB][kNB + 1];
  // block pair p -> (i, j), kb < j <= i < nrb
  const int m = nrb - kb - 1;
  int p = blockIdx.x, jj = 0;
  while (p >= m - jj) { p -= m - jj; ++jj; }
  const int bj = kb + 1 + jj, bi = bj + p;
  const int tid = threadIdx.x;
  const int c0 = kNB * kb, nc = (n - c0 < kNB) ? n - c0 : kNB;
  for (int t = tid; t < kNB * kNB; t += 256) {
    const int r = t / kNB, c = t - r * kNB;
    const int ri = kNB * bi + r, rj = kNB * bj + r;
    Li[r][c] = (ri <= n && c < nc) ? A[static_cast<size_t>(ri) * n + c0 + c] : 0.0;
    Lj[r][c] = (rj < n && c < nc) ? A[static_cast<size_t>(rj) * n + c0 + c] : 0.0;        // (columns of the target block: rows rj < n)
  }
  __syncthreads();
  const int ty = tid >> 4, tx = tid & 15;                  // 3 x 3 outputs: rows 3 ty .., columns 3 tx ..
  double acc[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
#pragma unroll 4
  for (int k = 0; k < kNB; ++k) {
    double a[3], b[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) { a[u] = Li[3 * ty + u][k]; b[u] = Lj[3 * tx + u][k]; }
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
      for (int v = 0; v < 3; ++v) acc[u][v] += a[u] * b[v];
  }
#pragma unroll
  for (int u = 0; u < 3; ++u) {
    const int rr = kNB * bi + 3 * ty + u;
    if (rr > n) continue;
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      const int cc = kNB * bj + 3 * tx + v;
      if (cc < n && (bi > bj || cc <= rr)) A[static_cast<size_t>(rr) * n + cc] -= acc[u][v];
    }
  }
}

__global__ __launch_bounds__(256) void dense_back_kernel(const double* __restrict__ A, const double* __restrict__ Ldiag, double* __restrict__ yrow,
                                                         double* __restrict__ xvec, int n, int kb) {
  __shared__ double Lk[kNB][kNB + 1];
  __shared__ double s[kNB], xk[kNB], rinv[kNB];
  const int tid = threadIdx.x, lane = tid & 63;
  const int c0 = kNB * kb, nc = (n - c0 < kNB) ? n - c0 : kNB;
  const double* Ld = Ldiag + static_cast<size_t>(kb) * (kNB * kNB + kNB);
  for (int t = tid; t < kNB * kNB; t += 256) Lk[t / kNB][t % kNB] = Ld[t];
  if (tid < kNB) { rinv[tid] = Ld[kNB * kNB + tid]; s[tid] = tid < nc ? yrow[c0 + tid] : 0.0; }
  __syncthreads();
  if (tid < 64) {                                        // L_kk^T x_k = s, by one wave: x_j, then s_t -= L[j][t] x_j for t < j
    for (int j = nc - 1; j >= 0; --j) {
      if (lane == j) xk[j] = s[j] * rinv[j];
      const double xj = xk[j];                           // (the wave's own LDS write just above)
      if (lane < j) s[lane] -= Lk[j][lane] * xj;
    }
  }
  __syncthreads();
  const int bj = blockIdx.x;                             // column block j < kb: y_j -= L[rows of block kb][columns of block j]^T x_k;  bj == kb: keep x_k
  if (bj == kb) {
    if (tid < nc) xvec[c0 + tid] = xk[tid];
    return;
  }
  if (tid < kNB) {
    const int col = kNB * bj + tid;
    double v = yrow[col];
    for (int r = 0; r < nc; ++r) v -= A[static_cast<size_t>(c0 + r) * n + col] * xk[r];
    yrow[col] = v;
  }
}

// (with P = 0 the whole of a solve: the status words, and the riders)
__global__ __launch_bounds__(256) void dense_finish_kernel(const double* __restrict__ xvec, float* __restrict__ poses, float* __restrict__ dx_ws,
                                                           float* __restrict__ dx_out, int* __restrict__ meta, int* __restrict__ status_out,
                                                           int P, int t0, Riders riders) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  if (blockIdx.x > 0) {                                                  // rider workgroups (launched only with riders)
    ride(smem, riders, blockIdx.x - 1);
    return;
  }
  solve_epilogue([&](int i) { return xvec[i]; }, meta[4] | meta[2], true, 0, P, t0, poses, dx_ws, dx_out, meta, status_out, true, [] {});
}
}  // namespace
