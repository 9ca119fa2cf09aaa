// scan.h — the two prefix sums every compaction here is made of (map_points.hip, tsdf_mesh.h, tsdf_sparse.hip): a lane's rank inside its
// wave from a 64-bit __ballot mask, and ONE workgroup's exclusive scan of per-workgroup counts in index order.  Integers only, no
// atomics: an output index is a function of the counts alone.
#pragma once
#include "common.h"

constexpr int kScanThreads = 1024;    // threads of a scan kernel

__device__ __forceinline__ int lanes_below(unsigned long long mask) {
  return __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(mask >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(mask), 0));
}

// inclusive scan of one value per thread of a 1024-thread workgroup (Hillis-Steele); total = the last thread's
__device__ __forceinline__ int scan_workgroup(int s, int (*buf)[kScanThreads], int& total) {
  const int tid = threadIdx.x;
  int cur = 0;
  buf[0][tid] = s;
  __syncthreads();
#pragma unroll
  for (int off = 1; off < kScanThreads; off <<= 1) {
    buf[cur ^ 1][tid] = buf[cur][tid] + (tid >= off ? buf[cur][tid - off] : 0);
    cur ^= 1;
    __syncthreads();
  }
  const int inc = buf[cur][tid];
  total = buf[cur][kScanThreads - 1];
  __syncthreads();                        // buf is reused by the next scan
  return inc;
}

// the contiguous chunk [lo, hi) of [0, M) that thread t of a scan kernel owns: [t * chunk, (t + 1) * chunk)
struct ScanChunk { int lo, hi; };

// exclusive scans of the K count arrays cnt[k][0, M) in index order, by the one workgroup of a scan kernel.  Returns the thread's chunk;
// run[k] = the sum of cnt[k][0, lo), total[k] = the sum of cnt[k].  The caller walks its chunk:  out[i] = run[k]; run[k] += cnt[k][i];
template <int K>
__device__ __forceinline__ ScanChunk scan_counts(const int* const (&cnt)[K], int M, int (&run)[K], int (&total)[K]) {
  const int tid = threadIdx.x;
  const int chunk = (M + kScanThreads - 1) / kScanThreads;
  const int lo = static_cast<int>(min(static_cast<long long>(tid) * chunk, static_cast<long long>(M))), hi = min(lo + chunk, M);
  __shared__ int buf[2][kScanThreads];
#pragma unroll
  for (int k = 0; k < K; ++k) run[k] = 0;
  for (int i = lo; i < hi; ++i) {         // (one pass over the chunk for all K: the loads of a pass overlap, two passes would not)
#pragma unroll
    for (int k = 0; k < K; ++k) run[k] += cnt[k][i];
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int s = run[k];
    run[k] = scan_workgroup(s, buf, total[k]) - s;
  }
  return {lo, hi};
}
