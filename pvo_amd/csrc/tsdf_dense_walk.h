// tsdf_dense_walk.h — the dense volume under the voxel walk of tsdf_fuse.h (tsdf.hip, tsdf_reintegrate.hip): the walker that gives a
// thread its voxel by raster index, and the kernel that writes the dense calls' frame table.
#pragma once
#include "tsdf_fuse.h"

namespace {

struct DenseWalk {
  static constexpr int kThreads = 256;
  int nz, ny, nx;
  struct Thread { long long i; float xf, yf, zf; bool live; };

  __device__ __forceinline__ bool enter(Thread& t) const {
    const long long total = static_cast<long long>(nz) * ny * nx;
    t.i = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x;
    t.live = t.i < total;
    return true;
  }
  __device__ __forceinline__ void locate(Thread& t) const {
    const int x = static_cast<int>(t.i % nx), y = static_cast<int>((t.i / nx) % ny), z = static_cast<int>(t.i / (static_cast<long long>(nx) * ny));
    t.xf = static_cast<float>(x); t.yf = static_cast<float>(y); t.zf = static_cast<float>(z);
  }
  template <typename Apply>
  __device__ __forceinline__ int for_each_frame(const Thread&, const float* __restrict__ fc, int N, const Intr, const Fuse, Apply apply) const {
    for (int b = 0; b < N; ++b) {
      const float* __restrict__ c = fc + static_cast<long long>(kFrameFloats) * b;      // wave-uniform
      const int f = __float_as_int(c[12]);
      if (f < 0) continue;
      apply(c, f);
    }
    return 0;
  }
  __device__ __forceinline__ void keep(int) const {}
};

struct FrameSet { const float* poses; const int64_t* ix; int N; };

// slots [0, first.N) from the first set, slots [first.N, first.N + second.N) from the second: per slot the twelve pre-multiplied
// constants  voxel * R  and  R origin + t  (so that Xc = A (x, y, z) + b for the INTEGER voxel index) and the frame id, -1 for an id
// outside [0, nframes): sixteen floats per slot
__global__ __launch_bounds__(64) void tsdf_frames_kernel(const FrameSet first, const FrameSet second, float* __restrict__ fc, int nframes,
                                                         const Vol vol) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= first.N + second.N) return;
  const bool one = b < first.N;
  const float* __restrict__ poses = one ? first.poses : second.poses;
  const long long f = one ? first.ix[b] : second.ix[b - first.N];
  float* o = fc + static_cast<long long>(kFrameFloats) * b;
  if (f < 0 || f >= nframes) {            // never dereferenced
    o[12] = __int_as_float(-1);
    return;
  }
  tsdf_frame_constants(poses, f, vol, o);
}

}  // namespace
