// tsdf_brick_cull.h — what the brick volume's integration (tsdf_sparse.hip) and re-integration (tsdf_reintegrate.hip) share beyond the
// voxel arithmetic of tsdf_fuse.h: the per-slot constants with the cull's scalars, the test of one slot against one brick, and the
// chunked cull of a whole table that hands a brick its surviving slots in order (the frame loop of BrickWalk, the brick volume's walker for the kernels of tsdf_fuse.h).  Both
// translation units launch the same kernel and call the same functions, so a brick keeps or drops a frame identically in either.
#pragma once
#include "scan.h"
#include "tsdf_fuse.h"
#include "tsdf_host.h"

namespace {

constexpr int kCullBlock = 256;       // threads of sparse_frames_kernel
using tsdf_volume::kB;
constexpr int kBrick = kB * kB * kB;  // 512 voxels, one workgroup
static_assert(kB == 8 && kBrick == 512, "the index arithmetic of the brick kernels shifts by 3 and 6");

// per slot: the dense call's constants [0..12]; [13] zfar = the largest 1/d over the frame's valid pixels (-inf without one: a max,
// so the order of the reduction does not matter); [14] |origin|_1 + |t|_1; [15] |1 - n| + n, n = |q|^2: R(q) as the contract
// writes it is (1 - n) I + n Rot(q / |q|), so this bounds its spectral norm (1 for a unit quaternion)
__global__ __launch_bounds__(kCullBlock) void sparse_frames_kernel(const float* __restrict__ poses, const int64_t* __restrict__ ix,
                                                                  const float* __restrict__ disps, const float* __restrict__ weight,
                                                                  float* __restrict__ fc, int nframes, long long HW, const Vol vol) {
  const int b = blockIdx.x, tid = threadIdx.x;
  float* o = fc + static_cast<long long>(kFrameFloats) * b;
  const long long f = ix[b];
  if (f < 0 || f >= nframes) {            // never dereferenced (the whole workgroup leaves)
    if (tid == 0) o[12] = __int_as_float(-1);
    return;
  }
  float m = -__builtin_inff();
  for (long long k = tid; k < HW; k += kCullBlock) {
    const float d = disps[f * HW + k];
    const float w = weight ? weight[f * HW + k] : 1.0f;
    if (d > 0.0f && d < __builtin_inff() && w > 0.0f && w < __builtin_inff()) m = fmaxf(m, 1.0f / d);
  }
  __shared__ float red[kCullBlock];
  red[tid] = m;
  __syncthreads();
  for (int off = kCullBlock / 2; off > 0; off >>= 1) {
    if (tid < off) red[tid] = fmaxf(red[tid], red[tid + off]);
    __syncthreads();
  }
  if (tid != 0) return;
  tsdf_frame_constants(poses, f, vol, o);
  const Pose G = load_pose(poses + 7 * f);
  const float n = (G.q.x * G.q.x + G.q.y * G.q.y) + (G.q.z * G.q.z + G.q.w * G.q.w);
  o[13] = red[0];
  o[14] = ((fabsf(vol.ox) + fabsf(vol.oy)) + fabsf(vol.oz)) + ((fabsf(G.t.x) + fabsf(G.t.y)) + fabsf(G.t.z));
  o[15] = fabsf(1.0f - n) + n;
}

// May a voxel of the brick get a contribution of the slot with constants c?  false ONLY if none can.  (X, Y, Z) is the camera-frame
// position of the brick's centre, index cc = 8 b + 3.5 (exact in fp32); every voxel centre of the brick is within
// r = 3.5 sqrt(3) voxel |R| of it.  What the voxel's thread decides on are its OWN fp32 values (xc, yc, zc), so the radius is
// inflated to cover the difference between exact and computed positions:
//   tests/tsdf_reference.py bounds the error of a computed camera coordinate by 12 EPS M, M = voxel (x + y + z) + |o|_1 + |t|_1, which
//   also bounds the coordinate's magnitude; over three coordinates that is sqrt(3) 12 < 21 EPS M for the voxel and as much for the
//   centre (M taken at the brick's largest index sum, msum).  Evaluating a test - three products and sums of magnitude <= 2 M, or
//   1/d - zc with its one rounding EPS (zfar + M) - adds less than 10 EPS (M + zfar + trunc + z_near).  Together < 52 EPS (M + zfar +
//   trunc + z_near); the slack is 2^-17 = 128 EPS of it, and r itself is stretched by 2^-16 for the roundings of A = voxel R (6 EPS per
//   entry), of c[15] and of this function's own products.
// The frustum's sides are widened by half a pixel: a voxel is used only if floor(u + 0.5) >= 0 for ITS computed u, whose error given
// the computed (xc, zc) is below 5 EPS (|u| + 2 |cx|) < 0.5 for image sizes and principal points below 2^19 (others: no side test),
// so the point (xc, yc, zc) itself satisfies u > -1, i.e. fx xc + (cx + 1) zc > 0 for zc > 0 - a half-space that the inflated sphere
// must reach.  Likewise u < wd, v > -1, v < ht.  Every comparison is written so that a NaN keeps the frame.
__device__ __forceinline__ bool brick_sees_frame(const float* __restrict__ c, float ccx, float ccy, float ccz, float msum, float voxel,
                                                 const Intr K, const Fuse in) {
  if (__float_as_int(c[12]) < 0) return false;
  const float zfar = c[13];
  if (!(zfar > 0.0f)) return false;                     // no valid pixel (zfar is a max of finite positives, or -inf)
  const float X = c[0] * ccx + c[1] * ccy + c[2] * ccz + c[9];
  const float Y = c[3] * ccx + c[4] * ccy + c[5] * ccz + c[10];
  const float Z = c[6] * ccx + c[7] * ccy + c[8] * ccz + c[11];
  const float M = msum + c[14];
  const float R = (6.0621778f * voxel * c[15]) * (1.0f + 0x1p-16f) + 0x1p-17f * (M + zfar + in.trunc + in.z_near);
  if (Z + R < in.z_near) return false;                  // behind z_near
  if (Z - R > zfar + in.trunc) return false;            // beyond every surface the frame sees
  const float wdf = static_cast<float>(in.wd), htf = static_cast<float>(in.ht);
  if (K.fx > 0.0f && K.fy > 0.0f && wdf < 0x1p19f && htf < 0x1p19f && fabsf(K.cx) < 0x1p19f && fabsf(K.cy) < 0x1p19f) {
    const float l = K.cx + 1.0f, r = wdf - K.cx, t = K.cy + 1.0f, bo = htf - K.cy;
    if (K.fx * X + l * Z < -R * sqrtf(K.fx * K.fx + l * l)) return false;
    if (r * Z - K.fx * X < -R * sqrtf(K.fx * K.fx + r * r)) return false;
    if (K.fy * Y + t * Z < -R * sqrtf(K.fy * K.fy + t * t)) return false;
    if (bo * Z - K.fy * Y < -R * sqrtf(K.fy * K.fy + bo * bo)) return false;
  }
  return true;
}

// the slots [0, N) of the table fc against the brick, 512 at a time (one per thread of the brick's workgroup); the survivors, in slot
// order, applied to the thread's voxel by `apply`.  list [512] and wave_n [8] are LDS.  Returns the number of survivors
template <typename Apply>
__device__ __forceinline__ int brick_cull_and_apply(const float* __restrict__ fc, int N, float ccx, float ccy, float ccz, float msum,
                                                    float voxel, const Intr K, const Fuse in, int* list, int* wave_n, Apply apply) {
  const int tid = threadIdx.x;
  int survivors = 0;
  for (int c0 = 0; c0 < N; c0 += kBrick) {
    // stage 1: slot c0 + tid against the brick; the survivors in slot order
    const int b = c0 + tid;
    const bool keep = b < N && brick_sees_frame(fc + static_cast<long long>(kFrameFloats) * b, ccx, ccy, ccz, msum, voxel, K, in);
    const unsigned long long m = __ballot(keep);
    if ((tid & 63) == 0) wave_n[tid >> 6] = __popcll(m);
    __syncthreads();
    int pos = lanes_below(m), n = 0;
#pragma unroll
    for (int w = 0; w < kBrick / 64; ++w) {
      if (w < (tid >> 6)) pos += wave_n[w];
      n += wave_n[w];
    }
    if (keep) list[pos] = b;
    survivors += n;
    __syncthreads();
    // stage 2: the dense walk's loop over the survivors
    for (int k = 0; k < n; ++k) {
      const int s = __builtin_amdgcn_readfirstlane(list[k]);
      const float* __restrict__ c = fc + static_cast<long long>(kFrameFloats) * s;    // wave-uniform
      apply(c, __float_as_int(c[12]));
    }
    __syncthreads();                      // list and wave_n are rewritten by the next chunk
  }
  return survivors;
}

// the brick volume under the voxel walk of tsdf_fuse.h: one workgroup per brick in use, one thread per voxel
struct BrickWalk {
  static constexpr int kThreads = kBrick;
  const int32_t* coord; const int32_t* bricks;
  int cap;
  float voxel;
  int32_t* kept;                          // [cap] or NULL
  struct Thread { long long i; float xf, yf, zf; bool live; float ccx, ccy, ccz, msum; int* list; int* wave_n; };

  __device__ __forceinline__ bool enter(Thread& t) const {
    const int slot = blockIdx.x;
    if (slot >= min(bricks[0], cap)) return false;
    t.i = static_cast<long long>(slot) * kBrick + threadIdx.x;
    t.live = true;
    return true;
  }
  __device__ __forceinline__ void locate(Thread& t) const {
    const int slot = blockIdx.x, tid = threadIdx.x;
    __shared__ int list[kBrick];
    __shared__ int wave_n[kBrick / 64];
    t.list = list; t.wave_n = wave_n;
    const int bz = coord[3 * slot], by = coord[3 * slot + 1], bx = coord[3 * slot + 2];
    const int x = kB * bx + (tid & 7), y = kB * by + ((tid >> 3) & 7), z = kB * bz + (tid >> 6);
    t.xf = static_cast<float>(x); t.yf = static_cast<float>(y); t.zf = static_cast<float>(z);
    // the brick's centre (exact in fp32) and its largest index sum, for the cull
    t.ccx = static_cast<float>(kB * bx) + 3.5f; t.ccy = static_cast<float>(kB * by) + 3.5f; t.ccz = static_cast<float>(kB * bz) + 3.5f;
    t.msum = voxel * static_cast<float>(kB * (bx + by + bz) + 21);
  }
  template <typename Apply>
  __device__ __forceinline__ int for_each_frame(const Thread& t, const float* __restrict__ fc, int N, const Intr K, const Fuse in,
                                                Apply apply) const {
    return brick_cull_and_apply(fc, N, t.ccx, t.ccy, t.ccz, t.msum, voxel, K, in, t.list, t.wave_n, apply);
  }
  __device__ __forceinline__ void keep(int n) const {
    if (kept && threadIdx.x == 0) kept[blockIdx.x] = n;
  }
};

}  // namespace
