// map_points.hip — dense map export: the filtered, coloured, labelled point cloud of a set of keyframes in four launches.
//
// Reference: VO_Module/droid_slam/visualization.py:92-107,127-129 (depth_filter + iproj on the inverted poses, then
// count >= 2 & disp > 0.5 * mean, then three boolean-index gathers in torch).  Here nothing of size [N,HW,3] is written and
// read back: the only intermediate is one byte per candidate pixel.
//
//   (a) map_mean_kernel      one workgroup per exported frame: the frame's mean inverse depth, fp64 in a fixed order
//   (b) map_classify_kernel  grid (ceil(HW/256), N): votes (depth_vote.h, the bits of pvo_depth_filter) and the keep rule; leaves a
//                            byte per pixel (bit 7 = kept, low bits = votes) and the number of kept pixels of the workgroup
//   (c) map_scan_kernel      one workgroup: exclusive scan of the N * ceil(HW/256) counts in index order; writes frame_start
//   (d) map_emit_kernel      grid as (b): output index = scanned base + kept pixels of the lower waves + kept lower lanes of the
//                            own wave (64-bit __ballot masks), then the point, colour, label and source of every kept pixel
//
// No atomics: a pixel's output index is a function of the keep bits alone, so the same operands give the same bytes in the same
// order.  Compiled without multiply-add contraction (pvo_amd/build.py), like geom.hip.
#include "depth_vote.h"
#include "scan.h"

namespace {

constexpr int kBlock = 256;          // (b), (d): one pixel per thread, four waves

// a frame id outside [0, nframes) contributes no point and is never dereferenced
__device__ __forceinline__ bool frame_ok(long long f, int nframes) { return f >= 0 && f < nframes; }

__global__ __launch_bounds__(kBlock) void map_mean_kernel(const float* __restrict__ disps, const int64_t* __restrict__ ix,
                                                          float* __restrict__ mean, int nframes, int HW) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long f = ix[b];
  __shared__ double red[kBlock];
  double s = 0.0;
  if (frame_ok(f, nframes)) {
    const float* __restrict__ d = disps + f * HW;
    for (int k = tid; k < HW; k += kBlock) s += static_cast<double>(d[k]);
  }
  red[tid] = s;
  __syncthreads();
#pragma unroll
  for (int w = kBlock / 2; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) mean[b] = static_cast<float>(red[0] / static_cast<double>(HW));   // rounded to fp32 once
}

__global__ __launch_bounds__(kBlock) void map_classify_kernel(
    const float* __restrict__ poses, const float* __restrict__ disps, const float* __restrict__ intrinsics,
    const int64_t* __restrict__ ix, const float* __restrict__ thresh, const float* __restrict__ mean,
    const uint8_t* __restrict__ reject, int LW, int LHW, int label_div, float min_votes, float mean_frac,
    uint8_t* __restrict__ flags, int* __restrict__ counts, int nframes, int ht, int wd) {
  const int HW = ht * wd;
  const int b = blockIdx.y, tid = threadIdx.x;
  const int k = blockIdx.x * kBlock + tid;
  const long long f = ix[b];
  uint8_t flag = 0;
  if (k < HW && frame_ok(f, nframes)) {           // (no early return: every wave reaches the ballot and the barrier)
    const float votes = depth_votes(poses, disps, load_intr(intrinsics), static_cast<int>(f), thresh[b], nframes, ht, wd, k);
    const float d = disps[f * HW + k];
    bool keep = votes >= min_votes && d > mean_frac * mean[b] && d > 0.0f && d < __builtin_inff();   // (NaN fails every comparison)
    if (keep && reject) {
      const int y = k / wd, x = k - y * wd;
      keep = reject[f * LHW + (y / label_div) * LW + x / label_div] == 0;
    }
    flag = static_cast<uint8_t>(static_cast<int>(votes)) | (keep ? 0x80 : 0);
  }
  if (k < HW) flags[static_cast<long long>(b) * HW + k] = flag;
  const unsigned long long m = __ballot(flag & 0x80);
  __shared__ int wave_n[kBlock / 64];
  if ((tid & 63) == 0) wave_n[tid >> 6] = __popcll(m);
  __syncthreads();
  if (tid == 0) counts[b * gridDim.x + blockIdx.x] = (wave_n[0] + wave_n[1]) + (wave_n[2] + wave_n[3]);
}

// exclusive scan of counts[0, M) into base[0, M), M = N * G, in index order (scan.h).  frame_start[b] = base[b * G],
// frame_start[N] = the total (not clamped by any capacity).
__global__ __launch_bounds__(kScanThreads) void map_scan_kernel(const int* __restrict__ counts, int* __restrict__ base,
                                                                int* __restrict__ frame_start, int M, int G) {
  const int* const cnt[1] = {counts};
  int run[1], total[1];
  const ScanChunk c = scan_counts(cnt, M, run, total);
  for (int i = c.lo; i < c.hi; ++i) {
    base[i] = run[0];
    if (i % G == 0) frame_start[i / G] = run[0];
    run[0] += counts[i];
  }
  if (threadIdx.x == 0) frame_start[M / G] = total[0];
}

struct EmitOut {
  float* xyz; uint8_t* rgba; int32_t* label; int32_t* src;
  int capacity;
};
struct EmitIn {
  const uint8_t* images; int IH, IW, stride, offset;
  const int32_t* labels; int LW, LHW, label_div;
};

// the world point of pixel (x, y) of a frame with pose (t, q), world-to-camera:  R^T (Xc - t),  Xc = ((x-cx)/fx, (y-cy)/fy, 1) / d.
// R^T is formed from the quaternion as a matrix; every operation below is one fp32 rounding (no contraction), and the longest chain of
// them bounds the error by 12 * 2^-24 * (|t|_1 + |Xc|_1) per component (derivation: tests/map_reference.py).
__device__ __forceinline__ Vec3 world_point(const Pose G, const Intr K, int x, int y, float d) {
  const float Xc = ((static_cast<float>(x) - K.cx) / K.fx) / d;
  const float Yc = ((static_cast<float>(y) - K.cy) / K.fy) / d;
  const float Zc = 1.0f / d;
  const float vx = Xc - G.t.x, vy = Yc - G.t.y, vz = Zc - G.t.z;
  const Quat q = G.q;
  // rows of R^T = columns of R(q)
  const float r00 = 1.0f - 2.0f * (q.y * q.y + q.z * q.z), r01 = 2.0f * (q.x * q.y + q.z * q.w), r02 = 2.0f * (q.x * q.z - q.y * q.w);
  const float r10 = 2.0f * (q.x * q.y - q.z * q.w), r11 = 1.0f - 2.0f * (q.x * q.x + q.z * q.z), r12 = 2.0f * (q.y * q.z + q.x * q.w);
  const float r20 = 2.0f * (q.x * q.z + q.y * q.w), r21 = 2.0f * (q.y * q.z - q.x * q.w), r22 = 1.0f - 2.0f * (q.x * q.x + q.y * q.y);
  return {(r00 * vx + r01 * vy) + r02 * vz, (r10 * vx + r11 * vy) + r12 * vz, (r20 * vx + r21 * vy) + r22 * vz};
}

__global__ __launch_bounds__(kBlock) void map_emit_kernel(
    const float* __restrict__ poses, const float* __restrict__ disps, const float* __restrict__ intrinsics,
    const int64_t* __restrict__ ix, const uint8_t* __restrict__ flags, const int* __restrict__ base,
    const EmitIn in, const EmitOut out, int ht, int wd) {
  const int HW = ht * wd;
  const int b = blockIdx.y, tid = threadIdx.x;
  const int k = blockIdx.x * kBlock + tid;
  const uint8_t flag = k < HW ? flags[static_cast<long long>(b) * HW + k] : 0;
  const bool keep = (flag & 0x80) != 0;
  const unsigned long long m = __ballot(keep);
  __shared__ int wave_n[kBlock / 64];
  if ((tid & 63) == 0) wave_n[tid >> 6] = __popcll(m);
  __syncthreads();
  if (!keep) return;                      // (a kept pixel's frame id is in range: classify set the bit)
  const int wave = tid >> 6;
  int idx = base[b * gridDim.x + blockIdx.x] + lanes_below(m);
  for (int w = 0; w < wave; ++w) idx += wave_n[w];
  if (idx >= out.capacity) return;        // not written anywhere; the caller sees frame_start[N] > capacity
  const long long f = ix[b];
  const int y = k / wd, x = k - y * wd;
  const Vec3 p = world_point(load_pose(poses + 7 * f), load_intr(intrinsics), x, y, disps[f * HW + k]);
  float* o = out.xyz + 3ll * idx;
  o[0] = p.x; o[1] = p.y; o[2] = p.z;
  if (out.rgba) {
    uchar4 c = make_uchar4(0, 0, 0, flag & 0x7f);
    if (in.images) {                      // BGR planes -> RGB
      const long long plane = static_cast<long long>(in.IH) * in.IW;
      const uint8_t* im = in.images + 3 * plane * f + static_cast<long long>(in.stride * y + in.offset) * in.IW + (in.stride * x + in.offset);
      c.x = im[2 * plane]; c.y = im[plane]; c.z = im[0];
    }
    reinterpret_cast<uchar4*>(out.rgba)[idx] = c;
  }
  if (out.label) out.label[idx] = in.labels[f * in.LHW + (y / in.label_div) * in.LW + x / in.label_div];
  if (out.src) reinterpret_cast<int2*>(out.src)[idx] = make_int2(static_cast<int>(f), k);
}

constexpr size_t kAlign = 256;
inline size_t aligned(size_t n) { return (n + kAlign - 1) / kAlign * kAlign; }

struct Layout { size_t mean, counts, base, flags, total; };
inline Layout layout(int N, int ht, int wd) {
  const size_t HW = static_cast<size_t>(ht) * wd, G = (HW + kBlock - 1) / kBlock;
  Layout L;
  L.mean = 0;
  L.counts = L.mean + aligned(sizeof(float) * N);
  L.base = L.counts + aligned(sizeof(int) * N * G);
  L.flags = L.base + aligned(sizeof(int) * N * G);
  L.total = L.flags + aligned(N * HW);
  return L;
}

}  // namespace

#define PVO_REQ(c) do { if (!(c)) return PVO_EINVAL; } while (0)

extern "C" size_t pvo_map_points_args_size(void) { return sizeof(pvo_map_points_args); }

extern "C" size_t pvo_map_points_workspace_bytes(int N, int ht, int wd) {
  if (N <= 0 || ht <= 0 || wd <= 0) return 0;
  return layout(N, ht, wd).total;
}

extern "C" int pvo_map_points(const pvo_map_points_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  PVO_REQ(a);
  const int N = a->N, ht = a->ht, wd = a->wd;
  PVO_REQ(N >= 0 && ht >= 0 && wd >= 0 && a->nframes >= 0 && a->capacity >= 0 && a->frame_start);
  PVO_REQ(N <= 65535 && static_cast<long long>(N) * ht * wd < (1ll << 31) && static_cast<long long>(ht) * wd < (1ll << 31));
  hipStream_t s = pvo_stream(stream);
  if (N == 0 || ht * wd == 0) {          // an empty call: frame_start alone
    const hipError_t e = hipMemsetAsync(a->frame_start, 0, sizeof(int32_t) * (N + 1), s);
    if (e != hipSuccess) { pvo_note_hip_error(static_cast<int>(e)); return PVO_ELAUNCH; }
    return PVO_OK;
  }
  PVO_REQ(a->poses && a->disps && a->intrinsics && a->ix && a->thresh);
  PVO_REQ(a->capacity == 0 || a->xyz);
  if (a->images) {
    PVO_REQ(a->img_stride >= 1 && a->img_offset >= 0 && a->IH > 0 && a->IW > 0);
    PVO_REQ(static_cast<long long>(a->img_stride) * (ht - 1) + a->img_offset < a->IH);
    PVO_REQ(static_cast<long long>(a->img_stride) * (wd - 1) + a->img_offset < a->IW);
  }
  if (a->labels || a->reject) {
    PVO_REQ(a->label_div >= 1 && a->LH > 0 && a->LW > 0);
    PVO_REQ((ht - 1) / a->label_div < a->LH && (wd - 1) / a->label_div < a->LW);
  }
  PVO_REQ(!a->label || a->labels);        // a label output needs the label maps
  PVO_REQ(!((reinterpret_cast<uintptr_t>(a->rgba) & 3) | (reinterpret_cast<uintptr_t>(a->src) & 7)));
  const Layout L = layout(N, ht, wd);
  if (!workspace || workspace_bytes < L.total) return PVO_EWORKSPACE;
  PVO_REQ(!(reinterpret_cast<uintptr_t>(workspace) & 7));
  char* ws = static_cast<char*>(workspace);
  float* mean = reinterpret_cast<float*>(ws + L.mean);
  int* counts = reinterpret_cast<int*>(ws + L.counts);
  int* base = reinterpret_cast<int*>(ws + L.base);
  uint8_t* flags = reinterpret_cast<uint8_t*>(ws + L.flags);
  const int HW = ht * wd, G = (HW + kBlock - 1) / kBlock;
  const int LW = a->LW, LHW = a->LH * a->LW, ldiv = (a->labels || a->reject) ? a->label_div : 1;

  hipLaunchKernelGGL(map_mean_kernel, dim3(N), dim3(kBlock), 0, s, a->disps, a->ix, mean, a->nframes, HW);
  PVO_CHECK_LAUNCH();
  hipLaunchKernelGGL(map_classify_kernel, dim3(G, N), dim3(kBlock), 0, s, a->poses, a->disps, a->intrinsics, a->ix, a->thresh, mean,
                     a->reject, LW, LHW, ldiv, static_cast<float>(a->min_votes), a->mean_frac, flags, counts, a->nframes, ht, wd);
  PVO_CHECK_LAUNCH();
  hipLaunchKernelGGL(map_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, counts, base, a->frame_start, N * G, G);
  PVO_CHECK_LAUNCH();
  const EmitIn in = {a->images, a->IH, a->IW, a->img_stride, a->img_offset, a->labels, LW, LHW, ldiv};
  const EmitOut out = {a->xyz, a->rgba, a->label, a->src, a->capacity};
  hipLaunchKernelGGL(map_emit_kernel, dim3(G, N), dim3(kBlock), 0, s, a->poses, a->disps, a->intrinsics, a->ix, flags, base, in, out,
                     ht, wd);
  PVO_CHECK_LAUNCH();
  return PVO_OK;
}
