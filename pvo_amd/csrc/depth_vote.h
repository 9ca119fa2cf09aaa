// depth_vote.h — the per-pixel vote of the depth filter (droid_kernels.cu:640-754), shared by depth_filter_kernel (geom.hip) and the
// map export's classify kernel (map_points.hip).  Both translation units are compiled without multiply-add contraction
// (pvo_amd/build.py EXTRA_FLAGS), so the two callers perform the same roundings and get the same counts.
#pragma once
#include "se3.h"

struct Intr { float fx, fy, cx, cy; };
__device__ __forceinline__ Intr load_intr(const float* p) { return {p[0], p[1], p[2], p[3]}; }

// in how many of the six neighbour views ix-1, ix-2, ix-3, ix+3, ix+4, ix+5 (droid_kernels.cu:674) the inverse depth of pixel k of
// frame ix is confirmed to within t.  ix must lie in [0, nframes) and k in [0, ht*wd); every other index is guarded here: a
// neighbour outside [0, nframes) is skipped, and the four taps are read only where the floor of the projection (saturated, NaN -> 0:
// pvo_floor_to_int) lies in [0, wd-1) x [0, ht-1).
__device__ __forceinline__ float depth_votes(const float* __restrict__ poses, const float* __restrict__ disps, const Intr K,
                                             int ix, float t, int nframes, int ht, int wd, int k) {
  const int HW = ht * wd;
  const Pose Gi = load_pose(poses + 7 * static_cast<long long>(ix));
  const int i = k / wd, j = k - i * wd;
  const float di = disps[static_cast<long long>(ix) * HW + k];
  const float Xi[4] = {(static_cast<float>(j) - K.cx) / K.fx, (static_cast<float>(i) - K.cy) / K.fy, 1.0f, di};
  // the reference votes with one atomicAdd per neighbour view (grid.y = 6); the six
  // votes are summed in a register here and stored once.
  float votes = 0.f;
#pragma unroll
  for (int neigh = 0; neigh < 6; ++neigh) {
    const int jx = (neigh < 3) ? ix - neigh - 1 : ix + neigh;   // droid_kernels.cu:674
    if (jx < 0 || jx >= nframes) continue;
    const Pose G = rel_pose(Gi, load_pose(poses + 7 * static_cast<long long>(jx)));
    float Xj[4];
    act4(G, Xi, Xj);
    const float uj = K.fx * (Xj[0] / Xj[2]) + K.cx;
    const float vj = K.fy * (Xj[1] / Xj[2]) + K.cy;
    const float dj = Xj[3] / Xj[2];
    const int u0 = pvo_floor_to_int(uj), v0 = pvo_floor_to_int(vj);
    if (u0 >= 0 && v0 >= 0 && u0 < wd - 1 && v0 < ht - 1) {
      const float* dm = disps + static_cast<long long>(jx) * HW;
      const float d00 = dm[v0 * wd + u0], d01 = dm[v0 * wd + u0 + 1];
      const float d10 = dm[(v0 + 1) * wd + u0], d11 = dm[(v0 + 1) * wd + u0 + 1];
      // droid_kernels.cu:748-751: double-precision reciprocal differences
      const double idj = 1.0 / static_cast<double>(dj);
      if (fabs(idj - 1.0 / static_cast<double>(d00)) < t) votes += 1.0f;
      else if (fabs(idj - 1.0 / static_cast<double>(d01)) < t) votes += 1.0f;
      else if (fabs(idj - 1.0 / static_cast<double>(d10)) < t) votes += 1.0f;
      else if (fabs(idj - 1.0 / static_cast<double>(d11)) < t) votes += 1.0f;
    }
  }
  return votes;
}
