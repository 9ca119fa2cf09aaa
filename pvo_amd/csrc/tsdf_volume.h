// tsdf_volume.h — where a cell's eight corners are stored: the dense volume and the brick volume as the adapters tsdf_ray.h's walk asks
// for (n, tsdf, wsum, rgb, label, min_weight, corners(), kBricks); the limits of the two volumes come with tsdf_host.h.  Shared by the render
// (tsdf_render.hip) and the frame-to-model tracker (tsdf_track.hip): both look at a volume through the same adapter, so the brick call
// of either gives the bytes of its dense call.
#pragma once
#include "tsdf_host.h"
#include "tsdf_ray.h"

struct DenseVolume {
  static constexpr bool kBricks = false;
  const float* tsdf; const float* wsum; const float* rgb; const int32_t* label;
  int n[3];                               // nx, ny, nz
  float min_weight;
  __device__ __forceinline__ int corners(const int (&cell)[3], int (&at)[8]) const {
    const int base = (cell[2] * n[1] + cell[1]) * n[0] + cell[0];         // (nz ny nx < 2^31)
#pragma unroll
    for (int j = 0; j < 8; ++j) at[j] = base + ((j >> 2) * n[1] + ((j >> 1) & 1)) * n[0] + (j & 1);
    return 0;
  }
};

struct BrickVolume {
  static constexpr bool kBricks = true;
  const float* tsdf; const float* wsum; const float* rgb; const int32_t* label;
  int n[3];                               // 8 gx, 8 gy, 8 gz
  float min_weight;
  const int32_t* grid;
  int gy, gx, cap;
  int last[3], last_slot;                 // the last brick looked up (corner 0's) and its slot, in registers

  // the slot of brick (bx,by,bz), inside the grid; -1 = not stored (a slot the pool does not have is no brick)
  __device__ __forceinline__ int read_grid(int bx, int by, int bz) const {
    const int s = grid[(static_cast<long long>(bz) * gy + by) * gx + bx];
    return s < cap ? s : -1;
  }
  __device__ __forceinline__ int corners(const int (&cell)[3], int (&at)[8]) {
    const int bx = cell[0] >> 3, by = cell[1] >> 3, bz = cell[2] >> 3;
    if (bx != last[0] || by != last[1] || bz != last[2]) {
      last_slot = read_grid(bx, by, bz);
      last[0] = bx; last[1] = by; last[2] = bz;
    }
    const int s0 = last_slot;
    if (s0 < 0) return 2;
    const int lx = cell[0] & 7, ly = cell[1] & 7, lz = cell[2] & 7;
    if (lx < 7 && ly < 7 && lz < 7) {     // the whole cell in corner 0's brick
      const int base = s0 * 512 + ((lz << 6) | (ly << 3) | lx);
#pragma unroll
      for (int j = 0; j < 8; ++j) at[j] = base + ((j >> 2) << 6) + (((j >> 1) & 1) << 3) + (j & 1);
      return 0;
    }
    bool all = true;                      // the cell straddles a brick face: back to the grid for the corners beyond it
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int x = cell[0] + (j & 1), y = cell[1] + ((j >> 1) & 1), z = cell[2] + (j >> 2);      // (<= n - 1: inside the grid)
      const bool same = (x >> 3) == bx && (y >> 3) == by && (z >> 3) == bz;
      const int s = same ? s0 : read_grid(x >> 3, y >> 3, z >> 3);
      all = all && s >= 0;
      at[j] = (s >= 0 ? s : 0) * 512 + (((z & 7) << 6) | ((y & 7) << 3) | (x & 7));
    }
    return all ? 0 : 1;
  }
};
