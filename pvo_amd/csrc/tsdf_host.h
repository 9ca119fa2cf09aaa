// tsdf_host.h — what the host side of every TSDF call shares (tsdf.hip, tsdf_sparse.hip, tsdf_reintegrate.hip, tsdf_render.hip,
// tsdf_track.hip): the limits of the two volumes, the workspace granule, the size of a frame table, the argument predicates that more
// than one call states, and the choice of a kernel's <RGB, LAB> instantiation.  A predicate is templated over the argument struct:
// the dense and the brick structs of include/pvo_hip.h name these fields alike.
#pragma once
#include <type_traits>
#include "common.h"

#define PVO_REQ(c) do { if (!(c)) return PVO_EINVAL; } while (0)

namespace tsdf_volume {

constexpr size_t kAlign = 256;
static inline size_t aligned(size_t n) { return (n + kAlign - 1) / kAlign * kAlign; }
static inline bool finite_f(float v) { return v - v == 0.0f; }

static inline bool volume_ok(int nz, int ny, int nx) {
  return nz >= 0 && ny >= 0 && nx >= 0 && static_cast<long long>(nz) * ny < (1ll << 31) && static_cast<long long>(nz) * ny * nx < (1ll << 31);
}
constexpr int kB = PVO_TSDF_BRICK;
constexpr int kMaxBricksPerAxis = (1 << 21) / kB;
static inline bool world_ok(int gz, int gy, int gx, int cap) {
  return gz >= 0 && gy >= 0 && gx >= 0 && gz <= kMaxBricksPerAxis && gy <= kMaxBricksPerAxis && gx <= kMaxBricksPerAxis &&
         static_cast<long long>(gz) * gy < (1ll << 31) && static_cast<long long>(gz) * gy * gx < (1ll << 31) && cap >= 0 &&
         static_cast<long long>(cap) * 512 < (1ll << 31);
}

// a table of N slots of sixteen floats (tsdf_fuse.h kFrameFloats)
static inline size_t table_bytes(long long N) { return N <= 0 ? 0 : aligned(sizeof(float) * 16 * static_cast<size_t>(N)); }

template <typename Args>
bool origin_ok(const Args* a) { return finite_f(a->origin[0]) && finite_f(a->origin[1]) && finite_f(a->origin[2]); }

// the scalars of a fusion: the slots and frames, the volume's scale, the truncation and the weight cap
template <typename Args>
bool fuse_scalars_ok(const Args* a) {
  return a->N >= 0 && a->nframes >= 0 && a->ht >= 0 && a->wd >= 0 && static_cast<long long>(a->ht) * a->wd < (1ll << 31) &&
         a->voxel > 0.0f && finite_f(a->voxel) && a->trunc > 0.0f && finite_f(a->trunc) &&
         a->z_near >= 0.0f && finite_f(a->z_near) && a->w_max >= 0.0f && finite_f(a->w_max) && origin_ok(a);
}

// a colour volume needs the images; the images' sampling must stay inside them
template <typename Args>
bool images_ok(const Args* a) {
  if (a->rgb && !a->images) return false;
  return !a->images || (a->img_stride >= 1 && a->img_offset >= 0 && a->IH > 0 && a->IW > 0 &&
                        static_cast<long long>(a->img_stride) * (a->ht - 1) + a->img_offset < a->IH &&
                        static_cast<long long>(a->img_stride) * (a->wd - 1) + a->img_offset < a->IW);
}

// pvo_tsdf_panoptic_args beside a fusion's arguments: the label maps cover the depth maps
template <typename Args>
bool panoptic_ok(const pvo_tsdf_panoptic_args* p, const Args* a) {
  return p && p->label && p->lconf && p->labels && p->label_div >= 1 && static_cast<long long>(p->lh) * p->label_div >= a->ht &&
         static_cast<long long>(p->lw) * p->label_div >= a->wd;
}

// a mesh call's scalars and outputs, before the "no cell" exit and after it
template <typename Args>
bool mesh_scalars_ok(const Args* a) {
  return a->voxel > 0.0f && finite_f(a->voxel) && a->min_weight == a->min_weight && origin_ok(a) && a->vcap >= 0 && a->fcap >= 0 &&
         a->counts && !(reinterpret_cast<uintptr_t>(a->rgba) & 3);
}
template <typename Args>
bool mesh_labels_ok(const pvo_tsdf_mesh_labels_args* p, const Args* a) { return p && p->label && (a->vcap == 0 || p->vlabel); }
template <typename Args>
bool mesh_outputs_ok(const Args* a) { return (a->vcap == 0 || a->verts) && (a->fcap == 0 || a->faces); }

// f(RGB, LAB) with the two flags as std::bool_constant: the caller's generic lambda names the instantiation
template <typename F>
void pick_rgb_lab(bool rgb, bool lab, F f) {
  if (lab) {
    if (rgb) f(std::true_type{}, std::true_type{});
    else f(std::false_type{}, std::true_type{});
  } else if (rgb) f(std::true_type{}, std::false_type{});
  else f(std::false_type{}, std::false_type{});
}

}  // namespace tsdf_volume
