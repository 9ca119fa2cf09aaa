// feature_transport.hip — the VO -> VPS link: the previous frame's feature pyramid carried into the current frame along the odometry's
// flow, a depth test deciding between the cells that land on one target.  Contract: include/pvo_hip.h (pvo_feature_transport);
// yardstick: tests/feature_transport_reference.py.  Everything is an integer or an individually rounded fp32 operation (this file is
// compiled without multiply-add contraction, and says so itself below), so the same operands give the same bytes.
//
//   (a) transport_clear_kernel     the key table (one 64-bit key per cell of every level) set to "nobody", on the stream
//   (b) transport_depth_kernel     only with rel_pose: the depth map carried into the current camera, at its own resolution
//   (c) transport_resolve_kernel   one thread per source cell of all levels in one grid: flow sample, target cell, depth sample, one
//                                  64-bit atomicMin on (key(d) << 32) | ~s into the target's slot (global_atomic_umin_x2).  A minimum
//                                  over integers: the table is the same in whatever order the atomics arrive
//   (d) transport_gather_kernel    all levels in one grid, one thread per 16 bytes of `out`: [cur | alpha * ref[winner]] and src.  With
//                                  C = 256 in 16 bits a wave moves one cell's whole output row (1 KB), a workgroup four cells; no LDS
//
// No allocation, no host synchronisation; capturable.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr unsigned long long kNobody = ~0ull;

struct Level {
  const char* ref; const char* cur; char* out; int32_t* src;
  int H, W;
  float sx, sy;
  long long first;        // the level's first cell among all levels' cells (its slot in the key table)
  long long first_chunk;  // the level's first 16-byte piece among all levels' output pieces
  int per_cell;           // 16-byte pieces per output cell: row16, or 2 * row16 with cur
};

struct Plan {
  Level level[PVO_TRANSPORT_MAX_LEVELS];
  const float* flow; const float* depth;      // depth: the ordering key's map (the transported one with rel_pose), or NULL
  unsigned long long* keys;
  long long cells, chunks;
  int Hf, Wf, Hd, Wd, L, mode, order, dtype, row16;
  float alpha;
};

__global__ __launch_bounds__(kBlock) void transport_clear_kernel(unsigned long long* __restrict__ keys, long long cells) {
  const long long k = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (k < cells) keys[k] = kNobody;
}

// rel_pose (12 floats, rows of [R|t]) and intrinsics (fx, fy, cx, cy) are device data: read here, never on the host
__global__ __launch_bounds__(kBlock) void transport_depth_kernel(const float* __restrict__ depth, float* __restrict__ out,
                                                                 const float* __restrict__ rel_pose, const float* __restrict__ intrinsics,
                                                                 int Hd, int Wd) {
  const int p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= Hd * Wd) return;
  const int v = p / Wd, u = p - v * Wd;
  const float fx = intrinsics[0], fy = intrinsics[1], cx = intrinsics[2], cy = intrinsics[3];
  const float Z = depth[p];
  const float X = (static_cast<float>(u) - cx) / fx * Z;
  const float Y = (static_cast<float>(v) - cy) / fy * Z;
  out[p] = ((rel_pose[8] * X + rel_pose[9] * Y) + rel_pose[10] * Z) + rel_pose[11];
}

// one axis of the align_corners resize: cell i of n_out onto a map of n_in (n_in >= 1)
struct Axis { int i0, i1; float l, h; };
__device__ __forceinline__ Axis resize_axis(int n_in, int n_out, int i) {
  const float r = n_out > 1 ? static_cast<float>(n_in - 1) / static_cast<float>(n_out - 1) : 0.0f;
  const float p = r * static_cast<float>(i);
  Axis a;
  a.i0 = min(static_cast<int>(p), n_in - 1);
  a.i1 = a.i0 + (a.i0 < n_in - 1 ? 1 : 0);
  a.l = p - static_cast<float>(a.i0);
  a.h = 1.0f - a.l;
  return a;
}

// A: [Ha,Wa,stride] floats, component c
__device__ __forceinline__ float bilinear(const float* __restrict__ A, int Wa, int stride, int c, const Axis& ay, const Axis& ax) {
  const size_t r0 = static_cast<size_t>(ay.i0) * Wa, r1 = static_cast<size_t>(ay.i1) * Wa;
  const float a00 = A[(r0 + ax.i0) * stride + c], a01 = A[(r0 + ax.i1) * stride + c];
  const float a10 = A[(r1 + ax.i0) * stride + c], a11 = A[(r1 + ax.i1) * stride + c];
  return ay.h * (ax.h * a00 + ax.l * a01) + ay.l * (ax.h * a10 + ax.l * a11);
}

__device__ __forceinline__ int level_of(const Plan& in, long long g, bool chunks) {
  int l = 0;
#pragma unroll
  for (int k = 1; k < PVO_TRANSPORT_MAX_LEVELS; ++k)
    if (k < in.L && g >= (chunks ? in.level[k].first_chunk : in.level[k].first)) l = k;
  return l;
}

__device__ __forceinline__ bool is_finite(float v) { return v - v == 0.0f; }

__global__ __launch_bounds__(kBlock) void transport_resolve_kernel(const Plan in) {
  const long long g = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (g >= in.cells) return;
  const int l = level_of(in, g, false);
  const Level& lv = in.level[l];
  const int H = lv.H, W = lv.W;
  const int s = static_cast<int>(g - lv.first);
  const int y = s / W, x = s - y * W;
  const Axis fy_ax = resize_axis(in.Hf, H, y), fx_ax = resize_axis(in.Wf, W, x);
  const float fx = bilinear(in.flow, in.Wf, 2, 0, fy_ax, fx_ax);
  const float fy = bilinear(in.flow, in.Wf, 2, 1, fy_ax, fx_ax);
  if (!is_finite(fx) || !is_finite(fy)) return;
  float rx, ry;
  if (in.mode == PVO_TRANSPORT_NEAREST) {
    const float tx = static_cast<float>(x) + fx * lv.sx, ty = static_cast<float>(y) + fy * lv.sy;
    rx = floorf(tx + 0.5f);
    ry = floorf(ty + 0.5f);
  } else {
    const float qx = truncf(fx), qy = truncf(fy);
    if (qx <= -1.0f || qy <= -1.0f || fabsf(fx) >= 32768.0f || fabsf(fy) >= 32768.0f) return;
    rx = static_cast<float>(x) + qx;
    ry = static_cast<float>(y) + qy;
  }
  // compared as floats: a NaN fails every comparison, 1e30 the upper one; only then converted
  if (!(rx >= 0.0f && rx <= static_cast<float>(W - 1) && ry >= 0.0f && ry <= static_cast<float>(H - 1))) return;
  uint32_t hi = 0;
  if (in.depth) {
    const float d = bilinear(in.depth, in.Wd, 1, 0, resize_axis(in.Hd, H, y), resize_axis(in.Wd, W, x));
    if (!(is_finite(d) && d > 0.0f)) return;
    hi = in.order > 0 ? __float_as_uint(d) : ~__float_as_uint(d);      // positive floats order as their bits
  }
  const long long t = static_cast<long long>(static_cast<int>(ry)) * W + static_cast<int>(rx);
  const unsigned long long key = (static_cast<unsigned long long>(hi) << 32) | static_cast<uint32_t>(~static_cast<uint32_t>(s));
  atomicMin(in.keys + lv.first + t, key);
}

// eight (16-bit) or four (fp32) elements times alpha, each rounded to the storage type
__device__ __forceinline__ uint4 scale16(uint4 v, float alpha, int dtype) {
  uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (dtype == PVO_F32) {
      w[k] = __float_as_uint(__uint_as_float(w[k]) * alpha);
    } else if (dtype == PVO_F16) {
      const _Float16 lo = __builtin_bit_cast(_Float16, static_cast<uint16_t>(w[k] & 0xffffu));
      const _Float16 hi = __builtin_bit_cast(_Float16, static_cast<uint16_t>(w[k] >> 16));
      const uint16_t a = __builtin_bit_cast(uint16_t, static_cast<_Float16>(static_cast<float>(lo) * alpha));
      const uint16_t b = __builtin_bit_cast(uint16_t, static_cast<_Float16>(static_cast<float>(hi) * alpha));
      w[k] = static_cast<uint32_t>(a) | (static_cast<uint32_t>(b) << 16);
    } else {
      const uint16_t a = pvo_f32_to_bf16(pvo_bf16_to_f32(static_cast<uint16_t>(w[k] & 0xffffu)) * alpha);
      const uint16_t b = pvo_f32_to_bf16(pvo_bf16_to_f32(static_cast<uint16_t>(w[k] >> 16)) * alpha);
      w[k] = static_cast<uint32_t>(a) | (static_cast<uint32_t>(b) << 16);
    }
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ __launch_bounds__(kBlock) void transport_gather_kernel(const Plan in) {
  const long long g = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (g >= in.chunks) return;
  const int l = level_of(in, g, true);
  const Level& lv = in.level[l];
  const long long local = g - lv.first_chunk;
  long long cell;
  int piece;
  if ((local >> 32) == 0) {                                     // (the usual case: a 32-bit division)
    const uint32_t c = static_cast<uint32_t>(local) / static_cast<uint32_t>(lv.per_cell);
    cell = c;
    piece = static_cast<int>(static_cast<uint32_t>(local) - c * static_cast<uint32_t>(lv.per_cell));
  } else {
    cell = local / lv.per_cell;
    piece = static_cast<int>(local - cell * lv.per_cell);
  }
  const int row16 = in.row16;
  const size_t row = static_cast<size_t>(row16) * 16, out_row = static_cast<size_t>(lv.per_cell) * 16;
  char* out = lv.out + cell * out_row;
  if (piece < lv.per_cell - row16) {                            // the cur half: a byte copy
    *reinterpret_cast<uint4*>(out + static_cast<size_t>(piece) * 16) =
        *reinterpret_cast<const uint4*>(lv.cur + cell * row + static_cast<size_t>(piece) * 16);
    return;
  }
  const int c = piece - (lv.per_cell - row16);
  const unsigned long long key = in.keys[lv.first + cell];
  const int s = key == kNobody ? -1 : static_cast<int>(~static_cast<uint32_t>(key));
  if (c == 0) lv.src[cell] = s;
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (s >= 0) {
    v = *reinterpret_cast<const uint4*>(lv.ref + static_cast<size_t>(s) * row + static_cast<size_t>(c) * 16);
    if (in.alpha != 1.0f) v = scale16(v, in.alpha, in.dtype);
  }
  *reinterpret_cast<uint4*>(out + static_cast<size_t>(piece) * 16) = v;
}

size_t align16(size_t n) { return (n + 15) & ~static_cast<size_t>(15); }

// the argument checks that need no pointer of a level; on success the cell count of all levels
int check_shapes(const pvo_feature_transport_args* a, long long* cells) {
  if (!a) return PVO_EINVAL;
  if (a->L < 0 || a->L > PVO_TRANSPORT_MAX_LEVELS) return PVO_EINVAL;
  if (a->dtype != PVO_F16 && a->dtype != PVO_BF16 && a->dtype != PVO_F32) return PVO_EINVAL;
  const int es = a->dtype == PVO_F32 ? 4 : 2;
  if (a->C < 1 || (static_cast<long long>(a->C) * es) % 16 != 0) return PVO_EINVAL;
  if (a->mode != PVO_TRANSPORT_NEAREST && a->mode != PVO_TRANSPORT_REFERENCE) return PVO_EINVAL;
  if (a->order != 1 && a->order != -1) return PVO_EINVAL;
  if (!(a->alpha - a->alpha == 0.0f)) return PVO_EINVAL;
  if (a->Hf < 0 || a->Wf < 0 || a->Hd < 0 || a->Wd < 0) return PVO_EINVAL;
  if (static_cast<long long>(a->Hf) * a->Wf >= (1ll << 31) || static_cast<long long>(a->Hd) * a->Wd >= (1ll << 31)) return PVO_EINVAL;
  long long n = 0;
  for (int l = 0; l < a->L; ++l) {
    const pvo_transport_level& v = a->level[l];
    if (v.H < 0 || v.W < 0 || static_cast<long long>(v.H) * v.W >= (1ll << 31)) return PVO_EINVAL;
    n += static_cast<long long>(v.H) * v.W;
  }
  if (a->rel_pose && (!a->depth || !a->intrinsics || a->order != 1)) return PVO_EINVAL;
  *cells = n;
  return PVO_OK;
}

}  // namespace

extern "C" size_t pvo_feature_transport_args_size(void) { return sizeof(pvo_feature_transport_args); }

extern "C" size_t pvo_feature_transport_workspace_bytes(const pvo_feature_transport_args* a) {
  long long cells = 0;
  if (check_shapes(a, &cells) != PVO_OK) return 0;
  const size_t moved = a->rel_pose ? static_cast<size_t>(a->Hd) * a->Wd * sizeof(float) : 0;
  return align16(static_cast<size_t>(cells) * sizeof(unsigned long long)) + align16(moved);
}

extern "C" int pvo_feature_transport(const pvo_feature_transport_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  long long cells = 0;
  const int rc = check_shapes(a, &cells);
  if (rc != PVO_OK) return rc;
  if (a->L == 0) return PVO_OK;
  const int es = a->dtype == PVO_F32 ? 4 : 2;
  Plan p = {};
  p.row16 = a->C * es / 16;
  long long chunks = 0, first = 0;
  for (int l = 0; l < a->L; ++l) {
    const pvo_transport_level& v = a->level[l];
    const long long n = static_cast<long long>(v.H) * v.W;
    if (n > 0 && (!v.ref || !v.out || !v.src)) return PVO_EINVAL;
    if (pvo_misaligned16(static_cast<const char*>(v.ref), static_cast<const char*>(v.cur), static_cast<const char*>(v.out))) return PVO_EINVAL;
    Level& d = p.level[l];
    d.ref = static_cast<const char*>(v.ref); d.cur = static_cast<const char*>(v.cur); d.out = static_cast<char*>(v.out); d.src = v.src;
    d.H = v.H; d.W = v.W; d.sx = v.sx; d.sy = v.sy;
    d.first = first; d.first_chunk = chunks;
    d.per_cell = v.cur ? 2 * p.row16 : p.row16;
    first += n;
    chunks += n * d.per_cell;
  }
  if (cells > 0 && (!a->flow || a->Hf < 1 || a->Wf < 1)) return PVO_EINVAL;
  if (cells > 0 && a->depth && (a->Hd < 1 || a->Wd < 1)) return PVO_EINVAL;
  const size_t key_bytes = align16(static_cast<size_t>(cells) * sizeof(unsigned long long));
  const size_t moved = a->rel_pose ? align16(static_cast<size_t>(a->Hd) * a->Wd * sizeof(float)) : 0;
  if (key_bytes + moved > 0 && (!workspace || workspace_bytes < key_bytes + moved || pvo_misaligned16(static_cast<const char*>(workspace))))
    return PVO_EINVAL;
  const long long gather_blocks = (chunks + kBlock - 1) / kBlock;
  if (gather_blocks >= (1ll << 31)) return PVO_EINVAL;
  if (cells == 0) return PVO_OK;
  hipStream_t s = pvo_stream(stream);
  p.flow = a->flow; p.depth = a->depth; p.keys = static_cast<unsigned long long*>(workspace);
  p.cells = cells; p.chunks = chunks;
  p.Hf = a->Hf; p.Wf = a->Wf; p.Hd = a->Hd; p.Wd = a->Wd; p.L = a->L; p.mode = a->mode; p.order = a->order; p.dtype = a->dtype;
  p.alpha = a->alpha;
  const unsigned cell_blocks = static_cast<unsigned>((cells + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(transport_clear_kernel, dim3(cell_blocks), dim3(kBlock), 0, s, p.keys, cells);
  PVO_CHECK_LAUNCH();
  if (a->rel_pose) {
    // rel_pose and intrinsics are device data: the kernel reads them (no host copy, no synchronisation)
    float* out = reinterpret_cast<float*>(static_cast<char*>(workspace) + key_bytes);
    const long long n = static_cast<long long>(a->Hd) * a->Wd;
    hipLaunchKernelGGL(transport_depth_kernel, dim3(static_cast<unsigned>((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a->depth, out,
                       a->rel_pose, a->intrinsics, a->Hd, a->Wd);
    PVO_CHECK_LAUNCH();
    p.depth = out;
  }
  hipLaunchKernelGGL(transport_resolve_kernel, dim3(cell_blocks), dim3(kBlock), 0, s, p);
  PVO_CHECK_LAUNCH();
  hipLaunchKernelGGL(transport_gather_kernel, dim3(static_cast<unsigned>(gather_blocks)), dim3(kBlock), 0, s, p);
  PVO_CHECK_LAUNCH();
  return PVO_OK;
}
