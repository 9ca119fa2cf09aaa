// ba.hip — dense bundle adjustment for gfx950 (MI355X), device-resident end to end.
//
// Replaces ba_cuda and everything under it (reference VO_Module/src/droid_kernels.cu:
// projective_transform_kernel :177-403, accum_cuda/accum_kernel :833-853,927-977,
// EEt6x6/Ev6x1/EvT6x1 :980-1094, SparseBlock :1096-1198, schur_block :1201-1290,
// pose/disp retraction :856-925, ba_cuda :1293-1410).
//
// The reference runs ~12 launches and >=8 device<->host copies per iteration: the
// CSR index lists, the (a,b,k) Schur triple list and the Eigen sparse LLT are all
// built / solved on the host.  Here nothing leaves the device:
//
//   plan     (once per call, 1 workgroup)  kx = unique([t0,t1) U ii) as a presence
//            bitmap + scan, per-depth-frame CSR of outgoing edges.
//   per Gauss-Newton step, 5 launches:
//   assemble grid (pixel chunk, edge): Jacobians per pixel in registers; the 78+12
//            pose-block sums are wave-shuffle reduced (no 256-float LDS tree per scalar)
//            and added into the dense fp64 pose system with fp64 atomics; Eii/Eij/Cii/bz
//            stored for the depth elimination.
//   depth    grid (pixel chunk, depth frame): C, w, Q = 1/(C+eta) and the window rows Ei.
//   schur    grid (pixel chunk, depth frame): all rows coupling this depth frame to free
//            poses form M; (M Q) M^T and M (Q w) are accumulated by fp32 MFMA
//            (v_mfma_f32_16x16x4_f32, exact fp32 FMA chains, K = pixels) and atomically
//            SUBTRACTED from the system.
//   solve    damping, fp64 Cholesky, forward/back substitution, dx, pose retraction, in the
//            form solve_form picks by size: dense on the matrix cores (windows), envelope
//            (chains), dense in 48 x 48 blocks (densely connected global graphs).
//   backsub  grid (pixel chunk, depth frame): dz = Q (w - sum_r E_r^T dx), disps += dz.
//
// `sys` = [(6P)^2 row-major A-S | 6P rhs] in fp64 is also the message an edge-sharded
// multi-GPU run all-reduces between `schur` and `solve` (pvo_ba_local / pvo_ba_finish).
//
// Semantics kept from the reference: MIN_DEPTH 0.25 on the TARGET depth only, weights
// scaled by 1e-3, poses below t0 fixed, fp64 solve with `diag += ep + lm*diag`, zero
// update when the factorisation fails, EvT6x1's skip of window pose 0 in the depth
// back-substitution (:1084).  Deviation: expSE3 uses xi[5], not xi[45] (:154).
//
// One translation unit.  The stages are headers, included in their order of definition:
//   ba_workspace.h     fix_add, chunk constants, Plan / Ws / carve, staging slots, the prior / stereo / plan kernels
//   ba_assemble.h      EdgeGeom, the edge pixel (project_pixel, depth_jacobian, pose_jacobian), pixel_terms, ba_assemble_kernel
//   ba_schur.h         row passes, ba_schur_mfma_kernel, ba_schur_reduce_kernel, ba_depth_kernel
//   ba_solve.h         the pose-solve forms (envelope, dense on the matrix cores, 48 x 48 blocks), Riders, solve_epilogue
//   ba_backsub.h       ba_backsub_body, ba_backsub_kernel
//   ba_sigma.h         the uncertainty kernels
//   ba_calib.h         CalibWs, the calibration kernels
// Here: the probe hooks and the host entry points.  (Every __global__ kernel of this unit is in a header: tests/test_c_abi.py
// tells a unit with device code by that word in its own text, which is why it stands in this sentence.)
#include <stdlib.h>
#include "ba_workspace.h"
#include "ba_assemble.h"
#include "ba_schur.h"
#include "ba_solve.h"
#include "ba_backsub.h"
#include "ba_sigma.h"
#include "ba_calib.h"

namespace {

int check_common(int E, int F, int ht, int wd, int t0, int t1) {
  if (E < 0 || F <= 0 || ht <= 0 || wd <= 0 || t0 < 0 || t1 < t0 || t1 > F) return PVO_EINVAL;
  if (E > 65535) return PVO_EUNSUPPORTED;
  return PVO_OK;
}

}  // namespace

#if defined(PVO_BA_PROBE) && PVO_BA_PROBE == 3
extern "C" int pvo_debug_ba_wg_probe(void* buf) { return hipMemcpyToSymbol(HIP_SYMBOL(g_ba_wg_probe), &buf, sizeof(buf)) == hipSuccess ? 0 : 1; }
#endif
#ifdef PVO_BA_PROBE
extern "C" int pvo_debug_ba_probe(void* buf) { return hipMemcpyToSymbol(HIP_SYMBOL(g_ba_probe), &buf, sizeof(buf)) == hipSuccess ? 0 : 1; }
#endif

extern "C" size_t pvo_ba_workspace_bytes(int E, int P, int nframes, int HW) {
  if (E < 0 || P < 0 || nframes < 0 || HW < 0) return 0;
  return carve(nullptr, E, P, nframes, HW).bytes + 256;
}

static inline void* ws_base(void* workspace) {
  return reinterpret_cast<void*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~static_cast<uintptr_t>(255));
}

// the caller's workspace carved for these sizes; false: it is shorter than pvo_ba_workspace_bytes asks (PVO_EWORKSPACE)
static bool carve_checked(Ws* w, void* workspace, size_t workspace_bytes, int E, int P, int nframes, int HW) {
  if (workspace_bytes < pvo_ba_workspace_bytes(E, P, nframes, HW)) return false;
  *w = carve(ws_base(workspace), E, P, nframes, HW);
  return true;
}

// operand checks shared by the entry points that take a sensor-depth prior / a stereo baseline
static bool prior_ok(const float* sens, float alpha) { return !sens || alpha > 0.0f; }      // (alpha stands in C's denominator; NaN fails here too)
static bool baseline_ok(float baseline) { return baseline >= 0.0f && baseline < __builtin_inff(); }      // (NaN fails the first comparison)

static int launch_plan(const Ws& w, const int64_t* ii, const int64_t* jj, int E, int nframes, int t0, int t1, int K_eta, int motion_only,
                       const float* sens, float alpha, float baseline, hipStream_t st) {
  hipLaunchKernelGGL(ba_plan_kernel, dim3(1), dim3(256), 0, st, ii, jj, w.plan, E, nframes, t0, t1, K_eta, motion_only, sens, alpha, baseline);
  PVO_CHECK_LAUNCH();
  return PVO_OK;
}

extern "C" int pvo_ba_plan(const int64_t* ii, const int64_t* jj, int E, int nframes, int HW,
                           int K_eta, int t0, int t1, void* workspace, size_t workspace_bytes,
                           void* stream) {
  if (E < 0 || nframes <= 0 || t0 < 0 || t1 < t0 || t1 > nframes || !workspace) return PVO_EINVAL;
  if (E > 0 && (!ii || !jj)) return PVO_EINVAL;
  Ws w;
  if (!carve_checked(&w, workspace, workspace_bytes, E, t1 - t0, nframes, HW)) return PVO_EWORKSPACE;
  return launch_plan(w, ii, jj, E, nframes, t0, t1, K_eta, K_eta < 0 ? 1 : 0, nullptr, 0.0f, 0.0f, pvo_stream(stream));
}

// A setting of every later pvo_ba_local on this workspace: one single-thread launch (`kernel`, on the plan's meta words and
// `operands`) - no host synchronisation, capturable; pvo_ba_plan resets it
template <class Kernel, class... Operands>
static int set_plan_words(void* workspace, size_t workspace_bytes, int E, int P, int nframes, int HW, bool operands_ok, void* stream,
                          Kernel kernel, Operands... operands) {
  if (!workspace || E < 0 || P < 0 || nframes <= 0 || HW <= 0 || !operands_ok) return PVO_EINVAL;
  Ws w;
  if (!carve_checked(&w, workspace, workspace_bytes, E, P, nframes, HW)) return PVO_EWORKSPACE;
  hipLaunchKernelGGL(kernel, dim3(1), dim3(1), 0, pvo_stream(stream), w.plan.meta, operands...);
  PVO_CHECK_LAUNCH();
  return PVO_OK;
}

// the sensor-depth prior ...
extern "C" int pvo_ba_depth_prior(void* workspace, size_t workspace_bytes, int E, int P, int nframes, int HW,
                                  const float* disps_sens, float alpha, void* stream) {
  return set_plan_words(workspace, workspace_bytes, E, P, nframes, HW, prior_ok(disps_sens, alpha), stream, ba_prior_kernel, disps_sens, alpha);
}

// ... and the stereo baseline (0: none)
extern "C" int pvo_ba_stereo(void* workspace, size_t workspace_bytes, int E, int P, int nframes, int HW, float baseline, void* stream) {
  return set_plan_words(workspace, workspace_bytes, E, P, nframes, HW, baseline_ok(baseline), stream, ba_stereo_kernel, baseline);
}

extern "C" int pvo_ba_local(const float* poses, const float* disps, const float* intrinsics,
                            const float* targets, const float* weights, const float* eta,
                            const int64_t* ii, const int64_t* jj,
                            int E, int nframes, int ht, int wd, int K_eta, int t0, int t1,
                            int motion_only, void* sys_,
                            void* workspace, size_t workspace_bytes, void* stream) {
  long long* sys = static_cast<long long*>(sys_);
  int rc = check_common(E, nframes, ht, wd, t0, t1);
  if (rc != PVO_OK) return rc;
  const int P = t1 - t0, HW = ht * wd;
  if (!poses || !disps || !intrinsics || !sys || !workspace) return PVO_EINVAL;
  if (E > 0 && (!targets || !weights || !ii || !jj)) return PVO_EINVAL;
  if (!motion_only && !eta) return PVO_EINVAL;
  if (P > 5400 || nframes >= (1 << 28)) return PVO_EUNSUPPORTED;      // (the Schur kernel's row table: 6 P + 5 in a short, row indices in 28 bits)
  Ws w;
  if (!carve_checked(&w, workspace, workspace_bytes, E, P, nframes, HW)) return PVO_EWORKSPACE;
  hipStream_t st = pvo_stream(stream);
  // pvo_ba_finish leaves `sys` zeroed after reading it; callers that chain local -> finish -> local on the same buffer
  // say so with bit 1 of motion_only and save the memset
  const size_t n6 = static_cast<size_t>(6) * P;
  const bool clean = (motion_only & 2) != 0;
  motion_only &= 1;
  if (!clean && hipMemsetAsync(sys, 0, sizeof(long long) * (n6 * n6 + n6), st) != hipSuccess) return PVO_ELAUNCH;
  if (E == 0) return PVO_OK;
  const bool two_stage = !motion_only;      // the chunk sums go through the Schur kernel (there is none in a motion-only BA)
  const int chunksA = (HW + kChunkA - 1) / kChunkA;
  hipLaunchKernelGGL(ba_assemble_kernel, dim3((HW + kChunkA - 1) / kChunkA, E), dim3(256), 0, st,
                     poses, disps, intrinsics, targets, weights, ii, jj, w.Eii, w.Eij, w.Cii, w.bz,
                     sys, w.plan.meta, HW, wd, t0, P, motion_only, two_stage ? w.part : nullptr);
  PVO_CHECK_LAUNCH();
  if (!motion_only) {
    const int Kmax = depth_rows_bound(nframes, P, E);
    // pixels per workgroup: 256 while the grid fits the chip's resident slots (two 55 KB workgroups per CU); a global bundle
    // adjustment (64 keyframes x 12 chunks: 768 workgroups in two rounds, every one issuing ~1000 atomics into the same 63 x 63
    // blocks) takes bigger chunks - fewer, longer workgroups, a fraction of the atomics
    // (a function of the map size and the POSE WINDOW only - never of this rank's edge count: the chunking fixes the fp32
    // partial sums, and an edge-sharded run must form the same ones as the whole graph; t0 / t1 are the same on every rank.
    // Depth frames optimised = the window's frames + the few source frames in front of it, so P + 1 stands for their number.
    // Until round 5 this was the BUFFER length: a 1024-frame video buffer - the reference driver's default - put every window-
    // sized BA on 1024-pixel chunks, 3 x K workgroups, 443 us instead of 20: found by the full-sequence run of bench.py)
    const int frames_opt = (nframes < P + 1) ? nframes : (P + 1);
    const long long wg256 = static_cast<long long>((HW + 255) / 256) * frames_opt;
    // (256-pixel chunks only up to ~190 workgroups, i.e. windows of up to 15 poses at 12 chunks a frame: a frontend window of the
    // full-sequence run - 21-25 poses, frames with 18 neighbours - took 86.5 us with 256-pixel chunks and 73.4 with 512: half the
    // tile-pair atomics and half the workgroups that each redo row table and depth phase per z-slice; 2 / 8 slices and 1024-pixel
    // chunks were all slower, tools/_probe sweep of a dumped window)
    // Round 6: a DENSE window (up to kDenseMaxPoses poses whose 256-pixel grid would not fit: the frontend's window with its
    // inactive edges) stays on 256-pixel chunks and ONE slice, with the dynamic LDS segment for a frame's rows (schur_rowpass_lds);
    // its depth phase is ba_depth_kernel's.  By P and the map size only, like the chunk rule: the same on every rank.
    const bool dense_window = P <= kDenseMaxPoses && wg256 > 192;
    const int pix = (wg256 <= 192 || dense_window) ? 256 : (wg256 <= 1024 ? 512 : 1024);
    const int gx = (HW + pix - 1) / pix;
    const int deal_rows = two_stage ? (E + kDealEdges * gx - 1) / (kDealEdges * gx) : 0;      // workgroups that add up the assembly's chunk sums: kDealEdges edges each
    // rows of the grid = depth frames: the caller's eta has one row per depth frame (K_eta == K, checked by the plan kernel and
    // reported in the status words), so that is the count; only a broadcast eta (one row) leaves the host with the bound P + E -
    // which at a real window's 48 + 400 edges meant 454 grid rows x 12 chunks x 4 slices for 27 depth frames
    const int Kgrid = (K_eta > 1 && K_eta <= Kmax) ? K_eta : Kmax;
    const dim3 sgrid(gx, Kgrid + deal_rows, dense_window ? 1 : 4);      // (z: slices for the row-tile passes of many-neighbour frames, see ba_schur_body)
    const int depth_done = (pix != 256 || dense_window) ? 1 : 0;       // (by map size and pose window only: the same on every rank of a sharded run)
    // dynamic LDS of the dense-window form: what the CU's 160 KB leave beside the kernel's static tables (49.7 KB)
    constexpr int kSchurRowsLds = 110 * 1024;
    const size_t sdyn = dense_window ? kSchurRowsLds : 0;
    const int lds_floats = static_cast<int>(sdyn / sizeof(float));
    if (dense_window && !(pvo_allow_lds<ba_schur_mfma_kernel<true, 256>>(kSchurRowsLds) && pvo_allow_lds<ba_schur_mfma_kernel<false, 256>>(kSchurRowsLds)))
      return PVO_ELAUNCH;
    if (depth_done) {
      hipLaunchKernelGGL(ba_depth_kernel, dim3((HW + 255) / 256, Kgrid), dim3(256), 0, st, w.plan, eta, K_eta, w.Eii, w.Cii, w.bz, w.Ei, w.Q, w.w, HW, t0, P, disps);
      PVO_CHECK_LAUNCH();
    }
    // two-stage Schur sums: on for every dense window; WHICH frames are staged is the kernel's choice by frame identity
    // (schur_stage_slot: the window's frames and the kSchurStageFront in front of them - the slots the workspace holds).  Until this
    // rule it was `Kgrid <= P + 8`, a count of THIS call's depth frames: a whole graph with more than 8 source frames in front of
    // the window ran unstaged while its shards (fewer local depth rows) ran staged, and a broadcast eta (Kgrid = Kmax) flipped it too.
    const bool stage2 = dense_window;
#define PVO_SCHUR_LAUNCH(V, PX) hipLaunchKernelGGL((ba_schur_mfma_kernel<V, PX>), sgrid, dim3(256), (PX == 256 ? sdyn : 0), st, w.plan, jj, eta, K_eta, w.Eii, w.Cii, w.bz, w.Ei, \
                                                   w.Eij, w.Q, w.w, sys, HW, t0, P, two_stage ? w.part : nullptr, ii, E, chunksA, deal_rows, w.Mrg, depth_done, (PX == 256 ? lds_floats : 0), \
                                                   (stage2 && PX == 256) ? w.spart : nullptr, w.srow, stage2 ? w.sT : nullptr, disps)
    if ((HW & 3) == 0) { if (pix == 256) PVO_SCHUR_LAUNCH(true, 256); else if (pix == 512) PVO_SCHUR_LAUNCH(true, 512); else PVO_SCHUR_LAUNCH(true, 1024); }
    else { if (pix == 256) PVO_SCHUR_LAUNCH(false, 256); else if (pix == 512) PVO_SCHUR_LAUNCH(false, 512); else PVO_SCHUR_LAUNCH(false, 1024); }
#undef PVO_SCHUR_LAUNCH
    PVO_CHECK_LAUNCH();
    if (stage2) {
      hipLaunchKernelGGL(ba_schur_reduce_kernel, dim3(kSchurStagePairs, Kgrid), dim3(256), 0, st, w.plan, w.spart, w.srow, w.sT, sys, gx, 6 * P, t0);
      PVO_CHECK_LAUNCH();
    }
  }
  return PVO_OK;
}

// The form that factorises the reduced pose system, from the free poses P, the edge count E OF THE WHOLE GRAPH, whether the system
// arrives as a packed message and the debug knob PVO_KNOB_BA_SOLVER.  Every rank of an edge-sharded step factorises the same summed
// system and must choose alike, so nothing here may be rank-local: a call on a shard whose system was all-reduced densely says how
// many edges the whole graph has (pvo_ba_finish_graph); every other entry point's E is the graph's own count - the single-GPU
// choice.  (Until this rule E was this call's count: of two unequal shards of a 438-edge, 39-pose graph, one with more than 8 P
// edges took the 48 x 48 blocks and the other the envelope solve.)  pvo_ba_solve_kind states the rule to the host.  Shipped (knob 0):
//   P = 0                     status words only (a packed message: nothing at all);
//   P <= kDenseMaxPoses       dense on the fp64 matrix cores, ba_solve_dense_kernel: a window, one launch;
//   E > 8 P, dense image      dense in 48 x 48 blocks over many workgroups: a global graph connected by proximity rather than a
//                             keyframe chain, whose envelope fits no LDS and has no separator;
//   otherwise                 the envelope solve, partitioned where the chain allows it (ba_solve_twin_kernel).
// Knob 1-3: the envelope solve as one chain with the named factorisation (tests compare them bit for bit); 4: the envelope solve at
// every size; 5: the shipped choice without the 48 x 48 form; 6: the 48 x 48 form for every dense image.
enum SolveKind { kSolveStatus, kSolveDense, kSolveEnvelope, kSolveChain, kSolveBlocks };
struct SolveForm { SolveKind kind; int chol; };      // chol: the one-chain factorisation, 0 blocked | 1 wave | 2 pipelined
static SolveForm solve_form(int P, int E, bool packed, int knob) {
  if (P == 0) return {kSolveStatus, 0};
  if (knob >= 1 && knob <= 3) return {kSolveChain, knob - 1};
  if (knob == 4) return {kSolveEnvelope, 2};
  if (knob == 6 && !packed) return {kSolveBlocks, 0};
  if (P <= kDenseMaxPoses) return {kSolveDense, 0};
  if (knob != 5 && !packed && static_cast<long long>(E) > 8LL * P) return {kSolveBlocks, 0};
  return {kSolveEnvelope, 2};
}

// host only, no GPU: the kind solve_form picks (0 status words only, 1 dense, 2 envelope, 3 one chain, 4 48 x 48 blocks) from what it
// reads - the free poses, the whole graph's edge count, whether the system is a packed message - under the current debug knob
extern "C" int pvo_ba_solve_kind(int P, int graph_edges, int packed) {
  if (P < 0 || graph_edges < 0) return -1;
  return static_cast<int>(solve_form(P, graph_edges, packed != 0, pvo_knob(PVO_KNOB_BA_SOLVER)).kind);
}

// The caller's jobs, checked, as the solve kernels take them (zeroed: none), and the dynamic LDS their workgroups need.
static int riders_from(const pvo_ba_riders* jobs, Riders* out, size_t* lds) {
  Riders rider{};
  size_t rider_lds = 0;
  if (jobs && jobs->cy && jobs->crows > 0) {
    if (!jobs->cx || !jobs->cw || jobs->cCout <= 0 || jobs->cCout % 192) return PVO_EINVAL;
    if (jobs->cdtype != PVO_F16 && jobs->cdtype != PVO_BF16) return PVO_EUNSUPPORTED;
    if (pvo_misaligned16(jobs->cx, jobs->cw, jobs->cy)) return PVO_EINVAL;
    if (jobs->crows > (1LL << 24)) return PVO_EUNSUPPORTED;
    rider.cx = static_cast<const uint16_t*>(jobs->cx); rider.cw = static_cast<const uint16_t*>(jobs->cw); rider.cbias = jobs->cbias;
    rider.cy = static_cast<uint16_t*>(jobs->cy); rider.crows = jobs->crows; rider.cCout = jobs->cCout; rider.cdtype = jobs->cdtype;
    rider.crow_blocks = static_cast<int>((jobs->crows + 63) / 64);
    rider.cblocks = rider.crow_blocks * (jobs->cCout / 192);
    rider_lds = c1t::kTileBytes;
  }
  if (jobs && jobs->gpart && jobs->gE > 0 && jobs->gHW > 0) {
    if (!jobs->gnet || !jobs->gw || jobs->gE > 65535) return PVO_EINVAL;
    if (jobs->gdtype != PVO_F16 && jobs->gdtype != PVO_BF16) return PVO_EUNSUPPORTED;
    if (pvo_misaligned16(jobs->gnet, jobs->gw)) return PVO_EINVAL;
    rider.gnet = static_cast<const uint16_t*>(jobs->gnet); rider.gw = static_cast<const uint16_t*>(jobs->gw); rider.gbias = jobs->gbias;
    rider.gpart = jobs->gpart; rider.gHW = jobs->gHW; rider.gchunks = (jobs->gHW + 255) / 256; rider.gdtype = jobs->gdtype;
    rider.gblocks = jobs->gE * rider.gchunks;
    if (rider_lds < static_cast<size_t>(glt::kTileBytes)) rider_lds = glt::kTileBytes;
  }
  if (jobs && jobs->xg && jobs->xE > 0) {
    if (!jobs->xpart || !jobs->xwt || !jobs->xbias || jobs->xchunks <= 0) return PVO_EINVAL;
    rider.xpart = jobs->xpart; rider.xwt = jobs->xwt; rider.xbias = jobs->xbias; rider.xg = jobs->xg;
    rider.xchunks = jobs->xchunks; rider.xblocks = jobs->xE;
    if (rider_lds < 512) rider_lds = 512;
  }
  *out = rider;
  *lds = rider_lds;
  return PVO_OK;
}

static int ba_finish_impl(float* poses, float* disps, void* sys_, const long long* msg, const int* first_s,
                          const int64_t* ii, const int64_t* jj,
                          int E, int nframes, int ht, int wd, int t0, int t1,
                          float lm, float ep, int motion_only, int clamp_frames, float disp_min,
                          float* dx_out, float* dz_out, int dz_rows, int* status_out,
                          void* workspace, size_t workspace_bytes,
                          const pvo_ba_riders* jobs, int graph_edges, void* stream) {
  Riders rider;
  size_t rider_lds;
  int rc = riders_from(jobs, &rider, &rider_lds);      // (first, as ever: a bad job is reported before a bad window)
  if (rc != PVO_OK) return rc;
  const int rider_blocks = rider.cblocks + rider.gblocks + rider.xblocks;
  rc = check_common(E, nframes, ht, wd, t0, t1);
  if (rc != PVO_OK) return rc;
  if (clamp_frames < 0 || clamp_frames > nframes) return PVO_EINVAL;
  const int P = t1 - t0, HW = ht * wd;
  long long* sys = static_cast<long long*>(sys_);
  if (!poses || !disps || (!sys && !msg) || !workspace) return PVO_EINVAL;
  if (P > kMaxEnvBlocks) return PVO_EUNSUPPORTED;           // (a 12288^2 fp64 system: 1.2 GB)
  Ws w;
  if (!carve_checked(&w, workspace, workspace_bytes, E, P, nframes, HW)) return PVO_EWORKSPACE;
  hipStream_t st = pvo_stream(stream);
  const int n6 = 6 * P;
  const SolveForm form = solve_form(P, graph_edges >= 0 ? graph_edges : E, msg != nullptr, pvo_knob(PVO_KNOB_BA_SOLVER));
  if (msg && form.kind == kSolveStatus) return PVO_OK;
  constexpr size_t kSolveLdsMax = 142000;      // dynamic LDS of a one-workgroup solve: the CU's 163840 B minus the envelope solve's 20528 B of static tables
  if (form.kind == kSolveDense) {
    const size_t dl = dense_lds_bytes(n6);
    const size_t lds = dl > rider_lds ? dl : rider_lds;
    const int Td = dense_N(n6) / 16;                            // tiles per side: 4 slots per wave up to 5 (15 tiles), 14 up to 10 (55: 26 poses), 17 up to 11
    if (!pvo_allow_lds<ba_solve_dense_kernel<4>>(kSolveLdsMax) || !pvo_allow_lds<ba_solve_dense_kernel<14>>(kSolveLdsMax) ||
        !pvo_allow_lds<ba_solve_dense_kernel<17>>(kSolveLdsMax))
      return PVO_ELAUNCH;
    const auto kernel = Td <= 5 ? ba_solve_dense_kernel<4> : (Td <= 10 ? ba_solve_dense_kernel<14> : ba_solve_dense_kernel<17>);
    hipLaunchKernelGGL(kernel, dim3(1 + rider_blocks), dim3(256), lds, st, sys, msg, first_s, poses, w.dx, dx_out, w.plan.meta, status_out,
                       P, t0, lm, ep, rider);
  } else if (form.kind == kSolveEnvelope || form.kind == kSolveChain) {
    int* part = form.kind == kSolveEnvelope ? reinterpret_cast<int*>(w.xchg) : nullptr;      // where ba_prepare_* writes the partition
    if (msg) {
      hipLaunchKernelGGL(ba_env_packed_kernel, dim3(P), dim3(256), 0, st, msg, first_s, w.plan.env, n6);
      hipLaunchKernelGGL(ba_prepare_packed_kernel, dim3(P + 1), dim3(256), 0, st, msg, first_s, w.chol, w.plan.env, n6, lm, ep,
                         static_cast<long long>(kSolveLdsMax), part);
    } else {
      hipLaunchKernelGGL(ba_env_kernel, dim3((n6 * n6 + 2047) / 2048), dim3(256), 0, st, sys, w.plan.env, n6);
      hipLaunchKernelGGL(ba_prepare_kernel, dim3((n6 * n6 + n6 + 2047) / 2048), dim3(256), 0, st, sys, w.chol, w.plan.env, n6, lm, ep,
                         static_cast<long long>(kSolveLdsMax), part);
    }
    PVO_CHECK_LAUNCH();
    if (!part && hipMemsetAsync(w.xchg, 0, 16, st) != hipSuccess) return PVO_ELAUNCH;      // (one chain: no partition)
    if (!pvo_allow_lds<ba_solve_twin_kernel>(kSolveLdsMax)) return PVO_ELAUNCH;
    hipLaunchKernelGGL(ba_solve_twin_kernel, dim3(2 + rider_blocks), dim3(256), kSolveLdsMax > rider_lds ? kSolveLdsMax : rider_lds, st,
                       w.chol, poses, w.dx, dx_out, w.plan.meta, status_out, P, t0, w.plan.env, static_cast<long long>(kSolveLdsMax), w.xchg,
                       form.chol, rider);
  } else {                                                      // 48 x 48 blocks, or no free pose: dense_finish_kernel ends the solve
    if (form.kind == kSolveBlocks) {
      // (no envelope pass: ba_prepare_kernel with no LDS budget writes the dense row-major image whatever `env` holds - INT_MAX between solves)
      hipLaunchKernelGGL(ba_prepare_kernel, dim3((n6 * n6 + n6 + 2047) / 2048), dim3(256), 0, st, sys, w.chol, w.plan.env, n6, lm, ep,
                         0LL /* no LDS budget: the dense row-major image */, static_cast<int*>(nullptr));
      PVO_CHECK_LAUNCH();
      if (hipMemsetAsync(w.xchg, 0, 16, st) != hipSuccess) return PVO_ELAUNCH;                                       // (no partition)
      const int nkb = (n6 + kNB - 1) / kNB, nrb = (n6 + 1 + kNB - 1) / kNB;
      for (int kb = 0; kb < nkb; ++kb) {
        hipLaunchKernelGGL(dense_panel_kernel, dim3(nrb - kb), dim3(256), 0, st, w.chol, w.ldiag, n6, kb, w.plan.meta);
        const int m = nrb - kb - 1;
        if (m > 0) hipLaunchKernelGGL(dense_update_kernel, dim3(m * (m + 1) / 2), dim3(256), 0, st, w.chol, n6, kb, nrb);
      }
      PVO_CHECK_LAUNCH();
      double* yrow = w.chol + static_cast<size_t>(n6) * n6;
      for (int kb = nkb - 1; kb >= 0; --kb)
        hipLaunchKernelGGL(dense_back_kernel, dim3(kb + 1), dim3(256), 0, st, w.chol, w.ldiag, yrow, w.xvec, n6, kb);
      PVO_CHECK_LAUNCH();
    }
    if (rider_lds > 48 * 1024 && !pvo_allow_lds<dense_finish_kernel>(kSolveLdsMax)) return PVO_ELAUNCH;
    hipLaunchKernelGGL(dense_finish_kernel, dim3(1 + rider_blocks), dim3(256), rider_lds, st, w.xvec, poses, w.dx, dx_out, w.plan.meta, status_out, P, t0, rider);
  }
  PVO_CHECK_LAUNCH();
  if (!motion_only && E + P > 0) {
    const int Kmax = depth_rows_bound(nframes, P, E);
    hipLaunchKernelGGL(ba_backsub_kernel, dim3((HW + 255) / 256, Kmax > clamp_frames ? Kmax : clamp_frames), dim3(256), 0, st,
                       w.plan, jj, w.Ei, w.Eij, w.Q, w.w, w.dx, disps, dz_out, dz_rows, HW, t0, P, clamp_frames, disp_min);
    PVO_CHECK_LAUNCH();
  }
  return PVO_OK;
}

extern "C" int pvo_ba_finish(float* poses, float* disps, void* sys_,
                             const int64_t* ii, const int64_t* jj,
                             int E, int nframes, int ht, int wd, int t0, int t1,
                             float lm, float ep, int motion_only, int clamp_frames, float disp_min,
                             float* dx_out, float* dz_out, int dz_rows, int* status_out,
                             void* workspace, size_t workspace_bytes, void* stream) {
  return pvo_ba_finish_riders(poses, disps, sys_, ii, jj, E, nframes, ht, wd, t0, t1, lm, ep, motion_only, clamp_frames, disp_min,
                              dx_out, dz_out, dz_rows, status_out, workspace, workspace_bytes, nullptr, stream);
}

extern "C" int pvo_ba_finish_conv1x1(float* poses, float* disps, void* sys_,
                                     const int64_t* ii, const int64_t* jj,
                                     int E, int nframes, int ht, int wd, int t0, int t1,
                                     float lm, float ep, int motion_only, int clamp_frames, float disp_min,
                                     float* dx_out, float* dz_out, int dz_rows, int* status_out,
                                     void* workspace, size_t workspace_bytes,
                                     const void* cx, const void* cw, const float* cbias, void* cy, long long crows, int cCout, int cdtype,
                                     void* stream) {
  pvo_ba_riders r{};
  r.cx = cx; r.cw = cw; r.cbias = cbias; r.cy = cy; r.crows = crows; r.cCout = cCout; r.cdtype = cdtype;
  return pvo_ba_finish_riders(poses, disps, sys_, ii, jj, E, nframes, ht, wd, t0, t1, lm, ep, motion_only, clamp_frames, disp_min,
                              dx_out, dz_out, dz_rows, status_out, workspace, workspace_bytes, cy ? &r : nullptr, stream);
}

extern "C" int pvo_ba_finish_riders(float* poses, float* disps, void* sys_,
                                    const int64_t* ii, const int64_t* jj,
                                    int E, int nframes, int ht, int wd, int t0, int t1,
                                    float lm, float ep, int motion_only, int clamp_frames, float disp_min,
                                    float* dx_out, float* dz_out, int dz_rows, int* status_out,
                                    void* workspace, size_t workspace_bytes,
                                    const pvo_ba_riders* jobs, void* stream) {
  if (!sys_) return PVO_EINVAL;
  return ba_finish_impl(poses, disps, sys_, nullptr, nullptr, ii, jj, E, nframes, ht, wd, t0, t1, lm, ep, motion_only, clamp_frames, disp_min,
                        dx_out, dz_out, dz_rows, status_out, workspace, workspace_bytes, jobs, -1, stream);
}

extern "C" int pvo_ba_finish_graph(float* poses, float* disps, void* sys_,
                                   const int64_t* ii, const int64_t* jj,
                                   int E, int nframes, int ht, int wd, int t0, int t1,
                                   float lm, float ep, int motion_only, int clamp_frames, float disp_min,
                                   float* dx_out, float* dz_out, int dz_rows, int* status_out,
                                   void* workspace, size_t workspace_bytes, int graph_edges, void* stream) {
  if (!sys_ || graph_edges < E) return PVO_EINVAL;
  return ba_finish_impl(poses, disps, sys_, nullptr, nullptr, ii, jj, E, nframes, ht, wd, t0, t1, lm, ep, motion_only, clamp_frames, disp_min,
                        dx_out, dz_out, dz_rows, status_out, workspace, workspace_bytes, nullptr, graph_edges, stream);
}

extern "C" size_t pvo_ba_packed_elems(const int* first_host, int P) {
  if (!first_host || P < 0) return 0;
  size_t blocks = 0;
  for (int b = 0; b < P; ++b) {
    const int f = first_host[b] < b ? (first_host[b] < 0 ? 0 : first_host[b]) : b;
    blocks += static_cast<size_t>(b - f + 1) * 36;
  }
  return blocks + static_cast<size_t>(6) * P;
}

extern "C" int pvo_ba_pack(void* sys_, const int* first_s, void* msg, int P, void* stream) {
  if (!sys_ || !first_s || !msg || P < 0) return PVO_EINVAL;
  if (P > kMaxEnvBlocks) return PVO_EUNSUPPORTED;
  if (P == 0) return PVO_OK;
  const int n6 = 6 * P;
  hipLaunchKernelGGL(ba_pack_kernel, dim3((n6 * n6 + n6 + 2047) / 2048), dim3(256), 0, pvo_stream(stream),
                     static_cast<long long*>(sys_), first_s, static_cast<long long*>(msg), n6);
  PVO_CHECK_LAUNCH();
  return PVO_OK;
}

extern "C" int pvo_ba_finish_packed(float* poses, float* disps, const void* msg, const int* first_s,
                                    const int64_t* ii, const int64_t* jj,
                                    int E, int nframes, int ht, int wd, int t0, int t1,
                                    float lm, float ep, int motion_only, int clamp_frames, float disp_min,
                                    float* dx_out, float* dz_out, int dz_rows, int* status_out,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  if (!msg || !first_s) return PVO_EINVAL;
  return ba_finish_impl(poses, disps, nullptr, static_cast<const long long*>(msg), first_s, ii, jj, E, nframes, ht, wd, t0, t1, lm, ep, motion_only,
                        clamp_frames, disp_min, dx_out, dz_out, dz_rows, status_out, workspace, workspace_bytes, nullptr, -1, stream);
}

// diagnostic (tests, tools): the partition the last pvo_ba_finish on this workspace chose - out[0] = m, out[1] = s, both 0 when the
// pose chain was solved in one piece.  Synchronises the stream.
extern "C" int pvo_ba_last_partition(void* workspace, size_t workspace_bytes, int E, int P, int nframes, int HW, int* out, void* stream) {
  if (!workspace || !out || E < 0 || P < 0) return PVO_EINVAL;
  if (workspace_bytes < pvo_ba_workspace_bytes(E, P, nframes, HW)) return PVO_EWORKSPACE;
  out[0] = out[1] = 0;
  const SolveKind kind = solve_form(P, E, false, pvo_knob(PVO_KNOB_BA_SOLVER)).kind;
  if (kind == kSolveStatus || kind == kSolveDense) return PVO_OK;      // (nothing to partition; a packed message never asks here)
  Ws w = carve(ws_base(workspace), E, P, nframes, HW);
  int host[4] = {0, 0, 0, 0};
  if (hipMemcpyAsync(host, w.xchg, sizeof(host), hipMemcpyDeviceToHost, pvo_stream(stream)) != hipSuccess) return PVO_ELAUNCH;
  if (hipStreamSynchronize(pvo_stream(stream)) != hipSuccess) return PVO_ELAUNCH;
  out[0] = host[2]; out[1] = host[3];
  return PVO_OK;
}

extern "C" int pvo_ba_rig(float* poses, float* disps, const float* intrinsics,
                          const float* targets, const float* weights, const float* eta,
                          const int64_t* ii, const int64_t* jj,
                          int E, int nframes, int ht, int wd, int K_eta,
                          int t0, int t1, int iterations, float lm, float ep, int motion_only,
                          float* dx_out, float* dz_out, int dz_rows, int* status_out,
                          void* workspace, size_t workspace_bytes,
                          const float* disps_sens, float alpha, float baseline, void* stream) {
  int rc = check_common(E, nframes, ht, wd, t0, t1);
  if (rc != PVO_OK) return rc;
  if (iterations < 0) return PVO_EINVAL;
  if (!prior_ok(disps_sens, alpha) || !baseline_ok(baseline)) return PVO_EINVAL;
  const int P = t1 - t0, HW = ht * wd;
  if (!workspace) return PVO_EINVAL;
  Ws w;
  if (!carve_checked(&w, workspace, workspace_bytes, E, P, nframes, HW)) return PVO_EWORKSPACE;
  rc = launch_plan(w, ii, jj, E, nframes, t0, t1, K_eta, motion_only, disps_sens, alpha, baseline, pvo_stream(stream));
  if (rc != PVO_OK) return rc;
  for (int it = 0; it < iterations; ++it) {
    rc = pvo_ba_local(poses, disps, intrinsics, targets, weights, eta, ii, jj, E, nframes, ht, wd, K_eta,
                      t0, t1, (motion_only ? 1 : 0) | (it > 0 ? 2 : 0), w.sys, workspace, workspace_bytes, stream);
    if (rc != PVO_OK) return rc;
    rc = pvo_ba_finish(poses, disps, w.sys, ii, jj, E, nframes, ht, wd, t0, t1, lm, ep, motion_only, 0, 0.0f,
                       dx_out, dz_out, dz_rows, status_out, workspace, workspace_bytes, stream);
    if (rc != PVO_OK) return rc;
  }
  return PVO_OK;
}

extern "C" int pvo_ba_prior(float* poses, float* disps, const float* intrinsics,
                            const float* targets, const float* weights, const float* eta,
                            const int64_t* ii, const int64_t* jj,
                            int E, int nframes, int ht, int wd, int K_eta,
                            int t0, int t1, int iterations, float lm, float ep, int motion_only,
                            float* dx_out, float* dz_out, int dz_rows, int* status_out,
                            void* workspace, size_t workspace_bytes,
                            const float* disps_sens, float alpha, void* stream) {
  return pvo_ba_rig(poses, disps, intrinsics, targets, weights, eta, ii, jj, E, nframes, ht, wd, K_eta, t0, t1, iterations, lm, ep,
                    motion_only, dx_out, dz_out, dz_rows, status_out, workspace, workspace_bytes, disps_sens, alpha, 0.0f, stream);
}

extern "C" int pvo_ba(float* poses, float* disps, const float* intrinsics,
                      const float* targets, const float* weights, const float* eta,
                      const int64_t* ii, const int64_t* jj,
                      int E, int nframes, int ht, int wd, int K_eta,
                      int t0, int t1, int iterations, float lm, float ep, int motion_only,
                      float* dx_out, float* dz_out, int dz_rows, int* status_out,
                      void* workspace, size_t workspace_bytes, void* stream) {
  return pvo_ba_prior(poses, disps, intrinsics, targets, weights, eta, ii, jj, E, nframes, ht, wd, K_eta, t0, t1, iterations, lm, ep,
                      motion_only, dx_out, dz_out, dz_rows, status_out, workspace, workspace_bytes, nullptr, 0.0f, stream);
}

// The inverse of the damped reduced pose system `sys` (n = 6 P > 0 unknowns) into cov [n][n], through the workspace's `chol` scratch:
// prepare / factor / invtri / product (the sigma stage above).  status_out: where the factorisation reports, or nullptr.
static int launch_pose_cov(const Ws& w, const long long* sys, int n, float lm, float ep, double* cov, int* status_out, hipStream_t st) {
  hipLaunchKernelGGL(ba_sigma_prepare_kernel, dim3((n * n + 255) / 256), dim3(256), 0, st, sys, w.chol, n, lm, ep);
  hipLaunchKernelGGL(ba_sigma_factor_kernel, dim3(1), dim3(1024), 0, st, w.chol, n, w.plan.meta, status_out);
  hipLaunchKernelGGL(ba_sigma_invtri_kernel, dim3(n), dim3(64), 0, st, w.chol, n);
  hipLaunchKernelGGL(ba_sigma_product_kernel, dim3((n + 63) / 64, n), dim3(64), 0, st, w.chol, cov, n);
  PVO_CHECK_LAUNCH();
  return PVO_OK;
}

// Depth and pose uncertainty of the step pvo_ba_local has just assembled on this planned workspace (include/pvo_hip.h).  Reads
// `sys`, the plan and the workspace's Q / Ei / Eij; writes the workspace's `chol` scratch and the caller's outputs only.
extern "C" int pvo_ba_sigma(const void* sys_, void* workspace, size_t workspace_bytes,
                            const int64_t* ii, const int64_t* jj,
                            int E, int P, int nframes, int ht, int wd, int t0, float lm, float ep,
                            double* pose_cov, float* var_cond, float* var_pose, int* status_out, void* stream) {
  if (P < 0) return PVO_EINVAL;
  int rc = check_common(E, nframes, ht, wd, t0, t0 + P);
  if (rc != PVO_OK) return rc;
  if (P > kSigmaMaxPoses) return PVO_EUNSUPPORTED;
  if (!workspace || (P > 0 && (!sys_ || !pose_cov))) return PVO_EINVAL;
  if (E == 0 || !ii || !jj) return PVO_EINVAL;              // (without an edge pvo_ba_local assembles nothing: there is no Q to report)
  const int HW = ht * wd, n = 6 * P;
  Ws w;
  if (!carve_checked(&w, workspace, workspace_bytes, E, P, nframes, HW)) return PVO_EWORKSPACE;
  hipStream_t st = pvo_stream(stream);
  if (P > 0) {
    rc = launch_pose_cov(w, static_cast<const long long*>(sys_), n, lm, ep, pose_cov, status_out, st);
    if (rc != PVO_OK) return rc;
  }
  const int Kmax = depth_rows_bound(nframes, P, E);      // (>= 1: E >= 1)
  if (var_cond || var_pose || (P == 0 && status_out)) {
    hipLaunchKernelGGL(ba_sigma_kernel, dim3((HW + 255) / 256, Kmax), dim3(256), 0, st, w.plan, jj, w.Ei, w.Eij, w.Q, pose_cov,
                       reinterpret_cast<const int*>(w.chol + static_cast<size_t>(n) * n), var_cond, var_pose, HW, t0, P, P == 0 ? status_out : nullptr);
    PVO_CHECK_LAUNCH();
  }
  return PVO_OK;
}

// plan + sensor-depth prior + stereo baseline + pvo_ba_local (depth BA) + pvo_ba_sigma, on the workspace's own `sys`
extern "C" int pvo_ba_uncertainty(const float* poses, const float* disps, const float* intrinsics,
                                  const float* targets, const float* weights, const float* eta,
                                  const int64_t* ii, const int64_t* jj,
                                  int E, int nframes, int ht, int wd, int K_eta,
                                  int t0, int t1, float lm, float ep,
                                  double* pose_cov, float* var_cond, float* var_pose, int* status_out,
                                  void* workspace, size_t workspace_bytes,
                                  const float* disps_sens, float alpha, float baseline, void* stream) {
  int rc = check_common(E, nframes, ht, wd, t0, t1);
  if (rc != PVO_OK) return rc;
  if (!prior_ok(disps_sens, alpha) || !baseline_ok(baseline)) return PVO_EINVAL;
  const int P = t1 - t0, HW = ht * wd;
  if (P > kSigmaMaxPoses) return PVO_EUNSUPPORTED;
  if (!workspace) return PVO_EINVAL;
  Ws w;
  if (!carve_checked(&w, workspace, workspace_bytes, E, P, nframes, HW)) return PVO_EWORKSPACE;
  rc = launch_plan(w, ii, jj, E, nframes, t0, t1, K_eta, 0, disps_sens, alpha, baseline, pvo_stream(stream));
  if (rc != PVO_OK) return rc;
  rc = pvo_ba_local(poses, disps, intrinsics, targets, weights, eta, ii, jj, E, nframes, ht, wd, K_eta, t0, t1, 0, w.sys,
                    workspace, workspace_bytes, stream);
  if (rc != PVO_OK) return rc;
  return pvo_ba_sigma(w.sys, workspace, workspace_bytes, ii, jj, E, P, nframes, ht, wd, t0, lm, ep, pose_cov, var_cond, var_pose,
                      status_out, stream);
}

extern "C" size_t pvo_ba_calib_workspace_bytes(int E, int P, int nframes, int HW) {
  if (E < 0 || P < 0 || nframes < 0 || HW < 0) return 0;
  return carve_calib(nullptr, E, P, nframes, HW).bytes + 256;
}

// plan + iterations x (pvo_ba_local, calibrating finish) - include/pvo_hip.h.  The plan is this call's own: no sensor-depth prior, no
// stereo baseline.  Every step starts from a cleared `sys` (the sigma stage's prepare kernel reads it without zeroing it).
extern "C" int pvo_ba_calib(float* poses, float* disps, float* intrinsics,
                            const float* targets, const float* weights, const float* eta,
                            const int64_t* ii, const int64_t* jj,
                            int E, int nframes, int ht, int wd, int K_eta,
                            int t0, int t1, int iterations, float lm, float ep, float ep_c, int free_mask,
                            float* dx_out, float* dz_out, int dz_rows, float* dc_out, int* status_out,
                            void* workspace, size_t workspace_bytes, void* calib_workspace, size_t calib_bytes, void* stream) {
  int rc = check_common(E, nframes, ht, wd, t0, t1);
  if (rc != PVO_OK) return rc;
  const int P = t1 - t0, HW = ht * wd, n = 6 * P;
  if (P < 1 || P > kCalibMaxPoses) return PVO_EUNSUPPORTED;
  if (E < 1 || iterations < 0 || !(ep_c >= 0.0f) || free_mask < 0 || free_mask > 15) return PVO_EINVAL;
  if (!poses || !disps || !intrinsics || !targets || !weights || !eta || !ii || !jj || !workspace || !calib_workspace) return PVO_EINVAL;
  Ws w;
  if (!carve_checked(&w, workspace, workspace_bytes, E, P, nframes, HW)) return PVO_EWORKSPACE;
  if (calib_bytes < pvo_ba_calib_workspace_bytes(E, P, nframes, HW)) return PVO_EWORKSPACE;
  CalibWs c = carve_calib(ws_base(calib_workspace), E, P, nframes, HW);
  hipStream_t st = pvo_stream(stream);
  rc = launch_plan(w, ii, jj, E, nframes, t0, t1, K_eta, 0, nullptr, 0.0f, 0.0f, st);
  if (rc != PVO_OK) return rc;
  if (hipMemsetAsync(c.dc, 0, sizeof(float) * 8, st) != hipSuccess) return PVO_ELAUNCH;
  int* cflag = reinterpret_cast<int*>(c.dc) + 5;
  const int Kmax = depth_rows_bound(nframes, P, E);
  const int chunks = (HW + 255) / 256;
  for (int it = 0; it < iterations; ++it) {
    rc = pvo_ba_local(poses, disps, intrinsics, targets, weights, eta, ii, jj, E, nframes, ht, wd, K_eta, t0, t1, 0, w.sys,
                      workspace, workspace_bytes, stream);
    if (rc != PVO_OK) return rc;
    if (hipMemsetAsync(c.fix, 0, sizeof(long long) * (static_cast<size_t>(n) * 4 + 20), st) != hipSuccess) return PVO_ELAUNCH;
    hipLaunchKernelGGL(ba_calib_assemble_kernel, dim3(chunks, E), dim3(256), 0, st, poses, disps, intrinsics, targets, weights, ii, jj,
                       c.gc, c.fix, cflag, HW, wd, t0, P);
    hipLaunchKernelGGL(ba_calib_schur_kernel, dim3(chunks, Kmax), dim3(256), 0, st, w.plan, jj, w.Ei, w.Eij, w.Q, w.w, c.gc, c.Gc,
                       c.fix, cflag, HW, t0, P);
    PVO_CHECK_LAUNCH();
    rc = launch_pose_cov(w, w.sys, n, lm, ep, c.X, nullptr, st);
    if (rc != PVO_OK) return rc;
    hipLaunchKernelGGL(ba_calib_solve_kernel, dim3(1), dim3(1024), 0, st, w.sys, c.X, reinterpret_cast<const int*>(w.chol + static_cast<size_t>(n) * n),
                       c.fix, w.plan.meta, poses, intrinsics, w.dx, dx_out, c.dc, dc_out, status_out, P, t0, lm, ep_c, free_mask);
    hipLaunchKernelGGL(ba_calib_backsub_kernel, dim3(chunks, Kmax), dim3(256), 0, st, w.plan, jj, w.Ei, w.Eij, w.Q, w.w, w.dx, c.Gc, c.dc,
                       disps, dz_out, dz_rows, HW, t0, P);
    PVO_CHECK_LAUNCH();
  }
  return PVO_OK;
}
