// Does the wide convolution (conv3x3_big_kernel) gain from v_mfma_f32_16x16x32_f16 over v_mfma_f32_32x32x16_f16 on this chip?
// Stand-alone (no library code, no torch):
//
//   hipcc --offload-arch=gfx950 -O3 -o tools/_probe/mfma_shape_probe tools/mfma_shape_probe.hip     (here)
//   tools/_probe/mfma_shape_probe                                                                 (on the GPU box)
//
// Two loops with the kernel's geometry and the SAME work per K step: 4 waves per workgroup, 2 workgroups per compute unit, every
// compute unit busy; a wave tile of 128 pixels x 64 channels; per (32-channel chunk, tap) step every wave re-reads its A fragments
// from an 18 x 18 halo in LDS by ds_read_b128 (8 per lane and step) and streams its B fragments as four 1 KB global_load_dwordx4
// from an L2-resident buffer, two steps ahead into three rotating register sets, exactly as the kernel does.
//   s32   16 x v_mfma_f32_32x32x16_f16 per step (4 M-tiles of 8 rows x 4 columns x 2 N-tiles x 2 k-halves), 80-byte position stride
//   s16   32 x v_mfma_f32_16x16x32_f16 per step (8 M-tiles of 8 rows x 2 columns x 4 N-tiles), 96-byte position stride
// Operands are random fp16.  Each shape runs back to back for >= 2 s; the last launch records, per workgroup, s_memtime and
// s_memrealtime around its loop (a buffer of their own): the in-kernel shader clock is dtime / drealtime x 100 MHz.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(2); } } while (0)

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f16v __attribute__((ext_vector_type(16)));

constexpr int kSteps = 90;                       // 10 chunks x 9 taps per pass (the gates: Cin = 320)
constexpr int kFragElems = kSteps * 8 * 512;     // one channel group's filter fragments: 737 KB, L2-resident

template <bool S16>
__global__ __launch_bounds__(256, 2) void shape_loop(const uint16_t* __restrict__ halo_src, const uint16_t* __restrict__ wt,
                                                     float* __restrict__ out, unsigned long long* __restrict__ stamps, int passes) {
  constexpr int kStride = S16 ? 96 : 80, kPitch = S16 ? 18 : 20;
  constexpr int kAcc = S16 ? 32 : 8;
  __shared__ __attribute__((aligned(16))) unsigned char As[18 * 20 * 96 + 1024];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  for (int i = tid; i < (18 * 20 * 96) / 16; i += 256)
    reinterpret_cast<u32x4*>(As)[i] = reinterpret_cast<const u32x4*>(halo_src)[(blockIdx.x * 131 + i) & 8191];
  __syncthreads();
  const unsigned char* Abase;
  if (S16) { const int p = lane & 15; Abase = As + ((8 * wm + (p >> 1)) * kPitch + (p & 1)) * kStride + (lane >> 4) * 16; }
  else { const int li = lane & 31; Abase = As + ((8 * wm + (li >> 2)) * kPitch + (li & 3)) * kStride + (lane >> 5) * 16; }
  const uint16_t* wf = wt + wn * 4 * 512 + lane * 8;
  f16v acc32[S16 ? 1 : 8];
  f4 acc16[S16 ? 32 : 1];
  for (int i = 0; i < (S16 ? 1 : 8); ++i) for (int r = 0; r < 16; ++r) acc32[i][r] = 0.0f;
  for (int i = 0; i < (S16 ? 32 : 1); ++i) for (int r = 0; r < 4; ++r) acc16[i][r] = 0.0f;
  u32x4 bset[3][4];
  auto fetch_bf = [&](u32x4 (&r)[4], int s) {
    const uint16_t* p = wf + static_cast<size_t>(s % kSteps) * 4096;
#pragma unroll
    for (int f = 0; f < 4; ++f) r[f] = *reinterpret_cast<const u32x4*>(p + f * 512);
  };
  // half h of a step: s32 = k-half h of M-tiles 0..3, s16 = M-tiles 4h .. 4h+3
  auto read_half = [&](u32x4 (&a)[4], int toff, int h) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      a[i] = *reinterpret_cast<const u32x4*>(Abase + toff + (S16 ? (4 * h + i) * 2 * kStride : i * 4 * kStride + h * 32));
  };
  fetch_bf(bset[0], 0); fetch_bf(bset[1], 1);
  const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
  __builtin_amdgcn_s_waitcnt(0xC07F);
  for (int pass = 0; pass < passes; ++pass) {
#pragma unroll 1
    for (int cc = 0; cc < kSteps / 9; ++cc) {
      u32x4 a0[4], a1[4];
      read_half(a0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int toff = ((t / 3) * kPitch + (t % 3)) * kStride;
        fetch_bf(bset[(t + 2) % 3], cc * 9 + t + 2);
        read_half(a1, toff, 1);
        const u32x4 (&bf)[4] = bset[t % 3];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (S16) {
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
              acc16[i * 4 + nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, a0[i]), __builtin_bit_cast(h8, bf[nt]), acc16[i * 4 + nt], 0, 0, 0);
          } else {
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
              acc32[i * 2 + nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8, a0[i]), __builtin_bit_cast(h8, bf[nt * 2]), acc32[i * 2 + nt], 0, 0, 0);
          }
        }
        // one LDS read / one global load behind every 2 (s16) resp. 1 (s32) MFMAs
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x8, S16 ? 2 : 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x8, S16 ? 2 : 1, 0); __builtin_amdgcn_sched_group_barrier(0x20, 1, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (t < 8) read_half(a0, ((((t + 1) / 3) * kPitch) + ((t + 1) % 3)) * kStride, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (S16) {
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
              acc16[16 + i * 4 + nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, a1[i]), __builtin_bit_cast(h8, bf[nt]), acc16[16 + i * 4 + nt], 0, 0, 0);
          } else {
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
              acc32[i * 2 + nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8, a1[i]), __builtin_bit_cast(h8, bf[nt * 2 + 1]), acc32[i * 2 + nt], 0, 0, 0);
          }
        }
        if (t < 8) {
#pragma unroll
          for (int i = 0; i < 4; ++i) { __builtin_amdgcn_sched_group_barrier(0x8, S16 ? 2 : 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  __builtin_amdgcn_s_waitcnt(0xC07F);
  const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
  float s = 0.0f;
  if (S16) { for (int i = 0; i < kAcc; ++i) for (int r = 0; r < 4; ++r) s += acc16[i][r]; }
  else { for (int i = 0; i < kAcc; ++i) for (int r = 0; r < 16; ++r) s += acc32[i][r]; }
  out[blockIdx.x * 256 + tid] = s;
  if (stamps && tid == 0) { stamps[blockIdx.x * 2] = t1 - t0; stamps[blockIdx.x * 2 + 1] = r1 - r0; }
}

template <bool S16>
static void run(const char* name, const uint16_t* halo, const uint16_t* wt, float* out, unsigned long long* stamps, int nwg, int cus) {
  const int passes = 40;
  const double flop_per_launch = static_cast<double>(nwg) * 4 * passes * kSteps * (128.0 * 64 * 32 * 2);
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  shape_loop<S16><<<nwg, 256>>>(halo, wt, out, nullptr, passes);          // warm-up / code load
  CK(hipDeviceSynchronize());
  // back to back for >= 2 s, then one timed batch of 20 launches, then the stamped launch (still under load)
  const auto start = std::chrono::steady_clock::now();
  while (std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count() < 2.0) {
    for (int i = 0; i < 10; ++i) shape_loop<S16><<<nwg, 256>>>(halo, wt, out, nullptr, passes);
    CK(hipDeviceSynchronize());
  }
  CK(hipEventRecord(e0));
  for (int i = 0; i < 20; ++i) shape_loop<S16><<<nwg, 256>>>(halo, wt, out, nullptr, passes);
  CK(hipEventRecord(e1));
  shape_loop<S16><<<nwg, 256>>>(halo, wt, out, stamps, passes);
  CK(hipDeviceSynchronize());
  float ms = 0.0f;
  CK(hipEventElapsedTime(&ms, e0, e1));
  std::vector<unsigned long long> st(2 * nwg);
  CK(hipMemcpy(st.data(), stamps, st.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  std::vector<double> ghz(nwg);
  for (int i = 0; i < nwg; ++i) ghz[i] = st[2 * i + 1] ? 0.1 * static_cast<double>(st[2 * i]) / static_cast<double>(st[2 * i + 1]) : 0.0;
  std::sort(ghz.begin(), ghz.end());
  std::vector<double> cyc(nwg);
  for (int i = 0; i < nwg; ++i) cyc[i] = static_cast<double>(st[2 * i]);
  std::sort(cyc.begin(), cyc.end());
  const double tflops = flop_per_launch * 20 / (ms * 1e-3) / 1e12;
  printf("{\"shape\": \"%s\", \"workgroups\": %d, \"cus\": %d, \"launch_us\": %.1f, \"wall_tflops\": %.1f, "
         "\"in_kernel_clock_ghz_median\": %.3f, \"in_kernel_clock_ghz_min\": %.3f, \"in_kernel_clock_ghz_max\": %.3f, "
         "\"loop_cycles_median\": %.0f}\n",
         name, nwg, cus, ms * 1e3 / 20, tflops, ghz[nwg / 2], ghz[0], ghz[nwg - 1], cyc[nwg / 2]);
  CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
}

int main() {
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount, nwg = 2 * cus;
  std::vector<uint16_t> h(kFragElems);
  srand(12345);
  for (auto& v : h) { const _Float16 f = static_cast<_Float16>((rand() / static_cast<float>(RAND_MAX) - 0.5f) * 2.0f); v = __builtin_bit_cast(uint16_t, f); }
  uint16_t *halo, *wt; float* out; unsigned long long* stamps;
  CK(hipMalloc(&halo, 8192 * 16));
  CK(hipMalloc(&wt, kFragElems * sizeof(uint16_t) + 4096 * 16));
  CK(hipMalloc(&out, nwg * 256 * sizeof(float)));
  CK(hipMalloc(&stamps, 2 * nwg * sizeof(unsigned long long)));
  CK(hipMemcpy(halo, h.data(), 8192 * 16, hipMemcpyHostToDevice));
  CK(hipMemcpy(wt, h.data(), kFragElems * sizeof(uint16_t), hipMemcpyHostToDevice));
  // alternate the shapes: s32, s16, s32, s16 (the second pair checks the first)
  for (int rep = 0; rep < 2; ++rep) {
    run<false>("32x32x16", halo, wt, out, stamps, nwg, cus);
    run<true>("16x16x32", halo, wt, out, stamps, nwg, cus);
  }
  CK(hipFree(halo)); CK(hipFree(wt)); CK(hipFree(out)); CK(hipFree(stamps));
  return 0;
}
