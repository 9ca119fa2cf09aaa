// conv_range.h — edges [e0, e1) of the wide 3x3 convolution's launchers (conv_small.hip), for update_exec.hip's edge-blocked
// schedule.  Each is its exported namesake with every per-edge operand moved to edge e0 and grid.z = e1 - e0: the same
// workgroups on the same operands, so any partition of [0, E) writes the bits the whole launch writes.  Not part of the C ABI.
#pragma once

#define PVO_INTERNAL __attribute__((visibility("hidden")))

int pvo_internal_conv3x3_range(const void* x, const void* w_taps, const float* bias, void* y, int E, int e0, int e1, int H, int W,
                               int Cin, int Cout, int relu, int ystride, int yoff, int dtype, void* stream) PVO_INTERNAL;
int pvo_internal_conv3x3_heads_range(const void* x, const void* w1_taps, const float* bias1, const void* w2_frags, float* z,
                                     int E, int e0, int e1, int H, int W, int dtype, void* stream) PVO_INTERNAL;
int pvo_internal_gru_conv_gates_range(const void* net, const void* cf, int cf_channels, const void* w_taps, const float* g,
                                      const void* P_zr, const int* p_slots, void* Z, void* RN, int E, int e0, int e1, int H, int W,
                                      int dtype, void* stream) PVO_INTERNAL;
int pvo_internal_gru_conv_candidate_range(const void* RN, const void* cf, int cf_channels, const void* w_taps, const float* g,
                                          const void* P_q, const int* p_slots, const void* Z, const void* net, void* net_out,
                                          int E, int e0, int e1, int H, int W, int dtype, void* stream) PVO_INTERNAL;

#undef PVO_INTERNAL
