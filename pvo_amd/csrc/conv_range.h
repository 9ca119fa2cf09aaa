// conv_range.h — edges [e0, e1) of the wide 3x3 convolution's launchers (conv_small.hip) and of the trunk's launches (the lookup,
// the encoders' convolutions), for update_exec.hip's edge-blocked schedule.  Each is its exported namesake with every per-edge
// operand moved to edge e0 and the grid's edge dimension = e1 - e0: the same workgroups on the same operands, so any partition of
// [0, E) writes the bits the whole launch writes.  Not part of the C ABI.
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
// the trunk: pvo_conv7x7_c8 and pvo_conv3x3_c128 (conv_small.hip; grid.z = edge), pvo_corr_lookup_encode_tiled (corr_lookup.hip; grid.y =
// edge: coords, out and the slot table move, the pool base and num_slots stay - without a slot table each level's base moves) and
// pvo_corr_encode (operator_small.hip; a grid of 64-row tiles over rows [e0 * H * W, e1 * H * W): every output row is a function of
// its own input row alone, so a block that does not start on a tile boundary of the whole launch still writes the same bits)
int pvo_internal_conv7x7_c8_range(const void* x, const void* w_taps, const float* bias, void* y, int E, int e0, int e1, int H, int W,
                                  int dtype, void* stream) PVO_INTERNAL;
int pvo_internal_conv3x3_c128_range(const void* x, const void* w_taps, const float* bias, void* y, int E, int e0, int e1, int H, int W,
                                    int Cout, int relu, int ystride, int yoff, int dtype, void* stream) PVO_INTERNAL;
int pvo_internal_corr_lookup_encode_tiled_range(const void* const* volumes_host, const float* coords, const void* enc_weight,
                                                const float* enc_bias, void* out, int N, int e0, int e1, int h1, int w1, int dtype,
                                                const int* slots, int num_slots, void* stream) PVO_INTERNAL;
int pvo_internal_corr_encode_range(const void* corr, const void* enc_weight, const float* enc_bias, void* y, int E, int e0, int e1,
                                   int HW, int dtype, void* stream) PVO_INTERNAL;

#undef PVO_INTERNAL
