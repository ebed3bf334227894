// Continuous-filter convolution (spk_cfconv.hip) and its table-driven experiment (spk_tabfilter.hip): what the drivers call.
#pragma once
#include "spk_common.h"

int spk_cfconv_fwd_internal(const spk_graph_t* g, const spk_radial_t* rb, const float* h,
                            const float* r_ij, const float* w1, const float* b1, const float* w2,
                            const float* b2, int nf, float* y, hipStream_t stream, bool pre_zeroed,
                            float* gsave);
int spk_cfconv_bwd_internal(const spk_graph_t* g, const spk_radial_t* rb, const float* h,
                            const float* gy, const float* r_ij, const float* w1, const float* b1,
                            const float* w2, const float* b2, int nf, float* gh, float* gr,
                            hipStream_t stream, bool pre_zeroed, const float* gload, bool gr_assign, bool want_gh);
// floats of filter save space per interaction if the pair kernel will run for this graph/shape, else 0
int64_t spk_cfconv_gsave_floats(const spk_graph_t* g, const spk_radial_t* rb, int nf);

// per-call compaction of the pair list (pairs inside the cutoff, order kept) and the floats of workspace it needs
int64_t spk_active_pairs_floats(int64_t n_half);
int spk_active_pairs_internal(const spk_graph_t* g, const float* r_ij, float cutoff, float* ws, hipStream_t stream,
                              const int32_t** half_out, const int32_t** count_out);

// EXPERIMENT (spk_tabfilter.hip): layers with a registered filter table, found by the device pointer of filter_network.1.weight,
// run the table-driven row kernels
bool spk_filter_table_lookup(const float* key, const float** table, int* n_knots, float* d_max);
int spk_cfconv_tab_bwd_internal(const spk_graph_t* g, const float* r_ij, const float* h, const float* gy, const float* table, int n_knots, float d_max,
                                float cutoff, float* gh, float* gr, bool gr_assign, hipStream_t stream);
