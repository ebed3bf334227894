// Dense layers and fused Dense chains (spk_dense.hip, spk_chain.hip): what the other translation units call.
#pragma once
#include "spk_common.h"

// one Dense layer on the single-layer kernels, any shape (spk_dense.hip)
int spk_dense_internal(const float* in, const float* pre_in, const float* w, const float* b,
                       const float* res, float* out, float* pre_out, int64_t M, int KC, int NW,
                       int act, bool trans, int pro, hipStream_t stream);

// packed fp32 image of a Linear weight (spk_pack_weight_f32) and its split-precision image (spk_split.h), spk_chain.hip
int spk_pack_weight_internal(const float* w, int n_out, int k_in, int transposed, float* packed, hipStream_t stream);
int spk_pack_weight_split_internal(const float* w, int n_out, int k_in, int transposed, float* packed, hipStream_t stream);

// spk_dense_chain_f32 with the split-precision images of its layers: w_split is NULL, or c->n_layers images that belong to the
// packed images in c->layers[l].w (NULL entries allowed).  The split-precision kernel runs when 32-row tiles are in use, the split
// path is switched on (spk_set_split), every layer has an image and every contraction length is a multiple of 64.
int spk_dense_chain_launch(const spk_chain_t* c, const float* const* w_split, hipStream_t stream);

static inline spk_chain_layer_t spk_chain_layer(const float* w, const float* b, const float* res, float* out, float* pre_out,
                                                const float* post_pre, int k, int n_out, int act, int trans, int post_act) {
  spk_chain_layer_t L;
  L.w = w; L.b = b; L.res = res; L.out = out; L.pre_out = pre_out; L.post_pre = post_pre;
  L.k = k; L.n_out = n_out; L.act = act; L.trans = trans; L.post_act = post_act;
  return L;
}

// forward layer from either the [out,in] weight or its transposed copy (coalesced reads)
static inline spk_chain_layer_t spk_chain_fwd_layer(const float* w, const float* wT, const float* b, const float* res, float* out,
                                                    float* pre_out, int k, int n_out, int act) {
  return wT ? spk_chain_layer(wT, b, res, out, pre_out, nullptr, k, n_out, act, 1, 0)
            : spk_chain_layer(w, b, res, out, pre_out, nullptr, k, n_out, act, 0, 0);
}
