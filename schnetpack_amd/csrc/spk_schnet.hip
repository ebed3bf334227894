// Whole-representation drivers for SchNet (representation/schnet.py:147-173): every kernel of one
// forward (or one first-order backward) is enqueued on the caller's stream from a single C call.
// Per interaction: ONE fused edge kernel (cfconv) and ONE fused atom-wise chain kernel
// (f2out.0 -> f2out.1 + residual -> next in2f; resp. their transposes in the backward), which also
// clears the accumulation buffer of the next edge kernel.
#include "spk_common.h"
#include "spk_cfconv.h"
#include "spk_schnet_mol.h"

// EXPERIMENT (spk_tabfilter.hip): a model whose first interaction has a registered filter table runs the general driver with the
// table-driven cfconv kernels (the molecule-resident launches evaluate the filter network themselves)
static bool schnet_tabulated(const spk_schnet_t* m) {
  const float* tab; int nk; float dmax;
  return m && m->layers && m->n_interactions > 0 && spk_filter_table_lookup(m->layers[0].fn_w2, &tab, &nk, &dmax);
}

static int check_model(const spk_schnet_t* m, const char* who) {
  SPK_CHECK_ARG(m != nullptr && m->layers != nullptr, "%s: null model", who);
  SPK_CHECK_ARG(m->n_atom_basis > 0 && m->n_filters > 0 && m->n_interactions >= 0, "%s: bad model sizes", who);
  return SPK_OK;
}

// saved: per interaction h [N,nf] | pre3 [N,F], followed (optionally) by the raw filter outputs
// g_e of every interaction ([n_half_padded, nf] each) when `n_edges_hint` > 0 was given
extern "C" int64_t spk_schnet_saved_floats(const spk_schnet_t* m, int64_t n_atoms) {
  if (!m) return 0;
  return (int64_t)m->n_interactions * n_atoms * (m->n_filters + m->n_atom_basis);
}
// the per-call compacted pair list lives behind the saved filters (only when the pair kernels run)
static bool schnet_filter_on(const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb) {
  // (the experimental group-local kernels address `half` through per-group offsets: no compaction there)
  return g->filter_pairs && g->n_half > 0 && spk_get_variant() != SPK_VARIANT_MFMA_MOL &&
         spk_cfconv_gsave_floats(g, rb, m->n_filters) > 0;
}
static int64_t schnet_saved_floats_before_records(const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb) {
  return spk_schnet_saved_floats(m, g->n_atoms) + (int64_t)m->n_interactions * spk_cfconv_gsave_floats(g, rb, m->n_filters) +
         (schnet_filter_on(m, g, rb) ? spk_active_pairs_floats(g->n_half) : 0);
}
// The records region (spk_schnet_mol.hip: the pair records of every group, handed from the molecule-resident forward to the backward)
// lies behind every other region of `saved`, so no other offset depends on it.  It exists exactly when the caller asked for it (bit 1
// of the model word: `saved` is sized for it), the filters are saved and the molecule-resident backward covers the list -- the
// condition under which the forward compacts its pair tiles.  *off: first float of the region, rounded up to a multiple of four
// (16-byte records); *floats: what spk_schnet_saved_floats_graph() grows by = that padding + 8 n_half + n_groups
// (records 4 n_half | pair vectors 3 n_half | record index per list position n_half | records per group n_groups).
bool spk_schnet_mol_records_region(const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb, int64_t* off, int64_t* floats) {
  *off = 0; *floats = 0;
  if (!m || !g || !rb || (m->reserved & 3) != 3 || !m->layers || m->n_interactions <= 0) return false;
  if (spk_cfconv_gsave_floats(g, rb, m->n_filters) <= 0 || !spk_schnet_mol_bwd_eligible(m, g, rb)) return false;
  const int64_t end = schnet_saved_floats_before_records(m, g, rb);
  *off = (end + 3) & ~(int64_t)3;
  *floats = (*off - end) + 8 * (int64_t)g->n_half + g->n_groups;
  return true;
}
extern "C" int64_t spk_schnet_mol_records_floats(const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb) {
  int64_t off, floats;
  spk_schnet_mol_records_region(m, g, rb, &off, &floats);
  return floats;
}
extern "C" int64_t spk_schnet_saved_floats_graph(const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb) {
  if (!m || !g || !rb) return 0;
  return schnet_saved_floats_before_records(m, g, rb) + spk_schnet_mol_records_floats(m, g, rb);
}

// scratch: forward  y0 | y1 | t0 | t1            (2 nf + 2 max(F, nf))
//          backward gh0 | gh1 | gy | gxb | t0 | t1
extern "C" int64_t spk_schnet_scratch_floats(const spk_schnet_t* m, int64_t n_atoms) {
  if (!m) return 0;
  const int64_t mx = m->n_filters > m->n_atom_basis ? m->n_filters : m->n_atom_basis;
  return n_atoms * (3 * (int64_t)m->n_filters + (int64_t)m->n_atom_basis + 2 * mx);
}

// order of the packed images in spk_schnet_t::wpack: per interaction in2f, f2out.0, f2out.1 (forward, transposed each)
static bool schnet_pack_shapes_ok(const spk_schnet_t* m) { return m->n_atom_basis % 128 == 0 && m->n_filters % 128 == 0 && m->n_atom_basis <= 384 && m->n_filters <= 384; }
static SpkPackTable schnet_pack_table(const spk_schnet_t* m) {
  SpkPackTable T;
  const int F = m->n_atom_basis, NF = m->n_filters;
  for (int l = 0; l < m->n_interactions; ++l) {
    const spk_schnet_layer_t& P = m->layers[l];
    T.add(P.in2f_w, P.in2f_wT, NF, F);
    T.add(P.f2out_w1, P.f2out_w1T, F, NF);
    T.add(P.f2out_w2, P.f2out_w2T, F, F);
  }
  // the split-precision LDS image of filter_network.1.weight of every interaction (spk_schnet_mol.hip: staged by a plain copy)
  if (NF == 128)
    for (int l = 0; l < m->n_interactions; ++l) T.add_extra(m->layers[l].fn_w2, 128 * 128);
  T.base = m->wpack;
  return T;
}
extern "C" int64_t spk_schnet_packed_floats(const spk_schnet_t* m) {
  if (!m || !m->layers || m->n_interactions <= 0 || !schnet_pack_shapes_ok(m)) return 0;
  return schnet_pack_table(m).total;
}
extern "C" int spk_schnet_pack_weights_f32(const spk_schnet_t* m, float* wpack, void* stream) {
  SPK_CHECK_ARG(m && wpack && spk_schnet_packed_floats(m) > 0, "spk_schnet_pack_weights_f32: model shapes have no packed form (see spk_schnet_packed_floats)");
  const SpkPackTable T = schnet_pack_table(m);
  int rc = spk_pack_all(T, wpack, (hipStream_t)stream);
  for (const SpkPackExtra& q : T.x) {
    if (rc) break;
    rc = spk_schnet_mol_pack_w2(q.raw, wpack + q.off, (hipStream_t)stream);
  }
  return rc;
}

extern "C" int spk_schnet_forward_f32(const spk_schnet_t* m, const spk_graph_t* g,
                                      const spk_radial_t* rb, const float* x0, const float* r_ij,
                                      float* x_out, float* saved, float* scratch, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "spk_schnet_forward_f32";
  SPK_TRY(check_model(m, who));
  const SpkPackTable ptab = (m->wpack && schnet_pack_shapes_ok(m)) ? schnet_pack_table(m) : SpkPackTable();
  SPK_CHECK_ARG(g != nullptr && rb != nullptr, "%s: null graph/radial", who);
  const int64_t N = g->n_atoms;
  const int F = m->n_atom_basis, NF = m->n_filters, L = m->n_interactions;
  if (N == 0) return SPK_OK;
  SPK_CHECK_ARG(x0 && x_out && (L == 0 || (saved && scratch)), "%s: null buffer", who);
  if (L == 0) {
    SPK_HIP_TRY(hipMemcpyAsync(x_out, x0, (size_t)N * F * sizeof(float), hipMemcpyDeviceToDevice, stream));
    return SPK_OK;
  }
  const int64_t mx = NF > F ? NF : F;
  float* ybuf[2] = {scratch, scratch + N * (int64_t)NF};
  float* tmp0 = scratch + 2 * N * (int64_t)NF;
  float* tmp1 = tmp0 + N * mx;
  auto hbuf = [&](int l) { return saved + (int64_t)l * N * (NF + F); };
  const int64_t gsz = (m->reserved & 1) ? spk_cfconv_gsave_floats(g, rb, NF) : 0;  // bit 0: saved has filter space
  float* gbase = saved + (int64_t)L * N * (NF + F);
  // batches of small molecules with the filters saved for the backward: the whole forward is one molecule-resident launch
  if (gsz > 0 && ptab.base && spk_schnet_mol_eligible(m, g, rb) && !schnet_tabulated(m))
    return spk_schnet_mol_forward(m, g, rb, ptab, x0, r_ij, x_out, saved, gsz, stream);
  // skin lists: compact the pair list of THIS call (pairs inside the cutoff, order kept) behind the saved filters
  spk_graph_t gact = *g;
  if (gsz > 0 && schnet_filter_on(m, g, rb)) {
    const int32_t *ah = nullptr, *ac = nullptr;
    SPK_TRY(spk_active_pairs_internal(g, r_ij, rb->cutoff, gbase + (int64_t)L * gsz, stream, &ah, &ac));
    gact.half = ah; gact.n_half_dev = ac;
  }
  g = &gact;
  // prelude: h_0 = in2f_0(x0); clear y of the first edge kernel
  {
    spk_chain_t c = {};
    c.n_layers = 1; c.m = N; c.in = x0; c.zero_ptr = ybuf[0]; c.zero_count = N * (int64_t)NF;
    c.tmp[0] = tmp0; c.tmp[1] = tmp1;
    c.layers[0] = spk_chain_fwd_layer(m->layers[0].in2f_w, m->layers[0].in2f_wT, nullptr, nullptr, hbuf(0), nullptr, F, NF, SPK_ACT_NONE);
    SPK_TRY(spk_chain_run(c, ptab, stream));
  }
  for (int l = 0; l < L; ++l) {
    const spk_schnet_layer_t& P = m->layers[l];
    float* h = hbuf(l);
    float* pre3 = h + N * (int64_t)NF;
    float* y = ybuf[l & 1];
    const float* xin = (l == 0) ? x0 : x_out;
    SPK_TRY(spk_cfconv_fwd_internal(g, rb, h, r_ij, P.fn_w1, P.fn_b1, P.fn_w2, P.fn_b2, NF, y, stream, true,
                                    gsz > 0 ? gbase + l * gsz : nullptr));
    spk_chain_t c = {};
    c.m = N; c.in = y; c.tmp[0] = tmp0; c.tmp[1] = tmp1;
    c.layers[0] = spk_chain_fwd_layer(P.f2out_w1, P.f2out_w1T, P.f2out_b1, nullptr, nullptr, pre3, NF, F, SPK_ACT_SSP);
    c.layers[1] = spk_chain_fwd_layer(P.f2out_w2, P.f2out_w2T, P.f2out_b2, xin, x_out, nullptr, F, F, SPK_ACT_NONE);
    c.n_layers = 2;
    if (l + 1 < L) {
      c.layers[2] = spk_chain_fwd_layer(m->layers[l + 1].in2f_w, m->layers[l + 1].in2f_wT, nullptr, nullptr, hbuf(l + 1), nullptr, F, NF, SPK_ACT_NONE);
      c.n_layers = 3;
      c.zero_ptr = ybuf[(l + 1) & 1]; c.zero_count = N * (int64_t)NF;
    }
    SPK_TRY(spk_chain_run(c, ptab, stream));
  }
  return SPK_OK;
}

extern "C" int spk_schnet_backward_f32(const spk_schnet_t* m, const spk_graph_t* g,
                                       const spk_radial_t* rb, const float* gx_out,
                                       const float* r_ij, const float* saved, float* scratch,
                                       float* gr, float* gx0, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "spk_schnet_backward_f32";
  SPK_TRY(check_model(m, who));
  const SpkPackTable ptab = (m->wpack && schnet_pack_shapes_ok(m)) ? schnet_pack_table(m) : SpkPackTable();
  SPK_CHECK_ARG(g != nullptr && rb != nullptr, "%s: null graph/radial", who);
  const int64_t N = g->n_atoms, E = g->n_edges;
  const int F = m->n_atom_basis, NF = m->n_filters, L = m->n_interactions;
  // batches of small molecules: the whole backward is one molecule-resident launch (it assigns every entry of gr)
  if (L > 0 && N > 0 && E > 0 && (m->reserved & 1) && ptab.base && gx_out && saved && gr && spk_schnet_mol_bwd_eligible(m, g, rb) && !schnet_tabulated(m)) {
    const int64_t gsz_m = spk_cfconv_gsave_floats(g, rb, NF);
    if (gsz_m > 0) return spk_schnet_mol_backward(m, g, rb, ptab, gx_out, r_ij, saved, gsz_m, gr, gx0, stream);
  }
  SPK_CHECK_ARG(spk_schnet_mol_bwd_records_mode() != 2, "%s: records mode 2, but `saved` of this model / list has no records region", who);
  // with saved filters the pair kernel runs and writes every entry of gr exactly once per interaction: the
  // first interaction of the backward assigns, the others accumulate -- no clearing pass
  const bool gr_assign = L > 0 && (m->reserved & 1) && E > 0 && spk_cfconv_gsave_floats(g, rb, NF) > 0 &&
                         (!schnet_filter_on(m, g, rb) || (ptab.base && spk_schnet_mol_eligible(m, g, rb)));
  if (E > 0) {
    SPK_CHECK_ARG(gr != nullptr, "%s: null gr", who);
    if (!gr_assign) SPK_TRY(spk_zero_async(gr, (size_t)E * 3 * sizeof(float), stream));
  }
  if (N == 0) return SPK_OK;
  SPK_CHECK_ARG(gx_out && (L == 0 || (saved && scratch)), "%s: null buffer", who);
  if (L == 0) {
    if (gx0) SPK_HIP_TRY(hipMemcpyAsync(gx0, gx_out, (size_t)N * F * sizeof(float), hipMemcpyDeviceToDevice, stream));
    return SPK_OK;
  }
  const int64_t mx = NF > F ? NF : F;
  float* ghbuf[2] = {scratch, scratch + N * (int64_t)NF};
  float* gy = scratch + 2 * N * (int64_t)NF;
  float* gxb = gy + N * (int64_t)NF;
  float* tmp0 = gxb + N * (int64_t)F;
  float* tmp1 = tmp0 + N * mx;
  auto hbuf = [&](int l) { return saved + (int64_t)l * N * (NF + F); };
  auto pre3 = [&](int l) { return saved + (int64_t)l * N * (NF + F) + N * (int64_t)NF; };
  const int64_t gsz = (m->reserved & 1) ? spk_cfconv_gsave_floats(g, rb, NF) : 0;
  const float* gbase = saved + (int64_t)L * N * (NF + F);
  // the compacted pair list written by the forward of this call (the molecule-resident forward writes none: it keeps
  // the full pair list, and so does this backward then -- saved filters are addressed by pair position)
  const bool mol_fwd = gsz > 0 && ptab.base && spk_schnet_mol_eligible(m, g, rb) && !schnet_tabulated(m);
  spk_graph_t gact = *g;
  if (gsz > 0 && !mol_fwd && schnet_filter_on(m, g, rb)) {
    const int32_t* ah = (const int32_t*)(gbase + (int64_t)L * gsz);
    gact.half = ah; gact.n_half_dev = ah + g->n_half;
  }
  const bool filtered = gact.n_half_dev != nullptr;
  // prelude: gy_{L-1} = ((gx W4) * ssp'(pre3)) W3 ; clear gh of the first edge kernel
  {
    const spk_schnet_layer_t& P = m->layers[L - 1];
    spk_chain_t c = {};
    c.n_layers = 2; c.m = N; c.in = gx_out; c.zero_ptr = ghbuf[(L - 1) & 1]; c.zero_count = N * (int64_t)NF;
    c.tmp[0] = tmp0; c.tmp[1] = tmp1;
    c.layers[0] = spk_chain_layer(P.f2out_w2, nullptr, nullptr, nullptr, nullptr, pre3(L - 1), F, F, SPK_ACT_NONE, 1, SPK_ACT_SSP);
    c.layers[1] = spk_chain_layer(P.f2out_w1, nullptr, nullptr, gy, nullptr, nullptr, F, NF, SPK_ACT_NONE, 1, 0);
    SPK_TRY(spk_chain_run(c, ptab, stream));
  }
  const float* gx = gx_out;
  for (int l = L - 1; l >= 0; --l) {
    const spk_schnet_layer_t& P = m->layers[l];
    float* gh = ghbuf[l & 1];
    SPK_TRY(spk_cfconv_bwd_internal(filtered ? &gact : g, rb, hbuf(l), gy, r_ij, P.fn_w1, P.fn_b1, P.fn_w2, P.fn_b2, NF, gh, gr, stream, true,
                                    gsz > 0 ? gbase + l * gsz : nullptr, gr_assign && l == L - 1, !(l == 0 && !gx0)));
    if (l == 0 && !gx0) break;  // dL/dx0 not requested (eval path): nothing below feeds dL/dr_ij, and the edge kernel
                                // above was told not to form dL/dh (no transposed sum, no atomics)
    float* out = (l == 0) ? gx0 : gxb;
    spk_chain_t c = {};
    c.m = N; c.in = gh; c.tmp[0] = tmp0; c.tmp[1] = tmp1;
    // in2f: h = x W_in^T ; residual path adds gx
    c.layers[0] = spk_chain_layer(P.in2f_w, nullptr, gx, out, nullptr, nullptr, NF, F, SPK_ACT_NONE, 1, 0);
    c.n_layers = 1;
    if (l > 0) {
      const spk_schnet_layer_t& Q = m->layers[l - 1];
      c.layers[0].post_pre = nullptr;
      c.layers[1] = spk_chain_layer(Q.f2out_w2, nullptr, nullptr, nullptr, nullptr, pre3(l - 1), F, F, SPK_ACT_NONE, 1, SPK_ACT_SSP);
      c.layers[2] = spk_chain_layer(Q.f2out_w1, nullptr, nullptr, gy, nullptr, nullptr, F, NF, SPK_ACT_NONE, 1, 0);
      c.n_layers = 3;
      c.zero_ptr = ghbuf[(l - 1) & 1]; c.zero_count = N * (int64_t)NF;
    }
    SPK_TRY(spk_chain_run(c, ptab, stream));
    gx = out;
  }
  return SPK_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// The standard potential  PairwiseDistances -> SchNet -> Atomwise(sum) -> Forces  on batches of small molecules: TWO launches, forward
// and backward -- and ONE for the force call (energies and forces, dL/dE = 1: schnet_potential_forces below), which runs the two
// back to back in one kernel
// (atomistic/distances.py:14-26, representation/schnet.py:147-173, atomistic/atomwise.py:69-88, atomistic/response.py:59-76).
static bool potential_ok(const spk_schnet_t* m, const spk_head_t* head, const spk_graph_t* g, const spk_radial_t* rb) {
  if (!m || !head || !g || !rb || !m->layers || m->n_interactions <= 0 || !(m->reserved & 1)) return false;
  if (schnet_tabulated(m)) return false;          // (experiment) registered filter tables: the stage-by-stage path runs the table kernels
  if (!m->wpack || !schnet_pack_shapes_ok(m)) return false;
  if (!head->w1 || !head->w1t || !head->b1 || !head->w2 || head->n_hidden < 32 || head->n_hidden > 128 || head->n_hidden % 32) return false;
  if (head->act != SPK_ACT_SSP && head->act != SPK_ACT_SILU) return false;
  if (getenv("SPK_NO_POTENTIAL")) return false;
  return spk_schnet_mol_eligible(m, g, rb) && spk_schnet_mol_bwd_eligible(m, g, rb) && spk_cfconv_gsave_floats(g, rb, m->n_filters) > 0;
}
extern "C" int spk_schnet_potential_supported(const spk_schnet_t* m, const spk_head_t* head, const spk_graph_t* g, const spk_radial_t* rb) {
  return potential_ok(m, head, g, rb) ? 1 : 0;
}

extern "C" int spk_schnet_potential_forward_f32(const spk_schnet_t* m, const spk_head_t* head, const spk_graph_t* g, const spk_radial_t* rb,
                                                const float* x0, const float* R, const float* offsets, const int64_t* idx_m, int64_t n_mol,
                                                float* x_out, float* E, float* pre_h, float* saved, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "spk_schnet_potential_forward_f32";
  SPK_TRY(check_model(m, who));
  SPK_CHECK_ARG(potential_ok(m, head, g, rb), "%s: model / list not covered by the fused potential (see spk_schnet_potential_supported)", who);
  SPK_CHECK_ARG(n_mol >= 0 && (n_mol == 0 || E), "%s: null energy buffer", who);
  if (n_mol > 0) SPK_TRY(spk_zero_async(E, (size_t)n_mol * sizeof(float), stream));
  if (g->n_atoms == 0) return SPK_OK;
  SPK_CHECK_ARG(x0 && R && idx_m && x_out && pre_h && saved, "%s: null buffer", who);
  MolHeadDev h;
  h.w1 = head->w1; h.w1t = head->w1t; h.b1 = head->b1; h.w2 = head->w2; h.b2 = head->b2; h.H = head->n_hidden; h.act = head->act;
  h.idx_m = idx_m; h.E = E; h.pre_h = pre_h; h.gE = nullptr; h.direct_store = 0; h.negate = 0;
  return spk_schnet_mol_forward_ex(m, g, rb, schnet_pack_table(m), x0, nullptr, R, offsets, &h, x_out, saved,
                                   spk_cfconv_gsave_floats(g, rb, m->n_filters), stream);
}

extern "C" int spk_schnet_potential_backward_f32(const spk_schnet_t* m, const spk_head_t* head, const spk_graph_t* g, const spk_radial_t* rb,
                                                 const float* gE, const float* gx_out, const float* R, const float* offsets, const int64_t* idx_m,
                                                 const float* pre_h, const float* saved, float* gR, float* gx0, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "spk_schnet_potential_backward_f32";
  SPK_TRY(check_model(m, who));
  SPK_CHECK_ARG(potential_ok(m, head, g, rb), "%s: model / list not covered by the fused potential (see spk_schnet_potential_supported)", who);
  if (g->n_atoms == 0) return SPK_OK;
  SPK_CHECK_ARG(gE && R && idx_m && pre_h && saved && gR, "%s: null buffer", who);
  MolHeadDev h;
  h.w1 = head->w1; h.w1t = head->w1t; h.b1 = head->b1; h.w2 = head->w2; h.b2 = head->b2; h.H = head->n_hidden; h.act = head->act;
  h.idx_m = idx_m; h.E = nullptr; h.pre_h = const_cast<float*>(pre_h); h.gE = gE; h.direct_store = 0; h.negate = 0;
  return spk_schnet_mol_backward_ex(m, g, rb, schnet_pack_table(m), gx_out, nullptr, R, offsets, &h, saved,
                                    spk_cfconv_gsave_floats(g, rb, m->n_filters), nullptr, gR, gx0, stream);
}

// Energies and FORCES of the standard potential in one launch (or the two launches: see below), nothing else: x0 may be NULL (the rows of the nuclear
// embedding table `emb` [n_types, F] are looked up by Z inside the forward launch), dL/dE is 1 (forces of the summed energy), the
// backward writes -dE/dR.  all_inside != 0: the caller guarantees that every molecule's atoms lie inside ONE group of the plan and
// that every molecule has an atom -- the energies are then stored, not accumulated, and E needs no clearing launch.
static int schnet_potential_forces(const spk_schnet_t* m, const spk_head_t* head, const spk_graph_t* g, const spk_radial_t* rb,
                                               const float* x0, const float* emb, const int64_t* Z, int32_t n_types, const float* R,
                                               const float* offsets, const int64_t* idx_m, int64_t n_mol, int32_t all_inside, float* x_out, float* E,
                                               float* F, float* gr, float* pre_h, float* saved, const char* who, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPK_TRY(check_model(m, who));
  SPK_CHECK_ARG(potential_ok(m, head, g, rb), "%s: model / list not covered by the fused potential (see spk_schnet_potential_supported)", who);
  SPK_CHECK_ARG(n_mol >= 0 && (n_mol == 0 || E), "%s: null energy buffer", who);
  SPK_CHECK_ARG(x0 || (emb && Z && n_types > 0), "%s: neither features nor an embedding table", who);
  if (n_mol > 0 && !all_inside) SPK_TRY(spk_zero_async(E, (size_t)n_mol * sizeof(float), stream));
  if (g->n_atoms == 0) return SPK_OK;
  SPK_CHECK_ARG(R && idx_m && x_out && F && pre_h && saved, "%s: null buffer", who);
  MolHeadDev h;
  h.w1 = head->w1; h.w1t = head->w1t; h.b1 = head->b1; h.w2 = head->w2; h.b2 = head->b2; h.H = head->n_hidden; h.act = head->act;
  h.idx_m = idx_m; h.E = E; h.pre_h = pre_h; h.gE = nullptr; h.direct_store = all_inside ? 1 : 0; h.negate = 1;
  const SpkPackTable ptab = schnet_pack_table(m);
  const int64_t gsz = spk_cfconv_gsave_floats(g, rb, m->n_filters);
  // One launch (k_schnet_mol_force) where the call is eligible -- split path, records region in `saved`, records mode not 1 -- and the
  // per-launch profile is off; with the profile on the two launches stay, so that its tags schnet_mol_fwd / schnet_mol_bwd keep
  // telling which half ran and what to book to it.  spk_schnet_mol_set_force_launches(): 1 = one launch regardless, 2 = two.
  const int launches = spk_schnet_mol_force_launches();
  const bool can_fuse = spk_schnet_mol_force_eligible(m, g, rb, gsz);
  SPK_CHECK_ARG(launches != 1 || can_fuse, "%s: force launches = 1, but this call is not eligible for one launch (split path off, no records region, or records mode 1)", who);
  if (can_fuse && (launches == 1 || (launches == 0 && !spk_prof_enabled())))
    return spk_schnet_mol_force_ex(m, g, rb, ptab, x0, R, offsets, &h, x_out, saved, gsz, gr, F, stream, x0 ? nullptr : emb, Z, n_types);
  SPK_TRY(spk_schnet_mol_forward_ex(m, g, rb, ptab, x0, nullptr, R, offsets, &h, x_out, saved, gsz, stream, x0 ? nullptr : emb, Z, n_types));
  return spk_schnet_mol_backward_ex(m, g, rb, ptab, nullptr, nullptr, R, offsets, &h, saved, gsz, gr, F, nullptr, stream);
}

extern "C" int spk_schnet_potential_forces_f32(const spk_schnet_t* m, const spk_head_t* head, const spk_graph_t* g, const spk_radial_t* rb,
                                               const float* x0, const float* emb, const int64_t* Z, int32_t n_types, const float* R,
                                               const float* offsets, const int64_t* idx_m, int64_t n_mol, int32_t all_inside, float* x_out, float* E,
                                               float* F, float* pre_h, float* saved, void* stream_) {
  return schnet_potential_forces(m, head, g, rb, x0, emb, Z, n_types, R, offsets, idx_m, n_mol, all_inside, x_out, E, F, nullptr, pre_h, saved,
                                 "spk_schnet_potential_forces_f32", stream_);
}

// The same, and the backward launch also writes dE/dr [E, 3] of every edge (the input of the virial, spk_edge_virial_f32); the forces are
// those of spk_schnet_potential_forces_f32 bit for bit.
extern "C" int spk_schnet_potential_forces_gr_f32(const spk_schnet_t* m, const spk_head_t* head, const spk_graph_t* g, const spk_radial_t* rb,
                                                  const float* x0, const float* emb, const int64_t* Z, int32_t n_types, const float* R,
                                                  const float* offsets, const int64_t* idx_m, int64_t n_mol, int32_t all_inside, float* x_out,
                                                  float* E, float* F, float* gr, float* pre_h, float* saved, void* stream_) {
  const char* who = "spk_schnet_potential_forces_gr_f32";
  SPK_CHECK_ARG(g && (g->n_edges == 0 || gr), "%s: null edge gradient", who);
  return schnet_potential_forces(m, head, g, rb, x0, emb, Z, n_types, R, offsets, idx_m, n_mol, all_inside, x_out, E, F, gr, pre_h, saved, who,
                                 stream_);
}
