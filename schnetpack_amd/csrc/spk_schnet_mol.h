// Molecule-resident SchNet kernels (spk_schnet_mol.hip): what the general driver (spk_schnet.hip) calls.
#pragma once
#include "spk_common.h"
#include "spk_pack.h"

// The callers either side of the representation, folded into the two launches when the model is the standard potential
// (PairwiseDistances -> SchNet -> Atomwise(sum) -> Forces; atomistic/distances.py:14-26, atomwise.py:69-88, response.py:59-76):
// r_ij is formed from the positions, the default 2-layer energy head runs on the atom tile that is still in LDS, and the
// backward starts from dE/dE_mol and ends at dE/dR.
struct MolHeadDev {
  const float* w1;        // outnet.0.weight [H, F]   (null: no head)
  const float* w1t;       // its transpose   [F, H]   (backward)
  const float* b1;        // [H]
  const float* w2;        // outnet.1.weight [H]
  const float* b2;        // [1]
  int H, act;
  const int64_t* idx_m;   // [N]
  float* E;               // forward: [n_mol], accumulated with one atomic per (group, molecule): cleared by the caller ...
  float* pre_h;           // [N, H] pre-activation of the head's hidden layer (saved for the backward)
  const float* gE;        // backward: dL/dE [n_mol]; null = ones (forces of the summed energy)
  int direct_store;       // ... unless every molecule lies inside one group: plain stores, nothing to clear
  int negate;             // backward: write -dL/dR (= the forces when gE is ones)
};

// block-diagonal lists with <= 32 atoms per group (everything else runs the general driver)
bool spk_schnet_mol_eligible(const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb);
bool spk_schnet_mol_bwd_eligible(const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb);
int spk_schnet_mol_bwd_records_mode();      // spk_schnet_mol_set_bwd_records()
// the records region inside `saved` (defined in spk_schnet.hip; one predicate for the sizing function and both launchers)
bool spk_schnet_mol_records_region(const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb, int64_t* off, int64_t* floats);
// split-precision LDS image of filter_network.1.weight [128, 128]
int spk_schnet_mol_pack_w2(const float* w2, float* image, hipStream_t stream);

int spk_schnet_mol_forward(const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb, const SpkPackTable& ptab,
                           const float* x0, const float* r_ij, float* x_out, float* saved, int64_t gsz, hipStream_t stream);
int spk_schnet_mol_backward(const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb, const SpkPackTable& ptab,
                            const float* gx_out, const float* r_ij, const float* saved, int64_t gsz, float* gr, float* gx0,
                            hipStream_t stream);
int spk_schnet_mol_forward_ex(const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb, const SpkPackTable& ptab,
                              const float* x0, const float* r_ij, const float* R, const float* offsets, const MolHeadDev* head, float* x_out,
                              float* saved, int64_t gsz, hipStream_t stream, const float* emb = nullptr, const int64_t* Z = nullptr, int n_types = 0);
int spk_schnet_mol_backward_ex(const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb, const SpkPackTable& ptab,
                               const float* gx_out, const float* r_ij, const float* R, const float* offsets, const MolHeadDev* head,
                               const float* saved, int64_t gsz, float* gr, float* gR, float* gx0, hipStream_t stream);
// The force call of the standard potential (forward, then backward with dL/dE = 1) in ONE launch: k_schnet_mol_force.
int spk_schnet_mol_force_launches();        // spk_schnet_mol_set_force_launches(): 0 = automatic, 1 = one launch, 2 = two launches
bool spk_schnet_mol_force_eligible(const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb, int64_t gsz);
int spk_schnet_mol_force_ex(const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb, const SpkPackTable& ptab, const float* x0,
                            const float* R, const float* offsets, const MolHeadDev* head, float* x_out, float* saved, int64_t gsz, float* gr,
                            float* gR, hipStream_t stream, const float* emb = nullptr, const int64_t* Z = nullptr, int n_types = 0);
