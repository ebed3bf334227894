// Virial of a pair potential from the per-edge gradient g_e = dE/dr_e (atomistic/response.py:434-464, Strain + Forces(calc_stress)).
//
// The reference strains R, offsets and cell by S^T (row vectors), so every pair vector becomes r_e (1 + S^T) and
//   dE/dS [m] = sum over the edges e of molecule m of  g_e r_e^T          (3 x 3, g as the row index),
// which this file calls the virial W[m] (energy units; stress = W / V is formed by the caller).  Three launches, no float atomics,
// no host synchronisation (a HIP-graph capture takes the call as it is), results bit-identical run to run on the same list:
//   k_edge_virial_row   16 lanes per atom walk the atom's CSR row (the plan's rowptr on lists sorted by idx_i, else a stable by-centre
//                       permutation built on the device by spk_transpose_plan); r_e is recomputed from R, idx_j and offsets with the
//                       arithmetic of k_pairwise ((R[j] - R[i]) + offsets, fp32); the lanes meet by fixed shuffles -> W_i [N, 9]
//   k_virial_chunk      atoms in chunks of 64: the first atom of every (chunk, molecule) segment sums the segment in atom order -> P
//   k_virial_mol        one wave per molecule: lane l sums the molecule's chunk partials l, l + 64, ... in order, then a fixed
//                       butterfly -> W [n_mol, 9].  A molecule of 32 k atoms (a periodic box) is 500 partials, not one serial loop.
#include "spk_common.h"

namespace {

constexpr int kVirChunk = 64;
constexpr int kVirLanes = 16;

inline size_t vir_align(size_t b) { return (b + 255) & ~(size_t)255; }

__global__ __launch_bounds__(256) void k_edge_virial_row(const float* __restrict__ gr, const float* __restrict__ R, const float* __restrict__ off,
                                                         const int64_t* __restrict__ idx_j, const int32_t* __restrict__ rowptr,
                                                         const int32_t* __restrict__ perm, int64_t N, float* __restrict__ Wa) {
  const int sub = threadIdx.x & (kVirLanes - 1);
  for (int64_t a = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kVirLanes; a < N; a += ((int64_t)gridDim.x * blockDim.x) / kVirLanes) {
    const int e0 = rowptr[a], e1 = rowptr[a + 1];
    const float xi = R[3 * a], yi = R[3 * a + 1], zi = R[3 * a + 2];
    float w[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) w[k] = 0.f;
    for (int k = e0 + sub; k < e1; k += kVirLanes) {
      const int64_t e = perm ? (int64_t)perm[k] : (int64_t)k;
      int64_t j = idx_j[e];
      j = j < 0 ? 0 : (j >= N ? N - 1 : j);          // a malformed list must not read out of bounds (the plan reports it)
      float x = R[3 * j] - xi, y = R[3 * j + 1] - yi, z = R[3 * j + 2] - zi;
      if (off) { x += off[3 * e]; y += off[3 * e + 1]; z += off[3 * e + 2]; }
      const float gx = gr[3 * e], gy = gr[3 * e + 1], gz = gr[3 * e + 2];
      w[0] += gx * x; w[1] += gx * y; w[2] += gx * z;
      w[3] += gy * x; w[4] += gy * y; w[5] += gy * z;
      w[6] += gz * x; w[7] += gz * y; w[8] += gz * z;
    }
#pragma unroll
    for (int m = kVirLanes / 2; m >= 1; m >>= 1) {
#pragma unroll
      for (int k = 0; k < 9; ++k) w[k] += __shfl_xor(w[k], m, 64);
    }
    if (sub == 0) {
#pragma unroll
      for (int k = 0; k < 9; ++k) Wa[9 * a + k] = w[k];
    }
  }
}

// P[a] = sum of W_i over the atoms a .. of a's molecule inside a's chunk, for every atom a that starts such a segment
__global__ __launch_bounds__(256) void k_virial_chunk(const float* __restrict__ Wa, const int64_t* __restrict__ idx_m, int64_t N,
                                                      float* __restrict__ P) {
  const int64_t a = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (a >= N) return;
  const int64_t m = idx_m[a];
  if ((a % kVirChunk) != 0 && idx_m[a - 1] == m) return;
  const int64_t end = ((a / kVirChunk + 1) * kVirChunk < N) ? (a / kVirChunk + 1) * kVirChunk : N;
  float s[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) s[k] = Wa[9 * a + k];
  for (int64_t b = a + 1; b < end && idx_m[b] == m; ++b) {
#pragma unroll
    for (int k = 0; k < 9; ++k) s[k] += Wa[9 * b + k];
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) P[9 * a + k] = s[k];
}

// W[m] = sum over the chunks c the molecule's atoms [a0, a1) touch of P[max(a0, 64 c)]; one wave per molecule
__global__ __launch_bounds__(256) void k_virial_mol(const float* __restrict__ P, const int32_t* __restrict__ molptr, int64_t n_mol,
                                                    float* __restrict__ W) {
  const int lane = threadIdx.x & 63;
  const int64_t m = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  if (m >= n_mol) return;                            // uniform over the wave
  const int64_t a0 = molptr[m], a1 = molptr[m + 1];
  float s[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) s[k] = 0.f;
  if (a1 > a0) {
    const int64_t c0 = a0 / kVirChunk, c1 = (a1 - 1) / kVirChunk;
    for (int64_t c = c0 + lane; c <= c1; c += 64) {
      const int64_t p = (c * kVirChunk > a0) ? c * kVirChunk : a0;
#pragma unroll
      for (int k = 0; k < 9; ++k) s[k] += P[9 * p + k];
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
    for (int k = 0; k < 9; ++k) s[k] += __shfl_xor(s[k], d, 64);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) W[9 * m + k] = s[k];
  }
}

struct VirialWs {
  int32_t* molptr; float* P; float* Wa; int32_t* rowptr; int32_t* perm; void* sort_tmp;
  size_t bytes;
};

VirialWs virial_ws(char* base, const spk_graph_t* g, int64_t n_mol, bool own_wa) {
  const int64_t N = g->n_atoms, E = g->n_edges;
  const bool by_centre = !(g->sorted && g->rowptr);
  VirialWs w;
  size_t o = 0;
  w.molptr = (int32_t*)(base ? base + o : nullptr); o += vir_align((size_t)(n_mol + 1) * 4);
  w.P = (float*)(base ? base + o : nullptr); o += vir_align((size_t)(N > 0 ? N : 1) * 9 * 4);
  w.Wa = nullptr;
  if (own_wa) { w.Wa = (float*)(base ? base + o : nullptr); o += vir_align((size_t)(N > 0 ? N : 1) * 9 * 4); }
  w.rowptr = nullptr; w.perm = nullptr; w.sort_tmp = nullptr;
  if (by_centre) {
    w.rowptr = (int32_t*)(base ? base + o : nullptr); o += vir_align((size_t)(N + 2) * 4);    // (spk_transpose_plan: N + 2 entries)
    w.perm = (int32_t*)(base ? base + o : nullptr); o += vir_align((size_t)(E > 0 ? E : 1) * 4);
    w.sort_tmp = base ? base + o : nullptr; o += vir_align((size_t)spk_transpose_plan_bytes(E, N));
  }
  w.bytes = o;
  return w;
}

}  // namespace

extern "C" int64_t spk_edge_virial_workspace_bytes(const spk_graph_t* g, int64_t n_mol, int32_t with_atom_virial) {
  if (!g || g->n_atoms < 0 || g->n_edges < 0 || n_mol < 0) return -1;
  return (int64_t)virial_ws(nullptr, g, n_mol, with_atom_virial == 0).bytes;
}

extern "C" int spk_edge_virial_f32(const float* gr, const float* R, const float* offsets, const spk_graph_t* g, const int64_t* idx_m,
                                   int64_t n_mol, float* W, float* W_atom, void* workspace, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "spk_edge_virial_f32";
  SPK_CHECK_ARG(g != nullptr && g->n_atoms >= 0 && g->n_edges >= 0 && n_mol >= 0, "%s: bad graph", who);
  const int64_t N = g->n_atoms, E = g->n_edges;
  SPK_CHECK_ARG(N < (1LL << 31) - 2 && E < (1LL << 31), "%s: list too large for 32-bit row pointers", who);
  SPK_CHECK_ARG((n_mol == 0 || W) && workspace, "%s: null output / workspace", who);
  SPK_CHECK_ARG(N == 0 || (R && idx_m), "%s: null positions / molecule index", who);
  SPK_CHECK_ARG(E == 0 || (gr && g->idx_i && g->idx_j), "%s: null edge gradient / list", who);
  VirialWs w = virial_ws((char*)workspace, g, n_mol, W_atom == nullptr);
  float* Wa = W_atom ? W_atom : w.Wa;
  if (N > 0) {
    const int32_t* rowptr = g->rowptr;
    const int32_t* perm = nullptr;
    if (!(g->sorted && g->rowptr)) {               // by-centre order of an unsorted list: stable radix sort of idx_i (same order on every call)
      SPK_TRY(spk_transpose_plan(g->idx_i, E, N, w.rowptr, w.perm, w.sort_tmp, stream));
      rowptr = w.rowptr; perm = w.perm;
    }
    SpkProfScope prof("edge_virial", stream);
    hipLaunchKernelGGL(k_edge_virial_row, dim3(spk_grid_for(N * kVirLanes, 256, spk_num_cus() * 16)), dim3(256), 0, stream,
                       gr, R, offsets, g->idx_j, rowptr, perm, N, Wa);
    SPK_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_virial_chunk, dim3(spk_grid_for(N, 256, 1 << 30)), dim3(256), 0, stream, Wa, idx_m, N, w.P);
    SPK_LAUNCH_CHECK();
  }
  if (n_mol == 0) return SPK_OK;
  SPK_TRY(spk_segment_rowptr_i32(idx_m, N, n_mol, w.molptr, nullptr, stream));
  SpkProfScope prof("virial_mol", stream);
  hipLaunchKernelGGL(k_virial_mol, dim3(spk_grid_for(n_mol * 64, 256, 1 << 30)), dim3(256), 0, stream, w.P, w.molptr, n_mol, W);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}
