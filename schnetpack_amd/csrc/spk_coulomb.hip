// Point-charge electrostatics over a neighbour list (atomistic/electrostatic.py:14-152 and the real-space part of :266-308), the reference's
// formula:
//   phi_i = sum_{j in row i} q_j v(d_ij),   E_atom[i] = 1/2 ke q_i phi_i,   E[m] = sum_{i in m} E_atom[i].
// The pair function chi(d) is selected by 8 floats in device memory (a replayed HIP graph sees what the host last wrote there)
//   prm = ke, kind, rc (0: no cutoff), shift, switch_on, switch_off, alpha, screened (0 / 1)
//   kind 0   chi = 1/d                                                       (CoulombPotential)
//   kind 1   chi = s(d) / sqrt(d^2 + 1) + (1 - s(d)) / d                     (DampedCoulombPotential with SwitchFunction)
//   kind 2   chi = erfc(sqrt(alpha) d) / d, times (1 - s(d)) when screened   (EnergyEwald._real_space)
// with the switch s = 1 / (1 + exp(u)), u = 1/(1 - x) - 1/x, x = (d - on) / (off - on), exactly 1 at x <= 0 and exactly 0 at x >= 1.  With
// rc > 0 (kinds 0 and 1) v = chi + shift^2/chi - 2 shift for d <= rc, computed as (chi - shift)^2 / chi (the three-term form cancels near the
// cutoff in float32), and exactly 0 beyond; otherwise v = chi.  Accurate expf / erfcf / division throughout: the parity contract is relative.
//
//   k_coul_row    16 lanes per atom walk the atom's CSR row (sorted lists), the lanes meet by fixed shuffles: phi_i and E_atom[i].
//   k_coul_edge   one lane per directed edge.  MODE 0: q_j v(d) (forward of lists without row pointers, landed by the library's scatter);
//                 MODE 1: gr[e] = gE[m] 1/2 ke q_i q_j v'(d) r/d, and, when asked, the two per-edge shares of dE/dq
//                 (gE[m] 1/2 ke q_j v for atom i, gE[m] 1/2 ke q_i v for atom j) that the library's scatter lands over idx_i and idx_j.
//   k_coul_atom   E_atom from phi (edge route of the forward) or gq[i] = gE[m] ke phi_i (sorted symmetric lists: no second pass over the pairs).
//   k_coul_chunk / k_coul_mol   per-molecule sums as in spk_zbl.hip / spk_virial.hip (idx_m ascending, chunks of 64 atoms, one wave per
//                 molecule): no float atomics, the same list gives the same bits on every call.
// Pairs with q_i q_j = 0 (pad atoms, also stacked on one point) give exact zeros; indices outside the atoms are clamped for the read.
#include <math.h>
#include "spk_common.h"

namespace {

constexpr int kCoulLanes = 16;
constexpr int kCoulChunk = 64;

inline size_t coul_align(size_t b) { return (b + 255) & ~(size_t)255; }

struct CoulPrm { float ke, rc, shift, on, off, alpha; int kind, screened; };

__device__ __forceinline__ CoulPrm coul_load(const float* __restrict__ prm) {
  CoulPrm p;
  p.ke = prm[0]; p.kind = (int)prm[1]; p.rc = prm[2]; p.shift = prm[3]; p.on = prm[4]; p.off = prm[5]; p.alpha = prm[6]; p.screened = prm[7] != 0.f;
  return p;
}

// s(d) and ds/dd; the ends are exact and no inf - inf / 0 * inf appears
__device__ __forceinline__ void coul_switch(const CoulPrm& p, float d, float& s, float& ds) {
  const float w = p.off - p.on;
  const float x = (d - p.on) / w;
  ds = 0.f;
  if (!(x > 0.f)) { s = 1.f; return; }
  if (!(x < 1.f)) { s = 0.f; return; }
  const float ix = 1.0f / x, iy = 1.0f / (1.0f - x);
  const float e = expf(iy - ix);
  if (e == 0.f) { s = 1.f; return; }
  if (e > 1e30f) { s = 0.f; return; }
  s = 1.0f / (1.0f + e);
  ds = -(s * (e * s)) * (iy * iy + ix * ix) / w;        // s (1 - s) = e / (1 + e)^2
}

// v(d) and v'(d) of one pair
__device__ __forceinline__ void coul_pair(const CoulPrm& p, float d, float& v, float& dv) {
  const float inv = 1.0f / d;
  float chi, dchi;
  if (p.kind == 2) {
    const float a = sqrtf(p.alpha);
    const float ec = erfcf(a * d);
    chi = ec * inv;
    dchi = (-1.1283791670955126f * a * expf(-(a * d) * (a * d)) - chi) * inv;
    if (p.screened) {
      float s, ds;
      coul_switch(p, d, s, ds);
      dchi = dchi * (1.0f - s) - chi * ds;
      chi = chi * (1.0f - s);
    }
    v = chi; dv = dchi;
    return;
  }
  if (p.kind == 1) {
    float s, ds;
    coul_switch(p, d, s, ds);
    const float dm = 1.0f / sqrtf(d * d + 1.0f);
    chi = s * dm + (1.0f - s) * inv;
    dchi = ds * (dm - inv) - s * d * dm * dm * dm - (1.0f - s) * inv * inv;
  } else {
    chi = inv;
    dchi = -inv * inv;
  }
  if (p.rc > 0.f) {
    if (d <= p.rc) {
      const float t = chi - p.shift;
      v = t * t / chi;
      dv = dchi * t * (chi + p.shift) / (chi * chi);
    } else {
      v = 0.f; dv = 0.f;
    }
    return;
  }
  v = chi; dv = dchi;
}

__global__ __launch_bounds__(256) void k_coul_row(const float* __restrict__ rij, const float* __restrict__ q, const int64_t* __restrict__ idx_j,
                                                  const int32_t* __restrict__ rowptr, int64_t N, const float* __restrict__ prm,
                                                  float* __restrict__ Ea, float* __restrict__ phi) {
  const CoulPrm p = coul_load(prm);
  const int sub = threadIdx.x & (kCoulLanes - 1);
  for (int64_t a = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kCoulLanes; a < N; a += ((int64_t)gridDim.x * blockDim.x) / kCoulLanes) {
    const int e0 = rowptr[a], e1 = rowptr[a + 1];
    float ps = 0.f;
    for (int e = e0 + sub; e < e1; e += kCoulLanes) {
      int64_t j = idx_j[e];
      j = j < 0 ? 0 : (j >= N ? N - 1 : j);          // a malformed list must not read out of bounds (the plan reports it)
      const float qj = q[j];
      if (qj == 0.f) continue;                        // pad atoms, also stacked on one point: exact zeros
      const float x = rij[3 * (int64_t)e], y = rij[3 * (int64_t)e + 1], z = rij[3 * (int64_t)e + 2];
      float v, dv;
      coul_pair(p, sqrtf(x * x + y * y + z * z), v, dv);
      ps += qj * v;
    }
#pragma unroll
    for (int m = kCoulLanes / 2; m >= 1; m >>= 1) ps += __shfl_xor(ps, m, 64);
    if (sub == 0) {
      const float qi = q[a];
      phi[a] = ps;
      Ea[a] = qi == 0.f ? 0.f : 0.5f * p.ke * qi * ps;
    }
  }
}

// MODE 0: out[e] = q_j v(d_e).  MODE 1: out[3 e ..] = gr[e]; with ti / tj the per-edge shares of dE/dq of the two atoms.
template <int MODE>
__global__ __launch_bounds__(256) void k_coul_edge(const float* __restrict__ rij, const float* __restrict__ q, const int64_t* __restrict__ idx_i,
                                                   const int64_t* __restrict__ idx_j, const int64_t* __restrict__ idx_m, const float* __restrict__ gE,
                                                   int64_t E, int64_t N, int64_t n_mol, const float* __restrict__ prm, float* __restrict__ out,
                                                   float* __restrict__ ti, float* __restrict__ tj) {
  const CoulPrm p = coul_load(prm);
  const float nan = __int_as_float(0x7fc00000);
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    int64_t i = idx_i[e], j = idx_j[e];
    i = i < 0 ? 0 : (i >= N ? N - 1 : i);
    j = j < 0 ? 0 : (j >= N ? N - 1 : j);
    const float qi = q[i], qj = q[j];
    const float x = rij[3 * e], y = rij[3 * e + 1], z = rij[3 * e + 2];
    const float d = sqrtf(x * x + y * y + z * z);
    float v = 0.f, dv = 0.f;
    if (MODE == 0) {
      if (qj != 0.f) coul_pair(p, d, v, dv);
      out[e] = qj == 0.f ? 0.f : qj * v;
      continue;
    }
    const int64_t m = idx_m[i];
    const float gm = (m >= 0 && m < n_mol) ? gE[m] : nan;
    const float h = 0.5f * p.ke * gm;
    if (qi != 0.f || qj != 0.f) coul_pair(p, d, v, dv);
    const float qq = qi * qj;
    const float g = (qq == 0.f || dv == 0.f) ? 0.f : h * qq * dv / d;     // (pad / beyond-cutoff pairs: exact zeros whatever the incoming gradient)
    out[3 * e] = g * x; out[3 * e + 1] = g * y; out[3 * e + 2] = g * z;
    if (ti) {
      ti[e] = qj == 0.f ? 0.f : h * qj * v;
      tj[e] = qi == 0.f ? 0.f : h * qi * v;
    }
  }
}

// gE == NULL: Ea[i] = 1/2 ke q_i phi_i.  Else out[i] = gE[m] ke phi_i (+ add[i] when given: the edge route's second scatter).
__global__ __launch_bounds__(256) void k_coul_atom(const float* __restrict__ q, const float* __restrict__ phi, const int64_t* __restrict__ idx_m,
                                                   const float* __restrict__ gE, const float* __restrict__ add, int64_t N, int64_t n_mol,
                                                   const float* __restrict__ prm, float* __restrict__ out) {
  const int64_t a = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (a >= N) return;
  const float ke = prm[0];
  if (!gE) { const float qi = q[a]; out[a] = qi == 0.f ? 0.f : 0.5f * ke * qi * phi[a]; return; }
  if (add) { out[a] += add[a]; return; }
  const int64_t m = idx_m[a];
  out[a] = ((m >= 0 && m < n_mol) ? gE[m] : __int_as_float(0x7fc00000)) * ke * phi[a];
}

// P[a] = sum of A over the atoms a .. of a's molecule inside a's chunk, for every atom a that starts such a segment
__global__ __launch_bounds__(256) void k_coul_chunk(const float* __restrict__ A, const int64_t* __restrict__ idx_m, int64_t N, float* __restrict__ P) {
  const int64_t a = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (a >= N) return;
  const int64_t m = idx_m[a];
  if ((a % kCoulChunk) != 0 && idx_m[a - 1] == m) return;
  const int64_t end = ((a / kCoulChunk + 1) * kCoulChunk < N) ? (a / kCoulChunk + 1) * kCoulChunk : N;
  float s = A[a];
  for (int64_t b = a + 1; b < end && idx_m[b] == m; ++b) s += A[b];
  P[a] = s;
}

// one wave per molecule: E[m] = sum of the chunk partials
__global__ __launch_bounds__(256) void k_coul_mol(const float* __restrict__ P, const int32_t* __restrict__ molptr, int64_t n_mol, float* __restrict__ Eo) {
  const int lane = threadIdx.x & 63;
  const int64_t m = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  if (m >= n_mol) return;                            // uniform over the wave
  const int64_t a0 = molptr[m], a1 = molptr[m + 1];
  float s = 0.f;
  if (a1 > a0) {
    const int64_t c0 = a0 / kCoulChunk, c1 = (a1 - 1) / kCoulChunk;
    for (int64_t c = c0 + lane; c <= c1; c += 64) s += P[(c * kCoulChunk > a0) ? c * kCoulChunk : a0];
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
  if (lane == 0) Eo[m] = s;
}

struct CoulWs { int32_t* molptr; float* P; float* ta; float* tb; float* c; size_t bytes; };

CoulWs coul_ws(char* base, int64_t N, int64_t E, int64_t n_mol) {
  CoulWs w;
  size_t o = 0;
  const size_t rows = coul_align((size_t)(N > 0 ? N : 1) * 4), edges = coul_align((size_t)(E > 0 ? E : 1) * 4);
  w.molptr = (int32_t*)(base ? base + o : nullptr); o += coul_align((size_t)(n_mol + 1) * 4);
  w.P = (float*)(base ? base + o : nullptr); o += rows;
  w.c = (float*)(base ? base + o : nullptr); o += rows;
  w.ta = (float*)(base ? base + o : nullptr); o += edges;
  w.tb = (float*)(base ? base + o : nullptr); o += edges;
  w.bytes = o;
  return w;
}

int coul_check(const char* who, const spk_graph_t* g, int64_t n_mol) {
  SPK_CHECK_ARG(g != nullptr && g->n_atoms >= 0 && g->n_edges >= 0 && n_mol >= 0, "%s: bad graph", who);
  SPK_CHECK_ARG(g->n_atoms < (1LL << 31) - 2 && g->n_edges < (1LL << 31), "%s: list too large for 32-bit row pointers", who);
  return SPK_OK;
}

}  // namespace

extern "C" int64_t spk_coulomb_workspace_bytes(const spk_graph_t* g, int64_t n_mol) {
  if (!g || g->n_atoms < 0 || g->n_edges < 0 || n_mol < 0) return -1;
  return (int64_t)coul_ws(nullptr, g->n_atoms, g->n_edges, n_mol).bytes;
}

extern "C" int spk_coulomb_fwd_f32(const float* r_ij, const float* q, const spk_graph_t* g, const int64_t* idx_m, int64_t n_mol, const float* params,
                                   float* E, float* E_atom, float* phi, void* workspace, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "spk_coulomb_fwd_f32";
  SPK_TRY(coul_check(who, g, n_mol));
  const int64_t N = g->n_atoms, Ne = g->n_edges;
  SPK_CHECK_ARG(params && workspace && (n_mol == 0 || E) && (N == 0 || (E_atom && phi && q && idx_m)), "%s: null argument", who);
  SPK_CHECK_ARG(Ne == 0 || (r_ij && g->idx_i && g->idx_j), "%s: null pair vectors / list", who);
  CoulWs w = coul_ws((char*)workspace, N, Ne, n_mol);
  if (Ne == 0 || N == 0) {                           // no pairs: zeros (the plan of an empty list carries no row pointers)
    if (N > 0) { SPK_TRY(spk_zero_async(E_atom, (size_t)N * 4, stream)); SPK_TRY(spk_zero_async(phi, (size_t)N * 4, stream)); }
    return n_mol > 0 ? spk_zero_async(E, (size_t)n_mol * 4, stream) : SPK_OK;
  }
  {
    SpkProfScope prof("coulomb_fwd", stream);
    if (g->sorted && g->rowptr) {
      hipLaunchKernelGGL(k_coul_row, dim3(spk_grid_for(N * kCoulLanes, 256, spk_num_cus() * 16)), dim3(256), 0, stream, r_ij, q, g->idx_j, g->rowptr, N,
                         params, E_atom, phi);
      SPK_LAUNCH_CHECK();
    } else {                                         // no row pointers: per-edge terms, landed by the library's scatter
      hipLaunchKernelGGL((k_coul_edge<0>), dim3(spk_grid_for(Ne, 256, spk_num_cus() * 16)), dim3(256), 0, stream, r_ij, q, g->idx_i, g->idx_j, idx_m,
                         (const float*)nullptr, Ne, N, n_mol, params, w.ta, (float*)nullptr, (float*)nullptr);
      SPK_LAUNCH_CHECK();
      SPK_TRY(spk_scatter_add_f32(w.ta, g->idx_i, nullptr, 1, Ne, 1, N, phi, stream));
      hipLaunchKernelGGL(k_coul_atom, dim3(spk_grid_for(N, 256, 1 << 30)), dim3(256), 0, stream, q, (const float*)phi, idx_m, (const float*)nullptr,
                         (const float*)nullptr, N, n_mol, params, E_atom);
      SPK_LAUNCH_CHECK();
    }
  }
  hipLaunchKernelGGL(k_coul_chunk, dim3(spk_grid_for(N, 256, 1 << 30)), dim3(256), 0, stream, (const float*)E_atom, idx_m, N, w.P);
  SPK_LAUNCH_CHECK();
  if (n_mol == 0) return SPK_OK;
  SPK_TRY(spk_segment_rowptr_i32(idx_m, N, n_mol, w.molptr, nullptr, stream));
  hipLaunchKernelGGL(k_coul_mol, dim3(spk_grid_for(n_mol * 64, 256, 1 << 30)), dim3(256), 0, stream, (const float*)w.P, (const int32_t*)w.molptr, n_mol, E);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" int spk_coulomb_bwd_f32(const float* gE, const float* r_ij, const float* q, const float* phi, const spk_graph_t* g, const int64_t* idx_m,
                                   int64_t n_mol, const float* params, float* gr, float* gq, void* workspace, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "spk_coulomb_bwd_f32";
  SPK_TRY(coul_check(who, g, n_mol));
  const int64_t N = g->n_atoms, Ne = g->n_edges;
  if (N == 0) return SPK_OK;
  SPK_CHECK_ARG(gE && q && idx_m && params && workspace && (gr || gq), "%s: null argument", who);
  if (Ne == 0) return gq ? spk_zero_async(gq, (size_t)N * 4, stream) : SPK_OK;
  SPK_CHECK_ARG(r_ij && g->idx_i && g->idx_j, "%s: null pair vectors / list", who);
  CoulWs w = coul_ws((char*)workspace, N, Ne, n_mol);
  SpkProfScope prof("coulomb_bwd", stream);
  const bool rows = gq && phi && g->sorted && g->rowptr && g->symmetric;      // dE/dq_i = gE[m] ke phi_i: no second pass over the pairs
  const bool edges = gq && !rows;
  if (gr || edges) {
    float* out = gr ? gr : nullptr;
    SPK_CHECK_ARG(out != nullptr, "%s: the edge route of dE/dq needs gr as well", who);
    hipLaunchKernelGGL((k_coul_edge<1>), dim3(spk_grid_for(Ne, 256, spk_num_cus() * 16)), dim3(256), 0, stream, r_ij, q, g->idx_i, g->idx_j, idx_m, gE,
                       Ne, N, n_mol, params, out, edges ? w.ta : (float*)nullptr, edges ? w.tb : (float*)nullptr);
    SPK_LAUNCH_CHECK();
  }
  if (rows) {
    hipLaunchKernelGGL(k_coul_atom, dim3(spk_grid_for(N, 256, 1 << 30)), dim3(256), 0, stream, q, phi, idx_m, gE, (const float*)nullptr, N, n_mol,
                       params, gq);
    SPK_LAUNCH_CHECK();
  } else if (edges) {
    SPK_TRY(spk_scatter_add_f32(w.ta, g->idx_i, (g->sorted && g->rowptr) ? g->rowptr : nullptr, 1, Ne, 1, N, gq, stream));
    SPK_TRY(spk_scatter_add_f32(w.tb, g->idx_j, nullptr, 1, Ne, 1, N, w.c, stream));
    hipLaunchKernelGGL(k_coul_atom, dim3(spk_grid_for(N, 256, 1 << 30)), dim3(256), 0, stream, q, (const float*)nullptr, idx_m, gE, (const float*)w.c, N,
                       n_mol, params, gq);
    SPK_LAUNCH_CHECK();
  }
  return SPK_OK;
}
