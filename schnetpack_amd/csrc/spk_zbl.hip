// Ziegler-Biersack-Littmark nuclear repulsion (atomistic/nuclear_repulsion.py:70-108), the reference's formula:
//   a_z = z^p,  a_ij = (a_zi + a_zj) s,  phi(d) = sum_k c_k exp(-a_ij alpha_k d),  e(d) = z_i z_j phi(d) f_c(d) / d,
//   E_atom[i] = 1/2 ke sum_{j in row i} e(d_ij),  E[m] = sum_{i in m} E_atom[i].
// The kernels take the EFFECTIVE parameters (after softplus / L1 normalisation) as 12 floats in device memory
//   prm = ke, cutoff (0: no cutoff function), p, s, alpha[4], c[4]
// so that a replayed HIP graph sees parameters the host has refreshed.  f_c is the cosine cutoff with the term's own radius; pairs at or beyond
// it contribute exact zeros.  Accurate expf / sincosf / division throughout: the energies span eight orders of magnitude between 0.3 A and the
// cutoff and the parity contract is relative.
//
//   k_zbl_row    16 lanes per atom walk the atom's CSR row (sorted lists), a_z from a 128-entry table built once per workgroup in LDS (one powf
//                each, none per edge); the lanes meet by fixed shuffles.  From r_ij it writes E_atom (forward); from R / offsets it also ADDS
//                F_i += ke sum_row e'(d) r/d (both directed edges of a pair carry half of e, e is symmetric: no transposed sum, no atomics) and
//                the row's virial 1/2 ke sum_row e'(d)/d r r^T.
//   k_zbl_edge   one lane per directed edge: e (forward of lists that are not sorted) or gr = gE[m] 1/2 ke e'(d) r/d (backward; lands on the
//                atoms through spk_pairwise_bwd_graph_f32 and on the virial through spk_edge_virial_f32).
//   k_zbl_chunk / k_zbl_mol   per-molecule sums of the per-atom rows as in spk_virial.hip (idx_m ascending, chunks of 64 atoms, one wave per
//                molecule): no float atomics, the same list gives the same bits on every call.
#include <math.h>
#include "spk_common.h"

namespace {

constexpr int kZblTable = 128;   // atomic numbers [0, 128): beyond it the outputs of the atom are NaN
constexpr int kZblLanes = 16;
constexpr int kZblChunk = 64;

inline size_t zbl_align(size_t b) { return (b + 255) & ~(size_t)255; }

struct ZblPrm { float ke, rc, p, s, al[4], c[4]; };

__device__ __forceinline__ ZblPrm zbl_load(const float* __restrict__ prm) {
  ZblPrm q;
  q.ke = prm[0]; q.rc = prm[1]; q.p = prm[2]; q.s = prm[3];
#pragma unroll
  for (int k = 0; k < 4; ++k) { q.al[k] = prm[4 + k]; q.c[k] = prm[8 + k]; }
  return q;
}

__device__ __forceinline__ void zbl_table(float* az, float p) {
  for (int t = threadIdx.x; t < kZblTable; t += blockDim.x) az[t] = t == 0 ? 0.f : powf((float)t, p);
  __syncthreads();
}

// e(d) and e'(d) of one directed pair; zz = z_i z_j, asum = a_zi + a_zj
__device__ __forceinline__ void zbl_pair(const ZblPrm& q, float zz, float asum, float d, float& e, float& de) {
  e = 0.f; de = 0.f;
  if (zz == 0.f || (q.rc > 0.f && !(d < q.rc))) return;       // pad atoms and skin pairs: exact zeros
  const float a = asum * q.s;
  float phi = 0.f, dphi = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float ak = a * q.al[k];
    const float t = q.c[k] * expf(-ak * d);
    phi += t;
    dphi -= ak * t;
  }
  float fc = 1.f, dfc = 0.f;
  if (q.rc > 0.f) spk_cutoff_eval(q.rc, d, fc, dfc);
  const float inv = 1.0f / d;
  const float pf = phi * fc;
  e = zz * pf * inv;
  de = zz * ((dphi * fc + phi * dfc) - pf * inv) * inv;
}

// FROM_R = false: r_ij given, writes A[K a] = E_atom only.  FROM_R = true: pair vectors from R / offsets, F += ..., and with K == 10 the row's
// virial into A[K a + 1 .. 9].
template <bool FROM_R, int K>
__global__ __launch_bounds__(256) void k_zbl_row(const float* __restrict__ rij, const float* __restrict__ R, const float* __restrict__ off,
                                                 const int64_t* __restrict__ Z, const int64_t* __restrict__ idx_j,
                                                 const int32_t* __restrict__ rowptr, int64_t N, const float* __restrict__ prm,
                                                 float* __restrict__ A, float* __restrict__ F) {
  __shared__ float az[kZblTable];
  const ZblPrm q = zbl_load(prm);
  zbl_table(az, q.p);
  const int sub = threadIdx.x & (kZblLanes - 1);
  const float nan = __int_as_float(0x7fc00000);
  for (int64_t a = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kZblLanes; a < N; a += ((int64_t)gridDim.x * blockDim.x) / kZblLanes) {
    const int e0 = rowptr[a], e1 = rowptr[a + 1];
    const int64_t zi = Z[a];
    const bool bad_i = zi < 0 || zi >= kZblTable;
    const float fzi = bad_i ? 0.f : (float)zi, azi = bad_i ? 0.f : az[zi];
    float xi = 0.f, yi = 0.f, zc = 0.f;
    if (FROM_R) { xi = R[3 * a]; yi = R[3 * a + 1]; zc = R[3 * a + 2]; }
    float es = 0.f, f[3] = {0.f, 0.f, 0.f}, w[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int e = e0 + sub; e < e1; e += kZblLanes) {
      int64_t j = idx_j[e];
      j = j < 0 ? 0 : (j >= N ? N - 1 : j);          // a malformed list must not read out of bounds (the plan reports it)
      const int64_t zj = Z[j];
      const bool bad_j = zj < 0 || zj >= kZblTable;
      float x, y, z;
      if (FROM_R) {
        x = R[3 * j] - xi; y = R[3 * j + 1] - yi; z = R[3 * j + 2] - zc;
        if (off) { x += off[3 * (int64_t)e]; y += off[3 * (int64_t)e + 1]; z += off[3 * (int64_t)e + 2]; }
      } else {
        x = rij[3 * (int64_t)e]; y = rij[3 * (int64_t)e + 1]; z = rij[3 * (int64_t)e + 2];
      }
      const float d = sqrtf(x * x + y * y + z * z);
      float ee, de;
      zbl_pair(q, bad_j ? 1.f : fzi * (float)zj, azi + (bad_j ? 0.f : az[zj]), d, ee, de);
      if (bad_j) { ee = nan; de = nan; }
      es += ee;
      if (FROM_R) {
        const float g = (de == 0.f) ? 0.f : de / d;   // e'(d) / d  (pad atoms stacked on one point: 0 / 0 must stay an exact zero)
        f[0] += g * x; f[1] += g * y; f[2] += g * z;
        if (K == 10) {
          w[0] += g * x * x; w[1] += g * x * y; w[2] += g * x * z;
          w[3] += g * y * y; w[4] += g * y * z; w[5] += g * z * z;
        }
      }
    }
#pragma unroll
    for (int m = kZblLanes / 2; m >= 1; m >>= 1) {
      es += __shfl_xor(es, m, 64);
      if (FROM_R) {
#pragma unroll
        for (int k = 0; k < 3; ++k) f[k] += __shfl_xor(f[k], m, 64);
        if (K == 10) {
#pragma unroll
          for (int k = 0; k < 6; ++k) w[k] += __shfl_xor(w[k], m, 64);
        }
      }
    }
    if (sub == 0) {
      const float h = 0.5f * q.ke;
      A[(int64_t)K * a] = bad_i ? nan : h * es;
      if (FROM_R) {
        if (bad_i) { F[3 * a] = nan; F[3 * a + 1] = nan; F[3 * a + 2] = nan; }
        else if (e1 > e0) { F[3 * a] += q.ke * f[0]; F[3 * a + 1] += q.ke * f[1]; F[3 * a + 2] += q.ke * f[2]; }   // (an empty row leaves F untouched)
        if (K == 10) {
          float* o = A + (int64_t)K * a + 1;
          const float s = bad_i ? nan : h;
          o[0] = s * w[0]; o[1] = s * w[1]; o[2] = s * w[2];
          o[3] = s * w[1]; o[4] = s * w[3]; o[5] = s * w[4];
          o[6] = s * w[2]; o[7] = s * w[4]; o[8] = s * w[5];
        }
      }
    }
  }
}

// gE == NULL: ee[e] = 1/2 ke e(d_e) (the forward of lists without row pointers); else gr[e] = gE[idx_m[i]] 1/2 ke e'(d_e) r_e / d_e
__global__ __launch_bounds__(256) void k_zbl_edge(const float* __restrict__ rij, const int64_t* __restrict__ Z, const int64_t* __restrict__ idx_i,
                                                  const int64_t* __restrict__ idx_j, const int64_t* __restrict__ idx_m, const float* __restrict__ gE,
                                                  int64_t E, int64_t N, int64_t n_mol, const float* __restrict__ prm, float* __restrict__ out) {
  __shared__ float az[kZblTable];
  const ZblPrm q = zbl_load(prm);
  zbl_table(az, q.p);
  const float nan = __int_as_float(0x7fc00000);
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    int64_t i = idx_i[e], j = idx_j[e];
    i = i < 0 ? 0 : (i >= N ? N - 1 : i);
    j = j < 0 ? 0 : (j >= N ? N - 1 : j);
    const int64_t zi = Z[i], zj = Z[j];
    const bool bad = zi < 0 || zi >= kZblTable || zj < 0 || zj >= kZblTable;
    const float x = rij[3 * e], y = rij[3 * e + 1], z = rij[3 * e + 2];
    const float d = sqrtf(x * x + y * y + z * z);
    float ee = nan, de = nan;
    if (!bad) zbl_pair(q, (float)zi * (float)zj, az[zi] + az[zj], d, ee, de);
    const float h = 0.5f * q.ke;
    if (!gE) { out[e] = h * ee; continue; }
    const int64_t m = idx_m[i];
    const float gm = (m >= 0 && m < n_mol) ? gE[m] : nan;
    const float g = (de == 0.f) ? 0.f : gm * h * de / d;     // (skin / pad pairs: exact zeros whatever the incoming gradient)
    out[3 * e] = g * x; out[3 * e + 1] = g * y; out[3 * e + 2] = g * z;
  }
}

// P[K a ..] = sum of the rows A of the atoms a .. of a's molecule inside a's chunk, for every atom a that starts such a segment
template <int K>
__global__ __launch_bounds__(256) void k_zbl_chunk(const float* __restrict__ A, const int64_t* __restrict__ idx_m, int64_t N, float* __restrict__ P) {
  const int64_t a = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (a >= N) return;
  const int64_t m = idx_m[a];
  if ((a % kZblChunk) != 0 && idx_m[a - 1] == m) return;
  const int64_t end = ((a / kZblChunk + 1) * kZblChunk < N) ? (a / kZblChunk + 1) * kZblChunk : N;
  float s[K];
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = A[K * a + k];
  for (int64_t b = a + 1; b < end && idx_m[b] == m; ++b) {
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] += A[K * b + k];
  }
#pragma unroll
  for (int k = 0; k < K; ++k) P[K * a + k] = s[k];
}

// one wave per molecule: E[m] = sum of the chunk partials (column 0), W[m] += columns 1 .. 9
template <int K>
__global__ __launch_bounds__(256) void k_zbl_mol(const float* __restrict__ P, const int32_t* __restrict__ molptr, int64_t n_mol,
                                                 float* __restrict__ Eo, float* __restrict__ W) {
  const int lane = threadIdx.x & 63;
  const int64_t m = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  if (m >= n_mol) return;                            // uniform over the wave
  const int64_t a0 = molptr[m], a1 = molptr[m + 1];
  float s[K];
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = 0.f;
  if (a1 > a0) {
    const int64_t c0 = a0 / kZblChunk, c1 = (a1 - 1) / kZblChunk;
    for (int64_t c = c0 + lane; c <= c1; c += 64) {
      const int64_t p = (c * kZblChunk > a0) ? c * kZblChunk : a0;
#pragma unroll
      for (int k = 0; k < K; ++k) s[k] += P[K * p + k];
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] += __shfl_xor(s[k], d, 64);
  }
  if (lane == 0) {
    Eo[m] = s[0];
    if (K == 10) {
#pragma unroll
      for (int k = 0; k < 9; ++k) W[9 * m + k] += s[1 + k];
    }
  }
}

struct ZblWs { int32_t* molptr; float* A; float* P; float* ee; size_t bytes; };

ZblWs zbl_ws(char* base, int64_t N, int64_t E, int64_t n_mol) {
  ZblWs w;
  size_t o = 0;
  const size_t rows = zbl_align((size_t)(N > 0 ? N : 1) * 10 * 4);
  w.molptr = (int32_t*)(base ? base + o : nullptr); o += zbl_align((size_t)(n_mol + 1) * 4);
  w.A = (float*)(base ? base + o : nullptr); o += rows;
  w.P = (float*)(base ? base + o : nullptr); o += rows;
  w.ee = (float*)(base ? base + o : nullptr); o += zbl_align((size_t)(E > 0 ? E : 1) * 4);
  w.bytes = o;
  return w;
}

int zbl_check(const char* who, const spk_graph_t* g, int64_t n_mol) {
  SPK_CHECK_ARG(g != nullptr && g->n_atoms >= 0 && g->n_edges >= 0 && n_mol >= 0, "%s: bad graph", who);
  SPK_CHECK_ARG(g->n_atoms < (1LL << 31) - 2 && g->n_edges < (1LL << 31), "%s: list too large for 32-bit row pointers", who);
  return SPK_OK;
}

template <int K>
int zbl_reduce(const float* A, const int64_t* idx_m, int64_t N, int64_t n_mol, const ZblWs& w, float* Eo, float* W, hipStream_t stream) {
  if (N > 0) {
    hipLaunchKernelGGL((k_zbl_chunk<K>), dim3(spk_grid_for(N, 256, 1 << 30)), dim3(256), 0, stream, A, idx_m, N, w.P);
    SPK_LAUNCH_CHECK();
  }
  if (n_mol == 0) return SPK_OK;
  SPK_TRY(spk_segment_rowptr_i32(idx_m, N, n_mol, w.molptr, nullptr, stream));
  hipLaunchKernelGGL((k_zbl_mol<K>), dim3(spk_grid_for(n_mol * 64, 256, 1 << 30)), dim3(256), 0, stream, w.P, w.molptr, n_mol, Eo, W);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

}  // namespace

extern "C" int64_t spk_zbl_workspace_bytes(const spk_graph_t* g, int64_t n_mol) {
  if (!g || g->n_atoms < 0 || g->n_edges < 0 || n_mol < 0) return -1;
  return (int64_t)zbl_ws(nullptr, g->n_atoms, g->n_edges, n_mol).bytes;
}

extern "C" int spk_zbl_fwd_f32(const float* r_ij, const int64_t* Z, const spk_graph_t* g, const int64_t* idx_m, int64_t n_mol, const float* params,
                               float* E, float* E_atom, void* workspace, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "spk_zbl_fwd_f32";
  SPK_TRY(zbl_check(who, g, n_mol));
  const int64_t N = g->n_atoms, Ne = g->n_edges;
  SPK_CHECK_ARG(params && workspace && (n_mol == 0 || E) && (N == 0 || (E_atom && Z && idx_m)), "%s: null argument", who);
  SPK_CHECK_ARG(Ne == 0 || (r_ij && g->idx_i && g->idx_j), "%s: null pair vectors / list", who);
  ZblWs w = zbl_ws((char*)workspace, N, Ne, n_mol);
  if (Ne == 0) {                                     // no pairs: zeros (the plan of an empty list carries no row pointers)
    if (N > 0) SPK_TRY(spk_zero_async(E_atom, (size_t)N * 4, stream));
    return n_mol > 0 ? spk_zero_async(E, (size_t)n_mol * 4, stream) : SPK_OK;
  }
  if (N > 0) {
    SpkProfScope prof("zbl_fwd", stream);
    if (g->sorted && g->rowptr) {
      hipLaunchKernelGGL((k_zbl_row<false, 1>), dim3(spk_grid_for(N * kZblLanes, 256, spk_num_cus() * 16)), dim3(256), 0, stream,
                         r_ij, (const float*)nullptr, (const float*)nullptr, Z, g->idx_j, g->rowptr, N, params, E_atom, (float*)nullptr);
      SPK_LAUNCH_CHECK();
    } else {                                         // no row pointers: per-edge energies, landed by the library's scatter
      if (Ne > 0) {
        hipLaunchKernelGGL(k_zbl_edge, dim3(spk_grid_for(Ne, 256, spk_num_cus() * 16)), dim3(256), 0, stream, r_ij, Z, g->idx_i, g->idx_j, idx_m,
                           (const float*)nullptr, Ne, N, n_mol, params, w.ee);
        SPK_LAUNCH_CHECK();
      }
      SPK_TRY(spk_scatter_add_f32(w.ee, g->idx_i, nullptr, 1, Ne, 1, N, E_atom, stream));
    }
  }
  return zbl_reduce<1>(E_atom, idx_m, N, n_mol, w, E, nullptr, stream);
}

extern "C" int spk_zbl_bwd_f32(const float* gE, const float* r_ij, const int64_t* Z, const spk_graph_t* g, const int64_t* idx_m, int64_t n_mol,
                               const float* params, float* gr, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "spk_zbl_bwd_f32";
  SPK_TRY(zbl_check(who, g, n_mol));
  const int64_t N = g->n_atoms, Ne = g->n_edges;
  if (Ne == 0) return SPK_OK;
  SPK_CHECK_ARG(N > 0 && gE && r_ij && Z && idx_m && params && gr && g->idx_i && g->idx_j, "%s: null argument", who);
  SpkProfScope prof("zbl_bwd", stream);
  hipLaunchKernelGGL(k_zbl_edge, dim3(spk_grid_for(Ne, 256, spk_num_cus() * 16)), dim3(256), 0, stream, r_ij, Z, g->idx_i, g->idx_j, idx_m, gE, Ne, N,
                     n_mol, params, gr);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" int spk_zbl_forces_f32(const float* R, const float* offsets, const int64_t* Z, const spk_graph_t* g, const int64_t* idx_m, int64_t n_mol,
                                  const float* params, float* E_zbl, float* F, float* W, void* workspace, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "spk_zbl_forces_f32";
  SPK_TRY(zbl_check(who, g, n_mol));
  const int64_t N = g->n_atoms, Ne = g->n_edges;
  SPK_CHECK_ARG(Ne == 0 || (g->sorted && g->rowptr && g->symmetric && g->idx_j),
                "%s: the row pass needs a sorted, symmetric list (other lists: spk_zbl_bwd_f32 + spk_pairwise_bwd_graph_f32 / spk_edge_virial_f32)", who);
  SPK_CHECK_ARG(params && workspace && (n_mol == 0 || E_zbl) && (N == 0 || (R && Z && idx_m && F && g->rowptr)), "%s: null argument", who);
  ZblWs w = zbl_ws((char*)workspace, N, Ne, n_mol);
  if (Ne == 0) return n_mol > 0 ? spk_zero_async(E_zbl, (size_t)n_mol * 4, stream) : SPK_OK;      // no pairs: F and W stay as they are
  if (N > 0) {
    SpkProfScope prof("zbl_forces", stream);
    const dim3 grid(spk_grid_for(N * kZblLanes, 256, spk_num_cus() * 16));
    if (W) hipLaunchKernelGGL((k_zbl_row<true, 10>), grid, dim3(256), 0, stream, (const float*)nullptr, R, offsets, Z, g->idx_j, g->rowptr, N, params, w.A, F);
    else hipLaunchKernelGGL((k_zbl_row<true, 1>), grid, dim3(256), 0, stream, (const float*)nullptr, R, offsets, Z, g->idx_j, g->rowptr, N, params, w.A, F);
    SPK_LAUNCH_CHECK();
  }
  return W ? zbl_reduce<10>(w.A, idx_m, N, n_mol, w, E_zbl, W, stream) : zbl_reduce<1>(w.A, idx_m, N, n_mol, w, E_zbl, nullptr, stream);
}
