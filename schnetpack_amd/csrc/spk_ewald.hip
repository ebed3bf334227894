// Reciprocal-space part of the Ewald sum (atomistic/electrostatic.py:310-375), the reference's formula: per molecule m with cell C, volume
// V = |det C|, k = n 2 pi C^-T for the integer vectors n of `kvecs`, g_k = exp(-k^2 / 4 alpha) / k^2,
//   S(k) = sum_{i in m} q_i e^{i k r_i},   E_rec[m] = ke (2 pi / V sum_k g_k |S(k)|^2 - sqrt(alpha / pi) sum_{i in m} q_i^2).
// In fractional coordinates s_i = r_i C^-1 the phase is k r_i = 2 pi n s_i, so e^{i k r_i} is a product of three factors e^{2 pi i n_a s_a}
// taken from a per-atom table of n = 0 .. k_max (sincospif of 2 n s directly -- no recurrence: atoms may sit outside their cell and the phase
// must stay accurate; negative n by conjugation): two complex multiplies per (atom, k) where the reference takes a sin and a cos and
// materialises [n_atoms, K, 3] tensors.  params: 2 floats in device memory, ke and alpha.  |n_a| <= kEwaldKmax = 8 (17 factors per axis): the
// table of a 64-atom tile is 13.5 KiB of LDS; entries of kvecs beyond it are clamped for the read (the module mirror takes its ATen route).
//
//   k_ewald_cell     one lane per molecule: C^-1, V (a cell without volume -- |det| <= 1e-8, or <= 1e-5 of the product of its edge lengths, i.e.
//                    rounding residue -- gets NaN: the energies and gradients of that molecule become NaN).
//   k_ewald_sfac     grid (k-chunk of 256, slab of 256 atoms): the block stages the tables of 64 atoms at a time in LDS, each lane owns one
//                    k-vector and accumulates S(k) in registers; where the molecule changes inside the slab the partial sum is flushed to
//                    part[slab + m] (idx_m ascending: the id grows with every segment, so every segment has its own).
//   k_ewald_reduce   one block per molecule: S(k) = the partials of the molecule's slabs in ascending order, c_k = g_k S(k) (kept for the
//                    backward), E_rec[m] with a fixed reduction tree over k and over the molecule's atoms (self term).
//   k_ewald_bwd      one wave per atom, lanes over k, the same factors:
//                      dE/dq_i = gE[m] ke (4 pi / V sum_k Re(c_k* e^{i k r_i}) - 2 sqrt(alpha / pi) q_i)
//                      dE/dr_i = -gE[m] ke (4 pi / V) q_i sum_k k Im(c_k* e^{i k r_i})
//                    (d|S|^2/dr_i = 2 Re(S* i k q_i e_i) = -2 k q_i Im(S* e_i)); the sum over k is taken in the integer vectors n and turned into
//                    Cartesian components once per atom.
// No float atomics anywhere: the same input gives the same bits on every call.
#include <math.h>
#include "spk_common.h"

namespace {

constexpr int kEwaldKmax = 8;
constexpr int kEwaldNf = kEwaldKmax + 1;     // factors n = 0 .. k_max per axis
constexpr int kEwaldTile = 64;               // atoms whose tables are staged at a time
constexpr int kEwaldSlab = 256;              // atoms per block of the structure-factor kernel
constexpr int kEwaldCell = 12;               // floats per molecule: C^-1 [9], V, unused [2]
constexpr float kTwoPi = 6.283185307179586f;

inline size_t ew_align(size_t b) { return (b + 255) & ~(size_t)255; }

__global__ __launch_bounds__(256) void k_ewald_cell(const float* __restrict__ cell, int64_t n_mol, float* __restrict__ info) {
  const int64_t m = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (m >= n_mol) return;
  const float* c = cell + 9 * m;
  const float a00 = c[4] * c[8] - c[5] * c[7], a01 = c[2] * c[7] - c[1] * c[8], a02 = c[1] * c[5] - c[2] * c[4];
  const float a10 = c[5] * c[6] - c[3] * c[8], a11 = c[0] * c[8] - c[2] * c[6], a12 = c[2] * c[3] - c[0] * c[5];
  const float a20 = c[3] * c[7] - c[4] * c[6], a21 = c[1] * c[6] - c[0] * c[7], a22 = c[0] * c[4] - c[1] * c[3];
  const float det = c[0] * a00 + c[1] * a10 + c[2] * a20;
  const float nan = __int_as_float(0x7fc00000);
  // no volume: the reference's test (isclose(|det|, 0), which raises there), and a determinant that is rounding residue of its own terms
  const float scale = sqrtf((c[0] * c[0] + c[1] * c[1] + c[2] * c[2]) * (c[3] * c[3] + c[4] * c[4] + c[5] * c[5]) * (c[6] * c[6] + c[7] * c[7] + c[8] * c[8]));
  const bool vol = fabsf(det) > 1e-8f && fabsf(det) > 1e-5f * scale;
  const float id = vol ? 1.0f / det : nan;
  float* o = info + kEwaldCell * m;
  o[0] = a00 * id; o[1] = a01 * id; o[2] = a02 * id;
  o[3] = a10 * id; o[4] = a11 * id; o[5] = a12 * id;
  o[6] = a20 * id; o[7] = a21 * id; o[8] = a22 * id;
  o[9] = vol ? fabsf(det) : nan;
  o[10] = 0.f; o[11] = 0.f;
}

// the three integer components of k-vector k, clamped to the table
__device__ __forceinline__ void ew_kvec(const float* __restrict__ kvecs, int64_t k, int& nx, int& ny, int& nz) {
  nx = (int)kvecs[3 * k]; ny = (int)kvecs[3 * k + 1]; nz = (int)kvecs[3 * k + 2];
  nx = nx < -kEwaldKmax ? -kEwaldKmax : (nx > kEwaldKmax ? kEwaldKmax : nx);
  ny = ny < -kEwaldKmax ? -kEwaldKmax : (ny > kEwaldKmax ? kEwaldKmax : ny);
  nz = nz < -kEwaldKmax ? -kEwaldKmax : (nz > kEwaldKmax ? kEwaldKmax : nz);
}

// tab[axis][n] = e^{2 pi i n s_axis} (times w on axis 0) of the atom at r with the inverse cell ci; item = axis * kEwaldNf + n
__device__ __forceinline__ void ew_factor(const float* __restrict__ r, const float* __restrict__ ci, int item, int k_max, float w, float2* __restrict__ tab) {
  const int ax = item / kEwaldNf, n = item - ax * kEwaldNf;
  if (n > k_max) return;
  const float s = r[0] * ci[ax] + r[1] * ci[3 + ax] + r[2] * ci[6 + ax];
  float sn, cs;
  sincospif(2.0f * (float)n * s, &sn, &cs);
  if (ax == 0) { sn *= w; cs *= w; }
  tab[item] = make_float2(cs, sn);
}

// e = tab_x[|nx|] tab_y[|ny|] tab_z[|nz|] with conjugates for negative components
__device__ __forceinline__ float2 ew_phase(const float2* __restrict__ tab, int nx, int ny, int nz) {
  float2 a = tab[nx < 0 ? -nx : nx], b = tab[kEwaldNf + (ny < 0 ? -ny : ny)], c = tab[2 * kEwaldNf + (nz < 0 ? -nz : nz)];
  if (nx < 0) a.y = -a.y;
  if (ny < 0) b.y = -b.y;
  if (nz < 0) c.y = -c.y;
  const float pr = a.x * b.x - a.y * b.y, pi = a.x * b.y + a.y * b.x;
  return make_float2(pr * c.x - pi * c.y, pr * c.y + pi * c.x);
}

__global__ __launch_bounds__(256) void k_ewald_sfac(const float* __restrict__ R, const float* __restrict__ q, const int64_t* __restrict__ idx_m,
                                                    const float* __restrict__ info, const float* __restrict__ kvecs, int64_t N, int64_t K, int64_t n_mol,
                                                    int k_max, float* __restrict__ part) {
  __shared__ float2 tab[kEwaldTile][3 * kEwaldNf];
  __shared__ int mol[kEwaldTile];
  const int64_t slab = blockIdx.y;
  const int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const bool live = k < K;
  int nx = 0, ny = 0, nz = 0;
  if (live) ew_kvec(kvecs, k, nx, ny, nz);
  const int64_t a_begin = slab * kEwaldSlab, a_end = (a_begin + kEwaldSlab < N) ? a_begin + kEwaldSlab : N;
  int64_t cur = -1;
  float sr = 0.f, si = 0.f;
  for (int64_t t0 = a_begin; t0 < a_end; t0 += kEwaldTile) {
    const int nt = (int)((a_end - t0 < kEwaldTile) ? a_end - t0 : kEwaldTile);
    __syncthreads();                                 // the previous tile has been read
    for (int w = threadIdx.x; w < nt * 3 * kEwaldNf; w += blockDim.x) {
      const int t = w / (3 * kEwaldNf), item = w - t * (3 * kEwaldNf);
      const int64_t a = t0 + t;
      int64_t m = idx_m[a];
      m = m < 0 ? 0 : (m >= n_mol ? n_mol - 1 : m);  // (never an out-of-bounds read)
      if (item == 0) mol[t] = (int)m;
      ew_factor(R + 3 * a, info + kEwaldCell * m, item, k_max, q[a], tab[t]);
    }
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
      const int64_t m = mol[t];                      // uniform over the block
      if (m != cur) {
        if (cur >= 0 && live) { float* o = part + ((slab + cur) * K + k) * 2; o[0] = sr; o[1] = si; }
        cur = m; sr = 0.f; si = 0.f;
      }
      const float2 e = ew_phase(tab[t], nx, ny, nz);
      sr += e.x; si += e.y;
    }
  }
  if (cur >= 0 && live) { float* o = part + ((slab + cur) * K + k) * 2; o[0] = sr; o[1] = si; }
}

// fixed tree over the 256 lanes of a block; the result is valid in every lane
__device__ __forceinline__ float ew_block_sum(float v, float* __restrict__ sh) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__global__ __launch_bounds__(256) void k_ewald_reduce(const float* __restrict__ part, const float* __restrict__ q, const int32_t* __restrict__ molptr,
                                                      const float* __restrict__ info, const float* __restrict__ kvecs, int64_t K,
                                                      const float* __restrict__ prm, float* __restrict__ coef, float* __restrict__ Eo) {
  __shared__ float sh[4];
  const int64_t m = blockIdx.x;
  const float ke = prm[0], alpha = prm[1];
  const float* ci = info + kEwaldCell * m;
  const float V = ci[9];
  const int64_t a0 = molptr[m], a1 = molptr[m + 1];
  float acc = 0.f;
  for (int64_t k = threadIdx.x; k < K; k += blockDim.x) {
    float sr = 0.f, si = 0.f;
    if (a1 > a0) {
      for (int64_t s = a0 / kEwaldSlab; s <= (a1 - 1) / kEwaldSlab; ++s) {
        const float* p = part + ((s + m) * K + k) * 2;
        sr += p[0]; si += p[1];
      }
    }
    const float n0 = kvecs[3 * k], n1 = kvecs[3 * k + 1], n2 = kvecs[3 * k + 2];
    const float kx = kTwoPi * (ci[0] * n0 + ci[1] * n1 + ci[2] * n2), ky = kTwoPi * (ci[3] * n0 + ci[4] * n1 + ci[5] * n2),
                kz = kTwoPi * (ci[6] * n0 + ci[7] * n1 + ci[8] * n2);
    const float k2 = kx * kx + ky * ky + kz * kz;
    const float g = expf(-0.25f * k2 / alpha) / k2;
    coef[(m * K + k) * 2] = g * sr; coef[(m * K + k) * 2 + 1] = g * si;
    acc += g * (sr * sr + si * si);
  }
  const float rec = ew_block_sum(acc, sh);
  float qq = 0.f;
  for (int64_t a = a0 + threadIdx.x; a < a1; a += blockDim.x) qq += q[a] * q[a];
  const float self = ew_block_sum(qq, sh);
  if (threadIdx.x == 0) Eo[m] = ke * (kTwoPi / V * rec - sqrtf(alpha / SPK_PI_F) * self);
}

__global__ __launch_bounds__(256) void k_ewald_bwd(const float* __restrict__ gE, const float* __restrict__ R, const float* __restrict__ q,
                                                   const int64_t* __restrict__ idx_m, const float* __restrict__ info, const float* __restrict__ kvecs,
                                                   const float* __restrict__ coef, int64_t N, int64_t K, int64_t n_mol, int k_max,
                                                   const float* __restrict__ prm, float* __restrict__ gR, float* __restrict__ gq) {
  __shared__ float2 tab[4][3 * kEwaldNf];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float ke = prm[0], alpha = prm[1];
  for (int64_t base = blockIdx.x * (int64_t)4; base < N; base += (int64_t)gridDim.x * 4) {      // uniform over the block
    const int64_t a = base + wave;
    const bool valid = a < N;
    int64_t m = 0;
    if (valid) {
      m = idx_m[a];
      m = m < 0 ? 0 : (m >= n_mol ? n_mol - 1 : m);
    }
    const float* ci = info + kEwaldCell * m;
    __syncthreads();
    if (valid && lane < 3 * kEwaldNf) ew_factor(R + 3 * a, ci, lane, k_max, 1.0f, tab[wave]);
    __syncthreads();
    if (!valid) continue;
    float sq = 0.f, s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int64_t k = lane; k < K; k += 64) {
      int nx, ny, nz;
      ew_kvec(kvecs, k, nx, ny, nz);
      const float2 e = ew_phase(tab[wave], nx, ny, nz);
      const float cr = coef[(m * K + k) * 2], cim = coef[(m * K + k) * 2 + 1];
      sq += cr * e.x + cim * e.y;                   // Re(c* e)
      const float t = cr * e.y - cim * e.x;         // Im(c* e)
      s0 += (float)nx * t; s1 += (float)ny * t; s2 += (float)nz * t;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      sq += __shfl_xor(sq, d, 64); s0 += __shfl_xor(s0, d, 64); s1 += __shfl_xor(s1, d, 64); s2 += __shfl_xor(s2, d, 64);
    }
    if (lane == 0) {
      const float qi = q[a];
      const float gm = gE[m] * ke;
      const float pref = 2.0f * kTwoPi / ci[9];
      if (gq) gq[a] = gm * (pref * sq - 2.0f * sqrtf(alpha / SPK_PI_F) * qi);
      if (gR) {
        const float f = -gm * pref * qi * kTwoPi;
        gR[3 * a] = f * (ci[0] * s0 + ci[1] * s1 + ci[2] * s2);
        gR[3 * a + 1] = f * (ci[3] * s0 + ci[4] * s1 + ci[5] * s2);
        gR[3 * a + 2] = f * (ci[6] * s0 + ci[7] * s1 + ci[8] * s2);
      }
    }
  }
}

struct EwaldWs { int32_t* molptr; float* info; float* part; size_t bytes; };

EwaldWs ewald_ws(char* base, int64_t N, int64_t K, int64_t n_mol) {
  EwaldWs w;
  size_t o = 0;
  const int64_t n_slabs = (N + kEwaldSlab - 1) / kEwaldSlab;
  w.molptr = (int32_t*)(base ? base + o : nullptr); o += ew_align((size_t)(n_mol + 1) * 4);
  w.info = (float*)(base ? base + o : nullptr); o += ew_align((size_t)(n_mol > 0 ? n_mol : 1) * kEwaldCell * 4);
  w.part = (float*)(base ? base + o : nullptr); o += ew_align((size_t)(n_slabs + n_mol + 1) * (size_t)(K > 0 ? K : 1) * 8);
  w.bytes = o;
  return w;
}

int ewald_check(const char* who, int64_t N, int64_t K, int64_t n_mol, int32_t k_max) {
  SPK_CHECK_ARG(N >= 0 && K >= 0 && n_mol >= 0, "%s: bad sizes", who);
  SPK_CHECK_ARG(k_max >= 0 && k_max <= kEwaldKmax, "%s: k_max = %d is beyond the factor table (at most %d)", who, (int)k_max, kEwaldKmax);
  SPK_CHECK_ARG(N < (1LL << 31) - 2 && K < (1LL << 24), "%s: too many atoms / k-vectors", who);
  return SPK_OK;
}

}  // namespace

extern "C" int32_t spk_ewald_max_kmax(void) { return kEwaldKmax; }
extern "C" int32_t spk_ewald_atom_tile(void) { return kEwaldTile; }
extern "C" int32_t spk_ewald_atom_slab(void) { return kEwaldSlab; }

extern "C" int64_t spk_ewald_workspace_bytes(int64_t n_atoms, int64_t n_kvecs, int64_t n_mol) {
  if (n_atoms < 0 || n_kvecs < 0 || n_mol < 0) return -1;
  return (int64_t)ewald_ws(nullptr, n_atoms, n_kvecs, n_mol).bytes;
}

extern "C" int spk_ewald_recip_fwd_f32(const float* R, const float* q, const float* cell, const int64_t* idx_m, int64_t N, int64_t n_mol,
                                       const float* kvecs, int64_t K, int32_t k_max, const float* params, float* E, float* coeffs, void* workspace,
                                       void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "spk_ewald_recip_fwd_f32";
  SPK_TRY(ewald_check(who, N, K, n_mol, k_max));
  if (n_mol == 0) return SPK_OK;
  SPK_CHECK_ARG(params && workspace && E && cell && (K == 0 || (kvecs && coeffs)) && (N == 0 || (R && q && idx_m)), "%s: null argument", who);
  EwaldWs w = ewald_ws((char*)workspace, N, K, n_mol);
  float* cellinfo = w.info;
  SpkProfScope prof("ewald_recip_fwd", stream);
  hipLaunchKernelGGL(k_ewald_cell, dim3(spk_grid_for(n_mol, 256, 1 << 30)), dim3(256), 0, stream, cell, n_mol, cellinfo);
  SPK_LAUNCH_CHECK();
  SPK_TRY(spk_segment_rowptr_i32(idx_m, N, n_mol, w.molptr, nullptr, stream));
  if (N > 0 && K > 0) {
    const int64_t n_slabs = (N + kEwaldSlab - 1) / kEwaldSlab;
    SPK_CHECK_ARG(n_slabs <= 65535, "%s: more than 65535 atom slabs", who);
    hipLaunchKernelGGL(k_ewald_sfac, dim3((unsigned)((K + 255) / 256), (unsigned)n_slabs), dim3(256), 0, stream, R, q, idx_m, (const float*)cellinfo, kvecs, N,
                       K, n_mol, (int)k_max, w.part);
    SPK_LAUNCH_CHECK();
  }
  SPK_CHECK_ARG(n_mol <= 0x7fffffff, "%s: too many molecules", who);
  hipLaunchKernelGGL(k_ewald_reduce, dim3((unsigned)n_mol), dim3(256), 0, stream, (const float*)w.part, q, (const int32_t*)w.molptr, (const float*)cellinfo,
                     kvecs, K, params, coeffs, E);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" int spk_ewald_recip_bwd_f32(const float* gE, const float* R, const float* q, const float* cell, const int64_t* idx_m, int64_t N,
                                       int64_t n_mol, const float* kvecs, int64_t K, int32_t k_max, const float* params, const float* coeffs,
                                       float* gR, float* gq, void* workspace, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "spk_ewald_recip_bwd_f32";
  SPK_TRY(ewald_check(who, N, K, n_mol, k_max));
  if (N == 0) return SPK_OK;
  SPK_CHECK_ARG(n_mol > 0 && gE && R && q && cell && idx_m && params && workspace && (gR || gq) && (K == 0 || (kvecs && coeffs)), "%s: null argument", who);
  float* cellinfo = ewald_ws((char*)workspace, N, K, n_mol).info;
  SpkProfScope prof("ewald_recip_bwd", stream);
  hipLaunchKernelGGL(k_ewald_cell, dim3(spk_grid_for(n_mol, 256, 1 << 30)), dim3(256), 0, stream, cell, n_mol, cellinfo);
  SPK_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ewald_bwd, dim3(spk_grid_for(N, 4, spk_num_cus() * 32)), dim3(256), 0, stream, gE, R, q, idx_m, (const float*)cellinfo, kvecs, coeffs, N, K, n_mol,
                     (int)k_max, params, gR, gq);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}
