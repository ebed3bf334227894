// Ring-polymer thermostats in normal-mode space (md/simulation_hooks/thermostats_rpmd.py) next to PILE-L of spk_md.hip: the
// Nose-Hoover chain per normal mode (NHCRingPolymerThermostat, local and global centroid) and PILE-G (PILEGlobalThermostat: PILE-L
// on the modes k >= 1, stochastic velocity rescaling per molecule on the centroid).  fp32, wave64, no float atomics, no host
// synchronisation, no allocation; one thread per (atom, component) t, momenta p_all [B, N, 3], C [B, B] = normal_mode_matrix in LDS.
// The per-molecule sums go through spk_md_kinetic_f32, the molecule chains through spk_md_nhc_global_f32.
#include "spk_common.h"
#include "spk_md_common.h"

namespace {

// p_c[t] = C[0][0] sum_b p_b[t]  (mode 0 has C[0][b] = 1 / sqrt(B) for every bead; the plain sum of a polymer at rest is exactly 0)
// and, with xi_c given, the centroid noise of k_md_pile: mode 0 of mode pair 0 (spk_pile_noise_pair).
__global__ __launch_bounds__(256) void k_rp_centroid(const float* __restrict__ p_all, float c00, int B, int64_t n3, float* __restrict__ p_c,
                                                     float* __restrict__ xi_c, uint32_t seed_lo, uint32_t seed_hi, uint64_t step_host,
                                                     const int64_t* __restrict__ step_dev, uint32_t which) {
  const uint64_t step = step_dev ? (uint64_t)step_dev[0] : step_host;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n3; t += (int64_t)gridDim.x * blockDim.x) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += p_all[(int64_t)b * n3 + t];
    p_c[t] = s * c00;
    if (xi_c) {
      float x0, x1;
      spk_pile_noise_pair(t, 0, step, which, seed_lo, seed_hi, x0, x1);
      xi_c[t] = x0;
    }
  }
}

// NHC on the normal modes: p_nm[k] = sum_b C[k][b] p_b, one chain per (mode, component) with kinetic term p_nm^2 / m, one degree of
// freedom, every link mass mlink[k]; p'_nm[k] = scale_k p_nm[k]; p_out[bl] = sum_k C[k][bead0 + bl] p'_nm[k].  With scale_c (global
// centroid) mode 0 is multiplied by scale_c[idx_m[atom]] and its per-component chain is left alone.  Chain state [L, B, n3]: every
// caller updates ALL modes.  BMAX / LMAX bound the unrolled, predicated loops: the bead and chain vectors stay in registers.
template <int BMAX, int LMAX>
__global__ __launch_bounds__(256) void k_rp_nhc(const float* __restrict__ p_all, const float* __restrict__ masses, const float* __restrict__ C,
                                                const float* __restrict__ mlink, int B, int64_t n_atoms, int bead0, int n_local, int L,
                                                int multi_step, int order, YsSteps ys, float kT, float* __restrict__ vel, float* __restrict__ frc,
                                                const float* __restrict__ scale_c, const int64_t* __restrict__ idx_m, int64_t n_mol,
                                                int32_t* __restrict__ err, float* __restrict__ p_out) {
  extern __shared__ float sC[];   // [B][B] + [B]
  float* sm = sC + B * B;
  for (int s = threadIdx.x; s < B * B; s += blockDim.x) sC[s] = C[s];
  for (int s = threadIdx.x; s < B; s += blockDim.x) sm[s] = mlink[s];
  __syncthreads();
  const int64_t n3 = 3 * n_atoms;
  int bad = 0;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n3; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t at = t / 3;
    const float im = 1.0f / masses[at];
    float pb[BMAX], out[BMAX];
#pragma unroll
    for (int b = 0; b < BMAX; ++b) { pb[b] = b < B ? p_all[(int64_t)b * n3 + t] : 0.f; out[b] = 0.f; }
    for (int k = 0; k < B; ++k) {
      const float* row = sC + k * B;
      float pn = 0.f;
#pragma unroll
      for (int b = 0; b < BMAX; ++b) if (b < B) pn = fmaf(row[b], pb[b], pn);
      float s;
      if (k == 0 && scale_c) {
        const int64_t m = idx_m[at];
        if ((uint64_t)m >= (uint64_t)n_mol) { bad = 2; s = 1.0f; } else s = scale_c[m];
      } else {
        float v[LMAX], f[LMAX];
        const int64_t base = (int64_t)k * n3 + t, stride = (int64_t)B * n3;
#pragma unroll
        for (int l = 0; l < LMAX; ++l) { v[l] = l < L ? vel[l * stride + base] : 0.f; f[l] = l < L ? frc[l * stride + base] : 0.f; }
        const float mq = sm[k];
        s = nhc_propagate<LMAX>(v, f, L, pn * pn * im, kT, kT, mq, mq, multi_step, order, ys);
#pragma unroll
        for (int l = 0; l < LMAX; ++l) if (l < L) { vel[l * stride + base] = v[l]; frc[l * stride + base] = f[l]; }
      }
      pn *= s;
#pragma unroll
      for (int u = 0; u < BMAX; ++u) if (u < n_local) out[u] = fmaf(row[bead0 + u], pn, out[u]);
    }
#pragma unroll
    for (int u = 0; u < BMAX; ++u) if (u < n_local) p_out[(int64_t)u * n3 + t] = out[u];
  }
  if (bad && err) atomicOr(err, bad);
}

// alpha[m] of the stochastic velocity rescaling (PILEGlobalThermostat._apply_thermostat), one thread per molecule:
//   g = (1 - c) kT / K,  alpha^2 = c + S g + 2 R1 sqrt(c g),  alpha = sqrt(alpha^2) sign(R1 + sqrt(c / g))
// K = ke2[m] (centroid), S = s2[m] (sum of the squared centroid noise), R1 = the noise of the x component of the molecule's FIRST
// atom.  A molecule without atoms or with K = 0 gets alpha = 1; a first atom outside [0, n_atoms) sets err and gives alpha = 1.
__global__ __launch_bounds__(64) void k_pile_alpha(const float* __restrict__ ke2, const float* __restrict__ s2, const float* __restrict__ xi_c,
                                                   const int64_t* __restrict__ n_atoms_mol, const int64_t* __restrict__ first_atom, int64_t n_mol,
                                                   int64_t n_atoms, float c, float omc_kT, float* __restrict__ alpha, int32_t* __restrict__ err) {
  const int64_t m = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (m >= n_mol) return;
  float a = 1.0f;
  const int64_t na = n_atoms_mol[m], a0 = first_atom[m];
  const float K = ke2[m];
  if (na > 0 && ((uint64_t)a0 >= (uint64_t)n_atoms)) {
    if (err) atomicOr(err, 2);
  } else if (na > 0 && K > 0.f) {
    const float R1 = xi_c[3 * a0];
    const float g = omc_kT / K;
    const float a2 = c + s2[m] * g + 2.0f * R1 * sqrtf(c * g);
    const float sg = R1 + sqrtf(c / g);
    a = sqrtf(fmaxf(a2, 0.f)) * (sg > 0.f ? 1.0f : (sg < 0.f ? -1.0f : 0.f));
  }
  alpha[m] = a;
}

// PILE-G application: the body of k_md_pile (spk_pile_component of spk_md_common.h, so mode k >= 1 of component t draws what it
// draws in spk_md_pile_f32) on M with the centroid taken out (c1[0] = c2[0] = 0), plus alpha[idx_m[atom]] p_c[t] C[0][0] for the centroid.
__global__ void k_rp_pile_global(const float* __restrict__ p_all, const float* __restrict__ masses, const float* __restrict__ M, float scale,
                                 uint32_t seed_lo, uint32_t seed_hi, uint64_t step_host, const int64_t* __restrict__ step_dev, uint32_t which,
                                 int B, int64_t n_atoms, int bead0, int n_local, const float* __restrict__ p_c, const float* __restrict__ alpha,
                                 const int64_t* __restrict__ idx_m, int64_t n_mol, float c00, int32_t* __restrict__ err, float* __restrict__ p_out) {
  extern __shared__ float sM[];   // [2][B][B]
  for (int s = threadIdx.x; s < 2 * B * B; s += blockDim.x) sM[s] = M[s];
  __syncthreads();
  const uint64_t step = step_dev ? (uint64_t)step_dev[0] : step_host;
  const int64_t n3 = 3 * n_atoms;
  int bad = 0;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n3; t += (int64_t)gridDim.x * blockDim.x) {
    const float sm = sqrtf(masses[t / 3]) * scale;
    const int64_t m = idx_m[t / 3];
    float al = 1.0f;
    if ((uint64_t)m >= (uint64_t)n_mol) bad = 2; else al = alpha[m];
    const float cen = al * p_c[t] * c00;
    spk_pile_component<true>(p_all, sM, sm, seed_lo, seed_hi, step, which, B, n3, t, bead0, n_local, cen, p_out);
  }
  if (bad && err) atomicOr(err, bad);
}

int check_beads(const char* who, int32_t n_beads, int64_t n_atoms, int32_t bead0, int32_t n_local) {
  SPK_CHECK_ARG(n_beads >= 1 && n_beads <= 64 && n_atoms >= 0, "%s: bad sizes (1 <= n_beads <= 64)", who);
  SPK_CHECK_ARG(n_atoms < (1LL << 31) - 2, "%s: too many atoms", who);
  SPK_CHECK_ARG(bead0 >= 0 && n_local >= 0 && bead0 + n_local <= n_beads, "%s: bead range outside [0, n_beads)", who);
  return SPK_OK;
}

}  // namespace

extern "C" int spk_md_rp_centroid_f32(const float* p_all, int32_t n_beads, int64_t n_atoms, float* p_c, float* xi_c, uint64_t seed, uint64_t step,
                                      const int64_t* step_dev, int32_t which, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "spk_md_rp_centroid_f32";
  SPK_TRY(check_beads(who, n_beads, n_atoms, 0, n_beads));
  if (n_atoms == 0) return SPK_OK;
  SPK_CHECK_ARG(p_all && p_c && p_c != p_all && xi_c != p_all, "%s: null pointer / output aliases the input", who);
  SpkProfScope prof("md_rp_centroid", stream);
  hipLaunchKernelGGL(k_rp_centroid, dim3(spk_grid_for(3 * n_atoms, 256, spk_num_cus() * 8)), dim3(256), 0, stream, p_all,
                     (float)(1.0 / sqrt((double)n_beads)), n_beads, 3 * n_atoms, p_c, xi_c, (uint32_t)seed, (uint32_t)(seed >> 32), step, step_dev,
                     (uint32_t)which);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

#define RP_NHC_LAUNCH(BM, LM) hipLaunchKernelGGL((k_rp_nhc<BM, LM>), grid, dim3(256), lds, stream, p_all, masses, C, link_masses, n_beads, n_atoms, bead0, \
                                                 n_local, chain_length, multi_step, integration_order, ys, kT, velocities, forces, scale_centroid, idx_m, \
                                                 n_mol, err, p_out)
#define RP_NHC_BEADS(LM) do { if (n_beads <= 4) RP_NHC_LAUNCH(4, LM); else if (n_beads <= 8) RP_NHC_LAUNCH(8, LM); else if (n_beads <= 16) RP_NHC_LAUNCH(16, LM); \
                              else if (n_beads <= 32) RP_NHC_LAUNCH(32, LM); else RP_NHC_LAUNCH(64, LM); } while (0)

extern "C" int spk_md_rp_nhc_f32(const float* p_all, const float* masses, const float* C, const float* link_masses, int32_t n_beads, int64_t n_atoms,
                                 int32_t bead0, int32_t n_local, int32_t chain_length, int32_t multi_step, int32_t integration_order,
                                 const float* sub_steps, float kT, float* velocities, float* forces, const float* scale_centroid,
                                 const int64_t* idx_m, int64_t n_mol, int32_t* err, float* p_out, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "spk_md_rp_nhc_f32";
  YsSteps ys;
  SPK_TRY(check_chain(who, chain_length, multi_step, integration_order, sub_steps, &ys));
  SPK_TRY(check_beads(who, n_beads, n_atoms, bead0, n_local));
  SPK_CHECK_ARG(kT > 0.f, "%s: kT must be positive", who);
  SPK_CHECK_ARG(n_mol >= 0, "%s: bad number of molecules", who);
  if (n_atoms == 0) return SPK_OK;
  SPK_CHECK_ARG(p_all && masses && C && link_masses && velocities && forces, "%s: null pointer", who);
  SPK_CHECK_ARG(n_local == 0 || (p_out && p_out != p_all), "%s: null output / output aliases the input", who);
  SPK_CHECK_ARG(scale_centroid == nullptr || idx_m != nullptr, "%s: the molecule factors of the centroid need idx_m", who);
  const size_t lds = sizeof(float) * ((size_t)n_beads * n_beads + n_beads);      // <= 16.3 KB
  const dim3 grid(spk_grid_for(3 * n_atoms, 256, spk_num_cus() * 8));
  SpkProfScope prof("md_rp_nhc", stream);
  if (chain_length <= 4) RP_NHC_BEADS(4); else if (chain_length <= 8) RP_NHC_BEADS(8); else RP_NHC_BEADS(16);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" int spk_md_pile_alpha_f32(const float* ke2, const float* noise2, const float* xi_c, const int64_t* n_atoms_mol, const int64_t* first_atom,
                                     int64_t n_mol, int64_t n_atoms, float c1_centroid, float one_minus_c1_kT, float* alpha, int32_t* err,
                                     void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "spk_md_pile_alpha_f32";
  SPK_CHECK_ARG(n_mol >= 0 && n_atoms >= 0, "%s: bad sizes", who);
  SPK_CHECK_ARG(c1_centroid > 0.f && c1_centroid <= 1.f && one_minus_c1_kT >= 0.f, "%s: c1 must be in (0, 1] and (1 - c1) kT not negative", who);
  if (n_mol == 0) return SPK_OK;
  SPK_CHECK_ARG(ke2 && noise2 && n_atoms_mol && first_atom && alpha && (xi_c || n_atoms == 0), "%s: null pointer", who);
  hipLaunchKernelGGL(k_pile_alpha, dim3(spk_grid_for(n_mol, 64, 1 << 30)), dim3(64), 0, stream, ke2, noise2, xi_c, n_atoms_mol, first_atom, n_mol,
                     n_atoms, c1_centroid, one_minus_c1_kT, alpha, err);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" int spk_md_pile_global_f32(const float* p_all, const float* masses, const float* M, float noise_scale, uint64_t seed, uint64_t step,
                                      const int64_t* step_dev, int32_t which, int32_t n_beads, int64_t n_atoms, int32_t bead0, int32_t n_local,
                                      const float* p_c, const float* alpha, const int64_t* idx_m, int64_t n_mol, int32_t* err, float* p_out,
                                      void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "spk_md_pile_global_f32";
  SPK_TRY(check_beads(who, n_beads, n_atoms, bead0, n_local));
  SPK_CHECK_ARG(n_mol >= 0, "%s: bad number of molecules", who);
  if (n_atoms == 0 || n_local == 0) return SPK_OK;
  SPK_CHECK_ARG(p_all && masses && M && p_c && alpha && idx_m && p_out && p_out != p_all, "%s: null pointer / output aliases the input", who);
  const size_t lds = sizeof(float) * 2 * (size_t)n_beads * n_beads;      // <= 32 KB
  SpkProfScope prof("md_pile_global", stream);
  hipLaunchKernelGGL(k_rp_pile_global, dim3(spk_grid_for(3 * n_atoms, 256, spk_num_cus() * 8)), dim3(256), lds, stream, p_all, masses, M, noise_scale,
                     (uint32_t)seed, (uint32_t)(seed >> 32), step, step_dev, (uint32_t)which, n_beads, n_atoms, bead0, n_local, p_c, alpha, idx_m,
                     n_mol, (float)(1.0 / sqrt((double)n_beads)), err, p_out);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}
