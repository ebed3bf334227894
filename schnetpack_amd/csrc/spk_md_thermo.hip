// Classical NVT thermostats next to the velocity-Verlet kernels of spk_md.hip (md/simulation_hooks/thermostats.py): the per-molecule
// kinetic reduction, the Nose-Hoover chain in its global (one chain per replica x molecule) and massive (one chain per momentum
// component) forms, Berendsen rescaling, and the pass that multiplies the atoms of molecule m by scale[m].  fp32, wave64, no float
// atomics, no host synchronisation, no allocation: a HIP-graph capture takes every call as it is.  Langevin needs no kernel of its
// own (spk_md_pile_f32 at one bead).
//
// Kinetic reduction -- the scheme of spk_virial.hip, results bit-identical from call to call:
//   k_kin_chunk   atoms in chunks of 64: the first atom of every (chunk, molecule) segment sums |p|^2 / m over the segment in atom
//                 order -> P; the same launch derives the molecules' atom ranges molptr from the ascending idx_m
//   k_kin_mol     one wave per (replica, molecule): lane l sums the chunk partials l, l + 64, ... in order, then a fixed butterfly.
//                 A 32 k-atom molecule is 500 partials over 64 lanes, 600 three-atom molecules are 600 waves.
#include "spk_common.h"
#include "spk_md_common.h"

namespace {

constexpr int kKinChunk = 64;

inline size_t thermo_align(size_t b) { return (b + 255) & ~(size_t)255; }

// P[r, a] = sum over the atoms a .. of a's molecule inside a's chunk of |p_a|^2 / m_a, for every atom that starts such a segment.
// idx_m is only ever COMPARED here and clamped into [-1, n_mol] before it bounds the molptr loop: a malformed index (descending,
// out of range) sets err and can write no element outside molptr [n_mol + 1].
__global__ __launch_bounds__(256) void k_kin_chunk(const float* __restrict__ p, const float* __restrict__ masses, const int64_t* __restrict__ idx_m,
                                                   int64_t N, int64_t n_mol, float* __restrict__ P, int32_t* __restrict__ molptr,
                                                   int32_t* __restrict__ err) {
  const int64_t a = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t r = blockIdx.y;
  if (r == 0 && a <= N) {               // molptr[m] = first atom a with idx_m[a] >= m
    int64_t prev = (a > 0) ? idx_m[a - 1] : -1;
    int64_t cur = (a < N) ? idx_m[a] : n_mol;
    int bad = 0;
    if (a < N && (cur < 0 || cur >= n_mol)) bad |= 2;
    if (a > 0 && a < N && prev > cur) bad |= 1;
    if (prev < -1) prev = -1;
    if (cur > n_mol) cur = n_mol;
    for (int64_t m = prev + 1; m <= cur; ++m) molptr[m] = (int32_t)a;
    if (bad && err) atomicOr(err, bad);
  }
  if (a >= N) return;
  const int64_t m = idx_m[a];
  if ((a % kKinChunk) != 0 && idx_m[a - 1] == m) return;
  const int64_t end = ((a / kKinChunk + 1) * kKinChunk < N) ? (a / kKinChunk + 1) * kKinChunk : N;
  const float* pr = p + 3 * r * N;
  float s = 0.f;
  for (int64_t b = a; b < end && idx_m[b] == m; ++b) {
    const float x = pr[3 * b], y = pr[3 * b + 1], z = pr[3 * b + 2];
    s += (x * x + y * y + z * z) / masses[b];
  }
  P[r * N + a] = s;
}

// ke2[r, m] = sum over the chunks the molecule's atoms [a0, a1) touch of P[r, max(a0, 64 c)].  A range that is not inside [0, N]
// (molptr of a malformed idx_m) gives 0 and sets err; it is never used as an address.
__global__ __launch_bounds__(256) void k_kin_mol(const float* __restrict__ P, const int32_t* __restrict__ molptr, int64_t N, int64_t n_mol,
                                                 int64_t n_rep, float* __restrict__ ke2, int32_t* __restrict__ err) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  if (w >= n_mol * n_rep) return;                     // uniform over the wave
  const int64_t r = w / n_mol, m = w - r * n_mol;
  const int64_t a0 = molptr[m], a1 = molptr[m + 1];
  float s = 0.f;
  if (a0 < 0 || a1 > N || a0 > a1) {
    if (lane == 0 && err) atomicOr(err, 1);
  } else if (a1 > a0) {
    const int64_t c0 = a0 / kKinChunk, c1 = (a1 - 1) / kKinChunk;
    for (int64_t c = c0 + lane; c <= c1; c += 64) s += P[r * N + ((c * kKinChunk > a0) ? c * kKinChunk : a0)];
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
  if (lane == 0) ke2[w] = s;
}

// global form: one thread per (replica, molecule) chain; state [n_chains, L].  A molecule without atoms keeps its chain, scale = 1.
template <int LMAX>
__global__ __launch_bounds__(64) void k_nhc_global(const float* __restrict__ ke2, const int64_t* __restrict__ n_atoms_mol, int64_t n_chains, int64_t n_mol,
                                                   int L, int multi_step, int order, YsSteps ys, float kT, float mq, float* __restrict__ vel,
                                                   float* __restrict__ frc, float* __restrict__ scale) {
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= n_chains) return;
  const int64_t na = n_atoms_mol[c % n_mol];
  if (na <= 0) { scale[c] = 1.0f; return; }
  float v[LMAX], f[LMAX];
#pragma unroll
  for (int l = 0; l < LMAX; ++l) { v[l] = l < L ? vel[c * L + l] : 0.f; f[l] = l < L ? frc[c * L + l] : 0.f; }
  const float dof = 3.0f * (float)na;
  scale[c] = nhc_propagate<LMAX>(v, f, L, ke2[c], dof * kT, kT, dof * mq, mq, multi_step, order, ys);
#pragma unroll
  for (int l = 0; l < LMAX; ++l) if (l < L) { vel[c * L + l] = v[l]; frc[c * L + l] = f[l]; }
}

// massive form: one thread per momentum component t of [n_rep, N, 3]; chain state [L, n_dof] (link-major: consecutive threads read
// consecutive floats of every link), kinetic term p^2 / m, one degree of freedom; 2 L + 1 floats in and out per component.
template <int LMAX>
__global__ __launch_bounds__(256) void k_nhc_massive(float* __restrict__ p, const float* __restrict__ masses, int64_t N, int64_t n_dof, int L, int multi_step,
                                                     int order, YsSteps ys, float kT, float mq, float* __restrict__ vel, float* __restrict__ frc) {
  const int64_t n3 = 3 * N;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n_dof; t += (int64_t)gridDim.x * blockDim.x) {
    float v[LMAX], f[LMAX];
#pragma unroll
    for (int l = 0; l < LMAX; ++l) { v[l] = l < L ? vel[(int64_t)l * n_dof + t] : 0.f; f[l] = l < L ? frc[(int64_t)l * n_dof + t] : 0.f; }
    const float pv = p[t];
    const float ke = pv * pv / masses[(t % n3) / 3];
    const float s = nhc_propagate<LMAX>(v, f, L, ke, kT, kT, mq, mq, multi_step, order, ys);
    p[t] = pv * s;
#pragma unroll
    for (int l = 0; l < LMAX; ++l) if (l < L) { vel[(int64_t)l * n_dof + t] = v[l]; frc[(int64_t)l * n_dof + t] = f[l]; }
  }
}

// scale[r, m] = sqrt(1 + dt / tau (T0 / T - 1)),  T = ke2 / (3 n_atoms kB)   (thermostats.py:172-189, system.py:407-421);
// 1 for a molecule without atoms or without kinetic energy (the reference divides by zero there).
__global__ void k_berendsen_scale(const float* __restrict__ ke2, const int64_t* __restrict__ n_atoms_mol, int64_t n_chains, int64_t n_mol,
                                  float dt_over_tau, float T0, float kB, float* __restrict__ scale) {
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= n_chains) return;
  const int64_t na = n_atoms_mol[c % n_mol];
  const float k = ke2[c];
  float s = 1.0f;
  if (na > 0 && k > 0.f) {
    const float T = 2.0f / (3.0f * (float)na * kB) * (0.5f * k);
    s = sqrtf(1.0f + dt_over_tau * (T0 / T - 1.0f));
  }
  scale[c] = s;
}

// p[r, a, :] *= scale[r, idx_m[a]]; an index outside [0, n_mol) sets err and leaves the atom alone
__global__ void k_scale_molecules(float* __restrict__ p, const float* __restrict__ scale, const int64_t* __restrict__ idx_m, int64_t N, int64_t n_mol,
                                  int64_t n_rep, int32_t* __restrict__ err) {
  const int64_t n3 = 3 * N, n = n3 * n_rep;
  int bad = 0;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = t / n3, m = idx_m[(t - r * n3) / 3];
    if ((uint64_t)m >= (uint64_t)n_mol) { bad = 2; continue; }
    p[t] *= scale[r * n_mol + m];
  }
  if (bad && err) atomicOr(err, bad);
}

}  // namespace

extern "C" int64_t spk_md_kinetic_workspace_bytes(int64_t n_replicas, int64_t n_atoms, int64_t n_mol) {
  if (n_replicas < 0 || n_atoms < 0 || n_mol < 0) return -1;
  const int64_t np = n_replicas * n_atoms;
  return (int64_t)(thermo_align((size_t)(n_mol + 1) * 4) + thermo_align((size_t)(np > 0 ? np : 1) * 4));
}

extern "C" int spk_md_kinetic_f32(const float* p, const float* masses, const int64_t* idx_m, int64_t n_replicas, int64_t n_atoms, int64_t n_mol,
                                  float* ke2, int32_t* err, void* workspace, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "spk_md_kinetic_f32";
  SPK_CHECK_ARG(n_replicas >= 0 && n_atoms >= 0 && n_mol >= 0, "%s: bad sizes", who);
  SPK_CHECK_ARG(n_atoms < (1LL << 31) - 2 && n_replicas < 65536, "%s: too many atoms for 32-bit row pointers / replicas for one grid", who);
  if (n_replicas == 0 || n_mol == 0) return SPK_OK;
  SPK_CHECK_ARG(ke2 && workspace, "%s: null output / workspace", who);
  SPK_CHECK_ARG(n_atoms == 0 || (p && masses && idx_m), "%s: null momenta / masses / molecule index", who);
  int32_t* molptr = (int32_t*)workspace;
  float* P = (float*)((char*)workspace + thermo_align((size_t)(n_mol + 1) * 4));
  SpkProfScope prof("md_kinetic", stream);
  hipLaunchKernelGGL(k_kin_chunk, dim3(spk_grid_for(n_atoms + 1, 256, 1 << 30), (unsigned)n_replicas), dim3(256), 0, stream,
                     p, masses, idx_m, n_atoms, n_mol, P, molptr, err);
  SPK_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_kin_mol, dim3(spk_grid_for(n_mol * n_replicas * 64, 256, 1 << 30)), dim3(256), 0, stream, P, molptr, n_atoms, n_mol,
                     n_replicas, ke2, err);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

#define NHC_DISPATCH(L, CALL) do { if ((L) <= 4) { constexpr int LM = 4; CALL; } else if ((L) <= 8) { constexpr int LM = 8; CALL; } else { constexpr int LM = 16; CALL; } } while (0)

extern "C" int spk_md_nhc_global_f32(const float* ke2, const int64_t* n_atoms_mol, int64_t n_replicas, int64_t n_mol, int32_t chain_length,
                                     int32_t multi_step, int32_t integration_order, const float* sub_steps, float kT, float link_mass,
                                     float* velocities, float* forces, float* scale, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "spk_md_nhc_global_f32";
  YsSteps ys;
  SPK_TRY(check_chain(who, chain_length, multi_step, integration_order, sub_steps, &ys));
  SPK_CHECK_ARG(n_replicas >= 0 && n_mol >= 0, "%s: bad sizes", who);
  SPK_CHECK_ARG(kT > 0.f && link_mass > 0.f, "%s: kT and the thermostat mass must be positive", who);
  const int64_t n_chains = n_replicas * n_mol;
  if (n_chains == 0) return SPK_OK;
  SPK_CHECK_ARG(ke2 && n_atoms_mol && velocities && forces && scale, "%s: null pointer", who);
  SpkProfScope prof("md_nhc_global", stream);
  NHC_DISPATCH(chain_length, hipLaunchKernelGGL(k_nhc_global<LM>, dim3(spk_grid_for(n_chains, 64, 1 << 30)), dim3(64), 0, stream, ke2, n_atoms_mol, n_chains,
                                                n_mol, chain_length, multi_step, integration_order, ys, kT, link_mass, velocities, forces, scale));
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" int spk_md_nhc_massive_f32(float* p, const float* masses, int64_t n_replicas, int64_t n_atoms, int32_t chain_length, int32_t multi_step,
                                      int32_t integration_order, const float* sub_steps, float kT, float link_mass, float* velocities,
                                      float* forces, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "spk_md_nhc_massive_f32";
  YsSteps ys;
  SPK_TRY(check_chain(who, chain_length, multi_step, integration_order, sub_steps, &ys));
  SPK_CHECK_ARG(n_replicas >= 0 && n_atoms >= 0, "%s: bad sizes", who);
  SPK_CHECK_ARG(kT > 0.f && link_mass > 0.f, "%s: kT and the thermostat mass must be positive", who);
  const int64_t n_dof = 3 * n_replicas * n_atoms;
  if (n_dof == 0) return SPK_OK;
  SPK_CHECK_ARG(p && masses && velocities && forces, "%s: null pointer", who);
  SpkProfScope prof("md_nhc_massive", stream);
  NHC_DISPATCH(chain_length, hipLaunchKernelGGL(k_nhc_massive<LM>, dim3(spk_grid_for(n_dof, 256, spk_num_cus() * 8)), dim3(256), 0, stream, p, masses, n_atoms,
                                                n_dof, chain_length, multi_step, integration_order, ys, kT, link_mass, velocities, forces));
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" int spk_md_berendsen_scale_f32(const float* ke2, const int64_t* n_atoms_mol, int64_t n_replicas, int64_t n_mol, float dt_over_tau,
                                          float temperature_bath, float kB, float* scale, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "spk_md_berendsen_scale_f32";
  SPK_CHECK_ARG(n_replicas >= 0 && n_mol >= 0, "%s: bad sizes", who);
  SPK_CHECK_ARG(kB > 0.f && temperature_bath >= 0.f, "%s: kB must be positive and the bath temperature not negative", who);
  const int64_t n_chains = n_replicas * n_mol;
  if (n_chains == 0) return SPK_OK;
  SPK_CHECK_ARG(ke2 && n_atoms_mol && scale, "%s: null pointer", who);
  hipLaunchKernelGGL(k_berendsen_scale, dim3(spk_grid_for(n_chains, 256, 1 << 30)), dim3(256), 0, stream, ke2, n_atoms_mol, n_chains, n_mol,
                     dt_over_tau, temperature_bath, kB, scale);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" int spk_md_scale_molecules_f32(float* p, const float* scale, const int64_t* idx_m, int64_t n_replicas, int64_t n_atoms, int64_t n_mol,
                                          int32_t* err, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "spk_md_scale_molecules_f32";
  SPK_CHECK_ARG(n_replicas >= 0 && n_atoms >= 0 && n_mol >= 0, "%s: bad sizes", who);
  if (n_replicas * n_atoms == 0) return SPK_OK;
  SPK_CHECK_ARG(p && scale && idx_m, "%s: null pointer", who);
  hipLaunchKernelGGL(k_scale_molecules, dim3(spk_grid_for(3 * n_replicas * n_atoms, 256, spk_num_cus() * 8)), dim3(256), 0, stream, p, scale, idx_m,
                     n_atoms, n_mol, n_replicas, err);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}
