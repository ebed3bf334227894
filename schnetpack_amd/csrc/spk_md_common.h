// What the MD thermostat files share (spk_md.hip, spk_md_thermo.hip, spk_md_rp_thermo.hip): the counter-based noise of the PILE
// kernels and the Yoshida-Suzuki pass over one Nose-Hoover chain.  Moved here unchanged; every user computes what it computed.
#pragma once
#include "spk_common.h"

constexpr int kMaxOrder = 7;
constexpr int kMaxChain = 16;

struct YsSteps { float dt[kMaxOrder]; };


__device__ __forceinline__ void spk_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// two standard normals from two 32-bit words (Box-Muller; u in (0, 1])
__device__ __forceinline__ void spk_box_muller(uint32_t a, uint32_t b, float& n0, float& n1) {
  const float u = ((float)(a >> 8) + 1.0f) * (1.0f / 16777216.0f);
  const float v = (float)(b >> 8) * (1.0f / 16777216.0f);
  const float r = sqrtf(-2.0f * logf(u));
  float s, c;
  sincosf(6.283185307179586f * v, &s, &c);
  n0 = r * c; n1 = r * s;
}

// THE noise of the PILE kernels: the standard normals of the modes 2 k2 and 2 k2 + 1 of (atom, component) t, one Philox block with
// counter = (t, mode pair, step, application).  Every kernel that needs the number of a mode takes it from here, so that PILE-L
// (spk_md_pile_f32), PILE-G and the centroid noise of spk_md_rp_centroid_f32 draw the same one.
__device__ __forceinline__ void spk_pile_noise_pair(int64_t t, int k2, uint64_t step, uint32_t which, uint32_t seed_lo, uint32_t seed_hi, float& x0,
                                                    float& x1) {
  uint32_t w[4];
  spk_philox4x32_10((uint32_t)t, (uint32_t)((uint64_t)t >> 32) ^ ((uint32_t)k2 << 8) ^ which, (uint32_t)step, (uint32_t)(step >> 32), seed_lo, seed_hi, w);
  spk_box_muller(w[0], w[1], x0, x1);
}

// PILE in bead space for ONE (atom, component) t:  p_out[bl] = sum_n M1[b][n] p_n + sm sum_k M2[b][k] xi_k (+ cen), b = bead0 + bl,
// sM = [2][B][B] in LDS, sm = sqrt(mass) x noise scale.  PILE_CHUNK local beads per pass (accumulators per thread); more local beads
// = more passes, the noise regenerated per pass.  CENTROID: the term PILE-G adds for the centroid it took out of the matrices.
#define PILE_CHUNK 8
template <bool CENTROID>
__device__ __forceinline__ void spk_pile_component(const float* p_all, const float* sM, float sm, uint32_t seed_lo, uint32_t seed_hi,
                                                   uint64_t step, uint32_t which, int B, int64_t n3, int64_t t, int bead0, int n_local, float cen,
                                                   float* p_out) {
  for (int b0 = 0; b0 < n_local; b0 += PILE_CHUNK) {
    float det[PILE_CHUNK], noi[PILE_CHUNK];
#pragma unroll
    for (int u = 0; u < PILE_CHUNK; ++u) { det[u] = 0.f; noi[u] = 0.f; }
    for (int n = 0; n < B; ++n) {
      const float pv = p_all[(int64_t)n * n3 + t];
#pragma unroll
      for (int u = 0; u < PILE_CHUNK; ++u)
        if (b0 + u < n_local) det[u] = fmaf(sM[(bead0 + b0 + u) * B + n], pv, det[u]);
    }
    for (int k2 = 0; k2 < (B + 1) / 2; ++k2) {       // modes 2 k2 and 2 k2 + 1 from one Philox block
      float x0, x1;
      spk_pile_noise_pair(t, k2, step, which, seed_lo, seed_hi, x0, x1);
#pragma unroll
      for (int u = 0; u < PILE_CHUNK; ++u)
        if (b0 + u < n_local) {
          const float* row = sM + B * B + (bead0 + b0 + u) * B;
          noi[u] = fmaf(row[2 * k2], x0, noi[u]);
          if (2 * k2 + 1 < B) noi[u] = fmaf(row[2 * k2 + 1], x1, noi[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < PILE_CHUNK; ++u)
      if (b0 + u < n_local) {
        const float lang = det[u] + sm * noi[u];
        p_out[(int64_t)(b0 + u) * n3 + t] = CENTROID ? lang + cen : lang;
      }
  }
}


// One multi_step x integration_order Yoshida-Suzuki pass over ONE chain held in registers (thermostats.py:398-468, operation for
// operation): ke = the kinetic term of the chain, dof_kT = degrees of freedom x kB T, m0 / mq = thermostat mass of the innermost /
// every other link.  Returns the factor the momenta are multiplied by.  LMAX bounds the unrolled loops; L <= LMAX.
template <int LMAX>
__device__ __forceinline__ float nhc_propagate(float (&v)[LMAX], float (&f)[LMAX], int L, float ke, float dof_kT, float kT, float m0, float mq,
                                               int multi_step, int order, const YsSteps& ys) {
  f[0] = (ke - dof_kT) / m0;
  float scale = 1.0f;
  for (int ms = 0; ms < multi_step; ++ms) {
    for (int k = 0; k < order; ++k) {
      const float ts = ys.dt[k];
#pragma unroll
      for (int c = 0; c < LMAX; ++c) if (c == L - 1) v[c] += 0.25f * f[c] * ts;            // outermost link
#pragma unroll
      for (int c = LMAX - 2; c >= 0; --c) if (c <= L - 2) {
        const float coeff = expf(-0.125f * ts * v[c + 1]);
        v[c] = v[c] * (coeff * coeff) + 0.25f * f[c] * coeff * ts;
      }
      scale *= expf(-0.5f * ts * v[0]);
      f[0] = (scale * scale * ke - dof_kT) / m0;
#pragma unroll
      for (int c = 0; c < LMAX - 1; ++c) if (c <= L - 2) {
        const float coeff = expf(-0.125f * ts * v[c + 1]);
        v[c] = v[c] * (coeff * coeff) + 0.25f * f[c] * coeff * ts;
        f[c + 1] = ((c == 0 ? m0 : mq) * v[c] * v[c] - kT) / mq;
      }
#pragma unroll
      for (int c = 0; c < LMAX; ++c) if (c == L - 1) v[c] += 0.25f * f[c] * ts;
    }
  }
  return scale;
}

static int check_chain(const char* who, int32_t chain_length, int32_t multi_step, int32_t order, const float* sub_steps, YsSteps* ys) {
  SPK_CHECK_ARG(chain_length >= 1 && chain_length <= kMaxChain, "%s: chain_length must be in [1, %d]", who, kMaxChain);
  SPK_CHECK_ARG(multi_step >= 1, "%s: multi_step must be at least 1", who);
  SPK_CHECK_ARG(order == 1 || order == 3 || order == 5 || order == 7, "%s: integration_order must be 1, 3, 5 or 7", who);
  SPK_CHECK_ARG(sub_steps != nullptr, "%s: null sub-step array", who);
  for (int k = 0; k < kMaxOrder; ++k) ys->dt[k] = k < order ? sub_steps[k] : 0.f;
  return SPK_OK;
}
