// Tensorial output heads (atomistic/atomwise.py:91-293): the gated equivariant MLP (nn/equivariant.py:11-71, nn/blocks.py:79-156) of a
// DipoleMoment / Polarizability head in ONE launch, and the per-molecule moment sums in one more.
//
// One gated equivariant block, s [N, n], v [N, 3, n] -> s' [N, m], v' [N, 3, m] with hidden width g:
//   [V | W] = v Wmix^T            Wmix [2 m, n], no bias, per Cartesian axis
//   Vn      = sqrt(sum_c V_c^2)   (torch.norm over the axis: NO epsilon -- forward only, a zero row gives an exact 0)
//   x       = W2 act(W1 [s | Vn] + b1) + b2        W1 [g, n + m], W2 [2 m, g]
//   s'      = sact(x[:m]),   v'_c = x[m:] * W_c
// The default head, build_gated_equivariant_mlp(n_in = F, n_out = 1, n_layers = 2), is block 0: F -> F/2 (g = F, sact = act) and block 1:
// F/2 -> 1 (g = F/2, no sact).
//
//   k_gated_mlp<F>   one workgroup of four waves per tile of 32 atoms.  The tile of s and v is staged in LDS once (coalesced 16-byte loads); the
//                    three Dense products of block 0 and the hidden layer of block 1 run on v_mfma_f32_32x32x2_f32 (exact fp32 fma chains: the parity
//                    bar is relative and the heads' outputs are sums with cancellation), atoms on the rows, output features on the columns.  Wave w owns
//                    the 32-column tiles w, w + 4, ... of every product; in the vector mix its three accumulators (one per axis) share each weight
//                    operand.  A lane's operand of a k-step is four consecutive k (one 16-byte load: weights straight from L2, activations from LDS),
//                    spent on four instructions -- the two lane halves take k + 0..3 and k + 4..7.  V never leaves the registers (the norm is taken on
//                    the accumulators), W, the hidden layer, s' and v' of block 0 live in LDS only; the width-1 / width-2 products of block 1 are dot
//                    products on the vector unit.  Nothing but s_out [N, 1] and v_out [N, 3, 1] goes to memory.  Rows past N are zero-filled and never
//                    stored.
//   k_moment<KIND>   one wave per molecule; its atom range comes from two binary searches in the ascending idx_m (no row-pointer launch), lanes stride
//                    over the atoms, fixed butterfly: no float atomics, the same inputs give the same bits.  An atom of the range that carries another
//                    molecule index (idx_m not ascending) turns that molecule's outputs into NaN.  A molecule without atoms gives zeros (the
//                    reference's 0 / 0 charge correction of such a molecule is never gathered by an atom).
#include <math.h>
#include "spk_common.h"
#include "spk_mfma_tile.h"

namespace {

constexpr int kGmTile = 32;      // atoms per workgroup = rows of one matrix instruction
constexpr int kGmWaves = 4;
constexpr int kGmPad = 4;        // floats: rows stay 16-byte aligned and start on different banks

template <int F>
struct GmLds {
  static constexpr int H = F / 2;
  static constexpr int LDV = F + kGmPad;          // v tile, hidden layer of block 0
  static constexpr int LDC = F + H + kGmPad;      // [s | Vn]
  static constexpr int LDW = H + kGmPad;          // W -> v', s', hidden layer of block 1
  static constexpr int oV = 0;                                 // [3][32][LDV]; dead after the mix, then:
  static constexpr int oHid = 0;                               //   [32][LDV]
  static constexpr int oS1 = oHid + kGmTile * LDV;             //   [32][LDW]
  static constexpr int oH1 = oS1 + kGmTile * LDW;              //   [32][LDW]
  static constexpr int oCtx = oV + 3 * kGmTile * LDV;          // [32][LDC]
  static constexpr int oW = oCtx + kGmTile * LDC;              // [3][32][LDW]
  static constexpr int oVw = oW + 3 * kGmTile * LDW;           // [6][32]: (V, W) x axis of block 1
  static constexpr int total = oVw + 6 * kGmTile;
  static_assert(oH1 + kGmTile * LDW <= oCtx, "aliases must fit the v tile");
};

struct GmArgs {
  const float *s, *v;
  int64_t N;
  const float *wm0, *w10, *b10, *w20, *b20;       // block 0
  const float *wm1, *w11, *b11, *w21, *b21;       // block 1
  float *s_out, *v_out;
};

// acc[c] += A_c W^T on one 32-column tile: A_c = A + c * plane [32][lda] in LDS, W = 32 rows of ldw floats in memory, K % 8 == 0.
// VEC: the rows of W are 16-byte aligned.
template <int NC, bool VEC>
__device__ __forceinline__ void gm_mm(const float* A, int lda, int plane, const float* __restrict__ W, int ldw, int K, f32x16 (&acc)[NC]) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const float* wrow = W + (size_t)r * ldw + 4 * h;
  const float* arow = A + r * lda + 4 * h;
#pragma unroll 4
  for (int kb = 0; kb < K; kb += 8) {
    f32x4 b;
    if (VEC) b = *(const f32x4*)(wrow + kb);
    else { b.x = wrow[kb]; b.y = wrow[kb + 1]; b.z = wrow[kb + 2]; b.w = wrow[kb + 3]; }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const f32x4 a = *(const f32x4*)(arow + c * plane + kb);
      acc[c] = SPK_MFMA(a.x, b.x, acc[c]);
      acc[c] = SPK_MFMA(a.y, b.y, acc[c]);
      acc[c] = SPK_MFMA(a.z, b.z, acc[c]);
      acc[c] = SPK_MFMA(a.w, b.w, acc[c]);
    }
  }
}
// |(x, y, z)| as ONE chain of explicit fused operations.  Written as x x + y y + z z the sixteen norms of an accumulator were contracted (and packed
// by the SLP vectoriser) differently from register to register, so the last bit of an atom's result depended on its row in the tile.
__device__ __forceinline__ float gm_norm3(float x, float y, float z) { return sqrtf(fmaf(z, z, fmaf(y, y, x * x))); }
// (spk_acc_row(r, hi): row = atom of the tile of accumulator register r in lane half hi; the column is lane & 31)

template <int F, int ACT>
__global__ __launch_bounds__(64 * kGmWaves) void k_gated_mlp(GmArgs a) {
  typedef GmLds<F> L;
  constexpr int H = L::H;
  extern __shared__ __attribute__((aligned(16))) float gm_lds[];
  float* vt = gm_lds + L::oV;
  float* hid = gm_lds + L::oHid;
  float* s1 = gm_lds + L::oS1;
  float* h1 = gm_lds + L::oH1;
  float* ctx = gm_lds + L::oCtx;
  float* wv = gm_lds + L::oW;
  float* vw = gm_lds + L::oVw;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, hi = lane >> 5;
  const int64_t atom0 = (int64_t)blockIdx.x * kGmTile;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  // ---- stage the tile: s -> ctx[:, 0:F], v -> vt[axis][atom][:]
  for (int i = tid; i < kGmTile * (F / 4); i += 64 * kGmWaves) {
    const int row = i / (F / 4), c4 = i % (F / 4);
    const int64_t at = atom0 + row;
    *(f32x4*)(ctx + row * L::LDC + 4 * c4) = at < a.N ? *(const f32x4*)(a.s + at * F + 4 * c4) : zero4;
  }
  for (int i = tid; i < kGmTile * 3 * (F / 4); i += 64 * kGmWaves) {
    const int row = i / (3 * (F / 4)), rem = i % (3 * (F / 4)), ax = rem / (F / 4), c4 = rem % (F / 4);
    const int64_t at = atom0 + row;
    *(f32x4*)(vt + (ax * kGmTile + row) * L::LDV + 4 * c4) = at < a.N ? *(const f32x4*)(a.v + (at * 3 + ax) * F + 4 * c4) : zero4;
  }
  __syncthreads();

  // ---- block 0, vector mix: [V | W] = v Wmix^T per axis; V -> its norm (ctx[:, F:]), W -> LDS
  for (int ct = wave; ct < F / 32; ct += kGmWaves) {
    const int o0 = 32 * ct;
    f32x16 acc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
    gm_mm<3, true>(vt, L::LDV, kGmTile * L::LDV, a.wm0 + (size_t)o0 * F, F, F, acc);
    if (o0 < H) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        ctx[spk_acc_row(r, hi) * L::LDC + F + o0 + col] = gm_norm3(acc[0][r], acc[1][r], acc[2][r]);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) wv[(c * kGmTile + spk_acc_row(r, hi)) * L::LDW + o0 - H + col] = acc[c][r];
    }
  }
  __syncthreads();      // (the v tile is dead from here: hid / s1 / h1 take its place)

  // ---- block 0, scalar net layer 1: hid = act(W1 [s | Vn] + b1)
  for (int ct = wave; ct < F / 32; ct += kGmWaves) {
    const int o0 = 32 * ct;
    f32x16 acc[1];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][r] = 0.f;
    gm_mm<1, true>(ctx, L::LDC, 0, a.w10 + (size_t)o0 * (F + H), F + H, F + H, acc);
    const float b = a.b10[o0 + col];
#pragma unroll
    for (int r = 0; r < 16; ++r) hid[spk_acc_row(r, hi) * L::LDV + o0 + col] = spk_act<ACT>(acc[0][r] + b);
  }
  __syncthreads();

  // ---- block 0, scalar net layer 2: x = W2 hid + b2; s' = act(x[:H]) (sactivation = activation), v'_c = x[H:] W_c (in place)
  for (int ct = wave; ct < F / 32; ct += kGmWaves) {
    const int o0 = 32 * ct;
    f32x16 acc[1];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][r] = 0.f;
    gm_mm<1, true>(hid, L::LDV, 0, a.w20 + (size_t)o0 * F, F, F, acc);
    const float b = a.b20[o0 + col];
    if (o0 < H) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s1[spk_acc_row(r, hi) * L::LDW + o0 + col] = spk_act<ACT>(acc[0][r] + b);
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float g = acc[0][r] + b;
#pragma unroll
        for (int c = 0; c < 3; ++c) wv[(c * kGmTile + spk_acc_row(r, hi)) * L::LDW + o0 - H + col] *= g;
      }
    }
  }
  __syncthreads();

  // ---- block 1, vector mix (two output rows): vw[2 axis + which][atom] = v'_axis[atom] . Wmix1[which]
  if (tid < 6 * kGmTile) {
    const int at = tid & 31, q = tid >> 5, ax = q >> 1, which = q & 1;
    const float* x = wv + (ax * kGmTile + at) * L::LDW;
    const float* w = a.wm1 + which * H;
    float d = 0.f;
#pragma unroll 8
    for (int o = 0; o < H; ++o) d = fmaf(x[o], w[o], d);
    vw[q * kGmTile + at] = d;
  }
  __syncthreads();

  // ---- block 1, scalar net layer 1: h1 = act(W1 [s' | Vn'] + b1), W1 [H, H + 1]: the matrix part over s', the norm column in the epilogue
  for (int ct = wave; ct < H / 32; ct += kGmWaves) {
    const int o0 = 32 * ct;
    f32x16 acc[1];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][r] = 0.f;
    gm_mm<1, false>(s1, L::LDW, 0, a.w11 + (size_t)o0 * (H + 1), H + 1, H, acc);
    const float b = a.b11[o0 + col], wn = a.w11[(size_t)(o0 + col) * (H + 1) + H];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int at = spk_acc_row(r, hi);
      const float v0 = vw[at], v1 = vw[2 * kGmTile + at], v2 = vw[4 * kGmTile + at];
      h1[at * L::LDW + o0 + col] = spk_act<ACT>(fmaf(wn, gm_norm3(v0, v1, v2), acc[0][r]) + b);
    }
  }
  __syncthreads();

  // ---- block 1, scalar net layer 2 (two output rows, no scalar activation) and the gate
  if (tid < 2 * kGmTile) {
    const int at = tid & 31, k = tid >> 5;
    const float* x = h1 + at * L::LDW;
    const float* w = a.w21 + k * H;
    float d = 0.f;
#pragma unroll 8
    for (int o = 0; o < H; ++o) d = fmaf(x[o], w[o], d);
    d += a.b21[k];
    const int64_t g = atom0 + at;
    if (g < a.N) {
      if (k == 0) a.s_out[g] = d;
      else {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.v_out[3 * g + c] = d * vw[(2 * c + 1) * kGmTile + at];
      }
    }
  }
}

template <int F, int ACT>
int launch_gated_mlp(const GmArgs& a, hipStream_t stream) {
  const size_t lds = sizeof(float) * (size_t)GmLds<F>::total;
  auto kern = k_gated_mlp<F, ACT>;
  static SpkPerDevice attr_set;
  int attr_dev;
  if (attr_set.pending(&attr_dev)) {
    SPK_HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr_set.mark(attr_dev);
  }
  const int64_t ntiles = (a.N + kGmTile - 1) / kGmTile;
  SpkProfScope prof("gated_mlp", stream);
  hipLaunchKernelGGL(kern, dim3((unsigned)ntiles), dim3(64 * kGmWaves), lds, stream, a);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

// ------------------------------------------------------------------------------------------------ per-molecule moments
// first index in [0, n) whose entry is >= key (idx ascending)
__device__ __forceinline__ int64_t mo_lower_bound(const int64_t* __restrict__ idx, int64_t n, int64_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (idx[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

struct MoArgs {
  const float *q, *d, *R, *total;      // q [N]: charges (dipole) or isotropic part (polarizability); d [N, 3] or NULL; total [n_mol] or NULL
  const int64_t* idx_m;
  int64_t N, n_mol;
  int correct;
  float *out, *q_out;                  // out [n_mol, 3] (dipole) or [n_mol, 3, 3]; q_out [N] or NULL
};

// KIND 0: dipole moment, 1: polarizability
template <int KIND>
__global__ __launch_bounds__(256) void k_moment(MoArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t m = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  if (m >= a.n_mol) return;                          // uniform over the wave
  const int64_t a0 = mo_lower_bound(a.idx_m, a.N, m), a1 = mo_lower_bound(a.idx_m, a.N, m + 1);
  const float nan = __int_as_float(0x7fc00000);
  float bad = 0.f;
  if (KIND == 0) {
    float corr = 0.f;
    if (a.correct && a1 > a0) {
      float sq = 0.f;
      for (int64_t i = a0 + lane; i < a1; i += 64) sq += a.q[i];
      sq = spk_wave_sum(sq);
      corr = ((a.total ? a.total[m] : 0.f) - sq) / (float)(a1 - a0);
    }
    float mu[3] = {0.f, 0.f, 0.f};
    for (int64_t i = a0 + lane; i < a1; i += 64) {
      if (a.idx_m[i] != m) bad = 1.f;
      const float qc = a.q[i] + corr;
      if (a.q_out) a.q_out[i] = qc;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float t = qc * a.R[3 * i + c];
        if (a.d) t += a.d[3 * i + c];
        mu[c] += t;
      }
    }
    bad = spk_wave_max(bad);
#pragma unroll
    for (int c = 0; c < 3; ++c) mu[c] = spk_wave_sum(mu[c]);
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) a.out[3 * m + c] = bad != 0.f ? nan : mu[c];
    }
  } else {
    // alpha = sum_i a0_i 1 + d_i R_i^T + R_i d_i^T: the six distinct entries are summed, the mirror image is a copy (alpha == alpha^T to the bit)
    float s[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // xx, yy, zz, xy, xz, yz
    for (int64_t i = a0 + lane; i < a1; i += 64) {
      if (a.idx_m[i] != m) bad = 1.f;
      const float iso = a.q[i];
      const float dx = a.d[3 * i], dy = a.d[3 * i + 1], dz = a.d[3 * i + 2];
      const float x = a.R[3 * i], y = a.R[3 * i + 1], z = a.R[3 * i + 2];
      s[0] += iso + 2.f * (dx * x);
      s[1] += iso + 2.f * (dy * y);
      s[2] += iso + 2.f * (dz * z);
      s[3] += dx * y + x * dy;
      s[4] += dx * z + x * dz;
      s[5] += dy * z + y * dz;
    }
    bad = spk_wave_max(bad);
#pragma unroll
    for (int k = 0; k < 6; ++k) s[k] = spk_wave_sum(s[k]);
    if (lane == 0) {
      if (bad != 0.f) {
#pragma unroll
        for (int k = 0; k < 6; ++k) s[k] = nan;
      }
      float* o = a.out + 9 * m;
      o[0] = s[0]; o[1] = s[3]; o[2] = s[4];
      o[3] = s[3]; o[4] = s[1]; o[5] = s[5];
      o[6] = s[4]; o[7] = s[5]; o[8] = s[2];
    }
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int spk_gated_mlp_supported(int32_t n_in, int32_t n_layers, int32_t act) {
  return ((n_in == 64 || n_in == 128) && n_layers == 2 && act == SPK_ACT_SILU) ? 1 : 0;
}

extern "C" int spk_gated_mlp_fwd_f32(const float* s, const float* v, int64_t N, int32_t n_in, int32_t n_layers, int32_t act,
                                     const float* const* host_weights, float* s_out, float* v_out, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "spk_gated_mlp_fwd_f32";
  SPK_CHECK_ARG(spk_gated_mlp_supported(n_in, n_layers, act), "%s: head n_in = %d, n_layers = %d, act = %d is not covered (spk_gated_mlp_supported)", who,
                (int)n_in, (int)n_layers, (int)act);
  SPK_CHECK_ARG(N >= 0 && N < (1LL << 31) * kGmTile, "%s: bad atom count", who);
  if (N == 0) return SPK_OK;
  SPK_CHECK_ARG(s && v && host_weights && s_out && v_out, "%s: null argument", who);
  for (int k = 0; k < 10; ++k) SPK_CHECK_ARG(host_weights[k] != nullptr, "%s: null weight %d", who, k);
  GmArgs a;
  a.s = s; a.v = v; a.N = N;
  a.wm0 = host_weights[0]; a.w10 = host_weights[1]; a.b10 = host_weights[2]; a.w20 = host_weights[3]; a.b20 = host_weights[4];
  a.wm1 = host_weights[5]; a.w11 = host_weights[6]; a.b11 = host_weights[7]; a.w21 = host_weights[8]; a.b21 = host_weights[9];
  a.s_out = s_out; a.v_out = v_out;
  SPK_CHECK_ARG(aligned16(s) && aligned16(v) && aligned16(a.wm0) && aligned16(a.w10) && aligned16(a.w20),
                "%s: s, v and the block-0 weight matrices must be 16-byte aligned", who);
  if (n_in == 128) return launch_gated_mlp<128, SPK_ACT_SILU>(a, stream);
  return launch_gated_mlp<64, SPK_ACT_SILU>(a, stream);
}

extern "C" int spk_moment_reduce_f32(int32_t kind, const float* q, const float* d, const float* R, const int64_t* idx_m, int64_t N, int64_t n_mol,
                                     const float* total_charge, int32_t correct, float* out, float* q_out, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "spk_moment_reduce_f32";
  SPK_CHECK_ARG(kind == SPK_MOMENT_DIPOLE || kind == SPK_MOMENT_POLARIZABILITY, "%s: kind must be SPK_MOMENT_DIPOLE or SPK_MOMENT_POLARIZABILITY", who);
  SPK_CHECK_ARG(N >= 0 && n_mol >= 0 && n_mol < (1LL << 31), "%s: bad sizes", who);
  if (n_mol == 0) return SPK_OK;
  SPK_CHECK_ARG(out && (N == 0 || (q && R && idx_m)), "%s: null argument", who);
  SPK_CHECK_ARG(kind == SPK_MOMENT_DIPOLE || N == 0 || d, "%s: the polarizability needs the atomic vectors d", who);
  MoArgs a;
  a.q = q; a.d = d; a.R = R; a.total = total_charge; a.idx_m = idx_m; a.N = N; a.n_mol = n_mol; a.correct = correct ? 1 : 0;
  a.out = out; a.q_out = kind == SPK_MOMENT_DIPOLE ? q_out : nullptr;
  SpkProfScope prof("moment_reduce", stream);
  const dim3 grid(spk_grid_for(n_mol * 64, 256, 1 << 30));
  if (kind == SPK_MOMENT_DIPOLE) hipLaunchKernelGGL((k_moment<0>), grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL((k_moment<1>), grid, dim3(256), 0, stream, a);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}
