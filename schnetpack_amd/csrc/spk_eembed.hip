// Electronic embedding (nn/embedding.py:239-349, nn/blocks.py:159-296): the attention-like block that spreads a molecule's total charge or spin
// multiplicity psi_m over its atoms, forward only, in THREE launches.
//
//   e_m = (relu(psi), relu(-psi)) (charge) or |psi| (spin),  e^_m = e_m / max(e_m, 1),  k_m = W_k e^_m,  v_m = W_v e_m
//   w_i = k_m(i) . (W_q x_i + b_q) / sqrt(F)
//   a_i = softmax_{all atoms of the batch}(w)_i / (sum_{j in m(i)} softmax(w)_j + eps)          (the reference: its result depends on the batch)
//       = exp(w_i - M_m) / (S_m + eps Z exp(M - M_m))       M_m = max_{i in m} w_i, S_m = sum_{i in m} exp(w_i - M_m), M = max_m M_m,
//                                                            Z = sum_i exp(w_i - M)        (the same quantity, per molecule and without overflow;
//                                                            where the eps term overflows a_i = 0: there the reference's softmax underflows)
//   y_i = a_i v_m;  per residual block y <- y + W2 act(W1 act(y));  out = W_L act(y)  (no biases);  with add_input the result is x + out.
//
//   k_ee_logit   a workgroup per chunk of 64 atoms, sixteen lanes per atom (16-byte loads of x).  q_i is never formed: w_i = e^_m . (A^T x_i + c) with A = W_q^T W_k / sqrt(F)
//                [F, n_e] and c = W_k^T b_q / sqrt(F), which every workgroup builds in LDS (F n_e dot products of length F out of L2).  Writes w [N]
//                and the chunk's (max, sum exp) by one fixed butterfly.
//   k_ee_stats   a wave per molecule: (M, Z) from the chunk partials (every wave, the same order), its atom range from two bisections of the
//                ascending idx_m (side by side, scalar loads), then M_m, S_m by butterflies.  Writes (M_m, denominator) and the range.  An atom of the range that carries another
//                molecule index turns the denominator into NaN.
//   k_ee_stack   a workgroup of four waves per tile of 32 atoms, modelled on k_gated_mlp: y = a v staged in LDS next to act(y); every F x F
//                product on v_mfma_f32_32x32x2_f32 (exact fp32 chains), atoms on the rows, wave w owns the column tiles w, w + 4, ...; weights by
//                16-byte loads out of L2, accumulators in registers across the barriers, intermediates in LDS only.  Rows >= N are never stored.
//
// No float atomics, no host synchronisation, no allocation: the same inputs give the same bits, and the call can be captured.  An idx_m entry
// outside [0, n_mol) is never used as an address; such an atom, an atom outside the range its molecule was found at, and every atom of a molecule
// whose range holds a foreign atom receive NaN.  A molecule without atoms writes nothing.  psi = 0 gives exact zeros.
#include <math.h>
#include "spk_common.h"
#include "spk_mfma_tile.h"

namespace {

constexpr int kEeChunk = 64;      // atoms per workgroup of k_ee_logit = entries per partial
constexpr int kEeTile = 32;       // atoms per workgroup of k_ee_stack = rows of one matrix instruction
constexpr int kEeWaves = 4;
constexpr int kEePad = 4;         // floats: rows stay 16-byte aligned and start on different banks
constexpr int kEeMaxRes = 4;
constexpr int kEeMaxF = 256;

struct EeArgs {
  const float *x, *psi;
  const int64_t* idx_m;
  int64_t N, n_mol;
  int F, n_res, n_e, add_input;
  float eps;
  const float *wq, *bq, *wk, *wv, *wl;
  const float *w1[kEeMaxRes], *w2[kEeMaxRes];
  float *w, *partial, *molstat;      // workspace: logits [N], (max, sum exp) per chunk, (M_m, denominator) per molecule
  int64_t* range;                    //            [n_mol][2]
  float* out;
};

__device__ __forceinline__ void ee_features(float psi, int n_e, float (&e)[2]) {
  if (n_e == 2) { e[0] = fmaxf(psi, 0.f); e[1] = fmaxf(-psi, 0.f); }
  else { e[0] = fabsf(psi); e[1] = 0.f; }
}

// The first activation acts on y ~ v / n_atoms, and max(x, 0) + log(1 + exp(-|x|)) - ln 2 loses RELATIVE precision near zero (an absolute error of
// an ulp of ln 2 on a value of x / 2).  Near zero: ssp(x) = x / 2 + log cosh(x / 2) by its series (|x| < 1/2: the u^12 term is below 1e-8 of u^2 / 2).
template <int ACT>
__device__ __forceinline__ float ee_act(float x) {
  if (ACT == SPK_ACT_SSP) {
    if (fabsf(x) < 0.5f) {
      const float u = 0.5f * x, u2 = u * u;
      const float p = fmaf(u2, fmaf(u2, fmaf(u2, fmaf(u2, 31.f / 14175.f, -17.f / 2520.f), 1.f / 45.f), -1.f / 12.f), 0.5f);
      return fmaf(u2, p, u);
    }
    return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))) - SPK_LN2_F;
  }
  return x / (1.0f + expf(-x));
}

__global__ __launch_bounds__(256) void k_ee_logit(EeArgs a) {
  __shared__ __attribute__((aligned(16))) float A[2 * kEeMaxF];
  __shared__ float cvec[2];
  __shared__ float wl[kEeChunk];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, F = a.F, ne = a.n_e;
  const float scale = 1.0f / sqrtf((float)F);
  if (tid < F) {
    float s0 = 0.f, s1 = 0.f;
#pragma unroll 32
    for (int g = 0; g < F; ++g) {      // (F % 32 == 0: 32 independent loads of a column of W_q in flight)
      const float q = a.wq[(size_t)g * F + tid];
      s0 = fmaf(q, a.wk[g * ne], s0);
      if (ne == 2) s1 = fmaf(q, a.wk[g * ne + 1], s1);
    }
    A[2 * tid] = s0 * scale;
    A[2 * tid + 1] = s1 * scale;
  }
  if (tid >= 254) {      // (the last two lanes: F may be as wide as the workgroup)
    const int e = tid - 254;
    float s = 0.f;
    if (e < ne)
      for (int g = 0; g < F; ++g) s = fmaf(a.wk[g * ne + e], a.bq[g], s);
    cvec[e] = s * scale;
  }
  __syncthreads();
  // sixteen lanes per atom, four atoms per wave and step, four steps: the loads of a step do not wait for one another
  const int q = lane >> 4, l16 = lane & 15;
  const int64_t base = (int64_t)blockIdx.x * kEeChunk;
  const float ninf = -INFINITY;
  float p0[4] = {0.f, 0.f, 0.f, 0.f}, p1[4] = {0.f, 0.f, 0.f, 0.f};
  for (int f = 4 * l16; f < F; f += 64) {
    const f32x4 a0 = *(const f32x4*)(A + 2 * f), a1 = *(const f32x4*)(A + 2 * f + 4);      // (A[f][0], A[f][1], A[f+1][0], ...)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int64_t i = base + 16 * wave + 4 * t + q;
      const f32x4 xv = i < a.N ? *(const f32x4*)(a.x + i * F + f) : f32x4{0.f, 0.f, 0.f, 0.f};
      p0[t] = fmaf(xv.w, a1.z, fmaf(xv.z, a1.x, fmaf(xv.y, a0.z, fmaf(xv.x, a0.x, p0[t]))));
      p1[t] = fmaf(xv.w, a1.w, fmaf(xv.z, a1.y, fmaf(xv.y, a0.w, fmaf(xv.x, a0.y, p1[t]))));
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) {
      p0[t] += __shfl_xor(p0[t], off, 64);
      p1[t] += __shfl_xor(p1[t], off, 64);
    }
    const int local = 16 * wave + 4 * t + q;
    const int64_t i = base + local;
    float wi = ninf;
    if (i < a.N) {
      const int64_t m = a.idx_m[i];
      if (m >= 0 && m < a.n_mol) {
        float e[2];
        ee_features(a.psi[m], ne, e);
        wi = (e[0] / fmaxf(e[0], 1.f)) * (p0[t] + cvec[0]);
        if (ne == 2) wi = fmaf(e[1] / fmaxf(e[1], 1.f), p1[t] + cvec[1], wi);
      }
    }
    if (l16 == 0) {
      wl[local] = wi;
      if (i < a.N) a.w[i] = wi;
    }
  }
  __syncthreads();
  if (wave == 0) {      // the chunk's (max, sum exp), one fixed butterfly
    const float mine = wl[lane];
    const float mx = spk_wave_max(mine);
    const float sm = spk_wave_sum(mine > ninf ? expf(mine - mx) : 0.f);
    if (lane == 0) {
      a.partial[2 * blockIdx.x] = mx;
      a.partial[2 * blockIdx.x + 1] = sm;
    }
  }
}

// [a0, a1) = the first indices in [0, n) whose entries are >= m and >= m + 1 (idx ascending): two bisections, step by step side by side so that
// their loads overlap.  m is the same on every lane and handed over in a scalar register: the probes are scalar loads.
__device__ __forceinline__ void ee_range(const int64_t* __restrict__ idx, int64_t n, int64_t m, int64_t& a0, int64_t& a1) {
  int64_t lo0 = 0, hi0 = n, lo1 = 0, hi1 = n;
  while (lo0 < hi0 || lo1 < hi1) {
    if (lo0 < hi0) {
      const int64_t mid = lo0 + ((hi0 - lo0) >> 1);
      if (idx[mid] < m) lo0 = mid + 1; else hi0 = mid;
    }
    if (lo1 < hi1) {
      const int64_t mid = lo1 + ((hi1 - lo1) >> 1);
      if (idx[mid] <= m) lo1 = mid + 1; else hi1 = mid;
    }
  }
  a0 = lo0;
  a1 = lo1;
}

__global__ __launch_bounds__(256) void k_ee_stats(EeArgs a, int64_t n_chunks) {
  const int lane = threadIdx.x & 63;
  const int64_t m = (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (m >= a.n_mol) return;                          // uniform over the wave
  const float ninf = -INFINITY;
  // the batch: M = max_i w_i, Z = sum_i exp(w_i - M)
  float M = ninf;
  for (int64_t c = lane; c < n_chunks; c += 64) M = fmaxf(M, a.partial[2 * c]);
  M = spk_wave_max(M);
  float Z = 0.f;
  for (int64_t c = lane; c < n_chunks; c += 64) {
    const float mc = a.partial[2 * c];
    if (mc > ninf) Z += a.partial[2 * c + 1] * expf(mc - M);
  }
  Z = spk_wave_sum(Z);
  // the molecule
  int64_t a0, a1;
  ee_range(a.idx_m, a.N, m, a0, a1);
  float Mm = ninf, bad = 0.f;
  for (int64_t i = a0 + lane; i < a1; i += 64) {
    if (a.idx_m[i] != m) bad = 1.f;
    Mm = fmaxf(Mm, a.w[i]);
  }
  Mm = spk_wave_max(Mm);
  bad = spk_wave_max(bad);
  float S = 0.f;
  for (int64_t i = a0 + lane; i < a1; i += 64) S += expf(a.w[i] - Mm);
  S = spk_wave_sum(S);
  if (lane == 0) {
    float D = S;
    if (a.eps != 0.f) D += a.eps * Z * expf(M - Mm);      // inf where the term overflows: the atoms' weights are 0 there
    if (bad != 0.f) D = __int_as_float(0x7fc00000);
    a.molstat[2 * m] = Mm;
    a.molstat[2 * m + 1] = D;
    a.range[2 * m] = a0;
    a.range[2 * m + 1] = a1;
  }
}

// acc += A W^T on one 32-column tile: A [32][lda] in LDS, W = 32 rows of K floats in memory (16-byte aligned), K % 32 == 0.  A lane's operand of a
// k-step is four consecutive k, spent on four instructions; the two lane halves take k + 0..3 and k + 4..7 (the scheme of k_gated_mlp).  K is a
// run-time value here, so the weight loads are pipelined by hand: the four 16-byte loads of the next 32 k are in flight under the sixteen matrix
// instructions of the current ones.
__device__ __forceinline__ void ee_mm(const float* A, int lda, const float* __restrict__ W, int K, f32x16& acc) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const float* wrow = W + (size_t)r * K + 4 * h;
  const float* arow = A + r * lda + 4 * h;
  f32x4 b[4], bn[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) b[u] = *(const f32x4*)(wrow + 8 * u);
  for (int kb = 0; kb < K; kb += 32) {
    const int kn = kb + 32 < K ? kb + 32 : kb;      // (the last group reloads itself: no branch around the loads)
#pragma unroll
    for (int u = 0; u < 4; ++u) bn[u] = *(const f32x4*)(wrow + kn + 8 * u);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const f32x4 x = *(const f32x4*)(arow + kb + 8 * u);
      acc = SPK_MFMA(x.x, b[u].x, acc);
      acc = SPK_MFMA(x.y, b[u].y, acc);
      acc = SPK_MFMA(x.z, b[u].z, acc);
      acc = SPK_MFMA(x.w, b[u].w, acc);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) b[u] = bn[u];
  }
}
// (spk_acc_row(r, hi): row = atom of the tile of accumulator register r in lane half hi; the column is lane & 31)

// NT: column tiles per wave (F <= 128 NT: 1, else 2)
template <int NT, int ACT>
__global__ __launch_bounds__(64 * kEeWaves) void k_ee_stack(EeArgs a) {
  extern __shared__ __attribute__((aligned(16))) float ee_lds[];
  const int F = a.F, ld = F + kEePad, nct = F / 32;
  float* Y = ee_lds;                        // [32][ld]  y
  float* B = Y + kEeTile * ld;              // [32][ld]  act(y), then the hidden layer of a block
  float* rowv = B + kEeTile * ld;           // [3][32]   a_i, e_0, e_1 of the row's molecule
  int* rowk = (int*)(rowv + 3 * kEeTile);   // [32]      0: past N, 1: regular, 2: neutral (exact zeros), 3: NaN
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, hi = lane >> 5;
  const int64_t atom0 = (int64_t)blockIdx.x * kEeTile;
  const float nan = __int_as_float(0x7fc00000);

  if (tid < kEeTile) {
    const int64_t g = atom0 + tid;
    int kind = 0;
    float al = 0.f, e[2] = {0.f, 0.f};
    if (g < a.N) {
      const int64_t m = a.idx_m[g];
      kind = 3;
      if (m >= 0 && m < a.n_mol && g >= a.range[2 * m] && g < a.range[2 * m + 1]) {
        const float D = a.molstat[2 * m + 1];
        if (D == D) {
          ee_features(a.psi[m], a.n_e, e);
          al = expf(a.w[g] - a.molstat[2 * m]) / D;
          kind = (e[0] == 0.f && e[1] == 0.f) ? 2 : 1;
        }
      }
    }
    rowv[tid] = al; rowv[kEeTile + tid] = e[0]; rowv[2 * kEeTile + tid] = e[1];
    rowk[tid] = kind;
  }
  __syncthreads();

  // ---- stage y = a v and act(y)
  for (int i = tid; i < kEeTile * F; i += 64 * kEeWaves) {
    const int row = i / F, c = i - row * F;
    const int kind = rowk[row];
    float y = 0.f;
    if (kind == 1) {
      float v = a.wv[c * a.n_e] * rowv[kEeTile + row];
      if (a.n_e == 2) v = fmaf(a.wv[c * 2 + 1], rowv[2 * kEeTile + row], v);
      y = rowv[row] * v;
    } else if (kind == 3) {
      y = nan;
    }
    Y[row * ld + c] = y;
    B[row * ld + c] = ee_act<ACT>(y);
  }
  __syncthreads();

  f32x16 acc[NT];
  for (int b = 0; b < a.n_res; ++b) {
    // hidden = act(W1 act(y))
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int ct = wave + kEeWaves * t;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
      if (ct < nct) ee_mm(B, ld, a.w1[b] + (size_t)(32 * ct) * F, F, acc[t]);
    }
    __syncthreads();      // every wave has read act(y)
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int ct = wave + kEeWaves * t;
      if (ct < nct) {
#pragma unroll
        for (int r = 0; r < 16; ++r) B[spk_acc_row(r, hi) * ld + 32 * ct + col] = ee_act<ACT>(acc[t][r]);
      }
    }
    __syncthreads();
    // y += W2 hidden
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int ct = wave + kEeWaves * t;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
      if (ct < nct) ee_mm(B, ld, a.w2[b] + (size_t)(32 * ct) * F, F, acc[t]);
    }
    __syncthreads();      // every wave has read the hidden layer
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int ct = wave + kEeWaves * t;
      if (ct < nct) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int o = spk_acc_row(r, hi) * ld + 32 * ct + col;
          const float y = Y[o] + acc[t][r];
          Y[o] = y;
          B[o] = ee_act<ACT>(y);
        }
      }
    }
    __syncthreads();
  }

  // ---- out = W_L act(y) (+ x)
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int ct = wave + kEeWaves * t;
    if (ct < nct) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
      ee_mm(B, ld, a.wl + (size_t)(32 * ct) * F, F, acc[t]);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = spk_acc_row(r, hi);
        const int64_t g = atom0 + row;
        if (g < a.N) {
          const int kind = rowk[row];
          const size_t o = (size_t)g * F + 32 * ct + col;
          float v = kind == 2 ? 0.f : acc[t][r];      // (no biases and act(0) = 0: a neutral molecule's rows are exactly zero)
          if (a.add_input) v += a.x[o];
          a.out[o] = v;
        }
      }
    }
  }
}

size_t ee_stack_lds(int F) { return sizeof(float) * (size_t)(2 * kEeTile * (F + kEePad) + 4 * kEeTile); }

template <int NT, int ACT>
int launch_ee_stack(const EeArgs& a, hipStream_t stream) {
  const size_t lds = ee_stack_lds(a.F), lds_max = ee_stack_lds(kEeMaxF);
  auto kern = k_ee_stack<NT, ACT>;
  static SpkPerDevice attr_set;
  int attr_dev;
  if (attr_set.pending(&attr_dev)) {
    SPK_HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
    attr_set.mark(attr_dev);
  }
  const int64_t ntiles = (a.N + kEeTile - 1) / kEeTile;
  SpkProfScope prof("eembed_stack", stream);
  hipLaunchKernelGGL(kern, dim3((unsigned)ntiles), dim3(64 * kEeWaves), lds, stream, a);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

bool ee_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
int64_t ee_align(int64_t b) { return (b + 255) & ~(int64_t)255; }
int64_t ee_chunks(int64_t N) { return (N + kEeChunk - 1) / kEeChunk; }

}  // namespace

extern "C" int spk_eembed_supported(int32_t F, int32_t n_residual, int32_t act) {
  return (F >= 32 && F <= kEeMaxF && F % 32 == 0 && n_residual >= 0 && n_residual <= kEeMaxRes && (act == SPK_ACT_SSP || act == SPK_ACT_SILU)) ? 1 : 0;
}

extern "C" int64_t spk_eembed_lds_bytes(int32_t F) { return (F >= 32 && F <= kEeMaxF && F % 32 == 0) ? (int64_t)ee_stack_lds(F) : -1; }

extern "C" int64_t spk_eembed_workspace_bytes(int64_t N, int64_t n_mol) {
  if (N < 0 || n_mol < 0) return -1;
  return ee_align(4 * N) + ee_align(8 * ee_chunks(N)) + ee_align(8 * n_mol) + ee_align(16 * n_mol);
}

extern "C" int spk_eembed_fwd_f32(const float* x, const float* psi, const int64_t* idx_m, int64_t N, int64_t n_mol, int32_t F, int32_t n_residual,
                                  int32_t act, int32_t is_charged, float eps, int32_t add_input, const float* const* host_weights, float* out,
                                  void* workspace, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "spk_eembed_fwd_f32";
  SPK_CHECK_ARG(spk_eembed_supported(F, n_residual, act), "%s: F = %d, n_residual = %d, act = %d is not covered (spk_eembed_supported)", who, (int)F,
                (int)n_residual, (int)act);
  SPK_CHECK_ARG(N >= 0 && N < (1LL << 31) * kEeTile && n_mol >= 0 && n_mol < (1LL << 31), "%s: bad sizes", who);
  if (N == 0) return SPK_OK;
  SPK_CHECK_ARG(n_mol > 0, "%s: atoms without molecules", who);
  SPK_CHECK_ARG(x && psi && idx_m && host_weights && out && workspace, "%s: null argument", who);
  const int nw = 5 + 2 * n_residual;
  for (int k = 0; k < nw; ++k) SPK_CHECK_ARG(host_weights[k] != nullptr, "%s: null weight %d", who, k);
  EeArgs a;
  a.x = x; a.psi = psi; a.idx_m = idx_m; a.N = N; a.n_mol = n_mol; a.F = F; a.n_res = n_residual; a.n_e = is_charged ? 2 : 1; a.add_input = add_input ? 1 : 0;
  a.eps = eps;
  a.wq = host_weights[0]; a.bq = host_weights[1]; a.wk = host_weights[2]; a.wv = host_weights[3];
  for (int b = 0; b < kEeMaxRes; ++b) {
    a.w1[b] = b < n_residual ? host_weights[4 + 2 * b] : nullptr;
    a.w2[b] = b < n_residual ? host_weights[5 + 2 * b] : nullptr;
    SPK_CHECK_ARG(ee_aligned16(a.w1[b]) && ee_aligned16(a.w2[b]), "%s: the weight matrices must be 16-byte aligned", who);
  }
  a.wl = host_weights[4 + 2 * n_residual];
  SPK_CHECK_ARG(ee_aligned16(a.wl) && ee_aligned16(workspace) && ee_aligned16(x), "%s: x, the weight matrices and the workspace must be 16-byte aligned", who);
  char* ws = (char*)workspace;
  const int64_t n_chunks = ee_chunks(N);
  a.w = (float*)ws; ws += ee_align(4 * N);
  a.partial = (float*)ws; ws += ee_align(8 * n_chunks);
  a.molstat = (float*)ws; ws += ee_align(8 * n_mol);
  a.range = (int64_t*)ws;
  a.out = out;
  {
    SpkProfScope prof("eembed_logit", stream);
    hipLaunchKernelGGL(k_ee_logit, dim3((unsigned)n_chunks), dim3(256), 0, stream, a);
    SPK_LAUNCH_CHECK();
  }
  {
    SpkProfScope prof("eembed_stats", stream);
    hipLaunchKernelGGL(k_ee_stats, dim3(spk_grid_for(n_mol * 64, 256, 1 << 30)), dim3(256), 0, stream, a, n_chunks);
    SPK_LAUNCH_CHECK();
  }
  if (F <= 128) return act == SPK_ACT_SSP ? launch_ee_stack<1, SPK_ACT_SSP>(a, stream) : launch_ee_stack<1, SPK_ACT_SILU>(a, stream);
  return act == SPK_ACT_SSP ? launch_ee_stack<2, SPK_ACT_SSP>(a, stream) : launch_ee_stack<2, SPK_ACT_SILU>(a, stream);
}
