// SO(3)-equivariant layers of SO3net (nn/so3.py:18-307 of the reference; representation/so3net.py): real spherical harmonics, the
// Clebsch-Gordan convolution over a neighbour list and the Clebsch-Gordan tensor product, forward and first-order backward, float32.
// Combined index s = l^2 + l + m, S = (lmax + 1)^2, lmax 1..3; features F a multiple of 32 up to 256.
//
//   y[i,s,f] = sum_{p in row i} sum_{(s1,s2)->s} C  (Y[p,s1] fcut[p])  W[p,l(s1),f]  x[j(p),s2,f]          (convolution; W [P, (lmax+1) F])
//   y[n,s,f] = sum_{(s1,s2)->s} C  x1[n,s1,f]  x2[n,s2,f]                                                  (tensor product)
//
// The filter W is materialised by the caller (a Dense layer); the [P, n_cg, F] products of the reference never are.  The Clebsch-Gordan
// contraction is straight-line code from the compiled-in table (spk_so3_tables.h: 10 / 83 / 353 non-zeros, two vector instructions each), all
// operands in registers: 3 S + lmax + 1 live values per lane, no LDS, no scratch.
//
//   k_so3_conv<L, 0>   a wavefront per (centre atom, 64-feature slice), lanes over features, walks the CSR row in list order with S
//                      accumulators; Y and fcut of the pair are wave-uniform reads.  Rows without neighbours write zeros.  No atomics.
//   k_so3_conv<L, 1>   the same walk for gx: row j reads Y, fcut, W at rev[p] (the edge i <- j of its own edge j <- i) and gy at the neighbour,
//                      gx[j,s2,f] = sum C a[s1] gy[i,s,f].  rev is a bijection between row j and the edges that point at j (every image of a
//                      pair, i = j images included, has its own reverse edge: spk_edge_plan matches (j <- i, -r)), so nothing is counted twice.
//   k_so3_edge<L>      per (row i, slice): t[s1,f] = sum C x[j,s2,f] gy[i,s,f] per pair; writes gW[p,l,f] = fcut sum_{s1 in l} Y[s1] t[s1,f] and
//                      the slice's share of gYeff[p,s1] = sum_f W[l(s1),f] t[s1,f] (butterfly over the 64 lanes, fixed order).
//   k_so3_edge_fin     per pair: adds the slices in slice order, gY = fcut gYeff, gfcut = sum_s1 Y[s1] gYeff[s1].
//   k_so3_prod_fwd / _bwd   a wavefront per (atom, slice).
//   k_rsh_fwd / _bwd   a pair per lane: Y_lm = N_l Pi_l^|m|(z) AB_m(x, y) as closed polynomials with x, y, z independent (the module does not
//                      normalise), and the exact derivative of that polynomial.
// The same inputs give the same bits on every call.  Indices outside the atoms / pairs are clamped for the read.
#include <math.h>
#include "spk_common.h"
#include "spk_so3_tables.h"

namespace {

constexpr int kSo3MaxF = 256;

__host__ __device__ constexpr int so3_l_of(int s) { return s == 0 ? 0 : (s < 4 ? 1 : (s < 9 ? 2 : 3)); }

// the table of LMAX applied to a statement macro X(s1, s2, s, C)
#define SO3_CG_APPLY(LMAX, X)                 \
  do {                                        \
    if constexpr ((LMAX) == 1) { SPK_SO3_CG_L1(X) }      \
    else if constexpr ((LMAX) == 2) { SPK_SO3_CG_L2(X) } \
    else { SPK_SO3_CG_L3(X) }                 \
  } while (0)

struct So3Unit { int64_t row; int f; bool live; bool any; };

// wave -> (row, 64-feature slice); rows * nsl units, four per block
__device__ __forceinline__ So3Unit so3_unit(int64_t rows, int F, int nsl) {
  So3Unit u;
  const int64_t unit = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // in a scalar register
  u.any = unit < rows * nsl;
  u.row = u.any ? unit / nsl : 0;
  const int sl = u.any ? (int)(unit % nsl) : 0;
  u.f = sl * 64 + (threadIdx.x & 63);
  u.live = u.any && u.f < F;
  if (!u.live) u.f = 0;                                  // dead lanes of a tail slice read feature 0 and write nothing
  return u;
}

template <int LMAX, int BWD>
__global__ __launch_bounds__(256) void k_so3_conv(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ Y,
                                                  const float* __restrict__ fcut, const int64_t* __restrict__ idx_j,
                                                  const int32_t* __restrict__ rowptr, const int32_t* __restrict__ rev, int64_t N, int64_t P, int F,
                                                  int nsl, float* __restrict__ y) {
  constexpr int S = (LMAX + 1) * (LMAX + 1), NL = LMAX + 1;
  const So3Unit u = so3_unit(N, F, nsl);
  if (!u.any) return;                                    // uniform over the wave
  const int64_t a = u.row;
  const int e0 = rowptr[a], e1 = rowptr[a + 1];
  float acc[S];
#pragma unroll
  for (int s = 0; s < S; ++s) acc[s] = 0.f;
  for (int e = e0; e < e1; ++e) {
    int64_t j = idx_j[e];
    j = j < 0 ? 0 : (j >= N ? N - 1 : j);
    int64_t p = BWD ? (int64_t)rev[e] : (int64_t)e;
    p = p < 0 ? 0 : (p >= P ? P - 1 : p);
    const float fc = fcut[p];
    float w[NL], av[S], xs[S];
#pragma unroll
    for (int l = 0; l < NL; ++l) w[l] = W[(p * NL + l) * F + u.f] * fc;
#pragma unroll
    for (int s = 0; s < S; ++s) {
      av[s] = Y[p * S + s] * w[so3_l_of(s)];
      xs[s] = x[(j * S + s) * F + u.f];
    }
    if constexpr (BWD == 0) {
#define SO3_X(s1, s2, s, c) acc[s] = fmaf((c) * av[s1], xs[s2], acc[s]);
      SO3_CG_APPLY(LMAX, SO3_X);
#undef SO3_X
    } else {
#define SO3_X(s1, s2, s, c) acc[s2] = fmaf((c) * av[s1], xs[s], acc[s2]);
      SO3_CG_APPLY(LMAX, SO3_X);
#undef SO3_X
    }
  }
  if (u.live) {
#pragma unroll
    for (int s = 0; s < S; ++s) y[(a * S + s) * F + u.f] = acc[s];
  }
}

template <int LMAX>
__global__ __launch_bounds__(256) void k_so3_edge(const float* __restrict__ gy, const float* __restrict__ x, const float* __restrict__ W,
                                                  const float* __restrict__ Y, const float* __restrict__ fcut, const int64_t* __restrict__ idx_j,
                                                  const int32_t* __restrict__ rowptr, int64_t N, int64_t P, int F, int nsl, float* __restrict__ gW,
                                                  float* __restrict__ gYp) {
  constexpr int S = (LMAX + 1) * (LMAX + 1), NL = LMAX + 1;
  const So3Unit u = so3_unit(N, F, nsl);
  if (!u.any) return;
  const int64_t a = u.row;
  const int lane = threadIdx.x & 63;
  const int sl = (int)(((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) % nsl);
  const int e0 = rowptr[a], e1 = rowptr[a + 1];
  float g[S];
#pragma unroll
  for (int s = 0; s < S; ++s) g[s] = gy[(a * S + s) * F + u.f];
  for (int e = e0; e < e1; ++e) {
    int64_t j = idx_j[e];
    j = j < 0 ? 0 : (j >= N ? N - 1 : j);
    float xs[S], t[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      xs[s] = x[(j * S + s) * F + u.f];
      t[s] = 0.f;
    }
#define SO3_X(s1, s2, s, c) t[s1] = fmaf((c) * xs[s2], g[s], t[s1]);
    SO3_CG_APPLY(LMAX, SO3_X);
#undef SO3_X
    const float fc = fcut[e];
    float gw[NL], w[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      gw[l] = 0.f;
      w[l] = u.live ? W[((int64_t)e * NL + l) * F + u.f] : 0.f;
    }
#pragma unroll
    for (int s = 0; s < S; ++s) {
      gw[so3_l_of(s)] = fmaf(Y[(int64_t)e * S + s], t[s], gw[so3_l_of(s)]);
      float r = w[so3_l_of(s)] * t[s];                   // dead lanes add exact zeros
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) r += __shfl_xor(r, d, 64);
      if (lane == 0) gYp[((int64_t)sl * P + e) * S + s] = r;
    }
    if (u.live) {
#pragma unroll
      for (int l = 0; l < NL; ++l) gW[((int64_t)e * NL + l) * F + u.f] = fc * gw[l];
    }
  }
}

__global__ __launch_bounds__(256) void k_so3_edge_fin(const float* __restrict__ gYp, const float* __restrict__ Y, const float* __restrict__ fcut,
                                                      int64_t P, int S, int nsl, float* __restrict__ gY, float* __restrict__ gfcut) {
  const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (p >= P) return;
  const float fc = fcut[p];
  float gf = 0.f;
  for (int s = 0; s < S; ++s) {
    float v = 0.f;
    for (int k = 0; k < nsl; ++k) v += gYp[((int64_t)k * P + p) * S + s];
    gY[p * S + s] = fc * v;
    gf = fmaf(Y[p * S + s], v, gf);
  }
  gfcut[p] = gf;
}

template <int LMAX>
__global__ __launch_bounds__(256) void k_so3_prod_fwd(const float* __restrict__ x1, const float* __restrict__ x2, int64_t N, int F, int nsl,
                                                      float* __restrict__ y) {
  constexpr int S = (LMAX + 1) * (LMAX + 1);
  const So3Unit u = so3_unit(N, F, nsl);
  if (!u.live) return;
  float a[S], b[S], acc[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    a[s] = x1[(u.row * S + s) * F + u.f];
    b[s] = x2[(u.row * S + s) * F + u.f];
    acc[s] = 0.f;
  }
#define SO3_X(s1, s2, s, c) acc[s] = fmaf((c) * a[s1], b[s2], acc[s]);
  SO3_CG_APPLY(LMAX, SO3_X);
#undef SO3_X
#pragma unroll
  for (int s = 0; s < S; ++s) y[(u.row * S + s) * F + u.f] = acc[s];
}

template <int LMAX>
__global__ __launch_bounds__(256) void k_so3_prod_bwd(const float* __restrict__ gy, const float* __restrict__ x1, const float* __restrict__ x2,
                                                      int64_t N, int F, int nsl, float* __restrict__ gx1, float* __restrict__ gx2) {
  constexpr int S = (LMAX + 1) * (LMAX + 1);
  const So3Unit u = so3_unit(N, F, nsl);
  if (!u.live) return;
  float a[S], b[S], g[S], ga[S], gb[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    a[s] = x1[(u.row * S + s) * F + u.f];
    b[s] = x2[(u.row * S + s) * F + u.f];
    g[s] = gy[(u.row * S + s) * F + u.f];
    ga[s] = 0.f;
    gb[s] = 0.f;
  }
#define SO3_X(s1, s2, s, c)                    \
  {                                            \
    const float cg_ = (c) * g[s];              \
    ga[s1] = fmaf(cg_, b[s2], ga[s1]);         \
    gb[s2] = fmaf(cg_, a[s1], gb[s2]);         \
  }
  SO3_CG_APPLY(LMAX, SO3_X);
#undef SO3_X
#pragma unroll
  for (int s = 0; s < S; ++s) {
    gx1[(u.row * S + s) * F + u.f] = ga[s];
    gx2[(u.row * S + s) * F + u.f] = gb[s];
  }
}

// AB_m(x, y), Pi_l^|m|(z) of every component and their derivatives; Y[s] = N_l PI[s] AB[s]
template <int LMAX>
struct RshTerms {
  static constexpr int S = (LMAX + 1) * (LMAX + 1);
  float N[S], AB[S], ABx[S], ABy[S], PI[S], PIz[S];
  __device__ __forceinline__ RshTerms(float x, float y, float z) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
      AB[s] = SPK_RSH_AB0; ABx[s] = 0.f; ABy[s] = 0.f; PI[s] = 1.f; PIz[s] = 0.f;
      N[s] = so3_l_of(s) == 0 ? SPK_RSH_N0 : (so3_l_of(s) == 1 ? SPK_RSH_N1 : (so3_l_of(s) == 2 ? SPK_RSH_N2 : SPK_RSH_N3));
    }
    PI[0] = SPK_RSH_PI00_Z0;
    // l = 1: m = -1 (B1 = y), 0, +1 (A1 = x)
    AB[1] = y; ABy[1] = 1.f; PI[1] = SPK_RSH_PI11_Z0;
    PI[2] = SPK_RSH_PI10_Z1 * z; PIz[2] = SPK_RSH_PI10_Z1;
    AB[3] = x; ABx[3] = 1.f; PI[3] = SPK_RSH_PI11_Z0;
    if constexpr (LMAX >= 2) {
      const float A2 = x * x - y * y, B2 = 2.f * x * y;
      AB[4] = B2; ABx[4] = 2.f * y; ABy[4] = 2.f * x; PI[4] = SPK_RSH_PI22_Z0;
      AB[5] = y; ABy[5] = 1.f; PI[5] = SPK_RSH_PI21_Z1 * z; PIz[5] = SPK_RSH_PI21_Z1;
      PI[6] = fmaf(SPK_RSH_PI20_Z2 * z, z, SPK_RSH_PI20_Z0); PIz[6] = 2.f * SPK_RSH_PI20_Z2 * z;
      AB[7] = x; ABx[7] = 1.f; PI[7] = SPK_RSH_PI21_Z1 * z; PIz[7] = SPK_RSH_PI21_Z1;
      AB[8] = A2; ABx[8] = 2.f * x; ABy[8] = -2.f * y; PI[8] = SPK_RSH_PI22_Z0;
      if constexpr (LMAX >= 3) {
        const float A3 = x * x * x - 3.f * x * y * y, B3 = 3.f * x * x * y - y * y * y;
        AB[9] = B3; ABx[9] = 3.f * B2; ABy[9] = 3.f * A2; PI[9] = SPK_RSH_PI33_Z0;
        AB[10] = B2; ABx[10] = 2.f * y; ABy[10] = 2.f * x; PI[10] = SPK_RSH_PI32_Z1 * z; PIz[10] = SPK_RSH_PI32_Z1;
        AB[11] = y; ABy[11] = 1.f; PI[11] = fmaf(SPK_RSH_PI31_Z2 * z, z, SPK_RSH_PI31_Z0); PIz[11] = 2.f * SPK_RSH_PI31_Z2 * z;
        PI[12] = (SPK_RSH_PI30_Z3 * z * z + SPK_RSH_PI30_Z1) * z; PIz[12] = fmaf(3.f * SPK_RSH_PI30_Z3 * z, z, SPK_RSH_PI30_Z1);
        AB[13] = x; ABx[13] = 1.f; PI[13] = PI[11]; PIz[13] = PIz[11];
        AB[14] = A2; ABx[14] = 2.f * x; ABy[14] = -2.f * y; PI[14] = PI[10]; PIz[14] = PIz[10];
        AB[15] = A3; ABx[15] = 3.f * A2; ABy[15] = -3.f * B2; PI[15] = SPK_RSH_PI33_Z0;
      }
    }
  }
};

template <int LMAX>
__global__ __launch_bounds__(256) void k_rsh_fwd(const float* __restrict__ dir, int64_t P, float* __restrict__ Y) {
  constexpr int S = (LMAX + 1) * (LMAX + 1);
  const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (p >= P) return;
  const RshTerms<LMAX> T(dir[3 * p], dir[3 * p + 1], dir[3 * p + 2]);
#pragma unroll
  for (int s = 0; s < S; ++s) Y[p * S + s] = T.N[s] * T.PI[s] * T.AB[s];
}

template <int LMAX>
__global__ __launch_bounds__(256) void k_rsh_bwd(const float* __restrict__ gY, const float* __restrict__ dir, int64_t P, float* __restrict__ gdir) {
  constexpr int S = (LMAX + 1) * (LMAX + 1);
  const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (p >= P) return;
  const RshTerms<LMAX> T(dir[3 * p], dir[3 * p + 1], dir[3 * p + 2]);
  float gx = 0.f, gy = 0.f, gz = 0.f;
#pragma unroll
  for (int s = 1; s < S; ++s) {
    const float g = gY[p * S + s] * T.N[s];
    gx = fmaf(g * T.PI[s], T.ABx[s], gx);
    gy = fmaf(g * T.PI[s], T.ABy[s], gy);
    gz = fmaf(g * T.PIz[s], T.AB[s], gz);
  }
  gdir[3 * p] = gx; gdir[3 * p + 1] = gy; gdir[3 * p + 2] = gz;
}

inline size_t so3_align(size_t b) { return (b + 255) & ~(size_t)255; }
inline int so3_slices(int F) { return (F + 63) / 64; }

int so3_check_shape(const char* who, int32_t lmax, int32_t F) {
  SPK_CHECK_ARG(lmax >= 1 && lmax <= 3, "%s: lmax %d outside 1..3", who, (int)lmax);
  SPK_CHECK_ARG(F >= 32 && F <= kSo3MaxF && F % 32 == 0, "%s: %d features (a multiple of 32 up to %d)", who, (int)F, kSo3MaxF);
  return SPK_OK;
}

int so3_check_graph(const char* who, const spk_graph_t* g, bool need_rev) {
  SPK_CHECK_ARG(g != nullptr && g->n_atoms >= 0 && g->n_edges >= 0, "%s: bad graph", who);
  SPK_CHECK_ARG(g->n_atoms < (1LL << 31) - 2 && g->n_edges < (1LL << 31), "%s: list too large for 32-bit row pointers", who);
  if (g->n_edges == 0) return SPK_OK;
  SPK_CHECK_ARG(g->sorted && g->rowptr && g->idx_j, "%s: the list must be sorted by idx_i (row pointers)", who);
  SPK_CHECK_ARG(!need_rev || (g->symmetric && g->rev), "%s: the list must be symmetric (reverse-edge map)", who);
  return SPK_OK;
}

inline dim3 so3_grid(int64_t rows, int nsl) { return dim3((unsigned)((rows * nsl + 3) / 4)); }

#define SO3_DISPATCH(lmax, CALL) \
  do {                           \
    if ((lmax) == 1) { CALL(1); } else if ((lmax) == 2) { CALL(2); } else { CALL(3); } \
  } while (0)

}  // namespace

extern "C" int spk_so3_supported(int32_t lmax, int32_t F) { return lmax >= 1 && lmax <= 3 && F >= 32 && F <= kSo3MaxF && F % 32 == 0; }

// host only: the compiled-in Clebsch-Gordan table of lmax; returns the number of non-zeros (and fills up to cap of them), -1 for another lmax
extern "C" int32_t spk_so3_cg_table(int32_t lmax, int32_t cap, int32_t* s1, int32_t* s2, int32_t* s, float* c) {
  struct Row { int32_t a, b, o; float c; };
#define SO3_ROW(a, b, o, v) {a, b, o, v},
  static const Row t1[] = {SPK_SO3_CG_L1(SO3_ROW)};
  static const Row t2[] = {SPK_SO3_CG_L2(SO3_ROW)};
  static const Row t3[] = {SPK_SO3_CG_L3(SO3_ROW)};
#undef SO3_ROW
  const Row* t = lmax == 1 ? t1 : (lmax == 2 ? t2 : (lmax == 3 ? t3 : nullptr));
  if (!t) return -1;
  const int32_t n = lmax == 1 ? SPK_SO3_NCG_L1 : (lmax == 2 ? SPK_SO3_NCG_L2 : SPK_SO3_NCG_L3);
  for (int32_t k = 0; k < n && k < cap; ++k) {
    if (s1) s1[k] = t[k].a;
    if (s2) s2[k] = t[k].b;
    if (s) s[k] = t[k].o;
    if (c) c[k] = t[k].c;
  }
  return n;
}

extern "C" int spk_rsh_fwd_f32(const float* directions, int64_t P, int32_t lmax, float* Y, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPK_CHECK_ARG(lmax >= 1 && lmax <= 3 && P >= 0, "spk_rsh_fwd_f32: lmax %d outside 1..3 / bad count", (int)lmax);
  if (P == 0) return SPK_OK;
  SPK_CHECK_ARG(directions && Y, "spk_rsh_fwd_f32: null argument");
#define SO3_CALL(L) hipLaunchKernelGGL((k_rsh_fwd<L>), dim3(spk_grid_for(P, 256, 1 << 30)), dim3(256), 0, stream, directions, P, Y)
  SO3_DISPATCH(lmax, SO3_CALL);
#undef SO3_CALL
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" int spk_rsh_bwd_f32(const float* gY, const float* directions, int64_t P, int32_t lmax, float* gdir, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPK_CHECK_ARG(lmax >= 1 && lmax <= 3 && P >= 0, "spk_rsh_bwd_f32: lmax %d outside 1..3 / bad count", (int)lmax);
  if (P == 0) return SPK_OK;
  SPK_CHECK_ARG(gY && directions && gdir, "spk_rsh_bwd_f32: null argument");
#define SO3_CALL(L) hipLaunchKernelGGL((k_rsh_bwd<L>), dim3(spk_grid_for(P, 256, 1 << 30)), dim3(256), 0, stream, gY, directions, P, gdir)
  SO3_DISPATCH(lmax, SO3_CALL);
#undef SO3_CALL
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" int64_t spk_so3_conv_workspace_bytes(const spk_graph_t* g, int32_t lmax, int32_t F) {
  if (!g || g->n_edges < 0 || !spk_so3_supported(lmax, F)) return -1;
  const int64_t S = (lmax + 1) * (lmax + 1);
  return (int64_t)so3_align((size_t)so3_slices(F) * (size_t)(g->n_edges > 0 ? g->n_edges : 1) * (size_t)S * 4);
}

extern "C" int spk_so3_conv_fwd_f32(const float* x, const float* W, const float* Y, const float* fcut, const spk_graph_t* g, int32_t lmax, int32_t F,
                                    float* y, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "spk_so3_conv_fwd_f32";
  SPK_TRY(so3_check_shape(who, lmax, F));
  SPK_TRY(so3_check_graph(who, g, false));
  const int64_t N = g->n_atoms, P = g->n_edges, S = (lmax + 1) * (lmax + 1);
  if (N == 0) return SPK_OK;
  SPK_CHECK_ARG(y != nullptr, "%s: null output", who);
  if (P == 0) return spk_zero_async(y, (size_t)N * S * F * 4, stream);          // (the plan of an empty list carries no row pointers)
  SPK_CHECK_ARG(x && W && Y && fcut, "%s: null argument", who);
  SpkProfScope prof("so3_conv_fwd", stream);
  const int nsl = so3_slices(F);
#define SO3_CALL(L) hipLaunchKernelGGL((k_so3_conv<L, 0>), so3_grid(N, nsl), dim3(256), 0, stream, x, W, Y, fcut, g->idx_j, g->rowptr, \
                                       (const int32_t*)nullptr, N, P, (int)F, nsl, y)
  SO3_DISPATCH(lmax, SO3_CALL);
#undef SO3_CALL
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" int spk_so3_conv_bwd_f32(const float* gy, const float* x, const float* W, const float* Y, const float* fcut, const spk_graph_t* g,
                                    int32_t lmax, int32_t F, float* gx, float* gW, float* gY, float* gfcut, void* workspace, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "spk_so3_conv_bwd_f32";
  SPK_TRY(so3_check_shape(who, lmax, F));
  SPK_TRY(so3_check_graph(who, g, gx != nullptr));
  const int64_t N = g->n_atoms, P = g->n_edges, S = (lmax + 1) * (lmax + 1);
  if (N == 0) return SPK_OK;
  if (P == 0) return gx ? spk_zero_async(gx, (size_t)N * S * F * 4, stream) : SPK_OK;
  SPK_CHECK_ARG(gy && x && W && Y && fcut, "%s: null argument", who);
  const bool edges = gW || gY || gfcut;
  SPK_CHECK_ARG(!edges || (gW && gY && gfcut && workspace), "%s: the pair gradients gW, gY, gfcut come together and need the workspace", who);
  SpkProfScope prof("so3_conv_bwd", stream);
  const int nsl = so3_slices(F);
  if (gx) {
#define SO3_CALL(L) hipLaunchKernelGGL((k_so3_conv<L, 1>), so3_grid(N, nsl), dim3(256), 0, stream, gy, W, Y, fcut, g->idx_j, g->rowptr, g->rev, N, P, \
                                       (int)F, nsl, gx)
    SO3_DISPATCH(lmax, SO3_CALL);
#undef SO3_CALL
    SPK_LAUNCH_CHECK();
  }
  if (edges) {
    float* gYp = (float*)workspace;
#define SO3_CALL(L) hipLaunchKernelGGL((k_so3_edge<L>), so3_grid(N, nsl), dim3(256), 0, stream, gy, x, W, Y, fcut, g->idx_j, g->rowptr, N, P, (int)F, nsl, \
                                       gW, gYp)
    SO3_DISPATCH(lmax, SO3_CALL);
#undef SO3_CALL
    SPK_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_so3_edge_fin, dim3(spk_grid_for(P, 256, 1 << 30)), dim3(256), 0, stream, (const float*)gYp, Y, fcut, P, (int)S, nsl, gY, gfcut);
    SPK_LAUNCH_CHECK();
  }
  return SPK_OK;
}

extern "C" int spk_so3_product_fwd_f32(const float* x1, const float* x2, int64_t N, int32_t lmax, int32_t F, float* y, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "spk_so3_product_fwd_f32";
  SPK_TRY(so3_check_shape(who, lmax, F));
  SPK_CHECK_ARG(N >= 0 && N < (1LL << 31), "%s: bad atom count", who);
  if (N == 0) return SPK_OK;
  SPK_CHECK_ARG(x1 && x2 && y, "%s: null argument", who);
  const int nsl = so3_slices(F);
#define SO3_CALL(L) hipLaunchKernelGGL((k_so3_prod_fwd<L>), so3_grid(N, nsl), dim3(256), 0, stream, x1, x2, N, (int)F, nsl, y)
  SO3_DISPATCH(lmax, SO3_CALL);
#undef SO3_CALL
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

extern "C" int spk_so3_product_bwd_f32(const float* gy, const float* x1, const float* x2, int64_t N, int32_t lmax, int32_t F, float* gx1, float* gx2,
                                       void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "spk_so3_product_bwd_f32";
  SPK_TRY(so3_check_shape(who, lmax, F));
  SPK_CHECK_ARG(N >= 0 && N < (1LL << 31), "%s: bad atom count", who);
  if (N == 0) return SPK_OK;
  SPK_CHECK_ARG(gy && x1 && x2 && gx1 && gx2, "%s: null argument", who);
  const int nsl = so3_slices(F);
#define SO3_CALL(L) hipLaunchKernelGGL((k_so3_prod_bwd<L>), so3_grid(N, nsl), dim3(256), 0, stream, gy, x1, x2, N, (int)F, nsl, gx1, gx2)
  SO3_DISPATCH(lmax, SO3_CALL);
#undef SO3_CALL
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}
