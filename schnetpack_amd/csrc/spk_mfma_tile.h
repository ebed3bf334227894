// Matrix-tile helpers of the fused kernels (device code only): the "T-GEMM" convention of every kernel of this library that uses the
// fp32 matrix core (v_mfma_f32_32x32x2_f32, exact fp32, 64 lanes), written down once.  tests/test_mfma_layout_model.py replays it
// on the CPU.
//
//   The wave computes a 32x32 tile of OUT^T:  rows = output features i, columns = samples m.
//   A operand (weights):  lane l holds A[i = i0 + (l & 31)][kk],
//   B operand (samples):  lane l holds B[kk][m = m0 + (l & 31)] = in[m][kk],
//   where for k-step s = 4u + v the lane half hi = l >> 5 supplies kk = 8u + 4hi + v
//   (any bijection between (step, half) and kk is legal as long as A and B agree; this one lets
//   each lane fetch 4 consecutive kk with one 16-byte load),
//   C/D accumulator:      acc[r] <-> row i = i0 + spk_acc_row(r, hi) = i0 + (r & 3) + 8 (r >> 2) + 4 hi, column m0 + (l & 31):
//   a lane owns 16 rows of ONE column, as four runs of four consecutive rows, 8 apart.
//   Because the accumulator rows use the same (r>>2, r&3, hi) -> index map as the k-steps, an
//   accumulator tile can be fed straight back as the B operand of the next layer (chained GEMMs
//   without leaving registers) -- used by the fused cfconv kernels.
//   Packed weight image (spk_pack.h): P[((t * KB + ug) * 64 + lane) * 4 + v] = W[32 t + (lane & 31)][8 ug + 4 (lane >> 5) + v] --
//   k-block ug of tile t is one 16-byte load per lane, kSpkKBlockBytes per wave, and IS the A operand of its four k-steps.
#pragma once
#include "spk_common.h"
#include "spk_split.h"

#define SPK_MFMA(A, B, C) __builtin_amdgcn_mfma_f32_32x32x2f32((A), (B), (C), 0, 0, 0)

// row of register r of the lane half hi of a 32x32 accumulator whose first row is i0
__device__ __forceinline__ int spk_acc_row(int r, int hi, int i0 = 0) { return i0 + (r & 3) + 8 * (r >> 2) + 4 * hi; }

// Global accesses as  wave-uniform base (SGPR pair) + 32-bit per-lane byte offset: one VGPR per address instead of a 64-bit
// pair -- with 64-bit per-lane addresses the compiler hoists dozens of address pairs out of the loops and spills them.
template <class T>
__device__ __forceinline__ T spk_ld(const void* sbase, unsigned voff) { return *(const T*)((const char*)sbase + voff); }
template <class T>
__device__ __forceinline__ void spk_st(void* sbase, unsigned voff, T v) { *(T*)((char*)sbase + voff) = v; }

// Keeps the memory accesses written in front of it in front of it: the LOADS stay where they are written, not the matrix
// instructions (a kernel that needs the scheduler stopped as well adds __builtin_amdgcn_sched_barrier(0) itself).
#define SPK_PIN() asm volatile("" ::: "memory")
// Workgroup barrier that waits for the LDS traffic of the wave only (like ck's block_sync_lds): __syncthreads() also drains
// vmcnt, i.e. waits until the global STORES of the phase have been acknowledged by L2 (~5 k cycles each time) and until the
// weight tiles prefetched for the next phase have arrived -- neither is needed at the barrier.
#define SPK_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

// ---- Dense block of the molecule-resident kernels: A = packed weights straight from L2, B = activations [32][LD] in LDS;
// accumulator rows = output features 32 t + spk_acc_row(r, hi), columns = atoms (lane & 31).
constexpr int kSpkKBlockBytes = 1024;      // one k-block of a packed tile: 64 lanes x 16 bytes

// k-block kb0 of tile t (wave-uniform) of a packed image with KB k-blocks per tile
__device__ __forceinline__ const char* spk_tile_base(const float* __restrict__ wp, int KB, int t, int kb0) {
  return (const char*)wp + ((size_t)t * KB + kb0) * kSpkKBlockBytes;
}
// NB k-blocks from `sb` on, all requested at once (the weights do not depend on the data: a caller may issue this a phase EARLY)
template <int NB>
__device__ __forceinline__ void spk_tile_load(f32x4 (&av)[NB], const char* sb /* wave-uniform */, int lane) {
#pragma unroll
  for (int u = 0; u < NB; ++u) av[u] = spk_ld<f32x4>(sb, (unsigned)(lane * 16 + u * kSpkKBlockBytes));
}
// the lane's B operands in a [32][LD] fp32 tile from contraction index k0 on: row lane & 31, then 4 hi (fp32 form, KHI = 4) or 8 hi (split form)
template <int LD, int KHI = 4>
__device__ __forceinline__ const float* spk_tile_brow(const float* __restrict__ sB, int lane, int k0 = 0) {
  return sB + (lane & 31) * LD + KHI * (lane >> 5) + k0;
}
// fp32 block.  B operands are requested four k-blocks ahead of their MFMAs and pinned there: left alone the compiler issues every
// ds_read right in front of the four MFMAs that need it and the matrix pipe waits ~100 cycles per group of four.
template <int NB>
__device__ __forceinline__ f32x16 spk_tile_mma(const f32x4 (&av)[NB], const float* __restrict__ brow /* spk_tile_brow<LD, 4> */, f32x16 acc) {
  static_assert(NB >= 4, "the first four k-blocks are requested up front");
  f32x4 bv[NB];
#pragma unroll
  for (int u = 0; u < 4; ++u) bv[u] = *(const f32x4*)(brow + 8 * u);
  SPK_PIN();
#pragma unroll
  for (int u = 0; u < NB; ++u) {
    acc = SPK_MFMA(av[u].x, bv[u].x, acc);
    acc = SPK_MFMA(av[u].y, bv[u].y, acc);
    acc = SPK_MFMA(av[u].z, bv[u].z, acc);
    acc = SPK_MFMA(av[u].w, bv[u].w, acc);
    if (u + 4 < NB) { bv[u + 4] = *(const f32x4*)(brow + 8 * (u + 4)); SPK_PIN(); }
  }
  return acc;
}
// Split block (spk_split.h), NS k-steps of 16: `av` holds 2 NS chunks of the SPLIT weight image (k_pack_weight_split: chunk 2 s = the
// high parts of k-step s, chunk 2 s + 1 its 2^11-scaled low parts -- same bytes, same offsets as the fp32 image), the activations
// are read from the fp32 tile as eight consecutive values per k-step, AHEAD k-steps ahead of their use, and split in registers;
// three f16 instructions per 16 k instead of eight f32 ones, the cross terms in their own accumulator, folded in at the end.
template <int NS, int AHEAD>
__device__ __forceinline__ f32x16 spk_tile_mma_sp(const f32x4* __restrict__ av, const float* __restrict__ brow /* spk_tile_brow<LD, 8> */, f32x16 acc) {
  f32x16 cx;
#pragma unroll
  for (int r = 0; r < 16; ++r) cx[r] = 0.f;
  f32x4 b0[NS], b1[NS];
#pragma unroll
  for (int s = 0; s < AHEAD && s < NS; ++s) { b0[s] = *(const f32x4*)(brow + 16 * s); b1[s] = *(const f32x4*)(brow + 16 * s + 4); }
  SPK_PIN();
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    if (s + AHEAD < NS) { b0[s + AHEAD] = *(const f32x4*)(brow + 16 * (s + AHEAD)); b1[s + AHEAD] = *(const f32x4*)(brow + 16 * (s + AHEAD) + 4); SPK_PIN(); }
    h16x4 h0, l0, h1, l1;
    sp_split4(b0[s], h0, l0);
    sp_split4(b1[s], h1, l1);
    SP_STEP(__builtin_bit_cast(h16x8, av[2 * s]), __builtin_bit_cast(h16x8, av[2 * s + 1]), sp_cat(h0, h1), sp_cat(l0, l1), acc, cx);
  }
  SP_FOLD(acc, cx);
  return acc;
}
// accumulator that starts as the bias of output tile t
__device__ __forceinline__ f32x16 spk_bias_acc(const float* __restrict__ b, int t, int hi) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = b[32 * t + spk_acc_row(r, hi)];
  return acc;
}
