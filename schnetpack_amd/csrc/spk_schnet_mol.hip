// Molecule-resident SchNet representation (representation/schnet.py:147-173) for BATCHES OF SMALL MOLECULES.
//
// A batch produced by the reference's collate function (data/loader.py:35-46) is block diagonal: no edge leaves a
// molecule.  With <= 32 atoms per block the whole representation of a block -- every interaction: in2f, the
// continuous-filter convolution, f2out, the residual -- is local to ONE workgroup: the atom features live in LDS for the
// whole kernel and nothing but the saved-for-backward tensors goes to memory.  One launch replaces the 1 + 2 L launches
// of the general driver (spk_schnet.hip), the float atomics of the pair kernels and their memsets; configs[1] of
// BASELINE.json (256 aspirin frames) maps one molecule onto each of the 256 compute units.
//
// Workgroup = 8 wavefronts, one group of atoms (a block, or several small blocks, <= 32 atoms).  Set-up once per group: atom
// features and per-pair records (atoms, distance, f_c) in LDS, shared by every interaction.  The waves are two teams of four, wave t
// of a team owns channel tile t.  Per interaction:
//   A. pair tiles of 32 undirected pairs, alternating between the teams (team 1 runs in2f, h = x W_in^T, first):
//        hidden layer ONCE per tile and team: radial basis from a table staged per launch (ml_basis_split_lin) -> GEMM 1 ->
//          ssp -> one LDS tile, wave t its 32 hidden channels;
//        per wave: GEMM 2 with swapped operands (rows = pairs, columns = its 32 channels) -> raw filter outputs g to memory (the
//          tensor the backward reads; L2-resident) -> modulation W = g f_c, products W h[j], W h[i] -> accumulated into
//          y[atom, channel] by the 0/1 incidence of the tile ON THE MATRIX CORE; branch-free: padding rows of the last tile
//          repeat its last pair with weight zero.  No atomics, no scatter pass, deterministic
//   C. t = ssp((y_team0 + y_team1) W3^T + b3);  x += t W4^T + b4      (two T-GEMM phases; the idle team stages the filter
//        weights of the next interaction into LDS meanwhile, all its loads in flight at once: one round trip to L2.  Split
//        instances: t is written to LDS as the split image and the second phase reads it as it lies -- split once, at the writer)
// then the energy head on the atom tile that is still in LDS (split instances: its weights staged into the dead images of the filter
// network by the team that idles in the last phase C1, x_L as a split image, the hidden layer on the split path).
// Matrix products run on the split-precision path (spk_split.h: fp32
// operands as two fp16 images on v_mfma_f32_32x32x16_f16; 1e-5 parity with the reference rules out plain bf16 / fp16), or, with
// spk_set_split(0), on v_mfma_f32_32x32x2_f32 (the <KPB, false> instances).
#include "spk_common.h"
#include "spk_pack.h"
#include "spk_schnet_mol.h"
#include "spk_mfma_tile.h"
#include "spk_split.h"
#include "spk_filter_split.h"

#define ML_MAXL 6
#define ML_LD 132          // row stride (floats) of the [32][128] activation tiles in LDS: conflict-free 16-byte accesses
#define ML_MAXPAIRS 384    // pairs per group (28 fully connected atoms; LDS budget of the backward)
#define ML_MAXEDGES 768

struct MolPair;
// The records region of `saved` (spk_schnet_mol_records_region()): what ml_pair_records() of the forward computed, as the backward's
// set-up wants it -- rec[p0 + r] = compacted record r of the group whose pair list starts at p0, map[p0 + s] = record of list
// position s or -1, vec[3 (p0 + s)] = its pair vector, np[group] = number of records.  rec == null: no region.
struct MolHandoff { MolPair* rec; float* vec; int* map; int* np; };

struct MolLayerDev {
  const float* in2f_p;                  // packed forward image of in2f.weight [NF, F] (spk_pack_weight_f32)
  const float *w1, *b1, *w2, *b2;       // filter network, raw state_dict tensors
  const float* w2_img;                  // split-precision LDS image of w2 (wpack), or null: made from w2 while staging
  const float *o1_p, *o1_b, *o2_p, *o2_b;  // packed forward images of f2out.0 / f2out.1 and their biases
};

struct MolFwdArgs {
  MolLayerDev L[ML_MAXL];
  int n_layers;
  const float* x0;          // [N, 128], or null: rows of the embedding table
  const float* emb;         // [n_types, 128] nuclear embedding table (schnet.py:126-128) with
  const int64_t* Z;         // [N] atomic numbers
  int n_types;
  float* x_out;             // [N, 128]
  const float* rij;         // [E, 3], or null: r_ij = R[j] - R[i] + offsets
  const float* R;           // [N, 3]
  const float* offsets;     // [E, 3] or null
  MolHeadDev head;
  const int64_t* idx_i;
  const int64_t* idx_j;
  const int32_t* half;      // canonical edge of every undirected pair (ascending)
  const int32_t* rowptr;    // CSR of idx_i
  const int32_t* edge_pair; // position in `half` of the pair every directed edge belongs to
  const int32_t* grp_atom0; // [G+1]
  const int32_t* grp_pair0; // [G+1]
  int n_groups;
  float* saved;             // per interaction h [N,128] | pre3 [N,128]
  float* gbase;             // per interaction [gsz] raw filter outputs, row = position of the pair in `half`
  int64_t gsz, N;
  RadialDev rb;
  int compact;              // drop the pairs beyond the cutoff from the tiles (lists with a skin); the backward does the same
  MolHandoff ho;            // records region of `saved` (rec == null: none): written by the group set-up for the backward
  long long* dbg;           // tuning aid: cycle stamps, see spk_schnet_mol_set_debug_buffer (null in production)
};
#define ML_STAMP(n) do { if (a.dbg && blockIdx.x == 0 && threadIdx.x == 0) a.dbg[n] = (long long)__builtin_readcyclecounter(); } while (0)
// per wave, when its memory operations have landed: entries [n, n + 8) -- which half of a Dense phase the barrier behind it waits for
#define ML_WSTAMP(n) do { if (a.dbg && blockIdx.x == 0 && lane == 0) { __builtin_amdgcn_s_waitcnt(0); a.dbg[(n) + wv] = (long long)__builtin_readcyclecounter(); } } while (0)

// per pair of a group: local atoms i | j << 8, distance, f_c(d), f_c'(d) -- computed once per group, used by every interaction
struct __attribute__((aligned(16))) MolPair { int ij; float d; float fc; float dfc; };
// the record as the split forward keeps it (rewritten in place once per group; it never needs f_c'): what a row of the modulation
// loop would otherwise derive from `ij` in every tile visit of every interaction --
// ij = byte offset of atom i's row of an [32][ML_LD] LDS tile | that of atom j << 16, dfc = the BITS of the byte offset of the
// pair's row of the saved filter outputs
__device__ __forceinline__ MolPair ml_fwd_pair(const MolPair p) {
  return MolPair{(p.ij & 255) * (ML_LD * 4) | (((p.ij >> 8) & 255) * (ML_LD * 4)) << 16, p.d, p.fc, __int_as_float((p.ij >> 16) * (128 * 4))};
}

// pair records of a group: geometry is the same for every interaction.  ij = local i | local j << 8 | position of the pair in the
// group's pair list << 16.  With `compact` (lists with a skin: MD) only the pairs INSIDE the cutoff get a record -- the others
// contribute exactly zero (f_c = f_c' = 0) and are not worth a tile of filter GEMMs; the order of the list is kept (ballot +
// prefix over the waves: deterministic, the backward reproduces it), sMap[position] = record index or -1.  Returns the number of
// records (uniform over the workgroup).  Contains workgroup barriers: call it from uniform code, np <= 512.
__device__ __forceinline__ void ml_edge_vector(const float* __restrict__ rij, const float* __restrict__ R, const float* __restrict__ offsets,
                                               const int64_t* __restrict__ idx_i, const int64_t* __restrict__ idx_j, int64_t e, float& rx, float& ry,
                                               float& rz) {
  if (rij) { rx = rij[3 * e]; ry = rij[3 * e + 1]; rz = rij[3 * e + 2]; return; }
  const int64_t i = idx_i[e], j = idx_j[e];
  rx = R[3 * j] - R[3 * i]; ry = R[3 * j + 1] - R[3 * i + 1]; rz = R[3 * j + 2] - R[3 * i + 2];
  if (offsets) { rx += offsets[3 * e]; ry += offsets[3 * e + 1]; rz += offsets[3 * e + 2]; }
}

__device__ __forceinline__ int ml_pair_records(MolPair* sP, short* sMap, int* sScan, const int32_t* __restrict__ half, const float* __restrict__ rij,
                                               const float* __restrict__ R, const float* __restrict__ offsets,
                                               const int64_t* __restrict__ idx_i, const int64_t* __restrict__ idx_j, int p0, int np, int a0,
                                               float cutoff, bool compact, int tid, float* r_keep = nullptr, const MolHandoff* ho = nullptr,
                                               int grp = 0) {
  // r_keep (3 floats of the caller, or null): the vector of the pair at position `tid` of the list (np <= 512: one pair per thread)
  // ho (or null): the records region of `saved` -- every thread also stores what it holds here for the backward (fire and forget)
  const int lane = tid & 63, wv = tid >> 6;
  MolPair pr;
  bool keep = false;
  float vx = 0.f, vy = 0.f, vz = 0.f;
  if (r_keep) { r_keep[0] = 0.f; r_keep[1] = 0.f; r_keep[2] = 0.f; }
  if (tid < np) {
    const int64_t e = half[p0 + tid];
    float rx, ry, rz;
    ml_edge_vector(rij, R, offsets, idx_i, idx_j, e, rx, ry, rz);
    if (r_keep) { r_keep[0] = rx; r_keep[1] = ry; r_keep[2] = rz; }
    vx = rx; vy = ry; vz = rz;
    pr.ij = (int)(idx_i[e] - a0) | ((int)(idx_j[e] - a0) << 8) | (tid << 16);
    pr.d = sqrtf(rx * rx + ry * ry + rz * rz);
    spk_cutoff_eval_fast(cutoff, pr.d, pr.fc, pr.dfc);
    keep = !compact || pr.d < cutoff;
  }
  const unsigned long long bal = __ballot(keep);
  if (lane == 0) sScan[wv] = __popcll(bal);
  __syncthreads();
  int off = 0, total = 0;
#pragma unroll
  for (int w = 0; w < 8; ++w) {
    const int c = sScan[w];
    if (w < wv) off += c;
    total += c;
  }
  const int pos = off + __popcll(bal & ((1ull << lane) - 1ull));
  if (keep) sP[pos] = pr;
  if (sMap && tid < np) sMap[tid] = keep ? (short)pos : (short)-1;
  if (ho) {
    if (keep) ho->rec[p0 + pos] = pr;
    if (tid < np) {
      ho->map[p0 + tid] = keep ? pos : -1;
      float* v = ho->vec + 3 * (size_t)(p0 + tid);
      v[0] = vx; v[1] = vy; v[2] = vz;
    }
    if (tid == 0) ho->np[grp] = total;
  }
  __syncthreads();
  return total;
}

// Packed LDS image of a weight matrix W[NOUT][K] (row-major, K padded with zeros to 8*KB; the layout of spk_mfma_tile.h)
template <int NTHREADS, int SLOTS>
__device__ __forceinline__ void ml_stage_packed(float* dst, const float* __restrict__ w, int K, int KB, int tid) {
  constexpr int PER = (SLOTS + NTHREADS - 1) / NTHREADS;
  constexpr int BATCH = PER < 8 ? PER : 8;       // loads in flight per thread (bounds the live registers)
  const bool vec = (K & 3) == 0;
#pragma unroll 1
  for (int p0 = 0; p0 < PER; p0 += BATCH) {
    f32x4 v[BATCH];
#pragma unroll
    for (int p = 0; p < BATCH; ++p) {
      const int s = tid + (p0 + p) * NTHREADS;
      v[p] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (s < SLOTS) {
        const int lane = s & 63;
        const int ug = (s >> 6) % KB;
        const int t = (s >> 6) / KB;
        const int row = 32 * t + (lane & 31);
        const int k0 = 8 * ug + 4 * (lane >> 5);
        const float* src = w + (int64_t)row * K + k0;
        if (vec) {
          if (k0 < K) v[p] = *(const f32x4*)src;
        } else {
          if (k0 + 0 < K) v[p].x = src[0];
          if (k0 + 1 < K) v[p].y = src[1];
          if (k0 + 2 < K) v[p].z = src[2];
          if (k0 + 3 < K) v[p].w = src[3];
        }
      }
    }
#pragma unroll
    for (int p = 0; p < BATCH; ++p) {
      const int s = tid + (p0 + p) * NTHREADS;
      if (s < SLOTS) *(f32x4*)(dst + (int64_t)s * 4) = v[p];
    }
  }
}

// the same image made once per weight version in global memory (wpack, spk_schnet_pack_weights_f32): staging is then a plain copy
__global__ void k_mol_pack_w2(const float* __restrict__ w2, float* __restrict__ image) {
  ml_stage_w2_split<256>((h16x8*)image, (h16x8*)image + 2048, w2, threadIdx.x);
}
int spk_schnet_mol_pack_w2(const float* w2, float* image, hipStream_t stream) {
  hipLaunchKernelGGL(k_mol_pack_w2, dim3(1), dim3(256), 0, stream, w2, image);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}
// the copy by 256 threads with ALL 16 pieces of a thread in flight at once (64 VGPRs), in two parts like ml_stage_w1_load / _store: a
// team that stages during a Dense phase has nothing else in its registers, and every further round trip to L2 is time the team
// that runs the GEMM spends waiting at the barrier
__device__ __forceinline__ void ml_w2_image_load(f32x4 (&v)[16], const float* __restrict__ img, int t2) {
#pragma unroll
  for (int p = 0; p < 16; ++p) v[p] = *(const f32x4*)((const char*)img + (unsigned)((t2 + p * 256) * 16));
}
__device__ __forceinline__ void ml_w2_image_store(float* __restrict__ dst, const f32x4 (&v)[16], int t2) {
#pragma unroll
  for (int p = 0; p < 16; ++p) *(f32x4*)(dst + (t2 + p * 256) * 4) = v[p];
}
template <int NTHREADS>
__device__ __forceinline__ void ml_stage_w2_image(float* __restrict__ dst, const float* __restrict__ img, int tid) {
  constexpr int PER = 4096 / NTHREADS;      // 16-byte pieces per thread (64 KB)
#pragma unroll 1
  for (int p0 = 0; p0 < PER; p0 += 8) {
    f32x4 v[8];
#pragma unroll
    for (int p = 0; p < 8; ++p) v[p] = *(const f32x4*)((const char*)img + (unsigned)((tid + (p0 + p) * NTHREADS) * 16));
#pragma unroll
    for (int p = 0; p < 8; ++p) *(f32x4*)(dst + (tid + (p0 + p) * NTHREADS) * 4) = v[p];
  }
}
// The energy head's first layer, outnet.0.weight [H][128], as the split A-operand image of its H / 32 row tiles: slot (row tile,
// k-step S, lane) = the eight values W[32 tile + el][16 S + 8 hi + e], high halves in `dh`, low halves in `dl` -- the slot order of
// the W2 image, with the contraction index in natural order (the B operand is a split activation tile, ml_dense_mma_sp_pre).
// Staged by 256 threads, in two parts like the W2 image above: eight slots per thread, all requested before the first is used;
// slot t2 + 256 p lies in row tile p >> 1 (uniform), tiles >= HT are neither read nor written.
__device__ __forceinline__ void ml_head_w1_load(f32x4 (&v)[16], const float* __restrict__ w1, int HT, int t2) {
  const unsigned o = (unsigned)((((t2 & 31) * 128) + 16 * ((t2 >> 6) & 3) + 8 * ((t2 >> 5) & 1)) * 4);
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    v[2 * p] = f32x4{0.f, 0.f, 0.f, 0.f}; v[2 * p + 1] = f32x4{0.f, 0.f, 0.f, 0.f};
    if ((p >> 1) < HT) {
      const unsigned op = o + (unsigned)((32 * (p >> 1) * 128 + 64 * (p & 1)) * 4);
      v[2 * p] = *(const f32x4*)((const char*)w1 + op);
      v[2 * p + 1] = *(const f32x4*)((const char*)w1 + op + 16u);
    }
  }
}
__device__ __forceinline__ void ml_head_w1_store(h16x8* __restrict__ dh, h16x8* __restrict__ dl, const f32x4 (&v)[16], int HT, int t2) {
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    if ((p >> 1) < HT) {
      h16x4 ah, al, bh, bl;
      sp_split4(v[2 * p], ah, al);
      sp_split4(v[2 * p + 1], bh, bl);
      dh[t2 + 256 * p] = sp_cat(ah, bh);
      dl[t2 + 256 * p] = sp_cat(al, bl);
    }
  }
}

// gh[at][c] = sum over the directed edges of the row of `at`:  sSrc[neighbour][c] * g[pair][c] * f_c(pair)   (the transpose of
// the forward's row sum), as a task of one wavefront per atom.
// sEb: per directed edge (row of the saved filter tensor << 8 | local neighbour [| 1 << 24: pair beyond the cutoff], f_c of the pair).
// A lane owns FOUR channels (16-byte loads: 32 lanes span the 128 channels, a wave-load moves two whole filter rows) and the two
// halves of the wavefront take the even / odd entries of a row, meeting through one shuffle at the end.  RB entries per half are
// in flight at once, so a row of <= 2 RB neighbours costs ONE round trip to the saved filters (which the forward
// left in L2 / Infinity Cache).  Branch-free: entries beyond the end of a row re-read its last entry with weight 0.  Fixed
// summation order.  (The first form -- a lane per channel, 4-byte loads, four dependent round trips per task -- made the
// row-sum waves the stragglers of phase E: 18 k of its 79 k cycles.)
template <int RB>
__device__ __forceinline__ void ml_row_sums4(float* __restrict__ sDst, const float* __restrict__ sSrc, const float* __restrict__ g_g,
                                             const int2* __restrict__ sEb, const int* __restrict__ sRow, int at, int lane) {
  const int hi = lane >> 5;
  const unsigned c4 = 4u * (unsigned)(lane & 31);
  int rs = sRow[at] + hi;
  const int re = sRow[at + 1];
  const int last = re > 0 ? re - 1 : 0;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  while (true) {
    int2 rec[RB];
    f32x4 gv[RB];
#pragma unroll
    for (int u = 0; u < RB; ++u) {
      const int idx = rs + 2 * u;
      rec[u] = sEb[idx < re ? idx : last];
      if (idx >= re) rec[u].y = 0;                 // weight 0 beyond the row
    }
#pragma unroll
    for (int u = 0; u < RB; ++u) gv[u] = spk_ld<f32x4>(g_g, ((unsigned)((rec[u].x >> 8) & 0xFFFF) * 128u + c4) * 4u);
#pragma unroll
    for (int u = 0; u < RB; ++u) {
      const f32x4 sv = *(const f32x4*)(sSrc + (rec[u].x & 255) * ML_LD + c4);
      const float w = __int_as_float(rec[u].y);
      acc.x = fmaf(sv.x * w, gv[u].x, acc.x);
      acc.y = fmaf(sv.y * w, gv[u].y, acc.y);
      acc.z = fmaf(sv.z * w, gv[u].z, acc.z);
      acc.w = fmaf(sv.w * w, gv[u].w, acc.w);
    }
    rs += 2 * RB;
    if (rs - hi >= re) break;                      // (wave-uniform: both halves leave together)
  }
  acc.x += __shfl_xor(acc.x, 32, 64); acc.y += __shfl_xor(acc.y, 32, 64);
  acc.z += __shfl_xor(acc.z, 32, 64); acc.w += __shfl_xor(acc.w, 32, 64);
  if (hi == 0) *(f32x4*)(sDst + at * ML_LD + c4) = acc;
}

// One 32-column output tile of a Dense layer over the 32 atom rows of the group is a Dense block of spk_mfma_tile.h: A = packed
// weights straight from L2 (16 k-blocks of 8), B = activations [32][ML_LD] in LDS.
// The weights do not depend on the data: ml_dense_load() is issued a phase EARLY -- before the barrier that completes the
// activations -- so that a Dense phase pays no L2 round trip.  A whole tile (NB = 16) or half `half` of it (NB = 8): the first half
// is requested a phase early (32 VGPRs across the phase in between), the second half at the start of the phase -- its latency
// hides behind the 32 MFMAs of the first half
template <int NB>
__device__ __forceinline__ void ml_dense_load(f32x4 (&av)[NB], const float* __restrict__ wp, int t /* wave-uniform */, int lane, int half = 0) {
  spk_tile_load(av, spk_tile_base(wp, 16, t, 8 * half), lane);
}
// The pin (SPK_PIN) keeps the LOADS where they are written, not the matrix instructions: in the split chains whose operands all come from LDS
// the scheduler moved every k-step up to its reads ("ds_read x 4, wait, three matrix instructions") and the distance was gone.  The
// fence stops the scheduler as well.  Decided chain by chain, not in SPK_PIN(): a fence costs registers -- on all pins of this file the
// split forward goes from 68 to 252 B per lane of scratch (profiles/r12_mol_matrix_overlap.md).
#define ML_FENCE() do { SPK_PIN(); __builtin_amdgcn_sched_barrier(0); } while (0)
// Split form of a Dense block (SP; spk_tile_mma_sp): the activations are read from the fp32 tile and split in registers.
// This on-the-fly form serves the tiles that must stay fp32 in LDS because something else reads or accumulates into them (x, the two
// partial sums y, dL/dx, the row sums dL/dh); a tile that is ONLY a B operand is written as the split image instead and read by
// ml_dense_mma_sp_pre below (phase C2 of the forward).  The Dense phases of the backward stay on this form: their length is set by
// the half of the workgroup that stages weights, not by the GEMM waves (profiles/r09_mol_dense_operands.md).
#ifndef SP_AHEAD
#define SP_AHEAD 1      // k-steps of LDS operands requested ahead of their use in the split Dense blocks
#endif
// Pre-split form: the activation tile lies in LDS as the SPLIT IMAGE its writer made -- row = atom, stride ML_LD * 4 bytes, bytes
// [0, 256) the 128 high halves, [256, 512) the 128 low halves (the layout of the hidden tile of phase A).  A k-step is two 16-byte
// reads and SP_STEP: no vector-unit work in the loop, so the operands are requested SP_PRE_AHEAD k-steps ahead (4 = all of a half
// tile up front; phase C2 of the forward 3.9 k cycles on the fp32 tile, 2.9 k with 2 ahead, 2.5 k with 4:
// profiles/r09_mol_dense_operands.md).  Same products in the same order as spk_tile_mma_sp on the fp32 tile: the writer splits the
// same fp32 values with the same sp_split.
#ifndef SP_PRE_AHEAD
#define SP_PRE_AHEAD 4
#endif
template <int NS>
__device__ __forceinline__ f32x16 ml_dense_mma_sp_pre(const f32x4* __restrict__ av, const char* __restrict__ brow /* lane's row + 16 hi + first k-step */, f32x16 acc) {
  f32x16 cx;
#pragma unroll
  for (int r = 0; r < 16; ++r) cx[r] = 0.f;
  h16x8 bh[NS], bl[NS];
#pragma unroll
  for (int s = 0; s < SP_PRE_AHEAD && s < NS; ++s) { bh[s] = *(const h16x8*)(brow + 32 * s); bl[s] = *(const h16x8*)(brow + 256 + 32 * s); }
  SPK_PIN();
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    if (s + SP_PRE_AHEAD < NS) { bh[s + SP_PRE_AHEAD] = *(const h16x8*)(brow + 32 * (s + SP_PRE_AHEAD)); bl[s + SP_PRE_AHEAD] = *(const h16x8*)(brow + 256 + 32 * (s + SP_PRE_AHEAD)); SPK_PIN(); }
    SP_STEP(__builtin_bit_cast(h16x8, av[2 * s]), __builtin_bit_cast(h16x8, av[2 * s + 1]), bh[s], bl[s], acc, cx);
  }
  SP_FOLD(acc, cx);
  return acc;
}
// half a Dense tile (8 k-blocks = 4 k-steps) on a split image
__device__ __forceinline__ f32x16 ml_dense_mma8_pre(const f32x4 (&av)[8], const float* __restrict__ sIn, int lane, int half, f32x16 acc) {
  return ml_dense_mma_sp_pre<4>(av, (const char*)sIn + (lane & 31) * (ML_LD * 4) + 16 * (lane >> 5) + 128 * half, acc);
}
// the writer's side: four consecutive K values of row `row` -> their place in the split image (two 8-byte stores)
__device__ __forceinline__ void ml_store_split4(float* __restrict__ tile, int row, int k0, const f32x4 v) {
  h16x4 h, l;
  sp_split4(v, h, l);
  char* p = (char*)tile + row * (ML_LD * 4) + 2 * k0;
  *(h16x4*)p = h;
  *(h16x4*)(p + 256) = l;
}
// NB k-blocks (a whole tile, or half `half` of it) against the LDS tile sIn
template <bool SP = false, int NB>
__device__ __forceinline__ f32x16 ml_dense_mma(const f32x4 (&av)[NB], const float* __restrict__ sIn, int lane, int half, f32x16 acc) {
  if constexpr (SP) return spk_tile_mma_sp<NB / 2, SP_AHEAD>(av, spk_tile_brow<ML_LD, 8>(sIn, lane, 64 * half), acc);
  return spk_tile_mma(av, spk_tile_brow<ML_LD>(sIn, lane, 64 * half), acc);
}

// B operand of a Dense half-tile that is the SUM of two LDS tiles (the two teams' partial cfconv outputs)
template <bool SP = false>
__device__ __forceinline__ f32x16 ml_dense_mma8_sum(const f32x4 (&av)[8], const float* __restrict__ sIn0, const float* __restrict__ sIn1, int lane, int half,
                                                    f32x16 acc) {
  const int hi = lane >> 5, el = lane & 31;
  if constexpr (SP) {
    const int o = el * ML_LD + 8 * hi + 64 * half;
    f32x16 cx;
#pragma unroll
    for (int r = 0; r < 16; ++r) cx[r] = 0.f;
    f32x4 p0[4], p1[4], q0[4], q1[4];
#pragma unroll
    for (int s = 0; s < SP_AHEAD; ++s) {
      p0[s] = *(const f32x4*)(sIn0 + o + 16 * s); p1[s] = *(const f32x4*)(sIn0 + o + 16 * s + 4);
      q0[s] = *(const f32x4*)(sIn1 + o + 16 * s); q1[s] = *(const f32x4*)(sIn1 + o + 16 * s + 4);
    }
    SPK_PIN();
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (s + SP_AHEAD < 4) {
        p0[s + SP_AHEAD] = *(const f32x4*)(sIn0 + o + 16 * (s + SP_AHEAD)); p1[s + SP_AHEAD] = *(const f32x4*)(sIn0 + o + 16 * (s + SP_AHEAD) + 4);
        q0[s + SP_AHEAD] = *(const f32x4*)(sIn1 + o + 16 * (s + SP_AHEAD)); q1[s + SP_AHEAD] = *(const f32x4*)(sIn1 + o + 16 * (s + SP_AHEAD) + 4);
        SPK_PIN();
      }
      h16x4 h0, l0, h1, l1;
      sp_split4(p0[s] + q0[s], h0, l0);
      sp_split4(p1[s] + q1[s], h1, l1);
      SP_STEP(__builtin_bit_cast(h16x8, av[2 * s]), __builtin_bit_cast(h16x8, av[2 * s + 1]), sp_cat(h0, h1), sp_cat(l0, l1), acc, cx);
    }
    SP_FOLD(acc, cx);
    return acc;
  }
  const int off = el * ML_LD + 4 * hi + 64 * half;
  f32x4 b0[8], b1[8];
#pragma unroll
  for (int u = 0; u < 4; ++u) { b0[u] = *(const f32x4*)(sIn0 + off + 8 * u); b1[u] = *(const f32x4*)(sIn1 + off + 8 * u); }
  SPK_PIN();
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    acc = SPK_MFMA(av[u].x, b0[u].x + b1[u].x, acc);
    acc = SPK_MFMA(av[u].y, b0[u].y + b1[u].y, acc);
    acc = SPK_MFMA(av[u].z, b0[u].z + b1[u].z, acc);
    acc = SPK_MFMA(av[u].w, b0[u].w + b1[u].w, acc);
    if (u + 4 < 8) { b0[u + 4] = *(const f32x4*)(sIn0 + off + 8 * (u + 4)); b1[u + 4] = *(const f32x4*)(sIn1 + off + 8 * (u + 4)); SPK_PIN(); }
  }
  return acc;
}

// Forward, third form.  The 8 waves are two TEAMS of four (one wave per SIMD each); wave t of a team owns channel tile t.
// Per pair tile the team computes the hidden layer ONCE -- wave t its 32 hidden channels (12 MFMAs + 16 softplus per lane
// instead of 48 + 64) -- and shares it through one LDS tile; every wave then runs GEMM 2 for its channel tile with the
// hidden activations as A operand from LDS, writes the raw filter outputs (the tensor the backward reads), and accumulates
//     y[a, c] += sum_pairs ( [i = a] h[j, c] + [j = a] h[i, c] ) W[pair, c]
// ON THE MATRIX CORE: A = the 0/1 incidence of the pair tile (rows = atoms), B = the modulated products (rows = pairs,
// columns = channels), 32 MFMAs per tile and wave, accumulator = 16 registers that live across all tiles of the wave.
// No atomics, no re-read of the filters, no scatter pass; team 1 runs in2f while team 0 starts the first tile.
template <int KPB, bool SP>
__global__ __launch_bounds__(512) void k_schnet_mol_fwd(MolFwdArgs a) {
  constexpr int NF = 128, KB2 = 16;
  constexpr int W1F = SP ? 2 * MlW1Image<KPB>::BYTES / 4 : NF * KPB * 8;     // floats of the W1 image(s)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sW2 = smem;                                  // NF*NF  (SP: high image | low image, 32 KB each)
  float* sW1 = sW2 + NF * NF;                         // NF*KPB*8  (SP: high image | low image)
  float* sb1 = sW1 + W1F;                             // NF
  h16x8* const sW2h = (h16x8*)sW2;
  h16x8* const sW2l = sW2h + 2048;
  char* const sW1h = (char*)sW1;
  char* const sW1l = sW1h + MlW1Image<KPB>::BYTES;
  float* sb2 = sb1 + NF;                              // NF
  float* sX = sb2 + NF;                               // [32][ML_LD] atom features x_l
  float* sH = sX + 32 * ML_LD;                        // h = in2f(x); later the hidden layer of f2out
  float* sY = sH + 32 * ML_LD;                        // team 0: hidden activations of its pair tile, then its partial y
  float* sT = sY + 32 * ML_LD;                        // team 1: the same
  MolPair* sP = (MolPair*)(sT + 32 * ML_LD);          // per pair: local atoms, d, f_c, f_c'
  float* sRb = (float*)(sP + ML_MAXPAIRS);            // [2][32] radial basis parameters
  int* sScan = (int*)(sRb + 64);                      // [8] per-wave counts of the pair compaction

  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);   // wv: SGPR
  const int hi = lane >> 5, el = lane & 31;
  const int team = wv >> 2, t = wv & 3;
  if constexpr (SP) ml_basis_table(sRb, a.rb, tid);          // (offset, exponent coefficient) per slot: ml_basis_split_lin()
  else if (tid < 64) {
    const int k = tid & 31;
    const float* src = (tid < 32) ? a.rb.p0 : a.rb.p1;
    sRb[tid] = (src && k < a.rb.n_rbf) ? src[k] : 1.0f;
  }

  for (int grp = blockIdx.x; grp < a.n_groups; grp += gridDim.x) {
    const int a0 = a.grp_atom0[grp], na = a.grp_atom0[grp + 1] - a0;
    const int p0 = a.grp_pair0[grp], np_list = a.grp_pair0[grp + 1] - p0;
    __syncthreads();   // the previous group is done with every LDS buffer
    ML_STAMP(0);

    // ---- group set-up: features, pair geometry (shared by all interactions), first filter weights
    for (int s = tid; s < 32 * 32; s += 512) {
      const int row = s >> 5, c4 = s & 31;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (row < na) {
        if (a.x0) v = spk_ld<f32x4>(a.x0 + (size_t)a0 * NF, (unsigned)(s * 16));
        else {
          const long long z = a.Z[a0 + row];
          if (z >= 0 && z < a.n_types) v = *(const f32x4*)(a.emb + (size_t)z * NF + 4 * c4);
          else { const float qn = __builtin_nanf(""); v = f32x4{qn, qn, qn, qn}; }     // no such row (nn.Embedding raises): NaN, never out of bounds
        }
      }
      *(f32x4*)(sX + row * ML_LD + 4 * c4) = v;
    }
    // (the records go to `saved` from the registers that hold them, before ml_fwd_pair() below rewrites sP in place)
    const int np = ml_pair_records(sP, nullptr, sScan, a.half, a.rij, a.R, a.offsets, a.idx_i, a.idx_j, p0, np_list, a0, a.rb.cutoff, a.compact != 0, tid,
                                   nullptr, a.ho.rec ? &a.ho : nullptr, grp);
    const int ntile = (np + 31) / 32;
    if constexpr (SP) {      // (each thread its own record; the barrier at the top of the first interaction publishes them)
      // The last tile is PADDED here, once per group: entries [np, 32 ntile) are the last pair's record with f_c = 0, so the tile
      // blocks below read sP at constant offsets and need neither a row count nor a select.  A padding entry and record np - 1 lie
      // in the same aligned block of 32 -- the same wave, whose LDS reads complete in order before its writes.
      static_assert(ML_MAXPAIRS % 32 == 0, "the padded last tile must fit sP");
      if (tid < 32 * ntile) {
        MolPair q = ml_fwd_pair(sP[tid < np ? tid : np - 1]);
        if (tid >= np) q.fc = 0.f;
        sP[tid] = q;
      }
    }
    // (W2 of the first interaction -- first read by GEMM 2 of the first tile -- is staged by team 0 behind its first hidden tile,
    // while team 1 is still busy with in2f)
    if constexpr (SP) ml_stage_w1_split<KPB>(sW1h, sW1l, a.L[0].w1, a.rb.n_rbf, tid);
    else ml_stage_packed<512, NF * KPB * 2>(sW1, a.L[0].w1, a.rb.n_rbf, KPB, tid);
    if (tid < NF) { sb1[tid] = a.L[0].b1[tid]; sb2[tid] = a.L[0].b2[tid]; }

    for (int l = 0; l < a.n_layers; ++l) {
      const MolLayerDev& P = a.L[l];
      float* h_g = a.saved + (int64_t)l * a.N * (2 * NF);
      float* pre3_g = h_g + a.N * (int64_t)NF;
      float* g_g = a.gbase + (int64_t)l * a.gsz + (int64_t)p0 * NF;
      __syncthreads();
      ML_STAMP(1 + 5 * l);

      // ================= phase A: pair tiles, team 0 takes tiles 0, 2, 4, ..., team 1 in2f and then tiles 1, 3, ...
      float* zbuf = team ? sT : sY;
      f32x16 yacc;
#pragma unroll
      for (int r = 0; r < 16; ++r) yacc[r] = 0.f;
      // The loop runs over HALF-STEPS -- one block and one barrier each -- with the teams half a round apart:
      //     team 0:  hidden(0)  tile(0)    hidden(2)  tile(2)    ...
      //     team 1:  in2f       hidden(1)  tile(1)    hidden(3)  tile(3)  ...
      // Waves w and w + 4 share a SIMD: in every half-step it holds one wave in a hidden block (vector work: basis, softplus, split)
      // and one in a tile block (the GEMM 2 chain), so the matrix chain of one runs beside the vector instructions of the other
      // instead of both chains together and then both vector blocks, and team 1 does not wait out the tile block of a first round
      // in which it has only in2f: an even tile count takes one block less than rounds did, an odd one as many
      // (profiles/r14_mol_stagger.md: the blocks saved are the measured gain, the co-execution alone is none).  Each team visits
      // its tiles in the order it always did; the count of half-steps is the larger of the two teams' and the same for every wave.
      const int nh0 = 2 * ((ntile + 1) / 2), nh1 = 1 + 2 * (ntile / 2);
      const int n_half = nh0 > nh1 ? nh0 : nh1;
      for (int hs = 0; hs < n_half; ++hs) {
        const int k = hs - team;                       // the team's own half-step; team 1: -1 = in2f
        const bool in2f = k < 0;
        const int tile = in2f ? 0 : 2 * (k >> 1) + team;
        const bool active = !in2f && tile < ntile;
        const bool hidden = (k & 1) == 0;
        const int pfirst = 32 * tile;
        const int nvalid = active ? ((np - pfirst) < 32 ? (np - pfirst) : 32) : 0;
        if (in2f) {
          // ---- h[:, 32t : 32t+32] = x W_in^T  (kept in LDS for the modulation, saved for the backward)
          f32x16 acc;
          f32x4 av[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[r] = 0.f;
          ml_dense_load(av, P.in2f_p, t, lane);
          acc = ml_dense_mma(av, sX, lane, 0, acc);     // (fp32 image: this tile runs beside the other team's first pair tile, off the
                                                        //  critical path, and its split form pushed the kernel 170 B/lane further into scratch)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const f32x4 hv = {acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
            *(f32x4*)(sH + el * ML_LD + 32 * t + 8 * q + 4 * hi) = hv;
            if (el < na) spk_st<f32x4>(h_g + (size_t)a0 * NF + 32 * t, (unsigned)((el * NF + 8 * q + 4 * hi) * 4), hv);
          }
        } else if (active && hidden) {
          // ---- this wave's quarter of the hidden layer: z[pairs][32t : 32t+32] = ssp(W1 phi + b1)
          // lanes 32..63 mirror lanes 0..31; a padding lane takes the last pair's distance (split form: from the padded records)
          const float d = SP ? sP[pfirst + el].d : sP[pfirst + (el < nvalid ? el : (nvalid - 1))].d;
          f32x16 zc;
#pragma unroll
          for (int r = 0; r < 16; ++r) zc[r] = sb1[32 * t + spk_acc_row(r, hi)];
          if constexpr (SP) {
            // split form: A = the (high, low) images of W1, B = this pair's basis values in the lane's k-slots; three f16 matrix
            // instructions per k-step, the cross terms in their own accumulator
            h16x8 ph[2], pl[2], dh_[2], dl_[2];
            ml_basis_split_lin<KPB, false>(a.rb.kind, sRb, hi, d, ph, pl, dh_, dl_);
            f32x16 zx;
#pragma unroll
            for (int r = 0; r < 16; ++r) zx[r] = 0.f;
#pragma unroll
            for (int s = 0; s < (KPB > 2 ? 2 : 1); ++s) {
              h16x8 wh, wl;
              ml_w1_operand<KPB>(sW1h, sW1l, s, t * 64 + lane, wh, wl);
              SP_STEP(wh, wl, ph[s], pl[s], zc, zx);
            }
            SP_FOLD(zc, zx);
            // the hidden tile in LDS as the split A operand of GEMM 2: row = pair, [high: 128 halves | low: 128 halves], contraction
            // index in accumulator order -- the lane's registers 8 s' .. 8 s' + 7 are slot (2 t + s', hi) as they lie
            char* zr = (char*)zbuf + el * (ML_LD * 4) + 16 * hi;
#pragma unroll
            for (int sp = 0; sp < 2; ++sp) {
              float v[8];
#pragma unroll
              for (int e = 0; e < 8; ++e) v[e] = spk_fast_ssp(zc[8 * sp + e]);
              h16x8 h, l2;
              sp_split8(v, h, l2);
              *(h16x8*)(zr + 32 * (2 * t + sp)) = h;
              *(h16x8*)(zr + 256 + 32 * (2 * t + sp)) = l2;
            }
          } else {
#pragma unroll
          for (int u = 0; u < KPB; ++u) {
            const f32x4 wq = *(const f32x4*)(sW1 + ((t * KPB + u) * 64 + lane) * 4);
            float ph[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) {
              float dp;
              ml_rbf(a.rb.kind, a.rb.n_rbf, sRb, sRb + 32, 8 * u + 4 * hi + v, d, ph[v], dp);
            }
            zc = SPK_MFMA(wq.x, ph[0], zc);
            zc = SPK_MFMA(wq.y, ph[1], zc);
            zc = SPK_MFMA(wq.z, ph[2], zc);
            zc = SPK_MFMA(wq.w, ph[3], zc);
          }
#pragma unroll
          for (int q = 0; q < 4; ++q)
            *(f32x4*)(zbuf + el * ML_LD + 32 * t + 8 * q + 4 * hi) =
                f32x4{spk_fast_ssp(zc[4 * q]), spk_fast_ssp(zc[4 * q + 1]), spk_fast_ssp(zc[4 * q + 2]), spk_fast_ssp(zc[4 * q + 3])};
          }
        }
        if (l == 0 && hs == 0 && team == 0) {
          if constexpr (SP) { if (a.L[0].w2_img) ml_stage_w2_image<256>(sW2, a.L[0].w2_img, tid); else ml_stage_w2_split<256>(sW2h, sW2l, a.L[0].w2, tid); }
          else ml_stage_packed<256, NF * NF / 4>(sW2, a.L[0].w2, NF, KB2, tid);
        }
        if (active && !hidden) {      // (the barrier that ended the previous half-step completed the team's hidden tile -- and h, W2 before tile 0)
          // ---- GEMM 2, operands swapped (rows = pairs, columns = channels 32 t + el): g = W2 z + b2, A operand from LDS
          f32x16 g;
          const int c0 = 32 * t + el;
          const float bias2 = sb2[c0];
#pragma unroll
          for (int r = 0; r < 16; ++r) g[r] = bias2;
          if constexpr (SP) {
            // A = hidden tile (rows = pairs) from LDS, B = W2 image (columns = channels): both split, requested ONE k-step ahead and
            // fenced there -- the four reads of step s + 1 fly under the three matrix instructions of step s.  (Two and three steps
            // ahead keep 16 / 32 registers more in flight and gained half as much / nothing: profiles/r12_mol_matrix_overlap.md)
            constexpr int AHEAD = 1;
            f32x16 gx;
#pragma unroll
            for (int r = 0; r < 16; ++r) gx[r] = 0.f;
            const h16x8* wbh = sW2h + (t * 8) * 64 + lane;
            const h16x8* wbl = sW2l + (t * 8) * 64 + lane;
            const char* zr = (const char*)zbuf + el * (ML_LD * 4) + 16 * hi;
            h16x8 zh[8], zl[8], wh[8], wl[8];
#pragma unroll
            for (int s = 0; s < AHEAD; ++s) {
              zh[s] = *(const h16x8*)(zr + 32 * s); zl[s] = *(const h16x8*)(zr + 256 + 32 * s);
              wh[s] = wbh[s * 64]; wl[s] = wbl[s * 64];
            }
            ML_FENCE();
#pragma unroll
            for (int s = 0; s < 8; ++s) {
              if (s + AHEAD < 8) {
                zh[s + AHEAD] = *(const h16x8*)(zr + 32 * (s + AHEAD)); zl[s + AHEAD] = *(const h16x8*)(zr + 256 + 32 * (s + AHEAD));
                wh[s + AHEAD] = wbh[(s + AHEAD) * 64]; wl[s + AHEAD] = wbl[(s + AHEAD) * 64];
                ML_FENCE();
              }
              SP_STEP(zh[s], zl[s], wh[s], wl[s], g, gx);
            }
            SP_FOLD(g, gx);
          } else {
            const float* wbase = sW2 + ((int64_t)t * KB2 * 64 + lane) * 4;
            const float* zrow = zbuf + el * ML_LD + 4 * hi;
            // both operands come from LDS: requested THREE k-blocks ahead and pinned there (the one-ahead form written here
            // before was collapsed by the compiler to "two ds_reads, wait for both, four MFMAs": the LDS round trip of every
            // k-block sat in the MFMA chain)
            f32x4 wb[KB2], zb[KB2];
#pragma unroll
            for (int ug = 0; ug < 3; ++ug) { wb[ug] = *(const f32x4*)(wbase + ug * 256); zb[ug] = *(const f32x4*)(zrow + 8 * ug); }
            SPK_PIN();
#pragma unroll
            for (int ug = 0; ug < KB2; ++ug) {
              if (ug + 3 < KB2) { wb[ug + 3] = *(const f32x4*)(wbase + (ug + 3) * 256); zb[ug + 3] = *(const f32x4*)(zrow + 8 * (ug + 3)); SPK_PIN(); }
              g = SPK_MFMA(zb[ug].x, wb[ug].x, g);
              g = SPK_MFMA(zb[ug].y, wb[ug].y, g);
              g = SPK_MFMA(zb[ug].z, wb[ug].z, g);
              g = SPK_MFMA(zb[ug].w, wb[ug].w, g);
            }
          }
          // raw filter outputs for the backward (row = position of the pair in the list, 128-byte row segments per half wave)
          // ---- and modulation + accumulation on the matrix core: y[atom][c0] += [i = atom] W h[j][c0] + [j = atom] W h[i][c0]
          float* gt = g_g + 32 * t;
          if constexpr (SP) {
            // incidence product on the f16 matrix instruction: A (0 / 1, exact) carries the weight 2^-11 of the low parts itself, so
            // the accumulator that lives across the tiles stays ONE
            // Branch-free: a padding row carries the record of the tile's last pair with f_c = 0 (padded once per group, above).  The
            // hidden layer took that pair's distance for the padded lanes, so the row of g is that pair's row bit for bit and the store
            // below writes the same value to the same address again (tests/test_gpu_mol_fwd_operands.py); its weight is zero.
            const MolPair* sQ = sP + pfirst + 4 * hi;    // forward-side records: ml_fwd_pair(); row spk_acc_row(r, hi) = spk_acc_row(r, 0) + 4 hi
            const char* hcol = (const char*)(sH + c0);
            const int own = el * (ML_LD * 4);
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
              float tI[8], tJ[8];
              h16x8 ai, aj;
#pragma unroll
              for (int e = 0; e < 8; ++e) {
                const int r = 8 * s2 + e;
                const MolPair rec = sQ[spk_acc_row(r, 0)];
                const int oi = rec.ij & 0xFFFF, oj = rec.ij >> 16;
                spk_st<float>(gt, (unsigned)(__float_as_int(rec.dfc) + el * 4), g[r]);
                const float W = g[r] * rec.fc;
                tI[e] = W * *(const float*)(hcol + oj); tJ[e] = W * *(const float*)(hcol + oi);
                ai[e] = oi == own ? (_Float16)1.0f : (_Float16)0.0f;
                aj[e] = oj == own ? (_Float16)1.0f : (_Float16)0.0f;
              }
              h16x8 ih, il, jh, jl;
              sp_split8(tI, ih, il);
              sp_split8(tJ, jh, jl);
              const h16x8 ais = ai * (_Float16)SP_DOWN, ajs = aj * (_Float16)SP_DOWN;
              yacc = SP_MFMA(ai, ih, yacc);
              yacc = SP_MFMA(ais, il, yacc);
              yacc = SP_MFMA(aj, jh, yacc);
              yacc = SP_MFMA(ajs, jl, yacc);
            }
          } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int pr = spk_acc_row(r, hi);
            const bool ok = pr < nvalid;
            const MolPair rec = sP[pfirst + (ok ? pr : 0)];
            const int pi = rec.ij & 255, pj = (rec.ij >> 8) & 255;
            if (ok) spk_st<float>(gt, (unsigned)(((rec.ij >> 16) * NF + el) * 4), g[r]);
            const float W = ok ? g[r] * rec.fc : 0.f;
            const float tI = W * sH[pj * ML_LD + c0], tJ = W * sH[pi * ML_LD + c0];
            yacc = SPK_MFMA(pi == el ? 1.0f : 0.0f, tI, yacc);
            yacc = SPK_MFMA(pj == el ? 1.0f : 0.0f, tJ, yacc);
          }
          }
        }
        __syncthreads();     // hidden block: the team's hidden tile is complete; tile block: every wave of the team is done with it
      }
      ML_STAMP(2 + 5 * l);
      // the two teams' partial sums: rows = atoms spk_acc_row(r, hi), columns = channels 32 t + el
#pragma unroll
      for (int r = 0; r < 16; ++r) zbuf[spk_acc_row(r, hi) * ML_LD + 32 * t + el] = yacc[r];
      __syncthreads();
      ML_STAMP(4 + 5 * l);

      // ================= phase C1: pre3 = (y0 + y1) W3^T + b3 (saved), hidden = ssp(pre3) -> sH; the other team stages weights
      // (split instances: the wave that computes the hidden layer writes it to sH as the SPLIT IMAGE, phase C2 reads it with
      //  ml_dense_mma8_pre -- activations are split once, by whoever writes them.  The input of C1 stays on the on-the-fly form:
      //  forming and splitting y0 + y1 once costs a pass of the workgroup and a barrier, and did not shorten the phase)
      f32x4 avC[8];        // team 0: first half of the weight tile of phase C2, requested BEFORE the stores of pre3 -- loads and
                           // stores share one in-order counter, a load issued behind a store cannot be waited for without it
      if (team == 0) {
        f32x4 avA[8], avB[8];
        ml_dense_load(avA, P.o1_p, t, lane, 0);
        ml_dense_load(avB, P.o1_p, t, lane, 1);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = P.o1_b[32 * t + spk_acc_row(r, hi)];
        acc = ml_dense_mma8_sum<SP>(avA, sY, sT, lane, 0, acc);
        acc = ml_dense_mma8_sum<SP>(avB, sY, sT, lane, 1, acc);
        ml_dense_load(avC, P.o2_p, t, lane, 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 pv = {acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
          if (el < na) spk_st<f32x4>(pre3_g + (size_t)a0 * NF + 32 * t, (unsigned)((el * NF + 8 * q + 4 * hi) * 4), pv);
          const f32x4 hv = {spk_fast_ssp(pv.x), spk_fast_ssp(pv.y), spk_fast_ssp(pv.z), spk_fast_ssp(pv.w)};
          if constexpr (SP) ml_store_split4(sH, el, 32 * t + 8 * q + 4 * hi, hv);
          else *(f32x4*)(sH + el * ML_LD + 32 * t + 8 * q + 4 * hi) = hv;
        }
      } else if (l + 1 < a.n_layers) {     // the filter GEMMs of this interaction are done: their LDS images can be replaced
        const int t2 = tid - 256;
        bool staged = false;                // the split instances' one-round-trip form below has written the biases too
        if constexpr (SP) {
          if (a.L[l + 1].w2_img) {
            // every staging load of this thread is requested before the first one is used: ONE round trip to L2.  In turn -- two
            // batches of the W2 image, W1, the biases: four round trips -- this team reached the barrier 2 ... 3 k cycles behind the
            // GEMM waves, and the phase was as long as the staging (ML_WSTAMP below; profiles/r09_mol_dense_operands.md)
            f32x4 v[16];
            float x0[8], x1[8], bv1 = 0.f, bv2 = 0.f;
            ml_w2_image_load(v, a.L[l + 1].w2_img, t2);
            ml_stage_w1_load<KPB>(x0, x1, a.L[l + 1].w1, a.rb.n_rbf, t2);
            if (t2 < NF) { bv1 = a.L[l + 1].b1[t2]; bv2 = a.L[l + 1].b2[t2]; }
            SPK_PIN();
            ml_w2_image_store(sW2, v, t2);
            ml_stage_w1_store<KPB>(sW1h, sW1l, x0, x1, t2);
            if (t2 < NF) { sb1[t2] = bv1; sb2[t2] = bv2; }
            staged = true;
          } else {
            ml_stage_w2_split<256>(sW2h, sW2l, a.L[l + 1].w2, t2);
            ml_stage_w1_split<KPB>(sW1h, sW1l, a.L[l + 1].w1, a.rb.n_rbf, t2);
          }
        } else {
          ml_stage_packed<256, NF * NF / 4>(sW2, a.L[l + 1].w2, NF, KB2, t2);
          ml_stage_packed<256, NF * KPB * 2>(sW1, a.L[l + 1].w1, a.rb.n_rbf, KPB, t2);
        }
        if (!staged && t2 < NF) { sb1[t2] = a.L[l + 1].b1[t2]; sb2[t2] = a.L[l + 1].b2[t2]; }
      } else {
        if constexpr (SP) {
          if (a.head.w1) {
            // last interaction: this team stages the energy head into the images of the filter network, which nobody reads after the
            // last phase A -- outnet.0.weight as split A operand -> sW2, its bias -> sb1, outnet.1.weight -> sb2, its bias -> sW1[0];
            // one round trip, so that the head below starts from LDS (the next group's set-up overwrites all of it behind the
            // barrier at the top of the group loop)
            const MolHeadDev& Hd = a.head;
            int t2 = tid - 256;
            asm volatile("" : "+v"(t2));      // opaque: the slot addresses are formed here, not ahead of the interaction loop
            f32x4 v[16];
            float hb1 = 0.f, hw2 = 0.f, hb2 = 0.f;
            ml_head_w1_load(v, Hd.w1, Hd.H / 32, t2);
            if (t2 < Hd.H) { hb1 = Hd.b1[t2]; hw2 = Hd.w2[t2]; }
            if (t2 == 0 && Hd.b2) hb2 = Hd.b2[0];
            SPK_PIN();
            ml_head_w1_store(sW2h, sW2l, v, Hd.H / 32, t2);
            if (t2 < Hd.H) { sb1[t2] = hb1; sb2[t2] = hw2; }
            if (t2 == 0) sW1[0] = hb2;
          }
        }
      }
      if constexpr (SP) { if (l == 1) ML_WSTAMP(64); if (l == 2) ML_WSTAMP(80); }
      __syncthreads();
      ML_STAMP(5 + 5 * l);

      // ================= phase C2: x += hidden W4^T + b4
      if (team == 0) {
        f32x4 avB[8];
        ml_dense_load(avB, P.o2_p, t, lane, 1);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = P.o2_b[32 * t + spk_acc_row(r, hi)];
        if constexpr (SP) {
          acc = ml_dense_mma8_pre(avC, sH, lane, 0, acc);
          acc = ml_dense_mma8_pre(avB, sH, lane, 1, acc);
        } else {
          acc = ml_dense_mma(avC, sH, lane, 0, acc);
          acc = ml_dense_mma(avB, sH, lane, 1, acc);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float* xp = sX + el * ML_LD + 32 * t + 8 * q + 4 * hi;
          f32x4 xv = *(const f32x4*)xp;
          xv.x += acc[4 * q]; xv.y += acc[4 * q + 1]; xv.z += acc[4 * q + 2]; xv.w += acc[4 * q + 3];
          if (el >= na) xv = f32x4{0.f, 0.f, 0.f, 0.f};       // padding rows stay zero (in2f has no bias: h pads stay zero too)
          *(f32x4*)xp = xv;
          if (l + 1 == a.n_layers && el < na) spk_st<f32x4>(a.x_out + (size_t)a0 * NF + 32 * t, (unsigned)((el * NF + 8 * q + 4 * hi) * 4), xv);
          if constexpr (SP) {      // x_L once more as the split image, the B operand of the energy head (sY: last read by phase C1)
            if (l + 1 == a.n_layers) ml_store_split4(sY, el, 32 * t + 8 * q + 4 * hi, xv);
          }
        }
      }
      if constexpr (SP) {
        if (l == 1) ML_WSTAMP(72);
        // (the interaction counter re-derived through an opaque asm, like the lane in the backward's derivative task -- DESIGN.md
        //  section 4.3a.  Found by elimination, not in the listing: the per-wave stamp above alone took k_schnet_mol_fwd<3, true> from
        //  136 to 92 B per lane of scratch and the group set-up from 10.4 k to 8.6 k cycles, and of what the stamp consists of only
        //  this -- a counter the compiler cannot follow through the loop -- does the same without it; a scheduling barrier, a memory
        //  clobber or a wait in its place do not.  Presumably the per-interaction addresses are otherwise formed ahead of the loop and
        //  parked in scratch by the prologue.  profiles/r09_mol_dense_operands.md, section 2)
        asm volatile("" : "+s"(l));
      }
      // (the barrier at the top of the next interaction / group closes this phase)
    }
    if (a.head.w1) {
      // ================= energy head on the atom tile that is still in LDS: y = w2 . act(W1 x + b1) + b2, E[mol] += sum_atoms y
      const MolHeadDev& Hd = a.head;
      const int HT = Hd.H / 32;
      ML_STAMP(101);
      long long my_mol = -1;
      if (wv == 1 && lane < 32) my_mol = lane < na ? Hd.idx_m[a0 + lane] : -2;      // wave 1: molecule id of atom `lane`
      __syncthreads();                    // x_L is complete
      const int hw = wv;
      if constexpr (SP) {
        // split instances: everything the head reads is in LDS -- its weights as staged by team 1 during phase C1 of the last
        // interaction, x_L as the split image the C2 epilogue wrote to sY.  8 k-steps of three f16 matrix instructions per row tile
        // in place of 64 dependent fp32 ones behind a round trip for the weights and another for outnet.1.weight.
        if (hw < HT) {
          int ln = lane;
          asm volatile("" : "+v"(ln));      // opaque, as above: nothing of the head is prepared ahead of the group loop
          const int hi = ln >> 5, el = ln & 31;
          f32x4 av[16];
#pragma unroll
          for (int s = 0; s < 8; ++s) {
            av[2 * s] = __builtin_bit_cast(f32x4, sW2h[(hw * 8 + s) * 64 + ln]);
            av[2 * s + 1] = __builtin_bit_cast(f32x4, sW2l[(hw * 8 + s) * 64 + ln]);
          }
          f32x16 acc;
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[r] = sb1[32 * hw + spk_acc_row(r, hi)];
          acc = ml_dense_mma_sp_pre<8>(av, (const char*)sY + el * (ML_LD * 4) + 16 * hi, acc);
          float part = 0.f;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const f32x4 pv = {acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
            if (el < na) spk_st<f32x4>(Hd.pre_h + (size_t)a0 * Hd.H + 32 * hw, (unsigned)((el * Hd.H + 8 * q + 4 * hi) * 4), pv);
            const f32x4 wv2 = *(const f32x4*)(sb2 + 32 * hw + 8 * q + 4 * hi);
            if (Hd.act == SPK_ACT_SILU)
              part += pv.x * spk_fast_sigmoid(pv.x) * wv2.x + pv.y * spk_fast_sigmoid(pv.y) * wv2.y + pv.z * spk_fast_sigmoid(pv.z) * wv2.z + pv.w * spk_fast_sigmoid(pv.w) * wv2.w;
            else
              part += spk_fast_ssp(pv.x) * wv2.x + spk_fast_ssp(pv.y) * wv2.y + spk_fast_ssp(pv.z) * wv2.z + spk_fast_ssp(pv.w) * wv2.w;
          }
          part += __shfl_xor(part, 32, 64);
          if (hi == 0) sH[hw * 32 + el] = part;          // (sH: the hidden tile of the last f2out is no longer needed)
        }
      } else
      if (hw < HT) {
        f32x4 av[16];                     // (requested after the barrier: register arrays that live across one get spilled)
#pragma unroll
        for (int u = 0; u < 16; ++u) av[u] = spk_ld<f32x4>(Hd.w1 + (size_t)(32 * hw) * NF, (unsigned)((el * NF + 8 * u + 4 * hi) * 4));
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = Hd.b1[32 * hw + spk_acc_row(r, hi)];
        acc = ml_dense_mma(av, sX, lane, 0, acc);
        float part = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 pv = {acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
          if (el < na) spk_st<f32x4>(Hd.pre_h + (size_t)a0 * Hd.H + 32 * hw, (unsigned)((el * Hd.H + 8 * q + 4 * hi) * 4), pv);
          const f32x4 wv2 = *(const f32x4*)(Hd.w2 + 32 * hw + 8 * q + 4 * hi);
          if (Hd.act == SPK_ACT_SILU)
            part += pv.x * spk_fast_sigmoid(pv.x) * wv2.x + pv.y * spk_fast_sigmoid(pv.y) * wv2.y + pv.z * spk_fast_sigmoid(pv.z) * wv2.z + pv.w * spk_fast_sigmoid(pv.w) * wv2.w;
          else
            part += spk_fast_ssp(pv.x) * wv2.x + spk_fast_ssp(pv.y) * wv2.y + spk_fast_ssp(pv.z) * wv2.z + spk_fast_ssp(pv.w) * wv2.w;
        }
        part += __shfl_xor(part, 32, 64);
        if (hi == 0) sH[hw * 32 + el] = part;          // (sH: the hidden tile of the last f2out is no longer needed)
      }
      ML_STAMP(102);
      __syncthreads();
      // wave 1 holds the molecule id of atom (lane) in my_mol: segment heads add their run, one atomic per (group, molecule)
      if (wv == 1) {
        float y = 0.f;
        if (lane < 32) {
          if constexpr (SP) y = sW1[0];                 // outnet.1.bias as staged with the head's weights (0 when there is none)
          else y = Hd.b2 ? Hd.b2[0] : 0.f;
          for (int w = 0; w < HT; ++w) y += sH[w * 32 + lane];
          if (lane >= na) y = 0.f;
        }
        const long long first_mol = __shfl(my_mol, 0, 64);
        if (__all(lane >= na || my_mol == first_mol)) {
          // the whole group is one molecule (the usual case): a butterfly over the 32 atom lanes (y is 0 beyond na)
          float sum = y;
#pragma unroll
          for (int m = 16; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, 64);
          if (lane == 0 && na > 0) { if (Hd.direct_store) Hd.E[my_mol] = sum; else unsafeAtomicAdd(Hd.E + my_mol, sum); }
        } else {
          const long long prev = __shfl_up(my_mol, 1, 64);
          const bool head_of_run = lane < na && (lane == 0 || prev != my_mol);
          float sum = 0.f;
          for (int b = 0; b < 32; ++b) {               // runs are contiguous: every head walks forward while the id matches
            const float yb = spk_readlane_f(y, b);
            const long long mb = __shfl(my_mol, b, 64);
            if (head_of_run && b >= lane && b < na && mb == my_mol) sum += yb;
          }
          if (head_of_run) { if (Hd.direct_store) Hd.E[my_mol] = sum; else unsafeAtomicAdd(Hd.E + my_mol, sum); }
        }
      }
    }
    ML_STAMP(31);
  }
}

// ------------------------------------------------------------------------------------------ host side
static long long* g_mol_dbg = nullptr;
// tuning aid (scripts/mol_timing.py; include/spk_hip.h): device buffer of int64 that receives cycle stamps -- entries
// [0, 128): phases of thread 0 of workgroup 0 (64-87: per-wave stamps of forward Dense phases, 101 / 102: the energy head); [128 + 4 b, 128 + 4 b + 4): real-time and cycle stamps at the start / end of workgroup b
// of the backward launch, so the buffer must hold 128 + 4 * (number of groups) entries.  NULL: off (production)
extern "C" void spk_schnet_mol_set_debug_buffer(void* p) { g_mol_dbg = (long long*)p; }
// derivative tasks per pair tile in phase E of the backward: 0 = automatic (the rule at the task queue of k_schnet_mol_bwd), 1, 2
static int g_mol_bwd_task_split = 0;
extern "C" void spk_schnet_mol_set_bwd_task_split(int split) { g_mol_bwd_task_split = (split == 1 || split == 2) ? split : 0; }

// set-up of the backward: 0 = automatic (pair records from the records region of `saved` where the forward left one), 1 = always
// recompute them (the chain half -> idx_i, idx_j -> R, the form before), 2 = require the region (an error where there is none).
// The forward writes the region whenever it exists: 1 against 2 is an A/B of the backward alone.
static int g_mol_bwd_records = 0;
extern "C" void spk_schnet_mol_set_bwd_records(int mode) { g_mol_bwd_records = (mode == 1 || mode == 2) ? mode : 0; }
int spk_schnet_mol_bwd_records_mode() { return g_mol_bwd_records; }
// the records region inside `saved` (spk_schnet_mol_records_region) as device pointers
static MolHandoff mol_handoff(const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb, int64_t gsz, const float* saved) {
  MolHandoff h = {nullptr, nullptr, nullptr, nullptr};
  int64_t off = 0, floats = 0;
  if (gsz <= 0 || !spk_schnet_mol_records_region(m, g, rb, &off, &floats)) return h;
  float* base = const_cast<float*>(saved) + off;       // 16-byte aligned: rec | vec | map | np
  h.rec = (MolPair*)base;
  h.vec = base + 4 * (int64_t)g->n_half;
  h.map = (int*)(base + 7 * (int64_t)g->n_half);
  h.np = (int*)(base + 8 * (int64_t)g->n_half);
  return h;
}

static size_t mol_w1_floats(int kpb, bool sp) {      // LDS floats of the staged W1 image(s): MlW1Image<KPB>::BYTES twice in the split form
  return sp ? (size_t)2 * (4096 + (kpb > 2 ? (kpb == 4 ? 4096 : 2048) : 0)) / 4 : (size_t)128 * kpb * 8;
}
static size_t mol_fwd_lds(int kpb, bool sp) {
  return (size_t)(128 * 128 + mol_w1_floats(kpb, sp) + 2 * 128 + 4 * 32 * ML_LD + 64 + 8) * sizeof(float) + ML_MAXPAIRS * sizeof(MolPair);
}

// Shapes / lists the molecule-resident kernels cover (everything else runs the general driver of spk_schnet.hip).
bool spk_schnet_mol_eligible(const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb) {
  const int variant = spk_get_variant();
  if (variant != SPK_VARIANT_AUTO && variant != SPK_VARIANT_MFMA_PAIR && variant != SPK_VARIANT_MFMA) return false;
  if (getenv("SPK_NO_MOL")) return false;
  if (m->n_atom_basis != 128 || m->n_filters != 128 || m->n_interactions < 1 || m->n_interactions > ML_MAXL || !m->wpack) return false;
  const int kpb = (rb->n_rbf + 7) / 8;
  if (kpb < 1 || kpb > 4) return false;
  if (!(g->symmetric && g->sorted && g->half && g->rev && g->edge_pair && g->rowptr && g->n_half > 0)) return false;
  if (g->n_groups <= 0 || !g->grp_atom0 || !g->grp_pair0 || g->max_group_atoms > 32) return false;
  if (g->max_group_pairs <= 0 || g->max_group_pairs > ML_MAXPAIRS) return false;
  if (g->n_half_dev) return false;       // a per-call compacted pair list is already in place
  // (skin lists, g->filter_pairs: pairs beyond the cutoff carry f_c = f_c' = 0 and contribute exactly zero here -- no compaction)
  return true;
}

template <int KPB, bool SP>
static int launch_mol_fwd_sp(const MolFwdArgs& a, hipStream_t stream);
template <int KPB>
static int launch_mol_fwd(const MolFwdArgs& a, hipStream_t stream) {
  return spk_get_split() ? launch_mol_fwd_sp<KPB, true>(a, stream) : launch_mol_fwd_sp<KPB, false>(a, stream);
}
template <int KPB, bool SP>
static int launch_mol_fwd_sp(const MolFwdArgs& a, hipStream_t stream) {
  const size_t lds = mol_fwd_lds(KPB, SP);
  auto kern = k_schnet_mol_fwd<KPB, SP>;
  static SpkPerDevice attr_set;
  int attr_dev;
  if (attr_set.pending(&attr_dev)) {
    SPK_HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr_set.mark(attr_dev);
  }
  int grid = a.n_groups;
  const int maxg = spk_num_cus();
  if (grid > maxg) grid = maxg;
  SpkProfScope prof("schnet_mol_fwd", stream);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, stream, a);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

// `saved` as laid out by spk_schnet_saved_floats_graph(): L x (h | pre3), then L x gsz floats of raw filter outputs, then (lists the
// pair kernels would compact) the space of the per-call pair list, which these launches leave alone, then -- model word bit 1, lists
// the molecule-resident backward covers -- the records region: per record of a group its MolPair, per list position the pair vector
// and the record index, per group the number of records (MolHandoff; spk_schnet_mol_records_region()).
int spk_schnet_mol_forward(const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb, const SpkPackTable& ptab,
                           const float* x0, const float* r_ij, float* x_out, float* saved, int64_t gsz, hipStream_t stream) {
  return spk_schnet_mol_forward_ex(m, g, rb, ptab, x0, r_ij, nullptr, nullptr, nullptr, x_out, saved, gsz, stream);
}
int spk_schnet_mol_forward_ex(const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb, const SpkPackTable& ptab,
                              const float* x0, const float* r_ij, const float* R, const float* offsets, const MolHeadDev* head, float* x_out,
                              float* saved, int64_t gsz, hipStream_t stream, const float* emb, const int64_t* Z, int n_types) {
  MolFwdArgs a;
  a.R = R; a.offsets = offsets;
  a.emb = emb; a.Z = Z; a.n_types = n_types;
  if (head) a.head = *head; else a.head.w1 = nullptr;
  const bool split = spk_get_split() != 0;     // the launch takes the same decision (launch_mol_fwd): split images for the split kernels
  a.n_layers = m->n_interactions;
  for (int l = 0; l < m->n_interactions; ++l) {
    const spk_schnet_layer_t& P = m->layers[l];
    MolLayerDev& D = a.L[l];
    D.in2f_p = spk_packed_of(ptab, P.in2f_w, 0);
    D.o1_p = split ? spk_packed_split_of(ptab, P.f2out_w1, 0) : spk_packed_of(ptab, P.f2out_w1, 0);
    D.o2_p = split ? spk_packed_split_of(ptab, P.f2out_w2, 0) : spk_packed_of(ptab, P.f2out_w2, 0);
    SPK_CHECK_ARG(D.in2f_p && D.o1_p && D.o2_p, "spk_schnet_mol_forward: packed weight images missing");
    D.w1 = P.fn_w1; D.b1 = P.fn_b1; D.w2 = P.fn_w2; D.b2 = P.fn_b2; D.o1_b = P.f2out_b1; D.o2_b = P.f2out_b2;
    D.w2_img = split ? ptab.extra_of(P.fn_w2) : nullptr;
  }
  a.x0 = x0; a.x_out = x_out; a.rij = r_ij; a.idx_i = g->idx_i; a.idx_j = g->idx_j;
  a.half = g->half; a.rowptr = g->rowptr; a.edge_pair = g->edge_pair; a.grp_atom0 = g->grp_atom0; a.grp_pair0 = g->grp_pair0;
  a.n_groups = g->n_groups; a.saved = saved; a.N = g->n_atoms; a.gsz = gsz;
  a.gbase = saved + (int64_t)m->n_interactions * g->n_atoms * (m->n_filters + m->n_atom_basis);
  a.rb = spk_radial_dev(rb);
  a.compact = spk_schnet_mol_bwd_eligible(m, g, rb) ? 1 : 0;     // only when the molecule-resident backward (which compacts too) will consume `saved`
  a.ho = mol_handoff(m, g, rb, gsz, saved);
  a.dbg = g_mol_dbg;
  switch ((rb->n_rbf + 7) / 8) {
    case 1: return launch_mol_fwd<1>(a, stream);
    case 2: return launch_mol_fwd<2>(a, stream);
    case 3: return launch_mol_fwd<3>(a, stream);
    case 4: return launch_mol_fwd<4>(a, stream);
  }
  spk_set_error("spk_schnet_mol_forward: n_rbf = %d unsupported", rb->n_rbf);
  return SPK_ERR_ARG;
}

// ==========================================================================================================
// Backward (first order, what Forces asks for): dL/dr_ij and optionally dL/dx0 from dL/dx_L, one launch.
//
// Per interaction, last to first (notation of SURVEY.md Appendix B; everything below is local to the group):
//   D1. gt = (gx W4) * ssp'(pre3)          D2. gy = gt W3                                (two T-GEMM phases)
//   E.  task queue:  derivative tasks (one per pair tile)  +  row-sum tasks  +  the four tiles of G
//         derivative task: phi, phi' -> GEMM 1 value and derivative (a, a') -> z' = sigmoid(a) a' -- the hidden layer, once per
//           pair tile: it does not depend on the channel tile -- then a loop over the two channel-tile pairs tp: GEMM 2' (rows =
//           channels, columns = pairs: lane = pair) -> D = g' f_c + g f_c' with the SAVED raw filter outputs g ->
//           s1 = sum_c gy_i h_j D,  s2 = sum_c gy_j h_i D  (in-lane sums over the 16 channels a lane owns, one LDS add per
//           pair and tp, in the order tp = 0, 1: one wave builds a pair's sum in one fixed order); the per-pair sums are kept in
//           LDS across all interactions and become dL/dr once, at the end.  (spk_schnet_mol_set_bwd_task_split(2): one task
//           per (pair tile, tp), the hidden layer twice per tile -- the form before; the rule of the automatic choice is at the queue)
//         row-sum task:    gh[a] = sum_{b in row(a)} gy[b] * g[pair(a,b)] * f_c           (the transpose of the forward row sum)
//         G task (channel tile t): gx[:, 32 t : 32 t + 32] += gh W_in -- waits for the row sums only (LDS counter)
// ==========================================================================================================
struct MolBwdLayerDev {
  const float *w1, *b1, *w2;               // filter network (raw)
  const float* w2_img;                     // split-precision LDS image of w2 (wpack), or null
  const float *in2f_t, *o1_t, *o2_t;       // packed input-gradient images of in2f / f2out.0 / f2out.1
};

struct MolBwdArgs {
  MolBwdLayerDev L[ML_MAXL];
  int n_layers;
  const float* gx_out;      // [N, 128]
  float* gx0;               // [N, 128] or null
  float* gr;                // [E, 3], assigned (may be null when gR is asked for)
  const float* rij;         // [E, 3], or null: from R / offsets
  const float* R;
  const float* offsets;
  float* gR;                // [N, 3] or null: dL/dR, every entry written (the pairwise transpose folded in)
  MolHeadDev head;          // head.w1t != null: dL/dx_L comes from the energy head (+ gx_out when that is given)
  const int64_t* idx_i;
  const int64_t* idx_j;
  const int32_t *half, *rev, *rowptr, *edge_pair, *grp_atom0, *grp_pair0;
  int n_groups;
  const float* saved;
  const float* gbase;
  int64_t gsz, N;
  RadialDev rb;
  int compact;              // as in the forward
  int task_split;           // derivative tasks per pair tile in phase E: 0 = automatic, 1, 2 (spk_schnet_mol_set_bwd_task_split)
  MolHandoff ho;            // records region of `saved` as the forward of this call left it (rec == null: recompute the records)
  long long* dbg;
};

// HO: the pair records of a group come from the records region of `saved` (a.ho); the instances without it carry the recomputing
// set-up alone (both in one kernel cost the split instances 48 B per lane of scratch: profiles/r11_mol_bwd_setup.md)
template <int KPB, bool SP, bool HO>
__global__ __launch_bounds__(512) void k_schnet_mol_bwd(MolBwdArgs a) {
  constexpr int NF = 128, NT = 4, KB2 = 16;
  constexpr int W1F = SP ? 2 * MlW1Image<KPB>::BYTES / 4 : NF * KPB * 8;     // floats of the W1 image(s)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sW2 = smem;                                  // NF*NF  (SP: high image | low image, 32 KB each)
  float* sW1 = sW2 + NF * NF;                         // NF*KPB*8  (SP: high image | low image)
  float* sb1 = sW1 + W1F;                             // NF (+ NF unused: same footprint as the forward)
  h16x8* const sW2h = (h16x8*)sW2;
  h16x8* const sW2l = sW2h + 2048;
  char* const sW1h = (char*)sW1;
  char* const sW1l = sW1h + MlW1Image<KPB>::BYTES;
  float* sGx = sb1 + 2 * NF;                          // [32][ML_LD] dL/dx of the current level
  float* sH = sGx + 32 * ML_LD;                       // h_l (saved by the forward)
  float* sGy = sH + 32 * ML_LD;                       // dL/dy_l
  float* sGh = sGy + 32 * ML_LD;                      // dL/dh_l; before that the hidden gradient of f2out
  MolPair* sP = (MolPair*)(sGh + 32 * ML_LD);         // per pair: local atoms, d, f_c, f_c'
  int2* sEb = (int2*)(sP + ML_MAXPAIRS);              // per directed edge: ((local pair << 8) | local neighbour, f_c)
  int* sRow = (int*)(sEb + ML_MAXEDGES);              // [33]
  int* sCnt = sRow + 36;                              // [4]
  float* sRb = (float*)(sCnt + 4);                    // [2][32] radial basis parameters
  float* sS = sRb + 64;                               // [ML_MAXPAIRS][2] per-pair geometry sums, all interactions
  short* sMap = (short*)(sS + 2 * ML_MAXPAIRS);       // [ML_MAXPAIRS] position in the pair list -> record (-1: beyond the cutoff)
  int* sScan = (int*)(sMap + ML_MAXPAIRS);            // [8]

  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);   // wv: SGPR
  const int hi = lane >> 5, el = lane & 31;
  if constexpr (SP) ml_basis_table(sRb, a.rb, tid);          // as in the forward: ml_basis_split_lin()
  else if (tid < 64) {
    const int k = tid & 31;
    const float* src = (tid < 32) ? a.rb.p0 : a.rb.p1;
    sRb[tid] = (src && k < a.rb.n_rbf) ? src[k] : 1.0f;
  }

  if (a.dbg && tid == 0) { a.dbg[128 + 4 * blockIdx.x] = (long long)__builtin_amdgcn_s_memrealtime(); a.dbg[130 + 4 * blockIdx.x] = (long long)__builtin_readcyclecounter(); }
  for (int grp = blockIdx.x; grp < a.n_groups; grp += gridDim.x) {
    const int a0 = a.grp_atom0[grp], na = a.grp_atom0[grp + 1] - a0;
    const int p0 = a.grp_pair0[grp], np_list = a.grp_pair0[grp + 1] - p0;
    const int e0 = a.rowptr[a0], ne = a.rowptr[a0 + na] - e0;
    const int Ltop = a.n_layers - 1;
    __syncthreads();

    // ---- group set-up.  Everything here is short and latency-bound, so the independent pieces share their round trips and
    //      barriers: the head's hidden gradient is filled while the pair records are loaded (the first barrier inside
    //      ml_pair_records() publishes both), the head GEMM (waves 0-3) runs beside the per-edge records (waves 4-7), and the
    //      filter weights of the top interaction are staged by the idle half of the two Dense phases below -- the derivative tasks
    //      of phase E are their first reader.
    const bool with_head = a.head.w1t != nullptr;
    constexpr bool handoff = HO;
    MolPair ho_pr = {0, 0.f, 0.f, 0.f};
    int ho_map = -1, ho_np = 0;
    float pr3[3] = {0.f, 0.f, 0.f};      // this thread's pair vector: used again at the very end (dL/dr, dL/dR) without going back to memory
    for (int s = tid; s < 32 * 32; s += 512) {
      const int row = s >> 5, c4 = s & 31;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (row < na && a.gx_out) v = spk_ld<f32x4>(a.gx_out + (size_t)a0 * NF, (unsigned)(s * 16));
      *(f32x4*)(sGx + row * ML_LD + 4 * c4) = v;
      *(f32x4*)(sH + row * ML_LD + 4 * c4) = f32x4{0.f, 0.f, 0.f, 0.f};
      if (!with_head) *(f32x4*)(sGh + row * ML_LD + 4 * c4) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    ML_STAMP(120);
    // With the records region of `saved` (written by the forward of this call: ml_pair_records() there) a thread requests its
    // record, its map entry and its pair vector here, in one round of independent loads in front of those of the head: no chain
    // half -> idx_i, idx_j -> R, no distance, no cutoff function, no ballot / prefix -- and one barrier, not two.  (Requested at the
    // top of the group instead, in front of the feature gradient, the set-up is as long: profiles/r11_mol_bwd_setup.md)
    if constexpr (handoff) {
      ho_np = a.ho.np[grp];
      ho_np = ho_np < 0 ? 0 : (ho_np > np_list ? np_list : ho_np);      // (never beyond the group's span of the region)
      if (tid < np_list) {
        ho_map = spk_ld<int>(a.ho.map + p0, (unsigned)tid * 4u);
        pr3[0] = spk_ld<float>(a.ho.vec + 3 * (size_t)p0, (unsigned)tid * 12u);
        pr3[1] = spk_ld<float>(a.ho.vec + 3 * (size_t)p0, (unsigned)tid * 12u + 4u);
        pr3[2] = spk_ld<float>(a.ho.vec + 3 * (size_t)p0, (unsigned)tid * 12u + 8u);
      }
      if (tid < ho_np) ho_pr = spk_ld<MolPair>(a.ho.rec + p0, (unsigned)tid * 16u);
    }
    if (with_head) {
      // ---- dL/dx_L through the energy head, part 1: the hidden gradient gE[mol] w2 . act'(pre_h) -> sGh[:, :H]
      //      (the columns beyond H are not read by part 2, and the first Dense phase rewrites sGh in full)
      const MolHeadDev& Hd = a.head;
      for (int s = tid; s < 32 * Hd.H; s += 512) {
        const int row = s / Hd.H, k = s - row * Hd.H;
        float v = 0.f;
        if (row < na) {
          const float pre = Hd.pre_h[(size_t)(a0 + row) * Hd.H + k];
          const float sg = spk_fast_sigmoid(pre);
          const float da = Hd.act == SPK_ACT_SILU ? sg * (1.0f + pre * (1.0f - sg)) : sg;
          v = (Hd.gE ? Hd.gE[Hd.idx_m[a0 + row]] : 1.0f) * Hd.w2[k] * da;
        }
        sGh[row * ML_LD + k] = v;
      }
    }
    int np;
    if constexpr (handoff) {
      if (tid < np_list) sMap[tid] = (short)ho_map;
      if (tid < ho_np) sP[tid] = ho_pr;
      __syncthreads();        // publishes the records and the head's hidden gradient
      np = ho_np;
    } else {
      np = ml_pair_records(sP, sMap, sScan, a.half, a.rij, a.R, a.offsets, a.idx_i, a.idx_j, p0, np_list, a0, a.rb.cutoff, a.compact != 0, tid, pr3);
    }
    const int ntile = (np + 31) / 32;
    ML_STAMP(123);
    if (wv < NT) {
      if (with_head) {
        // ---- part 2: gx += hidden gradient x W1
        const MolHeadDev& Hd = a.head;
        const int KH = Hd.H / 8;
        const int t = wv;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const float* brow = sGh + el * ML_LD + 4 * hi;
        for (int c = 0; c < KH; c += 8) {            // H is a multiple of 32 (KH of 4): chunks of eight k-blocks, masked (A = rows of W1^T)
          f32x4 a8[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            a8[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (c + u < KH) a8[u] = spk_ld<f32x4>(Hd.w1t + (size_t)(32 * t) * Hd.H, (unsigned)((el * Hd.H + 8 * (c + u) + 4 * hi) * 4));
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            if (c + u < KH) {
              const f32x4 bv = *(const f32x4*)(brow + 8 * (c + u));
              acc = SPK_MFMA(a8[u].x, bv.x, acc);
              acc = SPK_MFMA(a8[u].y, bv.y, acc);
              acc = SPK_MFMA(a8[u].z, bv.z, acc);
              acc = SPK_MFMA(a8[u].w, bv.w, acc);
            }
          }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float* xp = sGx + el * ML_LD + 32 * t + 8 * q + 4 * hi;
          f32x4 xv = *(const f32x4*)xp;
          xv.x += acc[4 * q]; xv.y += acc[4 * q + 1]; xv.z += acc[4 * q + 2]; xv.w += acc[4 * q + 3];
          if (el >= na) xv = f32x4{0.f, 0.f, 0.f, 0.f};
          *(f32x4*)xp = xv;
        }
      }
    } else {
      // per directed edge: (row of the saved filter tensor << 8 | local neighbour, f_c); edges of dropped pairs point at the
      // first record's row with weight 0 (their own row was never written)
      const int t2 = tid - 256;
      const int row0 = np > 0 ? (sP[0].ij >> 16) : 0;
      for (int s = t2; s < ne; s += 256) {
        const int pos = spk_ld<int>(a.edge_pair + e0, (unsigned)s * 4u) - p0;
        const int rec = sMap[pos];
        const int nb = (int)(spk_ld<long long>(a.idx_j + e0, (unsigned)s * 8u) - a0);
        sEb[s] = rec >= 0 ? make_int2((pos << 8) | nb, __float_as_int(sP[rec].fc)) : make_int2((row0 << 8) | nb | (1 << 24), 0);
      }
      for (int s = t2; s < 2 * np; s += 256) sS[s] = 0.f;
      if (t2 <= na) sRow[t2] = a.rowptr[a0 + t2] - e0;
    }
    __syncthreads();
    ML_STAMP(32);

    for (int l = Ltop; l >= 0; --l) {
      const MolBwdLayerDev& P = a.L[l];
      const float* h_g = a.saved + (int64_t)l * a.N * (2 * NF);
      const float* pre3_g = h_g + a.N * (int64_t)NF;
      const float* g_g = a.gbase + (int64_t)l * a.gsz + (int64_t)p0 * NF;
      const bool last = (l == 0) && !a.gx0;     // nothing below consumes dL/dh_0: no row sums, no in2f transpose

      // ================= D1: gt = (gx W4) * ssp'(pre3);  the other half stages W2 of this interaction's filter network
      if (wv < NT) {
        const int t = wv;
        f32x4 avA[8], avB[8];
        ml_dense_load(avA, P.o2_t, t, lane, 0);
        ml_dense_load(avB, P.o2_t, t, lane, 1);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        f32x4 pv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          pv[q] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (el < na) pv[q] = spk_ld<f32x4>(pre3_g + (size_t)a0 * NF + 32 * t, (unsigned)((el * NF + 8 * q + 4 * hi) * 4));
        }
        acc = ml_dense_mma<SP>(avA, sGx, lane, 0, acc);
        acc = ml_dense_mma<SP>(avB, sGx, lane, 1, acc);
#pragma unroll
        for (int q = 0; q < 4; ++q)
          *(f32x4*)(sGh + el * ML_LD + 32 * t + 8 * q + 4 * hi) =
              f32x4{acc[4 * q] * spk_fast_sigmoid(pv[q].x), acc[4 * q + 1] * spk_fast_sigmoid(pv[q].y), acc[4 * q + 2] * spk_fast_sigmoid(pv[q].z), acc[4 * q + 3] * spk_fast_sigmoid(pv[q].w)};
      } else {
        // (sW2 was last read by the derivative tasks of the interaction above: two barriers ago)
        if constexpr (SP) { if (P.w2_img) ml_stage_w2_image<256>(sW2, P.w2_img, tid - 256); else ml_stage_w2_split<256>(sW2h, sW2l, P.w2, tid - 256); }
        else ml_stage_packed<256, NF * NF / 4>(sW2, P.w2, NF, KB2, tid - 256);
      }
      if (tid == 0) { sCnt[0] = 0; sCnt[1] = 0; }
      __syncthreads();
      ML_STAMP(33 + 6 * (Ltop - l));

      // ================= D2: gy = gt W3;  the other half loads h_l and stages W1, b1
      if (wv < NT) {
        const int t = wv;
        f32x4 avA[8], avB[8];
        ml_dense_load(avA, P.o1_t, t, lane, 0);
        ml_dense_load(avB, P.o1_t, t, lane, 1);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        acc = ml_dense_mma<SP>(avA, sGh, lane, 0, acc);
        acc = ml_dense_mma<SP>(avB, sGh, lane, 1, acc);
#pragma unroll
        for (int q = 0; q < 4; ++q)
          *(f32x4*)(sGy + el * ML_LD + 32 * t + 8 * q + 4 * hi) = f32x4{acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
      } else {
        const int t2 = tid - 256;
        for (int s = t2; s < na * 32; s += 256) {
          const int row = s >> 5, c4 = s & 31;
          *(f32x4*)(sH + row * ML_LD + 4 * c4) = spk_ld<f32x4>(h_g + (size_t)a0 * NF, (unsigned)(s * 16));
        }
        if constexpr (SP) ml_stage_w1_split<KPB>(sW1h, sW1l, P.w1, a.rb.n_rbf, t2);
        else ml_stage_packed<256, NF * KPB * 2>(sW1, P.w1, a.rb.n_rbf, KPB, t2);
        if (t2 < NF) sb1[t2] = P.b1[t2];
      }
      __syncthreads();
      ML_STAMP(34 + 6 * (Ltop - l));

      // ================= E: derivative tasks (pair tile, pair of channel tiles) + row-sum tasks (one atom, all channels)
      // The queue hands out the derivative tasks first, then the row sums, then -- unless nothing below consumes dL/dx -- the four
      // channel tiles of G (gx += gh W_in): G only waits for the row sums (a counter in LDS), not for the derivative tasks, so it
      // runs on the waves that the derivative tasks leave idle instead of being a phase of its own.
      // A derivative task covers pair tile `tile` and the channel-tile pairs [tp0, tp1): the hidden layer of the filter network does
      // not depend on the channel tile, so a task computes it once and loops over its channel-tile pairs behind it.  `split` tasks
      // per tile (uniform over the group): 1 = one task does both pairs (hidden layer once per tile), 2 = one pair each (twice).
      // Automatic = 1 for every group.  The candidate exception -- two tasks per tile while they fit one round, 2 ntile <= 8 -- lost
      // where it would apply (profiles/r07_mol_bwd_task_split.md; backward launch, 1 against 2 tasks per tile): 256 ethanol frames,
      // groups of 2 ... 4 tiles, 61.7 against 65.9 us; 16-atom blobs, 8 tiles, 76.5 against 92.1 us; aspirin, 5 tiles, 63.6 against
      // 73.0 us -- spread of the call times 0.2 ... 0.4 us.
      const int split = a.task_split ? a.task_split : 1;
      const int nder = split * ntile;
      const int nrow = (last || np == 0) ? 0 : na;
      const int ng = last ? 0 : NT;
      if (np == 0 && !last) {    // no pair inside the cutoff: dL/dh = 0 (the buffer still holds the hidden gradient of f2out)
        for (int s = tid; s < 32 * 32; s += 512) *(f32x4*)(sGh + (s >> 5) * ML_LD + 4 * (s & 31)) = f32x4{0.f, 0.f, 0.f, 0.f};
        __syncthreads();         // (uniform over the workgroup)
      }
      while (true) {
        int k = 0;
        if (lane == 0) k = atomicAdd(&sCnt[0], 1);
        k = __builtin_amdgcn_readfirstlane(k);
        if (k >= nder + nrow + ng) break;
        if (k >= nder + nrow) {
          // ---- G, channel tile t: gx[:, 32 t : 32 t + 32] += gh W_in (weights requested before the wait for the row sums)
          const int t = k - nder - nrow;
          f32x4 avA[8], avB[8];
          ml_dense_load(avA, P.in2f_t, t, lane, 0);
          ml_dense_load(avB, P.in2f_t, t, lane, 1);
          if (nrow > 0) {
            while (__hip_atomic_load(&sCnt[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < nrow) __builtin_amdgcn_s_sleep(2);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
          }
          f32x16 acc;
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[r] = 0.f;
          acc = ml_dense_mma<SP>(avA, sGh, lane, 0, acc);
          acc = ml_dense_mma<SP>(avB, sGh, lane, 1, acc);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            float* xp = sGx + el * ML_LD + 32 * t + 8 * q + 4 * hi;
            f32x4 xv = *(const f32x4*)xp;
            xv.x += acc[4 * q]; xv.y += acc[4 * q + 1]; xv.z += acc[4 * q + 2]; xv.w += acc[4 * q + 3];
            if (el >= na) xv = f32x4{0.f, 0.f, 0.f, 0.f};
            *(f32x4*)xp = xv;
            if (l == 0 && el < na) spk_st<f32x4>(a.gx0 + (size_t)a0 * NF + 32 * t, (unsigned)((el * NF + 8 * q + 4 * hi) * 4), xv);
          }
          continue;
        }
        if (k >= nder) {
          // ---- gh[a][c] = sum over the row of a of gy[b][c] g[pair][c] f_c
          ml_row_sums4<10>(sGh, sGy, g_g, sEb, sRow, k - nder, lane);
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
          if (lane == 0) atomicAdd(&sCnt[1], 1);
          continue;
        }
        const int tile = split == 2 ? k >> 1 : k;
        const int tp0 = split == 2 ? (k & 1) : 0, tp1 = split == 2 ? tp0 + 1 : 2;
        const int pfirst = 32 * tile;
        const int nvalid = (np - pfirst) < 32 ? (np - pfirst) : 32;
        const bool valid = el < nvalid;
        const int pl = pfirst + (valid ? el : (nvalid - 1));
        const MolPair pr = sP[pl];
        const float fc = valid ? pr.fc : 0.f, dfc = valid ? pr.dfc : 0.f;
        const int pi = pr.ij & 255, pj = (pr.ij >> 8) & 255;
        const int grow = pr.ij >> 16;                       // row of this pair in the saved filter tensor
        float* const sums = sS + 2 * pl;                    // this pair's (s1, s2)
        if constexpr (SP) {
          // ---- split form (spk_split.h).  GEMM 1, value and derivative, for the four hidden tiles: A = the W1 images, B = this pair's
          // basis values / slopes in the lane's k-slots; z' = sigmoid(a) a' goes from the accumulator registers into the B operand
          // of GEMM 2' as it lies (W2 is staged with its contraction index in accumulator order).
          // (lane re-derived through an opaque asm: the LDS offsets below are then formed here and not hoisted out of the task loop
          //  into the prologue of the kernel, where the allocator parks them in scratch -- section 4.3a of DESIGN.md)
          int lane_o = lane;
          asm volatile("" : "+v"(lane_o));
          const int hi_o = lane_o >> 5;
          h16x8 ph[2], pl[2], dh[2], dl[2];
          ml_basis_split_lin<KPB, true>(a.rb.kind, sRb, hi_o, pr.d, ph, pl, dh, dl);
          h16x8 zph[NT][2], zpl[NT][2];
#pragma unroll
          for (int c = 0; c < NT; ++c) {
            f32x16 zc, zcx, zq, zqx;
#pragma unroll
            for (int r = 0; r < 16; ++r) { zc[r] = sb1[32 * c + spk_acc_row(r, hi_o)]; zcx[r] = 0.f; zq[r] = 0.f; zqx[r] = 0.f; }
#pragma unroll
            for (int s = 0; s < (KPB > 2 ? 2 : 1); ++s) {
              h16x8 wh, wl;
              ml_w1_operand<KPB>(sW1h, sW1l, s, c * 64 + lane_o, wh, wl);
              SP_STEP(wh, wl, ph[s], pl[s], zc, zcx);
              SP_STEP(wh, wl, dh[s], dl[s], zq, zqx);
            }
#pragma unroll
            for (int sp = 0; sp < 2; ++sp) {
              float v[8];
#pragma unroll
              for (int e = 0; e < 8; ++e) {
                const int r = 8 * sp + e;
                v[e] = fmaf(zqx[r], SP_DOWN, zq[r]) * spk_fast_sigmoid(fmaf(zcx[r], SP_DOWN, zc[r]));
              }
              sp_split8(v, zph[c][sp], zpl[c][sp]);
            }
          }
          // ---- GEMM 2' per channel tile (rows = channels 32 t + spk_acc_row(r, hi), columns = pairs): g' = W2 z'
          const float* gyi_p = sGy + pi * ML_LD + 4 * hi_o;
          const float* gyj_p = sGy + pj * ML_LD + 4 * hi_o;
          const float* hi_p = sH + pi * ML_LD + 4 * hi_o;
          const float* hj_p = sH + pj * ML_LD + 4 * hi_o;
#pragma unroll 1
          for (int tp = tp0; tp < tp1; ++tp) {
            // the saved raw filter outputs of this lane's pair for both channel tiles of the pair: requested in front of the
            // matrix instructions of this iteration, used behind them
            f32x4 gl[2][4];
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
              for (int q = 0; q < 4; ++q) gl[tt][q] = spk_ld<f32x4>(g_g + 64 * tp, (unsigned)((grow * NF + 4 * hi + 32 * tt + 8 * q) * 4));
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
              const int t = 2 * tp + tt;
              f32x16 gp, gpx;
#pragma unroll
              for (int r = 0; r < 16; ++r) { gp[r] = 0.f; gpx[r] = 0.f; }
              const h16x8* wbh = sW2h + (t * 8) * 64 + lane_o;
              const h16x8* wbl = sW2l + (t * 8) * 64 + lane_o;
              h16x8 wh[8], wl[8];
#pragma unroll
              for (int s = 0; s < 2; ++s) { wh[s] = wbh[s * 64]; wl[s] = wbl[s * 64]; }
              ML_FENCE();      // (fenced: with the pin alone every k-step waited for reads issued directly in front of it)
#pragma unroll
              for (int s = 0; s < 8; ++s) {
                if (s + 2 < 8) { wh[s + 2] = wbh[(s + 2) * 64]; wl[s + 2] = wbl[(s + 2) * 64]; ML_FENCE(); }
                SP_STEP(wh[s], wl[s], zph[s >> 1][s & 1], zpl[s >> 1][s & 1], gp, gpx);
              }
              SP_FOLD(gp, gpx);
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                const int col = 32 * t + 8 * q;
                const f32x4 gyi = *(const f32x4*)(gyi_p + col), gyj = *(const f32x4*)(gyj_p + col);
                const f32x4 hvi = *(const f32x4*)(hi_p + col), hvj = *(const f32x4*)(hj_p + col);
                const f32x4 gq = gl[tt][q];
                const float D0 = gp[4 * q] * fc + gq.x * dfc, D1 = gp[4 * q + 1] * fc + gq.y * dfc;
                const float D2 = gp[4 * q + 2] * fc + gq.z * dfc, D3 = gp[4 * q + 3] * fc + gq.w * dfc;
                s1 += gyi.x * hvj.x * D0 + gyi.y * hvj.y * D1 + gyi.z * hvj.z * D2 + gyi.w * hvj.w * D3;
                s2 += gyj.x * hvi.x * D0 + gyj.y * hvi.y * D1 + gyj.z * hvi.z * D2 + gyj.w * hvi.w * D3;
              }
            }
            // one partial per channel-tile pair, added in the order tp = 0, 1 (the LDS operations of a wave stay in order): with one
            // task per tile the sum of a pair is built by one wave in one order
            s1 += __shfl_xor(s1, 32, 64);
            s2 += __shfl_xor(s2, 32, 64);
            if (hi == 0 && valid) { atomicAdd(sums, s1); atomicAdd(sums + 1, s2); }
          }
        } else {
        float phi[KPB][4], dphi[KPB][4];
#pragma unroll
        for (int u = 0; u < KPB; ++u)
#pragma unroll
          for (int v = 0; v < 4; ++v) ml_rbf(a.rb.kind, a.rb.n_rbf, sRb, sRb + 32, 8 * u + 4 * hi + v, pr.d, phi[u][v], dphi[u][v]);
        // ---- GEMM 1, value and derivative (rows = hidden channels, columns = pairs): z' = sigmoid(W1 phi + b1) * (W1 phi')
        // Software-pipelined by hand: a wave issues in order, so an activation block placed between two MFMA groups leaves the
        // matrix pipe idle for its whole length.  The MFMAs of hidden tile c + 1 are therefore interleaved with the activations
        // of tile c (one or two of its 16 accumulator rows per MFMA pair): the VALU work runs in the shadow of the MFMAs.
        f32x16 zp[NT];
        {
          constexpr int NSTEP = 4 * KPB;
          f32x4 wq = *(const f32x4*)(sW1 + lane * 4);
          f32x16 zc, zq;
#pragma unroll
          for (int r = 0; r < 16; ++r) { zc[r] = sb1[spk_acc_row(r, hi)]; zq[r] = 0.f; }
#pragma unroll
          for (int u = 0; u < KPB; ++u) {
            f32x4 wn = wq;
            if (u + 1 < NT * KPB) wn = *(const f32x4*)(sW1 + ((u + 1) * 64 + lane) * 4);
            zc = SPK_MFMA(wq.x, phi[u][0], zc); zq = SPK_MFMA(wq.x, dphi[u][0], zq);
            zc = SPK_MFMA(wq.y, phi[u][1], zc); zq = SPK_MFMA(wq.y, dphi[u][1], zq);
            zc = SPK_MFMA(wq.z, phi[u][2], zc); zq = SPK_MFMA(wq.z, dphi[u][2], zq);
            zc = SPK_MFMA(wq.w, phi[u][3], zc); zq = SPK_MFMA(wq.w, dphi[u][3], zq);
            wq = wn;
          }
#pragma unroll
          for (int c = 0; c < NT; ++c) {
            f32x16 zcn = zc, zqn = zq;
            if (c + 1 < NT) {
#pragma unroll
              for (int r = 0; r < 16; ++r) { zcn[r] = sb1[32 * (c + 1) + spk_acc_row(r, hi)]; zqn[r] = 0.f; }
#pragma unroll
              for (int u = 0; u < KPB; ++u) {
                const int nxt = (c + 1) * KPB + u + 1;
                f32x4 wn = wq;
                if (nxt < NT * KPB) wn = *(const f32x4*)(sW1 + (nxt * 64 + lane) * 4);
                const float wv4[4] = {wq.x, wq.y, wq.z, wq.w};
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                  zcn = SPK_MFMA(wv4[v], phi[u][v], zcn);
                  zqn = SPK_MFMA(wv4[v], dphi[u][v], zqn);
                  const int st = 4 * u + v;
#pragma unroll
                  for (int r = (16 * st) / NSTEP; r < (16 * (st + 1)) / NSTEP; ++r) {
                    zq[r] *= spk_fast_sigmoid(zc[r]);
                  }
                }
                wq = wn;
              }
            } else {
#pragma unroll
              for (int r = 0; r < 16; ++r) {
                zq[r] *= spk_fast_sigmoid(zc[r]);
              }
            }
            zp[c] = zq;
            zc = zcn; zq = zqn;
          }
        }
        // ---- GEMM 2' per channel tile (rows = channels 32 t + spk_acc_row(r, hi), columns = pairs): g' = W2 z'
        const float* gyi_p = sGy + pi * ML_LD + 4 * hi;
        const float* gyj_p = sGy + pj * ML_LD + 4 * hi;
        const float* hi_p = sH + pi * ML_LD + 4 * hi;
        const float* hj_p = sH + pj * ML_LD + 4 * hi;
#pragma unroll 1
        for (int tp = tp0; tp < tp1; ++tp) {
          // the saved raw filter outputs of this lane's pair for both channel tiles of the pair: requested in front of the
          // matrix instructions of this iteration, used behind them
          f32x4 gl[2][4];
#pragma unroll
          for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int q = 0; q < 4; ++q) gl[tt][q] = spk_ld<f32x4>(g_g + 64 * tp, (unsigned)((grow * NF + 4 * hi + 32 * tt + 8 * q) * 4));
          float s1 = 0.f, s2 = 0.f;
#pragma unroll
          for (int tt = 0; tt < 2; ++tt) {
            const int t = 2 * tp + tt;
            f32x16 gp;
#pragma unroll
            for (int r = 0; r < 16; ++r) gp[r] = 0.f;
            {
              // weights from LDS, requested three k-blocks ahead and pinned there (the one-ahead form was collapsed by the compiler
              // to "ds_read, wait, four MFMAs": a derivative task alone on its SIMD then waits out the LDS round trip of every k-block)
              const float* wbase = sW2 + ((int64_t)t * KB2 * 64 + lane) * 4;
              f32x4 wb[KB2];
#pragma unroll
              for (int ug = 0; ug < 3; ++ug) wb[ug] = *(const f32x4*)(wbase + ug * 256);
              SPK_PIN();
#pragma unroll
              for (int ug = 0; ug < KB2; ++ug) {
                const int c = ug >> 2, q = ug & 3;
                if (ug + 3 < KB2) { wb[ug + 3] = *(const f32x4*)(wbase + (ug + 3) * 256); SPK_PIN(); }
                gp = SPK_MFMA(wb[ug].x, zp[c][4 * q + 0], gp);
                gp = SPK_MFMA(wb[ug].y, zp[c][4 * q + 1], gp);
                gp = SPK_MFMA(wb[ug].z, zp[c][4 * q + 2], gp);
                gp = SPK_MFMA(wb[ug].w, zp[c][4 * q + 3], gp);
              }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const int col = 32 * t + 8 * q;
              const f32x4 gyi = *(const f32x4*)(gyi_p + col), gyj = *(const f32x4*)(gyj_p + col);
              const f32x4 hvi = *(const f32x4*)(hi_p + col), hvj = *(const f32x4*)(hj_p + col);
              const f32x4 gq = gl[tt][q];
              const float D0 = gp[4 * q] * fc + gq.x * dfc, D1 = gp[4 * q + 1] * fc + gq.y * dfc;
              const float D2 = gp[4 * q + 2] * fc + gq.z * dfc, D3 = gp[4 * q + 3] * fc + gq.w * dfc;
              s1 += gyi.x * hvj.x * D0 + gyi.y * hvj.y * D1 + gyi.z * hvj.z * D2 + gyi.w * hvj.w * D3;
              s2 += gyj.x * hvi.x * D0 + gyj.y * hvi.y * D1 + gyj.z * hvi.z * D2 + gyj.w * hvi.w * D3;
            }
          }
          // one partial per channel-tile pair, added in the order tp = 0, 1 (the LDS operations of a wave stay in order): with one
          // task per tile the sum of a pair is built by one wave in one order
          s1 += __shfl_xor(s1, 32, 64);
          s2 += __shfl_xor(s2, 32, 64);
          if (hi == 0 && valid) { atomicAdd(sums, s1); atomicAdd(sums + 1, s2); }
        }
        }
      }
      ML_STAMP(35 + 6 * (Ltop - l));
      __syncthreads();
      ML_STAMP(36 + 6 * (Ltop - l));
      if (last) break;

    }

    // ---- dL/dr of both directions of every pair, once for all interactions (pairs beyond the cutoff: zero); with gR the pair's
    //      contribution (s1 + s2) r / d is parked in LDS for the per-atom pass below (sGh is free by now)
    float* sV = sGh;                                    // [ML_MAXPAIRS][3]
    if (a.gR) __syncthreads();
    if (tid < np_list) {                                // one pair per thread (np_list <= ML_MAXPAIRS < 512), its vector still in registers
      const int s = tid;
      const int rec = sMap[s];
      float s1 = 0.f, s2 = 0.f;
      if (rec >= 0) {
        const float d = sP[rec].d;
        const float inv = d > 0.f ? 1.0f / d : 0.f;
        s1 = sS[2 * rec] * inv; s2 = sS[2 * rec + 1] * inv;
      }
      const float rx = pr3[0], ry = pr3[1], rz = pr3[2];
      if (a.gr) {
        const int64_t e = a.half[p0 + s];
        const int64_t e2 = a.rev[e];
        a.gr[3 * e] = s1 * rx; a.gr[3 * e + 1] = s1 * ry; a.gr[3 * e + 2] = s1 * rz;
        a.gr[3 * e2] = -s2 * rx; a.gr[3 * e2 + 1] = -s2 * ry; a.gr[3 * e2 + 2] = -s2 * rz;
      }
      if (a.gR && rec >= 0) {
        const float w = s1 + s2;
        sV[3 * rec] = w * rx; sV[3 * rec + 1] = w * ry; sV[3 * rec + 2] = w * rz;
      }
    }
    // ---- dL/dR: the transpose of r_ij = R_j - R_i + offsets, per atom over its row (each pair of the atom appears once
    //      there): the pair (i, j) with canonical vector r gives -(s1 + s2) r / d to i and +(s1 + s2) r / d to j.  Fixed order.
    if (a.gR) {
      __syncthreads();
      // eight lanes per (atom, component): they walk the row's edges with stride 8 and meet by shuffles (fixed order)
      const int slot = tid & 7, q = tid >> 3;          // q < 64 >= 3 * na / ... : na <= 21 atoms fill 63 of the 64 groups; larger groups loop
      for (int s = q; s < 3 * na; s += 64) {
        const int at = s / 3, comp = s - 3 * at;
        float acc = 0.f;
        for (int e = sRow[at] + slot; e < sRow[at + 1]; e += 8) {
          const int x = sEb[e].x;
          if (x & (1 << 24)) continue;
          const int rec = sMap[(x >> 8) & 0xFFFF];
          const float v = sV[3 * rec + comp];
          acc += ((sP[rec].ij & 255) == at) ? -v : v;
        }
        acc += __shfl_xor(acc, 1, 64);
        acc += __shfl_xor(acc, 2, 64);
        acc += __shfl_xor(acc, 4, 64);
        if (slot == 0) a.gR[3 * (size_t)(a0 + at) + comp] = a.head.negate ? -acc : acc;
      }
    }
    ML_STAMP(63);
  }
  if (a.dbg && tid == 0) { a.dbg[129 + 4 * blockIdx.x] = (long long)__builtin_amdgcn_s_memrealtime(); a.dbg[131 + 4 * blockIdx.x] = (long long)__builtin_readcyclecounter(); }
}

static size_t mol_bwd_lds(int kpb, bool sp) {
  return (size_t)(128 * 128 + mol_w1_floats(kpb, sp) + 2 * 128 + 4 * 32 * ML_LD + 64 + 2 * ML_MAXPAIRS) * sizeof(float) + ML_MAXPAIRS * sizeof(MolPair) +
         (2 * ML_MAXEDGES + 36 + 4 + 8) * sizeof(int) + ML_MAXPAIRS * sizeof(short);
}

template <int KPB, bool SP, bool HO>
static int launch_mol_bwd_sp(const MolBwdArgs& a, hipStream_t stream);
template <int KPB>
static int launch_mol_bwd(const MolBwdArgs& a, hipStream_t stream) {
  if (a.ho.rec) return spk_get_split() ? launch_mol_bwd_sp<KPB, true, true>(a, stream) : launch_mol_bwd_sp<KPB, false, true>(a, stream);
  return spk_get_split() ? launch_mol_bwd_sp<KPB, true, false>(a, stream) : launch_mol_bwd_sp<KPB, false, false>(a, stream);
}
template <int KPB, bool SP, bool HO>
static int launch_mol_bwd_sp(const MolBwdArgs& a, hipStream_t stream) {
  const size_t lds = mol_bwd_lds(KPB, SP);
  auto kern = k_schnet_mol_bwd<KPB, SP, HO>;
  static SpkPerDevice attr_set;
  int attr_dev;
  if (attr_set.pending(&attr_dev)) {
    SPK_HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr_set.mark(attr_dev);
  }
  int grid = a.n_groups;
  const int maxg = spk_num_cus();
  if (grid > maxg) grid = maxg;
  SpkProfScope prof("schnet_mol_bwd", stream);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, stream, a);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

// n_rbf up to 24 (3 k-blocks): the LDS budget of the backward (per-pair sums) ends there; wider bases take the general driver
bool spk_schnet_mol_bwd_eligible(const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb) {
  return spk_schnet_mol_eligible(m, g, rb) && (rb->n_rbf + 7) / 8 <= 3 && !getenv("SPK_NO_MOL_BWD");
}

int spk_schnet_mol_backward(const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb, const SpkPackTable& ptab,
                            const float* gx_out, const float* r_ij, const float* saved, int64_t gsz, float* gr, float* gx0,
                            hipStream_t stream) {
  return spk_schnet_mol_backward_ex(m, g, rb, ptab, gx_out, r_ij, nullptr, nullptr, nullptr, saved, gsz, gr, nullptr, gx0, stream);
}
int spk_schnet_mol_backward_ex(const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb, const SpkPackTable& ptab,
                               const float* gx_out, const float* r_ij, const float* R, const float* offsets, const MolHeadDev* head,
                               const float* saved, int64_t gsz, float* gr, float* gR, float* gx0, hipStream_t stream) {
  MolBwdArgs a;
  a.R = R; a.offsets = offsets; a.gR = gR;
  if (head) a.head = *head; else { a.head.w1 = nullptr; a.head.w1t = nullptr; a.head.negate = 0; }
  const bool split = spk_get_split() != 0;
  a.n_layers = m->n_interactions;
  for (int l = 0; l < m->n_interactions; ++l) {
    const spk_schnet_layer_t& P = m->layers[l];
    MolBwdLayerDev& D = a.L[l];
    D.in2f_t = split ? spk_packed_split_of(ptab, P.in2f_w, 1) : spk_packed_of(ptab, P.in2f_w, 1);
    D.o1_t = split ? spk_packed_split_of(ptab, P.f2out_w1, 1) : spk_packed_of(ptab, P.f2out_w1, 1);
    D.o2_t = split ? spk_packed_split_of(ptab, P.f2out_w2, 1) : spk_packed_of(ptab, P.f2out_w2, 1);
    SPK_CHECK_ARG(D.in2f_t && D.o1_t && D.o2_t, "spk_schnet_mol_backward: packed weight images missing");
    D.w1 = P.fn_w1; D.b1 = P.fn_b1; D.w2 = P.fn_w2;
    D.w2_img = split ? ptab.extra_of(P.fn_w2) : nullptr;
  }
  a.gx_out = gx_out; a.gx0 = gx0; a.gr = gr; a.rij = r_ij; a.idx_i = g->idx_i; a.idx_j = g->idx_j;
  a.half = g->half; a.rev = g->rev; a.rowptr = g->rowptr; a.edge_pair = g->edge_pair; a.grp_atom0 = g->grp_atom0; a.grp_pair0 = g->grp_pair0;
  a.n_groups = g->n_groups; a.saved = saved; a.N = g->n_atoms; a.gsz = gsz;
  a.gbase = saved + (int64_t)m->n_interactions * g->n_atoms * (m->n_filters + m->n_atom_basis);
  a.rb = spk_radial_dev(rb);
  a.compact = 1;
  a.dbg = g_mol_dbg;
  a.task_split = g_mol_bwd_task_split;
  a.ho = mol_handoff(m, g, rb, gsz, saved);
  SPK_CHECK_ARG(g_mol_bwd_records != 2 || a.ho.rec, "spk_schnet_mol_backward: records mode 2, but `saved` of this model / list has no records region");
  if (g_mol_bwd_records == 1) a.ho.rec = nullptr;
  switch ((rb->n_rbf + 7) / 8) {
    case 1: return launch_mol_bwd<1>(a, stream);
    case 2: return launch_mol_bwd<2>(a, stream);
    case 3: return launch_mol_bwd<3>(a, stream);
  }
  spk_set_error("spk_schnet_mol_backward: n_rbf = %d unsupported", rb->n_rbf);
  return SPK_ERR_ARG;
}
