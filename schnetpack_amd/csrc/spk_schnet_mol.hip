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
//
// Kernels: k_schnet_mol_fwd<KPB, SP> and k_schnet_mol_bwd<KPB, SP, HO> (further down), one launch each -- and k_schnet_mol_force<KPB>,
// the FORCE CALL of the standard potential in one launch: the same two bodies back to back in one kernel, a group's backward in the
// workgroup that ran its forward (spk_schnet_mol_force_ex; which calls take it: schnet_potential_forces in spk_schnet.hip).  The bodies
// live in spk_schnet_mol_fwd_body.h / spk_schnet_mol_bwd_body.h and are included as text into the kernels that run them.
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
#include "spk_schnet_mol_fwd_body.h"
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
static int mol_fwd_args(MolFwdArgs& a, const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb, const SpkPackTable& ptab,
                        const float* x0, const float* r_ij, const float* R, const float* offsets, const MolHeadDev* head, float* x_out,
                        float* saved, int64_t gsz, const float* emb, const int64_t* Z, int n_types);
int spk_schnet_mol_forward(const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb, const SpkPackTable& ptab,
                           const float* x0, const float* r_ij, float* x_out, float* saved, int64_t gsz, hipStream_t stream) {
  return spk_schnet_mol_forward_ex(m, g, rb, ptab, x0, r_ij, nullptr, nullptr, nullptr, x_out, saved, gsz, stream);
}
int spk_schnet_mol_forward_ex(const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb, const SpkPackTable& ptab,
                              const float* x0, const float* r_ij, const float* R, const float* offsets, const MolHeadDev* head, float* x_out,
                              float* saved, int64_t gsz, hipStream_t stream, const float* emb, const int64_t* Z, int n_types) {
  MolFwdArgs a;
  SPK_TRY(mol_fwd_args(a, m, g, rb, ptab, x0, r_ij, R, offsets, head, x_out, saved, gsz, emb, Z, n_types));
  switch ((rb->n_rbf + 7) / 8) {
    case 1: return launch_mol_fwd<1>(a, stream);
    case 2: return launch_mol_fwd<2>(a, stream);
    case 3: return launch_mol_fwd<3>(a, stream);
    case 4: return launch_mol_fwd<4>(a, stream);
  }
  spk_set_error("spk_schnet_mol_forward: n_rbf = %d unsupported", rb->n_rbf);
  return SPK_ERR_ARG;
}
// the argument block of a forward launch (shared with the one-launch force call)
static int mol_fwd_args(MolFwdArgs& a, const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb, const SpkPackTable& ptab,
                        const float* x0, const float* r_ij, const float* R, const float* offsets, const MolHeadDev* head, float* x_out,
                        float* saved, int64_t gsz, const float* emb, const int64_t* Z, int n_types) {
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
  return SPK_OK;
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
#include "spk_schnet_mol_bwd_body.h"
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

// ==========================================================================================================
// The force call in ONE launch: forward and backward of the standard potential (spk_schnet.hip: schnet_potential_forces) back to
// back in one kernel -- the two bodies above as they are, split path and records hand-over on.  Both launches use the same grid and
// the same loop over the groups, so a group's backward runs in the workgroup that ran its forward, and it reads nothing another
// workgroup wrote: dL/dE is 1 on this route, the energies are outputs only.  What goes away is a launch boundary per call.
// The argument block is the two launches' blocks side by side (about 1.6 KB of the 4 KB kernarg segment): both bodies index their
// table of interactions with a run-time counter, which needs the table in memory as the kernarg segment has it, and the existing
// kernels keep their layouts -- the geometry pointers the two have in common are what is stored twice.
// ==========================================================================================================
struct MolForceArgs { MolFwdArgs f; MolBwdArgs b; };
static_assert(sizeof(MolForceArgs) <= 2048, "the kernarg segment of k_schnet_mol_force stays well under 4 KB");

template <int KPB>
__global__ __launch_bounds__(512) void k_schnet_mol_force(MolForceArgs fa) {
  constexpr bool SP = true, HO = true;
  {
    const MolFwdArgs& a = fa.f;
#include "spk_schnet_mol_fwd_body.h"
  }
  // Between the halves: the forward wrote h, pre3, the raw filter rows g, the records region and pre_h with global stores, and OTHER
  // threads of this workgroup read them below.  Release / barrier / acquire at WORKGROUP scope suffices: the eight waves of a
  // workgroup sit on one compute unit and share its vector L1, which writes through -- a wave's release waits for its stores, and a
  // load issued behind the barrier by any wave of the same unit sees them.  No line of these buffers can be stale in that L1 either:
  // the workgroup reads none of them before it has written its groups' part.  (Nothing of another workgroup is read, so nothing
  // wider than the workgroup is needed; the compiler, which sees the stores, keeps the loads below off the scalar cache.)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  {
    const MolBwdArgs& a = fa.b;
#include "spk_schnet_mol_bwd_body.h"
  }
}

template <int KPB>
static int launch_mol_force(const MolForceArgs& a, hipStream_t stream) {
  const size_t lf = mol_fwd_lds(KPB, true), lb = mol_bwd_lds(KPB, true);
  const size_t lds = lf > lb ? lf : lb;
  auto kern = k_schnet_mol_force<KPB>;
  static SpkPerDevice attr_set;
  int attr_dev;
  if (attr_set.pending(&attr_dev)) {
    SPK_HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr_set.mark(attr_dev);
  }
  int grid = a.f.n_groups;
  const int maxg = spk_num_cus();
  if (grid > maxg) grid = maxg;
  SpkProfScope prof("schnet_mol_force", stream);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, stream, a);
  SPK_LAUNCH_CHECK();
  return SPK_OK;
}

// n_rbf up to 24 (3 k-blocks): the LDS budget of the backward (per-pair sums) ends there; wider bases take the general driver
bool spk_schnet_mol_bwd_eligible(const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb) {
  return spk_schnet_mol_eligible(m, g, rb) && (rb->n_rbf + 7) / 8 <= 3 && !getenv("SPK_NO_MOL_BWD");
}

static int mol_bwd_args(MolBwdArgs& a, const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb, const SpkPackTable& ptab,
                        const float* gx_out, const float* r_ij, const float* R, const float* offsets, const MolHeadDev* head,
                        const float* saved, int64_t gsz, float* gr, float* gR, float* gx0);
int spk_schnet_mol_backward(const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb, const SpkPackTable& ptab,
                            const float* gx_out, const float* r_ij, const float* saved, int64_t gsz, float* gr, float* gx0,
                            hipStream_t stream) {
  return spk_schnet_mol_backward_ex(m, g, rb, ptab, gx_out, r_ij, nullptr, nullptr, nullptr, saved, gsz, gr, nullptr, gx0, stream);
}
int spk_schnet_mol_backward_ex(const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb, const SpkPackTable& ptab,
                               const float* gx_out, const float* r_ij, const float* R, const float* offsets, const MolHeadDev* head,
                               const float* saved, int64_t gsz, float* gr, float* gR, float* gx0, hipStream_t stream) {
  MolBwdArgs a;
  SPK_TRY(mol_bwd_args(a, m, g, rb, ptab, gx_out, r_ij, R, offsets, head, saved, gsz, gr, gR, gx0));
  switch ((rb->n_rbf + 7) / 8) {
    case 1: return launch_mol_bwd<1>(a, stream);
    case 2: return launch_mol_bwd<2>(a, stream);
    case 3: return launch_mol_bwd<3>(a, stream);
  }
  spk_set_error("spk_schnet_mol_backward: n_rbf = %d unsupported", rb->n_rbf);
  return SPK_ERR_ARG;
}
// the argument block of a backward launch (shared with the one-launch force call)
static int mol_bwd_args(MolBwdArgs& a, const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb, const SpkPackTable& ptab,
                        const float* gx_out, const float* r_ij, const float* R, const float* offsets, const MolHeadDev* head,
                        const float* saved, int64_t gsz, float* gr, float* gR, float* gx0) {
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
  return SPK_OK;
}

// ---- the force call: one launch or two.  0 = automatic (one launch where the call is eligible and the per-launch profile is off:
// the profile's unit is the launch, and its tags schnet_mol_fwd / schnet_mol_bwd are how the two halves are told apart and booked),
// 1 = one launch even with the profile on (tag schnet_mol_force; an error where the call is not eligible), 2 = always two launches.
// SPK_MOL_FORCE_LAUNCHES in the environment sets the initial value: one build runs both ways under an unmodified caller.
static int g_mol_force_launches = [] { const char* e = getenv("SPK_MOL_FORCE_LAUNCHES"); return (e && (e[0] == '1' || e[0] == '2') && !e[1]) ? e[0] - '0' : 0; }();
extern "C" void spk_schnet_mol_set_force_launches(int mode) { g_mol_force_launches = (mode == 1 || mode == 2) ? mode : 0; }
int spk_schnet_mol_force_launches() { return g_mol_force_launches; }
// eligible: the split path is on, `saved` has a records region and the backward is not told to ignore it
bool spk_schnet_mol_force_eligible(const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb, int64_t gsz) {
  int64_t off = 0, floats = 0;
  return spk_get_split() != 0 && g_mol_bwd_records != 1 && gsz > 0 && spk_schnet_mol_bwd_eligible(m, g, rb) &&
         spk_schnet_mol_records_region(m, g, rb, &off, &floats);
}
int spk_schnet_mol_force_ex(const spk_schnet_t* m, const spk_graph_t* g, const spk_radial_t* rb, const SpkPackTable& ptab, const float* x0,
                            const float* R, const float* offsets, const MolHeadDev* head, float* x_out, float* saved, int64_t gsz, float* gr,
                            float* gR, hipStream_t stream, const float* emb, const int64_t* Z, int n_types) {
  SPK_CHECK_ARG(head && head->w1 && head->w1t && !head->gE, "spk_schnet_mol_force: the one-launch call is the forces route (energy head, dL/dE = 1)");
  SPK_CHECK_ARG(spk_schnet_mol_force_eligible(m, g, rb, gsz), "spk_schnet_mol_force: call not eligible for one launch (split path off, or no records region in `saved`, or records mode 1)");
  MolForceArgs a;
  SPK_TRY(mol_fwd_args(a.f, m, g, rb, ptab, x0, nullptr, R, offsets, head, x_out, saved, gsz, emb, Z, n_types));
  SPK_TRY(mol_bwd_args(a.b, m, g, rb, ptab, nullptr, nullptr, R, offsets, head, saved, gsz, gr, gR, nullptr));
  SPK_CHECK_ARG(a.f.ho.rec && a.b.ho.rec, "spk_schnet_mol_force: no records region");
  switch ((rb->n_rbf + 7) / 8) {
    case 1: return launch_mol_force<1>(a, stream);
    case 2: return launch_mol_force<2>(a, stream);
    case 3: return launch_mol_force<3>(a, stream);
  }
  spk_set_error("spk_schnet_mol_force: n_rbf = %d unsupported", rb->n_rbf);
  return SPK_ERR_ARG;
}
