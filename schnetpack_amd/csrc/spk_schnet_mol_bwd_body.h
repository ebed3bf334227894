// Body of the molecule-resident SchNet backward (spk_schnet_mol.hip), included as text into k_schnet_mol_bwd<KPB, SP, HO> and into the
// one-launch force call k_schnet_mol_force<KPB>.  In scope at the point of inclusion: the template constants KPB, SP and HO, and `a`,
// the MolBwdArgs of the launch.  (Why text: spk_schnet_mol_fwd_body.h.)
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
