// Body of the molecule-resident SchNet forward (spk_schnet_mol.hip), included as text into k_schnet_mol_fwd<KPB, SP> and into the
// one-launch force call k_schnet_mol_force<KPB>.  In scope at the point of inclusion: the template constants KPB and SP, and `a`, the
// MolFwdArgs of the launch.  Text, not a device function: with the body behind a by-value or by-reference parameter the existing
// instances compile to other register allocations (k_schnet_mol_bwd<3, false, false> 56 -> 144 B per lane of scratch, over its
// budget; profiles/r15_mol_force_launch.md), included in place they compile to the instructions they had.
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
