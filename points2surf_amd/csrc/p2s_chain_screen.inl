// Screened conv3 (K = 128, N = 1024) + exact max-pool of ONE point tile -- textually included by p2s_chain.hip inside
// p2s_chain_kernel<false, true> (the same reason as p2s_chain_conv3.inl: the pooled state stays in registers / LDS).
//
// conv3 feeds only a max over the item's points: of the P x 1024 dot products 1024 reach the output.  This path decides on
// the fp16-pair MFMA which products can be the maximum and computes only those in fp32:
//   screen   t[p][c] = acc0 + acc1 * 2^-11 on v_mfma_f32_32x32x16_f16, h and w as fp16 pairs (the arithmetic of
//            p2s_chain_bf16_kernel<2, true>: 3 MFMAs per product at 1/16 of the fp32 MFMA's cost each);
//   margin   mu_c = 2 (k_screen + k_fp32) (|w_c| + 2^-10) (H + 2^-10),  H >= |h_p| for every row of every tile of the item so
//            far, this one included (a running maximum: the margin only grows from tile to tile);
//   select   (p, c) is a candidate iff t[p][c] >= R_c - mu_c, R_c = the running maximum of t[.][c] over the tiles so far,
//            this one included -- every record-breaker is a candidate;
//   confirm  each candidate at once, while its fp32 row h[p] is still in LDS: one chain of 128 fmaf in the k order of the
//            32x32x2 MFMA chain of p2s_chain_conv3.inl (k-groups ascending, t = 0..3, 8g+t then 8g+4+t; rows of the 16-row
//            tail: the two half chains, then one add), one lane per candidate;  E_c = max of the confirmed values.
//
// Exactness.  Write s*_x for the real-number dot product of row x, fl(s_x) for the fp32 chain, d_x >= |t_x - s*_x| and
// g_x >= |fl(s_x) - s*_x|; both scale with |w_c| |h_x|: d_x + g_x <= (k_screen + k_fp32) (|w_c| + 2^-10) (|h_x| + 2^-10).  A
// dismissed p had t_p < R - mu_c at its tile, with R = t_q of a row q of THAT OR AN EARLIER tile that was a candidate when it
// set the record (t_q = R >= R - mu_c; if q is a padding row, the item's last point, which it replicates, has the same
// operands and lies within d of it).  mu_c is built from H >= max(|h_p|, |h_q|) -- the running maximum over the tiles so
// far, not this tile's alone: the record holder may be a row of larger norm than any of the current tile -- so
// (d_p + g_p) + (d_q + g_q) <= mu_c and
//     fl(s_p) <= s*_p + g_p <= t_p + d_p + g_p < t_q - mu_c + d_p + g_p <= t_q - d_q - g_q <= s*_q - g_q <= fl(s_q):
// p cannot hold the maximum over all P fp32 values and E_c is that maximum: the value p2s_chain_kernel<false> pools.
//
// The two k, per unit |w_c| |h_p| (>= sum |w| |h|):
//   operands    an fp16 pair keeps |x - (h0 + h1 2^-11)| <= 2^-22 |x| + 2^-36 (the second term: pieces below fp16's normal
//               range).  Both operands: 2 * 2^-22; the absolute parts are what the + 2^-10 of the margin's two factors pay for
//               (2^-22 * 2^-10 >= 2^-36 * sqrt(128));
//   h1 h1'      the dropped piece product: 2^-22;
//   screen sum  8 MFMAs of 16 exact products each into an fp32 accumulator; allowing every one of the 136 additions a
//               truncation (2^-23, twice round-to-nearest) of a partial sum <= sum |w| |h|: 136 * 2^-23 = 2^-15.9;
//               the second accumulator enters times 2^-11, the final fma adds 2^-24;
//   fp32 chain  128 roundings of a partial sum <= sum |w| |h|, again allowing truncation: 128 * 2^-23 = 2^-16 (the tail
//               rows' extra add included in the slack).
//   k_screen + k_fp32 <= 2^-15.8 + 2^-16 < 2^-14 = P2S_SCR_KAPPA, the constant the coefficients are built with (1.8 x slack).
//
// What the screen cannot decide runs densely: an item with an activation beyond the half range, or with more candidates
// in one column tile than the wave's queue holds (a patch of identical points: every product ties), sets `undec`, and the
// workgroup runs the item again through the dense conv3 (p2s_chain_kernel's own) when its screened pass ends.
{
            unsigned short *hp0 = reinterpret_cast<unsigned short *>(bufA);      // h0 [64][SCR_HB] over the conv2 input tile
            unsigned short *hp1 = reinterpret_cast<unsigned short *>(scr_h1);    // h1 [64][SCR_HB]
            // ---- the weight stream: ONE ring over the tile's 8 column tiles x 8 k-blocks ---------------------------------
            // A wave's fragments of consecutive k-blocks and column tiles are consecutive KBs of the packed pieces, so the
            // stream does not know column tiles: the fragments of k-block j + 3 are requested while the MFMAs of k-block j
            // issue (4 slots of 2 x 4 registers, 3 in flight), across the select, the queue and the confirm of a column tile
            // too.  The first three are requested here and land during the split.  (The last three requests of a tile run
            // past the wave's own fragments: they read the next wave's, or, past the end of the buffer, zeros; nothing uses them.)
            const int soff0 = wave * 8 * 8 * 1024;          // bytes: 8 k-blocks of 64 lanes x 16 B per column tile
            u32x4 rb0[4], rb1[4];
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                rb0[s] = scr_bufld(rs3h, lane16, soff0 + s * 1024);
                rb1[s] = scr_bufld(rs3h, lane16, (int)(P2S_SCR_PIECE * 2) + soff0 + s * 1024);
            }
            float mu_c = scr_mu[256 * wave + (lane & 31)];                       // margin coefficient of column tile 0
            // ---- h -> fp16 pair beside the fp32 tile; row norms --------------------------------------------------------
            if (scr_abl != 5) {
                const int p = tid >> 2, q = tid & 3;
                const float *src = bufB + p * SB + 32 * q;
                float ss = 0.0f;
                bool oor = false;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const f32x4 v0 = lds4(src + 8 * i), v1 = lds4(src + 8 * i + 4);
                    unsigned q0[4], q1[4];
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        scr_split(v0[2 * u], v0[2 * u + 1], q0[u], q1[u]);
                        scr_split(v1[2 * u], v1[2 * u + 1], q0[2 + u], q1[2 + u]);
                    }
                    const u32x4 w0 = {q0[0], q0[1], q0[2], q0[3]}, w1 = {q1[0], q1[1], q1[2], q1[3]};
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        ss = fmaf(v0[u], v0[u], ss);
                        ss = fmaf(v1[u], v1[u], ss);
                        oor = oor || p2s_f16_out_of_range(v0[u]) || p2s_f16_out_of_range(v1[u]);
                    }
                    *reinterpret_cast<u32x4 *>(hp0 + p * SCR_HB + 32 * q + 8 * i) = w0;
                    *reinterpret_cast<u32x4 *>(hp1 + p * SCR_HB + 32 * q + 8 * i) = w1;
                }
                ss += __shfl_xor(ss, 1);
                ss += __shfl_xor(ss, 2);
#pragma unroll
                for (int d = 4; d < 64; d <<= 1) ss = fmaxf(ss, __shfl_xor(ss, d));
                if (lane == 0) scr_red[wave] = ss;
                if (__ballot(oor) != 0ull) undec = true;
            }
            if (tile + 1 < ntiles) load_point(tile + 1, nx0, nx1, nx2);   // lands during the screen
            __syncthreads();
            // largest squared row norm of the item's tiles so far: the record R_c may be held by a row of an earlier tile
            scr_Hsq = fmaxf(scr_Hsq, fmaxf(fmaxf(scr_red[0], scr_red[1]), fmaxf(scr_red[2], scr_red[3])));
            const float Heff = sqrtf(scr_Hsq) * (1.0f + 0x1p-10f) + 0x1p-10f;
            const bool tail = tile == ntiles - 1 && P - tile * MT <= 48;         // the dense kernel's 16-row tail tile
            // rows of this tile that are points of the item, as a mask over this lane's 32 values of a column.  A tail tile with
            // at most 32 points: the dense kernel pools its padded rows 32 .. 47 too, replicas of the last point summed by the
            // two-chain form, while that point's own row takes the plain chain -- row 32 stands for them here
            unsigned vmask = 0;
            {
                const int nvalid = P - tile * MT;
                const bool replica = tail && nvalid <= 32;
#pragma unroll
                for (int j = 0; j < 32; ++j) {
                    const int row = 32 * (j >> 4) + (j & 3) + 8 * ((j & 15) >> 2) + 4 * (lane >> 5);
                    vmask |= (row < nvalid || (replica && row == 32) ? 1u : 0u) << j;
                }
            }
            // A fragments one k-block ahead of their MFMAs; they are the same for every column tile, so k-block 7 fetches
            // k-block 0 of the next one
            u32x4 fa[2][2];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                fa[r][0] = scr_lds_a(hp0, 32 * r, 0, lane);
                fa[r][1] = scr_lds_a(hp1, 32 * r, 0, lane);
            }
            int qn = 0;                                                          // entries in this wave's queue (wave-uniform)
#pragma unroll 1
            for (int ct = 0; ct < 8; ++ct) {
                const int soff = soff0 + ct * 8 * 1024;
                f32x16 acc[2][2];
                // per accumulator the order of the products is a1 b0, a0 b1 (acc1) and a0 b0 (acc0), k-blocks ascending; the two
                // row tiles alternate so that no MFMA follows one it depends on.  One memory instruction per MFMA shadow.
#pragma unroll
                for (int kb = 0; kb < 8; ++kb) {
                    const int use = kb & 3, req = (kb + 3) & 3;
                    const u32x4 b0 = rb0[use], b1 = rb1[use];
                    rb0[req] = scr_bufld(rs3h, lane16, soff + (kb + 3) * 1024);
                    rb1[req] = scr_bufld(rs3h, lane16, (int)(P2S_SCR_PIECE * 2) + soff + (kb + 3) * 1024);
                    u32x4 na[2][2];
                    // the h1 fragments first: their registers are free after the first two MFMAs
                    na[0][1] = scr_lds_a(hp1, 0, (kb + 1) & 7, lane);
                    na[1][1] = scr_lds_a(hp1, 32, (kb + 1) & 7, lane);
                    na[0][0] = scr_lds_a(hp0, 0, (kb + 1) & 7, lane);
                    na[1][0] = scr_lds_a(hp0, 32, (kb + 1) & 7, lane);
                    if (kb == 0) {
                        acc[0][1] = scr_mfma(fa[0][1], b0, zero16());
                        acc[1][1] = scr_mfma(fa[1][1], b0, zero16());
                    } else {
                        acc[0][1] = scr_mfma(fa[0][1], b0, acc[0][1]);
                        acc[1][1] = scr_mfma(fa[1][1], b0, acc[1][1]);
                    }
                    acc[0][1] = scr_mfma(fa[0][0], b1, acc[0][1]);
                    acc[1][1] = scr_mfma(fa[1][0], b1, acc[1][1]);
                    if (kb == 0) {
                        acc[0][0] = scr_mfma(fa[0][0], b0, zero16());
                        acc[1][0] = scr_mfma(fa[1][0], b0, zero16());
                    } else {
                        acc[0][0] = scr_mfma(fa[0][0], b0, acc[0][0]);
                        acc[1][0] = scr_mfma(fa[1][0], b0, acc[1][0]);
                    }
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                    }
#pragma unroll
                    for (int r = 0; r < 2; ++r) {
                        fa[r][0] = na[r][0];
                        fa[r][1] = na[r][1];
                    }
                }
                if (scr_abl == 3) {       // MFMAs and their loads only: one value of each accumulator, pooled, keeps them live
                    sr0 = fmaxf(sr0, (acc[0][0][0] + acc[0][1][0]) + (acc[1][0][0] + acc[1][1][0]));
                    if (ct == 7) scr_E[lane] = sr0;
                    continue;
                }
                const float mu = mu_c * Heff;
                mu_c = scr_mu[256 * wave + 32 * (ct < 7 ? ct + 1 : 7) + (lane & 31)];   // the next column tile's, behind the ring's requests
                float tv[32];
#pragma unroll
                for (int j = 0; j < 32; ++j) tv[j] = fmaf(acc[j >> 4][1][j & 15], 0x1p-11f, acc[j >> 4][0][j & 15]);
                float m = fmaxf(tv[0], tv[1]);
#pragma unroll
                for (int j = 2; j < 32; j += 2) m = fmaxf(fmaxf(m, tv[j]), tv[j + 1]);
                m = half_max(m);
                float R;
                if (ct == 0) R = sr0 = fmaxf(sr0, m);
                else if (ct == 1) R = sr1 = fmaxf(sr1, m);
                else if (ct == 2) R = sr2 = fmaxf(sr2, m);
                else if (ct == 3) R = sr3 = fmaxf(sr3, m);
                else if (ct == 4) R = sr4 = fmaxf(sr4, m);
                else if (ct == 5) R = sr5 = fmaxf(sr5, m);
                else if (ct == 6) R = sr6 = fmaxf(sr6, m);
                else R = sr7 = fmaxf(sr7, m);
                const float thr = R - mu;
                unsigned mask = 0;
#pragma unroll
                for (int j = 0; j < 32; ++j) mask |= (tv[j] >= thr ? 1u : 0u) << j;
                mask &= vmask;
                // candidates -> this wave's queue, one per lane and round (ballot / mbcnt compaction)
                while (!undec) {
                    const bool has = mask != 0u;
                    const unsigned long long bal = __ballot(has);
                    if (bal == 0ull) break;
                    const int n = __popcll(bal);
                    if (qn + n > SCR_QCAP) {
                        undec = true;
                        break;
                    }
                    if (has) {
                        const int j = __ffs(mask) - 1;
                        mask &= mask - 1u;
                        const int row = 32 * (j >> 4) + (j & 3) + 8 * ((j & 15) >> 2) + 4 * (lane >> 5);
                        const int idx = qn + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
                        scr_q[idx] = ((unsigned)row << 16) | (unsigned)(32 * ct + (lane & 31));
                    }
                    qn += n;
                }
                __builtin_amdgcn_wave_barrier();
                if (scr_abl == 4) qn = 0; // everything but the confirm
                // full batches now, the rest with the tile's last column tile (the fp32 rows leave LDS with the tile).  Rows of
                // the 16-row tail take the two-chain form, every other candidate the plain chain: the form is chosen per
                // batch, wave-uniformly, and a batch of a tail tile that holds both runs both, each under its own lanes
                while (!undec && (qn >= 64 || (ct == 7 && qn > 0))) {
                    const int n = qn < 64 ? qn : 64;
                    const unsigned entry = scr_q[qn - n + (lane < n ? lane : 0)];
                    const bool split = tail && (entry >> 16) >= 32u;
                    if (lane < n && !split) scr_confirm<false>(entry, bufB, w3, wave, scr_E);
                    if (tail && __ballot(lane < n && split) != 0ull) {
                        if (lane < n && split) scr_confirm<true>(entry, bufB, w3, wave, scr_E);
                    }
                    qn -= n;
                    nconf += n;
                }
                __builtin_amdgcn_wave_barrier();
            }
            __syncthreads();          // h0 lies over the next tile's first-layer output
}
