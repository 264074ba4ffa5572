// Screened conv3 (K = 128, N = 1024) + exact max-pool of ONE point tile -- textually included by p2s_chain.hip inside
// p2s_chain_kernel<false, true> (the same reason as p2s_chain_conv3.inl: the pooled state stays in registers / LDS).
//
// conv3 feeds only a max over the item's points: of the P x 1024 dot products 1024 reach the output.  This path decides on
// ONE fp16 MFMA per product block which products can be the maximum and computes only those in fp32:
//   screen   t[p][c] = sum_k fp16(h_pk) fp16(w_ck) on v_mfma_f32_32x32x16_f16, fp32 accumulate, two accumulator sets (one
//            column tile is selected while the next one's MFMAs issue: Schedule, below);
//   margin   mu_c = 2 (k_screen + k_fp32) (|w_c| + 2^-10) (H + 2^-10),  H >= |h_p| for every row of every tile of the item so
//            far, this one included (a running maximum: the margin only grows from tile to tile);
//   select   (p, c) is a candidate iff t[p][c] >= max(R_c - mu_c, E_c - mu_c / 2), R_c = the running maximum of t[.][c] over
//            the tiles so far, this one included -- every record-breaker passes the first term -- and E_c = the exact pool
//            of the EARLIER tiles (below; -inf in an item's first tile, where the rule is the first term alone);
//   confirm  each candidate at once, while its fp32 row h[p] is still in LDS: one chain of 128 fmaf in the k order of the
//            32x32x2 MFMA chain of p2s_chain_conv3.inl (k-groups ascending, t = 0..3, 8g+t then 8g+4+t; rows of the 16-row
//            tail: the two half chains, then one add), one lane per candidate;  E_c = max of the confirmed values.
// The pooled value never comes from the screen: the screen only has to say safely which products cannot win.
//
// Exactness.  Write s*_x for the real-number dot product of row x, fl(s_x) for the fp32 chain, d_x >= |t_x - s*_x| and
// g_x >= |fl(s_x) - s*_x|; both scale with |w_c| |h_x|: d_x + g_x <= (k_screen + k_fp32) (|w_c| + 2^-10) (|h_x| + 2^-10).  A
// dismissed p had t_p < R - mu_c at its tile, with R = t_q of a row q of THAT OR AN EARLIER tile that was a candidate when it
// set the record (t_q = R >= R - mu_c; if q is a padding row, the item's last point, which it replicates, has the same
// operands and the same t).  mu_c is built from H >= max(|h_p|, |h_q|) -- the running maximum over the tiles so
// far, not this tile's alone: the record holder may be a row of larger norm than any of the current tile -- so
// (d_p + g_p) + (d_q + g_q) <= mu_c and
//     fl(s_p) <= s*_p + g_p <= t_p + d_p + g_p < t_q - mu_c + d_p + g_p <= t_q - d_q - g_q <= s*_q - g_q <= fl(s_q):
// p cannot hold the maximum over all P fp32 values and E_c is that maximum: the value p2s_chain_kernel<false> pools.
//
// The pool bound (r10).  R is a screen value with an error of its own, which is why the R rule needs both halves of mu_c.  E_c,
// read from scr_E when a column tile is selected, has none: it is the maximum of fl(s_q) over the rows q confirmed in the
// EARLIER tiles of the item (the candidates of this column tile are queued after the read, and the last column tile of every
// tile empties the queue; scr_E of a wave is written by that wave's own confirms only, in program order).  Every value that
// can sit in E_c is a value the dense kernel pools for that channel:
//   plain chains     a row of a full tile, or a row < 32 of a tail tile: the 32x32x2 chain of that row, bit for bit;
//   tail rows        a row >= 32 of the 16-row tail that is a point of the item: the two half chains and their sum, which is
//                    what tail_colmax pools for it;
//   row 32 of a short tail (at most 32 points left): the two-chain sum over the operands of the item's last point -- the dense
//                    kernel pools exactly that value for its replicas in rows 32 .. 47, beside the plain chain of the point's
//                    own row -- so it stands for values the dense kernel pools, and for no other.
// Padding rows are never queued (vmask), so E_c <= M_c, the maximum the dense kernel pools, at every moment.  A row p with
//     t_p + (d_p + g_p) < E_c     has     fl(s_p) <= s*_p + g_p <= t_p + d_p + g_p < E_c <= M_c
// in either of its forms (g_p covers the extra add of the two-chain form, and row 32 has the t of the point it replicates):
// it does not hold the maximum, and dismissing it leaves max(confirmed) = M_c, because a holder of M_c itself has
// t >= M_c - (d + g) >= E_c - (d + g) and passes.  With d_p + g_p <= kappa (|w_c| + 2^-10) (|h_p| + 2^-10) <= kappa (|w_c| +
// 2^-10) (H + 2^-10) = mu_c / 2 (H bounds |h_p|: p is of the current tile; the row that set E_c needs no bound), the second
// term of the select is E_c - mu_c / 2.  The argument never uses R: the two terms dismiss independently, and a row has to pass
// both.  Once a record holder q has been confirmed, E_c >= fl(s_q) >= t_q - mu_c / 2, so the new term is the stronger one for
// every later tile whose record is still t_q.
//   rounding   mu_c / 2 is exact (a power of two; mu_c >= 2^-29 is far from the subnormals); fl(E - mu/2) errs by at most
//              2^-24 (|E| + mu/2) <= 2^-24 (1 + 2^-9) |w_c| H + 2^-24 mu/2 (|E| = |fl(s_q)| <= (1 + 2^-16) |w_c| |h_q| and H, a
//              running maximum, bounds |h_q| too).  The slack is the same as for R - mu: mu_c and Heff are each rounded up
//              by (1 + 2^-10), which makes mu/2 larger than kappa (|w_c| + 2^-10)(H + 2^-10) by 2^-9 of itself, >= 2^-19 |w_c| H
//              -- 32 times the rounding above; the roundings of the two norms (2^-20 on |w_c|, about 2^-21 on H: 36 fmaf
//              and a square root) and of the product mu_c * Heff (2^-24) take less than a tenth of it.  Checked, not copied:
//              the bound on |E| is by the row's own norm, the one on |R| was by the screen value.
//   -inf, NaN  E_c = -inf (an item's first tile: nothing is confirmed before its first select) gives -inf for the second
//              term and fmaxf leaves R - mu.  A NaN in E_c (a chain over a non-finite activation) is dropped by fmaxf in the
//              same way and dismisses nothing; the item is poisoned by `bad` as before.  E_c = +inf can only come from an
//              fp32 chain that overflowed: every later row is then dismissed unless its t is +inf too, and the pool is
//              +inf either way.
// The candidate set stays a function of the item alone (E_c depends on the earlier tiles' candidates only, never on timing).
// Not built: the per-row form |h_p| + H of the margin (CPU model: 6.27 instead of 7.33 candidates per channel; 32 more live
// values per lane in the select).
//
// The two k.  S = sum_k |w_k| |h_k| <= |w_c| |h_p| (Cauchy-Schwarz), N1 = sum_k |x_k| <= sqrt(128) |x|.
//   operands    each is rounded ONCE to fp16: |fp16(x) - x| <= 2^-11 |x| in the normal range, <= 2^-25 below 2^-14 (half a
//               subnormal step), so always <= 2^-11 |x| + 2^-25 (values beyond the range never get here: `undec`).  Per product
//               |fp16(h) fp16(w) - h w| <= (2^-10 + 2^-22) |h| |w| + 2^-25 (1 + 2^-11) (|h| + |w|) + 2^-50; over the 128 k:
//                   (2^-10 + 2^-22) S   +   2^-21.5 (1 + 2^-11) (|h_p| + |w_c|) + 2^-43.
//               The second part is what the + 2^-10 of the margin's two factors pay for: k 2^-10 (|w_c| + |h_p|) + k 2^-20 with
//               k >= 2^-10 is 2^-20 (|w_c| + |h_p|) + 2^-30, 2.8 times what is needed -- the floor of the pair screen
//               (2^-36 sqrt(128) against 2^-22 2^-10) was tighter than this one, the terms stay as they are;
//   screen sum  8 MFMAs of 16 exact products each into an fp32 accumulator; allowing every one of the 136 additions a
//               truncation (2^-23, twice round-to-nearest) of a partial sum <= sum |fp16(w)| |fp16(h)| <= (1 + 2^-9) S + the
//               absolute part above: 136 * 2^-23 (1 + 2^-9) < 2^-15.9;
//   fp32 chain  128 roundings of a partial sum <= S, again allowing truncation: 128 * 2^-23 = 2^-16 (the tail
//               rows' extra add included in the slack).
//   k_screen + k_fp32 <= 2^-10 (1 + 2^-12 + 2^-5.9 + 2^-6) < 1.0326 * 2^-10  <=  1.0625 * 2^-10 = P2S_SCR_KAPPA (0x1.1p-10,
//   2.9 % slack; the candidate count grows with the constant -- about twice per doubling -- so it is not rounded up further).
//   The threshold R - mu is one more fp32 rounding (2^-24 |R|, |R| <= about |w_c| H): the two factors (1 + 2^-10) with which
//   mu_c and H are rounded up add 2^-9 mu >= 2^-19 |w_c| H and pay for it and for the roundings of the norms.
//
// What the screen cannot decide runs densely: an item with an activation beyond the half range, or with more candidates
// in one column tile than the wave's queue holds (a patch of identical points: every product ties), sets `undec`, and the
// workgroup runs the item again through the dense conv3 (p2s_chain_kernel's own) when its screened pass ends.
//
// Schedule.  With one MFMA per fragment pair (64 matrix-pipe cycles per k-block of the two row tiles) every operand byte
// counts: the A fragments of the tile (the fp16 rows, the same for all 8 column tiles) are read from LDS ONCE into 64
// registers -- re-reading them per column tile (2 x ds_read_b128 per k-block and wave) alone would take the LDS port of the
// CU for as long as the MFMAs take -- and the weight stream is one ring of 8 slots over the tile's 8 x 8 k-blocks, 7
// requests (7 KB per wave) in flight: k-block j + 7 is requested between the two MFMAs of k-block j, across the select, the
// queue and the confirm of a column tile too.
// The column tiles are a pipeline two deep (r11): the 16 MFMAs of column tile ct + 1 go into a second accumulator set and the
// select of column tile ct (column maximum, record, threshold, 32 compares, mask: about 100 VALU instructions, which read the
// first set only) is issued between them; then come the queue and the confirm of ct, as before.  The 32 registers of the
// second set are the 24 that held `1 << j` for the mask (now shifted in row by row through the carry: sel_rows3), the 8 running
// maxima R (now in LDS beside E, like the margin coefficients, which were a global load with a full drain per column tile)
// and 16 that the dense pass had reserved across the screen (profiles/r11/kernel_resources.txt).
{
            unsigned short *hp0 = reinterpret_cast<unsigned short *>(bufA);      // fp16(h) [64][SCR_HB] over the conv2 input tile
            // ---- the weight stream: ONE ring over the tile's 8 column tiles x 8 k-blocks ---------------------------------
            // A wave's fragments of consecutive k-blocks and column tiles are consecutive KBs of the packed fragments, so the
            // stream does not know column tiles.  The first seven are requested here and land during the conversion.  (The
            // last seven requests of a tile run past the wave's own fragments: they read the next wave's, or, past the end of
            // the buffer, zeros; nothing uses them.)
            const int soff0 = wave * 8 * 8 * 1024;          // bytes: 8 k-blocks of 64 lanes x 16 B per column tile
            u32x4 rb[8];
#pragma unroll
            for (int s = 0; s < 7; ++s) rb[s] = scr_bufld(rs3h, lane16, soff0 + s * 1024);
            // ---- h -> fp16 beside the fp32 tile; row norms -------------------------------------------------------------
            if (scr_abl != 5) {
                const int p = tid >> 2, q = tid & 3;
                const float *src = bufB + p * SB + 32 * q;
                float ss = 0.0f;
                bool oor = false;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const f32x4 v0 = lds4(src + 8 * i), v1 = lds4(src + 8 * i + 4);
                    const u32x4 w0 = {scr_half2(v0[0], v0[1]), scr_half2(v0[2], v0[3]), scr_half2(v1[0], v1[1]), scr_half2(v1[2], v1[3])};
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        ss = fmaf(v0[u], v0[u], ss);
                        ss = fmaf(v1[u], v1[u], ss);
                        oor = oor || p2s_f16_out_of_range(v0[u]) || p2s_f16_out_of_range(v1[u]);
                    }
                    *reinterpret_cast<u32x4 *>(hp0 + p * SCR_HB + 32 * q + 8 * i) = w0;
                }
                ss += __shfl_xor(ss, 1);
                ss += __shfl_xor(ss, 2);
#pragma unroll
                for (int d = 4; d < 64; d <<= 1) ss = fmaxf(ss, __shfl_xor(ss, d));
                if (lane == 0) scr_red[wave] = ss;
                if (__ballot(oor) != 0ull) undec = true;
            }
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
            // the tile's A fragments, once: both row tiles x 8 k-blocks
            u32x4 fa[8][2];
#pragma unroll
            for (int kb = 0; kb < 8; ++kb) {
                fa[kb][0] = scr_lds_a(hp0, 0, kb, lane);
                fa[kb][1] = scr_lds_a(hp0, 32, kb, lane);
            }
            int qn = 0;                                                          // entries in this wave's queue (wave-uniform)
            const int l31 = lane & 31;
            float keep = -INFINITY;                                              // (development variants 3 and 8 only)
            unsigned keepm = 0;                                                  // (development variants 7 and 8 only)
            // k-block kb of one column tile into `acc`: the two row tiles alternate so that no MFMA follows the one it depends
            // on, the ring's request sits between them (the callers' sched_group_barriers say where)
            auto kblock = [&](f32x16 (&acc)[2], int soff, int kb) __attribute__((always_inline)) {
                const u32x4 b = rb[kb];
                rb[(kb + 7) & 7] = scr_bufld(rs3h, lane16, soff + (kb + 7) * 1024);
                if (kb == 0) {
                    acc[0] = scr_mfma(fa[0][0], b, zero16());
                    acc[1] = scr_mfma(fa[0][1], b, zero16());
                } else {
                    acc[0] = scr_mfma(fa[kb][0], b, acc[0]);
                    acc[1] = scr_mfma(fa[kb][1], b, acc[1]);
                }
            };
            // The select of column tile ct from its finished accumulators, in the pieces the pipeline places: the column
            // maximum of row tile 0, then that of row tile 1 and the threshold, then the mask in six pieces of rows.
            struct Sel {
                float mul, Ec, Rold, m, thr;
                unsigned mask;
            };
            // The three LDS reads (mu's coefficient, E, R) are requested in the stage's first k-block and nothing of that k-block
            // uses them: their first use is the threshold, one k-block -- two MFMAs -- later (until r13 the product mul * Heff
            // was taken here, and the wait for the reads stood behind the eight v_max of this piece).  Requested a whole column
            // tile ahead, in the stage of ct - 1, the values live across the queue and the confirm, and the save kernel and
            // p2s_chain_kernel<false, true> spill 4 and 2 VGPRs (with two of the three carried as with all three): not built
            auto sel_begin = [&](Sel &s, const f32x16 (&acc)[2], int ct) __attribute__((always_inline)) {
                s.mul = scr_mul[32 * ct + l31];
                // the exact pool of this lane's channel over the EARLIER tiles: candidates of this column tile are queued
                // after this and confirmed after that, and every batch of an earlier tile has run (ct == 7 empties the queue);
                // scr_E of a wave is written by that wave's own confirms only, the wave barriers order them before this read
                s.Ec = __uint_as_float(scr_E[32 * ct + l31]);
                s.Rold = scr_R[32 * ct + l31];
                float m = fmaxf(acc[0][0], acc[0][1]);
#pragma unroll
                for (int j = 2; j < 16; j += 2) m = fmaxf(fmaxf(m, acc[0][j]), acc[0][j + 1]);
                s.m = m;
                s.mask = 0;
            };
            auto sel_threshold = [&](Sel &s, const f32x16 (&acc)[2], int ct) __attribute__((always_inline)) {
                float m = s.m;
#pragma unroll
                for (int j = 0; j < 16; j += 2) m = fmaxf(fmaxf(m, acc[1][j]), acc[1][j + 1]);
                {   // half_max() without `volatile`: a volatile asm is ordered against the ring's loads and would pin the
                    // select behind the last of them
                    const unsigned u = __float_as_uint(m);
                    const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
                    const float x = __uint_as_float(r[0]), y = __uint_as_float(r[1]);
                    asm("v_max_f32 %0, %1, %2" : "=v"(m) : "v"(x), "v"(y));
                }
                const float R = fmaxf(s.Rold, m);
                scr_R[32 * ct + l31] = R;
                // -inf (nothing confirmed yet) leaves the R rule; fmaxf drops a NaN operand, so a NaN in E dismisses nothing
                const float mu = s.mul * Heff;
                s.thr = fmaxf(R - mu, s.Ec - 0.5f * mu);
            };
            // The mask, two VALU instructions per row (r13): the rows are taken from 31 down to 0, each compares into a carry
            // register and `mask = mask + mask + carry` shifts it in, so row j ends at bit j, as the queue decodes it.
            // v_cmp_ge_f32 is the compare the C++ `>=` compiled to: false on a NaN.  A VALU read of a carry a VALU instruction
            // wrote needs two wait states on gfx950, and the compiler pads nothing inside an asm: three carry registers (VCC
            // and two SGPR pairs) rotate so that two other instructions of the group always stand between a compare and the
            // add that reads it, and no s_nop is needed.  The adds' own carry-outs (always 0: 32 shifts of a mask that starts
            // at 0) go to the register just read, which is dead.  Plain asm in groups of three and five rows, not volatile
            // and not one block: the pipeline places one piece per k-block between the MFMAs (a volatile asm is pinned)
            auto sel_rows3 = [&](Sel &s, float a2, float a1, float a0) __attribute__((always_inline)) {
                unsigned long long c0, c1;
                asm("v_cmp_ge_f32_e32 vcc, %3, %6\n\t"
                    "v_cmp_ge_f32_e64 %1, %4, %6\n\t"
                    "v_cmp_ge_f32_e64 %2, %5, %6\n\t"
                    "v_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"
                    "v_addc_co_u32_e64 %0, %1, %0, %0, %1\n\t"
                    "v_addc_co_u32_e64 %0, %2, %0, %0, %2"
                    : "+v"(s.mask), "=&s"(c0), "=&s"(c1)
                    : "v"(a2), "v"(a1), "v"(a0), "v"(s.thr)
                    : "vcc");
            };
            auto sel_rows5 = [&](Sel &s, float a4, float a3, float a2, float a1, float a0) __attribute__((always_inline)) {
                unsigned long long c0, c1;
                asm("v_cmp_ge_f32_e32 vcc, %3, %8\n\t"
                    "v_cmp_ge_f32_e64 %1, %4, %8\n\t"
                    "v_cmp_ge_f32_e64 %2, %5, %8\n\t"
                    "v_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"
                    "v_cmp_ge_f32_e32 vcc, %6, %8\n\t"
                    "v_addc_co_u32_e64 %0, %1, %0, %0, %1\n\t"
                    "v_cmp_ge_f32_e64 %1, %7, %8\n\t"
                    "v_addc_co_u32_e64 %0, %2, %0, %0, %2\n\t"
                    "v_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"
                    "v_addc_co_u32_e64 %0, %1, %0, %0, %1"
                    : "+v"(s.mask), "=&s"(c0), "=&s"(c1)
                    : "v"(a4), "v"(a3), "v"(a2), "v"(a1), "v"(a0), "v"(s.thr)
                    : "vcc");
            };
            // piece gi of the mask, one per k-block 2 .. 7 of a stage: rows 31 .. 26, 25 .. 20, then four times five rows
            auto sel_group = [&](Sel &s, const f32x16 (&acc)[2], int gi) __attribute__((always_inline)) {
                auto a = [&](int j) __attribute__((always_inline)) { return acc[j >> 4][j & 15]; };
                if (gi < 2) {
                    const int hi = 31 - 6 * gi;
                    sel_rows3(s, a(hi), a(hi - 1), a(hi - 2));
                    sel_rows3(s, a(hi - 3), a(hi - 4), a(hi - 5));
                } else {
                    const int hi = 19 - 5 * (gi - 2);
                    sel_rows5(s, a(hi), a(hi - 1), a(hi - 2), a(hi - 3), a(hi - 4));
                }
            };
            // candidates of column tile ct -> this wave's queue, then the confirm of what is due
            auto queue_confirm = [&](unsigned mask, int ct) __attribute__((always_inline)) {
                // one candidate per lane and round (ballot / mbcnt compaction)
                if (scr_abl == 7 || scr_abl == 8) keepm |= mask; // the select alone: no queue (one use keeps the mask), no confirm
                else while (!undec) {
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
                        scr_q[idx] = ((unsigned)row << 16) | (unsigned)(32 * ct + l31);
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
                    if (lane < n && !split) scr_confirm<false>(entry, bufB, w3rsrc, wave, scr_E);
                    if (tail && __ballot(lane < n && split) != 0ull) {
                        if (lane < n && split) scr_confirm<true>(entry, bufB, w3rsrc, wave, scr_E);
                    }
                    qn -= n;
                    nconf += n;
                }
                __builtin_amdgcn_wave_barrier();
            };
            // one stage of the column-tile pipeline (r11): the MFMAs of column tile ct + 1 into accN, and in their issue
            // shadow the select of column tile ct from accS, whose MFMAs were the stage before.  The select needs nothing of
            // ct + 1.  Each k-block of ct + 1 (MFMA, the ring's request, MFMA: 64 matrix-pipe cycles, 16 VALU issue slots)
            // is a scheduling region of its own together with one piece of the select -- left to one region of 16 MFMAs the
            // scheduler packed the MFMAs and put the select behind them in some builds
            auto stage = [&](f32x16 (&accN)[2], const f32x16 (&accS)[2], int ct, bool has_next) __attribute__((always_inline)) -> unsigned {
                const int soff = soff0 + (ct + 1) * 8 * 1024;
                Sel s;
                s.mask = 0;
#pragma unroll
                for (int kb = 0; kb < 8; ++kb) {
                    if (has_next) kblock(accN, soff, kb);
                    if (scr_abl == 3) {          // MFMAs and their loads only: one value of each accumulator keeps them live
                        if (kb == 0) keep = fmaxf(keep, accS[0][0] + accS[1][0]);
                    } else if (kb == 0) sel_begin(s, accS, ct);
                    else if (kb == 1) {
                        sel_threshold(s, accS, ct);
                        if (scr_abl == 8) keep = fmaxf(keep, s.thr); // the select without its mask: one use keeps the threshold
                    } else if (scr_abl != 8) sel_group(s, accS, kb - 2);
                    if (has_next) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                return s.mask & vmask;
            };
            // The order of events per column tile is the one the exactness argument uses: E read and select of ct, queue,
            // confirm, and only then the select of ct + 1; only the MFMAs of ct + 1 have moved ahead of them, and they touch
            // nothing the select, the queue or the confirm reads.  Two accumulator sets, the loop unrolled by two so that each
            // has its registers; the last column tile has no MFMAs beside its select, and empties the queue as before
            f32x16 accA[2], accB[2];
#pragma unroll
            for (int kb = 0; kb < 8; ++kb) {
                kblock(accA, soff0, kb);
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            }
            // (STEM_LOAD: the last two column tiles stand behind the loop, below)
#pragma unroll 1
            for (int ct = 0; ct < (STEM_LOAD ? 6 : 8); ct += 2) {
                unsigned mask = stage(accB, accA, ct, true);
                if (scr_abl != 3) queue_confirm(mask, ct);
                if (ct < 6) mask = stage(accA, accB, ct + 1, true);
                else {
                    // the next tile's point: requested here, where the second accumulator set is dead and its registers are
                    // free (requested before the screen, its three registers were what spilled), it lands during the last
                    // select, queue and confirm
                    if (tile + 1 < ntiles) load_point(tile + 1, nx0, nx1, nx2);
                    mask = stage(accA, accB, ct + 1, false);
                }
                if (scr_abl != 3) queue_confirm(mask, ct + 1);
            }
            if constexpr (STEM_LOAD) {
                // What is requested for the next tile here is not three coordinates but the 32 registers of conv1's A
                // fragments.  Requested inside the loop they would be allocated across all of it (a value defined in one
                // iteration of a loop and used behind it lives through the loop); behind the loop they live from here, where the
                // second accumulator set, the A fragments of the screen and the weight ring are dead, to the next tile's conv1
                unsigned mask = stage(accB, accA, 6, true);
                if (scr_abl != 3) queue_confirm(mask, 6);
                if (tile + 1 < ntiles) load_point(tile + 1, nx0, nx1, nx2);
                mask = stage(accA, accB, 7, false);
                if (scr_abl != 3) queue_confirm(mask, 7);
            }
            if (scr_abl == 3) scr_E[lane] = __float_as_uint(keep);
            if (scr_abl == 7 || scr_abl == 8) scr_q[lane] = keepm ^ __float_as_uint(keep);
            __syncthreads();          // fp16(h) lies over the next tile's first-layer output
}
