// The body of the chain kernels -- textually included by p2s_chain.hip inside p2s_chain_kernel<SUM, SCREEN> (STEM_SAVE = STEM_LOAD
// = false) and inside the two kernels of a model that reuses the stem (SUM = false, SCREEN = true): p2s_chain_save_kernel
// (STEM_SAVE) and p2s_chain_reuse_kernel (STEM_LOAD), with `args` the kernel's ChainArgs.  Text and not a function: handed to a function, by reference or by value, the kernel's argument block is copied and every field of
// ChainBranch is then loaded for both branches and selected, where the kernels index the block by the branch (102 SGPR
// spills in the dense kernel, which has none; profiles/r12/kernel_resources.txt).
// STEM_SAVE (the STN pass of a model that reuses the stem): conv1 stores the A fragments it reads to ChainBranch.stem_out.  A
// kernel of its own and not a run-time branch of the screened kernel: with the branch in it that kernel lost 0.15 ms per
// launch in both passes whether the branch was taken or not (profiles/r12/variants.json).
// STEM_LOAD (the main pass of such a model): no point, no centre, no rotation, no conv0a and no conv0b -- a tile starts at
// conv1, whose A fragments the STN pass left in ChainBranch.stem_in
{
    static_assert(!(SUM && SCREEN), "the screen selects for a max");
    static_assert(SCREEN || !(STEM_LOAD || STEM_SAVE), "the saved stem belongs to the screened kernel only");
    static_assert(!(STEM_LOAD && STEM_SAVE), "written by one pass, read by the other");
    float *smem;
    if constexpr (SCREEN) {
        extern __shared__ __attribute__((aligned(16))) float smem_screen[];
        smem = smem_screen;
    } else {
        __shared__ __attribute__((aligned(16))) float smem_dense[MT * SA + MT * SB];
        smem = smem_dense;
    }
    float *bufA = smem;
    float *bufB = smem + MT * SA;

    // (not const: the screened instantiation renews them per tile, below)
    int tid = threadIdx.x;
    int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    int item = blockIdx.x;
    int bsel = 0;
    if (item >= args.br[0].n_items) {
        item -= args.br[0].n_items;
        bsel = 1;
    }
    const ChainBranch &br = args.br[bsel];
    const int P = br.P, P1 = br.P1;
    const float *__restrict__ w0a = br.w0a;
    const float *__restrict__ b0a = br.b0a;
    const float *__restrict__ w1 = br.w1 + (long long)item * br.w1_item_stride;
    const float *__restrict__ w3 = br.w3;
    // (the kernels of the stem reuse take full chains only, like every screened launch; they say so at compile time: with the
    // short chain's path into conv2 beside it, the compiler's wait for the conv2 weights was the short chain's, which also
    // waits for the stem's stores behind them)
    const bool short_chain = !(STEM_SAVE || STEM_LOAD) && br.short_chain != 0;

    float cx = 0.f, cy = 0.f, cz = 0.f;
    if (!STEM_LOAD && br.center) {
        cx = br.center[item * 3 + 0];
        cy = br.center[item * 3 + 1];
        cz = br.center[item * 3 + 2];
    }
    float R[9];
    const bool has_rot = !STEM_LOAD && br.rot != nullptr;
    if (has_rot) {
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = br.rot[item * 9 + i];
    }

    // eight named scalars, not an array: the pair index pr is a run-time value, an indexed array would live in scratch
    const float pool0 = SUM ? 0.0f : -INFINITY;
    float rm0 = pool0, rm1 = pool0, rm2 = pool0, rm3 = pool0, rm4 = pool0, rm5 = pool0, rm6 = pool0, rm7 = pool0;
    // torch's conv/ReLU/MaxPool propagate NaN (a non-finite coordinate poisons every channel of the
    // item); v_max_f32 does not.  Track non-finite inputs and poison the pooled output instead.
    bool bad = false;
    if constexpr (STEM_LOAD) bad = br.stem_bad[item] != 0;

    // buffer descriptors of the layer weights (wave-uniform): SGPR base + scalar offset + 16 * lane
    int lane16 = lane * 16;
    const __amdgpu_buffer_rsrc_t rs0b = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(br.w0b), 0, 4096 * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(w1), 0, 4096 * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(br.w2), 0, 8192 * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t w3rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(w3), 0, 128 * 1024 * 4, 0x00020000);
    // this wave's 8 conv3 column tiles start at byte offset wave * 8 * 16 KB of the packed weights
    const int w3soff = wave * (8 * 16 * 1024);

    // the item's saved stem (16 KB per tile), written by the STN pass (STEM_SAVE) or read by the main pass (STEM_LOAD)
    const int ntiles = (P + MT - 1) / MT;
    __amdgpu_buffer_rsrc_t rsst;
    if constexpr (STEM_SAVE || STEM_LOAD) {
        float *stem = STEM_LOAD ? const_cast<float *>(br.stem_in) : br.stem_out;
        rsst = __builtin_amdgcn_make_buffer_rsrc(stem + (long long)item * ntiles * (MT * 64), 0, ntiles * (MT * 64 * 4), 0x00020000);
    } else rsst = __builtin_amdgcn_make_buffer_rsrc((float *)nullptr, 0, 0, 0x00020000);
    constexpr bool stem_store = STEM_SAVE;
    B8 sf;                                     // STEM_LOAD: the A fragments of conv1 of the tile at hand / of the next one

    // coordinates of this lane's point of a tile (all 4 waves load the same 64 points; L1/L2 hits);
    // the next tile's point is fetched under conv3 of the current one.  STEM_LOAD: what is fetched there is not the point
    // but the eight fragments of this wave's row tile (HBM: 2.8 GB per chunk do not stay in L2)
    auto load_point = [&](int tile, float &x0, float &x1, float &x2) {
        if constexpr (STEM_LOAD) {
            load_b8(sf, rsst, lane16, tile * (MT * 64 * 4) + (wave >> 1) * 8192);
            return;
        }
        int p = tile * MT + lane;
        if (p >= P) p = P - 1;
        if (p < P1) {
            const float *src = br.ptsA + ((long long)item * P1 + p) * 3;
            x0 = src[0]; x1 = src[1]; x2 = src[2];
        } else {
            const float *src = br.ptsB + ((long long)item * (P - P1) + (p - P1)) * 3;
            x0 = src[0] - cx; x1 = src[1] - cy; x2 = src[2] - cz;
        }
    };

#ifdef P2S_DEV_ABLATE
    const int ablate = args.ablate;   // timing-only variants (wrong results): tools/ablate.sh builds with -DP2S_DEV_ABLATE=<variant>
    constexpr int scr_abl = P2S_DEV_ABLATE + 0;   // 3 .. 5, 7, 8, of the screened conv3, at compile time: its schedule stays the shipped one
#else
    constexpr int ablate = 0, scr_abl = 0;
#endif
    float nx0, nx1, nx2;
    // screened conv3: the state of p2s_chain_screen.inl
    // the exact pool: float bits, held as the unsigned the confirm's integer atomics work on -- every access has that type
    unsigned *scr_E = reinterpret_cast<unsigned *>(smem + SCR_OFF_E) + 256 * wave;
    float *scr_red = smem + SCR_OFF_RED;
    unsigned *scr_q = reinterpret_cast<unsigned *>(smem + SCR_OFF_Q) + SCR_QCAP * wave;
    const float *__restrict__ scr_mu = args.w3mu[bsel];
    const __amdgpu_buffer_rsrc_t rs3h = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short *>(args.w3h[bsel]), 0,
                                                                           (int)(P2S_SCR_PIECE * 2), 0x00020000);
    // running maxima of the screen values of this wave's 256 columns and their margin coefficients: in LDS, so that the second
    // accumulator set of the column-tile pipeline has their registers (lanes l and l ^ 32 hold and write the same value)
    float *scr_R = smem + SCR_OFF_R + 256 * wave;
    float *scr_mul = smem + SCR_OFF_MU + 256 * wave;
    bool undec = false;                        // the screen cannot decide this item (wave-uniform)
    float scr_Hsq = 0.0f;                      // largest squared row norm of the conv2 tiles of the item so far
    int nconf = 0;                             // fp32 chains this wave ran
    bool dense_pass = !SCREEN;
    if constexpr (SCREEN) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            scr_E[64 * i + lane] = __float_as_uint(-INFINITY);
            scr_R[64 * i + lane] = -INFINITY;
            scr_mul[64 * i + lane] = scr_mu[256 * wave + 64 * i + lane];     // read by this wave only: no barrier
        }
        if constexpr (!STEM_LOAD) {
            // conv0a's 256 operands are the launch's: from LDS a tile reads them in a few cycles, where its 16 vector loads were
            // a trip to L2 in front of the tile's first fma (the screen's weight ring leaves nothing of them in L1)
            smem[SCR_OFF_W0 + tid] = tid < 192 ? w0a[tid] : b0a[tid - 192];
            __syncthreads();
        }
    }
    const float *w0lds = smem + (SCREEN ? SCR_OFF_W0 : 0);
    auto conv0a_w = [&](int i) { return SCREEN ? w0lds[i] : w0a[i]; };
    auto conv0a_b = [&](int o) { return SCREEN ? w0lds[192 + o] : b0a[o]; };
    for (;;) {
    load_point(0, nx0, nx1, nx2);
    for (int tile = 0; tile < ntiles; ++tile) {
      // screened kernel: the thread's index is made opaque at the top of every tile, so that the per-lane addresses of the tile's
      // layers are built in the tile and are not kept in registers across the screen and its confirm (hoisted out of the
      // item's loops they were what spilled: profiles/r10/kernel_resources.txt; tests/test_chain_kernel_resources.py holds the
      // budget).  The values are the same; the other instantiations have no code here
      if constexpr (SCREEN) {
          asm volatile("" : "+v"(tid));
          lane = tid & 63;
          lane16 = lane * 16;
      }
      f32x4 bA0, bA1, aA0, aA1, bB0, bB1, aB0, aB1;   // conv3 operand register sets
      if (STEM_LOAD && ablate != 1) {
        // ---- conv1 from the saved stem: registers -> bufA (free: the screen ends with a barrier behind its last read of
        // fp16(h), the dense conv3 reads bufB); the barrier behind it also puts every wave past its conv3 reads of bufB
        // A layer's bias is requested with its weights, in front of its MFMAs: requested by the epilogue it was a trip to
        // the argument block and one to L1/L2, both waited for in full behind the layer's last MFMA.  The fences keep all
        // eight requests of W1' in front of conv1's first MFMA (per item: the screen's weight ring has pushed it out of L1);
        // left alone, the scheduler requested one fragment per k-group and waited for it in front of the k-group's MFMAs
        B8 wb;
        load_b8(wb, rs1, lane16, (wave & 1) * 8192);
        __builtin_amdgcn_sched_barrier(0);         // (the bias behind W1': its pointer is a trip to the argument block)
        const float bias1 = br.b1[32 * (wave & 1) + (lane & 31)];
        __builtin_amdgcn_sched_barrier(0);
        float bias2;
        {
            const int rt = wave >> 1, nt = wave & 1;
            f32x16 acc;
            layer_k64_regs(sf, wb, acc, rs2, lane16, wave * 8192);         // (and the conv2 weights)
            bias2 = br.b2[32 * wave + (lane & 31)];
            store_tile_bias_relu(acc, bufA, SA, 32 * rt, 32 * nt, bias1, lane);
        }
        __syncthreads();
        {
            f32x16 acc[2];
            layer_k64<2>(bufA, SA, 0, wb, lane, acc);
            store_tile_bias_relu(acc[0], bufB, SB, 0, 32 * wave, bias2, lane);
            store_tile_bias_relu(acc[1], bufB, SB, 32, 32 * wave, bias2, lane);
        }
        __syncthreads();
      } else if (ablate != 1) {
        float x0 = nx0, x1 = nx1, x2 = nx2;
        B8 wb;
        B8 wb2;                                // (stem_store: the conv2 weights)
        // the bias of a layer's epilogue, requested with the layer's weights (stem_store: conv1's and conv2's with conv1's weights)
        float bias0b = 0.0f, bias1 = 0.0f, bias2 = 0.0f;
        if (!short_chain) {
            load_b8(wb, rs0b, lane16, (wave & 1) * 8192);                    // conv0b weights, in flight across the barrier
            bias0b = br.b0b[32 * (wave & 1) + (lane & 31)];
        } else {
            load_b8(wb, rs2, lane16, wave * 8192);
            bias2 = br.b2[32 * wave + (lane & 31)];
        }
        if (has_rot) {
            // spelled out, contraction off: left to the compiler, the choice of which products fuse differed between the
            // instantiations of this kernel, and the screened and the dense conv3 must see the same points bit for bit.
            // The pattern is the one the compiler had chosen for the dense kernel before (read off its disassembly: y0's
            // third product is rounded on its own and added, y1 / y2 are two nested fma), so its results are unchanged
#pragma clang fp contract(off)
            const float y0 = __builtin_fmaf(R[0], x0, R[1] * x1) + R[2] * x2;
            const float y1 = __builtin_fmaf(R[5], x2, __builtin_fmaf(R[3], x0, R[4] * x1));
            const float y2 = __builtin_fmaf(R[8], x2, __builtin_fmaf(R[6], x0, R[7] * x1));
            x0 = y0; x1 = y1; x2 = y2;
        }
        bad = bad || !(fabsf(x0) <= 3.0e38f) || !(fabsf(x1) <= 3.0e38f) || !(fabsf(x2) <= 3.0e38f);
        // ---- first layer (K = 3) on the VALU: wave w produces channels [16w, 16w+16) -------------
        {
            float *dst = bufA + lane * SA + 16 * wave;
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) {
                f32x4 v;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int o = 16 * wave + 4 * c4 + c;   // wave-uniform (screened kernels: from LDS)
                    float s = conv0a_b(o);
                    s = fmaf(conv0a_w(o), x0, s);
                    s = fmaf(conv0a_w(64 + o), x1, s);
                    s = fmaf(conv0a_w(128 + o), x2, s);
                    v[c] = fmaxf(s, 0.0f);
                }
                *reinterpret_cast<f32x4 *>(dst + 4 * c4) = v;
            }
        }
        __syncthreads();   // bufA ready; every wave is past its conv3 reads of bufB (previous tile)

        if (!short_chain) {
            // ---- conv0b: bufA[64x64] -> bufB[:, 0:64] ; wave = (row tile, col tile) ---------------
            {
                const int rt = wave >> 1, nt = wave & 1;
                f32x16 acc[1];
                if constexpr (stem_store) {
                    // Loads and stores return through one counter (vmcnt), and with stores in flight the compiler's waits for
                    // a load are waits for the stores' round trip to HBM as well (conv1's bias and the conv2 weights requested
                    // behind the stores cost the STN launch 0.45 ms, requested in front of them and waited for behind them
                    // 0.3 ms: profiles/r12/variants.json).  So everything the tile loads before the screen is requested here,
                    // a layer, an epilogue and a barrier ahead of conv1 (the conv1 weights: by conv0b's k-groups), and has
                    // arrived before the first store: nothing waits for a load while the stores are in flight
                    load_b8(wb2, rs2, lane16, wave * 8192);                    // conv2 weights
                    bias1 = br.b1[32 * nt + (lane & 31)];
                    bias2 = br.b2[32 * wave + (lane & 31)];
                }
                layer_k64<1, true>(bufA, SA, 32 * rt, wb, lane, acc, rs1, lane16, nt * 8192);     // (and the conv1 weights)
                if constexpr (!stem_store) bias1 = br.b1[32 * nt + (lane & 31)];
                store_tile_bias_relu(acc[0], bufB, SB, 32 * rt, 32 * nt, bias0b, lane);
            }
            __syncthreads();
            // ---- conv1 (STN: shared weights; main: per-item W1' = W1 . trans2): bufB -> bufA ---------
            {
                const int rt = wave >> 1, nt = wave & 1;
                f32x16 acc[1];
                if constexpr (stem_store) {
                    // every load of the tile so far has arrived (vmcnt(0); requested before the barrier above)
                    __builtin_amdgcn_sched_barrier(0);
                    __builtin_amdgcn_s_waitcnt(0x0f70);
                    __builtin_amdgcn_sched_barrier(0);
                    const int soff = tile * (MT * 64 * 4) + rt * 8192;
                    if (nt == 0) layer_k64_store<0>(bufB, SB, 32 * rt, wb, lane, acc[0], rsst, lane16, soff);
                    else layer_k64_store<1>(bufB, SB, 32 * rt, wb, lane, acc[0], rsst, lane16, soff);
                    wb = wb2;
                    store_tile_bias_relu(acc[0], bufA, SA, 32 * rt, 32 * nt, bias1, lane);
                } else {
                    layer_k64<1, true>(bufB, SB, 32 * rt, wb, lane, acc, rs2, lane16, wave * 8192);     // (and the conv2 weights)
                    bias2 = br.b2[32 * wave + (lane & 31)];
                    store_tile_bias_relu(acc[0], bufA, SA, 32 * rt, 32 * nt, bias1, lane);
                }
            }
            __syncthreads();
        }
        // ---- conv2: bufA[64x64] -> bufB[64x128]; wave w = column tile w, both row tiles --------------
        {
            f32x16 acc[2];
            layer_k64<2>(bufA, SA, 0, wb, lane, acc);
            // first conv3 weight fragments, in flight across the barrier (the screened kernel requests them in front of its
            // dense conv3, below: requested here, their eight registers stayed reserved across the screen)
            if constexpr (!SCREEN) {
                bA0 = bufld4(w3rsrc, lane16, w3soff);
                bA1 = bufld4(w3rsrc, lane16, w3soff + 16 * 1024);
            }
            store_tile_bias_relu(acc[0], bufB, SB, 0, 32 * wave, bias2, lane);
            store_tile_bias_relu(acc[1], bufB, SB, 32, 32 * wave, bias2, lane);
        }
        __syncthreads();
      } else {
        bA0 = bufld4(w3rsrc, lane16, w3soff);
        bA1 = bufld4(w3rsrc, lane16, w3soff + 16 * 1024);
      }
      if (ablate == 2) continue;
      if constexpr (SCREEN) {
        if (!dense_pass) {
#include "p2s_chain_screen.inl"
            // the screened pass never pools into rm0 .. rm7: saying so here keeps the eight registers from being carried
            // through the screen for the dense pass that may follow
            rm0 = rm1 = rm2 = rm3 = rm4 = rm5 = rm6 = rm7 = pool0;
            continue;
        }
        bA0 = bufld4(w3rsrc, lane16, w3soff);
        bA1 = bufld4(w3rsrc, lane16, w3soff + 16 * 1024);
      }
        // ---- conv3 (K = 128, N = 1024) + running max over points -----------------------------------
        // wave w owns channels [256w, 256w+256) = 8 column tiles, processed as 4 pairs with a
        // 2 (row tiles) x 2 (column tiles) register block: 64 accumulator registers.
        // One continuous software pipeline over the 4 x 16 k-groups: two operand register sets (A/B)
        // ping-pong, the operands of k-group g+1 are fetched while the 16 MFMAs of k-group g issue --
        // across pair boundaries too -- and every memory instruction sits in its own MFMA shadow.
        // P2S_TAIL (see mfma16b): the item's last tile with <= 48 points -- row tile 1 runs as 16 rows on the 4-block MFMA.
        // sum pool: padded rows are masked per row of the 32x32 layout (tile_colsum) -- keeps the full tile
        if (!SUM && tile == ntiles - 1 && P - tile * MT <= 48) {
#define P2S_TAIL 1
#include "p2s_chain_conv3.inl"
#undef P2S_TAIL
        } else {
#define P2S_TAIL 0
#include "p2s_chain_conv3.inl"
#undef P2S_TAIL
        }
        // next tile's first layer writes bufA, whose last readers (conv2) are behind the barrier above
    }
    if constexpr (SCREEN) {
        if (!dense_pass) {
            // the item's verdict: one wave that could not decide sends the whole workgroup through the dense conv3
            if (lane == 0) scr_red[4 + wave] = undec ? 1.0f : 0.0f;
            __syncthreads();
            const bool redo = (scr_red[4] + scr_red[5] + scr_red[6] + scr_red[7]) != 0.0f;
            if (args.scr_counters) {
                if (lane == 0 && !redo) atomicAdd(args.scr_counters + 0, (unsigned long long)nconf);
                if (tid == 0) {
                    atomicAdd(args.scr_counters + 2, 1ull);
                    if (redo) atomicAdd(args.scr_counters + 1, 1ull);
                }
            }
            if (redo) {
                dense_pass = true;
                continue;
            }
            __builtin_amdgcn_wave_barrier();
            rm0 = __uint_as_float(scr_E[(lane & 31)]);       rm1 = __uint_as_float(scr_E[32 + (lane & 31)]);
            rm2 = __uint_as_float(scr_E[64 + (lane & 31)]);  rm3 = __uint_as_float(scr_E[96 + (lane & 31)]);
            rm4 = __uint_as_float(scr_E[128 + (lane & 31)]); rm5 = __uint_as_float(scr_E[160 + (lane & 31)]);
            rm6 = __uint_as_float(scr_E[192 + (lane & 31)]); rm7 = __uint_as_float(scr_E[224 + (lane & 31)]);
        }
    }
    break;
    }

    // ---- pooled affine epilogue: out = [relu](max + bias) ------------------------------------------
    const bool any_bad = __ballot(bad) != 0ull;
    if (stem_store && tid == 0) br.stem_bad[item] = any_bad ? 1 : 0;       // the four waves saw the same 64 points per tile
    if (lane < 32) {
        float *out = br.out + (long long)item * 1024 + 256 * wave + lane;
        const float *b3 = br.b3 + 256 * wave + lane;
        const float rmax[8] = {rm0, rm1, rm2, rm3, rm4, rm5, rm6, rm7};
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            float v = rmax[t] + (SUM ? (float)P * b3[32 * t] : b3[32 * t]);     // sum: the bias once per point
            if (br.relu_out) v = fmaxf(v, 0.0f);
            if (any_bad) v = __builtin_nanf("");
            out[32 * t] = v;
        }
    }
}
