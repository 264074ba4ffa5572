// The network's forward pass: workspace, one chunk through the encoders (+ decoder), the fp32 fallback of the fp16 pair mode.
#include "p2s_common.h"
#include "p2s_internal.h"
#include <cstring>
#include <algorithm>

namespace {

// the per-chunk workspace of C queries; the 16-bit region is last, so a run at P2S_FP32 finds every other buffer where a run at
// the model's own precision has it
struct Ws {
    float *g_stn, *h1, *h2, *T, *w1p, *feat, *d1, *d2, *d3, *qg, *qg2, *qh1, *qh2, *rot;
    unsigned short *w1h;     // W1' of both encoders as 16-bit fragments, per piece
    // stem reuse: conv0b's output of every tile of both branches as conv1's A fragments, [branch][item][tile][rt 2][kg 8][lane 64][4]
    // (branch 0 = the sub-sample, as in the launches), and the items' non-finite flags [2][C]
    float *stem;
    int *stem_bad;
    size_t floats;           // all of it
};

constexpr size_t STEM_TILE = 4096;       // floats per 64-point tile
size_t stem_tiles(int points) { return ((size_t)points + 63) / 64; }
size_t stem_floats(const p2s_model_cfg &cfg, size_t C) { return C * (stem_tiles(cfg.points_per_patch) + stem_tiles(cfg.sub_sample_size)) * STEM_TILE; }

// stem: the workspace holds the stem region (p2s_model_s.ws_stem; never with 16-bit pieces)
Ws carve(float *base, const p2s_model_cfg &cfg, Precision prec, int C, bool stem) {       // base == NULL: the size alone
    Ws w;
    size_t at = 0;
    auto take = [&](size_t n, bool present = true) {        // an absent region: NULL, no room
        float *r = base && present ? base + at : nullptr; at += present ? n : 0; return r;
    };
    w.g_stn = take((size_t)2 * C * 1024);
    w.h1 = take((size_t)2 * C * 512);
    w.h2 = take((size_t)2 * C * 256);
    w.T = take((size_t)2 * C * 4096);
    w.w1p = take((size_t)2 * C * 4096);
    w.feat = take((size_t)2 * C * 1024);
    w.d1 = take((size_t)C * 1024);
    w.d2 = take((size_t)C * 256);
    w.d3 = take((size_t)C * 128);
    w.qg = take((size_t)C * 1024, cfg.use_point_stn);
    w.qg2 = take((size_t)C * 1024, cfg.use_point_stn);
    w.qh1 = take((size_t)C * 512, cfg.use_point_stn);
    w.qh2 = take((size_t)C * 256, cfg.use_point_stn);
    w.rot = take((size_t)C * 16, cfg.use_point_stn);
    w.w1h = reinterpret_cast<unsigned short *>(take((size_t)C * 4096 * prec.pieces, prec.pieces != 0));
    w.stem = take(stem_floats(cfg, C), stem);
    w.stem_bad = reinterpret_cast<int *>(take((size_t)2 * C, stem));
    w.floats = at;
    return w;
}

// one chunk in flight: what the helpers below fill kernel arguments from
struct Chunk {
    const p2s_model_s *m;
    Precision prec;
    const float *patch, *sub, *query, *rot;
    int C;
    Ws w;
};

// ChainBranch's weight fields are untyped: the 16-bit chain kernels read 16-bit fragments through them
const float *chain_operand(const unsigned short *h) { return reinterpret_cast<const float *>(h); }
const float *chain_operand(const Chunk &c, P2sLayer l, int e) { return c.prec.pieces ? chain_operand(c.m->w16(l, e)) : c.m->w32(l, e); }

enum Pass { PASS_QSTN, PASS_STN, PASS_MAIN };

// the branch of `pass` over the points of encoder e: 1 = the sub-sample minus the query point, 0 = the patch
void fill_branch(ChainBranch &b, const Chunk &c, Pass pass, int e) {
    const p2s_model_s *m = c.m;
    const float *W = m->blob.get();
    const p2s_encoder_offsets &eo = m->offs.enc[e];
    const size_t C = c.C;
    if (e == 1) { b.ptsA = nullptr; b.ptsB = c.sub; b.center = c.query; b.P = m->cfg.sub_sample_size; b.P1 = 0; }
    else        { b.ptsA = c.patch; b.ptsB = nullptr; b.center = nullptr; b.P = b.P1 = m->cfg.points_per_patch; }
    b.n_items = c.C;
    b.rot = c.rot;                  // NULL until the QSTN has run
    b.relu_out = pass != PASS_MAIN;
    b.short_chain = pass == PASS_QSTN;
    b.pool_sum = pass == PASS_MAIN && m->cfg.sym_sum;        // sym_op='sum': PointNetfeat's pool only (the STN / QSTN trunks keep the max)
    // stem reuse: the STN pass saves what the main pass starts from (branch 0 of the region = the sub-sample, e = 1)
    b.stem_out = nullptr; b.stem_in = nullptr; b.stem_bad = nullptr;
    if (c.w.stem && pass != PASS_QSTN) {
        float *stem = c.w.stem + (e == 1 ? 0 : C * stem_tiles(m->cfg.sub_sample_size) * STEM_TILE);
        if (pass == PASS_STN) b.stem_out = stem; else b.stem_in = stem;
        b.stem_bad = c.w.stem_bad + (e == 1 ? 0 : C);
    }
    const P2sLayer l2 = pass == PASS_QSTN ? L_QC2 : pass == PASS_STN ? L_S2 : L_M2;       // the 64 -> 128 -> 1024 end of the pass
    const P2sLayer l3 = pass == PASS_QSTN ? L_QC3 : pass == PASS_STN ? L_S3 : L_M3;
    const int z = pass == PASS_QSTN ? 0 : e;
    b.w2 = chain_operand(c, l2, z); b.b2 = m->bias(l2, z);
    b.w3 = chain_operand(c, l3, z); b.b3 = m->bias(l3, z);
    if (pass == PASS_QSTN) {
        b.w0a = W + m->offs.qstn.c1; b.b0a = W + m->offs.qstn.cb1;
        b.w0b = b.b0b = nullptr; b.w1 = W; b.b1 = nullptr; b.w1_item_stride = 0;
        b.out = e == 1 ? c.w.qg : c.w.qg2;
        return;
    }
    b.w0a = W + eo.w0a; b.b0a = W + eo.b0a;
    b.w0b = chain_operand(c, L_W0B, e); b.b0b = m->bias(L_W0B, e);
    if (pass == PASS_STN) {         // stem + STN trunk
        b.w1 = chain_operand(c, L_S1, e); b.b1 = m->bias(L_S1, e); b.w1_item_stride = 0;
        b.out = c.w.g_stn + e * C * 1024;
    } else {                        // stem (recomputed, or read from stem_in) + the item's own W1' + conv2 + conv3
        b.w1 = c.prec.pieces ? chain_operand(c.w.w1h + e * C * 4096) : c.w.w1p + e * C * 4096;
        b.b1 = W + eo.mb1; b.w1_item_stride = 4096;
        b.out = c.w.feat + e * C * 1024;
    }
}

// both branches empty; launched on the fp32 or the 16-bit chain kernel (the fp32 one does not read the 16-bit fields)
ChainArgs chain_args(const Chunk &c) {
    ChainArgs a;
    memset(&a, 0, sizeof(a));
    a.ns = c.prec.pieces;
    a.f16 = c.prec.f16;
    a.bad_items = c.m->fb.flags.get();
    a.piece_stride = (long long)c.m->h_total;
    a.w1_piece_stride = (long long)2 * c.C * 4096;
    return a;
}
// an fp32 run of the STN or main pass (slot 0 = encoder 1, slot 1 = encoder 0): conv3 is screened where the model holds the
// screen operands and the pass pools by max
int launch_chain(ChainArgs &a, const Chunk &c, hipStream_t s, Pass pass = PASS_QSTN) {
    if (c.prec.pieces) return p2s_launch_chain_bf16(a, s);
    a.screen = pass != PASS_QSTN && c.m->scr_w3h && !a.br[0].pool_sum && !a.br[1].pool_sum;
    if (a.screen) {
        const P2sLayer l3 = pass == PASS_STN ? L_S3 : L_M3;
        for (int slot = 0; slot < 2; ++slot) {
            a.w3h[slot] = c.m->screen_w(l3, 1 - slot);
            a.w3mu[slot] = c.m->screen_mu(l3, 1 - slot);
        }
        a.scr_counters = c.m->scr_counters.get();
    }
    return p2s_launch_chain(a, s);
}

// FC layer `layer` over the g.Z slices of dense rows A [Z][C][K] -> out (+ z * c_z) [C][ldc]; g keeps M, Z, relu and A2.  The
// encoder-side head layers of an fp16-pair run go through their 16-bit fragments
int fc(GemmArgs &g, const Chunk &c, P2sLayer layer, const float *A, float *out, long long ldc, long long c_z, hipStream_t s) {
    const P2sLayerDesc &d = p2s_layers[layer];
    const bool h16 = c.prec.f16 && d.kind != LK_FP32;
    for (int z = 0; z < 2; ++z) {
        g.W[z] = c.m->w32(layer, z);
        g.bias[z] = c.m->bias(layer, z);
        g.Wh[z] = h16 ? c.m->w16(layer, z) : nullptr;
    }
    g.wh_piece = h16 ? (long long)c.m->h_total : 0;
    g.bad_rows = h16 ? c.m->fb.flags.get() : nullptr;
    g.A = A; g.lda = d.K; g.a_z = g.Z == 2 ? (long long)c.C * d.K : 0;
    g.C = out; g.ldc = ldc; g.c_z = c_z; g.N = d.N; g.K = d.K;
    return p2s_launch_gemm(g, s);
}

}  // namespace

int p2s_model_reserve(p2s_model_s *m, int chunk) {
    if (chunk <= m->ws_chunk) return P2S_OK;
    if (m->ws) {
        P2S_HIP_CHECK(hipDeviceSynchronize());
        m->ws.reset();
        m->ws_chunk = 0;
    }
    const Precision prec = p2s_precision(m->cfg);
    const size_t n = carve(nullptr, m->cfg, prec, 1, false).floats * (size_t)chunk;
    // with the stem region where it is allowed and fits the device; a chunk that does not get it recomputes the stem
    m->ws_stem = m->stem_reuse && !prec.pieces && stem_floats(m->cfg, chunk) * sizeof(float) <= m->stem_max_bytes &&
                 m->ws.alloc(carve(nullptr, m->cfg, prec, 1, true).floats * (size_t)chunk);
    if (!m->ws_stem && !m->ws.alloc(n)) {
        p2s_set_error("allocation of the workspace (%zu MB) failed", n * 4 >> 20);
        return P2S_ENOMEM;
    }
    m->ws_chunk = chunk;
    return P2S_OK;
}

// fp16 pair mode: one workgroup per query of the chunk; a flagged query (ChainArgs.bad_items / GemmArgs.bad_rows) takes the
// next slot of the side buffers and its network inputs are copied there
__global__ __launch_bounds__(256) void p2s_fb_collect_kernel(int *__restrict__ flags, int *__restrict__ count, int cap,
                                                             const float *__restrict__ patch, const float *__restrict__ sub,
                                                             const float *__restrict__ query, const float *__restrict__ radius,
                                                             int k3, int n3, long long index0, float *__restrict__ fpatch,
                                                             float *__restrict__ fsub, float *__restrict__ fquery,
                                                             float *__restrict__ fradius, long long *__restrict__ findex) {
    __shared__ int s_slot;
    const int q = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        int slot = -1;
        if (flags[q]) {
            flags[q] = 0;
            slot = atomicAdd(count, 1);
        }
        s_slot = slot;
    }
    __syncthreads();
    const int slot = s_slot;
    if (slot < 0 || slot >= cap) return;
    for (int i = tid; i < k3; i += 256) fpatch[(size_t)slot * k3 + i] = patch[(size_t)q * k3 + i];
    for (int i = tid; i < n3; i += 256) fsub[(size_t)slot * n3 + i] = sub[(size_t)q * n3 + i];
    if (tid < 3) fquery[(size_t)slot * 3 + tid] = query[(size_t)q * 3 + tid];
    if (tid == 3) {
        if (radius) fradius[slot] = radius[q];
        findex[slot] = index0 + q;
    }
}

__global__ void p2s_fb_scatter_kernel(const long long *__restrict__ index, const float *__restrict__ sdf,
                                      const float *__restrict__ logits, int n, int od, float *__restrict__ sdf_out,
                                      float *__restrict__ logits_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long d = index[i];
    if (sdf_out) sdf_out[d] = sdf[i];
    if (logits_out)
        for (int j = 0; j < od; ++j) logits_out[d * od + j] = logits[(size_t)i * od + j];
}

int p2s_run_chunk(p2s_model_s *m, Precision prec, const float *patch, const float *sub, const float *query, const float *radius,
                  int C, float *logits_out, float *sdf_out, float *feat_local_out, float *feat_global_out,
                  hipStream_t s, long long index0) {
    const p2s_weight_offsets &o = m->offs;
    const float *W = m->blob.get();
    Chunk c = {m, prec, patch, sub, query, nullptr, C, carve(m->ws.get(), m->cfg, prec, C, m->ws_stem && !prec.pieces)};
    const Ws &w = c.w;
    int rc;
    const int ev0 = p2s_prof_mark(m, s);
    int evq1 = -1, evq2 = -1;                         // QSTN models: behind the QSTN trunk launch / behind its head layers

    if (m->cfg.use_point_stn) {
        // shared QSTN over cat(patch, sub-sample - q): reference points_to_surf_model.py:325-331, :100-131; without
        // shared_transformer the QSTN belongs to feat_global and sees the sub-sample alone (:283-284, :177-185), its
        // rotation is applied to the sub-sample and to the patch (:337-339) -- the same kernels, other points
        const bool qstn_shared = m->cfg.shared_transformer != 0 || m->cfg.single_transformer != 0;
        // the shared QSTN's 1300 points run as TWO workgroups per query -- sub-sample (1000) and patch (300), like the
        // encoder passes -- and the head takes max(pool, pool): 4096 equal 1300-point workgroups filled the 768
        // workgroup slots in 5.33 rounds (105 TFLOP/s), 8192 unequal ones pack like the encoder passes (141 TFLOP/s)
        ChainArgs a = chain_args(c);
        fill_branch(a.br[0], c, PASS_QSTN, 1);
        fill_branch(a.br[1], c, PASS_QSTN, qstn_shared ? 0 : 1);
        if (!qstn_shared) a.br[1].n_items = 0;
        if ((rc = launch_chain(a, c, s))) return rc;
        evq1 = p2s_prof_mark(m, s);
        m->counters.launches_chain += 1;
        GemmArgs g;
        memset(&g, 0, sizeof(g));
        g.M = C; g.Z = 1; g.relu = 1;
        g.A2 = qstn_shared ? w.qg2 : nullptr;
        if ((rc = fc(g, c, L_QF1, w.qg, w.qh1, 512, 0, s))) return rc;
        g.A2 = nullptr;
        if ((rc = fc(g, c, L_QF2, w.qh1, w.qh2, 256, 0, s))) return rc;
        if ((rc = p2s_launch_qstn_tail(w.qh2, W + o.qstn.f3, W + o.qstn.fb3, w.rot, C, 256, s))) return rc;
        c.rot = w.rot;
        evq2 = p2s_prof_mark(m, s);
    }

    // ---- pass 1: stem + STN trunk + max-pool, both encoders (global items first: longest first) ----
    ChainArgs a = chain_args(c);
    for (int slot = 0; slot < 2; ++slot) fill_branch(a.br[slot], c, PASS_STN, 1 - slot);   // slot 0 = feat_global (e=1), slot 1 = feat_local (e=0)
    if ((rc = launch_chain(a, c, s, PASS_STN))) return rc;
    const int ev1 = p2s_prof_mark(m, s);

    // ---- STN head: 1024 -> 512 -> 256 -> 4096 (+I), then W1' = W1 . trans2 -------------------------
    GemmArgs hd;
    memset(&hd, 0, sizeof(hd));
    hd.M = C; hd.Z = 2; hd.relu = 1;
    if (m->cfg.single_transformer) {      // one encoder over both point sets: its pool = max of the two branches' pools
        hd.A2 = w.g_stn + (size_t)C * 1024;
        hd.a2_z = -(long long)C * 1024;
    }
    if ((rc = fc(hd, c, L_SF1, w.g_stn, w.h1, 512, (long long)C * 512, s))) return rc;
    hd.A2 = nullptr;
    if ((rc = fc(hd, c, L_SF2, w.h1, w.h2, 256, (long long)C * 256, s))) return rc;
    hd.relu = 0;
    if ((rc = fc(hd, c, L_SF3, w.h2, w.T, 4096, (long long)C * 4096, s))) return rc;
    FoldArgs f;
    memset(&f, 0, sizeof(f));
    for (int e = 0; e < 2; ++e) {
        f.T[e] = w.T + (size_t)e * C * 4096;
        f.m1t[e] = W + o.enc[e].m1t;
        f.out[e] = w.w1p + (size_t)e * C * 4096;
        f.outh[e] = prec.pieces ? w.w1h + (size_t)e * C * 4096 : nullptr;      // 16-bit modes: pieces written by the fold itself
    }
    f.h_piece_stride = (long long)2 * C * 4096;
    f.ns = prec.pieces;
    f.f16 = prec.f16;
    f.bad_items = prec.f16 ? m->fb.flags.get() : nullptr;
    f.n_items = C;
    if ((rc = p2s_launch_fold(f, s))) return rc;
    const int ev2 = p2s_prof_mark(m, s);

    // ---- pass 2: stem (recomputed, or the one pass 1 saved) + transformed conv1 + conv2 + conv3 + max-pool ---
    for (int slot = 0; slot < 2; ++slot) fill_branch(a.br[slot], c, PASS_MAIN, 1 - slot);
    if ((rc = launch_chain(a, c, s, PASS_MAIN))) return rc;
    const int ev3 = p2s_prof_mark(m, s);
    m->counters.launches_chain += 2;
    if (w.stem) m->counters.stem_items_reused += 2 * (int64_t)C;

    if (feat_local_out) P2S_HIP_CHECK(hipMemcpyAsync(feat_local_out, w.feat, (size_t)C * 1024 * 4, hipMemcpyDeviceToDevice, s));
    if (feat_global_out)
        P2S_HIP_CHECK(hipMemcpyAsync(feat_global_out, w.feat + (size_t)C * 1024, (size_t)C * 1024 * 4, hipMemcpyDeviceToDevice, s));

    if (logits_out || sdf_out) {
        GemmArgs g;
        memset(&g, 0, sizeof(g));
        g.M = C; g.Z = 2; g.relu = 1;       // fc1_local | fc1_global -> cat (local first): reference points_to_surf_model.py:335,343,346
        if (m->cfg.single_transformer) {      // fc1_local_global reads the ONE pooled feature; d1l / d1g are its column halves
            g.A2 = w.feat + (size_t)C * 1024;
            g.a2_z = -(long long)C * 1024;
            g.a2_add = m->cfg.sym_sum ? 1 : 0;        // sym_op='sum': the pool over both point sets = the sum of the two sums
        }
        if ((rc = fc(g, c, L_D1, w.feat, w.d1, 1024, 512, s))) return rc;
        g.Z = 1; g.A2 = nullptr;
        if ((rc = fc(g, c, L_D2, w.d1, w.d2, 256, 0, s))) return rc;
        if ((rc = fc(g, c, L_D3, w.d2, w.d3, 128, 0, s))) return rc;
        if ((rc = p2s_launch_decoder_tail(w.d3, W + o.d4, W + o.db4, radius, logits_out, sdf_out, C, 128, m->cfg.output_dim, s))) return rc;
    }
    const int ev4 = p2s_prof_mark(m, s);
    if (evq1 >= 0 && evq2 >= 0) {
        p2s_prof_span(m, ST_CHAIN_QSTN, ev0, evq1);
        p2s_prof_span(m, ST_HEAD, evq1, evq2);
        p2s_prof_span(m, ST_CHAIN_STN, evq2, ev1);
    } else {
        p2s_prof_span(m, ST_CHAIN_STN, ev0, ev1);
    }
    p2s_prof_span(m, ST_HEAD, ev1, ev2);
    p2s_prof_span(m, ST_CHAIN_MAIN, ev2, ev3);
    p2s_prof_span(m, ST_DECODER, ev3, ev4);
    if (prec.f16 && m->fb.flags) {
        // fp16 pair mode: the inputs of the queries the 16-bit kernels flagged are put aside (the chunk buffers are reused
        // two chunks on); one workgroup per query, all but the flagged ones return at once
        hipLaunchKernelGGL(p2s_fb_collect_kernel, dim3(C), dim3(256), 0, s, m->fb.flags.get(), m->fb.count.get(), m->fb.cap, patch, sub, query,
                           radius, m->cfg.points_per_patch * 3, m->cfg.sub_sample_size * 3, index0, m->fb.patch.get(), m->fb.sub.get(), m->fb.query.get(), m->fb.radius.get(), m->fb.index.get());
        P2S_LAUNCH_CHECK("p2s_fb_collect_kernel");
    }
    return P2S_OK;
}

extern "C" int p2s_debug_stn_pool(p2s_model_t m, int n_queries, float *out_dev, void *stream) {
    if (!m || !out_dev || n_queries < 1 || n_queries > m->ws_chunk || n_queries > m->max_chunk) {
        p2s_set_error("p2s_debug_stn_pool: no workspace of a call of %d queries (one internal batch)", n_queries);
        return P2S_EINVAL;
    }
    P2S_HIP_CHECK(hipSetDevice(m->device));
    const Ws w = carve(m->ws.get(), m->cfg, p2s_precision(m->cfg), n_queries, false);       // (g_stn comes first)
    P2S_HIP_CHECK(hipMemcpyAsync(out_dev, w.g_stn, (size_t)2 * n_queries * 1024 * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return P2S_OK;
}

int p2s_fallback_finish(p2s_model_s *m, float *logits_out, float *sdf_out, hipStream_t s) {
    p2s_model_s::Fallback &fb = m->fb;
    if (!fb.count) return P2S_OK;
    int h = 0;
    P2S_HIP_CHECK(hipMemcpyAsync(&h, fb.count.get(), 4, hipMemcpyDeviceToHost, s));
    P2S_HIP_CHECK(hipStreamSynchronize(s));
    if (!h) return P2S_OK;
    if (h > fb.cap || (!logits_out && !sdf_out)) {
        p2s_set_error("fp16 pair encoder (encoder_bf16 = 4): %d queries of this call have activations beyond the half range (> 6e4)%s "
                      "-- use encoder_bf16 = 3 or 0 for this model", h,
                      h > fb.cap ? ", more than the fp32 fallback takes per call (16384)" : " and the call has no output the fp32 fallback could repair");
        return P2S_EINVAL;
    }
    m->counters.fallback_queries += h;
    // the same queries through the fp32 kernels (the fp32 fragments of every layer are resident in any mode)
    const size_t k3 = (size_t)m->cfg.points_per_patch * 3, n3 = (size_t)m->cfg.sub_sample_size * 3;
    const int od = m->cfg.output_dim;
    int rc = P2S_OK;
    for (int i0 = 0; i0 < h && rc == P2S_OK; i0 += m->ws_chunk) {
        const int C = std::min(m->ws_chunk, h - i0);
        rc = p2s_run_chunk(m, P2S_FP32, fb.patch.get() + i0 * k3, fb.sub.get() + i0 * n3, fb.query.get() + (size_t)i0 * 3, sdf_out ? fb.radius.get() + i0 : nullptr, C,
                           fb.logits.get() + (size_t)i0 * od, sdf_out ? fb.sdf.get() + i0 : nullptr, nullptr, nullptr, s, 0);
    }
    if (rc) return rc;
    hipLaunchKernelGGL(p2s_fb_scatter_kernel, dim3((h + 255) / 256), dim3(256), 0, s, fb.index.get(), fb.sdf.get(), fb.logits.get(), h, od, sdf_out, logits_out);
    P2S_LAUNCH_CHECK("p2s_fb_scatter_kernel");
    P2S_HIP_CHECK(hipStreamSynchronize(s));
    return P2S_OK;
}
