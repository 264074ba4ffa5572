// C-ABI glue: error reporting, scratch lock, model handle, profiling, one model call, the p2s_encode_* entries.
#include "p2s_common.h"
#include "p2s_internal.h"
#include <vector>
#include <cstring>
#include <algorithm>
#include <mutex>
#include <cstdlib>

static thread_local char g_err[512] = "";

void p2s_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// Process-wide grow-only scratch buffer per device (P2sScratchLock, p2s_common.h; when to use it and when a handle's own
// DevBuf: DESIGN.md, "who owns device memory").
namespace {
struct DevScratch {
    std::mutex mu;
    void *p = nullptr;
    size_t cap = 0;
};
DevScratch g_scratch[P2S_MAX_DEVICES];
}  // namespace

P2sScratchLock::P2sScratchLock(int device) : dev_(device) {
    if (dev_ >= 0 && dev_ < P2S_MAX_DEVICES) g_scratch[dev_].mu.lock();
}
P2sScratchLock::~P2sScratchLock() {
    if (dev_ >= 0 && dev_ < P2S_MAX_DEVICES) g_scratch[dev_].mu.unlock();
}
void *P2sScratchLock::get(size_t bytes) {
    if (dev_ < 0 || dev_ >= P2S_MAX_DEVICES) return nullptr;
    DevScratch &sl = g_scratch[dev_];
    if (bytes <= sl.cap) return sl.p;
    if (sl.p) (void)hipFree(sl.p);
    sl.p = nullptr;
    sl.cap = 0;
    const size_t want = bytes + bytes / 8;
    if (hipMalloc(&sl.p, want) != hipSuccess) {
        (void)hipGetLastError();
        sl.p = nullptr;
        return nullptr;
    }
    sl.cap = want;
    return sl.p;
}

// the operands of the screened conv3 (p2s_chain_screen.inl) of the fp32 encoders (mode 0; the 16-bit modes are untouched: the
// fp32 re-run of the fp16 pair mode takes queries with an activation beyond the half range, which the screen would hand to the
// dense conv3 anyway).  P2S_CONV3_DENSE=1, read here once, keeps the dense conv3 (the A/B switch); so does a conv3 weight that
// does not fit the half range
static int screen_init(p2s_model_s *m) {
    if (m->cfg.encoder_bf16 != 0) return P2S_OK;
    const char *dense = getenv("P2S_CONV3_DENSE");
    if (dense && atoi(dense) != 0) return P2S_OK;
    DevBuf<int> flag;
    const bool ok = p2s_alloc_all(m->scr_w3h, (size_t)4 * P2S_SCR_PIECE, m->scr_mu, (size_t)4 * 1024, m->scr_counters, 3, flag, 1) &&
                    hipMemset(m->scr_counters.get(), 0, 3 * 8) == hipSuccess && hipMemset(flag.get(), 0, 4) == hipSuccess;
    int rc = P2S_OK, h = 0;
    if (!ok) {
        (void)hipGetLastError();
        p2s_set_error("allocation of the screen operands of conv3 failed");
        rc = P2S_ENOMEM;
    }
    for (int i = 0; i < 4 && rc == P2S_OK; ++i) {
        const P2sLayer layer = i < 2 ? L_S3 : L_M3;
        rc = p2s_launch_screen_prepare(m->w32(layer, i & 1), const_cast<unsigned short *>(m->screen_w(layer, i & 1)),
                                       const_cast<float *>(m->screen_mu(layer, i & 1)), nullptr, flag.get());
    }
    if (rc == P2S_OK && hipMemcpy(&h, flag.get(), 4, hipMemcpyDeviceToHost) != hipSuccess) {
        p2s_set_error("hipMemcpy(conv3 range flag) failed");
        rc = P2S_EHIP;
    }
    if (rc == P2S_OK && h) {          // a conv3 weight beyond the half range: this model keeps the dense conv3
        m->scr_w3h.reset();
        m->scr_mu.reset();
    }
    // stem reuse: both passes of the model run the screened kernel (a sym_op='sum' main pass keeps the dense conv3).  The default
    // cap holds the 2688 MB of an 8192-query chunk of 300 + 1000 points (21 tiles of 16 KB per query).  The switch and the cap
    // are members of the configuration, not environment variables: the library keeps to its 20
    m->stem_reuse = rc == P2S_OK && m->scr_w3h && !m->cfg.sym_sum && !m->cfg.stem_recompute;
    m->stem_max_bytes = (size_t)(m->cfg.stem_reuse_max_mb > 0 ? m->cfg.stem_reuse_max_mb : 3072) << 20;
    return rc;
}

// p2s_model_create: the device side of a new handle; on failure the caller destroys the half-built handle
static int model_init(p2s_model_s *m, const float *blob_host, size_t n_floats) {
    const p2s_model_cfg &cfg = m->cfg;
    if (!m->blob.alloc(n_floats)) {
        p2s_set_error("allocation of the weights failed");
        return P2S_ENOMEM;
    }
    const hipError_t e = hipMemcpy(m->blob.get(), blob_host, n_floats * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        p2s_set_error("hipMemcpy(weights) failed: %s", hipGetErrorString(e));
        return P2S_EHIP;
    }
    const Precision prec = p2s_precision(cfg);
    {
        const int rc = screen_init(m);
        if (rc) return rc;
    }
    if (!prec.pieces) return P2S_OK;
    // 16-bit fragments of the layers that have them in this mode, packed on the device from the fp32 fragments: blob_h holds
    // the kinds of p2s_layers in turn, a per-encoder kind encoder by encoder
    struct Item { P2sLayer layer; int z; };
    std::vector<Item> items;
    for (int kind = LK_ENC; kind < LK_FP32; ++kind) {
        if (!p2s_kind_packed((P2sLayerKind)kind, cfg)) continue;
        const int slices = kind == LK_ENC || kind == LK_ENC_HEAD ? 2 : 1;
        for (int z = 0; z < slices; ++z)
            for (int l = 0; l < P2S_LAYERS; ++l) {
                if (p2s_layers[l].kind != kind) continue;
                m->h_off[l][z] = m->h_off[l][1] = m->h_total;          // a layer without slices: the same twice
                items.push_back({(P2sLayer)l, z});
                m->h_total += (size_t)p2s_layers[l].K * p2s_layers[l].N;
            }
    }
    if (!m->blob_h.alloc(m->h_total * prec.pieces)) {
        p2s_set_error("allocation of the 16-bit weights failed");
        return P2S_ENOMEM;
    }
    DevBuf<int> wflag;          // fp16 pair: raised by the packing kernel when a BN-folded weight does not fit the half range
    if (prec.f16 && (!wflag.alloc(1) || hipMemset(wflag.get(), 0, 4) != hipSuccess)) {
        (void)hipGetLastError();
        p2s_set_error("allocation of the weight range flag failed");
        return P2S_ENOMEM;
    }
    for (int piece = 0; piece < prec.pieces; ++piece)
        for (const Item &it : items) {
            const P2sLayerDesc &d = p2s_layers[it.layer];
            const int rc = p2s_launch_pack_bf16(m->w32(it.layer, it.z), m->blob_h.get() + (size_t)piece * m->h_total + m->h_off[it.layer][it.z],
                                                d.K, d.N, 0, 0, 1, piece, prec.f16, nullptr, wflag.get());
            if (rc) return rc;
        }
    if (prec.f16) {
        int h = 0;
        const hipError_t e2 = hipMemcpy(&h, wflag.get(), 4, hipMemcpyDeviceToHost);
        if (e2 != hipSuccess) {
            p2s_set_error("hipMemcpy(weight range flag) failed: %s", hipGetErrorString(e2));
            return P2S_EHIP;
        }
        if (h) {
            p2s_set_error("fp16 pair encoder (encoder_bf16 = 4): a BatchNorm-folded weight of this checkpoint does not fit the half "
                          "range (|w| > 6e4, or non-finite) -- use encoder_bf16 = 3 (the same accuracy) or 0 for this model");
            return P2S_EINVAL;
        }
        // side buffers of the fp32 fallback: inputs + results of up to 16384 flagged queries per call (256 MB at k = 300,
        // n = 1000; touched only when a query is flagged)
        p2s_model_s::Fallback &fb = m->fb;
        fb.cap = 16384;
        const size_t k3 = (size_t)cfg.points_per_patch * 3, n3 = (size_t)cfg.sub_sample_size * 3, cap = fb.cap;
        const bool ok = p2s_alloc_all(fb.flags, (size_t)m->max_chunk, fb.count, 1, fb.patch, cap * k3, fb.sub, cap * n3, fb.query, cap * 3,
                                      fb.radius, cap, fb.index, cap, fb.sdf, cap, fb.logits, cap * 2) &&
                        hipMemset(fb.flags.get(), 0, (size_t)m->max_chunk * 4) == hipSuccess && hipMemset(fb.count.get(), 0, 4) == hipSuccess &&
                        hipMemset(fb.radius.get(), 0, cap * 4) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            p2s_set_error("allocation of the fp32 fallback buffers of the fp16 pair mode failed");
            return P2S_ENOMEM;
        }
    }
    P2S_HIP_CHECK(hipDeviceSynchronize());
    return P2S_OK;
}

extern "C" {

int p2s_abi_version(void) { return P2S_ABI_VERSION; }
const char *p2s_last_error(void) { return g_err; }

int p2s_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int p2s_release_scratch(int device) {
    if (device < 0 || device >= P2S_MAX_DEVICES || device >= p2s_device_count()) {
        p2s_set_error("p2s_release_scratch: no HIP device %d", device);
        return P2S_ENODEVICE;
    }
    P2S_HIP_CHECK(hipSetDevice(device));
    {
        std::lock_guard<std::mutex> g(g_scratch[device].mu);     // waits for a running volume / iso-surface call
        if (g_scratch[device].p) (void)hipFree(g_scratch[device].p);
        g_scratch[device].p = nullptr;
        g_scratch[device].cap = 0;
    }
    p2s_cloud_pool_release(device);
    return P2S_OK;
}

int p2s_model_create(const p2s_model_cfg *cfg, const float *blob_host, size_t n_floats,
                     const p2s_weight_offsets *offs, int device, p2s_model_t *out) {
    if (!cfg || !blob_host || !offs || !out || n_floats == 0) {
        p2s_set_error("p2s_model_create: null argument");
        return P2S_EINVAL;
    }
    if (cfg->net_size != 1024 || (cfg->output_dim != 2 && cfg->output_dim != 1) || cfg->points_per_patch < 1 || cfg->sub_sample_size < 1) {
        p2s_set_error("p2s_model_create: unsupported cfg (net_size=%d output_dim=%d)", cfg->net_size, cfg->output_dim);
        return P2S_EINVAL;
    }
    if (p2s_device_count() <= device || device < 0) {
        p2s_set_error("p2s_model_create: no HIP device %d", device);
        return P2S_ENODEVICE;
    }
    if (cfg->encoder_bf16 < 0 || cfg->encoder_bf16 > 4) {
        p2s_set_error("p2s_model_create: encoder_bf16 = %d (0 fp32, 1 bf16, 2 / 3 split bf16, 4 fp16 pair)", cfg->encoder_bf16);
        return P2S_EINVAL;
    }
    P2S_HIP_CHECK(hipSetDevice(device));
    p2s_model_s *m = new p2s_model_s(*cfg, *offs, device);
    const int rc = model_init(m, blob_host, n_floats);
    if (rc) p2s_model_destroy(m);
    else *out = m;
    return rc;
}

int p2s_model_destroy(p2s_model_t m) {
    if (!m) return P2S_OK;
    (void)hipSetDevice(m->device);
    delete m;          // the members release what they own; the streams (declared first) go last
    return P2S_OK;
}

int p2s_set_profiling(p2s_model_t m, int enabled) {
    if (!m) return P2S_EINVAL;
    m->profiling = enabled != 0;
    return P2S_OK;
}

int p2s_get_counters(p2s_model_t m, p2s_counters *out) {
    if (!m || !out) return P2S_EINVAL;
    *out = m->counters;
    if (m->scr_counters) {            // the screened conv3 counts on the device; valid once the call's stream is synchronised
        unsigned long long h[3] = {};
        P2S_HIP_CHECK(hipSetDevice(m->device));
        P2S_HIP_CHECK(hipMemcpy(h, m->scr_counters.get(), sizeof(h), hipMemcpyDeviceToHost));
        out->conv3_confirmed = (int64_t)h[0];
        out->conv3_items_dense = (int64_t)h[1];
        out->conv3_items = (int64_t)h[2];
    }
    return P2S_OK;
}

}  // extern "C"

int p2s_prof_mark(p2s_model_s *m, hipStream_t s) {
    if (!m->profiling) return -1;
    if (m->ev_used >= (int)m->evpool.size()) {
        DevEvent e;
        if (!e.create()) return -1;
        m->evpool.push_back(std::move(e));
    }
    const int i = m->ev_used++;
    if (hipEventRecord(m->evpool[i].get(), s) != hipSuccess) return -1;
    return i;
}

void p2s_prof_span(p2s_model_s *m, int stage, int a, int b) {
    if (a >= 0 && b >= 0) m->spans.push_back({stage, a, b});
}

static void prof_reset(p2s_model_s *m) {
    m->ev_used = 0;
    m->spans.clear();
    memset(&m->counters, 0, sizeof(m->counters));
}

static void prof_collect(p2s_model_s *m) {           // synchronises the last event
    if (!m->profiling || m->ev_used == 0) return;
    (void)hipEventSynchronize(m->evpool[m->ev_used - 1].get());
    for (const auto &sp : m->spans) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, m->evpool[sp.a].get(), m->evpool[sp.b].get()) != hipSuccess) {
            (void)hipGetLastError();          // an event that was never reached: only this complaint is dropped
            continue;
        }
        double *dst = nullptr;
        switch (sp.stage) {
            case ST_CHAIN_STN: dst = &m->counters.ms_chain_stn; break;
            case ST_HEAD: dst = &m->counters.ms_stn_head; break;
            case ST_CHAIN_MAIN: dst = &m->counters.ms_chain_main; break;
            case ST_DECODER: dst = &m->counters.ms_decoder; break;
            case ST_KNN: dst = &m->counters.ms_knn; break;
            case ST_SUB: dst = &m->counters.ms_subsample; break;
            case ST_GRID: dst = &m->counters.ms_grid; break;
            case ST_CHAIN_QSTN: dst = &m->counters.ms_chain_qstn; break;
        }
        if (dst) *dst += ms;
    }
    m->ev_used = 0;
    m->spans.clear();
}

ModelCall::ModelCall(p2s_model_s *m_, hipStream_t s_, bool pipeline_) : m(m_), s(s_), pipeline(pipeline_) {
    if (!m) return;
    if (pipeline) {
        logits = m->logits_capture;
        logits_room = m->logits_capacity;
        m->logits_capture = nullptr;
        m->logits_capacity = 0;
    }
    rc = [&]() -> int {
        P2S_HIP_CHECK(hipSetDevice(m->device));
        prof_reset(m);
        if (m->scr_counters) P2S_HIP_CHECK(hipMemsetAsync(m->scr_counters.get(), 0, 3 * 8, s));
        if (m->fb.count) {
            P2S_HIP_CHECK(hipMemsetAsync(m->fb.count.get(), 0, 4, s));
            P2S_HIP_CHECK(hipMemsetAsync(m->fb.flags.get(), 0, (size_t)m->max_chunk * 4, s));
        }
        return P2S_OK;
    }();
}

int ModelCall::fail(int code) {
    if (!m) return code;
    (void)hipStreamSynchronize(s);          // (an error here is a real fault and stays pending)
    if (pipeline && m->aux) (void)hipStreamSynchronize(m->aux.get());
    if (pipeline && m->ball) (void)hipStreamSynchronize(m->ball.get());
    return code;
}

int ModelCall::finish(float *logits_out, float *sdf_out, int64_t nq) {
    m->counters.queries += nq;
    const int rc2 = p2s_fallback_finish(m, logits_out, sdf_out, s);
    if (rc2) return fail(rc2);
    prof_collect(m);
    return P2S_OK;
}

static int run_batched(p2s_model_s *m, const float *patch, const float *sub, const float *query, const float *radius,
                       int B, float *logits, float *sdf, float *fl, float *fg, hipStream_t s) {
    ModelCall call(m, s, false);
    if (!m || B < 0 || !patch || !sub || !query) {
        p2s_set_error("encode: null argument");
        return call.fail(P2S_EINVAL);
    }
    if (sdf && !radius) {
        p2s_set_error("encode: sdf_out requested without radius");
        return call.fail(P2S_EINVAL);
    }
    const int chunk = std::min(B, m->max_chunk);
    int rc = call.rc ? call.rc : p2s_model_reserve(m, chunk);
    if (rc) return call.fail(rc);
    const int PL = m->cfg.points_per_patch, PG = m->cfg.sub_sample_size;
    for (int q0 = 0; q0 < B; q0 += chunk) {
        const int C = std::min(chunk, B - q0);
        rc = p2s_run_chunk(m, p2s_precision(m->cfg), patch + (size_t)q0 * PL * 3, sub + (size_t)q0 * PG * 3, query + (size_t)q0 * 3,
                           radius ? radius + q0 : nullptr, C, logits ? logits + (size_t)q0 * m->cfg.output_dim : nullptr,
                           sdf ? sdf + q0 : nullptr, fl ? fl + (size_t)q0 * 1024 : nullptr,
                           fg ? fg + (size_t)q0 * 1024 : nullptr, s, q0);
        if (rc) return call.fail(rc);
    }
    return call.finish(logits, sdf, B);
}

extern "C" {

int p2s_encode_decode(p2s_model_t m, const float *patch_ps_dev, const float *sub_ms_dev, const float *query_dev,
                      const float *radius_dev, int B, float *logits_out_dev, float *sdf_out_dev, void *stream) {
    if (!logits_out_dev && !sdf_out_dev) {
        p2s_set_error("p2s_encode_decode: no output requested");
        return P2S_EINVAL;
    }
    return run_batched(m, patch_ps_dev, sub_ms_dev, query_dev, radius_dev, B, logits_out_dev, sdf_out_dev, nullptr,
                       nullptr, (hipStream_t)stream);
}

int p2s_encode_features(p2s_model_t m, const float *patch_ps_dev, const float *sub_ms_dev, const float *query_dev,
                        int B, float *feat_local_dev, float *feat_global_dev, void *stream) {
    if (!feat_local_dev && !feat_global_dev) {
        p2s_set_error("p2s_encode_features: no output requested");
        return P2S_EINVAL;
    }
    return run_batched(m, patch_ps_dev, sub_ms_dev, query_dev, nullptr, B, nullptr, nullptr, feat_local_dev,
                       feat_global_dev, (hipStream_t)stream);
}

}  // extern "C"
