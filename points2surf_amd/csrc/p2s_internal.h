// Handle definitions shared by the API translation units.
#pragma once
#include "p2s_common.h"
#include "p2s_devmem.h"
#include <vector>
#include <cstddef>

// per-shape pipeline buffers (p2s_pipeline.hip): owned by the model handle, grown on demand, reused across
// shapes, released by p2s_model_destroy -- no allocation and no leak on the per-shape path
struct PipeBuffers {
    DevBuf<float> patch[2];         // [C][k][3]
    DevBuf<float> radius[2];        // [C]
    DevBuf<int32_t> sub_ids[2];     // [C][n]
    DevBuf<float> sub[2];           // [C][n][3]
    DevBuf<float> qrot[2];          // [C][3]   rotated query points (GT-query pass)
    DevBuf<double> rot[2];          // [C][9]   per-query rotation (GT-query pass)
    DevEvent ready[2];              // data path of the buffer finished (aux stream)
    DevEvent freed[2];              // the gather has read the sub-sample ids of the buffer (compute stream)
    DevEvent done[2];               // encoders finished reading the buffer (main stream)
    DevEvent ball_ready[2];         // fixed-radius patch of the buffer finished (ball stream)
    DevEvent grid;
    DevBuf<int32_t> knn_ids[2];     // [C][k]   } only for clouds with fewer points than the sub-sample
    DevBuf<int32_t> perm[2];        // [C][N]   } (shape.pts is shuffled in place by every query)
    int cap_chunk = 0, cap_k = 0, cap_n = 0, cap_small = 0;
};

// Precision of one run of the network.  cfg.encoder_bf16: 0 fp32, 1 bf16, 2 / 3 split bf16, 4 fp16 pair (2 pieces, two
// accumulators; the encoder-side head layers on 16-bit fragments too, queries beyond the half range flagged and collected)
struct Precision {
    int pieces;              // 16-bit pieces per operand of the per-point layers; 0: the fp32 kernels
    bool f16;                // the pieces are an fp16 pair
};
constexpr Precision P2S_FP32 = {0, false};
inline Precision p2s_precision(const p2s_model_cfg &c) { return {c.encoder_bf16 == 4 ? 2 : c.encoder_bf16, c.encoder_bf16 == 4}; }

// The FC / per-point layers whose weights are packed MFMA B fragments, each named once: where p2s_weight_offsets holds the
// offsets of its fp32 fragments and of its bias (slice 1 -- the second encoder, fc1_global -- `slice` bytes further), its
// shape, and when it has 16-bit fragments in blob_h as well.  The kinds are the groups of blob_h, in its order.
enum P2sLayerKind {
    LK_ENC,                  // per-point layers of both encoders: any 16-bit precision, encoder by encoder
    LK_QSTN,                 // per-point layers of the QSTN: any 16-bit precision, models with use_point_stn
    LK_ENC_HEAD,             // STN fc1..fc3 of both encoders: fp16 pair, encoder by encoder
    LK_QSTN_HEAD,            // QSTN fc1 / fc2: fp16 pair, models with use_point_stn
    LK_FP32                  // decoder: fp32 only
};
enum P2sLayer { L_W0B, L_S1, L_S2, L_S3, L_M2, L_M3, L_QC2, L_QC3, L_SF1, L_SF2, L_SF3, L_QF1, L_QF2, L_D1, L_D2, L_D3, P2S_LAYERS };
struct P2sLayerDesc { P2sLayerKind kind; size_t w, b, slice; int K, N; };
#define P2S_AT(w, b) offsetof(p2s_weight_offsets, w), offsetof(p2s_weight_offsets, b)
constexpr size_t P2S_PER_ENC = sizeof(p2s_encoder_offsets);
inline constexpr P2sLayerDesc p2s_layers[P2S_LAYERS] = {
    {LK_ENC, P2S_AT(enc[0].w0b, enc[0].b0b), P2S_PER_ENC, 64, 64},         {LK_ENC, P2S_AT(enc[0].s1, enc[0].sb1), P2S_PER_ENC, 64, 64},
    {LK_ENC, P2S_AT(enc[0].s2, enc[0].sb2), P2S_PER_ENC, 64, 128},         {LK_ENC, P2S_AT(enc[0].s3, enc[0].sb3), P2S_PER_ENC, 128, 1024},
    {LK_ENC, P2S_AT(enc[0].m2, enc[0].mb2), P2S_PER_ENC, 64, 128},         {LK_ENC, P2S_AT(enc[0].m3, enc[0].mb3), P2S_PER_ENC, 128, 1024},
    {LK_QSTN, P2S_AT(qstn.c2, qstn.cb2), 0, 64, 128},                      {LK_QSTN, P2S_AT(qstn.c3, qstn.cb3), 0, 128, 1024},
    {LK_ENC_HEAD, P2S_AT(enc[0].sf1, enc[0].sfb1), P2S_PER_ENC, 1024, 512}, {LK_ENC_HEAD, P2S_AT(enc[0].sf2, enc[0].sfb2), P2S_PER_ENC, 512, 256},
    {LK_ENC_HEAD, P2S_AT(enc[0].sf3, enc[0].sfb3), P2S_PER_ENC, 256, 4096},
    {LK_QSTN_HEAD, P2S_AT(qstn.f1, qstn.fb1), 0, 1024, 512},               {LK_QSTN_HEAD, P2S_AT(qstn.f2, qstn.fb2), 0, 512, 256},
    {LK_FP32, P2S_AT(d1l, db1l), offsetof(p2s_weight_offsets, d1g) - offsetof(p2s_weight_offsets, d1l), 1024, 512},
    {LK_FP32, P2S_AT(d2, db2), 0, 1024, 256},                              {LK_FP32, P2S_AT(d3, db3), 0, 256, 128},
};
#undef P2S_AT
// does a model of this configuration hold 16-bit fragments of the layers of `kind`?
inline bool p2s_kind_packed(P2sLayerKind kind, const p2s_model_cfg &c) {
    const Precision p = p2s_precision(c);
    const bool head = kind == LK_ENC_HEAD || kind == LK_QSTN_HEAD, qstn = kind == LK_QSTN || kind == LK_QSTN_HEAD;
    return kind != LK_FP32 && (head ? p.f16 : p.pieces != 0) && (!qstn || c.use_point_stn);
}

struct p2s_model_s {
    const p2s_model_cfg cfg;
    const p2s_weight_offsets offs;
    const int device;
    // auxiliary stream: the data path (kNN, sub-sample) of chunk i+1, i+2 overlaps the encoders of chunk i.  The streams are
    // declared in front of every buffer: members go in reverse order, so the streams are destroyed after the buffers are released
    DevStream aux;                 // high-priority stream of the sub-sample generator
    DevStream ball;                // fixed-radius models: the serial walk along the first generator's stream (one wave) -- its own
                                   // stream so that it runs beside the sub-sample kernels of the auxiliary stream, not behind them
    DevBuf<float> blob;
    // 16-bit encoder modes: 16-bit B fragments of the layers p2s_kind_packed() names, converted once at creation
    DevBuf<unsigned short> blob_h;         // [pieces][h_total]
    size_t h_total = 0;
    size_t h_off[P2S_LAYERS][2] = {};      // of slice 0 / 1 of a layer within a piece (a layer without slices: the same twice)
    p2s_model_s(const p2s_model_cfg &c, const p2s_weight_offsets &o, int dev) : cfg(c), offs(o), device(dev) {}
    // the operands of `layer`, slice z: fp32 fragments / bias in blob, piece 0 of the 16-bit fragments in blob_h
    const float *w32(P2sLayer layer, int z) const { return blob.get() + offset(p2s_layers[layer].w + z * p2s_layers[layer].slice); }
    const float *bias(P2sLayer layer, int z) const { return blob.get() + offset(p2s_layers[layer].b + z * p2s_layers[layer].slice); }
    const unsigned short *w16(P2sLayer layer, int z) const { return blob_h.get() + h_off[layer][z]; }
    uint64_t offset(size_t member) const { return *reinterpret_cast<const uint64_t *>(reinterpret_cast<const char *>(&offs) + member); }
    // screened conv3 of the fp32 kernel (p2s_chain_screen.inl; mode 0 only): the conv3
    // layers of the STN and main trunks (layer = L_S3 / L_M3, encoder z) rounded to fp16, as fragments [2][2][P2S_SCR_PIECE], and
    // their margin coefficients [2][2][1024], built at creation; NULL: the dense conv3 (P2S_CONV3_DENSE=1, a sym_op='sum' main
    // trunk keeps it for that pass, a conv3 weight beyond the half range for the model)
    DevBuf<unsigned short> scr_w3h;
    DevBuf<float> scr_mu;
    DevBuf<unsigned long long> scr_counters;        // device [3]: fp32 chains run, items re-run densely, items -- per call
    const unsigned short *screen_w(P2sLayer layer, int z) const { return scr_w3h.get() + ((layer == L_M3 ? 2 : 0) + z) * P2S_SCR_PIECE; }
    const float *screen_mu(P2sLayer layer, int z) const { return scr_mu.get() + ((layer == L_M3 ? 2 : 0) + z) * 1024; }
    // fp16 pair mode: queries with an activation beyond the half range are flagged by the 16-bit kernels, collected per
    // chunk (inputs copied aside) and re-run through the fp32 kernels at the end of the same call (ModelCall::finish)
    struct Fallback {
        DevBuf<int> flags;                 // [max_chunk] per query of the chunk in flight
        DevBuf<int> count;                 // queries collected by the call (may run past cap: overflow)
        DevBuf<float> patch, sub, query, radius;   // [cap] inputs of the collected queries
        DevBuf<long long> index;           // [cap] position in the call's output arrays
        DevBuf<float> sdf, logits;         // [cap] results of the fp32 run
        int cap = 0;
    } fb;
    // one-shot capture of the decoder logits of the next pipeline call (p2s_model_capture_logits; the drop-in's tie report)
    float *logits_capture = nullptr;
    int64_t logits_capacity = 0;
    DevBuf<float> ws;         // per-chunk workspace, grown on demand
    int ws_chunk = 0;
    // stem reuse: the main encoder pass starts at conv1 from the conv0b output the STN pass saved in the
    // workspace.  Decided once, at creation: the model's own precision is fp32, its conv3 is screened and its main pass pools by
    // max (cfg.stem_recompute switches it off) -- not per run: the fp32 fall-back of an fp16 pair model runs inside that model's
    // 16-bit workspace.  stem_max_bytes (cfg.stem_reuse_max_mb): a chunk whose region would be larger, or does not fit the
    // device, is reserved without it (ws_stem) and recomputes the stem
    bool stem_reuse = false;
    size_t stem_max_bytes = 0;
    bool ws_stem = false;
    int max_chunk = 8192;     // queries per internal batch (r03: 4096 -> 8192: 180.4 -> 182.0 k queries/s, the launch boundaries
                              // of a chunk -- four drains of the chip -- weigh half as much; 12288: 182.1 k)
    // profiling: HIP events recorded on the launch stream, no host synchronisation until collect
    bool profiling = false;
    std::vector<DevEvent> evpool;
    int ev_used = 0;
    struct Span { int stage, a, b; };
    std::vector<Span> spans;
    p2s_counters counters = {};
    bool overlap = true;
    PipeBuffers pipe;
    int fault_chunk = -1;          // test hook (p2s_debug_fault_chunk): fail with P2S_EHIP before this chunk
    // workers mode (p2s_streams.hip): the stream-ordered queries, their source indices and the SDF / logits produced in that
    // order, before the scatter to the caller's buffers; grown on demand
    struct Workers {
        DevBuf<float> q, sdf, logits;
        DevBuf<int64_t> src;
        int64_t cap = 0;
    } wk;
};

// consecutive pipeline queries and their generators (first: patch choice / rotation, NULL if unused): dataset mode is one
// segment, workers mode (p2s_streams.hip) one per non-empty stream
struct P2sSegment {
    p2s_rng_s *sub;
    p2s_rng_s *first;
    int64_t rows;
};
int p2s_workers_reserve(p2s_model_s *m, int64_t n);
// validation of a p2s_worker_streams (need_first: the call draws from the first generators); counts: the per-stream query
// counts of n queries at ws->first_position; segs: the non-empty streams as pipeline segments
int p2s_workers_check(const p2s_worker_streams *ws, bool need_first, const char *who);
int p2s_workers_segments(const p2s_worker_streams *ws, int64_t n, std::vector<P2sSegment> &segs);
int p2s_launch_stream_order(int64_t g0, int64_t n, int W, int B, const float *q_in, float *q_out, int64_t *src, hipStream_t s);
int p2s_launch_unpermute(const int64_t *src, int64_t n, const float *sdf_in, float *sdf_out, const float *logits_in,
                         float *logits_out, int dim, hipStream_t s);

// One call of a model entry point (p2s_encode_*, the pipeline calls), constructed first.  Construction (m == NULL: nothing)
// takes the one-shot logits capture off the model (pipeline calls, whatever the outcome), sets the device, resets the profile
// and clears the fp16-pair fallback state on `s`: nothing an earlier call left there is re-run or scattered by this one.
struct ModelCall {
    p2s_model_s *const m;
    const hipStream_t s;
    const bool pipeline;
    float *logits = nullptr;      // pipeline calls: the capture buffer [logits_room][output_dim] (p2s_model_capture_logits)
    int64_t logits_room = 0;
    int rc = P2S_OK;              // outcome of the set-up
    ModelCall(p2s_model_s *m, hipStream_t s, bool pipeline);
    // every error exit: drains `s` (pipeline calls: the model's own streams too), so the next call's reset is ordered; -> code
    int fail(int code);
    // the success exit: counters.queries += nq; fp16 pair mode: the flagged queries (an activation beyond the half range) re-run
    // in fp32 into logits_out [.][output_dim] / sdf_out (either may be NULL; synchronises `s`; more than the 16384 the side
    // buffers hold, or neither output: P2S_EINVAL); the profile is collected
    int finish(float *logits_out, float *sdf_out, int64_t nq);
};

enum P2SStage { ST_CHAIN_STN = 0, ST_HEAD, ST_CHAIN_MAIN, ST_DECODER, ST_KNN, ST_SUB, ST_GRID, ST_CHAIN_QSTN };
int p2s_prof_mark(p2s_model_s *m, hipStream_t s);                 // event index or -1
void p2s_prof_span(p2s_model_s *m, int stage, int a, int b);

// the forward pass (p2s_forward.hip)
int p2s_model_reserve(p2s_model_s *m, int chunk);
// One chunk (C <= ws_chunk queries) at `prec`: the model's own, or P2S_FP32 (the fp32 fragments are resident in any mode).
// index0: position of the chunk's first query in the output arrays of the call's finish() (what the fp32 fallback scatters to)
int p2s_run_chunk(p2s_model_s *m, Precision prec, const float *patch, const float *sub, const float *query, const float *radius,
                  int C, float *logits_out, float *sdf_out, float *feat_local_out, float *feat_global_out,
                  hipStream_t s, long long index0 = 0);
// fp16 pair mode (ModelCall::finish): the collected queries through the fp32 kernels, their results scattered over the outputs
int p2s_fallback_finish(p2s_model_s *m, float *logits_out, float *sdf_out, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// cloud / rng handles (p2s_cloud.hip, p2s_rng.hip)
// ---------------------------------------------------------------------------------------------
struct CloudDev {
    const float *pts;        // [n][3] original order (owned copy)
    const float4 *spts;      // [n] sorted by cell: xyz + original id (bit cast)
    const int *cell_start;   // [G^3 + 1]
    const int *sat;          // [(G+1)^3] inclusive 3-D prefix sums of the per-cell counts
    float lo[3];
    float inv_cell;
    int G;
    int n;
};

struct p2s_cloud_s {
    int device = 0;
    CloudDev d = {};
    // one block of the device's cache (p2s_pool_alloc) holds pts, spts, cell_start, sat, totals + the build scratch
    char *arena = nullptr;
    float *pts = nullptr;
    float4 *spts = nullptr;
    int *cell_start = nullptr;
    int *sat = nullptr;
    // streams that may have work on this handle's memory in flight: drained before its blocks return to the cache
    hipStream_t streams[4] = {};
    int n_streams = 0;
    bool many_streams = false;
    // > 0 while a per-shape pipeline runs on this handle: the model-owned auxiliary streams it uses are NOT noted --
    // run_pipeline drains them on every exit, and a handle must never synchronise a stream it does not own (the model
    // may be destroyed before the cloud)
    int foreign_streams_quiet = 0;
    // query-grid scratch (grown on demand)
    uint32_t *occ = nullptr;
    size_t occ_words = 0;
    int *blk_cnt = nullptr;
    size_t blk_cap = 0;
    long long *totals = nullptr;   // [2] device: total count, error flag
    int *shuffle_perm = nullptr;   // clouds with fewer points than the sub-sample: current row order of shape.pts
    // the last query grid stays on the handle: the pipeline and the callers that size their outputs share it
    float *qcache = nullptr;
    int qc_res = 0, qc_eps = 0;
    long long qc_n = -1, qc_cap = 0;
    hipEvent_t grid_ev = nullptr;  // recorded behind the compaction of the cached grid on grid_stream
    hipStream_t grid_stream = nullptr;
    // summation plan of np.sum(float32[n]) for the weighted sub-sample (p2s_wchoice.hip), built on first use
    int *wc_plan = nullptr;        // device: leaves [L][3], ops [O][3], level offsets [levels+1]
    int wc_leaves = 0, wc_ops_at = 0, wc_lvl_at = 0, wc_levels = 0, wc_root = 0, wc_nodes = 0;
    // fixed-radius patches (p2s_ball.hip), built on first use: the cloud in scipy's cKDTree(pts, 1000).indices order
    char *kd_blob = nullptr;
    float4 *kd_pts = nullptr;      // [n] xyz + original id
    int *kd_leaf = nullptr;        // [kd_leaves + 1] leaf ranges
    float *kd_box = nullptr;       // [kd_leaves][6] lo, hi of each leaf's points
    int kd_leaves = 0;
};

// one run of items of a cloud-set sub-sample that draw from clouds of the same size, as the serial generator walks it
// (p2s_mt_randint_seg_kernel): `count` values in [0, rng] by masked rejection, written from out[out_begin] on
struct P2sRandSeg {
    uint32_t rng, mask;
    long long out_begin, count;
};

// a set of clouds behind one handle (p2s_cloudset_*): borrows the clouds, owns the descriptor table and the per-call buffers
struct p2s_cloudset_s {
    int device = 0;
    std::vector<int> n_points;     // per cloud (host)
    int min_points = 0;
    DevBuf<CloudDev> table;        // device [n_clouds]
    // per-call inputs: filled in pinned host memory, copied on the call's stream; `copied` is recorded behind the copies
    // and waited for before the pinned side is written again
    struct Items {
        PinnedBuf<int32_t> cloud_of_pin;
        PinnedBuf<P2sRandSeg> seg_pin;
        DevBuf<int32_t> cloud_of_dev;
        DevBuf<P2sRandSeg> seg_dev;
        int64_t cap = 0;
    } items;
    DevEvent copied;
    hipStream_t last = nullptr;    // stream of the last call: a call on another one waits for it (the buffers are shared)
    bool used = false;
    hipStream_t streams[4] = {};   // as p2s_cloud_s: drained by destroy
    int n_streams = 0;
    bool many_streams = false;
};

struct p2s_rng_s {
    int device = 0;
    DevBuf<uint32_t> state;        // [624] mt + [1] pos
    // parallel generation (GF(2) jump-ahead), optional: tables uploaded by p2s_rng_set_jump_tables
    int levels_max = 0;            // jump tables uploaded (sessions use 2^levels_max streams)
    int levels_alloc = 0;          // tmp / blk_cum sized for 2^levels_alloc streams
    int blocks_per_stream = 0;
    // session (p2s_rng.hip): 0 closed, 1 randint values, 2 raw words
    int sess_mode = 0;
    uint32_t sess_rng = 0, sess_mask = 0;
    long long sess_cursor = 0;     // mode 1: values handed out; mode 2: conservative word estimate
    long long sess_limit = 0;
    DevBuf<uint16_t> jump_sup;     // concatenated supports of the jump polynomials
    int jump_off[16] = {};         // offset / count per level
    int jump_cnt[16] = {};
    DevBuf<uint32_t> streams;      // [S][624] block states
    DevBuf<uint32_t> tmp;          // [S][B*624] accepted values per stream
    DevBuf<int> blk_cum;           // [S][B] cumulative accepted count per block
    DevBuf<long long> meta;        // [S] offsets + locate record + sticky error flag + raw-request record
    // weighted sub-sample workspace (p2s_wchoice.hip), grown on demand
    struct WChoice {
        DevBuf<double> S;          // [C][n]   exact prefix sums of the probabilities
        DevBuf<void> T;            // [C][K]   guide records of the cdf (16 B each)
        DevBuf<double> sc;         // [C][5]   per-query scalars (stot, word offset, pmax, dmax + sum, mu)
        DevBuf<void> spec;         // offsets pass: ctl, window origins, verdicts [SP_B][SP_W], tentative path, saved windows, scratch
        DevBuf<unsigned short> J;  // [2 SP_B][SP_W] ruler of jump tables of the offsets chain (p2s_wchoice.hip)
        size_t cap_q = 0, cap_n = 0, cap_k = 0;
        DevBuf<long long> stats;   // [16] development counters (P2S_WC_STATS)
    } wc;
    // fixed-radius patches (p2s_ball.hip): hit counts of a shape's queries (device + pinned host), batch work space
    DevBuf<int32_t> ball_counts_dev;
    PinnedBuf<int32_t> ball_counts_host;
    size_t ball_counts_cap = 0;
    DevBuf<void> ball_ws;
    size_t ball_ws_bytes = 0;
};

// per-device cache of device-memory blocks for the cloud handles (p2s_cloud.hip)
void *p2s_pool_alloc(int device, size_t bytes);
void p2s_pool_free(int device, void *p);
void p2s_cloud_note_stream(p2s_cloud_s *c, hipStream_t s);


// query grid of (res, eps), computed once per cloud handle and kept on the device (p2s_cloud.hip); *q is owned by
// the handle and valid until the next call with other parameters; stream-ordered on `s` (synchronises it once to
// learn the count)
int p2s_cloud_grid(p2s_cloud_s *c, int res, int eps, const float **q, long long *n, hipStream_t s);

// serial generator (p2s_cloud.hip) and parallel generator (p2s_rng.hip)
int p2s_rng_serial_randint(p2s_rng_s *r, uint32_t rng, uint32_t mask, long long target, int32_t *out, hipStream_t s);
// sessions: one large generated segment of the stream that many calls draw from (p2s_rng.hip)
long long p2s_rng_session_words(const p2s_rng_s *r);           // raw words a session holds
long long *p2s_rng_raw_meta(p2s_rng_s *r);                     // device: [0] word cursor of the raw session, [1] sticky error
int p2s_rng_session_close(p2s_rng_s *r, hipStream_t s);        // advance the generator to the cursor; no-op if closed
int p2s_rng_session_randint(p2s_rng_s *r, uint32_t rng, uint32_t mask, long long target, int32_t *out, hipStream_t s);
int p2s_rng_session_raw(p2s_rng_s *r, long long need_words, hipStream_t s);
// fixed-radius patches (p2s_ball.hip)
int p2s_cloud_kd_prepare(p2s_cloud_s *c);
int p2s_ball_counts_to_host(p2s_rng_s *r, p2s_cloud_s *c, const float *q_dev, int64_t nq, double radius, int32_t **count_dev,
                            const int32_t **count_host, hipStream_t s);
// patch_out_dev == NULL: advance the generator only
int p2s_ball_patch_counted(p2s_rng_s *r, p2s_cloud_s *c, const float *q_dev, const int32_t *count_dev, const int32_t *count_host,
                           int64_t nq, double radius, int k, int tail_words, int32_t *ids_out_dev, float *patch_out_dev,
                           float *radius_out_dev, double *rot_out_dev, hipStream_t s);
// rand(3) -> rotation matrix for n queries whose 6 words lie contiguously at six_dev[6 * i] (p2s_pipeline.hip)
int p2s_rotations_from_words(const uint32_t *six_dev, long long n, double *rot_out_dev, hipStream_t s);
void p2s_mt_seed_host(uint32_t seed, uint32_t st[625]);                 // init_genrand
int p2s_rng_reseed(p2s_rng_s *r, uint32_t seed, hipStream_t s);         // rng.seed(seed): closes any session
int p2s_wc_subsample_fixed(p2s_rng_s *r, p2s_cloud_s *c, const float *q_dev, int64_t nq, int n_sel, uint32_t seed,
                           int32_t *ids_out_dev, float *pts_out_dev, hipStream_t s);
