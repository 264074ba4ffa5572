// Workers mode: the reference's sub-sample streams under ``--workers W --batchSize B`` (include/p2s_hip.h,
// points2surf_amd/streams.py is the host model).
//
// The query at dataset position g draws from worker stream (g // B) mod W.  The pipeline runs over the queries in
// stream-major order -- stream 0's queries in increasing g, then stream 1's, ... -- as consecutive segments, each on its
// own generator twins; the SDF (and captured logits) come out in that order and one scatter puts them back.
//
//   p2s_stream_order       the permutation, arithmetically from (g0, n, W, B): no host table, one pass
//   p2s_subsample_workers  the global sub-sample in workers mode, in query order (data-path tests, stream skip)
#include "p2s_common.h"
#include "p2s_internal.h"
#include <algorithm>
#include <vector>

namespace {

constexpr int kMaxStreams = 1024;     // worker processes of one DataLoader: far beyond any real --workers

// number of positions g in [0, x) with (g / B) % W == w
__host__ __device__ inline long long stream_count_below(long long x, long long w, long long W, long long B) {
    const long long cyc = W * B;
    const long long rem = x % cyc - w * B;
    return (x / cyc) * B + (rem < 0 ? 0 : (rem > B ? B : rem));
}

// slot i of the stream-major order: the stream whose prefix range holds i (binary search over the per-stream offsets the
// block computed into LDS), then the (rank)-th position of that stream at or after g0
__global__ __launch_bounds__(256) void p2s_stream_order_kernel(long long g0, long long n, int W, int B, const float *__restrict__ q_in,
                                                               float *__restrict__ q_out, long long *__restrict__ src) {
    __shared__ long long off[kMaxStreams + 1];
    __shared__ long long base[kMaxStreams];
    for (int w = threadIdx.x; w < W; w += blockDim.x) base[w] = stream_count_below(g0, w, W, B);
    __syncthreads();
    if (threadIdx.x == 0) {
        long long acc = 0;
        for (int w = 0; w < W; ++w) {
            off[w] = acc;
            acc += stream_count_below(g0 + n, w, W, B) - base[w];
        }
        off[W] = acc;
    }
    __syncthreads();
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int lo = 0, hi = W - 1;           // the last w with off[w] <= i
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    const long long k = base[lo] + (i - off[lo]);
    const long long g = (k / B) * ((long long)W * B) + (long long)lo * B + k % B;
    const long long j = g - g0;
    if (src) src[i] = j;
    if (q_out) {
        q_out[3 * i + 0] = q_in[3 * j + 0];
        q_out[3 * i + 1] = q_in[3 * j + 1];
        q_out[3 * i + 2] = q_in[3 * j + 2];
    }
}

// out[src[i]][d] = in[i][d] for rows of `dim` 32-bit values
__global__ __launch_bounds__(256) void p2s_scatter_rows_kernel(const long long *__restrict__ src, long long total, int dim,
                                                               const uint32_t *__restrict__ in, uint32_t *__restrict__ out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const long long i = t / dim, d = t - i * dim;
    out[src[i] * dim + d] = in[t];
}

int scatter_rows(const int64_t *src, int64_t n, int dim, const void *in, void *out, hipStream_t s) {
    const long long total = (long long)n * dim;
    if (total <= 0) return P2S_OK;
    hipLaunchKernelGGL(p2s_scatter_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const long long *)src, total,
                       dim, (const uint32_t *)in, (uint32_t *)out);
    P2S_LAUNCH_CHECK("p2s_scatter_rows_kernel");
    return P2S_OK;
}

void stream_counts(int64_t g0, int64_t n, int W, int B, int64_t *counts) {
    for (int w = 0; w < W; ++w)
        counts[w] = stream_count_below(g0 + n, w, W, B) - stream_count_below(g0, w, W, B);
}

}  // namespace

int p2s_launch_stream_order(int64_t g0, int64_t n, int W, int B, const float *q_in, float *q_out, int64_t *src, hipStream_t s) {
    if (n <= 0) return P2S_OK;
    hipLaunchKernelGGL(p2s_stream_order_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (long long)g0, (long long)n, W, B,
                       q_in, q_out, (long long *)src);
    P2S_LAUNCH_CHECK("p2s_stream_order_kernel");
    return P2S_OK;
}

int p2s_launch_unpermute(const int64_t *src, int64_t n, const float *sdf_in, float *sdf_out, const float *logits_in,
                         float *logits_out, int dim, hipStream_t s) {
    int rc = scatter_rows(src, n, 1, sdf_in, sdf_out, s);
    if (!rc && logits_in && logits_out) rc = scatter_rows(src, n, dim, logits_in, logits_out, s);
    return rc;
}

int p2s_workers_reserve(p2s_model_s *m, int64_t n) {
    p2s_model_s::Workers &w = m->wk;
    if (w.cap >= n) return P2S_OK;
    P2S_HIP_CHECK(hipDeviceSynchronize());
    w = p2s_model_s::Workers();
    const size_t cap = n + n / 4 + 1024;
    const int dim = std::max(m->cfg.output_dim, 1);
    if (!p2s_alloc_all(w.q, cap * 3, w.src, cap, w.sdf, cap, w.logits, cap * dim)) {
        p2s_set_error("workers mode: allocation of the stream-order buffers failed (%lld queries)", (long long)cap);
        return P2S_ENOMEM;
    }
    w.cap = cap;
    return P2S_OK;
}

int p2s_workers_check(const p2s_worker_streams *ws, bool need_first, const char *who) {
    if (!ws || !ws->sub) {
        p2s_set_error("%s: no worker streams", who);
        return P2S_EINVAL;
    }
    const int W = ws->n_streams;
    if (W < 1 || W > kMaxStreams || ws->batch < 1 || ws->first_position < 0) {
        p2s_set_error("%s: workers %d (1..%d), batch size %d (>= 1), first position %lld (>= 0)", who, W, kMaxStreams, ws->batch,
                      (long long)ws->first_position);
        return P2S_EINVAL;
    }
    if (need_first && !ws->first) {
        p2s_set_error("%s: the call draws from the first generator (patch choice / rotation): worker streams without it", who);
        return P2S_EINVAL;
    }
    std::vector<p2s_rng_s *> all;
    for (int w = 0; w < W; ++w) {
        all.push_back(ws->sub[w]);
        if (ws->first) all.push_back(ws->first[w]);
    }
    for (p2s_rng_s *r : all)
        if (!r) {
            p2s_set_error("%s: null generator handle among the worker streams", who);
            return P2S_EINVAL;
        }
    std::sort(all.begin(), all.end());
    if (std::adjacent_find(all.begin(), all.end()) != all.end()) {
        p2s_set_error("%s: a generator handle appears twice among the worker streams (every worker owns its own)", who);
        return P2S_EINVAL;
    }
    return P2S_OK;
}

int p2s_workers_segments(const p2s_worker_streams *ws, int64_t n, std::vector<P2sSegment> &segs) {
    std::vector<int64_t> counts(ws->n_streams);
    stream_counts(ws->first_position, n, ws->n_streams, ws->batch, counts.data());
    segs.clear();
    for (int w = 0; w < ws->n_streams; ++w)
        if (counts[w] > 0) segs.push_back({ws->sub[w], ws->first ? ws->first[w] : nullptr, counts[w]});
    return P2S_OK;
}

extern "C" int p2s_stream_order(int64_t first_position, int64_t n, int n_streams, int batch, const float *q_in_dev, float *q_out_dev,
                                int64_t *src_out_dev, int64_t *counts_host, void *stream) {
    if (n < 0 || first_position < 0 || n_streams < 1 || n_streams > kMaxStreams || batch < 1 || (!q_in_dev) != (!q_out_dev) ||
        (q_in_dev && q_in_dev == q_out_dev)) {
        p2s_set_error("p2s_stream_order: bad argument (n %lld, first position %lld, workers %d of at most %d, batch %d; q_in / q_out "
                      "both given and distinct, or both NULL)", (long long)n, (long long)first_position, n_streams, kMaxStreams, batch);
        return P2S_EINVAL;
    }
    if (counts_host) stream_counts(first_position, n, n_streams, batch, counts_host);
    if (n == 0 || (!q_out_dev && !src_out_dev)) return P2S_OK;
    return p2s_launch_stream_order(first_position, n, n_streams, batch, q_in_dev, q_out_dev, src_out_dev, (hipStream_t)stream);
}

extern "C" int p2s_subsample_workers(p2s_cloud_t c, const p2s_worker_streams *ws, const float *q_dev, int64_t n_queries, int n,
                                     int weighted, int32_t *ids_out_dev, float *pts_out_dev, void *stream) {
    if (!c || n_queries < 0 || n < 1 || (weighted && n_queries > 0 && !q_dev) || (pts_out_dev && !ids_out_dev)) {
        p2s_set_error("p2s_subsample_workers: bad argument (weighted needs the queries, the points need the ids)");
        return P2S_EINVAL;
    }
    int rc = p2s_workers_check(ws, false, "p2s_subsample_workers");
    if (rc) return rc;
    if (c->d.n < n) {
        p2s_set_error("p2s_subsample_workers: cloud of %d points, fewer than the sub-sample of %d: every worker shuffles its own "
                      "cached copy of shape.pts -- not modelled", c->d.n, n);
        return P2S_EINVAL;
    }
    if (n_queries == 0) return P2S_OK;
    P2S_HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    std::vector<P2sSegment> segs;
    p2s_workers_segments(ws, n_queries, segs);
    DevBuf<float> q_perm;
    DevBuf<int64_t> src;
    DevBuf<int32_t> ids_perm;
    // every exit drains the stream before the buffers above go out of scope: kernels queued on it read and write them
    auto release = [&](int code) {
        const hipError_t e = hipStreamSynchronize(s);
        if (code == P2S_OK && e != hipSuccess) {
            p2s_set_error("p2s_subsample_workers: %s", hipGetErrorString(e));
            return (int)P2S_EHIP;
        }
        return code;
    };
    if (!p2s_alloc_all(q_perm, weighted ? (size_t)n_queries * 3 : 0, src, n_queries, ids_perm,
                       ids_out_dev ? (size_t)n_queries * n : 0)) {
        p2s_set_error("p2s_subsample_workers: allocation failed (%lld queries)", (long long)n_queries);
        return release(P2S_ENOMEM);
    }
    if ((rc = p2s_launch_stream_order(ws->first_position, n_queries, ws->n_streams, ws->batch, weighted ? q_dev : nullptr, q_perm.get(), src.get(), s)))
        return release(rc);
    int64_t at = 0;
    for (const P2sSegment &g : segs) {
        int32_t *ids = ids_perm ? ids_perm.get() + (size_t)at * n : nullptr;
        rc = weighted ? p2s_subsample_weighted(g.sub, c, q_perm.get() + (size_t)at * 3, g.rows, n, ids, nullptr, s)
                      : p2s_subsample_uniform(g.sub, c, g.rows, n, ids, nullptr, s);
        if (rc) return release(rc);
        at += g.rows;
    }
    if (ids_out_dev && (rc = scatter_rows(src.get(), n_queries, n, ids_perm.get(), ids_out_dev, s))) return release(rc);
    if (pts_out_dev && (rc = p2s_gather_points(c, ids_out_dev, n_queries * n, pts_out_dev, s))) return release(rc);
    for (const P2sSegment &g : segs)
        if ((rc = p2s_rng_check(g.sub, s))) return release(rc);
    return release(P2S_OK);
}
