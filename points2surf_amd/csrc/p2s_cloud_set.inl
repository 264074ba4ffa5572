// A set of clouds behind one handle (included at the end of p2s_cloud.hip): the training loader's batches draw every item
// from another cloud, and one call serves them all.  The set borrows its clouds -- it copies their descriptors (CloudDev)
// into one device table and keeps their point counts on the host; the clouds must outlive it.
namespace {

void cloudset_note_stream(p2s_cloudset_s *s, hipStream_t st) {
    for (int i = 0; i < s->n_streams; ++i)
        if (s->streams[i] == st) return;
    if (s->n_streams < 4) s->streams[s->n_streams++] = st;
    else s->many_streams = true;
}

// Host checks of one call (`who`: its name; `limit`: its k or n, named `what`, which no item's cloud may fall short of),
// then the per-item cloud ids on the device in s->items.cloud_of_dev, ordered on `st`.  When this returns P2S_OK the pinned
// buffers are free for writing and the device buffers hold at least nq entries.
int cloudset_begin(p2s_cloudset_s *s, const char *who, const char *what, const int32_t *cloud_of, int64_t nq, int limit,
                   hipStream_t st) {
    const int nc = (int)s->n_points.size();
    for (int64_t i = 0; i < nq; ++i) {
        const int c = cloud_of[i];
        if (c < 0 || c >= nc) {
            p2s_set_error("%s: item %lld names cloud %d; the set holds clouds 0 .. %d", who, (long long)i, c, nc - 1);
            return P2S_EINVAL;
        }
        if (limit > s->n_points[c]) {
            p2s_set_error("%s: item %lld: cloud %d has %d points < %s=%d", who, (long long)i, c, s->n_points[c], what, limit);
            return P2S_EINVAL;
        }
    }
    P2S_HIP_CHECK(hipSetDevice(s->device));
    // the per-call buffers are shared by all calls: work of another stream, and the last copy out of the pinned side, first
    if (s->used && s->last != st) P2S_HIP_CHECK(hipStreamSynchronize(s->last));
    if (s->used) P2S_HIP_CHECK(hipEventSynchronize(s->copied.get()));
    p2s_cloudset_s::Items &b = s->items;
    if (nq > b.cap) {
        drain_streams(s->streams, s->n_streams, s->many_streams, who);
        b = p2s_cloudset_s::Items();
        const int64_t cap = std::max<int64_t>(nq, 1024);
        if (!p2s_alloc_all(b.cloud_of_pin, cap, b.seg_pin, cap, b.cloud_of_dev, cap, b.seg_dev, cap)) {
            p2s_set_error("%s: allocation of the buffers of %lld items failed", who, (long long)cap);
            return P2S_ENOMEM;
        }
        b.cap = cap;
    }
    cloudset_note_stream(s, st);
    s->last = st;
    s->used = true;
    memcpy(b.cloud_of_pin.get(), cloud_of, (size_t)nq * 4);
    P2S_HIP_CHECK(hipMemcpyAsync(b.cloud_of_dev.get(), b.cloud_of_pin.get(), (size_t)nq * 4, hipMemcpyHostToDevice, st));
    P2S_HIP_CHECK(hipEventRecord(s->copied.get(), st));
    return P2S_OK;
}

}  // namespace

extern "C" {

int p2s_cloudset_create(const p2s_cloud_t *clouds, int n_clouds, int device, p2s_cloudset_t *out) {
    if (!clouds || n_clouds <= 0 || !out) {
        p2s_set_error("p2s_cloudset_create: bad argument (n_clouds=%d)", n_clouds);
        return P2S_EINVAL;
    }
    *out = nullptr;
    for (int i = 0; i < n_clouds; ++i) {
        if (!clouds[i]) {
            p2s_set_error("p2s_cloudset_create: cloud %d is NULL", i);
            return P2S_EINVAL;
        }
        if (clouds[i]->device != device) {
            p2s_set_error("p2s_cloudset_create: cloud %d lives on device %d, the set on device %d", i, clouds[i]->device, device);
            return P2S_EINVAL;
        }
    }
    if (p2s_device_count() <= device || device < 0 || device >= P2S_MAX_DEVICES) {
        p2s_set_error("p2s_cloudset_create: no HIP device %d", device);
        return P2S_ENODEVICE;
    }
    P2S_HIP_CHECK(hipSetDevice(device));
    p2s_cloudset_s *s = new p2s_cloudset_s();
    s->device = device;
    std::vector<CloudDev> table((size_t)n_clouds);
    s->n_points.resize((size_t)n_clouds);
    s->min_points = clouds[0]->d.n;
    for (int i = 0; i < n_clouds; ++i) {
        table[i] = clouds[i]->d;
        s->n_points[i] = clouds[i]->d.n;
        s->min_points = std::min(s->min_points, clouds[i]->d.n);
    }
    const int rc = [&]() -> int {
        if (!s->table.alloc(table.size())) {
            p2s_set_error("p2s_cloudset_create: allocation of the table of %d clouds failed", n_clouds);
            return P2S_ENOMEM;
        }
        P2S_HIP_CHECK(hipMemcpy(s->table.get(), table.data(), table.size() * sizeof(CloudDev), hipMemcpyHostToDevice));
        if (!s->copied.create(hipEventDisableTiming)) {
            p2s_set_error("p2s_cloudset_create: hipEventCreateWithFlags failed");
            return P2S_EHIP;
        }
        return P2S_OK;
    }();
    if (rc != P2S_OK) {
        p2s_cloudset_destroy(s);
        return rc;
    }
    *out = s;
    return P2S_OK;
}

int p2s_cloudset_destroy(p2s_cloudset_t s) {
    if (!s) return P2S_OK;
    (void)hipSetDevice(s->device);
    drain_streams(s->streams, s->n_streams, s->many_streams, "p2s_cloudset_destroy");
    delete s;
    return P2S_OK;
}

int p2s_cloudset_size(p2s_cloudset_t s, int32_t *n_clouds, int32_t *min_points) {
    if (!s) {
        p2s_set_error("p2s_cloudset_size: null handle");
        return P2S_EINVAL;
    }
    if (n_clouds) *n_clouds = (int32_t)s->n_points.size();
    if (min_points) *min_points = s->min_points;
    return P2S_OK;
}

int p2s_cloudset_knn_patch(p2s_cloudset_t s, const int32_t *cloud_of_host, const float *query_dev, int64_t nq, int k,
                           int32_t *ids_out_dev, float *patch_ps_out_dev, float *radius_out_dev, void *stream) {
    if (!s || nq < 0 || k < 1 || (nq > 0 && (!cloud_of_host || !query_dev))) {
        p2s_set_error("p2s_cloudset_knn_patch: bad argument");
        return P2S_EINVAL;
    }
    if (k > KNN_CAP - 128) {
        p2s_set_error("p2s_cloudset_knn_patch: k=%d exceeds the supported maximum %d", k, KNN_CAP - 128);
        return P2S_EINVAL;
    }
    if (nq == 0) return P2S_OK;
    hipStream_t st = (hipStream_t)stream;
    const int rc = cloudset_begin(s, "p2s_cloudset_knn_patch", "k", cloud_of_host, nq, k, st);
    if (rc) return rc;
    const unsigned grid = (unsigned)std::min<int64_t>(nq, 256 * 64);
    hipLaunchKernelGGL(p2s_knn_set_kernel, dim3(grid), dim3(64), 0, st, s->table.get(), s->items.cloud_of_dev.get(), query_dev, (long long)nq, k,
                       ids_out_dev, patch_ps_out_dev, radius_out_dev);
    P2S_LAUNCH_CHECK("p2s_knn_set_kernel");
    return P2S_OK;
}

int p2s_cloudset_subsample_uniform(p2s_rng_t r, p2s_cloudset_t s, const int32_t *cloud_of_host, int64_t nq, int n,
                                   int32_t *ids_out_dev, float *pts_out_dev, void *stream) {
    if (!r || !s || nq < 0 || n < 1 || (nq > 0 && !cloud_of_host) || (!ids_out_dev && pts_out_dev)) {
        p2s_set_error("p2s_cloudset_subsample_uniform: bad argument (pts_out_dev needs ids_out_dev)");
        return P2S_EINVAL;
    }
    if (r->device != s->device) {
        p2s_set_error("p2s_cloudset_subsample_uniform: the generator lives on device %d, the set on device %d", r->device, s->device);
        return P2S_EINVAL;
    }
    if (nq == 0) return P2S_OK;
    hipStream_t st = (hipStream_t)stream;
    int rc = cloudset_begin(s, "p2s_cloudset_subsample_uniform", "n", cloud_of_host, nq, n, st);
    if (rc) return rc;
    // runs of items whose clouds have the same size are one segment of the stream; a cloud of one point draws nothing
    P2sRandSeg *const segs = s->items.seg_pin.get();
    int64_t n_segs = 0;
    bool zeros = false;
    for (int64_t i = 0; i < nq; ++i) {
        const uint32_t rng = (uint32_t)(s->n_points[cloud_of_host[i]] - 1);
        if (rng == 0) {
            zeros = true;
            continue;
        }
        P2sRandSeg *last = n_segs ? &segs[n_segs - 1] : nullptr;
        if (last && last->rng == rng && last->out_begin + last->count == (long long)i * n) {
            last->count += n;
            continue;
        }
        uint32_t mask = rng;
        mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
        segs[n_segs++] = P2sRandSeg{rng, mask, (long long)i * n, (long long)n};
    }
    const long long target = (long long)nq * n;
    if ((rc = p2s_rng_session_close(r, st))) return rc;         // the state lags behind an open session
    if (zeros && ids_out_dev) P2S_HIP_CHECK(hipMemsetAsync(ids_out_dev, 0, (size_t)target * 4, st));
    if (n_segs) {
        P2S_HIP_CHECK(hipMemcpyAsync(s->items.seg_dev.get(), s->items.seg_pin.get(), (size_t)n_segs * sizeof(P2sRandSeg), hipMemcpyHostToDevice, st));
        P2S_HIP_CHECK(hipEventRecord(s->copied.get(), st));
        // one workgroup, pure latency: large requests keep a CU to themselves (see p2s_rng_serial_randint)
        constexpr int hog = 120 * 1024;
        (void)hipFuncSetAttribute((const void *)p2s_mt_randint_seg_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
        const int lds = target >= 100000 ? hog : 0;
        hipLaunchKernelGGL(p2s_mt_randint_seg_kernel, dim3(1), dim3(128), lds, st, r->state.get(), s->items.seg_dev.get(), (int)n_segs, ids_out_dev);
        P2S_LAUNCH_CHECK("p2s_mt_randint_seg_kernel");
    }
    if (pts_out_dev) {
        hipLaunchKernelGGL(p2s_gather_set_kernel, dim3((unsigned)((target + 255) / 256)), dim3(256), 0, st, s->table.get(),
                           s->items.cloud_of_dev.get(), ids_out_dev, target, n, pts_out_dev);
        P2S_LAUNCH_CHECK("p2s_gather_set_kernel");
    }
    return P2S_OK;
}

}  // extern "C"
