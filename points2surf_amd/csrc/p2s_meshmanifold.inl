// a triangle mesh made 2-manifold -- faces removed at the edges of more than two faces, vertices split where
// their faces do not form one fan.  Definition: include/p2s_hip.h (p2s_mesh_manifold); the project's own, not vcglib's.
// Included at the end of p2s_meshdist.hip, behind p2s_meshcomponents.inl: the edge table (EdgeTable, build_edges with fmn /
// fmx, rp_edge_slot, p2s_rp_edge_stats_kernel), the union-find primitives (uf_find, p2s_uf_compress_kernel, p2s_iota_kernel),
// mc_validate, mc_bad_mesh, SM_NO_KEY, wave_count, read_counters and the host scaffold are those files', used here and not copied.
//   p2s_mf_repeat_kernel      a face with a repeated index (refused)
//   p2s_mf_q_kernel           q = |u x w|^2 per face and the sort key ~bits(q): ascending keys are descending q
//   p2s_mf_rank_kernel        rank[f]: the position of face f in the stable sort (q descending, face id ascending)
//   p2s_mf_keeper_kernel      per edge of more than two faces the smallest rank (pass 0) and the smallest other rank (pass 1),
//                             integer atomicMin; a lane asks only when the slot's value read is still larger than its own
//   p2s_mf_mark_kernel        keep01[f] = 0 iff an edge of more than two faces has f and f is neither of its keepers
//   p2s_mf_compact_kernel     the kept faces in input order, with their input ids
//   p2s_mf_hook_kernel        union-find over the 3 F corners: per edge of exactly two faces f < g, the thread of f's edge unites
//                             the two corners at each end, the larger root hooked to the smaller by atomicMin
//   p2s_mf_vmin_kernel / p2s_mf_vclass_kernel      without the split: the class of a corner is the smallest corner of its vertex
//   p2s_mf_heads_kernel       (vertex id << 32 | root corner) for every class root, SM_NO_KEY elsewhere
//   p2s_mf_ids_kernel         position k of a sorted root key: the output id of its class, and the class's input vertex; the
//                             position behind the last root key is the count of the output vertices (one writer)
//   p2s_mf_split_stats_kernel vertices added, input vertices of more than one class
//   p2s_mf_faces_kernel       the faces over the output ids
//   p2s_mf_out_stats_kernel   the output's boundary edges, its two-face edges on an input edge of more than two faces, and the
//                             edges of more than two faces that the guarantee excludes (an internal error)
//   p2s_mf_write_verts_kernel the coordinates of the classes' input vertices, bit for bit
// The guarantee (rule f).  Rule b: an edge of more than two faces retains at most its two keepers, and removing faces makes
// no edge fuller.  Rule c: around an input vertex a take the faces at a as nodes and the two-face edges at a as links.  A face
// has exactly two edges at a, so its degree is at most 2, and the classes at a are paths or cycles.  A face on an edge {a, b}
// of more than two faces lacks that link: it is a path end, or alone.  A path has at most two ends, so of the faces on {a, b}
// at most two share a class at a -- the two ends of one path -- and only faces that share a class at a AND at b share the
// output edge: at most two (report [10] counts the edges where two do).  Every input two-face
// edge unites its corners at both ends, so it survives as a two-face edge of the output, every class stays connected through
// two-face edges, and the faces of an output vertex form one fan (a path) or one closed fan (a cycle).  A second call finds
// one class per vertex and nothing to remove: vertices and faces come back in their order, the same bytes.
// Determinism: ranks come from a stable radix sort of integer keys, keepers and roots are integer minima, output ids come from
// a radix sort of distinct keys, counts are integer sums.  No floating-point atomic; q is computed per face, contraction off.
// Termination: uf_find walks strictly decreasing parents.  A round of hooks that changes something turns at least one root
// into a non-root (the thread that raised `changed` saw two different roots and lowered the parent of the larger), and a
// corner never becomes a root again: after at most 3 F - 1 such rounds and one that changes nothing the host loop ends; more
// than 3 F + 1 rounds is an internal error.  The final root of a class is its smallest corner 3 f + j, so its smallest face.
// No thread waits for another.

namespace {

__global__ __launch_bounds__(256) void p2s_mf_repeat_kernel(const int *__restrict__ faces, long long F, int *__restrict__ err) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (a == b || b == c || a == c) *err = 1;
}

__global__ __launch_bounds__(256) void p2s_mf_q_kernel(const float *__restrict__ verts, const int *__restrict__ faces, long long F,
                                                       unsigned long long *__restrict__ qkey, int *__restrict__ fid) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    double u[3], w[3], n[3];
    for (int k = 0; k < 3; ++k) {
        const double a = verts[3 * (long long)faces[3 * f] + k];
        u[k] = (double)verts[3 * (long long)faces[3 * f + 1] + k] - a;
        w[k] = (double)verts[3 * (long long)faces[3 * f + 2] + k] - a;
    }
    cross3(u, w, n);
    const double q = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];       // finite and >= +0: its bit pattern orders as its value
    qkey[f] = ~__builtin_bit_cast(unsigned long long, q);
    fid[f] = (int)f;
}
__global__ __launch_bounds__(256) void p2s_mf_rank_kernel(const int *__restrict__ fsorted, long long F, int *__restrict__ rank) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < F) rank[fsorted[i]] = (int)i;
}
// k1, k2 [cap]: 0x7f7f7f7f initially.  A value read that is no larger than the lane's own can only have shrunk since
__global__ __launch_bounds__(256) void p2s_mf_keeper_kernel(const int *__restrict__ faces, long long F, EdgeTable t, const int *__restrict__ rank,
                                                            int *k1, int *k2, int pass) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= 3 * F) return;
    const long long f = i / 3;
    const int e = (int)(i - 3 * f);
    const unsigned h = rp_edge_slot(t, faces[3 * f + e], faces[3 * f + (e + 1) % 3]);
    if (t.cnt[2 * h] + t.cnt[2 * h + 1] <= 2) return;
    const int r = rank[f];
    if (pass == 0) {
        if (k1[h] > r) atomicMin(&k1[h], r);
    } else if (r != k1[h] && k2[h] > r) {
        atomicMin(&k2[h], r);
    }
}
__global__ __launch_bounds__(256) void p2s_mf_mark_kernel(const int *__restrict__ faces, long long F, EdgeTable t, const int *__restrict__ rank,
                                                          const int *__restrict__ k1, const int *__restrict__ k2, int *__restrict__ keep01) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int r = rank[f];
    int keep = 1;
    for (int e = 0; e < 3; ++e) {
        const unsigned h = rp_edge_slot(t, faces[3 * f + e], faces[3 * f + (e + 1) % 3]);
        if (t.cnt[2 * h] + t.cnt[2 * h + 1] > 2 && r != k1[h] && r != k2[h]) keep = 0;
    }
    keep01[f] = keep;
}
__global__ __launch_bounds__(256) void p2s_mf_compact_kernel(const int *__restrict__ faces, long long F, const int *__restrict__ keep01,
                                                             const int *__restrict__ kstart, int *__restrict__ wf, int *__restrict__ src) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F || !keep01[f]) return;
    const long long at = kstart[f];
    for (int j = 0; j < 3; ++j) wf[3 * at + j] = faces[3 * f + j];
    src[at] = (int)f;
}

// the corner of face g at vertex v (g has it)
__device__ __forceinline__ int mf_corner(const int *__restrict__ wf, int g, int v) {
    const long long g3 = 3 * (long long)g;
    return (int)g3 + (wf[g3] == v ? 0 : (wf[g3 + 1] == v ? 1 : 2));
}
__device__ __forceinline__ void mf_unite(int *parent, int x, int y, int *changed) {
    const int rx = uf_find(parent, x), ry = uf_find(parent, y);
    if (rx != ry) {
        atomicMin(&parent[max(rx, ry)], min(rx, ry));
        *changed = 1;
    }
}
__global__ __launch_bounds__(256) void p2s_mf_hook_kernel(const int *__restrict__ wf, long long F, EdgeTable t, const int *__restrict__ fmn,
                                                          const int *__restrict__ fmx, int *parent, int *changed) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= 3 * F) return;
    const long long f = i / 3;
    const int e = (int)(i - 3 * f), e1 = (e + 1) % 3;
    const int a = wf[3 * f + e], b = wf[3 * f + e1];
    const unsigned h = rp_edge_slot(t, a, b);
    if (t.cnt[2 * h] + t.cnt[2 * h + 1] != 2 || fmn[h] != (int)f) return;      // two different faces: no face has a repeated index
    const int g = fmx[h];
    mf_unite(parent, (int)(3 * f) + e, mf_corner(wf, g, a), changed);
    mf_unite(parent, (int)(3 * f) + e1, mf_corner(wf, g, b), changed);
}
// cmin [V]: 0x7f7f7f7f initially
__global__ __launch_bounds__(256) void p2s_mf_vmin_kernel(const int *__restrict__ wf, long long n, int *cmin) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c < n && cmin[wf[c]] > (int)c) atomicMin(&cmin[wf[c]], (int)c);
}
__global__ __launch_bounds__(256) void p2s_mf_vclass_kernel(const int *__restrict__ wf, long long n, const int *__restrict__ cmin,
                                                            int *__restrict__ parent) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c < n) parent[c] = cmin[wf[c]];
}

enum ManifoldCtr { MF_HEADS = 0, MF_ADDED, MF_SPLIT, MF_BOUNDARY_OUT, MF_REJOINED, MF_OVERFULL };

// parent is fully compressed: a class root is its smallest corner
__global__ __launch_bounds__(256) void p2s_mf_heads_kernel(const int *__restrict__ wf, long long n, const int *__restrict__ parent,
                                                           unsigned long long *__restrict__ key) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c < n) key[c] = parent[c] == (int)c ? (((unsigned long long)(unsigned)wf[c] << 32) | (unsigned)c) : SM_NO_KEY;
}
// the root keys come first in `sorted`; the position behind the last of them is their count (one writer: no atomic -- a count per
// wave on one address took longer than the hook rounds)
__global__ __launch_bounds__(256) void p2s_mf_ids_kernel(const unsigned long long *__restrict__ sorted, long long n, int *__restrict__ oid,
                                                         int *__restrict__ vsrc, unsigned long long *__restrict__ ctr) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= n || sorted[k] == SM_NO_KEY) return;
    oid[(unsigned)sorted[k]] = (int)k;
    vsrc[k] = (int)(sorted[k] >> 32);
    if (k + 1 == n || sorted[k + 1] == SM_NO_KEY) ctr[MF_HEADS] = (unsigned long long)(k + 1);
}
__global__ __launch_bounds__(256) void p2s_mf_split_stats_kernel(const unsigned long long *__restrict__ sorted, long long n, unsigned long long *ctr) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    unsigned long long added = 0, second = 0;
    if (k > 0 && k < n && sorted[k] != SM_NO_KEY) {
        const unsigned v = (unsigned)(sorted[k] >> 32);
        added = (unsigned)(sorted[k - 1] >> 32) == v;
        second = added && (k < 2 || (unsigned)(sorted[k - 2] >> 32) != v);
    }
    wave_count(ctr + MF_ADDED, added);
    wave_count(ctr + MF_SPLIT, second);
}
__global__ __launch_bounds__(256) void p2s_mf_faces_kernel(const int *__restrict__ parent, const int *__restrict__ oid, long long n,
                                                           int *__restrict__ fo) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c < n) fo[c] = oid[parent[c]];
}
// out: the edge table of the output faces, in: that of the input faces
__global__ __launch_bounds__(256) void p2s_mf_out_stats_kernel(EdgeTable out, const int *__restrict__ vsrc, EdgeTable in, unsigned long long *ctr) {
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    unsigned long long boundary = 0, rejoined = 0, overfull = 0;
    if (i <= out.mask && out.key[i] != EDGE_EMPTY) {
        const int c = out.cnt[2 * i] + out.cnt[2 * i + 1];
        boundary = c == 1;
        overfull = c > 2;
        if (c == 2) {
            const unsigned h = rp_edge_slot(in, vsrc[(int)(out.key[i] >> 32)], vsrc[(int)(unsigned)out.key[i]]);
            rejoined = in.cnt[2 * h] + in.cnt[2 * h + 1] > 2;
        }
    }
    wave_count(ctr + MF_BOUNDARY_OUT, boundary);
    wave_count(ctr + MF_REJOINED, rejoined);
    wave_count(ctr + MF_OVERFULL, overfull);
}
__global__ __launch_bounds__(256) void p2s_mf_write_verts_kernel(const float *__restrict__ verts, const int *__restrict__ vsrc, long long n,
                                                                 float *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < 3 * n) out[i] = verts[3 * (long long)vsrc[i / 3] + i % 3];
}

struct MfWs {                                    // what the input's sizes give
    int *ctl;
    unsigned long long *ctr;
    int *fmn, *fmx, *fid, *fsorted, *rank, *keep01, *kstart, *wf, *src, *cmin;
    unsigned long long *qkey, *qsorted;
    EdgeTable t;
    void *tmp;
    char *base;
    size_t bytes;
};
MfWs carve_mf(char *base, size_t V, size_t F, unsigned ecap, int mode, size_t tmp_bytes) {
    Carver c{base};
    const bool rm = mode & 1, split = mode & 2;
    MfWs w;
    w.ctl = c.take<int>(16);
    w.ctr = c.take<unsigned long long>(16);
    w.fmn = c.take<int>(ecap);
    w.fmx = c.take<int>(ecap);
    w.fid = c.take<int>(F, rm);
    w.fsorted = c.take<int>(F, rm);
    w.rank = c.take<int>(F, rm);
    w.keep01 = c.take<int>(F + 1, rm);
    w.kstart = c.take<int>(F + 1, rm);
    w.wf = c.take<int>(F * 3, rm);
    w.src = c.take<int>(F, rm);
    w.cmin = c.take<int>(V, !split);
    w.qkey = c.take<unsigned long long>(F, rm);
    w.qsorted = c.take<unsigned long long>(F, rm);
    w.t = carve_edges(c, ecap);
    w.tmp = c.take<char>(tmp_bytes, rm);
    return c.done(w);
}
struct MfOutWs {                                 // what the kept faces' count gives
    int *parent, *oid, *vsrc, *fo;
    unsigned long long *key, *sorted;
    EdgeTable t;
    void *tmp;
    char *base;
    size_t bytes;
};
MfOutWs carve_mf_out(char *base, size_t F1, unsigned ecap1, size_t tmp_bytes) {
    Carver c{base};
    MfOutWs w;
    w.parent = c.take<int>(F1 * 3);
    w.oid = c.take<int>(F1 * 3);
    w.vsrc = c.take<int>(F1 * 3);
    w.fo = c.take<int>(F1 * 3);
    w.key = c.take<unsigned long long>(F1 * 3);
    w.sorted = c.take<unsigned long long>(F1 * 3);
    w.t = carve_edges(c, ecap1);
    w.tmp = c.take<char>(tmp_bytes);
    return c.done(w);
}

}  // namespace

extern "C" int p2s_mesh_manifold(const float *verts_dev, int64_t n_verts, const int32_t *faces_dev, int64_t n_faces, int mode,
                                 float *verts_out_dev, int64_t cap_verts, int32_t *faces_out_dev, int64_t cap_faces,
                                 int32_t *vert_src_out_dev, int32_t *face_src_out_dev, int64_t *report_host, int device, void *stream) {
    static const char *const who = "p2s_mesh_manifold";
    const char *bad = mc_bad_mesh(verts_dev, n_verts, faces_dev, n_faces, report_host);
    if (!bad) {
        if (mode < 1 || mode > 3) bad = "mode is not 1, 2 or 3";
        else if (cap_verts < 0) bad = "cap_verts < 0";
        else if (cap_faces < 0) bad = "cap_faces < 0";
        else if (cap_verts > 0 && !verts_out_dev) bad = "verts_out_dev is NULL";
        else if (cap_faces > 0 && !faces_out_dev) bad = "faces_out_dev is NULL";
    }
    if (bad) {
        p2s_set_error("%s: bad argument (%s)", who, bad);
        return P2S_EINVAL;
    }
    if (int rc = select_device(who, device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const long long V = n_verts, F = n_faces;
    long long rep_out[16] = {};
    rep_out[0] = V | (F << 32);
    rep_out[7] = V;
    auto publish = [&]() {
        for (int k = 0; k < 16; ++k) report_host[k] = rep_out[k];
    };
    PoolScratch pool(device, s);
    int rc;

    // ---- a. validate; the edge table of the input
    const unsigned ecap = rp_table_cap(3 * F);
    size_t t1 = 0, t2 = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, t1, (int *)nullptr, (int *)nullptr, (int)(F + 1), nullptr);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, t2, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (int *)nullptr,
                                             (int *)nullptr, (int)F, 0, 64, nullptr);
    const size_t tmp_bytes = std::max(t1, t2) + 256;
    const MfWs W = pool.carve([&](char *b) { return carve_mf(b, (size_t)V, (size_t)F, ecap, mode, tmp_bytes); });
    if (!W.base) return dev_oom(who, s);
    if (V > 0 || F > 0) {
        if ((rc = mc_validate(who, verts_dev, V, faces_dev, F, W.ctl, s)) != P2S_OK) return rc;
    }
    if (F == 0) {                                                    // the empty result; every vertex is unreferenced
        publish();
        return P2S_OK;
    }
    int repeated = 0;
    DEV_CHECK(who, hipMemsetAsync(W.ctl, 0, 4, s));
    hipLaunchKernelGGL(p2s_mf_repeat_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, faces_dev, F, W.ctl);
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipMemcpyAsync(&repeated, W.ctl, 4, hipMemcpyDeviceToHost, s));
    DEV_CHECK(who, hipStreamSynchronize(s));
    if (repeated) {
        p2s_set_error("%s: a face with a repeated index", who);
        return P2S_EINVAL;
    }
    const bool rm = mode & 1, split = mode & 2;
    unsigned long long hc[8] = {};
    DEV_CHECK(who, hipMemsetAsync(W.ctr, 0, MESH_COUNTERS, s));
    if ((rc = build_edges(who, faces_dev, F, W.t, rm ? nullptr : W.fmn, rm ? nullptr : W.fmx, s)) != P2S_OK) return rc;
    hipLaunchKernelGGL(p2s_rp_edge_stats_kernel, dim3(blocks((long long)ecap, 256)), dim3(256), 0, s, W.t, W.ctr);
    if ((rc = read_counters(who, W.ctr, hc, -1, "", s)) != P2S_OK) return rc;
    rep_out[8] = (long long)hc[0];
    rep_out[3] = (long long)hc[1];

    // ---- b. the faces that no edge of more than two faces rejects
    const int *wf = faces_dev;
    long long F1 = F;
    if (rm) {
        int *k1 = W.fmn, *k2 = W.fmx;                                // the two keepers' ranks; free again before c fills fmn, fmx
        hipLaunchKernelGGL(p2s_mf_q_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, verts_dev, faces_dev, F, W.qkey, W.fid);
        DEV_CHECK(who, hipGetLastError());
        size_t tb = tmp_bytes;
        DEV_CHECK(who, hipcub::DeviceRadixSort::SortPairs(W.tmp, tb, W.qkey, W.qsorted, W.fid, W.fsorted, (int)F, 0, 64, s));
        DEV_CHECK(who, hipMemsetAsync(k1, 0x7f, (size_t)ecap * 4, s));
        DEV_CHECK(who, hipMemsetAsync(k2, 0x7f, (size_t)ecap * 4, s));
        DEV_CHECK(who, hipMemsetAsync(W.keep01 + F, 0, 4, s));
        hipLaunchKernelGGL(p2s_mf_rank_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, W.fsorted, F, W.rank);
        for (int pass = 0; pass < 2; ++pass)
            hipLaunchKernelGGL(p2s_mf_keeper_kernel, dim3(blocks(3 * F, 256)), dim3(256), 0, s, faces_dev, F, W.t, W.rank, k1, k2, pass);
        hipLaunchKernelGGL(p2s_mf_mark_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, faces_dev, F, W.t, W.rank, k1, k2, W.keep01);
        DEV_CHECK(who, hipGetLastError());
        tb = tmp_bytes;
        DEV_CHECK(who, hipcub::DeviceScan::ExclusiveSum(W.tmp, tb, W.keep01, W.kstart, (int)(F + 1), s));
        hipLaunchKernelGGL(p2s_mf_compact_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, faces_dev, F, W.keep01, W.kstart, W.wf, W.src);
        DEV_CHECK(who, hipGetLastError());
        int hF = 0;
        DEV_CHECK(who, hipMemcpyAsync(&hF, W.kstart + F, 4, hipMemcpyDeviceToHost, s));
        DEV_CHECK(who, hipStreamSynchronize(s));
        wf = W.wf;
        F1 = hF;
    }
    rep_out[2] = F1;
    rep_out[4] = F - F1;

    // ---- c. the classes of the 3 F1 corners
    const long long n = 3 * F1;
    const unsigned ecap1 = rp_table_cap(n);
    size_t t3 = 0;
    (void)hipcub::DeviceRadixSort::SortKeys(nullptr, t3, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (int)n, 0, 64, nullptr);
    const MfOutWs O = pool.carve([&](char *b) { return carve_mf_out(b, (size_t)F1, ecap1, t3 + 256); });
    if (!O.base) return dev_oom(who, s);
    if (split) {
        EdgeTable t = W.t;                                           // the table whose two-face edges unite: of the kept faces
        if (rm) {
            t = O.t;
            if ((rc = build_edges(who, wf, F1, t, W.fmn, W.fmx, s)) != P2S_OK) return rc;
        }
        hipLaunchKernelGGL(p2s_iota_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, O.parent, n);
        rc = until_unchanged(who, "the classes of the corners", n + 1, W.ctl, s, [&](long long) {      // the cap: see the head of this file
            hipLaunchKernelGGL(p2s_mf_hook_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, wf, F1, t, W.fmn, W.fmx, O.parent, W.ctl);
            hipLaunchKernelGGL(p2s_uf_compress_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, O.parent, n);
        }, &rep_out[11]);
        if (rc != P2S_OK) return rc;
    } else {
        DEV_CHECK(who, hipMemsetAsync(W.cmin, 0x7f, (size_t)V * 4, s));
        hipLaunchKernelGGL(p2s_mf_vmin_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, wf, n, W.cmin);
        hipLaunchKernelGGL(p2s_mf_vclass_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, wf, n, W.cmin, O.parent);
    }

    // ---- d, e. output ids in the order (input vertex, smallest face of the class); the counts, before the capacity decides
    int end_bit = 33;                                                // 2^(end_bit - 32) - 1 >= V > every vertex id: SM_NO_KEY stays last
    while ((1ll << (end_bit - 32)) <= V) ++end_bit;
    DEV_CHECK(who, hipMemsetAsync(W.ctr, 0, MESH_COUNTERS, s));
    hipLaunchKernelGGL(p2s_mf_heads_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, wf, n, O.parent, O.key);
    DEV_CHECK(who, hipGetLastError());
    size_t tb = t3 + 256;
    DEV_CHECK(who, hipcub::DeviceRadixSort::SortKeys(O.tmp, tb, O.key, O.sorted, (int)n, 0, end_bit, s));
    hipLaunchKernelGGL(p2s_mf_ids_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, O.sorted, n, O.oid, O.vsrc, W.ctr);
    hipLaunchKernelGGL(p2s_mf_split_stats_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, O.sorted, n, W.ctr);
    hipLaunchKernelGGL(p2s_mf_faces_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, O.parent, O.oid, n, O.fo);
    if ((rc = build_edges(who, O.fo, F1, O.t, nullptr, nullptr, s)) != P2S_OK) return rc;
    hipLaunchKernelGGL(p2s_mf_out_stats_kernel, dim3(blocks((long long)ecap1, 256)), dim3(256), 0, s, O.t, O.vsrc, W.t, W.ctr);
    if ((rc = read_counters(who, W.ctr, hc, MF_OVERFULL, "internal error (an output edge of more than two faces)", s)) != P2S_OK) return rc;
    const long long V1 = (long long)hc[MF_HEADS], referenced = V1 - (long long)hc[MF_ADDED];
    rep_out[1] = V1;
    rep_out[5] = (long long)hc[MF_SPLIT];
    rep_out[6] = (long long)hc[MF_ADDED];
    rep_out[7] = V - referenced;
    rep_out[9] = (long long)hc[MF_BOUNDARY_OUT];
    rep_out[10] = (long long)hc[MF_REJOINED];
    publish();
    if (cap_verts < V1 || cap_faces < F1) {
        p2s_set_error("%s: output buffers too small (%lld vertices and %lld faces needed, cap_verts = %lld and cap_faces = %lld given)", who, V1,
                      F1, (long long)cap_verts, (long long)cap_faces);
        return P2S_EINVAL;
    }
    hipLaunchKernelGGL(p2s_mf_write_verts_kernel, dim3(blocks(3 * V1, 256)), dim3(256), 0, s, verts_dev, O.vsrc, V1, verts_out_dev);
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipMemcpyAsync(faces_out_dev, O.fo, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    if (vert_src_out_dev) DEV_CHECK(who, hipMemcpyAsync(vert_src_out_dev, O.vsrc, (size_t)V1 * 4, hipMemcpyDeviceToDevice, s));
    if (face_src_out_dev) {
        if (rm) DEV_CHECK(who, hipMemcpyAsync(face_src_out_dev, W.src, (size_t)F1 * 4, hipMemcpyDeviceToDevice, s));
        else hipLaunchKernelGGL(p2s_iota_kernel, dim3(blocks(F1, 256)), dim3(256), 0, s, face_src_out_dev, F1);
        DEV_CHECK(who, hipGetLastError());
    }
    DEV_CHECK(who, hipStreamSynchronize(s));
    return P2S_OK;
}
