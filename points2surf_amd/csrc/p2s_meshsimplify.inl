// simplification of a triangle mesh by quadric vertex clustering (Lindstrom 2000).  Definitions:
// include/p2s_hip.h (p2s_mesh_simplify).  Included at the end of p2s_meshdist.hip, behind p2s_meshrepair.inl: the
// validation with the ordered-integer bounding box, the edge table (build_edges, p2s_rp_edge_stats_kernel), the face hash
// of the repair (p2s_rp_face_weld_kernel / p2s_rp_face_insert_kernel / p2s_rp_face_keep_kernel with the cell's smallest
// vertex id in the place of the weld's representative), DEGENERATE_REL and the host scaffold are those files', used here
// and not copied.  The grid is that of p2s_prepare_voxel_thin (pp_cell of p2s_prepare.hip, another translation unit):
// sm_cell restates its three lines of arithmetic, and tests/simplify_model.py holds both to the same numpy expression.
//   p2s_sm_count_kernel        a probe of the search: the faces whose corners lie in three different cells (nothing else)
//   p2s_sm_cell_insert_kernel  occupied cells in an open-addressing table of linear cell ids; the smallest vertex id per cell
//   p2s_sm_rep_kernel          per vertex the smallest vertex id of its cell
//   p2s_sm_used_kernel         cells that hold a corner of a surviving face
//   p2s_sm_vkeys_kernel        vert_map; (output id << 32 | vertex id) per vertex of such a cell
//   p2s_sm_fkeys_kernel        degenerate faces; (output id << 32 | face id) once per cell that a face touches
//   p2s_sm_seg_kernel          where an output id's run begins and ends in the sorted keys
//   p2s_sm_place_kernel        one thread per output vertex: the mean, the quadric, the solve, the fallback
//   p2s_sm_faces_kernel        the surviving faces in input order, mapped
//   p2s_iota_kernel            (p2s_devprim.inl) the identity maps of a copied mesh
// Determinism: the tables hold the smallest id of a class (atomicMin), counters are integer sums, positions come from
// exclusive scans (hipcub), and a cell's float64 sums run over keys that a radix sort put in ascending id.  One thread
// walks a cell's list: a few entries at useful R, 10^5 at R = 2 -- slow there, and finite.
#include <hipcub/hipcub.hpp>

namespace {

struct SmGrid {
    double lo[3];
    double scale;      // R / ext (0 for ext = 0)
    double cell;       // ext / R
    int R;
};
__device__ __forceinline__ int sm_cell(const SmGrid &g, const float *__restrict__ p, int *idx) {
    int lin = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double rel = (double)p[a] - g.lo[a];
        const int ia = (int)fmin(floor(rel * g.scale), (double)(g.R - 1));
        if (idx) idx[a] = ia;
        lin = lin * g.R + ia;
    }
    return lin;                                  // < 2^30
}

__global__ __launch_bounds__(256) void p2s_sm_count_kernel(const float *__restrict__ verts, const int *__restrict__ faces, long long F, SmGrid g,
                                                           unsigned long long *__restrict__ surviving) {
    __shared__ int ws[4];
    int n = 0;                                   // a fixed grid strides over the faces: one atomic per workgroup
    for (long long f = (long long)blockIdx.x * 256 + threadIdx.x; f < F; f += (long long)gridDim.x * 256) {
        const int a = sm_cell(g, verts + 3 * (long long)faces[3 * f], nullptr), b = sm_cell(g, verts + 3 * (long long)faces[3 * f + 1], nullptr),
                  c = sm_cell(g, verts + 3 * (long long)faces[3 * f + 2], nullptr);
        n += a != b && b != c && c != a;
    }
    for (int d = 32; d > 0; d >>= 1) n += __shfl_xor(n, d);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0 && ws[0] + ws[1] + ws[2] + ws[3]) atomicAdd(surviving, (unsigned long long)(ws[0] + ws[1] + ws[2] + ws[3]));
}

// ckey [mask + 1] (-1 initially), linear probing, load factor <= 1/2; cmin: the smallest vertex id of the slot's cell
__global__ __launch_bounds__(256) void p2s_sm_cell_insert_kernel(const float *__restrict__ verts, long long V, SmGrid g, int *ckey, unsigned mask,
                                                                 int *cmin, int *__restrict__ vslot, unsigned long long *__restrict__ occupied) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    int fresh = 0;
    if (v < V) {
        const int cell = sm_cell(g, verts + 3 * v, nullptr);
        unsigned h = edge_hash((unsigned long long)(unsigned)cell) & mask;
        for (;;) {
            const int prev = atomicCAS(&ckey[h], -1, cell);
            if (prev == -1) fresh = 1;
            if (prev == -1 || prev == cell) break;
            h = (h + 1) & mask;
        }
        atomicMin(&cmin[h], (int)v);
        vslot[v] = (int)h;
    }
    const unsigned long long m = __ballot(fresh);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(occupied, (unsigned long long)__popcll(m));
}
__global__ __launch_bounds__(256) void p2s_sm_rep_kernel(long long V, const int *__restrict__ vslot, const int *__restrict__ cmin,
                                                         int *__restrict__ rep) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v < V) rep[v] = cmin[vslot[v]];
}
// wfa: the faces in cell representatives (p2s_rp_face_weld_kernel); keep: 1 where the three differ
__global__ __launch_bounds__(256) void p2s_sm_used_kernel(const int *__restrict__ wfa, long long F, const int *__restrict__ keep,
                                                          int *__restrict__ used) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F || !keep[f]) return;
    for (int k = 0; k < 3; ++k) used[wfa[3 * f + k]] = 1;
}
constexpr unsigned long long SM_NO_KEY = ~0ull;      // sorts behind every key
__global__ __launch_bounds__(256) void p2s_sm_vkeys_kernel(long long V, const int *__restrict__ rep, const int *__restrict__ used,
                                                           const int *__restrict__ vstart, int *__restrict__ vmap,
                                                           unsigned long long *__restrict__ vkey) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const int r = rep[v], o = used[r] ? vstart[r] : -1;
    vmap[v] = o;
    vkey[v] = o < 0 ? SM_NO_KEY : (((unsigned long long)(unsigned)o << 32) | (unsigned)v);
}
// fkey [3 F] (NULL: only the count; degenerate NULL: only the keys): corner j of a face emits the face for its cell unless an earlier corner did
__global__ __launch_bounds__(256) void p2s_sm_fkeys_kernel(const float *__restrict__ verts, const int *__restrict__ faces, long long F,
                                                           const int *__restrict__ rep, const int *__restrict__ used,
                                                           const int *__restrict__ vstart, unsigned long long *__restrict__ fkey,
                                                           unsigned long long *__restrict__ degenerate) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    int deg = 0;
    if (f < F) {
        double P[9], ab[3], ac[3], n[3];
        int c[3];
        for (int j = 0; j < 3; ++j) {
            const int v = faces[3 * f + j];
            c[j] = rep[v];
            for (int k = 0; k < 3; ++k) P[3 * j + k] = verts[3 * (long long)v + k];
        }
        for (int k = 0; k < 3; ++k) {
            ab[k] = P[3 + k] - P[k];
            ac[k] = P[6 + k] - P[k];
        }
        cross3(ab, ac, n);
        deg = !(dot3(n, n) > DEGENERATE_REL * (dot3(ab, ab) * dot3(ac, ac)));
        if (fkey) {
            for (int j = 0; j < 3; ++j) {
                const bool first = (j < 1 || c[j] != c[0]) && (j < 2 || c[j] != c[1]);
                const bool emit = !deg && first && used[c[j]];
                fkey[3 * f + j] = emit ? (((unsigned long long)(unsigned)vstart[c[j]] << 32) | (unsigned)f) : SM_NO_KEY;
            }
        }
    }
    const unsigned long long m = __ballot(deg);
    if (degenerate && (threadIdx.x & 63) == 0 && m) atomicAdd(degenerate, (unsigned long long)__popcll(m));
}
// seg [2][n_out] (zeroed: an output id without a key has the empty run)
__global__ __launch_bounds__(256) void p2s_sm_seg_kernel(const unsigned long long *__restrict__ key, long long n, long long n_out,
                                                         int *__restrict__ seg) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || key[i] == SM_NO_KEY) return;
    const unsigned o = (unsigned)(key[i] >> 32);
    if (i == 0 || (unsigned)(key[i - 1] >> 32) != o) seg[o] = (int)i;
    if (i == n - 1 || (unsigned)(key[i + 1] >> 32) != o) seg[n_out + o] = (int)(i + 1);
}

// ctr[0] placed by the quadric, ctr[1] tr(A) = 0, ctr[2] fell back to the mean
__global__ __launch_bounds__(256) void p2s_sm_place_kernel(const float *__restrict__ verts, const int *__restrict__ faces, SmGrid g, long long n_out,
                                                           const unsigned long long *__restrict__ vkey, const int *__restrict__ vseg,
                                                           const unsigned long long *__restrict__ fkey, const int *__restrict__ fseg,
                                                           int placement, double epsilon, float *__restrict__ out,
                                                           unsigned long long *__restrict__ ctr) {
    const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
    int what = -1;
    if (o < n_out) {
        const int v0 = vseg[o], v1 = vseg[n_out + o];                // never empty: the cell's smallest vertex comes first
        int idx[3];
        (void)sm_cell(g, verts + 3 * (long long)(unsigned)vkey[v0], idx);
        double c[3], m[3] = {0.0, 0.0, 0.0}, x[3];
        for (int k = 0; k < 3; ++k) c[k] = g.lo[k] + ((double)idx[k] + 0.5) * g.cell;
        for (int i = v0; i < v1; ++i) {
            const float *p = verts + 3 * (long long)(unsigned)vkey[i];
            for (int k = 0; k < 3; ++k) m[k] += (double)p[k] - c[k];
        }
        for (int k = 0; k < 3; ++k) x[k] = m[k] = m[k] / (double)(v1 - v0);
        if (placement == 1) {
            double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, r[3] = {0.0, 0.0, 0.0};       // xx xy xz yy yz zz
            for (int i = fseg[o]; i < fseg[n_out + o]; ++i) {
                const long long f = (long long)(unsigned)fkey[i];
                double P[9], ab[3], ac[3], n[3];
                for (int j = 0; j < 3; ++j)
                    for (int k = 0; k < 3; ++k) P[3 * j + k] = (double)verts[3 * (long long)faces[3 * f + j] + k] - c[k];
                for (int k = 0; k < 3; ++k) {
                    ab[k] = P[3 + k] - P[k];
                    ac[k] = P[6 + k] - P[k];
                }
                cross3(ab, ac, n);
                const double d = -dot3(n, P);
                A[0] += n[0] * n[0];
                A[1] += n[0] * n[1];
                A[2] += n[0] * n[2];
                A[3] += n[1] * n[1];
                A[4] += n[1] * n[2];
                A[5] += n[2] * n[2];
                for (int k = 0; k < 3; ++k) r[k] += d * n[k];
            }
            const double tr = (A[0] + A[3]) + A[5];
            if (tr == 0.0) {
                what = 1;
            } else {
                const double lam = epsilon * tr;
                const double b0 = ((A[0] * m[0] + A[1] * m[1]) + A[2] * m[2]) + r[0], b1 = ((A[1] * m[0] + A[3] * m[1]) + A[4] * m[2]) + r[1],
                             b2 = ((A[2] * m[0] + A[4] * m[1]) + A[5] * m[2]) + r[2];
                // Cholesky of A + lam I (positive definite: A is a sum of n n^T and lam > 0)
                const double l00 = sqrt(A[0] + lam), l10 = A[1] / l00, l20 = A[2] / l00;
                const double l11 = sqrt((A[3] + lam) - l10 * l10), l21 = (A[4] - l20 * l10) / l11;
                const double l22 = sqrt(((A[5] + lam) - l20 * l20) - l21 * l21);
                const double z0 = b0 / l00, z1 = (b1 - l10 * z0) / l11, z2 = ((b2 - l20 * z0) - l21 * z1) / l22;
                const double y2 = z2 / l22, y1 = (z1 - l21 * y2) / l11, y0 = ((z0 - l10 * y1) - l20 * y2) / l00;
                const double q[3] = {m[0] - y0, m[1] - y1, m[2] - y2};
                const double big = fmax(fmax(fabs(q[0]), fabs(q[1])), fabs(q[2]));
                if (big > g.cell || !(big == big)) {
                    what = 2;
                } else {
                    what = 0;
                    for (int k = 0; k < 3; ++k) x[k] = q[k];
                }
            }
        }
        for (int k = 0; k < 3; ++k) out[3 * o + k] = (float)(c[k] + x[k]);
    }
    for (int w = 0; w < 3; ++w) {
        const unsigned long long b = __ballot(what == w);
        if ((threadIdx.x & 63) == 0 && b) atomicAdd(&ctr[w], (unsigned long long)__popcll(b));
    }
}

__global__ __launch_bounds__(256) void p2s_sm_faces_kernel(const int *__restrict__ wfa, long long F, const int *__restrict__ keep,
                                                           const int *__restrict__ kstart, const int *__restrict__ vstart,
                                                           int *__restrict__ wf, int *__restrict__ src) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F || !keep[f]) return;
    const long long at = kstart[f];
    for (int k = 0; k < 3; ++k) wf[3 * at + k] = vstart[wfa[3 * f + k]];
    src[at] = (int)f;
}

enum SimplifyCtr {
    SM_BOUNDARY = 0, SM_NONMANIFOLD, SM_INCONSISTENT,                                        // p2s_rp_edge_stats_kernel
    SM_SURVIVING = 0,                                                                        // a probe
    SM_OCCUPIED = 0, SM_COLLAPSED, SM_DUPLICATE, SM_DEGENERATE,                              // b .. d
    SM_QUADRIC = 3, SM_TRACE0, SM_FALLBACK                                                   // e, behind the output's edges
};

struct SmEdgeWs {                                // report [13], then [12] on the same block
    int *ctl;
    unsigned long long *ctr;
    EdgeTable t;
    char *base;
    size_t bytes;
};
SmEdgeWs carve_sm_edges(char *base, unsigned ecap) {
    Carver c{base};
    SmEdgeWs w;
    w.ctl = c.take<int>(16);
    w.ctr = c.take<unsigned long long>(8);
    w.t = carve_edges(c, ecap);
    return c.done(w);
}
struct SmClusterWs {                             // b .. d, f
    int *ckey, *cmin, *vslot, *rep, *used, *vstart, *vmap, *fslot, *wfa, *keep, *kstart;
    void *tmp;
    char *base;
    size_t bytes;
};
SmClusterWs carve_sm_cluster(char *base, size_t V, size_t F, unsigned vcap, unsigned fcap, size_t tmp_bytes) {
    Carver c{base};
    SmClusterWs w;
    w.ckey = c.take<int>(vcap);
    w.cmin = c.take<int>(vcap);
    w.vslot = c.take<int>(V);
    w.rep = c.take<int>(V);
    w.used = c.take<int>(V + 1);
    w.vstart = c.take<int>(V + 1);
    w.vmap = c.take<int>(V);
    w.fslot = c.take<int>(fcap);
    w.wfa = c.take<int>(F * 3);
    w.keep = c.take<int>(F + 1);
    w.kstart = c.take<int>(F + 1);
    w.tmp = c.take<char>(tmp_bytes);
    return c.done(w);
}
struct SmPlaceWs {                               // e, and the outputs until the capacity is known to suffice
    unsigned long long *vkey, *vsorted, *fkey, *fsorted;
    int *vseg, *fseg, *wf, *src;
    float *vout;
    void *tmp;
    char *base;
    size_t bytes;
};
SmPlaceWs carve_sm_place(char *base, size_t V, size_t F, size_t V1, size_t F0, bool quadric, size_t tmp_bytes) {
    Carver c{base};
    SmPlaceWs w;
    w.vkey = c.take<unsigned long long>(V);
    w.vsorted = c.take<unsigned long long>(V);
    w.fkey = c.take<unsigned long long>(F * 3, quadric);
    w.fsorted = c.take<unsigned long long>(F * 3, quadric);
    w.vseg = c.take<int>(V1 * 2);
    w.fseg = c.take<int>(V1 * 2);
    w.wf = c.take<int>(F0 * 3);
    w.src = c.take<int>(F0);
    w.vout = c.take<float>(V1 * 3);
    w.tmp = c.take<char>(tmp_bytes);
    return c.done(w);
}

// boundary edges | edges of more than two faces << 32 of `faces`, on the table `t`
int sm_edge_word(const char *who, const int *faces, long long F, EdgeTable t, unsigned long long *ctr, unsigned long long *hc, long long *word,
                 hipStream_t s) {
    int rc;
    if ((rc = build_edges(who, faces, F, t, nullptr, nullptr, s)) != P2S_OK) return rc;
    hipLaunchKernelGGL(p2s_rp_edge_stats_kernel, dim3(blocks((long long)t.mask + 1, 256)), dim3(256), 0, s, t, ctr + SM_BOUNDARY);
    if ((rc = read_counters(who, ctr, hc, -1, nullptr, s)) != P2S_OK) return rc;
    *word = (long long)hc[SM_BOUNDARY] | ((long long)hc[SM_NONMANIFOLD] << 32);
    return P2S_OK;
}

}  // namespace

extern "C" int p2s_mesh_simplify(const float *verts_dev, int64_t n_verts, const int32_t *faces_dev, int64_t n_faces, int resolution,
                                 int64_t max_faces, int placement, double epsilon, float *verts_out_dev, int64_t cap_verts,
                                 int32_t *faces_out_dev, int32_t *face_src_out_dev, int64_t cap_faces, int32_t *vert_map_out_dev,
                                 int64_t *report_host, int device, void *stream) {
    static const char *const who = "p2s_mesh_simplify";
    const char *bad = nullptr;
    if (!report_host) bad = "report_host is NULL";
    else if (n_verts < 0 || n_verts > (1ll << 27)) bad = "n_verts outside 0 .. 2^27";
    else if (n_faces < 0 || n_faces > (1ll << 27)) bad = "n_faces outside 0 .. 2^27";
    else if (cap_verts < 0) bad = "cap_verts < 0";
    else if (cap_faces < 0) bad = "cap_faces < 0";
    else if (resolution < 0 || resolution > 1024) bad = "resolution outside 0 .. 1024";
    else if (resolution == 0 && max_faces < 0) bad = "max_faces < 0 with resolution = 0";
    else if (placement != 0 && placement != 1) bad = "placement is neither 0 (mean) nor 1 (quadric)";
    else if (!(epsilon >= 1e-6 && epsilon <= 1.0)) bad = "epsilon outside [1e-6, 1]";
    else if (n_verts > 0 && !verts_dev) bad = "verts_dev is NULL";
    else if (n_faces > 0 && !faces_dev) bad = "faces_dev is NULL";
    else if (cap_verts > 0 && !verts_out_dev) bad = "verts_out_dev is NULL";
    else if (cap_faces > 0 && !faces_out_dev) bad = "faces_out_dev is NULL";
    if (bad) {
        p2s_set_error("%s: bad argument (%s)", who, bad);
        return P2S_EINVAL;
    }
    if (int rc = select_device(who, device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const long long V = n_verts, F = n_faces;
    long long rep_out[16] = {};
    rep_out[0] = V | (F << 32);
    rep_out[3] = resolution;
    auto publish = [&]() {
        for (int k = 0; k < 16; ++k) report_host[k] = rep_out[k];
    };
    auto too_small = [&](long long v_need, long long f_need) {
        p2s_set_error("%s: output buffers too small (%lld vertices and %lld faces needed, cap_verts = %lld and cap_faces = %lld given)", who,
                      v_need, f_need, (long long)cap_verts, (long long)cap_faces);
        return P2S_EINVAL;
    };
    PoolScratch pool(device, s);
    int rc;

    // ---- a. validate; the edges of the input
    const unsigned ecap = rp_table_cap(3 * F);
    const SmEdgeWs E = pool.carve([&](char *b) { return carve_sm_edges(b, ecap); });
    if (!E.base) return dev_oom(who, s);
    int *ctl = E.ctl;
    unsigned long long *ctr = E.ctr, hc[8] = {};
    float box[6] = {};
    if (V > 0 || F > 0) {
        if ((rc = mesh_validate(who, verts_dev, V, faces_dev, F, ctl, box, s)) != P2S_OK) return rc;
    }
    if (F == 0) {                                                    // the empty result
        if (vert_map_out_dev && V > 0) {
            DEV_CHECK(who, hipMemsetAsync(vert_map_out_dev, 0xff, (size_t)V * 4, s));
            DEV_CHECK(who, hipStreamSynchronize(s));
        }
        publish();
        return P2S_OK;
    }
    DEV_CHECK(who, hipMemsetAsync(ctr, 0, MESH_COUNTERS, s));
    if ((rc = sm_edge_word(who, faces_dev, F, E.t, ctr, hc, &rep_out[13], s)) != P2S_OK) return rc;

    // ---- b. the grid
    double ext = 0.0;
    for (int a = 0; a < 3; ++a) ext = std::max(ext, (double)box[3 + a] - (double)box[a]);
    auto grid = [&](int R) {
        SmGrid g;
        for (int a = 0; a < 3; ++a) g.lo[a] = (double)box[a];
        g.scale = ext > 0.0 ? (double)R / ext : 0.0;
        g.cell = ext / (double)R;
        g.R = R;
        return g;
    };
    int R = resolution;
    if (R == 0) {
        if (F <= max_faces) {                                        // nothing to do: the input, bit for bit
            rep_out[1] = V;
            rep_out[2] = F;
            rep_out[12] = rep_out[13];
            publish();
            if (cap_verts < V || cap_faces < F) return too_small(V, F);
            DEV_CHECK(who, hipMemcpyAsync(verts_out_dev, verts_dev, (size_t)V * 12, hipMemcpyDeviceToDevice, s));
            DEV_CHECK(who, hipMemcpyAsync(faces_out_dev, faces_dev, (size_t)F * 12, hipMemcpyDeviceToDevice, s));
            if (face_src_out_dev) hipLaunchKernelGGL(p2s_iota_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, face_src_out_dev, F);
            if (vert_map_out_dev) hipLaunchKernelGGL(p2s_iota_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, vert_map_out_dev, V);
            DEV_CHECK(who, hipGetLastError());
            DEV_CHECK(who, hipStreamSynchronize(s));
            return P2S_OK;
        }
        // surviving(R) is not monotone over grids that do not nest: this search IS the definition of R
        int lo = 1, hi = 1024;
        while (lo < hi) {
            const int mid = (lo + hi + 1) / 2;
            DEV_CHECK(who, hipMemsetAsync(ctr, 0, MESH_COUNTERS, s));
            hipLaunchKernelGGL(p2s_sm_count_kernel, dim3(std::min(blocks(F, 256), 2048u)), dim3(256), 0, s, verts_dev, faces_dev, F, grid(mid), ctr + SM_SURVIVING);
            if ((rc = read_counters(who, ctr, hc, -1, nullptr, s)) != P2S_OK) return rc;
            ++rep_out[11];
            if ((long long)hc[SM_SURVIVING] <= max_faces) lo = mid;
            else hi = mid - 1;
        }
        R = lo;
    }
    rep_out[3] = R;
    const SmGrid g = grid(R);

    // ---- c, d. cells, surviving faces, duplicates (the face hash of the repair over the cells' smallest vertex ids)
    const unsigned vcap = rp_table_cap(V), fcap = rp_table_cap(F);
    size_t t1 = 0, t2 = 0, t3 = 0, t4 = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, t1, (int *)nullptr, (int *)nullptr, (int)(V + 1), nullptr);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, t2, (int *)nullptr, (int *)nullptr, (int)(F + 1), nullptr);
    (void)hipcub::DeviceRadixSort::SortKeys(nullptr, t3, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (int)V, 0, 64, nullptr);
    (void)hipcub::DeviceRadixSort::SortKeys(nullptr, t4, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (int)(3 * F), 0, 64, nullptr);
    const size_t scan_tmp = std::max(t1, t2) + 256, sort_tmp = std::max(t3, t4) + 256;
    const SmClusterWs C = pool.carve([&](char *b) { return carve_sm_cluster(b, (size_t)V, (size_t)F, vcap, fcap, scan_tmp); });
    if (!C.base) return dev_oom(who, s);
    DEV_CHECK(who, hipMemsetAsync(C.ckey, 0xff, (size_t)vcap * 4, s));
    DEV_CHECK(who, hipMemsetAsync(C.cmin, 0x7f, (size_t)vcap * 4, s));
    DEV_CHECK(who, hipMemsetAsync(C.fslot, 0xff, (size_t)fcap * 4, s));
    DEV_CHECK(who, hipMemsetAsync(C.used, 0, (size_t)(V + 1) * 4, s));
    DEV_CHECK(who, hipMemsetAsync(C.keep + F, 0, 4, s));
    DEV_CHECK(who, hipMemsetAsync(ctr, 0, MESH_COUNTERS, s));
    hipLaunchKernelGGL(p2s_sm_cell_insert_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, verts_dev, V, g, C.ckey, vcap - 1, C.cmin, C.vslot,
                       ctr + SM_OCCUPIED);
    hipLaunchKernelGGL(p2s_sm_rep_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, V, C.vslot, C.cmin, C.rep);
    hipLaunchKernelGGL(p2s_rp_face_weld_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, faces_dev, F, C.rep, C.wfa, C.keep, ctr + SM_COLLAPSED);
    hipLaunchKernelGGL(p2s_sm_used_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, C.wfa, F, C.keep, C.used);
    hipLaunchKernelGGL(p2s_rp_face_insert_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, C.wfa, F, C.keep, C.fslot, fcap - 1);
    hipLaunchKernelGGL(p2s_rp_face_keep_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, C.wfa, F, C.keep, C.fslot, fcap - 1, ctr + SM_DUPLICATE);
    hipLaunchKernelGGL(p2s_sm_fkeys_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, verts_dev, faces_dev, F, C.rep, C.used, C.vstart,
                       (unsigned long long *)nullptr, ctr + SM_DEGENERATE);
    DEV_CHECK(who, hipGetLastError());
    size_t tb = scan_tmp;
    DEV_CHECK(who, hipcub::DeviceScan::ExclusiveSum(C.tmp, tb, C.used, C.vstart, (int)(V + 1), s));
    tb = scan_tmp;
    DEV_CHECK(who, hipcub::DeviceScan::ExclusiveSum(C.tmp, tb, C.keep, C.kstart, (int)(F + 1), s));
    int hV1 = 0, hF0 = 0;
    DEV_CHECK(who, hipMemcpyAsync(&hV1, C.vstart + V, 4, hipMemcpyDeviceToHost, s));
    DEV_CHECK(who, hipMemcpyAsync(&hF0, C.kstart + F, 4, hipMemcpyDeviceToHost, s));
    if ((rc = read_counters(who, ctr, hc, -1, nullptr, s)) != P2S_OK) return rc;
    const long long V1 = hV1, F0 = hF0;
    rep_out[1] = V1;
    rep_out[2] = F0;
    rep_out[4] = (long long)hc[SM_OCCUPIED];
    rep_out[5] = (long long)hc[SM_COLLAPSED];
    rep_out[6] = (long long)hc[SM_DUPLICATE];
    rep_out[7] = (long long)hc[SM_DEGENERATE];

    // ---- e. placement, f. the faces: into scratch, the report is whole before the capacity decides
    const SmPlaceWs D = pool.carve([&](char *b) { return carve_sm_place(b, (size_t)V, (size_t)F, (size_t)V1, (size_t)F0, placement == 1, sort_tmp); });
    if (!D.base) return dev_oom(who, s);
    DEV_CHECK(who, hipMemsetAsync(ctr, 0, MESH_COUNTERS, s));
    hipLaunchKernelGGL(p2s_sm_vkeys_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, V, C.rep, C.used, C.vstart, C.vmap, D.vkey);
    if (F0 > 0) {
        DEV_CHECK(who, hipMemsetAsync(D.vseg, 0, (size_t)V1 * 8, s));
        tb = sort_tmp;
        int end_bit = 33;                                            // 2^(end_bit - 32) - 1 >= V1 > every output id: SM_NO_KEY stays last
        while ((1ll << (end_bit - 32)) <= V1) ++end_bit;
        DEV_CHECK(who, hipcub::DeviceRadixSort::SortKeys(D.tmp, tb, D.vkey, D.vsorted, (int)V, 0, end_bit, s));
        hipLaunchKernelGGL(p2s_sm_seg_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, D.vsorted, V, V1, D.vseg);
        if (placement == 1) {
            DEV_CHECK(who, hipMemsetAsync(D.fseg, 0, (size_t)V1 * 8, s));
            hipLaunchKernelGGL(p2s_sm_fkeys_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, verts_dev, faces_dev, F, C.rep, C.used, C.vstart, D.fkey,
                               (unsigned long long *)nullptr);       // the degenerate faces were counted above
            tb = sort_tmp;
            DEV_CHECK(who, hipcub::DeviceRadixSort::SortKeys(D.tmp, tb, D.fkey, D.fsorted, (int)(3 * F), 0, end_bit, s));
            hipLaunchKernelGGL(p2s_sm_seg_kernel, dim3(blocks(3 * F, 256)), dim3(256), 0, s, D.fsorted, 3 * F, V1, D.fseg);
        }
        hipLaunchKernelGGL(p2s_sm_place_kernel, dim3(blocks(V1, 256)), dim3(256), 0, s, verts_dev, faces_dev, g, V1, D.vsorted, D.vseg, D.fsorted,
                           D.fseg, placement, epsilon, D.vout, ctr + SM_QUADRIC);
        hipLaunchKernelGGL(p2s_sm_faces_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, C.wfa, F, C.keep, C.kstart, C.vstart, D.wf, D.src);
        EdgeTable t = E.t;
        t.mask = rp_table_cap(3 * F0) - 1;                           // <= ecap: F0 <= F
        if ((rc = sm_edge_word(who, D.wf, F0, t, ctr, hc, &rep_out[12], s)) != P2S_OK) return rc;
        rep_out[8] = (long long)hc[SM_QUADRIC];
        rep_out[9] = (long long)hc[SM_TRACE0];
        rep_out[10] = (long long)hc[SM_FALLBACK];
    }
    publish();
    if (cap_verts < V1 || cap_faces < F0) {
        (void)hipStreamSynchronize(s);
        return too_small(V1, F0);
    }
    if (V1 > 0) DEV_CHECK(who, hipMemcpyAsync(verts_out_dev, D.vout, (size_t)V1 * 12, hipMemcpyDeviceToDevice, s));
    if (F0 > 0) {
        DEV_CHECK(who, hipMemcpyAsync(faces_out_dev, D.wf, (size_t)F0 * 12, hipMemcpyDeviceToDevice, s));
        if (face_src_out_dev) DEV_CHECK(who, hipMemcpyAsync(face_src_out_dev, D.src, (size_t)F0 * 4, hipMemcpyDeviceToDevice, s));
    }
    if (vert_map_out_dev) DEV_CHECK(who, hipMemcpyAsync(vert_map_out_dev, C.vmap, (size_t)V * 4, hipMemcpyDeviceToDevice, s));
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipStreamSynchronize(s));
    return P2S_OK;
}
