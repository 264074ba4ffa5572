// the connected components of a triangle mesh with their measures, and the sub-mesh of a face mask.
// Definitions: include/p2s_hip.h (p2s_mesh_components, p2s_mesh_submesh).  Included at the end of p2s_meshdist.hip, behind
// p2s_meshsimplify.inl: the edge table's layout and hash (EdgeTable, edge_key, edge_hash), the union-find
// primitives (uf_find, p2s_uf_compress_kernel), p2s_rp_used_kernel, p2s_rp_write_verts_kernel, p2s_sm_seg_kernel and
// the host scaffold are those files', used here and not copied.
//   p2s_mc_hook_kernel        union-find over the VERTICES: a face hooks (v0, v1) and (v1, v2), the larger root to the
//                             smaller by atomicMin; a pair whose ends already share a root is skipped
//   p2s_mc_first_kernel       the smallest face id per root (atomicMin; of a run of lanes with one root only the first asks)
//   p2s_mc_flag_kernel        1 at the smallest face of every component; its exclusive scan is the rank
//   p2s_mc_rank_kernel        comp[f] and the sort key (rank << 32 | face id)
//   p2s_mc_vkeys_kernel       (rank << 32 | vertex id) per referenced vertex
//   p2s_mc_face_part_kernel   per 256 sorted faces: the area and volume terms, summed per run of one rank in ascending face id
//   p2s_mc_vert_part_kernel   per 256 sorted vertices: the box of every run of one rank (integer atomicMin / atomicMax on the
//                             ordered bit pattern: no order can change it; p2s_mc_box_init_kernel sets the empty boxes)
//   p2s_mc_edges_kernel       the undirected edges a != b, once per face that uses them, into the edge table
//   p2s_mc_edge_stats_kernel  boundary edges and edges of more than two faces per component: the lanes of a wave that share a
//                             rank count among themselves, one atomicAdd per rank and wave
//   p2s_mc_collect_kernel     one wave per component: lane l adds the block partials l, l + 64, ... of the component's run in
//                             ascending order, a butterfly adds the 64 lane sums; writes counts [5] and measures [8]
//   p2s_mc_validate_kernel    indices in range, vertices finite (the box that p2s_md_validate_kernel also builds, with six
//                             atomics per wave, is not needed here)
//   p2s_mc_best_kernel        one workgroup: the most faces, the rank of the largest area, the referenced vertices
//   p2s_mc_keep_used_kernel / p2s_mc_submesh_faces_kernel / p2s_mc_vmap_kernel      the sub-mesh
// Determinism: roots, first faces and boxes are integer minima and maxima, counts are integer sums, ranks come from an
// exclusive scan (hipcub), and a component's float64 sums run over keys that a radix sort put in ascending face id: first
// within each block of 256 sorted keys, then over the blocks as p2s_mc_collect_kernel fixes it.  No floating-point atomic.
// Termination: uf_find walks strictly decreasing parents.  A round of hooks that changes something turns at least one root
// into a non-root (the thread that raised `changed` saw two different roots and lowered the parent of the larger), and a
// vertex never becomes a root again: after at most V - 1 such rounds and one that changes nothing the host loop ends; more
// than V + 1 rounds is an internal error.  No thread waits for another.

namespace {

__global__ __launch_bounds__(256) void p2s_mc_hook_kernel(const int *__restrict__ faces, long long F, int *parent, int *changed) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int v[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
    for (int e = 0; e < 2; ++e) {
        const int ra = uf_find(parent, v[e]), rb = uf_find(parent, v[e + 1]);
        if (ra != rb) {
            atomicMin(&parent[max(ra, rb)], min(ra, rb));
            *changed = 1;
        }
    }
}
// parent is fully compressed.  fmin [V]: 0x7f7f7f7f initially
__global__ __launch_bounds__(256) void p2s_mc_first_kernel(const int *__restrict__ faces, long long F, const int *__restrict__ parent, int *fmin) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    const int root = f < F ? parent[faces[3 * f]] : -1;
    const int prev = __shfl_up(root, 1);
    // the lane before holds a smaller face id; a value read that is no larger than f can only have shrunk since
    if (f < F && ((threadIdx.x & 63) == 0 || prev != root) && fmin[root] > (int)f) atomicMin(&fmin[root], (int)f);
}
__global__ __launch_bounds__(256) void p2s_mc_flag_kernel(const int *__restrict__ faces, long long F, const int *__restrict__ parent,
                                                          const int *__restrict__ fmin, int *__restrict__ flag) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f < F) flag[f] = fmin[parent[faces[3 * f]]] == (int)f;
}
__global__ __launch_bounds__(256) void p2s_mc_rank_kernel(const int *__restrict__ faces, long long F, const int *__restrict__ parent,
                                                          const int *__restrict__ fmin, const int *__restrict__ fstart, int *__restrict__ comp,
                                                          unsigned long long *__restrict__ fkey) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int r = fstart[fmin[parent[faces[3 * f]]]];
    comp[f] = r;
    fkey[f] = ((unsigned long long)(unsigned)r << 32) | (unsigned)f;
}
__global__ __launch_bounds__(256) void p2s_mc_vkeys_kernel(long long V, const int *__restrict__ used, const int *__restrict__ parent,
                                                           const int *__restrict__ fmin, const int *__restrict__ fstart,
                                                           unsigned long long *__restrict__ vkey) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    vkey[v] = used[v] ? (((unsigned long long)(unsigned)fstart[fmin[parent[v]]] << 32) | (unsigned)v) : SM_NO_KEY;
}

// part [F][2]: at the first key of a block, and at every key whose rank differs from the key before it, the sums of the area
// and volume terms of the run of that rank up to the end of the block, in ascending position
__global__ __launch_bounds__(256) void p2s_mc_face_part_kernel(const float *__restrict__ verts, const int *__restrict__ faces,
                                                               const unsigned long long *__restrict__ fsorted, long long F,
                                                               double *__restrict__ part) {
    __shared__ double sa[256], sv[256];
    __shared__ unsigned sr[256];
    const int tid = threadIdx.x;
    const long long i = (long long)blockIdx.x * 256 + tid;
    unsigned r = 0xffffffffu;                    // no rank: C <= 2^27
    if (i < F) {
        const unsigned long long key = fsorted[i];
        const long long f = (long long)(unsigned)key;
        r = (unsigned)(key >> 32);
        double a[3], b[3], c[3], u[3], w[3], n[3];
        for (int k = 0; k < 3; ++k) {
            a[k] = verts[3 * (long long)faces[3 * f] + k];
            b[k] = verts[3 * (long long)faces[3 * f + 1] + k];
            c[k] = verts[3 * (long long)faces[3 * f + 2] + k];
            u[k] = b[k] - a[k];
            w[k] = c[k] - a[k];
        }
        cross3(u, w, n);
        sa[tid] = 0.5 * sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
        cross3(b, c, n);
        sv[tid] = ((a[0] * n[0] + a[1] * n[1]) + a[2] * n[2]) / 6.0;
    }
    sr[tid] = r;
    __syncthreads();
    if (i < F && (tid == 0 || sr[tid - 1] != r)) {
        double area = 0.0, vol = 0.0;
        for (int j = tid; j < 256 && sr[j] == r; ++j) {
            area += sa[j];
            vol += sv[j];
        }
        part[2 * i] = area;
        part[2 * i + 1] = vol;
    }
}
// boxi [C][6]: ordered minima and maxima of the components' referenced vertices
__global__ __launch_bounds__(256) void p2s_mc_box_init_kernel(int *__restrict__ boxi, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) boxi[i] = i % 6 < 3 ? 0x7fffffff : (int)0x80000000;
}
__global__ __launch_bounds__(256) void p2s_mc_vert_part_kernel(const float *__restrict__ verts, const unsigned long long *__restrict__ vsorted,
                                                               long long V, int *boxi) {
    __shared__ int so[3][256];
    __shared__ unsigned sr[256];
    const int tid = threadIdx.x;
    const long long i = (long long)blockIdx.x * 256 + tid;
    unsigned r = 0xffffffffu;
    if (i < V && vsorted[i] != SM_NO_KEY) {
        const unsigned long long key = vsorted[i];
        r = (unsigned)(key >> 32);
        for (int k = 0; k < 3; ++k) so[k][tid] = f2o(verts[3 * (long long)(unsigned)key + k]);
    }
    sr[tid] = r;
    __syncthreads();
    if (r != 0xffffffffu && (tid == 0 || sr[tid - 1] != r)) {
        int lo[3], hi[3];
        for (int k = 0; k < 3; ++k) lo[k] = hi[k] = so[k][tid];
        for (int j = tid + 1; j < 256 && sr[j] == r; ++j)
            for (int k = 0; k < 3; ++k) {
                lo[k] = min(lo[k], so[k][j]);
                hi[k] = max(hi[k], so[k][j]);
            }
        for (int k = 0; k < 3; ++k) {                                  // a bound read that already covers the run can only have widened since
            if (boxi[6 * (long long)r + k] > lo[k]) atomicMin(&boxi[6 * (long long)r + k], lo[k]);
            if (boxi[6 * (long long)r + 3 + k] < hi[k]) atomicMax(&boxi[6 * (long long)r + 3 + k], hi[k]);
        }
    }
}

// cnt[2 h] of an edge: the faces that use it.  A face with a repeated index has one edge a != b, which it uses once
__global__ __launch_bounds__(256) void p2s_mc_edges_kernel(const int *__restrict__ faces, long long F, EdgeTable t) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= 3 * F) return;
    const long long f = i / 3;
    const int e = (int)(i - 3 * f);
    const int v[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
    const int a = v[e], b = v[(e + 1) % 3];
    if (a == b) return;
    const unsigned long long key = edge_key(a, b);
    for (int d = 0; d < e; ++d)
        if (v[d] != v[(d + 1) % 3] && edge_key(v[d], v[(d + 1) % 3]) == key) return;      // an earlier edge of this face
    unsigned h = edge_hash(key) & t.mask;
    for (;;) {                                   // load factor <= 1/2: an empty slot exists
        const unsigned long long prev = atomicCAS(&t.key[h], EDGE_EMPTY, key);
        if (prev == EDGE_EMPTY || prev == key) break;
        h = (h + 1) & t.mask;
    }
    atomicAdd(&t.cnt[2 * h], 1);
}
// ecount [C][2]: boundary edges, edges of more than two faces; an edge belongs to the component of its smaller endpoint
__global__ __launch_bounds__(256) void p2s_mc_edge_stats_kernel(EdgeTable t, const int *__restrict__ parent, const int *__restrict__ fmin,
                                                                const int *__restrict__ fstart, unsigned long long *ecount) {
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int kind = -1, r = -1;
    if (i <= t.mask && t.key[i] != EDGE_EMPTY) {
        const int c = t.cnt[2 * i];
        kind = c == 1 ? 0 : (c > 2 ? 1 : -1);
        if (kind >= 0) r = fstart[fmin[parent[(int)(t.key[i] >> 32)]]];
    }
    bool todo = kind >= 0;
    for (unsigned long long open = __ballot(todo); open; open = __ballot(todo)) {
        const int leader = __ffsll((long long)open) - 1;
        const int lr = __shfl(r, leader);
        const bool mine = todo && r == lr;
        const unsigned long long m0 = __ballot(mine && kind == 0), m1 = __ballot(mine && kind == 1);
        if (lane == leader) {
            if (m0) atomicAdd(&ecount[2 * (long long)lr], (unsigned long long)__popcll(m0));
            if (m1) atomicAdd(&ecount[2 * (long long)lr + 1], (unsigned long long)__popcll(m1));
        }
        todo = todo && !mine;
    }
}

__global__ __launch_bounds__(256) void p2s_mc_collect_kernel(long long C, const unsigned long long *__restrict__ fsorted, const int *__restrict__ fseg,
                                                             const int *__restrict__ vseg, const double *__restrict__ part,
                                                             const int *__restrict__ boxi, const unsigned long long *__restrict__ ecount,
                                                             long long *__restrict__ counts, double *__restrict__ meas) {
    const long long r = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;      // one wave per component
    const int lane = threadIdx.x & 63;
    if (r >= C) return;
    const long long s = fseg[r], e = fseg[C + r];                     // never empty
    double area = 0.0, vol = 0.0;
    for (long long b = s / 256 + lane; b * 256 < e; b += 64) {         // lane l: the run's partials of its blocks l, l + 64, ... in order
        const long long i = max(b * 256, s);
        area += part[2 * i];
        vol += part[2 * i + 1];
    }
    for (int d = 32; d > 0; d >>= 1) {                                 // the 64 lane sums: a fixed butterfly, the same in every lane
        area += __shfl_xor(area, d);
        vol += __shfl_xor(vol, d);
    }
    if (lane) return;
    counts[5 * r] = (long long)(unsigned)fsorted[s];
    counts[5 * r + 1] = e - s;
    counts[5 * r + 2] = (long long)vseg[C + r] - vseg[r];
    counts[5 * r + 3] = (long long)ecount[2 * r];
    counts[5 * r + 4] = (long long)ecount[2 * r + 1];
    meas[8 * r] = area;
    meas[8 * r + 1] = vol;
    for (int k = 0; k < 6; ++k) meas[8 * r + 2 + k] = (double)o2f(boxi[6 * r + k]);
}
// out[0] the most faces of a component, out[1] the rank of the largest area (of equal ones the smallest), out[2] referenced vertices
__global__ __launch_bounds__(1024) void p2s_mc_best_kernel(long long C, const long long *__restrict__ counts, const double *__restrict__ meas,
                                                           long long *__restrict__ out) {
    __shared__ long long sf[16], sn[16], sk[16];
    __shared__ double sa[16];
    const int tid = threadIdx.x;
    long long faces = 0, nv = 0, rank = -1;
    double area = -1.0;
    for (long long r = tid; r < C; r += 1024) {                        // ascending ranks: > keeps the smallest of equal areas
        faces = max(faces, counts[5 * r + 1]);
        nv += counts[5 * r + 2];
        if (meas[8 * r] > area) {
            area = meas[8 * r];
            rank = r;
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        const long long of = __shfl_xor(faces, d), on = __shfl_xor(nv, d), ok = __shfl_xor(rank, d);
        const double oa = __shfl_xor(area, d);
        faces = max(faces, of);
        nv += on;
        if (ok >= 0 && (oa > area || (oa == area && ok < rank))) {
            area = oa;
            rank = ok;
        }
    }
    if ((tid & 63) == 0) {
        sf[tid >> 6] = faces;
        sn[tid >> 6] = nv;
        sk[tid >> 6] = rank;
        sa[tid >> 6] = area;
    }
    __syncthreads();
    if (tid == 0) {
        for (int j = 1; j < 16; ++j) {
            faces = max(faces, sf[j]);
            nv += sn[j];
            if (sk[j] >= 0 && (sa[j] > area || (sa[j] == area && sk[j] < rank))) {
                area = sa[j];
                rank = sk[j];
            }
        }
        out[0] = faces;
        out[1] = rank;
        out[2] = nv;
    }
}

// keep01 [F + 1]: 1 for a kept face; used [V + 1]: 1 for a vertex of a kept face (zeroed)
__global__ __launch_bounds__(256) void p2s_mc_keep_used_kernel(const int *__restrict__ faces, long long F, const int *__restrict__ keep,
                                                               int *__restrict__ keep01, int *__restrict__ used) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int k = keep[f] != 0;
    keep01[f] = k;
    if (k)
        for (int j = 0; j < 3; ++j) used[faces[3 * f + j]] = 1;
}
__global__ __launch_bounds__(256) void p2s_mc_submesh_faces_kernel(const int *__restrict__ faces, long long F, const int *__restrict__ keep01,
                                                                   const int *__restrict__ kstart, const int *__restrict__ vstart,
                                                                   int *__restrict__ faces_out, int *__restrict__ src_out) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F || !keep01[f]) return;
    const long long at = kstart[f];
    for (int j = 0; j < 3; ++j) faces_out[3 * at + j] = vstart[faces[3 * f + j]];
    if (src_out) src_out[at] = (int)f;
}
__global__ __launch_bounds__(256) void p2s_mc_vmap_kernel(long long V, const int *__restrict__ used, const int *__restrict__ vstart,
                                                          int *__restrict__ vmap) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v < V) vmap[v] = used[v] ? vstart[v] : -1;
}

// err |= 1 for a non-finite vertex, 2 for an index out of range
__global__ __launch_bounds__(256) void p2s_mc_validate_kernel(const float *__restrict__ verts, long long V, const int *__restrict__ faces,
                                                              long long F, int *__restrict__ err) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    int e = 0;
    if (i < 3 * V && !(fabsf(verts[i]) <= 3.4028235e38f)) e |= 1;
    if (i < 3 * F && (faces[i] < 0 || faces[i] >= V)) e |= 2;
    if (e) atomicOr(err, e);
}
int mc_validate(const char *who, const float *verts, long long V, const int *faces, long long F, int *ctl, hipStream_t s) {
    int h = 0;
    DEV_CHECK(who, hipMemsetAsync(ctl, 0, 4, s));
    hipLaunchKernelGGL(p2s_mc_validate_kernel, dim3(blocks(3 * std::max(V, F), 256)), dim3(256), 0, s, verts, V, faces, F, ctl);
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipMemcpyAsync(&h, ctl, 4, hipMemcpyDeviceToHost, s));
    DEV_CHECK(who, hipStreamSynchronize(s));
    if (h) {
        p2s_set_error("%s: %s", who, (h & 2) ? "face index out of range" : "non-finite vertex");
        return P2S_EINVAL;
    }
    return P2S_OK;
}

struct McWs {                                    // everything whose size the input gives
    int *ctl;
    long long *best;
    int *parent, *fmin, *used, *flag, *fstart, *comp;
    unsigned long long *fkey, *fsorted, *vkey, *vsorted;
    double *part;
    EdgeTable t;
    void *tmp;
    char *base;
    size_t bytes;
};
McWs carve_mc(char *base, size_t V, size_t F, unsigned ecap, size_t tmp_bytes) {
    Carver c{base};
    McWs w;
    w.ctl = c.take<int>(16);
    w.best = c.take<long long>(8);
    w.parent = c.take<int>(V);
    w.fmin = c.take<int>(V);
    w.used = c.take<int>(V);
    w.flag = c.take<int>(F + 1);
    w.fstart = c.take<int>(F + 1);
    w.comp = c.take<int>(F);
    w.fkey = c.take<unsigned long long>(F);
    w.fsorted = c.take<unsigned long long>(F);
    w.vkey = c.take<unsigned long long>(V);
    w.vsorted = c.take<unsigned long long>(V);
    w.part = c.take<double>(F * 2);
    w.t = carve_edges(c, ecap);
    w.tmp = c.take<char>(tmp_bytes);
    return c.done(w);
}
struct McOutWs {                                 // per component, until the capacity is known to suffice
    int *fseg, *vseg, *boxi;
    unsigned long long *ecount;
    long long *counts;
    double *meas;
    char *base;
    size_t bytes;
};
McOutWs carve_mc_out(char *base, size_t C) {
    Carver c{base};
    McOutWs w;
    w.fseg = c.take<int>(C * 2);
    w.vseg = c.take<int>(C * 2);
    w.boxi = c.take<int>(C * 6);
    w.ecount = c.take<unsigned long long>(C * 2);
    w.counts = c.take<long long>(C * 5);
    w.meas = c.take<double>(C * 8);
    return c.done(w);
}
struct McSubWs {
    int *ctl, *keep01, *kstart, *used, *vstart;
    void *tmp;
    char *base;
    size_t bytes;
};
McSubWs carve_mc_sub(char *base, size_t V, size_t F, size_t tmp_bytes) {
    Carver c{base};
    McSubWs w;
    w.ctl = c.take<int>(16);
    w.keep01 = c.take<int>(F + 1);
    w.kstart = c.take<int>(F + 1);
    w.used = c.take<int>(V + 1);
    w.vstart = c.take<int>(V + 1);
    w.tmp = c.take<char>(tmp_bytes);
    return c.done(w);
}

// the arguments that both calls share; NULL: fine
const char *mc_bad_mesh(const float *verts, int64_t V, const int32_t *faces, int64_t F, const int64_t *report) {
    if (!report) return "report_host is NULL";
    if (V < 0 || V > (1ll << 27)) return "n_verts outside 0 .. 2^27";
    if (F < 0 || F > (1ll << 27)) return "n_faces outside 0 .. 2^27";
    if (V > 0 && !verts) return "verts_dev is NULL";
    if (F > 0 && !faces) return "faces_dev is NULL";
    return nullptr;
}

}  // namespace

extern "C" int p2s_mesh_components(const float *verts_dev, int64_t n_verts, const int32_t *faces_dev, int64_t n_faces, int32_t *comp_out_dev,
                                   int64_t cap_components, int64_t *counts_out_dev, double *measures_out_dev, int64_t *report_host, int device,
                                   void *stream) {
    static const char *const who = "p2s_mesh_components";
    const char *bad = mc_bad_mesh(verts_dev, n_verts, faces_dev, n_faces, report_host);
    if (!bad) {
        if (cap_components < 0) bad = "cap_components < 0";
        else if (n_faces > 0 && !comp_out_dev) bad = "comp_out_dev is NULL";
        else if (cap_components > 0 && !counts_out_dev) bad = "counts_out_dev is NULL";
        else if (cap_components > 0 && !measures_out_dev) bad = "measures_out_dev is NULL";
    }
    if (bad) {
        p2s_set_error("%s: bad argument (%s)", who, bad);
        return P2S_EINVAL;
    }
    if (int rc = select_device(who, device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const long long V = n_verts, F = n_faces;
    long long rep_out[8] = {};
    rep_out[0] = V | (F << 32);
    rep_out[4] = V;
    auto publish = [&]() {
        for (int k = 0; k < 8; ++k) report_host[k] = rep_out[k];
    };
    PoolScratch pool(device, s);
    int rc;

    // ---- a. validate
    const unsigned ecap = rp_table_cap(3 * F);
    size_t t1 = 0, t2 = 0, t3 = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, t1, (int *)nullptr, (int *)nullptr, (int)(F + 1), nullptr);
    (void)hipcub::DeviceRadixSort::SortKeys(nullptr, t2, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (int)F, 0, 64, nullptr);
    (void)hipcub::DeviceRadixSort::SortKeys(nullptr, t3, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (int)V, 0, 64, nullptr);
    const size_t tmp_bytes = std::max(t1, std::max(t2, t3)) + 256;
    const McWs W = pool.carve([&](char *b) { return carve_mc(b, (size_t)V, (size_t)F, ecap, tmp_bytes); });
    if (!W.base) return dev_oom(who, s);
    if (V > 0 || F > 0) {
        if ((rc = mc_validate(who, verts_dev, V, faces_dev, F, W.ctl, s)) != P2S_OK) return rc;
    }
    if (F == 0) {                                                    // no component; every vertex is unreferenced
        publish();
        return P2S_OK;
    }

    // ---- b. the union-find over the vertices
    hipLaunchKernelGGL(p2s_iota_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, W.parent, V);
    rc = until_unchanged(who, "the connected components", V + 1, W.ctl, s, [&](long long) {      // the cap: see the head of this file
        hipLaunchKernelGGL(p2s_mc_hook_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, faces_dev, F, W.parent, W.ctl);
        hipLaunchKernelGGL(p2s_uf_compress_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, W.parent, V);
    }, &rep_out[5]);
    if (rc != P2S_OK) return rc;

    // ---- c. the order of the components, the ranks
    DEV_CHECK(who, hipMemsetAsync(W.fmin, 0x7f, (size_t)V * 4, s));
    DEV_CHECK(who, hipMemsetAsync(W.used, 0, (size_t)V * 4, s));
    DEV_CHECK(who, hipMemsetAsync(W.flag + F, 0, 4, s));
    hipLaunchKernelGGL(p2s_mc_first_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, faces_dev, F, W.parent, W.fmin);
    hipLaunchKernelGGL(p2s_mc_flag_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, faces_dev, F, W.parent, W.fmin, W.flag);
    hipLaunchKernelGGL(p2s_rp_used_kernel, dim3(blocks(3 * F, 256)), dim3(256), 0, s, faces_dev, F, W.used);
    DEV_CHECK(who, hipGetLastError());
    size_t tb = tmp_bytes;
    DEV_CHECK(who, hipcub::DeviceScan::ExclusiveSum(W.tmp, tb, W.flag, W.fstart, (int)(F + 1), s));
    int hC = 0;
    DEV_CHECK(who, hipMemcpyAsync(&hC, W.fstart + F, 4, hipMemcpyDeviceToHost, s));
    DEV_CHECK(who, hipStreamSynchronize(s));
    const long long C = hC;
    rep_out[1] = C;

    // ---- d, e. counts and measures, into scratch: the report is whole before the capacity decides
    const McOutWs O = pool.carve([&](char *b) { return carve_mc_out(b, (size_t)C); });
    if (!O.base) return dev_oom(who, s);
    int end_bit = 33;                                                // 2^(end_bit - 32) - 1 >= C > every rank: SM_NO_KEY stays last
    while ((1ll << (end_bit - 32)) <= C) ++end_bit;
    hipLaunchKernelGGL(p2s_mc_rank_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, faces_dev, F, W.parent, W.fmin, W.fstart, W.comp, W.fkey);
    hipLaunchKernelGGL(p2s_mc_vkeys_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, V, W.used, W.parent, W.fmin, W.fstart, W.vkey);
    DEV_CHECK(who, hipGetLastError());
    tb = tmp_bytes;
    DEV_CHECK(who, hipcub::DeviceRadixSort::SortKeys(W.tmp, tb, W.fkey, W.fsorted, (int)F, 0, end_bit, s));
    tb = tmp_bytes;
    DEV_CHECK(who, hipcub::DeviceRadixSort::SortKeys(W.tmp, tb, W.vkey, W.vsorted, (int)V, 0, end_bit, s));
    DEV_CHECK(who, hipMemsetAsync(O.fseg, 0, (size_t)C * 8, s));
    DEV_CHECK(who, hipMemsetAsync(O.vseg, 0, (size_t)C * 8, s));
    DEV_CHECK(who, hipMemsetAsync(O.ecount, 0, (size_t)C * 16, s));
    hipLaunchKernelGGL(p2s_mc_box_init_kernel, dim3(blocks(6 * C, 256)), dim3(256), 0, s, O.boxi, 6 * C);
    hipLaunchKernelGGL(p2s_sm_seg_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, W.fsorted, F, C, O.fseg);
    hipLaunchKernelGGL(p2s_sm_seg_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, W.vsorted, V, C, O.vseg);
    hipLaunchKernelGGL(p2s_mc_face_part_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, verts_dev, faces_dev, W.fsorted, F, W.part);
    hipLaunchKernelGGL(p2s_mc_vert_part_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, verts_dev, W.vsorted, V, O.boxi);
    DEV_CHECK(who, hipMemsetAsync(W.t.key, 0xff, (size_t)ecap * 8, s));
    DEV_CHECK(who, hipMemsetAsync(W.t.cnt, 0, (size_t)ecap * 8, s));
    hipLaunchKernelGGL(p2s_mc_edges_kernel, dim3(blocks(3 * F, 256)), dim3(256), 0, s, faces_dev, F, W.t);
    hipLaunchKernelGGL(p2s_mc_edge_stats_kernel, dim3(blocks((long long)ecap, 256)), dim3(256), 0, s, W.t, W.parent, W.fmin, W.fstart, O.ecount);
    hipLaunchKernelGGL(p2s_mc_collect_kernel, dim3(blocks(64 * C, 256)), dim3(256), 0, s, C, W.fsorted, O.fseg, O.vseg, W.part, O.boxi, O.ecount,
                       O.counts, O.meas);
    hipLaunchKernelGGL(p2s_mc_best_kernel, dim3(1), dim3(1024), 0, s, C, O.counts, O.meas, W.best);
    DEV_CHECK(who, hipGetLastError());
    long long best[3] = {};
    DEV_CHECK(who, hipMemcpyAsync(best, W.best, sizeof(best), hipMemcpyDeviceToHost, s));
    DEV_CHECK(who, hipStreamSynchronize(s));
    rep_out[2] = best[0];
    rep_out[3] = best[1];
    rep_out[4] = V - best[2];
    publish();
    if (cap_components < C) {
        p2s_set_error("%s: output buffers too small (%lld components, cap_components = %lld given)", who, C, (long long)cap_components);
        return P2S_EINVAL;
    }
    DEV_CHECK(who, hipMemcpyAsync(comp_out_dev, W.comp, (size_t)F * 4, hipMemcpyDeviceToDevice, s));
    DEV_CHECK(who, hipMemcpyAsync(counts_out_dev, O.counts, (size_t)C * 40, hipMemcpyDeviceToDevice, s));
    DEV_CHECK(who, hipMemcpyAsync(measures_out_dev, O.meas, (size_t)C * 64, hipMemcpyDeviceToDevice, s));
    DEV_CHECK(who, hipStreamSynchronize(s));
    return P2S_OK;
}

extern "C" int p2s_mesh_submesh(const float *verts_dev, int64_t n_verts, const int32_t *faces_dev, int64_t n_faces, const int32_t *keep_dev,
                                float *verts_out_dev, int64_t cap_verts, int32_t *faces_out_dev, int32_t *face_src_out_dev, int64_t cap_faces,
                                int32_t *vert_map_out_dev, int64_t *report_host, int device, void *stream) {
    static const char *const who = "p2s_mesh_submesh";
    const char *bad = mc_bad_mesh(verts_dev, n_verts, faces_dev, n_faces, report_host);
    if (!bad) {
        if (cap_verts < 0) bad = "cap_verts < 0";
        else if (cap_faces < 0) bad = "cap_faces < 0";
        else if (n_faces > 0 && !keep_dev) bad = "keep_dev is NULL";
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
    report_host[0] = V | (F << 32);
    report_host[1] = report_host[2] = 0;
    PoolScratch pool(device, s);
    int rc;
    size_t t1 = 0, t2 = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, t1, (int *)nullptr, (int *)nullptr, (int)(V + 1), nullptr);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, t2, (int *)nullptr, (int *)nullptr, (int)(F + 1), nullptr);
    const size_t tmp_bytes = std::max(t1, t2) + 256;
    const McSubWs W = pool.carve([&](char *b) { return carve_mc_sub(b, (size_t)V, (size_t)F, tmp_bytes); });
    if (!W.base) return dev_oom(who, s);
    if (V > 0 || F > 0) {
        if ((rc = mc_validate(who, verts_dev, V, faces_dev, F, W.ctl, s)) != P2S_OK) return rc;
    }
    DEV_CHECK(who, hipMemsetAsync(W.used, 0, (size_t)(V + 1) * 4, s));
    DEV_CHECK(who, hipMemsetAsync(W.keep01 + F, 0, 4, s));
    if (F > 0) hipLaunchKernelGGL(p2s_mc_keep_used_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, faces_dev, F, keep_dev, W.keep01, W.used);
    DEV_CHECK(who, hipGetLastError());
    size_t tb = tmp_bytes;
    DEV_CHECK(who, hipcub::DeviceScan::ExclusiveSum(W.tmp, tb, W.used, W.vstart, (int)(V + 1), s));
    tb = tmp_bytes;
    DEV_CHECK(who, hipcub::DeviceScan::ExclusiveSum(W.tmp, tb, W.keep01, W.kstart, (int)(F + 1), s));
    int hV = 0, hF = 0;
    DEV_CHECK(who, hipMemcpyAsync(&hV, W.vstart + V, 4, hipMemcpyDeviceToHost, s));
    DEV_CHECK(who, hipMemcpyAsync(&hF, W.kstart + F, 4, hipMemcpyDeviceToHost, s));
    DEV_CHECK(who, hipStreamSynchronize(s));
    report_host[1] = hV;
    report_host[2] = hF;
    if (cap_verts < hV || cap_faces < hF) {
        p2s_set_error("%s: output buffers too small (%d vertices and %d faces needed, cap_verts = %lld and cap_faces = %lld given)", who, hV, hF,
                      (long long)cap_verts, (long long)cap_faces);
        return P2S_EINVAL;
    }
    if (hF > 0) {
        hipLaunchKernelGGL(p2s_rp_write_verts_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, verts_dev, V, W.used, W.vstart, verts_out_dev);
        hipLaunchKernelGGL(p2s_mc_submesh_faces_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, faces_dev, F, W.keep01, W.kstart, W.vstart,
                           faces_out_dev, face_src_out_dev);
    }
    if (vert_map_out_dev && V > 0)
        hipLaunchKernelGGL(p2s_mc_vmap_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, V, W.used, W.vstart, vert_map_out_dev);
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipStreamSynchronize(s));
    return P2S_OK;
}
