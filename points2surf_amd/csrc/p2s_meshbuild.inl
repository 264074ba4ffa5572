// The mesh handle and its construction (p2s_trimesh_create / destroy / info).  Included by p2s_meshdist.hip behind the
// shared primitives and the octree (p2s_mesh_octree.inl); what the handle holds and why: the head of that file.

struct p2s_trimesh_s {
    int device = 0;
    long long V = 0, F = 0;
    int closed = 0, inverted = 0;
    long long bad_edges = 0;
    int components = 0;            // connected components (closed meshes only)
    int comp_root[16] = {};        // 2..16 components: the label (smallest face id) of each, ascending
    int comp_orient[16] = {};      // and the sign of its own signed volume as stored (+1 outward, -1 inward)
    int *comp = nullptr;           // [F]     component label of every face
    int *scomp = nullptr;          // [F]     the same in the order of sface
    int G = 1, L = 0;
    double scale = 1.0;            // largest |coordinate| of the mesh
    float lo[3] = {}, cell = 1.f, inv_cell = 1.f;
    char *arena = nullptr;         // one block of the device's cache (p2s_pool_alloc)
    double *tri = nullptr;         // [F][9]  a, b, c (flipped when inverted)
    int *fidx = nullptr;           // [F][3]
    double *fn = nullptr;          // [F][3]  unit normal, 0 for a degenerate face
    int *adj = nullptr;            // [F][3]  face across ab, bc, ca (-1: none)
    long long *vn = nullptr;       // [V][4]  angle-weighted normal and the sum of the angles, fixed point 2^-40
    int *cell_start = nullptr;     // [G^3 + 1]
    int *sface = nullptr;          // [F]     face ids sorted by cell
    double *stri = nullptr;        // [F][9]  triangles in that order
    int *nodes = nullptr;          // [(8^(L+1) - 1) / 7][6]  lo, hi as ordered integers of the float32 bounds
    double *mom = nullptr;         // [same][4]  sum of the area vectors 1/2 (b - a) x (c - a) and of the areas of the node's triangles
    long long n_degenerate = 0;    // faces under the 2^-90 rule (they add nothing to the moments)
    unsigned char *fbad = nullptr; // [F]     the face's normal is not trusted (zero area, or a sliver: see SLIVER_REL)
    int *vbad = nullptr;           // [V]     the vertex touches such a face
    long long last_tests = 0;
};

namespace {

__global__ __launch_bounds__(256) void p2s_md_edge_check_kernel(EdgeTable t, unsigned long long *__restrict__ bad) {
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i > t.mask) return;
    if (t.key[i] != EDGE_EMPTY && !(t.cnt[2 * i] == 1 && t.cnt[2 * i + 1] == 1)) atomicAdd(bad, 1ull);
}

struct SetupArgs {
    const float *verts;
    const int *faces;
    long long F;
    int flip;
    EdgeTable t;
    double *tri;
    int *fidx;
    double *fn;
    int *adj;
    unsigned long long *vn;
    unsigned char *fbad;
    int *vbad;
    int *fcell, *count;
    float lo[3], inv_cell;
    int G;
};

__global__ __launch_bounds__(256) void p2s_md_setup_kernel(SetupArgs s) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= s.F) return;
    int id[3] = {s.faces[3 * f], s.faces[3 * f + 1], s.faces[3 * f + 2]};
    if (s.flip) {
        const int t = id[1];
        id[1] = id[2];
        id[2] = t;
    }
    double P[9];
    for (int j = 0; j < 3; ++j)
        for (int k = 0; k < 3; ++k) P[3 * j + k] = s.verts[3 * (long long)id[j] + k];
    double ab[3], ac[3], n[3];
    for (int k = 0; k < 3; ++k) {
        ab[k] = P[3 + k] - P[k];
        ac[k] = P[6 + k] - P[k];
    }
    cross3(ab, ac, n);
    const double nn = dot3(n, n);
    const bool degenerate = !(nn > DEGENERATE_REL * (dot3(ab, ab) * dot3(ac, ac)));
    double bc[3];
    for (int k = 0; k < 3; ++k) bc[k] = P[6 + k] - P[3 + k];
    const double l0 = dot3(ab, ab), l1 = dot3(ac, ac), l2 = dot3(bc, bc);
    // smallest corner sine: |n|^2 over the product of the two longest squared edges
    const bool sliver = degenerate || !(nn > SLIVER_REL * ((l0 * l1 * l2) / fmin(l0, fmin(l1, l2))));
    s.fbad[f] = sliver ? 1 : 0;
    if (sliver)
        for (int j = 0; j < 3; ++j) atomicOr(&s.vbad[id[j]], 1);
    const double inv = degenerate ? 0.0 : 1.0 / sqrt(nn);
    for (int k = 0; k < 3; ++k) n[k] = degenerate ? 0.0 : n[k] * inv;
    for (int k = 0; k < 9; ++k) s.tri[9 * f + k] = P[k];
    for (int k = 0; k < 3; ++k) {
        s.fidx[3 * f + k] = id[k];
        s.fn[3 * f + k] = n[k];
    }
    for (int e = 0; e < 3; ++e) {
        const int a = id[e], b = id[(e + 1) % 3];
        const unsigned long long key = edge_key(a, b);
        unsigned h = edge_hash(key) & s.t.mask;
        int other = -1;
        for (unsigned step = 0; step <= s.t.mask; ++step) {
            const unsigned long long k = s.t.key[h];
            if (k == key) {
                // the face's own direction in the ORIGINAL orientation (a flipped face traversed b -> a there)
                const int mine = s.flip ? (b < a ? 0 : 1) : (a < b ? 0 : 1);
                other = s.t.face[2 * h + (1 - mine)];
                break;
            }
            if (k == EDGE_EMPTY) break;
            h = (h + 1) & s.t.mask;
        }
        s.adj[3 * f + e] = other;
    }
    if (!degenerate) {
        // angle-weighted vertex normals: exact integer sums of the 2^-40 fixed-point contributions (order-independent)
        for (int j = 0; j < 3; ++j) {
            double u[3], v[3], x[3];
            for (int k = 0; k < 3; ++k) {
                u[k] = P[3 * ((j + 1) % 3) + k] - P[3 * j + k];
                v[k] = P[3 * ((j + 2) % 3) + k] - P[3 * j + k];
            }
            cross3(u, v, x);
            const double ang = atan2(sqrt(dot3(x, x)), dot3(u, v));
            for (int k = 0; k < 3; ++k)
                atomicAdd(&s.vn[4 * (long long)id[j] + k], (unsigned long long)llrint(ang * n[k] * FIX));
            atomicAdd(&s.vn[4 * (long long)id[j] + 3], (unsigned long long)llrint(ang * FIX));
        }
    }
    int cell = 0;
    for (int k = 0; k < 3; ++k) {
        const float c = (float)(((P[k] + P[3 + k]) + P[6 + k]) / 3.0);
        int ci = (int)((c - s.lo[k]) * s.inv_cell);
        ci = min(max(ci, 0), s.G - 1);
        cell = cell * s.G + ci;
    }
    s.fcell[f] = cell;
    atomicAdd(&s.count[cell], 1);
}

__global__ __launch_bounds__(256) void p2s_md_cc_roots_kernel(const int *__restrict__ parent, long long F, int *__restrict__ n_roots,
                                                              int *__restrict__ roots) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f < F && parent[f] == (int)f) {
        const int at = atomicAdd(n_roots, 1);
        if (at < 16) roots[at] = (int)f;
    }
}
__global__ __launch_bounds__(256) void p2s_md_scomp_kernel(const int *__restrict__ comp, const int *__restrict__ sface, long long F,
                                                           int *__restrict__ scomp) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < F) scomp[t] = comp[sface[t]];
}

__global__ __launch_bounds__(256) void p2s_md_nodes_init_kernel(int *__restrict__ nodes, long long n_nodes) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_nodes) return;
    for (int k = 0; k < 3; ++k) {
        nodes[6 * i + k] = 0x7f800000;               // +inf
        nodes[6 * i + 3 + k] = (int)0x807fffff;      // -inf
    }
}

// the order within a cell is whatever the atomics give; p2s_md_cell_sort_kernel then makes it ascending in the face id
__global__ __launch_bounds__(256) void p2s_md_fill_kernel(const double *__restrict__ tri, const int *__restrict__ fcell, long long F,
                                                          const int *__restrict__ start, int *__restrict__ cursor,
                                                          int *__restrict__ sface, int *__restrict__ leaf) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int cell = fcell[f];
    const int at = start[cell] + atomicAdd(&cursor[cell], 1);
    sface[at] = (int)f;
    for (int k = 0; k < 3; ++k) {
        const float a = (float)tri[9 * f + k], b = (float)tri[9 * f + 3 + k], c = (float)tri[9 * f + 6 + k];      // exact: float32 vertices
        atomicMin(&leaf[6 * (long long)cell + k], f2o(fminf(a, fminf(b, c))));
        atomicMax(&leaf[6 * (long long)cell + 3 + k], f2o(fmaxf(a, fmaxf(b, c))));
    }
}

// The face ids of every cell in ascending order, so that two handles of one mesh hold the same sface / stri and every sum
// taken "in sface order" (the node moments, the exact terms of p2s_md_wtree_kernel) is reproducible.  No distance or ray
// result depends on the order (ties are decided by face id).  One thread per cell, in place: insertion sort for the usual
// handful of faces, heapsort beyond (a cell holds one to two triangles on average, see the choice of G).
__global__ __launch_bounds__(256) void p2s_md_cell_sort_kernel(const int *__restrict__ start, long long cells, int *__restrict__ sface) {
    const long long cell = (long long)blockIdx.x * 256 + threadIdx.x;
    if (cell >= cells) return;
    int *a = sface + start[cell];
    const int n = start[cell + 1] - start[cell];
    if (n <= 16) {
        for (int i = 1; i < n; ++i) {
            const int v = a[i];
            int j = i;
            for (; j > 0 && a[j - 1] > v; --j) a[j] = a[j - 1];
            a[j] = v;
        }
        return;
    }
    auto sift = [&](int root, int end) {             // max-heap on a[0, end)
        const int v = a[root];
        for (;;) {
            int ch = 2 * root + 1;
            if (ch >= end) break;
            if (ch + 1 < end && a[ch + 1] > a[ch]) ++ch;
            if (a[ch] <= v) break;
            a[root] = a[ch];
            root = ch;
        }
        a[root] = v;
    };
    for (int i = n / 2 - 1; i >= 0; --i) sift(i, n);
    for (int end = n - 1; end > 0; --end) {
        const int v = a[0];
        a[0] = a[end];
        a[end] = v;
        sift(0, end);
    }
}
__global__ __launch_bounds__(256) void p2s_md_stri_kernel(const double *__restrict__ tri, const int *__restrict__ sface, long long F,
                                                          double *__restrict__ stri) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= F) return;
    const long long f = sface[t];
    for (int k = 0; k < 9; ++k) stri[9 * t + k] = tri[9 * f + k];
}

// moments of a leaf cell: N = sum 1/2 (b - a) x (c - a), A = sum 1/2 |(b - a) x (c - a)| over its triangles in sface order
// (ascending face id), one thread per cell; a face under the 2^-90 degenerate rule adds 0 to both and is counted
__global__ __launch_bounds__(256) void p2s_md_moments_leaf_kernel(const double *__restrict__ stri, const int *__restrict__ start, long long cells,
                                                                  double *__restrict__ mom, unsigned long long *__restrict__ n_degenerate) {
    const long long cell = (long long)blockIdx.x * 256 + threadIdx.x;
    if (cell >= cells) return;
    double N[3] = {0.0, 0.0, 0.0}, A = 0.0;
    unsigned long long deg = 0;
    const int t1 = start[cell + 1];
    for (int t = start[cell]; t < t1; ++t) {
        const double *P = stri + 9 * (long long)t;
        double ab[3], ac[3], n[3];
        for (int k = 0; k < 3; ++k) {
            ab[k] = P[3 + k] - P[k];
            ac[k] = P[6 + k] - P[k];
        }
        cross3(ab, ac, n);
        const double nn = dot3(n, n);
        if (!(nn > DEGENERATE_REL * (dot3(ab, ab) * dot3(ac, ac)))) {
            ++deg;
            continue;
        }
        for (int k = 0; k < 3; ++k) N[k] += 0.5 * n[k];
        A += 0.5 * sqrt(nn);
    }
    for (int k = 0; k < 3; ++k) mom[4 * cell + k] = N[k];
    mom[4 * cell + 3] = A;
    if (deg) atomicAdd(n_degenerate, deg);
}

// level l (n = 2^l nodes per axis) from level l + 1
// and the parent's moments: its children's, added in the fixed order 0..7
__global__ __launch_bounds__(256) void p2s_md_nodes_up_kernel(int *__restrict__ parent, const int *__restrict__ child, double *__restrict__ pmom,
                                                              const double *__restrict__ cmom, int l) {
    const int n = 1 << l;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)n * n * n) return;
    const int z = (int)(i & (n - 1)), y = (int)((i >> l) & (n - 1)), x = (int)(i >> (2 * l));
    int mn[3] = {0x7f800000, 0x7f800000, 0x7f800000}, mx[3] = {(int)0x807fffff, (int)0x807fffff, (int)0x807fffff};
    double mo[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < 8; ++c) {
        const long long j = ((long long)(2 * x + (c >> 2)) * (2 * n) + (2 * y + ((c >> 1) & 1))) * (2 * n) + (2 * z + (c & 1));
        for (int k = 0; k < 3; ++k) {
            mn[k] = min(mn[k], child[6 * j + k]);
            mx[k] = max(mx[k], child[6 * j + 3 + k]);
        }
        for (int k = 0; k < 4; ++k) mo[k] += cmom[4 * j + k];
    }
    for (int k = 0; k < 3; ++k) {
        parent[6 * i + k] = mn[k];
        parent[6 * i + 3 + k] = mx[k];
    }
    for (int k = 0; k < 4; ++k) pmom[4 * i + k] = mo[k];
}

OctreeDev octree_of(const p2s_trimesh_s *m) { return {m->nodes, m->mom, m->cell_start, m->sface, m->stri, m->scomp, m->L, m->scale}; }

struct TrimeshDelete {
    void operator()(p2s_trimesh_s *m) const {
        p2s_pool_free(m->device, m->arena);
        delete m;
    }
};

// the handle's arrays in its arena (V, F set); returns the size
size_t carve_handle(p2s_trimesh_s *m, char *base, long long cells, long long n_nodes) {
    Carver c{base};
    const size_t F = (size_t)m->F, V = (size_t)m->V;
    m->tri = c.take<double>(F * 9);
    m->stri = c.take<double>(F * 9);
    m->fn = c.take<double>(F * 3);
    m->vn = c.take<long long>(V * 4);
    m->fidx = c.take<int>(F * 3);
    m->adj = c.take<int>(F * 3);
    m->sface = c.take<int>(F);
    m->cell_start = c.take<int>((size_t)cells + 1);
    m->nodes = c.take<int>((size_t)n_nodes * 6);
    m->mom = c.take<double>((size_t)n_nodes * 4);
    m->comp = c.take<int>(F);
    m->scomp = c.take<int>(F);
    m->fbad = c.take<unsigned char>(F);
    m->vbad = c.take<int>(V);
    return c.at;
}
// build scratch: a block of its own, back in the cache when the build is over
struct BuildWs {
    int *ctl;                      // 16 words: validation; then [0] the union-find's `changed`, the number of roots
    unsigned long long *ctr;
    EdgeTable t;
    int *fcell, *count, *cursor, *roots;
    double *vol;
    char *base;
    size_t bytes;
};
BuildWs carve_build(char *base, long long F, long long cells, unsigned cap) {
    Carver c{base};
    BuildWs w;
    w.ctl = c.take<int>(16);
    w.ctr = c.take<unsigned long long>(8);
    w.t = carve_edges(c, cap);
    w.fcell = c.take<int>((size_t)F);
    w.count = c.take<int>((size_t)cells);
    w.cursor = c.take<int>((size_t)cells);
    w.roots = c.take<int>(16);
    w.vol = c.take<double>(16);
    return c.done(w);
}
enum BuildCtr { BC_BAD_EDGES, BC_VOLUME, BC_DEGENERATE, BC_COMPONENTS };

}  // namespace

extern "C" int p2s_trimesh_destroy(p2s_trimesh_t m) {
    if (!m) return P2S_OK;
    (void)hipSetDevice(m->device);
    TrimeshDelete()(m);
    return P2S_OK;
}

extern "C" int p2s_trimesh_create(const float *verts_dev, int64_t n_verts, const int32_t *faces_dev, int64_t n_faces, int device,
                                  void *stream, p2s_trimesh_t *out) {
    static const char *const who = "p2s_trimesh_create";
    if (out) *out = nullptr;
    if (!verts_dev || !faces_dev || !out || n_verts < 1 || n_faces < 1 || n_verts > (1ll << 27) || n_faces > (1ll << 27)) {
        p2s_set_error("p2s_trimesh_create: bad argument (1 <= vertices, faces <= 2^27)");
        return P2S_EINVAL;
    }
    if (int rc = select_device(who, device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const long long V = n_verts, F = n_faces;

    // the index: G a power of two in [2, 128], the smallest with 8 G^2 >= F: a surface occupies a few G^2 cells, so one to
    // two triangles per occupied cell (measured on the 0.92 M-face mesh: ~110 triangle tests per query); the octree over
    // the G^3 cells is 24 bytes per node (55 MB at G = 128)
    int L = 1;
    while (L < MD_MAX_L && (double)(1 << L) * (double)(1 << L) * 8.0 < (double)F) ++L;
    const int G = 1 << L;
    const long long cells = (long long)G * G * G, n_nodes = oct_level_offset(L + 1), leaf_off = oct_level_offset(L);
    unsigned cap = 1024;
    while ((long long)cap < 6 * F) cap <<= 1;                      // 3 F half-edges at most: load factor <= 1/2

    std::unique_ptr<p2s_trimesh_s, TrimeshDelete> m(new p2s_trimesh_s());      // destroyed after `pool`: both behind a drained stream
    m->device = device;
    m->V = V;
    m->F = F;
    m->G = G;
    m->L = L;
    const size_t persistent = carve_handle(m.get(), nullptr, cells, n_nodes);
    m->arena = (char *)p2s_pool_alloc(device, persistent);
    PoolScratch pool(device, s);
    const BuildWs w = pool.carve([&](char *b) { return carve_build(b, F, cells, cap); });
    if (!m->arena || !w.base) {
        p2s_set_error("p2s_trimesh_create: out of device memory (%zu + %zu bytes)", persistent, w.bytes);
        return P2S_ENOMEM;
    }
    carve_handle(m.get(), m->arena, cells, n_nodes);
    float box[6];
    int rc = mesh_validate(who, verts_dev, V, faces_dev, F, w.ctl, box, s);
    if (rc != P2S_OK) return rc;
    float ext = 0.f;
    m->scale = 0.0;
    for (int k = 0; k < 3; ++k) {
        const float lo = box[k], hi = box[3 + k];
        m->lo[k] = lo;
        ext = std::max(ext, hi - lo);
        m->scale = std::max(m->scale, (double)std::max(std::fabs(lo), std::fabs(hi)));
    }
    if (!(ext > 0.f)) ext = 1.f;                                   // a single point: every centroid lands in cell 0
    m->cell = ext / (float)G;
    m->inv_cell = (float)G / ext;

    // closed? inverted?
    unsigned long long hc[8] = {};
    DEV_CHECK(who, hipMemsetAsync(w.ctr, 0, MESH_COUNTERS, s));
    if ((rc = build_edges(who, faces_dev, F, w.t, nullptr, nullptr, s)) != P2S_OK) return rc;
    hipLaunchKernelGGL(p2s_md_edge_check_kernel, dim3(blocks(cap, 256)), dim3(256), 0, s, w.t, w.ctr + BC_BAD_EDGES);
    hipLaunchKernelGGL(p2s_md_volume_kernel, dim3(1), dim3(1024), 0, s, verts_dev, faces_dev, F, (double *)(w.ctr + BC_VOLUME));
    if ((rc = read_counters(who, w.ctr, hc, -1, nullptr, s)) != P2S_OK) return rc;
    double vol6;
    memcpy(&vol6, &hc[BC_VOLUME], 8);
    m->bad_edges = (long long)hc[BC_BAD_EDGES];
    m->closed = m->bad_edges == 0;
    m->inverted = m->closed && vol6 < 0.0;
    if (!m->closed) m->comp = m->scomp = nullptr;

    // the stored triangles and the index
    const SetupArgs a = {verts_dev, faces_dev, F, m->inverted, w.t, m->tri, m->fidx, m->fn, m->adj, (unsigned long long *)m->vn,
                         m->fbad, m->vbad, w.fcell, w.count, {m->lo[0], m->lo[1], m->lo[2]}, m->inv_cell, G};
    DEV_CHECK(who, hipMemsetAsync(m->vn, 0, (size_t)V * 32, s));
    DEV_CHECK(who, hipMemsetAsync(m->vbad, 0, (size_t)V * 4, s));
    DEV_CHECK(who, hipMemsetAsync(w.count, 0, (size_t)cells * 4, s));
    DEV_CHECK(who, hipMemsetAsync(w.cursor, 0, (size_t)cells * 4, s));
    hipLaunchKernelGGL(p2s_md_nodes_init_kernel, dim3(blocks(n_nodes, 256)), dim3(256), 0, s, m->nodes, n_nodes);
    hipLaunchKernelGGL(p2s_md_setup_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(p2s_scan_kernel, dim3(1), dim3(1024), 0, s, w.count, cells, m->cell_start);
    hipLaunchKernelGGL(p2s_md_fill_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, m->tri, w.fcell, F, m->cell_start, w.cursor, m->sface,
                       m->nodes + 6 * leaf_off);
    hipLaunchKernelGGL(p2s_md_cell_sort_kernel, dim3(blocks(cells, 256)), dim3(256), 0, s, m->cell_start, cells, m->sface);
    hipLaunchKernelGGL(p2s_md_stri_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, m->tri, m->sface, F, m->stri);
    hipLaunchKernelGGL(p2s_md_moments_leaf_kernel, dim3(blocks(cells, 256)), dim3(256), 0, s, m->stri, m->cell_start, cells,
                       m->mom + 4 * leaf_off, w.ctr + BC_DEGENERATE);
    for (int l = L - 1; l >= 0; --l) {
        const long long off = oct_level_offset(l), coff = oct_level_offset(l + 1);
        hipLaunchKernelGGL(p2s_md_nodes_up_kernel, dim3(blocks(coff - off, 256)), dim3(256), 0, s, m->nodes + 6 * off, m->nodes + 6 * coff,
                           m->mom + 4 * off, m->mom + 4 * coff, l);
    }
    if (m->closed) {                                               // connected components
        int *parent = m->comp;
        hipLaunchKernelGGL(p2s_iota_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, parent, F);
        rc = until_unchanged(who, "the connected components", 100000, w.ctl, s, [&](long long) {
            hipLaunchKernelGGL(p2s_md_cc_hook_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, m->adj, parent, F, w.ctl);
            hipLaunchKernelGGL(p2s_uf_compress_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, parent, F);
        });
        if (rc != P2S_OK) return rc;
        hipLaunchKernelGGL(p2s_md_cc_count_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, parent, F, w.ctr + BC_COMPONENTS);
    }
    if ((rc = read_counters(who, w.ctr, hc, -1, nullptr, s)) != P2S_OK) return rc;
    m->n_degenerate = (long long)hc[BC_DEGENERATE];
    m->components = (int)hc[BC_COMPONENTS];
    if (m->components >= 2 && m->components <= 16) {
        // the labels of the components (host-sorted: the atomics' order is arbitrary) and each one's own orientation
        const int nc = m->components;
        int hr[16] = {};
        double hv[16] = {};
        DEV_CHECK(who, hipMemsetAsync(w.ctl, 0, 4, s));
        hipLaunchKernelGGL(p2s_md_cc_roots_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, m->comp, F, w.ctl, w.roots);
        DEV_CHECK(who, hipGetLastError());
        DEV_CHECK(who, hipMemcpyAsync(hr, w.roots, 64, hipMemcpyDeviceToHost, s));
        DEV_CHECK(who, hipStreamSynchronize(s));
        std::sort(hr, hr + nc);
        DEV_CHECK(who, hipMemcpyAsync(w.roots, hr, 64, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(p2s_md_comp_volume_kernel, dim3((unsigned)nc), dim3(1024), 0, s, m->tri, m->comp, F, w.roots, w.vol);
        hipLaunchKernelGGL(p2s_md_scomp_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, m->comp, m->sface, F, m->scomp);
        DEV_CHECK(who, hipGetLastError());
        DEV_CHECK(who, hipMemcpyAsync(hv, w.vol, 128, hipMemcpyDeviceToHost, s));
        DEV_CHECK(who, hipStreamSynchronize(s));
        for (int k = 0; k < nc; ++k) {
            m->comp_root[k] = hr[k];
            m->comp_orient[k] = hv[k] < 0.0 ? -1 : 1;
        }
    }
    *out = m.release();                                            // the stream is drained: `pool` goes back to the cache
    return P2S_OK;
}

extern "C" int p2s_trimesh_info(p2s_trimesh_t m, int64_t *info_host) {
    if (!m || !info_host) {
        p2s_set_error("p2s_trimesh_info: bad argument");
        return P2S_EINVAL;
    }
    const int64_t v[8] = {m->F, m->closed, m->inverted, m->bad_edges, m->G, m->last_tests, m->components, m->n_degenerate};
    for (int k = 0; k < 8; ++k) info_host[k] = v[k];
    return P2S_OK;
}
