// "next" row f-7: repair of a raw triangle mesh (weld, drop, orient, fill small holes, fix inversion, compact) and its
// normalisation -- the stages 02_meshes_cleaned / 03_meshes of the reference's make_dataset.py (:383-413, :71-88), which
// call trimesh.  Definitions: include/p2s_hip.h (p2s_mesh_repair).  Included at the end of p2s_meshdist.hip: the edge
// table with its hash (p2s_md_edges_kernel), the connected components (p2s_md_cc_*), the one-workgroup scan, the
// fixed-order volume sums (p2s_md_volume_kernel, p2s_md_comp_volume_kernel), the validation with the ordered-integer
// bounding box and DEGENERATE_REL are that file's, used here and not copied.
//   p2s_rp_weld_insert_kernel / p2s_rp_weld_map_kernel    vertices into a table keyed by their coordinates; representative
//   p2s_rp_face_weld_kernel / p2s_rp_face_insert_kernel / p2s_rp_face_keep_kernel   welded faces, collapsed, duplicates
//   p2s_rp_gather_kernel      the surviving faces in input order; degenerate count
//   p2s_rp_edge_faces_kernel  smallest and largest face id of every edge (the two faces of an edge that two faces use)
//   p2s_rp_adj_kernel         neighbour across every edge and whether the two traverse it in the same direction
//   p2s_rp_par_hook_kernel / p2s_rp_par_compress_kernel / p2s_rp_par_check_kernel / p2s_rp_par_apply_kernel
//                             union-find with a parity bit (hooking to the smaller root, full compression): orientation
//   p2s_rp_boundary_kernel / p2s_rp_hole_kernel / p2s_rp_hole_fill_kernel   boundary edges per vertex, hole loops, fans
//   p2s_rp_bhook_kernel / p2s_rp_bcount_kernel            connected groups of the boundary edges that remain
//   p2s_rp_edge_stats_kernel / p2s_rp_open_kernel / p2s_rp_roots_kernel / p2s_rp_tri_kernel / p2s_rp_invert_kernel
//   p2s_rp_used_kernel / p2s_rp_write_verts_kernel / p2s_rp_write_faces_kernel      compaction
//   p2s_rp_normalize_kernel
// Determinism: every table holds the SMALLEST id of a class (atomicMin), counters are integer sums, positions come from
// exclusive scans, float64 sums run in the fixed order of the shared volume kernels; where a slot is written by whichever
// thread comes last (a vertex's next boundary vertex) the value is used only if one thread writes it.

namespace {

__device__ __forceinline__ unsigned rp_bits(float x) {              // -0.0 counts as +0.0
    const unsigned b = __float_as_uint(x);
    return b == 0x80000000u ? 0u : b;
}
struct RpVertKey {
    const float *verts;
    __device__ unsigned hash(int i) const {
        const unsigned long long x = rp_bits(verts[3 * (long long)i]), y = rp_bits(verts[3 * (long long)i + 1]),
                                 z = rp_bits(verts[3 * (long long)i + 2]);
        return edge_hash(((x << 32) | y) ^ (z * 0x9e3779b97f4a7c15ull));
    }
    __device__ bool equal(int i, int j) const {
        for (int k = 0; k < 3; ++k)
            if (rp_bits(verts[3 * (long long)i + k]) != rp_bits(verts[3 * (long long)j + k])) return false;
        return true;
    }
};
struct RpFaceKey {                                                  // the vertex set of a welded face
    const int *wfa;
    __device__ void sorted(int f, int *s) const {
        int a = wfa[3 * (long long)f], b = wfa[3 * (long long)f + 1], c = wfa[3 * (long long)f + 2];
        if (a > b) { const int t = a; a = b; b = t; }
        if (b > c) { const int t = b; b = c; c = t; }
        if (a > b) { const int t = a; a = b; b = t; }
        s[0] = a; s[1] = b; s[2] = c;
    }
    __device__ unsigned hash(int f) const {
        int s[3];
        sorted(f, s);
        return edge_hash((((unsigned long long)(unsigned)s[0] << 32) | (unsigned)s[1]) ^ ((unsigned long long)(unsigned)s[2] * 0x9e3779b97f4a7c15ull));
    }
    __device__ bool equal(int f, int g) const {
        int s[3], t[3];
        sorted(f, s);
        sorted(g, t);
        return s[0] == t[0] && s[1] == t[1] && s[2] == t[2];
    }
};
// open addressing, load factor <= 1/2; a slot holds the smallest id of the items equal to its first one
template <class K> __device__ __forceinline__ void rp_insert(const K &k, int *slot, unsigned mask, int i) {
    unsigned h = k.hash(i) & mask;
    for (;;) {
        const int cur = atomicCAS(&slot[h], -1, i);
        if (cur == -1) return;
        if (k.equal(cur, i)) {                   // whichever member `cur` was: all members are equal
            atomicMin(&slot[h], i);
            return;
        }
        h = (h + 1) & mask;
    }
}
template <class K> __device__ __forceinline__ int rp_find(const K &k, const int *slot, unsigned mask, int i) {
    unsigned h = k.hash(i) & mask;
    for (;;) {                                   // i was inserted: the walk ends
        const int cur = slot[h];
        if (cur == -1) return i;
        if (k.equal(cur, i)) return cur;
        h = (h + 1) & mask;
    }
}

__global__ __launch_bounds__(256) void p2s_rp_weld_insert_kernel(const float *__restrict__ verts, long long V, int *slot, unsigned mask) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < V) rp_insert(RpVertKey{verts}, slot, mask, (int)i);
}
__global__ __launch_bounds__(256) void p2s_rp_weld_map_kernel(const float *__restrict__ verts, long long V, const int *__restrict__ slot,
                                                              unsigned mask, int *__restrict__ rep, unsigned long long *__restrict__ welded) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    const int r = rp_find(RpVertKey{verts}, slot, mask, (int)i);
    rep[i] = r;
    if (r != (int)i) atomicAdd(welded, 1ull);
}
// flag: 0 kept so far, 1 collapsed
__global__ __launch_bounds__(256) void p2s_rp_face_weld_kernel(const int *__restrict__ faces, long long F, const int *__restrict__ rep,
                                                               int *__restrict__ wfa, int *__restrict__ keep,
                                                               unsigned long long *__restrict__ collapsed) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int a = rep[faces[3 * f]], b = rep[faces[3 * f + 1]], c = rep[faces[3 * f + 2]];
    wfa[3 * f] = a;
    wfa[3 * f + 1] = b;
    wfa[3 * f + 2] = c;
    const bool bad = a == b || b == c || c == a;
    keep[f] = bad ? 0 : 1;
    if (bad) atomicAdd(collapsed, 1ull);
}
__global__ __launch_bounds__(256) void p2s_rp_face_insert_kernel(const int *__restrict__ wfa, long long F, const int *__restrict__ keep,
                                                                 int *slot, unsigned mask) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f < F && keep[f]) rp_insert(RpFaceKey{wfa}, slot, mask, (int)f);
}
__global__ __launch_bounds__(256) void p2s_rp_face_keep_kernel(const int *__restrict__ wfa, long long F, int *__restrict__ keep,
                                                               const int *__restrict__ slot, unsigned mask,
                                                               unsigned long long *__restrict__ duplicate) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F || !keep[f]) return;
    if (rp_find(RpFaceKey{wfa}, slot, mask, (int)f) != (int)f) {
        keep[f] = 0;
        atomicAdd(duplicate, 1ull);
    }
}
__global__ __launch_bounds__(256) void p2s_rp_gather_kernel(const float *__restrict__ verts, const int *__restrict__ wfa, long long F,
                                                            const int *__restrict__ keep, const int *__restrict__ start,
                                                            int *__restrict__ wf, int *__restrict__ src,
                                                            unsigned long long *__restrict__ degenerate) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F || !keep[f]) return;
    const long long at = start[f];
    double P[9];
    for (int j = 0; j < 3; ++j) {
        const int v = wfa[3 * f + j];
        wf[3 * at + j] = v;
        for (int k = 0; k < 3; ++k) P[3 * j + k] = verts[3 * (long long)v + k];
    }
    src[at] = (int)f;
    double ab[3], ac[3], n[3];
    for (int k = 0; k < 3; ++k) {
        ab[k] = P[3 + k] - P[k];
        ac[k] = P[6 + k] - P[k];
    }
    cross3(ab, ac, n);
    if (!(dot3(n, n) > DEGENERATE_REL * (dot3(ab, ab) * dot3(ac, ac)))) atomicAdd(degenerate, 1ull);
}

// adj: the other face of an edge that exactly two faces use, else -1; par: 1 when both traverse it in the same direction
__global__ __launch_bounds__(256) void p2s_rp_adj_kernel(const int *__restrict__ faces, long long F, EdgeTable t, const int *__restrict__ fmn,
                                                         const int *__restrict__ fmx, int *__restrict__ adj, unsigned char *__restrict__ par) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= 3 * F) return;
    const long long f = i / 3;
    const int e = (int)(i - 3 * f);
    const unsigned h = rp_edge_slot(t, faces[3 * f + e], faces[3 * f + (e + 1) % 3]);
    const int c0 = t.cnt[2 * h], c1 = t.cnt[2 * h + 1];
    int g = -1;
    if (c0 + c1 == 2) g = fmn[h] == (int)f ? fmx[h] : fmn[h];
    adj[i] = g;
    if (par) par[i] = (c0 == 1 && c1 == 1) ? 0 : 1;
}

// Union-find with parity.  link[f] = parent << 1 | p, p = whether f is flipped relative to its parent; a root is f << 1.
// A hook is a compare-and-swap on a root's word, so a word is written once as a root and then only shortened by the
// compression: every state of every word is valid and a walk that races with them still ends at an ancestor with the
// right parity.  Parents only decrease: the root of a finished component is its smallest face id.
__device__ __forceinline__ int rp_find_par(const int *link, int x, int *parity) {
    int acc = 0;
    for (;;) {
        const int w = __atomic_load_n(&link[x], __ATOMIC_RELAXED);
        if ((w >> 1) == x) break;
        acc ^= w & 1;
        x = w >> 1;
    }
    *parity = acc;
    return x;
}
__global__ __launch_bounds__(256) void p2s_rp_par_hook_kernel(const int *__restrict__ adj, const unsigned char *__restrict__ par, int *link,
                                                              long long F, int *changed) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    for (int e = 0; e < 3; ++e) {
        const int g = adj[3 * f + e];
        if (g < 0) continue;
        int pf, pg;
        const int rf = rp_find_par(link, (int)f, &pf), rg = rp_find_par(link, g, &pg);
        if (rf != rg) {
            const int hi = max(rf, rg), lo = min(rf, rg);
            atomicCAS(&link[hi], hi << 1, (lo << 1) | (pf ^ pg ^ (int)par[3 * f + e]));      // lost: the next round tries again
            *changed = 1;
        }
    }
}
__global__ __launch_bounds__(256) void p2s_rp_par_compress_kernel(int *link, long long F, int init) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    if (init) {
        link[f] = (int)f << 1;
        return;
    }
    int p;
    const int r = rp_find_par(link, (int)f, &p);
    __atomic_store_n(&link[f], (r << 1) | p, __ATOMIC_RELAXED);
}
// after convergence: an edge whose two faces' parities do not differ by its own makes the component unorientable
__global__ __launch_bounds__(256) void p2s_rp_par_check_kernel(const int *__restrict__ adj, const unsigned char *__restrict__ par,
                                                               const int *__restrict__ link, long long F, int *__restrict__ badroot) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    for (int e = 0; e < 3; ++e) {
        const int g = adj[3 * f + e];
        if (g >= 0 && (((link[f] ^ link[g]) & 1) != (int)par[3 * f + e])) badroot[link[f] >> 1] = 1;
    }
}
// ctr[0] faces flipped, ctr[1] unorientable components
__global__ __launch_bounds__(256) void p2s_rp_par_apply_kernel(const int *__restrict__ link, const int *__restrict__ badroot, long long F,
                                                               int *__restrict__ wf, unsigned char *__restrict__ flipped,
                                                               unsigned char *__restrict__ unor, unsigned long long *__restrict__ ctr) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int r = link[f] >> 1, bad = badroot[r];
    unor[f] = bad ? 1 : 0;
    const bool flip = !bad && (link[f] & 1);
    flipped[f] = flip ? 1 : 0;
    if (flip) {
        const int t = wf[3 * f + 1];
        wf[3 * f + 1] = wf[3 * f + 2];
        wf[3 * f + 2] = t;
        atomicAdd(&ctr[0], 1ull);
    }
    if (bad && r == (int)f) atomicAdd(&ctr[1], 1ull);
}

// boundary edges (one face) as that face traverses them: outgoing / incoming count per vertex, the vertex after it.  unor
// (faces of components that cannot be oriented) may be NULL: p2s_mesh_fill_holes has none, and blocked is not touched then
__global__ __launch_bounds__(256) void p2s_rp_boundary_kernel(const int *__restrict__ faces, long long F, EdgeTable t,
                                                              const unsigned char *__restrict__ unor, int *outc, int *inc, int *nxt, int *blocked) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= 3 * F) return;
    const long long f = i / 3;
    const int e = (int)(i - 3 * f);
    const int a = faces[3 * f + e], b = faces[3 * f + (e + 1) % 3];
    const unsigned h = rp_edge_slot(t, a, b);
    if (t.cnt[2 * h] + t.cnt[2 * h + 1] != 1) return;
    atomicAdd(&outc[a], 1);
    atomicAdd(&inc[b], 1);
    nxt[a] = b;                                  // used only where outc[a] == 1: one writer
    if (unor && unor[f]) {
        blocked[a] = 1;
        blocked[b] = 1;
    }
}
// v is the smallest vertex of a hole of n <= K edges: addc[v] = n - 2 faces
__global__ __launch_bounds__(256) void p2s_rp_hole_kernel(long long V, int K, const int *__restrict__ outc, const int *__restrict__ inc,
                                                          const int *__restrict__ nxt, const int *__restrict__ blocked, int *__restrict__ addc,
                                                          unsigned long long *__restrict__ holes) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    int add = 0;
    if (outc[v] == 1 && inc[v] == 1 && !blocked[v]) {
        int x = nxt[v], n = 1;
        bool ok = true;
        while (x != (int)v) {
            if (n >= K || x < (int)v || !(outc[x] == 1 && inc[x] == 1 && !blocked[x])) {
                ok = false;
                break;
            }
            x = nxt[x];
            ++n;
        }
        if (ok && n >= 3 && n <= K) add = n - 2;
    }
    addc[v] = add;
    if (add) atomicAdd(holes, 1ull);
}
__global__ __launch_bounds__(256) void p2s_rp_hole_fill_kernel(long long V, const int *__restrict__ nxt, const int *__restrict__ addc,
                                                               const int *__restrict__ addstart, long long F0, int *__restrict__ wf) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= V || !addc[v]) return;
    int prev = nxt[v], cur = nxt[prev];
    for (int k = 0; k < addc[v]; ++k) {
        const long long at = F0 + addstart[v] + k;
        wf[3 * at] = (int)v;
        wf[3 * at + 1] = cur;
        wf[3 * at + 2] = prev;
        prev = cur;
        cur = nxt[cur];
    }
}
// groups of the boundary edges that remain: union-find over the vertices (uf_find, hooking to the smaller root)
__global__ __launch_bounds__(256) void p2s_rp_bhook_kernel(const int *__restrict__ faces, long long F, EdgeTable t, int *parent, int *changed) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= 3 * F) return;
    const long long f = i / 3;
    const int e = (int)(i - 3 * f);
    const int a = faces[3 * f + e], b = faces[3 * f + (e + 1) % 3];
    const unsigned h = rp_edge_slot(t, a, b);
    if (t.cnt[2 * h] + t.cnt[2 * h + 1] != 1) return;
    const int ra = uf_find(parent, a), rb = uf_find(parent, b);
    if (ra != rb) {
        atomicMin(&parent[max(ra, rb)], min(ra, rb));
        *changed = 1;
    }
}
__global__ __launch_bounds__(256) void p2s_rp_bmark_kernel(const int *__restrict__ faces, long long F, EdgeTable t, int *__restrict__ onb) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= 3 * F) return;
    const long long f = i / 3;
    const int e = (int)(i - 3 * f);
    const int a = faces[3 * f + e], b = faces[3 * f + (e + 1) % 3];
    const unsigned h = rp_edge_slot(t, a, b);
    if (t.cnt[2 * h] + t.cnt[2 * h + 1] == 1) {
        onb[a] = 1;
        onb[b] = 1;
    }
}
__global__ __launch_bounds__(256) void p2s_rp_bcount_kernel(const int *__restrict__ parent, const int *__restrict__ onb, long long V,
                                                            unsigned long long *__restrict__ count) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v < V && onb[v] && parent[v] == (int)v) atomicAdd(count, 1ull);
}

// ctr[0] boundary edges, ctr[1] edges of more than two faces, ctr[2] edges of two faces that traverse them the same way
__global__ __launch_bounds__(256) void p2s_rp_edge_stats_kernel(EdgeTable t, unsigned long long *__restrict__ ctr) {
    unsigned long long boundary = 0, overfull = 0, same_way = 0;
    for (unsigned long long i = blockIdx.x * 256ull + threadIdx.x; i <= t.mask; i += gridDim.x * 256ull) {      // any grid
        if (t.key[i] == EDGE_EMPTY) continue;
        const int c0 = t.cnt[2 * i], c1 = t.cnt[2 * i + 1];
        boundary += c0 + c1 == 1;
        overfull += c0 + c1 > 2;
        same_way += c0 + c1 == 2 && c0 != 1;
    }
    wave_count(&ctr[0], boundary);               // one atomic per wave: a mesh of many boundary edges queued on one address
    wave_count(&ctr[1], overfull);
    wave_count(&ctr[2], same_way);
}
__global__ __launch_bounds__(256) void p2s_rp_open_kernel(const int *__restrict__ faces, long long F, EdgeTable t, const int *__restrict__ parent,
                                                          int *__restrict__ open) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= 3 * F) return;
    const long long f = i / 3;
    const int e = (int)(i - 3 * f);
    const unsigned h = rp_edge_slot(t, faces[3 * f + e], faces[3 * f + (e + 1) % 3]);
    if (t.cnt[2 * h] + t.cnt[2 * h + 1] == 1) open[parent[f]] = 1;
}
// open[f] becomes: 1 = f is the root of a component without a boundary edge
__global__ __launch_bounds__(256) void p2s_rp_roots_flag_kernel(const int *__restrict__ parent, long long F, int *__restrict__ open) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f < F) open[f] = (parent[f] == (int)f && !open[f]) ? 1 : 0;
}
__global__ __launch_bounds__(256) void p2s_rp_roots_kernel(const int *__restrict__ flag, const int *__restrict__ start, long long F,
                                                           int *__restrict__ roots) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f < F && flag[f]) roots[start[f]] = (int)f;
}
__global__ __launch_bounds__(256) void p2s_rp_tri_kernel(const float *__restrict__ verts, const int *__restrict__ faces, long long F,
                                                         double *__restrict__ tri) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= 9 * F) return;
    const long long f = i / 9;
    const int r = (int)(i - 9 * f);
    tri[i] = verts[3 * (long long)faces[3 * f + r / 3] + r % 3];
}
__global__ __launch_bounds__(256) void p2s_rp_invert_kernel(const int *__restrict__ parent, const int *__restrict__ flag,
                                                            const int *__restrict__ start, const double *__restrict__ vol, long long F,
                                                            int *__restrict__ wf, unsigned long long *__restrict__ inverted) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int r = parent[f];
    if (!flag[r] || !(vol[start[r]] < 0.0)) return;
    const int t = wf[3 * f + 1];
    wf[3 * f + 1] = wf[3 * f + 2];
    wf[3 * f + 2] = t;
    if (r == (int)f) atomicAdd(inverted, 1ull);
}

__global__ __launch_bounds__(256) void p2s_rp_used_kernel(const int *__restrict__ wf, long long F, int *__restrict__ used) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < 3 * F) used[wf[i]] = 1;
}
__global__ __launch_bounds__(256) void p2s_rp_write_verts_kernel(const float *__restrict__ verts, long long V, const int *__restrict__ used,
                                                                 const int *__restrict__ start, float *__restrict__ out) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= V || !used[v]) return;
    for (int k = 0; k < 3; ++k) out[3 * (long long)start[v] + k] = verts[3 * v + k];
}
__global__ __launch_bounds__(256) void p2s_rp_write_faces_kernel(const int *__restrict__ wf, const int *__restrict__ src, long long F,
                                                                 long long F0, const int *__restrict__ start, int *__restrict__ faces_out,
                                                                 int *__restrict__ src_out) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    for (int k = 0; k < 3; ++k) faces_out[3 * f + k] = start[wf[3 * f + k]];
    src_out[f] = f < F0 ? src[f] : -1;
}

__global__ __launch_bounds__(256) void p2s_rp_normalize_kernel(const float *__restrict__ verts, long long n, double cx, double cy, double cz,
                                                               double s, float *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= 3 * n) return;
    const int k = (int)(i % 3);
    const double c = k == 0 ? cx : (k == 1 ? cy : cz);
    out[i] = (float)(((double)verts[i] - c) * s);
}

unsigned rp_table_cap(long long n) {             // a power of two >= 2 n: load factor <= 1/2
    unsigned cap = 1024;
    while ((long long)cap < 2 * n) cap <<= 1;
    return cap;
}

// the counters of p2s_mesh_repair, zeroed before each of its three phases
enum RepairCtr {
    RP_WELDED = 0, RP_COLLAPSED, RP_DUPLICATE,                                               // b, c
    RP_DEGENERATE = 0, RP_FLIPPED, RP_UNORIENTABLE, RP_HOLES,                                // d, e
    RP_BOUNDARY = 0, RP_NONMANIFOLD, RP_INCONSISTENT, RP_COMPONENTS, RP_BGROUPS, RP_INVERTED, RP_VOLUME      // f, g
};

// the four blocks of p2s_mesh_repair, each carved when its sizes are known
struct RpWeldWs {                                // b, c
    int *ctl;
    unsigned long long *ctr;
    int *vslot, *fslot, *rep, *wfa, *keep, *kstart;
    char *base;
    size_t bytes;
};
RpWeldWs carve_weld(char *base, size_t V, size_t F, unsigned vcap, unsigned fcap) {
    Carver c{base};
    RpWeldWs w;
    w.ctl = c.take<int>(16);
    w.ctr = c.take<unsigned long long>(8);
    w.vslot = c.take<int>(vcap);
    w.fslot = c.take<int>(fcap);
    w.rep = c.take<int>(V);
    w.wfa = c.take<int>(F * 3);
    w.keep = c.take<int>(F);
    w.kstart = c.take<int>(F + 1);
    return c.done(w);
}
struct RpOrientWs {                              // d, e: on the F0 surviving faces
    int *wf, *src, *fmn, *fmx, *adj, *link, *badroot;
    unsigned char *par, *flipped, *unor;
    int *vtx;                                    // [5][V] outc, inc, nxt, blocked, addc (zeroed as one)
    int *bparent, *addstart;
    EdgeTable t;
    char *base;
    size_t bytes;
};
RpOrientWs carve_orient(char *base, size_t V, size_t F0, unsigned ecap) {
    Carver c{base};
    RpOrientWs w;
    w.wf = c.take<int>(F0 * 3);
    w.src = c.take<int>(F0);
    w.t = carve_edges(c, ecap);
    w.fmn = c.take<int>(ecap);
    w.fmx = c.take<int>(ecap);
    w.adj = c.take<int>(F0 * 3);
    w.par = c.take<unsigned char>(F0 * 3);
    w.link = c.take<int>(F0);
    w.badroot = c.take<int>(F0);
    w.flipped = c.take<unsigned char>(F0);
    w.unor = c.take<unsigned char>(F0);
    w.vtx = c.take<int>(V * 5);
    w.bparent = c.take<int>(V);
    w.addstart = c.take<int>(V + 1);
    return c.done(w);
}
struct RpFillWs {                                // f, g: on the F1 faces of the filled mesh
    int *wf, *fmn, *fmx, *adj, *parent, *flag, *rstart, *used, *vstart, *onb;
    EdgeTable t;
    char *base;
    size_t bytes;
};
RpFillWs carve_fill(char *base, size_t V, size_t F1, unsigned ecap) {
    Carver c{base};
    RpFillWs w;
    w.wf = c.take<int>(F1 * 3);
    w.t = carve_edges(c, ecap);
    w.fmn = c.take<int>(ecap);
    w.fmx = c.take<int>(ecap);
    w.adj = c.take<int>(F1 * 3);
    w.parent = c.take<int>(F1);
    w.flag = c.take<int>(F1);
    w.rstart = c.take<int>(F1 + 1);
    w.used = c.take<int>(V);
    w.vstart = c.take<int>(V + 1);
    w.onb = c.take<int>(V);
    return c.done(w);
}
struct RpVolumeWs {                              // f: the closed components' own volumes
    double *tri, *vol;
    int *roots;
    char *base;
    size_t bytes;
};
RpVolumeWs carve_volume(char *base, size_t F1, size_t n_closed) {
    Carver c{base};
    RpVolumeWs w;
    w.tri = c.take<double>(F1 * 9);
    w.roots = c.take<int>(n_closed);
    w.vol = c.take<double>(n_closed);
    return c.done(w);
}

}  // namespace

extern "C" int p2s_mesh_repair(const float *verts_dev, int64_t n_verts, const int32_t *faces_dev, int64_t n_faces, int max_hole_edges,
                               float *verts_out_dev, int64_t cap_verts, int32_t *faces_out_dev, int32_t *face_src_out_dev,
                               int64_t cap_faces, int64_t *report_host, int device, void *stream) {
    static const char *const who = "p2s_mesh_repair";
    if (!report_host || n_verts < 0 || n_faces < 0 || n_verts > (1ll << 27) || n_faces > (1ll << 25) || max_hole_edges < 0 ||
        max_hole_edges > 64 || cap_verts < 0 || cap_faces < 0 || (n_verts > 0 && !verts_dev) || (n_faces > 0 && !faces_dev) ||
        (cap_verts > 0 && !verts_out_dev) || (cap_faces > 0 && (!faces_out_dev || !face_src_out_dev))) {
        p2s_set_error("p2s_mesh_repair: bad argument (vertices <= 2^27, faces <= 2^25, max_hole_edges in 0..64)");
        return P2S_EINVAL;
    }
    if (int rc = select_device(who, device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const long long V = n_verts, F = n_faces;
    const int K = max_hole_edges;
    long long rep_out[16] = {};
    rep_out[0] = V | (F << 32);
    auto publish = [&]() {
        for (int k = 0; k < 16; ++k) report_host[k] = rep_out[k];
    };
    PoolScratch pool(device, s);
    int rc;

    // ---- a. validate
    const unsigned vcap = rp_table_cap(V), fcap = rp_table_cap(F);
    const RpWeldWs A = pool.carve([&](char *b) { return carve_weld(b, (size_t)V, (size_t)F, vcap, fcap); });
    if (!A.base) return dev_oom(who, s);
    int *ctl = A.ctl;
    unsigned long long *ctr = A.ctr, hc[8] = {};
    if (V > 0 || F > 0) {
        float box[6];
        if ((rc = mesh_validate(who, verts_dev, V, faces_dev, F, ctl, box, s)) != P2S_OK) return rc;
    }
    if (F == 0) {                                                    // nothing references a vertex: the empty mesh
        rep_out[15] = 1 | 2;                                         // no edge at all; no volume
        publish();
        return P2S_OK;
    }

    // ---- b, c. weld, collapsed and duplicate faces
    DEV_CHECK(who, hipMemsetAsync(A.vslot, 0xff, (size_t)vcap * 4, s));
    DEV_CHECK(who, hipMemsetAsync(A.fslot, 0xff, (size_t)fcap * 4, s));
    DEV_CHECK(who, hipMemsetAsync(ctr, 0, MESH_COUNTERS, s));
    hipLaunchKernelGGL(p2s_rp_weld_insert_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, verts_dev, V, A.vslot, vcap - 1);
    hipLaunchKernelGGL(p2s_rp_weld_map_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, verts_dev, V, A.vslot, vcap - 1, A.rep, ctr + RP_WELDED);
    hipLaunchKernelGGL(p2s_rp_face_weld_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, faces_dev, F, A.rep, A.wfa, A.keep, ctr + RP_COLLAPSED);
    hipLaunchKernelGGL(p2s_rp_face_insert_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, A.wfa, F, A.keep, A.fslot, fcap - 1);
    hipLaunchKernelGGL(p2s_rp_face_keep_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, A.wfa, F, A.keep, A.fslot, fcap - 1, ctr + RP_DUPLICATE);
    hipLaunchKernelGGL(p2s_scan_kernel, dim3(1), dim3(1024), 0, s, A.keep, F, A.kstart);
    int hF0 = 0;
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipMemcpyAsync(&hF0, A.kstart + F, 4, hipMemcpyDeviceToHost, s));
    if ((rc = read_counters(who, ctr, hc, -1, nullptr, s)) != P2S_OK) return rc;
    const long long F0 = hF0;
    rep_out[3] = (long long)hc[RP_WELDED];
    rep_out[4] = (long long)hc[RP_COLLAPSED];
    rep_out[5] = (long long)hc[RP_DUPLICATE];
    if (F0 == 0) {
        rep_out[15] = 1 | 2;
        publish();
        return P2S_OK;
    }

    // ---- d. orient
    const RpOrientWs B = pool.carve([&](char *b) { return carve_orient(b, (size_t)V, (size_t)F0, rp_table_cap(3 * F0)); });
    if (!B.base) return dev_oom(who, s);
    DEV_CHECK(who, hipMemsetAsync(ctr, 0, MESH_COUNTERS, s));
    hipLaunchKernelGGL(p2s_rp_gather_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, verts_dev, A.wfa, F, A.keep, A.kstart, B.wf, B.src,
                       ctr + RP_DEGENERATE);
    if ((rc = build_edges(who, B.wf, F0, B.t, B.fmn, B.fmx, s)) != P2S_OK) return rc;
    hipLaunchKernelGGL(p2s_rp_adj_kernel, dim3(blocks(3 * F0, 256)), dim3(256), 0, s, B.wf, F0, B.t, B.fmn, B.fmx, B.adj, B.par);
    hipLaunchKernelGGL(p2s_rp_par_compress_kernel, dim3(blocks(F0, 256)), dim3(256), 0, s, B.link, F0, 1);
    rc = until_unchanged(who, "the orientation", 100000, ctl, s, [&](long long) {
        hipLaunchKernelGGL(p2s_rp_par_hook_kernel, dim3(blocks(F0, 256)), dim3(256), 0, s, B.adj, B.par, B.link, F0, ctl);
        hipLaunchKernelGGL(p2s_rp_par_compress_kernel, dim3(blocks(F0, 256)), dim3(256), 0, s, B.link, F0, 0);
    });
    if (rc != P2S_OK) return rc;
    DEV_CHECK(who, hipMemsetAsync(B.badroot, 0, (size_t)F0 * 4, s));
    hipLaunchKernelGGL(p2s_rp_par_check_kernel, dim3(blocks(F0, 256)), dim3(256), 0, s, B.adj, B.par, B.link, F0, B.badroot);
    hipLaunchKernelGGL(p2s_rp_par_apply_kernel, dim3(blocks(F0, 256)), dim3(256), 0, s, B.link, B.badroot, F0, B.wf, B.flipped, B.unor,
                       ctr + RP_FLIPPED);                            // and RP_UNORIENTABLE behind it

    // ---- e. holes, on the oriented faces
    if ((rc = build_edges(who, B.wf, F0, B.t, nullptr, nullptr, s)) != P2S_OK) return rc;
    int *outc = B.vtx, *inc = outc + V, *nxt = inc + V, *blocked = nxt + V, *addc = blocked + V;
    DEV_CHECK(who, hipMemsetAsync(B.vtx, 0, (size_t)V * 4 * 5, s));
    hipLaunchKernelGGL(p2s_rp_boundary_kernel, dim3(blocks(3 * F0, 256)), dim3(256), 0, s, B.wf, F0, B.t, B.unor, outc, inc, nxt, blocked);
    hipLaunchKernelGGL(p2s_rp_hole_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, V, K, outc, inc, nxt, blocked, addc, ctr + RP_HOLES);
    hipLaunchKernelGGL(p2s_scan_kernel, dim3(1), dim3(1024), 0, s, addc, V, B.addstart);
    int h_added = 0;
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipMemcpyAsync(&h_added, B.addstart + V, 4, hipMemcpyDeviceToHost, s));
    if ((rc = read_counters(who, ctr, hc, -1, nullptr, s)) != P2S_OK) return rc;
    rep_out[6] = (long long)hc[RP_DEGENERATE];
    rep_out[7] = (long long)hc[RP_FLIPPED];
    rep_out[9] = (long long)hc[RP_UNORIENTABLE];
    rep_out[11] = (long long)hc[RP_HOLES];
    rep_out[12] = h_added;
    const long long F1 = F0 + h_added;

    // ---- f. components of the filled mesh, inversion
    const unsigned ecap1 = rp_table_cap(3 * F1);
    const RpFillWs C = pool.carve([&](char *b) { return carve_fill(b, (size_t)V, (size_t)F1, ecap1); });
    if (!C.base) return dev_oom(who, s);
    DEV_CHECK(who, hipMemcpyAsync(C.wf, B.wf, (size_t)F0 * 12, hipMemcpyDeviceToDevice, s));
    if (h_added) hipLaunchKernelGGL(p2s_rp_hole_fill_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, V, nxt, addc, B.addstart, F0, C.wf);
    DEV_CHECK(who, hipMemsetAsync(ctr, 0, MESH_COUNTERS, s));
    if ((rc = build_edges(who, C.wf, F1, C.t, C.fmn, C.fmx, s)) != P2S_OK) return rc;
    hipLaunchKernelGGL(p2s_rp_edge_stats_kernel, dim3(blocks(ecap1, 256)), dim3(256), 0, s, C.t, ctr + RP_BOUNDARY);      // .. RP_INCONSISTENT
    hipLaunchKernelGGL(p2s_rp_adj_kernel, dim3(blocks(3 * F1, 256)), dim3(256), 0, s, C.wf, F1, C.t, C.fmn, C.fmx, C.adj, (unsigned char *)nullptr);
    hipLaunchKernelGGL(p2s_iota_kernel, dim3(blocks(F1, 256)), dim3(256), 0, s, C.parent, F1);
    hipLaunchKernelGGL(p2s_iota_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, B.bparent, V);
    rc = until_unchanged(who, "the connected components", 100000, ctl, s, [&](long long) {
        hipLaunchKernelGGL(p2s_md_cc_hook_kernel, dim3(blocks(F1, 256)), dim3(256), 0, s, C.adj, C.parent, F1, ctl);
        hipLaunchKernelGGL(p2s_uf_compress_kernel, dim3(blocks(F1, 256)), dim3(256), 0, s, C.parent, F1);
        hipLaunchKernelGGL(p2s_rp_bhook_kernel, dim3(blocks(3 * F1, 256)), dim3(256), 0, s, C.wf, F1, C.t, B.bparent, ctl);
        hipLaunchKernelGGL(p2s_uf_compress_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, B.bparent, V);
    });
    if (rc != P2S_OK) return rc;
    DEV_CHECK(who, hipMemsetAsync(C.flag, 0, (size_t)F1 * 4, s));
    DEV_CHECK(who, hipMemsetAsync(C.onb, 0, (size_t)V * 4, s));
    hipLaunchKernelGGL(p2s_rp_open_kernel, dim3(blocks(3 * F1, 256)), dim3(256), 0, s, C.wf, F1, C.t, C.parent, C.flag);
    hipLaunchKernelGGL(p2s_rp_bmark_kernel, dim3(blocks(3 * F1, 256)), dim3(256), 0, s, C.wf, F1, C.t, C.onb);
    hipLaunchKernelGGL(p2s_rp_bcount_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, B.bparent, C.onb, V, ctr + RP_BGROUPS);
    hipLaunchKernelGGL(p2s_md_cc_count_kernel, dim3(blocks(F1, 256)), dim3(256), 0, s, C.parent, F1, ctr + RP_COMPONENTS);
    hipLaunchKernelGGL(p2s_rp_roots_flag_kernel, dim3(blocks(F1, 256)), dim3(256), 0, s, C.parent, F1, C.flag);
    hipLaunchKernelGGL(p2s_scan_kernel, dim3(1), dim3(1024), 0, s, C.flag, F1, C.rstart);
    int n_closed = 0;
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipMemcpyAsync(&n_closed, C.rstart + F1, 4, hipMemcpyDeviceToHost, s));
    DEV_CHECK(who, hipStreamSynchronize(s));
    if (n_closed > 0) {
        const RpVolumeWs D = pool.carve([&](char *b) { return carve_volume(b, (size_t)F1, (size_t)n_closed); });
        if (!D.base) return dev_oom(who, s);
        hipLaunchKernelGGL(p2s_rp_roots_kernel, dim3(blocks(F1, 256)), dim3(256), 0, s, C.flag, C.rstart, F1, D.roots);
        hipLaunchKernelGGL(p2s_rp_tri_kernel, dim3(blocks(9 * F1, 256)), dim3(256), 0, s, verts_dev, C.wf, F1, D.tri);
        hipLaunchKernelGGL(p2s_md_comp_volume_kernel, dim3((unsigned)n_closed), dim3(1024), 0, s, D.tri, C.parent, F1, D.roots, D.vol);
        hipLaunchKernelGGL(p2s_rp_invert_kernel, dim3(blocks(F1, 256)), dim3(256), 0, s, C.parent, C.flag, C.rstart, D.vol, F1, C.wf,
                           ctr + RP_INVERTED);
    }
    // ---- g. compaction, h. report
    DEV_CHECK(who, hipMemsetAsync(C.used, 0, (size_t)V * 4, s));
    hipLaunchKernelGGL(p2s_rp_used_kernel, dim3(blocks(3 * F1, 256)), dim3(256), 0, s, C.wf, F1, C.used);
    hipLaunchKernelGGL(p2s_scan_kernel, dim3(1), dim3(1024), 0, s, C.used, V, C.vstart);
    hipLaunchKernelGGL(p2s_md_volume_kernel, dim3(1), dim3(1024), 0, s, verts_dev, C.wf, F1, (double *)(ctr + RP_VOLUME));
    int hV1 = 0;
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipMemcpyAsync(&hV1, C.vstart + V, 4, hipMemcpyDeviceToHost, s));
    if ((rc = read_counters(who, ctr, hc, -1, nullptr, s)) != P2S_OK) return rc;      // also: every block of `pool` is idle from here on
    double vol6;
    memcpy(&vol6, &hc[RP_VOLUME], 8);
    rep_out[1] = hV1;
    rep_out[2] = F1;
    rep_out[8] = (long long)hc[RP_COMPONENTS];
    rep_out[10] = (long long)hc[RP_INVERTED];
    rep_out[13] = (long long)hc[RP_BGROUPS];
    rep_out[14] = (long long)hc[RP_BOUNDARY] | ((long long)hc[RP_NONMANIFOLD] << 32);
    const int watertight = hc[RP_BOUNDARY] == 0 && hc[RP_NONMANIFOLD] == 0, consistent = hc[RP_INCONSISTENT] == 0;
    rep_out[15] = (watertight ? 1 : 0) | (consistent ? 2 : 0) | ((watertight && consistent && vol6 > 0.0) ? 4 : 0);
    publish();
    if (cap_verts < hV1 || cap_faces < F1) {
        p2s_set_error("p2s_mesh_repair: output buffers too small (%lld vertices and %lld faces needed, %lld and %lld given)", (long long)hV1,
                      F1, (long long)cap_verts, (long long)cap_faces);
        return P2S_EINVAL;
    }
    hipLaunchKernelGGL(p2s_rp_write_verts_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, verts_dev, V, C.used, C.vstart, verts_out_dev);
    hipLaunchKernelGGL(p2s_rp_write_faces_kernel, dim3(blocks(F1, 256)), dim3(256), 0, s, C.wf, B.src, F1, F0, C.vstart, faces_out_dev,
                       face_src_out_dev);
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipStreamSynchronize(s));
    return P2S_OK;
}

extern "C" int p2s_mesh_normalize(const float *verts_dev, int64_t n_verts, float *verts_out_dev, double *info_host, int device, void *stream) {
    static const char *const who = "p2s_mesh_normalize";
    if (!verts_dev || !verts_out_dev || n_verts < 1 || n_verts > (1ll << 27)) {
        p2s_set_error("p2s_mesh_normalize: bad argument (1 <= vertices <= 2^27)");
        return P2S_EINVAL;
    }
    if (int rc = select_device(who, device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    PoolScratch pool(device, s);
    int *ctl = pool.get<int>(64);
    if (!ctl) return dev_oom(who, s);
    float box[6];
    const int rc = mesh_validate(who, verts_dev, (long long)n_verts, (const int *)nullptr, 0ll, ctl, box, s);
    if (rc != P2S_OK) return rc;
    double c[3], ext = 0.0;
    bool flat = false;
    for (int k = 0; k < 3; ++k) {
        const double lo = box[k], hi = box[3 + k];
        c[k] = (lo + hi) / 2.0;
        ext = std::max(ext, hi - lo);
        flat = flat || !(hi - lo > 0.0);
    }
    if (flat) {
        p2s_set_error("p2s_mesh_normalize: the bounding box has a zero extent on an axis");
        return P2S_EFLAT;
    }
    const double sc = 1.0 / ext;
    hipLaunchKernelGGL(p2s_rp_normalize_kernel, dim3(blocks(3 * n_verts, 256)), dim3(256), 0, s, verts_dev, (long long)n_verts, c[0], c[1], c[2],
                       sc, verts_out_dev);
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipStreamSynchronize(s));
    if (info_host) {
        info_host[0] = c[0];
        info_host[1] = c[1];
        info_host[2] = c[2];
        info_host[3] = sc;
    }
    return P2S_OK;
}
