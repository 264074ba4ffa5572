// "next" row f-5: ground-truth signed distance of query points to a triangle mesh -- what reference source/sdf.py:318-348
// (get_signed_distance -> trimesh.proximity.signed_distance, in batches of 1000 because "3k queries on a mesh with 27k
// vertices ... take around 8 GB") computes on the host for make_dataset.py:447-474 (05_query_dist/<shape>.npy).
//
// Handle (p2s_trimesh_create): the triangles in float64 (trimesh computes in float64 after loading the float32 PLY), unit
// face normals, the face across every edge, angle-weighted vertex normals (Baerentzen & Aanaes 2005: the sign of
// n_feature . (p - c) with the pseudonormal of the closest FEATURE -- face normal, sum of the two face normals of an edge,
// angle-weighted sum at a vertex -- is the inside / outside sign of a closed mesh), `closed` (every undirected edge is
// traversed exactly once in each direction), the sign of the signed volume (an inward-oriented mesh is stored flipped, as
// p2s_marching_cubes does for fix_inversion), and the index: triangles binned by centroid into G^3 cells (counting sort),
// the AABB of every cell's triangles, and above them an implicit octree of AABBs (parent = union of its 8 children).
//   p2s_md_validate_kernel    indices in range, vertices finite, bounding box             (before anything dereferences)
//   p2s_md_edges_kernel       undirected edges into an open-addressing table: traversal counts and faces per direction
//   p2s_md_edge_check_kernel  edges that are not (once forward, once backward)
//   p2s_md_volume_kernel      signed volume (one workgroup, fixed order)
//   p2s_md_setup_kernel       float64 triangles, normals, neighbours, vertex normals, centroid cell
//   p2s_md_cc_hook_kernel / p2s_md_cc_compress_kernel / p2s_md_cc_count_kernel   connected components (union-find over neighbours)
//   p2s_md_scan_kernel / p2s_md_fill_kernel / p2s_md_nodes_init_kernel / p2s_md_nodes_up_kernel     the index
//   p2s_md_index_kernel       exact nearest triangle per query: depth-first descent, near child first, pruned by AABB bound
//   p2s_md_exhaustive_kernel  every query against every triangle (yardstick of the index, and for tiny meshes)
//   p2s_md_finalize_kernel    closest point, distance, pseudonormal sign, flag of the queries whose sign is not trusted
//   p2s_md_winding_kernel     generalised winding number (Jacobson et al. 2013) of a flagged query: one workgroup each
//   p2s_md_cell_sort_kernel / p2s_md_stri_kernel / p2s_md_moments_leaf_kernel   fixed triangle order per cell, node moments
//   p2s_md_wtree_kernel       the winding number of every query by a walk of the octree: far nodes as dipoles with a
//                             certified error bound, near leaf cells exactly (p2s_mesh_winding, p2s_mesh_distance signed_ 2)
//   p2s_md_wsign_kernel       sign of the distance from that winding number
// First-hit ray casting, the time-of-flight scan and the query points on the same handle: p2s_meshray.inl (end of file).
// Repair and normalisation of a raw mesh with the same edge table, components, scan and volume sums: p2s_meshrepair.inl.
//
// The pseudonormal sign holds for ONE closed surface that does not intersect itself.  A closed mesh of several connected
// components may be a union of overlapping solids (the reference's 00011084 is: 170 of its 2,000 GT queries lie just outside
// one component and inside another).  The winding number of such a mesh is the sum over its components, and each component
// is one closed surface: w = sum_k o_k [p inside component k], o_k the sign of the component's own signed volume, the
// bracket from the pseudonormal of the nearest feature OF THAT COMPONENT (p2s_md_comp_sign_kernel, one filtered nearest-
// triangle pass per component).  Inside iff |w| > 0.5, as for the winding number itself.  Up to 16 components; a mesh of
// more has every signed query decided by the winding number (exact, O(F) per query).
// Rules, stated once:
//  * ties between triangles at the same squared distance go to the smallest face id;
//  * a triangle whose |ab x ac|^2 is not above 2^-90 |ab|^2 |ac|^2 (zero area, or collinear to float64 rounding) is
//    measured as its three segments, never through the barycentric division, and has the normal 0: it adds nothing to a
//    pseudonormal and never yields a NaN;
//  * trimesh: positive inside, negative outside, a query with d <= 1e-8 (tol.merge) keeps its unsigned d.
// All arithmetic is float64 VALU with contraction off: the CPU model (tests/mesh_sdf_model.py) performs the same
// operations in the same association.
#include "p2s_common.h"
#include "p2s_internal.h"
#include <algorithm>
#include <cmath>
#include <cstring>

#pragma clang fp contract(off)

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

constexpr unsigned long long EDGE_EMPTY = ~0ull;
constexpr double FIX = 1099511627776.0;          // 2^40
constexpr double DEGENERATE_REL = 8.077935669463161e-28;   // 2^-90
// a face with a corner sine below 2^-20: its unit normal carries more than 3 * 2^-53 / 2^-20 < 2^-31 of error, which the
// trust bound of the sign assumes -- queries whose pseudonormal involves such a face go to the winding number
constexpr double SLIVER_REL = 9.094947017729282e-13;       // 2^-40 (on sin^2)

__device__ __forceinline__ int f2o(float f) {      // order-preserving float <-> int (its own inverse)
    const int i = __float_as_int(f);
    return i >= 0 ? i : i ^ 0x7fffffff;
}
__device__ __forceinline__ float o2f(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7fffffff); }

__device__ __forceinline__ double dot3(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void cross3(const double *a, const double *b, double *o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// closest point of the segment a-b; feature: 0 = inside the segment, 1 = a, 2 = b
__device__ __forceinline__ double seg_closest(const double *p, const double *a, const double *b, double *c, int *end) {
    double ab[3], ap[3], r[3];
    for (int k = 0; k < 3; ++k) {
        ab[k] = b[k] - a[k];
        ap[k] = p[k] - a[k];
    }
    const double t = dot3(ab, ap), l = dot3(ab, ab);
    if (t <= 0.0) {
        *end = 1;
        for (int k = 0; k < 3; ++k) c[k] = a[k];
    } else if (t >= l) {
        *end = 2;
        for (int k = 0; k < 3; ++k) c[k] = b[k];
    } else {
        *end = 0;
        const double v = t / l;
        for (int k = 0; k < 3; ++k) c[k] = a[k] + v * ab[k];
    }
    for (int k = 0; k < 3; ++k) r[k] = p[k] - c[k];
    return dot3(r, r);
}

// Ericson, Real-Time Collision Detection 5.1.5.  feature: 0 face, 1 / 2 / 3 edge ab / bc / ca, 4 / 5 / 6 vertex a / b / c
__device__ __forceinline__ double tri_closest(const double *p, const double *t, double *c, int *feat) {
    const double *A = t, *B = t + 3, *C = t + 6;
    double ab[3], ac[3], ap[3], n[3], r[3];
    for (int k = 0; k < 3; ++k) {
        ab[k] = B[k] - A[k];
        ac[k] = C[k] - A[k];
        ap[k] = p[k] - A[k];
    }
    cross3(ab, ac, n);
    if (!(dot3(n, n) > DEGENERATE_REL * (dot3(ab, ab) * dot3(ac, ac)))) {
        double c2[3];
        int e, e2;
        double best = seg_closest(p, A, B, c, &e);
        *feat = e == 0 ? 1 : 3 + e;                          // a = 4, b = 5
        double d = seg_closest(p, B, C, c2, &e2);
        if (d < best) {
            best = d;
            *feat = e2 == 0 ? 2 : 4 + e2;                    // b = 5, c = 6
            for (int k = 0; k < 3; ++k) c[k] = c2[k];
        }
        d = seg_closest(p, C, A, c2, &e2);
        if (d < best) {
            best = d;
            *feat = e2 == 0 ? 3 : (e2 == 1 ? 6 : 4);         // c = 6, a = 4
            for (int k = 0; k < 3; ++k) c[k] = c2[k];
        }
        return best;
    }
    const double d1 = dot3(ab, ap), d2 = dot3(ac, ap);
    double bp[3], cp[3];
    for (int k = 0; k < 3; ++k) {
        bp[k] = p[k] - B[k];
        cp[k] = p[k] - C[k];
    }
    const double d3 = dot3(ab, bp), d4 = dot3(ac, bp), d5 = dot3(ab, cp), d6 = dot3(ac, cp);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if (d1 <= 0.0 && d2 <= 0.0) {
        *feat = 4;
        for (int k = 0; k < 3; ++k) c[k] = A[k];
    } else if (d3 >= 0.0 && d4 <= d3) {
        *feat = 5;
        for (int k = 0; k < 3; ++k) c[k] = B[k];
    } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        *feat = 1;
        const double v = d1 / (d1 - d3);
        for (int k = 0; k < 3; ++k) c[k] = A[k] + v * ab[k];
    } else if (d6 >= 0.0 && d5 <= d6) {
        *feat = 6;
        for (int k = 0; k < 3; ++k) c[k] = C[k];
    } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        *feat = 3;
        const double w = d2 / (d2 - d6);
        for (int k = 0; k < 3; ++k) c[k] = A[k] + w * ac[k];
    } else if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
        *feat = 2;
        const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        for (int k = 0; k < 3; ++k) c[k] = B[k] + w * (C[k] - B[k]);
    } else {
        *feat = 0;
        const double den = 1.0 / ((va + vb) + vc);
        const double v = vb * den, w = vc * den;
        for (int k = 0; k < 3; ++k) c[k] = (A[k] + ab[k] * v) + ac[k] * w;
    }
    for (int k = 0; k < 3; ++k) r[k] = p[k] - c[k];
    return dot3(r, r);
}

__device__ __forceinline__ bool finite3(const double *p) {
    return fabs(p[0]) <= 1.0e300 && fabs(p[1]) <= 1.0e300 && fabs(p[2]) <= 1.0e300;      // false for NaN and inf
}

// ---------------------------------------------------------------------------------------------
// handle construction
// ---------------------------------------------------------------------------------------------
// ctl: [0] error bits (1 non-finite vertex, 2 index out of range), [1..3] ordered min, [4..6] ordered max
__global__ __launch_bounds__(256) void p2s_md_validate_kernel(const float *__restrict__ verts, long long V, const int *__restrict__ faces,
                                                              long long F, int *__restrict__ ctl) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    int err = 0;
    int mn[3] = {0x7f800000, 0x7f800000, 0x7f800000}, mx[3] = {(int)0x807fffff, (int)0x807fffff, (int)0x807fffff};
    if (i < V) {
        for (int k = 0; k < 3; ++k) {
            const float x = verts[3 * i + k];
            if (!(fabsf(x) <= 3.4028235e38f)) err |= 1;
            else mn[k] = mx[k] = f2o(x);
        }
    }
    if (i < F) {
        for (int k = 0; k < 3; ++k) {
            const int v = faces[3 * i + k];
            if (v < 0 || v >= V) err |= 2;
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        err |= __shfl_xor(err, d);
        for (int k = 0; k < 3; ++k) {
            mn[k] = min(mn[k], __shfl_xor(mn[k], d));
            mx[k] = max(mx[k], __shfl_xor(mx[k], d));
        }
    }
    if ((threadIdx.x & 63) == 0) {
        if (err) atomicOr(&ctl[0], err);
        for (int k = 0; k < 3; ++k) {
            atomicMin(&ctl[1 + k], mn[k]);
            atomicMax(&ctl[4 + k], mx[k]);
        }
    }
}

struct EdgeTable {
    unsigned long long *key;     // [cap]
    int *cnt;                    // [cap][2] traversals low -> high, high -> low
    int *face;                   // [cap][2] a face of each direction
    unsigned mask;
};
__device__ __forceinline__ unsigned edge_hash(unsigned long long k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    return (unsigned)k;
}
__device__ __forceinline__ unsigned long long edge_key(int a, int b) {
    return ((unsigned long long)(unsigned)min(a, b) << 32) | (unsigned)max(a, b);
}

__global__ __launch_bounds__(256) void p2s_md_edges_kernel(const int *__restrict__ faces, long long F, EdgeTable t) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= 3 * F) return;
    const long long f = i / 3;
    const int e = (int)(i - 3 * f);
    const int a = faces[3 * f + e], b = faces[3 * f + (e + 1) % 3];
    const unsigned long long key = edge_key(a, b);
    unsigned h = edge_hash(key) & t.mask;
    for (;;) {                                   // load factor <= 1/2: an empty slot exists
        const unsigned long long prev = atomicCAS(&t.key[h], EDGE_EMPTY, key);
        if (prev == EDGE_EMPTY || prev == key) break;
        h = (h + 1) & t.mask;
    }
    const int dir = a < b ? 0 : 1;
    atomicAdd(&t.cnt[2 * h + dir], 1);
    t.face[2 * h + dir] = (int)f;                // one writer on a closed mesh; any of them otherwise (sign is refused then)
}

__global__ __launch_bounds__(256) void p2s_md_edge_check_kernel(EdgeTable t, unsigned long long *__restrict__ bad) {
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i > t.mask) return;
    if (t.key[i] != EDGE_EMPTY && !(t.cnt[2 * i] == 1 && t.cnt[2 * i + 1] == 1)) atomicAdd(bad, 1ull);
}

// six times the signed volume: sum of a . (b x c), one workgroup in a fixed order
__global__ __launch_bounds__(1024) void p2s_md_volume_kernel(const float *__restrict__ verts, const int *__restrict__ faces, long long F,
                                                             double *__restrict__ out) {
    __shared__ double ws[16];
    const int tid = threadIdx.x;
    double sm = 0.0;
    for (long long f = tid; f < F; f += 1024) {
        double a[3], b[3], c[3], n[3];
        for (int k = 0; k < 3; ++k) {
            a[k] = verts[3 * (long long)faces[3 * f] + k];
            b[k] = verts[3 * (long long)faces[3 * f + 1] + k];
            c[k] = verts[3 * (long long)faces[3 * f + 2] + k];
        }
        cross3(b, c, n);
        sm += dot3(a, n);
    }
    for (int d = 32; d > 0; d >>= 1) sm += __shfl_xor(sm, d);
    if ((tid & 63) == 0) ws[tid >> 6] = sm;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int w = 0; w < 16; ++w) s += ws[w];
        out[0] = s;
    }
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

// connected components: union-find with hooking to the smaller root and full compression, repeated until nothing changes
__device__ __forceinline__ int cc_find(const int *parent, int x) {
    for (int p = parent[x]; p != x; p = parent[x]) x = p;          // parents only decrease: no cycles
    return x;
}
__global__ __launch_bounds__(256) void p2s_md_cc_hook_kernel(const int *__restrict__ adj, int *parent, long long F, int *changed) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    for (int e = 0; e < 3; ++e) {
        const int g = adj[3 * f + e];
        if (g < 0) continue;
        const int rf = cc_find(parent, (int)f), rg = cc_find(parent, g);
        if (rf != rg) {
            atomicMin(&parent[max(rf, rg)], min(rf, rg));
            *changed = 1;
        }
    }
}
__global__ __launch_bounds__(256) void p2s_md_cc_compress_kernel(int *parent, long long F, int init) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    parent[f] = init ? (int)f : cc_find(parent, (int)f);
}
__global__ __launch_bounds__(256) void p2s_md_cc_count_kernel(const int *__restrict__ parent, long long F, unsigned long long *count) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f < F && parent[f] == (int)f) atomicAdd(count, 1ull);
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
// six times the signed volume of component blockIdx.x as stored: one workgroup each, fixed order
__global__ __launch_bounds__(1024) void p2s_md_comp_volume_kernel(const double *__restrict__ tri, const int *__restrict__ comp, long long F,
                                                                  const int *__restrict__ roots, double *__restrict__ out) {
    __shared__ double ws[16];
    const int tid = threadIdx.x, root = roots[blockIdx.x];
    double sm = 0.0;
    for (long long f = tid; f < F; f += 1024) {
        if (comp[f] != root) continue;
        double n[3];
        cross3(tri + 9 * f + 3, tri + 9 * f + 6, n);
        sm += dot3(tri + 9 * f, n);
    }
    for (int d = 32; d > 0; d >>= 1) sm += __shfl_xor(sm, d);
    if ((tid & 63) == 0) ws[tid >> 6] = sm;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int w = 0; w < 16; ++w) s += ws[w];
        out[blockIdx.x] = s;
    }
}

// exclusive scan of count [n] into start [n + 1] (one workgroup, chunks of 1024)
__global__ __launch_bounds__(1024) void p2s_md_scan_kernel(const int *__restrict__ count, long long n, int *__restrict__ start) {
    __shared__ int ws[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;
    for (long long b0 = 0; b0 < n; b0 += 1024) {
        const long long i = b0 + tid;
        const int c = i < n ? count[i] : 0;
        int v = c;
        for (int d = 1; d < 64; d <<= 1) {
            const int u = __shfl_up(v, d);
            if (lane >= d) v += u;
        }
        if (lane == 63) ws[wave] = v;
        __syncthreads();
        int base = carry, tot = 0;
        for (int w = 0; w < 16; ++w) {
            if (w < wave) base += ws[w];
            tot += ws[w];
        }
        if (i < n) start[i] = base + v - c;
        carry += tot;
        __syncthreads();
    }
    if (tid == 0) start[n] = carry;
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

// ---------------------------------------------------------------------------------------------
// queries
// ---------------------------------------------------------------------------------------------
struct IndexDev {
    const int *nodes;
    const int *cell_start;
    const int *sface;
    const double *stri;
    const int *scomp;
    int comp;            // >= 0: only the triangles of this component
    float lo[3], cell;
    int G, L;
    double scale;
};

__device__ __forceinline__ double aabb_bound(const int *__restrict__ node, const double *p) {
    double s = 0.0;
    for (int k = 0; k < 3; ++k) {
        const double lo = o2f(node[k]), hi = o2f(node[3 + k]);
        const double d = fmax(fmax(lo - p[k], p[k] - hi), 0.0);
        s += d * d;
    }
    return s;            // +inf for an empty node
}

// Exact nearest triangle.  A node is skipped only if the squared distance to its AABB exceeds
//     best + 2 E sqrt(best) + E^2,   E = 2^-32 max(|mesh|, |p|)
// i.e. its box lies more than E beyond the best DISTANCE: E covers the rounding of tri_closest (the closest point carries a
// few ulp of the coordinate magnitude, 2^-52) with 20 bits to spare, so a triangle whose computed d^2 would tie or beat the
// best is never skipped and the result equals the exhaustive kernel's bit for bit.
__global__ __launch_bounds__(64) void p2s_md_index_kernel(IndexDev ix, const float *__restrict__ q, long long n, int *__restrict__ best_face,
                                                          unsigned long long *__restrict__ tests_total) {
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    unsigned long long tests = 0;
    if (i < n) {
        const double p[3] = {(double)q[3 * i], (double)q[3 * i + 1], (double)q[3 * i + 2]};
        int bestf = -1;
        if (finite3(p)) {
            const double E = fmax(ix.scale, fmax(fabs(p[0]), fmax(fabs(p[1]), fabs(p[2])))) * 2.3283064365386963e-10;
            double best = INFINITY, thresh = INFINITY;
            int stack[64];
            int sp = 0;
            stack[sp++] = 0;
            while (sp > 0) {
                const int node = stack[--sp];
                const int l = node >> 27, lin = node & 0x7ffffff;
                const long long off = ((1ll << (3 * l)) - 1) / 7;
                const double lb = aabb_bound(ix.nodes + 6 * (off + lin), p);
                if (lb > thresh || lb == INFINITY) continue;
                if (l == ix.L) {
                    const int t1 = ix.cell_start[lin + 1];
                    for (int t = ix.cell_start[lin]; t < t1; ++t) {
                        if (ix.comp >= 0 && ix.scomp[t] != ix.comp) continue;
                        double c[3];
                        int feat;
                        const double d2 = tri_closest(p, ix.stri + 9 * (long long)t, c, &feat);
                        const int f = ix.sface[t];
                        ++tests;
                        if (d2 < best || (d2 == best && f < bestf)) {
                            best = d2;
                            bestf = f;
                            thresh = (best + 2.0 * E * sqrt(best)) + E * E;
                        }
                    }
                } else {
                    const int nn = 1 << l;
                    const int z = lin & (nn - 1), y = (lin >> l) & (nn - 1), x = lin >> (2 * l);
                    const int xyz[3] = {x, y, z};
                    const double half = (double)ix.cell * (double)(1 << (ix.L - l - 1));     // child size at level l + 1
                    int m = 0;                                                            // the child octant p lies towards
                    for (int k = 0; k < 3; ++k) m = (m << 1) | (p[k] > (double)ix.lo[k] + (2 * xyz[k] + 1) * half ? 1 : 0);
                    const long long coff = ((1ll << (3 * (l + 1))) - 1) / 7;
                    for (int j = 7; j >= 0; --j) {           // pushed far to near: the near child is popped first
                        const int c = j ^ m;
                        const int clin = ((2 * x + (c >> 2)) * (2 * nn) + (2 * y + ((c >> 1) & 1))) * (2 * nn) + (2 * z + (c & 1));
                        const double cb = aabb_bound(ix.nodes + 6 * (coff + clin), p);
                        if (cb > thresh || cb == INFINITY) continue;
                        if (sp < 64) stack[sp++] = ((l + 1) << 27) | clin;      // at most 7 L + 8 <= 57 entries (L <= 7)
                    }
                }
            }
        }
        best_face[i] = bestf;
    }
    for (int d = 32; d > 0; d >>= 1) tests += __shfl_xor(tests, d);
    if ((threadIdx.x & 63) == 0 && tests) atomicAdd(tests_total, tests);
}

// every query against the faces [y * per, (y + 1) * per): part_d2 / part_f [gridDim.y][n]
constexpr int EX_TILE = 128;
__global__ __launch_bounds__(256) void p2s_md_exhaustive_kernel(const double *__restrict__ tri, long long F, long long per,
                                                                const float *__restrict__ q, long long n, double *__restrict__ part_d2,
                                                                int *__restrict__ part_f, const int *__restrict__ comp_of, int comp) {
    __shared__ double tile[EX_TILE * 9];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long f0 = (long long)blockIdx.y * per, f1 = min(F, f0 + per);
    double p[3] = {0.0, 0.0, 0.0};
    bool live = false;
    if (i < n) {
        for (int k = 0; k < 3; ++k) p[k] = (double)q[3 * i + k];
        live = finite3(p);
    }
    double best = INFINITY;
    int bestf = -1;
    for (long long b0 = f0; b0 < f1; b0 += EX_TILE) {
        const int lim = (int)min((long long)EX_TILE, f1 - b0);
        for (int k = threadIdx.x; k < lim * 9; k += 256) tile[k] = tri[9 * b0 + k];
        __syncthreads();
        if (live) {
            for (int t = 0; t < lim; ++t) {
                if (comp >= 0 && comp_of[b0 + t] != comp) continue;
                double c[3];
                int feat;
                const double d2 = tri_closest(p, tile + 9 * t, c, &feat);
                if (d2 < best) {                 // ascending face ids: the smallest id keeps a tie
                    best = d2;
                    bestf = (int)(b0 + t);
                }
            }
        }
        __syncthreads();
    }
    if (i < n) {
        part_d2[(long long)blockIdx.y * n + i] = best;
        part_f[(long long)blockIdx.y * n + i] = bestf;
    }
}

struct FinalArgs {
    const double *tri, *fn;
    const int *fidx, *adj;
    const long long *vn;
    const unsigned char *fbad;
    const int *vbad;
    const float *q;
    long long n;
    const int *best_face;          // index method
    const double *part_d2;         // exhaustive method: [parts][n]
    const int *part_f;
    int parts;
    int signed_;
    int all_winding;               // more than 16 components: every sign from the winding number
    int *wsum, *bad;               // 2..16 components: [n] sum of the components' winding numbers, untrusted flag
    int orient;
    double scale;
    double *dist;
    int *face;
    double *closest;
    int *flagged;                  // [n] list of the queries whose sign the winding number decides
    unsigned long long *n_flagged;
};

// Sign of a closed mesh: outside iff n . (p - c) > 0 with the pseudonormal n of the closest feature.  The dot product is not
// trusted when
//     |n . (p - c)| <= 2^-30 W d + 2^-45 |n| s
// W = 1 (face), 2 (edge), the sum of the incident angles (vertex) = the largest |n| possible, d = |p - c|,
// s = max(|mesh|, |p|).  First term: a unit face normal of a triangle whose corner sines are above 2^-20 (any other face,
// zero-area ones included, makes the query untrusted outright: fbad / vbad) carries at most
// 3 * 2^-53 / 2^-20 < 2^-31 of error per component, the fixed-point vertex sums 2^-41 per contribution; second term: the
// closest point carries a few ulp (2^-52) of the coordinate magnitude.  Both from the number format, none from data.
__device__ __forceinline__ int final_face(const FinalArgs &a, long long i) {
    if (a.parts == 0) return a.best_face[i];
    int f = -1;
    double best = INFINITY;
    for (int y = 0; y < a.parts; ++y) {
        const double d2 = a.part_d2[(long long)y * a.n + i];
        if (d2 < best) {
            best = d2;
            f = a.part_f[(long long)y * a.n + i];
        }
    }
    return f;
}
// n_feature . (p - c) and the bound below which it is not trusted
__device__ __forceinline__ double pseudo_dot(const FinalArgs &a, long long f, int feat, const double *p, const double *c, double d,
                                             double *bound) {
    double n[3], W;
    bool untrusted = a.fbad[f] != 0;               // a zero-area or sliver face takes part in the pseudonormal
    if (feat == 0) {
        for (int k = 0; k < 3; ++k) n[k] = a.fn[3 * f + k];
        W = 1.0;
    } else if (feat <= 3) {
        const int g = a.adj[3 * f + feat - 1];
        for (int k = 0; k < 3; ++k) n[k] = a.fn[3 * f + k] + (g >= 0 ? a.fn[3 * (long long)g + k] : 0.0);
        W = 2.0;
        untrusted = untrusted || g < 0 || a.fbad[g] != 0;
    } else {
        const long long v = a.fidx[3 * f + feat - 4];
        for (int k = 0; k < 3; ++k) n[k] = (double)a.vn[4 * v + k] / FIX;
        W = (double)a.vn[4 * v + 3] / FIX;
        untrusted = untrusted || a.vbad[v] != 0;
    }
    const double r[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
    const double s = fmax(a.scale, fmax(fabs(p[0]), fmax(fabs(p[1]), fabs(p[2]))));
    *bound = untrusted ? INFINITY : 9.313225746154785e-10 * (W * d) + 2.842170943040401e-14 * (sqrt(dot3(n, n)) * s);
    return dot3(n, r);
}

__global__ __launch_bounds__(256) void p2s_md_finalize_kernel(FinalArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const int f = final_face(a, i);
    if (a.face) a.face[i] = f;
    if (a.wsum) {                                  // several components: the signs follow (p2s_md_comp_sign_kernel)
        a.wsum[i] = 0;
        a.bad[i] = 0;
    }
    if (f < 0) {                                   // non-finite query
        a.dist[i] = NAN;
        if (a.closest)
            for (int k = 0; k < 3; ++k) a.closest[3 * i + k] = NAN;
        return;
    }
    const double p[3] = {(double)a.q[3 * i], (double)a.q[3 * i + 1], (double)a.q[3 * i + 2]};
    double c[3];
    int feat;
    const double d = sqrt(tri_closest(p, a.tri + 9 * (long long)f, c, &feat));
    if (a.closest)
        for (int k = 0; k < 3; ++k) a.closest[3 * i + k] = c[k];
    if (!a.signed_ || d <= 1.0e-8 || a.wsum) {
        a.dist[i] = d;
        return;
    }
    double bound;
    const double dt = pseudo_dot(a, f, feat, p, c, d, &bound);
    if (a.all_winding || !(fabs(dt) > bound)) {
        a.dist[i] = d;
        a.flagged[atomicAdd(a.n_flagged, 1ull)] = (int)i;
        return;
    }
    a.dist[i] = dt > 0.0 ? -d : d;
}

// one component (a.orient = the sign of its own volume as stored): its nearest face is in best_face / the parts;
// wsum += orient [p inside the component]; bad: the dot product is not trusted, or p lies on the component (d_k <= 1e-8)
__global__ __launch_bounds__(256) void p2s_md_comp_sign_kernel(FinalArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const int f = final_face(a, i);
    if (f < 0) return;
    const double p[3] = {(double)a.q[3 * i], (double)a.q[3 * i + 1], (double)a.q[3 * i + 2]};
    double c[3], bound;
    int feat;
    const double d = sqrt(tri_closest(p, a.tri + 9 * (long long)f, c, &feat));
    const double dt = pseudo_dot(a, f, feat, p, c, d, &bound);
    if (d <= 1.0e-8 || !(fabs(dt) > bound)) a.bad[i] = 1;
    else if (dt * a.orient < 0.0) a.wsum[i] += a.orient;
}
// inside iff |w| > 0.5; the queries with an untrusted component go to the winding number itself
__global__ __launch_bounds__(256) void p2s_md_comp_apply_kernel(FinalArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const double d = a.dist[i];
    if (!(d > 1.0e-8)) return;                     // tol.merge, or NaN
    if (a.bad[i]) a.flagged[atomicAdd(a.n_flagged, 1ull)] = (int)i;
    else a.dist[i] = a.wsum[i] != 0 ? d : -d;
}

// generalised winding number w(p) = sum over faces of 2 atan2(a . (b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|) / 4 pi
// (a, b, c the corners minus p; van Oosterom & Strackee 1983); inside iff |w| > 0.5.
// The atan2 of one triangle t [9] (half its signed solid angle): the one place it is computed.
__device__ __forceinline__ double winding_term(const double *__restrict__ t, const double *p) {
    double a[3], b[3], c[3], x[3];
    for (int k = 0; k < 3; ++k) {
        a[k] = t[k] - p[k];
        b[k] = t[3 + k] - p[k];
        c[k] = t[6 + k] - p[k];
    }
    const double la = sqrt(dot3(a, a)), lb = sqrt(dot3(b, b)), lc = sqrt(dot3(c, c));
    cross3(b, c, x);
    const double num = dot3(a, x);
    const double den = ((la * lb * lc + dot3(a, b) * lc) + dot3(b, c) * la) + dot3(c, a) * lb;
    return atan2(num, den);
}

// The exact sum, one workgroup per query: query flagged[blockIdx.x], or blockIdx.x itself without a list.  With `dist` the
// sign of dist[i] is set from it; with `w_out` the value is written (its bound err_out[i], if asked for, is 0: this IS the
// yardstick).  A non-finite query gives NaN.
__global__ __launch_bounds__(256) void p2s_md_winding_kernel(const double *__restrict__ tri, long long F, const float *__restrict__ q,
                                                             const int *__restrict__ flagged, double *__restrict__ dist,
                                                             double *__restrict__ w_out, double *__restrict__ err_out) {
    __shared__ double ws[4];
    const long long i = flagged ? (long long)flagged[blockIdx.x] : (long long)blockIdx.x;
    const double p[3] = {(double)q[3 * i], (double)q[3 * i + 1], (double)q[3 * i + 2]};
    double sm = 0.0;
    for (long long f = threadIdx.x; f < F; f += 256) sm += winding_term(tri + 9 * f, p);
    for (int d = 32; d > 0; d >>= 1) sm += __shfl_xor(sm, d);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = sm;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double w = finite3(p) ? (((ws[0] + ws[1]) + ws[2]) + ws[3]) / 6.283185307179586 : NAN;
        if (dist) {
            const double d = fabs(dist[i]);
            dist[i] = fabs(w) > 0.5 ? d : -d;
        }
        if (w_out) w_out[i] = w;
        if (err_out) err_out[i] = finite3(p) ? 0.0 : NAN;
    }
}

// ---------------------------------------------------------------------------------------------
// hierarchical winding number
// ---------------------------------------------------------------------------------------------
// One query per lane walks the octree depth first.  A node with box centre c, half-diagonal r and moments N (sum of the
// area vectors) and A (sum of the areas) may stand for all its triangles as ONE dipole
//     w_node ~ N . (c - p) / (4 pi d^3),   d = |c - p|.
// Error.  The exact contribution of a triangle T with unit normal n and area a is the integral over T of
// K(x) = n . (x - p) / (4 pi |x - p|^3), and a K(c) is its share of the dipole.  4 pi |y|^3 grad K = n - 3 (n . y^) y^ (y = x - p)
// has the squared norm 1 + 3 cos^2 <= 4, so |grad K| <= 1 / (2 pi |y|^3).  Every point of the box lies within r of c, the
// segment from c to it stays at least d - r from p, hence |K(x) - K(c)| <= r / (2 pi (d - r)^3) and, summed with the areas,
//     |w_node - dipole| <= A r / (2 pi (d - r)^3) =: bound.
// A node is taken as a dipole only if  tau > 0,  d >= 2 r,  A <= 2 pi d^2  and  bound <= tau A / A_root;  otherwise it is
// opened: its non-empty children are pushed, or, for a leaf cell, its triangles are added exactly (winding_term, in sface
// order).  The accepted nodes are disjoint, so their areas sum to at most A_root and their bounds to at most tau.
// d >= 2 r and A <= 2 pi d^2 cost nothing where the budget rule holds (it asks for far more) and are what the rounding term
// below stands on: |dipole| <= A / (4 pi d^2) <= 1/2 like every exact term, and seen from p the corners of a triangle of the
// node lie within 60 degrees of each other, so the denominator of its atan2 is above 2.5 |a||b||c| and the exhaustive
// kernel's own term is within 4 ulp of the true solid angle.
// Outputs: w~ = (sum of the atan2 terms) / 2 pi + sum of the dipoles, and
//     eps = sum of the accepted bounds + 2^-53 F (K + F / 256 + 32) + D 2^-46 / pi,
// K = terms added for this query (triangles + dipoles), F = faces, D = degenerate faces of the mesh.  The second term
// covers, with u = 2^-53 and every term at most 1/2 in magnitude: this kernel's sequential sum (K u K / 2), the exhaustive
// kernel's sum of F terms in 256 strided partial sums and a reduction ((F / 256 + 10) u F / 2), the rounding of the moments
// (the cross products carry 4 u |ab||ac| <= 16 u r^2 each and the sums of at most F terms F u A, against 4 pi d^2: below
// 2 F u over all accepted nodes), the 4 ulp per triangle inside an accepted node (4 F u / 2 pi), the dipole's own arithmetic
// (2 u each) and the rounding of the bound sum (K u / 4): together below half of it.  The third: a degenerate face is not
// in the moments; its area is at most 2^-46 |ab||ac| <= 2^-46 (2 r)^2, so for d >= 2 r it contributes at most
// 2^-46 r^2 / (pi (d - r)^2) <= 2^-46 / pi.  The query is decided when | |w~| - 0.5 | > eps: inside / outside is then what the
// exact sum gives.  r is rounded up by 2^-30 (c and r come from float64 arithmetic on the float32 box).
// Stack: a pop of an inner node pushes at most 8, so the depth is at most 7 L + 1 = 50 for L <= MD_MAX_L = 7: one LDS
// column of WT_STACK = 52 entries per lane, 13 KiB per workgroup (the scheme of p2s_mr_index_kernel).  A push beyond it
// cannot happen; if it ever did the call fails (ctr[3]) instead of dropping a node.
constexpr int MD_MAX_L = 7;
constexpr int WT_STACK = 52;
static_assert(WT_STACK >= 7 * MD_MAX_L + 1, "depth-first stack: 7 entries stay per opened level, plus the 8th child of the last");
static_assert(3 * MD_MAX_L + 3 <= 27, "a node id is (level << 27) | linear index");

struct WTreeDev {
    const int *nodes;
    const double *mom;
    const int *cell_start;
    const double *stri;
    int L;
    long long F, n_degenerate;
    double tau;
};

__device__ __forceinline__ double wtree_rounding(double F, double K, double D) {
    return 1.1102230246251565e-16 * (F * ((K + F * 0.00390625) + 32.0)) + D * 4.523328512768113e-15;      // 2^-53, 2^-46 / pi
}

// ctr: [0] nodes accepted, [1] triangles evaluated, [2] undecided queries (with `undecided`: their list), [3] stack overflow
__global__ __launch_bounds__(64) void p2s_md_wtree_kernel(WTreeDev ix, const float *__restrict__ q, long long n, double *__restrict__ w_out,
                                                          double *__restrict__ err_out, int *__restrict__ undecided,
                                                          unsigned long long *__restrict__ ctr) {
    __shared__ int stack[WT_STACK * 64];
    const int lane = threadIdx.x;
    const long long i = (long long)blockIdx.x * 64 + lane;
    unsigned long long accepted = 0, tris = 0;
    if (i < n) {
        const double p[3] = {(double)q[3 * i], (double)q[3 * i + 1], (double)q[3 * i + 2]};
        if (!finite3(p)) {
            w_out[i] = NAN;
            if (err_out) err_out[i] = NAN;
        } else {
            const double a_root = ix.mom[3];
            double sa = 0.0, sd = 0.0, sb = 0.0;
            int sp = 0;
            stack[(sp++) * 64 + lane] = 0;
            while (sp > 0) {
                const int node = stack[(--sp) * 64 + lane];
                const int l = node >> 27, lin = node & 0x7ffffff;
                const long long at = ((1ll << (3 * l)) - 1) / 7 + lin;
                const int *bx = ix.nodes + 6 * at;
                const double *mo = ix.mom + 4 * at;
                double cp[3], e[3];
                for (int k = 0; k < 3; ++k) {
                    const double lo = o2f(bx[k]), hi = o2f(bx[3 + k]);
                    cp[k] = 0.5 * (lo + hi) - p[k];
                    e[k] = hi - lo;
                }
                const double r = (0.5 * sqrt(dot3(e, e))) * 1.0000000009313226, d = sqrt(dot3(cp, cp)), A = mo[3];
                if (ix.tau > 0.0 && d >= 2.0 * r && A <= 6.283185307179586 * (d * d)) {
                    const double g = d - r, g3 = g * g * g;
                    const double bound = (A * r) / (6.283185307179586 * g3);
                    if (g3 > 0.0 && bound * a_root <= ix.tau * A) {
                        sd += dot3(mo, cp) / (12.566370614359172 * (d * d * d));
                        sb += bound;
                        ++accepted;
                        continue;
                    }
                }
                if (l == ix.L) {
                    const int t1 = ix.cell_start[lin + 1];
                    for (int t = ix.cell_start[lin]; t < t1; ++t) {
                        sa += winding_term(ix.stri + 9 * (long long)t, p);
                        ++tris;
                    }
                } else {
                    const int nn = 1 << l;
                    const int z = lin & (nn - 1), y = (lin >> l) & (nn - 1), x = lin >> (2 * l);
                    const long long coff = ((1ll << (3 * (l + 1))) - 1) / 7;
                    for (int c = 7; c >= 0; --c) {           // child 0 is popped first: a fixed order
                        const int clin = ((2 * x + (c >> 2)) * (2 * nn) + (2 * y + ((c >> 1) & 1))) * (2 * nn) + (2 * z + (c & 1));
                        const int *cb = ix.nodes + 6 * (coff + clin);
                        if (cb[0] > cb[3]) continue;         // empty: no triangle, nothing to add
                        if (sp < WT_STACK) stack[(sp++) * 64 + lane] = ((l + 1) << 27) | clin;
                        else atomicOr(ctr + 3, 1ull);
                    }
                }
            }
            const double w = sa / 6.283185307179586 + sd;
            const double eps = sb + wtree_rounding((double)ix.F, (double)(accepted + tris), (double)ix.n_degenerate);
            w_out[i] = w;
            if (err_out) err_out[i] = eps;
            if (undecided && !(fabs(fabs(w) - 0.5) > eps)) undecided[atomicAdd(ctr + 2, 1ull)] = (int)i;
        }
    }
    for (int s = 32; s > 0; s >>= 1) {
        accepted += __shfl_xor(accepted, s);
        tris += __shfl_xor(tris, s);
    }
    if (lane == 0) {
        if (accepted) atomicAdd(ctr, accepted);
        if (tris) atomicAdd(ctr + 1, tris);
    }
}

// signed_ == 2: the sign of every distance from the winding number, inside iff |w| > 0.5; d <= 1e-8 (tol.merge) and NaN stay;
// an undecided query goes to the exact sum (p2s_md_winding_kernel)
__global__ __launch_bounds__(256) void p2s_md_wsign_kernel(const double *__restrict__ w, const double *__restrict__ err, long long n,
                                                           double *__restrict__ dist, int *__restrict__ flagged,
                                                           unsigned long long *__restrict__ n_flagged) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double d = dist[i];
    if (!(d > 1.0e-8)) return;
    if (!(fabs(fabs(w[i]) - 0.5) > err[i])) flagged[atomicAdd(n_flagged, 1ull)] = (int)i;
    else dist[i] = fabs(w[i]) > 0.5 ? d : -d;
}

unsigned blocks(long long n, int per) { return (unsigned)std::max<long long>(1, (n + per - 1) / per); }

constexpr double WINDING_TAU_DEFAULT = 0.0009765625;       // 2^-10

// ctr [4] as p2s_md_wtree_kernel takes it (zeroed by the caller)
void launch_wtree(const p2s_trimesh_s *m, const float *q, long long n, double tau, double *w, double *err, int *undecided,
                  unsigned long long *ctr, hipStream_t s) {
    WTreeDev ix;
    ix.nodes = m->nodes;
    ix.mom = m->mom;
    ix.cell_start = m->cell_start;
    ix.stri = m->stri;
    ix.L = m->L;
    ix.F = m->F;
    ix.n_degenerate = m->n_degenerate;
    ix.tau = tau;
    hipLaunchKernelGGL(p2s_md_wtree_kernel, dim3(blocks(n, 64)), dim3(64), 0, s, ix, q, n, w, err, undecided, ctr);
}

}  // namespace

extern "C" int p2s_trimesh_destroy(p2s_trimesh_t m) {
    if (!m) return P2S_OK;
    (void)hipSetDevice(m->device);
    p2s_pool_free(m->device, m->arena);
    delete m;
    return P2S_OK;
}

extern "C" int p2s_trimesh_create(const float *verts_dev, int64_t n_verts, const int32_t *faces_dev, int64_t n_faces, int device,
                                  void *stream, p2s_trimesh_t *out) {
    if (out) *out = nullptr;
    if (!verts_dev || !faces_dev || !out || n_verts < 1 || n_faces < 1 || n_verts > (1ll << 27) || n_faces > (1ll << 27)) {
        p2s_set_error("p2s_trimesh_create: bad argument (1 <= vertices, faces <= 2^27)");
        return P2S_EINVAL;
    }
    if (p2s_device_count() <= device || device < 0 || device >= P2S_MAX_DEVICES) {
        p2s_set_error("p2s_trimesh_create: no such device %d", device);
        return P2S_ENODEVICE;
    }
    P2S_HIP_CHECK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    const long long V = n_verts, F = n_faces;

    // the index: G a power of two in [2, 128], the smallest with 8 G^2 >= F: a surface occupies a few G^2 cells, so one to
    // two triangles per occupied cell (measured on the 0.92 M-face mesh: ~110 triangle tests per query); the octree over
    // the G^3 cells is 24 bytes per node (55 MB at G = 128)
    int L = 1;
    while (L < MD_MAX_L && (double)(1 << L) * (double)(1 << L) * 8.0 < (double)F) ++L;
    const int G = 1 << L;
    const long long cells = (long long)G * G * G, n_nodes = ((1ll << (3 * (L + 1))) - 1) / 7, leaf_off = ((1ll << (3 * L)) - 1) / 7;
    unsigned cap = 1024;
    while ((long long)cap < 6 * F) cap <<= 1;                      // 3 F half-edges at most: load factor <= 1/2

    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += up(bytes); return o; };
    const size_t o_tri = take((size_t)F * 72), o_stri = take((size_t)F * 72), o_fn = take((size_t)F * 24), o_vn = take((size_t)V * 32),
                 o_fidx = take((size_t)F * 12), o_adj = take((size_t)F * 12), o_sface = take((size_t)F * 4),
                 o_start = take((size_t)(cells + 1) * 4), o_nodes = take((size_t)n_nodes * 24), o_mom = take((size_t)n_nodes * 32),
                 o_parent = take((size_t)F * 4), o_scomp = take((size_t)F * 4), o_fbad = take((size_t)F), o_vbad = take((size_t)V * 4);
    const size_t persistent = at;
    // build scratch: a block of its own, back in the cache when the build is over
    at = 0;
    const size_t o_ctl = take(256), o_ctr = take(64), o_key = take((size_t)cap * 8), o_cnt = take((size_t)cap * 8), o_face = take((size_t)cap * 8),
                 o_fcell = take((size_t)F * 4), o_count = take((size_t)cells * 4), o_cursor = take((size_t)cells * 4);
    char *arena = (char *)p2s_pool_alloc(device, persistent);
    char *scratch = arena ? (char *)p2s_pool_alloc(device, at) : nullptr;
    if (!scratch) {
        p2s_pool_free(device, arena);
        p2s_set_error("p2s_trimesh_create: out of device memory (%zu + %zu bytes)", persistent, at);
        return P2S_ENOMEM;
    }
    auto fail = [&](int code) {
        (void)hipStreamSynchronize(s);
        p2s_pool_free(device, scratch);
        p2s_pool_free(device, arena);
        return code;
    };
    int *ctl = (int *)(scratch + o_ctl);
    unsigned long long *ctr = (unsigned long long *)(scratch + o_ctr);
    const int ctl_init[16] = {0, 0x7f800000, 0x7f800000, 0x7f800000, (int)0x807fffff, (int)0x807fffff, (int)0x807fffff, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    hipError_t e = hipMemcpyAsync(ctl, ctl_init, 64, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(p2s_md_validate_kernel, dim3(blocks(std::max(V, F), 256)), dim3(256), 0, s, verts_dev, V, faces_dev, F, ctl);
        e = hipGetLastError();
    }
    int h[16] = {};
    if (e == hipSuccess) e = hipMemcpyAsync(h, ctl, 64, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        p2s_set_error("p2s_trimesh_create: %s", hipGetErrorString(e));
        return fail(P2S_EHIP);
    }
    if (h[0]) {
        p2s_set_error("p2s_trimesh_create: %s", (h[0] & 2) ? "face index out of range" : "non-finite vertex");
        return fail(P2S_EINVAL);
    }
    p2s_trimesh_s *m = new p2s_trimesh_s();
    m->device = device;
    m->V = V;
    m->F = F;
    m->G = G;
    m->L = L;
    m->arena = arena;
    m->tri = (double *)(arena + o_tri);
    m->stri = (double *)(arena + o_stri);
    m->fn = (double *)(arena + o_fn);
    m->vn = (long long *)(arena + o_vn);
    m->fidx = (int *)(arena + o_fidx);
    m->adj = (int *)(arena + o_adj);
    m->sface = (int *)(arena + o_sface);
    m->cell_start = (int *)(arena + o_start);
    m->nodes = (int *)(arena + o_nodes);
    m->mom = (double *)(arena + o_mom);
    m->fbad = (unsigned char *)(arena + o_fbad);
    m->vbad = (int *)(arena + o_vbad);
    auto dec = [](int i) { const int b = i >= 0 ? i : i ^ 0x7fffffff; float f; memcpy(&f, &b, 4); return f; };
    float ext = 0.f;
    m->scale = 0.0;
    for (int k = 0; k < 3; ++k) {
        const float lo = dec(h[1 + k]), hi = dec(h[4 + k]);
        m->lo[k] = lo;
        ext = std::max(ext, hi - lo);
        m->scale = std::max(m->scale, (double)std::max(std::fabs(lo), std::fabs(hi)));
    }
    if (!(ext > 0.f)) ext = 1.f;                                   // a single point: every centroid lands in cell 0
    m->cell = ext / (float)G;
    m->inv_cell = (float)G / ext;

    EdgeTable t;
    t.key = (unsigned long long *)(scratch + o_key);
    t.cnt = (int *)(scratch + o_cnt);
    t.face = (int *)(scratch + o_face);
    t.mask = cap - 1;
    e = hipMemsetAsync(t.key, 0xff, (size_t)cap * 8, s);
    if (e == hipSuccess) e = hipMemsetAsync(t.cnt, 0, (size_t)cap * 8, s);
    if (e == hipSuccess) e = hipMemsetAsync(t.face, 0xff, (size_t)cap * 8, s);
    if (e == hipSuccess) e = hipMemsetAsync(ctr, 0, 64, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(p2s_md_edges_kernel, dim3(blocks(3 * F, 256)), dim3(256), 0, s, faces_dev, F, t);
        hipLaunchKernelGGL(p2s_md_edge_check_kernel, dim3(blocks(cap, 256)), dim3(256), 0, s, t, ctr + 2);
        hipLaunchKernelGGL(p2s_md_volume_kernel, dim3(1), dim3(1024), 0, s, verts_dev, faces_dev, F, (double *)(ctr + 3));
        e = hipGetLastError();
    }
    unsigned long long hc[4] = {};
    if (e == hipSuccess) e = hipMemcpyAsync(hc, ctr, 32, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) {
        double vol6;
        memcpy(&vol6, &hc[3], 8);
        m->bad_edges = (long long)hc[2];
        m->closed = hc[2] == 0;
        m->inverted = m->closed && vol6 < 0.0;
        SetupArgs a;
        a.verts = verts_dev;
        a.faces = faces_dev;
        a.F = F;
        a.flip = m->inverted;
        a.t = t;
        a.tri = m->tri;
        a.fidx = m->fidx;
        a.fn = m->fn;
        a.adj = m->adj;
        a.vn = (unsigned long long *)m->vn;
        a.fbad = m->fbad;
        a.vbad = m->vbad;
        a.fcell = (int *)(scratch + o_fcell);
        a.count = (int *)(scratch + o_count);
        for (int k = 0; k < 3; ++k) a.lo[k] = m->lo[k];
        a.inv_cell = m->inv_cell;
        a.G = G;
        int *cursor = (int *)(scratch + o_cursor);
        e = hipMemsetAsync(m->vn, 0, (size_t)V * 32, s);
        if (e == hipSuccess) e = hipMemsetAsync(m->vbad, 0, (size_t)V * 4, s);
        if (e == hipSuccess) e = hipMemsetAsync(a.count, 0, (size_t)cells * 4, s);
        if (e == hipSuccess) e = hipMemsetAsync(cursor, 0, (size_t)cells * 4, s);
        if (e == hipSuccess) e = hipMemsetAsync(ctr, 0, 64, s);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(p2s_md_nodes_init_kernel, dim3(blocks(n_nodes, 256)), dim3(256), 0, s, m->nodes, n_nodes);
            hipLaunchKernelGGL(p2s_md_setup_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, a);
            hipLaunchKernelGGL(p2s_md_scan_kernel, dim3(1), dim3(1024), 0, s, a.count, cells, m->cell_start);
            hipLaunchKernelGGL(p2s_md_fill_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, m->tri, a.fcell, F, m->cell_start, cursor, m->sface,
                               m->nodes + 6 * leaf_off);
            hipLaunchKernelGGL(p2s_md_cell_sort_kernel, dim3(blocks(cells, 256)), dim3(256), 0, s, m->cell_start, cells, m->sface);
            hipLaunchKernelGGL(p2s_md_stri_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, m->tri, m->sface, F, m->stri);
            hipLaunchKernelGGL(p2s_md_moments_leaf_kernel, dim3(blocks(cells, 256)), dim3(256), 0, s, m->stri, m->cell_start, cells,
                               m->mom + 4 * leaf_off, ctr + 4);
            for (int l = L - 1; l >= 0; --l) {
                const long long off = ((1ll << (3 * l)) - 1) / 7, coff = ((1ll << (3 * (l + 1))) - 1) / 7;
                hipLaunchKernelGGL(p2s_md_nodes_up_kernel, dim3(blocks(1ll << (3 * l), 256)), dim3(256), 0, s, m->nodes + 6 * off,
                                   m->nodes + 6 * coff, m->mom + 4 * off, m->mom + 4 * coff, l);
            }
            e = hipGetLastError();
        }
        unsigned long long n_deg = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(&n_deg, ctr + 4, 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        m->n_degenerate = (long long)n_deg;
        if (e == hipSuccess && m->closed) {
            int *parent = (int *)(arena + o_parent);
            hipLaunchKernelGGL(p2s_md_cc_compress_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, parent, F, 1);
            // until a round hooks nothing: every round that changes something merges two trees, so it ends; the cap only
            // guards the host loop, and hitting it is an error, never a handle with too many components
            int changed = 1;
            for (int it = 0; it < 100000 && changed && e == hipSuccess; ++it) {
                e = hipMemsetAsync(ctl, 0, 4, s);
                hipLaunchKernelGGL(p2s_md_cc_hook_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, m->adj, parent, F, ctl);
                hipLaunchKernelGGL(p2s_md_cc_compress_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, parent, F, 0);
                if (e == hipSuccess) e = hipGetLastError();
                if (e == hipSuccess) e = hipMemcpyAsync(&changed, ctl, 4, hipMemcpyDeviceToHost, s);
                if (e == hipSuccess) e = hipStreamSynchronize(s);
            }
            if (e == hipSuccess && changed) {
                p2s_set_error("p2s_trimesh_create: the connected components did not converge");
                delete m;
                return fail(P2S_EHIP);
            }
            unsigned long long nc = 0;
            hipLaunchKernelGGL(p2s_md_cc_count_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, parent, F, ctr + 2);
            if (e == hipSuccess) e = hipGetLastError();
            if (e == hipSuccess) e = hipMemcpyAsync(&nc, ctr + 2, 8, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipMemsetAsync(ctr, 0, 64, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            m->components = (int)nc;
            m->comp = parent;
            m->scomp = (int *)(arena + o_scomp);
            if (e == hipSuccess && nc >= 2 && nc <= 16) {
                // the labels of the components (host-sorted: the atomics' order is arbitrary) and each one's own orientation
                int *roots = ctl + 4;
                double *vol = (double *)(ctl + 4 + 16);          // scratch words 20..51 of the 64-word control block
                int hr[17] = {};
                double hv[16] = {};
                e = hipMemsetAsync(ctl, 0, 4, s);
                hipLaunchKernelGGL(p2s_md_cc_roots_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, parent, F, ctl, roots);
                if (e == hipSuccess) e = hipMemcpyAsync(hr, roots, 64, hipMemcpyDeviceToHost, s);
                if (e == hipSuccess) e = hipStreamSynchronize(s);
                std::sort(hr, hr + nc);
                if (e == hipSuccess) e = hipMemcpyAsync(roots, hr, 64, hipMemcpyHostToDevice, s);
                hipLaunchKernelGGL(p2s_md_comp_volume_kernel, dim3((unsigned)nc), dim3(1024), 0, s, m->tri, parent, F, roots, vol);
                hipLaunchKernelGGL(p2s_md_scomp_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, parent, m->sface, F, m->scomp);
                if (e == hipSuccess) e = hipGetLastError();
                if (e == hipSuccess) e = hipMemcpyAsync(hv, vol, 128, hipMemcpyDeviceToHost, s);
                if (e == hipSuccess) e = hipStreamSynchronize(s);
                for (int k = 0; k < (int)nc; ++k) {
                    m->comp_root[k] = hr[k];
                    m->comp_orient[k] = hv[k] < 0.0 ? -1 : 1;
                }
            }
        }
    }
    if (e != hipSuccess) {
        p2s_set_error("p2s_trimesh_create: %s", hipGetErrorString(e));
        delete m;
        return fail(P2S_EHIP);
    }
    p2s_pool_free(device, scratch);          // the stream is drained
    *out = m;
    return P2S_OK;
}

extern "C" int p2s_trimesh_info(p2s_trimesh_t m, int64_t *info_host) {
    if (!m || !info_host) {
        p2s_set_error("p2s_trimesh_info: bad argument");
        return P2S_EINVAL;
    }
    info_host[0] = m->F;
    info_host[1] = m->closed;
    info_host[2] = m->inverted;
    info_host[3] = m->bad_edges;
    info_host[4] = m->G;
    info_host[5] = m->last_tests;
    info_host[6] = m->components;
    info_host[7] = m->n_degenerate;
    return P2S_OK;
}

extern "C" int p2s_mesh_distance(p2s_trimesh_t m, const float *query_dev, int64_t n, int signed_, int method, double *dist_out_dev,
                                 int32_t *face_out_dev, double *closest_out_dev, int64_t *n_winding_host, void *stream) {
    if (n_winding_host) *n_winding_host = 0;
    if (!m || n < 0 || n > (1ll << 30) || (n > 0 && (!query_dev || !dist_out_dev)) || (method != 0 && method != 1)) {
        p2s_set_error("p2s_mesh_distance: bad argument");
        return P2S_EINVAL;
    }
    if (signed_ != 0 && signed_ != 1 && signed_ != 2) {
        p2s_set_error("p2s_mesh_distance: signed_ is 0 (unsigned), 1 (pseudonormal) or 2 (winding number)");
        return P2S_EINVAL;
    }
    const bool by_winding = signed_ == 2;          // the unsigned distance, then every sign from the winding number
    if (by_winding) signed_ = 0;
    if (signed_ && !m->closed) {
        p2s_set_error("p2s_mesh_distance: the mesh is not closed (%lld open or non-manifold edges): no signed distance", m->bad_edges);
        return P2S_EINVAL;
    }
    if (n == 0) return P2S_OK;
    P2S_HIP_CHECK(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    // exhaustive: the faces are split over grid.y until the grid fills the chip
    int parts = 0;
    long long per = m->F;
    if (method == 1) {
        const long long want = std::max<long long>(1, 2048 / (long long)blocks(n, 256));
        parts = (int)std::min<long long>(std::min<long long>(want, 256), std::max<long long>(1, m->F / EX_TILE));
        per = (m->F + parts - 1) / parts;
        per = (per + EX_TILE - 1) / EX_TILE * EX_TILE;
        parts = (int)((m->F + per - 1) / per);
    }
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const bool per_comp = signed_ && m->components >= 2 && m->components <= 16;
    const size_t b_face = up((size_t)n * 4), b_flag = up((size_t)n * 4 * (per_comp ? 3 : 1)), b_pd = up((size_t)n * parts * 8), b_pf = up((size_t)n * parts * 4);
    const size_t b_w = by_winding ? up((size_t)n * 16) : 0;                                // w~ and its bound
    char *ws = (char *)p2s_pool_alloc(m->device, b_face + b_flag + b_pd + b_pf + 256 + b_w);     // + the call's own counters
    if (!ws) {
        p2s_set_error("p2s_mesh_distance: out of device memory");
        return P2S_ENOMEM;
    }
    int *best_face = (int *)ws, *flagged = (int *)(ws + b_face);
    double *part_d2 = (double *)(ws + b_face + b_flag);
    int *part_f = (int *)(ws + b_face + b_flag + b_pd);
    unsigned long long *ctr = (unsigned long long *)(ws + b_face + b_flag + b_pd + b_pf);   // [0] tests, [1] flagged, [2] other tests
    hipError_t e = hipMemsetAsync(ctr, 0, 64, s);
    if (e == hipSuccess) {
        IndexDev ix = {};
        if (method == 0) {
            ix.nodes = m->nodes;
            ix.cell_start = m->cell_start;
            ix.sface = m->sface;
            ix.stri = m->stri;
            for (int k = 0; k < 3; ++k) ix.lo[k] = m->lo[k];
            ix.cell = m->cell;
            ix.G = m->G;
            ix.L = m->L;
            ix.scale = m->scale;
            ix.scomp = m->scomp;
            ix.comp = -1;
            hipLaunchKernelGGL(p2s_md_index_kernel, dim3(blocks(n, 64)), dim3(64), 0, s, ix, query_dev, (long long)n, best_face, ctr);
        } else {
            hipLaunchKernelGGL(p2s_md_exhaustive_kernel, dim3(blocks(n, 256), parts), dim3(256), 0, s, m->tri, m->F, per, query_dev,
                               (long long)n, part_d2, part_f, (const int *)nullptr, -1);
        }
        FinalArgs a;
        a.tri = m->tri;
        a.fn = m->fn;
        a.fidx = m->fidx;
        a.adj = m->adj;
        a.vn = m->vn;
        a.fbad = m->fbad;
        a.vbad = m->vbad;
        a.q = query_dev;
        a.n = n;
        a.best_face = best_face;
        a.part_d2 = part_d2;
        a.part_f = part_f;
        a.parts = parts;
        a.signed_ = signed_;
        a.all_winding = m->components > 16;
        a.wsum = per_comp ? flagged + n : nullptr;
        a.bad = per_comp ? flagged + 2 * n : nullptr;
        a.orient = 0;
        a.scale = m->scale;
        a.dist = dist_out_dev;
        a.face = face_out_dev;
        a.closest = closest_out_dev;
        a.flagged = flagged;
        a.n_flagged = ctr + 1;
        hipLaunchKernelGGL(p2s_md_finalize_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, a);
        for (int k = 0; per_comp && k < m->components; ++k) {        // the nearest face of component k, then its sign
            if (method == 0) {
                ix.comp = m->comp_root[k];
                hipLaunchKernelGGL(p2s_md_index_kernel, dim3(blocks(n, 64)), dim3(64), 0, s, ix, query_dev, (long long)n, best_face,
                                   ctr + 2);
            } else {
                hipLaunchKernelGGL(p2s_md_exhaustive_kernel, dim3(blocks(n, 256), parts), dim3(256), 0, s, m->tri, m->F, per, query_dev,
                                   (long long)n, part_d2, part_f, (const int *)m->comp, m->comp_root[k]);
            }
            a.orient = m->comp_orient[k];
            hipLaunchKernelGGL(p2s_md_comp_sign_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, a);
        }
        if (per_comp) hipLaunchKernelGGL(p2s_md_comp_apply_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, a);
        if (by_winding) {
            double *w = (double *)(ws + b_face + b_flag + b_pd + b_pf + 256), *err = w + n;
            launch_wtree(m, query_dev, (long long)n, WINDING_TAU_DEFAULT, w, err, nullptr, ctr + 4, s);
            hipLaunchKernelGGL(p2s_md_wsign_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, w, err, (long long)n, dist_out_dev, flagged, ctr + 1);
        }
        e = hipGetLastError();
    }
    unsigned long long hc[8] = {};
    if (e == hipSuccess) e = hipMemcpyAsync(hc, ctr, 64, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess && hc[7]) {
        p2s_pool_free(m->device, ws);
        p2s_set_error("p2s_mesh_distance: the winding walk overflowed its stack");
        return P2S_EHIP;
    }
    if (e == hipSuccess && hc[1] > 0) {
        hipLaunchKernelGGL(p2s_md_winding_kernel, dim3((unsigned)hc[1]), dim3(256), 0, s, m->tri, m->F, query_dev, flagged, dist_out_dev,
                           (double *)nullptr, (double *)nullptr);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
    p2s_pool_free(m->device, ws);
    if (e != hipSuccess) {
        p2s_set_error("p2s_mesh_distance: %s", hipGetErrorString(e));
        return P2S_EHIP;
    }
    m->last_tests = (long long)hc[0];
    if (n_winding_host) *n_winding_host = (int64_t)hc[1];
    return P2S_OK;
}

extern "C" int p2s_mesh_winding(p2s_trimesh_t m, const float *query_dev, int64_t n, int method, double tau, double *w_out_dev,
                                double *err_out_dev, int64_t *stats_host, void *stream) {
    if (stats_host) stats_host[0] = stats_host[1] = stats_host[2] = stats_host[3] = 0;
    if (!m || n < 0 || n > (1ll << 30) || (n > 0 && (!query_dev || !w_out_dev)) || (method != 0 && method != 1) ||
        !(tau >= 0.0 && tau <= 0.25)) {                       // false for NaN
        p2s_set_error("p2s_mesh_winding: bad argument (method 0 or 1, tau in [0, 0.25])");
        return P2S_EINVAL;
    }
    if (n == 0) return P2S_OK;
    P2S_HIP_CHECK(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    unsigned long long hc[4] = {};
    hipError_t e = hipSuccess;
    if (method == 1) {
        hipLaunchKernelGGL(p2s_md_winding_kernel, dim3((unsigned)n), dim3(256), 0, s, m->tri, m->F, query_dev, (const int *)nullptr,
                           (double *)nullptr, w_out_dev, err_out_dev);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        hc[1] = (unsigned long long)n * (unsigned long long)m->F;
    } else {
        const size_t b_list = ((size_t)n * 4 + 255) & ~(size_t)255;
        char *ws = (char *)p2s_pool_alloc(m->device, b_list + 256);
        if (!ws) {
            p2s_set_error("p2s_mesh_winding: out of device memory");
            return P2S_ENOMEM;
        }
        int *undecided = (int *)ws;
        unsigned long long *ctr = (unsigned long long *)(ws + b_list);
        e = hipMemsetAsync(ctr, 0, 64, s);
        if (e == hipSuccess) {
            launch_wtree(m, query_dev, (long long)n, tau, w_out_dev, err_out_dev, undecided, ctr, s);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(hc, ctr, 32, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e == hipSuccess && hc[3]) {
            p2s_pool_free(m->device, ws);
            p2s_set_error("p2s_mesh_winding: the walk overflowed its stack");
            return P2S_EHIP;
        }
        if (e == hipSuccess && hc[2] > 0) {                     // undecided: the exact value, bound 0
            hipLaunchKernelGGL(p2s_md_winding_kernel, dim3((unsigned)hc[2]), dim3(256), 0, s, m->tri, m->F, query_dev, (const int *)undecided,
                               (double *)nullptr, w_out_dev, err_out_dev);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipStreamSynchronize(s);
        }
        p2s_pool_free(m->device, ws);
    }
    if (e != hipSuccess) {
        p2s_set_error("p2s_mesh_winding: %s", hipGetErrorString(e));
        return P2S_EHIP;
    }
    if (stats_host) {
        stats_host[0] = (int64_t)hc[0];
        stats_host[1] = (int64_t)hc[1];
        stats_host[2] = (int64_t)hc[2];
    }
    return P2S_OK;
}

// ---------------------------------------------------------------------------------------------
// ray casting, time-of-flight scan and query points on the same handle
// ---------------------------------------------------------------------------------------------
#include "p2s_meshray.inl"
#include "p2s_meshrepair.inl"
