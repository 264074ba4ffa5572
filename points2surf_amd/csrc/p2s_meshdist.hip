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
// One translation unit (six kernels are launched by more than one part), read in this order:
//  1. shared primitives (this file): arithmetic, the shared kernels, the host scaffold of every entry point
//   p2s_md_validate_kernel    indices in range, vertices finite, bounding box             (before anything dereferences)
//   p2s_md_edges_kernel / p2s_rp_edge_faces_kernel   undirected edges into an open-addressing table: traversals and faces
//   p2s_md_volume_kernel / p2s_md_comp_volume_kernel   signed volume, of the mesh and per component (one workgroup, fixed order)
//   p2s_md_cc_hook_kernel / p2s_md_cc_count_kernel   connected components (union-find over neighbours)
//   p2s_devprim.inl           f2o / o2f, uf_find, p2s_uf_compress_kernel, p2s_iota_kernel, p2s_scan_kernel (exclusive scan,
//                             one workgroup); the host scaffold of the entry points is p2s_devcall.h
//  2. p2s_mesh_octree.inl: the implicit octree, its node ids, the stack and the counters of its three walks
//  3. p2s_meshbuild.inl: the handle, p2s_trimesh_create / destroy / info
//   p2s_md_edge_check_kernel  edges that are not (once forward, once backward)
//   p2s_md_setup_kernel       float64 triangles, normals, neighbours, vertex normals, centroid cell
//   p2s_md_cc_roots_kernel / p2s_md_scomp_kernel / p2s_md_fill_kernel / p2s_md_nodes_init_kernel / p2s_md_nodes_up_kernel
//                             the labels of 2..16 components; the index
//   p2s_md_cell_sort_kernel / p2s_md_stri_kernel / p2s_md_moments_leaf_kernel   fixed triangle order per cell, node moments
//  4. distance and winding queries (this file): p2s_mesh_distance, p2s_mesh_winding
//   p2s_md_index_kernel       exact nearest triangle per query: depth-first descent, near child first, pruned by AABB bound
//   p2s_md_exhaustive_kernel  every query against every triangle (yardstick of the index, and for tiny meshes)
//   p2s_md_finalize_kernel    closest point, distance, pseudonormal sign, flag of the queries whose sign is not trusted
//                             (p2s_md_comp_sign_kernel / p2s_md_comp_apply_kernel: the same for 2..16 components)
//   p2s_md_winding_kernel     generalised winding number (Jacobson et al. 2013) of a flagged query: one workgroup each
//   p2s_md_wtree_kernel       the winding number of every query by a walk of the octree: far nodes as dipoles with a
//                             certified error bound, near leaf cells exactly (p2s_mesh_winding, p2s_mesh_distance signed_ 2)
//   p2s_md_wsign_kernel       sign of the distance from that winding number
//  5. p2s_meshray.inl: first-hit ray casting, the time-of-flight scan and the query points on the same handle
//  6. p2s_meshrepair.inl: repair and normalisation of a raw mesh with the same edge table, components, scan and volume sums
//  7. p2s_meshcheck.inl: the pairs of faces that intersect and the non-manifold vertices, by a fourth walk of the octree
//  8. p2s_meshvoxel.inl: the occupancy of a closed mesh on the volume's grid, by a fifth walk (one column of voxels per
//     lane), and the reductions of the reconstruction-quality report
//  9. p2s_meshsimplify.inl: simplification by quadric vertex clustering, with the repair's face hash and the edge table
// 10. p2s_meshcomponents.inl: connected components with their measures, the sub-mesh of a face mask
// 11. p2s_meshmanifold.inl: faces removed at edges of more than two faces, non-manifold vertices split
// 12. p2s_meshholes.inl: boundary loops closed by their minimum-area triangulation (one workgroup per loop, the table in LDS)
// 13. p2s_meshsmooth.inl: vertices moved by the umbrella operator over a sorted CSR of the edge table
// 14. p2s_meshdenoise.inl: face normals filtered over the faces that share a vertex, vertices moved toward them
// 15. p2s_meshrender.inl: shaded pictures of the handle's mesh -- the first-hit walk over camera rays, any-hit occlusion rays
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
#include "p2s_devcall.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#pragma clang fp contract(off)

// ---- 1. shared primitives: arithmetic, the kernels that the build and the repair both launch, the host scaffold
namespace {

#include "p2s_devprim.inl"

constexpr unsigned long long EDGE_EMPTY = ~0ull;
constexpr double FIX = 1099511627776.0;          // 2^40
constexpr double DEGENERATE_REL = 8.077935669463161e-28;   // 2^-90
// a face with a corner sine below 2^-20: its unit normal carries more than 3 * 2^-53 / 2^-20 < 2^-31 of error, which the
// trust bound of the sign assumes -- queries whose pseudonormal involves such a face go to the winding number
constexpr double SLIVER_REL = 9.094947017729282e-13;       // 2^-40 (on sin^2)

__device__ __forceinline__ double dot3(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void cross3(const double *a, const double *b, double *o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ bool finite3(const double *p) {
    return fabs(p[0]) <= 1.0e300 && fabs(p[1]) <= 1.0e300 && fabs(p[2]) <= 1.0e300;      // false for NaN and inf
}

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

// the slot of an edge that p2s_md_edges_kernel inserted
__device__ __forceinline__ unsigned rp_edge_slot(const EdgeTable &t, int a, int b) {
    const unsigned long long key = edge_key(a, b);
    unsigned h = edge_hash(key) & t.mask;
    while (t.key[h] != key) h = (h + 1) & t.mask;
    return h;
}
__global__ __launch_bounds__(256) void p2s_rp_edge_faces_kernel(const int *__restrict__ faces, long long F, EdgeTable t, int *fmn, int *fmx) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= 3 * F) return;
    const long long f = i / 3;
    const int e = (int)(i - 3 * f);
    const unsigned h = rp_edge_slot(t, faces[3 * f + e], faces[3 * f + (e + 1) % 3]);
    atomicMin(&fmn[h], (int)f);
    atomicMax(&fmx[h], (int)f);
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

// connected components: union-find with hooking to the smaller root and full compression, repeated until nothing changes
__global__ __launch_bounds__(256) void p2s_md_cc_hook_kernel(const int *__restrict__ adj, int *parent, long long F, int *changed) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    for (int e = 0; e < 3; ++e) {
        const int g = adj[3 * f + e];
        if (g < 0) continue;
        const int rf = uf_find(parent, (int)f), rg = uf_find(parent, g);
        if (rf != rg) {
            atomicMin(&parent[max(rf, rg)], min(rf, rg));
            *changed = 1;
        }
    }
}
__global__ __launch_bounds__(256) void p2s_md_cc_count_kernel(const int *__restrict__ parent, long long F, unsigned long long *count) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f < F && parent[f] == (int)f) atomicAdd(count, 1ull);
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

// ---- the host scaffold of every entry point of this unit, on top of p2s_devcall.h.  Every entry point still ends drained
// on success and drains before it sets an error text; PoolScratch drains once more before its blocks return to the cache
EdgeTable carve_edges(Carver &c, unsigned cap) {
    EdgeTable t;
    t.key = c.take<unsigned long long>(cap);
    t.cnt = c.take<int>((size_t)cap * 2);
    t.face = c.take<int>((size_t)cap * 2);
    t.mask = cap - 1;
    return t;
}
// the edge table of `faces`: p2s_md_edges_kernel, then the two extreme face ids of every edge when asked for
int build_edges(const char *who, const int *faces, long long F, EdgeTable t, int *fmn, int *fmx, hipStream_t s) {
    const size_t cap = (size_t)t.mask + 1;
    DEV_CHECK(who, hipMemsetAsync(t.key, 0xff, cap * 8, s));
    DEV_CHECK(who, hipMemsetAsync(t.cnt, 0, cap * 8, s));
    DEV_CHECK(who, hipMemsetAsync(t.face, 0xff, cap * 8, s));
    hipLaunchKernelGGL(p2s_md_edges_kernel, dim3(blocks(3 * F, 256)), dim3(256), 0, s, faces, F, t);
    if (fmn) {
        DEV_CHECK(who, hipMemsetAsync(fmn, 0x7f, cap * 4, s));
        DEV_CHECK(who, hipMemsetAsync(fmx, 0xff, cap * 4, s));
        hipLaunchKernelGGL(p2s_rp_edge_faces_kernel, dim3(blocks(3 * F, 256)), dim3(256), 0, s, faces, F, t, fmn, fmx);
    }
    DEV_CHECK(who, hipGetLastError());
    return P2S_OK;
}

// p2s_md_validate_kernel over the vertices and the faces (ctl: 16 device words); box [6]: lo, hi of the vertices
int mesh_validate(const char *who, const float *verts, long long V, const int *faces, long long F, int *ctl, float *box, hipStream_t s) {
    const int init[16] = {0, 0x7f800000, 0x7f800000, 0x7f800000, (int)0x807fffff, (int)0x807fffff, (int)0x807fffff, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int h[16] = {};
    DEV_CHECK(who, hipMemcpyAsync(ctl, init, 64, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(p2s_md_validate_kernel, dim3(blocks(std::max(V, F), 256)), dim3(256), 0, s, verts, V, faces, F, ctl);
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipMemcpyAsync(h, ctl, 64, hipMemcpyDeviceToHost, s));
    DEV_CHECK(who, hipStreamSynchronize(s));
    if (h[0]) {
        p2s_set_error("%s: %s", who, (h[0] & 2) ? "face index out of range" : "non-finite vertex");
        return P2S_EINVAL;
    }
    for (int k = 0; k < 6; ++k) box[k] = o2f(h[1 + k]);
    return P2S_OK;
}

// The counters of a call are 8 device words, zeroed before its launches (MESH_COUNTERS bytes); each call names its slots
// in an enum.  This is the end of the launches: their errors, the counters back on the host, the stream drained; a raised
// overflow word (overflow >= 0: its slot) fails the call.
constexpr size_t MESH_COUNTERS = 64;
int read_counters(const char *who, const unsigned long long *ctr, unsigned long long *host, int overflow, const char *overflow_msg,
                  hipStream_t s) {
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipMemcpyAsync(host, ctr, MESH_COUNTERS, hipMemcpyDeviceToHost, s));
    DEV_CHECK(who, hipStreamSynchronize(s));
    if (overflow >= 0 && host[overflow]) {
        p2s_set_error("%s: %s", who, overflow_msg);
        return P2S_EHIP;
    }
    return P2S_OK;
}

// the exhaustive kernels' split of the faces over grid.y until the grid fills the chip: `parts` of `per` faces each, `per`
// a multiple of the kernel's LDS tile
void exhaustive_parts(long long F, long long n, int tile, int *parts, long long *per) {
    const long long want = std::max<long long>(1, 2048 / (long long)blocks(n, 256));
    const int p = (int)std::min<long long>(std::min<long long>(want, 256), std::max<long long>(1, F / tile));
    const long long q = ((F + p - 1) / p + tile - 1) / tile * tile;
    *parts = (int)((F + q - 1) / q);
    *per = q;
}

}  // namespace

// ---- 2. the octree, 3. the handle and its build
#include "p2s_mesh_octree.inl"
#include "p2s_meshbuild.inl"

// ---- 4. distance and winding queries
namespace {

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
// comp >= 0: only the triangles of this component.  lo, cell: the grid's corner and cell size (the child octant p lies in).
// The stack is a private array per lane (scratch, no LDS), sized like every walk's by OCT_MAX_DEPTH; a push beyond it
// cannot happen.
constexpr int MD_INDEX_STACK = 64;
static_assert(MD_INDEX_STACK >= OCT_MAX_DEPTH, "the nearest-triangle walk's private stack");
__global__ __launch_bounds__(64) void p2s_md_index_kernel(OctreeDev ix, int comp, float3 lo, float cell, const float *__restrict__ q, long long n,
                                                          int *__restrict__ best_face, unsigned long long *__restrict__ tests_total) {
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    unsigned long long tests = 0;
    if (i < n) {
        const double p[3] = {(double)q[3 * i], (double)q[3 * i + 1], (double)q[3 * i + 2]};
        const float glo[3] = {lo.x, lo.y, lo.z};
        int bestf = -1;
        if (finite3(p)) {
            const double E = fmax(ix.scale, fmax(fabs(p[0]), fmax(fabs(p[1]), fabs(p[2])))) * 2.3283064365386963e-10;
            double best = INFINITY, thresh = INFINITY;
            int stack[MD_INDEX_STACK];
            int sp = 0;
            stack[sp++] = oct_id(0, 0);
            while (sp > 0) {
                const int node = stack[--sp];
                const int l = oct_level(node), lin = oct_lin(node);
                const double lb = aabb_bound(oct_box(ix, l, lin), p);
                if (lb > thresh || lb == INFINITY) continue;
                if (l == ix.L) {
                    int t0, t1;
                    oct_leaf_range(ix, lin, &t0, &t1);
                    for (int t = t0; t < t1; ++t) {
                        if (comp >= 0 && ix.scomp[t] != comp) continue;
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
                    int xyz[3];
                    oct_xyz(l, lin, xyz);
                    const double half = (double)cell * (double)(1 << (ix.L - l - 1));        // child size at level l + 1
                    int m = 0;                                                            // the child octant p lies towards
                    for (int k = 0; k < 3; ++k) m = (m << 1) | (p[k] > (double)glo[k] + (2 * xyz[k] + 1) * half ? 1 : 0);
                    for (int j = 7; j >= 0; --j) {           // pushed far to near: the near child is popped first
                        const int clin = oct_child_lin(l, xyz, j ^ m);
                        const double cb = aabb_bound(oct_box(ix, l + 1, clin), p);
                        if (cb > thresh || cb == INFINITY) continue;
                        if (sp < MD_INDEX_STACK) stack[sp++] = oct_id(l + 1, clin);
                    }
                }
            }
        }
        best_face[i] = bestf;
    }
    wave_count(tests_total, tests);
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

// ---- hierarchical winding number
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
// Stack: a LaneStack (p2s_mesh_octree.inl), 13 KiB of LDS per workgroup; its overflow word is WT_OVERFLOW.
__device__ __forceinline__ double wtree_rounding(double F, double K, double D) {
    return 1.1102230246251565e-16 * (F * ((K + F * 0.00390625) + 32.0)) + D * 4.523328512768113e-15;      // 2^-53, 2^-46 / pi
}

// the four counters of the walk (with `undecided`, WT_UNDECIDED also indexes their list)
enum WalkCtr { WT_ACCEPTED, WT_TRIS, WT_UNDECIDED, WT_OVERFLOW };

__global__ __launch_bounds__(64) void p2s_md_wtree_kernel(OctreeDev ix, long long F, long long n_degenerate, double tau,
                                                          const float *__restrict__ q, long long n, double *__restrict__ w_out,
                                                          double *__restrict__ err_out, int *__restrict__ undecided,
                                                          unsigned long long *__restrict__ ctr) {
    __shared__ int lds[OCT_STACK * 64];
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
            LaneStack stack(lds, lane);
            stack.push(oct_id(0, 0), ctr + WT_OVERFLOW);
            while (!stack.empty()) {
                const int node = stack.pop();
                const int l = oct_level(node), lin = oct_lin(node);
                const int *bx = oct_box(ix, l, lin);
                const double *mo = oct_moments(ix, l, lin);
                double cp[3], e[3];
                for (int k = 0; k < 3; ++k) {
                    const double lo = o2f(bx[k]), hi = o2f(bx[3 + k]);
                    cp[k] = 0.5 * (lo + hi) - p[k];
                    e[k] = hi - lo;
                }
                const double r = (0.5 * sqrt(dot3(e, e))) * 1.0000000009313226, d = sqrt(dot3(cp, cp)), A = mo[3];
                if (tau > 0.0 && d >= 2.0 * r && A <= 6.283185307179586 * (d * d)) {
                    const double g = d - r, g3 = g * g * g;
                    const double bound = (A * r) / (6.283185307179586 * g3);
                    if (g3 > 0.0 && bound * a_root <= tau * A) {
                        sd += dot3(mo, cp) / (12.566370614359172 * (d * d * d));
                        sb += bound;
                        ++accepted;
                        continue;
                    }
                }
                if (l == ix.L) {
                    int t0, t1;
                    oct_leaf_range(ix, lin, &t0, &t1);
                    for (int t = t0; t < t1; ++t) {
                        sa += winding_term(ix.stri + 9 * (long long)t, p);
                        ++tris;
                    }
                } else {
                    int xyz[3];
                    oct_xyz(l, lin, xyz);
                    for (int c = 7; c >= 0; --c) {           // child 0 is popped first: a fixed order
                        const int clin = oct_child_lin(l, xyz, c);
                        const int *cb = oct_box(ix, l + 1, clin);
                        if (cb[0] > cb[3]) continue;         // empty: no triangle, nothing to add
                        stack.push(oct_id(l + 1, clin), ctr + WT_OVERFLOW);
                    }
                }
            }
            const double w = sa / 6.283185307179586 + sd;
            const double eps = sb + wtree_rounding((double)F, (double)(accepted + tris), (double)n_degenerate);
            w_out[i] = w;
            if (err_out) err_out[i] = eps;
            if (undecided && !(fabs(fabs(w) - 0.5) > eps)) undecided[atomicAdd(ctr + WT_UNDECIDED, 1ull)] = (int)i;
        }
    }
    wave_count(ctr + WT_ACCEPTED, accepted);
    wave_count(ctr + WT_TRIS, tris);
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

constexpr double WINDING_TAU_DEFAULT = 0.0009765625;       // 2^-10

// ctr: the four WalkCtr words (zeroed by the caller)
void launch_wtree(const p2s_trimesh_s *m, const float *q, long long n, double tau, double *w, double *err, int *undecided,
                  unsigned long long *ctr, hipStream_t s) {
    hipLaunchKernelGGL(p2s_md_wtree_kernel, dim3(blocks(n, 64)), dim3(64), 0, s, octree_of(m), m->F, m->n_degenerate, tau, q, n, w, err,
                       undecided, ctr);
}

enum DistCtr { DC_TESTS, DC_FLAGGED, DC_COMP_TESTS, DC_WTREE = 4 };      // DC_WTREE: the four WalkCtr words of signed_ == 2
struct DistWs {
    int *best_face, *flagged;      // index method: nearest face; the queries whose sign the winding number decides
    int *wsum, *bad;               // 2..16 components
    double *part_d2;               // exhaustive method: [parts][n]
    int *part_f;
    double *w, *err;               // signed_ == 2: w~ and its bound
    unsigned long long *ctr;
    char *base;
    size_t bytes;
};
DistWs carve_dist(char *base, size_t n, int parts, bool per_comp, bool by_winding) {
    Carver c{base};
    DistWs w;
    w.best_face = c.take<int>(n);
    w.flagged = c.take<int>(n);
    w.wsum = c.take<int>(n, per_comp);
    w.bad = c.take<int>(n, per_comp);
    w.part_d2 = c.take<double>(n * parts);
    w.part_f = c.take<int>(n * parts);
    w.w = c.take<double>(n, by_winding);
    w.err = c.take<double>(n, by_winding);
    w.ctr = c.take<unsigned long long>(8);
    return c.done(w);
}

}  // namespace

extern "C" int p2s_mesh_distance(p2s_trimesh_t m, const float *query_dev, int64_t n, int signed_, int method, double *dist_out_dev,
                                 int32_t *face_out_dev, double *closest_out_dev, int64_t *n_winding_host, void *stream) {
    static const char *const who = "p2s_mesh_distance";
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
    int parts = 0;
    long long per = m->F;
    if (method == 1) exhaustive_parts(m->F, n, EX_TILE, &parts, &per);
    const bool per_comp = signed_ && m->components >= 2 && m->components <= 16;
    PoolScratch pool(m->device, s);
    const DistWs w = pool.carve([&](char *b) { return carve_dist(b, (size_t)n, parts, per_comp, by_winding); });
    if (!w.base) return dev_oom(who, s);
    DEV_CHECK(who, hipMemsetAsync(w.ctr, 0, MESH_COUNTERS, s));
    const OctreeDev ix = octree_of(m);
    // the nearest face of the whole mesh (comp < 0) or of one component, into best_face or the parts
    auto nearest = [&](int comp, unsigned long long *tests) {
        if (method == 0)
            hipLaunchKernelGGL(p2s_md_index_kernel, dim3(blocks(n, 64)), dim3(64), 0, s, ix, comp, make_float3(m->lo[0], m->lo[1], m->lo[2]),
                               m->cell, query_dev, (long long)n, w.best_face, tests);
        else
            hipLaunchKernelGGL(p2s_md_exhaustive_kernel, dim3(blocks(n, 256), parts), dim3(256), 0, s, m->tri, m->F, per, query_dev,
                               (long long)n, w.part_d2, w.part_f, comp < 0 ? (const int *)nullptr : (const int *)m->comp, comp);
    };
    nearest(-1, w.ctr + DC_TESTS);
    FinalArgs a = {m->tri, m->fn, m->fidx, m->adj, m->vn, m->fbad, m->vbad, query_dev, n, w.best_face, w.part_d2, w.part_f, parts, signed_,
                   m->components > 16, w.wsum, w.bad, 0, m->scale, dist_out_dev, face_out_dev, closest_out_dev, w.flagged, w.ctr + DC_FLAGGED};
    hipLaunchKernelGGL(p2s_md_finalize_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, a);
    for (int k = 0; per_comp && k < m->components; ++k) {        // the nearest face of component k, then its sign
        nearest(m->comp_root[k], w.ctr + DC_COMP_TESTS);
        a.orient = m->comp_orient[k];
        hipLaunchKernelGGL(p2s_md_comp_sign_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, a);
    }
    if (per_comp) hipLaunchKernelGGL(p2s_md_comp_apply_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, a);
    if (by_winding) {
        launch_wtree(m, query_dev, (long long)n, WINDING_TAU_DEFAULT, w.w, w.err, nullptr, w.ctr + DC_WTREE, s);
        hipLaunchKernelGGL(p2s_md_wsign_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, w.w, w.err, (long long)n, dist_out_dev, w.flagged,
                           w.ctr + DC_FLAGGED);
    }
    unsigned long long hc[8] = {};
    const int rc = read_counters(who, w.ctr, hc, DC_WTREE + WT_OVERFLOW, "the winding walk overflowed its stack", s);
    if (rc != P2S_OK) return rc;
    if (hc[DC_FLAGGED] > 0) {
        hipLaunchKernelGGL(p2s_md_winding_kernel, dim3((unsigned)hc[DC_FLAGGED]), dim3(256), 0, s, m->tri, m->F, query_dev,
                           (const int *)w.flagged, dist_out_dev, (double *)nullptr, (double *)nullptr);
        DEV_CHECK(who, hipGetLastError());
        DEV_CHECK(who, hipStreamSynchronize(s));
    }
    m->last_tests = (long long)hc[DC_TESTS];
    if (n_winding_host) *n_winding_host = (int64_t)hc[DC_FLAGGED];
    return P2S_OK;
}

extern "C" int p2s_mesh_winding(p2s_trimesh_t m, const float *query_dev, int64_t n, int method, double tau, double *w_out_dev,
                                double *err_out_dev, int64_t *stats_host, void *stream) {
    static const char *const who = "p2s_mesh_winding";
    if (stats_host) stats_host[0] = stats_host[1] = stats_host[2] = stats_host[3] = 0;
    if (!m || n < 0 || n > (1ll << 30) || (n > 0 && (!query_dev || !w_out_dev)) || (method != 0 && method != 1) ||
        !(tau >= 0.0 && tau <= 0.25)) {                       // false for NaN
        p2s_set_error("p2s_mesh_winding: bad argument (method 0 or 1, tau in [0, 0.25])");
        return P2S_EINVAL;
    }
    if (n == 0) return P2S_OK;
    P2S_HIP_CHECK(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    unsigned long long hc[8] = {}, n_exact = (unsigned long long)n;
    const int *list = nullptr;                                 // the queries of the exact sum: every one, or the walk's undecided
    PoolScratch pool(m->device, s);
    if (method == 1) {
        hc[WT_TRIS] = (unsigned long long)n * (unsigned long long)m->F;
    } else {
        struct Ws {
            int *undecided;
            unsigned long long *ctr;
            char *base;
            size_t bytes;
        };
        const Ws w = pool.carve([&](char *b) {
            Carver c{b};
            Ws r;
            r.undecided = c.take<int>((size_t)n);
            r.ctr = c.take<unsigned long long>(8);
            return c.done(r);
        });
        if (!w.base) return dev_oom(who, s);
        DEV_CHECK(who, hipMemsetAsync(w.ctr, 0, MESH_COUNTERS, s));
        launch_wtree(m, query_dev, (long long)n, tau, w_out_dev, err_out_dev, w.undecided, w.ctr, s);
        const int rc = read_counters(who, w.ctr, hc, WT_OVERFLOW, "the walk overflowed its stack", s);
        if (rc != P2S_OK) return rc;
        list = w.undecided;
        n_exact = hc[WT_UNDECIDED];
    }
    if (n_exact > 0) {                                         // the exact value, bound 0
        hipLaunchKernelGGL(p2s_md_winding_kernel, dim3((unsigned)n_exact), dim3(256), 0, s, m->tri, m->F, query_dev, list,
                           (double *)nullptr, w_out_dev, err_out_dev);
        DEV_CHECK(who, hipGetLastError());
        DEV_CHECK(who, hipStreamSynchronize(s));
    }
    if (stats_host) {
        stats_host[0] = (int64_t)hc[WT_ACCEPTED];
        stats_host[1] = (int64_t)hc[WT_TRIS];
        stats_host[2] = (int64_t)hc[WT_UNDECIDED];
    }
    return P2S_OK;
}

// ---- 5. ray casting, time-of-flight scan and query points on the same handle; 6. repair and normalisation of a raw mesh
#include "p2s_meshray.inl"
#include "p2s_meshrepair.inl"
// ---- 7. self-intersections and non-manifold vertices of the handle's mesh
#include "p2s_meshcheck.inl"
// ---- 8. occupancy on the volume's grid and the reductions of the quality report
#include "p2s_meshvoxel.inl"
// ---- 9. simplification by quadric vertex clustering
#include "p2s_meshsimplify.inl"
// ---- 10. connected components with their measures; the sub-mesh of a face mask
#include "p2s_meshcomponents.inl"
// ---- 11. 2-manifold repair: faces removed at edges of more than two faces, non-manifold vertices split
#include "p2s_meshmanifold.inl"
// ---- 12. holes closed by the minimum-area triangulation of their boundary loops
#include "p2s_meshholes.inl"
// ---- 13. vertices moved by the umbrella operator: Taubin and Laplacian smoothing
#include "p2s_meshsmooth.inl"
// ---- 14. denoising that keeps sharp edges: face normals filtered, vertices moved toward them
#include "p2s_meshdenoise.inl"
// ---- 15. shaded pictures: primary rays through the first-hit walk, shading and any-hit occlusion rays, the resolve
#include "p2s_meshrender.inl"
