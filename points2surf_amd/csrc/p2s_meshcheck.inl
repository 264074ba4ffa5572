// Self-intersections and non-manifold vertices of the mesh of a handle (p2s_mesh_check).  Included by p2s_meshdist.hip
// behind the repair; the rule is the project's own (trimesh offers none) and is stated in include/p2s_hip.h.
//   p2s_mc_prep_kernel         per face: the ordered-integer AABB and the degenerate flag
//   p2s_mc_index_kernel        one face per lane walks the octree with its own AABB as the query box; the faces g > f of
//                              every leaf it opens go to the narrow phase
//   p2s_mc_exhaustive_kernel   every face against every face g > f, the faces g staged through LDS (the yardstick)
//   p2s_mc_vertex_faces_kernel / p2s_mc_fan_kernel   faces per vertex and its smallest face; the fan walk
//   p2s_mc_flags_kernel        the flag words as bytes, and their counts
//   p2s_mc_unpack_kernel       the sorted (g, class) words of every face as pairs and class bytes
// Both pair kernels run twice: a count pass (counters, flags, stored pairs per face), then, behind p2s_scan_kernel, a
// fill pass that writes (g << 2 | class) into the face's own range; p2s_md_cell_sort_kernel sorts every range, so the
// pairs are ascending in (f, g) whatever order lanes or atomics arrived in.
//
// Arithmetic: float64, contraction off, orient3(a, b, c, d) = ((b - a) x (c - a)) . (d - a) through cross3 and dot3, the one
// place a side value (a, b, c a triangle) or a tetrahedron volume (a, b an edge of one triangle, c, d of the other) is
// computed; orient2 the same in the plane.  tests/mesh_check_model.py performs the same operations in the same order.
//
// The filter bound.  Let S be the largest |coordinate| of the mesh and u = 2^-53; every coordinate is a float32 value held
// exactly in float64.  A difference fl(b - a) = (b - a)(1 + d), |d| <= u, is at most 2 S in magnitude.  A component of the
// cross product is fl(fl(x y) - fl(z w)) of such differences: each product is at most 4 S^2 and carries (1 + u)^3 - 1, so
// 12 u S^2 to first order, the subtraction adds u 8 S^2: |n^ - n| <= 32 u S^2 per component, |n| <= 8 S^2.  A product of the
// dot, fl(n^_k w^_k), differs from n_k w_k (at most 16 S^3) by 32 u S^2 * 2 S + 8 S^2 * 2 S u + 16 S^3 u = 96 u S^3; three of them
// 288 u S^3; the two additions of (x + y) + z add u 32 S^3 and u 48 S^3.  Together 368 u S^3 to first order, and the second-order
// terms are below 10 u of that.  MC_EPS3 = 2^10 u S^3 = 2^-43 S^3 is above it with a factor 2.7 to spare, which also covers the
// two roundings of (S S) S: a computed orient3 beyond MC_EPS3 in magnitude has the sign of the exact value.  In the plane
// each product of orient2 is at most 4 S^2 with 12 u S^2 of error and the subtraction adds u 8 S^2: 32 u S^2 < MC_EPS2 = 2^6 u S^2 =
// 2^-47 S^2.  (A difference of two float32 values is NOT always exact in float64 -- their exponents may lie more than 29
// apart -- so the signs in the plane get a bound like the others.)  A value within its bound is the sign 0.

namespace {

constexpr int MC_DISJOINT = 0, MC_INTERSECTING = 1, MC_COPLANAR = 2, MC_TOUCHING = 3, MC_DUPLICATE = 4;
constexpr int MC_FACE_DEGENERATE = 8;              // face flag bits 1, 2, 4: in a pair of class 1, 2, 3

__device__ __forceinline__ double orient3(const double *a, const double *b, const double *c, const double *d) {
    double u[3], v[3], w[3], n[3];
    for (int k = 0; k < 3; ++k) {
        u[k] = b[k] - a[k];
        v[k] = c[k] - a[k];
        w[k] = d[k] - a[k];
    }
    cross3(u, v, n);
    return dot3(n, w);
}
__device__ __forceinline__ int mc_sign(double x, double eps) { return x > eps ? 1 : (x < -eps ? -1 : 0); }      // NaN: 0

// a triangle in the plane: the axis of the largest |n| dropped (the first among equals), i0 < i1 the two kept.  mc_at:
// coordinate i of a point by selects, so that a triangle held in registers stays there.
__device__ __forceinline__ double mc_at(const double *p, int i) { return i == 0 ? p[0] : (i == 1 ? p[1] : p[2]); }
__device__ __forceinline__ void mc_axes(const double *T, int *i0, int *i1) {
    double u[3], v[3], n[3];
    for (int k = 0; k < 3; ++k) {
        u[k] = T[3 + k] - T[k];
        v[k] = T[6 + k] - T[k];
    }
    cross3(u, v, n);
    int ax = fabs(n[1]) > fabs(n[0]) ? 1 : 0;
    if (fabs(n[2]) > fmax(fabs(n[0]), fabs(n[1]))) ax = 2;
    *i0 = ax == 0 ? 1 : 0;
    *i1 = ax == 2 ? 1 : 2;
}
__device__ __forceinline__ int orient2_sign(const double *a, const double *b, const double *c, int i0, int i1, double eps2) {
    return mc_sign((mc_at(b, i0) - mc_at(a, i0)) * (mc_at(c, i1) - mc_at(a, i1)) - (mc_at(b, i1) - mc_at(a, i1)) * (mc_at(c, i0) - mc_at(a, i0)), eps2);
}

// two triangles in one plane.  COPLANAR when no edge line of either has the other triangle on its outer closed side (they
// overlap in an open set; a sign 0 counts as outside, so the class needs strict evidence).  Otherwise a pair with a shared
// index meets in its shared vertices only: DISJOINT; a pair without one is DISJOINT when some edge line has the other
// triangle strictly outside, else TOUCHING.
// the edge lines of P (orientation o) against the vertices of Q: *sep when one has all of Q outside or on it, *strict
// when one has all of Q strictly outside
__device__ __forceinline__ void mc_edge_lines(const double *P, int o, const double *Q, int i0, int i1, double eps2, bool *sep, bool *strict) {
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const double *x = P + 3 * e, *y = P + 3 * ((e + 1) % 3);
        bool le = true, lt = true;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int s = o * orient2_sign(x, y, Q + 3 * j, i0, i1, eps2);
            le = le && s <= 0;
            lt = lt && s < 0;
        }
        *sep = *sep || le;
        *strict = *strict || lt;
    }
}
__device__ __forceinline__ int mc_coplanar(const double *A, const double *B, bool shared, double eps2) {
    int i0, i1;
    mc_axes(A, &i0, &i1);
    const int oA = orient2_sign(A, A + 3, A + 6, i0, i1, eps2), oB = orient2_sign(B, B + 3, B + 6, i0, i1, eps2);
    if (oA == 0 || oB == 0) return MC_TOUCHING;
    bool sep = false, strict = false;
    mc_edge_lines(A, oA, B, i0, i1, eps2, &sep, &strict);
    mc_edge_lines(B, oB, A, i0, i1, eps2, &sep, &strict);
    return !sep ? MC_COPLANAR : (strict || shared ? MC_DISJOINT : MC_TOUCHING);
}

// the edge p-q against the triangle T, sp / sq the signs of side_T(p) / side_T(q): 0 = it does not pierce the interior of T,
// 2 = it does (end points strictly on opposite sides, the three volumes of one strict sign), 1 = neither is certain.  An
// edge in the plane of T (both signs 0) has all three volumes 0: it is decided in the plane, 0 when an edge line of T has
// both end points strictly outside or the line p-q has T strictly on one side.
__device__ __forceinline__ int mc_edge(const double *p, const double *q, const double *T, int sp, int sq, double eps3, double eps2) {
    if (sp * sq > 0) return 0;
    if (sp == 0 && sq == 0) {
        int i0, i1;
        mc_axes(T, &i0, &i1);
        const int o = orient2_sign(T, T + 3, T + 6, i0, i1, eps2);
        if (o == 0) return 1;
        int r[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double *x = T + 3 * k, *y = T + 3 * ((k + 1) % 3);
            if (o * orient2_sign(x, y, p, i0, i1, eps2) < 0 && o * orient2_sign(x, y, q, i0, i1, eps2) < 0) return 0;
            r[k] = orient2_sign(p, q, x, i0, i1, eps2);
        }
        return r[0] != 0 && r[0] == r[1] && r[1] == r[2] ? 0 : 1;
    }
    bool pos = false, neg = false, zero = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int v = mc_sign(orient3(p, q, T + 3 * k, T + 3 * ((k + 1) % 3)), eps3);
        pos = pos || v > 0;
        neg = neg || v < 0;
        zero = zero || v == 0;
    }
    if (pos && neg) return 0;
    return sp * sq < 0 && !zero ? 2 : 1;
}

// the class of the pair of the non-degenerate triangles A, B [9] with the vertex indices ia, ib [3] and the ordered-integer
// boxes ba, bb [6] (the rule: include/p2s_hip.h)
__device__ __forceinline__ int mc_classify(const double *A, const int *ia, const int *ba, const double *B, const int *ib, const int *bb,
                                           double eps3, double eps2) {
    int sa = 0, sb = 0, ns = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (ia[i] == ib[j]) {
                sa |= 1 << i;
                sb |= 1 << j;
                ++ns;
            }
    if (ns == 3) return MC_DUPLICATE;
    for (int k = 0; k < 3; ++k)
        if (ba[k] > bb[3 + k] || bb[k] > ba[3 + k]) return MC_DISJOINT;
    int sB[3], sA[3];
    bool flat = true, posB = true, negB = true, posA = true, negA = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const bool sh = (sb >> j) & 1;
        sB[j] = sh ? 0 : mc_sign(orient3(A, A + 3, A + 6, B + 3 * j), eps3);
        flat = flat && sB[j] == 0;
        posB = posB && (sh || sB[j] > 0);
        negB = negB && (sh || sB[j] < 0);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const bool sh = (sa >> i) & 1;
        sA[i] = sh ? 0 : mc_sign(orient3(B, B + 3, B + 6, A + 3 * i), eps3);
        flat = flat && sA[i] == 0;
        posA = posA && (sh || sA[i] > 0);
        negA = negA && (sh || sA[i] < 0);
    }
    if (flat) return mc_coplanar(A, B, ns > 0, eps2);
    if (ns == 2 || posB || negB || posA || negA) return MC_DISJOINT;
    int best = 0;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const int e1 = (e + 1) % 3;
        if (!((sb >> e) & 1) && !((sb >> e1) & 1)) best = max(best, mc_edge(B + 3 * e, B + 3 * e1, A, sB[e], sB[e1], eps3, eps2));
        if (!((sa >> e) & 1) && !((sa >> e1) & 1)) best = max(best, mc_edge(A + 3 * e, A + 3 * e1, B, sA[e], sA[e1], eps3, eps2));
    }
    return best == 2 ? MC_INTERSECTING : (best == 1 ? MC_TOUCHING : MC_DISJOINT);
}

__global__ __launch_bounds__(256) void p2s_mc_prep_kernel(const double *__restrict__ tri, long long F, int *__restrict__ fbox,
                                                          unsigned char *__restrict__ deg, int *__restrict__ fflag) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const double *P = tri + 9 * f;
    double ab[3], ac[3], n[3];
    for (int k = 0; k < 3; ++k) {
        ab[k] = P[3 + k] - P[k];
        ac[k] = P[6 + k] - P[k];
        const float a = (float)P[k], b = (float)P[3 + k], c = (float)P[6 + k];                  // exact: float32 vertices
        fbox[6 * f + k] = f2o(fminf(a, fminf(b, c)));
        fbox[6 * f + 3 + k] = f2o(fmaxf(a, fmaxf(b, c)));
    }
    cross3(ab, ac, n);
    const bool d = !(dot3(n, n) > DEGENERATE_REL * (dot3(ab, ab) * dot3(ac, ac)));
    deg[f] = d ? 1 : 0;
    fflag[f] = d ? MC_FACE_DEGENERATE : 0;
}

enum CheckCtr { CK_CANDIDATES, CK_INTERSECTING, CK_COPLANAR, CK_TOUCHING, CK_DUPLICATE, CK_INSIDE, CK_OVERFLOW };
enum CheckCtr2 { CV_FACES, CV_VERTS };

struct CheckArgs {
    const double *tri;             // [F][9]
    const int *fidx;               // [F][3]
    const int *fbox;               // [F][6]
    const unsigned char *deg;      // [F]
    const int *comp;               // [F] or NULL
    long long F;
    double eps3, eps2;
    int *fflag;                    // count pass: [F] flag words
    int *count;                    // count pass: [F] stored pairs of face f (g > f)
    const int *start;              // fill pass: [F + 1]
    int *cursor;                   // fill pass of the exhaustive kernel: [F], zeroed
    int *packed;                   // fill pass: [stored] g << 2 | class; NULL in the count pass
    unsigned long long *ctr;
};

// what one lane keeps of its pairs
struct CheckTally {
    unsigned long long cand = 0, intersecting = 0, coplanar = 0, touching = 0, duplicate = 0, inside = 0;
    int stored = 0, flags = 0;
};
// the pair (f, g), g > f, both tested faces: its class, tallied; in the count pass the flags and the component count too.
// true: the pair is stored (the caller places its word)
__device__ __forceinline__ bool mc_pair(const CheckArgs &a, int f, const double *A, const int *ia, const int *ba, int g, const double *B,
                                        const int *ib, const int *bb, CheckTally &t, int *cls_out) {
    ++t.cand;
    const int cls = mc_classify(A, ia, ba, B, ib, bb, a.eps3, a.eps2);
    t.intersecting += cls == MC_INTERSECTING;
    t.coplanar += cls == MC_COPLANAR;
    t.touching += cls == MC_TOUCHING;
    t.duplicate += cls == MC_DUPLICATE;
    *cls_out = cls;
    if (cls == MC_DISJOINT || cls == MC_DUPLICATE) return false;
    if (!a.packed) {
        const int bit = 1 << (cls - 1);
        t.flags |= bit;
        atomicOr(&a.fflag[g], bit);
        if (cls != MC_TOUCHING && a.comp && a.comp[f] == a.comp[g]) ++t.inside;
    }
    return true;
}
__device__ __forceinline__ void mc_tally(const CheckArgs &a, const CheckTally &t) {
    wave_count(a.ctr + CK_CANDIDATES, t.cand);
    wave_count(a.ctr + CK_INTERSECTING, t.intersecting);
    wave_count(a.ctr + CK_COPLANAR, t.coplanar);
    wave_count(a.ctr + CK_TOUCHING, t.touching);
    wave_count(a.ctr + CK_DUPLICATE, t.duplicate);
    wave_count(a.ctr + CK_INSIDE, t.inside);
}

// Broad phase.  The faces are binned by centroid, so a cell says nothing about where its triangles reach: the node BOXES
// (the union of the triangles' own boxes) decide what is opened, box against box on the ordered integers, closed on both
// ends like the test mc_classify starts with -- a pair it would not reject is in a leaf whose box meets the face's.  A pair
// is produced once, by its smaller face, whichever cells the two sit in.  Stack: a LaneStack, overflow word CK_OVERFLOW.
__global__ __launch_bounds__(64) void p2s_mc_index_kernel(OctreeDev ix, CheckArgs a) {
    __shared__ int lds[OCT_STACK * 64];
    const int lane = threadIdx.x;
    const long long fl = (long long)blockIdx.x * 64 + lane;
    CheckTally t;
    if (fl < a.F && !a.deg[fl]) {
        const int f = (int)fl;
        double A[9];
        int ia[3], ba[6];
        for (int k = 0; k < 9; ++k) A[k] = a.tri[9 * fl + k];
        for (int k = 0; k < 3; ++k) ia[k] = a.fidx[3 * fl + k];
        for (int k = 0; k < 6; ++k) ba[k] = a.fbox[6 * fl + k];
        const int at = a.packed ? a.start[f] : 0;
        LaneStack stack(lds, lane);
        stack.push(oct_id(0, 0), a.ctr + CK_OVERFLOW);
        while (!stack.empty()) {
            const int node = stack.pop();
            const int l = oct_level(node), lin = oct_lin(node);
            if (l == ix.L) {
                int t0, t1;
                oct_leaf_range(ix, lin, &t0, &t1);
                for (int s = t0; s < t1; ++s) {
                    const int g = ix.sface[s];
                    if (g <= f || a.deg[g]) continue;
                    int cls;
                    if (!mc_pair(a, f, A, ia, ba, g, ix.stri + 9 * (long long)s, a.fidx + 3 * (long long)g, a.fbox + 6 * (long long)g, t, &cls))
                        continue;
                    if (a.packed) a.packed[at + t.stored] = (g << 2) | cls;
                    ++t.stored;
                }
            } else {
                int xyz[3];
                oct_xyz(l, lin, xyz);
                for (int c = 7; c >= 0; --c) {
                    const int clin = oct_child_lin(l, xyz, c);
                    const int *cb = oct_box(ix, l + 1, clin);
                    bool meets = true;                       // false for an empty node too (lo = +inf, hi = -inf)
                    for (int k = 0; k < 3; ++k) meets = meets && cb[k] <= ba[3 + k] && ba[k] <= cb[3 + k];
                    if (meets) stack.push(oct_id(l + 1, clin), a.ctr + CK_OVERFLOW);
                }
            }
        }
        if (!a.packed) {
            a.count[f] = t.stored;
            if (t.flags) atomicOr(&a.fflag[f], t.flags);
        }
    }
    if (!a.packed) mc_tally(a, t);
}

// every face f against the faces g > f of [y * per, (y + 1) * per), staged through LDS
constexpr int CX_TILE = 128;
__global__ __launch_bounds__(256) void p2s_mc_exhaustive_kernel(CheckArgs a, long long per) {
    __shared__ double tile[CX_TILE * 9];
    __shared__ int tidx[CX_TILE * 3], tbox[CX_TILE * 6];
    __shared__ unsigned char tdeg[CX_TILE];
    const long long fl = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long f0 = (long long)blockIdx.y * per, f1 = min(a.F, f0 + per);
    const bool live = fl < a.F && !a.deg[fl < a.F ? fl : 0];
    const int f = (int)fl;
    double A[9];
    int ia[3], ba[6];
    CheckTally t;
    if (live) {
        for (int k = 0; k < 9; ++k) A[k] = a.tri[9 * fl + k];
        for (int k = 0; k < 3; ++k) ia[k] = a.fidx[3 * fl + k];
        for (int k = 0; k < 6; ++k) ba[k] = a.fbox[6 * fl + k];
    }
    for (long long b0 = f0; b0 < f1; b0 += CX_TILE) {
        const int lim = (int)min((long long)CX_TILE, f1 - b0);
        if (b0 + lim - 1 <= (long long)blockIdx.x * 256) continue;       // no g > f for any face of this workgroup (uniform)
        for (int k = threadIdx.x; k < lim * 9; k += 256) tile[k] = a.tri[9 * b0 + k];
        for (int k = threadIdx.x; k < lim * 3; k += 256) tidx[k] = a.fidx[3 * b0 + k];
        for (int k = threadIdx.x; k < lim * 6; k += 256) tbox[k] = a.fbox[6 * b0 + k];
        if ((int)threadIdx.x < lim) tdeg[threadIdx.x] = a.deg[b0 + threadIdx.x];
        __syncthreads();
        if (live) {
            for (int j = 0; j < lim; ++j) {
                const int g = (int)(b0 + j);
                if (g <= f || tdeg[j]) continue;
                int cls;
                if (!mc_pair(a, f, A, ia, ba, g, tile + 9 * j, tidx + 3 * j, tbox + 6 * j, t, &cls)) continue;
                if (a.packed) a.packed[a.start[f] + atomicAdd(&a.cursor[f], 1)] = (g << 2) | cls;      // sorted afterwards
                ++t.stored;
            }
        }
        __syncthreads();
    }
    if (!a.packed) {
        if (live && t.stored) atomicAdd(&a.count[f], t.stored);
        if (live && t.flags) atomicOr(&a.fflag[f], t.flags);
        mc_tally(a, t);
    }
}

// Non-manifold vertices.  Faces are neighbours across an undirected edge that exactly two faces use (edges of more than two
// faces connect nothing, as in the repair; on an oriented mesh this is the handle's adj).  vdeg: faces at the vertex,
// vmin: the smallest of them.
__global__ __launch_bounds__(256) void p2s_mc_vertex_faces_kernel(const int *__restrict__ fidx, long long F, int *__restrict__ vdeg,
                                                                  int *__restrict__ vmin) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int id[3] = {fidx[3 * f], fidx[3 * f + 1], fidx[3 * f + 2]};
    for (int j = 0; j < 3; ++j) {
        if ((j > 0 && id[j] == id[0]) || (j > 1 && id[j] == id[1])) continue;       // a repeated index counts once
        atomicAdd(&vdeg[id[j]], 1);
        atomicMin(&vmin[id[j]], (int)f);
    }
}
// The fan of vertex v: from its smallest face f0 across the edge (v, w) to the other face of that edge, whose third vertex
// is the next w, first from the corner after v, then, unless the fan closed, from the corner before it.  The vertex is
// flagged when the walk reaches fewer faces than the vertex has.
__global__ __launch_bounds__(256) void p2s_mc_fan_kernel(const int *__restrict__ fidx, long long V, EdgeTable t, const int *__restrict__ fmn,
                                                         const int *__restrict__ fmx, const int *__restrict__ vdeg,
                                                         const int *__restrict__ vmin, int *__restrict__ vflag) {
    const long long vl = (long long)blockIdx.x * 256 + threadIdx.x;
    if (vl >= V) return;
    const int v = (int)vl, deg = vdeg[v];
    int flag = 0;
    if (deg > 0) {
        const int f0 = vmin[v];
        const int id[3] = {fidx[3 * (long long)f0], fidx[3 * (long long)f0 + 1], fidx[3 * (long long)f0 + 2]};
        const int j = id[0] == v ? 0 : (id[1] == v ? 1 : 2);
        int reached = 1;
        bool closed = false;
        for (int dir = 0; dir < 2 && !closed; ++dir) {
            int w = id[(j + 1 + dir) % 3], cur = f0;
            while (reached < deg) {
                const unsigned h = rp_edge_slot(t, v, w);
                if (t.cnt[2 * h] + t.cnt[2 * h + 1] != 2) break;
                const int g = fmn[h] + fmx[h] - cur;
                if (g == cur) break;
                if (g == f0) {
                    closed = true;
                    break;
                }
                ++reached;
                const long long g3 = 3 * (long long)g;
                w = fidx[g3] + fidx[g3 + 1] + fidx[g3 + 2] - v - w;
                cur = g;
            }
        }
        flag = reached < deg ? 1 : 0;
    }
    vflag[v] = flag;
}

// the flag words as bytes (outputs may be NULL) and, with ctr, the faces in an intersecting or coplanar pair and the
// flagged vertices
__global__ __launch_bounds__(256) void p2s_mc_flags_kernel(const int *__restrict__ fflag, long long F, const int *__restrict__ vflag,
                                                           long long V, unsigned char *__restrict__ face_out,
                                                           unsigned char *__restrict__ vert_out, unsigned long long *ctr) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    unsigned long long nf = 0, nv = 0;
    if (i < F) {
        const int w = fflag[i];
        if (face_out) face_out[i] = (unsigned char)w;
        nf = (w & 3) ? 1 : 0;
    }
    if (i < V) {
        const int w = vflag[i];
        if (vert_out) vert_out[i] = (unsigned char)w;
        nv = w ? 1 : 0;
    }
    if (ctr) {
        wave_count(ctr + CV_FACES, nf);
        wave_count(ctr + CV_VERTS, nv);
    }
}

__global__ __launch_bounds__(256) void p2s_mc_unpack_kernel(const int *__restrict__ start, const int *__restrict__ packed, long long F,
                                                            int *__restrict__ pairs, unsigned char *__restrict__ cls) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int s1 = start[f + 1];
    for (int s = start[f]; s < s1; ++s) {
        const int w = packed[s];
        pairs[2 * (long long)s] = (int)f;
        pairs[2 * (long long)s + 1] = w >> 2;
        if (cls) cls[s] = (unsigned char)(w & 3);
    }
}

struct CheckWs {
    int *fbox, *fflag, *count, *start, *cursor, *packed, *vdeg, *vmin, *vflag, *fmn, *fmx;
    unsigned char *deg;
    EdgeTable t;
    unsigned long long *ctr, *ctr2;
    char *base;
    size_t bytes;
};
CheckWs carve_check(char *base, size_t F, size_t V, unsigned cap) {
    Carver c{base};
    CheckWs w;
    w.fbox = c.take<int>(F * 6);
    w.fflag = c.take<int>(F);
    w.count = c.take<int>(F);
    w.start = c.take<int>(F + 1);
    w.cursor = c.take<int>(F);
    w.vdeg = c.take<int>(V);
    w.vmin = c.take<int>(V);
    w.vflag = c.take<int>(V);
    w.deg = c.take<unsigned char>(F);
    w.t = carve_edges(c, cap);
    w.fmn = c.take<int>(cap);
    w.fmx = c.take<int>(cap);
    w.ctr = c.take<unsigned long long>(8);
    w.ctr2 = c.take<unsigned long long>(8);
    w.packed = nullptr;
    return c.done(w);
}

}  // namespace

extern "C" int p2s_mesh_check(p2s_trimesh_t m, int method, int64_t cap_pairs, int32_t *pairs_out_dev, uint8_t *class_out_dev,
                              uint8_t *face_flags_out_dev, uint8_t *vert_flags_out_dev, int64_t *report_host, void *stream) {
    static const char *const who = "p2s_mesh_check";
    if (report_host)
        for (int k = 0; k < 16; ++k) report_host[k] = 0;
    if (!m || !report_host || (method != 0 && method != 1) || cap_pairs < 0 || (!pairs_out_dev && class_out_dev)) {
        p2s_set_error("p2s_mesh_check: bad argument (method 0 or 1, a report, no classes without pairs)");
        return P2S_EINVAL;
    }
    P2S_HIP_CHECK(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    const long long F = m->F, V = m->V;
    unsigned cap = 1024;
    while ((long long)cap < 6 * F) cap <<= 1;
    PoolScratch pool(m->device, s);
    const CheckWs w = pool.carve([&](char *b) { return carve_check(b, (size_t)F, (size_t)V, cap); });
    if (!w.base) return dev_oom(who, s);
    DEV_CHECK(who, hipMemsetAsync(w.ctr, 0, MESH_COUNTERS, s));
    DEV_CHECK(who, hipMemsetAsync(w.ctr2, 0, MESH_COUNTERS, s));
    DEV_CHECK(who, hipMemsetAsync(w.count, 0, (size_t)F * 4, s));
    DEV_CHECK(who, hipMemsetAsync(w.vdeg, 0, (size_t)V * 4, s));
    DEV_CHECK(who, hipMemsetAsync(w.vmin, 0x7f, (size_t)V * 4, s));
    hipLaunchKernelGGL(p2s_mc_prep_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, m->tri, F, w.fbox, w.deg, w.fflag);

    const double S = m->scale;
    CheckArgs a = {m->tri, m->fidx, w.fbox, w.deg, m->closed ? m->comp : nullptr, F, ((S * S) * S) * 1.1368683772161603e-13,
                   (S * S) * 7.105427357601002e-15, w.fflag, w.count, w.start, w.cursor, nullptr, w.ctr};      // 2^-43, 2^-47
    int parts = 1;
    long long per = F;
    if (method == 1) exhaustive_parts(F, F, CX_TILE, &parts, &per);
    auto pairs_pass = [&] {
        if (method == 0) hipLaunchKernelGGL(p2s_mc_index_kernel, dim3(blocks(F, 64)), dim3(64), 0, s, octree_of(m), a);
        else hipLaunchKernelGGL(p2s_mc_exhaustive_kernel, dim3(blocks(F, 256), parts), dim3(256), 0, s, a, per);
    };
    pairs_pass();

    // the fans
    int rc = build_edges(who, m->fidx, F, w.t, w.fmn, w.fmx, s);
    if (rc != P2S_OK) return rc;
    hipLaunchKernelGGL(p2s_mc_vertex_faces_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, m->fidx, F, w.vdeg, w.vmin);
    hipLaunchKernelGGL(p2s_mc_fan_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, m->fidx, V, w.t, w.fmn, w.fmx, w.vdeg, w.vmin, w.vflag);
    hipLaunchKernelGGL(p2s_mc_flags_kernel, dim3(blocks(std::max(F, V), 256)), dim3(256), 0, s, w.fflag, F, w.vflag, V,
                       (unsigned char *)nullptr, (unsigned char *)nullptr, w.ctr2);
    unsigned long long hc[8] = {}, hv[8] = {};
    if ((rc = read_counters(who, w.ctr, hc, CK_OVERFLOW, "the walk overflowed its stack", s)) != P2S_OK) return rc;
    if ((rc = read_counters(who, w.ctr2, hv, -1, nullptr, s)) != P2S_OK) return rc;

    const unsigned long long hard = hc[CK_INTERSECTING] + hc[CK_COPLANAR], stored = hard + hc[CK_TOUCHING];
    const int64_t rep[16] = {F - m->n_degenerate, m->n_degenerate, (int64_t)hc[CK_CANDIDATES], (int64_t)hc[CK_INTERSECTING],
                             (int64_t)hc[CK_COPLANAR], (int64_t)hc[CK_TOUCHING], (int64_t)hc[CK_DUPLICATE], (int64_t)hv[CV_FACES],
                             m->closed ? (int64_t)hc[CK_INSIDE] : -1, m->closed ? (int64_t)(hard - hc[CK_INSIDE]) : -1,
                             (int64_t)hv[CV_VERTS], (int64_t)stored, 0, 0, 0, 0};
    for (int k = 0; k < 16; ++k) report_host[k] = rep[k];
    if (stored > 0x7fffffffull) {
        p2s_set_error("p2s_mesh_check: %llu pairs to store, more than the layout holds", stored);
        return P2S_EINVAL;
    }
    if (pairs_out_dev && (unsigned long long)cap_pairs < stored) {
        p2s_set_error("p2s_mesh_check: room for %lld pairs, %llu needed (report [11])", (long long)cap_pairs, stored);
        return P2S_EINVAL;
    }
    if (pairs_out_dev && stored > 0) {
        a.packed = pool.get<int>((size_t)stored);
        if (!a.packed) return dev_oom(who, s);
        DEV_CHECK(who, hipMemsetAsync(w.cursor, 0, (size_t)F * 4, s));
        hipLaunchKernelGGL(p2s_scan_kernel, dim3(1), dim3(1024), 0, s, w.count, F, w.start);
        pairs_pass();
        hipLaunchKernelGGL(p2s_md_cell_sort_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, w.start, F, a.packed);
        hipLaunchKernelGGL(p2s_mc_unpack_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, w.start, a.packed, F, pairs_out_dev, class_out_dev);
    }
    if (face_flags_out_dev || vert_flags_out_dev)
        hipLaunchKernelGGL(p2s_mc_flags_kernel, dim3(blocks(std::max(F, V), 256)), dim3(256), 0, s, w.fflag, F, w.vflag, V, face_flags_out_dev,
                           vert_flags_out_dev, (unsigned long long *)nullptr);
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipStreamSynchronize(s));
    return P2S_OK;
}
