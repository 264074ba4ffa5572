// f11: point normals from the cloud alone: the PCA normal of every point's k nearest neighbours and a
// deterministic, parallel orientation of the field (Hoppe's propagation along the minimum spanning forest of the kNN graph).
//
//  p2s_normals_estimate  the neighbourhood of p2s_knn_patch (fp64 ranking, ties by id) -> centroid and covariance in float64
//                        -> cyclic Jacobi, NR_SWEEPS sweeps (no trip count depends on the data) -> the eigenvector of the
//                        smallest eigenvalue, normalised in float64, rounded once to float32.
//  p2s_normals_orient    Boruvka rounds over the directed kNN edges.  The order of the edges is total -- (w, min id, max id) --
//                        so the forest is unique, and every reduction is an integer atomicMin / atomicMax: the result does not
//                        depend on scheduling.  Parities ride on the union-find links as in p2s_meshrepair.inl (rp_find_par).
//
// All float64 with contraction off: tests/normals_model.py performs the same operations for d, the only value whose bits
// decide anything.  Scratch comes from the device's block cache and returns to it before a call ends.
#include "p2s_internal.h"
#include "p2s_devcall.h"
#include <algorithm>
#include <vector>

#pragma clang fp contract(off)

namespace {

constexpr int NR_MIN_K = 4, NR_MAX_K = 64;
constexpr int NR_SWEEPS = 8;       // a 3 x 3 symmetric matrix is diagonal to the last bit after 4 or 5; quadratic convergence
constexpr unsigned long long NR_NONE = ~0ull;
constexpr int NR_BATCH = 4;        // Boruvka rounds between two reads of the hook counts
constexpr int NR_MAX_ROUNDS = 32;  // 2^rounds <= n <= 2^30, rounded up to whole batches
// ctl: [0] non-finite normal, [2] components, [3] normals flipped, [NR_CTL_ROUND + r] hooks of round r
constexpr int NR_CTL_ROUND = 4, NR_CTL = NR_CTL_ROUND + NR_MAX_ROUNDS + NR_BATCH;

// ---------------------------------------------------------------------------------------------
// estimate: one thread per point
// ---------------------------------------------------------------------------------------------
// one Jacobi rotation of the symmetric a (upper triangle: a[0] xx, a[1] xy, a[2] xz, a[3] yy, a[4] yz, a[5] zz) in the
// plane (P, Q); R the third axis; v the eigenvector columns.  An off-diagonal element that is exactly 0 leaves a and v
// untouched (c = 1, s = 0), so a matrix that is diagonal in an axis keeps that axis exactly.
template <int P, int Q, int R>
__device__ __forceinline__ void nr_rotate(double (&m)[3][3], double (&v)[3][3]) {
    const double apq = m[P][Q];
    const double theta = (m[Q][Q] - m[P][P]) / (2.0 * apq);
    double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    if (apq == 0.0) t = 0.0;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    const double app = m[P][P] - t * apq, aqq = m[Q][Q] + t * apq;
    const double arp = c * m[R][P] - s * m[R][Q], arq = s * m[R][P] + c * m[R][Q];
    m[P][P] = app;
    m[Q][Q] = aqq;
    m[P][Q] = m[Q][P] = 0.0;
    m[R][P] = m[P][R] = arp;
    m[R][Q] = m[Q][R] = arq;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double vp = c * v[r][P] - s * v[r][Q], vq = s * v[r][P] + c * v[r][Q];
        v[r][P] = vp;
        v[r][Q] = vq;
    }
}

__global__ __launch_bounds__(256) void nr_pca_kernel(const float *__restrict__ pts, const int *__restrict__ ids, int n, int k,
                                                     float *__restrict__ normals, float *__restrict__ variation) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int *row = ids + (long long)i * k;
    // the ids of p2s_knn_patch lie inside the cloud (a non-finite query's are clamped there)
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int j = 0; j < k; ++j) {
        const int id = row[j];
        sx += (double)pts[3 * id + 0];
        sy += (double)pts[3 * id + 1];
        sz += (double)pts[3 * id + 2];
    }
    const double cx = sx / (double)k, cy = sy / (double)k, cz = sz / (double)k;
    double xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
    for (int j = 0; j < k; ++j) {
        const int id = row[j];
        const double dx = (double)pts[3 * id + 0] - cx, dy = (double)pts[3 * id + 1] - cy, dz = (double)pts[3 * id + 2] - cz;
        xx += dx * dx;
        xy += dx * dy;
        xz += dx * dz;
        yy += dy * dy;
        yz += dy * dz;
        zz += dz * dz;
    }
    double m[3][3] = {{xx, xy, xz}, {xy, yy, yz}, {xz, yz, zz}};
    double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    const bool zero = xx == 0.0 && yy == 0.0 && zz == 0.0;      // C = 0: the diagonal of a sum of squares
#pragma unroll 1
    for (int sweep = 0; sweep < NR_SWEEPS; ++sweep) {
        nr_rotate<0, 1, 2>(m, v);
        nr_rotate<0, 2, 1>(m, v);
        nr_rotate<1, 2, 0>(m, v);
    }
    // the smallest eigenvalue; of equal ones the first axis
    const double l0 = m[0][0], l1 = m[1][1], l2 = m[2][2];
    int a = 0;
    double lmin = l0;
    if (l1 < lmin) { a = 1; lmin = l1; }
    if (l2 < lmin) { a = 2; lmin = l2; }
    double nx = a == 0 ? v[0][0] : a == 1 ? v[0][1] : v[0][2];
    double ny = a == 0 ? v[1][0] : a == 1 ? v[1][1] : v[1][2];
    double nz = a == 0 ? v[2][0] : a == 1 ? v[2][1] : v[2][2];
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    nx /= len;
    ny /= len;
    nz /= len;
    const double tr = (l0 + l1) + l2;
    float var = (float)(fmax(lmin, 0.0) / tr);
    if (zero || !(tr > 0.0)) {
        nx = ny = nz = 0.0;
        var = 0.0f;
    }
    normals[3 * i + 0] = (float)nx;
    normals[3 * i + 1] = (float)ny;
    normals[3 * i + 2] = (float)nz;
    if (variation) variation[i] = var;
}

// ---------------------------------------------------------------------------------------------
// orient
// ---------------------------------------------------------------------------------------------
// d of the edge {a, b}: symmetric in a and b bit for bit (products commute, the order of the additions is fixed)
__device__ __forceinline__ double nr_dot(const float *__restrict__ nrm, int a, int b) {
    const double ax = nrm[3 * a + 0], ay = nrm[3 * a + 1], az = nrm[3 * a + 2];
    const double bx = nrm[3 * b + 0], by = nrm[3 * b + 1], bz = nrm[3 * b + 2];
    return (ax * bx + ay * by) + az * bz;
}
// w = 1 - |d| as an unsigned key in the order of w: its bit pattern with the sign bit set for w >= 0, complemented for
// w < 0 (|d| > 1: two float32 unit vectors that agree can reach 1 + 2^-23).  w is never -0 and never NaN (finite normals).
__device__ __forceinline__ unsigned long long nr_wkey(double d) {
    const double w = 1.0 - fabs(d);
    const unsigned long long b = (unsigned long long)__double_as_longlong(w);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ unsigned long long nr_pair(int i, int j) {
    return ((unsigned long long)(unsigned)min(i, j) << 32) | (unsigned long long)(unsigned)max(i, j);
}
__device__ __forceinline__ int nr_find(const int *link, int x, int *parity) {
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

// link[i] = i << 1; ctl[0] |= 1 for a non-finite normal
__global__ __launch_bounds__(256) void nr_init_kernel(const float *__restrict__ nrm, int n, int *__restrict__ link, int *__restrict__ ctl) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    link[i] = i << 1;
    const float s = (nrm[3 * i + 0] * 0.0f + nrm[3 * i + 1] * 0.0f) + nrm[3 * i + 2] * 0.0f;      // NaN iff one of them is not finite
    if (s != s) atomicOr(&ctl[0], 1);
}
// undirected edges: the directed edge i -> j (j != i) counts unless j -> i exists as well and j < i
__global__ __launch_bounds__(256) void nr_count_edges_kernel(const int *__restrict__ ids, int n, int k, unsigned long long *__restrict__ cnt) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    int one = 0;
    if (e < (long long)n * k) {
        const int i = (int)(e / k), j = ids[e];
        if (j != i) {
            // a point met twice in one list cannot happen: the ids of one query are distinct
            bool back = false;
            if (j < i) {
                const int *row = ids + (long long)j * k;
                for (int t = 0; t < k; ++t) back = back || row[t] == i;
            }
            one = back ? 0 : 1;
        }
    }
    const unsigned long long m = __ballot(one);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(cnt, (unsigned long long)__popcll(m));
}
__global__ __launch_bounds__(256) void nr_reset_kernel(int n, unsigned long long *__restrict__ best_w, unsigned long long *__restrict__ best_e) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    best_w[i] = NR_NONE;
    best_e[i] = NR_NONE;
}
// PASS 0: the smallest weight key that leaves each component; PASS 1: among the edges of that weight the smallest id pair.
// link is compressed: link[x] >> 1 is the root of x.
template <int PASS>
__global__ __launch_bounds__(256) void nr_min_edge_kernel(const float *__restrict__ nrm, const int *__restrict__ ids, int n, int k,
                                                          const int *__restrict__ link, unsigned long long *__restrict__ best_w,
                                                          unsigned long long *__restrict__ best_e) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)n * k) return;
    const int i = (int)(e / k), j = ids[e];
    if (j == i) return;
    const int ri = link[i] >> 1, rj = link[j] >> 1;
    if (ri == rj) return;
    const unsigned long long key = nr_wkey(nr_dot(nrm, min(i, j), max(i, j)));
    if (PASS == 0) {
        if (key < best_w[ri]) atomicMin(&best_w[ri], key);      // (the plain read only spares atomics: the minimum falls monotonically)
        if (key < best_w[rj]) atomicMin(&best_w[rj], key);
    } else {
        const unsigned long long pr = nr_pair(i, j);
        if (key == best_w[ri] && pr < best_e[ri]) atomicMin(&best_e[ri], pr);
        if (key == best_w[rj] && pr < best_e[rj]) atomicMin(&best_e[rj], pr);
    }
}
// Every root with an edge hooks to the root at the edge's other end; of two roots that chose the same edge the smaller
// stays (the edges chosen in a round form a forest under a total order, but for these pairs).  *hooks += roots hooked.
__global__ __launch_bounds__(256) void nr_hook_kernel(const float *__restrict__ nrm, int n, const int *__restrict__ link_in,
                                                      const unsigned long long *__restrict__ best_e, int *__restrict__ link_out,
                                                      int *__restrict__ hooks) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    int hooked = 0;
    if (r < n) {
        int w = link_in[r];
        const unsigned long long pr = best_e[r];
        if ((w >> 1) == r && pr != NR_NONE) {
            const int lo = (int)(pr >> 32), hi = (int)(pr & 0xffffffffull);
            const int wl = link_in[lo], wh = link_in[hi];
            const int other = (wl >> 1) == r ? (wh >> 1) : (wl >> 1);
            if (!(best_e[other] == pr && r < other)) {
                const int flip = nr_dot(nrm, lo, hi) < 0.0 ? 1 : 0;
                w = (other << 1) | ((wl ^ wh ^ flip) & 1);
                hooked = 1;
            }
        }
        link_out[r] = w;
    }
    const unsigned long long m = __ballot(hooked);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(hooks, __popcll(m));
}
// pointer jumping, the parities xor-ed along the way
__global__ __launch_bounds__(256) void nr_compress_kernel(int *link, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int p;
    const int r = nr_find(link, i, &p);
    __atomic_store_n(&link[i], (r << 1) | p, __ATOMIC_RELAXED);
}
// per component (at its root): the seed = largest z, of equal ones the smallest id; the smallest id.  The lanes of a wave
// that share a root reduce among themselves first and send one atomic: a cloud of one component would otherwise queue all
// of its points on two addresses.  Maximum and minimum are order-free, so the grouping changes no result.
__global__ __launch_bounds__(256) void nr_seed_kernel(const float *__restrict__ pts, int n, const int *__restrict__ link,
                                                      unsigned long long *__restrict__ seed, int *__restrict__ min_id) {
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    bool todo = i < n;
    int r = -1;
    unsigned long long key = 0ull;
    if (todo) {
        r = link[i] >> 1;
        const unsigned zb = (unsigned)__float_as_int(pts[3 * i + 2] + 0.0f);   // -0 -> +0
        const unsigned zk = (zb >> 31) ? ~zb : (zb | 0x80000000u);             // in the order of z
        key = ((unsigned long long)zk << 32) | (unsigned long long)(0xffffffffu - (unsigned)i);
    }
    for (unsigned long long open = __ballot(todo); open; open = __ballot(todo)) {
        const int leader = __ffsll((long long)open) - 1;
        const int lr = __shfl(r, leader);
        const bool mine = todo && r == lr;
        unsigned long long kmax = mine ? key : 0ull;
        int imin = mine ? i : 0x7fffffff;
        for (int d = 32; d > 0; d >>= 1) {
            const unsigned long long ko = __shfl_xor(kmax, d);
            const int io = __shfl_xor(imin, d);
            kmax = ko > kmax ? ko : kmax;
            imin = min(imin, io);
        }
        if (lane == leader) {
            atomicMax(&seed[lr], kmax);
            atomicMin(&min_id[lr], imin);
        }
        todo = todo && !mine;
    }
}
// g[r] of every root: the component is negated as a whole iff its seed's oriented n_z < 0; ctl[2] += components
__global__ __launch_bounds__(256) void nr_component_kernel(const float *__restrict__ nrm, int n, const int *__restrict__ link,
                                                           const unsigned long long *__restrict__ seed, int *__restrict__ neg, int *__restrict__ ctl) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    int root = 0;
    if (r < n && (link[r] >> 1) == r) {
        root = 1;
        const int sd = (int)(0xffffffffu - (unsigned)(seed[r] & 0xffffffffull));
        const float nz = nrm[3 * sd + 2];
        neg[r] = ((link[sd] & 1) ? -nz : nz) < 0.0f ? 1 : 0;
    }
    const unsigned long long m = __ballot(root);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&ctl[2], __popcll(m));
}
// out = in with the sign bits of a flipped point inverted (in may be out); ctl[3] += flipped points
__global__ __launch_bounds__(256) void nr_apply_kernel(const float *nrm_in, int n, const int *__restrict__ link, const int *__restrict__ neg,
                                                       const int *__restrict__ min_id, float *nrm_out, int *__restrict__ component,
                                                       int *__restrict__ ctl) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int flip = 0;
    if (i < n) {
        const int w = link[i], r = w >> 1;
        flip = (w & 1) ^ neg[r];
        const unsigned mask = flip ? 0x80000000u : 0u;
#pragma unroll
        for (int a = 0; a < 3; ++a) nrm_out[3 * i + a] = __int_as_float(__float_as_int(nrm_in[3 * i + a]) ^ (int)mask);
        if (component) component[i] = min_id[r];
    }
    const unsigned long long m = __ballot(flip);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&ctl[3], __popcll(m));
}

int nr_args(const char *who, p2s_cloud_t c, int k) {
    if (!c) {
        p2s_set_error("%s: bad argument (no cloud)", who);
        return P2S_EINVAL;
    }
    if (c->d.n > (1 << 30)) {                        // the links hold id << 1 | parity
        p2s_set_error("%s: more than 2^30 points", who);
        return P2S_EINVAL;
    }
    if (k < NR_MIN_K || k > NR_MAX_K || k > c->d.n) {
        p2s_set_error("%s: k = %d outside %d .. %d or beyond the cloud's %d points", who, k, NR_MIN_K, NR_MAX_K, c->d.n);
        return P2S_EINVAL;
    }
    return P2S_OK;
}

// the k nearest points of every point of the cloud, [n][k], ascending (distance, id)
int nr_neighbours(const char *who, p2s_cloud_t c, int k, PoolScratch &scr, hipStream_t s, int **ids) {
    *ids = scr.get<int>((size_t)c->d.n * k);
    if (!*ids) return dev_oom(who, s);
    return p2s_knn_patch(c, c->d.pts, c->d.n, k, *ids, nullptr, nullptr, s);
}

}  // namespace

extern "C" int p2s_normals_estimate(p2s_cloud_t c, int k, float *normals_out_dev, float *variation_out_dev, void *stream) {
    const char *who = "p2s_normals_estimate";
    if (int rc = nr_args(who, c, k)) return rc;
    if (!normals_out_dev) {
        p2s_set_error("%s: bad argument (no output)", who);
        return P2S_EINVAL;
    }
    P2S_HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    p2s_cloud_note_stream(c, s);
    PoolScratch scr(c->device, s);
    int *ids = nullptr;
    if (int rc = nr_neighbours(who, c, k, scr, s, &ids)) return rc;
    hipLaunchKernelGGL(nr_pca_kernel, dim3(blocks(c->d.n)), dim3(256), 0, s, c->d.pts, ids, c->d.n, k, normals_out_dev, variation_out_dev);
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipStreamSynchronize(s));
    return P2S_OK;
}

extern "C" int p2s_normals_orient(p2s_cloud_t c, int k, const float *normals_in_dev, float *normals_out_dev, int32_t *component_out_dev,
                                  int64_t *info_host, void *stream) {
    const char *who = "p2s_normals_orient";
    if (int rc = nr_args(who, c, k)) return rc;
    if (!normals_in_dev || !normals_out_dev) {
        p2s_set_error("%s: bad argument (no normals)", who);
        return P2S_EINVAL;
    }
    P2S_HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    p2s_cloud_note_stream(c, s);
    const int n = c->d.n;
    const long long E = (long long)n * k;
    PoolScratch scr(c->device, s);
    int *link[2] = {scr.get<int>(n), scr.get<int>(n)}, *neg = scr.get<int>(n), *min_id = scr.get<int>(n), *ctl = scr.get<int>(NR_CTL);
    unsigned long long *best_w = scr.get<unsigned long long>(n), *best_e = scr.get<unsigned long long>(n), *cnt = scr.get<unsigned long long>(1);
    if (!link[0] || !link[1] || !neg || !min_id || !ctl || !best_w || !best_e || !cnt) return dev_oom(who, s);
    int *ids = nullptr;
    if (int rc = nr_neighbours(who, c, k, scr, s, &ids)) return rc;
    int host[NR_CTL] = {};
    DEV_CHECK(who, hipMemsetAsync(ctl, 0, sizeof(host), s));
    DEV_CHECK(who, hipMemsetAsync(cnt, 0, 8, s));
    hipLaunchKernelGGL(nr_init_kernel, dim3(blocks(n)), dim3(256), 0, s, normals_in_dev, n, link[0], ctl);
    hipLaunchKernelGGL(nr_count_edges_kernel, dim3(blocks(E)), dim3(256), 0, s, ids, n, k, cnt);
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipMemcpyAsync(host, ctl, sizeof(host), hipMemcpyDeviceToHost, s));
    DEV_CHECK(who, hipStreamSynchronize(s));
    if (host[0]) {
        p2s_set_error("%s: non-finite normal", who);
        return P2S_EINVAL;
    }
    // A round at least halves the components that still have an edge: n >= 2^rounds.  The rounds go out NR_BATCH at a time
    // between two reads of their hook counts; a round behind the last one that joined anything finds no edge and changes nothing.
    int rounds = 0, cur = 0;
    for (bool open = true; open;) {
        if (rounds >= NR_MAX_ROUNDS) {
            p2s_set_error("%s: the forest did not close in %d rounds (internal error)", who, NR_MAX_ROUNDS);
            return P2S_EHIP;
        }
        for (int r = rounds; r < rounds + NR_BATCH; ++r, cur ^= 1) {
            hipLaunchKernelGGL(nr_reset_kernel, dim3(blocks(n)), dim3(256), 0, s, n, best_w, best_e);
            hipLaunchKernelGGL(nr_min_edge_kernel<0>, dim3(blocks(E)), dim3(256), 0, s, normals_in_dev, ids, n, k, link[cur], best_w, best_e);
            hipLaunchKernelGGL(nr_min_edge_kernel<1>, dim3(blocks(E)), dim3(256), 0, s, normals_in_dev, ids, n, k, link[cur], best_w, best_e);
            hipLaunchKernelGGL(nr_hook_kernel, dim3(blocks(n)), dim3(256), 0, s, normals_in_dev, n, link[cur], best_e, link[cur ^ 1],
                               ctl + NR_CTL_ROUND + r);
            hipLaunchKernelGGL(nr_compress_kernel, dim3(blocks(n)), dim3(256), 0, s, link[cur ^ 1], n);
        }
        DEV_CHECK(who, hipGetLastError());
        DEV_CHECK(who, hipMemcpyAsync(host, ctl, sizeof(host), hipMemcpyDeviceToHost, s));
        DEV_CHECK(who, hipStreamSynchronize(s));
        for (int r = 0; r < NR_BATCH && open; ++r) {
            if (host[NR_CTL_ROUND + rounds]) ++rounds;
            else open = false;
        }
    }
    unsigned long long *seed = best_w;               // free again
    DEV_CHECK(who, hipMemsetAsync(seed, 0, (size_t)n * 8, s));
    DEV_CHECK(who, hipMemsetAsync(min_id, 0x7f, (size_t)n * 4, s));
    hipLaunchKernelGGL(nr_seed_kernel, dim3(blocks(n)), dim3(256), 0, s, c->d.pts, n, link[cur], seed, min_id);
    hipLaunchKernelGGL(nr_component_kernel, dim3(blocks(n)), dim3(256), 0, s, normals_in_dev, n, link[cur], seed, neg, ctl);
    hipLaunchKernelGGL(nr_apply_kernel, dim3(blocks(n)), dim3(256), 0, s, normals_in_dev, n, link[cur], neg, min_id, normals_out_dev,
                       component_out_dev, ctl);
    unsigned long long edges = 0;
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipMemcpyAsync(host, ctl, sizeof(host), hipMemcpyDeviceToHost, s));
    DEV_CHECK(who, hipMemcpyAsync(&edges, cnt, 8, hipMemcpyDeviceToHost, s));
    DEV_CHECK(who, hipStreamSynchronize(s));
    if (info_host) {
        for (int a = 0; a < 8; ++a) info_host[a] = 0;
        info_host[0] = host[2];
        info_host[1] = (int64_t)edges;
        info_host[2] = rounds;                       // rounds that joined components
        info_host[3] = host[3];
    }
    return P2S_OK;
}
