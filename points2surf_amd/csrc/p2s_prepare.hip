// f12: raw scans -> 04_pts: drop non-finite points, crop gross strays by exact per-axis order statistics, remove
// statistical outliers (the PCL / Open3D definition over the exact kNN of p2s_knn_patch), thin to at most one point per cell of
// an R^3 grid, normalise to the unit cube -- and the way back (restore).
//
//  pp_compact        the one stable compaction behind every selecting stage: flags -> per-block counts -> one-block scan
//                    (p2s_scan_kernel of p2s_devprim.inl, in place) -> scatter of the surviving rows and their ids.
//  rank bisection    the order statistic of rank r is the smallest ordered key K with count(key <= K) > r: built bit by bit from
//                    the top, 32 counting passes (six thresholds at once: two bounds on three axes), no read-back in between.
//  voxel             occupied cells live in an open-addressing hash set of linear cell ids (integer CAS); the winner of a cell is
//                    an integer atomicMin over the float64 distance's bit pattern, then over the id: no order can change it.
//
// All selection logic is float64 with contraction off: tests/prepare_model.py performs the same operations in numpy.  No
// floating-point atomics.  Scratch comes from the device's block cache and returns to it before a call ends (PoolScratch,
// p2s_devcall.h).
#include "p2s_internal.h"
#include "p2s_devcall.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#pragma clang fp contract(off)

namespace {

#include "p2s_devprim.inl"

constexpr long long PP_MAX_N = 1ll << 27;
constexpr int PP_MAX_K = 64, PP_MAX_R = 1024;
constexpr int PP_EMPTY = -1;

// float32 -> unsigned key in the order of the values; -0 counts as +0
__device__ __forceinline__ unsigned pp_key(float x) {
    const unsigned b = (unsigned)__float_as_int(x + 0.0f);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
inline float pp_unkey(unsigned k) {
    const unsigned b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float f;
    memcpy(&f, &b, 4);
    return f;
}
__device__ __forceinline__ bool pp_finite(float x) { return ((unsigned)__float_as_int(x) & 0x7f800000u) != 0x7f800000u; }

// ---------------------------------------------------------------------------------------------
// compaction
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void p2s_pp_block_count_kernel(const int *__restrict__ flags, int n, int *__restrict__ blk) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int cnt = __syncthreads_count(i < n && flags[i] != 0);
    if (threadIdx.x == 0) blk[blockIdx.x] = cnt;
}
__global__ __launch_bounds__(256) void p2s_pp_scatter_kernel(const float *__restrict__ pts, const int *__restrict__ flags, int n,
                                                             const int *__restrict__ off, float *__restrict__ pts_out,
                                                             int *__restrict__ ids_out) {
    __shared__ int wc[4];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int i = blockIdx.x * 256 + t;
    const bool keep = i < n && flags[i] != 0;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wc[w] = __popcll(m);
    __syncthreads();
    if (!keep) return;
    int o = off[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
    for (int j = 0; j < w; ++j) o += wc[j];
    pts_out[3 * (long long)o + 0] = pts[3 * (long long)i + 0];
    pts_out[3 * (long long)o + 1] = pts[3 * (long long)i + 1];
    pts_out[3 * (long long)o + 2] = pts[3 * (long long)i + 2];
    ids_out[o] = i;
}
// flags [n] -> the surviving rows and ids, in input order; synchronises s
int pp_compact(const char *who, PoolScratch &scr, hipStream_t s, const float *pts, const int *flags, int n, float *pts_out, int *ids_out,
               int64_t *m_out) {
    const int nb = (int)blocks(n);
    int *blk = scr.get<int>((size_t)nb + 1);
    if (!blk) return dev_oom(who, s);
    hipLaunchKernelGGL(p2s_pp_block_count_kernel, dim3(nb), dim3(256), 0, s, flags, n, blk);
    hipLaunchKernelGGL(p2s_scan_kernel, dim3(1), dim3(1024), 0, s, blk, (long long)nb, blk);      // in place; blk[nb] = the total
    hipLaunchKernelGGL(p2s_pp_scatter_kernel, dim3(nb), dim3(256), 0, s, pts, flags, n, blk, pts_out, ids_out);
    int m = 0;
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipMemcpyAsync(&m, blk + nb, 4, hipMemcpyDeviceToHost, s));
    DEV_CHECK(who, hipStreamSynchronize(s));
    *m_out = m;
    return P2S_OK;
}
// a stage that is switched off: the input's bytes and 0 .. n - 1
int pp_identity(const char *who, hipStream_t s, const float *pts, int n, float *pts_out, int *ids_out, int64_t *m_out) {
    if (n > 0) {
        DEV_CHECK(who, hipMemcpyAsync(pts_out, pts, (size_t)n * 12, hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(p2s_iota_kernel, dim3(blocks(n)), dim3(256), 0, s, ids_out, n);
        DEV_CHECK(who, hipGetLastError());
    }
    DEV_CHECK(who, hipStreamSynchronize(s));
    *m_out = n;
    return P2S_OK;
}

// ---------------------------------------------------------------------------------------------
// bounding box, non-finite points
// ---------------------------------------------------------------------------------------------
// box [6]: keys of the minima (initially ~0) and maxima (initially 0) per axis; *bad |= 1 for a non-finite coordinate.  A fixed
// grid strides over the points; one atomic per block and bound
__global__ __launch_bounds__(256) void p2s_pp_box_kernel(const float *__restrict__ pts, int n, unsigned *__restrict__ box,
                                                         int *__restrict__ bad) {
    __shared__ unsigned part[4][6];
    unsigned lo[3] = {~0u, ~0u, ~0u}, hi[3] = {0u, 0u, 0u};
    int nonfinite = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float x = pts[3 * i + a];
            if (pp_finite(x)) {
                const unsigned key = pp_key(x);
                lo[a] = min(lo[a], key);
                hi[a] = max(hi[a], key);
            } else {
                nonfinite = 1;
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        for (int d = 32; d > 0; d >>= 1) {
            lo[a] = min(lo[a], (unsigned)__shfl_xor((int)lo[a], d));
            hi[a] = max(hi[a], (unsigned)__shfl_xor((int)hi[a], d));
        }
        if ((threadIdx.x & 63) == 0) {
            part[threadIdx.x >> 6][a] = lo[a];
            part[threadIdx.x >> 6][3 + a] = hi[a];
        }
    }
    const unsigned long long m = __ballot(nonfinite);
    if ((threadIdx.x & 63) == 0 && m) atomicOr(bad, 1);
    __syncthreads();
    if (threadIdx.x < 3) atomicMin(&box[threadIdx.x], min(min(part[0][threadIdx.x], part[1][threadIdx.x]), min(part[2][threadIdx.x], part[3][threadIdx.x])));
    else if (threadIdx.x < 6) atomicMax(&box[threadIdx.x], max(max(part[0][threadIdx.x], part[1][threadIdx.x]), max(part[2][threadIdx.x], part[3][threadIdx.x])));
}
__global__ __launch_bounds__(256) void p2s_pp_finite_flag_kernel(const float *__restrict__ pts, int n, int *__restrict__ flags) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    flags[i] = pp_finite(pts[3 * (long long)i + 0]) && pp_finite(pts[3 * (long long)i + 1]) && pp_finite(pts[3 * (long long)i + 2]);
}

// the bounding box of finite points as floats: lo[3], hi[3]; a non-finite coordinate: P2S_EINVAL.  ctl: 8 words of scratch
int pp_box(const char *who, hipStream_t s, const float *pts, int n, unsigned *ctl, float box[6]) {
    unsigned host[8] = {~0u, ~0u, ~0u, 0u, 0u, 0u, 0u, 0u};
    DEV_CHECK(who, hipMemcpyAsync(ctl, host, sizeof(host), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(p2s_pp_box_kernel, dim3(std::min(blocks(n), 1024u)), dim3(256), 0, s, pts, n, ctl, (int *)(ctl + 6));
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipMemcpyAsync(host, ctl, sizeof(host), hipMemcpyDeviceToHost, s));
    DEV_CHECK(who, hipStreamSynchronize(s));
    if (host[6]) {
        p2s_set_error("%s: non-finite point (p2s_prepare_finite drops them)", who);
        return P2S_EINVAL;
    }
    for (int a = 0; a < 6; ++a) box[a] = pp_unkey(host[a]);
    return P2S_OK;
}

// ---------------------------------------------------------------------------------------------
// crop
// ---------------------------------------------------------------------------------------------
// cnt[j] += points whose key on axis j / 2 is below T[j]  (j = 2 axis + bound).  A fixed grid strides over the points and sends
// one atomic per block and threshold: with one per wave a million points queued 15,625 adds on each of six addresses per pass
__global__ __launch_bounds__(256) void p2s_pp_rank_count_kernel(const float *__restrict__ pts, int n, const unsigned *__restrict__ T,
                                                                int *__restrict__ cnt) {
    __shared__ int part[4][6];
    unsigned t[6];
    int c[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        t[j] = T[j];
        c[j] = 0;
    }
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        unsigned key[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) key[a] = pp_key(pts[3 * i + a]);
#pragma unroll
        for (int j = 0; j < 6; ++j) c[j] += key[j >> 1] < t[j] ? 1 : 0;
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        for (int d = 32; d > 0; d >>= 1) c[j] += __shfl_xor(c[j], d);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][j] = c[j];
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int sum = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
        if (sum) atomicAdd(&cnt[threadIdx.x], sum);
    }
}
// one step of the six bisections: the bit stays set iff no more than rank[j] keys lie below the threshold
__global__ void p2s_pp_rank_step_kernel(unsigned *__restrict__ K, unsigned *__restrict__ T, int *__restrict__ cnt,
                                        const int *__restrict__ rank, int bit) {
    const int j = threadIdx.x;
    if (j >= 6) return;
    if (cnt[j] <= rank[j]) K[j] = T[j];
    T[j] = bit > 0 ? (K[j] | (1u << (bit - 1))) : K[j];
    cnt[j] = 0;
}
struct PpBox {
    double lo[3], hi[3];
};
__global__ __launch_bounds__(256) void p2s_pp_crop_flag_kernel(const float *__restrict__ pts, int n, PpBox b, int *__restrict__ flags) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    bool in = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double x = (double)pts[3 * (long long)i + a];
        in = in && x >= b.lo[a] && x <= b.hi[a];
    }
    flags[i] = in ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------
// statistical outliers
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void p2s_pp_knn_stat_kernel(const float *__restrict__ pts, const int *__restrict__ ids, int n, int k1,
                                                              double kdiv, double *__restrict__ d) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double px = pts[3 * (long long)i + 0], py = pts[3 * (long long)i + 1], pz = pts[3 * (long long)i + 2];
    const int *row = ids + (long long)i * k1;
    double sum = 0.0;
    for (int j = 0; j < k1; ++j) {
        const long long id = row[j];      // inside the cloud (p2s_knn_patch)
        const double dx = (double)pts[3 * id + 0] - px, dy = (double)pts[3 * id + 1] - py, dz = (double)pts[3 * id + 2] - pz;
        sum += sqrt((dx * dx + dy * dy) + dz * dz);
    }
    d[i] = sum / kdiv;
}
// fixed tree: partial[b] = sum over the block of d (MODE 0) or (d - mean)^2 (MODE 1)
__device__ __forceinline__ double pp_block_tree(double v, double *sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (t < st) sh[t] += sh[t + st];
        __syncthreads();
    }
    return sh[0];
}
template <int MODE>
__global__ __launch_bounds__(256) void p2s_pp_sum_kernel(const double *__restrict__ d, int n, double mean, double *__restrict__ partial) {
    __shared__ double sh[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    double v = 0.0;
    if (i < n) {
        const double x = d[i];
        v = MODE == 0 ? x : (x - mean) * (x - mean);
    }
    const double r = pp_block_tree(v, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}
__global__ __launch_bounds__(256) void p2s_pp_sum_final_kernel(const double *__restrict__ partial, int nb, double *__restrict__ out) {
    __shared__ double sh[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) acc += partial[i];
    const double r = pp_block_tree(acc, sh);
    if (threadIdx.x == 0) *out = r;
}
__global__ __launch_bounds__(256) void p2s_pp_outlier_flag_kernel(const double *__restrict__ d, int n, double thr, int *__restrict__ flags) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) flags[i] = d[i] <= thr ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------
// voxel thinning
// ---------------------------------------------------------------------------------------------
struct PpGrid {
    double lo[3];
    double scale;      // R / ext (0 for ext = 0)
    double cell;       // ext / R
    int R;
};
__device__ __forceinline__ int pp_cell(const PpGrid &g, const float *__restrict__ p, double *dist2) {
    int lin = 0;
    double d[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double rel = (double)p[a] - g.lo[a];
        const double f = floor(rel * g.scale);
        const int ia = (int)fmin(f, (double)(g.R - 1));
        const double c = g.lo[a] + ((double)ia + 0.5) * g.cell;
        d[a] = (double)p[a] - c;
        lin = lin * g.R + ia;
    }
    *dist2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    return lin;
}
// the set of occupied cells: keys [2^log2_slots] (PP_EMPTY initially), linear probing; *occupied += cells seen for the first time;
// slot_of [n] (may be NULL): where the point's cell lives
__global__ __launch_bounds__(256) void p2s_pp_vox_insert_kernel(const float *__restrict__ pts, int n, PpGrid g, int *__restrict__ keys,
                                                                int log2_slots, int *__restrict__ slot_of, int *__restrict__ occupied) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int fresh = 0;
    if (i < n) {
        double d2;
        const int cell = pp_cell(g, pts + 3 * (long long)i, &d2);
        // the product's TOP bits: the low ones are those of the cell id, whose low bits are z and y alone
        const unsigned mask = (1u << log2_slots) - 1u;
        unsigned h = ((unsigned)cell * 2654435761u) >> (32 - log2_slots);
        for (;;) {                                   // ends: the table has at least twice as many slots as there are points
            const int prev = atomicCAS(&keys[h], PP_EMPTY, cell);
            if (prev == PP_EMPTY) fresh = 1;
            if (prev == PP_EMPTY || prev == cell) break;
            h = (h + 1u) & mask;
        }
        if (slot_of) slot_of[i] = (int)h;
    }
    const unsigned long long m = __ballot(fresh);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(occupied, __popcll(m));
}
// PASS 0: the smallest squared distance to the centre per cell (the bit pattern of a non-negative double orders as the value);
// PASS 1: among the points at that distance the lowest id
template <int PASS>
__global__ __launch_bounds__(256) void p2s_pp_vox_min_kernel(const float *__restrict__ pts, int n, PpGrid g, const int *__restrict__ slot_of,
                                                             unsigned long long *__restrict__ best_d, int *__restrict__ best_id) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double d2;
    (void)pp_cell(g, pts + 3 * (long long)i, &d2);
    const unsigned long long bits = (unsigned long long)__double_as_longlong(d2);
    const int slot = slot_of[i];
    if (PASS == 0) atomicMin(&best_d[slot], bits);
    else if (bits == best_d[slot]) atomicMin(&best_id[slot], i);
}
__global__ __launch_bounds__(256) void p2s_pp_vox_flag_kernel(int n, const int *__restrict__ slot_of, const int *__restrict__ best_id,
                                                              int *__restrict__ flags) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) flags[i] = best_id[slot_of[i]] == i ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------
// normalise, gather, restore
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void p2s_pp_normalize_kernel(const float *pts, long long n3, double cx, double cy, double cz, double sc,
                                                               float *out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n3) return;
    const int a = (int)(e % 3);
    const double c = a == 0 ? cx : a == 1 ? cy : cz;
    out[e] = (float)(((double)pts[e] - c) * sc);
}
__global__ __launch_bounds__(256) void p2s_pp_gather_kernel(const unsigned *__restrict__ src, long long n_src, int width,
                                                            const int *__restrict__ ids, long long n_out, unsigned *__restrict__ out,
                                                            int *__restrict__ bad) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_out * width) return;
    const long long row = e / width;
    const int col = (int)(e - row * width);
    const long long id = ids[row];
    if (id < 0 || id >= n_src) {
        atomicOr(bad, 1);
        out[e] = 0u;
        return;
    }
    out[e] = src[id * width + col];
}
__global__ __launch_bounds__(256) void p2s_pp_restore_kernel(const float *__restrict__ v, long long n3, double cx, double cy, double cz,
                                                             double scale, double *__restrict__ out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n3) return;
    const int a = (int)(e % 3);
    const double c = a == 0 ? cx : a == 1 ? cy : cz;
    out[e] = (double)v[e] / scale + c;
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
int pp_count_arg(const char *who, int64_t n) {
    if (n < 0 || n > PP_MAX_N) {
        p2s_set_error("%s: bad argument (n = %lld outside 0 .. 2^27)", who, (long long)n);
        return P2S_EINVAL;
    }
    return P2S_OK;
}
int pp_select_args(const char *who, const float *pts, int64_t n, const float *pts_out, const int32_t *ids_out, const int64_t *n_out) {
    if (!pts || !pts_out || !ids_out || !n_out) {
        p2s_set_error("%s: bad argument (%s is NULL)", who, !pts ? "pts_dev" : !pts_out ? "pts_out_dev" : !ids_out ? "ids_out_dev" : "n_out_host");
        return P2S_EINVAL;
    }
    return pp_count_arg(who, n);
}
struct PpCloud {                 // the cloud handle of one outlier call
    p2s_cloud_t c = nullptr;
    ~PpCloud() {
        if (c) (void)p2s_cloud_destroy(c);
    }
};

}  // namespace

extern "C" int p2s_prepare_finite(const float *pts_dev, int64_t n, float *pts_out_dev, int32_t *ids_out_dev, int64_t *n_out_host, int device,
                                  void *stream) {
    const char *who = "p2s_prepare_finite";
    if (int rc = pp_select_args(who, pts_dev, n, pts_out_dev, ids_out_dev, n_out_host)) return rc;
    if (int rc = select_device(who, device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    *n_out_host = 0;
    if (n == 0) return P2S_OK;
    PoolScratch scr(device, s);
    int *flags = scr.get<int>((size_t)n);
    if (!flags) return dev_oom(who, s);
    hipLaunchKernelGGL(p2s_pp_finite_flag_kernel, dim3(blocks(n)), dim3(256), 0, s, pts_dev, (int)n, flags);
    return pp_compact(who, scr, s, pts_dev, flags, (int)n, pts_out_dev, ids_out_dev, n_out_host);
}

extern "C" int p2s_prepare_crop(const float *pts_dev, int64_t n, double quantile, double margin, float *pts_out_dev, int32_t *ids_out_dev,
                                int64_t *n_out_host, double *bounds_host, int device, void *stream) {
    const char *who = "p2s_prepare_crop";
    if (int rc = pp_select_args(who, pts_dev, n, pts_out_dev, ids_out_dev, n_out_host)) return rc;
    if (!(quantile >= 0.0 && quantile < 0.5)) {
        p2s_set_error("%s: bad argument (quantile = %g outside [0, 0.5))", who, quantile);
        return P2S_EINVAL;
    }
    if (!(margin >= 0.0) || !std::isfinite(margin)) {
        p2s_set_error("%s: bad argument (margin = %g is negative or not finite)", who, margin);
        return P2S_EINVAL;
    }
    if (int rc = select_device(who, device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    *n_out_host = 0;
    if (bounds_host) std::fill(bounds_host, bounds_host + 12, 0.0);
    if (n == 0) return P2S_OK;
    PoolScratch scr(device, s);
    unsigned *ctl = scr.get<unsigned>(64);
    if (!ctl) return dev_oom(who, s);
    float box[6];
    if (int rc = pp_box(who, s, pts_dev, (int)n, ctl, box)) return rc;
    if (quantile == 0.0) return pp_identity(who, s, pts_dev, (int)n, pts_out_dev, ids_out_dev, n_out_host);
    int *flags = scr.get<int>((size_t)n);
    if (!flags) return dev_oom(who, s);
    // ctl: K [6], T [6], cnt [6], rank [6]
    const int r_lo = (int)std::floor(quantile * (double)(n - 1)), r_hi = (int)std::ceil((1.0 - quantile) * (double)(n - 1));
    unsigned host[24];
    for (int j = 0; j < 6; ++j) {
        host[j] = 0u;
        host[6 + j] = 0x80000000u;
        host[12 + j] = 0u;
        host[18 + j] = (unsigned)((j & 1) ? r_hi : r_lo);
    }
    DEV_CHECK(who, hipMemcpyAsync(ctl, host, sizeof(host), hipMemcpyHostToDevice, s));
    for (int bit = 31; bit >= 0; --bit) {
        hipLaunchKernelGGL(p2s_pp_rank_count_kernel, dim3(std::min(blocks(n), 1024u)), dim3(256), 0, s, pts_dev, (int)n, ctl + 6, (int *)(ctl + 12));
        hipLaunchKernelGGL(p2s_pp_rank_step_kernel, dim3(1), dim3(64), 0, s, ctl, ctl + 6, (int *)(ctl + 12), (const int *)(ctl + 18), bit);
    }
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipMemcpyAsync(host, ctl, 24, hipMemcpyDeviceToHost, s));
    DEV_CHECK(who, hipStreamSynchronize(s));
    PpBox b;
    double stat[6];
    for (int a = 0; a < 3; ++a) {
        const double lo = (double)pp_unkey(host[2 * a]), hi = (double)pp_unkey(host[2 * a + 1]);
        const double w = margin * (hi - lo);
        stat[a] = lo;
        stat[3 + a] = hi;
        b.lo[a] = lo - w;
        b.hi[a] = hi + w;
    }
    if (bounds_host) {
        for (int a = 0; a < 3; ++a) {
            bounds_host[a] = stat[a];
            bounds_host[3 + a] = stat[3 + a];
            bounds_host[6 + a] = b.lo[a];
            bounds_host[9 + a] = b.hi[a];
        }
    }
    hipLaunchKernelGGL(p2s_pp_crop_flag_kernel, dim3(blocks(n)), dim3(256), 0, s, pts_dev, (int)n, b, flags);
    return pp_compact(who, scr, s, pts_dev, flags, (int)n, pts_out_dev, ids_out_dev, n_out_host);
}

extern "C" int p2s_prepare_outliers(const float *pts_dev, int64_t n, int k, double std_ratio, double *d_out_dev, float *pts_out_dev,
                                    int32_t *ids_out_dev, int64_t *n_out_host, double *info_host, int device, void *stream) {
    const char *who = "p2s_prepare_outliers";
    if (int rc = pp_select_args(who, pts_dev, n, pts_out_dev, ids_out_dev, n_out_host)) return rc;
    if (k < 1 || k > PP_MAX_K) {
        p2s_set_error("%s: bad argument (k = %d outside 1 .. %d)", who, k, PP_MAX_K);
        return P2S_EINVAL;
    }
    if (!(std_ratio >= 0.0) || !std::isfinite(std_ratio)) {
        p2s_set_error("%s: bad argument (std_ratio = %g is negative or not finite)", who, std_ratio);
        return P2S_EINVAL;
    }
    if (int rc = select_device(who, device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    *n_out_host = 0;
    if (info_host) std::fill(info_host, info_host + 4, 0.0);
    if (n == 0) return P2S_OK;
    PoolScratch scr(device, s);
    if (std_ratio == 0.0 || n < 2) {
        unsigned *ctl = scr.get<unsigned>(64);
        if (!ctl) return dev_oom(who, s);
        float box[6];
        if (int rc = pp_box(who, s, pts_dev, (int)n, ctl, box)) return rc;
        return pp_identity(who, s, pts_dev, (int)n, pts_out_dev, ids_out_dev, n_out_host);
    }
    k = (int)std::min<int64_t>(k, n - 1);
    const int k1 = k + 1, nb = (int)blocks(n);
    int *flags = scr.get<int>((size_t)n), *ids = scr.get<int>((size_t)n * k1);
    double *d = d_out_dev ? d_out_dev : scr.get<double>((size_t)n), *partial = scr.get<double>((size_t)nb + 1);
    if (!flags || !ids || !d || !partial) return dev_oom(who, s);
    PpCloud cloud;
    if (int rc = p2s_cloud_create(pts_dev, (int)n, device, stream, &cloud.c)) return rc;      // refuses non-finite points
    if (int rc = p2s_knn_patch(cloud.c, cloud.c->d.pts, n, k1, ids, nullptr, nullptr, stream)) return rc;
    hipLaunchKernelGGL(p2s_pp_knn_stat_kernel, dim3(nb), dim3(256), 0, s, pts_dev, ids, (int)n, k1, (double)k, d);
    double sum = 0.0, sq = 0.0;
    hipLaunchKernelGGL(p2s_pp_sum_kernel<0>, dim3(nb), dim3(256), 0, s, d, (int)n, 0.0, partial);
    hipLaunchKernelGGL(p2s_pp_sum_final_kernel, dim3(1), dim3(256), 0, s, partial, nb, partial + nb);
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipMemcpyAsync(&sum, partial + nb, 8, hipMemcpyDeviceToHost, s));
    DEV_CHECK(who, hipStreamSynchronize(s));
    const double mean = sum / (double)n;
    hipLaunchKernelGGL(p2s_pp_sum_kernel<1>, dim3(nb), dim3(256), 0, s, d, (int)n, mean, partial);
    hipLaunchKernelGGL(p2s_pp_sum_final_kernel, dim3(1), dim3(256), 0, s, partial, nb, partial + nb);
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipMemcpyAsync(&sq, partial + nb, 8, hipMemcpyDeviceToHost, s));
    DEV_CHECK(who, hipStreamSynchronize(s));
    const double sd = std::sqrt(sq / (double)n);
    const double spread = std_ratio * sd;
    const double thr = mean + spread;
    if (info_host) {
        info_host[0] = mean;
        info_host[1] = sd;
        info_host[2] = thr;
        info_host[3] = (double)k;
    }
    hipLaunchKernelGGL(p2s_pp_outlier_flag_kernel, dim3(nb), dim3(256), 0, s, d, (int)n, thr, flags);
    return pp_compact(who, scr, s, pts_dev, flags, (int)n, pts_out_dev, ids_out_dev, n_out_host);
}

extern "C" int p2s_prepare_voxel_thin(const float *pts_dev, int64_t n, int64_t max_points, int resolution, float *pts_out_dev,
                                      int32_t *ids_out_dev, int64_t *n_out_host, int64_t *info_host, int device, void *stream) {
    const char *who = "p2s_prepare_voxel_thin";
    if (int rc = pp_select_args(who, pts_dev, n, pts_out_dev, ids_out_dev, n_out_host)) return rc;
    if (resolution < 0 || resolution > PP_MAX_R || (resolution == 0 && max_points < 1)) {
        p2s_set_error("%s: bad argument (resolution = %d outside 1 .. %d%s)", who, resolution, PP_MAX_R,
                      resolution == 0 ? " and no max_points >= 1 to search one for" : "");
        return P2S_EINVAL;
    }
    if (int rc = select_device(who, device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    *n_out_host = 0;
    if (info_host) info_host[0] = info_host[1] = 0;
    if (n == 0) return P2S_OK;
    PoolScratch scr(device, s);
    unsigned *ctl = scr.get<unsigned>(64);
    if (!ctl) return dev_oom(who, s);
    float box[6];
    if (int rc = pp_box(who, s, pts_dev, (int)n, ctl, box)) return rc;
    if (resolution == 0 && n <= max_points) return pp_identity(who, s, pts_dev, (int)n, pts_out_dev, ids_out_dev, n_out_host);
    double ext = 0.0;
    for (int a = 0; a < 3; ++a) ext = std::max(ext, (double)box[3 + a] - (double)box[a]);
    auto grid = [&](int R) {
        PpGrid g;
        for (int a = 0; a < 3; ++a) g.lo[a] = (double)box[a];
        g.scale = ext > 0.0 ? (double)R / ext : 0.0;
        g.cell = ext / (double)R;
        g.R = R;
        return g;
    };
    int log2_slots = 10;
    while ((1ll << log2_slots) < 2 * (long long)n) ++log2_slots;      // <= 28
    const unsigned cap = 1u << log2_slots;
    int *flags = scr.get<int>((size_t)n), *slot_of = scr.get<int>((size_t)n), *keys = scr.get<int>(cap), *best_id = scr.get<int>(cap);
    unsigned long long *best_d = scr.get<unsigned long long>(cap);
    int *occ_dev = (int *)(ctl + 8);
    if (!flags || !slot_of || !keys || !best_id || !best_d) return dev_oom(who, s);
    int occupied = 0;
    auto insert = [&](int R, int *slots) -> int {
        DEV_CHECK(who, hipMemsetAsync(keys, 0xff, (size_t)cap * 4, s));
        DEV_CHECK(who, hipMemsetAsync(occ_dev, 0, 4, s));
        hipLaunchKernelGGL(p2s_pp_vox_insert_kernel, dim3(blocks(n)), dim3(256), 0, s, pts_dev, (int)n, grid(R), keys, log2_slots, slots, occ_dev);
        DEV_CHECK(who, hipGetLastError());
        DEV_CHECK(who, hipMemcpyAsync(&occupied, occ_dev, 4, hipMemcpyDeviceToHost, s));
        DEV_CHECK(who, hipStreamSynchronize(s));
        return P2S_OK;
    };
    int R = resolution;
    if (R == 0) {
        // count(R) is not monotone over grids that do not nest: this search IS the definition of R
        int lo = 1, hi = PP_MAX_R;
        while (lo < hi) {
            const int mid = (lo + hi + 1) / 2;
            if (int rc = insert(mid, nullptr)) return rc;
            if (occupied <= max_points) lo = mid;
            else hi = mid - 1;
        }
        R = lo;
    }
    if (int rc = insert(R, slot_of)) return rc;
    const PpGrid g = grid(R);
    DEV_CHECK(who, hipMemsetAsync(best_d, 0xff, (size_t)cap * 8, s));
    DEV_CHECK(who, hipMemsetAsync(best_id, 0x7f, (size_t)cap * 4, s));
    hipLaunchKernelGGL(p2s_pp_vox_min_kernel<0>, dim3(blocks(n)), dim3(256), 0, s, pts_dev, (int)n, g, slot_of, best_d, best_id);
    hipLaunchKernelGGL(p2s_pp_vox_min_kernel<1>, dim3(blocks(n)), dim3(256), 0, s, pts_dev, (int)n, g, slot_of, best_d, best_id);
    hipLaunchKernelGGL(p2s_pp_vox_flag_kernel, dim3(blocks(n)), dim3(256), 0, s, (int)n, slot_of, best_id, flags);
    if (info_host) {
        info_host[0] = R;
        info_host[1] = occupied;
    }
    return pp_compact(who, scr, s, pts_dev, flags, (int)n, pts_out_dev, ids_out_dev, n_out_host);
}

extern "C" int p2s_prepare_normalize(const float *pts_dev, int64_t n, float *pts_out_dev, double *info_host, int device, void *stream) {
    const char *who = "p2s_prepare_normalize";
    if (!pts_dev || !pts_out_dev) {
        p2s_set_error("%s: bad argument (%s is NULL)", who, !pts_dev ? "pts_dev" : "pts_out_dev");
        return P2S_EINVAL;
    }
    if (n < 1 || n > PP_MAX_N) {
        p2s_set_error("%s: bad argument (n = %lld outside 1 .. 2^27)", who, (long long)n);
        return P2S_EINVAL;
    }
    if (int rc = select_device(who, device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    PoolScratch scr(device, s);
    unsigned *ctl = scr.get<unsigned>(64);
    if (!ctl) return dev_oom(who, s);
    float box[6];
    if (int rc = pp_box(who, s, pts_dev, (int)n, ctl, box)) return rc;
    double c[3], ext = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double lo = box[a], hi = box[3 + a];
        c[a] = (lo + hi) * 0.5;
        ext = std::max(ext, hi - lo);
    }
    if (!(ext > 0.0)) {
        p2s_set_error("%s: extent 0 (all %lld points coincide)", who, (long long)n);
        return P2S_EFLAT;
    }
    const double sc = 1.0 / ext;
    hipLaunchKernelGGL(p2s_pp_normalize_kernel, dim3(blocks(3 * n)), dim3(256), 0, s, pts_dev, (long long)(3 * n), c[0], c[1], c[2], sc,
                       pts_out_dev);
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

extern "C" int p2s_prepare_gather(const void *src_dev, int64_t n_src, int width, const int32_t *ids_dev, int64_t n_ids, void *out_dev,
                                  int device, void *stream) {
    const char *who = "p2s_prepare_gather";
    if (!src_dev || !ids_dev || !out_dev) {
        p2s_set_error("%s: bad argument (%s is NULL)", who, !src_dev ? "src_dev" : !ids_dev ? "ids_dev" : "out_dev");
        return P2S_EINVAL;
    }
    if (width < 1 || width > 16) {
        p2s_set_error("%s: bad argument (width = %d outside 1 .. 16)", who, width);
        return P2S_EINVAL;
    }
    if (int rc = pp_count_arg(who, n_src)) return rc;
    if (int rc = pp_count_arg(who, n_ids)) return rc;
    if (int rc = select_device(who, device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (n_ids == 0) return P2S_OK;
    PoolScratch scr(device, s);
    int *bad = scr.get<int>(1);
    if (!bad) return dev_oom(who, s);
    int host = 0;
    DEV_CHECK(who, hipMemsetAsync(bad, 0, 4, s));
    hipLaunchKernelGGL(p2s_pp_gather_kernel, dim3(blocks(n_ids * width)), dim3(256), 0, s, (const unsigned *)src_dev, (long long)n_src, width,
                       ids_dev, (long long)n_ids, (unsigned *)out_dev, bad);
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipMemcpyAsync(&host, bad, 4, hipMemcpyDeviceToHost, s));
    DEV_CHECK(who, hipStreamSynchronize(s));
    if (host) {
        p2s_set_error("%s: an id outside [0, %lld)", who, (long long)n_src);
        return P2S_EINVAL;
    }
    return P2S_OK;
}

extern "C" int p2s_prepare_restore(const float *verts_dev, int64_t n, const double *centre_host, double scale, double *out_dev, int device,
                                   void *stream) {
    const char *who = "p2s_prepare_restore";
    if (!verts_dev || !centre_host || !out_dev) {
        p2s_set_error("%s: bad argument (%s is NULL)", who, !verts_dev ? "verts_dev" : !centre_host ? "centre_host" : "out_dev");
        return P2S_EINVAL;
    }
    if (!(scale > 0.0) || !std::isfinite(scale)) {
        p2s_set_error("%s: bad argument (scale = %g is not a positive finite number)", who, scale);
        return P2S_EINVAL;
    }
    if (int rc = pp_count_arg(who, n)) return rc;
    if (int rc = select_device(who, device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) return P2S_OK;
    hipLaunchKernelGGL(p2s_pp_restore_kernel, dim3(blocks(3 * n)), dim3(256), 0, s, verts_dev, (long long)(3 * n), centre_host[0],
                       centre_host[1], centre_host[2], scale, out_dev);
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipStreamSynchronize(s));
    return P2S_OK;
}

// ---- the clusters of a cloud and the removal of the small ones
#include "p2s_prepare_clusters.inl"
