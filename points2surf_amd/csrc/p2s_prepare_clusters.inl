// the clusters of a point cloud -- the classes of "i and j lie within `radius`", transitively closed -- and the
// removal of the small ones.  Definition: include/p2s_hip.h (p2s_prepare_clusters).  Included at the end of p2s_prepare.hip: the
// scratch, the bounding box, the compaction and the argument checks are that file's.
//   p2s_pp_cl_key_kernel       the 64-bit key (cx << 40 | cy << 20 | cz) of a point's cell
//   p2s_pp_cl_gather_kernel    the points in the order of the sorted keys (hipcub radix sort of (key, id))
//   p2s_pp_cl_pair_kernel      the hot kernel: one thread per sorted point; the 27 neighbouring cells are 9 columns of up to
//                              three consecutive keys, each found by one binary search in the sorted keys and walked; a pair
//                              is tested once, by its earlier end; behind the first round two ends that already share a parent
//                              are skipped before the distance is computed; a linked pair hooks the larger root to the smaller
//                              (atomicMin)
//   p2s_uf_compress_kernel     (p2s_devprim.inl) parent[i] = root, between the rounds
//   p2s_pp_cl_size_kernel      points per root: the lanes of a wave that share a root count among themselves
//   p2s_pp_cl_stats_kernel     clusters; the largest, of equal ones the smallest label (integer atomicMax over a packed word)
//   p2s_pp_cl_flag_kernel      the keep flags for pp_compact; the clusters removed
// The cells have the edge radius (1 + 2^-20): the link test rounds (two squares, two sums), a point's cell index rounds
// (a difference, a quotient, together below 2^-32 of a cell at 2^20 cells on an axis), and with the margin two linked
// points always lie in cells whose indices differ by at most one on every axis.  Memory is O(n).  A radius comparable to
// the cloud's extent puts every point into a few cells: the pair tests then number O(n^2).
// Termination: uf_find walks strictly decreasing parents; a round that changes something turns at least one root into
// a non-root for good, so the host loop ends after at most n - 1 such rounds and one that changes nothing; more than
// n + 1 rounds is an internal error.  No thread waits for another.
#include <hipcub/hipcub.hpp>

namespace {

struct PpClGrid {
    double lo[3];
    double cell;
    int n[3];
};
__device__ __forceinline__ unsigned long long pp_cl_key(int cx, int cy, int cz) {
    return ((unsigned long long)cx << 40) | ((unsigned long long)cy << 20) | (unsigned long long)cz;
}
__global__ __launch_bounds__(256) void p2s_pp_cl_key_kernel(const float *__restrict__ pts, int n, PpClGrid g, unsigned long long *__restrict__ key,
                                                            int *__restrict__ id) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double q = floor(((double)pts[3 * (long long)i + a] - g.lo[a]) / g.cell);
        c[a] = (int)fmin(fmax(q, 0.0), (double)(g.n[a] - 1));
    }
    key[i] = pp_cl_key(c[0], c[1], c[2]);
    id[i] = i;
}
__global__ __launch_bounds__(256) void p2s_pp_cl_gather_kernel(const float *__restrict__ pts, const int *__restrict__ sid, int n,
                                                               float *__restrict__ spts) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const long long i = sid[j];
    spts[3 * (long long)j + 0] = pts[3 * i + 0];
    spts[3 * (long long)j + 1] = pts[3 * i + 1];
    spts[3 * (long long)j + 2] = pts[3 * i + 2];
}
__global__ __launch_bounds__(256) void p2s_pp_cl_pair_kernel(const float *__restrict__ spts, const unsigned long long *__restrict__ skey,
                                                             const int *__restrict__ sid, int n, PpClGrid g, double r2, int first,
                                                             int *parent, int *changed) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < n) {
        const unsigned long long mine = skey[j];
        const int cx = (int)(mine >> 40), cy = (int)((mine >> 20) & 0xfffffu), cz = (int)(mine & 0xfffffu);
        const int i = sid[j];
        const double px = spts[3 * (long long)j], py = spts[3 * (long long)j + 1], pz = spts[3 * (long long)j + 2];
        const int z0 = max(cz - 1, 0), z1 = min(cz + 1, g.n[2] - 1);
        for (int ax = max(cx - 1, 0); ax <= min(cx + 1, g.n[0] - 1); ++ax)
            for (int ay = max(cy - 1, 0); ay <= min(cy + 1, g.n[1] - 1); ++ay) {
                const unsigned long long klo = pp_cl_key(ax, ay, z0), khi = pp_cl_key(ax, ay, z1);
                if (khi < mine) continue;                            // every point of this column lies before j: its thread tests the pair
                int lo = j + 1, hi = n;                              // the first position behind j whose key is >= klo
                while (lo < hi) {
                    const int mid = lo + (hi - lo) / 2;
                    if (skey[mid] < klo) lo = mid + 1;
                    else hi = mid;
                }
                for (int k = lo; k < n && skey[k] <= khi; ++k) {
                    const int o = sid[k];
                    // linking needs connectivity, not every pair: behind the first round nearly all ends share a parent already
                    // (compressed between the rounds); in the first round nearly none does, and the coalesced distance comes first
                    if (!first && parent[i] == parent[o]) continue;
                    const double dx = px - (double)spts[3 * (long long)k], dy = py - (double)spts[3 * (long long)k + 1],
                                 dz = pz - (double)spts[3 * (long long)k + 2];
                    if (!((dx * dx + dy * dy) + dz * dz <= r2)) continue;
                    const int ra = uf_find(parent, i), rb = uf_find(parent, o);
                    if (ra != rb) {
                        atomicMin(&parent[max(ra, rb)], min(ra, rb));
                        *changed = 1;
                    }
                }
            }
    }
}
__global__ __launch_bounds__(256) void p2s_pp_cl_size_kernel(const int *__restrict__ parent, int n, int *size) {
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    bool todo = i < n;
    const int r = todo ? parent[i] : -1;
    for (unsigned long long open = __ballot(todo); open; open = __ballot(todo)) {
        const int leader = __ffsll((long long)open) - 1;
        const int lr = __shfl(r, leader);
        const bool mine = todo && r == lr;
        const unsigned long long m = __ballot(mine);
        if (lane == leader) atomicAdd(&size[lr], __popcll(m));
        todo = todo && !mine;
    }
}
// ctr[0] clusters, ctr[1] max over the roots of (size << 32 | ~label)
__global__ __launch_bounds__(256) void p2s_pp_cl_stats_kernel(const int *__restrict__ parent, const int *__restrict__ size, int n,
                                                              unsigned long long *ctr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool root = i < n && parent[i] == i;
    unsigned long long best = root ? (((unsigned long long)(unsigned)size[i] << 32) | (0xffffffffu - (unsigned)i)) : 0ull;
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long o = __shfl_xor(best, d);
        best = o > best ? o : best;
    }
    const unsigned long long m = __ballot(root);
    if ((threadIdx.x & 63) == 0 && m) {
        atomicAdd(&ctr[0], (unsigned long long)__popcll(m));
        atomicMax(&ctr[1], best);
    }
}
__global__ __launch_bounds__(256) void p2s_pp_cl_flag_kernel(const int *__restrict__ parent, const int *__restrict__ size, int n, int least,
                                                             int *__restrict__ flags, int *__restrict__ label, unsigned long long *ctr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool gone = false;
    if (i < n) {
        const int r = parent[i], keep = size[r] >= least;
        flags[i] = keep;
        if (label) label[i] = r;
        gone = r == i && !keep;
    }
    const unsigned long long m = __ballot(gone);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&ctr[2], (unsigned long long)__popcll(m));
}

}  // namespace

extern "C" int p2s_prepare_clusters(const float *pts_dev, int64_t n, double radius, int64_t min_points, int32_t *label_out_dev,
                                    float *pts_out_dev, int32_t *ids_out_dev, int64_t *n_out_host, int64_t *info_host, int device,
                                    void *stream) {
    const char *who = "p2s_prepare_clusters";
    if (int rc = pp_select_args(who, pts_dev, n, pts_out_dev, ids_out_dev, n_out_host)) return rc;
    if (!(radius > 0.0) || !std::isfinite(radius)) {
        p2s_set_error("%s: bad argument (radius = %g is not a positive finite number)", who, radius);
        return P2S_EINVAL;
    }
    if (min_points < 1) {
        p2s_set_error("%s: bad argument (min_points = %lld < 1)", who, (long long)min_points);
        return P2S_EINVAL;
    }
    if (int rc = select_device(who, device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    *n_out_host = 0;
    if (info_host) std::fill(info_host, info_host + 4, (int64_t)0);
    if (n == 0) return P2S_OK;
    PoolScratch scr(device, s);
    unsigned *ctl = scr.get<unsigned>(64);
    if (!ctl) return dev_oom(who, s);
    float box[6];
    if (int rc = pp_box(who, s, pts_dev, (int)n, ctl, box)) return rc;
    PpClGrid g;
    g.cell = radius * (1.0 + 9.5367431640625e-07);                   // 2^-20: see the head of this file
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = (double)box[a];
        const double cells = std::floor(((double)box[3 + a] - (double)box[a]) / g.cell) + 1.0;
        if (!(cells <= 1048576.0)) {
            p2s_set_error("%s: radius too small for this extent (radius = %g needs %.0f cells on axis %d, at most 2^20 are possible)", who, radius,
                          cells, a);
            return P2S_EINVAL;
        }
        g.n[a] = (int)cells;
    }
    const int N = (int)n;
    size_t tmp_bytes = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (int *)nullptr,
                                             (int *)nullptr, N, 0, 60, nullptr);
    unsigned long long *key = scr.get<unsigned long long>((size_t)n), *skey = scr.get<unsigned long long>((size_t)n);
    int *id = scr.get<int>((size_t)n), *sid = scr.get<int>((size_t)n), *parent = scr.get<int>((size_t)n), *size = scr.get<int>((size_t)n),
        *flags = scr.get<int>((size_t)n);
    float *spts = scr.get<float>((size_t)n * 3);
    char *tmp = scr.get<char>(tmp_bytes + 256);
    unsigned long long *ctr = (unsigned long long *)(ctl + 16);      // [0] clusters [1] the largest [2] removed
    if (!key || !skey || !id || !sid || !parent || !size || !flags || !spts || !tmp) return dev_oom(who, s);
    DEV_CHECK(who, hipMemsetAsync(ctr, 0, 32, s));
    DEV_CHECK(who, hipMemsetAsync(size, 0, (size_t)n * 4, s));
    hipLaunchKernelGGL(p2s_pp_cl_key_kernel, dim3(blocks(n)), dim3(256), 0, s, pts_dev, N, g, key, id);
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, key, skey, id, sid, N, 0, 60, s));
    hipLaunchKernelGGL(p2s_pp_cl_gather_kernel, dim3(blocks(n)), dim3(256), 0, s, pts_dev, sid, N, spts);
    hipLaunchKernelGGL(p2s_iota_kernel, dim3(blocks(n)), dim3(256), 0, s, parent, N);
    const double r2 = radius * radius;
    const int rc = until_unchanged(who, "the clusters", n + 1, (int *)ctl, s, [&](long long round) {      // the cap: see the head of this file
        hipLaunchKernelGGL(p2s_pp_cl_pair_kernel, dim3(blocks(n)), dim3(256), 0, s, spts, skey, sid, N, g, r2, round == 0, parent, (int *)ctl);
        hipLaunchKernelGGL(p2s_uf_compress_kernel, dim3(blocks(n)), dim3(256), 0, s, parent, N);
    });
    if (rc != P2S_OK) return rc;
    hipLaunchKernelGGL(p2s_pp_cl_size_kernel, dim3(blocks(n)), dim3(256), 0, s, parent, N, size);
    hipLaunchKernelGGL(p2s_pp_cl_stats_kernel, dim3(blocks(n)), dim3(256), 0, s, parent, size, N, ctr);
    unsigned long long hc[4] = {};
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipMemcpyAsync(hc, ctr, 32, hipMemcpyDeviceToHost, s));
    DEV_CHECK(who, hipStreamSynchronize(s));
    const long long largest = (long long)(hc[1] >> 32), least = std::min<long long>(min_points, largest);
    hipLaunchKernelGGL(p2s_pp_cl_flag_kernel, dim3(blocks(n)), dim3(256), 0, s, parent, size, N, (int)least, flags, label_out_dev, ctr);
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipMemcpyAsync(hc, ctr, 32, hipMemcpyDeviceToHost, s));
    DEV_CHECK(who, hipStreamSynchronize(s));
    if (info_host) {
        info_host[0] = (int64_t)hc[0];
        info_host[1] = largest;
        info_host[2] = (int64_t)(0xffffffffu - (unsigned)(hc[1] & 0xffffffffu));
        info_host[3] = (int64_t)hc[2];
    }
    return pp_compact(who, scr, s, pts_dev, flags, N, pts_out_dev, ids_out_dev, n_out_host);
}
