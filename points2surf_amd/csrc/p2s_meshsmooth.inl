// the vertices of a triangle mesh moved by the umbrella operator, lambda | mu (Taubin 1995) or plain Laplacian.
// Definition: include/p2s_hip.h (p2s_mesh_smooth); the project's own, not vcglib's.  Included at the end of p2s_meshdist.hip,
// behind p2s_meshholes.inl: the edge table (EdgeTable, build_edges, rp_table_cap), p2s_mf_repeat_kernel, mc_validate,
// mc_bad_mesh, wave_count, read_counters and the host scaffold are those files', used here and not copied.
//   p2s_smooth_degree_kernel      per occupied slot of the edge table: the degree of both ends, their count of edges of exactly one
//                                 face, a mark at the ends of an edge of more than two faces (integer atomics); the edges counted
//   p2s_smooth_class_kernel       per vertex: the class of rule c and the length of its row -- all neighbours (class 0), the two
//                                 boundary neighbours (class 1), nothing (fixed); the counts of the report
//   p2s_smooth_pairs_kernel       per occupied slot: the directed pairs i -> j that a row of i holds, as keys i << 32 | j, at
//                                 positions that one atomic per workgroup hands out.  The keys are distinct, so the radix sort that
//                                 follows gives one order whatever the arrival: the rows of the CSR, each ascending in j
//   p2s_smooth_col_kernel         the low words of the sorted keys: the column indices
//   p2s_smooth_pack_kernel<S>     the input positions into both ping-pong buffers, records of S floats (S = 3, or 4 with a pad)
//   p2s_smooth_step_kernel<S>     THE HOT PATH, one launch per half-step, one vertex per thread: an empty row is a fixed vertex,
//                                 whose position both buffers hold from the start, so nothing is written; any other row is
//                                 added up in its order, however long it is (the loads do not depend on the sum, so four are
//                                 in flight).  Reads one buffer, writes the other: the update is simultaneous.  No atomic.
//                                 Measured against a wave per row of more than 64 neighbours, which gathered 64 at once and
//                                 added them up in every lane by v_readlane_b32: the sum is sequential by rule d, a wave has
//                                 nothing to add in parallel, and at 3,000 neighbours it took 158 us against this kernel's
//                                 187 us, at 100,000 5.3 ms against 6.2 ms -- not worth a second path
//   p2s_smooth_measure_kernel<S>  the non-finite coordinates of the result and the largest squared displacement (atomicMax on the
//                                 bits of non-negative doubles, one per wave)
//   p2s_smooth_unpack_kernel<S>   the result into verts_out_dev
// Determinism: classes, degrees and counts are integer sums, the rows come out of a sort of distinct keys, every output
// coordinate is computed by one lane in one order with contraction off.  No thread spins on another.  Bounds: a column index
// is an end of an edge of a validated face, so below n_verts; a row lies in [start[i], start[i + 1]) of a scan whose total sized
// the arrays, and the pairs written are counted against that total.

#ifndef P2S_SMOOTH_STRIDE
#define P2S_SMOOTH_STRIDE 3                      // floats per position record of the ping-pong buffers (3, or 4: padded)
#endif

namespace {

constexpr int SMOOTH_STRIDE = P2S_SMOOTH_STRIDE;
static_assert(SMOOTH_STRIDE == 3 || SMOOTH_STRIDE == 4, "position records are 12 or 16 bytes");
enum SmoothCtr { SMOOTH_CLASS0 = 0, SMOOTH_EDGES = 6, SMOOTH_MAXDEG = 7 };                                      // ctr
enum SmoothCtr2 { SMOOTH_PAIR_AT = 0, SMOOTH_NONFINITE, SMOOTH_MAXDISP };                                       // ctr2

template <int S> __device__ __forceinline__ void smooth_load(const float *__restrict__ p, long long j, double *o) {
    if constexpr (S == 4) {
        const float4 q = *reinterpret_cast<const float4 *>(p + 4 * j);
        o[0] = q.x;
        o[1] = q.y;
        o[2] = q.z;
    } else {
        o[0] = p[3 * j];
        o[1] = p[3 * j + 1];
        o[2] = p[3 * j + 2];
    }
}

__global__ __launch_bounds__(256) void p2s_smooth_degree_kernel(EdgeTable t, int *__restrict__ deg, int *__restrict__ bdeg, int *__restrict__ nm,
                                                                unsigned long long *__restrict__ ctr) {
    unsigned long long edges = 0;
    for (unsigned long long i = blockIdx.x * 256ull + threadIdx.x; i <= t.mask; i += gridDim.x * 256ull) {      // any grid
        const unsigned long long key = t.key[i];
        if (key == EDGE_EMPTY) continue;
        const int a = (int)(key >> 32), b = (int)(key & 0xffffffffu), n = t.cnt[2 * i] + t.cnt[2 * i + 1];
        ++edges;
        atomicAdd(&deg[a], 1);
        atomicAdd(&deg[b], 1);
        if (n == 1) {
            atomicAdd(&bdeg[a], 1);
            atomicAdd(&bdeg[b], 1);
        } else if (n > 2) {
            nm[a] = 1;
            nm[b] = 1;
        }
    }
    wave_count(&ctr[SMOOTH_EDGES], edges);
}
// rowlen [V + 1]: the last entry stays 0.  Any grid: a thread keeps its counts over its vertices, a wave adds them up once
__global__ __launch_bounds__(256) void p2s_smooth_class_kernel(long long V, int mode, const unsigned char *__restrict__ fixed,
                                                               const int *__restrict__ deg, const int *__restrict__ bdeg, const int *__restrict__ nm,
                                                               unsigned char *__restrict__ cls, int *__restrict__ rowlen,
                                                               unsigned long long *__restrict__ ctr) {
    unsigned long long count[6] = {0, 0, 0, 0, 0, 0};
    int mx = 0;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < V; v += (long long)gridDim.x * 256) {
        const int d = deg[v], bd = bdeg[v];
        int c;
        if (fixed && fixed[v]) c = 4;
        else if (d == 0) c = 5;
        else if (mode == 2) c = 0;
        else if (nm[v]) c = 3;
        else if (bd > 0) c = (mode == 1 && bd == 2) ? 1 : 2;
        else c = 0;
        const int len = c == 0 ? d : (c == 1 ? 2 : 0);
        cls[v] = (unsigned char)c;
        rowlen[v] = len;
        for (int k = 0; k < 6; ++k) count[k] += c == k;
        mx = max(mx, len);
    }
    for (int k = 0; k < 6; ++k) wave_count(&ctr[SMOOTH_CLASS0 + k], count[k]);
    for (int d = 32; d > 0; d >>= 1) mx = max(mx, __shfl_xor(mx, d));
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(&ctr[SMOOTH_MAXDEG], (unsigned long long)mx);
}
// the directed pairs of slot i that a row holds: a -> b into k0, b -> a behind it
__device__ __forceinline__ int smooth_slot_pairs(const EdgeTable &t, const unsigned char *__restrict__ cls, unsigned long long i,
                                                 unsigned long long *__restrict__ k0, unsigned long long *__restrict__ k1) {
    const unsigned long long key = t.key[i];
    if (key == EDGE_EMPTY) return 0;
    const unsigned a = (unsigned)(key >> 32), b = (unsigned)(key & 0xffffffffu);
    const bool one = t.cnt[2 * i] + t.cnt[2 * i + 1] == 1;
    const int ca = cls[a], cb = cls[b];
    const bool ab = ca == 0 || (ca == 1 && one), ba = cb == 0 || (cb == 1 && one);
    const unsigned long long back = ((unsigned long long)b << 32) | a;
    *k0 = ab ? key : back;
    *k1 = back;
    return (int)ab + (int)ba;
}
// A workgroup takes a run of (mask + 1) / gridDim.x slots, a multiple of 256 (both powers of two, gridDim.x <= (mask + 1) /
// 256): it counts the pairs of its run, takes their room with ONE atomic, and fills it chunk by chunk behind a scan.  (One
// atomic per wave of slots queued 130,000 of them on one address: 1.6 ms on the 256^3 stand-in mesh.)
__global__ __launch_bounds__(256) void p2s_smooth_pairs_kernel(EdgeTable t, const unsigned char *__restrict__ cls,
                                                               unsigned long long *__restrict__ pairs, unsigned long long *__restrict__ ctr2) {
    __shared__ unsigned long long room;
    __shared__ int wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long per = ((unsigned long long)t.mask + 1) / gridDim.x, lo = blockIdx.x * per, hi = lo + per;
    unsigned long long k0 = 0, k1 = 0;
    int mine = 0;
    for (unsigned long long i = lo + tid; i < hi; i += 256) mine += smooth_slot_pairs(t, cls, i, &k0, &k1);
    for (int d = 32; d > 0; d >>= 1) mine += __shfl_xor(mine, d);
    if (lane == 0) wsum[wave] = mine;
    __syncthreads();
    if (tid == 0) {
        const int total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        room = total ? atomicAdd(&ctr2[SMOOTH_PAIR_AT], (unsigned long long)total) : 0ull;
    }
    __syncthreads();
    unsigned long long at = room;
    for (unsigned long long c = lo; c < hi; c += 256) {              // the same trips for every thread of the workgroup
        const int n = smooth_slot_pairs(t, cls, c + tid, &k0, &k1);
        int incl = n;                                                // the inclusive scan of n over the wave
        for (int d = 1; d < 64; d <<= 1) {
            const int u = __shfl_up(incl, d);
            if (lane >= d) incl += u;
        }
        __syncthreads();                                             // wsum: the reads of the trip before are done
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        unsigned long long mine_at = at + (unsigned long long)(incl - n);
        for (int w = 0; w < 4; ++w) {
            if (w < wave) mine_at += (unsigned long long)wsum[w];
            at += (unsigned long long)wsum[w];
        }
        if (n > 0) pairs[mine_at] = k0;
        if (n > 1) pairs[mine_at + 1] = k1;
    }
}
__global__ __launch_bounds__(256) void p2s_smooth_col_kernel(const unsigned long long *__restrict__ sorted, long long n, int *__restrict__ col) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k < n) col[k] = (int)(sorted[k] & 0xffffffffu);
}
template <int S>
__global__ __launch_bounds__(256) void p2s_smooth_pack_kernel(const float *__restrict__ verts, long long V, float *__restrict__ a,
                                                              float *__restrict__ b) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    for (int k = 0; k < S; ++k) {
        const float x = k < 3 ? verts[3 * v + k] : 0.0f;
        a[S * v + k] = x;
        b[S * v + k] = x;
    }
}

template <int S> __device__ __forceinline__ void smooth_move(const float *__restrict__ pin, float *__restrict__ pout, long long i, const double *s,
                                                             int d, double w) {
    double p[3];
    smooth_load<S>(pin, i, p);
    for (int k = 0; k < 3; ++k) {
        const double m = s[k] / (double)d;
        pout[S * i + k] = (float)(p[k] + w * (m - p[k]));
    }
}
template <int S>
__global__ __launch_bounds__(256) void p2s_smooth_step_kernel(long long V, const int *__restrict__ start, const int *__restrict__ col, double w,
                                                              const float *__restrict__ pin, float *__restrict__ pout) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    const int r0 = start[i], r1 = start[i + 1], d = r1 - r0;
    if (d == 0) return;                                              // fixed: both buffers hold its position from the start
    double s[3];
    smooth_load<S>(pin, col[r0], s);                                 // the sum starts AS the first neighbour, not as 0 + it
#pragma unroll 4
    for (int r = r0 + 1; r < r1; ++r) {
        double q[3];
        smooth_load<S>(pin, col[r], q);
        s[0] = s[0] + q[0];
        s[1] = s[1] + q[1];
        s[2] = s[2] + q[2];
    }
    smooth_move<S>(pin, pout, i, s, d, w);
}

template <int S>
__global__ __launch_bounds__(256) void p2s_smooth_measure_kernel(const float *__restrict__ verts, const float *__restrict__ p, long long V,
                                                                 unsigned long long *__restrict__ ctr2) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    unsigned long long bad = 0, bits = 0;
    if (v < V) {
        double q[3], dd[3];
        smooth_load<S>(p, v, q);
        for (int k = 0; k < 3; ++k) {
            bad += !(fabs(q[k]) <= 3.4028234663852886e38);
            dd[k] = q[k] - (double)verts[3 * v + k];
        }
        if (!bad) bits = (unsigned long long)__double_as_longlong((dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2]);
    }
    wave_count(&ctr2[SMOOTH_NONFINITE], bad);
    for (int d = 32; d > 0; d >>= 1) bits = max(bits, __shfl_xor(bits, d));
    if ((threadIdx.x & 63) == 0 && bits) atomicMax(&ctr2[SMOOTH_MAXDISP], bits);
}
template <int S>
__global__ __launch_bounds__(256) void p2s_smooth_unpack_kernel(const float *__restrict__ p, long long V, float *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < 3 * V) out[i] = p[S * (i / 3) + i % 3];
}

struct SmoothWs {                                // what the input's sizes give
    int *ctl;
    unsigned long long *ctr, *ctr2;
    int *vtx;                                    // [3][V] deg, bdeg, nm (zeroed as one)
    int *rowlen, *start;
    unsigned char *cls;
    EdgeTable t;
    void *tmp;
    char *base;
    size_t bytes;
};
SmoothWs carve_smooth(char *base, size_t V, unsigned ecap, size_t tmp_bytes) {
    Carver c{base};
    SmoothWs w;
    w.ctl = c.take<int>(16);
    w.ctr = c.take<unsigned long long>(8);
    w.ctr2 = c.take<unsigned long long>(8);
    w.vtx = c.take<int>(V * 3);
    w.rowlen = c.take<int>(V + 1);
    w.start = c.take<int>(V + 1);
    w.cls = c.take<unsigned char>(V);
    w.t = carve_edges(c, ecap);
    w.tmp = c.take<char>(tmp_bytes);
    return c.done(w);
}
struct SmoothRowWs {                             // what the total of the rows (T) gives
    unsigned long long *pairs, *sorted;
    int *col;                                    // lies over pairs, which the sort has read by then
    float *pa, *pb;
    void *tmp;
    char *base;
    size_t bytes;
};
SmoothRowWs carve_smooth_rows(char *base, size_t V, size_t T, size_t tmp_bytes) {
    Carver c{base};
    SmoothRowWs w;
    w.pairs = c.take<unsigned long long>(T);
    w.col = (int *)w.pairs;
    w.sorted = c.take<unsigned long long>(T);
    w.pa = c.take<float>(V * SMOOTH_STRIDE);
    w.pb = c.take<float>(V * SMOOTH_STRIDE);
    w.tmp = c.take<char>(tmp_bytes);
    return c.done(w);
}

}  // namespace

extern "C" int p2s_mesh_smooth(const float *verts_dev, int64_t n_verts, const int32_t *faces_dev, int64_t n_faces, int iterations, double lambda,
                               double mu, int boundary_mode, const uint8_t *fixed_dev, float *verts_out_dev, uint8_t *class_out_dev,
                               int64_t *report_host, int device, void *stream) {
    static const char *const who = "p2s_mesh_smooth";
    const char *bad = mc_bad_mesh(verts_dev, n_verts, faces_dev, n_faces, report_host);
    if (!bad) {
        const uintptr_t in = (uintptr_t)verts_dev, out = (uintptr_t)verts_out_dev, span = (uintptr_t)n_verts * 12;
        if (iterations < 0 || iterations > 10000) bad = "iterations outside 0 .. 10000";
        else if (!(lambda > 0.0 && lambda <= 1.0)) bad = "lambda outside 0 < lambda <= 1";      // NaN fails both
        else if (!(mu >= -2.0 && mu <= 0.0)) bad = "mu outside -2 .. 0";
        else if (boundary_mode < 0 || boundary_mode > 2) bad = "boundary_mode outside 0 .. 2";
        else if (n_verts > 0 && !verts_out_dev) bad = "verts_out_dev is NULL";
        else if (n_verts > 0 && in < out + span && out < in + span) bad = "verts_out_dev overlaps verts_dev: the update is not in place";
    }
    if (bad) {
        p2s_set_error("%s: bad argument (%s)", who, bad);
        return P2S_EINVAL;
    }
    if (int rc = select_device(who, device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const long long V = n_verts, F = n_faces;
    const int per_iteration = mu != 0.0 ? 2 : 1;
    PoolScratch pool(device, s);
    int rc;

    // ---- a. validate; the edge table; classes and row lengths
    const unsigned ecap = rp_table_cap(3 * F);
    size_t t1 = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, t1, (int *)nullptr, (int *)nullptr, (int)(V + 1), nullptr);
    const SmoothWs W = pool.carve([&](char *b) { return carve_smooth(b, (size_t)V, ecap, t1 + 256); });
    if (!W.base) return dev_oom(who, s);
    if (V > 0 || F > 0) {
        if ((rc = mc_validate(who, verts_dev, V, faces_dev, F, W.ctl, s)) != P2S_OK) return rc;
    }
    int repeated = 0;
    DEV_CHECK(who, hipMemsetAsync(W.ctl, 0, 4, s));
    hipLaunchKernelGGL(p2s_mf_repeat_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, faces_dev, F, W.ctl);
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipMemcpyAsync(&repeated, W.ctl, 4, hipMemcpyDeviceToHost, s));
    DEV_CHECK(who, hipStreamSynchronize(s));
    if (repeated) {
        p2s_set_error("%s: a face with a repeated index", who);
        return P2S_EINVAL;
    }
    unsigned long long hc[8] = {}, hc2[8] = {};
    int *deg = W.vtx, *bdeg = deg + V, *nm = bdeg + V;
    DEV_CHECK(who, hipMemsetAsync(W.ctr, 0, MESH_COUNTERS, s));
    DEV_CHECK(who, hipMemsetAsync(W.ctr2, 0, MESH_COUNTERS, s));
    if (V > 0) DEV_CHECK(who, hipMemsetAsync(W.vtx, 0, (size_t)V * 3 * 4, s));
    DEV_CHECK(who, hipMemsetAsync(W.rowlen + V, 0, 4, s));
    if ((rc = build_edges(who, faces_dev, F, W.t, nullptr, nullptr, s)) != P2S_OK) return rc;
    hipLaunchKernelGGL(p2s_smooth_degree_kernel, dim3(std::min(blocks((long long)ecap, 256), 4096u)), dim3(256), 0, s, W.t, deg, bdeg, nm, W.ctr);
    hipLaunchKernelGGL(p2s_smooth_class_kernel, dim3(std::min(blocks(V, 256), 256u)), dim3(256), 0, s, V, boundary_mode,
                       (const unsigned char *)fixed_dev, deg, bdeg, nm, W.cls, W.rowlen, W.ctr);
    DEV_CHECK(who, hipGetLastError());
    {
        size_t tb = t1 + 256;
        DEV_CHECK(who, hipcub::DeviceScan::ExclusiveSum(W.tmp, tb, W.rowlen, W.start, (int)(V + 1), s));
    }
    int total = 0;
    DEV_CHECK(who, hipMemcpyAsync(&total, W.start + V, 4, hipMemcpyDeviceToHost, s));
    if ((rc = read_counters(who, W.ctr, hc, -1, nullptr, s)) != P2S_OK) return rc;
    const long long T = total;
    const long long steps = T > 0 ? (long long)iterations * per_iteration : 0;
    long long rep_out[16] = {};
    rep_out[0] = V | (F << 32);
    for (int k = 0; k < 6; ++k) rep_out[1 + k] = (long long)hc[SMOOTH_CLASS0 + k];
    rep_out[7] = (long long)hc[SMOOTH_EDGES];
    rep_out[8] = (long long)hc[SMOOTH_MAXDEG];
    rep_out[9] = steps;

    // ---- b. the rows; c. the half-steps; d. the measures of the result
    const float *result = nullptr;                                   // NULL: the input's bytes
    SmoothRowWs R = {};
    if (steps > 0) {
        size_t t2 = 0;
        (void)hipcub::DeviceRadixSort::SortKeys(nullptr, t2, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (int)T, 0, 64, nullptr);
        R = pool.carve([&](char *b) { return carve_smooth_rows(b, (size_t)V, (size_t)T, t2 + 256); });
        if (!R.base) return dev_oom(who, s);
        hipLaunchKernelGGL(p2s_smooth_pairs_kernel, dim3(std::min(ecap / 256, 1024u)), dim3(256), 0, s, W.t, W.cls, R.pairs, W.ctr2);
        DEV_CHECK(who, hipGetLastError());
        int end_bit = 33;
        while (end_bit < 64 && (V >> (end_bit - 32)) != 0) ++end_bit;
        size_t tb = t2 + 256;
        DEV_CHECK(who, hipcub::DeviceRadixSort::SortKeys(R.tmp, tb, R.pairs, R.sorted, (int)T, 0, end_bit, s));
        hipLaunchKernelGGL(p2s_smooth_col_kernel, dim3(blocks(T, 256)), dim3(256), 0, s, R.sorted, T, R.col);
        hipLaunchKernelGGL(p2s_smooth_pack_kernel<SMOOTH_STRIDE>, dim3(blocks(V, 256)), dim3(256), 0, s, verts_dev, V, R.pa, R.pb);
        float *pin = R.pa, *pout = R.pb;
        for (long long h = 0; h < steps; ++h) {
            const double w = (per_iteration == 2 && (h & 1)) ? mu : lambda;
            hipLaunchKernelGGL(p2s_smooth_step_kernel<SMOOTH_STRIDE>, dim3(blocks(V, 256)), dim3(256), 0, s, V, W.start, R.col, w, pin, pout);
            std::swap(pin, pout);
        }
        hipLaunchKernelGGL(p2s_smooth_measure_kernel<SMOOTH_STRIDE>, dim3(blocks(V, 256)), dim3(256), 0, s, verts_dev, pin, V, W.ctr2);
        if ((rc = read_counters(who, W.ctr2, hc2, -1, nullptr, s)) != P2S_OK) return rc;
        if ((long long)hc2[SMOOTH_PAIR_AT] != T) {
            p2s_set_error("%s: internal error (the rows hold %llu entries, the classes promised %lld)", who, hc2[SMOOTH_PAIR_AT], T);
            return P2S_EHIP;
        }
        rep_out[10] = (long long)hc2[SMOOTH_MAXDISP];
        rep_out[11] = (long long)hc2[SMOOTH_NONFINITE];
        result = pin;
    }
    for (int k = 0; k < 16; ++k) report_host[k] = rep_out[k];
    if (rep_out[11] > 0) {
        p2s_set_error("%s: the result is not finite (%lld coordinates)", who, rep_out[11]);
        return P2S_EINVAL;
    }
    if (result) hipLaunchKernelGGL(p2s_smooth_unpack_kernel<SMOOTH_STRIDE>, dim3(blocks(3 * V, 256)), dim3(256), 0, s, result, V, verts_out_dev);
    else if (V > 0) DEV_CHECK(who, hipMemcpyAsync(verts_out_dev, verts_dev, (size_t)V * 12, hipMemcpyDeviceToDevice, s));
    DEV_CHECK(who, hipGetLastError());
    if (class_out_dev && V > 0) DEV_CHECK(who, hipMemcpyAsync(class_out_dev, W.cls, (size_t)V, hipMemcpyDeviceToDevice, s));
    DEV_CHECK(who, hipStreamSynchronize(s));
    return P2S_OK;
}
