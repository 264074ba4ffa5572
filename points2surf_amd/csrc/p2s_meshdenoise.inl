// a triangle mesh denoised with its sharp edges kept -- the face normals filtered with the weight
// max(0, ni . nj - T)^2 over the faces that share a vertex, then the vertices moved toward the filtered normals (Sun, Rosin,
// Martin and Langbein 2007).  Definition: include/p2s_hip.h (p2s_mesh_denoise).  Included at the end of p2s_meshdist.hip, behind
// p2s_meshsmooth.inl: the edge table (EdgeTable, build_edges, rp_table_cap), p2s_mf_repeat_kernel, mc_validate, mc_bad_mesh,
// wave_count, read_counters, the host scaffold, and of the smooth unit p2s_smooth_degree_kernel (the vertices on an edge of one
// face), p2s_smooth_pack_kernel, p2s_smooth_measure_kernel and p2s_smooth_unpack_kernel with their counter slots are those
// files', used here and not copied.
//   p2s_denoise_normals_kernel   per face: the geometric normal of rule b into both ping-pong buffers, the pairs (v, f) of its
//                                corners at 3 f + corner (no atomic for the place), the faces per vertex (integer atomicAdd),
//                                the dead faces counted.  The pairs are written in ascending f and the radix sort that follows
//                                sorts them by v alone and is STABLE, so it gives the vertex -> face rows, each ascending in f
//                                (strictly: a repeated index is refused), whatever the arrival.  Sorting the distinct 64-bit
//                                keys v << 32 | f instead, as the smooth unit sorts its pairs, gave the same rows by sorting
//                                32 + log2(V) bits of 8-byte keys in place of log2(V) bits (the times: DESIGN 4.8 f18)
//   p2s_denoise_class_kernel     per vertex: the class of rule e (its row is searched for a live face), the counts of the report
//   p2s_denoise_count_kernel     per live face: |N(i)| by the three-way merge below with no normal read; the largest one
//   p2s_denoise_filter_kernel    HOT PATH 1, one launch per normal iteration, one face per thread.  N(i) in ascending order is
//                                the three-way merge of the rows of the face's three vertices, equal heads taken once: no
//                                face -> face table exists.  The merge runs four neighbours ahead of the sum: the indices of a
//                                batch are found first, its four normals (12-byte records) are then loaded together, and the
//                                sequential float64 sum of rule d follows.  A dead neighbour has the normal 0, so d = 0 <= T:
//                                it adds nothing without a test of its own.  Reads one buffer, writes the other.  No atomic.
//                                Measured once on the 256^3 stand-in mesh (850,336 faces, 12.98 neighbours on average): 32.6 us
//                                per launch, which asks for 245 MB (132 MB of neighbour normals, 61 MB of column indices), 44 MB
//                                of them compulsory.  A face -> face CSR was to be built only if this cost more than about
//                                twice the vertex step; it costs less, so the CSR is unbuilt and unmeasured.
//   p2s_denoise_vertex_kernel    HOT PATH 2, one launch per vertex iteration, one vertex of class 0 per thread: its row, and
//                                per live face of it the three corner indices, their positions and the target normal.  Reads one
//                                position buffer, writes the other.  No atomic.  Measured in the same run (427,475 vertices):
//                                41.0 us per launch, which asks for 177 MB (92 MB of corner positions), 45 MB compulsory.
// Both ask for more than HBM delivers in that time and need far less: gathers out of the L2 and the Infinity Cache, bound by
// cache bandwidth and the latency of the dependent index loads -- reasoned from the bytes, no counter run.
// 12-byte records as in the smooth unit, which measured a 16-byte pad as slower; the pad was not tried here.
// Determinism: counts are integer sums, the rows come out of a sort of distinct keys, every output value is computed by one
// lane in one order with contraction off.  No thread spins on another.  Bounds: a row lies in [start[v], start[v + 1]) of a scan
// of the faces per vertex, whose total is 3 F, the number of keys; a column is a face id below F; a corner of a validated face
// is below n_verts.  A fan of d faces at one vertex costs d visits per face, O(d^2) per launch of the filter (9 M at d = 3,000).

namespace {

enum DenoiseCtr { DENOISE_CLASS0 = 0, DENOISE_DEAD = 5, DENOISE_EDGES = SMOOTH_EDGES, DENOISE_MAXNB = 7 };       // ctr
static_assert(DENOISE_EDGES == 6, "p2s_smooth_degree_kernel counts the edges into the one slot that this unit leaves unused");
constexpr int DENOISE_AHEAD = 4;                 // neighbours whose normals are in flight while the sum waits

__device__ __forceinline__ bool denoise_dead(const float *__restrict__ n, long long f) {
    return n[3 * f] == 0.0f && n[3 * f + 1] == 0.0f && n[3 * f + 2] == 0.0f;
}

__global__ __launch_bounds__(256) void p2s_denoise_normals_kernel(const float *__restrict__ verts, const int *__restrict__ faces, long long F,
                                                                  float *__restrict__ na, float *__restrict__ nb,
                                                                  unsigned *__restrict__ vkey, int *__restrict__ fval, int *__restrict__ vdeg,
                                                                  unsigned long long *__restrict__ ctr) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    unsigned long long dead = 0;
    if (f < F) {
        const int v[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
        double e1[3], e2[3], m[3];
        for (int k = 0; k < 3; ++k) {
            const double a = verts[3 * (long long)v[0] + k];
            e1[k] = (double)verts[3 * (long long)v[1] + k] - a;
            e2[k] = (double)verts[3 * (long long)v[2] + k] - a;
        }
        cross3(e1, e2, m);
        const double l = sqrt(dot3(m, m));
        const bool live = l > 0.0 && l <= 1.7976931348623157e308;                    // false for 0, inf and NaN
        for (int k = 0; k < 3; ++k) {
            const float x = live ? (float)(m[k] / l) : 0.0f;
            na[3 * f + k] = x;
            nb[3 * f + k] = x;
            vkey[3 * f + k] = (unsigned)v[k];
            fval[3 * f + k] = (int)f;
            atomicAdd(&vdeg[v[k]], 1);
        }
        dead = !live;
    }
    wave_count(&ctr[DENOISE_DEAD], dead);
}
// vdeg [V + 1]: the last entry stays 0.  Any grid: a thread keeps its counts over its vertices, a wave adds them up once
__global__ __launch_bounds__(256) void p2s_denoise_class_kernel(long long V, int mode, const unsigned char *__restrict__ fixed,
                                                                const int *__restrict__ start, const int *__restrict__ col,
                                                                const float *__restrict__ n, const int *__restrict__ bdeg,
                                                                unsigned char *__restrict__ cls, unsigned long long *__restrict__ ctr) {
    unsigned long long count[5] = {0, 0, 0, 0, 0};
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < V; v += (long long)gridDim.x * 256) {
        const int r0 = start[v], r1 = start[v + 1];
        int c;
        if (fixed && fixed[v]) c = 2;
        else if (r0 == r1) c = 3;
        else {
            bool live = false;
            for (int r = r0; r < r1 && !live; ++r) live = !denoise_dead(n, col[r]);
            c = !live ? 4 : ((mode == 0 && bdeg[v] > 0) ? 1 : 0);
        }
        cls[v] = (unsigned char)c;
        for (int k = 0; k < 5; ++k) count[k] += c == k;
    }
    for (int k = 0; k < 5; ++k) wave_count(&ctr[DENOISE_CLASS0 + k], count[k]);
}

// The three-way merge of the rows of a face's corners: next() is the smallest head, every row that shows it moves on.
struct DenoiseMerge {
    const int *__restrict__ col;
    int at[3], end[3], head[3];
    __device__ __forceinline__ DenoiseMerge(const int *__restrict__ faces, long long f, const int *__restrict__ start,
                                            const int *__restrict__ col_) : col(col_) {
        for (int k = 0; k < 3; ++k) {
            const int v = faces[3 * f + k];
            at[k] = start[v];
            end[k] = start[v + 1];
            head[k] = at[k] < end[k] ? col[at[k]] : 0x7fffffff;
        }
    }
    __device__ __forceinline__ int next() {                           // 0x7fffffff: the rows are used up
        const int j = min(head[0], min(head[1], head[2]));
        if (j != 0x7fffffff) {
            for (int k = 0; k < 3; ++k) {
                if (head[k] == j) {
                    ++at[k];
                    head[k] = at[k] < end[k] ? col[at[k]] : 0x7fffffff;
                }
            }
        }
        return j;
    }
};

__global__ __launch_bounds__(256) void p2s_denoise_count_kernel(const int *__restrict__ faces, long long F, const int *__restrict__ start,
                                                                const int *__restrict__ col, const float *__restrict__ n,
                                                                unsigned long long *__restrict__ ctr) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    int count = 0;
    if (f < F && !denoise_dead(n, f)) {
        DenoiseMerge m(faces, f, start, col);
        while (m.next() != 0x7fffffff) ++count;
    }
    for (int d = 32; d > 0; d >>= 1) count = max(count, __shfl_xor(count, d));
    if ((threadIdx.x & 63) == 0 && count) atomicMax(&ctr[DENOISE_MAXNB], (unsigned long long)count);
}

__global__ __launch_bounds__(256) void p2s_denoise_filter_kernel(const int *__restrict__ faces, long long F, const int *__restrict__ start,
                                                                 const int *__restrict__ col, double T, const float *__restrict__ nin,
                                                                 float *__restrict__ nout) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const double ni[3] = {nin[3 * f], nin[3 * f + 1], nin[3 * f + 2]};
    if (ni[0] == 0.0 && ni[1] == 0.0 && ni[2] == 0.0) return;        // dead: both buffers hold its zero from the start
    DenoiseMerge m(faces, f, start, col);
    double s[3] = {0.0, 0.0, 0.0};
    for (bool more = true; more;) {
        int j[DENOISE_AHEAD];
        float q[DENOISE_AHEAD][3];
#pragma unroll
        for (int b = 0; b < DENOISE_AHEAD; ++b) {
            j[b] = more ? m.next() : 0x7fffffff;
            more = j[b] != 0x7fffffff;
        }
#pragma unroll
        for (int b = 0; b < DENOISE_AHEAD; ++b) {
            const long long at = j[b] != 0x7fffffff ? j[b] : f;       // a slot past the end reads the face's own record: in bounds
            q[b][0] = nin[3 * at];
            q[b][1] = nin[3 * at + 1];
            q[b][2] = nin[3 * at + 2];
        }
#pragma unroll
        for (int b = 0; b < DENOISE_AHEAD; ++b) {
            if (j[b] == 0x7fffffff) continue;
            const double nj[3] = {q[b][0], q[b][1], q[b][2]};
            const double d = dot3(ni, nj);
            if (d > T) {
                const double w = (d - T) * (d - T);
                s[0] = s[0] + w * nj[0];
                s[1] = s[1] + w * nj[1];
                s[2] = s[2] + w * nj[2];
            }
        }
    }
    const double l = sqrt(dot3(s, s));
    const bool ok = l > 0.0 && l <= 1.7976931348623157e308;
    for (int k = 0; k < 3; ++k) nout[3 * f + k] = ok ? (float)(s[k] / l) : (float)ni[k];
}

__global__ __launch_bounds__(256) void p2s_denoise_vertex_kernel(long long V, const unsigned char *__restrict__ cls, const int *__restrict__ start,
                                                                 const int *__restrict__ col, const int *__restrict__ faces,
                                                                 const float *__restrict__ n, const float *__restrict__ pin,
                                                                 float *__restrict__ pout) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= V || cls[v] != 0) return;                               // fixed: both buffers hold its position from the start
    const double p[3] = {pin[3 * v], pin[3 * v + 1], pin[3 * v + 2]};
    double s[3] = {0.0, 0.0, 0.0};
    int k = 0;
    const int r1 = start[v + 1];
#pragma unroll 2
    for (int r = start[v]; r < r1; ++r) {
        const long long f = col[r];
        const double nf[3] = {n[3 * f], n[3 * f + 1], n[3 * f + 2]};
        if (nf[0] == 0.0 && nf[1] == 0.0 && nf[2] == 0.0) continue;  // dead
        const long long a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
        double g[3];
        for (int x = 0; x < 3; ++x) g[x] = (((double)pin[3 * a + x] + (double)pin[3 * b + x]) + (double)pin[3 * c + x]) / 3.0 - p[x];
        const double d = dot3(nf, g);
        s[0] = s[0] + nf[0] * d;
        s[1] = s[1] + nf[1] * d;
        s[2] = s[2] + nf[2] * d;
        ++k;
    }
    for (int x = 0; x < 3; ++x) pout[3 * v + x] = (float)(p[x] + s[x] / (double)k);       // class 0: k > 0
}

struct DenoiseWs {
    int *ctl;
    unsigned long long *ctr, *ctr2;
    int *vtx;                                    // [3][V] deg, bdeg, nm of p2s_smooth_degree_kernel (mode 0 only; zeroed as one)
    int *vdeg, *start;                           // [V + 1]
    unsigned char *cls;
    unsigned *vkey, *vsorted;                    // [3 F] the vertex of every corner, as written and sorted
    int *fval, *col;                             // [3 F] the face of every corner, as written and sorted: the rows
    float *na, *nb;                              // [F][3]
    float *pa, *pb;                              // [V][3]
    EdgeTable t;
    void *tmp;
    char *base;
    size_t bytes;
};
DenoiseWs carve_denoise(char *base, size_t V, size_t F, unsigned ecap, bool moves, size_t tmp_bytes) {
    Carver c{base};
    DenoiseWs w;
    w.ctl = c.take<int>(16);
    w.ctr = c.take<unsigned long long>(8);
    w.ctr2 = c.take<unsigned long long>(8);
    w.vtx = c.take<int>(V * 3, ecap != 0);
    w.vdeg = c.take<int>(V + 1);
    w.start = c.take<int>(V + 1);
    w.cls = c.take<unsigned char>(V);
    w.vkey = c.take<unsigned>(F * 3);
    w.vsorted = c.take<unsigned>(F * 3);
    w.fval = c.take<int>(F * 3);
    w.col = c.take<int>(F * 3);
    w.na = c.take<float>(F * 3);
    w.nb = c.take<float>(F * 3);
    w.pa = c.take<float>(V * 3, moves);
    w.pb = c.take<float>(V * 3, moves);
    w.t = ecap ? carve_edges(c, ecap) : EdgeTable{};
    w.tmp = c.take<char>(tmp_bytes);
    return c.done(w);
}

}  // namespace

extern "C" int p2s_mesh_denoise(const float *verts_dev, int64_t n_verts, const int32_t *faces_dev, int64_t n_faces, double threshold,
                                int normal_iterations, int vertex_iterations, int boundary_mode, const uint8_t *fixed_dev, float *verts_out_dev,
                                float *normals_out_dev, uint8_t *class_out_dev, int64_t *report_host, int device, void *stream) {
    static const char *const who = "p2s_mesh_denoise";
    const char *bad = mc_bad_mesh(verts_dev, n_verts, faces_dev, n_faces, report_host);
    if (!bad) {
        const uintptr_t in = (uintptr_t)verts_dev, out = (uintptr_t)verts_out_dev, span = (uintptr_t)n_verts * 12;
        if (!(threshold >= 0.0 && threshold < 1.0)) bad = "threshold outside 0 <= threshold < 1";                // NaN fails both
        else if (normal_iterations < 0 || normal_iterations > 10000) bad = "normal_iterations outside 0 .. 10000";
        else if (vertex_iterations < 0 || vertex_iterations > 10000) bad = "vertex_iterations outside 0 .. 10000";
        else if (boundary_mode < 0 || boundary_mode > 1) bad = "boundary_mode outside 0 .. 1";
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
    PoolScratch pool(device, s);
    int rc;

    // ---- a. validate; normals, keys, rows; the edge table (mode 0); classes
    const bool table = boundary_mode == 0 && F > 0;
    const unsigned ecap = table ? rp_table_cap(3 * F) : 0;
    size_t t1 = 0, t2 = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, t1, (int *)nullptr, (int *)nullptr, (int)(V + 1), nullptr);
    if (F > 0)
        (void)hipcub::DeviceRadixSort::SortPairs(nullptr, t2, (unsigned *)nullptr, (unsigned *)nullptr, (int *)nullptr, (int *)nullptr, (int)(3 * F),
                                                 0, 32, nullptr);
    const DenoiseWs W = pool.carve([&](char *b) { return carve_denoise(b, (size_t)V, (size_t)F, ecap, vertex_iterations > 0, std::max(t1, t2) + 256); });
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
    DEV_CHECK(who, hipMemsetAsync(W.ctr, 0, MESH_COUNTERS, s));
    DEV_CHECK(who, hipMemsetAsync(W.ctr2, 0, MESH_COUNTERS, s));
    DEV_CHECK(who, hipMemsetAsync(W.vdeg, 0, (size_t)(V + 1) * 4, s));
    int *bdeg = nullptr;
    if (table) {
        int *deg = W.vtx, *nm = deg + 2 * V;
        bdeg = deg + V;
        DEV_CHECK(who, hipMemsetAsync(W.vtx, 0, (size_t)V * 3 * 4, s));
        if ((rc = build_edges(who, faces_dev, F, W.t, nullptr, nullptr, s)) != P2S_OK) return rc;
        hipLaunchKernelGGL(p2s_smooth_degree_kernel, dim3(std::min(blocks((long long)ecap, 256), 4096u)), dim3(256), 0, s, W.t, deg, bdeg, nm, W.ctr);
    }
    if (F > 0) {
        hipLaunchKernelGGL(p2s_denoise_normals_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, verts_dev, faces_dev, F, W.na, W.nb, W.vkey, W.fval,
                           W.vdeg, W.ctr);
        DEV_CHECK(who, hipGetLastError());
        int end_bit = 1;
        while (end_bit < 32 && (V >> end_bit) != 0) ++end_bit;
        size_t tb = t2 + 256;
        DEV_CHECK(who, hipcub::DeviceRadixSort::SortPairs(W.tmp, tb, W.vkey, W.vsorted, W.fval, W.col, (int)(3 * F), 0, end_bit, s));
    }
    {
        size_t tb = t1 + 256;
        DEV_CHECK(who, hipcub::DeviceScan::ExclusiveSum(W.tmp, tb, W.vdeg, W.start, (int)(V + 1), s));
    }
    hipLaunchKernelGGL(p2s_denoise_class_kernel, dim3(std::min(blocks(V, 256), 256u)), dim3(256), 0, s, V, boundary_mode,
                       (const unsigned char *)fixed_dev, W.start, W.col, W.na, bdeg, W.cls, W.ctr);
    if (F > 0) hipLaunchKernelGGL(p2s_denoise_count_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, faces_dev, F, W.start, W.col, W.na, W.ctr);
    if ((rc = read_counters(who, W.ctr, hc, -1, nullptr, s)) != P2S_OK) return rc;
    const long long live = F - (long long)hc[DENOISE_DEAD];
    const long long n_it = live > 0 ? normal_iterations : 0, v_it = hc[DENOISE_CLASS0] > 0 ? vertex_iterations : 0;
    long long rep_out[16] = {};
    rep_out[0] = V | (F << 32);
    for (int k = 0; k < 5; ++k) rep_out[1 + k] = (long long)hc[DENOISE_CLASS0 + k];
    rep_out[6] = (long long)hc[DENOISE_DEAD];
    rep_out[7] = (long long)hc[DENOISE_MAXNB];
    rep_out[8] = n_it;
    rep_out[9] = v_it;

    // ---- b. the normal iterations; c. the vertex iterations; d. the measures of the result
    float *nin = W.na, *nout = W.nb;
    for (long long h = 0; h < n_it; ++h) {
        hipLaunchKernelGGL(p2s_denoise_filter_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, faces_dev, F, W.start, W.col, threshold, nin, nout);
        std::swap(nin, nout);
    }
    const float *result = nullptr;                                   // NULL: the input's bytes
    if (v_it > 0) {
        hipLaunchKernelGGL(p2s_smooth_pack_kernel<3>, dim3(blocks(V, 256)), dim3(256), 0, s, verts_dev, V, W.pa, W.pb);
        float *pin = W.pa, *pout = W.pb;
        for (long long h = 0; h < v_it; ++h) {
            hipLaunchKernelGGL(p2s_denoise_vertex_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, V, W.cls, W.start, W.col, faces_dev, nin, pin, pout);
            std::swap(pin, pout);
        }
        hipLaunchKernelGGL(p2s_smooth_measure_kernel<3>, dim3(blocks(V, 256)), dim3(256), 0, s, verts_dev, pin, V, W.ctr2);
        if ((rc = read_counters(who, W.ctr2, hc2, -1, nullptr, s)) != P2S_OK) return rc;
        rep_out[10] = (long long)hc2[SMOOTH_MAXDISP];
        rep_out[11] = (long long)hc2[SMOOTH_NONFINITE];
        result = pin;
    }
    for (int k = 0; k < 16; ++k) report_host[k] = rep_out[k];
    if (rep_out[11] > 0) {
        p2s_set_error("%s: the result is not finite (%lld coordinates)", who, rep_out[11]);
        return P2S_EINVAL;
    }
    if (result) hipLaunchKernelGGL(p2s_smooth_unpack_kernel<3>, dim3(blocks(3 * V, 256)), dim3(256), 0, s, result, V, verts_out_dev);
    else if (V > 0) DEV_CHECK(who, hipMemcpyAsync(verts_out_dev, verts_dev, (size_t)V * 12, hipMemcpyDeviceToDevice, s));
    DEV_CHECK(who, hipGetLastError());
    if (normals_out_dev && F > 0) DEV_CHECK(who, hipMemcpyAsync(normals_out_dev, nin, (size_t)F * 12, hipMemcpyDeviceToDevice, s));
    if (class_out_dev && V > 0) DEV_CHECK(who, hipMemcpyAsync(class_out_dev, W.cls, (size_t)V, hipMemcpyDeviceToDevice, s));
    DEV_CHECK(who, hipStreamSynchronize(s));
    return P2S_OK;
}
