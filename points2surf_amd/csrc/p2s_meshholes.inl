// the holes of a triangle mesh closed by the minimum-area triangulation of their boundary loops (Barequet &
// Sharir 1995; the first stage of Liepa 2003).  Definition: include/p2s_hip.h (p2s_mesh_fill_holes); the project's own, not
// vcglib's ear cutting.  Included at the end of p2s_meshdist.hip, behind p2s_meshmanifold.inl: the edge table (EdgeTable,
// build_edges, edge_key, edge_hash, p2s_rp_edge_stats_kernel), the boundary kernels of the repair (p2s_rp_boundary_kernel,
// p2s_rp_bhook_kernel, p2s_rp_bmark_kernel, p2s_rp_bcount_kernel), p2s_mf_repeat_kernel, mc_validate, mc_bad_mesh, uf_find,
// p2s_uf_compress_kernel, p2s_iota_kernel, cross3, read_counters and the host scaffold are those files', used here and not copied.
//   p2s_hf_init_kernel        per vertex: simple (one outgoing and one incoming boundary edge) -> its successor, else dead
//   p2s_hf_jump_kernel        one round of pointer jumping: the successor 2^r steps on and the smallest vertex on the way; a
//                             vertex whose way meets a dead one is dead.  Reads one pair of arrays, writes the other
//   p2s_hf_count_kernel       the vertices of every loop, counted at its smallest vertex (integer atomicAdd)
//   p2s_hf_flags_kernel       per vertex: the head of a loop / of a candidate loop (n <= max_hole_edges)
//   p2s_hf_loops_kernel       the per-hole table in ascending v0, and per candidate its head, length and table size
//   p2s_hf_walk_kernel        the vertices of every candidate loop, in loop order from v0
//   p2s_hf_dp_kernel<NT, NMAX>  THE HOT PATH.  One workgroup of NT threads per candidate loop of nlo < n <= NMAX edges:
//                             <64, 32> is one wave per small loop, <256, 128> four waves per large one.  In LDS: the loop's
//                             positions in float64 (three arrays: 8-byte accesses of consecutive lanes fall on consecutive
//                             banks), the forbidden-chord bits (one edge-table lookup per chord, integer atomicOr), and the
//                             triangular table W, stored diagonal by diagonal so that the lanes of consecutive cells read
//                             consecutive doubles.  <256, 128>: 65,024 + 3,072 + 512 + 1,016 = 69,624 bytes, two workgroups
//                             (8 waves) per compute unit of 160 KiB; <64, 32>: 3,968 + 768 + 128 + 64 = 4,928 bytes, where the
//                             wave slots bound the occupancy, not the LDS.  The split indices go straight to global memory (the
//                             DP never reads them back), which is what lets two large workgroups share a compute unit.
//                             Diagonal d = 2 .. n - 1 with a barrier behind each; the n - d cells of a diagonal get G lanes
//                             each (G the largest power of two with G (n - d) <= NT, at most 64, all in one wave), lane g
//                             takes k = i + 1 + g, + G, ..., and the G partial minima meet in a butterfly of (value, k) pairs
//                             ordered by value, then by k: the smallest k among the minima, however the cells are spread.
//   p2s_hf_emit_kernel        per filled candidate: the split tree in pre-order with an explicit stack; faces at the scanned
//                             offsets; the hole's row of the table
//   p2s_hf_src_kernel         face_src: the input id, or -1
// The guarantee (rule f).  A chord (i, j) is used only when {v_i, v_j} is no edge of the input, so it is an edge of the
// triangulation alone, where it has exactly two faces (every inner edge of a triangulated polygon has).  The vertex sets of
// two loops are disjoint (a loop vertex has one outgoing boundary edge), so no two holes share a chord, and a chord is never
// an edge of a face added to another hole.  A loop edge had one face and gains exactly one: the triangle on it.  So no edge
// gains a third face, and [11] is the input's count.  At a loop vertex v the added faces are the triangles of the polygon's
// triangulation at v: a chain from the triangle on the outgoing boundary edge to the one on the incoming boundary edge, linked
// by chords of two faces.  If the faces at v formed one fan, that fan ended in exactly these two boundary edges, and the chain
// closes it: still one fan.  Other vertices get no face.  Idempotence: the filled loops have no boundary edge left; a loop that
// was too long is as long as before; a blocked loop has the same vertices, and every chord that was an edge still is, so it
// stays blocked; non-simple vertices stay non-simple, since no boundary edge at them changed.  A second call adds nothing.
// Determinism: the loops, their order and their offsets come from integer minima, integer counts and scans; W is a function of
// the loop's positions and chord bits alone, every candidate value is computed by one lane with contraction off, and the minimum
// with its tie rule is associative and commutative.  No floating-point atomic.  No thread waits for another.
// Termination: pointer jumping runs a number of rounds fixed by the host (2^R > boundary edges); a walk makes n steps; the DP
// loops are counted; the emit stack loses one interval per step and the step count is capped at n - 2.

namespace {

constexpr int HF_MAX_EDGES = 128, HF_SMALL_EDGES = 32;
enum HolesCtr { HF_BOUNDARY = 0, HF_NONMANIFOLD, HF_INCONSISTENT, HF_BGROUPS, HF_FILLED, HF_LONGEST };

// is {a, b} an edge of the table (of any face count)?  Load factor <= 1/2: an empty slot ends the probe
__device__ __forceinline__ bool hf_is_edge(const EdgeTable &t, int a, int b) {
    const unsigned long long key = edge_key(a, b);
    unsigned h = edge_hash(key) & t.mask;
    for (;;) {
        const unsigned long long k = t.key[h];
        if (k == key) return true;
        if (k == EDGE_EMPTY) return false;
        h = (h + 1) & t.mask;
    }
}
// the cell (i, i + d) of a triangular table over n positions, stored diagonal by diagonal from d = 1
__device__ __forceinline__ int hf_cell(int n, int d, int i) { return (d - 1) * n - ((d - 1) * d) / 2 + i; }

__global__ __launch_bounds__(256) void p2s_hf_init_kernel(long long V, const int *__restrict__ outc, const int *__restrict__ inc,
                                                          const int *__restrict__ nxt, int *__restrict__ jmp, int *__restrict__ mn) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    jmp[v] = (outc[v] == 1 && inc[v] == 1) ? nxt[v] : -1;
    mn[v] = (int)v;
}
__global__ __launch_bounds__(256) void p2s_hf_jump_kernel(long long V, const int *__restrict__ jmp, const int *__restrict__ mn,
                                                          int *__restrict__ jmp_out, int *__restrict__ mn_out) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const int j = jmp[v];
    int jo = -1, mo = mn[v];
    if (j >= 0 && jmp[j] >= 0) {
        jo = jmp[j];
        mo = min(mo, mn[j]);
    }
    jmp_out[v] = jo;
    mn_out[v] = mo;
}
__global__ __launch_bounds__(256) void p2s_hf_count_kernel(long long V, const int *__restrict__ jmp, const int *__restrict__ mn, int *cnt) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v < V && jmp[v] >= 0) atomicAdd(&cnt[mn[v]], 1);
}
// hflag, cflag [V + 1]: the last entry stays 0
__global__ __launch_bounds__(256) void p2s_hf_flags_kernel(long long V, int K, const int *__restrict__ jmp, const int *__restrict__ mn,
                                                           const int *__restrict__ cnt, int *__restrict__ hflag, int *__restrict__ cflag) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const int head = jmp[v] >= 0 && mn[v] == (int)v;
    hflag[v] = head;
    cflag[v] = head && cnt[v] <= K;
}
// a candidate starts as blocked (reason 2): p2s_hf_emit_kernel rewrites the rows of the filled ones
__global__ __launch_bounds__(256) void p2s_hf_loops_kernel(long long V, const int *__restrict__ hflag, const int *__restrict__ cflag,
                                                           const int *__restrict__ hstart, const int *__restrict__ cstart,
                                                           const int *__restrict__ cnt, int *__restrict__ htab, double *__restrict__ harea,
                                                           int *__restrict__ cv0, int *__restrict__ cn, long long *__restrict__ ctri,
                                                           int *__restrict__ chole) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= V || !hflag[v]) return;
    const int h = hstart[v], n = cnt[v];
    htab[4 * (long long)h] = (int)v;
    htab[4 * (long long)h + 1] = n;
    htab[4 * (long long)h + 2] = -1;
    htab[4 * (long long)h + 3] = cflag[v] ? 2 : 1;
    harea[h] = 0.0;
    if (cflag[v]) {
        const int c = cstart[v];
        cv0[c] = (int)v;
        cn[c] = n;
        ctri[c] = (long long)n * (n - 1) / 2;
        chole[c] = h;
    }
}
__global__ __launch_bounds__(256) void p2s_hf_walk_kernel(long long C, const int *__restrict__ cv0, const int *__restrict__ cn,
                                                          const int *__restrict__ voff, const int *__restrict__ nxt, int *__restrict__ loopv) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    int x = cv0[c];
    for (int i = 0; i < cn[c]; ++i) {
        loopv[voff[c] + i] = x;
        x = nxt[x];
    }
}

template <int NT, int NMAX>
__global__ __launch_bounds__(NT) void p2s_hf_dp_kernel(const float *__restrict__ verts, EdgeTable t, const int *__restrict__ cn,
                                                       const int *__restrict__ voff, const long long *__restrict__ loff,
                                                       const int *__restrict__ loopv, int nlo, unsigned char *__restrict__ lam,
                                                       double *__restrict__ area, int *__restrict__ fill01) {
    constexpr int CELLS = NMAX * (NMAX - 1) / 2;
    __shared__ double W[CELLS];
    __shared__ double px[NMAX], py[NMAX], pz[NMAX];
    __shared__ int vid[NMAX];
    __shared__ unsigned forb[(CELLS + 31) / 32];
    const int c = blockIdx.x, n = cn[c];
    if (n <= nlo || n > NMAX) return;                                // the other instance's loop (uniform over the workgroup)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int *lv = loopv + voff[c];
    unsigned char *lm = lam + loff[c];
    for (int i = tid; i < n; i += NT) {
        const int v = lv[i];
        vid[i] = v;
        px[i] = verts[3 * (long long)v];
        py[i] = verts[3 * (long long)v + 1];
        pz[i] = verts[3 * (long long)v + 2];
        if (i < n - 1) W[i] = 0.0;                                   // W(i, i + 1)
    }
    for (int i = tid; i < (n * (n - 1) / 2 + 31) / 32; i += NT) forb[i] = 0u;
    __syncthreads();
    for (int p = tid; p < n * n; p += NT) {                          // a chord that is an edge of the mesh already, (0, n - 1) apart
        const int i = p / n, j = p - i * n;
        if (j - i < 2 || (i == 0 && j == n - 1)) continue;
        if (hf_is_edge(t, vid[i], vid[j])) {
            const int at = hf_cell(n, j - i, i);
            atomicOr(&forb[at >> 5], 1u << (at & 31));
        }
    }
    __syncthreads();
    const double inf = __builtin_inf();
    for (int d = 2; d < n; ++d) {
        const int cells = n - d;
        int G = 64;
        while (G * cells > NT) G >>= 1;                              // >= 1: cells < NMAX <= NT
        const int cw = 64 / G, i = wave * cw + lane % cw, g = lane / cw, j = i + d;
        double best = inf;
        int bk = 0x7fffffff;
        if (i < cells) {
            const double ax = px[i], ay = py[i], az = pz[i];
            const double w[3] = {px[j] - ax, py[j] - ay, pz[j] - az};
            for (int k = i + 1 + g; k < j; k += G) {
                const double u[3] = {px[k] - ax, py[k] - ay, pz[k] - az};
                double nn[3];
                cross3(u, w, nn);
                const double a = 0.5 * __dsqrt_rn((nn[0] * nn[0] + nn[1] * nn[1]) + nn[2] * nn[2]);
                const double cand = (W[hf_cell(n, k - i, i)] + W[hf_cell(n, j - k, k)]) + a;
                if (cand < best) {
                    best = cand;
                    bk = k;
                }
            }
        }
        for (int s = cw; s < 64; s <<= 1) {                          // the G lanes of a cell: lane bits log2(cw) and up
            const double ob = __shfl_xor(best, s);
            const int ok = __shfl_xor(bk, s);
            if (ob < best || (ob == best && ok < bk)) {
                best = ob;
                bk = ok;
            }
        }
        if (i < cells && g == 0) {
            const int at = hf_cell(n, d, i);
            if ((forb[at >> 5] >> (at & 31)) & 1u) best = inf;
            W[at] = best;
            lm[at] = (unsigned char)(best < inf ? bk : i + 1);
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double total = W[hf_cell(n, n - 1, 0)];
        area[c] = total;
        fill01[c] = total < inf ? 1 : 0;
    }
}

// addc [C + 1]: the faces a candidate adds (n - 2 if filled); the last entry stays 0
__global__ __launch_bounds__(256) void p2s_hf_addc_kernel(long long C, const int *__restrict__ cn, const int *__restrict__ fill01,
                                                          int *__restrict__ addc) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c < C) addc[c] = fill01[c] ? cn[c] - 2 : 0;
}
__global__ __launch_bounds__(64) void p2s_hf_emit_kernel(long long C, const int *__restrict__ cn, const int *__restrict__ voff,
                                                         const long long *__restrict__ loff, const int *__restrict__ loopv,
                                                         const unsigned char *__restrict__ lam, const int *__restrict__ fill01,
                                                         const int *__restrict__ foff, const double *__restrict__ area,
                                                         const int *__restrict__ chole, long long F, int *__restrict__ wf,
                                                         int *__restrict__ htab, double *__restrict__ harea, unsigned long long *ctr) {
    __shared__ unsigned short stack[HF_MAX_EDGES][64];               // intervals of at least two edges that wait: fewer than n
    const long long c = (long long)blockIdx.x * 64 + threadIdx.x;
    if (c >= C || !fill01[c]) return;
    const int n = cn[c], h = chole[c];
    const int *lv = loopv + voff[c];
    const unsigned char *lm = lam + loff[c];
    const long long base = F + foff[c];
    htab[4 * (long long)h + 2] = (int)base;
    htab[4 * (long long)h + 3] = 0;
    harea[h] = area[c];
    atomicAdd(&ctr[HF_FILLED], 1ull);
    atomicMax(&ctr[HF_LONGEST], (unsigned long long)n);
    unsigned short *st = &stack[0][threadIdx.x];                     // entry e of this lane: st[64 e] = i << 8 | j
    int sp = 1, at = 0;
    st[0] = (unsigned short)(n - 1);
    while (sp > 0 && at < n - 2) {
        --sp;
        const int i = st[64 * sp] >> 8, j = st[64 * sp] & 255, k = lm[hf_cell(n, j - i, i)];
        if (k <= i || k >= j) break;                                 // not a split of (i, j): never, by the DP
        wf[3 * (base + at)] = lv[i];
        wf[3 * (base + at) + 1] = lv[j];
        wf[3 * (base + at) + 2] = lv[k];
        ++at;
        if (j - k >= 2) st[64 * sp++] = (unsigned short)(k << 8 | j);
        if (k - i >= 2) st[64 * sp++] = (unsigned short)(i << 8 | k);      // on top: (i, k) comes before (k, j)
    }
}
__global__ __launch_bounds__(256) void p2s_hf_src_kernel(long long F, long long F1, int *__restrict__ src) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f < F1) src[f] = f < F ? (int)f : -1;
}

struct HfWs {                                    // what the input's sizes give
    int *ctl;
    unsigned long long *ctr;
    int *vtx;                                    // [4][V] outc, inc, nxt, cnt (zeroed as one)
    int *jmp0, *jmp1, *mn0, *mn1, *hflag, *cflag, *hstart, *cstart, *bparent, *onb;
    EdgeTable t;
    void *tmp;
    char *base;
    size_t bytes;
};
HfWs carve_hf(char *base, size_t V, unsigned ecap, size_t tmp_bytes) {
    Carver c{base};
    HfWs w;
    w.ctl = c.take<int>(16);
    w.ctr = c.take<unsigned long long>(16);
    w.vtx = c.take<int>(V * 4);
    w.jmp0 = c.take<int>(V);
    w.jmp1 = c.take<int>(V);
    w.mn0 = c.take<int>(V);
    w.mn1 = c.take<int>(V);
    w.hflag = c.take<int>(V + 1);
    w.cflag = c.take<int>(V + 1);
    w.hstart = c.take<int>(V + 1);
    w.cstart = c.take<int>(V + 1);
    w.bparent = c.take<int>(V);
    w.onb = c.take<int>(V);
    w.t = carve_edges(c, ecap);
    w.tmp = c.take<char>(tmp_bytes);
    return c.done(w);
}
struct HfLoopWs {                                // what the counts of the loops (H) and of the candidates (C) give
    int *htab, *cv0, *cn, *voff, *chole, *fill01, *addc, *foff;
    long long *ctri, *loff;
    double *harea, *area;
    char *base;
    size_t bytes;
};
HfLoopWs carve_hf_loops(char *base, size_t H, size_t C) {
    Carver c{base};
    HfLoopWs w;
    w.htab = c.take<int>(H * 4);
    w.harea = c.take<double>(H);
    w.cv0 = c.take<int>(C);
    w.cn = c.take<int>(C + 1);
    w.voff = c.take<int>(C + 1);
    w.chole = c.take<int>(C);
    w.fill01 = c.take<int>(C);
    w.addc = c.take<int>(C + 1);
    w.foff = c.take<int>(C + 1);
    w.ctri = c.take<long long>(C + 1);
    w.loff = c.take<long long>(C + 1);
    w.area = c.take<double>(C);
    return c.done(w);
}
struct HfDpWs {                                  // what the candidates' lengths give
    int *loopv;
    unsigned char *lam;
    char *base;
    size_t bytes;
};
HfDpWs carve_hf_dp(char *base, size_t sum_n, size_t sum_cells) {
    Carver c{base};
    HfDpWs w;
    w.loopv = c.take<int>(sum_n);
    w.lam = c.take<unsigned char>(sum_cells);
    return c.done(w);
}
struct HfOutWs {                                 // what the count of the output faces gives
    int *wf;
    EdgeTable t;
    char *base;
    size_t bytes;
};
HfOutWs carve_hf_out(char *base, size_t F1, unsigned ecap1, bool table) {
    Carver c{base};
    HfOutWs w;
    w.wf = c.take<int>(F1 * 3);
    w.t = table ? carve_edges(c, ecap1) : EdgeTable{};
    return c.done(w);
}

}  // namespace

extern "C" int p2s_mesh_fill_holes(const float *verts_dev, int64_t n_verts, const int32_t *faces_dev, int64_t n_faces, int max_hole_edges,
                                   int32_t *faces_out_dev, int64_t cap_faces, int32_t *face_src_out_dev, int32_t *holes_out_dev,
                                   double *hole_area_out_dev, int64_t cap_holes, int64_t *report_host, int device, void *stream) {
    static const char *const who = "p2s_mesh_fill_holes";
    const char *bad = mc_bad_mesh(verts_dev, n_verts, faces_dev, n_faces, report_host);
    if (!bad) {
        if (max_hole_edges < 0 || max_hole_edges > HF_MAX_EDGES) bad = "max_hole_edges outside 0 .. 128";
        else if (cap_faces < 0) bad = "cap_faces < 0";
        else if (cap_holes < 0) bad = "cap_holes < 0";
        else if (cap_faces > 0 && !faces_out_dev) bad = "faces_out_dev is NULL";
    }
    if (bad) {
        p2s_set_error("%s: bad argument (%s)", who, bad);
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

    // ---- a. validate; the edge table of the input
    const unsigned ecap = rp_table_cap(3 * F);
    size_t t1 = 0, t2 = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, t1, (int *)nullptr, (int *)nullptr, (int)(V + 1), nullptr);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, t2, (long long *)nullptr, (long long *)nullptr, (int)(V + 1), nullptr);
    const size_t tmp_bytes = std::max(t1, t2) + 256;
    const HfWs W = pool.carve([&](char *b) { return carve_hf(b, (size_t)V, ecap, tmp_bytes); });
    if (!W.base) return dev_oom(who, s);
    auto scan = [&](auto *in, auto *out, long long n) {              // exclusive, n entries
        size_t tb = tmp_bytes;
        return hipcub::DeviceScan::ExclusiveSum(W.tmp, tb, in, out, (int)n, s);
    };
    if (V > 0 || F > 0) {
        if ((rc = mc_validate(who, verts_dev, V, faces_dev, F, W.ctl, s)) != P2S_OK) return rc;
    }
    if (F == 0) {                                                    // no face, no boundary: nothing is written
        publish();
        return P2S_OK;
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
    unsigned long long hc[8] = {};
    DEV_CHECK(who, hipMemsetAsync(W.ctr, 0, MESH_COUNTERS, s));
    if ((rc = build_edges(who, faces_dev, F, W.t, nullptr, nullptr, s)) != P2S_OK) return rc;
    hipLaunchKernelGGL(p2s_rp_edge_stats_kernel, dim3(std::min(blocks((long long)ecap, 256), 1024u)), dim3(256), 0, s, W.t, W.ctr);      // few atomics
    if ((rc = read_counters(who, W.ctr, hc, -1, nullptr, s)) != P2S_OK) return rc;
    const long long nb = (long long)hc[HF_BOUNDARY], overfull_in = (long long)hc[HF_NONMANIFOLD];
    rep_out[7] = nb;

    // ---- b. the loops: pointer jumping over the simple vertices, then the table in ascending v0
    int *outc = W.vtx, *inc = outc + V, *nxt = inc + V, *cnt = nxt + V;
    long long H = 0, C = 0;
    if (nb > 0) {
        DEV_CHECK(who, hipMemsetAsync(W.vtx, 0, (size_t)V * 4 * 4, s));
        hipLaunchKernelGGL(p2s_rp_boundary_kernel, dim3(blocks(3 * F, 256)), dim3(256), 0, s, faces_dev, F, W.t, (const unsigned char *)nullptr,
                           outc, inc, nxt, (int *)nullptr);
        hipLaunchKernelGGL(p2s_hf_init_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, V, outc, inc, nxt, W.jmp0, W.mn0);
        int *ja = W.jmp0, *ma = W.mn0, *jb = W.jmp1, *mb = W.mn1;
        for (long long reach = 1; reach <= nb; reach *= 2) {        // 2^R > nb >= the simple vertices: see the head of this file
            hipLaunchKernelGGL(p2s_hf_jump_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, V, ja, ma, jb, mb);
            std::swap(ja, jb);
            std::swap(ma, mb);
        }
        hipLaunchKernelGGL(p2s_hf_count_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, V, ja, ma, cnt);
        DEV_CHECK(who, hipMemsetAsync(W.hflag + V, 0, 4, s));
        DEV_CHECK(who, hipMemsetAsync(W.cflag + V, 0, 4, s));
        hipLaunchKernelGGL(p2s_hf_flags_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, V, K, ja, ma, cnt, W.hflag, W.cflag);
        DEV_CHECK(who, hipGetLastError());
        DEV_CHECK(who, scan(W.hflag, W.hstart, V + 1));
        DEV_CHECK(who, scan(W.cflag, W.cstart, V + 1));
        int hH = 0, hC = 0;
        DEV_CHECK(who, hipMemcpyAsync(&hH, W.hstart + V, 4, hipMemcpyDeviceToHost, s));
        DEV_CHECK(who, hipMemcpyAsync(&hC, W.cstart + V, 4, hipMemcpyDeviceToHost, s));
        DEV_CHECK(who, hipStreamSynchronize(s));
        H = hH;
        C = hC;
    }
    const HfLoopWs L = pool.carve([&](char *b) { return carve_hf_loops(b, (size_t)H, (size_t)C); });
    if (!L.base) return dev_oom(who, s);
    long long added = 0;
    DEV_CHECK(who, hipMemsetAsync(W.ctr, 0, MESH_COUNTERS, s));
    if (H > 0) {
        DEV_CHECK(who, hipMemsetAsync(L.cn + C, 0, 4, s));
        DEV_CHECK(who, hipMemsetAsync(L.ctri + C, 0, 8, s));
        DEV_CHECK(who, hipMemsetAsync(L.addc + C, 0, 4, s));
        hipLaunchKernelGGL(p2s_hf_loops_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, V, W.hflag, W.cflag, W.hstart, W.cstart, cnt, L.htab,
                           L.harea, L.cv0, L.cn, L.ctri, L.chole);
        DEV_CHECK(who, hipGetLastError());
    }
    // ---- c. the candidates: their vertices, the dynamic programme, the faces
    HfDpWs D = {};
    if (C > 0) {
        DEV_CHECK(who, scan(L.cn, L.voff, C + 1));
        DEV_CHECK(who, scan(L.ctri, L.loff, C + 1));
        int sum_n = 0;
        long long sum_cells = 0;
        DEV_CHECK(who, hipMemcpyAsync(&sum_n, L.voff + C, 4, hipMemcpyDeviceToHost, s));
        DEV_CHECK(who, hipMemcpyAsync(&sum_cells, L.loff + C, 8, hipMemcpyDeviceToHost, s));
        DEV_CHECK(who, hipStreamSynchronize(s));
        D = pool.carve([&](char *b) { return carve_hf_dp(b, (size_t)sum_n, (size_t)sum_cells); });
        if (!D.base) return dev_oom(who, s);
        hipLaunchKernelGGL(p2s_hf_walk_kernel, dim3(blocks(C, 256)), dim3(256), 0, s, C, L.cv0, L.cn, L.voff, nxt, D.loopv);
        hipLaunchKernelGGL((p2s_hf_dp_kernel<64, HF_SMALL_EDGES>), dim3((unsigned)C), dim3(64), 0, s, verts_dev, W.t, L.cn, L.voff, L.loff,
                           D.loopv, 0, D.lam, L.area, L.fill01);
        if (K > HF_SMALL_EDGES)
            hipLaunchKernelGGL((p2s_hf_dp_kernel<256, HF_MAX_EDGES>), dim3((unsigned)C), dim3(256), 0, s, verts_dev, W.t, L.cn, L.voff, L.loff,
                               D.loopv, HF_SMALL_EDGES, D.lam, L.area, L.fill01);
        hipLaunchKernelGGL(p2s_hf_addc_kernel, dim3(blocks(C, 256)), dim3(256), 0, s, C, L.cn, L.fill01, L.addc);
        DEV_CHECK(who, hipGetLastError());
        DEV_CHECK(who, scan(L.addc, L.foff, C + 1));
        int h_added = 0;
        DEV_CHECK(who, hipMemcpyAsync(&h_added, L.foff + C, 4, hipMemcpyDeviceToHost, s));
        DEV_CHECK(who, hipStreamSynchronize(s));
        added = h_added;
    }
    const long long F1 = F + added;
    const unsigned ecap1 = rp_table_cap(3 * F1);
    const HfOutWs O = pool.carve([&](char *b) { return carve_hf_out(b, (size_t)F1, ecap1, added > 0); });
    if (!O.base) return dev_oom(who, s);
    DEV_CHECK(who, hipMemcpyAsync(O.wf, faces_dev, (size_t)F * 12, hipMemcpyDeviceToDevice, s));
    if (added > 0)
        hipLaunchKernelGGL(p2s_hf_emit_kernel, dim3(blocks(C, 64)), dim3(64), 0, s, C, L.cn, L.voff, L.loff, D.loopv, D.lam, L.fill01, L.foff,
                           L.area, L.chole, F, O.wf, L.htab, L.harea, W.ctr);

    // ---- e. the report, from the edge table of the output (of the input again where nothing was added)
    EdgeTable to = W.t;
    if (added > 0) {
        to = O.t;
        if ((rc = build_edges(who, O.wf, F1, to, nullptr, nullptr, s)) != P2S_OK) return rc;
    }
    hipLaunchKernelGGL(p2s_rp_edge_stats_kernel, dim3(std::min(blocks((long long)to.mask + 1, 256), 1024u)), dim3(256), 0, s, to, W.ctr);
    hipLaunchKernelGGL(p2s_iota_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, W.bparent, V);
    rc = until_unchanged(who, "the groups of the boundary edges", V + 1, W.ctl, s, [&](long long) {
        hipLaunchKernelGGL(p2s_rp_bhook_kernel, dim3(blocks(3 * F1, 256)), dim3(256), 0, s, O.wf, F1, to, W.bparent, W.ctl);
        hipLaunchKernelGGL(p2s_uf_compress_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, W.bparent, V);
    });
    if (rc != P2S_OK) return rc;
    DEV_CHECK(who, hipMemsetAsync(W.onb, 0, (size_t)V * 4, s));
    hipLaunchKernelGGL(p2s_rp_bmark_kernel, dim3(blocks(3 * F1, 256)), dim3(256), 0, s, O.wf, F1, to, W.onb);
    hipLaunchKernelGGL(p2s_rp_bcount_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, W.bparent, W.onb, V, W.ctr + HF_BGROUPS);
    if ((rc = read_counters(who, W.ctr, hc, -1, nullptr, s)) != P2S_OK) return rc;
    const long long filled = (long long)hc[HF_FILLED];
    rep_out[1] = F1;
    rep_out[2] = H;
    rep_out[3] = filled;
    rep_out[4] = added;
    rep_out[5] = H - C;
    rep_out[6] = C - filled;
    rep_out[8] = (long long)hc[HF_BOUNDARY];
    rep_out[9] = (long long)hc[HF_BGROUPS];
    rep_out[10] = (long long)hc[HF_LONGEST];
    rep_out[11] = (long long)hc[HF_NONMANIFOLD];
    if (rep_out[11] != overfull_in) {
        p2s_set_error("%s: internal error (the fill changed the count of the edges of more than two faces)", who);
        return P2S_EHIP;
    }
    publish();
    const bool want_holes = holes_out_dev || hole_area_out_dev;
    if (cap_faces < F1 || (want_holes && cap_holes < H)) {
        p2s_set_error("%s: output buffers too small (%lld faces and %lld holes needed, cap_faces = %lld and cap_holes = %lld given)", who, F1, H,
                      (long long)cap_faces, (long long)cap_holes);
        return P2S_EINVAL;
    }
    DEV_CHECK(who, hipMemcpyAsync(faces_out_dev, O.wf, (size_t)F1 * 12, hipMemcpyDeviceToDevice, s));
    if (face_src_out_dev) hipLaunchKernelGGL(p2s_hf_src_kernel, dim3(blocks(F1, 256)), dim3(256), 0, s, F, F1, face_src_out_dev);
    DEV_CHECK(who, hipGetLastError());
    if (holes_out_dev && H > 0) DEV_CHECK(who, hipMemcpyAsync(holes_out_dev, L.htab, (size_t)H * 16, hipMemcpyDeviceToDevice, s));
    if (hole_area_out_dev && H > 0) DEV_CHECK(who, hipMemcpyAsync(hole_area_out_dev, L.harea, (size_t)H * 8, hipMemcpyDeviceToDevice, s));
    DEV_CHECK(who, hipStreamSynchronize(s));
    return P2S_OK;
}
