// Occupancy of a closed mesh on the volume's grid (p2s_mesh_voxelize) and the reductions of the quality report
// (p2s_surface_stats, p2s_occupancy_counts).  Included by p2s_meshdist.hip behind the check; the rule is the project's own
// and is stated in include/p2s_hip.h.
//   p2s_vx_index_kernel        one column (x, y) = (c(i), c(j)) per lane walks the octree: a node is opened when its closed
//                              xy rectangle contains the column; the faces of every leaf it opens get the column rule
//   p2s_vx_exhaustive_kernel   every column against every face, the faces staged through LDS (the yardstick)
//   p2s_vx_voxels_kernel       one voxel per lane: its side of every crossing of its column, the winding number
//   p2s_vx_apply_kernel        the undecided voxels from their exact winding sums (p2s_md_winding_kernel)
//   p2s_ss_partial_kernel / p2s_ss_final_kernel   the sums, the maximum and the counts of the surface samples
//   p2s_oc_counts_kernel       |A|, |B|, |A and B| of two occupancy arrays
// Both column kernels run twice, like the pair kernels of the check: a count pass (counters, crossings per column, the
// undecided columns), then, behind p2s_scan_kernel, a fill pass that writes the crossing faces (f for sigma = +1, ~f
// for sigma = -1) into the column's own range.  The order inside a range is whatever the atomics give: the winding number
// is a sum of integers and "undecided" an OR, so no result depends on it.  The voxel kernel runs twice too: a count pass
// (voxels inside, singly undecided voxels), after which U is known and the capacity rule is applied BEFORE any output is
// written, then the pass that writes.
//
// Why the filter bounds of p2s_meshcheck.inl hold here.  The proof there uses two facts about every operand of orient2 and
// orient3: it is a float32 value held exactly in float64, and its magnitude is at most S.  A voxel centre is the float32
// nearest to ((i + 0.5) / R) * 2 - 1 (the host computes the R centres once in float64 and rounds them; the kernels read that
// table), so it is a float32 value held exactly, and |c| <= 1 - 1 / R < 1.  With S' = max(S, 1) both facts hold for the vertices
// and for the centres alike, every step of the proof goes through with S' in the place of S, and a computed orient2 beyond
// 2^-47 S'^2, or orient3 beyond 2^-43 S'^3, has the sign of the exact value.  orient2 is taken on x and y (z dropped) through
// orient2_sign with the axes 0 and 1, orient3 through orient3 / mc_sign: the one place each is computed.

namespace {

enum VoxelCtr { VX_TESTS, VX_CROSSINGS, VX_UCOLS, VX_OVERFLOW, VX_INSIDE, VX_SINGLE, VX_LISTED, VX_FB_INSIDE };

struct ColumnArgs {
    const float *centre;           // [R] the voxel centres of one axis
    int R;
    double eps2;
    int *count;                    // count pass: [R^2] crossings of the column
    int *ucol;                     // count pass: [R^2] the column is undecided
    const int *start;              // fill pass: [R^2 + 1]
    int *cursor;                   // fill pass: [R^2], zeroed
    int *list;                     // fill pass: [crossings] f or ~f; NULL in the count pass
    unsigned long long *ctr;
};

// what one lane keeps of its column
struct ColumnTally {
    unsigned long long tests = 0, cross = 0;
    bool undecided = false;
};

// the column through P = (px, py, .) against the face T [9]: 0 = it misses, +1 / -1 = it crosses with that direction,
// 2 = the column is undecided
__device__ __forceinline__ int vx_face(const double *T, const double *P, double eps2) {
    if (P[0] < fmin(T[0], fmin(T[3], T[6])) || P[0] > fmax(T[0], fmax(T[3], T[6])) || P[1] < fmin(T[1], fmin(T[4], T[7])) ||
        P[1] > fmax(T[1], fmax(T[4], T[7])))
        return 0;
    const int s0 = orient2_sign(T + 3, T + 6, P, 0, 1, eps2), s1 = orient2_sign(T + 6, T, P, 0, 1, eps2),
              s2 = orient2_sign(T, T + 3, P, 0, 1, eps2);
    if ((s0 > 0 || s1 > 0 || s2 > 0) && (s0 < 0 || s1 < 0 || s2 < 0)) return 0;
    const int sigma = orient2_sign(T, T + 3, T + 6, 0, 1, eps2);
    return sigma != 0 && s0 == sigma && s1 == sigma && s2 == sigma ? sigma : 2;
}
__device__ __forceinline__ void vx_note(const ColumnArgs &a, long long col, int f, int code, ColumnTally &t) {
    ++t.tests;
    if (code == 2) t.undecided = true;
    else if (code != 0) {
        ++t.cross;
        if (a.list) a.list[a.start[col] + atomicAdd(&a.cursor[col], 1)] = code > 0 ? f : ~f;
    }
}
// the end of a lane's count pass: the column's own words (several lanes share a column in the exhaustive kernel), then
// the counters of the call; every lane of the wave arrives here
__device__ __forceinline__ void vx_tally(const ColumnArgs &a, bool live, long long col, const ColumnTally &t) {
    unsigned long long ucols = 0;
    if (live && t.cross) atomicAdd(&a.count[col], (int)t.cross);
    if (live && t.undecided && atomicOr(&a.ucol[col], 1) == 0) ucols = 1;      // counted by the first lane to say so
    wave_count(a.ctr + VX_TESTS, t.tests);
    wave_count(a.ctr + VX_CROSSINGS, t.cross);
    wave_count(a.ctr + VX_UCOLS, ucols);
}

// The node boxes are the float32 bounds of their triangles, so a column outside a node's closed rectangle is outside the
// closed xy box of every face below it: what is not opened would have missed.  The comparison is made on the values (not
// on the ordered integers, which tell -0.0 from +0.0), as vx_face makes it.  Every face sits in exactly one leaf.
__global__ __launch_bounds__(64) void p2s_vx_index_kernel(OctreeDev ix, ColumnArgs a) {
    __shared__ int lds[OCT_STACK * 64];
    const int lane = threadIdx.x;
    const long long col = (long long)blockIdx.x * 64 + lane;
    const bool live = col < (long long)a.R * a.R;
    ColumnTally t;
    if (live) {
        const int i = (int)(col / a.R), j = (int)(col - (long long)i * a.R);
        const double P[3] = {(double)a.centre[i], (double)a.centre[j], 0.0};
        LaneStack stack(lds, lane);
        stack.push(oct_id(0, 0), a.ctr + VX_OVERFLOW);
        while (!stack.empty()) {
            const int node = stack.pop();
            const int l = oct_level(node), lin = oct_lin(node);
            if (l == ix.L) {
                int t0, t1;
                oct_leaf_range(ix, lin, &t0, &t1);
                for (int s = t0; s < t1; ++s) vx_note(a, col, ix.sface[s], vx_face(ix.stri + 9 * (long long)s, P, a.eps2), t);
            } else {
                int xyz[3];
                oct_xyz(l, lin, xyz);
                for (int c = 7; c >= 0; --c) {
                    const int clin = oct_child_lin(l, xyz, c);
                    const int *cb = oct_box(ix, l + 1, clin);
                    if (cb[0] > cb[3]) continue;             // empty
                    if ((double)o2f(cb[0]) <= P[0] && P[0] <= (double)o2f(cb[3]) && (double)o2f(cb[1]) <= P[1] && P[1] <= (double)o2f(cb[4]))
                        stack.push(oct_id(l + 1, clin), a.ctr + VX_OVERFLOW);
                }
            }
        }
    }
    if (!a.list) vx_tally(a, live, col, t);
}

// every column against the faces [y * per, (y + 1) * per)
constexpr int VX_TILE = 128;
__global__ __launch_bounds__(256) void p2s_vx_exhaustive_kernel(const double *__restrict__ tri, long long F, long long per, ColumnArgs a) {
    __shared__ double tile[VX_TILE * 9];
    const long long col = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long f0 = (long long)blockIdx.y * per, f1 = min(F, f0 + per);
    const bool live = col < (long long)a.R * a.R;
    double P[3] = {0.0, 0.0, 0.0};
    if (live) {
        const int i = (int)(col / a.R), j = (int)(col - (long long)i * a.R);
        P[0] = (double)a.centre[i];
        P[1] = (double)a.centre[j];
    }
    ColumnTally t;
    for (long long b0 = f0; b0 < f1; b0 += VX_TILE) {
        const int lim = (int)min((long long)VX_TILE, f1 - b0);
        for (int k = threadIdx.x; k < lim * 9; k += 256) tile[k] = tri[9 * b0 + k];
        __syncthreads();
        if (live)
            for (int g = 0; g < lim; ++g) vx_note(a, col, (int)(b0 + g), vx_face(tile + 9 * g, P, a.eps2), t);
        __syncthreads();
    }
    if (!a.list) vx_tally(a, live, col, t);
}

struct VoxelArgs {
    const double *tri;             // [F][9]
    const float *centre;           // [R]
    int R;
    double eps3;
    const int *start, *list, *ucol;
    unsigned char *occ, *flags;    // write pass: the outputs (flags may be NULL); occ NULL: the count pass
    long long *uvox;               // write pass: [U] the undecided voxels
    float *uq;                     //             [U][3] and their centres
    unsigned long long cap;        //             U, as the count pass found it
    unsigned long long *ctr;
};

// voxel v = (i R + j) R + k.  Count pass: the voxels inside and the singly undecided ones; write pass: occ, flags, and the
// undecided voxels (every voxel of an undecided column, and the singly undecided) appended for the exact sum.
__global__ __launch_bounds__(256) void p2s_vx_voxels_kernel(VoxelArgs a) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    unsigned long long inside = 0, single = 0;
    if (v < ((long long)a.R * a.R) * a.R) {
        const long long col = v / a.R;
        const int k = (int)(v - col * a.R), i = (int)(col / a.R), j = (int)(col - (long long)i * a.R);
        const double p[3] = {(double)a.centre[i], (double)a.centre[j], (double)a.centre[k]};
        const bool column = a.ucol[col] != 0;
        bool one = false;
        int w = 0;
        if (!column) {
            const int s1 = a.start[col + 1];
            for (int s = a.start[col]; s < s1; ++s) {
                const int e = a.list[s], sigma = e >= 0 ? 1 : -1;
                const double *T = a.tri + 9 * (long long)(e >= 0 ? e : ~e);
                const int side = mc_sign(orient3(T, T + 3, T + 6, p), a.eps3) * sigma;
                one = one || side == 0;
                if (side < 0) w += sigma;
            }
        }
        const bool undecided = column || one;
        single = one ? 1 : 0;
        inside = !undecided && w != 0 ? 1 : 0;
        if (a.occ) {
            a.occ[v] = (unsigned char)inside;
            if (a.flags) a.flags[v] = undecided ? 1 : 0;
            if (undecided) {
                const unsigned long long u = atomicAdd(a.ctr + VX_LISTED, 1ull);
                if (u < a.cap) {
                    a.uvox[u] = v;
                    for (int d = 0; d < 3; ++d) a.uq[3 * u + d] = (float)p[d];
                }
            }
        }
    }
    if (!a.occ) {
        wave_count(a.ctr + VX_INSIDE, inside);
        wave_count(a.ctr + VX_SINGLE, single);
    }
}

__global__ __launch_bounds__(256) void p2s_vx_apply_kernel(const double *__restrict__ w, const long long *__restrict__ uvox, long long U,
                                                           unsigned char *__restrict__ occ, unsigned long long *ctr) {
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
    unsigned long long inside = 0;
    if (u < U) {
        inside = fabs(w[u]) > 0.5 ? 1 : 0;
        occ[uvox[u]] = (unsigned char)inside;
    }
    wave_count(ctr + VX_FB_INSIDE, inside);
}

struct VoxelWs {
    float *centre;
    int *count, *start, *cursor, *ucol;
    unsigned long long *ctr;
    char *base;
    size_t bytes;
};
struct VoxelFallbackWs {
    long long *uvox;
    float *uq;
    double *w;
    char *base;
    size_t bytes;
};

// ---- the reductions of the quality report
// Order of the sums (it depends on n alone): term i is added, in ascending i, by thread i mod 65536 of a fixed grid of 256
// workgroups of 256; the 64 lanes of a wave are combined by the butterfly xor 32, 16, .., 1 (a + b on both sides: the same
// bits in every lane), the four waves of a workgroup in ascending order, and the 256 workgroup values once more in the same
// way by one workgroup.  All float64, contraction off.
constexpr int SS_BLOCKS = 256, SS_MAX_TAUS = 8, SS_SLOTS = 5 + SS_MAX_TAUS;       // sum d, sum d^2, max d, sum |n.n|, pairs, counts
struct SurfaceTaus {
    double tau[SS_MAX_TAUS];
    int n;
};

// v [SS_SLOTS] of every thread of a workgroup of 256 into out [SS_SLOTS], written by thread 0 (slot 2 is a maximum)
__device__ __forceinline__ void ss_reduce(double *v, double *out) {
    __shared__ double ws[4][SS_SLOTS];
    for (int k = 0; k < SS_SLOTS; ++k) {
        for (int d = 32; d > 0; d >>= 1) {
            const double o = __shfl_xor(v[k], d);
            v[k] = k == 2 ? fmax(v[k], o) : v[k] + o;
        }
        if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 0; k < SS_SLOTS; ++k)
            out[k] = k == 2 ? fmax(fmax(ws[0][k], ws[1][k]), fmax(ws[2][k], ws[3][k])) : ((ws[0][k] + ws[1][k]) + ws[2][k]) + ws[3][k];
}

__global__ __launch_bounds__(256) void p2s_ss_partial_kernel(const double *__restrict__ dist, const int *__restrict__ face_from,
                                                             const int *__restrict__ face_to, long long n, const double *__restrict__ fn_from,
                                                             long long F_from, const double *__restrict__ fn_to, long long F_to,
                                                             SurfaceTaus taus, double *__restrict__ part) {
    double v[SS_SLOTS];
    for (int k = 0; k < SS_SLOTS; ++k) v[k] = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)SS_BLOCKS * 256) {
        const double d = dist[i];
        v[0] += d;
        v[1] += d * d;
        v[2] = fmax(v[2], d);
        const long long f = face_from[i], g = face_to[i];
        if (f >= 0 && f < F_from && g >= 0 && g < F_to) {
            const double *a = fn_from + 3 * f, *b = fn_to + 3 * g;
            const bool za = a[0] == 0.0 && a[1] == 0.0 && a[2] == 0.0, zb = b[0] == 0.0 && b[1] == 0.0 && b[2] == 0.0;
            if (!za && !zb) {                      // a face under the degenerate rule has the normal 0
                v[3] += fabs(dot3(a, b));
                v[4] += 1.0;
            }
        }
        for (int t = 0; t < taus.n; ++t) v[5 + t] += d <= taus.tau[t] ? 1.0 : 0.0;
    }
    ss_reduce(v, part + (long long)blockIdx.x * SS_SLOTS);
}
__global__ __launch_bounds__(256) void p2s_ss_final_kernel(const double *__restrict__ part, double *__restrict__ out) {
    double v[SS_SLOTS];
    for (int k = 0; k < SS_SLOTS; ++k) v[k] = part[(long long)threadIdx.x * SS_SLOTS + k];
    ss_reduce(v, out);
}

// a byte that is not 0 is occupied; ctr: |A|, |B|, |A and B|
__global__ __launch_bounds__(256) void p2s_oc_counts_kernel(const unsigned char *__restrict__ a, const unsigned char *__restrict__ b, long long n,
                                                            unsigned long long *ctr) {
    unsigned long long na = 0, nb = 0, nab = 0;
    for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 8; i < n; i += (long long)gridDim.x * 256 * 8) {
        const int lim = (int)min(8ll, n - i);
        for (int k = 0; k < lim; ++k) {
            const bool x = a[i + k] != 0, y = b[i + k] != 0;
            na += x;
            nb += y;
            nab += x && y;
        }
    }
    wave_count(ctr, na);
    wave_count(ctr + 1, nb);
    wave_count(ctr + 2, nab);
}

}  // namespace

extern "C" int p2s_mesh_voxelize(p2s_trimesh_t m, int grid_res, int method, int64_t max_fallback, uint8_t *occ_out_dev,
                                 uint8_t *flags_out_dev, int64_t *report_host, void *stream) {
    static const char *const who = "p2s_mesh_voxelize";
    if (report_host)
        for (int k = 0; k < 8; ++k) report_host[k] = 0;
    if (!m || !report_host || !occ_out_dev || grid_res < 2 || grid_res > 1024 || (method != 0 && method != 1) || max_fallback < 0) {
        p2s_set_error("p2s_mesh_voxelize: bad argument (grid_res in 2..1024, method 0 or 1, max_fallback >= 0, occ and a report)");
        return P2S_EINVAL;
    }
    if (!m->closed) {
        p2s_set_error("p2s_mesh_voxelize: the mesh is not closed (%lld open or non-manifold edges): no inside", m->bad_edges);
        return P2S_EINVAL;
    }
    P2S_HIP_CHECK(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    const long long R = grid_res, cols = R * R, voxels = cols * R, F = m->F;
    PoolScratch pool(m->device, s);
    const VoxelWs w = pool.carve([&](char *b) {
        Carver c{b};
        VoxelWs r;
        r.centre = c.take<float>((size_t)R);
        r.count = c.take<int>((size_t)cols);
        r.start = c.take<int>((size_t)cols + 1);
        r.cursor = c.take<int>((size_t)cols);
        r.ucol = c.take<int>((size_t)cols);
        r.ctr = c.take<unsigned long long>(8);
        return c.done(r);
    });
    if (!w.base) return dev_oom(who, s);
    std::vector<float> centre((size_t)R);
    for (long long i = 0; i < R; ++i) centre[(size_t)i] = (float)((((double)i + 0.5) / (double)R) * 2.0 - 1.0);
    DEV_CHECK(who, hipMemcpyAsync(w.centre, centre.data(), (size_t)R * 4, hipMemcpyHostToDevice, s));
    DEV_CHECK(who, hipMemsetAsync(w.ctr, 0, MESH_COUNTERS, s));
    DEV_CHECK(who, hipMemsetAsync(w.count, 0, (size_t)cols * 4, s));
    DEV_CHECK(who, hipMemsetAsync(w.cursor, 0, (size_t)cols * 4, s));
    DEV_CHECK(who, hipMemsetAsync(w.ucol, 0, (size_t)cols * 4, s));

    const double S = std::max(m->scale, 1.0);
    ColumnArgs ca = {w.centre, grid_res, (S * S) * 7.105427357601002e-15, w.count, w.ucol, w.start, w.cursor, nullptr, w.ctr};      // 2^-47
    int parts = 1;
    long long per = F;
    if (method == 1) exhaustive_parts(F, cols, VX_TILE, &parts, &per);
    auto columns_pass = [&] {
        if (method == 0) hipLaunchKernelGGL(p2s_vx_index_kernel, dim3(blocks(cols, 64)), dim3(64), 0, s, octree_of(m), ca);
        else hipLaunchKernelGGL(p2s_vx_exhaustive_kernel, dim3(blocks(cols, 256), parts), dim3(256), 0, s, m->tri, F, per, ca);
    };
    columns_pass();
    unsigned long long hc[8] = {};
    int rc = read_counters(who, w.ctr, hc, VX_OVERFLOW, "the walk overflowed its stack", s);
    if (rc != P2S_OK) return rc;
    if (hc[VX_CROSSINGS] > 0x7fffffffull) {
        p2s_set_error("p2s_mesh_voxelize: %llu crossings, more than the layout holds", hc[VX_CROSSINGS]);
        return P2S_ECAPACITY;
    }
    hipLaunchKernelGGL(p2s_scan_kernel, dim3(1), dim3(1024), 0, s, w.count, cols, w.start);
    if (hc[VX_CROSSINGS] > 0) {
        ca.list = pool.get<int>((size_t)hc[VX_CROSSINGS]);
        if (!ca.list) return dev_oom(who, s);
        columns_pass();
    }
    VoxelArgs va = {m->tri, w.centre, grid_res, ((S * S) * S) * 1.1368683772161603e-13, w.start, ca.list, w.ucol,      // 2^-43
                    nullptr, nullptr, nullptr, nullptr, 0, w.ctr};
    hipLaunchKernelGGL(p2s_vx_voxels_kernel, dim3(blocks(voxels, 256)), dim3(256), 0, s, va);
    if ((rc = read_counters(who, w.ctr, hc, VX_OVERFLOW, "the walk overflowed its stack", s)) != P2S_OK) return rc;

    const unsigned long long U = hc[VX_UCOLS] * (unsigned long long)R + hc[VX_SINGLE];
    report_host[0] = (int64_t)hc[VX_INSIDE];
    report_host[1] = (int64_t)hc[VX_UCOLS];
    report_host[2] = (int64_t)hc[VX_SINGLE];
    report_host[3] = (int64_t)U;
    report_host[4] = (int64_t)hc[VX_TESTS];
    report_host[5] = (int64_t)hc[VX_CROSSINGS];
    if (U > (unsigned long long)max_fallback || U > 0x7fffffffull) {
        p2s_set_error("p2s_mesh_voxelize: %llu undecided voxels (report [3]), max_fallback %lld", U, (long long)max_fallback);
        return P2S_ECAPACITY;
    }
    VoxelFallbackWs fw = {};
    if (U > 0) {
        fw = pool.carve([&](char *b) {
            Carver c{b};
            VoxelFallbackWs r;
            r.uvox = c.take<long long>((size_t)U);
            r.uq = c.take<float>((size_t)U * 3);
            r.w = c.take<double>((size_t)U);
            return c.done(r);
        });
        if (!fw.base) return dev_oom(who, s);
    }
    va.occ = occ_out_dev;
    va.flags = flags_out_dev;
    va.uvox = fw.uvox;
    va.uq = fw.uq;
    va.cap = U;
    hipLaunchKernelGGL(p2s_vx_voxels_kernel, dim3(blocks(voxels, 256)), dim3(256), 0, s, va);
    if (U > 0) {
        hipLaunchKernelGGL(p2s_md_winding_kernel, dim3((unsigned)U), dim3(256), 0, s, m->tri, F, (const float *)fw.uq, (const int *)nullptr,
                           (double *)nullptr, fw.w, (double *)nullptr);
        hipLaunchKernelGGL(p2s_vx_apply_kernel, dim3(blocks((long long)U, 256)), dim3(256), 0, s, fw.w, fw.uvox, (long long)U, occ_out_dev, w.ctr);
    }
    if ((rc = read_counters(who, w.ctr, hc, VX_OVERFLOW, "the walk overflowed its stack", s)) != P2S_OK) return rc;
    if (hc[VX_LISTED] != U) {
        p2s_set_error("p2s_mesh_voxelize: %llu undecided voxels listed, %llu counted", hc[VX_LISTED], U);
        return P2S_EHIP;
    }
    report_host[0] = (int64_t)(hc[VX_INSIDE] + hc[VX_FB_INSIDE]);
    return P2S_OK;
}

extern "C" int p2s_surface_stats(p2s_trimesh_t from, p2s_trimesh_t to, const double *dist_dev, const int32_t *face_from_dev,
                                 const int32_t *face_to_dev, int64_t n, const double *taus_host, int n_taus, double *out_host,
                                 int64_t *nc_pairs_host, void *stream) {
    static const char *const who = "p2s_surface_stats";
    if (!from || !to || from->device != to->device || n < 0 || n > (1ll << 30) || (n > 0 && (!dist_dev || !face_from_dev || !face_to_dev)) ||
        n_taus < 0 || n_taus > SS_MAX_TAUS || (n_taus > 0 && !taus_host) || !out_host || !nc_pairs_host) {
        p2s_set_error("p2s_surface_stats: bad argument (two handles of one device, at most 8 thresholds)");
        return P2S_EINVAL;
    }
    P2S_HIP_CHECK(hipSetDevice(from->device));
    hipStream_t s = (hipStream_t)stream;
    PoolScratch pool(from->device, s);
    double *part = pool.get<double>((size_t)(SS_BLOCKS + 1) * SS_SLOTS);
    if (!part) return dev_oom(who, s);
    SurfaceTaus taus = {};
    taus.n = n_taus;
    for (int t = 0; t < n_taus; ++t) taus.tau[t] = taus_host[t];
    double *out = part + (size_t)SS_BLOCKS * SS_SLOTS, h[SS_SLOTS] = {};
    hipLaunchKernelGGL(p2s_ss_partial_kernel, dim3(SS_BLOCKS), dim3(256), 0, s, dist_dev, face_from_dev, face_to_dev, (long long)n, from->fn,
                       from->F, to->fn, to->F, taus, part);
    hipLaunchKernelGGL(p2s_ss_final_kernel, dim3(1), dim3(256), 0, s, (const double *)part, out);
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipMemcpyAsync(h, out, sizeof(h), hipMemcpyDeviceToHost, s));
    DEV_CHECK(who, hipStreamSynchronize(s));
    for (int k = 0; k < 4; ++k) out_host[k] = h[k];
    *nc_pairs_host = (int64_t)h[4];
    for (int t = 0; t < n_taus; ++t) out_host[4 + t] = h[5 + t];
    return P2S_OK;
}

extern "C" int p2s_occupancy_counts(const uint8_t *occ_a_dev, const uint8_t *occ_b_dev, int64_t n, int64_t *counts_host, int device,
                                    void *stream) {
    static const char *const who = "p2s_occupancy_counts";
    if (n < 0 || (n > 0 && (!occ_a_dev || !occ_b_dev)) || !counts_host) {
        p2s_set_error("p2s_occupancy_counts: bad argument");
        return P2S_EINVAL;
    }
    P2S_HIP_CHECK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    PoolScratch pool(device, s);
    unsigned long long *ctr = pool.get<unsigned long long>(MESH_COUNTERS / 8), hc[8] = {};
    if (!ctr) return dev_oom(who, s);
    DEV_CHECK(who, hipMemsetAsync(ctr, 0, MESH_COUNTERS, s));
    hipLaunchKernelGGL(p2s_oc_counts_kernel, dim3((unsigned)std::min<long long>(blocks((n + 7) / 8, 256), 4096)), dim3(256), 0, s, occ_a_dev,
                       occ_b_dev, (long long)n, ctr);
    const int rc = read_counters(who, ctr, hc, -1, nullptr, s);
    if (rc != P2S_OK) return rc;
    for (int k = 0; k < 3; ++k) counts_host[k] = (int64_t)hc[k];
    return P2S_OK;
}
