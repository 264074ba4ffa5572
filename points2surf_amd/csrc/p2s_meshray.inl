// "next" row f-6: first-hit ray casting on the mesh handle, the time-of-flight scan built on it, and the query points of
// the GT data -- the part of the reference's make_dataset.py that starts one BlenSor process per mesh (:242-380, 5..30
// scans of 176 x 144 rays) and calls trimesh (source/sdf.py:288-315).  Included at the end of p2s_meshdist.hip: the
// handle, the octree with its walk helpers (p2s_mesh_octree.inl), the host scaffold, the ordered-integer bounds, dot3 /
// cross3 / finite3, DEGENERATE_REL and the one-workgroup scan (p2s_scan_kernel) are that unit's, used here, not copied.
//   p2s_mr_index_kernel       first hit per ray: depth-first descent of the octree, children in the ray's front-to-back order
//   p2s_mr_exhaustive_kernel  every ray against every triangle, faces split over grid.y, prepared triangles staged in LDS
//   p2s_mr_merge_kernel       the parts of the exhaustive kernel into one answer per ray
//   p2s_mr_rays_kernel        the rays of S poses of the time-of-flight sensor, in model space
//   p2s_mr_count_kernel / p2s_mr_compact_kernel    hits per scan and per block; stable compaction of the hits
//   p2s_mr_query_pts_kernel   far points and surface samples offset along their face normal (05_query_pts)
//
// Intersection: Moeller-Trumbore (1997) with the scalar triple products taken through the face's own cross product, which
// the degenerate rule needs anyway.  With e1 = b - a, e2 = c - a, n = e1 x e2, s = o - a, q = s x d, dn = d . n:
//     u = -(e2 . q) / dn      v = (e1 . q) / dn      t = -(s . n) / dn        (det of Moeller-Trumbore = -dn)
// float64, contraction off, dot3 = (x + y) + z, cross3 as in this file: the CPU model (tests/scan_model.py) performs the
// same operations in the same association.
// Rules, stated once:
//  * a hit needs u >= 0, v >= 0, u + v <= 1 and t in (0, t_max]; the smallest t wins; ties go to the smallest face id;
//  * both sides of a face are hit (no back-face culling: a scanner sees what is there); dn == 0 (ray in the plane) misses;
//  * a face that is degenerate by DEGENERATE_REL (|e1 x e2|^2 <= 2^-90 |e1|^2 |e2|^2) is never hit;
//  * a hit whose computed point o + t d lies more than E = 2^-24 max(|mesh|, |o|) outside the face's own bounding box is
//    discarded: exact arithmetic never produces one, rounding can only at conditioning beyond 2^-28 (a ray grazing the
//    plane, a sliver's normal), and it is what makes the index provably equal to the exhaustive kernel (below);
//  * a direction component below 2^-1022 in magnitude (subnormal) is taken as 0;
//  * a ray with a non-finite component (|x| > 1e300) or a zero direction misses: face -1, t = +inf; no NaN leaves a
//    kernel (every acceptance is a conjunction of comparisons, false for NaN).

namespace {

constexpr double RAY_BOX_REL = 5.960464477539063e-08;      // 2^-24

// what of a triangle does not depend on the ray: a, e1, e2, n [3 each], bounding box lo, hi [3 each], ok (0: degenerate)
constexpr int PREP_DOUBLES = 19;

__device__ __forceinline__ void tri_prep(const double *__restrict__ t, double *__restrict__ p) {
    double e1[3], e2[3], n[3];
    for (int k = 0; k < 3; ++k) {
        e1[k] = t[3 + k] - t[k];
        e2[k] = t[6 + k] - t[k];
    }
    cross3(e1, e2, n);
    const bool ok = dot3(n, n) > DEGENERATE_REL * (dot3(e1, e1) * dot3(e2, e2));
    for (int k = 0; k < 3; ++k) {
        p[k] = t[k];
        p[3 + k] = e1[k];
        p[6 + k] = e2[k];
        p[9 + k] = n[k];
        p[12 + k] = fmin(t[k], fmin(t[3 + k], t[6 + k]));
        p[15 + k] = fmax(t[k], fmax(t[3 + k], t[6 + k]));
    }
    p[18] = ok ? 1.0 : 0.0;
}

// t of the hit, or +inf
__device__ __forceinline__ double ray_tri(const double *__restrict__ p, const double *o, const double *d, double t_max, double E) {
    if (!(p[18] > 0.0)) return INFINITY;
    const double dn = dot3(d, p + 9);
    if (!(dn != 0.0)) return INFINITY;
    double s[3], q[3];
    for (int k = 0; k < 3; ++k) s[k] = o[k] - p[k];
    cross3(s, d, q);
    const double u = -dot3(p + 6, q) / dn, v = dot3(p + 3, q) / dn, t = -dot3(s, p + 9) / dn;
    if (!(u >= 0.0 && v >= 0.0 && u + v <= 1.0 && t > 0.0 && t <= t_max)) return INFINITY;
    for (int k = 0; k < 3; ++k) {
        const double x = o[k] + t * d[k];
        if (!(x >= p[12 + k] - E && x <= p[15 + k] + E)) return INFINITY;
    }
    return t;
}

// a direction component below the smallest normal float64 is taken as 0 (its reciprocal is not finite); every kernel
// loads directions through this
__device__ __forceinline__ double ray_dir(double x) { return fabs(x) < 2.2250738585072014e-308 ? 0.0 : x; }
__device__ __forceinline__ bool ray_valid(const double *o, const double *d) {
    return finite3(o) && finite3(d) && (d[0] != 0.0 || d[1] != 0.0 || d[2] != 0.0);
}
__device__ __forceinline__ double ray_margin(double scale, const double *o) {
    return fmax(scale, fmax(fabs(o[0]), fmax(fabs(o[1]), fabs(o[2])))) * RAY_BOX_REL;
}

// entry parameter (>= 0) of the ray into the node's box grown by g, +inf when the ray misses it or the node is empty
__device__ __forceinline__ double slab_entry(const int *__restrict__ node, const double *o, const double *d, const double *inv, double g) {
    if (node[0] > node[3]) return INFINITY;             // empty: lo = +inf, hi = -inf
    double entry = 0.0, exit = INFINITY;
    for (int k = 0; k < 3; ++k) {
        const double lo = (double)o2f(node[k]) - g, hi = (double)o2f(node[3 + k]) + g;
        if (d[k] == 0.0) {
            if (!(o[k] >= lo && o[k] <= hi)) return INFINITY;
        } else {
            const double t1 = (lo - o[k]) * inv[k], t2 = (hi - o[k]) * inv[k];
            entry = fmax(entry, fmin(t1, t2));
            exit = fmin(exit, fmax(t1, t2));
        }
    }
    return entry <= exit ? entry : INFINITY;
}

// the ray enters the grown box, and not beyond `limit` (which may be +inf: a miss is no entry at +inf)
__device__ __forceinline__ bool slab_reaches(const int *__restrict__ node, const double *o, const double *d, const double *inv, double g,
                                             double limit) {
    const double e = slab_entry(node, o, d, inv, g);
    return e < INFINITY && e <= limit;
}

// Thread -> ray.  tile_w == 0: thread i casts ray i.  Otherwise the rays are S images of tile_h rows x tile_w columns
// (ray = (scan * tile_h + row) * tile_w + column) and a wave holds an 8 x 8 pixel tile of one image: its 64 rays leave one
// point in a narrow bundle, descend the same nodes and test the same triangles, so the wave diverges little.
__device__ __forceinline__ long long ray_of_thread(long long i, long long n, int tile_w, int tile_h) {
    if (tile_w == 0) return i < n ? i : -1;
    const int tx = (tile_w + 7) >> 3, ty = (tile_h + 7) >> 3, lane = (int)(i & 63);
    const long long wave = i >> 6, scan = wave / (tx * ty);
    const int tile = (int)(wave - scan * (tx * ty));
    const int px = (tile % tx) * 8 + (lane & 7), py = (tile / tx) * 8 + (lane >> 3);
    if (px >= tile_w || py >= tile_h) return -1;
    const long long r = (scan * tile_h + py) * tile_w + px;
    return r < n ? r : -1;
}

// First hit through the index.  A node is skipped only if the ray's entry into its box GROWN BY 2 E lies beyond
// min(best, t_max) (or the ray misses the grown box): the margin is spatial, 2 E = 2^-23 max(|mesh|, |o|), i.e. 2 E / |d_k|
// in t on every slab.  Why no triangle whose computed t would tie or beat the best is ever skipped: an accepted hit has its
// computed point within E of the face's bounding box (the last rule above), which lies inside the box of every node
// above it (node boxes are exact unions of the float32 vertex bounds); the exact point of the ray at the computed t
// differs from the computed one by 2 ulp of max(|o|, |hit|) <= 2^-51 M, and the computed slab parameters carry 2 ulp of
// |bound - o| / |d_k| <= 2^-50 M / |d_k| against a slack of E / |d_k| = 2^-24 M / |d_k|.  So the computed entry into the
// grown box is <= the computed t of every hit inside, with 26 bits to spare, whatever the conditioning of the
// intersection itself: t and face equal the exhaustive kernel's bit for bit.  The order of the descent changes the cost
// only.  The stack is a LaneStack (p2s_mesh_octree.inl): 13 KiB of LDS per wave, 12 waves per CU by LDS; 64 entries =
// 16 KiB = 10 waves measured the same to within run-to-run noise (profiles/scan/README.md).  Its overflow word is RC_OVERFLOW.
enum RayCtr { RC_TESTS, RC_OVERFLOW };
__global__ __launch_bounds__(64) void p2s_mr_index_kernel(OctreeDev ix, const double *__restrict__ rays, long long n, double t_max,
                                                          int tile_w, int tile_h, double *__restrict__ t_out, int *__restrict__ face_out,
                                                          unsigned long long *__restrict__ ctr) {
    __shared__ int lds[OCT_STACK * 64];
    const int lane = threadIdx.x;
    const long long r = ray_of_thread((long long)blockIdx.x * 64 + lane, n, tile_w, tile_h);
    unsigned long long tests = 0;
    if (r >= 0) {
        double o[3], d[3];
        for (int k = 0; k < 3; ++k) {
            o[k] = rays[6 * r + k];
            d[k] = ray_dir(rays[6 * r + 3 + k]);
        }
        double best = INFINITY;
        int bestf = -1;
        if (ray_valid(o, d) && t_max > 0.0) {
            const double E = ray_margin(ix.scale, o), g = 2.0 * E;
            double inv[3];
            int m = 0;                                   // the octant the ray enters first
            for (int k = 0; k < 3; ++k) {
                inv[k] = 1.0 / d[k];
                m = (m << 1) | (d[k] < 0.0 ? 1 : 0);
            }
            LaneStack stack(lds, lane);
            stack.push(oct_id(0, 0), ctr + RC_OVERFLOW);
            while (!stack.empty()) {
                const int node = stack.pop();
                const int l = oct_level(node), lin = oct_lin(node);
                if (!slab_reaches(oct_box(ix, l, lin), o, d, inv, g, fmin(best, t_max))) continue;
                if (l == ix.L) {
                    int t0, t1;
                    oct_leaf_range(ix, lin, &t0, &t1);
                    for (int t = t0; t < t1; ++t) {
                        double p[PREP_DOUBLES];
                        tri_prep(ix.stri + 9 * (long long)t, p);
                        const double th = ray_tri(p, o, d, t_max, E);
                        const int f = ix.sface[t];
                        ++tests;
                        if (th < best || (th == best && th < INFINITY && f < bestf)) {
                            best = th;
                            bestf = f;
                        }
                    }
                } else {
                    int xyz[3];
                    oct_xyz(l, lin, xyz);
                    for (int j = 7; j >= 0; --j) {       // pushed back to front: the child the ray enters first is popped first
                        const int clin = oct_child_lin(l, xyz, j ^ m);
                        if (!slab_reaches(oct_box(ix, l + 1, clin), o, d, inv, g, fmin(best, t_max))) continue;
                        stack.push(oct_id(l + 1, clin), ctr + RC_OVERFLOW);
                    }
                }
            }
        }
        t_out[r] = best;
        face_out[r] = bestf;
    }
    wave_count(ctr + RC_TESTS, tests);
}

// every ray against the faces [y * per, (y + 1) * per): part_t / part_f [gridDim.y][n]
constexpr int RX_TILE = 128;
__global__ __launch_bounds__(256) void p2s_mr_exhaustive_kernel(const double *__restrict__ tri, long long F, long long per, double scale,
                                                                const double *__restrict__ rays, long long n, double t_max,
                                                                double *__restrict__ part_t, int *__restrict__ part_f) {
    __shared__ double tile[RX_TILE * PREP_DOUBLES];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long f0 = (long long)blockIdx.y * per, f1 = min(F, f0 + per);
    double o[3] = {0.0, 0.0, 0.0}, d[3] = {0.0, 0.0, 0.0};
    bool live = false;
    if (i < n) {
        for (int k = 0; k < 3; ++k) {
            o[k] = rays[6 * i + k];
            d[k] = ray_dir(rays[6 * i + 3 + k]);
        }
        live = ray_valid(o, d) && t_max > 0.0;
    }
    const double E = live ? ray_margin(scale, o) : 0.0;
    double best = INFINITY;
    int bestf = -1;
    for (long long b0 = f0; b0 < f1; b0 += RX_TILE) {
        const int lim = (int)min((long long)RX_TILE, f1 - b0);
        if ((int)threadIdx.x < lim) tri_prep(tri + 9 * (b0 + threadIdx.x), tile + PREP_DOUBLES * threadIdx.x);
        __syncthreads();
        if (live) {
            for (int t = 0; t < lim; ++t) {
                const double th = ray_tri(tile + PREP_DOUBLES * t, o, d, t_max, E);
                if (th < best) {                 // ascending face ids: the smallest id keeps a tie
                    best = th;
                    bestf = (int)(b0 + t);
                }
            }
        }
        __syncthreads();
    }
    if (i < n) {
        part_t[(long long)blockIdx.y * n + i] = best;
        part_f[(long long)blockIdx.y * n + i] = bestf;
    }
}

__global__ __launch_bounds__(256) void p2s_mr_merge_kernel(const double *__restrict__ part_t, const int *__restrict__ part_f, int parts,
                                                           long long n, double *__restrict__ t_out, int *__restrict__ face_out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double best = INFINITY;
    int f = -1;
    for (int y = 0; y < parts; ++y) {            // parts in ascending face order
        const double t = part_t[(long long)y * n + i];
        if (t < best) {
            best = t;
            f = part_f[(long long)y * n + i];
        }
    }
    t_out[i] = best;
    face_out[i] = f;
}

// Sensor frame (the project's own: DESIGN 4.8): camera at the origin looking along +y, x right, z up; the object is
// R(q) p + location.  Pixel (i = column, j = row) of a W x H image has the direction
//     normalise(((i + 1/2 - W/2) (2 tan(a_w / 2) / W),  1,  (j + 1/2 - H/2) (2 tan(a_h / 2) / H)))
// and the ray in model space is  o = R^T (-location),  d = R^T dir  (rigid: t is the sensor distance).
// pose [S][12]: R row-major, then o (both from the host, p2s_mesh_tof_scan).  ray = (scan * H + j) * W + i.
__global__ __launch_bounds__(256) void p2s_mr_rays_kernel(const double *__restrict__ pose, long long n, int W, int H, double tan_w, double tan_h,
                                                          double *__restrict__ rays) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int i = (int)(r % W), j = (int)((r / W) % H);
    const double *P = pose + 12 * (r / ((long long)W * H));
    const double sx = (((double)i + 0.5) - 0.5 * (double)W) * ((2.0 * tan_w) / (double)W);
    const double sz = (((double)j + 0.5) - 0.5 * (double)H) * ((2.0 * tan_h) / (double)H);
    const double len = sqrt((sx * sx + 1.0) + sz * sz);
    const double c[3] = {sx / len, 1.0 / len, sz / len};
    for (int k = 0; k < 3; ++k) {
        rays[6 * r + k] = P[9 + k];
        rays[6 * r + 3 + k] = (P[k] * c[0] + P[3 + k] * c[1]) + P[6 + k] * c[2];        // column k of R = row k of R^T
    }
}

// hits of every block of 1024 rays, and of every scan (per_scan rays each)
__global__ __launch_bounds__(1024) void p2s_mr_count_kernel(const int *__restrict__ face, long long n, long long per_scan,
                                                            int *__restrict__ block_count, int *__restrict__ scan_count) {
    __shared__ int ws[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long r = (long long)blockIdx.x * 1024 + tid;
    const bool hit = r < n && face[r] >= 0;
    const unsigned long long mask = __ballot(hit);
    const long long first = r - lane, last = min(first + 63, n - 1);
    if (first < n) {
        if (first / per_scan == last / per_scan) {
            if (lane == 0 && mask) atomicAdd(&scan_count[first / per_scan], __popcll(mask));
        } else if (hit) {
            atomicAdd(&scan_count[r / per_scan], 1);
        }
    }
    if (lane == 0) ws[wave] = __popcll(mask);
    __syncthreads();
    if (tid == 0) {
        int s = 0;
        for (int w = 0; w < 16; ++w) s += ws[w];
        block_count[blockIdx.x] = s;
    }
}

struct CompactArgs {
    const double *rays, *t, *noise, *fn;
    const int *face, *block_start;
    long long n;
    double sigma;
    double *noisy, *clean, *normal;
    int *face_out;
};

// the hits in ray order (scan-major, then rows, then columns): p_clean = o + t d, p_noisy = o + (t + sigma g) d (the
// noise acts along the ray, as the reference's inverse transform of the sensor-space points: make_dataset.py:124-144),
// the hit face and its stored unit normal
__global__ __launch_bounds__(1024) void p2s_mr_compact_kernel(CompactArgs a) {
    __shared__ int ws[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long r = (long long)blockIdx.x * 1024 + tid;
    const int f = r < a.n ? a.face[r] : -1;
    const unsigned long long mask = __ballot(f >= 0);
    if (lane == 0) ws[wave] = __popcll(mask);
    __syncthreads();
    if (f < 0) return;
    long long at = a.block_start[blockIdx.x] + __popcll(mask & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) at += ws[w];
    const double t = a.t[r], tn = t + a.sigma * a.noise[r];
    for (int k = 0; k < 3; ++k) {
        const double o = a.rays[6 * r + k], d = ray_dir(a.rays[6 * r + 3 + k]);
        a.clean[3 * at + k] = o + t * d;
        a.noisy[3 * at + k] = o + tn * d;
        a.normal[3 * at + k] = a.fn[3 * (long long)f + k];
    }
    a.face_out[at] = f;
}

// 05_query_pts (source/sdf.py:288-315): n_far points u - 1/2 of [-0.5, 0.5)^3, then the n_close surface samples moved
// along their face's stored unit normal by (u - 1/2) 2 patch_radius; float64 arithmetic, rounded once to float32
__global__ __launch_bounds__(256) void p2s_mr_query_pts_kernel(const double *__restrict__ fn, const float *__restrict__ samples,
                                                               const int *__restrict__ face, const double *__restrict__ u_off,
                                                               const double *__restrict__ u_far, long long n_close, long long n_far,
                                                               double patch_radius, long long F, float *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n_far) {
        for (int k = 0; k < 3; ++k) out[3 * i + k] = (float)(u_far[3 * i + k] - 0.5);
    } else if (i < n_far + n_close) {
        const long long c = i - n_far;
        const double off = ((u_off[c] - 0.5) * 2.0) * patch_radius;
        const long long f = face[c];
        for (int k = 0; k < 3; ++k)           // a face id out of range moves nothing
            out[3 * i + k] = (float)((double)samples[3 * c + k] + off * (f >= 0 && f < F ? fn[3 * f + k] : 0.0));
    }
}

// what a cast needs besides its rays: the parts of the exhaustive kernel [parts][n] (method 1) and the RayCtr words
struct CastWs {
    double *part_t;
    int *part_f;
    unsigned long long *ctr;
    char *base;                    // (p2s_mesh_raycast: a block of its own)
    size_t bytes;
};
CastWs carve_cast(Carver &c, size_t n, int parts) {
    CastWs w = {};
    w.part_t = c.take<double>(n * parts);
    w.part_f = c.take<int>(n * parts);
    w.ctr = c.take<unsigned long long>(8);
    return w;
}

// launches the cast of n rays (no synchronisation)
void ray_cast_launch(p2s_trimesh_t m, const double *rays, long long n, double t_max, int method, int tile_w, int tile_h, double *t_out,
                     int *face_out, const CastWs &w, int parts, long long per, hipStream_t s) {
    if (method == 0) {
        long long threads = n;
        if (tile_w > 0) threads = (n / ((long long)tile_w * tile_h)) * ((tile_w + 7) / 8) * ((tile_h + 7) / 8) * 64;
        hipLaunchKernelGGL(p2s_mr_index_kernel, dim3(blocks(threads, 64)), dim3(64), 0, s, octree_of(m), rays, n, t_max, tile_w, tile_h, t_out,
                           face_out, w.ctr);
    } else {
        hipLaunchKernelGGL(p2s_mr_exhaustive_kernel, dim3(blocks(n, 256), parts), dim3(256), 0, s, m->tri, m->F, per, m->scale, rays, n, t_max,
                           w.part_t, w.part_f);
        hipLaunchKernelGGL(p2s_mr_merge_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, w.part_t, w.part_f, parts, n, t_out, face_out);
    }
}
const char *const RAY_OVERFLOW = "traversal stack overflow (an index deeper than 7 levels)";

}  // namespace

extern "C" int p2s_mesh_raycast(p2s_trimesh_t m, const double *rays_dev, int64_t n, double t_max, int method, double *t_out_dev,
                                int32_t *face_out_dev, int64_t *tests_host, void *stream) {
    static const char *const who = "p2s_mesh_raycast";
    if (tests_host) *tests_host = 0;
    if (!m || n < 0 || n > (1ll << 30) || (n > 0 && (!rays_dev || !t_out_dev || !face_out_dev)) || (method != 0 && method != 1) ||
        !(t_max == t_max)) {
        p2s_set_error("p2s_mesh_raycast: bad argument");
        return P2S_EINVAL;
    }
    if (n == 0) return P2S_OK;
    P2S_HIP_CHECK(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    int parts = 0;
    long long per = m->F;
    if (method == 1) exhaustive_parts(m->F, n, RX_TILE, &parts, &per);
    PoolScratch pool(m->device, s);
    const CastWs w = pool.carve([&](char *b) {
        Carver c{b};
        return c.done(carve_cast(c, (size_t)n, parts));
    });
    if (!w.base) return dev_oom(who, s);
    DEV_CHECK(who, hipMemsetAsync(w.ctr, 0, MESH_COUNTERS, s));
    ray_cast_launch(m, rays_dev, n, t_max, method, 0, 0, t_out_dev, face_out_dev, w, parts, per, s);
    unsigned long long hc[8] = {};
    const int rc = read_counters(who, w.ctr, hc, RC_OVERFLOW, RAY_OVERFLOW, s);
    if (rc != P2S_OK) return rc;
    if (tests_host) *tests_host = method == 0 ? (int64_t)hc[RC_TESTS] : (int64_t)n * m->F;
    return P2S_OK;
}

namespace {
struct ScanWs {
    double *rays, *t, *pose;       // [n][6], [n], [S][12]
    int *face, *block_count, *block_start, *scan_count;
    CastWs cast;
    char *base;
    size_t bytes;
};
ScanWs carve_scan(char *base, size_t n, size_t n_scans, size_t nb, int parts) {
    Carver c{base};
    ScanWs w;
    w.rays = c.take<double>(n * 6);
    w.t = c.take<double>(n);
    w.face = c.take<int>(n);
    w.pose = c.take<double>(n_scans * 12);
    w.block_count = c.take<int>(nb + 1);
    w.block_start = c.take<int>(nb + 1);
    w.scan_count = c.take<int>(n_scans);
    w.cast = carve_cast(c, n, parts);
    return c.done(w);
}
}  // namespace

extern "C" int p2s_mesh_tof_scan(p2s_trimesh_t m, const double *poses_host, int32_t n_scans, const p2s_tof_sensor *sensor, double sigma,
                                 const double *noise_dev, int method, double *noisy_out_dev, double *clean_out_dev, int32_t *face_out_dev,
                                 double *normal_out_dev, int32_t *hits_per_scan_host, int64_t *n_hits_host, int64_t *tests_host, void *stream) {
    static const char *const who = "p2s_mesh_tof_scan";
    if (n_hits_host) *n_hits_host = 0;
    if (tests_host) *tests_host = 0;
    if (!m || n_scans < 0 || n_scans > 4096 || !sensor || !n_hits_host || (method != 0 && method != 1) || !(sigma >= 0.0) ||
        (n_scans > 0 && (!poses_host || !hits_per_scan_host))) {
        p2s_set_error("p2s_mesh_tof_scan: bad argument");
        return P2S_EINVAL;
    }
    const int W = sensor->width, H = sensor->height;
    if (W < 1 || H < 1 || W > 4096 || H > 4096 || !(sensor->tan_half_w > 0.0) || !(sensor->tan_half_h > 0.0) || !(sensor->max_distance > 0.0) ||
        !(sensor->tan_half_w <= 1.0e6) || !(sensor->tan_half_h <= 1.0e6)) {
        p2s_set_error("p2s_mesh_tof_scan: bad sensor (1 <= width, height <= 4096, 0 < tangents <= 1e6, max_distance > 0)");
        return P2S_EINVAL;
    }
    const long long per_scan = (long long)W * H, n = per_scan * n_scans;
    if (n > (1ll << 30) || (n > 0 && (!noise_dev || !noisy_out_dev || !clean_out_dev || !face_out_dev || !normal_out_dev))) {
        p2s_set_error("p2s_mesh_tof_scan: bad argument (at most 2^30 rays; the outputs hold one entry per ray)");
        return P2S_EINVAL;
    }
    if (n == 0) return P2S_OK;
    // R(q) of a unit quaternion (w, x, y, z) and o = R^T (-location): host float64, contraction off, in this association
    std::vector<double> pose((size_t)n_scans * 12);
    for (int sc = 0; sc < n_scans; ++sc) {
        const double *p = poses_host + 7 * sc, *l = p, w = p[3], x = p[4], y = p[5], z = p[6];
        for (int k = 0; k < 7; ++k)
            if (!(std::fabs(p[k]) <= 1.0e300)) {
                p2s_set_error("p2s_mesh_tof_scan: pose %d is not finite", sc);
                return P2S_EINVAL;
            }
        const double qq = ((w * w + x * x) + y * y) + z * z;
        if (!(std::fabs(qq - 1.0) <= 1.7763568394002505e-15)) {      // 2^-49: |q| = 1 to a few ulp
            p2s_set_error("p2s_mesh_tof_scan: the quaternion of pose %d is not a unit quaternion (|q|^2 = %.17g)", sc, qq);
            return P2S_EINVAL;
        }
        double *R = pose.data() + 12 * sc;
        R[0] = 1.0 - 2.0 * (y * y + z * z);
        R[1] = 2.0 * (x * y - w * z);
        R[2] = 2.0 * (x * z + w * y);
        R[3] = 2.0 * (x * y + w * z);
        R[4] = 1.0 - 2.0 * (x * x + z * z);
        R[5] = 2.0 * (y * z - w * x);
        R[6] = 2.0 * (x * z - w * y);
        R[7] = 2.0 * (y * z + w * x);
        R[8] = 1.0 - 2.0 * (x * x + y * y);
        for (int k = 0; k < 3; ++k) R[9 + k] = (R[k] * -l[0] + R[3 + k] * -l[1]) + R[6 + k] * -l[2];
    }
    P2S_HIP_CHECK(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    int parts = 0;
    long long per = m->F;
    if (method == 1) exhaustive_parts(m->F, n, RX_TILE, &parts, &per);
    const long long nb = (n + 1023) / 1024;
    PoolScratch pool(m->device, s);
    const ScanWs w = pool.carve([&](char *b) { return carve_scan(b, (size_t)n, (size_t)n_scans, (size_t)nb, parts); });
    if (!w.base) return dev_oom(who, s);
    DEV_CHECK(who, hipMemcpyAsync(w.pose, pose.data(), pose.size() * 8, hipMemcpyHostToDevice, s));
    DEV_CHECK(who, hipMemsetAsync(w.cast.ctr, 0, MESH_COUNTERS, s));
    DEV_CHECK(who, hipMemsetAsync(w.scan_count, 0, (size_t)n_scans * 4, s));
    hipLaunchKernelGGL(p2s_mr_rays_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, w.pose, n, W, H, sensor->tan_half_w, sensor->tan_half_h, w.rays);
    ray_cast_launch(m, w.rays, n, sensor->max_distance, method, W, H, w.t, w.face, w.cast, parts, per, s);
    hipLaunchKernelGGL(p2s_mr_count_kernel, dim3((unsigned)nb), dim3(1024), 0, s, w.face, n, per_scan, w.block_count, w.scan_count);
    hipLaunchKernelGGL(p2s_scan_kernel, dim3(1), dim3(1024), 0, s, w.block_count, nb, w.block_start);
    const CompactArgs a = {w.rays, w.t, noise_dev, m->fn, w.face, w.block_start, n, sigma, noisy_out_dev, clean_out_dev, normal_out_dev,
                           face_out_dev};
    hipLaunchKernelGGL(p2s_mr_compact_kernel, dim3((unsigned)nb), dim3(1024), 0, s, a);
    unsigned long long hc[8] = {};
    int total = 0;
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipMemcpyAsync(&total, w.block_start + nb, 4, hipMemcpyDeviceToHost, s));
    DEV_CHECK(who, hipMemcpyAsync(hits_per_scan_host, w.scan_count, (size_t)n_scans * 4, hipMemcpyDeviceToHost, s));
    const int rc = read_counters(who, w.cast.ctr, hc, RC_OVERFLOW, RAY_OVERFLOW, s);
    if (rc != P2S_OK) return rc;
    *n_hits_host = total;
    if (tests_host) *tests_host = method == 0 ? (int64_t)hc[RC_TESTS] : (int64_t)n * m->F;
    return P2S_OK;
}

extern "C" int p2s_mesh_query_points(p2s_trimesh_t m, const float *samples_dev, const int32_t *face_dev, const double *u_offset_dev,
                                     const double *u_far_dev, int64_t n_close, int64_t n_far, double patch_radius, float *out_dev,
                                     void *stream) {
    if (!m || n_close < 0 || n_far < 0 || n_close + n_far > (1ll << 30) || (n_close > 0 && (!samples_dev || !face_dev || !u_offset_dev)) ||
        (n_far > 0 && !u_far_dev) || (n_close + n_far > 0 && !out_dev) || !(std::fabs(patch_radius) <= 1.0e300)) {
        p2s_set_error("p2s_mesh_query_points: bad argument");
        return P2S_EINVAL;
    }
    if (n_close + n_far == 0) return P2S_OK;
    P2S_HIP_CHECK(hipSetDevice(m->device));
    hipLaunchKernelGGL(p2s_mr_query_pts_kernel, dim3(blocks(n_close + n_far, 256)), dim3(256), 0, (hipStream_t)stream, m->fn, samples_dev,
                       face_dev, u_offset_dev, u_far_dev, (long long)n_close, (long long)n_far, patch_radius, m->F, out_dev);
    P2S_LAUNCH_CHECK("p2s_mr_query_pts_kernel");
    return P2S_OK;
}
