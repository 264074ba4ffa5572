// a shaded picture of the handle's mesh -- first-hit rays of a pinhole or orthographic camera over ss x ss
// samples per pixel, a two-sided headlight, flat or smooth normals, vertex colours, ambient occlusion from a table of
// directions, 8-bit RGB at gamma 2.  Definition: include/p2s_hip.h (p2s_mesh_render).  Included at the end of
// p2s_meshdist.hip, behind p2s_meshdenoise.inl: the handle, the octree helpers and the LaneStack (p2s_mesh_octree.inl), dot3 /
// cross3 / finite3, wave_count, read_counters, the host scaffold, and of the ray unit ray_tri, tri_prep, ray_dir, ray_valid,
// ray_margin, slab_reaches, ray_of_thread, p2s_mr_index_kernel, carve_cast and ray_cast_launch are those files', used here
// and not copied.
//   p2s_rd_rays_kernel     sample (X, Y) of the (W ss) x (H ss) sample image -> its ray [6], ray = Y (W ss) + X
//   p2s_mr_index_kernel    THE PRIMARY PASS is the ray unit's own first-hit walk over these rays with the sample image as
//                          its tile image (ray_cast_launch, tile_w = W ss, tile_h = H ss): depth and face ARE what
//                          p2s_mesh_raycast returns for the same rays, by construction, and its G-buffer (t, face: 12 bytes
//                          per sample) is what the outputs depth_out / face_out hold anyway
//   p2s_rd_shade_kernel    HOT PATH, one sample per lane, a wave on the 8 x 8 tile of adjacent samples that ray_of_thread
//                          gives (the same mapping as the primary pass): (u, v) of the hit, the normal, the headlight, the
//                          albedo, then K occlusion rays, each an ANY-HIT walk of the octree; the sample's colour [3] float64
//   p2s_rd_resolve_kernel  one pixel per thread: the ss x ss sample colours summed b outer, a inner, / ss^2, gamma 2, bytes
// Occlusion runs from the G-buffer in a launch of its own, not fused into the primary walk: the primary pass is then the
// measured kernel of the ray unit, unchanged, and the occlusion walk's registers (the hit point, the basis, the table loop)
// are not live during it.  The fused placement was not built; profiles/figure/README.md has the times of this one.
// Any-hit walk: a node is skipped only if the ray misses its box grown by 2 E or enters it beyond ao_radius -- the skip
// argument of p2s_mr_index_kernel with the limit ao_radius in place of min(best, t_max): an accepted hit has t <= ao_radius
// and its computed point within E of the face's box, which lies in the box of every node above it, so the computed entry
// into the grown box is <= t <= ao_radius with 26 bits to spare and no node that holds an accepted hit is skipped.  The
// answer is a boolean (is there any accepted hit), so the order of the descent and the early exit change the cost alone.
// The children are pushed front to back all the same: the nearest occluder ends the walk soonest.
// Arithmetic: float64, contraction off, + - * / sqrt fmin fmax floor copysign and comparisons only, dot3 = (x + y) + z: the
// numpy model (tests/figure_model.py) performs the same operations in the same association.  No floating-point atomic.
// LDS: one LaneStack per wave, 13 KiB, as the primary pass: 12 waves per CU by LDS (160 KiB), 3 per SIMD.
// Bounds: a hit face is below F (written by the primary pass from sface), its corners are below V (validated at the build);
// a sample index is below n = W H ss^2 <= 2^28; the colour buffer holds 3 n doubles; the table K <= 64 rows.

namespace {

enum RenderCtr { RD_HITS, RD_AO_RAYS, RD_AO_OCCLUDED, RD_TESTS, RD_OVERFLOW };

struct RenderCam {
    int W, H, ss, projection;
    double eye[3], right[3], up[3], forward[3], ext_w, ext_h;      // ext: tan_half_* (pinhole) or half_* (orthographic)
};

__global__ __launch_bounds__(256) void p2s_rd_rays_kernel(RenderCam c, long long n, double *__restrict__ rays) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int Ws = c.W * c.ss;
    const int X = (int)(r % Ws), Y = (int)(r / Ws);
    const int i = X / c.ss, a = X - i * c.ss, j = Y / c.ss, b = Y - j * c.ss;
    const double sx = (2.0 * ((double)i + ((double)a + 0.5) / (double)c.ss)) / (double)c.W - 1.0;
    const double sy = 1.0 - (2.0 * ((double)j + ((double)b + 0.5) / (double)c.ss)) / (double)c.H;
    const double kx = sx * c.ext_w, ky = sy * c.ext_h;
    for (int k = 0; k < 3; ++k) {
        rays[6 * r + k] = c.projection == 0 ? c.eye[k] : (c.eye[k] + kx * c.right[k]) + ky * c.up[k];
        rays[6 * r + 3 + k] = c.projection == 0 ? (c.forward[k] + kx * c.right[k]) + ky * c.up[k] : c.forward[k];
    }
}

// is any face hit in (0, limit]?  The acceptance is ray_tri's; the walk: the header
__device__ __forceinline__ bool rd_any_hit(const OctreeDev &ix, int *lds, int lane, const double *o, const double *d, double limit,
                                           unsigned long long *overflow, unsigned long long *tests) {
    if (!(ray_valid(o, d) && limit > 0.0)) return false;
    const double E = ray_margin(ix.scale, o), g = 2.0 * E;
    double inv[3];
    int m = 0;
    for (int k = 0; k < 3; ++k) {
        inv[k] = 1.0 / d[k];
        m = (m << 1) | (d[k] < 0.0 ? 1 : 0);
    }
    LaneStack stack(lds, lane);
    stack.push(oct_id(0, 0), overflow);
    while (!stack.empty()) {
        const int node = stack.pop();
        const int l = oct_level(node), lin = oct_lin(node);
        if (l == ix.L) {
            int t0, t1;
            oct_leaf_range(ix, lin, &t0, &t1);
            for (int t = t0; t < t1; ++t) {
                double p[PREP_DOUBLES];
                tri_prep(ix.stri + 9 * (long long)t, p);
                ++*tests;
                if (ray_tri(p, o, d, limit, E) < INFINITY) return true;
            }
        } else {
            int xyz[3];
            oct_xyz(l, lin, xyz);
            for (int j = 7; j >= 0; --j) {
                const int clin = oct_child_lin(l, xyz, j ^ m);
                if (!slab_reaches(oct_box(ix, l + 1, clin), o, d, inv, g, limit)) continue;
                stack.push(oct_id(l + 1, clin), overflow);
            }
        }
    }
    return false;
}

struct ShadeArgs {
    OctreeDev ix;
    const double *tri, *fn;            // the handle's [F][9], [F][3]
    const int *fidx, *vbad;            // [F][3], [V]
    const long long *vn;               // [V][4]
    const double *rays, *t;            // [n][6], [n]
    const int *face;                   // [n]
    const float *vrgb;                 // [V][3] or NULL
    const double *ao;                  // [K][3] or NULL
    long long n;
    int Ws, Hs, K, smooth;
    double ao_radius, ao_bias, ambient, diffuse, base[3], bg[3];
    double *col;                       // [n][3]
    unsigned long long *ctr;
};

__device__ __forceinline__ double rd_clamp01(double x) { return fmin(fmax(x, 0.0), 1.0); }

__global__ __launch_bounds__(64) void p2s_rd_shade_kernel(ShadeArgs a) {
    __shared__ int lds[OCT_STACK * 64];
    const int lane = threadIdx.x;
    const long long r = ray_of_thread((long long)blockIdx.x * 64 + lane, a.n, a.Ws, a.Hs);
    unsigned long long hits = 0, ao_rays = 0, ao_occ = 0, tests = 0;
    if (r >= 0) {
        const int f = a.face[r];
        double col[3];
        if (f < 0) {
            for (int k = 0; k < 3; ++k) col[k] = rd_clamp01(a.bg[k]);
        } else {
            hits = 1;
            double o[3], d[3];
            for (int k = 0; k < 3; ++k) {
                o[k] = a.rays[6 * r + k];
                d[k] = ray_dir(a.rays[6 * r + 3 + k]);
            }
            const double t = a.t[r];
            // (u, v): the expressions of ray_tri on the face as the handle stores it
            const double *P = a.tri + 9 * (long long)f;
            double e1[3], e2[3], nf[3], s[3], q[3];
            for (int k = 0; k < 3; ++k) {
                e1[k] = P[3 + k] - P[k];
                e2[k] = P[6 + k] - P[k];
                s[k] = o[k] - P[k];
            }
            cross3(e1, e2, nf);
            cross3(s, d, q);
            const double dn = dot3(d, nf);
            const double u = -dot3(e2, q) / dn, v = dot3(e1, q) / dn, w0 = (1.0 - u) - v;
            const int vi[3] = {a.fidx[3 * (long long)f], a.fidx[3 * (long long)f + 1], a.fidx[3 * (long long)f + 2]};
            double nrm[3] = {a.fn[3 * (long long)f], a.fn[3 * (long long)f + 1], a.fn[3 * (long long)f + 2]};
            if (a.smooth && !(a.vbad[vi[0]] | a.vbad[vi[1]] | a.vbad[vi[2]])) {
                double m[3];
                for (int k = 0; k < 3; ++k)
                    m[k] = (w0 * ((double)a.vn[4 * (long long)vi[0] + k] / FIX) + u * ((double)a.vn[4 * (long long)vi[1] + k] / FIX)) +
                           v * ((double)a.vn[4 * (long long)vi[2] + k] / FIX);
                const double mm = dot3(m, m);
                if (mm > 0.0 && mm <= 1.0e300) {                     // 0 and NaN keep the face normal
                    const double l = sqrt(mm);
                    for (int k = 0; k < 3; ++k) nrm[k] = m[k] / l;
                }
            }
            const double ld = sqrt(dot3(d, d));
            const double dl[3] = {d[0] / ld, d[1] / ld, d[2] / ld};
            double c = dot3(nrm, dl);
            if (c > 0.0) {
                c = -c;
                for (int k = 0; k < 3; ++k) nrm[k] = -nrm[k];
            }
            const double lambert = -c;
            double alb[3];
            for (int k = 0; k < 3; ++k)
                alb[k] = a.vrgb ? (w0 * (double)a.vrgb[3 * (long long)vi[0] + k] + u * (double)a.vrgb[3 * (long long)vi[1] + k]) +
                                      v * (double)a.vrgb[3 * (long long)vi[2] + k]
                                : a.base[k];
            double ao = 1.0;
            if (a.K > 0) {
                // the branchless basis of Duff, Burgess, Christensen, Hery, Kensler, Liani and Villemin (JCGT 2017)
                const double sg = copysign(1.0, nrm[2]);
                const double ia = -1.0 / (sg + nrm[2]), ib = (nrm[0] * nrm[1]) * ia;
                const double t1[3] = {1.0 + ((sg * nrm[0]) * nrm[0]) * ia, sg * ib, -(sg * nrm[0])};
                const double t2[3] = {ib, sg + (nrm[1] * nrm[1]) * ia, -nrm[1]};
                double po[3];
                for (int k = 0; k < 3; ++k) po[k] = (o[k] + t * d[k]) + a.ao_bias * nrm[k];
                int occ = 0;
                for (int h = 0; h < a.K; ++h) {
                    const double hx = a.ao[3 * h], hy = a.ao[3 * h + 1], hz = a.ao[3 * h + 2];
                    double dir[3];
                    for (int k = 0; k < 3; ++k) dir[k] = ray_dir((hx * t1[k] + hy * t2[k]) + hz * nrm[k]);
                    occ += rd_any_hit(a.ix, lds, lane, po, dir, a.ao_radius, a.ctr + RD_OVERFLOW, &tests) ? 1 : 0;
                }
                ao_rays = (unsigned long long)a.K;
                ao_occ = (unsigned long long)occ;
                ao = (double)(a.K - occ) / (double)a.K;
            }
            const double shade = a.ambient * ao + a.diffuse * lambert;
            for (int k = 0; k < 3; ++k) col[k] = rd_clamp01(alb[k] * shade);
        }
        for (int k = 0; k < 3; ++k) a.col[3 * r + k] = col[k];
    }
    wave_count(a.ctr + RD_HITS, hits);
    wave_count(a.ctr + RD_AO_RAYS, ao_rays);
    wave_count(a.ctr + RD_AO_OCCLUDED, ao_occ);
    wave_count(a.ctr + RD_TESTS, tests);
}

__global__ __launch_bounds__(256) void p2s_rd_resolve_kernel(const double *__restrict__ col, int W, int H, int ss,
                                                             unsigned char *__restrict__ rgb) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long long)W * H) return;
    const int i = (int)(p % W), j = (int)(p / W);
    const long long Ws = (long long)W * ss;
    double sum[3] = {0.0, 0.0, 0.0};
    for (int b = 0; b < ss; ++b)
        for (int a = 0; a < ss; ++a) {
            const long long r = ((long long)j * ss + b) * Ws + ((long long)i * ss + a);
            for (int k = 0; k < 3; ++k) sum[k] = sum[k] + col[3 * r + k];
        }
    for (int k = 0; k < 3; ++k) rgb[3 * p + k] = (unsigned char)floor(255.0 * sqrt(sum[k] / (double)(ss * ss)) + 0.5);
}

struct RenderWs {
    double *rays, *t, *col;
    int *face;
    unsigned long long *ctr;
    CastWs cast;
    char *base;
    size_t bytes;
};
RenderWs carve_render(char *base, size_t n, bool own_t, bool own_face) {
    Carver c{base};
    RenderWs w;
    w.rays = c.take<double>(n * 6);
    w.t = c.take<double>(n, own_t);
    w.col = c.take<double>(n * 3);
    w.face = c.take<int>(n, own_face);
    w.ctr = c.take<unsigned long long>(8);
    w.cast = carve_cast(c, n, 0);
    return c.done(w);
}

inline double host_dot3(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// the refusals that need no device, in the order of include/p2s_hip.h; NULL: none
const char *render_bad(p2s_trimesh_t m, const p2s_render_params *p, const double *ao_dirs, const uint8_t *rgb_out) {
    if (!m) return "the handle is NULL";
    if (!p) return "prm is NULL";
    if (!rgb_out) return "rgb_out_dev is NULL";
    if (p->width < 1 || p->height < 1) return "width or height < 1";
    if (p->samples < 1 || p->samples > 4) return "samples outside 1 .. 4";
    if (p->ao_rays < 0 || p->ao_rays > 64) return "ao_rays outside 0 .. 64";
    if ((p->ao_rays > 0) != (ao_dirs != nullptr)) return "ao_dirs_dev is NULL iff ao_rays is 0";
    if (p->projection < 0 || p->projection > 1) return "projection outside 0 .. 1";
    if (p->shading < 0 || p->shading > 1) return "shading outside 0 .. 1";
    if ((long long)p->width * p->height > (1ll << 28) / (p->samples * p->samples)) return "width * height * samples^2 > 2^28";
    const double *vec[4] = {p->eye, p->right, p->up, p->forward};
    for (int a = 0; a < 4; ++a)
        for (int k = 0; k < 3; ++k)
            if (!(std::fabs(vec[a][k]) <= 1.0e300)) return "a camera vector is not finite";
    const double ext[2] = {p->projection == 0 ? p->tan_half_w : p->half_w, p->projection == 0 ? p->tan_half_h : p->half_h};
    if (!(ext[0] > 0.0 && ext[0] <= 1.0e300 && ext[1] > 0.0 && ext[1] <= 1.0e300))
        return "the extent of the projection (tan_half_* or half_*) is not finite and positive";
    const double par[4] = {p->ao_radius, p->ao_bias, p->ambient, p->diffuse};
    for (int k = 0; k < 4; ++k)
        if (!(std::fabs(par[k]) <= 1.0e300)) return "ao_radius, ao_bias, ambient or diffuse is not finite";
    for (int k = 0; k < 3; ++k)
        if (!(std::fabs(p->base_rgb[k]) <= 1.0e300 && std::fabs(p->background_rgb[k]) <= 1.0e300))
            return "base_rgb or background_rgb is not finite";
    const double tol = 9.094947017729282e-13;                        // 2^-40
    for (int a = 1; a < 4; ++a)
        for (int b = a; b < 4; ++b)
            if (!(std::fabs(host_dot3(vec[a], vec[b]) - (a == b ? 1.0 : 0.0)) <= tol)) return "right, up, forward are not orthonormal to 2^-40";
    if (p->ao_radius < 0.0) return "ao_radius < 0";
    if (p->ao_bias < 0.0) return "ao_bias < 0";
    return nullptr;
}

// a pointer that a kernel will dereference lies in this device's memory
bool render_on_device(const void *p, int device) {
    if (!p) return true;
    hipPointerAttribute_t at;
    const bool ok = hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeDevice && at.device == device;
    (void)hipGetLastError();
    return ok;
}

}  // namespace

extern "C" int p2s_mesh_render(p2s_trimesh_t m, const p2s_render_params *prm, const float *vertex_rgb_dev, const double *ao_dirs_dev,
                               uint8_t *rgb_out_dev, double *depth_out_dev, int32_t *face_out_dev, int64_t *stats_host, void *stream) {
    static const char *const who = "p2s_mesh_render";
    if (const char *bad = render_bad(m, prm, ao_dirs_dev, rgb_out_dev)) {
        p2s_set_error("%s: bad argument (%s)", who, bad);
        return P2S_EINVAL;
    }
    if (int rc = select_device(who, m->device)) return rc;
    const void *ptrs[5] = {vertex_rgb_dev, ao_dirs_dev, rgb_out_dev, depth_out_dev, face_out_dev};
    static const char *const names[5] = {"vertex_rgb_dev", "ao_dirs_dev", "rgb_out_dev", "depth_out_dev", "face_out_dev"};
    for (int k = 0; k < 5; ++k)
        if (!render_on_device(ptrs[k], m->device)) {
            p2s_set_error("%s: bad argument (%s is not memory of device %d)", who, names[k], m->device);
            return P2S_EINVAL;
        }
    hipStream_t s = (hipStream_t)stream;
    const int W = prm->width, H = prm->height, ss = prm->samples, K = prm->ao_rays;
    const long long n = (long long)W * H * ss * ss;
    PoolScratch pool(m->device, s);
    const RenderWs w = pool.carve([&](char *b) { return carve_render(b, (size_t)n, !depth_out_dev, !face_out_dev); });
    if (!w.base) return dev_oom(who, s);
    double *t = depth_out_dev ? depth_out_dev : w.t;
    int *face = face_out_dev ? face_out_dev : w.face;
    DEV_CHECK(who, hipMemsetAsync(w.ctr, 0, MESH_COUNTERS, s));
    DEV_CHECK(who, hipMemsetAsync(w.cast.ctr, 0, MESH_COUNTERS, s));
    RenderCam cam = {};
    cam.W = W, cam.H = H, cam.ss = ss, cam.projection = prm->projection;
    for (int k = 0; k < 3; ++k) {
        cam.eye[k] = prm->eye[k];
        cam.right[k] = prm->right[k];
        cam.up[k] = prm->up[k];
        cam.forward[k] = prm->forward[k];
    }
    cam.ext_w = prm->projection == 0 ? prm->tan_half_w : prm->half_w;
    cam.ext_h = prm->projection == 0 ? prm->tan_half_h : prm->half_h;
    hipLaunchKernelGGL(p2s_rd_rays_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, cam, n, w.rays);
    ray_cast_launch(m, w.rays, n, INFINITY, 0, W * ss, H * ss, t, face, w.cast, 0, m->F, s);
    ShadeArgs a = {};
    a.ix = octree_of(m);
    a.tri = m->tri, a.fn = m->fn, a.fidx = m->fidx, a.vbad = m->vbad, a.vn = m->vn;
    a.rays = w.rays, a.t = t, a.face = face, a.vrgb = vertex_rgb_dev, a.ao = ao_dirs_dev;
    a.n = n, a.Ws = W * ss, a.Hs = H * ss, a.K = K, a.smooth = prm->shading;
    a.ao_radius = prm->ao_radius, a.ao_bias = prm->ao_bias, a.ambient = prm->ambient, a.diffuse = prm->diffuse;
    for (int k = 0; k < 3; ++k) {
        a.base[k] = prm->base_rgb[k];
        a.bg[k] = prm->background_rgb[k];
    }
    a.col = w.col, a.ctr = w.ctr;
    const long long tiles = (long long)((W * ss + 7) / 8) * ((H * ss + 7) / 8);
    hipLaunchKernelGGL(p2s_rd_shade_kernel, dim3((unsigned)tiles), dim3(64), 0, s, a);
    hipLaunchKernelGGL(p2s_rd_resolve_kernel, dim3(blocks((long long)W * H, 256)), dim3(256), 0, s, w.col, W, H, ss, rgb_out_dev);
    unsigned long long hc[8] = {}, hr[8] = {};
    int rc = read_counters(who, w.cast.ctr, hc, RC_OVERFLOW, RAY_OVERFLOW, s);
    if (rc != P2S_OK) return rc;
    if ((rc = read_counters(who, w.ctr, hr, RD_OVERFLOW, RAY_OVERFLOW, s)) != P2S_OK) return rc;
    if (stats_host) {
        const long long st[8] = {n, (long long)hr[RD_HITS], (long long)hr[RD_AO_RAYS], (long long)hr[RD_AO_OCCLUDED],
                                 (long long)(hc[RC_TESTS] + hr[RD_TESTS]), 0, 0, 0};
        for (int k = 0; k < 8; ++k) stats_host[k] = st[k];
    }
    return P2S_OK;
}
