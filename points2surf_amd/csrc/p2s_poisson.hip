// Screened Poisson baseline on the device: an oriented cloud -> indicator-like volume -> mesh, the
// project's own definition of the stage the reference delegates to MeshLab (eval_dataset.py, poisson.mlx).
//
// A cascade of regular grids, level d = 3 .. D with R = 2^d + 1 nodes per axis over one cube around the cloud, trilinear
// (degree 1) elements.  Per level, with W the n x R^3 matrix of trilinear weights:
//     A = s(x)m(x)m + m(x)s(x)m + m(x)m(x)s + lambda W^T W          (m / s: 1-D mass / stiffness, natural ends)
//     b = (g(x)m(x)m) v_x + (m(x)g(x)m) v_y + (m(x)m(x)g) v_z,      v = (a / h^3) W^T (-N)
// solved by CG preconditioned with diag(A), started from the prolongation of the level below.
//
// Determinism: no floating-point atomic anywhere.  W^T is held as rows over the active nodes (node -> its (point, corner)
// entries, in the order of the cell-sorted points: two stable radix sorts), every node sum walks its row in that order,
// every norm and dot product is a two-stage reduction of a shape fixed by the problem size alone.
//
// Kernels
//   ps_validate        bounding box (ordered-integer atomics), non-finite / all-zero checks
//   ps_keys            cell of every point (float64: the model's floor((p - lo) / h), clamped)
//   ps_points          per cell-sorted point: base node, 8 trilinear weights (float64 product, rounded once), -N, the
//                      (node, entry) pairs of W^T, the number of distinct cells
//   ps_splat           v at the active nodes                      ps_rhs    b, 27-point, separable factors per thread
//   ps_diag / ps_diag_screen   diag(A)
//   ps_gather          u = W x        (per point, 8 nodes)
//   ps_stencil         y = (s m m + m s m + m m s) x  from an LDS tile with its halo: x read once, y written once,
//                      the separable 1-D factors applied plane by plane; p . y fused (one partial per workgroup)
//   ps_screen          y += lambda W^T u over the active nodes; its share of p . y
//   ps_cg_init / ps_cg_update / ps_cg_direction   the CG vector updates with |r|^2 and r . z fused; alpha, beta and the
//                      convergence test are formed on the device from the partial sums (every workgroup adds them in the
//                      same order), the host reads one status record every few iterations
//   ps_prolong         trilinear prolongation                      ps_iso    sum of (W chi)_p, float64 weights
//   ps_finish          chi - iso, the border rule                  ps_vertex_map   lo + h v
#include "p2s_internal.h"
#include "p2s_devcall.h"
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

#include "p2s_devprim.inl"          // f2o / o2f

constexpr int PS_MIN_DEPTH = 3, PS_MAX_DEPTH = 9;
// PS_TX / PS_TY / PS_TZ, PS_MAX_PART and PS_CHECK_EVERY are mirrored at the top of tests/test_gpu_poisson.py: change both
constexpr int PS_TX = 8, PS_TY = 8, PS_TZ = 32;                  // stencil tile: axis 0, 1, 2 (axis 2 fastest)
constexpr int PS_LY = PS_TY + 2, PS_LZ = PS_TZ + 2, PS_LX = PS_TX + 2;
constexpr int PS_MAX_PART = 1024;                                // partial sums per reduction
constexpr int PS_CHECK_EVERY = 8;                                // iterations between two reads of the status record

struct PsCoef {                  // the 1-D matrices in float32
    float mo, md_in, md_end;     // mass: off-diagonal h/6, diagonal 2h/3 inside, h/3 at the ends
    float so, sd_in, sd_end;     // stiffness: -1/h, 2/h, 1/h
};
struct PsStatus {                // device record of one level's CG
    double rr, bb;               // |r|^2 after the last iteration made, |b|^2
    int done_iter;               // iteration after which |r| <= tol |b| held, -1: not yet
    int iters;                   // iterations made
};

__device__ __forceinline__ double ps_wave_sum(double v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
// sum over the workgroup (256 threads), the same value in every thread; fixed order
__device__ __forceinline__ double ps_block_sum(double v) {
    __shared__ double red[4];
    v = ps_wave_sum(v);
    __syncthreads();                                 // red may still be read from the call before
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
// sum of `count` partials, by the whole workgroup, the same in every workgroup
__device__ __forceinline__ double ps_sum_partials(const double *__restrict__ part, int count) {
    double v = 0.0;
    for (int i = threadIdx.x; i < count; i += 256) v += part[i];
    return ps_block_sum(v);
}

// ctl: [0..2] min, [3..5] max (ordered ints), [6] bit 0 non-finite point, bit 1 non-finite normal, [7] a normal is not zero
__global__ __launch_bounds__(256) void ps_validate_kernel(const float *__restrict__ pts, const float *__restrict__ nrm, long long n,
                                                          int *__restrict__ ctl) {
    int mn[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, mx[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
    int bad = 0, nz = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        for (int a = 0; a < 3; ++a) {
            const float p = pts[3 * i + a], q = nrm[3 * i + a];
            if (!(fabsf(p) <= 3.4028235e38f)) bad |= 1;
            else {
                mn[a] = min(mn[a], f2o(p));
                mx[a] = max(mx[a], f2o(p));
            }
            if (!(fabsf(q) <= 3.4028235e38f)) bad |= 2;
            else if (q != 0.0f) nz = 1;
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        for (int a = 0; a < 3; ++a) {
            mn[a] = min(mn[a], __shfl_xor(mn[a], d));
            mx[a] = max(mx[a], __shfl_xor(mx[a], d));
        }
        bad |= __shfl_xor(bad, d);
        nz |= __shfl_xor(nz, d);
    }
    if ((threadIdx.x & 63) == 0) {
        for (int a = 0; a < 3; ++a) {
            atomicMin(&ctl[a], mn[a]);
            atomicMax(&ctl[3 + a], mx[a]);
        }
        if (bad) atomicOr(&ctl[6], bad);
        if (nz) atomicOr(&ctl[7], 1);
    }
}

struct PsBox { double lo[3], h; int R; };

__device__ __forceinline__ int ps_cell(double p, double lo, double h, int R, double *t) {
    const double g = (p - lo) / h;
    int c = (int)floor(g);
    c = min(max(c, 0), R - 2);
    *t = g - (double)c;
    return c;
}

__global__ __launch_bounds__(256) void ps_keys_kernel(const float *__restrict__ pts, int n, PsBox bx, unsigned *__restrict__ key,
                                                      int *__restrict__ id) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double t;
    const int cx = ps_cell((double)pts[3 * i], bx.lo[0], bx.h, bx.R, &t);
    const int cy = ps_cell((double)pts[3 * i + 1], bx.lo[1], bx.h, bx.R, &t);
    const int cz = ps_cell((double)pts[3 * i + 2], bx.lo[2], bx.h, bx.R, &t);
    key[i] = ((unsigned)cx * (unsigned)(bx.R - 1) + (unsigned)cy) * (unsigned)(bx.R - 1) + (unsigned)cz;
    id[i] = i;
}

// per cell-sorted point sp (original id sid[sp]): base node, weights of the 8 corners c = 4 cx + 2 cy + cz, -N, the pairs
// (node, 8 sp + c) of W^T; *n_occ counts the distinct cells
__global__ __launch_bounds__(256) void ps_points_kernel(const float *__restrict__ pts, const float *__restrict__ nrm, int n, PsBox bx,
                                                        const unsigned *__restrict__ skey, const int *__restrict__ sid,
                                                        int *__restrict__ pbase, float *__restrict__ pw, float *__restrict__ pn,
                                                        unsigned *__restrict__ ekey, int *__restrict__ eval, int *__restrict__ n_occ) {
    const int sp = blockIdx.x * 256 + threadIdx.x;
    bool head = false;
    if (sp < n) {
        const int i = sid[sp];
        double t[3];
        int c[3];
        for (int a = 0; a < 3; ++a) c[a] = ps_cell((double)pts[3 * i + a], bx.lo[a], bx.h, bx.R, &t[a]);
        const int base = (c[0] * bx.R + c[1]) * bx.R + c[2];
        pbase[sp] = base;
        for (int a = 0; a < 3; ++a) pn[3 * sp + a] = -nrm[3 * i + a];
        for (int k = 0; k < 8; ++k) {
            const int kx = k >> 2, ky = (k >> 1) & 1, kz = k & 1;
            const double w = (kx ? t[0] : 1.0 - t[0]) * (ky ? t[1] : 1.0 - t[1]) * (kz ? t[2] : 1.0 - t[2]);
            pw[8 * sp + k] = (float)w;
            ekey[8 * sp + k] = (unsigned)(base + (kx * bx.R + ky) * bx.R + kz);
            eval[8 * sp + k] = 8 * sp + k;
        }
        head = sp == 0 || skey[sp] != skey[sp - 1];
    }
    const int cnt = __popcll(__ballot(head));
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(n_occ, cnt);
}

// One row of W^T per group of 8 lanes.  f(entry index e) -> term; the group's sum in a fixed order (lane-strided, then a
// butterfly), the same in all 8 lanes.
template <class F> __device__ __forceinline__ double ps_row_sum(int start, int cnt, F f) {
    double acc = 0.0;
    for (int e = (int)(threadIdx.x & 7); e < cnt; e += 8) acc += f(start + e);
    acc += __shfl_xor(acc, 4);
    acc += __shfl_xor(acc, 2);
    acc += __shfl_xor(acc, 1);
    return acc;
}

// v = (a / h^3) W^T (-N) at the active nodes (the grids are zero elsewhere)
__global__ __launch_bounds__(256) void ps_splat_kernel(const int *__restrict__ n_rows, const unsigned *__restrict__ row_node,
                                                       const int *__restrict__ row_start, const int *__restrict__ row_cnt,
                                                       const int *__restrict__ sval, const float *__restrict__ pw, const float *__restrict__ pn,
                                                       double scale, float *__restrict__ vx, float *__restrict__ vy, float *__restrict__ vz) {
    const int r = (blockIdx.x * 256 + threadIdx.x) >> 3;
    const bool live = r < *n_rows;                   // uniform over the 8 lanes of a group
    const int start = live ? row_start[r] : 0, cnt = live ? row_cnt[r] : 0;
    double s[3];
    for (int a = 0; a < 3; ++a)
        s[a] = ps_row_sum(start, cnt, [&](int e) {
            const int v = sval[e];
            return (double)pw[v] * (double)pn[3 * (v >> 3) + a];
        });
    if (live && (threadIdx.x & 7) == 0) {
        const unsigned node = row_node[r];
        vx[node] = (float)(scale * s[0]);
        vy[node] = (float)(scale * s[1]);
        vz[node] = (float)(scale * s[2]);
    }
}

__device__ __forceinline__ float ps_at(const float *__restrict__ v, int R, int i, int j, int k) {
    return (i < 0 || j < 0 || k < 0 || i >= R || j >= R || k >= R) ? 0.0f : v[((long long)i * R + j) * R + k];
}
__device__ __forceinline__ float ps_md(const PsCoef &c, int i, int R) { return (i == 0 || i == R - 1) ? c.md_end : c.md_in; }
__device__ __forceinline__ float ps_sd(const PsCoef &c, int i, int R) { return (i == 0 || i == R - 1) ? c.sd_end : c.sd_in; }
// (g v)_i = v_{i-1} / 2 - v_{i+1} / 2, the end rows with -1/2 / +1/2 on the diagonal
__device__ __forceinline__ float ps_gd(int i, int R) { return i == 0 ? -0.5f : (i == R - 1 ? 0.5f : 0.0f); }

// b = (g m m) vx + (m g m) vy + (m m g) vz: per node, the factor along axis 2 first, then axis 1, then axis 0
__global__ __launch_bounds__(256) void ps_rhs_kernel(const float *__restrict__ vx, const float *__restrict__ vy, const float *__restrict__ vz,
                                                     int R, PsCoef c, float *__restrict__ b) {
    const long long N = (long long)R * R * R;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= N) return;
    const int k = (int)(idx % R), j = (int)((idx / R) % R), i = (int)(idx / ((long long)R * R));
    const float mdx = ps_md(c, i, R), mdy = ps_md(c, j, R), mdz = ps_md(c, k, R);
    const float gdx = ps_gd(i, R), gdy = ps_gd(j, R), gdz = ps_gd(k, R);
    float Tx[3], Ty[3], Tz[3];                       // per plane of axis 0: the axis-1 and axis-2 factors applied
    for (int a = 0; a < 3; ++a) {
        float lx[3], ly[3], lz[3];
        for (int bb = 0; bb < 3; ++bb) {
            const int ii = i - 1 + a, jj = j - 1 + bb;
            lx[bb] = (c.mo * ps_at(vx, R, ii, jj, k - 1) + mdz * ps_at(vx, R, ii, jj, k)) + c.mo * ps_at(vx, R, ii, jj, k + 1);
            ly[bb] = (c.mo * ps_at(vy, R, ii, jj, k - 1) + mdz * ps_at(vy, R, ii, jj, k)) + c.mo * ps_at(vy, R, ii, jj, k + 1);
            lz[bb] = (0.5f * ps_at(vz, R, ii, jj, k - 1) + gdz * ps_at(vz, R, ii, jj, k)) + -0.5f * ps_at(vz, R, ii, jj, k + 1);
        }
        Tx[a] = (c.mo * lx[0] + mdy * lx[1]) + c.mo * lx[2];
        Ty[a] = (0.5f * ly[0] + gdy * ly[1]) + -0.5f * ly[2];
        Tz[a] = (c.mo * lz[0] + mdy * lz[1]) + c.mo * lz[2];
    }
    const float bx = (0.5f * Tx[0] + gdx * Tx[1]) + -0.5f * Tx[2];
    const float by = (c.mo * Ty[0] + mdx * Ty[1]) + c.mo * Ty[2];
    const float bz = (c.mo * Tz[0] + mdx * Tz[1]) + c.mo * Tz[2];
    b[idx] = (bx + by) + bz;
}

__global__ __launch_bounds__(256) void ps_diag_kernel(int R, PsCoef c, float *__restrict__ diag) {
    const long long N = (long long)R * R * R;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= N) return;
    const int k = (int)(idx % R), j = (int)((idx / R) % R), i = (int)(idx / ((long long)R * R));
    const float mdx = ps_md(c, i, R), mdy = ps_md(c, j, R), mdz = ps_md(c, k, R);
    const float sdx = ps_sd(c, i, R), sdy = ps_sd(c, j, R), sdz = ps_sd(c, k, R);
    diag[idx] = ((sdx * mdy) * mdz + (mdx * sdy) * mdz) + (mdx * mdy) * sdz;
}

__global__ __launch_bounds__(256) void ps_diag_screen_kernel(const int *__restrict__ n_rows, const unsigned *__restrict__ row_node,
                                                             const int *__restrict__ row_start, const int *__restrict__ row_cnt,
                                                             const int *__restrict__ sval, const float *__restrict__ pw, double lambda,
                                                             float *__restrict__ diag) {
    const int r = (blockIdx.x * 256 + threadIdx.x) >> 3;
    const bool live = r < *n_rows;
    const double s = ps_row_sum(live ? row_start[r] : 0, live ? row_cnt[r] : 0, [&](int e) {
        const double w = (double)pw[sval[e]];
        return w * w;
    });
    if (live && (threadIdx.x & 7) == 0) {
        const unsigned node = row_node[r];
        diag[node] = (float)((double)diag[node] + lambda * s);
    }
}

// u = W x
__global__ __launch_bounds__(256) void ps_gather_kernel(const PsStatus *__restrict__ st, const float *__restrict__ x, int R, int n,
                                                        const int *__restrict__ pbase, const float *__restrict__ pw, float *__restrict__ u) {
    if (st && st->done_iter >= 0) return;
    const int sp = blockIdx.x * 256 + threadIdx.x;
    if (sp >= n) return;
    const int base = pbase[sp];
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        acc += (double)pw[8 * sp + k] * (double)x[base + (((k >> 2) * R + ((k >> 1) & 1)) * R + (k & 1))];
    u[sp] = (float)acc;
}

// y = (s m m + m s m + m m s) x.  One workgroup walks tiles of PS_TX x PS_TY x PS_TZ nodes (a grid of a fixed size, tiles
// strided over it); per tile x with its halo goes to LDS (nodes beyond the grid: 0), thread (ty, tz) then walks the
// planes of axis 0: per plane the factors along axis 2 and axis 1 (P = m m x, Q = (s m + m s) x), per output
// y = s P + m Q along axis 0 from the last three planes.  part[block] = its share of x . y.
__global__ __launch_bounds__(256) void ps_stencil_kernel(const PsStatus *__restrict__ st, const float *__restrict__ x, int R, PsCoef c,
                                                         int tiles_y, int tiles_z, int n_tiles, float *__restrict__ y,
                                                         double *__restrict__ part) {
    if (st && st->done_iter >= 0) return;
    __shared__ float L[PS_LX][PS_LY][PS_LZ];
    const int tz = threadIdx.x & (PS_TZ - 1), ty = threadIdx.x >> 5;
    double dot = 0.0;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int k0 = (tile % tiles_z) * PS_TZ, j0 = ((tile / tiles_z) % tiles_y) * PS_TY, i0 = (tile / (tiles_z * tiles_y)) * PS_TX;
        __syncthreads();                             // the tile before has been read
        for (int e = threadIdx.x; e < PS_LX * PS_LY * PS_LZ; e += 256) {
            const int a = e / (PS_LY * PS_LZ), rem = e - a * (PS_LY * PS_LZ), bq = rem / PS_LZ, cq = rem - bq * PS_LZ;
            (&L[0][0][0])[e] = ps_at(x, R, i0 - 1 + a, j0 - 1 + bq, k0 - 1 + cq);
        }
        __syncthreads();
        const int j = j0 + ty, k = k0 + tz;
        if (j < R && k < R) {
            const float mdy = ps_md(c, j, R), mdz = ps_md(c, k, R), sdy = ps_sd(c, j, R), sdz = ps_sd(c, k, R);
            float P0 = 0.0f, P1 = 0.0f, Q0 = 0.0f, Q1 = 0.0f;
#pragma unroll
            for (int a = 0; a < PS_LX; ++a) {
                float Mz[3], Sz[3];
#pragma unroll
                for (int bq = 0; bq < 3; ++bq) {
                    const float xm = L[a][ty + bq][tz], x0 = L[a][ty + bq][tz + 1], xp = L[a][ty + bq][tz + 2];
                    Mz[bq] = (c.mo * xm + mdz * x0) + c.mo * xp;
                    Sz[bq] = (c.so * xm + sdz * x0) + c.so * xp;
                }
                const float P2 = (c.mo * Mz[0] + mdy * Mz[1]) + c.mo * Mz[2];
                const float Q2 = ((c.so * Mz[0] + sdy * Mz[1]) + c.so * Mz[2]) + ((c.mo * Sz[0] + mdy * Sz[1]) + c.mo * Sz[2]);
                if (a >= 2) {
                    const int i = i0 + a - 2;        // the output plane: LDS plane a - 1
                    if (i < R) {
                        const float mdx = ps_md(c, i, R), sdx = ps_sd(c, i, R);
                        const float out = ((c.so * P0 + sdx * P1) + c.so * P2) + ((c.mo * Q0 + mdx * Q1) + c.mo * Q2);
                        y[((long long)i * R + j) * R + k] = out;
                        dot += (double)L[a - 1][ty + 1][tz + 1] * (double)out;
                    }
                }
                P0 = P1; P1 = P2; Q0 = Q1; Q1 = Q2;
            }
        }
    }
    const double s = ps_block_sum(dot);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// y += lambda W^T u at the active nodes; part[block] = its share of x . (lambda W^T u)
__global__ __launch_bounds__(256) void ps_screen_kernel(const PsStatus *__restrict__ st, const int *__restrict__ n_rows,
                                                        const unsigned *__restrict__ row_node, const int *__restrict__ row_start,
                                                        const int *__restrict__ row_cnt, const int *__restrict__ sval,
                                                        const float *__restrict__ pw, const float *__restrict__ u, double lambda,
                                                        const float *__restrict__ x, float *__restrict__ y, double *__restrict__ part) {
    if (st && st->done_iter >= 0) return;
    const int rows = *n_rows;
    double dot = 0.0;
    for (int r0 = blockIdx.x * 32; r0 < rows; r0 += gridDim.x * 32) {          // 32 rows per workgroup and pass
        const int r = r0 + (int)(threadIdx.x >> 3);
        const bool live = r < rows;
        const double s = ps_row_sum(live ? row_start[r] : 0, live ? row_cnt[r] : 0, [&](int e) {
            const int v = sval[e];
            return (double)pw[v] * (double)u[v >> 3];
        });
        if (live && (threadIdx.x & 7) == 0) {
            const unsigned node = row_node[r];
            const double t = lambda * s;
            y[node] = (float)((double)y[node] + t);
            dot += (double)x[node] * t;
        }
    }
    const double s = ps_block_sum(dot);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// r = b - y, p = z = r / diag; partials of |r|^2, r . z, |b|^2
__global__ __launch_bounds__(256) void ps_cg_init_kernel(const float *__restrict__ b, const float *__restrict__ y, const float *__restrict__ diag,
                                                         long long N, float *__restrict__ r, float *__restrict__ p,
                                                         double *__restrict__ part_rr, double *__restrict__ part_rz, double *__restrict__ part_bb) {
    double rr = 0.0, rz = 0.0, bb = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long long)gridDim.x * 256) {
        const float bv = b[i], rv = bv - y[i], zv = rv / diag[i];
        r[i] = rv;
        p[i] = zv;
        rr += (double)rv * (double)rv;
        rz += (double)rv * (double)zv;
        bb += (double)bv * (double)bv;
    }
    rr = ps_block_sum(rr);
    rz = ps_block_sum(rz);
    bb = ps_block_sum(bb);
    if (threadIdx.x == 0) {
        part_rr[blockIdx.x] = rr;
        part_rz[blockIdx.x] = rz;
        part_bb[blockIdx.x] = bb;
    }
}

// alpha = (r . z) / (p . A p) from the partial sums; x += alpha p, r -= alpha A p, z = r / diag; partials of |r|^2, r . z
__global__ __launch_bounds__(256) void ps_cg_update_kernel(const PsStatus *__restrict__ st, const double *__restrict__ part_rz_old, int n_vec,
                                                           const double *__restrict__ part_pap_a, int n_a, const double *__restrict__ part_pap_b,
                                                           int n_b, const float *__restrict__ p, const float *__restrict__ ap,
                                                           const float *__restrict__ diag, long long N, float *__restrict__ x,
                                                           float *__restrict__ r, double *__restrict__ part_rr, double *__restrict__ part_rz_new) {
    if (st->done_iter >= 0) return;
    const double rz = ps_sum_partials(part_rz_old, n_vec);
    const double pap = ps_sum_partials(part_pap_a, n_a) + ps_sum_partials(part_pap_b, n_b);
    const float alpha = pap > 0.0 ? (float)(rz / pap) : 0.0f;
    double rr = 0.0, rzn = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long long)gridDim.x * 256) {
        x[i] = x[i] + alpha * p[i];
        const float rv = r[i] - alpha * ap[i];
        r[i] = rv;
        rr += (double)rv * (double)rv;
        rzn += (double)rv * (double)(rv / diag[i]);
    }
    rr = ps_block_sum(rr);
    rzn = ps_block_sum(rzn);
    if (threadIdx.x == 0) {
        part_rr[blockIdx.x] = rr;
        part_rz_new[blockIdx.x] = rzn;
    }
}

// beta = (r . z)_new / (r . z)_old, p = z + beta p; workgroup 0 records |r|^2 and whether iteration `iter` converged
__global__ __launch_bounds__(256) void ps_cg_direction_kernel(PsStatus *__restrict__ st, int iter, double tol2,
                                                              const double *__restrict__ part_rz_old, const double *__restrict__ part_rz_new,
                                                              const double *__restrict__ part_rr, const double *__restrict__ part_bb, int n_vec,
                                                              const float *__restrict__ r, const float *__restrict__ diag, long long N,
                                                              float *__restrict__ p) {
    const int done = st->done_iter;                  // written by workgroup 0 of THIS launch at the earliest with `iter`
    if (done >= 0 && done < iter) return;
    const double rz_old = ps_sum_partials(part_rz_old, n_vec), rz_new = ps_sum_partials(part_rz_new, n_vec);
    const double rr = ps_sum_partials(part_rr, n_vec), bb = ps_sum_partials(part_bb, n_vec);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->rr = rr;
        st->bb = bb;
        st->iters = iter;
        if (rr <= tol2 * bb) st->done_iter = iter;
    }
    if (rr <= tol2 * bb) return;                     // the same decision in every workgroup
    const float beta = rz_old > 0.0 ? (float)(rz_new / rz_old) : 0.0f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long long)gridDim.x * 256)
        p[i] = r[i] / diag[i] + beta * p[i];
}

// trilinear prolongation: every second node of the fine level is a node of the coarse one
__global__ __launch_bounds__(256) void ps_prolong_kernel(const float *__restrict__ xc, int Rc, float *__restrict__ xf, int Rf) {
    const long long N = (long long)Rf * Rf * Rf;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= N) return;
    const int k = (int)(idx % Rf), j = (int)((idx / Rf) % Rf), i = (int)(idx / ((long long)Rf * Rf));
    float acc = 0.0f;
    for (int a = 0; a <= (i & 1); ++a)
        for (int bq = 0; bq <= (j & 1); ++bq)
            for (int cq = 0; cq <= (k & 1); ++cq)
                acc += xc[((long long)((i >> 1) + a) * Rc + ((j >> 1) + bq)) * Rc + ((k >> 1) + cq)];
    const int odd = (i & 1) + (j & 1) + (k & 1);
    xf[idx] = acc * (odd == 0 ? 1.0f : odd == 1 ? 0.5f : odd == 2 ? 0.25f : 0.125f);
}

// partials of sum_p (W chi)_p with float64 weights
__global__ __launch_bounds__(256) void ps_iso_kernel(const float *__restrict__ pts, int n, PsBox bx, const float *__restrict__ chi,
                                                     double *__restrict__ part) {
    double acc = 0.0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        double t[3];
        int c[3];
        for (int a = 0; a < 3; ++a) c[a] = ps_cell((double)pts[3 * i + a], bx.lo[a], bx.h, bx.R, &t[a]);
        const int base = (c[0] * bx.R + c[1]) * bx.R + c[2];
        double v = 0.0;
        for (int k = 0; k < 8; ++k) {
            const int kx = k >> 2, ky = (k >> 1) & 1, kz = k & 1;
            const double w = (kx ? t[0] : 1.0 - t[0]) * (ky ? t[1] : 1.0 - t[1]) * (kz ? t[2] : 1.0 - t[2]);
            v += w * (double)chi[base + (kx * bx.R + ky) * bx.R + kz];
        }
        acc += v;
    }
    acc = ps_block_sum(acc);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// volume = chi - iso; a node on one of the six border faces: -|value|
__global__ __launch_bounds__(256) void ps_finish_kernel(const float *__restrict__ chi, int R, double iso, float *__restrict__ vol) {
    const long long N = (long long)R * R * R;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= N) return;
    const int k = (int)(idx % R), j = (int)((idx / R) % R), i = (int)(idx / ((long long)R * R));
    float v = (float)((double)chi[idx] - iso);
    if (i == 0 || j == 0 || k == 0 || i == R - 1 || j == R - 1 || k == R - 1) v = -fabsf(v);
    vol[idx] = v;
}

__global__ __launch_bounds__(256) void ps_vertex_map_kernel(float *__restrict__ verts, long long n3, PsBox bx) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n3) return;
    verts[i] = (float)(bx.lo[i % 3] + bx.h * (double)verts[i]);
}

// ---- host side
struct PsSetup {                 // what the validation leaves on the host
    double centre[3], side;
};

// the arguments every entry point shares; the box of the cloud
int ps_validate(const char *who, const float *pts, const float *nrm, int64_t n, const p2s_poisson_params_t *prm, int device,
                hipStream_t s, PoolScratch &scr, PsSetup *out) {
    if (!pts || !nrm || !prm || n < 1 || n > (1 << 24)) {
        p2s_set_error("%s: bad argument (n = %lld)", who, (long long)n);
        return P2S_EINVAL;
    }
    if (prm->depth < PS_MIN_DEPTH || prm->depth > PS_MAX_DEPTH || !(prm->point_weight > 0.0) || !std::isfinite(prm->point_weight) ||
        !(prm->scale >= 1.0) || !std::isfinite(prm->scale) || !(prm->cg_tol > 0.0) || !std::isfinite(prm->cg_tol) || prm->max_iters < 1) {
        p2s_set_error("%s: depth %d (3..9), point_weight %g (> 0), scale %g (>= 1), cg_tol %g (> 0), max_iters %d (>= 1)", who,
                      prm->depth, prm->point_weight, prm->scale, prm->cg_tol, prm->max_iters);
        return P2S_EINVAL;
    }
    int *ctl = scr.get<int>(8);
    if (!ctl) return dev_oom(who, s);
    const int init[8] = {0x7fffffff, 0x7fffffff, 0x7fffffff, (int)0x80000000, (int)0x80000000, (int)0x80000000, 0, 0};
    int h[8];
    DEV_CHECK(who, hipMemcpyAsync(ctl, init, sizeof(init), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(ps_validate_kernel, dim3(std::min(blocks(n), 1024u)), dim3(256), 0, s, pts, nrm, (long long)n, ctl);
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipMemcpyAsync(h, ctl, sizeof(h), hipMemcpyDeviceToHost, s));
    DEV_CHECK(who, hipStreamSynchronize(s));
    if (h[6] || !h[7]) {
        p2s_set_error("%s: %s", who, (h[6] & 1) ? "non-finite point" : (h[6] & 2) ? "non-finite normal" : "every normal is zero");
        return P2S_EINVAL;
    }
    double ext = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double lo = (double)o2f(h[a]), hi = (double)o2f(h[3 + a]);
        out->centre[a] = (lo + hi) / 2.0;
        ext = std::max(ext, hi - lo);
    }
    if (!(ext > 0.0) || !std::isfinite(ext)) {
        p2s_set_error("%s: the cloud has no extent", who);
        return P2S_EINVAL;
    }
    out->side = prm->scale * ext;
    return P2S_OK;
}

PsBox ps_box(const PsSetup &su, int d) {
    PsBox b;
    for (int a = 0; a < 3; ++a) b.lo[a] = su.centre[a] - su.side / 2.0;
    b.h = su.side / (double)(1 << d);
    b.R = (1 << d) + 1;
    return b;
}

struct PsLevel {                 // one level's system on the device
    PsBox bx;
    PsCoef c;
    double lambda, area;
    int n_occ, n;
    int *pbase, *sval, *row_start, *row_cnt, *n_rows;
    unsigned *row_node;
    float *pw, *pn, *u;
    int tiles_y, tiles_z, n_tiles, g_stencil, g_screen, g_vec;
};

struct PsWork {                  // buffers sized for the finest level the call makes
    unsigned *key, *skey, *ekey, *sekey, *row_node;
    int *id, *sid, *eval, *sval, *pbase, *row_start, *row_cnt, *counters;       // counters: [0] n_occ, [1] rows
    float *pw, *pn, *u;
    void *tmp;
    size_t tmp_bytes;
    double *part;                // [6][PS_MAX_PART]
    PsStatus *status;
};

int ps_work_alloc(const char *who, PoolScratch &scr, int n, PsWork *w) {
    const size_t e = (size_t)8 * n;
    size_t t1 = 0, t2 = 0, t3 = 0, t4 = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, t1, (unsigned *)nullptr, (unsigned *)nullptr, (int *)nullptr, (int *)nullptr, n, 0, 32, nullptr);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, t2, (unsigned *)nullptr, (unsigned *)nullptr, (int *)nullptr, (int *)nullptr, (int)e, 0, 32, nullptr);
    (void)hipcub::DeviceRunLengthEncode::Encode(nullptr, t3, (unsigned *)nullptr, (unsigned *)nullptr, (int *)nullptr, (int *)nullptr, (int)e, nullptr);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, t4, (int *)nullptr, (int *)nullptr, (int)e, nullptr);
    w->tmp_bytes = std::max(std::max(t1, t2), std::max(t3, t4)) + 256;
    w->key = scr.get<unsigned>(n);
    w->skey = scr.get<unsigned>(n);
    w->id = scr.get<int>(n);
    w->sid = scr.get<int>(n);
    w->ekey = scr.get<unsigned>(e);
    w->sekey = scr.get<unsigned>(e);
    w->eval = scr.get<int>(e);
    w->sval = scr.get<int>(e);
    w->row_node = scr.get<unsigned>(e);
    w->row_start = scr.get<int>(e);
    w->row_cnt = scr.get<int>(e);
    w->pbase = scr.get<int>(n);
    w->pw = scr.get<float>(e);
    w->pn = scr.get<float>((size_t)3 * n);
    w->u = scr.get<float>(n);
    w->counters = scr.get<int>(4);
    w->tmp = scr.get<char>(w->tmp_bytes);
    w->part = scr.get<double>((size_t)6 * PS_MAX_PART);
    w->status = scr.get<PsStatus>(1);
    if (!w->key || !w->skey || !w->id || !w->sid || !w->ekey || !w->sekey || !w->eval || !w->sval || !w->row_node || !w->row_start ||
        !w->row_cnt || !w->pbase || !w->pw || !w->pn || !w->u || !w->counters || !w->tmp || !w->part || !w->status)
        return dev_oom(who, scr.s);
    return P2S_OK;
}

// the cell sort, W^T as rows, n_occ (one 8-byte read-back), lambda
int ps_level_setup(const char *who, const float *pts, const float *nrm, int n, const PsSetup &su, const p2s_poisson_params_t *prm, int d,
                   PsWork &w, hipStream_t s, PsLevel *L) {
    const PsBox bx = ps_box(su, d);
    const int e = 8 * n;
    DEV_CHECK(who, hipMemsetAsync(w.counters, 0, 16, s));
    DEV_CHECK(who, hipMemsetAsync(w.row_cnt, 0, (size_t)e * 4, s));
    hipLaunchKernelGGL(ps_keys_kernel, dim3(blocks(n)), dim3(256), 0, s, pts, n, bx, w.key, w.id);
    size_t tb = w.tmp_bytes;
    DEV_CHECK(who, hipcub::DeviceRadixSort::SortPairs(w.tmp, tb, w.key, w.skey, w.id, w.sid, n, 0, 3 * d, s));
    hipLaunchKernelGGL(ps_points_kernel, dim3(blocks(n)), dim3(256), 0, s, pts, nrm, n, bx, w.skey, w.sid, w.pbase, w.pw, w.pn, w.ekey,
                       w.eval, w.counters);
    tb = w.tmp_bytes;
    DEV_CHECK(who, hipcub::DeviceRadixSort::SortPairs(w.tmp, tb, w.ekey, w.sekey, w.eval, w.sval, e, 0, 3 * d + 3, s));
    tb = w.tmp_bytes;
    DEV_CHECK(who, hipcub::DeviceRunLengthEncode::Encode(w.tmp, tb, w.sekey, w.row_node, w.row_cnt, w.counters + 1, e, s));
    tb = w.tmp_bytes;
    DEV_CHECK(who, hipcub::DeviceScan::ExclusiveSum(w.tmp, tb, w.row_cnt, w.row_start, e, s));
    int host[2] = {0, 0};
    DEV_CHECK(who, hipGetLastError());
    DEV_CHECK(who, hipMemcpyAsync(host, w.counters, 8, hipMemcpyDeviceToHost, s));
    DEV_CHECK(who, hipStreamSynchronize(s));
    L->bx = bx;
    L->n = n;
    L->n_occ = host[0];
    const double h = bx.h;
    L->area = (double)host[0] * h * h / (double)n;
    L->lambda = prm->point_weight * L->area / h;
    L->c = PsCoef{(float)(h / 6.0), (float)(2.0 * h / 3.0), (float)(h / 3.0), (float)(-1.0 / h), (float)(2.0 / h), (float)(1.0 / h)};
    L->pbase = w.pbase;
    L->sval = w.sval;
    L->row_start = w.row_start;
    L->row_cnt = w.row_cnt;
    L->n_rows = w.counters + 1;
    L->row_node = w.row_node;
    L->pw = w.pw;
    L->pn = w.pn;
    L->u = w.u;
    L->tiles_y = (bx.R + PS_TY - 1) / PS_TY;
    L->tiles_z = (bx.R + PS_TZ - 1) / PS_TZ;
    L->n_tiles = ((bx.R + PS_TX - 1) / PS_TX) * L->tiles_y * L->tiles_z;
    L->g_stencil = std::min(L->n_tiles, PS_MAX_PART);
    L->g_screen = (int)std::min(blocks(e, 256), (unsigned)PS_MAX_PART);      // 32 rows per workgroup and pass, at most 8 n rows
    L->g_vec = (int)std::min(blocks((long long)bx.R * bx.R * bx.R, 1024), (unsigned)PS_MAX_PART);
    return P2S_OK;
}

unsigned ps_row_blocks(const PsLevel &L) { return blocks((long long)8 * L.n * 8, 256); }       // 8 lanes per row, at most 8 n rows

// b and diag(A); vx, vy, vz: three grids of scratch
int ps_level_system(const char *who, const PsLevel &L, float *vx, float *vy, float *vz, float *b, float *diag, hipStream_t s) {
    const long long N = (long long)L.bx.R * L.bx.R * L.bx.R;
    const double h = L.bx.h;
    DEV_CHECK(who, hipMemsetAsync(vx, 0, (size_t)N * 4, s));
    DEV_CHECK(who, hipMemsetAsync(vy, 0, (size_t)N * 4, s));
    DEV_CHECK(who, hipMemsetAsync(vz, 0, (size_t)N * 4, s));
    hipLaunchKernelGGL(ps_splat_kernel, dim3(ps_row_blocks(L)), dim3(256), 0, s, L.n_rows, L.row_node, L.row_start, L.row_cnt, L.sval, L.pw,
                       L.pn, L.area / (h * h * h), vx, vy, vz);
    hipLaunchKernelGGL(ps_rhs_kernel, dim3(blocks(N)), dim3(256), 0, s, vx, vy, vz, L.bx.R, L.c, b);
    hipLaunchKernelGGL(ps_diag_kernel, dim3(blocks(N)), dim3(256), 0, s, L.bx.R, L.c, diag);
    hipLaunchKernelGGL(ps_diag_screen_kernel, dim3(ps_row_blocks(L)), dim3(256), 0, s, L.n_rows, L.row_node, L.row_start, L.row_cnt, L.sval,
                       L.pw, L.lambda, diag);
    DEV_CHECK(who, hipGetLastError());
    return P2S_OK;
}

// y = A x; part_a [g_stencil], part_b [g_screen]: the shares of x . y; st: skip when the level has converged (may be NULL)
int ps_apply(const char *who, const PsLevel &L, const PsStatus *st, const float *x, float *y, double *part_a, double *part_b, hipStream_t s) {
    hipLaunchKernelGGL(ps_gather_kernel, dim3(blocks(L.n)), dim3(256), 0, s, st, x, L.bx.R, L.n, L.pbase, L.pw, L.u);
    hipLaunchKernelGGL(ps_stencil_kernel, dim3(L.g_stencil), dim3(256), 0, s, st, x, L.bx.R, L.c, L.tiles_y, L.tiles_z, L.n_tiles, y, part_a);
    hipLaunchKernelGGL(ps_screen_kernel, dim3(L.g_screen), dim3(256), 0, s, st, L.n_rows, L.row_node, L.row_start, L.row_cnt, L.sval, L.pw,
                       L.u, L.lambda, x, y, part_b);
    DEV_CHECK(who, hipGetLastError());
    return P2S_OK;
}

}  // namespace

extern "C" int p2s_poisson_system(const float *points_dev, const float *normals_dev, int64_t n, const p2s_poisson_params_t *params,
                                  int level, const float *x_in_dev, float *b_out_dev, float *ax_out_dev, float *diag_out_dev,
                                  double *info_host, int device, void *stream) {
    const char *who = "p2s_poisson_system";
    if (!params || level < PS_MIN_DEPTH || level > params->depth || (ax_out_dev && !x_in_dev)) {
        p2s_set_error("%s: bad argument (level %d)", who, level);
        return P2S_EINVAL;
    }
    if (int rc = select_device(who, device, "no HIP device")) return rc;
    hipStream_t s = (hipStream_t)stream;
    PoolScratch scr(device, s);
    PsSetup su;
    if (int rc = ps_validate(who, points_dev, normals_dev, n, params, device, s, scr, &su)) return rc;
    PsWork w;
    if (int rc = ps_work_alloc(who, scr, (int)n, &w)) return rc;
    PsLevel L;
    if (int rc = ps_level_setup(who, points_dev, normals_dev, (int)n, su, params, level, w, s, &L)) return rc;
    const size_t N = (size_t)L.bx.R * L.bx.R * L.bx.R;
    float *vx = scr.get<float>(N), *vy = scr.get<float>(N), *vz = scr.get<float>(N), *b = scr.get<float>(N), *diag = scr.get<float>(N);
    if (!vx || !vy || !vz || !b || !diag) return dev_oom(who, s);
    if (int rc = ps_level_system(who, L, vx, vy, vz, b, diag, s)) return rc;
    if (b_out_dev) DEV_CHECK(who, hipMemcpyAsync(b_out_dev, b, N * 4, hipMemcpyDeviceToDevice, s));
    if (diag_out_dev) DEV_CHECK(who, hipMemcpyAsync(diag_out_dev, diag, N * 4, hipMemcpyDeviceToDevice, s));
    if (ax_out_dev)
        if (int rc = ps_apply(who, L, nullptr, x_in_dev, ax_out_dev, w.part, w.part + PS_MAX_PART, s)) return rc;
    DEV_CHECK(who, hipStreamSynchronize(s));
    if (info_host) {
        for (int k = 0; k < P2S_POISSON_INFO; ++k) info_host[k] = 0.0;
        for (int a = 0; a < 3; ++a) info_host[a] = L.bx.lo[a];
        info_host[3] = L.bx.h;
        info_host[5] = 1.0;
        double *lv = info_host + 8 + 5 * (level - PS_MIN_DEPTH);
        lv[0] = L.lambda;
        lv[1] = (double)L.n_occ;
    }
    return P2S_OK;
}

extern "C" int p2s_poisson_reconstruct(const float *points_dev, const float *normals_dev, int64_t n, const p2s_poisson_params_t *params,
                                       float *vol_out_dev, float *verts_out_dev, int64_t cap_verts, int32_t *faces_out_dev,
                                       int64_t cap_faces, int64_t *n_verts, int64_t *n_faces, double *info_host, int device, void *stream) {
    const char *who = "p2s_poisson_reconstruct";
    if (!n_verts || !n_faces || cap_verts < 0 || cap_faces < 0 || (cap_verts > 0 && !verts_out_dev) || (cap_faces > 0 && !faces_out_dev)) {
        p2s_set_error("%s: bad argument", who);
        return P2S_EINVAL;
    }
    if (int rc = select_device(who, device, "no HIP device")) return rc;
    hipStream_t s = (hipStream_t)stream;
    double info[P2S_POISSON_INFO] = {};
    int rc_mc = P2S_OK;
    PsBox fine;
    {
        PoolScratch scr(device, s);
        PsSetup su;
        if (int rc = ps_validate(who, points_dev, normals_dev, n, params, device, s, scr, &su)) return rc;
        const int D = params->depth;
        PsWork w;
        if (int rc = ps_work_alloc(who, scr, (int)n, &w)) return rc;
        fine = ps_box(su, D);
        const size_t NF = (size_t)fine.R * fine.R * fine.R, NC = (size_t)((fine.R + 1) / 2) * ((fine.R + 1) / 2) * ((fine.R + 1) / 2);
        float *x = scr.get<float>(NF), *xc = scr.get<float>(NC), *b = scr.get<float>(NF), *diag = scr.get<float>(NF), *r = scr.get<float>(NF),
              *p = scr.get<float>(NF), *ap = scr.get<float>(NF);
        float *vol = vol_out_dev ? vol_out_dev : nullptr;
        if (!vol) vol = scr.get<float>(NF);
        if (!x || !xc || !b || !diag || !r || !p || !ap || !vol) return dev_oom(who, s);
        DevEvent ev[2];
        if (!ev[0].create() || !ev[1].create()) {
            p2s_set_error("%s: hipEventCreate failed", who);
            return P2S_EHIP;
        }
        double *part_pa = w.part, *part_pb = w.part + PS_MAX_PART, *part_rr = w.part + 2 * PS_MAX_PART, *part_bb = w.part + 3 * PS_MAX_PART;
        double *part_rz[2] = {w.part + 4 * PS_MAX_PART, w.part + 5 * PS_MAX_PART};
        const double tol2 = params->cg_tol * params->cg_tol;
        for (int d = PS_MIN_DEPTH; d <= D; ++d) {
            DEV_CHECK(who, hipEventRecord(ev[0].get(), s));
            PsLevel L;
            if (int rc = ps_level_setup(who, points_dev, normals_dev, (int)n, su, params, d, w, s, &L)) return rc;
            const long long N = (long long)L.bx.R * L.bx.R * L.bx.R;
            if (int rc = ps_level_system(who, L, r, p, ap, b, diag, s)) return rc;          // r, p, ap: the grids of v until the CG starts
            if (d == PS_MIN_DEPTH) {
                DEV_CHECK(who, hipMemsetAsync(x, 0, (size_t)N * 4, s));
            } else {
                DEV_CHECK(who, hipMemcpyAsync(xc, x, (size_t)((L.bx.R + 1) / 2) * ((L.bx.R + 1) / 2) * ((L.bx.R + 1) / 2) * 4, hipMemcpyDeviceToDevice, s));
                hipLaunchKernelGGL(ps_prolong_kernel, dim3(blocks(N)), dim3(256), 0, s, xc, (L.bx.R + 1) / 2, x, L.bx.R);
            }
            const PsStatus st0 = {0.0, 0.0, -1, 0};
            DEV_CHECK(who, hipMemcpyAsync(w.status, &st0, sizeof(st0), hipMemcpyHostToDevice, s));
            if (int rc = ps_apply(who, L, nullptr, x, ap, part_pa, part_pb, s)) return rc;
            hipLaunchKernelGGL(ps_cg_init_kernel, dim3(L.g_vec), dim3(256), 0, s, b, ap, diag, N, r, p, part_rr, part_rz[0], part_bb);
            PsStatus st = st0;
            int it = 0;
            while (it < params->max_iters && st.done_iter < 0) {
                const int stop = std::min(it + PS_CHECK_EVERY, params->max_iters);
                for (; it < stop; ++it) {
                    double *rz_old = part_rz[it & 1], *rz_new = part_rz[(it + 1) & 1];
                    if (int rc = ps_apply(who, L, w.status, p, ap, part_pa, part_pb, s)) return rc;
                    hipLaunchKernelGGL(ps_cg_update_kernel, dim3(L.g_vec), dim3(256), 0, s, w.status, rz_old, L.g_vec, part_pa, L.g_stencil,
                                       part_pb, L.g_screen, p, ap, diag, N, x, r, part_rr, rz_new);
                    hipLaunchKernelGGL(ps_cg_direction_kernel, dim3(L.g_vec), dim3(256), 0, s, w.status, it + 1, tol2, rz_old, rz_new, part_rr,
                                       part_bb, L.g_vec, r, diag, N, p);
                }
                DEV_CHECK(who, hipGetLastError());
                DEV_CHECK(who, hipMemcpyAsync(&st, w.status, sizeof(st), hipMemcpyDeviceToHost, s));
                DEV_CHECK(who, hipStreamSynchronize(s));
            }
            DEV_CHECK(who, hipEventRecord(ev[1].get(), s));
            DEV_CHECK(who, hipEventSynchronize(ev[1].get()));
            float ms = 0.0f;
            DEV_CHECK(who, hipEventElapsedTime(&ms, ev[0].get(), ev[1].get()));
            double *lv = info + 8 + 5 * (d - PS_MIN_DEPTH);
            lv[0] = L.lambda;
            lv[1] = (double)L.n_occ;
            lv[2] = (double)st.iters;
            lv[3] = st.bb > 0.0 ? std::sqrt(st.rr / st.bb) : 0.0;
            lv[4] = (double)ms;
        }
        // iso = the mean of chi at the points; the volume with its border rule
        const int g_iso = (int)std::min(blocks(n), (unsigned)PS_MAX_PART);
        hipLaunchKernelGGL(ps_iso_kernel, dim3(g_iso), dim3(256), 0, s, points_dev, (int)n, fine, x, part_pa);
        std::vector<double> hp(g_iso);
        DEV_CHECK(who, hipGetLastError());
        DEV_CHECK(who, hipMemcpyAsync(hp.data(), part_pa, (size_t)g_iso * 8, hipMemcpyDeviceToHost, s));
        DEV_CHECK(who, hipStreamSynchronize(s));
        double sum = 0.0;
        for (double v : hp) sum += v;
        const double iso = sum / (double)n;
        hipLaunchKernelGGL(ps_finish_kernel, dim3(blocks((long long)NF)), dim3(256), 0, s, x, fine.R, iso, vol);
        DEV_CHECK(who, hipGetLastError());
        for (int a = 0; a < 3; ++a) info[a] = fine.lo[a];
        info[3] = fine.h;
        info[4] = iso;
        info[5] = (double)(D - PS_MIN_DEPTH + 1);
        if (info_host) memcpy(info_host, info, sizeof(info));
        // the iso-surface at 0 (inside: value > 0), array-index coordinates; holds the volume scratch of its own
        rc_mc = p2s_marching_cubes(vol, fine.R, verts_out_dev, cap_verts, faces_out_dev, cap_faces, n_verts, n_faces, 0, 1, nullptr, device, stream);
        if (rc_mc == P2S_OK && *n_verts > 0) {
            hipLaunchKernelGGL(ps_vertex_map_kernel, dim3(blocks(3 * *n_verts)), dim3(256), 0, s, verts_out_dev, (long long)(3 * *n_verts), fine);
            DEV_CHECK(who, hipGetLastError());
            DEV_CHECK(who, hipStreamSynchronize(s));
        }
    }
    return rc_mc;
}
