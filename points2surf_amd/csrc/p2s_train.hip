// Training step of p2s_max / p2s_max_no_feat_stn on the device: train-mode forward (batch statistics), the two losses of
// the reference's compute_loss, backward and the SGD update, all fp32.
//
//   reference  source/points_to_surf_model.py:41-69 (STN), :177-234 (PointNetfeat), :296-352 (PointsToSurfModel)
//              source/points_to_surf_train.py:537-563 (compute_loss), source/sdf_nn.py:30-40
//              torch.nn.BatchNorm1d (momentum 0.1, eps 1e-5, unbiased running variance), torch.optim.SGD
//
// Activations are rows: [M = items * points][channels], so a 1x1 Conv1d is the same linear layer as an nn.Linear.  The
// network is ~30 times linear -> batch-norm -> ReLU; it runs on a small set of generic kernels:
//   p2s_train_gemm_kernel     C = A . B with free strides on both operands (fp32 MFMA 32x32x2), bounds-guarded tiles: the
//                             forward Y = X W^T + b, dX = dY W, dW = dY^T X (split over fixed row slabs), and the batched
//                             64x64 feature transform with its two backward products
//   p2s_train_colsum_kernel   per-channel sums over the rows in double, two fixed stages (batch statistics, the two
//                             reductions of the batch-norm backward, bias gradients, the K = 3 weight gradient)
//   element-wise kernels      batch-norm apply (+ReLU) and its backward, max-pool with argmax and its scatter, losses, SGD
// No floating-point atomics: every reduction has a fixed order, equal inputs and equal state give equal bytes.
#include "p2s_common.h"
#include "p2s_devmem.h"
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <vector>

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// generic GEMM, fp32 MFMA
// ---------------------------------------------------------------------------------------------------------------------
struct TGemm {
    const float *A; long long sam, sak, a_z;      // A[m][k] at A[m * sam + k * sak]
    const float *B; long long sbk, sbn, b_z;      // B[k][n] at B[k * sbk + n * sbn]
    float *C; long long ldc, c_z;                 // C[m][n] at C[m * ldc + n]
    const float *bias;                            // [N] added to every row, or null
    int M, N, K;
    int kslab;      // > 0: blockIdx.z is a slab of kslab rows of K (split-K partial products); 0: blockIdx.z is a batch index
    int accum;      // C += instead of C =
};
constexpr int TK = 32;      // k chunk in LDS
constexpr int TS = 65;      // LDS row stride (floats): [k][m] with m contiguous, transposed stores spread over the banks

__device__ __forceinline__ f32x16 tmfma(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// grid (ceil(M/64), ceil(N/64), Z), block 256: wave w owns the 32x32 tile (w & 1, w >> 1) of the 64x64 block tile.
// Every load and store is guarded: M, N and the k range need not be multiples of anything.
__global__ __launch_bounds__(256) void p2s_train_gemm_kernel(TGemm g) {
    __shared__ float As[TK * TS];
    __shared__ float Bs[TK * TS];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int z = blockIdx.z;
    int k0 = 0, k1 = g.K;
    if (g.kslab > 0) {
        k0 = z * g.kslab;
        k1 = min(g.K, k0 + g.kslab);
    }
    const float *__restrict__ A = g.A + (long long)z * g.a_z;
    const float *__restrict__ B = g.B + (long long)z * g.b_z;
    float *__restrict__ C = g.C + (long long)z * g.c_z;
    const int m0 = blockIdx.x * 64, n0 = blockIdx.y * 64;
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
    const bool a_kfast = (g.sak == 1), b_nfast = (g.sbn == 1);

    // four accumulators take the k pairs in turn: no MFMA waits for the one before it, and the rounding error of a long K
    // grows like that of four short sums
    f32x16 acc4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc4[j][i] = 0.f;

    float ra[8], rb[8];
    auto fetch = [&](int kc) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int e = tid + 256 * i;
            int k, m;
            if (a_kfast) { k = e & 31; m = e >> 5; } else { m = e & 63; k = e >> 6; }
            const int gm = m0 + m, gk = kc + k;
            ra[i] = (gm < g.M && gk < k1) ? A[(long long)gm * g.sam + (long long)gk * g.sak] : 0.f;
            int n;
            if (b_nfast) { n = e & 63; k = e >> 6; } else { k = e & 31; n = e >> 5; }
            const int gn = n0 + n;
            rb[i] = (gn < g.N && kc + k < k1) ? B[(long long)(kc + k) * g.sbk + (long long)gn * g.sbn] : 0.f;
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int e = tid + 256 * i;
            int k, m;
            if (a_kfast) { k = e & 31; m = e >> 5; } else { m = e & 63; k = e >> 6; }
            As[k * TS + m] = ra[i];
            int n;
            if (b_nfast) { n = e & 63; k = e >> 6; } else { k = e & 31; n = e >> 5; }
            Bs[k * TS + n] = rb[i];
        }
    };
    if (k0 < k1) fetch(k0);
    for (int kc = k0; kc < k1; kc += TK) {
        __syncthreads();              // every wave is done reading the previous chunk
        commit();
        __syncthreads();
        if (kc + TK < k1) fetch(kc + TK);
        const float *ap = As + (lane >> 5) * TS + wm + (lane & 31);
        const float *bp = Bs + (lane >> 5) * TS + wn + (lane & 31);
#pragma unroll
        for (int kk = 0; kk < TK; kk += 2) acc4[(kk >> 1) & 3] = tmfma(ap[kk * TS], bp[kk * TS], acc4[(kk >> 1) & 3]);
    }
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = (acc4[0][i] + acc4[1][i]) + (acc4[2][i] + acc4[3][i]);
    const int col = n0 + wn + (lane & 31);
    if (col >= g.N) return;
    const float bv = g.bias ? g.bias[col] : 0.f;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int row = m0 + wm + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
        if (row < g.M) {
            float *c = C + (long long)row * g.ldc + col;
            const float v = acc[reg] + bv;
            *c = g.accum ? (*c + v) : v;
        }
    }
}

// out[i] = sum over the slabs, in slab order
__global__ __launch_bounds__(256) void p2s_train_slab_reduce_kernel(const float *__restrict__ part, float *__restrict__ out,
                                                                    long long n, int slabs) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = part[i];
    for (int t = 1; t < slabs; ++t) s += part[(long long)t * n + i];
    out[i] = s;
}

// ---------------------------------------------------------------------------------------------------------------------
// per-channel sums over the rows, in double, two fixed stages
// ---------------------------------------------------------------------------------------------------------------------
enum { CS_STATS = 0, CS_BNBWD = 1, CS_SUM = 2, CS_LIN3 = 3 };
struct ColArgs {
    const float *a;            // STATS: y.  BNBWD: dz.  SUM: the summand.  LIN3: dy
    const float *y, *z;        // BNBWD: pre-batch-norm y, output z (ReLU mask)
    const float *mean, *invstd;
    const float *x3;           // LIN3: the [M][3] input
    double *part;              // [slabs][C][3]
    int M, C, rows_per_slab, mode, relu;
};

// grid (ceil(C/64), slabs), block 256 = 64 channels x 4 row lanes
__global__ __launch_bounds__(256) void p2s_train_colsum_kernel(ColArgs g) {
    __shared__ double sh[3][4][64];
    const int tid = threadIdx.x;
    const int c = blockIdx.x * 64 + (tid & 63);
    const int rl = tid >> 6;
    const int r0 = blockIdx.y * g.rows_per_slab;
    const int r1 = min(g.M, r0 + g.rows_per_slab);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    if (c < g.C) {
        float mean = 0.f, istd = 0.f;
        if (g.mode == CS_BNBWD) { mean = g.mean[c]; istd = g.invstd[c]; }
        for (int m = r0 + rl; m < r1; m += 4) {
            const long long i = (long long)m * g.C + c;
            const float a = g.a[i];
            if (g.mode == CS_STATS) {
                s0 += (double)a;
                s1 += (double)a * (double)a;
            } else if (g.mode == CS_BNBWD) {
                const float d = (g.relu && !(g.z[i] > 0.f)) ? 0.f : a;
                s0 += (double)d;
                s1 += (double)d * (double)((g.y[i] - mean) * istd);
            } else if (g.mode == CS_SUM) {
                s0 += (double)a;
            } else {
                const float *x = g.x3 + (long long)m * 3;
                s0 += (double)a * (double)x[0];
                s1 += (double)a * (double)x[1];
                s2 += (double)a * (double)x[2];
            }
        }
    }
    sh[0][rl][tid & 63] = s0;
    sh[1][rl][tid & 63] = s1;
    sh[2][rl][tid & 63] = s2;
    __syncthreads();
    if (rl == 0 && c < g.C) {
        double *p = g.part + ((long long)blockIdx.y * g.C + c) * 3;
#pragma unroll
        for (int j = 0; j < 3; ++j) p[j] = ((sh[j][0][tid] + sh[j][1][tid]) + sh[j][2][tid]) + sh[j][3][tid];
    }
}

struct ColFinish {
    const double *part;
    int slabs, C, M, mode;
    float *o0, *o1;            // STATS: mean, invstd.  BNBWD: mean(dz), mean(dz xhat).  SUM: sum.  LIN3: dW [C][3]
    float *g0, *g1;            // STATS: pending batch mean / unbiased variance.  BNBWD: d beta, d gamma
};
__global__ __launch_bounds__(256) void p2s_train_colsum_finish_kernel(ColFinish g) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= g.C) return;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int t = 0; t < g.slabs; ++t) {
        const double *p = g.part + ((long long)t * g.C + c) * 3;
        s0 += p[0];
        s1 += p[1];
        s2 += p[2];
    }
    const double M = (double)g.M;
    if (g.mode == CS_STATS) {
        const double mean = s0 / M;
        double var = s1 / M - mean * mean;          // biased
        if (var < 0.0) var = 0.0;
        g.o0[c] = (float)mean;
        g.o1[c] = (float)(1.0 / sqrt(var + 1e-5));
        g.g0[c] = (float)mean;
        g.g1[c] = (float)(var * (M / (M - 1.0)));
    } else if (g.mode == CS_BNBWD) {
        g.o0[c] = (float)(s0 / M);
        g.o1[c] = (float)(s1 / M);
        g.g0[c] = (float)s0;
        g.g1[c] = (float)s1;
    } else if (g.mode == CS_SUM) {
        g.o0[c] = (float)s0;
    } else {
        g.o0[3 * c + 0] = (float)s0;
        g.o0[3 * c + 1] = (float)s1;
        g.o0[3 * c + 2] = (float)s2;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// element-wise kernels
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void p2s_train_bn_apply_kernel(const float *__restrict__ y, float *__restrict__ z,
                                                                 const float *__restrict__ mean, const float *__restrict__ invstd,
                                                                 const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                 long long n, int C, int relu) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C);
    float v = (y[i] - mean[c]) * invstd[c] * gamma[c] + beta[c];
    if (relu) v = (v < 0.f) ? 0.f : v;                  // NaN stays NaN
    z[i] = v;
}

// in place: d (= dL/dz on entry) becomes dL/dy
__global__ __launch_bounds__(256) void p2s_train_bn_bwd_kernel(float *__restrict__ d, const float *__restrict__ y,
                                                               const float *__restrict__ z, const float *__restrict__ mean,
                                                               const float *__restrict__ invstd, const float *__restrict__ gamma,
                                                               const float *__restrict__ m1, const float *__restrict__ m2,
                                                               long long n, int C, int relu) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C);
    const float dz = (relu && !(z[i] > 0.f)) ? 0.f : d[i];
    const float xh = (y[i] - mean[c]) * invstd[c];
    d[i] = gamma[c] * invstd[c] * (dz - m1[c] - xh * m2[c]);
}

// the K = 3 input layers: y[m][n] = b[n] + sum_k x[m][k] w[n][k]
__global__ __launch_bounds__(256) void p2s_train_lin3_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                             const float *__restrict__ b, float *__restrict__ y, long long n, int N) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long m = i / N;
    const int c = (int)(i % N);
    const float *xp = x + m * 3;
    y[i] = fmaf(xp[2], w[3 * c + 2], fmaf(xp[1], w[3 * c + 1], fmaf(xp[0], w[3 * c + 0], b[c])));
}

// sub-sample in model space -> centred at the query point (reference points_to_surf_model.py:303)
__global__ __launch_bounds__(256) void p2s_train_center_kernel(const float *__restrict__ sub, const float *__restrict__ q,
                                                               float *__restrict__ out, long long n, int S) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long b = i / (3LL * S);
    out[i] = sub[i] - q[b * 3 + (i % 3)];
}

// max over the P rows of every item; the LOWEST index wins an exact tie (torch MaxPool1d)
__global__ __launch_bounds__(256) void p2s_train_pool_kernel(const float *__restrict__ z, float *__restrict__ out,
                                                             int *__restrict__ idx, int B, int P, int C) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)B * C) return;
    const int b = (int)(i / C), c = (int)(i % C);
    const float *p = z + (long long)b * P * C + c;
    float best = p[0];
    int bi = 0;
    for (int t = 1; t < P; ++t) {
        const float v = p[(long long)t * C];
        if (v > best) { best = v; bi = t; }
    }
    out[i] = best;
    idx[i] = bi;
}
__global__ __launch_bounds__(256) void p2s_train_pool_bwd_kernel(const float *__restrict__ dout, const int *__restrict__ idx,
                                                                 float *__restrict__ dz, long long n, int P, int C) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C);
    const long long row = i / C;
    const long long b = row / P;
    const int p = (int)(row % P);
    dz[i] = (idx[b * C + c] == p) ? dout[b * C + c] : 0.f;
}

// T = fc3 output + identity (64 x 64 per item)
__global__ __launch_bounds__(256) void p2s_train_add_identity_kernel(const float *__restrict__ t, float *__restrict__ out, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int e = (int)(i % 4096);
    out[i] = t[i] + (((e >> 6) == (e & 63)) ? 1.0f : 0.0f);
}

// the concat and its backward: dst[m][c] = src[m][c] for c < C with separate row strides
__global__ __launch_bounds__(256) void p2s_train_copy_cols_kernel(const float *__restrict__ src, long long lds_,
                                                                  float *__restrict__ dst, long long ldd, long long n, int C) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long m = i / C;
    const int c = (int)(i % C);
    dst[m * ldd + c] = src[m * lds_ + c];
}

// fc4 (K -> 2, no batch-norm): forward, dX, and dW / db with the rows summed in order
__global__ __launch_bounds__(256) void p2s_train_fc4_kernel(const float *__restrict__ h, const float *__restrict__ w,
                                                            const float *__restrict__ b, float *__restrict__ pred, int B, int K) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= B) return;
    float l0 = b[0], l1 = b[1];
    for (int k = 0; k < K; ++k) {
        const float v = h[(long long)m * K + k];
        l0 = fmaf(v, w[k], l0);
        l1 = fmaf(v, w[K + k], l1);
    }
    pred[2 * m + 0] = l0;
    pred[2 * m + 1] = l1;
}
__global__ __launch_bounds__(256) void p2s_train_fc4_bwd_kernel(const float *__restrict__ dpred, const float *__restrict__ h,
                                                                const float *__restrict__ w, float *__restrict__ dh,
                                                                float *__restrict__ dw, float *__restrict__ db, int B, int K) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < (long long)B * K) {
        const int m = (int)(i / K), k = (int)(i % K);
        dh[i] = fmaf(dpred[2 * m + 1], w[K + k], dpred[2 * m] * w[k]);
    }
    if (i < 2LL * K) {
        const int n = (int)(i / K), k = (int)(i % K);
        double s = 0.0;
        for (int m = 0; m < B; ++m) s += (double)dpred[2 * m + n] * (double)h[(long long)m * K + k];
        dw[i] = (float)s;
    } else if (i < 2LL * K + 2) {
        const int n = (int)(i - 2LL * K);
        double s = 0.0;
        for (int m = 0; m < B; ++m) s += (double)dpred[2 * m + n];
        db[n] = (float)s;
    }
}

// both losses and dL/dpred (NULL: the losses alone), one block; the items are summed in a fixed tree.  out[0] = magnitude
// loss, out[1] = sign loss
//   magnitude: mse(tanh|p0|, tanh(|d| / r));  sign: mean BCE-with-logits of p1 against the 0/1 target
__global__ __launch_bounds__(256) void p2s_train_loss_kernel(const float *__restrict__ pred, const float *__restrict__ dist,
                                                             const float *__restrict__ sign01, const float *__restrict__ radius,
                                                             float *__restrict__ dpred, double *__restrict__ out, int B) {
    __shared__ double sh[2][256];
    const int tid = threadIdx.x;
    double lm = 0.0, ls = 0.0;
    const double invB = 1.0 / (double)B;
    for (int i = tid; i < B; i += 256) {
        const double p0 = pred[2 * i], p1 = pred[2 * i + 1];
        const double t = tanh(fabs((double)(dist[i] / radius[i])));
        const double a = tanh(fabs(p0));
        const double d = a - t;
        lm += d * d;
        const double sg = (p0 > 0.0) ? 1.0 : ((p0 < 0.0) ? -1.0 : (p0 == 0.0 ? 0.0 : p0));
        if (dpred) dpred[2 * i] = (float)(2.0 * d * (1.0 - a * a) * sg * invB);
        const double y = sign01[i];
        ls += fmax(p1, 0.0) - p1 * y + log1p(exp(-fabs(p1)));
        const double sig = 1.0 / (1.0 + exp(-p1));
        if (dpred) dpred[2 * i + 1] = (float)((sig - y) * invB);
    }
    sh[0][tid] = lm;
    sh[1][tid] = ls;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            sh[0][tid] += sh[0][tid + s];
            sh[1][tid] += sh[1][tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        out[0] = sh[0][0] * invB;
        out[1] = sh[1][0] * invB;
    }
}

// flag[0] = 1 when a gradient or a loss is not finite (plain stores of the same value: no atomics needed)
__global__ __launch_bounds__(256) void p2s_train_finite_kernel(const float *__restrict__ g, long long n, const double *__restrict__ loss,
                                                               int *__restrict__ flag) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n && !(fabsf(g[i]) <= 3.4028235e38f)) flag[0] = 1;
    if (i < 2 && !(fabs(loss[i]) <= 1.7976931348623157e308)) flag[0] = 1;
}

// running = (1 - 0.1) running + 0.1 batch statistic (the variance already unbiased)
__global__ __launch_bounds__(256) void p2s_train_running_kernel(float *__restrict__ buf, const float *__restrict__ pend, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    buf[i] = 0.1f * pend[i] + 0.9f * buf[i];
}

// torch.optim.SGD(lr, momentum), no dampening / weight decay / Nesterov
__global__ __launch_bounds__(256) void p2s_train_sgd_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ mom,
                                                            long long n, float lr, float mu, int first) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float b = g[i];
    if (mu != 0.f) {
        if (!first) b = mu * mom[i] + b;
        mom[i] = b;
    }
    p[i] = p[i] - lr * b;
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
struct LinP { long long w, b; int K, N; };
struct BnP { long long g, be, rm, rv; int C; };
struct TrunkP { LinP conv1, conv2, conv3, fc1, fc2, fc3; BnP bn1, bn2, bn3, bn4, bn5; };
struct FeatP { TrunkP t; LinP c0a, c0b, c1, c2, c3; BnP b0a, b0b, b1, b2, b3; };
struct NetP { FeatP f[2]; LinP fc1[2]; BnP bn1[2]; LinP fc2, fc3, fc4; BnP bn2, bn3; };

struct Layout {
    long long np = 0, nb = 0;
    LinP lin(int K, int N) { LinP l; l.K = K; l.N = N; l.w = np; np += (long long)N * K; l.b = np; np += N; return l; }
    BnP bn(int C) { BnP b; b.C = C; b.g = np; np += C; b.be = np; np += C; b.rm = nb; nb += C; b.rv = nb; nb += C; return b; }
    // registration order of the reference's constructors = model_spec.state_shapes
    TrunkP trunk(int dim, int n, int n_out) {
        TrunkP t;
        t.conv1 = lin(dim, 64); t.conv2 = lin(64, 128); t.conv3 = lin(128, n);
        t.fc1 = lin(n, n / 2); t.fc2 = lin(n / 2, n / 4); t.fc3 = lin(n / 4, n_out);
        t.bn1 = bn(64); t.bn2 = bn(128); t.bn3 = bn(n); t.bn4 = bn(n / 2); t.bn5 = bn(n / 4);
        return t;
    }
    FeatP feat(int n, bool stn) {
        FeatP f{};
        if (stn) f.t = trunk(64, n, 64 * 64);
        f.c0a = lin(3, 64); f.c0b = lin(64, 64); f.b0a = bn(64); f.b0b = bn(64);
        f.c1 = lin(64, 64); f.c2 = lin(64, 128); f.c3 = lin(128, n);
        f.b1 = bn(64); f.b2 = bn(128); f.b3 = bn(n);
        return f;
    }
    NetP net(int n, bool stn) {
        NetP p{};
        p.f[0] = feat(n, stn); p.f[1] = feat(n, stn);
        p.fc1[0] = lin(n, n / 2); p.fc1[1] = lin(n, n / 2); p.bn1[0] = bn(n / 2); p.bn1[1] = bn(n / 2);
        p.fc2 = lin(n, n / 4); p.fc3 = lin(n / 4, n / 8); p.fc4 = lin(n / 8, 2);
        p.bn2 = bn(n / 4); p.bn3 = bn(n / 8);
        return p;
    }
};

// one linear -> batch-norm (-> ReLU) block with what its backward needs
struct Blk {
    LinP lin; BnP bn; int relu; int M;
    const float *X; float *Y, *Z; float *mean, *invstd, *m1, *m2;
};
struct FeatA {          // activations of one PointNetfeat
    int M, P;
    const float *x3;
    Blk b0a, b0b, t1, t2, t3, t4, t5, b1, b2, b3;
    float *tpool, *tf, *T, *xt, *pool;
    int *tidx, *idx;
    float *dT, *d64, *dpool;
};

enum { FAM_GEMM = 0, FAM_COLSUM, FAM_BN, FAM_POOL, FAM_SMALL, FAM_N };

}  // namespace

struct p2s_trainer_s {
    int device = 0, P = 0, S = 0, stn = 0;
    NetP net{};
    long long np = 0, nb = 0;
    // what the kernels read.  A trainer points them at its own blocks (`own`); the test hooks (DebugCtx) borrow the caller's
    // arrays for params / grads / pend and own only their scratch
    float *params = nullptr, *grads = nullptr, *mom = nullptr, *bufs = nullptr, *pend = nullptr;
    struct Owned {
        DevBuf<float> params, grads, mom, bufs, pend, arena, wpart;
        DevBuf<double> cpart;
    } own;
    int64_t nbt = 0;
    bool have_grads = false, first_step = true;
    // per-batch-size arena
    int B = 0;
    float *arena = nullptr;
    size_t arena_floats = 0;
    FeatA fa[2];
    Blk h1[2], h2, h3;
    float *cat = nullptr, *pred = nullptr, *dpred = nullptr, *G = nullptr, *H = nullptr, *wpart = nullptr, *dfeat[2] = {nullptr, nullptr};
    double *cpart = nullptr, *loss = nullptr;
    int *flag = nullptr;
    long long wpart_floats = 0;
    int profile = 0;
    double fam_ms[FAM_N] = {};
    std::vector<std::pair<int, std::pair<DevEvent, DevEvent>>> events;
    hipStream_t s = nullptr;
};

namespace {

typedef p2s_trainer_s T;

struct Prof {
    T *t; int fam; DevEvent a, b;
    Prof(T *t_, int fam_) : t(t_), fam(fam_) {
        if (!t->profile) return;
        if (!a.create() || !b.create()) { a.reset(); return; }
        (void)hipEventRecord(a.get(), t->s);
    }
    ~Prof() {
        if (!a) return;
        (void)hipEventRecord(b.get(), t->s);
        t->events.emplace_back(fam, std::make_pair(std::move(a), std::move(b)));
    }
};

inline dim3 g1(long long n) { return dim3((unsigned)((n + 255) / 256)); }

int colsum_slabs(int M) { return (int)std::min<long long>(512, ((long long)M + 255) / 256); }
// dW = dY^T X: the rows are split into a number of slabs fixed by M alone
int dw_slabs(int M) { return (int)std::min<long long>(128, ((long long)M + 2047) / 2048); }

int launch_gemm(T *t, const TGemm &g, int Z) {
    if (g.M <= 0 || g.N <= 0) return P2S_OK;
    Prof p(t, FAM_GEMM);
    hipLaunchKernelGGL(p2s_train_gemm_kernel, dim3((g.M + 63) / 64, (g.N + 63) / 64, Z), dim3(256), 0, t->s, g);
    P2S_LAUNCH_CHECK("p2s_train_gemm_kernel");
    return P2S_OK;
}

int colsum(T *t, ColArgs a, ColFinish f) {
    const int slabs = colsum_slabs(a.M);
    a.rows_per_slab = (a.M + slabs - 1) / slabs;
    a.part = t->cpart;
    Prof p(t, FAM_COLSUM);
    hipLaunchKernelGGL(p2s_train_colsum_kernel, dim3((a.C + 63) / 64, slabs), dim3(256), 0, t->s, a);
    P2S_LAUNCH_CHECK("p2s_train_colsum_kernel");
    f.part = t->cpart; f.slabs = slabs; f.C = a.C; f.M = a.M; f.mode = a.mode;
    hipLaunchKernelGGL(p2s_train_colsum_finish_kernel, g1(a.C), dim3(256), 0, t->s, f);
    P2S_LAUNCH_CHECK("p2s_train_colsum_finish_kernel");
    return P2S_OK;
}

#define TRY(e) do { const int _rc = (e); if (_rc != P2S_OK) return _rc; } while (0)

// Y = X W^T + b
int linear_fwd(T *t, const LinP &l, const float *X, float *Y, int M) {
    if (l.K == 3) {
        Prof p(t, FAM_SMALL);
        hipLaunchKernelGGL(p2s_train_lin3_kernel, g1((long long)M * l.N), dim3(256), 0, t->s, X, t->params + l.w, t->params + l.b, Y,
                           (long long)M * l.N, l.N);
        P2S_LAUNCH_CHECK("p2s_train_lin3_kernel");
        return P2S_OK;
    }
    TGemm g{};
    g.A = X; g.sam = l.K; g.sak = 1;
    g.B = t->params + l.w; g.sbk = 1; g.sbn = l.K;
    g.C = Y; g.ldc = l.N; g.bias = t->params + l.b;
    g.M = M; g.N = l.N; g.K = l.K;
    return launch_gemm(t, g, 1);
}

// dW = dY^T X, db = sum dY, dX = dY W (dX may be null)
int linear_bwd(T *t, const LinP &l, const float *X, const float *dY, float *dX, int M, int accum) {
    {
        ColArgs a{}; a.a = dY; a.M = M; a.C = l.N; a.mode = CS_SUM;
        ColFinish f{}; f.o0 = t->grads + l.b;
        TRY(colsum(t, a, f));
    }
    if (l.K == 3) {
        ColArgs a{}; a.a = dY; a.x3 = X; a.M = M; a.C = l.N; a.mode = CS_LIN3;
        ColFinish f{}; f.o0 = t->grads + l.w;
        TRY(colsum(t, a, f));
    } else {
        const int slabs = dw_slabs(M);
        const long long n = (long long)l.N * l.K;
        TGemm g{};
        g.A = dY; g.sam = 1; g.sak = l.N;             // A[n][row] = dY[row][n]
        g.B = X; g.sbk = l.K; g.sbn = 1;              // B[row][k] = X[row][k]
        g.M = l.N; g.N = l.K; g.K = M; g.ldc = l.K;
        if (slabs == 1) {
            g.C = t->grads + l.w;
            TRY(launch_gemm(t, g, 1));
        } else {
            if (n * slabs > t->wpart_floats) { p2s_set_error("trainer: slab scratch too small"); return P2S_EINVAL; }
            g.C = t->wpart; g.c_z = n;
            g.kslab = (((M + slabs - 1) / slabs) + TK - 1) / TK * TK;
            TRY(launch_gemm(t, g, slabs));
            Prof p(t, FAM_GEMM);
            hipLaunchKernelGGL(p2s_train_slab_reduce_kernel, g1(n), dim3(256), 0, t->s, t->wpart, t->grads + l.w, n, slabs);
            P2S_LAUNCH_CHECK("p2s_train_slab_reduce_kernel");
        }
    }
    if (dX) {
        TGemm g{};
        g.A = dY; g.sam = l.N; g.sak = 1;
        g.B = t->params + l.w; g.sbk = l.K; g.sbn = 1;  // B[n][k] = W[n][k]
        g.C = dX; g.ldc = l.K; g.M = M; g.N = l.K; g.K = l.N; g.accum = accum;
        TRY(launch_gemm(t, g, 1));
    }
    return P2S_OK;
}

// batch statistics of b.Y, then Z = batch-norm(Y) (+ReLU)
int bn_fwd(T *t, Blk &b) {
    ColArgs a{}; a.a = b.Y; a.M = b.M; a.C = b.bn.C; a.mode = CS_STATS;
    ColFinish f{}; f.o0 = b.mean; f.o1 = b.invstd; f.g0 = t->pend + b.bn.rm; f.g1 = t->pend + b.bn.rv;
    TRY(colsum(t, a, f));
    Prof p(t, FAM_BN);
    const long long n = (long long)b.M * b.bn.C;
    hipLaunchKernelGGL(p2s_train_bn_apply_kernel, g1(n), dim3(256), 0, t->s, b.Y, b.Z, b.mean, b.invstd, t->params + b.bn.g,
                       t->params + b.bn.be, n, b.bn.C, b.relu);
    P2S_LAUNCH_CHECK("p2s_train_bn_apply_kernel");
    return P2S_OK;
}

int blk_fwd(T *t, Blk &b) {
    TRY(linear_fwd(t, b.lin, b.X, b.Y, b.M));
    return bn_fwd(t, b);
}

// d: dL/dZ on entry, overwritten with dL/dY; d beta and d gamma
int bn_bwd(T *t, Blk &b, float *d) {
    ColArgs a{}; a.a = d; a.y = b.Y; a.z = b.Z; a.mean = b.mean; a.invstd = b.invstd; a.M = b.M; a.C = b.bn.C; a.mode = CS_BNBWD;
    a.relu = b.relu;
    ColFinish f{}; f.o0 = b.m1; f.o1 = b.m2; f.g0 = t->grads + b.bn.be; f.g1 = t->grads + b.bn.g;
    TRY(colsum(t, a, f));
    Prof p(t, FAM_BN);
    const long long n = (long long)b.M * b.bn.C;
    hipLaunchKernelGGL(p2s_train_bn_bwd_kernel, g1(n), dim3(256), 0, t->s, d, b.Y, b.Z, b.mean, b.invstd, t->params + b.bn.g, b.m1,
                       b.m2, n, b.bn.C, b.relu);
    P2S_LAUNCH_CHECK("p2s_train_bn_bwd_kernel");
    return P2S_OK;
}

// d: dL/dZ on entry (overwritten with dL/dY); dX (may be null) receives dL/dX
int blk_bwd(T *t, Blk &b, float *d, float *dX, int accum) {
    TRY(bn_bwd(t, b, d));
    return linear_bwd(t, b.lin, b.X, d, dX, b.M, accum);
}

int pool_fwd(T *t, const float *z, float *out, int *idx, int B, int P, int C) {
    Prof p(t, FAM_POOL);
    hipLaunchKernelGGL(p2s_train_pool_kernel, g1((long long)B * C), dim3(256), 0, t->s, z, out, idx, B, P, C);
    P2S_LAUNCH_CHECK("p2s_train_pool_kernel");
    return P2S_OK;
}
int pool_bwd(T *t, const float *dout, const int *idx, float *dz, int B, int P, int C) {
    Prof p(t, FAM_POOL);
    const long long n = (long long)B * P * C;
    hipLaunchKernelGGL(p2s_train_pool_bwd_kernel, g1(n), dim3(256), 0, t->s, dout, idx, dz, n, P, C);
    P2S_LAUNCH_CHECK("p2s_train_pool_bwd_kernel");
    return P2S_OK;
}
int copy_cols(T *t, const float *src, long long lds_, float *dst, long long ldd, int M, int C) {
    Prof p(t, FAM_SMALL);
    hipLaunchKernelGGL(p2s_train_copy_cols_kernel, g1((long long)M * C), dim3(256), 0, t->s, src, lds_, dst, ldd, (long long)M * C, C);
    P2S_LAUNCH_CHECK("p2s_train_copy_cols_kernel");
    return P2S_OK;
}

// ---- arena ----------------------------------------------------------------------------------------------------------
struct Bump {
    char *base; size_t off = 0;
    explicit Bump(void *b) : base((char *)b) {}
    template <class U> U *get(size_t n) {
        off = (off + 255) & ~(size_t)255;
        U *p = (U *)((uintptr_t)base + off);
        off += n * sizeof(U);
        return p;
    }
};

void plan_blk(Bump &a, Blk &b, const LinP &l, const BnP &bn, int relu, int M, const float *X) {
    b.lin = l; b.bn = bn; b.relu = relu; b.M = M; b.X = X;
    b.Y = a.get<float>((size_t)M * l.N);
    b.Z = a.get<float>((size_t)M * l.N);
    b.mean = a.get<float>(4 * (size_t)l.N);
    b.invstd = b.mean + l.N; b.m1 = b.mean + 2 * l.N; b.m2 = b.mean + 3 * l.N;
}

size_t plan(T *t, void *base, int B, const float *patch) {
    Bump a(base);
    const NetP &n = t->net;
    const int pts[2] = {t->P, t->S};
    float *centred = a.get<float>((size_t)B * t->S * 3);
    long long maxM = B;
    for (int e = 0; e < 2; ++e) {
        FeatA &f = t->fa[e];
        const FeatP &p = n.f[e];
        f.P = pts[e]; f.M = B * pts[e];
        maxM = std::max<long long>(maxM, f.M);
        f.x3 = e == 0 ? patch : centred;
        plan_blk(a, f.b0a, p.c0a, p.b0a, 1, f.M, f.x3);
        plan_blk(a, f.b0b, p.c0b, p.b0b, 1, f.M, f.b0a.Z);
        f.xt = f.b0b.Z;
        if (t->stn) {
            plan_blk(a, f.t1, p.t.conv1, p.t.bn1, 1, f.M, f.b0b.Z);
            plan_blk(a, f.t2, p.t.conv2, p.t.bn2, 1, f.M, f.t1.Z);
            plan_blk(a, f.t3, p.t.conv3, p.t.bn3, 1, f.M, f.t2.Z);
            f.tpool = a.get<float>((size_t)B * 1024);
            f.tidx = a.get<int>((size_t)B * 1024);
            plan_blk(a, f.t4, p.t.fc1, p.t.bn4, 1, B, f.tpool);
            plan_blk(a, f.t5, p.t.fc2, p.t.bn5, 1, B, f.t4.Z);
            f.tf = a.get<float>((size_t)B * 4096);
            f.T = a.get<float>((size_t)B * 4096);
            f.dT = a.get<float>((size_t)B * 4096);
            f.xt = a.get<float>((size_t)f.M * 64);
            f.d64 = a.get<float>((size_t)f.M * 64);
        }
        plan_blk(a, f.b1, p.c1, p.b1, 1, f.M, f.xt);
        plan_blk(a, f.b2, p.c2, p.b2, 1, f.M, f.b1.Z);
        plan_blk(a, f.b3, p.c3, p.b3, 0, f.M, f.b2.Z);
        f.pool = a.get<float>((size_t)B * 1024);
        f.idx = a.get<int>((size_t)B * 1024);
        f.dpool = a.get<float>((size_t)B * 1024);
        plan_blk(a, t->h1[e], n.fc1[e], n.bn1[e], 1, B, f.pool);
    }
    t->cat = a.get<float>((size_t)B * 1024);
    plan_blk(a, t->h2, n.fc2, n.bn2, 1, B, t->cat);
    plan_blk(a, t->h3, n.fc3, n.bn3, 1, B, t->h2.Z);
    t->pred = a.get<float>((size_t)B * 2);
    t->dpred = a.get<float>((size_t)B * 2);
    t->G = a.get<float>((size_t)maxM * 1024);
    t->H = a.get<float>((size_t)maxM * 1024);
    // split-K partials of the largest weight gradient: per layer slabs(M) * N * K
    long long wp = 0;
    for (int e = 0; e < 2; ++e) wp = std::max<long long>(wp, (long long)dw_slabs(B * pts[e]) * 128 * 1024);
    wp = std::max<long long>(wp, (long long)dw_slabs(B) * 4096 * 256);
    t->wpart_floats = wp;
    t->wpart = a.get<float>((size_t)wp);
    t->cpart = a.get<double>((size_t)512 * 4096 * 3);
    t->loss = a.get<double>(2);
    t->flag = a.get<int>(1);
    (void)centred;
    return a.off + 256;
}

int feat_fwd(T *t, FeatA &f, int B) {
    TRY(blk_fwd(t, f.b0a));
    TRY(blk_fwd(t, f.b0b));
    if (t->stn) {
        TRY(blk_fwd(t, f.t1));
        TRY(blk_fwd(t, f.t2));
        TRY(blk_fwd(t, f.t3));
        TRY(pool_fwd(t, f.t3.Z, f.tpool, f.tidx, B, f.P, 1024));
        TRY(blk_fwd(t, f.t4));
        TRY(blk_fwd(t, f.t5));
        const LinP &fc3 = (&f == &t->fa[0] ? t->net.f[0] : t->net.f[1]).t.fc3;
        TRY(linear_fwd(t, fc3, f.t5.Z, f.tf, B));
        {
            Prof p(t, FAM_SMALL);
            hipLaunchKernelGGL(p2s_train_add_identity_kernel, g1((long long)B * 4096), dim3(256), 0, t->s, f.tf, f.T, (long long)B * 4096);
            P2S_LAUNCH_CHECK("p2s_train_add_identity_kernel");
        }
        // y[b] = T[b] . x[b] (channels x points) = rows: xt[p][i] = sum_j x[p][j] T[i][j]
        TGemm g{};
        g.A = f.b0b.Z; g.sam = 64; g.sak = 1; g.a_z = (long long)f.P * 64;
        g.B = f.T; g.sbk = 1; g.sbn = 64; g.b_z = 4096;
        g.C = f.xt; g.ldc = 64; g.c_z = (long long)f.P * 64;
        g.M = f.P; g.N = 64; g.K = 64;
        TRY(launch_gemm(t, g, B));
    }
    TRY(blk_fwd(t, f.b1));
    TRY(blk_fwd(t, f.b2));
    TRY(blk_fwd(t, f.b3));
    return pool_fwd(t, f.b3.Z, f.pool, f.idx, B, f.P, 1024);
}

// f.dpool holds dL/d(pooled feature) on entry
int feat_bwd(T *t, FeatA &f, int B) {
    float *G = t->G, *H = t->H;
    TRY(pool_bwd(t, f.dpool, f.idx, G, B, f.P, 1024));
    TRY(blk_bwd(t, f.b3, G, H, 0));
    TRY(blk_bwd(t, f.b2, H, G, 0));
    TRY(blk_bwd(t, f.b1, G, H, 0));          // H = dL/d xt [M][64]
    float *d0b = H;
    if (t->stn) {
        const LinP &fc3 = (&f == &t->fa[0] ? t->net.f[0] : t->net.f[1]).t.fc3;
        TGemm g{};
        // dT[b][i][j] = sum_p dxt[p][i] x[p][j]
        g.A = H; g.sam = 1; g.sak = 64; g.a_z = (long long)f.P * 64;
        g.B = f.b0b.Z; g.sbk = 64; g.sbn = 1; g.b_z = (long long)f.P * 64;
        g.C = f.dT; g.ldc = 64; g.c_z = 4096; g.M = 64; g.N = 64; g.K = f.P;
        TRY(launch_gemm(t, g, B));
        // dx[p][j] = sum_i dxt[p][i] T[i][j]
        TGemm h{};
        h.A = H; h.sam = 64; h.sak = 1; h.a_z = (long long)f.P * 64;
        h.B = f.T; h.sbk = 64; h.sbn = 1; h.b_z = 4096;
        h.C = f.d64; h.ldc = 64; h.c_z = (long long)f.P * 64; h.M = f.P; h.N = 64; h.K = 64;
        TRY(launch_gemm(t, h, B));
        // the trunk: fc3 (no batch-norm), fc2, fc1, pool (after ReLU), conv3, conv2, conv1; its dX adds to d64
        TRY(linear_bwd(t, fc3, f.t5.Z, f.dT, G, B, 0));
        TRY(blk_bwd(t, f.t5, G, H, 0));
        TRY(blk_bwd(t, f.t4, H, G, 0));      // G = dL/d tpool [B][1024]
        TRY(pool_bwd(t, G, f.tidx, H, B, f.P, 1024));
        TRY(blk_bwd(t, f.t3, H, G, 0));
        TRY(blk_bwd(t, f.t2, G, H, 0));
        TRY(blk_bwd(t, f.t1, H, f.d64, 1));
        d0b = f.d64;
    }
    float *o = (d0b == G) ? H : G;
    TRY(blk_bwd(t, f.b0b, d0b, o, 0));
    return blk_bwd(t, f.b0a, o, nullptr, 0);
}

int step_impl(T *t, const float *patch, const float *sub, const float *query, const float *dist, const float *sign01,
              const float *radius, int B, double *losses_host) {
    if (B != t->B || !t->arena) {
        const size_t bytes = plan(t, nullptr, B, patch);
        t->own.arena.reset();
        t->arena = nullptr;
        t->B = 0;
        if (!t->own.arena.alloc(bytes / 4)) {
            p2s_set_error("trainer: cannot allocate %zu bytes of activations for B = %d", bytes, B);
            return P2S_ENOMEM;
        }
        t->arena = t->own.arena.get();
        t->arena_floats = bytes / 4;
        t->B = B;
    }
    plan(t, t->arena, B, patch);
    t->have_grads = false;
    P2S_HIP_CHECK(hipMemsetAsync(t->flag, 0, sizeof(int), t->s));
    {
        Prof p(t, FAM_SMALL);
        const long long n = (long long)B * t->S * 3;
        hipLaunchKernelGGL(p2s_train_center_kernel, g1(n), dim3(256), 0, t->s, sub, query, (float *)t->fa[1].x3, n, t->S);
        P2S_LAUNCH_CHECK("p2s_train_center_kernel");
    }
    // forward (the reference runs feat_global first; the order does not change any value)
    for (int e = 1; e >= 0; --e) {
        TRY(feat_fwd(t, t->fa[e], B));
        TRY(blk_fwd(t, t->h1[e]));
        TRY(copy_cols(t, t->h1[e].Z, 512, t->cat + 512 * e, 1024, B, 512));
    }
    TRY(blk_fwd(t, t->h2));
    TRY(blk_fwd(t, t->h3));
    const LinP &fc4 = t->net.fc4;
    {
        Prof p(t, FAM_SMALL);
        hipLaunchKernelGGL(p2s_train_fc4_kernel, g1(B), dim3(256), 0, t->s, t->h3.Z, t->params + fc4.w, t->params + fc4.b, t->pred, B, fc4.K);
        P2S_LAUNCH_CHECK("p2s_train_fc4_kernel");
        hipLaunchKernelGGL(p2s_train_loss_kernel, dim3(1), dim3(256), 0, t->s, t->pred, dist, sign01, radius, t->dpred, t->loss, B);
        P2S_LAUNCH_CHECK("p2s_train_loss_kernel");
        // backward
        hipLaunchKernelGGL(p2s_train_fc4_bwd_kernel, g1((long long)B * fc4.K + 2 * fc4.K + 2), dim3(256), 0, t->s, t->dpred, t->h3.Z,
                           t->params + fc4.w, t->G, t->grads + fc4.w, t->grads + fc4.b, B, fc4.K);
        P2S_LAUNCH_CHECK("p2s_train_fc4_bwd_kernel");
    }
    TRY(blk_bwd(t, t->h3, t->G, t->H, 0));
    TRY(blk_bwd(t, t->h2, t->H, t->G, 0));       // G = dL/d cat [B][1024]
    float *dcat = t->G;
    // both halves leave G before the encoders reuse it
    float *half[2] = {t->H, t->H + (size_t)B * 512};
    for (int e = 0; e < 2; ++e) TRY(copy_cols(t, dcat + 512 * e, 1024, half[e], 512, B, 512));
    for (int e = 0; e < 2; ++e) TRY(blk_bwd(t, t->h1[e], half[e], t->fa[e].dpool, 0));
    for (int e = 0; e < 2; ++e) TRY(feat_bwd(t, t->fa[e], B));
    {
        Prof p(t, FAM_SMALL);
        hipLaunchKernelGGL(p2s_train_finite_kernel, g1(t->np), dim3(256), 0, t->s, t->grads, t->np, t->loss, t->flag);
        P2S_LAUNCH_CHECK("p2s_train_finite_kernel");
    }
    double lh[2];
    int flag = 0;
    P2S_HIP_CHECK(hipMemcpyAsync(lh, t->loss, sizeof(lh), hipMemcpyDeviceToHost, t->s));
    P2S_HIP_CHECK(hipMemcpyAsync(&flag, t->flag, sizeof(int), hipMemcpyDeviceToHost, t->s));
    P2S_HIP_CHECK(hipStreamSynchronize(t->s));
    if (losses_host) { losses_host[0] = lh[0]; losses_host[1] = lh[1]; }
    if (flag) {
        p2s_set_error("p2s_trainer_forward_backward: non-finite loss or gradient (losses %g, %g); nothing was updated", lh[0], lh[1]);
        return P2S_EINVAL;
    }
    {
        Prof p(t, FAM_SMALL);
        hipLaunchKernelGGL(p2s_train_running_kernel, g1(t->nb), dim3(256), 0, t->s, t->bufs, t->pend, t->nb);
        P2S_LAUNCH_CHECK("p2s_train_running_kernel");
    }
    t->nbt += 1;
    t->have_grads = true;
    return P2S_OK;
}

}  // namespace

extern "C" {

int p2s_trainer_create(const p2s_model_cfg *cfg, int use_feat_stn, const float *params_host, int64_t n_params,
                       const float *buffers_host, int64_t n_buffers, int64_t num_batches_tracked, int device,
                       p2s_trainer_t *out) {
    if (!cfg || !params_host || !buffers_host || !out) {
        p2s_set_error("p2s_trainer_create: null argument");
        return P2S_EINVAL;
    }
    *out = nullptr;
    const char *why = nullptr;
    if (cfg->use_point_stn) why = "a QSTN (use_point_stn) is not trained on the device";
    else if (cfg->single_transformer) why = "the shared encoder (single_transformer) is not trained on the device";
    else if (cfg->shared_transformer) why = "a shared transformer is not trained on the device";
    else if (cfg->sym_sum) why = "sum pooling (sym_op='sum') is not trained on the device";
    else if (cfg->output_dim != 2) why = "regression (output_dim != 2) is not trained on the device";
    else if (cfg->patch_radius != 0.0) why = "a fixed patch radius is not trained on the device";
    else if (cfg->net_size != 1024) why = "only net size 1024 is trained on the device";
    else if (cfg->points_per_patch < 1 || cfg->sub_sample_size < 1) why = "points_per_patch and sub_sample_size must be positive";
    if (why) {
        p2s_set_error("p2s_trainer_create: %s (p2s_max and p2s_max_no_feat_stn only)", why);
        return P2S_EINVAL;
    }
    Layout L;
    const NetP net = L.net(1024, use_feat_stn != 0);
    if (n_params != L.np || n_buffers != L.nb) {
        p2s_set_error("p2s_trainer_create: %lld parameters / %lld buffer values given, the model has %lld / %lld",
                      (long long)n_params, (long long)n_buffers, L.np, L.nb);
        return P2S_EINVAL;
    }
    if (p2s_device_count() <= device || device < 0) {
        p2s_set_error("p2s_trainer_create: no HIP device %d", device);
        return P2S_ENODEVICE;
    }
    P2S_HIP_CHECK(hipSetDevice(device));
    p2s_trainer_s *t = new p2s_trainer_s();
    t->device = device; t->P = cfg->points_per_patch; t->S = cfg->sub_sample_size; t->stn = use_feat_stn != 0;
    t->net = net; t->np = L.np; t->nb = L.nb; t->nbt = num_batches_tracked;
    const int rc = [&]() -> int {
        p2s_trainer_s::Owned &o = t->own;
        if (!p2s_alloc_all(o.params, L.np, o.grads, L.np, o.mom, L.np, o.bufs, L.nb, o.pend, L.nb)) {
            p2s_set_error("p2s_trainer_create: cannot allocate %lld parameters and %lld buffer values", L.np, L.nb);
            return P2S_ENOMEM;
        }
        t->params = o.params.get(); t->grads = o.grads.get(); t->mom = o.mom.get(); t->bufs = o.bufs.get(); t->pend = o.pend.get();
        P2S_HIP_CHECK(hipMemcpy(t->params, params_host, L.np * 4, hipMemcpyHostToDevice));
        P2S_HIP_CHECK(hipMemcpy(t->bufs, buffers_host, L.nb * 4, hipMemcpyHostToDevice));
        P2S_HIP_CHECK(hipMemset(t->grads, 0, L.np * 4));
        P2S_HIP_CHECK(hipMemset(t->mom, 0, L.np * 4));
        P2S_HIP_CHECK(hipMemset(t->pend, 0, L.nb * 4));
        return P2S_OK;
    }();
    if (rc != P2S_OK) {
        p2s_trainer_destroy(t);
        return rc;
    }
    *out = t;
    return P2S_OK;
}

int p2s_trainer_destroy(p2s_trainer_t t) {
    if (!t) return P2S_OK;
    (void)hipSetDevice(t->device);
    delete t;
    return P2S_OK;
}

int p2s_trainer_sizes(p2s_trainer_t t, int64_t *n_params, int64_t *n_buffers, int64_t *n_pools, int64_t *resident_bytes) {
    if (!t) { p2s_set_error("p2s_trainer_sizes: null handle"); return P2S_EINVAL; }
    if (n_params) *n_params = t->np;
    if (n_buffers) *n_buffers = t->nb;
    if (n_pools) *n_pools = t->stn ? 4 : 2;
    if (resident_bytes) *resident_bytes = (int64_t)(t->arena ? t->arena_floats * 4 : 0) + (3 * t->np + 2 * t->nb) * 4;
    return P2S_OK;
}

int p2s_trainer_forward_backward(p2s_trainer_t t, const float *patch_ps_dev, const float *sub_ms_dev, const float *query_dev,
                                 const float *dist_abs_dev, const float *sign01_dev, const float *radius_dev, int B,
                                 double *losses_host, void *stream) {
    if (!t || !patch_ps_dev || !sub_ms_dev || !query_dev || !dist_abs_dev || !sign01_dev || !radius_dev) {
        p2s_set_error("p2s_trainer_forward_backward: null argument");
        return P2S_EINVAL;
    }
    if (B < 2) {
        p2s_set_error("p2s_trainer_forward_backward: B = %d; batch-norm on batch statistics needs at least 2 items", B);
        return P2S_EINVAL;
    }
    if ((long long)B * std::max(t->P, t->S) * 1024 >= (1LL << 31) * 1024) {
        p2s_set_error("p2s_trainer_forward_backward: B = %d: more than 2^31 point rows", B);
        return P2S_ECAPACITY;
    }
    P2S_HIP_CHECK(hipSetDevice(t->device));
    t->s = (hipStream_t)stream;
    for (double &m : t->fam_ms) m = 0.0;
    const int rc = step_impl(t, patch_ps_dev, sub_ms_dev, query_dev, dist_abs_dev, sign01_dev, radius_dev, B, losses_host);
    if (t->profile) {
        (void)hipStreamSynchronize(t->s);
        for (auto &e : t->events) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, e.second.first.get(), e.second.second.get()) == hipSuccess) t->fam_ms[e.first] += ms;
        }
        t->events.clear();
        (void)hipGetLastError();
    }
    return rc;
}

int p2s_trainer_sgd_step(p2s_trainer_t t, double lr, double momentum, void *stream) {
    if (!t) { p2s_set_error("p2s_trainer_sgd_step: null handle"); return P2S_EINVAL; }
    if (!t->have_grads) {
        p2s_set_error("p2s_trainer_sgd_step: no gradients (no successful p2s_trainer_forward_backward since the last step)");
        return P2S_EINVAL;
    }
    if (!(lr >= 0.0) || !(momentum >= 0.0)) {
        p2s_set_error("p2s_trainer_sgd_step: lr = %g, momentum = %g", lr, momentum);
        return P2S_EINVAL;
    }
    P2S_HIP_CHECK(hipSetDevice(t->device));
    hipLaunchKernelGGL(p2s_train_sgd_kernel, g1(t->np), dim3(256), 0, (hipStream_t)stream, t->params, t->grads, t->mom, t->np,
                       (float)lr, (float)momentum, t->first_step ? 1 : 0);
    P2S_LAUNCH_CHECK("p2s_train_sgd_kernel");
    if (momentum != 0.0) t->first_step = false;
    t->have_grads = false;
    return P2S_OK;
}

int p2s_trainer_copy_out(p2s_trainer_t t, int what, float *host, int64_t n_floats, int64_t *num_batches_tracked) {
    if (!t || (!host && n_floats > 0)) { p2s_set_error("p2s_trainer_copy_out: null argument"); return P2S_EINVAL; }
    const float *src = what == 0 ? t->params : (what == 1 ? t->bufs : (what == 2 ? t->grads : nullptr));
    const long long n = what == 1 ? t->nb : t->np;
    if (!src || n_floats != n) {
        p2s_set_error("p2s_trainer_copy_out: what = %d with %lld floats (0 parameters, 1 buffers, 2 gradients; %lld values)", what,
                      (long long)n_floats, n);
        return P2S_EINVAL;
    }
    P2S_HIP_CHECK(hipSetDevice(t->device));
    P2S_HIP_CHECK(hipDeviceSynchronize());
    P2S_HIP_CHECK(hipMemcpy(host, src, n * 4, hipMemcpyDeviceToHost));
    if (num_batches_tracked) *num_batches_tracked = t->nbt;
    return P2S_OK;
}

int p2s_trainer_pool_indices(p2s_trainer_t t, int32_t *host, int64_t n) {
    if (!t || !host) { p2s_set_error("p2s_trainer_pool_indices: null argument"); return P2S_EINVAL; }
    const int pools = t->stn ? 4 : 2;
    if (!t->arena || t->B < 2 || n != (int64_t)pools * t->B * 1024) {
        p2s_set_error("p2s_trainer_pool_indices: %lld values asked, the last step has %d pools of %d x 1024", (long long)n, pools, t->B);
        return P2S_EINVAL;
    }
    P2S_HIP_CHECK(hipSetDevice(t->device));
    P2S_HIP_CHECK(hipDeviceSynchronize());
    const size_t one = (size_t)t->B * 1024;
    int k = 0;
    for (int e = 0; e < 2; ++e) {
        if (t->stn) P2S_HIP_CHECK(hipMemcpy(host + one * k++, t->fa[e].tidx, one * 4, hipMemcpyDeviceToHost));
        P2S_HIP_CHECK(hipMemcpy(host + one * k++, t->fa[e].idx, one * 4, hipMemcpyDeviceToHost));
    }
    return P2S_OK;
}

int p2s_train_losses(const float *pred_dev, const float *dist_abs_dev, const float *sign01_dev, const float *radius_dev,
                     int B, double *losses_host, void *stream) {
    if (!pred_dev || !dist_abs_dev || !sign01_dev || !radius_dev || !losses_host) {
        p2s_set_error("p2s_train_losses: null argument");
        return P2S_EINVAL;
    }
    if (B < 1) {
        p2s_set_error("p2s_train_losses: B = %d; at least one item is needed", B);
        return P2S_EINVAL;
    }
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, pred_dev) != hipSuccess) {
        (void)hipGetLastError();
        p2s_set_error("p2s_train_losses: pred_dev is not device memory");
        return P2S_EINVAL;
    }
    P2S_HIP_CHECK(hipSetDevice(at.device));
    hipStream_t s = (hipStream_t)stream;
    P2sScratchLock scratch(at.device);
    double *out = (double *)scratch.get(2 * sizeof(double));
    if (!out) {
        p2s_set_error("p2s_train_losses: device allocation failed");
        return P2S_ENOMEM;
    }
    hipLaunchKernelGGL(p2s_train_loss_kernel, dim3(1), dim3(256), 0, s, pred_dev, dist_abs_dev, sign01_dev, radius_dev,
                       (float *)nullptr, out, B);
    P2S_LAUNCH_CHECK("p2s_train_loss_kernel");
    double lh[2];
    P2S_HIP_CHECK(hipMemcpyAsync(lh, out, sizeof(lh), hipMemcpyDeviceToHost, s));
    P2S_HIP_CHECK(hipStreamSynchronize(s));
    losses_host[0] = lh[0];
    losses_host[1] = lh[1];
    return P2S_OK;
}

}  // extern "C"

namespace {

// A trainer context for the test hooks: the caller's flat arrays in place of the model's, scratch of exactly the size the
// shape needs (what plan() provides for the network's layers), freed when the hook returns.
struct DebugCtx {
    p2s_trainer_s t;
    // every pointer must be device memory of one device, which becomes current
    int open(const char *who, std::initializer_list<const void *> ptrs, void *stream) {
        int dev = -1;
        for (const void *p : ptrs) {
            hipPointerAttribute_t at;
            if (!p || hipPointerGetAttributes(&at, p) != hipSuccess || at.type != hipMemoryTypeDevice || (dev >= 0 && at.device != dev)) {
                (void)hipGetLastError();
                p2s_set_error("%s: every array must be device memory of one device", who);
                return P2S_EINVAL;
            }
            dev = at.device;
        }
        P2S_HIP_CHECK(hipSetDevice(dev));
        t.device = dev;
        t.s = (hipStream_t)stream;
        return P2S_OK;
    }
    // column-sum partials for M rows of C channels, slab partials for a weight gradient of n values over M rows
    int scratch(const char *who, int M, int C, long long n) {
        const size_t cbytes = (size_t)colsum_slabs(M) * C * 3 * sizeof(double);
        const int slabs = dw_slabs(M);
        t.wpart_floats = slabs > 1 ? slabs * n : 0;
        if (!p2s_alloc_all(t.own.cpart, cbytes / sizeof(double), t.own.wpart, (size_t)t.wpart_floats)) {
            p2s_set_error("%s: cannot allocate %zu + %lld bytes of scratch", who, cbytes, t.wpart_floats * 4);
            return P2S_ENOMEM;
        }
        t.cpart = t.own.cpart.get();
        t.wpart = t.own.wpart.get();
        return P2S_OK;
    }
};

}  // namespace

extern "C" {

int p2s_debug_train_linear(const float *x_dev, const float *params_dev, int64_t b_offset, const float *dy_dev, float *y_dev,
                           float *dx_dev, float *grads_dev, int M, int N, int K, int accum, void *stream) {
    const char *who = "p2s_debug_train_linear";
    if (M <= 0 || N <= 0 || K <= 0 || (accum != 0 && accum != 1) || b_offset < (int64_t)N * K) {
        p2s_set_error("%s: M = %d, N = %d, K = %d must be positive, accum = %d must be 0 or 1, b_offset = %lld at least N * K", who, M,
                      N, K, accum, (long long)b_offset);
        return P2S_EINVAL;
    }
    if ((long long)M * std::max(N, K) >= (1LL << 31)) {
        p2s_set_error("%s: M = %d with N = %d, K = %d: more than 2^31 values in one array", who, M, N, K);
        return P2S_ECAPACITY;
    }
    DebugCtx c;
    TRY(c.open(who, {x_dev, params_dev, dy_dev, y_dev, dx_dev, grads_dev}, stream));
    TRY(c.scratch(who, M, N, (long long)N * K));
    c.t.params = const_cast<float *>(params_dev);
    c.t.grads = grads_dev;
    LinP l;
    l.K = K; l.N = N; l.w = 0; l.b = b_offset;
    TRY(linear_fwd(&c.t, l, x_dev, y_dev, M));
    TRY(linear_bwd(&c.t, l, x_dev, dy_dev, dx_dev, M, accum));
    P2S_HIP_CHECK(hipStreamSynchronize(c.t.s));
    return P2S_OK;
}

int p2s_debug_train_bn(const float *y_dev, const float *params_dev, int64_t second_offset, float *z_dev, float *mean_dev,
                       float *invstd_dev, float *pending_dev, float *d_dev, float *grads_dev, int M, int C, int relu, void *stream) {
    const char *who = "p2s_debug_train_bn";
    if (M < 2 || C <= 0 || second_offset < C) {
        p2s_set_error("%s: M = %d must be at least 2 (batch statistics), C = %d positive, second_offset = %lld at least C", who, M, C,
                      (long long)second_offset);
        return P2S_EINVAL;
    }
    if ((long long)M * C >= (1LL << 31)) {
        p2s_set_error("%s: M = %d with C = %d: more than 2^31 values in one array", who, M, C);
        return P2S_ECAPACITY;
    }
    DebugCtx c;
    TRY(c.open(who, {y_dev, params_dev, z_dev, mean_dev, invstd_dev, pending_dev, d_dev, grads_dev}, stream));
    TRY(c.scratch(who, M, C, 0));
    if (!c.t.own.arena.alloc(2 * (size_t)C)) {      // the two means of the backward
        p2s_set_error("%s: cannot allocate %zu bytes of scratch", who, 2 * (size_t)C * 4);
        return P2S_ENOMEM;
    }
    c.t.params = const_cast<float *>(params_dev);
    c.t.grads = grads_dev;
    c.t.pend = pending_dev;
    c.t.arena = c.t.own.arena.get();
    Blk b{};
    b.bn.C = C; b.bn.g = 0; b.bn.be = second_offset; b.bn.rm = 0; b.bn.rv = second_offset;
    b.relu = relu ? 1 : 0; b.M = M;
    b.Y = const_cast<float *>(y_dev); b.Z = z_dev;
    b.mean = mean_dev; b.invstd = invstd_dev; b.m1 = c.t.arena; b.m2 = c.t.arena + C;
    TRY(bn_fwd(&c.t, b));
    TRY(bn_bwd(&c.t, b, d_dev));
    P2S_HIP_CHECK(hipStreamSynchronize(c.t.s));
    return P2S_OK;
}

int p2s_debug_train_relu_masks(p2s_trainer_t t, uint8_t *host, int64_t n) {
    const char *who = "p2s_debug_train_relu_masks";
    if (!t || !host) { p2s_set_error("%s: null argument", who); return P2S_EINVAL; }
    if (!t->arena || t->B < 2) { p2s_set_error("%s: no training step has run on this trainer", who); return P2S_EINVAL; }
    // the order of the reference's forward: feat_global, fc1_global, feat_local, fc1_local, fc2, fc3
    std::vector<const Blk *> blks;
    for (int e = 1; e >= 0; --e) {
        const FeatA &f = t->fa[e];
        blks.push_back(&f.b0a); blks.push_back(&f.b0b);
        if (t->stn)
            for (const Blk *b : {&f.t1, &f.t2, &f.t3, &f.t4, &f.t5}) blks.push_back(b);
        blks.push_back(&f.b1); blks.push_back(&f.b2);
        blks.push_back(&t->h1[e]);
    }
    blks.push_back(&t->h2); blks.push_back(&t->h3);
    long long total = 0;
    for (const Blk *b : blks) total += (long long)b->M * b->bn.C;
    if (n != total) {
        p2s_set_error("%s: %lld values asked, the last step has %lld units behind a ReLU", who, (long long)n, total);
        return P2S_EINVAL;
    }
    P2S_HIP_CHECK(hipSetDevice(t->device));
    P2S_HIP_CHECK(hipDeviceSynchronize());
    std::vector<float> tmp;
    long long o = 0;
    for (const Blk *b : blks) {
        const size_t cnt = (size_t)b->M * b->bn.C;
        tmp.resize(cnt);
        P2S_HIP_CHECK(hipMemcpy(tmp.data(), b->Z, cnt * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < cnt; ++i) host[o + i] = tmp[i] > 0.f ? 1 : 0;
        o += (long long)cnt;
    }
    return P2S_OK;
}

int p2s_trainer_profile(p2s_trainer_t t, int enabled, double *family_ms) {
    if (!t) { p2s_set_error("p2s_trainer_profile: null handle"); return P2S_EINVAL; }
    if (family_ms)
        for (int i = 0; i < FAM_N; ++i) family_ms[i] = t->fam_ms[i];
    t->profile = enabled ? 1 : 0;
    return P2S_OK;
}

}  // extern "C"
