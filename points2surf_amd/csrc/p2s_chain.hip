// Fused PointNet point-wise MLP chain + symmetric max-pool for gfx950 (CDNA4).
//
// Replaces, per (query, encoder) item, the reference's eager op sequence
//   conv0a,bn0a,relu / conv0b,bn0b,relu            (source/points_to_surf_model.py:190-191)
//   [bmm(trans2, x)] conv1,bn1,relu / conv2,bn2,relu / conv3,bn3[,relu] / MaxPool1d(P)
//                                                   (:41-49 STN trunk, :195-212 PointNetfeat)
// with ONE kernel in which no per-point activation ever reaches HBM.
//
// Design (MI355X-first, not a translation of the ATen ops):
//  * one 256-thread workgroup (4 waves, one per SIMD) per item; 3 workgroups per CU (50 KB LDS
//    each) so that one workgroup's MFMA stream covers another's epilogue / staging phases;
//  * points are processed in tiles of 64; activations of a tile live in LDS as [point][channel]
//    (row stride K+4 floats -> conflict-free ds_read_b128 of 4 consecutive channels);
//  * every layer with K >= 64 runs on v_mfma_f32_32x32x2_f32 (exact fp32, 64 FLOP/clk/SIMD) with
//    points = MFMA rows (A operand, from LDS) and output channels = MFMA columns (B operand);
//    weights are BatchNorm-folded on the host and pre-packed in B-fragment order
//    [N/32][K/8][64 lanes][4] so one coalesced global_load_dwordx4 (L2-resident, 1 KB per wave)
//    feeds 4 MFMAs per accumulator -- weights never pass through LDS;
//    the k index inside a group of 8 is permuted (lane-half kk owns k = 8g+4kk+t) identically for
//    A and B, which is what makes 16-byte operand loads possible with the 32x32x2 layout;
//  * with points on rows, the max-pool over points is 15 in-lane v_max over the accumulator
//    registers + one cross-half exchange per 32x32 tile: the [P x 1024] activation of conv3
//    (87.7 % of all FLOPs) is reduced in registers and never stored anywhere;
//  * bias (and ReLU for STN trunks) commute with the max and are applied once per item.
// Padding rows of the last tile replicate the item's last point (max is idempotent).
#include "p2s_common.h"
#include <cstdlib>
#include <atomic>

namespace {

constexpr int MT = 64;    // points per tile
constexpr int SA = 68;    // LDS row stride (floats) of a 64-channel activation tile
constexpr int SB = 132;   // LDS row stride (floats) of a 128-channel activation tile

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ f32x4 ldg4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
__device__ __forceinline__ f32x4 lds4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
typedef unsigned u32x4s __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 bufld4(__amdgpu_buffer_rsrc_t rsrc, int voff, int soff) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, soff, 0);
    f32x4 r;
    r[0] = __uint_as_float(v[0]); r[1] = __uint_as_float(v[1]); r[2] = __uint_as_float(v[2]); r[3] = __uint_as_float(v[3]);
    return r;
}

// C/D layout of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
// (b: the bias of the lane's column, bias[col0 + (lane & 31)])
__device__ __forceinline__ void store_tile_bias_relu(const f32x16 &acc, float *dst, int stride, int row0,
                                                     int col0, float b, int lane) {
    const int col = col0 + (lane & 31);
    const int rbase = row0 + 4 * (lane >> 5);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int row = rbase + (reg & 3) + 8 * (reg >> 2);
        dst[row * stride + col] = fmaxf(acc[reg] + b, 0.0f);
    }
}

__device__ __forceinline__ void store_tile_bias_relu(const f32x16 &acc, float *dst, int stride, int row0,
                                                     int col0, const float *__restrict__ bias, int lane) {
    store_tile_bias_relu(acc, dst, stride, row0, col0, bias[col0 + (lane & 31)], lane);
}

__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = 0.0f;
    return z;
}

// B operand of one K=64 layer, one 32-column tile: 8 k-groups = 8 buffer loads (32 VGPRs).  Weights do not
// depend on the activations, so they are fetched BEFORE the barrier that guards the layer's input.
struct B8 {
    f32x4 v[8];
};
__device__ __forceinline__ void load_b8(B8 &b, __amdgpu_buffer_rsrc_t rsrc, int lane16, int soff) {
#pragma unroll
    for (int kg = 0; kg < 8; ++kg) b.v[kg] = bufld4(rsrc, lane16, soff + kg * 1024);
}

// one K=64 layer: RT row tiles (rows row0 + 32 r) x one 32-column tile; A from LDS one k-group ahead, each
// ds_read in its own MFMA shadow; the first k-group accumulates into the literal 0 (no v_mov init)
// NEXT: the registers of a k-group's weights take the same k-group of the NEXT layer's weights (nrs, byte offset nsoff) as soon
// as the k-group's MFMAs have issued: the request has the rest of this layer, its epilogue and a barrier to come back.
// The fences keep the order written here.  Left to itself the scheduler moved every ds_read directly in front of the four
// MFMAs that use it (one full lgkmcnt(0) per k-group, the row tiles one after the other); with the fences alone the next
// layer's weights, which it had hoisted into this layer's MFMAs, were requested behind the layer's last MFMA
template <int RT, bool NEXT>
__device__ __forceinline__ void layer_k64(const float *src, int ss, int row0, B8 &b, int lane, f32x16 (&acc)[RT],
                                          __amdgpu_buffer_rsrc_t nrs, int lane16, int nsoff) {
    const float *ap = src + (row0 + (lane & 31)) * ss + 4 * (lane >> 5);
    f32x4 a[RT], na[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) a[r] = lds4(ap + 32 * r * ss);
#pragma unroll
    for (int kg = 0; kg < 8; ++kg) {
        if (kg < 7) {
#pragma unroll
            for (int r = 0; r < RT; ++r) na[r] = lds4(ap + 32 * r * ss + 8 * (kg + 1));
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < RT; ++r)
                acc[r] = (kg == 0 && t == 0) ? mfma32(a[r][0], b.v[0][0], zero16()) : mfma32(a[r][t], b.v[kg][t], acc[r]);
        if constexpr (NEXT) b.v[kg] = bufld4(nrs, lane16, nsoff + kg * 1024);
        __builtin_amdgcn_sched_barrier(0);
        if (kg < 7) {
#pragma unroll
            for (int r = 0; r < RT; ++r) {
                __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
            }
#pragma unroll
            for (int r = 0; r < RT; ++r) a[r] = na[r];
        }
    }
}

template <int RT>
__device__ __forceinline__ void layer_k64(const float *src, int ss, int row0, B8 &b, int lane, f32x16 (&acc)[RT]) {
    layer_k64<RT, false>(src, ss, row0, b, lane, acc, __builtin_amdgcn_make_buffer_rsrc((float *)nullptr, 0, 0, 0x00020000), 0, 0);
}

// conv1 of the STN pass of a model that reuses the stem (ChainBranch.stem_out): layer_k64<1>, and the wave stores the A fragments
// it has just read -- the conv0b output of its row tile, as conv1 of the main pass will want it -- one coalesced 1 KB store per
// k-group.  The two waves of a row tile read the same fragments and share the eight stores: column tile NT writes k-groups
// 4 NT .. 4 NT + 3.  soff: byte offset of (tile, row tile) in the item's stem
template <int NT>
__device__ __forceinline__ void layer_k64_store(const float *src, int ss, int row0, const B8 &b, int lane, f32x16 &acc,
                                                __amdgpu_buffer_rsrc_t out, int lane16, int soff) {
    const float *ap = src + (row0 + (lane & 31)) * ss + 4 * (lane >> 5);
    f32x4 a = lds4(ap), na;
#pragma unroll
    for (int kg = 0; kg < 8; ++kg) {
        if (kg < 7) na = lds4(ap + 8 * (kg + 1));
        if ((kg >> 2) == NT) {
            const u32x4s v = {__float_as_uint(a[0]), __float_as_uint(a[1]), __float_as_uint(a[2]), __float_as_uint(a[3])};
            __builtin_amdgcn_raw_buffer_store_b128(v, out, lane16, soff + kg * 1024, 0);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) acc = (kg == 0 && t == 0) ? mfma32(a[0], b.v[0][0], zero16()) : mfma32(a[t], b.v[kg][t], acc);
        if (kg < 7) {
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            if ((kg >> 2) == NT) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x040, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            } else {
                __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
            }
            a = na;
        }
    }
}
// conv1 of the main pass of such a model: the A fragments come from registers (the stem the STN pass saved); the k order and the
// accumulator chain are layer_k64's, so every value is the one conv1 computed from LDS.  The next layer's weights follow every
// k-group as in layer_k64<RT, true>
__device__ __forceinline__ void layer_k64_regs(const B8 &a, B8 &b, f32x16 &acc, __amdgpu_buffer_rsrc_t nrs, int lane16, int nsoff) {
#pragma unroll
    for (int kg = 0; kg < 8; ++kg) {
#pragma unroll
        for (int t = 0; t < 4; ++t) acc = (kg == 0 && t == 0) ? mfma32(a.v[0][0], b.v[0][0], zero16()) : mfma32(a.v[kg][t], b.v[kg][t], acc);
        b.v[kg] = bufld4(nrs, lane16, nsoff + kg * 1024);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// max over the 32 accumulator values of one output column (two row tiles): 1 v_max + 15 v_max3.
// Inline asm because fmaxf() on MFMA results makes hipcc prepend an sNaN-quieting v_max(x, x) to every
// operand (IEEE mode), which doubled the epilogue; (LLVM also folds med3(a, b, +inf) back to that form).
// hipcc does not pad hazards for asm operands, so the first statement carries the XDL-write -> VALU-read
// wait states itself (16-pass MFMA: 19 states; s_nop 15 + s_nop 4 = 21).  asm volatile keeps the order.
__device__ __forceinline__ float tile_colmax(const f32x16 &a, const f32x16 &b) {
    float m;
    asm volatile("s_nop 15\n\ts_nop 4\n\tv_max_f32 %0, %1, %2" : "=v"(m) : "v"(a[0]), "v"(b[0]));
#pragma unroll
    for (int i = 1; i < 16; ++i) asm volatile("v_max3_f32 %0, %0, %1, %2" : "+v"(m) : "v"(a[i]), "v"(b[i]));
    return m;
}

// max of lane l and lane l^32 in both lanes, without an LDS round trip: v_permlane32_swap exchanges the
// upper half of its first operand with the lower half of the second
__device__ __forceinline__ float half_max(float m) {
    const unsigned u = __float_as_uint(m);
    const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    float x = __uint_as_float(r[0]), y = __uint_as_float(r[1]), o;
    asm volatile("v_max_f32 %0, %1, %2" : "=v"(o) : "v"(x), "v"(y));
    return o;
}

// ---- 16-row tail (the last point tile of an item when at most 48 of its 64 rows are points) -------------------------
// Row tile 1 of such a tile holds <= 16 points (P = 300: 12, P = 1000: 8).  v_mfma_f32_16x16x1_4b_f32 multiplies FOUR
// independent 16x16 outer products per instruction, block = lane / 16 -- with the B register of the 32x32x2 layout
// unchanged (lane = 32 kk + col) the blocks are (cols 0-15, kk 0), (cols 16-31, kk 0), (cols 0-15, kk 1), (cols 16-31,
// kk 1): 16 rows x 32 columns x 2 k per instruction at half the cycles of the 32x32x2 form (8 passes), same weight
// fragments, same LDS tile.  The two kk partial sums of a column are added before the pool (one rounding more than
// the 32x32x2 chain on these <= 16 rows).  Saves a quarter of conv3 on one tile in 5 (P = 300) / 16 (P = 1000).
__device__ __forceinline__ f32x16 mfma16b(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_16x16x1f32(a, b, c, 0, 0, 0);
}
template <bool TAIL>
__device__ __forceinline__ f32x16 mfma_r1(float a, float b, f32x16 c) {
    if constexpr (TAIL) return mfma16b(a, b, c);
    else return mfma32(a, b, c);
}
// max over the 16 accumulator values of one output column of ONE row tile (see tile_colmax for the asm)
__device__ __forceinline__ float tile_colmax1(const f32x16 &a) {
    float m;
    asm volatile("s_nop 15\n\ts_nop 4\n\tv_max_f32 %0, %1, %2" : "=v"(m) : "v"(a[0]), "v"(a[1]));
#pragma unroll
    for (int i = 2; i < 16; i += 2) asm volatile("v_max3_f32 %0, %0, %1, %2" : "+v"(m) : "v"(a[i]), "v"(a[i + 1]));
    return m;
}
// column max of the 4-block accumulator: D layout block b = regs 4b..4b+3, row = 4 (lane / 16) + reg, col = lane % 16.
// cols 0-15: blocks 0 + 2, cols 16-31: blocks 1 + 3.  Returns, in lane l, the max over the 8 rows that lane l and
// lane l ^ 16 hold of column (l & 31) -- the lane's own column in the 32x32 layout; the l ^ 32 exchange that follows
// in half_max() completes the 16 rows.  v_permlane16_swap(x, y) trades the odd 16-lane rows of x for the even ones of y.
__device__ __forceinline__ float tail_colmax(const f32x16 &c) {
    float sa[4], sb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        sa[i] = c[i] + c[8 + i];
        sb[i] = c[4 + i] + c[12 + i];
    }
    float ma, mb;
    asm volatile("v_max3_f32 %0, %1, %2, %3" : "=v"(ma) : "v"(sa[0]), "v"(sa[1]), "v"(sa[2]));
    asm volatile("v_max_f32 %0, %0, %1" : "+v"(ma) : "v"(sa[3]));
    asm volatile("v_max3_f32 %0, %1, %2, %3" : "=v"(mb) : "v"(sb[0]), "v"(sb[1]), "v"(sb[2]));
    asm volatile("v_max_f32 %0, %0, %1" : "+v"(mb) : "v"(sb[3]));
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(ma), __float_as_uint(mb), false, false);
    float x = __uint_as_float(r[0]), y = __uint_as_float(r[1]), o;
    asm volatile("v_max_f32 %0, %1, %2" : "=v"(o) : "v"(x), "v"(y));
    return o;
}

// sym_op='sum' (reference source/points_to_surf_model.py:213-214): sum over the VALID rows of the two row tiles of one
// output column.  Rows past the item's last point replicate that point (harmless for a max) and are masked here.
// Plain C++: the compiler pads the XDL-write -> VALU-read hazard itself and adds need no sNaN quieting.
__device__ __forceinline__ float tile_colsum(const f32x16 &a, const f32x16 &b, int nvalid, int lane) {
    float s = 0.0f;
    if (nvalid >= 64) {
#pragma unroll
        for (int i = 0; i < 16; ++i) s += a[i];
#pragma unroll
        for (int i = 0; i < 16; ++i) s += b[i];
    } else {
        const int r0 = 4 * (lane >> 5);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int r = r0 + (i & 3) + 8 * (i >> 2);
            s += (r < nvalid) ? a[i] : 0.0f;
            s += (r + 32 < nvalid) ? b[i] : 0.0f;
        }
    }
    return s;
}
__device__ __forceinline__ float half_sum(float m) {
    const unsigned u = __float_as_uint(m);
    const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// ---- screened conv3 (p2s_chain_screen.inl) --------------------------------------------------------------------------
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr int SCR_HB = 128 + 8;      // halfs per row of the fp16 copy of the conv2 output tile (the fp16 pair kernel's layout)
constexpr int SCR_QCAP = 256;        // candidates a wave's queue holds: < 64 left over + what one column tile may add
constexpr float P2S_SCR_KAPPA = 0x1.1p-10f;   // k_screen + k_fp32 of the margin (derived in p2s_chain_screen.inl)
// LDS of the screened kernel (floats): the two fp32 tiles (the fp16 copy of h lies over bufA), the exact pool E [1024], the four
// waves' candidate queues, the reduction scratch, the running screen maxima, the margin coefficients and conv0a's operands (67 KB in all)
constexpr int SCR_OFF_E = MT * SA + MT * SB;
constexpr int SCR_OFF_Q = SCR_OFF_E + 1024;
constexpr int SCR_OFF_RED = SCR_OFF_Q + 4 * SCR_QCAP;
constexpr int SCR_OFF_R = SCR_OFF_RED + 8;            // running screen maxima R [1024] (r11: out of the registers)
constexpr int SCR_OFF_MU = SCR_OFF_R + 1024;          // margin coefficients [1024], copied once per workgroup
constexpr int SCR_OFF_W0 = SCR_OFF_MU + 1024;         // conv0a's weights [3][64] and biases [64], copied once per workgroup
constexpr int SCR_LDS_FLOATS = SCR_OFF_W0 + 256;
static_assert(MT * SCR_HB * 2 <= MT * SA * 4, "the fp16 copy fits the 64-channel tile it lies over");
static_assert(2 * SCR_LDS_FLOATS * 4 <= 160 * 1024, "two workgroups per CU");

__device__ __forceinline__ u32x4 scr_bufld(__amdgpu_buffer_rsrc_t rsrc, int voff, int soff) {
    return __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, soff, 0);
}
// A fragment of rows row0 .. row0+31, k-block kb of the fp16 tile: 8 consecutive k of row l & 31, k = 16 kb + 8 (l >> 5) + [0, 8)
__device__ __forceinline__ u32x4 scr_lds_a(const unsigned short *buf, int row0, int kb, int lane) {
    return *reinterpret_cast<const u32x4 *>(buf + (row0 + (lane & 31)) * SCR_HB + 16 * kb + 8 * (lane >> 5));
}
__device__ __forceinline__ f32x16 scr_mfma(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
// two fp32 values -> fp16 (round to nearest even), packed (a low half)
__device__ __forceinline__ unsigned scr_half2(float a, float b) {
    const f32x2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2));
}
// One candidate (entry = row << 16 | channel within the wave's 256): the fp32 dot product of row `row` of the conv2 tile with
// column c of the packed conv3 fragments ([N/32][16][2][32][4]: k = 8 g + 4 kk + t), summed as the dense kernel's MFMA chain
// sums it -- g ascending, t = 0..3, k = 8g+t then 8g+4+t into one accumulator; a row of the 16-row tail (SPLIT): the kk = 0
// and the kk = 1 chain apart, then their sum (tail_colmax) -- and pooled into E[channel] by an order-preserving integer max.
// The form is a template parameter, chosen per batch: a per-lane choice cost 16 selects beside the 8 fmaf of every k-group.
// The w3 loads are issued ahead of their use, SCR_CDEPTH k-groups at a time (2 x 4 registers per k-group): a pass requests the
// 2 SCR_CDEPTH fragments of its k-groups back to back and only then starts its 8 SCR_CDEPTH fmaf, so a batch waits for
// 16 / SCR_CDEPTH L1/L2 round trips and not for one per k-group.  The depth is what the register file leaves: during a
// confirm the A fragments (64 registers) and the weight ring (32) are live, and beside the kernel's per-tile state 8 k-groups
// (64 registers) spilled 15 VGPRs, 6 k-groups one, 4 none (profiles/r10/kernel_resources.txt).  The passes are a loop:
// unrolled into one block of 16 k-groups the kernel spilled at every depth.  The loads go through the buffer descriptor of
// the dense conv3 (32-bit offsets, no 64-bit address per fragment).  The order of the 128 products and additions is the one above
constexpr int SCR_CDEPTH = 4;
static_assert(16 % SCR_CDEPTH == 0, "whole passes");
template <bool SPLIT>
__device__ __forceinline__ void scr_confirm(unsigned entry, const float *hB, __amdgpu_buffer_rsrc_t w3rsrc, int wave, unsigned *E) {
    const int row = (int)(entry >> 16), cw = (int)(entry & 0xffffu);
    const int c = 256 * wave + cw;
    const float *hrow = hB + row * SB;
    const int wcol = ((c >> 5) * (16 * 64) + (c & 31)) * 16;       // bytes; k-group g, half kk: + (2 g + kk) * 512
    float s0 = 0.0f, s1 = 0.0f;
#pragma unroll 1
    for (int g0 = 0; g0 < 16; g0 += SCR_CDEPTH) {
        f32x4 wa[SCR_CDEPTH], wb[SCR_CDEPTH];
#pragma unroll
        for (int j = 0; j < SCR_CDEPTH; ++j) {
            wa[j] = bufld4(w3rsrc, wcol + j * 1024, g0 * 1024);
            wb[j] = bufld4(w3rsrc, wcol + j * 1024 + 512, g0 * 1024);
        }
        // the requests above stay ahead of the first fmaf, whatever the scheduler would like to do with their registers
        __builtin_amdgcn_sched_barrier(0);
        const float *hh = hrow + 8 * g0;
#pragma unroll
        for (int j = 0; j < SCR_CDEPTH; ++j) {
            const f32x4 ha = lds4(hh + 8 * j), hb = lds4(hh + 8 * j + 4);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                s0 = fmaf(ha[t], wa[j][t], s0);
                if constexpr (SPLIT) s1 = fmaf(hb[t], wb[j][t], s1);
                else s0 = fmaf(hb[t], wb[j][t], s0);
            }
        }
    }
    const float s = SPLIT ? s0 + s1 : s0;
    const int bits = (int)__float_as_uint(s);
    if (bits >= 0) atomicMax(reinterpret_cast<int *>(E + cw), bits);
    else atomicMin(E + cw, (unsigned)bits);
}

// SCREEN (max pool, full chain only): conv3 through p2s_chain_screen.inl, two workgroups per CU (66 KB of LDS); an item the
// screen cannot decide runs a second time with the dense conv3 below.  The body is p2s_chain_body.inl
template <bool SUM, bool SCREEN = false>
__global__ __launch_bounds__(256, SCREEN ? 2 : 3) void p2s_chain_kernel(ChainArgs args) {
    constexpr bool STEM_SAVE = false, STEM_LOAD = false;
#include "p2s_chain_body.inl"
}
// the two passes of a model that reuses the stem, both screened with a max pool: the STN pass, whose conv1 stores its A
// fragments to ChainBranch.stem_out, and the main pass, which starts at conv1 from ChainBranch.stem_in
__global__ __launch_bounds__(256, 2) void p2s_chain_save_kernel(ChainArgs args) {
    constexpr bool SUM = false, SCREEN = true, STEM_SAVE = true, STEM_LOAD = false;
#include "p2s_chain_body.inl"
}
__global__ __launch_bounds__(256, 2) void p2s_chain_reuse_kernel(ChainArgs args) {
    constexpr bool SUM = false, SCREEN = true, STEM_SAVE = false, STEM_LOAD = true;
#include "p2s_chain_body.inl"
}

// W1'[o][j] = sum_i W1f[o][i] * T[i][j], emitted directly in packed B-fragment order.
// Computed transposed (rows = j, cols = o) so that the MFMA C layout (row = 8g + 4*half + t)
// coincides with the packed layout (k = 8 kg + 4 kk + t): each lane stores whole float4s.
__global__ __launch_bounds__(256) void p2s_fold_kernel(FoldArgs args) {
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int e = blockIdx.y;
    const int item = blockIdx.x;
    const float *__restrict__ T = args.T[e] + (long long)item * 4096;
    const float *__restrict__ wp = args.m1t[e];
    float *__restrict__ out = args.out[e] + (long long)item * 4096;
    const int jt = wave >> 1, ot = wave & 1;
    const int kk = lane >> 5;
    f32x16 acc = zero16();
#pragma unroll
    for (int kg = 0; kg < 8; ++kg) {
        const f32x4 b = ldg4(wp + ((ot * 8 + kg) * 64 + lane) * 4);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float a = T[(8 * kg + 4 * kk + t) * 64 + 32 * jt + (lane & 31)];
            acc = mfma32(a, b[t], acc);
        }
    }
    unsigned short *outh = args.outh[e];
    if (outh) {
        // 16-bit fragment order: element (k, n) sits at [n / 32][k / 16][lane' = 32 ((k / 8) & 1) + n % 32][k % 8]; this
        // lane holds k = 32 jt + 8 g + 4 kk + t, t = 0..3: four consecutive halfs (8 bytes) per k-group g and piece
        outh += (long long)item * 4096;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int kg = 4 * jt + g;
            unsigned short *dst = outh + ((ot * 4 + (kg >> 1)) * 64 + (kg & 1) * 32 + (lane & 31)) * 8 + 4 * kk;
            float x[4] = {acc[4 * g + 0], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
            if (args.f16 && args.bad_items &&
                (p2s_f16_out_of_range(x[0]) || p2s_f16_out_of_range(x[1]) || p2s_f16_out_of_range(x[2]) || p2s_f16_out_of_range(x[3])))
                args.bad_items[item] = 1;          // this item's folded weights leave the half range: its query re-runs in fp32
            for (int q = 0; q < args.ns; ++q) {
                unsigned short h[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if (args.f16) {                    // fp16 pair: h0 = fp16(x); h1 = fp16((x - h0) * 2^11)
                        const _Float16 h0 = (_Float16)x[t];
                        h[t] = __builtin_bit_cast(unsigned short, h0);
                        x[t] = (x[t] - (float)h0) * 2048.0f;
                    } else {                           // bf16 pieces: round to nearest even of the residual
                        unsigned u = __float_as_uint(x[t]);
                        u += 0x7fffu + ((u >> 16) & 1u);
                        h[t] = (unsigned short)(u >> 16);
                        x[t] -= __uint_as_float((unsigned)h[t] << 16);
                    }
                }
                uint2 pk;
                pk.x = (unsigned)h[0] | ((unsigned)h[1] << 16);
                pk.y = (unsigned)h[2] | ((unsigned)h[3] << 16);
                *reinterpret_cast<uint2 *>(dst + (long long)q * args.h_piece_stride) = pk;
            }
        }
        return;
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        f32x4 v = {acc[4 * g + 0], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
        *reinterpret_cast<f32x4 *>(out + ((ot * 8 + 4 * jt + g) * 64 + lane) * 4) = v;
    }
}

}  // namespace

int p2s_launch_chain(const ChainArgs &args_in, hipStream_t stream) {
    const int n = args_in.br[0].n_items + args_in.br[1].n_items;
    if (n <= 0) return P2S_OK;
    ChainArgs args = args_in;
    constexpr int padlds = 0;
#ifdef P2S_DEV_ABLATE
    args.ablate = P2S_DEV_ABLATE + 0;      // the variant is the value of the define (1 = conv3 only, 2 = all but conv3, 3 .. 5, 7, 8 = parts of the screen)
#endif
    // both branches of a launch pool alike (pass 2 of a sym_op='sum' model: sum; every other launch: max)
    const bool sum = args.br[0].pool_sum || (args.br[1].n_items > 0 && args.br[1].pool_sum);
    if (args.screen) {
        if (sum || args.br[0].short_chain || (args.br[1].n_items > 0 && args.br[1].short_chain) || !args.w3h[0] || !args.w3mu[0] ||
            (args.br[1].n_items > 0 && (!args.w3h[1] || !args.w3mu[1]))) {
            p2s_set_error("p2s_launch_chain: the screened conv3 takes full-chain max-pool passes with their screen operands");
            return P2S_EINVAL;
        }
        // the saved stem: written by both branches of a launch, read by both, or neither (which: 0 neither, 1 written, 2 read)
        const int which = args.br[0].stem_in ? 2 : args.br[0].stem_out ? 1 : 0;
        for (int b = 0; b < 2; ++b) {
            const ChainBranch &br = args.br[b];
            if (br.n_items > 0 && ((br.stem_in ? 2 : br.stem_out ? 1 : 0) != which || (br.stem_in && br.stem_out) || (which && !br.stem_bad))) {
                p2s_set_error("p2s_launch_chain: the saved stem is written, or read, by both branches of a launch, with their flags");
                return P2S_EINVAL;
            }
        }
        if (which && args.br[1].n_items <= 0) {
            p2s_set_error("p2s_launch_chain: the saved stem belongs to launches of both branches");
            return P2S_EINVAL;
        }
        // the kernels' LDS exceeds the default limit: raised once per device and kernel
        static std::atomic<bool> lds_set[3][P2S_MAX_DEVICES];
        const void *kernel = which == 2 ? (const void *)p2s_chain_reuse_kernel : which == 1 ? (const void *)p2s_chain_save_kernel
                                                                                            : (const void *)p2s_chain_kernel<false, true>;
        int dev = 0;
        P2S_HIP_CHECK(hipGetDevice(&dev));
        if (dev < 0 || dev >= P2S_MAX_DEVICES || !lds_set[which][dev].load()) {
            const hipError_t attr = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, SCR_LDS_FLOATS * 4);
            if (attr != hipSuccess) {
                p2s_set_error("p2s_launch_chain: %d bytes of LDS for the screened conv3 refused: %s", SCR_LDS_FLOATS * 4, hipGetErrorString(attr));
                return P2S_EHIP;
            }
            if (dev >= 0 && dev < P2S_MAX_DEVICES) lds_set[which][dev].store(true);
        }
        if (which == 2) hipLaunchKernelGGL(p2s_chain_reuse_kernel, dim3(n), dim3(256), SCR_LDS_FLOATS * 4, stream, args);
        else if (which == 1) hipLaunchKernelGGL(p2s_chain_save_kernel, dim3(n), dim3(256), SCR_LDS_FLOATS * 4, stream, args);
        else hipLaunchKernelGGL((p2s_chain_kernel<false, true>), dim3(n), dim3(256), SCR_LDS_FLOATS * 4, stream, args);
    } else if (args.br[0].stem_in || args.br[0].stem_out || args.br[1].stem_in || args.br[1].stem_out) {
        p2s_set_error("p2s_launch_chain: only the screened conv3 saves or reuses the stem");
        return P2S_EINVAL;
    } else if (sum)
        hipLaunchKernelGGL(p2s_chain_kernel<true>, dim3(n), dim3(256), padlds, stream, args);
    else
        hipLaunchKernelGGL(p2s_chain_kernel<false>, dim3(n), dim3(256), padlds, stream, args);
    P2S_LAUNCH_CHECK("p2s_chain_kernel");
    return P2S_OK;
}

// margin coefficient of the screened conv3, one thread per output channel: 2 kappa (|w_c| + 2^-10), |w_c| in double from the
// packed fp32 fragments and rounded up
__global__ void p2s_screen_mu_kernel(const float *__restrict__ w3, float *__restrict__ mu) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= 1024) return;
    double ss = 0.0;
    for (int g = 0; g < 16; ++g)
        for (int u = 0; u < 8; ++u) {
            const double w = w3[(((long long)(c >> 5) * 16 + g) * 64 + (u >> 2) * 32 + (c & 31)) * 4 + (u & 3)];
            ss += w * w;
        }
    const float norm = (float)(sqrt(ss) * (1.0 + 0x1p-20));
    mu[c] = 2.0f * P2S_SCR_KAPPA * (norm * (1.0f + 0x1p-10f) + 0x1p-10f);
}

int p2s_launch_screen_prepare(const float *w32, unsigned short *dst, float *mu, hipStream_t stream, int *range_flag) {
    const int rc = p2s_launch_pack_bf16(w32, dst, 128, 1024, 0, 0, 1, 0, 1, stream, range_flag);
    if (rc) return rc;
    hipLaunchKernelGGL(p2s_screen_mu_kernel, dim3(4), dim3(256), 0, stream, w32, mu);
    P2S_LAUNCH_CHECK("p2s_screen_mu_kernel");
    return P2S_OK;
}

int p2s_launch_fold(const FoldArgs &args, hipStream_t stream) {
    if (args.n_items <= 0) return P2S_OK;
    hipLaunchKernelGGL(p2s_fold_kernel, dim3(args.n_items, 2), dim3(256), 0, stream, args);
    P2S_LAUNCH_CHECK("p2s_fold_kernel");
    return P2S_OK;
}
