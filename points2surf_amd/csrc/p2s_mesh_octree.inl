// The implicit octree of the mesh handle, stated once for its three walks: p2s_md_index_kernel (nearest triangle),
// p2s_md_wtree_kernel (winding number) and p2s_mr_index_kernel (first hit of a ray).  Included by p2s_meshdist.hip ahead of
// the build (p2s_meshbuild.inl), which fills it.
// Level l has 2^l nodes per axis, stored x-major (lin = (x 2^l + y) 2^l + z) behind the levels above it; the leaves are
// the G^3 cells of level L (G = 2^L), whose triangles are stri / sface / scomp [cell_start[lin], cell_start[lin + 1]).
// A node on a walk's stack is (level << OCT_LIN_BITS) | lin.  A pop of an inner node pushes at most 8 children, so a
// depth-first walk holds at most 7 entries per opened level plus the 8th child of the last: OCT_MAX_DEPTH.
namespace {

constexpr int MD_MAX_L = 7;                              // G <= 128
constexpr int OCT_LIN_BITS = 27;
constexpr int OCT_MAX_DEPTH = 7 * MD_MAX_L + 1;          // 50
constexpr int OCT_STACK = 52;                            // entries of a LaneStack column: 13 KiB of LDS per 64 lanes
static_assert(3 * MD_MAX_L + 3 <= OCT_LIN_BITS, "a node id is (level << 27) | linear index");
static_assert(OCT_STACK >= OCT_MAX_DEPTH, "depth-first stack: 7 entries stay per opened level, plus the 8th child of the last");

struct OctreeDev {
    const int *nodes;            // [(8^(L+1) - 1) / 7][6]  lo, hi as ordered integers of the float32 bounds; empty: lo > hi
    const double *mom;           // [same][4]  sum of the area vectors and of the areas
    const int *cell_start;       // [G^3 + 1]
    const int *sface;            // [F]     face ids sorted by cell
    const double *stri;          // [F][9]  triangles in that order
    const int *scomp;            // [F]     component labels in that order (closed meshes of 2..16 components)
    int L;
    double scale;                // largest |coordinate| of the mesh
};

__host__ __device__ __forceinline__ long long oct_level_offset(int l) { return ((1ll << (3 * l)) - 1) / 7; }      // nodes above level l
__device__ __forceinline__ int oct_id(int l, int lin) { return (l << OCT_LIN_BITS) | lin; }
__device__ __forceinline__ int oct_level(int id) { return id >> OCT_LIN_BITS; }
__device__ __forceinline__ int oct_lin(int id) { return id & ((1 << OCT_LIN_BITS) - 1); }
__device__ __forceinline__ long long oct_at(int l, int lin) { return oct_level_offset(l) + lin; }
__device__ __forceinline__ const int *oct_box(const OctreeDev &ix, int l, int lin) { return ix.nodes + 6 * oct_at(l, lin); }
__device__ __forceinline__ const double *oct_moments(const OctreeDev &ix, int l, int lin) { return ix.mom + 4 * oct_at(l, lin); }
__device__ __forceinline__ void oct_xyz(int l, int lin, int *xyz) {
    const int nn = 1 << l;
    xyz[0] = lin >> (2 * l);
    xyz[1] = (lin >> l) & (nn - 1);
    xyz[2] = lin & (nn - 1);
}
// child c (bit 2: x, bit 1: y, bit 0: z) of the node xyz of level l, as a linear index of level l + 1
__device__ __forceinline__ int oct_child_lin(int l, const int *xyz, int c) {
    const int nn = 1 << l;
    return ((2 * xyz[0] + (c >> 2)) * (2 * nn) + (2 * xyz[1] + ((c >> 1) & 1))) * (2 * nn) + (2 * xyz[2] + (c & 1));
}
__device__ __forceinline__ void oct_leaf_range(const OctreeDev &ix, int lin, int *t0, int *t1) {
    *t1 = ix.cell_start[lin + 1];
    *t0 = ix.cell_start[lin];
}

// The stack of a walk, one LDS column per lane of a 64-lane workgroup: conflict-free, and no scratch round trips.  A push
// beyond OCT_STACK cannot happen for L <= MD_MAX_L; if it ever did it raises *overflow (the call then fails) instead of
// dropping a node.
struct LaneStack {
    int *lds;                    // [OCT_STACK * 64]
    int lane, sp;
    __device__ __forceinline__ LaneStack(int *lds_, int lane_) : lds(lds_), lane(lane_), sp(0) {}
    __device__ __forceinline__ bool empty() const { return sp == 0; }
    __device__ __forceinline__ int pop() { return lds[(--sp) * 64 + lane]; }
    __device__ __forceinline__ void push(int id, unsigned long long *overflow) {
        if (sp < OCT_STACK) lds[(sp++) * 64 + lane] = id;
        else atomicOr(overflow, 1ull);
    }
};

// a counter of a walk: the sum over the wave, added to *total by its first lane
__device__ __forceinline__ void wave_count(unsigned long long *total, unsigned long long v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(total, v);
}

}  // namespace
