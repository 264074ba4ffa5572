// The small device primitives that the geometry units share.  Included INSIDE a unit's anonymous namespace: the build has no
// relocatable device code, so every unit that includes this gets its own copy of the kernels.
//   f2o / o2f                order-preserving float <-> int, on the device and on the host
//   uf_find                  the root of a union-find whose parents only decrease
//   p2s_uf_compress_kernel   parent[i] = root of i
//   p2s_iota_kernel          out[i] = i
//   p2s_scan_kernel          exclusive scan of int counts, one workgroup; in place when start == count

// order-preserving float <-> int (its own inverse)
__host__ __device__ __forceinline__ int f2o(float f) {
    const int i = __builtin_bit_cast(int, f);
    return i >= 0 ? i : i ^ 0x7fffffff;
}
__host__ __device__ __forceinline__ float o2f(int i) { return __builtin_bit_cast(float, i >= 0 ? i : i ^ 0x7fffffff); }

// union-find with hooking to the smaller root: parents only decrease, so the walk meets no cycle
__device__ __forceinline__ int uf_find(const int *parent, int x) {
    for (int p = parent[x]; p != x; p = parent[x]) x = p;
    return x;
}
__global__ __launch_bounds__(256) void p2s_uf_compress_kernel(int *parent, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) parent[i] = uf_find(parent, (int)i);
}
__global__ __launch_bounds__(256) void p2s_iota_kernel(int *__restrict__ out, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (int)i;
}

// exclusive scan of count [n] into start [n + 1] (one workgroup, chunks of 1024: the scan of each wave, the 16 wave sums, a
// carry from chunk to chunk).  start may be count: a thread reads its element before it writes it, and no other touches it
__global__ __launch_bounds__(1024) void p2s_scan_kernel(const int *count, long long n, int *start) {
    __shared__ int ws[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;
    for (long long b0 = 0; b0 < n; b0 += 1024) {
        const long long i = b0 + tid;
        const int c = i < n ? count[i] : 0;
        int v = c;
        for (int d = 1; d < 64; d <<= 1) {
            const int u = __shfl_up(v, d);
            if (lane >= d) v += u;
        }
        if (lane == 63) ws[wave] = v;
        __syncthreads();
        int base = carry, tot = 0;
        for (int w = 0; w < 16; ++w) {
            if (w < wave) base += ws[w];
            tot += ws[w];
        }
        if (i < n) start[i] = base + v - c;
        carry += tot;
        __syncthreads();
    }
    if (tid == 0) start[n] = carry;
}
