// device_scan.hip — exclusive scan of a u32 array in place (side_util.h), three launches: tile sums, one-workgroup scan of the sums,
// tile scans.  Integer sums: exact in any order.  Used by the mesh extraction, the mesh filter and both evaluations (MESH.md).
#include <hip/hip_runtime.h>

#include "block_ops.h"
#include "side_util.h"

namespace surfel {

constexpr int SCAN_T = 256;      // threads per workgroup: 16 elements per thread
static_assert(SCAN_TILE == SCAN_T * 16, "a tile is 16 elements per thread");

// scans elements [base, base + SCAN_TILE) of a (thread t: 16 consecutive) adding `carry`; returns the tile total
__device__ uint32_t scan_tile(uint32_t* a, int64_t n, int64_t base, uint32_t carry, uint32_t* s_w) {
    uint32_t v[16], sum = 0, total;
    const int64_t b = base + 16 * (int64_t)threadIdx.x;
    for (int i = 0; i < 16; i++) { v[i] = b + i < n ? a[b + i] : 0u; sum += v[i]; }
    uint32_t run = block_excl_sum<SCAN_T>(sum, s_w, &total) + carry;
    for (int i = 0; i < 16; i++)
        if (b + i < n) { a[b + i] = run; run += v[i]; }
    return total;
}

__global__ void __launch_bounds__(SCAN_T) scan_sums_kernel(const uint32_t* __restrict__ a, int64_t n, uint32_t* __restrict__ sums) {
    __shared__ uint32_t s_w[SCAN_T / 64];
    const int64_t b = (int64_t)blockIdx.x * SCAN_TILE + 16 * (int64_t)threadIdx.x;
    uint32_t sum = 0, total;
    for (int i = 0; i < 16; i++) sum += b + i < n ? a[b + i] : 0u;
    block_excl_sum<SCAN_T>(sum, s_w, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ void __launch_bounds__(SCAN_T) scan_top_kernel(uint32_t* __restrict__ sums, int64_t ntiles) {      // sums[ntiles] = total
    __shared__ uint32_t s_w[SCAN_T / 64];
    uint32_t carry = 0;
    // (block_excl_sum opens with a barrier: every thread has read the previous round's s_w before this round writes it)
    for (int64_t base = 0; base < ntiles; base += SCAN_TILE) carry += scan_tile(sums, ntiles, base, carry, s_w);
    if (threadIdx.x == 0) sums[ntiles] = carry;
}

__global__ void __launch_bounds__(SCAN_T) scan_apply_kernel(uint32_t* __restrict__ a, int64_t n, const uint32_t* __restrict__ sums) {
    __shared__ uint32_t s_w[SCAN_T / 64];
    scan_tile(a, n, (int64_t)blockIdx.x * SCAN_TILE, sums[blockIdx.x], s_w);
}

int64_t scan_scratch_u32(int64_t n) { return (n + SCAN_TILE - 1) / SCAN_TILE + 1; }

void scan_u32(uint32_t* a, int64_t n, uint32_t* scratch, hipStream_t st) {
    const int64_t nt = (n + SCAN_TILE - 1) / SCAN_TILE;
    if (nt == 0) { (void)hipMemsetAsync(scratch, 0, 4, st); return; }
    hipLaunchKernelGGL(scan_sums_kernel, dim3((unsigned)nt), dim3(SCAN_T), 0, st, a, n, scratch);
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(SCAN_T), 0, st, scratch, nt);
    hipLaunchKernelGGL(scan_apply_kernel, dim3((unsigned)nt), dim3(SCAN_T), 0, st, a, n, scratch);
}

}  // namespace surfel
