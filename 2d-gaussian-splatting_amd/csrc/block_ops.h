// block_ops.h — sums and extrema over the 64 lanes of a wave, and scans and reductions over a workgroup of NT threads (a multiple of
// 64), device only.  Every thread of the wave / workgroup calls them together.  s_w: NT / 64 words of LDS; each workgroup function opens
// with a barrier, so s_w may be reused from call to call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace surfel {

// xor-shuffle reductions over the 64 lanes of a wave: every lane returns the result
template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = op(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) { return wave_reduce(v, [](uint32_t a, uint32_t b) { return a + b; }); }
__device__ __forceinline__ uint32_t wave_max(uint32_t v) { return wave_reduce(v, [](uint32_t a, uint32_t b) { return max(a, b); }); }
__device__ __forceinline__ uint32_t wave_min(uint32_t v) { return wave_reduce(v, [](uint32_t a, uint32_t b) { return min(a, b); }); }

// inclusive scan over the 64 lanes of a wave (lane: threadIdx.x & 63, for callers that hold it already)
__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t v) { return wave_incl_sum(v, threadIdx.x & 63); }

// exclusive scan of v over the workgroup; total = the sum
template <int NT>
__device__ __forceinline__ uint32_t block_excl_sum(uint32_t v, uint32_t* s_w, uint32_t* total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t incl = wave_incl_sum(v);
    __syncthreads();                         // (the previous round's reads of s_w are done)
    if (lane == 63) s_w[wv] = incl;
    __syncthreads();
    uint32_t before = 0, sum = 0;
#pragma unroll
    for (int k = 0; k < NT / 64; k++) {
        const uint32_t c = s_w[k];
        if (k < wv) before += c;
        sum += c;
    }
    *total = sum;
    return before + incl - v;
}

template <int NT>
__device__ __forceinline__ uint32_t block_scan_max(uint32_t v, uint32_t* s_w) {      // inclusive, towards higher threads
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(v, off, 64);
        if (lane >= off) v = max(v, o);
    }
    __syncthreads();
    if (lane == 63) s_w[wv] = v;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NT / 64; k++)
        if (k < wv) v = max(v, s_w[k]);
    return v;
}

template <int NT>
__device__ __forceinline__ uint32_t block_scan_min_suffix(uint32_t v, uint32_t* s_w) {      // inclusive, towards lower threads
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_down(v, off, 64);
        if (lane + off < 64) v = min(v, o);
    }
    __syncthreads();
    if (lane == 0) s_w[wv] = v;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NT / 64; k++)
        if (k > wv) v = min(v, s_w[k]);
    return v;
}

template <int NT>
__device__ __forceinline__ uint32_t block_min(uint32_t v, uint32_t* s_w) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    v = wave_min(v);
    __syncthreads();
    if (lane == 0) s_w[wv] = v;
    __syncthreads();
    uint32_t r = s_w[0];
#pragma unroll
    for (int k = 1; k < NT / 64; k++) r = min(r, s_w[k]);
    return r;
}

template <int NT>
__device__ __forceinline__ uint64_t block_sum64(uint64_t v, uint64_t* s_w) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    v = wave_reduce(v, [](uint64_t a, uint64_t b) { return a + b; });
    __syncthreads();
    if (lane == 0) s_w[wv] = v;
    __syncthreads();
    uint64_t r = 0;
#pragma unroll
    for (int k = 0; k < NT / 64; k++) r += s_w[k];
    return r;
}

template <int NT>
__device__ __forceinline__ uint32_t block_xor(uint32_t v, uint32_t* s_w) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    v = wave_reduce(v, [](uint32_t a, uint32_t b) { return a ^ b; });
    __syncthreads();
    if (lane == 0) s_w[wv] = v;
    __syncthreads();
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < NT / 64; k++) r ^= s_w[k];
    return r;
}

// acc[0 .. K - 1] of every thread -> their sums in sh[k * NT] (sh: K * NT elements), by a halving tree of fixed shape.  Oracles restate
// the order of the additions: floating-point results depend on it.
template <int NT, int K, class T>
__device__ __forceinline__ void block_tree_sum(const T (&acc)[K], T* sh) {
#pragma unroll
    for (int k = 0; k < K; k++) sh[k * NT + threadIdx.x] = acc[k];
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if (threadIdx.x < (unsigned)o) {
#pragma unroll
            for (int k = 0; k < K; k++) sh[k * NT + threadIdx.x] += sh[k * NT + threadIdx.x + o];
        }
        __syncthreads();
    }
}

}  // namespace surfel
