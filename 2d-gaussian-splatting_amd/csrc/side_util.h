// side_util.h — helpers shared by the modules beside the rasterizer (mesh, evaluation, metrics, scene, frames, viewer): launch, allocation
// and read-back on the host, the exclusive scan of device_scan.hip with the test that reads its result, and the sort workspace with the
// stable sort on a key of several words.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/surfel_hip.h"
#include "surfel_kernels.h"
#include "train_kernels.h"

namespace surfel {

// device_scan.hip: exclusive scan of a[n] (u32) in place, three launches; the total lands in scratch[scan_scratch_u32(n) - 1]
constexpr int SCAN_TILE = 4096;      // elements per scan tile
int64_t scan_scratch_u32(int64_t n);      // scratch words for n elements: one per tile and the total
void scan_u32(uint32_t* a, int64_t n, uint32_t* scratch, hipStream_t st);

inline int launched(const char* what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_fail(SURFEL_E_HIP, what, e);
}

inline unsigned blocks_for(int64_t n, int64_t per_block) { return (unsigned)((n + per_block - 1) / per_block); }

template <class T>
T* take(surfel_alloc_fn alloc, void* user, int64_t n) { return static_cast<T*>(alloc(user, (size_t)(n > 0 ? n : 1) * sizeof(T))); }

inline int bit_length(uint64_t v) { int b = 0; while (v) { b++; v >>= 1; } return b; }

// n 32-bit words device -> host on st, then the wait for the stream; wait = false leaves the wait to the next read
inline int read_words(const char* what, const void* dev, void* host, int64_t n, hipStream_t st, bool wait = true) {
    if (hipMemcpyAsync(host, dev, (size_t)n * 4, hipMemcpyDeviceToHost, st) != hipSuccess || (wait && hipStreamSynchronize(st) != hipSuccess))
        return api_fail(SURFEL_E_HIP, what, hipGetLastError());
    return 0;
}

// n flags and the words scan_u32 needs for them: scan() turns the flags into exclusive positions in place and leaves their sum in *total
struct ScanBuf {
    uint32_t* flags = nullptr; uint32_t* sums = nullptr; uint32_t* total = nullptr;
    int64_t n = 0;
    ScanBuf() = default;
    ScanBuf(uint32_t* f, uint32_t* s, int64_t n_) : flags(f), sums(s), total(s + scan_scratch_u32(n_) - 1), n(n_) {}
    static int64_t words(int64_t n) { return n + scan_scratch_u32(n); }      // flags | sums, as take_scan lays them out
    void scan(hipStream_t st) const { scan_u32(flags, n, sums, st); }
};

// one allocation: flags[n] | sums | extra_words behind the total (at total + 1); flags is null when the allocator fails
inline ScanBuf take_scan(surfel_alloc_fn alloc, void* user, int64_t n, int64_t extra_words = 0) {
    uint32_t* p = take<uint32_t>(alloc, user, ScanBuf::words(n) + extra_words);
    return p ? ScanBuf(p, p + n, n) : ScanBuf();
}

// after scan(): was element i of the n flagged (pos = the scanned flags)
__device__ __forceinline__ bool scanned_flag(const uint32_t* __restrict__ pos, const uint32_t* __restrict__ total, int64_t i, int64_t n) {
    return (i + 1 < n ? pos[i + 1] : *total) != pos[i];
}

// Two key / value buffer pairs for n pairs and the sort's scratch.  The caller fills (ka, va); after sort() (ka, va) name the sorted
// pairs, whichever buffers the last pass wrote.
struct SortPairs {
    uint32_t *ka, *va, *kb, *vb;
    void* scratch;
    int64_t n;
    SortPairs(surfel_alloc_fn alloc, void* user, int64_t n_)
        : ka(take<uint32_t>(alloc, user, n_)), va(take<uint32_t>(alloc, user, n_)), kb(take<uint32_t>(alloc, user, n_)),
          vb(take<uint32_t>(alloc, user, n_)), scratch(alloc(user, radix_sort_scratch_bytes((size_t)n_))), n(n_) {}
    bool ok() const { return ka && va && kb && vb && scratch; }
    // stable, on key bits [0, bits), bits held to 1 .. 32; negative when the sort fails
    int sort(int bits, hipStream_t st) {
        const int r = radix_sort_pairs_u32(ka, va, kb, vb, (size_t)n, 0, bits < 1 ? 1 : bits > 32 ? 32 : bits, scratch, st);
        if (r > 0) { uint32_t* t = ka; ka = kb; kb = t; t = va; va = vb; vb = t; }
        return r < 0 ? r : 0;
    }
};

// A stable sort on a key of several 32-bit words, least significant first.  KeyOf is a small struct of pointers with
// __device__ uint32_t operator()(uint32_t value, int word) const: word `word` of the key of the element a pair's value names.
constexpr int REKEY_T = 256;      // threads per workgroup

__device__ __forceinline__ uint32_t key_word(uint64_t key, int word) { return (uint32_t)(key >> (32 * word)); }

template <class KeyOf>
__global__ void __launch_bounds__(REKEY_T) rekey_kernel(int64_t n, const uint32_t* __restrict__ val, uint32_t* __restrict__ key, KeyOf key_of, int word) {
    const int64_t j = (int64_t)blockIdx.x * REKEY_T + threadIdx.x;
    if (j < n) key[j] = key_of(val[j], word);
}

// The caller has filled (s.ka, s.va) with word 0 of every key and its value.  Word w is sorted on bits[w] bits; the words above 0 are
// written from the values by one launch each.  Fails with SURFEL_E_LIMIT and `what`.
template <class KeyOf>
int sort_words(SortPairs& s, KeyOf key_of, int words, const int* bits, const char* what, hipStream_t st) {
    if (s.n <= 0) return 0;
    for (int w = 0; w < words; w++) {
        if (w > 0) hipLaunchKernelGGL(rekey_kernel<KeyOf>, dim3(blocks_for(s.n, REKEY_T)), dim3(REKEY_T), 0, st, s.n, s.va, s.ka, key_of, w);
        if (s.sort(bits[w], st) < 0) return api_fail(SURFEL_E_LIMIT, what);
    }
    return 0;
}

}  // namespace surfel
