// side_util.h — host helpers shared by the modules beside the rasterizer (mesh, evaluation, metrics, scene, frames, viewer), and the
// exclusive scan of device_scan.hip.
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

// A 64-bit key as two stable LSD sorts of its 32-bit words.  (ka, va) hold the low words and the values; after the first sort
// fill_hi(vals_sorted, keys_out) launches the caller's kernel that writes every sorted slot's high word.  Returns the value buffer of
// the final order (va or vb), or nullptr when a sort fails.
template <class F>
const uint32_t* sort_pairs_two_words(uint32_t* ka, uint32_t* va, uint32_t* kb, uint32_t* vb, int64_t n, int bits_lo, int bits_hi, void* scratch,
                                     hipStream_t st, F fill_hi) {
    int r = radix_sort_pairs_u32(ka, va, kb, vb, (size_t)n, 0, bits_lo, scratch, st);
    if (r < 0) return nullptr;
    if (r) { uint32_t* t = ka; ka = kb; kb = t; t = va; va = vb; vb = t; }
    fill_hi(va, ka);
    r = radix_sort_pairs_u32(ka, va, kb, vb, (size_t)n, 0, bits_hi, scratch, st);
    if (r < 0) return nullptr;
    return r ? vb : va;
}

}  // namespace surfel
