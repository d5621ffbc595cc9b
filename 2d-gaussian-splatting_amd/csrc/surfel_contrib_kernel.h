// surfel_contrib_kernel.h — argument block and launcher of the contribution pass (surfel_contrib.hip), shared with the C ABI (surfel_api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "surfel_tile_walk.h"

namespace surfel {

struct ContribArgs {
    WalkFrame frame;                                                        // the forward's buffers
    uint32_t view_tag;                                                      // >= 1, rising from call to call for one accumulator set
    unsigned long long* sum_q; unsigned long long* hits;                    // [P] += rint(w 2^24) | += 1 per composited pair
    uint32_t* max_bits; uint32_t* dominant; uint32_t* views; uint32_t* stamp;      // [P] max of w's bits | += pixels dominated | += 1 per view | last tag seen
    int32_t* dominant_id;                                                   // [H, W] or NULL: this view's heaviest surfel per pixel, -1 = none
    unsigned long long* stats;                                              // optional [8]: [7] += global atomics issued (surfel_debug_set_blend_stats)
};

void launch_contrib(const ContribArgs& a, hipStream_t s);

}  // namespace surfel
