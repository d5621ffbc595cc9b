// surfel_select_kernel.h — argument block and launcher of the label pass (surfel_select.hip), shared with the C ABI (surfel_api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "surfel_tile_walk.h"

namespace surfel {

constexpr int SELECT_MAX_LABELS = 32;

struct SelectArgs {
    WalkFrame frame;                                                        // the forward's buffers
    const uint8_t* labels;                                                  // [H, W]: the pixel's label; >= K = ignored
    int K;                                                                  // 1 .. SELECT_MAX_LABELS
    unsigned long long* votes;                                              // [P, K] += rint(w 2^24) of the pairs composited at pixels of label k
    unsigned long long* stats;                                              // optional [8]: [7] += global atomics issued (surfel_debug_set_blend_stats)
};

void launch_select(const SelectArgs& a, hipStream_t s);

}  // namespace surfel
