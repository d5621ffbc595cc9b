// surfel_select_kernel.h — argument block and launcher of the label pass (surfel_select.hip), shared with the C ABI (surfel_api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace surfel {

constexpr int SELECT_MAX_LABELS = 32;

struct SelectArgs {
    int W, H, gx, gy;
    const uint2* ranges; const uint32_t* point_list; const float* rec;      // the forward's tile lists and surfel records
    const int* tile_map; const uint32_t* map_flag; int map_len;             // as ContribArgs: the forward's tile order, the grid size
    const uint8_t* labels;                                                  // [H, W]: the pixel's label; >= K = ignored
    int K;                                                                  // 1 .. SELECT_MAX_LABELS
    unsigned long long* votes;                                              // [P, K] += rint(w 2^24) of the pairs composited at pixels of label k
    unsigned long long* stats;                                              // optional [8]: [7] += global atomics issued (surfel_debug_set_blend_stats)
};

void launch_select(const SelectArgs& a, hipStream_t s);

}  // namespace surfel
