// vis_pixels.h — what the frame kernels (frame_vis.hip) and the viewer's image kernels (view_image.hip) share: four pixels in, their
// interleaved bytes out, and the order-preserving 32-bit key of a float.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace surfel {

constexpr int PX = 4;        // consecutive pixels per lane: 16 B of every plane in, 4 C bytes out

// save_img_u8's arithmetic on one value (fp32, one rounding per operation); also the quantiser of the mesh viewer's shading (mesh_view.hip)
__device__ __forceinline__ uint32_t quant8(float v, float scale, float bias) {
    float y = __fadd_rn(__fmul_rn(v, scale), bias);
    if (y != y) y = 0.0f;                      // nan_to_num: NaN -> 0 (+-inf -> +-FLT_MAX, which the clip treats as it treats +-inf)
    y = y < 0.0f ? 0.0f : (y > 1.0f ? 1.0f : y);
    return (uint32_t)(int)__fmul_rn(y, 255.0f);
}

// ---- 4 pixels in, 4 C bytes out --------------------------------------------------------------------------------------------------------
// v[0..3] <- p[i .. i + 3]: one 16-byte load where the address allows it (the same answer for every lane of a plane: lanes are 16 B
// apart), four 4-byte loads otherwise; nothing at or behind p[n] is read
__device__ __forceinline__ void load4(const float* __restrict__ p, int64_t i, int64_t n, float (&v)[PX]) {
    const float* q = p + i;
    if (i + PX <= n && (reinterpret_cast<uintptr_t>(q) & 15) == 0) {
        const float4 f = *reinterpret_cast<const float4*>(q);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    } else {
#pragma unroll
        for (int j = 0; j < PX; j++) v[j] = i + j < n ? q[j] : 0.0f;
    }
}

// the first nbytes (<= 4 NW) bytes of the little-endian words w[] to q: whole dwords where q is 4-byte aligned and all bytes are there;
// otherwise the bytes up to the next dword boundary one by one, then whole dwords cut out of w[] at that byte offset, then the rest
// one by one.  Nothing outside [q, q + nbytes) is written.
template <int NW>
__device__ __forceinline__ void store_bytes(uint8_t* __restrict__ q, int nbytes, const uint32_t (&w)[NW]) {
    const int a = (int)(reinterpret_cast<uintptr_t>(q) & 3);
    if (a == 0 && nbytes == 4 * NW) {
#pragma unroll
        for (int k = 0; k < NW; k++) reinterpret_cast<uint32_t*>(q)[k] = w[k];
        return;
    }
    const int head = min((4 - a) & 3, nbytes);
    const int nd = (nbytes - head) >> 2;
#pragma unroll
    for (int k = 0; k < NW; k++) {
        const uint64_t pair = (uint64_t)w[k] | ((uint64_t)(k + 1 < NW ? w[k + 1] : 0u) << 32);
        if (k < nd) *reinterpret_cast<uint32_t*>(q + head + 4 * k) = (uint32_t)(pair >> (8 * head));
    }
#pragma unroll
    for (int b = 0; b < 4 * NW; b++)
        if (b < nbytes && (b < head || b >= head + 4 * nd)) q[b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
}

// ---- the order-preserving key ----------------------------------------------------------------------------------------------------------
// key: unsigned order = numpy's sort order of the floats (every NaN is the largest key; -0 sorts directly below +0)
__device__ __forceinline__ uint32_t order_key(float v) {
    const uint32_t u = __float_as_uint(v);
    if (v != v) return 0xffffffffu;
    return (u >> 31) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float order_value(uint32_t key) {
    if (key == 0xffffffffu) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((key >> 31) ? (key ^ 0x80000000u) : ~key);
}

}  // namespace surfel
