// mesh_raster.h — the clip-free homogeneous rasteriser that mesh_cull.hip (depth images, CULL.md) and mesh_view.hip (visibility buffer,
// MESHVIEW.md) share: one set-up, one pixel test, the two size-class kernels and the host loop over triangle chunks, all templated on the
// pixel type P.  P = uint32_t: the fp32 bits of the nearest z (an integer minimum).  P = uint64_t: (fp32 bits of z) << 32 | triangle
// index, so that the nearest z wins and, among equal bits, the lowest index.  Both files are compiled with -ffp-contract=off (build.py);
// the rasteriser spells its fused multiply-adds out (fmaf), so a pixel gets the same depth bits from either size class and either P.
// wave64; no LDS, no MFMA.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/surfel_cull.h"
#include "side_util.h"

namespace surfel {

constexpr int CT = 256;                          // threads per workgroup
constexpr int CULL_CHUNK = 1 << 18;              // triangles per launch = capacity of a view's queue
constexpr int CULL_LARGE_BLOCKS = 1024;          // workgroups per view that walk a view's queue
constexpr int CULL_TILE = 16;                    // the large class strides a box in CULL_TILE x CULL_TILE steps (CT lanes)
constexpr uint32_t CULL_INF = 0x7f800000u;       // fp32 +inf: the empty depth
constexpr int64_t CULL_MAX_ELEMS = ((int64_t)1 << 31) - 1;

struct CullCam { float m[12]; float fx, fy, cx, cy; };

// e_i(x, y) = a_i (x - cx) + (b_i (y - cy) + c_i) for the three edges and for their sum s, signed so that det > 0; the clamped box
struct CullTri {
    float a0, b0, c0, a1, b1, c1, a2, b2, c2, as, bs, cs, det;
    int x0, x1, y0, y1;
};

__device__ inline CullCam cull_cam(const float* __restrict__ w2c, const float* __restrict__ intrinsics, int n_intrinsics, int view) {
    CullCam c;
#pragma unroll
    for (int k = 0; k < 12; k++) c.m[k] = w2c[12 * (int64_t)view + k];
    const float* q = intrinsics + 4 * (int64_t)(n_intrinsics == 1 ? 0 : view);
    c.fx = q[0]; c.fy = q[1]; c.cx = q[2]; c.cy = q[3];
    return c;
}

// false: the triangle writes nothing in this view (bad index, non-finite, det == 0, outside the depth range, empty box)
__device__ inline bool cull_setup(int64_t t, int64_t V, const float* __restrict__ verts, const int32_t* __restrict__ tris, const CullCam& c, int H,
                                  int W, float znear, float zfar, CullTri& o) {
    const int64_t i0 = tris[3 * t], i1 = tris[3 * t + 1], i2 = tris[3 * t + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= V || i1 >= V || i2 >= V) return false;
    const float px0 = verts[3 * i0], py0 = verts[3 * i0 + 1], pz0 = verts[3 * i0 + 2];
    const float px1 = verts[3 * i1], py1 = verts[3 * i1 + 1], pz1 = verts[3 * i1 + 2];
    const float px2 = verts[3 * i2], py2 = verts[3 * i2 + 1], pz2 = verts[3 * i2 + 2];
    const float* m = c.m;
    const float X0 = ((m[0] * px0 + m[1] * py0) + m[2] * pz0) + m[3], Y0 = ((m[4] * px0 + m[5] * py0) + m[6] * pz0) + m[7],
                Z0 = ((m[8] * px0 + m[9] * py0) + m[10] * pz0) + m[11];
    const float X1 = ((m[0] * px1 + m[1] * py1) + m[2] * pz1) + m[3], Y1 = ((m[4] * px1 + m[5] * py1) + m[6] * pz1) + m[7],
                Z1 = ((m[8] * px1 + m[9] * py1) + m[10] * pz1) + m[11];
    const float X2 = ((m[0] * px2 + m[1] * py2) + m[2] * pz2) + m[3], Y2 = ((m[4] * px2 + m[5] * py2) + m[6] * pz2) + m[7],
                Z2 = ((m[8] * px2 + m[9] * py2) + m[10] * pz2) + m[11];
    if (!(isfinite(X0) && isfinite(Y0) && isfinite(Z0) && isfinite(X1) && isfinite(Y1) && isfinite(Z1) && isfinite(X2) && isfinite(Y2) && isfinite(Z2)))
        return false;
    if ((Z0 < znear && Z1 < znear && Z2 < znear) || (Z0 > zfar && Z1 > zfar && Z2 > zfar)) return false;
    // n0 = v1 x v2, n1 = v2 x v0, n2 = v0 x v1
    const float n0x = Y1 * Z2 - Z1 * Y2, n0y = Z1 * X2 - X1 * Z2, n0z = X1 * Y2 - Y1 * X2;
    const float n1x = Y2 * Z0 - Z2 * Y0, n1y = Z2 * X0 - X2 * Z0, n1z = X2 * Y0 - Y2 * X0;
    const float n2x = Y0 * Z1 - Z0 * Y1, n2y = Z0 * X1 - X0 * Z1, n2z = X0 * Y1 - Y0 * X1;
    const float det = (X0 * n0x + Y0 * n0y) + Z0 * n0z;
    if (!(det != 0.0f) || !isfinite(det)) return false;
    const float sg = det < 0.0f ? -1.0f : 1.0f;
    const float sx = (n0x + n1x) + n2x, sy = (n0y + n1y) + n2y, sz = (n0z + n1z) + n2z;
    o.det = sg * det;
    o.a0 = sg * (n0x / c.fx); o.b0 = sg * (n0y / c.fy); o.c0 = sg * n0z;
    o.a1 = sg * (n1x / c.fx); o.b1 = sg * (n1y / c.fy); o.c1 = sg * n1z;
    o.a2 = sg * (n2x / c.fx); o.b2 = sg * (n2y / c.fy); o.c2 = sg * n2z;
    o.as = sg * (sx / c.fx); o.bs = sg * (sy / c.fy); o.cs = sg * sz;
    if (Z0 >= znear && Z1 >= znear && Z2 >= znear) {
        // the projected box, one pixel wider on every side, clamped (the float clamp comes first: the conversion sees small values only)
        const float u0 = c.fx * (X0 / Z0) + c.cx, u1 = c.fx * (X1 / Z1) + c.cx, u2 = c.fx * (X2 / Z2) + c.cx;
        const float v0 = c.fy * (Y0 / Z0) + c.cy, v1 = c.fy * (Y1 / Z1) + c.cy, v2 = c.fy * (Y2 / Z2) + c.cy;
        const float ulo = fminf(fmaxf(fminf(fminf(u0, u1), u2), -2.0f), (float)W + 1.0f), uhi = fminf(fmaxf(fmaxf(fmaxf(u0, u1), u2), -2.0f), (float)W + 1.0f);
        const float vlo = fminf(fmaxf(fminf(fminf(v0, v1), v2), -2.0f), (float)H + 1.0f), vhi = fminf(fmaxf(fmaxf(fmaxf(v0, v1), v2), -2.0f), (float)H + 1.0f);
        o.x0 = max((int)ceilf(ulo) - 1, 0); o.x1 = min((int)floorf(uhi) + 1, W - 1);
        o.y0 = max((int)ceilf(vlo) - 1, 0); o.y1 = min((int)floorf(vhi) + 1, H - 1);
    } else {      // crosses the near plane (or the eye plane): the projection bounds nothing, so the whole image
        o.x0 = 0; o.x1 = W - 1; o.y0 = 0; o.y1 = H - 1;
    }
    return o.x1 >= o.x0 && o.y1 >= o.y0;
}

// The pixel sinks.  The plain read in front of the atomic only saves atomics: depths only fall, so a stale value that is already not
// above z proves the same of the current one.
__device__ inline void cull_sink(uint32_t* p, uint32_t bits, uint32_t) {
    if (bits < *p) atomicMin(p, bits);
}

// The read compares the depth half alone (the upper word of the little-endian key): skip only when the stored depth is strictly below
// z.  At equal depth bits the atomic decides, so the lowest triangle index wins whatever the order of arrival.
__device__ inline void cull_sink(uint64_t* p, uint32_t bits, uint32_t tri) {
    if (!(reinterpret_cast<const uint32_t*>(p)[1] < bits))
        atomicMin(reinterpret_cast<unsigned long long*>(p), (unsigned long long)bits << 32 | tri);
}

// one sample: px = x - cx, r_i = b_i (y - cy) + c_i of the row
template <class P>
__device__ inline void cull_pixel(const CullTri& t, float px, float r0, float r1, float r2, float rs, float znear, float zfar, P* p, uint32_t tri) {
    const float e0 = fmaf(t.a0, px, r0), e1 = fmaf(t.a1, px, r1), e2 = fmaf(t.a2, px, r2);
    if (e0 >= 0.0f && e1 >= 0.0f && e2 >= 0.0f) {
        const float s = fmaf(t.as, px, rs);
        if (s > 0.0f) {
            const float z = t.det / s;
            if (z >= znear && z <= zfar) cull_sink(p, __float_as_uint(z), tri);
        }
    }
}

// grid (triangle blocks of the chunk, views).  One lane per (triangle, view): set-up, then either the box itself (small class) or one queue
// slot (large class, one counter bump per wave).
template <class P>
__global__ void __launch_bounds__(CT) cull_small_kernel(int64_t V, int64_t t0, int tcount, const float* __restrict__ verts, const int32_t* __restrict__ tris,
                                                        const float* __restrict__ w2c, const float* __restrict__ intrinsics, int n_intrinsics, int H, int W,
                                                        float znear, float zfar, int small_pixels, P* depth, int32_t* __restrict__ queue,
                                                        uint32_t* qcount) {
    const int view = blockIdx.y;
    const int k = blockIdx.x * CT + threadIdx.x;
    const CullCam cam = cull_cam(w2c, intrinsics, n_intrinsics, view);
    CullTri t;
    bool large = false;
    if (k < tcount && cull_setup(t0 + k, V, verts, tris, cam, H, W, znear, zfar, t)) {
        const int bw = t.x1 - t.x0 + 1, bh = t.y1 - t.y0 + 1;
        if ((int64_t)bw * bh > small_pixels) {
            large = true;
        } else {
            P* img = depth + (int64_t)view * H * W;
            const uint32_t id = (uint32_t)(t0 + k);
            for (int y = t.y0; y <= t.y1; y++) {
                const float py = (float)y - cam.cy;
                const float r0 = fmaf(t.b0, py, t.c0), r1 = fmaf(t.b1, py, t.c1), r2 = fmaf(t.b2, py, t.c2), rs = fmaf(t.bs, py, t.cs);
                for (int x = t.x0; x <= t.x1; x++) cull_pixel(t, (float)x - cam.cx, r0, r1, r2, rs, znear, zfar, img + (int64_t)y * W + x, id);
            }
        }
    }
    const unsigned long long wave = __ballot(large);
    if (large) {
        const int lane = threadIdx.x & 63, leader = __ffsll((long long)wave) - 1;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(qcount + view, (uint32_t)__popcll(wave));
        base = __shfl(base, leader);
        const uint32_t slot = base + (uint32_t)__popcll(wave & ((1ull << lane) - 1ull));
        if (slot < (uint32_t)tcount) queue[(int64_t)view * CULL_CHUNK + slot] = k;      // (always: a view queues each triangle at most once)
    }
}

// grid (CULL_LARGE_BLOCKS, views).  A workgroup takes every gridDim.x-th entry of its view's queue, sets the triangle up again and strides
// its box in CULL_TILE x CULL_TILE steps.
template <class P>
__global__ void __launch_bounds__(CT) cull_large_kernel(int64_t V, int64_t t0, int tcount, const float* __restrict__ verts, const int32_t* __restrict__ tris,
                                                        const float* __restrict__ w2c, const float* __restrict__ intrinsics, int n_intrinsics, int H, int W,
                                                        float znear, float zfar, P* depth, const int32_t* __restrict__ queue,
                                                        const uint32_t* __restrict__ qcount) {
    const int view = blockIdx.y;
    const uint32_t n = min(qcount[view], (uint32_t)tcount);
    if (blockIdx.x >= n) return;
    const CullCam cam = cull_cam(w2c, intrinsics, n_intrinsics, view);
    P* img = depth + (int64_t)view * H * W;
    const int tx = threadIdx.x & (CULL_TILE - 1), ty = threadIdx.x / CULL_TILE;
    for (uint32_t q = blockIdx.x; q < n; q += gridDim.x) {
        const int k = queue[(int64_t)view * CULL_CHUNK + q];
        CullTri t;
        if (k < 0 || k >= tcount || !cull_setup(t0 + k, V, verts, tris, cam, H, W, znear, zfar, t)) continue;
        const uint32_t id = (uint32_t)(t0 + k);
        for (int y = t.y0 + ty; y <= t.y1; y += CULL_TILE) {
            const float py = (float)y - cam.cy;
            const float r0 = fmaf(t.b0, py, t.c0), r1 = fmaf(t.b1, py, t.c1), r2 = fmaf(t.b2, py, t.c2), rs = fmaf(t.bs, py, t.cs);
            for (int x = t.x0 + tx; x <= t.x1; x += CULL_TILE) cull_pixel(t, (float)x - cam.cx, r0, r1, r2, rs, znear, zfar, img + (int64_t)y * W + x, id);
        }
    }
}

inline bool cull_bad_cameras(int nviews, const float* w2c, const float* intrinsics, int n_intrinsics) {
    return nviews < 0 || (nviews > 0 && (!w2c || !intrinsics)) || (n_intrinsics != 1 && n_intrinsics != nviews);
}

// The host side of one call, behind the caller's argument checks: the queues from the caller's allocator, `init(img)` (every pixel
// empty), per chunk of CULL_CHUNK triangles the counters' reset and the two class launches, then `resolve(img)`.  init and resolve
// enqueue on st and return 0 or a negative code.  stage_ms (HOST, may be NULL): the launches are timed with events, the call
// synchronises and returns the number of (view, triangle) pairs of the large class; otherwise 0, without synchronising.  `what` names the
// entry point in error messages.
template <class P, class Init, class Resolve>
int64_t cull_rasterise(const char* what, surfel_alloc_fn alloc, void* user, int64_t V, int64_t F, const float* verts, const int32_t* tris, int nviews,
                       const float* w2c, const float* intrinsics, int n_intrinsics, int H, int W, float znear, float zfar, int small_pixels, P* img,
                       float* stage_ms, hipStream_t st, Init init, Resolve resolve) {
    const int small = small_pixels < 0 ? SURFEL_CULL_SMALL_PIXELS : small_pixels;
    int32_t* queue = nullptr;
    uint32_t* qcount = nullptr;
    if (F > 0) {
        const int64_t cap = F < CULL_CHUNK ? F : CULL_CHUNK;
        // one buffer: the counters of every view (padded to 64 words), then a queue of CULL_CHUNK slots per view (the last one cut to cap)
        const int64_t head = ((int64_t)nviews + 63) / 64 * 64;
        uint32_t* buf = static_cast<uint32_t*>(alloc(user, (size_t)(head + (int64_t)(nviews - 1) * CULL_CHUNK + cap) * 4));
        if (!buf) return api_fail(SURFEL_E_ALLOC, what, hipSuccess);
        qcount = buf;
        queue = reinterpret_cast<int32_t*>(buf + head);
    }
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    if (stage_ms)
        for (auto& e : ev)
            if (hipEventCreate(&e) != hipSuccess) return api_fail(SURFEL_E_HIP, what, hipGetLastError());
    auto mark = [&](int k) { if (stage_ms) (void)hipEventRecord(ev[k], st); };
    auto lap = [&](int stage, int a, int b) {
        float ms = 0.0f;
        if (stage_ms && hipEventSynchronize(ev[b]) == hipSuccess && hipEventElapsedTime(&ms, ev[a], ev[b]) == hipSuccess) stage_ms[stage] += ms;
    };
    int64_t queued = 0;
    int rc = 0;
    mark(0);
    rc = init(img);
    mark(1);
    lap(2, 0, 1);
    for (int64_t t0 = 0; t0 < F && rc == 0; t0 += CULL_CHUNK) {
        const int tcount = (int)(F - t0 < CULL_CHUNK ? F - t0 : CULL_CHUNK);
        if (hipMemsetAsync(qcount, 0, (size_t)nviews * 4, st) != hipSuccess) {
            rc = api_fail(SURFEL_E_HIP, what, hipGetLastError());
            break;
        }
        mark(0);
        hipLaunchKernelGGL(cull_small_kernel<P>, dim3(blocks_for(tcount, CT), (unsigned)nviews), dim3(CT), 0, st, V, t0, tcount, verts, tris, w2c,
                           intrinsics, n_intrinsics, H, W, znear, zfar, small, img, queue, qcount);
        mark(1);
        const unsigned nb = (unsigned)(tcount < CULL_LARGE_BLOCKS ? tcount : CULL_LARGE_BLOCKS);
        hipLaunchKernelGGL(cull_large_kernel<P>, dim3(nb, (unsigned)nviews), dim3(CT), 0, st, V, t0, tcount, verts, tris, w2c, intrinsics, n_intrinsics,
                           H, W, znear, zfar, img, queue, qcount);
        mark(2);
        rc = launched("cull_large_kernel");
        if (stage_ms && rc == 0) {
            lap(0, 0, 1);
            lap(1, 1, 2);
            for (int v = 0; v < nviews; v++) {
                uint32_t c = 0;
                if (hipMemcpyAsync(&c, qcount + v, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
                    rc = api_fail(SURFEL_E_HIP, what, hipGetLastError());
                    break;
                }
                queued += c;
            }
        }
    }
    if (rc == 0) {
        mark(2);
        rc = resolve(img);
        mark(3);
        lap(2, 2, 3);
    }
    if (stage_ms) {
        if (rc == 0 && hipStreamSynchronize(st) != hipSuccess) rc = api_fail(SURFEL_E_HIP, what, hipGetLastError());
        for (auto& e : ev) (void)hipEventDestroy(e);
    }
    return rc < 0 ? rc : queued;
}

}  // namespace surfel
