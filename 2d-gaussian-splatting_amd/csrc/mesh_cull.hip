// mesh_cull.hip — view culling of a mesh: depth images of a triangle mesh for a batch of views (a clip-free homogeneous rasteriser with an
// integer-minimum depth buffer) and the per-vertex view count of the reference's Mesher.point_masks (include/surfel_cull.h, CULL.md).
// Compiled with -ffp-contract=off (build.py): the visibility kernel rounds exactly as its restatement in tests/cull_oracle.py; the
// rasteriser spells its fused multiply-adds out (fmaf), so a pixel gets the same bits from either size class.  wave64; no LDS, no MFMA.
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

// one sample: px = x - cx, r_i = b_i (y - cy) + c_i of the row.  The plain read in front of the atomic only saves atomics: depths only
// fall, so a stale value that is already not above z proves the same of the current one.
__device__ inline void cull_pixel(const CullTri& t, float px, float r0, float r1, float r2, float rs, float znear, float zfar, uint32_t* p) {
    const float e0 = fmaf(t.a0, px, r0), e1 = fmaf(t.a1, px, r1), e2 = fmaf(t.a2, px, r2);
    if (e0 >= 0.0f && e1 >= 0.0f && e2 >= 0.0f) {
        const float s = fmaf(t.as, px, rs);
        if (s > 0.0f) {
            const float z = t.det / s;
            if (z >= znear && z <= zfar) {
                const uint32_t bits = __float_as_uint(z);
                if (bits < *p) atomicMin(p, bits);
            }
        }
    }
}

// grid (triangle blocks of the chunk, views).  One lane per (triangle, view): set-up, then either the box itself (small class) or one queue
// slot (large class, one counter bump per wave).
__global__ void __launch_bounds__(CT) cull_small_kernel(int64_t V, int64_t t0, int tcount, const float* __restrict__ verts, const int32_t* __restrict__ tris,
                                                        const float* __restrict__ w2c, const float* __restrict__ intrinsics, int n_intrinsics, int H, int W,
                                                        float znear, float zfar, int small_pixels, uint32_t* depth, int32_t* __restrict__ queue,
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
            uint32_t* img = depth + (int64_t)view * H * W;
            for (int y = t.y0; y <= t.y1; y++) {
                const float py = (float)y - cam.cy;
                const float r0 = fmaf(t.b0, py, t.c0), r1 = fmaf(t.b1, py, t.c1), r2 = fmaf(t.b2, py, t.c2), rs = fmaf(t.bs, py, t.cs);
                for (int x = t.x0; x <= t.x1; x++) cull_pixel(t, (float)x - cam.cx, r0, r1, r2, rs, znear, zfar, img + (int64_t)y * W + x);
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
__global__ void __launch_bounds__(CT) cull_large_kernel(int64_t V, int64_t t0, int tcount, const float* __restrict__ verts, const int32_t* __restrict__ tris,
                                                        const float* __restrict__ w2c, const float* __restrict__ intrinsics, int n_intrinsics, int H, int W,
                                                        float znear, float zfar, uint32_t* depth, const int32_t* __restrict__ queue,
                                                        const uint32_t* __restrict__ qcount) {
    const int view = blockIdx.y;
    const uint32_t n = min(qcount[view], (uint32_t)tcount);
    if (blockIdx.x >= n) return;
    const CullCam cam = cull_cam(w2c, intrinsics, n_intrinsics, view);
    uint32_t* img = depth + (int64_t)view * H * W;
    const int tx = threadIdx.x & (CULL_TILE - 1), ty = threadIdx.x / CULL_TILE;
    for (uint32_t q = blockIdx.x; q < n; q += gridDim.x) {
        const int k = queue[(int64_t)view * CULL_CHUNK + q];
        CullTri t;
        if (k < 0 || k >= tcount || !cull_setup(t0 + k, V, verts, tris, cam, H, W, znear, zfar, t)) continue;
        for (int y = t.y0 + ty; y <= t.y1; y += CULL_TILE) {
            const float py = (float)y - cam.cy;
            const float r0 = fmaf(t.b0, py, t.c0), r1 = fmaf(t.b1, py, t.c1), r2 = fmaf(t.b2, py, t.c2), rs = fmaf(t.bs, py, t.cs);
            for (int x = t.x0 + tx; x <= t.x1; x += CULL_TILE) cull_pixel(t, (float)x - cam.cx, r0, r1, r2, rs, znear, zfar, img + (int64_t)y * W + x);
        }
    }
}

__global__ void __launch_bounds__(CT) cull_resolve_kernel(int64_t n, uint32_t* depth) {
    const int64_t i = (int64_t)blockIdx.x * CT + threadIdx.x;
    if (i < n && depth[i] == CULL_INF) depth[i] = 0u;
}

// ---- the per-vertex view count (Mesher.point_masks) ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(CT) cull_visibility_kernel(int64_t N, const float* __restrict__ points, int nviews, const float* __restrict__ w2c,
                                                             const float* __restrict__ intrinsics, int n_intrinsics, int H, int W,
                                                             const float* __restrict__ depth, float eps, int32_t* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * CT + threadIdx.x;
    if (i >= N) return;
    const float x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
    const float wm = (float)(W - 1), hm = (float)(H - 1);
    int count = 0;
    for (int view = 0; view < nviews; view++) {
        const float* m = w2c + 12 * (int64_t)view;
        const float* q = intrinsics + 4 * (int64_t)(n_intrinsics == 1 ? 0 : view);
        const float X = ((m[0] * x + m[1] * y) + m[2] * z) + m[3], Y = ((m[4] * x + m[5] * y) + m[6] * z) + m[7], Z = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
        const float zz = Z + 1e-8f;
        const float u = (q[0] * X + q[2] * Z) / zz, v = (q[1] * Y + q[3] * Z) / zz;
        if (!(u >= 0.0f && u <= wm && v >= 0.0f && v <= hm && zz > 0.0f)) continue;      // (false for NaN: nothing non-finite indexes below)
        // grid_sample(padding_mode = 'border', align_corners = True) at the normalised (u, v): the round trip, the clip, four corners
        const float gx = u / wm * 2.0f - 1.0f, gy = v / hm * 2.0f - 1.0f;
        const float ix = fminf(wm, fmaxf(((gx + 1.0f) / 2.0f) * wm, 0.0f)), iy = fminf(hm, fmaxf(((gy + 1.0f) / 2.0f) * hm, 0.0f));
        const float fx0 = floorf(ix), fy0 = floorf(iy), fx1 = fx0 + 1.0f, fy1 = fy0 + 1.0f;
        const int x0 = (int)fx0, y0 = (int)fy0, x1 = x0 + 1, y1 = y0 + 1;
        const float nw = (fx1 - ix) * (fy1 - iy), ne = (ix - fx0) * (fy1 - iy), sw = (fx1 - ix) * (iy - fy0), se = (ix - fx0) * (iy - fy0);
        const float* img = depth + (int64_t)view * H * W;
        float sample = 0.0f;      // x0, y0 lie inside (clipped); x1, y1 may be W, H, where torch adds nothing
        sample += img[(int64_t)y0 * W + x0] * nw;
        if (x1 < W) sample += img[(int64_t)y0 * W + x1] * ne;
        if (y1 < H) sample += img[(int64_t)y1 * W + x0] * sw;
        if (x1 < W && y1 < H) sample += img[(int64_t)y1 * W + x1] * se;
        const bool front = sample > 0.0f ? zz < sample + eps : true;
        count += front;
    }
    counts[i] += count;
}

namespace {
inline unsigned grid(int64_t n) { return blocks_for(n, CT); }
constexpr int64_t CULL_MAX_ELEMS = ((int64_t)1 << 31) - 1;

bool bad_cameras(int nviews, const float* w2c, const float* intrinsics, int n_intrinsics) {
    return nviews < 0 || (nviews > 0 && (!w2c || !intrinsics)) || (n_intrinsics != 1 && n_intrinsics != nviews);
}
}  // namespace

extern "C" {

int64_t surfel_cull_mesh_depth(surfel_alloc_fn alloc, void* user, int64_t V, int64_t F, const float* verts, const int32_t* tris, int nviews,
                               const float* w2c, const float* intrinsics, int n_intrinsics, int H, int W, float znear, float zfar,
                               int small_pixels, float* depth, float* stage_ms, void* stream) {
    if (!alloc || V < 0 || F < 0 || (V > 0 && !verts) || (F > 0 && !tris) || bad_cameras(nviews, w2c, intrinsics, n_intrinsics) || H < 1 || W < 1 ||
        !(znear > 0.0f) || !(zfar >= znear) || !(zfar < INFINITY) || (nviews > 0 && !depth))
        return api_fail(SURFEL_E_INVALID, "cull_mesh_depth: bad arguments");
    if (V > CULL_MAX_ELEMS || F > CULL_MAX_ELEMS || (int64_t)H * W > CULL_MAX_ELEMS)
        return api_fail(SURFEL_E_LIMIT, "cull_mesh_depth: more than 2^31 - 1 vertices, triangles or pixels");
    if (nviews > SURFEL_CULL_MAX_VIEWS) return api_fail(SURFEL_E_LIMIT, "cull_mesh_depth: more than SURFEL_CULL_MAX_VIEWS views in one call");
    if (stage_ms) for (int k = 0; k < SURFEL_CULL_STAGES; k++) stage_ms[k] = 0.0f;
    if (nviews == 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t pixels = (int64_t)nviews * H * W;
    const int small = small_pixels < 0 ? SURFEL_CULL_SMALL_PIXELS : small_pixels;
    uint32_t* img = reinterpret_cast<uint32_t*>(depth);
    int32_t* queue = nullptr;
    uint32_t* qcount = nullptr;
    if (F > 0) {
        const int64_t cap = F < CULL_CHUNK ? F : CULL_CHUNK;
        // one buffer: the counters of every view (padded to 64 words), then a queue of CULL_CHUNK slots per view (the last one cut to cap)
        const int64_t head = ((int64_t)nviews + 63) / 64 * 64;
        uint32_t* buf = static_cast<uint32_t*>(alloc(user, (size_t)(head + (int64_t)(nviews - 1) * CULL_CHUNK + cap) * 4));
        if (!buf) return api_fail(SURFEL_E_ALLOC, "cull_mesh_depth: allocator returned NULL");
        qcount = buf;
        queue = reinterpret_cast<int32_t*>(buf + head);
    }
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    if (stage_ms)
        for (auto& e : ev)
            if (hipEventCreate(&e) != hipSuccess) return api_fail(SURFEL_E_HIP, "cull_mesh_depth: event", hipGetLastError());
    auto mark = [&](int k) { if (stage_ms) (void)hipEventRecord(ev[k], st); };
    auto lap = [&](int stage, int a, int b) {
        float ms = 0.0f;
        if (stage_ms && hipEventSynchronize(ev[b]) == hipSuccess && hipEventElapsedTime(&ms, ev[a], ev[b]) == hipSuccess) stage_ms[stage] += ms;
    };
    int64_t queued = 0;
    int rc = 0;
    mark(0);
    if (hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(img), (int)CULL_INF, (size_t)pixels, st) != hipSuccess)
        rc = api_fail(SURFEL_E_HIP, "cull_mesh_depth: memset", hipGetLastError());
    mark(1);
    lap(2, 0, 1);
    for (int64_t t0 = 0; t0 < F && rc == 0; t0 += CULL_CHUNK) {
        const int tcount = (int)(F - t0 < CULL_CHUNK ? F - t0 : CULL_CHUNK);
        if (hipMemsetAsync(qcount, 0, (size_t)nviews * 4, st) != hipSuccess) {
            rc = api_fail(SURFEL_E_HIP, "cull_mesh_depth: memset", hipGetLastError());
            break;
        }
        mark(0);
        hipLaunchKernelGGL(cull_small_kernel, dim3(grid(tcount), (unsigned)nviews), dim3(CT), 0, st, V, t0, tcount, verts, tris, w2c, intrinsics,
                           n_intrinsics, H, W, znear, zfar, small, img, queue, qcount);
        mark(1);
        const unsigned nb = (unsigned)(tcount < CULL_LARGE_BLOCKS ? tcount : CULL_LARGE_BLOCKS);
        hipLaunchKernelGGL(cull_large_kernel, dim3(nb, (unsigned)nviews), dim3(CT), 0, st, V, t0, tcount, verts, tris, w2c, intrinsics, n_intrinsics, H,
                           W, znear, zfar, img, queue, qcount);
        mark(2);
        rc = launched("cull_large_kernel");
        if (stage_ms && rc == 0) {
            lap(0, 0, 1);
            lap(1, 1, 2);
            for (int v = 0; v < nviews; v++) {
                uint32_t c = 0;
                if (hipMemcpyAsync(&c, qcount + v, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
                    rc = api_fail(SURFEL_E_HIP, "cull_mesh_depth: copy", hipGetLastError());
                    break;
                }
                queued += c;
            }
        }
    }
    if (rc == 0) {
        mark(2);
        hipLaunchKernelGGL(cull_resolve_kernel, dim3(grid(pixels)), dim3(CT), 0, st, pixels, img);
        mark(3);
        rc = launched("cull_resolve_kernel");
        lap(2, 2, 3);
    }
    if (stage_ms) {
        if (rc == 0 && hipStreamSynchronize(st) != hipSuccess) rc = api_fail(SURFEL_E_HIP, "cull_mesh_depth: synchronize", hipGetLastError());
        for (auto& e : ev) (void)hipEventDestroy(e);
    }
    return rc < 0 ? rc : queued;
}

int surfel_cull_visibility(int64_t N, const float* points, int nviews, const float* w2c, const float* intrinsics, int n_intrinsics, int H, int W,
                           const float* depth, float eps, int32_t* counts, void* stream) {
    if (N < 0 || (N > 0 && (!points || !counts)) || bad_cameras(nviews, w2c, intrinsics, n_intrinsics) || H < 2 || W < 2 || (nviews > 0 && !depth) ||
        !(eps == eps))
        return api_fail(SURFEL_E_INVALID, "cull_visibility: bad arguments");
    if (N > CULL_MAX_ELEMS || (int64_t)H * W > CULL_MAX_ELEMS) return api_fail(SURFEL_E_LIMIT, "cull_visibility: more than 2^31 - 1 points or pixels");
    if (N == 0 || nviews == 0) return 0;
    hipLaunchKernelGGL(cull_visibility_kernel, dim3(grid(N)), dim3(CT), 0, static_cast<hipStream_t>(stream), N, points, nviews, w2c, intrinsics,
                       n_intrinsics, H, W, depth, eps, counts);
    return launched("cull_visibility_kernel");
}

}  // extern "C"

}  // namespace surfel
