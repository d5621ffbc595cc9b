// mesh_texture.hip — texturing of a triangle mesh (include/surfel_texture.h, TEXTURE.md): the triangle atlas (classes, the stable rank
// of a triangle within its class through scan_u32, corner coordinates), the kernel that bakes a batch of views into the accumulator,
// the resolve into 8-bit texels and the shading of a visibility buffer with the atlas.  Compiled with -ffp-contract=off (build.py):
// every kernel rounds as its restatement in tests/texture_oracle.py — fp32 throughout, correctly rounded / and sqrt, no fused
// multiply-add.  wave64; no LDS, no MFMA; no floating-point atomics (the only atomics count triangles and texels).
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/surfel_meshview.h"
#include "../../include/surfel_texture.h"
#include "mesh_raster.h"
#include "mesh_sample.h"
#include "side_util.h"
#include "vis_pixels.h"

namespace surfel {

constexpr int TEX_CLASSES = SURFEL_TEXTURE_CLASSES;
constexpr int TEX_PAD = SURFEL_TEXTURE_PAD;
constexpr int64_t TEX_MAX_F = (int64_t)1 << 28;

__host__ __device__ inline int tex_legs(int c) { return 1 << (c + SURFEL_TEXTURE_MIN_LOG2); }

// The band table as the kernels take it (by value: scalar registers).  rows: rows of cells; block0: the first workgroup of the bake
// kernel's grid that works on the band (block0[TEX_CLASSES]: the grid), bands in class order.
struct TexBands {
    int y0[TEX_CLASSES], per_row[TEX_CLASSES], first[TEX_CLASSES], count[TEX_CLASSES], rows[TEX_CLASSES];
    int64_t block0[TEX_CLASSES + 1];
};

// A triangle with a patch: its corners in patch order — a at the right angle (the corner opposite the longest edge, the lowest corner
// index among equals), then b (along the patch's x) and c (along its y), the triangle's cyclic order kept — and its unit face normal
struct TexTri {
    int64_t ia, ib, ic;
    float ax, ay, az, bx, by, bz, cx, cy, cz;
    float nx, ny, nz;
    float longest2;      // the squared length of the longest edge
    int corner;          // which of the triangle's corners is a
};

// false: no patch (an index outside [0, V), a non-finite coordinate, a face normal of length zero or not finite)
__device__ inline bool tex_tri(int64_t t, int64_t V, const float* __restrict__ verts, const int32_t* __restrict__ tris, TexTri& o) {
    const int64_t i0 = tris[3 * t], i1 = tris[3 * t + 1], i2 = tris[3 * t + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= V || i1 >= V || i2 >= V) return false;
    const float x0 = verts[3 * i0], y0 = verts[3 * i0 + 1], z0 = verts[3 * i0 + 2];
    const float x1 = verts[3 * i1], y1 = verts[3 * i1 + 1], z1 = verts[3 * i1 + 2];
    const float x2 = verts[3 * i2], y2 = verts[3 * i2 + 1], z2 = verts[3 * i2 + 2];
    if (!(isfinite(x0) && isfinite(y0) && isfinite(z0) && isfinite(x1) && isfinite(y1) && isfinite(z1) && isfinite(x2) && isfinite(y2) && isfinite(z2)))
        return false;
    // the face normal as surfel_meshview_vertex_normals computes it
    const float ux = x1 - x0, uy = y1 - y0, uz = z1 - z0, vx = x2 - x0, vy = y2 - y0, vz = z2 - z0;
    const float fx = uy * vz - uz * vy, fy = uz * vx - ux * vz, fz = ux * vy - uy * vx;
    const float len = sqrtf((fx * fx + fy * fy) + fz * fz);
    if (!isfinite(len) || !(len > 0.0f)) return false;
    o.nx = fx / len; o.ny = fy / len; o.nz = fz / len;
    // edge k lies opposite corner k
    const float wx = x2 - x1, wy = y2 - y1, wz = z2 - z1;
    const float e0 = (wx * wx + wy * wy) + wz * wz, e1 = (vx * vx + vy * vy) + vz * vz, e2 = (ux * ux + uy * uy) + uz * uz;
    int r = 0;
    float m = e0;
    if (e1 > m) { r = 1; m = e1; }
    if (e2 > m) { r = 2; m = e2; }
    o.longest2 = m;
    o.corner = r;
    if (r == 0) {
        o.ia = i0; o.ib = i1; o.ic = i2;
        o.ax = x0; o.ay = y0; o.az = z0; o.bx = x1; o.by = y1; o.bz = z1; o.cx = x2; o.cy = y2; o.cz = z2;
    } else if (r == 1) {
        o.ia = i1; o.ib = i2; o.ic = i0;
        o.ax = x1; o.ay = y1; o.az = z1; o.bx = x2; o.by = y2; o.bz = z2; o.cx = x0; o.cy = y0; o.cz = z0;
    } else {
        o.ia = i2; o.ib = i0; o.ic = i1;
        o.ax = x2; o.ay = y2; o.az = z2; o.bx = x0; o.by = y0; o.bz = z0; o.cx = x1; o.cy = y1; o.cz = z1;
    }
    return true;
}

// the barycentrics (of a, b, c) of the patch coordinates (du, dv) in texels, clamped into the triangle (TEXTURE.md §Baking 1): every
// value is a multiple of 1 / (2 n), exact in fp32
__device__ inline void tex_bary(int n, int du, int dv, float& b0, float& b1, float& b2) {
    const float fn = (float)n;
    float a = fminf(fmaxf((float)du, 0.0f), fn), b = fminf(fmaxf((float)dv, 0.0f), fn);
    const float s = a + b;
    if (s > fn) {
        const float h = (s - fn) * 0.5f;
        a = a - h; b = b - h;
        if (a < 0.0f) { a = 0.0f; b = fn; }
        if (b < 0.0f) { b = 0.0f; a = fn; }
    }
    b1 = a / fn; b2 = b / fn;
    b0 = (1.0f - b1) - b2;
}

// cell-local texel (lx, ly) of a cell of legs n: the half that owns it and its patch coordinates
__device__ inline int tex_half(int n, int lx, int ly, int& du, int& dv) {
    const int half = lx + ly > n + 2 ? 1 : 0;
    du = half ? n + TEX_PAD - 2 - lx : lx;
    dv = half ? n + TEX_PAD - 2 - ly : ly;
    return half;
}

// the owner of atlas texel (x, y): band by y, cell, half, rank, triangle through `order`.  false: nobody owns it.
__device__ inline bool tex_owner(const TexBands& B, int Wa, int64_t F, int x, int y, const uint32_t* __restrict__ order, int64_t& tri, int& n, int& du,
                                 int& dv) {
    int band = -1, y0 = 0, per = 0, first = 0, count = 0;
#pragma unroll
    for (int c = 0; c < TEX_CLASSES; c++) {
        const int cell = tex_legs(c) + TEX_PAD;
        if (B.count[c] > 0 && y >= B.y0[c] && y < B.y0[c] + B.rows[c] * cell) { band = c; y0 = B.y0[c]; per = B.per_row[c]; first = B.first[c]; count = B.count[c]; }
    }
    if (band < 0) return false;
    n = tex_legs(band);
    const int cell = n + TEX_PAD;
    const int row = (y - y0) / cell, ly = (y - y0) - row * cell, col = x / cell, lx = x - col * cell;
    if (col >= per) return false;
    const int half = tex_half(n, lx, ly, du, dv);
    const int64_t rank = 2 * ((int64_t)row * per + col) + half;
    if (rank >= count) return false;
    tri = order[first + rank];
    return tri < F;
}

// ---- layout ------------------------------------------------------------------------------------------------------------------------------
__device__ inline int tex_class(float longest2, float density) {
    const float s = sqrtf(longest2) * density;
    return (s > 4.0f) + (s > 8.0f) + (s > 16.0f) + (s > 32.0f) + (s > 64.0f);
}

__global__ void __launch_bounds__(CT) texture_classify_kernel(int64_t V, int64_t F, const float* __restrict__ verts, const int32_t* __restrict__ tris,
                                                              float density, int32_t* __restrict__ cls, uint32_t* counts) {
    const int64_t t = (int64_t)blockIdx.x * CT + threadIdx.x;
    int c = -1;
    TexTri tri;
    if (t < F) {
        if (tex_tri(t, V, verts, tris, tri)) c = tex_class(tri.longest2, density);
        cls[t] = c;
    }
#pragma unroll
    for (int k = 0; k < TEX_CLASSES; k++) {
        const unsigned long long m = __ballot(c == k);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(counts + k, (uint32_t)__popcll(m));
    }
}

// ind[(5 - c) F + t] <- cls[t] == c: after the scan, the slot of triangle t in band order (largest class first, triangle order within)
__global__ void __launch_bounds__(CT) texture_indicator_kernel(int64_t F, const int32_t* __restrict__ cls, uint32_t* __restrict__ ind) {
    const int64_t t = (int64_t)blockIdx.x * CT + threadIdx.x;
    if (t >= F) return;
    const int c = cls[t];
#pragma unroll
    for (int k = 0; k < TEX_CLASSES; k++) ind[(int64_t)(TEX_CLASSES - 1 - k) * F + t] = c == k ? 1u : 0u;
}

__global__ void __launch_bounds__(CT) texture_place_kernel(int64_t V, int64_t F, const float* __restrict__ verts, const int32_t* __restrict__ tris,
                                                           const int32_t* __restrict__ cls, const uint32_t* __restrict__ slot, TexBands B,
                                                           uint32_t* __restrict__ order, float* __restrict__ uv) {
    const int64_t t = (int64_t)blockIdx.x * CT + threadIdx.x;
    if (t >= F) return;
    float q[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    const int c = cls[t];
    TexTri tri;
    if (c >= 0 && c < TEX_CLASSES && tex_tri(t, V, verts, tris, tri)) {
        int y0 = 0, per = 1, first = 0;
#pragma unroll
        for (int k = 0; k < TEX_CLASSES; k++)
            if (k == c) { y0 = B.y0[k]; per = B.per_row[k]; first = B.first[k]; }
        const int64_t g = slot[(int64_t)(TEX_CLASSES - 1 - c) * F + t];
        if (g < F) order[g] = (uint32_t)t;
        const int64_t rank = g - first, cellidx = rank >> 1;
        const int n = tex_legs(c), cell = n + TEX_PAD;
        const int row = (int)(cellidx / per), col = (int)(cellidx - (int64_t)row * per);
        const float ox = (float)(col * cell), oy = (float)(y0 + row * cell), fn = (float)n;
        float ua, va, ub, vb, uc, vc;
        if (rank & 1) {      // the upper half: the lower one turned by 180 degrees about the cell
            ua = ox + (float)(cell - 2); va = oy + (float)(cell - 2);
            ub = ua - fn; vb = va; uc = ua; vc = va - fn;
        } else {
            ua = ox; va = oy;
            ub = ua + fn; vb = va; uc = ua; vc = va + fn;
        }
        const int ka = tri.corner, kb = (tri.corner + 1) % 3, kc = (tri.corner + 2) % 3;
        q[2 * ka] = ua; q[2 * ka + 1] = va; q[2 * kb] = ub; q[2 * kb + 1] = vb; q[2 * kc] = uc; q[2 * kc + 1] = vc;
    }
#pragma unroll
    for (int k = 0; k < 6; k++) uv[6 * t + k] = q[k];
}

// ---- baking ------------------------------------------------------------------------------------------------------------------------------
// One sample of a planar image by CULL.md §Visibility rule 4's four corners: (x0, y0) lies inside, a corner outside adds nothing
__device__ inline float tex_corners(const float* __restrict__ img, int W, int H, int x0, int y0, float nw, float ne, float sw, float se) {
    const int x1 = x0 + 1, y1 = y0 + 1;
    float s = 0.0f;
    s += img[(int64_t)y0 * W + x0] * nw;
    if (x1 < W) s += img[(int64_t)y0 * W + x1] * ne;
    if (y1 < H) s += img[(int64_t)y1 * W + x0] * sw;
    if (x1 < W && y1 < H) s += img[(int64_t)y1 * W + x1] * se;
    return s;
}

// One thread per texel of the band's cells, cell after cell: a workgroup covers CT consecutive texels of a run of cells (small classes)
// or a few rows of one cell (large ones), so a wave's points are neighbours on the surface.  The view index, the camera block and the
// band are uniform: the compiler keeps them in scalar registers.
__global__ void __launch_bounds__(CT) texture_bake_kernel(int64_t V, int64_t F, const float* __restrict__ verts, const int32_t* __restrict__ tris, TexBands B,
                                                          const uint32_t* __restrict__ order, int Wa, int nviews, const float* __restrict__ w2c,
                                                          const float* __restrict__ intrinsics, int n_intrinsics, int H, int W,
                                                          const float* __restrict__ depth, const float* __restrict__ images, float eps, float cos_min,
                                                          int power, int blend, float* __restrict__ acc) {
    const int64_t blk = blockIdx.x;
    int band = 0;
#pragma unroll
    for (int c = 1; c < TEX_CLASSES; c++)
        if (blk >= B.block0[c]) band = c;
    int y0 = 0, per = 1, first = 0, count = 0;
    int64_t b0blk = 0;
#pragma unroll
    for (int c = 0; c < TEX_CLASSES; c++)
        if (c == band) { y0 = B.y0[c]; per = B.per_row[c]; first = B.first[c]; count = B.count[c]; b0blk = B.block0[c]; }
    const int n = tex_legs(band), cell = n + TEX_PAD;
    // (an accepted band table keeps a band's cells inside the atlas: fewer than 2^28 + CT texels, so 32-bit divisions)
    const int idx = (int)(blk - b0blk) * CT + (int)threadIdx.x;
    const int cellidx = idx / (cell * cell);
    const int local = idx - cellidx * (cell * cell);
    const int ly = local / cell, lx = local - ly * cell;
    int du, dv;
    const int64_t rank = 2 * (int64_t)cellidx + tex_half(n, lx, ly, du, dv);
    if (rank >= count) return;
    const int64_t t = order[first + rank];
    TexTri tri;
    if (t >= F || !tex_tri(t, V, verts, tris, tri)) return;
    const int row = cellidx / per, col = cellidx - row * per;
    const int x = col * cell + lx, y = y0 + row * cell + ly;
    float b0, b1, b2;
    tex_bary(n, du, dv, b0, b1, b2);
    const float px = (b0 * tri.ax + b1 * tri.bx) + b2 * tri.cx, py = (b0 * tri.ay + b1 * tri.by) + b2 * tri.cy, pz = (b0 * tri.az + b1 * tri.bz) + b2 * tri.cz;
    float4* const slot = reinterpret_cast<float4*>(acc) + ((int64_t)y * Wa + x);
    float4 a = *slot;
    const float wm = (float)(W - 1), hm = (float)(H - 1);
    const int64_t hw = (int64_t)H * W;
    for (int view = 0; view < nviews; view++) {
        const float* m = w2c + 12 * (int64_t)view;
        const float* q = intrinsics + 4 * (int64_t)(n_intrinsics == 1 ? 0 : view);
        // CULL.md §Visibility rules 1-3
        const float X = ((m[0] * px + m[1] * py) + m[2] * pz) + m[3], Y = ((m[4] * px + m[5] * py) + m[6] * pz) + m[7], Z = ((m[8] * px + m[9] * py) + m[10] * pz) + m[11];
        const float zz = Z + 1e-8f;
        const float u = (q[0] * X + q[2] * Z) / zz, v = (q[1] * Y + q[3] * Z) / zz;
        if (!(u >= 0.0f && u <= wm && v >= 0.0f && v <= hm && zz > 0.0f)) continue;
        // rule 4: the round trip, the clip, the corner weights
        const float gx = u / wm * 2.0f - 1.0f, gy = v / hm * 2.0f - 1.0f;
        const float ix = fminf(wm, fmaxf(((gx + 1.0f) / 2.0f) * wm, 0.0f)), iy = fminf(hm, fmaxf(((gy + 1.0f) / 2.0f) * hm, 0.0f));
        const float fx0 = floorf(ix), fy0 = floorf(iy), fx1 = fx0 + 1.0f, fy1 = fy0 + 1.0f;
        const int x0 = (int)fx0, yy0 = (int)fy0;
        const float nw = (fx1 - ix) * (fy1 - iy), ne = (ix - fx0) * (fy1 - iy), sw = (fx1 - ix) * (iy - fy0), se = (ix - fx0) * (iy - fy0);
        const float sample = tex_corners(depth + view * hw, W, H, x0, yy0, nw, ne, sw, se);
        // rule 5
        if (!(sample > 0.0f ? zz < sample + eps : true)) continue;
        // the cosine between the face normal and the ray, in camera space
        const float ncx = (m[0] * tri.nx + m[1] * tri.ny) + m[2] * tri.nz, ncy = (m[4] * tri.nx + m[5] * tri.ny) + m[6] * tri.nz,
                    ncz = (m[8] * tri.nx + m[9] * tri.ny) + m[10] * tri.nz;
        const float cs = fabsf((ncx * X + ncy * Y) + ncz * Z) / sqrtf((X * X + Y * Y) + Z * Z);
        if (!(cs >= cos_min)) continue;
        float cp = cs;
        for (int k = 1; k < power; k++) cp = cp * cs;
        const float w = cp / (zz * zz);
        const float* img = images + 3 * view * hw;
        const float r = tex_corners(img, W, H, x0, yy0, nw, ne, sw, se), g = tex_corners(img + hw, W, H, x0, yy0, nw, ne, sw, se),
                    b = tex_corners(img + 2 * hw, W, H, x0, yy0, nw, ne, sw, se);
        if (blend == SURFEL_TEXTURE_AVERAGE) {
            a.x = a.x + w * r; a.y = a.y + w * g; a.z = a.z + w * b; a.w = a.w + w;
        } else if (w > a.w) {
            a.x = r; a.y = g; a.z = b; a.w = w;
        }
    }
    *slot = a;
}

// ---- resolve -----------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CT) texture_resolve_kernel(int64_t V, int64_t F, const float* __restrict__ verts, const int32_t* __restrict__ tris,
                                                             const float* __restrict__ colors, TexBands B, const uint32_t* __restrict__ order, int Wa, int Ha,
                                                             const float* __restrict__ acc, int blend, float bg_r, float bg_g, float bg_b,
                                                             uint8_t* __restrict__ atlas, unsigned long long* stats) {
    const int64_t i = (int64_t)blockIdx.x * CT + threadIdx.x;
    bool owned = false, seen = false;
    if (i < (int64_t)Ha * Wa) {
        const int y = (int)(i / Wa), x = (int)(i - (int64_t)y * Wa);
        float r = bg_r, g = bg_g, b = bg_b;
        int64_t t;
        int n, du, dv;
        TexTri tri;
        if (tex_owner(B, Wa, F, x, y, order, t, n, du, dv) && tex_tri(t, V, verts, tris, tri)) {
            owned = true;
            const float4 a = reinterpret_cast<const float4*>(acc)[i];
            if (a.w > 0.0f) {
                seen = true;
                if (blend == SURFEL_TEXTURE_AVERAGE) { r = a.x / a.w; g = a.y / a.w; b = a.z / a.w; }
                else { r = a.x; g = a.y; b = a.z; }
            } else if (colors) {
                float b0, b1, b2;
                tex_bary(n, du, dv, b0, b1, b2);
                r = (b0 * colors[3 * tri.ia] + b1 * colors[3 * tri.ib]) + b2 * colors[3 * tri.ic];
                g = (b0 * colors[3 * tri.ia + 1] + b1 * colors[3 * tri.ib + 1]) + b2 * colors[3 * tri.ic + 1];
                b = (b0 * colors[3 * tri.ia + 2] + b1 * colors[3 * tri.ib + 2]) + b2 * colors[3 * tri.ic + 2];
            } else {
                r = g = b = 0.8f;
            }
        }
        atlas[3 * i] = (uint8_t)quant8(r, 1.0f, 0.0f);
        atlas[3 * i + 1] = (uint8_t)quant8(g, 1.0f, 0.0f);
        atlas[3 * i + 2] = (uint8_t)quant8(b, 1.0f, 0.0f);
    }
    const unsigned long long mo = __ballot(owned), ms = __ballot(seen);
    if ((threadIdx.x & 63) == 0) {
        if (mo) atomicAdd(stats, (unsigned long long)__popcll(mo));
        if (ms) atomicAdd(stats + 1, (unsigned long long)__popcll(ms));
    }
}

// ---- textured shading --------------------------------------------------------------------------------------------------------------------
struct TexColor { float r, g, b; };

// MESHVIEW.md §Shading steps 1-4 (mesh_sample.h), then the atlas at the interpolated uv
__device__ inline TexColor texture_sample(uint64_t key, float x, float y, const CullCam& c, int64_t V, int64_t F, const float* __restrict__ verts,
                                          const int32_t* __restrict__ tris, const float* __restrict__ uv, const uint8_t* __restrict__ atlas, int Wa, int Ha,
                                          TexColor bg) {
    MeshSample sm;
    if (!mesh_sample(key, x, y, c, V, F, verts, tris, sm)) return bg;
    const float l0 = sm.l0, l1 = sm.l1, l2 = sm.l2;
    // the texel coordinates, clamped into the atlas (a NaN becomes 0), and the four texels around them
    const float* q = uv + 6 * (int64_t)(uint32_t)key;
    const float u = fminf(fmaxf((l0 * q[0] + l1 * q[2]) + l2 * q[4], 0.0f), (float)(Wa - 1));
    const float v = fminf(fmaxf((l0 * q[1] + l1 * q[3]) + l2 * q[5], 0.0f), (float)(Ha - 1));
    const float fx0 = floorf(u), fy0 = floorf(v), fx1 = fx0 + 1.0f, fy1 = fy0 + 1.0f;
    const int x0 = (int)fx0, y0 = (int)fy0, x1 = x0 + 1, y1 = y0 + 1;
    const float nw = (fx1 - u) * (fy1 - v), ne = (u - fx0) * (fy1 - v), sw = (fx1 - u) * (v - fy0), se = (u - fx0) * (v - fy0);
    float s[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        s[k] += ((float)atlas[3 * ((int64_t)y0 * Wa + x0) + k] / 255.0f) * nw;
        if (x1 < Wa) s[k] += ((float)atlas[3 * ((int64_t)y0 * Wa + x1) + k] / 255.0f) * ne;
        if (y1 < Ha) s[k] += ((float)atlas[3 * ((int64_t)y1 * Wa + x0) + k] / 255.0f) * sw;
        if (x1 < Wa && y1 < Ha) s[k] += ((float)atlas[3 * ((int64_t)y1 * Wa + x1) + k] / 255.0f) * se;
    }
    TexColor o = {s[0], s[1], s[2]};
    return o;
}

// one thread per output pixel of every view (as meshview_shade_kernel)
__global__ void __launch_bounds__(CT) texture_shade_kernel(int64_t V, int64_t F, const float* __restrict__ verts, const int32_t* __restrict__ tris,
                                                           const float* __restrict__ uv, const uint8_t* __restrict__ atlas, int Wa, int Ha, int nviews,
                                                           const float* __restrict__ w2c, const float* __restrict__ intrinsics, int n_intrinsics, int H, int W,
                                                           int ssaa, const uint64_t* __restrict__ key, float bg_r, float bg_g, float bg_b,
                                                           uint8_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * CT + threadIdx.x;
    const int64_t hw = (int64_t)H * W;
    if (i >= hw * nviews) return;
    const int view = (int)(i / hw);
    const int y = (int)((i - view * hw) / W), x = (int)((i - view * hw) - (int64_t)y * W);
    const CullCam cam = cull_cam(w2c, intrinsics, n_intrinsics, view);
    const int64_t sW = (int64_t)W * ssaa;
    const uint64_t* img = key + view * hw * ssaa * ssaa;
    const TexColor bg = {bg_r, bg_g, bg_b};
    float r = 0.0f, g = 0.0f, b = 0.0f;
    for (int ky = 0; ky < ssaa; ky++)
        for (int kx = 0; kx < ssaa; kx++) {
            const int sx = x * ssaa + kx, sy = y * ssaa + ky;
            const TexColor c = texture_sample(img[sy * sW + sx], (float)sx, (float)sy, cam, V, F, verts, tris, uv, atlas, Wa, Ha, bg);
            r = r + c.r; g = g + c.g; b = b + c.b;
        }
    const float inv = 1.0f / (float)(ssaa * ssaa);
    out[3 * i] = (uint8_t)quant8(r * inv, 1.0f, 0.0f);
    out[3 * i + 1] = (uint8_t)quant8(g * inv, 1.0f, 0.0f);
    out[3 * i + 2] = (uint8_t)quant8(b * inv, 1.0f, 0.0f);
}

namespace {

// The kernels' form of a band table; false: the table does not describe an atlas of Wa x Ha texels over `order`[F] (every index the
// kernels form from an accepted table lies inside the atlas and inside `order`)
bool tex_bands(const int32_t* table, int Wa, int Ha, int64_t F, TexBands& B) {
    int64_t blocks = 0, used = 0;
    for (int c = 0; c < TEX_CLASSES; c++) {
        const int32_t* r = table + SURFEL_TEXTURE_BAND_INTS * c;
        const int64_t cell = tex_legs(c) + TEX_PAD;
        B.y0[c] = r[0]; B.per_row[c] = r[1]; B.first[c] = r[2]; B.count[c] = r[3]; B.rows[c] = 0;
        B.block0[c] = blocks;
        if (r[3] < 0) return false;
        if (r[3] == 0) continue;
        const int64_t cells = ((int64_t)r[3] + 1) / 2;
        if (r[1] < 1 || r[1] * cell > Wa || r[0] < 0 || r[2] < 0 || (int64_t)r[2] + r[3] > F) return false;
        const int64_t rows = (cells + r[1] - 1) / r[1];
        if (r[0] + rows * cell > Ha) return false;
        B.rows[c] = (int)rows;
        blocks += (cells * cell * cell + CT - 1) / CT;
        used += r[3];
    }
    B.block0[TEX_CLASSES] = blocks;
    return used <= F;
}

bool tex_bad_mesh(int64_t V, int64_t F, const float* verts, const int32_t* tris) { return V < 0 || F < 0 || (V > 0 && !verts) || (F > 0 && !tris); }

bool tex_bad_atlas(int Wa, int Ha) { return Wa < 1 || Ha < 1 || Wa > SURFEL_TEXTURE_MAX_SIDE || Ha > SURFEL_TEXTURE_MAX_SIDE; }

}  // namespace

extern "C" {

int surfel_texture_classify(surfel_alloc_fn alloc, void* user, int64_t V, int64_t F, const float* verts, const int32_t* tris, float density,
                            int32_t* cls, int64_t* counts, void* stream) {
    if (!alloc || tex_bad_mesh(V, F, verts, tris) || (F > 0 && !cls) || !counts || !(density > 0.0f) || !(density < INFINITY))
        return api_fail(SURFEL_E_INVALID, "texture_classify: bad arguments");
    if (V > CULL_MAX_ELEMS || F > TEX_MAX_F) return api_fail(SURFEL_E_LIMIT, "texture_classify: more than 2^31 - 1 vertices or 2^28 triangles");
    for (int k = 0; k < TEX_CLASSES; k++) counts[k] = 0;
    if (F == 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint32_t* dcounts = take<uint32_t>(alloc, user, 8);
    if (!dcounts) return api_fail(SURFEL_E_ALLOC, "texture_classify", hipSuccess);
    if (hipMemsetAsync(dcounts, 0, 8 * sizeof(uint32_t), st) != hipSuccess) return api_fail(SURFEL_E_HIP, "texture_classify: memset", hipGetLastError());
    hipLaunchKernelGGL(texture_classify_kernel, dim3(blocks_for(F, CT)), dim3(CT), 0, st, V, F, verts, tris, density, cls, dcounts);
    if (int rc = launched("texture_classify_kernel")) return rc;
    uint32_t host[8];
    if (int rc = read_words("texture_classify: counts", dcounts, host, 8, st)) return rc;
    for (int k = 0; k < TEX_CLASSES; k++) counts[k] = host[k];
    return 0;
}

int64_t surfel_texture_layout(surfel_alloc_fn alloc, void* user, int64_t V, int64_t F, const float* verts, const int32_t* tris, const int32_t* cls,
                              const int64_t* counts, int Wa, int32_t* table, uint32_t* order, float* uv, void* stream) {
    if (!alloc || tex_bad_mesh(V, F, verts, tris) || (F > 0 && (!cls || !order || !uv)) || !counts || !table || Wa < 1)
        return api_fail(SURFEL_E_INVALID, "texture_layout: bad arguments");
    int64_t total = 0;
    for (int c = 0; c < TEX_CLASSES; c++) {
        if (counts[c] < 0) return api_fail(SURFEL_E_INVALID, "texture_layout: a negative count");
        total += counts[c];
    }
    if (total > F) return api_fail(SURFEL_E_INVALID, "texture_layout: the counts exceed the triangles");
    if (V > CULL_MAX_ELEMS || F > TEX_MAX_F) return api_fail(SURFEL_E_LIMIT, "texture_layout: more than 2^31 - 1 vertices or 2^28 triangles");
    if (Wa > SURFEL_TEXTURE_MAX_SIDE) return api_fail(SURFEL_E_LIMIT, "texture_layout: the atlas is wider than SURFEL_TEXTURE_MAX_SIDE");
    // bands, largest class first
    int32_t tab[TEX_CLASSES * SURFEL_TEXTURE_BAND_INTS];
    int64_t y = 0, first = 0;
    for (int c = TEX_CLASSES - 1; c >= 0; c--) {
        const int64_t cell = tex_legs(c) + TEX_PAD;
        int32_t* r = tab + SURFEL_TEXTURE_BAND_INTS * c;
        const int64_t per = Wa / cell;
        r[0] = (int32_t)y; r[1] = (int32_t)per; r[2] = (int32_t)first; r[3] = (int32_t)counts[c];
        if (counts[c] == 0) continue;
        if (per < 1) return api_fail(SURFEL_E_LIMIT, "texture_layout: the atlas is narrower than a cell of the largest class in use");
        const int64_t cells = (counts[c] + 1) / 2;
        y += (cells + per - 1) / per * cell;
        first += counts[c];
        if (y > SURFEL_TEXTURE_MAX_SIDE) return api_fail(SURFEL_E_LIMIT, "texture_layout: the atlas is higher than SURFEL_TEXTURE_MAX_SIDE (lower the density)");
    }
    const int64_t Ha = y > 0 ? y : 1;
    TexBands B;
    if (!tex_bands(tab, Wa, (int)Ha, F, B)) return api_fail(SURFEL_E_INVALID, "texture_layout: inconsistent counts");
    for (int k = 0; k < TEX_CLASSES * SURFEL_TEXTURE_BAND_INTS; k++) table[k] = tab[k];
    if (F == 0) return Ha;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t n = (int64_t)TEX_CLASSES * F;
    const ScanBuf ind = take_scan(alloc, user, n);
    if (!ind.flags) return api_fail(SURFEL_E_ALLOC, "texture_layout", hipSuccess);
    hipLaunchKernelGGL(texture_indicator_kernel, dim3(blocks_for(F, CT)), dim3(CT), 0, st, F, cls, ind.flags);
    if (int rc = launched("texture_indicator_kernel")) return rc;
    ind.scan(st);
    if (int rc = launched("scan_u32")) return rc;
    hipLaunchKernelGGL(texture_place_kernel, dim3(blocks_for(F, CT)), dim3(CT), 0, st, V, F, verts, tris, cls, ind.flags, B, order, uv);
    if (int rc = launched("texture_place_kernel")) return rc;
    return Ha;
}

int surfel_texture_bake(int64_t V, int64_t F, const float* verts, const int32_t* tris, const int32_t* table, const uint32_t* order, int Wa, int Ha,
                        int nviews, const float* w2c, const float* intrinsics, int n_intrinsics, int H, int W, const float* depth, const float* images,
                        float eps, float cos_min, int power, int blend, float* acc, void* stream) {
    if (tex_bad_mesh(V, F, verts, tris) || !table || (F > 0 && !order) || Wa < 1 || Ha < 1 || cull_bad_cameras(nviews, w2c, intrinsics, n_intrinsics) || H < 2 ||
        W < 2 || (nviews > 0 && (!depth || !images)) || !acc || !(eps == eps) || !(cos_min == cos_min) || power < 1 || power > SURFEL_TEXTURE_MAX_POWER ||
        (blend != SURFEL_TEXTURE_AVERAGE && blend != SURFEL_TEXTURE_BEST) || (reinterpret_cast<uintptr_t>(acc) & 15))
        return api_fail(SURFEL_E_INVALID, "texture_bake: bad arguments");
    if (tex_bad_atlas(Wa, Ha)) return api_fail(SURFEL_E_LIMIT, "texture_bake: the atlas is larger than SURFEL_TEXTURE_MAX_SIDE");
    if (V > CULL_MAX_ELEMS || F > TEX_MAX_F || (int64_t)H * W > CULL_MAX_ELEMS)
        return api_fail(SURFEL_E_LIMIT, "texture_bake: more than 2^31 - 1 vertices or pixels, or 2^28 triangles");
    if (nviews > SURFEL_CULL_MAX_VIEWS) return api_fail(SURFEL_E_LIMIT, "texture_bake: more than SURFEL_CULL_MAX_VIEWS views in one call");
    TexBands B;
    if (!tex_bands(table, Wa, Ha, F, B)) return api_fail(SURFEL_E_INVALID, "texture_bake: the band table does not fit the atlas");
    const int64_t blocks = B.block0[TEX_CLASSES];
    if (blocks > CULL_MAX_ELEMS) return api_fail(SURFEL_E_LIMIT, "texture_bake: more than 2^31 - 1 workgroups");
    if (nviews == 0 || blocks == 0) return 0;
    hipLaunchKernelGGL(texture_bake_kernel, dim3((unsigned)blocks), dim3(CT), 0, static_cast<hipStream_t>(stream), V, F, verts, tris, B, order, Wa, nviews, w2c,
                       intrinsics, n_intrinsics, H, W, depth, images, eps, cos_min, power, blend, acc);
    return launched("texture_bake_kernel");
}

int surfel_texture_resolve(int64_t V, int64_t F, const float* verts, const int32_t* tris, const float* colors, const int32_t* table,
                           const uint32_t* order, int Wa, int Ha, const float* acc, int blend, float bg_r, float bg_g, float bg_b, uint8_t* atlas,
                           int64_t* stats, void* stream) {
    if (tex_bad_mesh(V, F, verts, tris) || !table || (F > 0 && !order) || Wa < 1 || Ha < 1 || !acc || !atlas || !stats ||
        (blend != SURFEL_TEXTURE_AVERAGE && blend != SURFEL_TEXTURE_BEST) || (reinterpret_cast<uintptr_t>(acc) & 15))
        return api_fail(SURFEL_E_INVALID, "texture_resolve: bad arguments");
    if (tex_bad_atlas(Wa, Ha)) return api_fail(SURFEL_E_LIMIT, "texture_resolve: the atlas is larger than SURFEL_TEXTURE_MAX_SIDE");
    if (V > CULL_MAX_ELEMS || F > TEX_MAX_F) return api_fail(SURFEL_E_LIMIT, "texture_resolve: more than 2^31 - 1 vertices or 2^28 triangles");
    TexBands B;
    if (!tex_bands(table, Wa, Ha, F, B)) return api_fail(SURFEL_E_INVALID, "texture_resolve: the band table does not fit the atlas");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(stats, 0, 2 * sizeof(int64_t), st) != hipSuccess) return api_fail(SURFEL_E_HIP, "texture_resolve: memset", hipGetLastError());
    hipLaunchKernelGGL(texture_resolve_kernel, dim3(blocks_for((int64_t)Ha * Wa, CT)), dim3(CT), 0, st, V, F, verts, tris, colors, B, order, Wa, Ha, acc, blend,
                       bg_r, bg_g, bg_b, atlas, reinterpret_cast<unsigned long long*>(stats));
    return launched("texture_resolve_kernel");
}

int surfel_texture_shade(int64_t V, int64_t F, const float* verts, const int32_t* tris, const float* uv, const uint8_t* atlas, int Wa, int Ha,
                         int nviews, const float* w2c, const float* intrinsics, int n_intrinsics, int H, int W, int ssaa, const uint64_t* key,
                         float bg_r, float bg_g, float bg_b, uint8_t* out, void* stream) {
    if (tex_bad_mesh(V, F, verts, tris) || (F > 0 && !uv) || !atlas || Wa < 1 || Ha < 1 || cull_bad_cameras(nviews, w2c, intrinsics, n_intrinsics) || H < 1 ||
        W < 1 || ssaa < 1 || ssaa > SURFEL_MESHVIEW_MAX_SSAA || (nviews > 0 && (!key || !out)))
        return api_fail(SURFEL_E_INVALID, "texture_shade: bad arguments");
    if (tex_bad_atlas(Wa, Ha)) return api_fail(SURFEL_E_LIMIT, "texture_shade: the atlas is larger than SURFEL_TEXTURE_MAX_SIDE");
    if (V > CULL_MAX_ELEMS || F > CULL_MAX_ELEMS || (int64_t)H * W * ssaa * ssaa > CULL_MAX_ELEMS)
        return api_fail(SURFEL_E_LIMIT, "texture_shade: more than 2^31 - 1 vertices, triangles or samples of a view");
    if (nviews > SURFEL_CULL_MAX_VIEWS) return api_fail(SURFEL_E_LIMIT, "texture_shade: more than SURFEL_CULL_MAX_VIEWS views in one call");
    if (nviews == 0) return 0;
    const int64_t n = (int64_t)nviews * H * W;
    if ((n + CT - 1) / CT > CULL_MAX_ELEMS) return api_fail(SURFEL_E_LIMIT, "texture_shade: more than 2^39 output pixels in one call");
    hipLaunchKernelGGL(texture_shade_kernel, dim3(blocks_for(n, CT)), dim3(CT), 0, static_cast<hipStream_t>(stream), V, F, verts, tris, uv, atlas, Wa, Ha,
                       nviews, w2c, intrinsics, n_intrinsics, H, W, ssaa, key, bg_r, bg_g, bg_b, out);
    return launched("texture_shade_kernel");
}

}  // extern "C"

}  // namespace surfel
