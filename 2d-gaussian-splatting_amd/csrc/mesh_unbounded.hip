// mesh_unbounded.hip — unbounded mesh extraction: TSDF fusion on a contracted lattice, marching cubes over z-slabs and vertex colours
// (include/surfel_mesh_unbounded.h, MESH.md §Unbounded).  Every output is written by exactly one thread and read back in a fixed
// order: no atomics, so the result does not depend on launch order.  The exclusive scan is device_scan.hip's; the case table and the
// triangle writer (mesh_mc.h) are shared with mesh_tsdf.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/surfel_mesh_unbounded.h"
#include "mesh_mc.h"
#include "side_util.h"

namespace surfel {
namespace {

constexpr int UT = 256;                      // threads per workgroup
constexpr int FBX = 8, FBY = 8, FBZ = 4;     // fusion brick: a wave is an 8 x 8 patch of one z plane
constexpr int MAX_M = 2048;
constexpr int64_t SLAB_DEFAULT = (int64_t)1 << 26;      // samples per slab by default
constexpr int64_t SLAB_MAX = (int64_t)1 << 28;          // scratch samples per slab: 5 triangles per cube stay below 2^32
constexpr int64_t MAX_INDEX = ((int64_t)1 << 31) - 1;

struct Lat {      // what the kernels need of surfel_unbounded_volume
    int M;
    float R, step, cx, cy, cz, radius, vs;
};

// ---- fusion --------------------------------------------------------------------------------------------------------------------
// bilinear sample of img[H, W] at the pixel coordinates of grid_sample(align_corners=True) for ndc in (-1, 1), border padding:
// px = (ndc + 1) / 2 * (W - 1); corner weights as ATen's (nw = (x1 - px)(y1 - py), ...)
struct Tap {
    int64_t i00, i01, i10, i11;
    float w00, w01, w10, w11;
};

__device__ inline Tap bilinear_tap(float nx, float ny, int H, int W) {
    const float px = (nx + 1.f) * 0.5f * (float)(W - 1), py = (ny + 1.f) * 0.5f * (float)(H - 1);
    const int x0 = min((int)px, W - 1), y0 = min((int)py, H - 1);      // px, py >= 0: truncation = floor
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);        // (a clamped corner carries weight 0)
    const float ax = px - (float)x0, bx = (float)(x0 + 1) - px, ay = py - (float)y0, by = (float)(y0 + 1) - py;
    Tap t;
    t.i00 = (int64_t)y0 * W + x0; t.i01 = (int64_t)y0 * W + x1; t.i10 = (int64_t)y1 * W + x0; t.i11 = (int64_t)y1 * W + x1;
    t.w00 = bx * by; t.w01 = ax * by; t.w10 = bx * ay; t.w11 = ax * ay;
    return t;
}

__device__ inline float tap(const float* __restrict__ img, const Tap& t) {
    return img[t.i00] * t.w00 + img[t.i01] * t.w01 + img[t.i10] * t.w10 + img[t.i11] * t.w11;
}

// (x, y, w) of a world point; false when the view does not see it (w <= 0 or ndc outside (-1, 1)); ndc out
__device__ inline bool project(const float* __restrict__ P, float px, float py, float pz, float& nx, float& ny, float& w) {
    w = P[8] * px + P[9] * py + P[10] * pz + P[11];
    if (!(w > 0.f)) return false;
    const float x = P[0] * px + P[1] * py + P[2] * pz + P[3];
    const float y = P[4] * px + P[5] * py + P[6] * pz + P[7];
    nx = x / w; ny = y / w;
    return nx > -1.f && nx < 1.f && ny > -1.f && ny < 1.f;
}

// world position of lattice coordinate (fx, fy, fz) (fractional along an edge): contracted s, uncontracted, unnormalised
__device__ inline void lattice_world(const Lat& L, float fx, float fy, float fz, float p[3], float* mag_out) {
    const float s[3] = {-L.R + fx * L.step, -L.R + fy * L.step, -L.R + fz * L.step};
    const float mag = sqrtf(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    const float k = mag < 1.f ? 1.f : 1.f / (2.f - mag) / mag;
    p[0] = L.cx + L.radius * (s[0] * k); p[1] = L.cy + L.radius * (s[1] * k); p[2] = L.cz + L.radius * (s[2] * k);
    *mag_out = mag;
}

// One thread per sample, workgroups on 8 x 8 x 4 bricks; every view in order, the running sum and count in registers.
__global__ void __launch_bounds__(UT) unb_fuse_kernel(Lat L, int nviews, const surfel_unbounded_view* __restrict__ views,
                                                      const float* __restrict__ depth, float* __restrict__ tsdf, uint16_t* __restrict__ count) {
    const int x = blockIdx.x * FBX + (threadIdx.x & 7), y = blockIdx.y * FBY + ((threadIdx.x >> 3) & 7), z = blockIdx.z * FBZ + (threadIdx.x >> 6);
    if (x >= L.M || y >= L.M || z >= L.M) return;
    float p[3], mag;
    lattice_world(L, (float)x, (float)y, (float)z, p, &mag);
    float trunc = 5.f * L.vs;
    if (mag > 1.f) trunc *= 1.f / (2.f - fminf(mag, 1.9f));      // adaptive truncation in the contracted shell
    float sum = -1.f;                                             // the initial state: tsdf -1 with weight 1
    int n = 0;
    for (int v = 0; v < nviews; v++) {
        const surfel_unbounded_view& V = views[v];
        float nx, ny, w;
        if (!project(V.proj, p[0], p[1], p[2], nx, ny, w)) continue;
        const Tap t = bilinear_tap(nx, ny, V.H, V.W);
        const float sdf = tap(depth + V.offset, t) - w;
        if (!(sdf > -trunc)) continue;
        sum += fminf(fmaxf(sdf / trunc, -1.f), 1.f);
        n++;
    }
    const int64_t i = (int64_t)x + (int64_t)L.M * ((int64_t)y + (int64_t)L.M * z);
    tsdf[i] = sum / (float)(1 + n);
    if (count) count[i] = (uint16_t)n;
}

// ---- extraction ------------------------------------------------------------------------------------------------------------------
// A slab covers cube planes [z0, z1) and keeps scratch for sample planes z0 .. z1 (local l = z - z0); sample (x, y, l) at
// x + M (y + M l).  info = cube case | vertex-edge mask << 8 | cube << 11.  A sample owns its +x, +y, +z edges; every lattice edge
// with a sign change gets a vertex (every cube is valid: every sample has weight >= 1).
__global__ void __launch_bounds__(UT) unb_count_kernel(Lat L, int z0, int z1, const float* __restrict__ tsdf, uint32_t* __restrict__ info,
                                                       uint32_t* __restrict__ vcnt, uint32_t* __restrict__ tcnt) {
    const int64_t M = L.M, M2 = M * M;
    const int64_t k = (int64_t)blockIdx.x * UT + threadIdx.x;
    if (k >= (int64_t)(z1 - z0 + 1) * M2) return;
    const uint32_t r = (uint32_t)k / (uint32_t)M;      // (k < SLAB_MAX: 32-bit division)
    const int x = (int)((uint32_t)k - r * (uint32_t)M), y = (int)(r % (uint32_t)M), l = (int)(r / (uint32_t)M);
    const int z = z0 + l;
    const int64_t g = (int64_t)x + M * ((int64_t)y + M * z);
    const bool in0 = tsdf[g] < 0.f;
    uint32_t mask = 0;
    if (x + 1 < M && (tsdf[g + 1] < 0.f) != in0) mask |= 1u;
    if (y + 1 < M && (tsdf[g + M] < 0.f) != in0) mask |= 2u;
    if (z + 1 < M && (tsdf[g + M2] < 0.f) != in0) mask |= 4u;
    uint32_t code = mask << 8, nt = 0;
    if (z < z1 && x + 1 < M && y + 1 < M) {
        uint32_t cs = 0;
        for (int c = 0; c < 8; c++)
            if (tsdf[g + (c & 1) + M * ((c >> 1) & 1) + M2 * ((c >> 2) & 1)] < 0.f) cs |= 1u << c;
        code |= cs | 1u << 11;
        nt = MC_NTRI[cs];
    }
    info[k] = code;
    vcnt[k] = __popc(mask);
    tcnt[k] = nt;
}

// per-slab vertex and triangle counts after the scans: the vertices of sample planes z0 .. z1 - 1 (and of plane z1 = M - 1 in the
// last slab), the triangles of cube planes z0 .. z1 - 1
__global__ void unb_slab_total_kernel(int64_t n, int64_t plane_end, int last, const uint32_t* __restrict__ info, const uint32_t* __restrict__ vbase,
                                      const uint32_t* __restrict__ tbase, int64_t* __restrict__ out) {
    if (threadIdx.x != 0) return;
    out[0] = last ? (int64_t)vbase[n - 1] + __popc(info[n - 1] >> 8 & 7u) : (int64_t)vbase[plane_end];
    out[1] = tbase[n - 1];      // (the last plane holds no cube)
}

__global__ void __launch_bounds__(UT) unb_emit_kernel(Lat L, int z0, int z1, int last, const float* __restrict__ tsdf, const uint32_t* __restrict__ info,
                                                      const uint32_t* __restrict__ vbase, const uint32_t* __restrict__ tbase,
                                                      const int64_t* __restrict__ base, float* __restrict__ verts, int32_t* __restrict__ tris) {
    const int64_t M = L.M, M2 = M * M;
    const int64_t k = (int64_t)blockIdx.x * UT + threadIdx.x;
    const int nl = z1 - z0 + (last ? 1 : 0);      // sample planes this slab owns
    if (k >= (int64_t)nl * M2) return;
    const uint32_t r = (uint32_t)k / (uint32_t)M;
    const int x = (int)((uint32_t)k - r * (uint32_t)M), y = (int)(r % (uint32_t)M), l = (int)(r / (uint32_t)M);
    const int z = z0 + l;
    const int64_t g = (int64_t)x + M * ((int64_t)y + M * z);
    const uint32_t code = info[k];
    const int64_t vb = base[0], tb = base[1];
    const uint32_t mask = code >> 8 & 7u;
    if (mask) {
        int64_t vo = vb + vbase[k];
        const float ta = tsdf[g];
        for (int a = 0; a < 3; a++) {
            if (!(mask >> a & 1u)) continue;
            const float tb_ = tsdf[g + (a == 0 ? 1 : a == 1 ? M : M2)];
            const float sv = ta / (ta - tb_);
            float q[3] = {(float)x, (float)y, (float)z};
            q[a] += sv;
            float p[3], mag;
            lattice_world(L, q[0], q[1], q[2], p, &mag);
            for (int j = 0; j < 3; j++) verts[3 * vo + j] = fminf(fmaxf(p[j], -32.f), 32.f);      // max_range
            vo++;
        }
    }
    if (!(code >> 11 & 1u)) return;
    mc_write_triangles(code & 255u, tris + 3 * (tb + tbase[k]), [&](const uint8_t* e) {
        const int64_t o = k + e[0] + M * e[1] + M2 * e[2];      // the edge's owner (plane l + 1 <= z1 - z0 is in the scratch)
        return vb + vbase[o] + __popc(info[o] >> 8 & ((1u << e[3]) - 1u));
    });
}

// ---- vertex colours ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(UT) unb_color_kernel(int64_t V, const float* __restrict__ verts, int nviews, const surfel_unbounded_view* __restrict__ views,
                                                       const float* __restrict__ depth, const float* __restrict__ rgb, float trunc,
                                                       float* __restrict__ colors) {
    const int64_t i = (int64_t)blockIdx.x * UT + threadIdx.x;
    if (i >= V) return;
    const float px = verts[3 * i], py = verts[3 * i + 1], pz = verts[3 * i + 2];
    float r = 0.f, g = 0.f, b = 0.f;      // the initial state: rgb 0 with weight 1
    int n = 0;
    for (int v = 0; v < nviews; v++) {
        const surfel_unbounded_view& Vw = views[v];
        float nx, ny, w;
        if (!project(Vw.proj, px, py, pz, nx, ny, w)) continue;
        const Tap t = bilinear_tap(nx, ny, Vw.H, Vw.W);
        if (!(tap(depth + Vw.offset, t) - w > -trunc)) continue;
        const int64_t hw = (int64_t)Vw.H * Vw.W;
        const float* c = rgb + 3 * Vw.offset;
        r += tap(c, t); g += tap(c + hw, t); b += tap(c + 2 * hw, t);
        n++;
    }
    const float inv = 1.f / (float)(1 + n);
    colors[3 * i] = r * inv; colors[3 * i + 1] = g * inv; colors[3 * i + 2] = b * inv;
}

inline unsigned grid(int64_t n) { return blocks_for(n, UT); }

inline Lat lat_of(const surfel_unbounded_volume* v) {
    return Lat{v->M, v->R, 2.f * v->R / (float)(v->M - 1), v->center[0], v->center[1], v->center[2], v->radius, v->voxel_size};
}

// the effective slab height: `slab` cube planes (0: about SLAB_DEFAULT samples), within [1, M - 1] and SLAB_MAX scratch samples
inline int slab_planes(const surfel_unbounded_volume* v) {
    const int64_t M2 = (int64_t)v->M * v->M;
    int64_t h = v->slab > 0 ? v->slab : SLAB_DEFAULT / M2;
    h = std::min<int64_t>(h, SLAB_MAX / M2 - 1);
    h = std::min<int64_t>(h, v->M - 1);
    return (int)std::max<int64_t>(h, 1);
}
inline int64_t nslabs_of(const surfel_unbounded_volume* v) { return (v->M - 2) / slab_planes(v) + 1; }
inline int64_t scratch_n(const surfel_unbounded_volume* v) { return (int64_t)(slab_planes(v) + 1) * v->M * v->M; }
inline bool fields_ok(const surfel_unbounded_volume* v) {
    return v && v->M >= 2 && v->M <= MAX_M && v->R > 0.f && v->R < 2.f && v->radius > 0.f && v->voxel_size > 0.f && v->slab >= 0;
}

// count kernel and both scans of slab s (cube planes z0 .. z1 - 1)
void count_slab(const surfel_unbounded_volume* v, int64_t s, int& z0, int& z1, hipStream_t st) {
    const int h = slab_planes(v);
    z0 = (int)(s * h);
    z1 = std::min(z0 + h, v->M - 1);
    const int64_t n = (int64_t)(z1 - z0 + 1) * v->M * v->M;
    hipLaunchKernelGGL(unb_count_kernel, dim3(grid(n)), dim3(UT), 0, st, lat_of(v), z0, z1, v->tsdf, v->info, v->vbase, v->tbase);
    scan_u32(v->vbase, n, v->scan_scratch, st);
    scan_u32(v->tbase, n, v->scan_scratch, st);
}

}  // namespace
}  // namespace surfel

// ================================================================================================================ C ABI
using namespace surfel;

extern "C" {

int64_t surfel_unbounded_bytes(const surfel_unbounded_volume* v) {
    if (!fields_ok(v)) return api_fail(SURFEL_E_INVALID, "unbounded_bytes: bad volume fields (2 <= M <= 2048, 0 < R < 2, radius, voxel_size > 0)");
    const int64_t M = v->M, n = scratch_n(v);
    return 4 * M * M * M + 12 * n + 4 * scan_scratch_u32(n) + 8 * (2 * nslabs_of(v) + 2);
}

int surfel_unbounded_init(surfel_unbounded_volume* v, surfel_alloc_fn alloc, void* user, void* stream) {
    if (!fields_ok(v) || !alloc) return api_fail(SURFEL_E_INVALID, "unbounded_init: bad arguments");
    if (surfel_unbounded_bytes(v) > v->budget_bytes)
        return api_fail(SURFEL_E_LIMIT, "unbounded_init: the lattice and its slab scratch exceed the byte budget (raise the budget or lower the resolution)");
    const int64_t M = v->M, n = scratch_n(v);
    v->slab = slab_planes(v);
    v->nslabs = nslabs_of(v);
    v->nverts = v->ntris = 0;
    v->tsdf = take<float>(alloc, user, M * M * M);
    v->info = take<uint32_t>(alloc, user, n);
    v->vbase = take<uint32_t>(alloc, user, n);
    v->tbase = take<uint32_t>(alloc, user, n);
    v->scan_scratch = take<uint32_t>(alloc, user, scan_scratch_u32(n));
    v->slab_base = take<int64_t>(alloc, user, 2 * v->nslabs + 2);
    if (!v->tsdf || !v->info || !v->vbase || !v->tbase || !v->scan_scratch || !v->slab_base)
        return api_fail(SURFEL_E_ALLOC, "unbounded_init: allocator returned NULL");
    (void)stream;
    return 0;
}

int surfel_unbounded_fuse(surfel_unbounded_volume* v, int nviews, const surfel_unbounded_view* views, const float* depth, uint16_t* count,
                          void* stream) {
    if (!fields_ok(v) || !v->tsdf || nviews < 0 || (nviews > 0 && (!views || !depth)) || (count && nviews > 65535))
        return api_fail(SURFEL_E_INVALID, "unbounded_fuse: bad arguments");
    const unsigned gx = (unsigned)((v->M + FBX - 1) / FBX), gz = (unsigned)((v->M + FBZ - 1) / FBZ);
    hipLaunchKernelGGL(unb_fuse_kernel, dim3(gx, gx, gz), dim3(UT), 0, static_cast<hipStream_t>(stream), lat_of(v), nviews, views, depth, v->tsdf, count);
    return launched("unb_fuse_kernel");
}

int surfel_unbounded_count(surfel_unbounded_volume* v, void* stream) {
    if (!fields_ok(v) || !v->tsdf || !v->slab_base) return api_fail(SURFEL_E_INVALID, "unbounded_count: bad arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t ns = v->nslabs, M2 = (int64_t)v->M * v->M;
    for (int64_t s = 0; s < ns; s++) {
        int z0, z1;
        count_slab(v, s, z0, z1, st);
        const int64_t n = (int64_t)(z1 - z0 + 1) * M2;
        hipLaunchKernelGGL(unb_slab_total_kernel, dim3(1), dim3(64), 0, st, n, (int64_t)(z1 - z0) * M2, (int)(s == ns - 1), v->info, v->vbase,
                           v->tbase, v->slab_base + 2 * s);
    }
    std::vector<int64_t> b((size_t)(2 * ns + 2));
    if (hipMemcpyAsync(b.data(), v->slab_base, (size_t)(2 * ns) * 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return api_fail(SURFEL_E_HIP, "unbounded_count: copy", hipGetLastError());
    int64_t V = 0, F = 0;
    for (int64_t s = 0; s < ns; s++) {      // per-slab counts -> exclusive bases, totals last
        const int64_t cv = b[2 * s], ct = b[2 * s + 1];
        b[2 * s] = V; b[2 * s + 1] = F;
        V += cv; F += ct;
    }
    b[2 * ns] = V; b[2 * ns + 1] = F;
    if (V > MAX_INDEX || F > MAX_INDEX)
        return api_fail(SURFEL_E_LIMIT, "unbounded_count: more vertices or triangles than 32-bit indices can address (lower the resolution)");
    if (surfel_unbounded_bytes(v) + 24 * V + 12 * F > v->budget_bytes)
        return api_fail(SURFEL_E_LIMIT, "unbounded_count: the lattice, its scratch and the mesh exceed the byte budget (raise the budget)");
    if (hipMemcpyAsync(v->slab_base, b.data(), b.size() * 8, hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return api_fail(SURFEL_E_HIP, "unbounded_count: copy", hipGetLastError());
    v->nverts = V; v->ntris = F;
    return launched("unb_count_kernel");
}

int surfel_unbounded_extract(const surfel_unbounded_volume* v, float* verts, int32_t* tris, void* stream) {
    if (!fields_ok(v) || !v->tsdf || !v->slab_base) return api_fail(SURFEL_E_INVALID, "unbounded_extract: bad arguments");
    if (v->nverts == 0 && v->ntris == 0) return 0;
    if (!verts || !tris) return api_fail(SURFEL_E_INVALID, "unbounded_extract: null output");
    if (v->slab != slab_planes(v) || v->nslabs != nslabs_of(v)) return api_fail(SURFEL_E_INVALID, "unbounded_extract: the slab changed after counting");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t ns = v->nslabs, M2 = (int64_t)v->M * v->M;
    for (int64_t s = 0; s < ns; s++) {
        int z0, z1;
        count_slab(v, s, z0, z1, st);
        const int last = s == ns - 1;
        const int64_t n = (int64_t)(z1 - z0 + last) * M2;
        hipLaunchKernelGGL(unb_emit_kernel, dim3(grid(n)), dim3(UT), 0, st, lat_of(v), z0, z1, last, v->tsdf, v->info, v->vbase, v->tbase,
                           v->slab_base + 2 * s, verts, tris);
    }
    return launched("unb_emit_kernel");
}

int surfel_unbounded_color(int64_t V, const float* verts, int nviews, const surfel_unbounded_view* views, const float* depth, const float* rgb,
                           float sdf_trunc, float* colors, void* stream) {
    if (V < 0 || nviews < 0 || (V > 0 && (!verts || !colors)) || (nviews > 0 && (!views || !depth || !rgb)) || !(sdf_trunc > 0.f))
        return api_fail(SURFEL_E_INVALID, "unbounded_color: bad arguments");
    if (V == 0) return 0;
    hipLaunchKernelGGL(unb_color_kernel, dim3(grid(V)), dim3(UT), 0, static_cast<hipStream_t>(stream), V, verts, nviews, views, depth, rgb, sdf_trunc,
                       colors);
    return launched("unb_color_kernel");
}

}  // extern "C"
