// mesh_tsdf.hip — bounded TSDF fusion, marching cubes and the connected-component filter (include/surfel_mesh.h, MESH.md).
// All kernels are memory-bound gathers / streams; no MFMA.  Compiled with -ffp-contract=off (build.py) so that the allocation pass
// rounds exactly as its fp32 restatement in tests/mesh_oracle.py.
#include <hip/hip_runtime.h>

#include "../../include/surfel_mesh.h"
#include "mesh_mc.h"
#include "mesh_topology.h"

namespace surfel {

constexpr int MB = SURFEL_TSDF_BLOCK;            // voxels per block edge
constexpr int MV = MB * MB * MB;                 // voxels per block (4096)
constexpr int MT = 256;                          // threads per workgroup: 16 voxels per thread
// V and F index with int32 and every voxel emits at most 3 vertices and MC_MAX_TRI triangles
constexpr int64_t MAX_BLOCKS = ((int64_t)1 << 31) / ((int64_t)MV * MC_MAX_TRI);

struct Vol {      // what the kernels need of surfel_tsdf_volume
    int ox, oy, oz, nx, ny, nz;
    float vs, trunc;
    const int32_t* table;
};

__device__ inline int table_index(const Vol& v, int bx, int by, int bz) {      // block coordinates -> table entry, -1 outside
    bx -= v.ox; by -= v.oy; bz -= v.oz;
    if (bx < 0 || by < 0 || bz < 0 || bx >= v.nx || by >= v.ny || bz >= v.nz) return -1;
    return bx + v.nx * (by + v.ny * bz);
}

// slot * 4096 + voxel-in-block of the global voxel (gx, gy, gz), or -1 when its block is not allocated
__device__ inline int64_t voxel_at(const Vol& v, int gx, int gy, int gz) {
    const int t = table_index(v, gx >> 4, gy >> 4, gz >> 4);      // (arithmetic shift = floor division for negative voxels)
    if (t < 0) return -1;
    const int s = v.table[t];
    if (s < 0) return -1;
    return (int64_t)s * MV + (gx & 15) + 16 * (gy & 15) + 256 * (gz & 15);
}

// ---- view preparation ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MT) mesh_prepare_kernel(int n, const float* __restrict__ depth, const float* __restrict__ rgb,
                                                          const float* __restrict__ mask, float depth_trunc, float* __restrict__ dout,
                                                          uint32_t* __restrict__ rgba) {
    const int i = blockIdx.x * MT + threadIdx.x;
    if (i >= n) return;
    float d = depth[i];
    if (!(d <= depth_trunc) || (mask && mask[i] < 0.5f)) d = 0.f;      // (NaN compares false: a hole too)
    dout[i] = d;
    uint32_t packed = 0;
    for (int c = 0; c < 3; c++) {
        const float x = fminf(fmaxf(rgb[(size_t)c * n + i], 0.f), 1.f) * 255.f;
        packed |= (uint32_t)x << (8 * c);      // truncation, as numpy's astype(np.uint8)
    }
    rgba[i] = packed;
}

// ---- allocation ----------------------------------------------------------------------------------------------------------
struct Cam {
    float r[9], t[3], fx, fy, cx, cy;
};
__device__ inline Cam load_cam(const float* __restrict__ c) {
    Cam k;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) k.r[3 * i + j] = c[4 * i + j];
        k.t[i] = c[4 * i + 3];
    }
    k.fx = c[12]; k.fy = c[13]; k.cx = c[14]; k.cy = c[15];
    return k;
}

// a block coordinate clamped to the table's range [o, o + n - 1] (lo side: to o; hi side: to o + n - 1), NaN-safe
__device__ inline int clamp_block(float b, int o, int n, int hi_side) {
    if (!(b >= (float)o)) return hi_side ? o - 1 : o;
    if (!(b <= (float)(o + n - 1))) return hi_side ? o + n - 1 : o + n;
    return (int)b;
}

// the block range [lo, hi] (block coordinates) a valid pixel touches; false for an invalid pixel
__device__ inline bool pixel_blocks(const Vol& v, const Cam& k, int u, int w, float d, int lo[3], int hi[3]) {
    if (!(d > 0.f)) return false;
    const float pc[3] = {((float)u - k.cx) * d / k.fx, ((float)w - k.cy) * d / k.fy, d};
    const float q[3] = {pc[0] - k.t[0], pc[1] - k.t[1], pc[2] - k.t[2]};
    const float bs = v.vs * (float)MB;
    for (int j = 0; j < 3; j++) {
        const float x = k.r[j] * q[0] + k.r[3 + j] * q[1] + k.r[6 + j] * q[2];      // R^T (p - t)
        lo[j] = clamp_block(floorf((x - v.trunc) / bs), j == 0 ? v.ox : j == 1 ? v.oy : v.oz, j == 0 ? v.nx : j == 1 ? v.ny : v.nz, 0);
        hi[j] = clamp_block(floorf((x + v.trunc) / bs), j == 0 ? v.ox : j == 1 ? v.oy : v.oz, j == 0 ? v.nx : j == 1 ? v.ny : v.nz, 1);
    }
    return true;      // (an empty range when the point lies outside the table: lo > hi)
}

__global__ void __launch_bounds__(MT) mesh_mark_kernel(Vol v, int H, int W, const float* __restrict__ depth, const float* __restrict__ cam,
                                                       int32_t* __restrict__ table) {
    const int i = blockIdx.x * MT + threadIdx.x;
    if (i >= H * W) return;
    const Cam k = load_cam(cam);
    int lo[3], hi[3];
    if (!pixel_blocks(v, k, i % W, i / W, depth[i], lo, hi)) return;
    for (int z = lo[2]; z <= hi[2]; z++)
        for (int y = lo[1]; y <= hi[1]; y++)
            for (int x = lo[0]; x <= hi[0]; x++) {
                const int t = table_index(v, x, y, z);
                if (t >= 0 && table[t] != -2) table[t] = -2;      // marked (same value from every thread: no atomics needed)
            }
}

__global__ void __launch_bounds__(MT) mesh_flag_kernel(int64_t n, const int32_t* __restrict__ table, uint32_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * MT + threadIdx.x;
    if (i < n) flags[i] = table[i] == -2 ? 1u : 0u;
}

__global__ void __launch_bounds__(MT) mesh_assign_kernel(int64_t n, int32_t* __restrict__ table, const uint32_t* __restrict__ slot,
                                                         int32_t* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * MT + threadIdx.x;
    if (i >= n || table[i] != -2) return;
    table[i] = (int32_t)slot[i];
    keys[slot[i]] = (int32_t)i;
}

// ---- integration ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MT) mesh_touch_kernel(Vol v, int H, int W, const float* __restrict__ depth, const float* __restrict__ cam,
                                                        uint32_t view, uint32_t* __restrict__ stamp, uint32_t* __restrict__ list) {
    const int i = blockIdx.x * MT + threadIdx.x;
    if (i >= H * W) return;
    const Cam k = load_cam(cam);
    int lo[3], hi[3];
    if (!pixel_blocks(v, k, i % W, i / W, depth[i], lo, hi)) return;
    for (int z = lo[2]; z <= hi[2]; z++)
        for (int y = lo[1]; y <= hi[1]; y++)
            for (int x = lo[0]; x <= hi[0]; x++) {
                const int t = table_index(v, x, y, z);
                if (t < 0) continue;
                const int s = v.table[t];
                if (s < 0) continue;      // (every touched block was marked by the same pass over the same view)
                // (a plain read first: the thousands of pixels that fall into one block then skip the atomic; a stale read only
                // sends a thread to atomicExch, which alone decides)
                if (stamp[s] != view && atomicExch(&stamp[s], view) != view)
                    list[1 + atomicAdd(&list[0], 1u)] = (uint32_t)s;
            }
}

// One workgroup per touched block; thread t owns voxels t + 256 k (k = z), so each wave's record loads and stores are one
// contiguous 1 KiB dwordx4 stream (tsdf, r, g, b) and one 256 B dword stream (weight).
__global__ void __launch_bounds__(MT) mesh_integrate_kernel(Vol v, int H, int W, const float* __restrict__ depth, const uint32_t* __restrict__ rgba,
                                                            const float* __restrict__ cam, const uint32_t* __restrict__ list,
                                                            const int32_t* __restrict__ keys, float4* __restrict__ trgb, float* __restrict__ wgt) {
    if (blockIdx.x >= list[0]) return;
    const int s = (int)list[1 + blockIdx.x];
    const int key = keys[s];
    const int bx = v.ox + key % v.nx, by = v.oy + (key / v.nx) % v.ny, bz = v.oz + key / (v.nx * v.ny);
    const Cam k = load_cam(cam);
    const int x = MB * bx + (threadIdx.x & 15), y = MB * by + (threadIdx.x >> 4);
    const float cx = ((float)x + 0.5f) * v.vs, cy = ((float)y + 0.5f) * v.vs;
    for (int z = 0; z < MB; z++) {
        const float cz = ((float)(MB * bz + z) + 0.5f) * v.vs;
        const float pz = k.r[6] * cx + k.r[7] * cy + k.r[8] * cz + k.t[2];
        if (!(pz > 0.f)) continue;
        const float px = k.r[0] * cx + k.r[1] * cy + k.r[2] * cz + k.t[0];
        const float py = k.r[3] * cx + k.r[4] * cy + k.r[5] * cz + k.t[1];
        const float uf = floorf(k.fx * px / pz + k.cx + 0.5f), vf = floorf(k.fy * py / pz + k.cy + 0.5f);
        if (!(uf >= 0.f && vf >= 0.f && uf < (float)W && vf < (float)H)) continue;
        const int pix = (int)vf * W + (int)uf;
        const float d = depth[pix];
        if (!(d > 0.f)) continue;      // valid means d > 0, as in pixel_blocks: zero, negative and NaN depths are holes
        const float a = (uf - k.cx) / k.fx, b = (vf - k.cy) / k.fy;
        const float sdf = (d - pz) * sqrtf(1.f + a * a + b * b);
        if (sdf <= -v.trunc) continue;
        const float t = fminf(1.f, sdf / v.trunc);
        const uint32_t c = rgba[pix];
        const int64_t vi = (int64_t)s * MV + threadIdx.x + MT * z;
        float4 r = trgb[vi];
        const float w = wgt[vi], w1 = w + 1.f;
        r.x = (r.x * w + t) / w1;
        r.y = (r.y * w + (float)(c & 255u)) / w1;
        r.z = (r.z * w + (float)((c >> 8) & 255u)) / w1;
        r.w = (r.w * w + (float)((c >> 16) & 255u)) / w1;
        trgb[vi] = r;
        wgt[vi] = w1;
    }
}

// ---- extraction ----------------------------------------------------------------------------------------------------------
__device__ inline void block_origin(const Vol& v, const int32_t* keys, int s, int& x, int& y, int& z) {
    const int key = keys[s];
    x = MB * (v.ox + key % v.nx); y = MB * (v.oy + (key / v.nx) % v.ny); z = MB * (v.oz + key / (v.nx * v.ny));
}

// cube case and validity of the cube whose lowest corner is voxel (x, y, z): case | 1 << 8 when all 8 corners are allocated with w > 0
__global__ void __launch_bounds__(MT) mesh_classify_kernel(Vol v, const int32_t* __restrict__ keys, const float4* __restrict__ trgb,
                                                           const float* __restrict__ wgt, uint32_t* __restrict__ info) {
    const int s = blockIdx.x;
    int x0, y0, z0;
    block_origin(v, keys, s, x0, y0, z0);
    const int x = x0 + (threadIdx.x & 15), y = y0 + (threadIdx.x >> 4);
    for (int z = 0; z < MB; z++) {
        uint32_t code = 1u << 8;
        for (int c = 0; c < 8; c++) {
            const int64_t i = voxel_at(v, x + (c & 1), y + ((c >> 1) & 1), z0 + z + ((c >> 2) & 1));
            if (i < 0 || !(wgt[i] > 0.f)) { code = 0; break; }
            if (trgb[i].x < 0.f) code |= 1u << c;
        }
        info[(int64_t)s * MV + threadIdx.x + MT * z] = code;
    }
}

// the vertex edges a voxel owns (+x, +y, +z edges with a crossing that a valid cube uses) and the per-voxel counts
__global__ void __launch_bounds__(MT) mesh_count_kernel(Vol v, const int32_t* __restrict__ keys, const float4* __restrict__ trgb,
                                                        const float* __restrict__ wgt, uint32_t* __restrict__ info, uint32_t* __restrict__ vcnt,
                                                        uint32_t* __restrict__ tcnt) {
    const int s = blockIdx.x;
    int x0, y0, z0;
    block_origin(v, keys, s, x0, y0, z0);
    const int x = x0 + (threadIdx.x & 15), y = y0 + (threadIdx.x >> 4);
    for (int z = 0; z < MB; z++) {
        const int64_t me = (int64_t)s * MV + threadIdx.x + MT * z;
        const int gz = z0 + z;
        uint32_t code = info[me], mask = 0;
        if (wgt[me] > 0.f) {
            const bool in0 = trgb[me].x < 0.f;
            for (int a = 0; a < 3; a++) {
                const int64_t o = voxel_at(v, x + (a == 0), y + (a == 1), gz + (a == 2));
                if (o < 0 || !(wgt[o] > 0.f) || (trgb[o].x < 0.f) == in0) continue;
                // the four cubes that share the edge: lowest corners me - {0, e1} - {0, e2}
                const int a1 = a == 0 ? 1 : 0, a2 = a == 2 ? 1 : 2;
                bool used = false;
                for (int q = 0; q < 4 && !used; q++) {
                    int p[3] = {x, y, gz};
                    p[a1] -= q & 1; p[a2] -= q >> 1;
                    const int64_t c = voxel_at(v, p[0], p[1], p[2]);
                    used = c >= 0 && (info[c] >> 8 & 1u);
                }
                if (used) mask |= 1u << a;
            }
        }
        info[me] = code | mask << 9;
        vcnt[me] = __popc(mask);
        tcnt[me] = (code >> 8 & 1u) ? MC_NTRI[code & 255u] : 0u;
    }
}

__global__ void __launch_bounds__(MT) mesh_emit_kernel(Vol v, const int32_t* __restrict__ keys, const float4* __restrict__ trgb,
                                                       const uint32_t* __restrict__ info, const uint32_t* __restrict__ vbase,
                                                       const uint32_t* __restrict__ tbase, float* __restrict__ verts, float* __restrict__ colors,
                                                       int32_t* __restrict__ tris) {
    const int s = blockIdx.x;
    int x0, y0, z0;
    block_origin(v, keys, s, x0, y0, z0);
    const int x = x0 + (threadIdx.x & 15), y = y0 + (threadIdx.x >> 4);
    for (int z = 0; z < MB; z++) {
        const int64_t me = (int64_t)s * MV + threadIdx.x + MT * z;
        const int gz = z0 + z;
        const uint32_t code = info[me];
        uint32_t vo = vbase[me];
        const uint32_t mask = code >> 9 & 7u;
        if (mask) {
            const float4 ra = trgb[me];
            for (int a = 0; a < 3; a++) {
                if (!(mask >> a & 1u)) continue;
                const float4 rb = trgb[voxel_at(v, x + (a == 0), y + (a == 1), gz + (a == 2))];
                const float sv = ra.x / (ra.x - rb.x);
                float p[3] = {(float)x + 0.5f, (float)y + 0.5f, (float)gz + 0.5f};
                p[a] += sv;
                for (int j = 0; j < 3; j++) verts[3 * (size_t)vo + j] = p[j] * v.vs;
                colors[3 * (size_t)vo + 0] = ((1.f - sv) * ra.y + sv * rb.y) / 255.f;
                colors[3 * (size_t)vo + 1] = ((1.f - sv) * ra.z + sv * rb.z) / 255.f;
                colors[3 * (size_t)vo + 2] = ((1.f - sv) * ra.w + sv * rb.w) / 255.f;
                vo++;
            }
        }
        if (!(code >> 8 & 1u)) continue;
        mc_write_triangles(code & 255u, tris + 3 * (size_t)tbase[me], [&](const uint8_t* e) {
            const int64_t o = voxel_at(v, x + e[0], y + e[1], gz + e[2]);      // the edge's owner: allocated, the cube is valid
            return vbase[o] + __popc(info[o] >> 9 & ((1u << e[3]) - 1u));
        });
    }
}

// ---- connected components over shared edges -------------------------------------------------------------------------------
// (min, max) key of edge e; an edge with an endpoint outside [0, V) (a negative id is a large unsigned one) gets the key (V, V), which
// sorts behind every valid group and links nothing
__device__ inline uint64_t edge_key(const int32_t* tris, uint32_t e, uint32_t V) {
    uint32_t a, b;
    half_edge_ends(tris, e, &a, &b);
    if (a >= V || b >= V) return (uint64_t)V << 32 | V;
    return a < b ? ((uint64_t)a << 32 | b) : ((uint64_t)b << 32 | a);
}

struct EdgeKey {      // the sort's key of an edge: word 0 = max, word 1 = min
    const int32_t* tris;
    uint32_t V;
    __device__ uint32_t operator()(uint32_t e, int word) const { return key_word(edge_key(tris, e, V), word); }
};

__global__ void __launch_bounds__(MT) edge_keys_kernel(int64_t F, EdgeKey key_of, uint32_t* __restrict__ key, uint32_t* __restrict__ val) {
    const int64_t e = (int64_t)blockIdx.x * MT + threadIdx.x;
    if (e >= 3 * F) return;
    key[e] = key_of((uint32_t)e, 0);      // the low half of the (min, max) key: sorted first
    val[e] = (uint32_t)e;
}

__device__ inline int32_t uf_find(const int32_t* parent, int32_t x) {
    int32_t p = parent[x];
    while (p != x) { x = p; p = parent[x]; }
    return x;
}

// hooking: the larger root goes under the smaller, so every cluster's root ends as its smallest triangle id
__global__ void __launch_bounds__(MT) uf_hook_kernel(int64_t n, uint32_t V, const int32_t* __restrict__ tris, const uint32_t* __restrict__ val, int32_t* parent) {
    const int64_t k = (int64_t)blockIdx.x * MT + threadIdx.x;
    if (k == 0 || k >= n) return;
    const uint64_t key = edge_key(tris, val[k], V);
    if (key >> 32 == V || key != edge_key(tris, val[k - 1], V)) return;      // (an edge with an id out of range links nothing)
    int32_t a = (int32_t)(val[k] / 3), b = (int32_t)(val[k - 1] / 3);
    while (true) {
        a = uf_find(parent, a); b = uf_find(parent, b);
        if (a == b) return;
        if (a < b) { const int32_t t = a; a = b; b = t; }
        const int32_t old = atomicCAS(&parent[a], a, b);
        if (old == a) return;
        a = old;
    }
}

__global__ void __launch_bounds__(MT) uf_init_kernel(int64_t F, int32_t* __restrict__ parent, int32_t* __restrict__ size) {
    const int64_t t = (int64_t)blockIdx.x * MT + threadIdx.x;
    if (t < F) { parent[t] = (int32_t)t; size[t] = 0; }
}

// pointer jumping: every triangle's root (its cluster's smallest id), written back as its parent so later walks are short
__global__ void __launch_bounds__(MT) uf_jump_kernel(int64_t F, int32_t* parent, int32_t* __restrict__ label) {
    const int64_t t = (int64_t)blockIdx.x * MT + threadIdx.x;
    if (t >= F) return;
    const int32_t r = uf_find(parent, (int32_t)t);
    parent[t] = r;      // (a racing walk reads the old or the new parent: both lie on the path to r)
    label[t] = r;
}

// cluster sizes: the triangles of a cluster are mostly neighbours in (cube, slot) order, so each wave adds every run of equal labels
// with one atomic from the run's first lane (one atomic per lane piled ~1e6 adds onto the largest cluster's counter)
__global__ void __launch_bounds__(MT) uf_size_kernel(int64_t F, const int32_t* __restrict__ label, int32_t* size) {
    const int64_t t = (int64_t)blockIdx.x * MT + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int32_t r = t < F ? label[t] : -1;
    const int32_t prev = __shfl_up(r, 1);
    const bool head = lane == 0 || prev != r;
    const uint64_t heads = __ballot(head);
    if (!head || r < 0) return;
    const uint64_t above = lane == 63 ? 0ull : (heads >> (lane + 1)) << (lane + 1);
    const int next = above ? __builtin_ctzll(above) : 64;
    atomicAdd(&size[r], next - lane);
}

// ---- filter ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MT) filter_mark_kernel(int64_t V, int64_t F, const int32_t* __restrict__ tris, const int32_t* __restrict__ label,
                                                         const int32_t* __restrict__ size, int threshold, uint32_t* __restrict__ tkeep,
                                                         uint32_t* __restrict__ vref) {
    const int64_t t = (int64_t)blockIdx.x * MT + threadIdx.x;
    if (t >= F) return;
    const int32_t a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
    const bool keep = size[label[t]] >= threshold && a >= 0 && b >= 0 && c >= 0 && a < V && b < V && c < V;      // (bad indices: dropped)
    if (keep) { vref[a] = 1u; vref[b] = 1u; vref[c] = 1u; }
    tkeep[t] = keep && a != b && b != c && a != c;
}

__global__ void __launch_bounds__(MT) filter_verts_kernel(int64_t V, const uint32_t* __restrict__ vflag, const uint32_t* __restrict__ vpos,
                                                          const float* __restrict__ verts, const float* __restrict__ colors,
                                                          float* __restrict__ vout, float* __restrict__ cout) {
    const int64_t i = (int64_t)blockIdx.x * MT + threadIdx.x;
    if (i >= V || !vflag[i]) return;
    const int64_t o = vpos[i];
    for (int j = 0; j < 3; j++) { vout[3 * o + j] = verts[3 * i + j]; cout[3 * o + j] = colors[3 * i + j]; }
}

__global__ void __launch_bounds__(MT) filter_tris_kernel(int64_t F, const uint32_t* __restrict__ tflag, const uint32_t* __restrict__ tpos,
                                                         const int32_t* __restrict__ tris, const uint32_t* __restrict__ vpos,
                                                         int32_t* __restrict__ tout) {
    const int64_t t = (int64_t)blockIdx.x * MT + threadIdx.x;
    if (t >= F || !tflag[t]) return;
    const int64_t o = tpos[t];
    for (int j = 0; j < 3; j++) tout[3 * o + j] = (int32_t)vpos[tris[3 * t + j]];
}

__global__ void __launch_bounds__(MT) copy_flags_kernel(int64_t n, const uint32_t* __restrict__ a, uint32_t* __restrict__ b) {
    const int64_t i = (int64_t)blockIdx.x * MT + threadIdx.x;
    if (i < n) b[i] = a[i];
}

}  // namespace surfel

// ================================================================================================================ C ABI
using namespace surfel;

namespace {
inline unsigned grid(int64_t n) { return blocks_for(n, MT); }
inline int64_t table_n(const surfel_tsdf_volume* v) { return (int64_t)v->dims[0] * v->dims[1] * v->dims[2]; }
inline Vol vol_of(const surfel_tsdf_volume* v) {
    return Vol{v->origin[0], v->origin[1], v->origin[2], v->dims[0], v->dims[1], v->dims[2], v->voxel_size, v->sdf_trunc, v->table};
}
}  // namespace

extern "C" {

int64_t surfel_tsdf_table_bytes(const surfel_tsdf_volume* v) {
    if (!v) return api_fail(SURFEL_E_INVALID, "tsdf_table_bytes: null volume");
    const int64_t n = table_n(v);
    return 8 * n + 4 * scan_scratch_u32(n);      // table + flags + scan sums
}

int64_t surfel_tsdf_block_bytes(void) { return (int64_t)MV * (16 + 4 + 12) + 12 + 4 * (MV / SCAN_TILE + 1); }

int surfel_mesh_prepare_view(int H, int W, const float* surf_depth, const float* rgb, const float* mask, float depth_trunc, float* depth_out,
                             uint32_t* rgba_out, void* stream) {
    if (H <= 0 || W <= 0 || !surf_depth || !rgb || !depth_out || !rgba_out) return api_fail(SURFEL_E_INVALID, "mesh_prepare_view: bad arguments");
    hipLaunchKernelGGL(mesh_prepare_kernel, dim3(grid((int64_t)H * W)), dim3(MT), 0, static_cast<hipStream_t>(stream), H * W, surf_depth, rgb,
                       mask, depth_trunc, depth_out, rgba_out);
    return launched("mesh_prepare_kernel");
}

int surfel_tsdf_init(surfel_tsdf_volume* v, surfel_alloc_fn alloc, void* user, void* stream) {
    if (!v || !alloc || v->dims[0] <= 0 || v->dims[1] <= 0 || v->dims[2] <= 0 || !(v->voxel_size > 0.f) || !(v->sdf_trunc > 0.f))
        return api_fail(SURFEL_E_INVALID, "tsdf_init: bad arguments");
    const int64_t n = table_n(v);
    if (n >= ((int64_t)1 << 31) || surfel_tsdf_table_bytes(v) > v->budget_bytes)
        return api_fail(SURFEL_E_LIMIT, "tsdf_init: the dense block table exceeds the byte budget (raise the budget or the voxel size)");
    v->table = take<int32_t>(alloc, user, n);
    v->scratch = take<uint32_t>(alloc, user, ScanBuf::words(n));
    if (!v->table || !v->scratch) return api_fail(SURFEL_E_ALLOC, "tsdf_init: allocator returned NULL");
    v->nblocks = 0; v->views = 0; v->nverts = v->ntris = 0;
    return hipMemsetAsync(v->table, 0xFF, (size_t)n * 4, static_cast<hipStream_t>(stream)) == hipSuccess ? 0
                                                                                                       : api_fail(SURFEL_E_HIP, "tsdf_init: memset");
}

int surfel_tsdf_mark(surfel_tsdf_volume* v, int H, int W, const float* depth, const float* cam, void* stream) {
    if (!v || !v->table || H <= 0 || W <= 0 || !depth || !cam) return api_fail(SURFEL_E_INVALID, "tsdf_mark: bad arguments");
    if (v->nblocks > 0 || v->keys) return api_fail(SURFEL_E_INVALID, "tsdf_mark: the volume is already allocated");
    hipLaunchKernelGGL(mesh_mark_kernel, dim3(grid((int64_t)H * W)), dim3(MT), 0, static_cast<hipStream_t>(stream), vol_of(v), H, W, depth, cam,
                       v->table);
    return launched("mesh_mark_kernel");
}

int64_t surfel_tsdf_allocate(surfel_tsdf_volume* v, surfel_alloc_fn alloc, void* user, void* stream) {
    if (!v || !v->table || !alloc || v->keys) return api_fail(SURFEL_E_INVALID, "tsdf_allocate: bad arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t n = table_n(v);
    const ScanBuf used(v->scratch, v->scratch + n, n);
    hipLaunchKernelGGL(mesh_flag_kernel, dim3(grid(n)), dim3(MT), 0, st, n, v->table, used.flags);
    used.scan(st);
    uint32_t nb = 0;
    if (int rc = read_words("tsdf_allocate: block count", used.total, &nb, 1, st)) return rc;
    if ((int64_t)nb > MAX_BLOCKS)
        return api_fail(SURFEL_E_LIMIT, "tsdf_allocate: more blocks than 32-bit vertex / triangle indices can address (raise the voxel size)");
    if (surfel_tsdf_table_bytes(v) + (int64_t)nb * surfel_tsdf_block_bytes() > v->budget_bytes)
        return api_fail(SURFEL_E_LIMIT, "tsdf_allocate: the voxel pool exceeds the byte budget (raise the budget or the voxel size)");
    v->nblocks = nb;
    if (nb == 0) return 0;
    const int64_t nv = (int64_t)nb * MV;
    v->keys = take<int32_t>(alloc, user, nb);
    v->stamp = take<uint32_t>(alloc, user, nb);
    v->list = take<uint32_t>(alloc, user, nb + 1);
    v->tsdf_rgb = take<float>(alloc, user, 4 * nv);
    v->weight = take<float>(alloc, user, nv);
    v->info = take<uint32_t>(alloc, user, nv);
    v->vbase = take<uint32_t>(alloc, user, nv);
    v->tbase = take<uint32_t>(alloc, user, nv);
    v->pool_scratch = take<uint32_t>(alloc, user, scan_scratch_u32(nv));
    if (!v->keys || !v->stamp || !v->list || !v->tsdf_rgb || !v->weight || !v->info || !v->vbase || !v->tbase || !v->pool_scratch)
        return api_fail(SURFEL_E_ALLOC, "tsdf_allocate: allocator returned NULL");
    hipLaunchKernelGGL(mesh_assign_kernel, dim3(grid(n)), dim3(MT), 0, st, n, v->table, used.flags, v->keys);
    (void)hipMemsetAsync(v->stamp, 0, (size_t)nb * 4, st);
    (void)hipMemsetAsync(v->tsdf_rgb, 0, (size_t)nv * 16, st);
    (void)hipMemsetAsync(v->weight, 0, (size_t)nv * 4, st);
    const int rc = launched("mesh_assign_kernel");
    return rc < 0 ? rc : (int64_t)nb;
}

int surfel_tsdf_integrate(surfel_tsdf_volume* v, int H, int W, const float* depth, const uint32_t* rgba, const float* cam, void* stream) {
    if (!v || !v->table || H <= 0 || W <= 0 || !depth || !rgba || !cam) return api_fail(SURFEL_E_INVALID, "tsdf_integrate: bad arguments");
    v->views++;
    if (v->nblocks == 0) return 0;
    if (!v->keys) return api_fail(SURFEL_E_INVALID, "tsdf_integrate: call surfel_tsdf_allocate first");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Vol vo = vol_of(v);
    (void)hipMemsetAsync(v->list, 0, 4, st);
    hipLaunchKernelGGL(mesh_touch_kernel, dim3(grid((int64_t)H * W)), dim3(MT), 0, st, vo, H, W, depth, cam, (uint32_t)v->views, v->stamp, v->list);
    hipLaunchKernelGGL(mesh_integrate_kernel, dim3((unsigned)v->nblocks), dim3(MT), 0, st, vo, H, W, depth, rgba, cam, v->list, v->keys,
                       reinterpret_cast<float4*>(v->tsdf_rgb), v->weight);
    return launched("mesh_integrate_kernel");
}

int surfel_tsdf_count(surfel_tsdf_volume* v, void* stream) {
    if (!v || !v->table) return api_fail(SURFEL_E_INVALID, "tsdf_count: bad arguments");
    v->nverts = v->ntris = 0;
    if (v->nblocks == 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Vol vo = vol_of(v);
    const int64_t nv = v->nblocks * MV;
    const float4* trgb = reinterpret_cast<const float4*>(v->tsdf_rgb);
    hipLaunchKernelGGL(mesh_classify_kernel, dim3((unsigned)v->nblocks), dim3(MT), 0, st, vo, v->keys, trgb, v->weight, v->info);
    hipLaunchKernelGGL(mesh_count_kernel, dim3((unsigned)v->nblocks), dim3(MT), 0, st, vo, v->keys, trgb, v->weight, v->info, v->vbase, v->tbase);
    uint32_t tot[2];
    const ScanBuf vb(v->vbase, v->pool_scratch, nv), tb(v->tbase, v->pool_scratch, nv);      // (one scratch for both scans)
    vb.scan(st);
    if (int rc = read_words("tsdf_count: copy", vb.total, &tot[0], 1, st, false)) return rc;
    tb.scan(st);      // (same stream: the copy above has read the vertex total)
    if (int rc = read_words("tsdf_count: copy", tb.total, &tot[1], 1, st)) return rc;
    v->nverts = tot[0]; v->ntris = tot[1];
    return launched("mesh_count_kernel");
}

int surfel_tsdf_extract(const surfel_tsdf_volume* v, float* verts, float* colors, int32_t* tris, void* stream) {
    if (!v || !v->table) return api_fail(SURFEL_E_INVALID, "tsdf_extract: bad arguments");
    if (v->nblocks == 0 || (v->nverts == 0 && v->ntris == 0)) return 0;
    if (!verts || !colors || !tris) return api_fail(SURFEL_E_INVALID, "tsdf_extract: null output");
    hipLaunchKernelGGL(mesh_emit_kernel, dim3((unsigned)v->nblocks), dim3(MT), 0, static_cast<hipStream_t>(stream), vol_of(v), v->keys,
                       reinterpret_cast<const float4*>(v->tsdf_rgb), v->info, v->vbase, v->tbase, verts, colors, tris);
    return launched("mesh_emit_kernel");
}

// Edges with a vertex id outside [0, V) carry the key (V, V): they sort behind every valid group and uf_hook_kernel skips them, so
// they link nothing and cannot come between two equal valid edges.
int surfel_mesh_clusters(surfel_alloc_fn alloc, void* user, int64_t V, int64_t F, const int32_t* tris, int32_t* label, int32_t* size, void* stream) {
    if (!alloc || V < 0 || F < 0 || (F > 0 && (!tris || !label || !size))) return api_fail(SURFEL_E_INVALID, "mesh_clusters: bad arguments");
    if (F == 0) return 0;
    const int64_t n = 3 * F;
    if (n >= ((int64_t)1 << 30) || V >= ((int64_t)1 << 31)) return api_fail(SURFEL_E_LIMIT, "mesh_clusters: more than 2^30 triangle edges");
    hipStream_t st = static_cast<hipStream_t>(stream);
    SortPairs s(alloc, user, n);
    int32_t* parent = take<int32_t>(alloc, user, F);
    if (!s.ok() || !parent) return api_fail(SURFEL_E_ALLOC, "mesh_clusters: allocator returned NULL");
    // (min, max) keys as two stable LSD sorts of 32-bit halves: max first, then min; bit_length(V) bits each, for the ids 0 .. V - 1
    // and the key V of the edges with an id out of range
    const EdgeKey key_of{tris, (uint32_t)V};
    const int bits[2] = {bit_length(V), bit_length(V)};
    hipLaunchKernelGGL(edge_keys_kernel, dim3(grid(n)), dim3(MT), 0, st, F, key_of, s.ka, s.va);
    if (int rc = sort_words(s, key_of, 2, bits, "mesh_clusters: sort", st)) return rc;
    hipLaunchKernelGGL(uf_init_kernel, dim3(grid(F)), dim3(MT), 0, st, F, parent, size);
    hipLaunchKernelGGL(uf_hook_kernel, dim3(grid(n)), dim3(MT), 0, st, n, (uint32_t)V, tris, s.va, parent);
    hipLaunchKernelGGL(uf_jump_kernel, dim3(grid(F)), dim3(MT), 0, st, F, parent, label);
    hipLaunchKernelGGL(uf_size_kernel, dim3(grid(F)), dim3(MT), 0, st, F, label, size);
    return launched("uf_size_kernel");
}

int surfel_mesh_filter(surfel_alloc_fn alloc, void* user, int64_t V, int64_t F, const float* verts, const float* colors, const int32_t* tris,
                       const int32_t* label, const int32_t* size, int threshold, float* verts_out, float* colors_out, int32_t* tris_out,
                       int64_t* counts_out, void* stream) {
    if (!alloc || V < 0 || F < 0 || !counts_out || (F > 0 && (!tris || !label || !size || !tris_out)) || (V > 0 && (!verts || !colors || !verts_out || !colors_out)))
        return api_fail(SURFEL_E_INVALID, "mesh_filter: bad arguments");
    counts_out[0] = counts_out[1] = 0;
    if (V == 0 || F == 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint32_t* vflag = take<uint32_t>(alloc, user, V);
    uint32_t* tflag = take<uint32_t>(alloc, user, F);
    const ScanBuf vpos = take_scan(alloc, user, V), tpos = take_scan(alloc, user, F);
    if (!vflag || !tflag || !vpos.flags || !tpos.flags) return api_fail(SURFEL_E_ALLOC, "mesh_filter: allocator returned NULL");
    (void)hipMemsetAsync(vflag, 0, (size_t)V * 4, st);
    hipLaunchKernelGGL(filter_mark_kernel, dim3(grid(F)), dim3(MT), 0, st, V, F, tris, label, size, threshold, tflag, vflag);
    hipLaunchKernelGGL(copy_flags_kernel, dim3(grid(V)), dim3(MT), 0, st, V, vflag, vpos.flags);
    hipLaunchKernelGGL(copy_flags_kernel, dim3(grid(F)), dim3(MT), 0, st, F, tflag, tpos.flags);
    vpos.scan(st);
    tpos.scan(st);
    hipLaunchKernelGGL(filter_verts_kernel, dim3(grid(V)), dim3(MT), 0, st, V, vflag, vpos.flags, verts, colors, verts_out, colors_out);
    hipLaunchKernelGGL(filter_tris_kernel, dim3(grid(F)), dim3(MT), 0, st, F, tflag, tpos.flags, tris, vpos.flags, tris_out);
    uint32_t tot[2];
    if (int rc = read_words("mesh_filter: copy", vpos.total, &tot[0], 1, st, false)) return rc;
    if (int rc = read_words("mesh_filter: copy", tpos.total, &tot[1], 1, st)) return rc;
    counts_out[0] = tot[0]; counts_out[1] = tot[1];
    return launched("filter_tris_kernel");
}

}  // extern "C"
