// eval_geometry.hip — DTU-style mesh evaluation: triangle sampling, greedy thinning, observation mask, exact nearest neighbour with
// a cut-off, fixed-order means, mask dilation and vertex culling (include/surfel_eval.h, EVAL.md).  Memory-bound gathers; no MFMA.
// Compiled with -ffp-contract=off (build.py): the sampling decisions (fp64) and the thinning's pair test (fp32) round exactly as
// their restatements in tests/eval_oracle.py.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/surfel_eval.h"
#include "block_ops.h"
#include "side_util.h"

namespace surfel {

constexpr int ET = 256;                    // threads per workgroup
constexpr int EVAL_MEAN_BLOCKS = 1024;     // partial sums of eval_mean_kernel

struct EGrid {      // what the kernels need of surfel_eval_grid
    float ox, oy, oz, cell;
    int nx, ny, nz;
    int64_t n;
    const float4* sorted;
    const uint32_t* order;
    const uint2* ranges;
};

__device__ inline int eval_cell_axis(float r, float cell, int dim) {      // (a NaN lands in cell 0)
    const float f = r / cell;
    return f > 0.f ? (f < (float)dim ? (int)f : dim - 1) : 0;
}

// ---- rule 1: sampling -----------------------------------------------------------------------------------------------------
struct TriSetup {
    double a[3], v1[3], v2[3];
    double n1, n2;      // floor(l1 / thr), floor(l2 / thr)
};

// false: the triangle has no samples (bad index, zero area, n1 or n2 of 0 or not finite)
__device__ inline bool eval_tri_setup(int64_t V, const float* __restrict__ verts, const int32_t* __restrict__ tris, int64_t t, double density,
                                      TriSetup& s) {
    const int32_t ia = tris[3 * t], ib = tris[3 * t + 1], ic = tris[3 * t + 2];
    if (ia < 0 || ib < 0 || ic < 0 || ia >= V || ib >= V || ic >= V) return false;
    double b[3], c[3];
    for (int k = 0; k < 3; k++) {
        s.a[k] = (double)verts[3 * (int64_t)ia + k]; b[k] = (double)verts[3 * (int64_t)ib + k]; c[k] = (double)verts[3 * (int64_t)ic + k];
        s.v1[k] = b[k] - s.a[k]; s.v2[k] = c[k] - s.a[k];
    }
    const double l1 = sqrt((s.v1[0] * s.v1[0] + s.v1[1] * s.v1[1]) + s.v1[2] * s.v1[2]);
    const double l2 = sqrt((s.v2[0] * s.v2[0] + s.v2[1] * s.v2[1]) + s.v2[2] * s.v2[2]);
    const double cx = s.v1[1] * s.v2[2] - s.v1[2] * s.v2[1], cy = s.v1[2] * s.v2[0] - s.v1[0] * s.v2[2], cz = s.v1[0] * s.v2[1] - s.v1[1] * s.v2[0];
    const double area2 = sqrt((cx * cx + cy * cy) + cz * cz);
    if (!(area2 > 0.0)) return false;
    const double thr = density * sqrt(l1 * l2 / area2);
    s.n1 = floor(l1 / thr); s.n2 = floor(l2 / thr);
    return s.n1 >= 1.0 && s.n2 >= 1.0 && s.n1 < 1e300 && s.n2 < 1e300;      // (NaN fails the first two)
}

// largest j in [-1, n2] with c0 + (j + 0.5) / n2 < 1 (the test is monotone in j: a division by a positive constant and a sum)
__device__ inline int eval_last_j(double c0, double n2) {
    double je = floor((1.0 - c0) * n2 - 0.5);
    int j = je < -1.0 ? -1 : (je > n2 ? (int)n2 : (int)je);
    while (j < (int)n2 && c0 + ((double)(j + 1) + 0.5) / n2 < 1.0) j++;
    while (j >= 0 && !(c0 + ((double)j + 0.5) / n2 < 1.0)) j--;
    return j;
}

// count[t] = samples of triangle t; flags[0] |= 1 when a triangle exceeds SURFEL_EVAL_MAX_N; total += every count (64 bit)
__global__ void __launch_bounds__(ET) eval_sample_count_kernel(int64_t V, int64_t F, const float* __restrict__ verts, const int32_t* __restrict__ tris,
                                                               double density, uint32_t* __restrict__ count, unsigned long long* total,
                                                               uint32_t* flags) {
    const int64_t t = (int64_t)blockIdx.x * ET + threadIdx.x;
    unsigned long long c = 0;
    if (t < F) {
        TriSetup s;
        if (eval_tri_setup(V, verts, tris, t, density, s)) {
            if (s.n1 > (double)SURFEL_EVAL_MAX_N || s.n2 > (double)SURFEL_EVAL_MAX_N) {
                atomicOr(flags, 1u);
            } else {
                const int n1 = (int)s.n1;
                for (int i = 0; i <= n1; i++) c += (unsigned)(eval_last_j(((double)i + 0.5) / s.n1, s.n2) + 1);
            }
        }
        count[t] = (uint32_t)c;
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(total, c);
}

__global__ void __launch_bounds__(ET) eval_sample_emit_kernel(int64_t V, int64_t F, const float* __restrict__ verts, const int32_t* __restrict__ tris,
                                                              double density, const uint32_t* __restrict__ offsets, int64_t total,
                                                              float* __restrict__ points) {
    const int64_t t = (int64_t)blockIdx.x * ET + threadIdx.x;
    if (t >= F) return;
    TriSetup s;
    if (!eval_tri_setup(V, verts, tris, t, density, s)) return;
    if (s.n1 > (double)SURFEL_EVAL_MAX_N || s.n2 > (double)SURFEL_EVAL_MAX_N) return;
    int64_t o = offsets[t];
    const int n1 = (int)s.n1;
    for (int i = 0; i <= n1; i++) {
        const double c0 = ((double)i + 0.5) / s.n1;
        const int jl = eval_last_j(c0, s.n2);
        for (int j = 0; j <= jl && o < total; j++, o++) {
            const double c1 = ((double)j + 0.5) / s.n2;
            float* p = points + 3 * (V + o);
            for (int k = 0; k < 3; k++) p[k] = (float)((s.v1[k] * c0 + s.v2[k] * c1) + s.a[k]);
        }
    }
}

__global__ void __launch_bounds__(ET) eval_copy_kernel(int64_t n, const float* __restrict__ a, float* __restrict__ b) {
    const int64_t i = (int64_t)blockIdx.x * ET + threadIdx.x;
    if (i < n) b[i] = a[i];
}

// ---- the grid ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(ET) eval_keys_kernel(EGrid g, int64_t n, const float* __restrict__ pts, uint32_t* __restrict__ key,
                                                       uint32_t* __restrict__ val) {
    const int64_t i = (int64_t)blockIdx.x * ET + threadIdx.x;
    if (i >= n) return;
    const int cx = eval_cell_axis(pts[3 * i] - g.ox, g.cell, g.nx), cy = eval_cell_axis(pts[3 * i + 1] - g.oy, g.cell, g.ny),
              cz = eval_cell_axis(pts[3 * i + 2] - g.oz, g.cell, g.nz);
    key[i] = (uint32_t)(cx + g.nx * (cy + g.ny * cz));
    val[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(ET) eval_gather_kernel(EGrid g, int64_t n, const float* __restrict__ pts, const uint32_t* __restrict__ rank,
                                                         const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                         float4* __restrict__ sorted, uint32_t* __restrict__ order, uint32_t* __restrict__ ranges) {
    const int64_t i = (int64_t)blockIdx.x * ET + threadIdx.x;
    if (i >= n) return;
    const uint32_t src = vals[i], k = keys[i];
    const uint32_t r = rank ? rank[src] : src;
    sorted[i] = make_float4(pts[3 * (int64_t)src] - g.ox, pts[3 * (int64_t)src + 1] - g.oy, pts[3 * (int64_t)src + 2] - g.oz, __uint_as_float(r));
    order[i] = src;
    if (i == 0 || keys[i - 1] != k) ranges[2 * (int64_t)k] = (uint32_t)i;
    if (i == n - 1 || keys[i + 1] != k) ranges[2 * (int64_t)k + 1] = (uint32_t)(i + 1);
}

// ---- rule 3: thinning ---------------------------------------------------------------------------------------------------------
// state[i] of sorted slot i: 0 undecided, 1 kept, 2 dropped.  A decision is final whenever it is made (kept: every earlier neighbour
// was seen dropped; dropped: one earlier neighbour was seen kept), so a state another workgroup writes during this launch may be read
// early or late: that changes the number of rounds, never the result.  Nothing waits inside a launch.
__global__ void __launch_bounds__(ET) eval_thin_round_kernel(EGrid g, float dd, uint32_t* state, uint32_t* decided) {
    const int64_t i = (int64_t)blockIdx.x * ET + threadIdx.x;
    bool now = false;
    if (i < g.n && state[i] == 0u) {
        const float4 p = g.sorted[i];
        const uint32_t rank = __float_as_uint(p.w);
        const int cx = eval_cell_axis(p.x, g.cell, g.nx), cy = eval_cell_axis(p.y, g.cell, g.ny), cz = eval_cell_axis(p.z, g.cell, g.nz);
        const int x0 = cx > 0 ? cx - 1 : 0, x1 = cx < g.nx - 1 ? cx + 1 : g.nx - 1;
        bool blocked = false, drop = false;
        for (int z = cz > 0 ? cz - 1 : 0; z <= (cz < g.nz - 1 ? cz + 1 : g.nz - 1) && !drop; z++)
            for (int y = cy > 0 ? cy - 1 : 0; y <= (cy < g.ny - 1 ? cy + 1 : g.ny - 1) && !drop; y++)
                for (int x = x0; x <= x1 && !drop; x++) {
                    const uint2 r = g.ranges[x + (int64_t)g.nx * (y + (int64_t)g.ny * z)];
                    for (uint32_t j = r.x; j < r.y; j++) {
                        const float4 q = g.sorted[j];
                        if (__float_as_uint(q.w) >= rank) continue;      // later in the order (or the point itself)
                        const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
                        if ((dx * dx + dy * dy) + dz * dz <= dd) {
                            const uint32_t s = state[j];
                            if (s == 1u) { drop = true; break; }
                            blocked |= s == 0u;
                        }
                    }
                }
        if (drop || !blocked) { state[i] = drop ? 2u : 1u; now = true; }
    }
    const uint64_t b = __ballot(now);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(decided, (uint32_t)__popcll(b));
}

__global__ void __launch_bounds__(ET) eval_thin_keep_kernel(int64_t n, const uint32_t* __restrict__ state, const uint32_t* __restrict__ order,
                                                            uint8_t* __restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * ET + threadIdx.x;
    if (i < n) keep[order[i]] = state[i] == 1u;
}

// ---- rule 4: bounding box, observation mask, plane ------------------------------------------------------------------------------
struct EObs {
    float lo[3], hi[3], bb0[3];
    double res;
    int dims[3];
};

__global__ void __launch_bounds__(ET) eval_obs_kernel(int64_t n, const float* __restrict__ pts, EObs o, const uint8_t* __restrict__ mask,
                                                      uint8_t* __restrict__ inbound, uint8_t* __restrict__ in_obs) {
    const int64_t i = (int64_t)blockIdx.x * ET + threadIdx.x;
    if (i >= n) return;
    const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    const bool in = x >= o.lo[0] && y >= o.lo[1] && z >= o.lo[2] && x < o.hi[0] && y < o.hi[1] && z < o.hi[2];
    bool obs = false;
    if (in) {
        // numpy's around: to the nearest integer, ties to even = rint in the default rounding mode; fp64 as the reference
        const double gx = rint(((double)x - (double)o.bb0[0]) / o.res), gy = rint(((double)y - (double)o.bb0[1]) / o.res),
                     gz = rint(((double)z - (double)o.bb0[2]) / o.res);
        if (gx >= 0.0 && gy >= 0.0 && gz >= 0.0 && gx < (double)o.dims[0] && gy < (double)o.dims[1] && gz < (double)o.dims[2])
            obs = mask[((int64_t)gx * o.dims[1] + (int64_t)gy) * o.dims[2] + (int64_t)gz] != 0;
    }
    inbound[i] = in;
    in_obs[i] = obs;
}

struct EPlane { double p[4]; };

__global__ void __launch_bounds__(ET) eval_plane_kernel(int64_t n, const float* __restrict__ pts, EPlane pl, uint8_t* __restrict__ above) {
    const int64_t i = (int64_t)blockIdx.x * ET + threadIdx.x;
    if (i >= n) return;
    const double s = ((pl.p[0] * (double)pts[3 * i] + pl.p[1] * (double)pts[3 * i + 1]) + pl.p[2] * (double)pts[3 * i + 2]) + pl.p[3];
    above[i] = s > 0.0;
}

// ---- rule 5: nearest neighbour with a cut-off -------------------------------------------------------------------------------------
__global__ void __launch_bounds__(ET) eval_query_keys_kernel(EGrid g, int64_t nq, const float* __restrict__ q, uint32_t* __restrict__ key,
                                                             uint32_t* __restrict__ val) {
    const int64_t i = (int64_t)blockIdx.x * ET + threadIdx.x;
    if (i >= nq) return;
    const int cx = eval_cell_axis(q[3 * i] - g.ox, g.cell, g.nx), cy = eval_cell_axis(q[3 * i + 1] - g.oy, g.cell, g.ny),
              cz = eval_cell_axis(q[3 * i + 2] - g.oz, g.cell, g.nz);
    key[i] = (uint32_t)(cx + g.nx * (cy + g.ny * cz));
    val[i] = (uint32_t)i;
}

__device__ inline void eval_scan_cell(const EGrid& g, int x, int y, int z, float px, float py, float pz, float& best2, uint32_t& besti) {
    const uint2 r = g.ranges[x + (int64_t)g.nx * (y + (int64_t)g.ny * z)];
    for (uint32_t j = r.x; j < r.y; j++) {
        const float4 c = g.sorted[j];
        const float dx = px - c.x, dy = py - c.y, dz = pz - c.z;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 < best2) { best2 = d2; besti = j; }
    }
}

// Lane s takes the s-th query in cell order, so neighbouring lanes walk the same cells.  Shell k holds the cells at Chebyshev distance
// k from the query's (clamped) cell; every point of it is at least (k - 1) * cell away (also for a query outside the grid, whose
// clamped cell is the nearest one), less 0.1 % for the rounding of the cell assignment.
__global__ void __launch_bounds__(ET) eval_nearest_kernel(EGrid g, int64_t nq, const float* __restrict__ q, const uint32_t* __restrict__ qorder,
                                                          float max_dist, float* __restrict__ dist, int32_t* __restrict__ index) {
    const int64_t s = (int64_t)blockIdx.x * ET + threadIdx.x;
    if (s >= nq) return;
    const int64_t qi = qorder[s];
    const float px = q[3 * qi] - g.ox, py = q[3 * qi + 1] - g.oy, pz = q[3 * qi + 2] - g.oz;
    const int cx = eval_cell_axis(px, g.cell, g.nx), cy = eval_cell_axis(py, g.cell, g.ny), cz = eval_cell_axis(pz, g.cell, g.nz);
    float best2 = INFINITY;
    uint32_t besti = 0xFFFFFFFFu;
    const int kmax = max(max(max(cx, g.nx - 1 - cx), max(cy, g.ny - 1 - cy)), max(cz, g.nz - 1 - cz));
    for (int k = 0; k <= kmax; k++) {
        const float lb = (float)(k - 1) * g.cell * 0.999f;
        if (k > 1 && (lb > max_dist || lb * lb > best2)) break;
        const int z0 = max(cz - k, 0), z1 = min(cz + k, g.nz - 1), y0 = max(cy - k, 0), y1 = min(cy + k, g.ny - 1);
        for (int z = z0; z <= z1; z++)
            for (int y = y0; y <= y1; y++) {
                if (abs(z - cz) == k || abs(y - cy) == k) {      // a face of the shell: the whole run in x
                    for (int x = max(cx - k, 0); x <= min(cx + k, g.nx - 1); x++) eval_scan_cell(g, x, y, z, px, py, pz, best2, besti);
                } else {                                          // inside: the two end cells
                    if (cx - k >= 0) eval_scan_cell(g, cx - k, y, z, px, py, pz, best2, besti);
                    if (cx + k < g.nx) eval_scan_cell(g, cx + k, y, z, px, py, pz, best2, besti);
                }
            }
    }
    const float d = sqrtf(best2);
    const bool hit = d < max_dist;
    dist[qi] = hit ? d : INFINITY;
    if (index) index[qi] = hit ? (int32_t)g.order[besti] : -1;
}

__global__ void __launch_bounds__(ET) eval_fill_none_kernel(int64_t n, float* __restrict__ dist, int32_t* __restrict__ index) {
    const int64_t i = (int64_t)blockIdx.x * ET + threadIdx.x;
    if (i >= n) return;
    dist[i] = INFINITY;
    if (index) index[i] = -1;
}

// ---- fixed-order means ----------------------------------------------------------------------------------------------------------
// partial[2 b], partial[2 b + 1] = sum and count of the d < bound among the elements b * ET + t + k * (blocks * ET)
__global__ void __launch_bounds__(ET) eval_mean_kernel(int64_t n, const float* __restrict__ d, float bound, double* __restrict__ partial) {
    __shared__ double sh[2 * ET];
    double acc[2] = {0.0, 0.0};      // sum, count
    for (int64_t i = (int64_t)blockIdx.x * ET + threadIdx.x; i < n; i += (int64_t)gridDim.x * ET) {
        const float v = d[i];
        if (v < bound) { acc[0] += (double)v; acc[1] += 1.0; }
    }
    block_tree_sum<ET>(acc, sh);
    if (threadIdx.x == 0) { partial[2 * blockIdx.x] = sh[0]; partial[2 * blockIdx.x + 1] = sh[ET]; }
}

__global__ void __launch_bounds__(ET) eval_mean_top_kernel(int nb, const double* __restrict__ partial, double* __restrict__ out) {
    __shared__ double sh[2 * ET];
    double acc[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < nb; i += ET) { acc[0] += partial[2 * i]; acc[1] += partial[2 * i + 1]; }
    block_tree_sum<ET>(acc, sh);
    if (threadIdx.x == 0) { out[0] = sh[0]; out[1] = sh[ET]; }
}

// ---- rule 7: dilation and culling -------------------------------------------------------------------------------------------------
// hd[v, y, x] = distance along the row to the nearest set pixel, 255 when there is none within r
__global__ void __launch_bounds__(ET) eval_dilate_rows_kernel(int64_t npix, int H, int W, const uint8_t* __restrict__ masks, int r,
                                                              uint8_t* __restrict__ hd) {
    const int64_t i = (int64_t)blockIdx.x * ET + threadIdx.x;
    if (i >= npix) return;
    const int x = (int)(i % W);
    const uint8_t* row = masks + (i - x);
    int best = 255;
    for (int d = 0; d <= r; d++)
        if ((x - d >= 0 && row[x - d]) || (x + d < W && row[x + d])) { best = d; break; }
    hd[i] = (uint8_t)best;
}

// out = 1 when some row y + dy, |dy| <= r, has a set pixel within floor(sqrt(r^2 - dy^2)) of x
__global__ void __launch_bounds__(ET) eval_dilate_cols_kernel(int64_t npix, int H, int W, const uint8_t* __restrict__ hd, int r,
                                                              uint8_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * ET + threadIdx.x;
    if (i >= npix) return;
    const int y = (int)((i / W) % H);
    bool set = false;
    for (int dy = -r; dy <= r && !set; dy++) {
        if (y + dy < 0 || y + dy >= H) continue;
        const int m = r * r - dy * dy;
        int w = (int)sqrtf((float)m);
        while ((w + 1) * (w + 1) <= m) w++;
        while (w * w > m) w--;
        set = (int)hd[i + (int64_t)dy * W] <= w;
    }
    out[i] = set;
}

__global__ void __launch_bounds__(ET) eval_cull_kernel(int64_t n, const float* __restrict__ verts, int nviews, const float* __restrict__ proj, int H,
                                                       int W, const uint8_t* __restrict__ dilated, uint8_t* __restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * ET + threadIdx.x;
    if (i >= n) return;
    const float vx = verts[3 * i], vy = verts[3 * i + 1], vz = verts[3 * i + 2];
    bool ok = true;
    for (int v = 0; v < nviews && ok; v++) {
        const float* m = proj + 12 * v;
        const float x = ((m[0] * vx + m[1] * vy) + m[2] * vz) + m[3], y = ((m[4] * vx + m[5] * vy) + m[6] * vz) + m[7],
                    z = ((m[8] * vx + m[9] * vy) + m[10] * vz) + m[11];
        const float zz = z + 1e-6f;
        const float nx = ((x / zz) / (float)(W - 1) - 0.5f) * 2.f, ny = ((y / zz) / (float)(H - 1) - 0.5f) * 2.f;
        const bool valid = nx > -1.f && nx < 1.f && ny > -1.f && ny < 1.f;
        if (!valid) continue;      // not seen by this view: survives it
        // grid_sample, nearest, align_corners: pixel = round-half-even((ndc + 1) / 2 * (size - 1)), zero outside
        const float fx = rintf((nx + 1.f) / 2.f * (float)(W - 1)), fy = rintf((ny + 1.f) / 2.f * (float)(H - 1));
        ok = fx >= 0.f && fy >= 0.f && fx <= (float)(W - 1) && fy <= (float)(H - 1) && dilated[((int64_t)v * H + (int64_t)fy) * W + (int64_t)fx] != 0;
    }
    keep[i] = ok;
}

}  // namespace surfel

// ================================================================================================================ C ABI
using namespace surfel;

namespace {
inline unsigned grid(int64_t n) { return blocks_for(n, ET); }
inline int64_t cells_of(const surfel_eval_grid* g) { return (int64_t)g->dims[0] * g->dims[1] * g->dims[2]; }
inline bool grid_fields_ok(const surfel_eval_grid* g) {
    return g && g->dims[0] > 0 && g->dims[1] > 0 && g->dims[2] > 0 && g->cell > 0.f && g->cell < INFINITY && cells_of(g) < ((int64_t)1 << 31) &&
           (int64_t)g->dims[0] * g->dims[1] < ((int64_t)1 << 31);
}
inline EGrid egrid_of(const surfel_eval_grid* g) {
    return EGrid{g->origin[0], g->origin[1], g->origin[2], g->cell, g->dims[0], g->dims[1], g->dims[2], g->n,
                 reinterpret_cast<const float4*>(g->sorted), g->order, reinterpret_cast<const uint2*>(g->ranges)};
}
inline int key_bits(int64_t ncells) { return bit_length(ncells - 1); }      // cell indices 0 .. ncells - 1
constexpr int64_t EVAL_MAX_POINTS = ((int64_t)1 << 31) - 1;
}  // namespace

extern "C" {

int64_t surfel_eval_sample_count(surfel_alloc_fn alloc, void* user, int64_t V, int64_t F, const float* verts, const int32_t* tris, double density,
                                 int64_t budget_bytes, uint32_t* offsets, void* stream) {
    if (!alloc || V < 0 || F < 0 || !(density > 0.0) || (F > 0 && (!tris || !offsets)) || (V > 0 && !verts))
        return api_fail(SURFEL_E_INVALID, "eval_sample_count: bad arguments");
    if (V > EVAL_MAX_POINTS || F > EVAL_MAX_POINTS) return api_fail(SURFEL_E_LIMIT, "eval_sample_count: more than 2^31 - 1 vertices or triangles");
    if (12 * V > budget_bytes) return api_fail(SURFEL_E_LIMIT, "eval_sample_count: the cloud exceeds the byte budget (raise the budget or the density)");
    if (F == 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint32_t* scratch = take<uint32_t>(alloc, user, scan_scratch_u32(F) + 4);      // scan sums | total (64 bit, 8-byte aligned) | flag
    if (!scratch) return api_fail(SURFEL_E_ALLOC, "eval_sample_count: allocator returned NULL");
    uint32_t* tail = scratch + (scan_scratch_u32(F) + 1) / 2 * 2;
    if (hipMemsetAsync(tail, 0, 12, st) != hipSuccess) return api_fail(SURFEL_E_HIP, "eval_sample_count: memset", hipGetLastError());
    hipLaunchKernelGGL(eval_sample_count_kernel, dim3(grid(F)), dim3(ET), 0, st, V, F, verts, tris, density, offsets,
                       reinterpret_cast<unsigned long long*>(tail), tail + 2);
    scan_u32(offsets, F, scratch, st);
    uint32_t host[3] = {0, 0, 0};
    if (int rc = read_words("eval_sample_count: copy", tail, host, 3, st)) return rc;
    const int rc = launched("eval_sample_count_kernel");
    if (rc < 0) return rc;
    if (host[2]) return api_fail(SURFEL_E_LIMIT, "eval_sample_count: a triangle wants more than SURFEL_EVAL_MAX_N samples along an edge (raise the density)");
    const uint64_t total = (uint64_t)host[0] | (uint64_t)host[1] << 32;
    if (total > (uint64_t)(EVAL_MAX_POINTS - V)) return api_fail(SURFEL_E_LIMIT, "eval_sample_count: more than 2^31 - 1 points (raise the density)");
    if (12 * (V + (int64_t)total) > budget_bytes)
        return api_fail(SURFEL_E_LIMIT, "eval_sample_count: the cloud exceeds the byte budget (raise the budget or the density)");
    return (int64_t)total;
}

int surfel_eval_sample_emit(int64_t V, int64_t F, const float* verts, const int32_t* tris, double density, const uint32_t* offsets, int64_t total,
                            float* points, void* stream) {
    if (V < 0 || F < 0 || total < 0 || !(density > 0.0) || (F > 0 && (!tris || !offsets)) || (V > 0 && !verts) || (V + total > 0 && !points))
        return api_fail(SURFEL_E_INVALID, "eval_sample_emit: bad arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (V > 0) hipLaunchKernelGGL(eval_copy_kernel, dim3(grid(3 * V)), dim3(ET), 0, st, 3 * V, verts, points);
    if (F > 0 && total > 0)
        hipLaunchKernelGGL(eval_sample_emit_kernel, dim3(grid(F)), dim3(ET), 0, st, V, F, verts, tris, density, offsets, total, points);
    return launched("eval_sample_emit_kernel");
}

int surfel_eval_grid_build(surfel_alloc_fn alloc, void* user, surfel_eval_grid* g, int64_t n, const float* points, const uint32_t* rank,
                           void* stream) {
    if (!alloc || !grid_fields_ok(g) || n < 0 || (n > 0 && !points)) return api_fail(SURFEL_E_INVALID, "eval_grid_build: bad arguments");
    if (n > EVAL_MAX_POINTS) return api_fail(SURFEL_E_LIMIT, "eval_grid_build: more than 2^31 - 1 points");
    const int64_t nc = cells_of(g);
    const size_t sort_bytes = radix_sort_scratch_bytes((size_t)(n > 0 ? n : 1));
    if (8 * nc + (16 + 4 + 16) * n + (int64_t)sort_bytes > g->budget_bytes)
        return api_fail(SURFEL_E_LIMIT, "eval_grid_build: the grid exceeds the byte budget (raise the budget or the cell size)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    g->n = n;
    g->ranges = take<uint32_t>(alloc, user, 2 * nc);
    g->sorted = take<float>(alloc, user, 4 * n);
    g->order = take<uint32_t>(alloc, user, n);
    if (!g->ranges || !g->sorted || !g->order) return api_fail(SURFEL_E_ALLOC, "eval_grid_build: allocator returned NULL");
    if (hipMemsetAsync(g->ranges, 0, (size_t)nc * 8, st) != hipSuccess) return api_fail(SURFEL_E_HIP, "eval_grid_build: memset", hipGetLastError());
    if (n == 0) return 0;
    SortPairs s(alloc, user, n);
    if (!s.ok()) return api_fail(SURFEL_E_ALLOC, "eval_grid_build: allocator returned NULL");
    const EGrid eg = egrid_of(g);
    hipLaunchKernelGGL(eval_keys_kernel, dim3(grid(n)), dim3(ET), 0, st, eg, n, points, s.ka, s.va);
    if (s.sort(key_bits(nc), st) < 0) return api_fail(SURFEL_E_LIMIT, "eval_grid_build: sort");
    hipLaunchKernelGGL(eval_gather_kernel, dim3(grid(n)), dim3(ET), 0, st, eg, n, points, rank, s.ka, s.va,
                       reinterpret_cast<float4*>(g->sorted), g->order, g->ranges);
    return launched("eval_gather_kernel");
}

int surfel_eval_thin(surfel_alloc_fn alloc, void* user, const surfel_eval_grid* g, float density, uint8_t* keep, int* rounds_out, void* stream) {
    if (!alloc || !grid_fields_ok(g) || !(density > 0.f) || (g->n > 0 && (!keep || !g->sorted || !g->order || !g->ranges)))
        return api_fail(SURFEL_E_INVALID, "eval_thin: bad arguments");
    if (!(g->cell >= density * (1.f + 1.f / 1024.f))) return api_fail(SURFEL_E_INVALID, "eval_thin: the grid's cell edge is below density * (1 + 2^-10)");
    if (rounds_out) *rounds_out = 0;
    const int64_t n = g->n;
    if (n == 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    constexpr int BATCH = 4;      // rounds between two looks at the counters
    uint32_t* state = take<uint32_t>(alloc, user, n + BATCH);
    if (!state) return api_fail(SURFEL_E_ALLOC, "eval_thin: allocator returned NULL");
    uint32_t* decided = state + n;
    if (hipMemsetAsync(state, 0, (size_t)n * 4, st) != hipSuccess) return api_fail(SURFEL_E_HIP, "eval_thin: memset", hipGetLastError());
    const EGrid eg = egrid_of(g);
    const float dd = density * density;
    int rounds = 0;
    // every round decides at least the earliest undecided point, so a round that decides nothing found none left: at most n + 1 rounds
    for (bool done = false; !done;) {
        if (hipMemsetAsync(decided, 0, BATCH * 4, st) != hipSuccess) return api_fail(SURFEL_E_HIP, "eval_thin: memset", hipGetLastError());
        for (int b = 0; b < BATCH; b++) hipLaunchKernelGGL(eval_thin_round_kernel, dim3(grid(n)), dim3(ET), 0, st, eg, dd, state, decided + b);
        uint32_t host[BATCH];
        if (int rc = read_words("eval_thin: copy", decided, host, BATCH, st)) return rc;
        const int rc = launched("eval_thin_round_kernel");
        if (rc < 0) return rc;
        for (int b = 0; b < BATCH && !done; b++) {
            rounds++;
            done = host[b] == 0;
        }
    }
    if (rounds_out) *rounds_out = rounds;
    hipLaunchKernelGGL(eval_thin_keep_kernel, dim3(grid(n)), dim3(ET), 0, st, n, state, g->order, keep);
    if (hipStreamSynchronize(st) != hipSuccess) return api_fail(SURFEL_E_HIP, "eval_thin: synchronize", hipGetLastError());
    return launched("eval_thin_keep_kernel");
}

int surfel_eval_obs_mask(int64_t n, const float* points, const float* bb, float patch, double res, const uint8_t* obs_mask, const int* dims,
                         uint8_t* inbound, uint8_t* in_obs, void* stream) {
    if (n < 0 || !bb || !dims || !obs_mask || !(res > 0.0) || dims[0] <= 0 || dims[1] <= 0 || dims[2] <= 0 || (n > 0 && (!points || !inbound || !in_obs)))
        return api_fail(SURFEL_E_INVALID, "eval_obs_mask: bad arguments");
    if (n == 0) return 0;
    EObs o;
    for (int k = 0; k < 3; k++) {
        o.bb0[k] = bb[k];
        o.lo[k] = bb[k] - patch;                  // fp32, as numpy's float32 array - Python float
        o.hi[k] = bb[3 + k] + patch * 2.f;        // (2 * patch is exact)
        o.dims[k] = dims[k];
    }
    o.res = res;
    hipLaunchKernelGGL(eval_obs_kernel, dim3(grid(n)), dim3(ET), 0, static_cast<hipStream_t>(stream), n, points, o, obs_mask, inbound, in_obs);
    return launched("eval_obs_kernel");
}

int surfel_eval_above_plane(int64_t n, const float* points, const double* plane, uint8_t* above, void* stream) {
    if (n < 0 || !plane || (n > 0 && (!points || !above))) return api_fail(SURFEL_E_INVALID, "eval_above_plane: bad arguments");
    if (n == 0) return 0;
    EPlane pl;
    for (int k = 0; k < 4; k++) pl.p[k] = plane[k];
    hipLaunchKernelGGL(eval_plane_kernel, dim3(grid(n)), dim3(ET), 0, static_cast<hipStream_t>(stream), n, points, pl, above);
    return launched("eval_plane_kernel");
}

int surfel_eval_nearest(surfel_alloc_fn alloc, void* user, const surfel_eval_grid* g, int64_t nq, const float* queries, float max_dist,
                        float* dist, int32_t* index, void* stream) {
    if (!alloc || !grid_fields_ok(g) || nq < 0 || !(max_dist > 0.f) || (nq > 0 && (!queries || !dist)) || (g->n > 0 && (!g->sorted || !g->order || !g->ranges)))
        return api_fail(SURFEL_E_INVALID, "eval_nearest: bad arguments");
    if (nq > EVAL_MAX_POINTS) return api_fail(SURFEL_E_LIMIT, "eval_nearest: more than 2^31 - 1 queries");
    if (nq == 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (g->n == 0) {
        hipLaunchKernelGGL(eval_fill_none_kernel, dim3(grid(nq)), dim3(ET), 0, st, nq, dist, index);
        return launched("eval_fill_none_kernel");
    }
    SortPairs s(alloc, user, nq);
    if (!s.ok()) return api_fail(SURFEL_E_ALLOC, "eval_nearest: allocator returned NULL");
    const EGrid eg = egrid_of(g);
    hipLaunchKernelGGL(eval_query_keys_kernel, dim3(grid(nq)), dim3(ET), 0, st, eg, nq, queries, s.ka, s.va);
    if (s.sort(key_bits(cells_of(g)), st) < 0) return api_fail(SURFEL_E_LIMIT, "eval_nearest: sort");
    hipLaunchKernelGGL(eval_nearest_kernel, dim3(grid(nq)), dim3(ET), 0, st, eg, nq, queries, s.va, max_dist, dist, index);
    return launched("eval_nearest_kernel");
}

int surfel_eval_mean_below(surfel_alloc_fn alloc, void* user, int64_t n, const float* dist, float bound, double* out, void* stream) {
    if (!alloc || n < 0 || !out || (n > 0 && !dist)) return api_fail(SURFEL_E_INVALID, "eval_mean_below: bad arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nb = (int)(grid(n) < (unsigned)EVAL_MEAN_BLOCKS ? grid(n) : (unsigned)EVAL_MEAN_BLOCKS);
    double* partial = take<double>(alloc, user, 2 * (int64_t)nb);
    if (!partial) return api_fail(SURFEL_E_ALLOC, "eval_mean_below: allocator returned NULL");
    if (nb > 0) hipLaunchKernelGGL(eval_mean_kernel, dim3((unsigned)nb), dim3(ET), 0, st, n, dist, bound, partial);
    hipLaunchKernelGGL(eval_mean_top_kernel, dim3(1), dim3(ET), 0, st, nb, partial, out);
    return launched("eval_mean_top_kernel");
}

int surfel_eval_dilate_masks(surfel_alloc_fn alloc, void* user, int V, int H, int W, const uint8_t* masks, int r, uint8_t* out, void* stream) {
    if (!alloc || V < 0 || H <= 0 || W <= 0 || r < 0 || r > 254 || (V > 0 && (!masks || !out)))
        return api_fail(SURFEL_E_INVALID, "eval_dilate_masks: bad arguments");
    if (V == 0) return 0;
    const int64_t npix = (int64_t)V * H * W;
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint8_t* hd = take<uint8_t>(alloc, user, npix);
    if (!hd) return api_fail(SURFEL_E_ALLOC, "eval_dilate_masks: allocator returned NULL");
    hipLaunchKernelGGL(eval_dilate_rows_kernel, dim3(grid(npix)), dim3(ET), 0, st, npix, H, W, masks, r, hd);
    hipLaunchKernelGGL(eval_dilate_cols_kernel, dim3(grid(npix)), dim3(ET), 0, st, npix, H, W, hd, r, out);
    return launched("eval_dilate_cols_kernel");
}

int surfel_eval_cull_vertices(int64_t n, const float* verts, int nviews, const float* proj, int H, int W, const uint8_t* dilated, uint8_t* keep,
                              void* stream) {
    if (n < 0 || nviews < 0 || H <= 1 || W <= 1 || (nviews > 0 && (!proj || !dilated)) || (n > 0 && (!verts || !keep)))
        return api_fail(SURFEL_E_INVALID, "eval_cull_vertices: bad arguments");
    if (n == 0) return 0;
    hipLaunchKernelGGL(eval_cull_kernel, dim3(grid(n)), dim3(ET), 0, static_cast<hipStream_t>(stream), n, verts, nviews, proj, H, W, dilated, keep);
    return launched("eval_cull_kernel");
}

}  // extern "C"
