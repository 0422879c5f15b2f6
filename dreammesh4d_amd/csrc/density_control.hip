// density_control.hip -- adaptive density control of free Gaussians (gfx950): densification statistics, classification,
// the plan of the output rows and the one row move that applies it to every parameter and Adam moment, the kernels behind
// dreammesh4d_amd/density_control.py (C ABI: include/dm4d_density.h).
//
// Reference: GaussianBaseModel, custom/threestudio-dreammesh4d/geometry/gaussian_base.py:575-579 (reset_opacity), 606-683 (the
// optimiser surgery), 720-812 (densify_and_split, densify_and_clone, densify, prune), 816-870 (the statistics and the schedule):
// chains of boolean-mask indexing, repeat, cat and bmm per tensor.  Here it is classify -> scan -> gather, and every row moves
// once.  Semantics: DESIGN.md "Adaptive density control".  Nothing below uses an atomic, and no kernel waits on another
// workgroup: the scan is reduce-then-scan in three launches, every loop has a bound known at launch.
//
//   k_dc_stats            one lane per Gaussian, all views of the step in ascending order
//   k_dc_classify_densify / k_dc_classify_prune      one lane per Gaussian -> kind (uint8)
//   k_dc_count            workgroup totals of the three ranks (kept, clone, split) over tiles of 4096 kinds
//   k_dc_scan_totals      ONE workgroup of 1024 lanes: exclusive scan of the totals in place (a lane owns a contiguous chunk of
//                         ceil(G / 1024) totals), and the four counts
//   k_dc_plan_rows        the tile's own scan again, then src / role of the output rows
//   k_dc_move             all arrays in one launch: a workgroup owns 1024 consecutive 4- or 16-byte units of one array's OUTPUT,
//                         so writes are coalesced and every moved float is read once and written once
//   k_dc_split_children   xyz and _scaling of the child rows
//   k_dc_reset_opacity
#include "common.h"
#include "hostcheck.h"
#include "../../include/dm4d.h"
#include "../../include/dm4d_density.h"

namespace dm4d {

constexpr int kDcThreads = 256;
constexpr int kDcPerLane = 16;                               // kinds per lane: one 16-byte load
constexpr int kDcTile = kDcThreads * kDcPerLane;             // kinds per workgroup of the scan
constexpr int kDcScanThreads = 1024;
constexpr int kDcMoveIters = 4;
constexpr int kDcMoveUnits = kDcThreads * kDcMoveIters;      // units (4 or 16 bytes) of one workgroup of the move
static_assert(DM4D_DC_KEEP == 0 && DM4D_DC_DROP == 1 && DM4D_DC_CLONE == 2 && DM4D_DC_SPLIT == 3, "the 2-bit codes below");
static_assert((int64_t)DM4D_DC_MAX_ROWS * DM4D_DC_MAX_CHILDREN <= (int64_t)1 << 31, "output rows stay below 2^31");

__device__ __forceinline__ float dc_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// exp of the three log-scales of row i; with `sphere` the exp of their float32 mean on all axes (get_scaling, :373-378)
__device__ __forceinline__ void dc_scales(const float *__restrict__ scaling, int64_t i, bool sphere, float (&s)[3])
{
    const float a = scaling[3 * i], b = scaling[3 * i + 1], c = scaling[3 * i + 2];
    if (sphere) {
        s[0] = s[1] = s[2] = expf((a + b + c) / 3.0f);
    } else {
        s[0] = expf(a); s[1] = expf(b); s[2] = expf(c);
    }
}

__global__ __launch_bounds__(kDcThreads) void k_dc_stats(const int B, const int64_t N, const float *__restrict__ grad2d,
                                                         const int32_t *__restrict__ radii, float *__restrict__ accum,
                                                         float *__restrict__ denom, float *__restrict__ max_radii)
{
    const int64_t i = (int64_t)blockIdx.x * kDcThreads + threadIdx.x;
    if (i >= N) return;
    float acc = accum[i], den = denom[i], mr = max_radii[i];
    for (int b = 0; b < B; ++b) {
        const int32_t r = radii[(int64_t)b * N + i];
        if (r > 0) {
            const float *g = grad2d + ((int64_t)b * N + i) * 3;
            const float gx = g[0], gy = g[1];
            acc += sqrtf(gx * gx + gy * gy);
            den += 1.0f;
        }
        mr = fmaxf(mr, (float)r);
    }
    accum[i] = acc; denom[i] = den; max_radii[i] = mr;
}

__global__ __launch_bounds__(kDcThreads) void k_dc_classify_densify(const int64_t N, const float *__restrict__ accum,
                                                                    const float *__restrict__ denom, const float *__restrict__ scaling,
                                                                    const float grad_threshold, const float split_thresh,
                                                                    const int sphere, uint8_t *__restrict__ kind)
{
    const int64_t i = (int64_t)blockIdx.x * kDcThreads + threadIdx.x;
    if (i >= N) return;
    const float d = denom[i];
    const float g = d == 0.0f ? 0.0f : accum[i] / d;
    float s[3];
    dc_scales(scaling, i, sphere != 0, s);
    const float nrm = sqrtf(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    uint8_t k = DM4D_DC_KEEP;
    if (g >= grad_threshold) k = nrm > split_thresh ? DM4D_DC_SPLIT : (nrm <= split_thresh ? DM4D_DC_CLONE : DM4D_DC_KEEP);
    kind[i] = k;
}

__global__ __launch_bounds__(kDcThreads) void k_dc_classify_prune(const int64_t N, const float *__restrict__ opacity,
                                                                  const float min_opacity, const float *__restrict__ max_radii,
                                                                  const float *__restrict__ radius_limit, uint8_t *__restrict__ kind)
{
    const int64_t i = (int64_t)blockIdx.x * kDcThreads + threadIdx.x;
    if (i >= N) return;
    bool drop = dc_sigmoid(opacity[i]) < min_opacity;
    if (radius_limit) drop = drop || max_radii[i] > radius_limit[0];
    kind[i] = drop ? DM4D_DC_DROP : DM4D_DC_KEEP;
}

// ------------------------------------------------------------------------------------------------ the plan
// The 16 kinds of a lane as 2-bit codes, element e in bits 2e .. 2e + 1; rows past N read as DROP.
__device__ __forceinline__ uint32_t dc_load_codes(const uint8_t *__restrict__ kind, int64_t base, int64_t N, bool aligned)
{
    uint32_t codes = 0;
    if (aligned && base + kDcPerLane <= N) {
        const uint4 v = *reinterpret_cast<const uint4 *>(kind + base);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int b = 0; b < 4; ++b) codes |= ((w[q] >> (8 * b)) & 3u) << (2 * (4 * q + b));
    } else {
#pragma unroll
        for (int e = 0; e < kDcPerLane; ++e) {
            const uint32_t k = base + e < N ? (uint32_t)(kind[base + e] & 3u) : (uint32_t)DM4D_DC_DROP;
            codes |= k << (2 * e);
        }
    }
    return codes;
}

// (kept | clone << 16, split) of a lane's codes: kept = KEEP or CLONE (low bit clear), clone = 2, split = 3
__device__ __forceinline__ void dc_count_codes(uint32_t codes, uint32_t &kc, uint32_t &sp)
{
    const uint32_t lo = codes & 0x55555555u, hi = (codes >> 1) & 0x55555555u;
    kc = (uint32_t)__popc(~lo & 0x55555555u) | ((uint32_t)__popc(hi & ~lo) << 16);
    sp = (uint32_t)__popc(hi & lo);
}

__global__ __launch_bounds__(kDcThreads) void k_dc_count(const int64_t N, const uint8_t *__restrict__ kind, const int aligned,
                                                         uint4 *__restrict__ wg_totals)
{
    __shared__ uint32_t s_kc[kDcThreads / DM4D_WAVE], s_sp[kDcThreads / DM4D_WAVE];
    const int64_t base = ((int64_t)blockIdx.x * kDcThreads + threadIdx.x) * kDcPerLane;
    uint32_t kc, sp;
    dc_count_codes(dc_load_codes(kind, base, N, aligned != 0), kc, sp);
    kc = wave_sum_u32(kc);                                   // a tile holds 4096 rows: both 16-bit fields hold their sums
    sp = wave_sum_u32(sp);
    const int wave = threadIdx.x / DM4D_WAVE;
    if (lane_id() == DM4D_WAVE - 1) { s_kc[wave] = kc; s_sp[wave] = sp; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t a = 0, b = 0;
#pragma unroll
        for (int w = 0; w < kDcThreads / DM4D_WAVE; ++w) { a += s_kc[w]; b += s_sp[w]; }
        wg_totals[blockIdx.x] = make_uint4(a & 0xffffu, a >> 16, b, 0u);
    }
}

// One workgroup.  Lane t owns totals [t * chunk, (t + 1) * chunk): its sum, an exclusive scan of the sums across the workgroup,
// then the running offsets written back in place.  totals_out = the number of KEEP, DROP, CLONE and SPLIT rows.
__global__ __launch_bounds__(kDcScanThreads) void k_dc_scan_totals(const int64_t N, const int G, const int chunk,
                                                                   uint4 *__restrict__ wg_totals, int64_t *__restrict__ totals_out)
{
    constexpr int kWaves = kDcScanThreads / DM4D_WAVE;
    __shared__ uint32_t s_w[3][kWaves];
    const int t = threadIdx.x, wave = t / DM4D_WAVE;
    const int begin = min(t * chunk, G), end = min(begin + chunk, G);      // chunk <= 64: t * chunk stays small
    uint32_t own[3] = {0u, 0u, 0u};
    for (int q = begin; q < end; ++q) {
        const uint4 v = wg_totals[q];
        own[0] += v.x; own[1] += v.y; own[2] += v.z;
    }
    uint32_t incl[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        incl[c] = wave_incl_scan_u32(own[c], 0);
        if (lane_id() == DM4D_WAVE - 1) s_w[c][wave] = incl[c];
    }
    __syncthreads();
    uint32_t run[3], all[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const uint32_t v = s_w[c][w];
            before += w < wave ? v : 0u;
            total += v;
        }
        run[c] = before + incl[c] - own[c];
        all[c] = total;
    }
    for (int q = begin; q < end; ++q) {
        const uint4 v = wg_totals[q];
        wg_totals[q] = make_uint4(run[0], run[1], run[2], 0u);
        run[0] += v.x; run[1] += v.y; run[2] += v.z;
    }
    if (t == 0) {
        totals_out[DM4D_DC_KEEP] = (int64_t)all[0] - (int64_t)all[1];
        totals_out[DM4D_DC_DROP] = N - (int64_t)all[0] - (int64_t)all[2];
        totals_out[DM4D_DC_CLONE] = (int64_t)all[1];
        totals_out[DM4D_DC_SPLIT] = (int64_t)all[2];
    }
}

__global__ __launch_bounds__(kDcThreads) void k_dc_plan_rows(const int64_t N, const uint8_t *__restrict__ kind, const int aligned,
                                                             const int S, const uint4 *__restrict__ wg_offsets,
                                                             const int64_t *__restrict__ totals, const int64_t M,
                                                             int32_t *__restrict__ src, uint8_t *__restrict__ role)
{
    __shared__ uint32_t s_kc[kDcThreads / DM4D_WAVE], s_sp[kDcThreads / DM4D_WAVE];
    const int64_t base = ((int64_t)blockIdx.x * kDcThreads + threadIdx.x) * kDcPerLane;
    const uint32_t codes = dc_load_codes(kind, base, N, aligned != 0);
    uint32_t kc, sp;
    dc_count_codes(codes, kc, sp);
    const uint32_t kc_incl = wave_incl_scan_u32(kc, 0), sp_incl = wave_incl_scan_u32(sp, 0);
    const int wave = threadIdx.x / DM4D_WAVE;
    if (lane_id() == DM4D_WAVE - 1) { s_kc[wave] = kc_incl; s_sp[wave] = sp_incl; }
    __syncthreads();
    uint32_t kc_before = 0, sp_before = 0;
#pragma unroll
    for (int w = 0; w < kDcThreads / DM4D_WAVE; ++w) {
        kc_before += w < wave ? s_kc[w] : 0u;
        sp_before += w < wave ? s_sp[w] : 0u;
    }
    const uint32_t kc_excl = kc_before + kc_incl - kc, sp_excl = sp_before + sp_incl - sp;
    const uint4 off = wg_offsets[blockIdx.x];
    const int64_t n_clone = totals[DM4D_DC_CLONE], n_split = totals[DM4D_DC_SPLIT];
    const int64_t n_kept = totals[DM4D_DC_KEEP] + n_clone;
    int64_t r_kept = (int64_t)off.x + (kc_excl & 0xffffu);
    int64_t r_clone = n_kept + (int64_t)off.y + (kc_excl >> 16);
    int64_t r_split = n_kept + n_clone + (int64_t)off.z + sp_excl;
#pragma unroll
    for (int e = 0; e < kDcPerLane; ++e) {
        const uint32_t k = (codes >> (2 * e)) & 3u;
        const int32_t i = (int32_t)(base + e);               // rows past N read as DROP
        if ((k & 1u) == 0u) {
            if (r_kept < M) { src[r_kept] = i; role[r_kept] = DM4D_DC_ROLE_KEPT; }
            ++r_kept;
        }
        if (k == DM4D_DC_CLONE) {
            if (r_clone < M) { src[r_clone] = i; role[r_clone] = DM4D_DC_ROLE_CLONE; }
            ++r_clone;
        }
        if (k == DM4D_DC_SPLIT) {
            for (int c = 0; c < S; ++c) {
                const int64_t j = r_split + (int64_t)c * n_split;
                if (j < M) { src[j] = i; role[j] = (uint8_t)(DM4D_DC_ROLE_CHILD + c); }
            }
            ++r_split;
        }
    }
}

// ------------------------------------------------------------------------------------------------ the move
struct DcMoveTable {
    const uint32_t *in[DM4D_DC_MAX_ARRAYS];
    uint32_t *out[DM4D_DC_MAX_ARRAYS];
    int64_t tile_start[DM4D_DC_MAX_ARRAYS + 1];              // first workgroup of every array
    int32_t units_per_row[DM4D_DC_MAX_ARRAYS];               // width, or width / 4 for the 16-byte path
    uint8_t vec[DM4D_DC_MAX_ARRAYS];
    uint8_t flags[DM4D_DC_MAX_ARRAYS];
    int32_t count;
};

__global__ __launch_bounds__(kDcThreads) void k_dc_move(const DcMoveTable T, const int64_t M, const int32_t *__restrict__ src,
                                                        const uint8_t *__restrict__ role)
{
    const int64_t tile = blockIdx.x;
    int a = 0;
    for (int q = 1; q < DM4D_DC_MAX_ARRAYS; ++q)
        if (q < T.count && tile >= T.tile_start[q]) a = q;
    const uint32_t upr = (uint32_t)T.units_per_row[a];
    const bool vec = T.vec[a] != 0, zero_new = (T.flags[a] & DM4D_DC_ZERO_NEW) != 0, skip_children = (T.flags[a] & DM4D_DC_SKIP_CHILDREN) != 0;
    const uint32_t *__restrict__ in = T.in[a];
    uint32_t *__restrict__ out = T.out[a];
    const int64_t u0 = (tile - T.tile_start[a]) * kDcMoveUnits;
    const int64_t row0 = u0 / upr;                           // uniform: once per workgroup
    const uint32_t rem0 = (uint32_t)(u0 - row0 * upr);
    const int64_t units = M * upr;
#pragma unroll
    for (int it = 0; it < kDcMoveIters; ++it) {
        const uint32_t l = (uint32_t)(it * kDcThreads + threadIdx.x);
        if (u0 + l >= units) continue;
        const uint32_t ll = rem0 + l, dr = ll / upr, c = ll - dr * upr;
        const int64_t j = row0 + dr;
        const uint8_t r = role[j];
        if (skip_children && r >= DM4D_DC_ROLE_CHILD) continue;
        const bool zero = zero_new && r != DM4D_DC_ROLE_KEPT;
        const int64_t from = (int64_t)src[j] * upr + c, to = j * upr + c;
        if (vec) {
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (!zero) v = reinterpret_cast<const uint4 *>(in)[from];
            reinterpret_cast<uint4 *>(out)[to] = v;
        } else {
            uint32_t v = 0u;
            if (!zero) v = in[from];
            out[to] = v;
        }
    }
}

__global__ __launch_bounds__(kDcThreads) void k_dc_split_children(const int64_t N, const int64_t M, const int64_t first_child,
                                                                  const int S, const int sphere, const int32_t *__restrict__ src,
                                                                  const uint8_t *__restrict__ role, const float *__restrict__ xyz_in,
                                                                  const float *__restrict__ scaling_in, const float *__restrict__ rotation_in,
                                                                  const float *__restrict__ noise, float *__restrict__ xyz_out,
                                                                  float *__restrict__ scaling_out)
{
    const int64_t j = first_child + (int64_t)blockIdx.x * kDcThreads + threadIdx.x;
    if (j >= M) return;
    const int k = (int)role[j] - DM4D_DC_ROLE_CHILD;
    const int64_t i = src[j];
    if (k < 0 || k >= S || i < 0 || i >= N) return;          // not a child row of this plan: nothing is read or written
    float s[3];
    dc_scales(scaling_in, i, sphere != 0, s);
    const float fS = (float)S;
    const float *e = noise + ((int64_t)k * N + i) * 3;
    const float v0 = e[0] * (s[0] / fS), v1 = e[1] * (s[1] / fS), v2 = e[2] * (s[2] / fS);
    const float r0 = rotation_in[4 * i], r1 = rotation_in[4 * i + 1], r2 = rotation_in[4 * i + 2], r3 = rotation_in[4 * i + 3];
    const float norm = sqrtf(r0 * r0 + r1 * r1 + r2 * r2 + r3 * r3);
    const float r = r0 / norm, x = r1 / norm, y = r2 / norm, z = r3 / norm;
    const float R00 = 1.0f - 2.0f * (y * y + z * z), R01 = 2.0f * (x * y - r * z), R02 = 2.0f * (x * z + r * y);
    const float R10 = 2.0f * (x * y + r * z), R11 = 1.0f - 2.0f * (x * x + z * z), R12 = 2.0f * (y * z - r * x);
    const float R20 = 2.0f * (x * z - r * y), R21 = 2.0f * (y * z + r * x), R22 = 1.0f - 2.0f * (x * x + y * y);
    xyz_out[3 * j] = (R00 * v0 + R01 * v1 + R02 * v2) + xyz_in[3 * i];
    xyz_out[3 * j + 1] = (R10 * v0 + R11 * v1 + R12 * v2) + xyz_in[3 * i + 1];
    xyz_out[3 * j + 2] = (R20 * v0 + R21 * v1 + R22 * v2) + xyz_in[3 * i + 2];
    const float shrink = 0.8f * fS;
    scaling_out[3 * j] = logf(s[0] / shrink);
    scaling_out[3 * j + 1] = logf(s[1] / shrink);
    scaling_out[3 * j + 2] = logf(s[2] / shrink);
}

__global__ __launch_bounds__(kDcThreads) void k_dc_reset_opacity(const int64_t N, float *__restrict__ opacity, float *__restrict__ exp_avg,
                                                                 float *__restrict__ exp_avg_sq)
{
    const int64_t i = (int64_t)blockIdx.x * kDcThreads + threadIdx.x;
    if (i >= N) return;
    const float o = dc_sigmoid(opacity[i]) * 0.9f;
    opacity[i] = logf(o / (1.0f - o));
    if (exp_avg) exp_avg[i] = 0.0f;
    if (exp_avg_sq) exp_avg_sq[i] = 0.0f;
}

// ------------------------------------------------------------------------------------------------ host side
static bool dc_bad_children(const char *fn, int32_t S)
{
    if (S >= 1 && S <= DM4D_DC_MAX_CHILDREN) return false;
    set_error("%s: S = %d children per split is outside [1, %d]", fn, S, DM4D_DC_MAX_CHILDREN);
    return true;
}

static int64_t dc_tiles(int64_t n) { return (n + kDcTile - 1) / kDcTile; }

}  // namespace dm4d

using namespace dm4d;

extern "C" {

int dm4d_dc_version(void) { return DM4D_DC_ABI_VERSION; }

int dm4d_dc_accumulate_stats(int32_t B, int64_t N, const void *grad2d, const void *radii, void *accum, void *denom, void *max_radii,
                             void *stream)
{
    const char *fn = "dm4d_dc_accumulate_stats";
    if (bad_count(fn, "N", N, DM4D_DC_MAX_ROWS)) return DM4D_ERR_INVALID;
    if (B < 0 || B > DM4D_DC_MAX_VIEWS) { set_error("%s: B = %d views is outside [0, %d]", fn, B, DM4D_DC_MAX_VIEWS); return DM4D_ERR_INVALID; }
    if (N == 0 || B == 0) return DM4D_OK;
    DM4D_REFUSE_NULL(!grad2d || !radii || !accum || !denom || !max_radii)
    hipLaunchKernelGGL(k_dc_stats, dim3(blocks(N, kDcThreads)), dim3(kDcThreads), 0, (hipStream_t)stream, (int)B, N, (const float *)grad2d,
                       (const int32_t *)radii, (float *)accum, (float *)denom, (float *)max_radii);
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

int dm4d_dc_classify_densify(int64_t N, const void *accum, const void *denom, const void *scaling, float grad_threshold,
                             float split_thresh, int32_t sphere, void *kind, void *stream)
{
    const char *fn = "dm4d_dc_classify_densify";
    if (bad_count(fn, "N", N, DM4D_DC_MAX_ROWS)) return DM4D_ERR_INVALID;
    if (!(grad_threshold > 0.0f)) { set_error("%s: grad_threshold = %g must be > 0", fn, (double)grad_threshold); return DM4D_ERR_INVALID; }
    if (!(split_thresh == split_thresh)) { set_error("%s: split_thresh is not a number", fn); return DM4D_ERR_INVALID; }
    if (N == 0) return DM4D_OK;
    DM4D_REFUSE_NULL(!accum || !denom || !scaling || !kind)
    hipLaunchKernelGGL(k_dc_classify_densify, dim3(blocks(N, kDcThreads)), dim3(kDcThreads), 0, (hipStream_t)stream, N, (const float *)accum,
                       (const float *)denom, (const float *)scaling, grad_threshold, split_thresh, (int)sphere, (uint8_t *)kind);
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

int dm4d_dc_classify_prune(int64_t N, const void *opacity, float min_opacity, const void *max_radii, const void *radius_limit,
                           void *kind, void *stream)
{
    const char *fn = "dm4d_dc_classify_prune";
    if (bad_count(fn, "N", N, DM4D_DC_MAX_ROWS)) return DM4D_ERR_INVALID;
    if (!(min_opacity == min_opacity)) { set_error("%s: min_opacity is not a number", fn); return DM4D_ERR_INVALID; }
    if (N == 0) return DM4D_OK;
    DM4D_REFUSE_NULL(!opacity || !kind || (radius_limit && !max_radii))
    hipLaunchKernelGGL(k_dc_classify_prune, dim3(blocks(N, kDcThreads)), dim3(kDcThreads), 0, (hipStream_t)stream, N, (const float *)opacity,
                       min_opacity, (const float *)max_radii, (const float *)radius_limit, (uint8_t *)kind);
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

int64_t dm4d_dc_plan_scratch_bytes(int64_t N)
{
    if (bad_count("dm4d_dc_plan_scratch_bytes", "N", N, DM4D_DC_MAX_ROWS)) return DM4D_ERR_INVALID;
    const int64_t G = dc_tiles(N);
    return (G > 0 ? G : 1) * (int64_t)sizeof(uint4);
}

int dm4d_dc_plan_count(int64_t N, const void *kind, void *scratch, int64_t scratch_bytes, void *totals, void *stream)
{
    const char *fn = "dm4d_dc_plan_count";
    if (bad_count(fn, "N", N, DM4D_DC_MAX_ROWS)) return DM4D_ERR_INVALID;
    DM4D_REFUSE_NULL(!totals || !scratch || (N > 0 && !kind))
    if (short_scratch(fn, scratch_bytes, dm4d_dc_plan_scratch_bytes(N))) return DM4D_ERR_CAPACITY;
    if (misaligned(scratch, 16) || misaligned(totals, 8)) { set_error("%s: scratch must be 16-byte, totals 8-byte aligned", fn); return DM4D_ERR_INVALID; }
    const int G = (int)dc_tiles(N);                          // <= 65536
    if (G > 0)
        hipLaunchKernelGGL(k_dc_count, dim3((unsigned)G), dim3(kDcThreads), 0, (hipStream_t)stream, N, (const uint8_t *)kind,
                           !misaligned(kind, 16), (uint4 *)scratch);
    const int chunk = (G + kDcScanThreads - 1) / kDcScanThreads;
    hipLaunchKernelGGL(k_dc_scan_totals, dim3(1), dim3(kDcScanThreads), 0, (hipStream_t)stream, N, G, chunk, (uint4 *)scratch,
                       (int64_t *)totals);
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

int dm4d_dc_plan_rows(int64_t N, const void *kind, int32_t S, const void *scratch, int64_t scratch_bytes, const void *totals, int64_t M,
                      void *src, void *role, void *stream)
{
    const char *fn = "dm4d_dc_plan_rows";
    if (bad_count(fn, "N", N, DM4D_DC_MAX_ROWS) || dc_bad_children(fn, S)) return DM4D_ERR_INVALID;
    if (bad_count(fn, "M", M, N * (int64_t)(S > 2 ? S : 2))) return DM4D_ERR_INVALID;
    if (N == 0 || M == 0) return DM4D_OK;
    DM4D_REFUSE_NULL(!kind || !scratch || !totals || !src || !role)
    if (short_scratch(fn, scratch_bytes, dm4d_dc_plan_scratch_bytes(N))) return DM4D_ERR_CAPACITY;
    if (misaligned(scratch, 16) || misaligned(totals, 8) || misaligned(src, 4)) {
        set_error("%s: scratch must be 16-byte, totals 8-byte, src 4-byte aligned", fn);
        return DM4D_ERR_INVALID;
    }
    hipLaunchKernelGGL(k_dc_plan_rows, dim3((unsigned)dc_tiles(N)), dim3(kDcThreads), 0, (hipStream_t)stream, N, (const uint8_t *)kind,
                       !misaligned(kind, 16), (int)S, (const uint4 *)scratch, (const int64_t *)totals, M, (int32_t *)src, (uint8_t *)role);
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

int dm4d_dc_move(int64_t N, int64_t M, const void *src, const void *role, const dm4d_dc_arrays *arrays, void *stream)
{
    const char *fn = "dm4d_dc_move";
    if (bad_count(fn, "N", N, DM4D_DC_MAX_ROWS) || bad_count(fn, "M", M, N * (int64_t)DM4D_DC_MAX_CHILDREN)) return DM4D_ERR_INVALID;
    DM4D_REFUSE_NULL(!arrays)
    if (arrays->count < 0 || arrays->count > DM4D_DC_MAX_ARRAYS) {
        set_error("%s: %d arrays, the table holds %d", fn, arrays->count, DM4D_DC_MAX_ARRAYS);
        return DM4D_ERR_INVALID;
    }
    DcMoveTable T = {};
    T.count = arrays->count;
    int64_t tiles = 0;
    for (int a = 0; a < arrays->count; ++a) {
        const int32_t w = arrays->width[a];
        if (w <= 0 || w > (1 << 20)) { set_error("%s: array %d has row width %d (must lie in [1, %d])", fn, a, w, 1 << 20); return DM4D_ERR_INVALID; }
        if (arrays->flags[a] & ~(DM4D_DC_ZERO_NEW | DM4D_DC_SKIP_CHILDREN)) { set_error("%s: array %d has unknown flags %d", fn, a, arrays->flags[a]); return DM4D_ERR_INVALID; }
        if (M > 0 && (!arrays->in[a] || !arrays->out[a])) { set_error("%s: array %d has a null pointer", fn, a); return DM4D_ERR_INVALID; }
        if (misaligned(arrays->in[a], 4) || misaligned(arrays->out[a], 4)) { set_error("%s: array %d is not 4-byte aligned", fn, a); return DM4D_ERR_INVALID; }
        const bool vec = w % 4 == 0 && !misaligned(arrays->in[a], 16) && !misaligned(arrays->out[a], 16);
        T.in[a] = (const uint32_t *)arrays->in[a];
        T.out[a] = (uint32_t *)arrays->out[a];
        T.vec[a] = vec;
        T.flags[a] = (uint8_t)arrays->flags[a];
        T.units_per_row[a] = vec ? w / 4 : w;
        T.tile_start[a] = tiles;
        tiles += (M * T.units_per_row[a] + kDcMoveUnits - 1) / kDcMoveUnits;
    }
    for (int a = arrays->count; a <= DM4D_DC_MAX_ARRAYS; ++a) T.tile_start[a] = tiles;
    // a launch's total size in threads is a 32-bit number
    if (tiles > (int64_t)(UINT32_MAX / kDcThreads)) {
        set_error("%s: %lld workgroups, a launch holds %u: move the arrays in several calls", fn, (long long)tiles, UINT32_MAX / kDcThreads);
        return DM4D_ERR_UNSUPPORTED;
    }
    if (M == 0 || arrays->count == 0) return DM4D_OK;
    DM4D_REFUSE_NULL(!src || !role)
    hipLaunchKernelGGL(k_dc_move, dim3((unsigned)tiles), dim3(kDcThreads), 0, (hipStream_t)stream, T, M, (const int32_t *)src,
                       (const uint8_t *)role);
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

int dm4d_dc_split_children(int64_t N, int64_t M, int64_t first_child, int32_t S, int32_t sphere, const void *src, const void *role,
                           const void *xyz_in, const void *scaling_in, const void *rotation_in, const void *noise, void *xyz_out,
                           void *scaling_out, void *stream)
{
    const char *fn = "dm4d_dc_split_children";
    if (bad_count(fn, "N", N, DM4D_DC_MAX_ROWS) || dc_bad_children(fn, S)) return DM4D_ERR_INVALID;
    if (bad_count(fn, "M", M, N * (int64_t)DM4D_DC_MAX_CHILDREN) || bad_count(fn, "first_child", first_child, M)) return DM4D_ERR_INVALID;
    if (first_child == M) return DM4D_OK;
    DM4D_REFUSE_NULL(!src || !role || !xyz_in || !scaling_in || !rotation_in || !noise || !xyz_out || !scaling_out)
    hipLaunchKernelGGL(k_dc_split_children, dim3(blocks(M - first_child, kDcThreads)), dim3(kDcThreads), 0, (hipStream_t)stream, N, M, first_child,
                       (int)S, (int)sphere, (const int32_t *)src, (const uint8_t *)role, (const float *)xyz_in, (const float *)scaling_in,
                       (const float *)rotation_in, (const float *)noise, (float *)xyz_out, (float *)scaling_out);
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

int dm4d_dc_reset_opacity(int64_t N, void *opacity, void *exp_avg, void *exp_avg_sq, void *stream)
{
    const char *fn = "dm4d_dc_reset_opacity";
    if (bad_count(fn, "N", N, DM4D_DC_MAX_ROWS)) return DM4D_ERR_INVALID;
    if (N == 0) return DM4D_OK;
    DM4D_REFUSE_NULL(!opacity)
    hipLaunchKernelGGL(k_dc_reset_opacity, dim3(blocks(N, kDcThreads)), dim3(kDcThreads), 0, (hipStream_t)stream, N, (float *)opacity,
                       (float *)exp_avg, (float *)exp_avg_sq);
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

}  // extern "C"
