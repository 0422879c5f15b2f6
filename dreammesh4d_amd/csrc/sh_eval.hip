// sh_eval.hip -- view-dependent colour of N Gaussians from spherical-harmonic coefficients of degree 0..3 (gfx950).
//
//   forward   dir = normalize(mean - campos);  v = sum_{k < M'} B_k(dir) sh[k] + 0.5 per channel;
//             rgb = max(v, 0), clamped = v < 0                                   M' = (degree + 1)^2 of the M stored
//   backward  dL_dsh[k] = clamped ? 0 : B_k(dir) dL_drgb (k < M'), 0 (k >= M');
//             dL_dmean  = (g - dir (dir . g)) / |mean - campos|,  g = sum_ch dL_drgb[ch] sum_k grad B_k(dir) sh[k][ch]
//
// Replaces the view-dependent branch of SuGaR.get_points_rgb (C/geometry/sugar.py:640-661, eval_sh at :733-820), and is the
// colour stage of the rasterizer for sh_degree > 0.
//
// One lane owns one Gaussian (no atomics: two runs are bit-identical); a wave owns 64 consecutive ones.  A Gaussian's
// coefficients are 12 M' contiguous bytes (192 at degree 3), so a lane reading its own row would make every wave load touch
// 64 lines.  Instead the wave copies its 64 rows through LDS: coalesced 16-byte global loads (the rows of a wave are one
// contiguous block when M' == M; 16-byte pieces of each row when only the row starts are aligned; dwords otherwise), an LDS
// image with an ODD row stride (3 M' | 1 floats), which each lane then reads along its row with ds_read_b32, conflict-free
// (64 different rows, stride coprime to the 32 banks).  The backward writes B_k dL_drgb over the coefficient it has just read,
// in place, and the wave streams the image out to dL_dsh the same way (all M coefficients of the 64 rows are one contiguous
// block; the columns >= 3 M' are written as zeros without passing through LDS).
//
// Bandwidth-bound: forward N (12 M' + 12) bytes in, N 15 out; backward N (12 M' + 12 + 12 + 3 [+ 4 radii]) in, N (12 M + 12) out
// [+ 12 N read when the direction term is added to an existing dL_dmeans3D].
#include "common.h"
#include "raster.h"
#include "sh.h"

namespace dm4d {

constexpr int kShThreads = 256;                 // 4 waves, 64 Gaussians each
constexpr int kShWaves = kShThreads / 64;
constexpr int sh_row_stride(int degree) { return (3 * sh_count(degree)) | 1; }

// Copies the first L floats of `rows` rows (row stride S floats, L <= S) from `src` into the wave's LDS image (row stride LP).
// `vec`: src is 16-byte aligned.
template <int L, int LP>
__device__ __forceinline__ void sh_stage_in(const float *__restrict__ src, const int S, const int rows, const bool vec,
                                            float *__restrict__ img, const int lane)
{
    if (vec && S == L) {                                  // one contiguous block of rows * L floats
        const int n = rows * L, nv = n >> 2;
#pragma unroll 4
        for (int j = lane; j < nv; j += 64) {
            const float4 v = reinterpret_cast<const float4 *>(src)[j];
            const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int f = 4 * j + c;
                img[(f / L) * LP + f % L] = e[c];
            }
        }
        const int f = 4 * nv + lane;                      // at most 3 floats of a last, partial tile
        if (f < n) img[(f / L) * LP + f % L] = src[f];
    } else if (vec && L % 4 == 0 && S % 4 == 0) {         // L / 4 aligned 16-byte pieces per row
        constexpr int Q = L / 4 > 0 ? L / 4 : 1;
        const int nv = rows * Q;
#pragma unroll 4
        for (int j = lane; j < nv; j += 64) {
            const int r = j / Q, q = j % Q;
            const float4 v = *reinterpret_cast<const float4 *>(src + (size_t)r * S + 4 * q);
            float *o = img + r * LP + 4 * q;
            o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
        }
    } else {
        const int n = rows * L;
#pragma unroll 4
        for (int f = lane; f < n; f += 64) {
            const int r = f / L, q = f % L;
            img[r * LP + q] = src[(size_t)r * S + q];
        }
    }
}

// Writes rows x S floats to `dst` (contiguous): column q < L of row r from the LDS image, zeros for q >= L.
template <int L, int LP>
__device__ __forceinline__ void sh_stage_out(float *__restrict__ dst, const int S, const int rows, const bool vec,
                                             const float *__restrict__ img, const int lane)
{
    const int n = rows * S;
    const int nv = vec ? n >> 2 : 0;
    // (r, q) = divmod(4 j, S) carried from one iteration to the next: j advances by 64, 4 j by 256
    const int dr = 256 / S, dq = 256 - dr * S;
    int r = (4 * lane) / S, q = 4 * lane - r * S;
    for (int j = lane; j < nv; j += 64) {
        float e[4];
        int rc = r, qc = q;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            e[c] = qc < L ? img[rc * LP + qc] : 0.f;
            if (++qc == S) { qc = 0; ++rc; }
        }
        reinterpret_cast<float4 *>(dst)[j] = make_float4(e[0], e[1], e[2], e[3]);
        r += dr;
        q += dq;
        if (q >= S) { q -= S; ++r; }
    }
    for (int f = 4 * nv + lane; f < n; f += 64) {        // a partial tile's last floats, or everything when dst is not aligned
        const int rf = f / S, qf = f - rf * S;
        dst[f] = qf < L ? img[rf * LP + qf] : 0.f;
    }
}

// orders a wave's LDS writes before the reads other lanes of the SAME wave make of them (a wave's DS operations execute in
// order; the fences keep the compiler from moving them across)
__device__ __forceinline__ void sh_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int DEG>
__global__ __launch_bounds__(kShThreads) void k_sh_eval_fwd(const int N, const int M, const float *__restrict__ means3D,
                                                            const float *__restrict__ campos, const float *__restrict__ shs,
                                                            const int vec, float *__restrict__ rgb, uint8_t *__restrict__ clamped)
{
    constexpr int K = sh_count(DEG), L = 3 * K, LP = sh_row_stride(DEG);
    __shared__ float s_img[kShWaves][64 * LP];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int i0 = (blockIdx.x * kShWaves + wv) * 64;     // first Gaussian of this wave
    if (i0 >= N) return;
    const int rows = min(64, N - i0), S = 3 * M;
    float *img = s_img[wv];
    sh_stage_in<L, LP>(shs + (size_t)i0 * S, S, rows, vec != 0, img, lane);
    sh_wave_sync();
    if (lane >= rows) return;
    const int i = i0 + lane;
    float x, y, z, len;
    sh_direction(means3D[3 * (size_t)i], means3D[3 * (size_t)i + 1], means3D[3 * (size_t)i + 2], campos[0], campos[1], campos[2],
                 x, y, z, len);
    float B[K];
    sh_basis<DEG>(x, y, z, B);
    const float *row = img + lane * LP;
    float v[3] = {B[0] * row[0], B[0] * row[1], B[0] * row[2]};
#pragma unroll
    for (int k = 1; k < K; ++k) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) v[ch] = v[ch] + B[k] * row[3 * k + ch];
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float w = v[ch] + 0.5f;
        clamped[3 * (size_t)i + ch] = (w < 0.f);
        rgb[3 * (size_t)i + ch] = fmaxf(w, 0.f);
    }
}

// radii: optional [N]; a Gaussian with radius 0 gets zero gradients (the rasterizer's culled ones).
// accumulate: the direction term is ADDED to dL_dmeans3D (the rasterizer's backward has already written the geometric part).
template <int DEG>
__global__ __launch_bounds__(kShThreads) void k_sh_eval_bwd(const int N, const int M, const float *__restrict__ means3D,
                                                            const float *__restrict__ campos, const float *__restrict__ shs,
                                                            const int vec, const uint8_t *__restrict__ clamped,
                                                            const int32_t *__restrict__ radii, const float *__restrict__ dL_drgb,
                                                            float *__restrict__ dL_dsh, float *__restrict__ dL_dmeans3D,
                                                            const int accumulate)
{
    constexpr int K = sh_count(DEG), L = 3 * K, LP = sh_row_stride(DEG);
    __shared__ float s_img[kShWaves][64 * LP];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int i0 = (blockIdx.x * kShWaves + wv) * 64;
    if (i0 >= N) return;
    const int rows = min(64, N - i0), S = 3 * M;
    float *img = s_img[wv];
    if (DEG > 0) sh_stage_in<L, LP>(shs + (size_t)i0 * S, S, rows, vec != 0, img, lane);   // degree 0 has no direction term
    sh_wave_sync();
    if (lane < rows) {
        const int i = i0 + lane;
        float x, y, z, len;
        sh_direction(means3D[3 * (size_t)i], means3D[3 * (size_t)i + 1], means3D[3 * (size_t)i + 2], campos[0], campos[1],
                     campos[2], x, y, z, len);
        const bool live = radii ? radii[i] > 0 : true;
        bool on[3];
        float g[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            on[ch] = live && !clamped[3 * (size_t)i + ch];
            g[ch] = on[ch] ? dL_drgb[3 * (size_t)i + ch] : 0.f;
        }
        float B[K];
        sh_basis<DEG>(x, y, z, B);
        float *row = img + lane * LP;
        float gd[3] = {0.f, 0.f, 0.f};      // dL/d(dir)
        if constexpr (DEG > 0) {
            float bx[K], by[K], bz[K];
            sh_basis_grad<DEG>(x, y, z, bx, by, bz);
#pragma unroll
            for (int k = 1; k < K; ++k) {
                const float t = (g[0] * row[3 * k] + g[1] * row[3 * k + 1]) + g[2] * row[3 * k + 2];
                gd[0] = gd[0] + bx[k] * t;
                gd[1] = gd[1] + by[k] * t;
                gd[2] = gd[2] + bz[k] * t;
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) row[3 * k + ch] = on[ch] ? B[k] * g[ch] : 0.f;
        }
        float dm[3] = {0.f, 0.f, 0.f};
        if (DEG > 0 && len > 0.f) {
            const float t = (x * gd[0] + y * gd[1]) + z * gd[2];
            dm[0] = (gd[0] - x * t) / len;
            dm[1] = (gd[1] - y * t) / len;
            dm[2] = (gd[2] - z * t) / len;
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            float *o = dL_dmeans3D + 3 * (size_t)i + a;
            *o = accumulate ? *o + dm[a] : dm[a];
        }
    }
    sh_wave_sync();
    sh_stage_out<L, LP>(dL_dsh + (size_t)i0 * S, S, rows, vec != 0, img, lane);
}

static bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

int launch_sh_eval_forward(int N, int degree, int M, const float *means3D, const float *campos, const float *shs, float *rgb,
                           uint8_t *clamped, hipStream_t st)
{
    if (N <= 0) return DM4D_OK;
    const dim3 grid((N + kShThreads - 1) / kShThreads), block(kShThreads);
    const int vec = aligned16(shs);
    switch (degree) {
    case 0: hipLaunchKernelGGL(k_sh_eval_fwd<0>, grid, block, 0, st, N, M, means3D, campos, shs, vec, rgb, clamped); break;
    case 1: hipLaunchKernelGGL(k_sh_eval_fwd<1>, grid, block, 0, st, N, M, means3D, campos, shs, vec, rgb, clamped); break;
    case 2: hipLaunchKernelGGL(k_sh_eval_fwd<2>, grid, block, 0, st, N, M, means3D, campos, shs, vec, rgb, clamped); break;
    default: hipLaunchKernelGGL(k_sh_eval_fwd<3>, grid, block, 0, st, N, M, means3D, campos, shs, vec, rgb, clamped); break;
    }
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

int launch_sh_eval_backward(int N, int degree, int M, const float *means3D, const float *campos, const float *shs,
                            const uint8_t *clamped, const int32_t *radii, const float *dL_drgb, float *dL_dsh, float *dL_dmeans3D,
                            int accumulate, hipStream_t st)
{
    if (N <= 0) return DM4D_OK;
    const dim3 grid((N + kShThreads - 1) / kShThreads), block(kShThreads);
    const int vec = aligned16(shs) && aligned16(dL_dsh);
#define DM4D_SH_BWD(D)                                                                                                          \
    hipLaunchKernelGGL(k_sh_eval_bwd<D>, grid, block, 0, st, N, M, means3D, campos, shs, vec, clamped, radii, dL_drgb, dL_dsh, \
                       dL_dmeans3D, accumulate)
    switch (degree) {
    case 0: DM4D_SH_BWD(0); break;
    case 1: DM4D_SH_BWD(1); break;
    case 2: DM4D_SH_BWD(2); break;
    default: DM4D_SH_BWD(3); break;
    }
#undef DM4D_SH_BWD
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

}  // namespace dm4d
