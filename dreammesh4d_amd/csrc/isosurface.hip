// isosurface.hip -- mesh extraction from Gaussians (gfx950): the occupancy field of a set of Gaussians and marching cubes on
// it, the kernels behind dreammesh4d_amd/isosurface.py (C ABI: include/dm4d_isosurface.h).
//
// Reference: GaussianIO.extract_fields / extract_mesh, custom/threestudio-dreammesh4d/geometry/gaussian_io.py:174-291 (a triple
// Python loop over blocks with [M, L, 6] temporaries, then mcubes.marching_cubes on the CPU) and gaussian_3d_coeff,
// geometry/gaussian_base.py:63-96.  Semantics: DESIGN.md "Mesh extraction from Gaussians".  Nothing below uses an atomic, so
// two runs give the same bytes.
//
//   k_iso_gaussian_records  Gaussian -> 16-float record (centre, opacity, inverse covariance in float64 rounded once, rgb),
//                           its box of eligible blocks and their number                       (one lane per Gaussian)
//   [caller: exclusive prefix sum of the counts]
//   k_iso_pair_keys         Gaussian -> one key block * N + g per block of its box
//   [caller: sort of the keys; first key position of every block]
//   k_iso_density_field     one workgroup per block (per 512-voxel chunk of a block when it has more): batches of 64 of the
//                           block's Gaussians staged in LDS, every thread owns two voxels and adds the batch to its float64
//                           sums in list order.  All lanes of a wave read the same LDS record (a broadcast), so the loop is
//                           VALU work: ~21 float32 operations for `power`, the exponential, one conversion and one float64 add
//                           per channel.
//   k_mc_classify / k_mc_vertices / k_mc_faces   marching cubes: case, triangle and vertex counts per voxel; one vertex per
//                           crossed edge owned by the voxel, recorded in a dense edge -> vertex table; faces through that table.
#include "common.h"
#include "hostcheck.h"
#include "mc_table.h"
#include "../../include/dm4d.h"
#include "../../include/dm4d_isosurface.h"

namespace dm4d {

constexpr int kIsoThreads = 256;
constexpr int kIsoVoxelsPerThread = 2;
constexpr int kIsoChunk = kIsoThreads * kIsoVoxelsPerThread;      // voxels of a block one workgroup owns
constexpr int kIsoBatch = kIsoThreads / 4;                        // Gaussians staged at once: four lanes load one 64-byte record
static_assert(DM4D_ISO_RECORD_FLOATS == 16, "a record is four float4");

__global__ __launch_bounds__(kIsoThreads) void k_iso_gaussian_records(const int64_t N, const float *__restrict__ xyzn,
                                                                      const float *__restrict__ stdn, const float *__restrict__ rotation,
                                                                      const float *__restrict__ opacity, const float *__restrict__ rgb,
                                                                      const int nb, const float *__restrict__ vmin,
                                                                      const float *__restrict__ vmax, float *__restrict__ records,
                                                                      int32_t *__restrict__ box, int64_t *__restrict__ count)
{
    const int64_t g = (int64_t)blockIdx.x * kIsoThreads + threadIdx.x;
    if (g >= N) return;
    // inverse covariance: everything from the float32 inputs on in float64, one rounding at the end
    double qw = rotation[4 * g], qx = rotation[4 * g + 1], qy = rotation[4 * g + 2], qz = rotation[4 * g + 3];
    const double norm = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
    qw /= norm; qx /= norm; qy /= norm; qz /= norm;
    const double R[3][3] = {{1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy)},
                            {2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx)},
                            {2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)}};
    double s2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) s2[k] = (double)stdn[3 * g + k] * (double)stdn[3 * g + k];
    auto cov = [&](int i, int j) { return R[i][0] * s2[0] * R[j][0] + R[i][1] * s2[1] * R[j][1] + R[i][2] * s2[2] * R[j][2]; };
    const double a = cov(0, 0), b = cov(0, 1), c = cov(0, 2), d = cov(1, 1), e = cov(1, 2), f = cov(2, 2);
    const double inv_det = 1.0 / (a * d * f + 2.0 * e * c * b - e * e * a - c * c * d - b * b * f + 1e-24);
    float *rec = records + DM4D_ISO_RECORD_FLOATS * g;
    const float cx = xyzn[3 * g], cy = xyzn[3 * g + 1], cz = xyzn[3 * g + 2];
    rec[0] = cx; rec[1] = cy; rec[2] = cz; rec[3] = opacity[g];
    rec[4] = (float)((d * f - e * e) * inv_det);
    rec[5] = (float)((e * c - b * f) * inv_det);
    rec[6] = (float)((e * b - c * d) * inv_det);
    rec[7] = (float)((a * f - c * c) * inv_det);
    rec[8] = (float)((b * c - e * a) * inv_det);
    rec[9] = (float)((a * d - b * b) * inv_det);
    rec[10] = rec[11] = 0.f;
    rec[12] = rgb ? rgb[3 * g] : 0.f;
    rec[13] = rgb ? rgb[3 * g + 1] : 0.f;
    rec[14] = rgb ? rgb[3 * g + 2] : 0.f;
    rec[15] = 0.f;
    // eligible blocks per axis: vmin and vmax ascend with b, so {b : vmin[b] < centre < vmax[b]} is an interval
    const float ctr[3] = {cx, cy, cz};
    int64_t n = 1;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        int first = nb, last = -1;
        for (int bb = 0; bb < nb; ++bb) {
            if (vmin[bb] < ctr[ax] && ctr[ax] < vmax[bb]) {
                first = first < bb ? first : bb;
                last = bb;
            }
        }
        box[6 * g + 2 * ax] = first;
        box[6 * g + 2 * ax + 1] = last;
        n *= last >= first ? (int64_t)(last - first + 1) : 0;
    }
    count[g] = n;
}

__global__ __launch_bounds__(kIsoThreads) void k_iso_pair_keys(const int64_t N, const int64_t P, const int nb, const int32_t *__restrict__ box,
                                                               const int64_t *__restrict__ offset, int64_t *__restrict__ keys)
{
    const int64_t g = (int64_t)blockIdx.x * kIsoThreads + threadIdx.x;
    if (g >= N) return;
    int lo[3], hi[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {                 // the box is re-checked against the grid before it addresses anything
        lo[ax] = box[6 * g + 2 * ax] < 0 ? 0 : box[6 * g + 2 * ax];
        hi[ax] = box[6 * g + 2 * ax + 1] >= nb ? nb - 1 : box[6 * g + 2 * ax + 1];
    }
    int64_t at = offset[g];
    if (at < 0) return;
    for (int bx = lo[0]; bx <= hi[0]; ++bx)
        for (int by = lo[1]; by <= hi[1]; ++by)
            for (int bz = lo[2]; bz <= hi[2]; ++bz) {
                if (at >= P) return;
                keys[at++] = (((int64_t)bx * nb + by) * nb + bz) * N + g;
            }
}

template <bool COLOR>
__global__ __launch_bounds__(kIsoThreads) void k_iso_density_field(const int64_t N, const int64_t P, const int R, const int nb, const int s,
                                                                   const int chunks, const float *__restrict__ coords,
                                                                   const float4 *__restrict__ records, const int64_t *__restrict__ keys,
                                                                   const int64_t *__restrict__ block_start, float *__restrict__ occ,
                                                                   float *__restrict__ csum)
{
    __shared__ float4 s_rec[kIsoBatch][4];
    const int tid = threadIdx.x;
    const int64_t blk = (int64_t)(blockIdx.x / (unsigned)chunks);
    const int chunk = (int)(blockIdx.x % (unsigned)chunks);
    const int bz = (int)(blk % nb), by = (int)((blk / nb) % nb), bx = (int)(blk / ((int64_t)nb * nb));
    const int s3 = s * s * s;
    float px[kIsoVoxelsPerThread], py[kIsoVoxelsPerThread], pz[kIsoVoxelsPerThread];
    int64_t out[kIsoVoxelsPerThread];
    double acc[kIsoVoxelsPerThread], accc[kIsoVoxelsPerThread][3];
#pragma unroll
    for (int k = 0; k < kIsoVoxelsPerThread; ++k) {
        const int l = chunk * kIsoChunk + k * kIsoThreads + tid;
        const bool valid = l < s3;
        const int lx = valid ? l / (s * s) : 0, ly = valid ? (l / s) % s : 0, lz = valid ? l % s : 0;
        const int ix = bx * s + lx, iy = by * s + ly, iz = bz * s + lz;         // < R: bx < nb, lx < s, nb * s == R
        px[k] = coords[ix]; py[k] = coords[iy]; pz[k] = coords[iz];
        out[k] = valid ? ((int64_t)ix * R + iy) * R + iz : -1;
        acc[k] = 0.0;
        accc[k][0] = accc[k][1] = accc[k][2] = 0.0;
    }
    int64_t begin = block_start[blk], end = block_start[blk + 1];
    begin = begin < 0 ? 0 : (begin > P ? P : begin);
    end = end < begin ? begin : (end > P ? P : end);
    for (int64_t base = begin; base < end; base += kIsoBatch) {
        const int n = end - base < kIsoBatch ? (int)(end - base) : kIsoBatch;
        const int gi = tid >> 2, part = tid & 3;
        if (gi < n) {
            const int64_t g = keys[base + gi] - blk * N;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);                          // opacity 0: a key outside the block adds nothing
            if ((uint64_t)g < (uint64_t)N && (COLOR || part < 3)) v = records[4 * g + part];
            s_rec[gi][part] = v;
        }
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            const float4 c = s_rec[j][0], q0 = s_rec[j][1], q1 = s_rec[j][2];
            float4 col = make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (COLOR) col = s_rec[j][3];
#pragma unroll
            for (int k = 0; k < kIsoVoxelsPerThread; ++k) {
                const float x = px[k] - c.x, y = py[k] - c.y, z = pz[k] - c.z;
                // the reference's expression, operation for operation (no contraction: -ffp-contract=off)
                float power = -0.5f * (((x * x) * q0.x + (y * y) * q0.w) + (z * z) * q1.y);
                power = power - (x * y) * q0.y;
                power = power - (x * z) * q0.z;
                power = power - (y * z) * q1.x;
                const float w = (!(power <= 0.f) || power < -86.0f) ? 0.f : det_expf(power);
                const float val = c.w * w;
                acc[k] = acc[k] + (double)val;
                if constexpr (COLOR) {
                    accc[k][0] = accc[k][0] + (double)(val * col.x);
                    accc[k][1] = accc[k][1] + (double)(val * col.y);
                    accc[k][2] = accc[k][2] + (double)(val * col.z);
                }
            }
        }
        __syncthreads();                             // the next batch overwrites the records
    }
#pragma unroll
    for (int k = 0; k < kIsoVoxelsPerThread; ++k) {
        if (out[k] < 0) continue;
        occ[out[k]] = (float)acc[k];
        if constexpr (COLOR) {
            csum[3 * out[k]] = (float)accc[k][0];
            csum[3 * out[k] + 1] = (float)accc[k][1];
            csum[3 * out[k] + 2] = (float)accc[k][2];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- marching cubes
__device__ __forceinline__ int64_t mc_corner(const int64_t n, const int c, const int R1, const int R2)
{
    return n + (int64_t)(c >> 2 & 1) * R1 * R2 + (int64_t)(c >> 1 & 1) * R2 + (c & 1);
}

__global__ __launch_bounds__(kIsoThreads) void k_mc_classify(const int R0, const int R1, const int R2, const float *__restrict__ f,
                                                             const double threshold, int32_t *__restrict__ code,
                                                             int32_t *__restrict__ n_tris, int32_t *__restrict__ n_verts)
{
    const int64_t total = (int64_t)R0 * R1 * R2;
    const int64_t n = (int64_t)blockIdx.x * kIsoThreads + threadIdx.x;
    if (n >= total) return;
    const int k = (int)(n % R2), j = (int)((n / R2) % R1), i = (int)(n / ((int64_t)R1 * R2));
    const bool more[3] = {i + 1 < R0, j + 1 < R1, k + 1 < R2};
    const bool in0 = (double)f[n] >= threshold;
    int flags = 0;
    if (more[0] && ((double)f[n + (int64_t)R1 * R2] >= threshold) != in0) flags |= 1;
    if (more[1] && ((double)f[n + R2] >= threshold) != in0) flags |= 2;
    if (more[2] && ((double)f[n + 1] >= threshold) != in0) flags |= 4;
    int cs = 0;
    if (more[0] && more[1] && more[2]) {
#pragma unroll
        for (int c = 0; c < 8; ++c) cs |= ((double)f[mc_corner(n, c, R1, R2)] >= threshold) ? 1 << c : 0;
    }
    code[n] = cs | flags << 8;
    n_tris[n] = kMcTriCount[cs];
    n_verts[n] = __popc(flags);
}

template <bool COLOR>
__global__ __launch_bounds__(kIsoThreads) void k_mc_vertices(const int R0, const int R1, const int R2, const float *__restrict__ f,
                                                             const float *__restrict__ csum, const double threshold,
                                                             const int32_t *__restrict__ code, const int64_t *__restrict__ vert_start,
                                                             const int64_t V, float *__restrict__ verts, float *__restrict__ colors,
                                                             int32_t *__restrict__ edge_vertex)
{
    const int64_t total = (int64_t)R0 * R1 * R2;
    const int64_t n = (int64_t)blockIdx.x * kIsoThreads + threadIdx.x;
    if (n >= total) return;
    const int flags = code[n] >> 8 & 7;
    if (!flags) return;
    const int idx[3] = {(int)(n / ((int64_t)R1 * R2)), (int)((n / R2) % R1), (int)(n % R2)};
    const int64_t step[3] = {(int64_t)R1 * R2, R2, 1};
    const bool more[3] = {idx[0] + 1 < R0, idx[1] + 1 < R1, idx[2] + 1 < R2};
    int64_t vid = vert_start[n];
    const double fa = (double)f[n];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        if (!(flags >> ax & 1) || !more[ax]) continue;
        if (vid < 0 || vid >= V) return;
        const int64_t m = n + step[ax];
        const double fb = (double)f[m];
        const double t = (threshold - fa) / (fb - fa);
#pragma unroll
        for (int d = 0; d < 3; ++d) verts[3 * vid + d] = d == ax ? (float)((double)idx[d] + t) : (float)idx[d];
        if constexpr (COLOR) {
            const double den = fa + t * (fb - fa);
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const double ca = (double)csum[3 * n + d], cb = (double)csum[3 * m + d];
                colors[3 * vid + d] = (float)((ca + t * (cb - ca)) / den);
            }
        }
        edge_vertex[3 * n + ax] = (int32_t)vid;
        ++vid;
    }
}

__global__ __launch_bounds__(kIsoThreads) void k_mc_faces(const int R0, const int R1, const int R2, const int32_t *__restrict__ code,
                                                          const int64_t *__restrict__ tri_start, const int32_t *__restrict__ edge_vertex,
                                                          const int64_t F, int64_t *__restrict__ faces)
{
    const int64_t total = (int64_t)R0 * R1 * R2;
    const int64_t n = (int64_t)blockIdx.x * kIsoThreads + threadIdx.x;
    if (n >= total) return;
    const int cs = code[n] & 255;
    const int nt = kMcTriCount[cs];
    if (!nt) return;
    // a case other than 0 is only ever written for a voxel with a cube, so every corner offset stays inside the grid; the check
    // below keeps a corrupted code from reading outside it
    const int k = (int)(n % R2), j = (int)((n / R2) % R1), i = (int)(n / ((int64_t)R1 * R2));
    if (!(i + 1 < R0 && j + 1 < R1 && k + 1 < R2)) return;
    const int64_t first = tri_start[n];
    for (int t = 0; t < nt; ++t) {
        const int64_t ft = first + t;
        if (ft < 0 || ft >= F) return;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int e = kMcTris[cs][3 * t + c];
            const int64_t m = mc_corner(n, kMcEdgeBase[e], R1, R2);
            faces[3 * ft + c] = (int64_t)edge_vertex[3 * m + kMcEdgeAxis[e]];
        }
    }
}

static bool iso_bad_grid(const char *fn, int32_t R0, int32_t R1, int32_t R2)
{
    if (R0 >= 1 && R1 >= 1 && R2 >= 1 && (int64_t)R0 * R1 * R2 * 3 <= (int64_t)INT32_MAX) return false;
    set_error("%s: grid %d x %d x %d (every extent must be at least 1 and 3 * R0 * R1 * R2 at most %d)", fn, R0, R1, R2, INT32_MAX);
    return true;
}

}  // namespace dm4d

using namespace dm4d;

extern "C" {

int dm4d_iso_version(void) { return DM4D_ISO_ABI_VERSION; }

int dm4d_iso_gaussian_records(int64_t N, const void *xyzn, const void *stdn, const void *rotation, const void *opacity, const void *rgb,
                              int32_t num_blocks, const void *vmin, const void *vmax, void *records, void *box, void *count, void *stream)
{
    const char *fn = "dm4d_iso_gaussian_records";
    if (bad_count(fn, "N", N)) return DM4D_ERR_INVALID;
    if (num_blocks < 1 || num_blocks > DM4D_ISO_MAX_RESOLUTION) { set_error("%s: num_blocks = %d is outside [1, %d]", fn, num_blocks, DM4D_ISO_MAX_RESOLUTION); return DM4D_ERR_INVALID; }
    if (N == 0) return DM4D_OK;
    DM4D_REFUSE_NULL(!xyzn || !stdn || !rotation || !opacity || !vmin || !vmax || !records || !box || !count)
    hipLaunchKernelGGL(k_iso_gaussian_records, dim3(blocks(N, kIsoThreads)), dim3(kIsoThreads), 0, (hipStream_t)stream, N, (const float *)xyzn,
                       (const float *)stdn, (const float *)rotation, (const float *)opacity, (const float *)rgb, (int)num_blocks,
                       (const float *)vmin, (const float *)vmax, (float *)records, (int32_t *)box, (int64_t *)count);
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

int dm4d_iso_pair_keys(int64_t N, int64_t P, int32_t num_blocks, const void *box, const void *offset, void *keys, void *stream)
{
    const char *fn = "dm4d_iso_pair_keys";
    if (bad_count(fn, "N", N) || bad_count(fn, "P", P, INT64_MAX / 2)) return DM4D_ERR_INVALID;
    if (num_blocks < 1 || num_blocks > DM4D_ISO_MAX_RESOLUTION) { set_error("%s: num_blocks = %d is outside [1, %d]", fn, num_blocks, DM4D_ISO_MAX_RESOLUTION); return DM4D_ERR_INVALID; }
    if (N == 0 || P == 0) return DM4D_OK;
    DM4D_REFUSE_NULL(!box || !offset || !keys)
    hipLaunchKernelGGL(k_iso_pair_keys, dim3(blocks(N, kIsoThreads)), dim3(kIsoThreads), 0, (hipStream_t)stream, N, P, (int)num_blocks,
                       (const int32_t *)box, (const int64_t *)offset, (int64_t *)keys);
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

int dm4d_iso_density_field(int64_t N, int64_t P, int32_t R, int32_t num_blocks, const void *coords, const void *records, const void *keys,
                           const void *block_start, void *occ, void *csum, void *stream)
{
    const char *fn = "dm4d_iso_density_field";
    if (bad_count(fn, "N", N) || bad_count(fn, "P", P, INT64_MAX / 2)) return DM4D_ERR_INVALID;
    if (R < 2 || R > DM4D_ISO_MAX_RESOLUTION || num_blocks < 1 || R % num_blocks != 0) {
        set_error("%s: resolution %d must lie in [2, %d] and be a multiple of num_blocks = %d", fn, R, DM4D_ISO_MAX_RESOLUTION, num_blocks);
        return DM4D_ERR_INVALID;
    }
    DM4D_REFUSE_NULL(!coords || !block_start || !occ || (P > 0 && (!records || !keys)))
    const int s = R / num_blocks;
    const int chunks = (s * s * s + kIsoChunk - 1) / kIsoChunk;
    const int64_t grid = (int64_t)num_blocks * num_blocks * num_blocks * chunks;      // <= R^3 <= 2^27
    if (csum)
        hipLaunchKernelGGL(k_iso_density_field<true>, dim3((unsigned)grid), dim3(kIsoThreads), 0, (hipStream_t)stream, N, P, (int)R, (int)num_blocks, s,
                           chunks, (const float *)coords, (const float4 *)records, (const int64_t *)keys, (const int64_t *)block_start,
                           (float *)occ, (float *)csum);
    else
        hipLaunchKernelGGL(k_iso_density_field<false>, dim3((unsigned)grid), dim3(kIsoThreads), 0, (hipStream_t)stream, N, P, (int)R, (int)num_blocks, s,
                           chunks, (const float *)coords, (const float4 *)records, (const int64_t *)keys, (const int64_t *)block_start,
                           (float *)occ, (float *)csum);
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

int dm4d_iso_mc_classify(int32_t R0, int32_t R1, int32_t R2, const void *f, double threshold, void *code, void *n_tris, void *n_verts,
                         void *stream)
{
    const char *fn = "dm4d_iso_mc_classify";
    if (iso_bad_grid(fn, R0, R1, R2)) return DM4D_ERR_INVALID;
    if (!(threshold == threshold)) { set_error("%s: the threshold is not a number", fn); return DM4D_ERR_INVALID; }
    DM4D_REFUSE_NULL(!f || !code || !n_tris || !n_verts)
    hipLaunchKernelGGL(k_mc_classify, dim3(blocks((int64_t)R0 * R1 * R2, kIsoThreads)), dim3(kIsoThreads), 0, (hipStream_t)stream, (int)R0, (int)R1, (int)R2,
                       (const float *)f, threshold, (int32_t *)code, (int32_t *)n_tris, (int32_t *)n_verts);
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

int dm4d_iso_mc_vertices(int32_t R0, int32_t R1, int32_t R2, const void *f, const void *csum, double threshold, const void *code,
                         const void *vert_start, int64_t V, void *verts, void *colors, void *edge_vertex, void *stream)
{
    const char *fn = "dm4d_iso_mc_vertices";
    if (iso_bad_grid(fn, R0, R1, R2) || bad_count(fn, "V", V)) return DM4D_ERR_INVALID;
    if (V == 0) return DM4D_OK;                      // nothing to write: an empty colour array has no address
    if ((csum != nullptr) != (colors != nullptr)) { set_error("%s: csum and colors go together", fn); return DM4D_ERR_INVALID; }
    DM4D_REFUSE_NULL(!f || !code || !vert_start || !verts || !edge_vertex)
    const dim3 grid(blocks((int64_t)R0 * R1 * R2, kIsoThreads)), block(kIsoThreads);
    if (csum)
        hipLaunchKernelGGL(k_mc_vertices<true>, grid, block, 0, (hipStream_t)stream, (int)R0, (int)R1, (int)R2, (const float *)f, (const float *)csum,
                           threshold, (const int32_t *)code, (const int64_t *)vert_start, V, (float *)verts, (float *)colors, (int32_t *)edge_vertex);
    else
        hipLaunchKernelGGL(k_mc_vertices<false>, grid, block, 0, (hipStream_t)stream, (int)R0, (int)R1, (int)R2, (const float *)f, (const float *)csum,
                           threshold, (const int32_t *)code, (const int64_t *)vert_start, V, (float *)verts, (float *)colors, (int32_t *)edge_vertex);
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

int dm4d_iso_mc_faces(int32_t R0, int32_t R1, int32_t R2, const void *code, const void *tri_start, const void *edge_vertex, int64_t F,
                      void *faces, void *stream)
{
    const char *fn = "dm4d_iso_mc_faces";
    if (iso_bad_grid(fn, R0, R1, R2) || bad_count(fn, "F", F, INT64_MAX / 4)) return DM4D_ERR_INVALID;
    if (F == 0) return DM4D_OK;
    DM4D_REFUSE_NULL(!code || !tri_start || !edge_vertex || !faces)
    hipLaunchKernelGGL(k_mc_faces, dim3(blocks((int64_t)R0 * R1 * R2, kIsoThreads)), dim3(kIsoThreads), 0, (hipStream_t)stream, (int)R0, (int)R1, (int)R2,
                       (const int32_t *)code, (const int64_t *)tri_start, (const int32_t *)edge_vertex, F, (int64_t *)faces);
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

}  // extern "C"
