// texbake.hip -- texture baking of the textured mesh export (gfx950).
//
// The reference's predict path (custom/threestudio-dreammesh4d/system/base.py:72-292) builds a square-packed UV atlas of
// the canonical surface mesh, initialises every texel from the face's Gaussians, then, for 120 views, rasterizes the mesh
// with pytorch3d, samples an "index texture" to find the texel under every covered pixel, and averages the Gaussian
// render into the texels.  pytorch3d has no ROCm build; its part is restated here:
//
//   k_tex_atlas_init   one thread per (face, texel of its triangle): the texel's point on the face from the atlas formula
//                      in closed form, the face's G Gaussians' Mahalanobis densities, the first-index argmax, SH2RGB of
//                      that Gaussian's DC coefficient written at the transposed and flipped position (base.py:137-209).
//   k_mesh_raster      one thread per (view, face): a z-buffer rasterizer with one 64-bit atomicMin of
//                      (depth bits << 32) | face per covered pixel: nearest view-space depth wins, the lower face on equal
//                      depth.  A face whose bounding box exceeds kBigFacePixels goes to a list instead,
//   k_mesh_sweep       which 32 x 32-pixel tiles sweep with whole workgroups (a full-screen face does not serialise on a lane).
//   k_mesh_resolve     one thread per (view, pixel): the winner's perspective-correct barycentrics, the interpolated UV and
//                      the nearest texel of pytorch3d's TexturesUV (align_corners, border padding, v flipped).
//   k_tex_claim        per view, the lowest linear pixel index among the view's pixels on a texel claims it: a u64 word
//                      per texel, (epoch << 32) | ~pixel, atomicMax (no clears: a later epoch always beats an older claim);
//   k_tex_accumulate   the claiming pixel adds its colour into sum[texel] and 1 into count[texel] with plain stores.
//                      One launch pair per view, in view order: the float sums have a fixed order.
//
// Projection: the rasterizer's own (raster_preprocess.hip: row-vector full_proj_transform, 1 / (w + 1e-7), ndc2Pix), so
// pixel (x, y) of the mesh image is pixel (x, y) of the Gaussian image; its centre is NDC (2x + 1) / W - 1, where
// pytorch3d puts it too.  The projected vertices are float32 as in the Gaussian path; the coverage tests, depths and
// barycentrics are evaluated in float64 from them (gfx950 has full-rate-enough FP64; the edge-inclusive rule then only
// depends on the float32 projection, which a CPU restatement reproduces bit for bit).
//
// Conventions restated from pytorch3d's published behaviour and NOT checked against pytorch3d (parity unpinned): coverage
// exactly on an edge (inclusive here), faces with a vertex at view depth <= znear (0.1) are skipped, the float arithmetic
// of grid_sample's nearest rounding.
#include <math.h>

#include "common.h"
#include "../../include/dm4d.h"

namespace dm4d {

constexpr int kTexThreads = 256;
constexpr int kBigFacePixels = 1024;     // bounding boxes above this many pixels are swept by workgroups
constexpr int kSweepTile = 32;           // a sweep workgroup covers a 32 x 32 pixel tile of one view
constexpr int kSweepRows = 16;           // gridDim.y of the sweep: list entries are strided over it
constexpr float kZnear = 0.1f;           // znear of the Gaussian camera (threestudio/utils/ops.py:398-413)
constexpr float kSHC0 = 0.28209479177387814f;

struct SV {                              // a projected vertex: pixel coordinates and view-space depth
    float px, py, z;
};

__device__ __forceinline__ SV project(const float *__restrict__ v, const float *__restrict__ V, const float *__restrict__ P,
                                      int W, int H)
{
    const float x = v[0], y = v[1], z = v[2];
    SV o;
    o.z = ((V[2] * x + V[6] * y) + V[10] * z) + V[14];
    const float hx = ((P[0] * x + P[4] * y) + P[8] * z) + P[12];
    const float hy = ((P[1] * x + P[5] * y) + P[9] * z) + P[13];
    const float hw = ((P[3] * x + P[7] * y) + P[11] * z) + P[15];
    const float pw = 1.0f / (hw + 0.0000001f);
    o.px = ((hx * pw + 1.0f) * (float)W - 1.0f) * 0.5f;
    o.py = ((hy * pw + 1.0f) * (float)H - 1.0f) * 0.5f;
    return o;
}

// twice the signed area of (a, b, p)
__device__ __forceinline__ double edge_fn(double ax, double ay, double bx, double by, double px, double py)
{
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
}

struct Tri {
    SV v[3];
    double area;
};

// the three projected vertices of face f in view b; false if the face is skipped (near plane, zero area)
__device__ __forceinline__ bool setup_tri(int f, const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                          const float *__restrict__ V, const float *__restrict__ P, int W, int H, Tri &t)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) t.v[k] = project(verts + 3 * (size_t)faces[3 * (size_t)f + k], V, P, W, H);
    if (!(t.v[0].z > kZnear && t.v[1].z > kZnear && t.v[2].z > kZnear)) return false;
    t.area = edge_fn(t.v[0].px, t.v[0].py, t.v[1].px, t.v[1].py, t.v[2].px, t.v[2].py);
    return t.area != 0.0 && isfinite(t.area);
}

// edge functions of pixel centre (x, y); true if inside or on an edge
__device__ __forceinline__ bool cover(const Tri &t, int x, int y, double w[3])
{
    const double px = x, py = y;
    w[0] = edge_fn(t.v[1].px, t.v[1].py, t.v[2].px, t.v[2].py, px, py);
    w[1] = edge_fn(t.v[2].px, t.v[2].py, t.v[0].px, t.v[0].py, px, py);
    w[2] = edge_fn(t.v[0].px, t.v[0].py, t.v[1].px, t.v[1].py, px, py);
    if (t.area > 0.0) return w[0] >= 0.0 && w[1] >= 0.0 && w[2] >= 0.0;
    return w[0] <= 0.0 && w[1] <= 0.0 && w[2] <= 0.0;
}

// perspective-correct barycentrics and view depth from the edge functions
__device__ __forceinline__ double persp(const Tri &t, const double w[3], double b[3])
{
    double q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = (w[k] / t.area) / (double)t.v[k].z;
    const double s = (q[0] + q[1]) + q[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) b[k] = q[k] / s;
    return 1.0 / s;
}

__device__ __forceinline__ void zbuf_min(unsigned long long *zbuf, double depth, int f)
{
    const unsigned long long key = ((unsigned long long)__float_as_uint((float)depth) << 32) | (unsigned long long)(uint32_t)f;
    atomicMin(zbuf, key);
}

struct Box {
    int x0, x1, y0, y1;
};

__device__ __forceinline__ Box bbox(const Tri &t, int W, int H)
{
    const float xmin = fminf(fminf(t.v[0].px, t.v[1].px), t.v[2].px), xmax = fmaxf(fmaxf(t.v[0].px, t.v[1].px), t.v[2].px);
    const float ymin = fminf(fminf(t.v[0].py, t.v[1].py), t.v[2].py), ymax = fmaxf(fmaxf(t.v[0].py, t.v[1].py), t.v[2].py);
    const float x0 = fmaxf(ceilf(xmin), 0.f), x1 = fminf(floorf(xmax), (float)(W - 1));
    const float y0 = fmaxf(ceilf(ymin), 0.f), y1 = fminf(floorf(ymax), (float)(H - 1));
    Box r{0, -1, 0, -1};                 // empty unless the clamped ranges are ordered (NaN compares false)
    if (x0 <= x1 && y0 <= y1) r = Box{(int)x0, (int)x1, (int)y0, (int)y1};
    return r;
}

// ---------------------------------------------------------------------------------------- atlas
__global__ __launch_bounds__(kTexThreads) void k_tex_atlas_init(int F, int G, int S, int n_axis, int T, const float *__restrict__ verts,
                                                                const int32_t *__restrict__ faces, const float *__restrict__ means,
                                                                const float *__restrict__ rotations, const float *__restrict__ scales,
                                                                const float *__restrict__ sh_dc, float *__restrict__ texture)
{
    const int n_tri = S * (S - 1) / 2;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= F * n_tri) return;
    const int f = idx / n_tri, k = idx - f * n_tri;
    const int top = f & 1, sq = f >> 1, a = sq / n_axis, bsq = sq - a * n_axis;
    // (ti, tj) of texel k: bottom rows ti = 0..S-2 hold tj = 0..ti; top rows ti = 0..S-1 hold tj = ti+1..S-1 (base.py:137-146)
    int ti = 0, tj, rem = k;
    float b1, b2;
    const float den = (float)(S - 3);
    if (!top) {
        while (rem > ti) { rem -= ti + 1; ++ti; }
        tj = rem;
        b1 = (float)(S - 2 - ti) / den;
        b2 = (float)(tj - 1) / den;
    } else {
        while (rem >= S - 1 - ti) { rem -= S - 1 - ti; ++ti; }
        tj = ti + 1 + rem;
        b1 = (float)(ti - 1) / den;
        b2 = (float)(S - 1 - tj) / den;
    }
    const float b0 = 1.0f - (b1 + b2);
    const float *v0 = verts + 3 * (size_t)faces[3 * (size_t)f], *v1 = verts + 3 * (size_t)faces[3 * (size_t)f + 1],
                *v2 = verts + 3 * (size_t)faces[3 * (size_t)f + 2];
    float p[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = (b0 * v0[c] + b1 * v1[c]) + b2 * v2[c];
    float best = -1.0f;
    int arg = 0;
    for (int g = 0; g < G; ++g) {
        const size_t i = (size_t)f * G + g;
        const float4 q = reinterpret_cast<const float4 *>(rotations)[i];      // (w, x, y, z)
        // quaternion_to_matrix (pytorch3d/transforms/rotation_conversions.py), then R diag(1 / clamp(s, 1e-8))
        const float r = q.x, qi = q.y, qj = q.z, qk = q.w;
        const float two_s = 2.0f / (((r * r + qi * qi) + qj * qj) + qk * qk);
        float R[9] = {1.0f - two_s * (qj * qj + qk * qk), two_s * (qi * qj - qk * r), two_s * (qi * qk + qj * r),
                      two_s * (qi * qj + qk * r), 1.0f - two_s * (qi * qi + qk * qk), two_s * (qj * qk - qi * r),
                      two_s * (qi * qk - qj * r), two_s * (qj * qk + qi * r), 1.0f - two_s * (qi * qi + qj * qj)};
        float d = 0.0f;
        const float sh[3] = {p[0] - means[3 * i], p[1] - means[3 * i + 1], p[2] - means[3 * i + 2]};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float inv = 1.0f / fmaxf(scales[3 * i + j], 1e-8f);
            const float w = ((R[j] * inv) * sh[0] + (R[3 + j] * inv) * sh[1]) + (R[6 + j] * inv) * sh[2];
            d = d + w * w;
        }
        d = fminf(fmaxf(d, 0.0f), 1e8f);
        const float dens = expf(-0.5f * d);
        if (dens > best) { best = dens; arg = g; }          // first index on ties (torch.argmax)
    }
    // texture_img[a S + ti, b S + tj] -> transpose -> flip(0): row T-1-(b S + tj), column a S + ti
    const size_t px = (size_t)(T - 1 - (bsq * S + tj)) * T + (size_t)(a * S + ti);
    const float *dc = sh_dc + 3 * ((size_t)f * G + arg);
#pragma unroll
    for (int c = 0; c < 3; ++c) texture[3 * px + c] = dc[c] * kSHC0 + 0.5f;
}

// ---------------------------------------------------------------------------------------- mesh rasterizer
__global__ __launch_bounds__(kTexThreads) void k_mesh_raster(int B, int F, int H, int W, const float *__restrict__ verts,
                                                             const int32_t *__restrict__ faces, const float *__restrict__ viewmats,
                                                             const float *__restrict__ projmats, unsigned long long *__restrict__ zbuf,
                                                             int32_t *__restrict__ n_big, int32_t *__restrict__ big)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * F) return;
    const int b = idx / F, f = idx - b * F;
    Tri t;
    if (!setup_tri(f, verts, faces, viewmats + 16 * b, projmats + 16 * b, W, H, t)) return;
    const Box r = bbox(t, W, H);
    if (r.x1 < r.x0) return;
    if ((int64_t)(r.x1 - r.x0 + 1) * (r.y1 - r.y0 + 1) > kBigFacePixels) {
        big[atomicAdd(n_big, 1)] = idx;                      // capacity B * F: never overflows
        return;
    }
    unsigned long long *zb = zbuf + (size_t)b * H * W;
    for (int y = r.y0; y <= r.y1; ++y)
        for (int x = r.x0; x <= r.x1; ++x) {
            double w[3], bc[3];
            if (cover(t, x, y, w)) zbuf_min(zb + (size_t)y * W + x, persp(t, w, bc), f);
        }
}

__global__ __launch_bounds__(kTexThreads) void k_mesh_sweep(int F, int H, int W, const float *__restrict__ verts,
                                                            const int32_t *__restrict__ faces, const float *__restrict__ viewmats,
                                                            const float *__restrict__ projmats, unsigned long long *__restrict__ zbuf,
                                                            const int32_t *__restrict__ n_big, const int32_t *__restrict__ big)
{
    const int n = *n_big;
    const int tiles_x = (W + kSweepTile - 1) / kSweepTile;
    const int tx0 = (blockIdx.x % tiles_x) * kSweepTile, ty0 = (blockIdx.x / tiles_x) * kSweepTile;
    for (int e = blockIdx.y; e < n; e += gridDim.y) {
        const int idx = big[e], b = idx / F, f = idx - b * F;
        Tri t;
        setup_tri(f, verts, faces, viewmats + 16 * b, projmats + 16 * b, W, H, t);     // (true: it was listed)
        const Box r = bbox(t, W, H);
        const int x0 = max(r.x0, tx0), x1 = min(r.x1, tx0 + kSweepTile - 1);
        const int y0 = max(r.y0, ty0), y1 = min(r.y1, ty0 + kSweepTile - 1);
        if (x1 < x0 || y1 < y0) continue;                    // uniform across the workgroup
        unsigned long long *zb = zbuf + (size_t)b * H * W;
        for (int i = threadIdx.x; i < kSweepTile * kSweepTile; i += blockDim.x) {
            const int x = tx0 + (i % kSweepTile), y = ty0 + (i / kSweepTile);
            double w[3], bc[3];
            if (x >= x0 && x <= x1 && y >= y0 && y <= y1 && cover(t, x, y, w)) zbuf_min(zb + (size_t)y * W + x, persp(t, w, bc), f);
        }
    }
}

// nearest texel of grid_sample(align_corners=True, padding_mode="border") at normalised coordinate c in [0, 1]
__device__ __forceinline__ int nearest_texel(float c, int T)
{
    const float g = c * 2.0f - 1.0f;
    const float x = fminf(fmaxf(((g + 1.0f) / 2.0f) * (float)(T - 1), 0.0f), (float)(T - 1));
    return (int)rintf(x);
}

__global__ __launch_bounds__(kTexThreads) void k_mesh_resolve(int B, int F, int H, int W, const float *__restrict__ verts,
                                                              const int32_t *__restrict__ faces, const float *__restrict__ viewmats,
                                                              const float *__restrict__ projmats, const float *__restrict__ verts_uv,
                                                              const int32_t *__restrict__ faces_uv, int T,
                                                              const unsigned long long *__restrict__ zbuf, int32_t *__restrict__ texel,
                                                              int32_t *__restrict__ face_out, float *__restrict__ bary_out)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * H * W) return;
    const int b = idx / (H * W), pix = idx - b * (H * W);
    const unsigned long long key = zbuf[idx];
    if (key == ~0ull) {
        texel[idx] = -1;
        if (face_out) {
            face_out[idx] = -1;
            bary_out[3 * (size_t)idx] = bary_out[3 * (size_t)idx + 1] = bary_out[3 * (size_t)idx + 2] = 0.0f;
        }
        return;
    }
    const int f = (int)(uint32_t)key;
    Tri t;
    setup_tri(f, verts, faces, viewmats + 16 * b, projmats + 16 * b, W, H, t);
    double w[3], bd[3];
    cover(t, pix % W, pix / W, w);
    persp(t, w, bd);
    const float bc[3] = {(float)bd[0], (float)bd[1], (float)bd[2]};
    // interpolate_face_attributes: sum_k bary_k * uv_k, then TexturesUV's nearest sample with v flipped (the map's rows reversed)
    float uv[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float *u0 = verts_uv + 2 * (size_t)faces_uv[3 * (size_t)f], *u1 = verts_uv + 2 * (size_t)faces_uv[3 * (size_t)f + 1],
                    *u2 = verts_uv + 2 * (size_t)faces_uv[3 * (size_t)f + 2];
        uv[c] = (bc[0] * u0[c] + bc[1] * u1[c]) + bc[2] * u2[c];
    }
    const int col = nearest_texel(uv[0], T), row = T - 1 - nearest_texel(uv[1], T);
    texel[idx] = row * T + col;
    if (face_out) {
        face_out[idx] = f;
#pragma unroll
        for (int c = 0; c < 3; ++c) bary_out[3 * (size_t)idx + c] = bc[c];
    }
}

// ---------------------------------------------------------------------------------------- accumulation
__device__ __forceinline__ unsigned long long claim_key(uint32_t epoch, int p)
{
    return ((unsigned long long)epoch << 32) | (unsigned long long)(~(uint32_t)p);
}

// a texel index outside [0, n_texels) is an uncovered pixel (-1 from k_mesh_resolve)
__global__ __launch_bounds__(kTexThreads) void k_tex_claim(int n, const int32_t *__restrict__ texel, int n_texels, uint32_t epoch,
                                                           unsigned long long *__restrict__ claim)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int t = texel[p];
    if (t >= 0 && t < n_texels) atomicMax(claim + t, claim_key(epoch, p));
}

__global__ __launch_bounds__(kTexThreads) void k_tex_accumulate(int n, const int32_t *__restrict__ texel, int n_texels, const float *__restrict__ rgb,
                                                                int64_t stride, uint32_t epoch, const unsigned long long *__restrict__ claim,
                                                                float *__restrict__ sum, float *__restrict__ count)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int t = texel[p];
    if (t < 0 || t >= n_texels || claim[t] != claim_key(epoch, p)) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) sum[3 * (size_t)t + c] = sum[3 * (size_t)t + c] + rgb[c * stride + p];
    count[t] = count[t] + 1.0f;
}

struct RasterLayout {
    size_t zbuf, n_big, big, total;
};

static RasterLayout raster_layout(int32_t B, int32_t H, int32_t W, int32_t F)
{
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    RasterLayout L;
    L.zbuf = 0;
    L.n_big = up((size_t)B * H * W * 8);
    L.big = L.n_big + 256;
    L.total = up(L.big + (size_t)B * F * 4);
    return L;
}

}  // namespace dm4d

using namespace dm4d;

extern "C" {

int32_t dm4d_tex_atlas_size(int32_t F, int32_t square_size)
{
    if (F < 1 || square_size < 4) return DM4D_ERR_INVALID;
    const int n_axis = (int)(sqrt((double)(F / 2 + 1)) + 1.0);
    return square_size * n_axis;
}

int dm4d_tex_atlas_init(int32_t F, int32_t G, int32_t square_size, const float *verts, const int32_t *faces, const float *means,
                        const float *rotations, const float *scales, const float *sh_dc, float *texture, dm4d_stream_t stream)
{
    if (F < 1 || G < 1 || square_size < 4 || !verts || !faces || !means || !rotations || !scales || !sh_dc || !texture) {
        set_error("dm4d_tex_atlas_init: bad arguments (F %d, G %d, square_size %d: F, G >= 1, square_size >= 4)", F, G, square_size);
        return DM4D_ERR_INVALID;
    }
    const int64_t n = (int64_t)F * (square_size * (square_size - 1) / 2);
    if (n >= (int64_t)1 << 31) { set_error("dm4d_tex_atlas_init: %lld texels exceed the 32-bit launch", (long long)n); return DM4D_ERR_INVALID; }
    const int T = dm4d_tex_atlas_size(F, square_size);
    hipLaunchKernelGGL(k_tex_atlas_init, dim3((unsigned)((n + kTexThreads - 1) / kTexThreads)), dim3(kTexThreads), 0, (hipStream_t)stream,
                       F, G, square_size, T / square_size, T, verts, faces, means, rotations, scales, sh_dc, texture);
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

size_t dm4d_mesh_raster_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t F)
{
    if (B < 0 || H < 0 || W < 0 || F < 0) return 0;
    return raster_layout(B, H, W, F).total;
}

int dm4d_mesh_raster(int32_t B, int32_t H, int32_t W, int32_t F, const float *verts, const int32_t *faces, const float *viewmatrix,
                     const float *projmatrix, const float *verts_uv, const int32_t *faces_uv, int32_t texture_size, void *scratch,
                     size_t scratch_bytes, int32_t *texel, int32_t *face_out, float *bary_out, dm4d_stream_t stream)
{
    if (B < 1 || H < 1 || W < 1 || F < 1 || texture_size < 1 || !verts || !faces || !viewmatrix || !projmatrix || !verts_uv || !faces_uv ||
        !texel || (face_out == nullptr) != (bary_out == nullptr)) {
        set_error("dm4d_mesh_raster: bad arguments (B %d, H %d, W %d, F %d, texture_size %d)", B, H, W, F, texture_size);
        return DM4D_ERR_INVALID;
    }
    if ((int64_t)B * H * W >= (int64_t)1 << 31 || (int64_t)B * F >= (int64_t)1 << 31) {
        set_error("dm4d_mesh_raster: B * H * W or B * F exceeds the 32-bit launch");
        return DM4D_ERR_INVALID;
    }
    const RasterLayout L = raster_layout(B, H, W, F);
    if (!scratch || scratch_bytes < L.total) {
        set_error("dm4d_mesh_raster: scratch too small: %zu < %zu bytes", scratch_bytes, L.total);
        return DM4D_ERR_CAPACITY;
    }
    hipStream_t st = (hipStream_t)stream;
    char *s = (char *)scratch;
    unsigned long long *zbuf = (unsigned long long *)(s + L.zbuf);
    int32_t *n_big = (int32_t *)(s + L.n_big), *big = (int32_t *)(s + L.big);
    DM4D_HIP_CHECK(hipMemsetAsync(zbuf, 0xFF, (size_t)B * H * W * 8, st));
    DM4D_HIP_CHECK(hipMemsetAsync(n_big, 0, 4, st));
    const int64_t nf = (int64_t)B * F, np = (int64_t)B * H * W;
    hipLaunchKernelGGL(k_mesh_raster, dim3((unsigned)((nf + kTexThreads - 1) / kTexThreads)), dim3(kTexThreads), 0, st, B, F, H, W, verts,
                       faces, viewmatrix, projmatrix, zbuf, n_big, big);
    const int tiles = ((W + kSweepTile - 1) / kSweepTile) * ((H + kSweepTile - 1) / kSweepTile);
    hipLaunchKernelGGL(k_mesh_sweep, dim3(tiles, kSweepRows), dim3(kTexThreads), 0, st, F, H, W, verts, faces, viewmatrix, projmatrix,
                       zbuf, n_big, big);
    hipLaunchKernelGGL(k_mesh_resolve, dim3((unsigned)((np + kTexThreads - 1) / kTexThreads)), dim3(kTexThreads), 0, st, B, F, H, W,
                       verts, faces, viewmatrix, projmatrix, verts_uv, faces_uv, texture_size, zbuf, texel, face_out, bary_out);
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

size_t dm4d_tex_claim_bytes(int32_t n_texels)
{
    return n_texels < 0 ? 0 : (size_t)n_texels * 8;
}

int dm4d_tex_accumulate(int32_t n_pixels, const int32_t *texel, const float *rgb, int64_t channel_stride, uint32_t epoch, void *claim,
                        size_t claim_bytes, int32_t n_texels, float *sum, float *count, dm4d_stream_t stream)
{
    if (n_pixels < 0 || n_texels < 0 || epoch == 0 || (n_pixels > 0 && (!texel || !rgb || !claim || !sum || !count))) {
        set_error("dm4d_tex_accumulate: bad arguments (n_pixels %d, n_texels %d, epoch %u: epoch >= 1)", n_pixels, n_texels, epoch);
        return DM4D_ERR_INVALID;
    }
    if (claim_bytes < dm4d_tex_claim_bytes(n_texels)) {
        set_error("dm4d_tex_accumulate: claim words too small: %zu < %zu bytes", claim_bytes, dm4d_tex_claim_bytes(n_texels));
        return DM4D_ERR_CAPACITY;
    }
    if (n_pixels == 0) return DM4D_OK;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((n_pixels + kTexThreads - 1) / kTexThreads));
    unsigned long long *cw = (unsigned long long *)claim;
    hipLaunchKernelGGL(k_tex_claim, grid, dim3(kTexThreads), 0, st, n_pixels, texel, n_texels, epoch, cw);
    hipLaunchKernelGGL(k_tex_accumulate, grid, dim3(kTexThreads), 0, st, n_pixels, texel, n_texels, rgb, channel_stride, epoch, cw, sum, count);
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

}  // extern "C"
