// sugar_reg.hip -- SuGaR density and normal regularisation of free Gaussians (gfx950), the kernels behind
// dreammesh4d_amd/sugar_reg.py (C ABI: include/dm4d_sugar_reg.h).
//
// Reference: SuGaRRegularizer.coarse_density_regulation, custom/threestudio-dreammesh4d/utils/sugar_utils.py:476-759, with
// get_field_values (:278-353), get_covariance (:256-262), get_smallest_axis (:355-372), get_beta (:420-423) and the sample point
// of sample_points_in_gaussians (:226-228): per-sample gathers of the K tracked neighbours as [S,K,3], [S,K,3,3] and [S,K]
// tensors, batched products over them, and autograd through all of it.  Here a Gaussian is prepared once into an 18-float
// record, a sample reads the K records of its Gaussian's neighbours, and the backward recomputes the forward.  Semantics:
// DESIGN.md "SuGaR density and normal regularisation".  Nothing below uses an atomic, no kernel waits on another workgroup, and
// every loop has a bound that is fixed when the kernel is launched.
//
//   k_sr_prepare     one lane per Gaussian: centre, M = R / max(s, 1e-8), opacity, m = min s, n = R[:, argmin], argmin
//   k_sr_forward     one lane per sample, in the order that groups samples by Gaussian (neighbouring lanes read the same records)
//   k_sr_partial / k_sr_final   the two means, float64 sums in a fixed order
//   k_sr_backward    a DPP row of 16 lanes owns a chunk of at most 16 samples of ONE Gaussian: a lane recomputes its sample, the
//                    row sums the 17-float gradient record of each neighbour slot and the 13-float record of the own Gaussian
//                    in a fixed lane order, lane 0 writes them
//   k_sr_gather      one lane per Gaussian j: its own chunks, then the chunks of every (g,k) that lists j in ascending
//                    (g, k, chunk) through the reverse table, in float64; then the chain through M, m, n and R to the inputs
#include "common.h"
#include "hostcheck.h"
#include "../../include/dm4d.h"
#include "../../include/dm4d_sugar_reg.h"

namespace dm4d {

constexpr int kSrThreads = 256;
constexpr int kSrRec = DM4D_SR_RECORD_FLOATS;
constexpr int kSrSlot = DM4D_SR_SLOT_FLOATS;
constexpr int kSrOwn = DM4D_SR_OWN_FLOATS;
constexpr int kSrChunk = DM4D_SR_CHUNK;
constexpr int kSrPartials = 1024;                           // workgroups of the first pass of the means
static_assert(kSrChunk == 16, "a chunk is one DPP row");
static_assert((int64_t)DM4D_SR_MAX_POINTS * DM4D_SR_MAX_K <= (int64_t)1 << 31, "flat positions of knn_idx stay below 2^31");

// pytorch3d's quaternion_to_matrix (real part first), two_s = 2 / (q.q)
__device__ __forceinline__ void sr_rotation(const float (&q)[4], float (&R)[9])
{
    const float r = q[0], i = q[1], j = q[2], k = q[3];
    const float two_s = 2.0f / (r * r + i * i + j * j + k * k);
    R[0] = 1.0f - two_s * (j * j + k * k);
    R[1] = two_s * (i * j - k * r);
    R[2] = two_s * (i * k + j * r);
    R[3] = two_s * (i * j + k * r);
    R[4] = 1.0f - two_s * (i * i + k * k);
    R[5] = two_s * (j * k - i * r);
    R[6] = two_s * (i * k - j * r);
    R[7] = two_s * (j * k + i * r);
    R[8] = 1.0f - two_s * (i * i + j * j);
}

// lowest axis on exact ties (torch leaves it open on a GPU)
__device__ __forceinline__ int sr_argmin(const float (&s)[3])
{
    int c = 0;
    if (s[1] < s[c]) c = 1;
    if (s[2] < s[c]) c = 2;
    return c;
}

__device__ __forceinline__ float sr_sign(float v) { return v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : 0.0f); }

__global__ __launch_bounds__(kSrThreads) void k_sr_prepare(const int N, const float *__restrict__ xyz, const float *__restrict__ scales,
                                                          const float *__restrict__ quats, const float *__restrict__ opac,
                                                          float *__restrict__ rec)
{
    const int j = blockIdx.x * kSrThreads + threadIdx.x;
    if (j >= N) return;
    const float q[4] = {quats[4 * j], quats[4 * j + 1], quats[4 * j + 2], quats[4 * j + 3]};
    const float s[3] = {scales[3 * j], scales[3 * j + 1], scales[3 * j + 2]};
    float R[9];
    sr_rotation(q, R);
    float *o = rec + (int64_t)j * kSrRec;
    o[0] = xyz[3 * j]; o[1] = xyz[3 * j + 1]; o[2] = xyz[3 * j + 2];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a = 1.0f / fmaxf(s[c], 1e-8f);
#pragma unroll
        for (int r = 0; r < 3; ++r) o[3 + 3 * r + c] = R[3 * r + c] * a;
    }
    const int cs = sr_argmin(s);
    o[12] = opac[j];
    o[13] = s[cs];
    o[14] = R[cs]; o[15] = R[3 + cs]; o[16] = R[6 + cs];
    o[17] = __int_as_float(cs);
}

// the sample point: v = (sampling_scale * s) * eps, p = q (0,v) conj(q) as two raw quaternion products, x = xyz + p
__device__ __forceinline__ void sr_sample_point(const float (&q)[4], const float (&s)[3], const float (&e)[3], const float ss,
                                                const float (&c)[3], float (&v)[3], float (&x)[3])
{
#pragma unroll
    for (int a = 0; a < 3; ++a) v[a] = (ss * s[a]) * e[a];
    const float aw = q[0] * 0.0f - q[1] * v[0] - q[2] * v[1] - q[3] * v[2];
    const float ax = q[0] * v[0] + q[1] * 0.0f + q[2] * v[2] - q[3] * v[1];
    const float ay = q[0] * v[1] - q[1] * v[2] + q[2] * 0.0f + q[3] * v[0];
    const float az = q[0] * v[2] + q[1] * v[1] - q[2] * v[0] + q[3] * 0.0f;
    const float bw = q[0], bx = -q[1], by = -q[2], bz = -q[3];
    const float px = aw * bx + ax * bw + ay * bz - az * by;
    const float py = aw * by - ax * bz + ay * bw + az * bx;
    const float pz = aw * bz + ax * by - ay * bx + az * bw;
    x[0] = c[0] + px; x[1] = c[1] + py; x[2] = c[2] + pz;
}

// what a sample reads of neighbour record r: shift, warped shift, its squared length, expf(-0.5 clamp), the opacity term
struct SrNeighbour {
    float sh[3], u[3], uu, e, w;
};

__device__ __forceinline__ void sr_neighbour(const float *__restrict__ r, const float (&x)[3], const float df, SrNeighbour &o)
{
#pragma unroll
    for (int a = 0; a < 3; ++a) o.sh[a] = x[a] - r[a];
#pragma unroll
    for (int c = 0; c < 3; ++c) o.u[c] = r[3 + c] * o.sh[0] + r[6 + c] * o.sh[1] + r[9 + c] * o.sh[2];
    o.uu = o.u[0] * o.u[0] + o.u[1] * o.u[1] + o.u[2] * o.u[2];
    const float m2 = fminf(fmaxf(o.uu, 0.0f), 1e8f);
    o.e = expf(-0.5f * m2);
    o.w = df * r[12] * o.e;
}

// the normal term's weight of a neighbour before its normalisation, and the sign that aligns its normal with n_g
__device__ __forceinline__ float sr_normal_weight(const float *__restrict__ r, const SrNeighbour &nb, const float (&ng)[3], float &sg)
{
    sg = sr_sign(r[14] * ng[0] + r[15] * ng[1] + r[16] * ng[2]);
    const float a = fabsf(nb.sh[0] * (r[14] * sg) + nb.sh[1] * (r[15] * sg) + nb.sh[2] * (r[16] * sg));
    const float mm = fmaxf(r[13], 1e-6f);
    return nb.w * a / (mm * mm);
}

// Everything of one sample that both directions need.
struct SrSample {
    float x[3], v[3], d[3], ng[3], sdf, density, beta, target, V, r[3];
};

__device__ __forceinline__ void sr_eval_sample(const int g, const int i, const int K, const float *__restrict__ xyz,
                                               const float *__restrict__ scales, const float *__restrict__ quats,
                                               const int32_t *__restrict__ knn, const float *__restrict__ eps, const float ss,
                                               const float df, const bool normal, const float *__restrict__ rec, SrSample &o)
{
    const float q[4] = {quats[4 * (int64_t)g], quats[4 * (int64_t)g + 1], quats[4 * (int64_t)g + 2], quats[4 * (int64_t)g + 3]};
    const float s[3] = {scales[3 * (int64_t)g], scales[3 * (int64_t)g + 1], scales[3 * (int64_t)g + 2]};
    const float c[3] = {xyz[3 * (int64_t)g], xyz[3 * (int64_t)g + 1], xyz[3 * (int64_t)g + 2]};
    const float e[3] = {eps[3 * (int64_t)i], eps[3 * (int64_t)i + 1], eps[3 * (int64_t)i + 2]};
    sr_sample_point(q, s, e, ss, c, o.v, o.x);
    const float *rg = rec + (int64_t)g * kSrRec;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        o.ng[a] = rg[14 + a];
        o.d[a] = o.x[a] - c[a];
    }
    o.sdf = o.d[0] * o.ng[0] + o.d[1] * o.ng[1] + o.d[2] * o.ng[2];
    float dens = 0.0f, msum = 0.0f, V = 0.0f;
    const int32_t *row = knn + (int64_t)g * K;
    for (int k = 0; k < K; ++k) {
        const float *r = rec + (int64_t)row[k] * kSrRec;
        SrNeighbour nb;
        sr_neighbour(r, o.x, df, nb);
        dens += nb.w;
        msum += r[13];
        if (normal) {
            float sg;
            V += sr_normal_weight(r, nb, o.ng, sg);
        }
    }
    o.density = dens;
    o.beta = msum / (float)K;
    o.target = expf(-0.5f * (o.sdf * o.sdf) / (o.beta * o.beta));
    o.V = V;
    o.r[0] = o.r[1] = o.r[2] = 0.0f;
    if (normal) {
        const float Vc = fmaxf(V, 1e-6f);
        float acc[3] = {0.0f, 0.0f, 0.0f};
        for (int k = 0; k < K; ++k) {
            const float *r = rec + (int64_t)row[k] * kSrRec;
            SrNeighbour nb;
            sr_neighbour(r, o.x, df, nb);
            float sg;
            const float vn = sr_normal_weight(r, nb, o.ng, sg) / Vc;
#pragma unroll
            for (int a = 0; a < 3; ++a) acc[a] += vn * (r[14 + a] * sg);
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) o.r[a] = o.ng[a] - acc[a];
    }
}

__global__ __launch_bounds__(kSrThreads) void k_sr_forward(const int K, const int S, const float *__restrict__ xyz,
                                                          const float *__restrict__ scales, const float *__restrict__ quats,
                                                          const int32_t *__restrict__ knn, const int32_t *__restrict__ sample_idx,
                                                          const int32_t *__restrict__ order, const float *__restrict__ eps,
                                                          const float ss, const float df, const int normal,
                                                          const float *__restrict__ rec, float *__restrict__ density,
                                                          float *__restrict__ beta, float *__restrict__ dterm, float *__restrict__ nterm)
{
    const int t = blockIdx.x * kSrThreads + threadIdx.x;
    if (t >= S) return;
    const int i = order[t];
    SrSample sm;
    sr_eval_sample(sample_idx[i], i, K, xyz, scales, quats, knn, eps, ss, df, normal != 0, rec, sm);
    density[i] = sm.density;
    beta[i] = sm.beta;
    dterm[i] = fabsf(sm.density - sm.target);
    if (nterm) nterm[i] = normal ? sm.r[0] * sm.r[0] + sm.r[1] * sm.r[1] + sm.r[2] * sm.r[2] : 0.0f;
}

// sum of a workgroup's values, valid in thread 0; a fixed tree
__device__ __forceinline__ double sr_block_sum(double v, double *sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int w = kSrThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    const double out = sh[0];
    __syncthreads();
    return out;
}

// partial[b], partial[kSrPartials + b]: the sums of workgroup b's contiguous range of the two term arrays (b may be NULL)
__global__ __launch_bounds__(kSrThreads) void k_sr_partial(const int S, const int per_block, const float *__restrict__ a,
                                                          const float *__restrict__ b, double *__restrict__ partial)
{
    __shared__ double sh[kSrThreads];
    const int64_t first = (int64_t)blockIdx.x * per_block;
    const int64_t last = first + per_block < S ? first + per_block : S;
    double sa = 0.0, sb = 0.0;
    for (int64_t i = first + threadIdx.x; i < last; i += kSrThreads) {
        sa += (double)a[i];
        if (b) sb += (double)b[i];
    }
    sa = sr_block_sum(sa, sh);
    sb = sr_block_sum(sb, sh);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = sa;
        partial[kSrPartials + blockIdx.x] = sb;
    }
}

__global__ __launch_bounds__(kSrThreads) void k_sr_final(const int S, const int blocks, const double *__restrict__ partial,
                                                        float *__restrict__ losses)
{
    __shared__ double sh[kSrThreads];
    double sa = 0.0, sb = 0.0;
    for (int i = threadIdx.x; i < blocks; i += kSrThreads) {
        sa += partial[i];
        sb += partial[kSrPartials + i];
    }
    sa = sr_block_sum(sa, sh);
    sb = sr_block_sum(sb, sh);
    if (threadIdx.x == 0) {
        losses[0] = (float)(sa / (double)S);
        losses[1] = (float)(sb / (double)S);
    }
}

// sum over the 16 lanes of a DPP row, in every lane of the row, in a fixed order
__device__ __forceinline__ float sr_row_sum(float v)
{
    v = dpp_add<0xB1>(v);        // quad_perm [1,0,3,2]
    v = dpp_add<0x4E>(v);        // quad_perm [2,3,0,1]
    v = dpp_add<0x141>(v);       // row_half_mirror
    v = dpp_add<0x140>(v);       // row_mirror
    return v;
}

__global__ __launch_bounds__(kSrThreads) void k_sr_backward(const int N, const int K, const int S, const float *__restrict__ xyz,
                                                           const float *__restrict__ scales, const float *__restrict__ quats,
                                                           const int32_t *__restrict__ knn, const int32_t *__restrict__ sample_idx,
                                                           const int32_t *__restrict__ order, const float *__restrict__ eps,
                                                           const float ss, const float df, const int normal,
                                                           const float *__restrict__ upstream, const int32_t *__restrict__ seg_ptr,
                                                           const int32_t *__restrict__ chunk_ptr, const float *__restrict__ rec,
                                                           float *__restrict__ slot, float *__restrict__ own)
{
    const int chunk = blockIdx.x * (kSrThreads / kSrChunk) + (int)threadIdx.x / kSrChunk;
    const int lane = (int)threadIdx.x % kSrChunk;
    if (chunk >= chunk_ptr[N]) return;                       // the whole row leaves together
    // the Gaussian g with chunk_ptr[g] <= chunk < chunk_ptr[g + 1]
    int lo = 0, hi = N;                                      // first index in (0, N] whose chunk_ptr exceeds `chunk`
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (chunk_ptr[mid] <= chunk) lo = mid; else hi = mid;
    }
    const int g = lo;
    const int first = seg_ptr[g] + (chunk - chunk_ptr[g]) * kSrChunk;
    const bool valid = first + lane < seg_ptr[g + 1];
    const int i = order[valid ? first + lane : first];       // a lane past the segment's end recomputes its first sample, weight 0
    SrSample sm;
    sr_eval_sample(g, i, K, xyz, scales, quats, knn, eps, ss, df, normal != 0, rec, sm);
    const float gd = valid ? upstream[0] / (float)S : 0.0f;
    const float gn = valid && normal ? upstream[1] / (float)S : 0.0f;
    const float sD = gd * sr_sign(sm.density - sm.target);  // d |.|: sign, 0 at equality
    const float bb = sm.beta * sm.beta;
    const float dsdf = -sD * sm.target * (-sm.sdf / bb);
    const float dm = (-sD * sm.target * (sm.sdf * sm.sdf / (bb * sm.beta))) / (float)K;
    const float Vc = fmaxf(sm.V, 1e-6f);
    float dr[3], dx[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int a = 0; a < 3; ++a) dr[a] = 2.0f * sm.r[a] * gn;
    const int32_t *row = knn + (int64_t)g * K;
    for (int k = 0; k < K; ++k) {
        const float *r = rec + (int64_t)row[k] * kSrRec;
        SrNeighbour nb;
        sr_neighbour(r, sm.x, df, nb);
        float out[kSrSlot];
        const float dm2 = (nb.uu >= 0.0f && nb.uu <= 1e8f) ? sD * nb.w * -0.5f : 0.0f;
        const float du[3] = {2.0f * nb.u[0] * dm2, 2.0f * nb.u[1] * dm2, 2.0f * nb.u[2] * dm2};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float dsh = r[3 + 3 * a] * du[0] + r[4 + 3 * a] * du[1] + r[5 + 3 * a] * du[2];
            dx[a] += dsh;
            out[a] = -dsh;
#pragma unroll
            for (int c = 0; c < 3; ++c) out[3 + 3 * a + c] = nb.sh[a] * du[c];
        }
        out[12] = sD * df * nb.e;
        out[13] = dm;
        out[14] = out[15] = out[16] = 0.0f;
        if (normal) {
            float sg;
            const float vn = sr_normal_weight(r, nb, sm.ng, sg) / Vc;
#pragma unroll
            for (int a = 0; a < 3; ++a) out[14 + a] = -(vn * sg) * dr[a];
        }
        float *o = slot + ((int64_t)chunk * K + k) * kSrSlot;
#pragma unroll
        for (int a = 0; a < kSrSlot; ++a) {
            const float total = sr_row_sum(out[a]);
            if (lane == 0) o[a] = total;
        }
    }
    // the own Gaussian: x = xyz_g + p(q_g, v), sdf = p . n_g (the two xyz_g of x - xyz_g cancel), v = (ss * s_g) * eps
    const float q[4] = {quats[4 * (int64_t)g], quats[4 * (int64_t)g + 1], quats[4 * (int64_t)g + 2], quats[4 * (int64_t)g + 3]};
    const float w = q[0], u[3] = {q[1], q[2], q[3]};
    float dp[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) dp[a] = dx[a] + dsdf * sm.ng[a];
    const float *v = sm.v;
    const float udp = u[0] * dp[0] + u[1] * dp[1] + u[2] * dp[2];
    const float vdp = v[0] * dp[0] + v[1] * dp[1] + v[2] * dp[2];
    const float uv = u[0] * v[0] + u[1] * v[1] + u[2] * v[2];
    const float uxdp[3] = {u[1] * dp[2] - u[2] * dp[1], u[2] * dp[0] - u[0] * dp[2], u[0] * dp[1] - u[1] * dp[0]};
    const float uxv[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
    const float vxdp[3] = {v[1] * dp[2] - v[2] * dp[1], v[2] * dp[0] - v[0] * dp[2], v[0] * dp[1] - v[1] * dp[0]};
    const float ww_uu = w * w - (u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    float out[kSrOwn];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float dv = ww_uu * dp[a] + 2.0f * udp * u[a] - 2.0f * w * uxdp[a];
        out[a] = dx[a];
        out[3 + a] = dv * (ss * eps[3 * (int64_t)i + a]);
        out[7 + a] = -2.0f * vdp * u[a] + 2.0f * uv * dp[a] + 2.0f * udp * v[a] + 2.0f * w * vxdp[a];
        out[10 + a] = dsdf * sm.d[a] + dr[a];
    }
    out[6] = 2.0f * w * vdp + 2.0f * (uxv[0] * dp[0] + uxv[1] * dp[1] + uxv[2] * dp[2]);
    float *o = own + (int64_t)chunk * kSrOwn;
#pragma unroll
    for (int a = 0; a < kSrOwn; ++a) {
        const float total = sr_row_sum(out[a]);
        if (lane == 0) o[a] = total;
    }
}

__global__ __launch_bounds__(kSrThreads) void k_sr_gather(const int N, const int K, const float *__restrict__ scales,
                                                         const float *__restrict__ quats, const int32_t *__restrict__ chunk_ptr,
                                                         const int32_t *__restrict__ rev_ptr, const int32_t *__restrict__ rev_pos,
                                                         const float *__restrict__ slot, const float *__restrict__ own,
                                                         float *__restrict__ d_xyz, float *__restrict__ d_scales,
                                                         float *__restrict__ d_quats, float *__restrict__ d_opac)
{
    const int j = blockIdx.x * kSrThreads + threadIdx.x;
    if (j >= N) return;
    double so[kSrOwn], sn[kSrSlot];
#pragma unroll
    for (int a = 0; a < kSrOwn; ++a) so[a] = 0.0;
#pragma unroll
    for (int a = 0; a < kSrSlot; ++a) sn[a] = 0.0;
    for (int c = chunk_ptr[j]; c < chunk_ptr[j + 1]; ++c) {
        const float *o = own + (int64_t)c * kSrOwn;
#pragma unroll
        for (int a = 0; a < kSrOwn; ++a) so[a] += (double)o[a];
    }
    for (int e = rev_ptr[j]; e < rev_ptr[j + 1]; ++e) {
        const int pos = rev_pos[e], g = pos / K, k = pos - g * K;
        for (int c = chunk_ptr[g]; c < chunk_ptr[g + 1]; ++c) {
            const float *o = slot + ((int64_t)c * K + k) * kSrSlot;
#pragma unroll
            for (int a = 0; a < kSrSlot; ++a) sn[a] += (double)o[a];
        }
    }
    const float q[4] = {quats[4 * (int64_t)j], quats[4 * (int64_t)j + 1], quats[4 * (int64_t)j + 2], quats[4 * (int64_t)j + 3]};
    const float s[3] = {scales[3 * (int64_t)j], scales[3 * (int64_t)j + 1], scales[3 * (int64_t)j + 2]};
    float R[9], dR[9], ds[3];
    sr_rotation(q, R);
    const int cs = sr_argmin(s);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a = 1.0f / fmaxf(s[c], 1e-8f);
        float da = 0.0f;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float dM = (float)sn[3 + 3 * r + c];
            dR[3 * r + c] = dM * a;
            da += dM * R[3 * r + c];
        }
        ds[c] = (float)so[3 + c] + (s[c] >= 1e-8f ? -da * a * a : 0.0f);   // the clamp passes nothing below its bound
    }
    ds[cs] += (float)sn[13];                                 // min's backward: the chosen axis only
#pragma unroll
    for (int r = 0; r < 3; ++r) dR[3 * r + cs] += (float)(sn[14 + r] + so[10 + r]);
    if (d_xyz) {
#pragma unroll
        for (int a = 0; a < 3; ++a) d_xyz[3 * (int64_t)j + a] = (float)(so[a] + sn[a]);
    }
    if (d_scales) {
#pragma unroll
        for (int a = 0; a < 3; ++a) d_scales[3 * (int64_t)j + a] = ds[a];
    }
    if (d_opac) d_opac[j] = (float)sn[12];
    if (d_quats) {
        // R = I + two_s B(q), two_s = 2 / (q.q)
        const float r = q[0], i = q[1], jj = q[2], k = q[3];
        const float qq = r * r + i * i + jj * jj + k * k;
        const float T = 2.0f / qq;
        const float dT = dR[0] * -(jj * jj + k * k) + dR[1] * (i * jj - k * r) + dR[2] * (i * k + jj * r) + dR[3] * (i * jj + k * r) +
                         dR[4] * -(i * i + k * k) + dR[5] * (jj * k - i * r) + dR[6] * (i * k - jj * r) + dR[7] * (jj * k + i * r) +
                         dR[8] * -(i * i + jj * jj);
        const float dqq = -2.0f / (qq * qq) * dT;
        float dq[4];
        dq[0] = T * (-k * dR[1] + jj * dR[2] + k * dR[3] - i * dR[5] - jj * dR[6] + i * dR[7]);
        dq[1] = T * (-2.0f * i * dR[4] - 2.0f * i * dR[8] + jj * dR[1] + k * dR[2] + jj * dR[3] - r * dR[5] + k * dR[6] + r * dR[7]);
        dq[2] = T * (-2.0f * jj * dR[0] - 2.0f * jj * dR[8] + i * dR[1] + r * dR[2] + i * dR[3] + k * dR[5] - r * dR[6] + k * dR[7]);
        dq[3] = T * (-2.0f * k * dR[0] - 2.0f * k * dR[4] - r * dR[1] + i * dR[2] + r * dR[3] + jj * dR[5] + i * dR[6] + jj * dR[7]);
#pragma unroll
        for (int a = 0; a < 4; ++a) d_quats[4 * (int64_t)j + a] = (float)so[6 + a] + dq[a] + 2.0f * q[a] * dqq;
    }
}

// ------------------------------------------------------------------------------------------------ host side
struct SrLayout {
    int64_t chunks, rec, partial, slot, own, bytes;           // offsets in bytes, every section 256-byte aligned
};

static int64_t sr_round(int64_t v) { return (v + 255) & ~(int64_t)255; }

static SrLayout sr_layout(int64_t N, int32_t K, int64_t S)
{
    SrLayout L;
    L.chunks = (S + kSrChunk - 1) / kSrChunk + (N < S ? N : S);   // sum_g ceil(count_g / 16) never exceeds this
    L.rec = 0;
    L.partial = sr_round(L.rec + N * kSrRec * 4);
    L.slot = sr_round(L.partial + 2 * kSrPartials * 8);
    L.own = sr_round(L.slot + L.chunks * K * kSrSlot * 4);
    L.bytes = sr_round(L.own + L.chunks * kSrOwn * 4);
    return L;
}

static bool sr_bad_sizes(const char *fn, int64_t N, int32_t K, int64_t S)
{
    if (bad_count(fn, "N", N, DM4D_SR_MAX_POINTS)) return true;
    if (K < 1 || K > DM4D_SR_MAX_K) { set_error("%s: K = %d is outside [1, %d]", fn, K, DM4D_SR_MAX_K); return true; }
    return bad_count(fn, "S", S, DM4D_SR_MAX_SAMPLES);
}

static bool sr_bad_scalars(const char *fn, float sampling_scale, float density_factor, int32_t with_normal_loss)
{
    if (!(fabsf(sampling_scale) <= 3.0e38f)) { set_error("%s: sampling_scale = %g is not finite", fn, (double)sampling_scale); return true; }
    if (!(fabsf(density_factor) <= 3.0e38f)) { set_error("%s: density_factor = %g is not finite", fn, (double)density_factor); return true; }
    if (with_normal_loss != 0 && with_normal_loss != 1) { set_error("%s: with_normal_loss = %d must be 0 or 1", fn, with_normal_loss); return true; }
    return false;
}

static bool sr_bad_scratch(const char *fn, const void *scratch)
{
    if (!scratch) { set_error("%s: null argument", fn); return true; }
    if (misaligned(scratch, 16)) { set_error("%s: scratch must be 16-byte aligned", fn); return true; }
    return false;
}

}  // namespace dm4d

using namespace dm4d;

extern "C" {

int dm4d_sr_version(void) { return DM4D_SR_ABI_VERSION; }

int64_t dm4d_sr_scratch_bytes(int64_t N, int32_t K, int64_t S)
{
    if (sr_bad_sizes("dm4d_sr_scratch_bytes", N, K, S)) return DM4D_ERR_INVALID;
    return sr_layout(N, K, S).bytes;
}

int dm4d_sr_forward(int64_t N, int32_t K, int64_t S, const void *xyz, const void *scales, const void *quats, const void *opac,
                    const void *knn_idx, const void *sample_idx, const void *order, const void *eps, float sampling_scale,
                    float density_factor, int32_t with_normal_loss, void *scratch, int64_t scratch_bytes, void *density, void *beta,
                    void *density_term, void *normal_term, void *losses, void *stream)
{
    const char *fn = "dm4d_sr_forward";
    if (sr_bad_sizes(fn, N, K, S) || sr_bad_scalars(fn, sampling_scale, density_factor, with_normal_loss)) return DM4D_ERR_INVALID;
    if (N == 0 || S == 0) return DM4D_OK;
    DM4D_REFUSE_NULL(!xyz || !scales || !quats || !opac || !knn_idx || !sample_idx || !order || !eps || !density || !beta || !density_term || !losses)
    DM4D_REFUSE_NULL(with_normal_loss && !normal_term)
    const SrLayout L = sr_layout(N, K, S);
    if (sr_bad_scratch(fn, scratch)) return DM4D_ERR_INVALID;
    if (short_scratch(fn, scratch_bytes, L.bytes)) return DM4D_ERR_CAPACITY;
    hipStream_t st = (hipStream_t)stream;
    float *rec = reinterpret_cast<float *>((char *)scratch + L.rec);
    double *partial = reinterpret_cast<double *>((char *)scratch + L.partial);
    hipLaunchKernelGGL(k_sr_prepare, dim3(blocks(N, kSrThreads)), dim3(kSrThreads), 0, st, (int)N, (const float *)xyz, (const float *)scales,
                       (const float *)quats, (const float *)opac, rec);
    DM4D_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_sr_forward, dim3(blocks(S, kSrThreads)), dim3(kSrThreads), 0, st, (int)K, (int)S, (const float *)xyz,
                       (const float *)scales, (const float *)quats, (const int32_t *)knn_idx, (const int32_t *)sample_idx,
                       (const int32_t *)order, (const float *)eps, sampling_scale, density_factor, (int)with_normal_loss,
                       (const float *)rec, (float *)density, (float *)beta, (float *)density_term, (float *)normal_term);
    DM4D_HIP_CHECK(hipGetLastError());
    const int64_t want = blocks(S, kSrThreads);
    const int n_partial = (int)(want < kSrPartials ? want : kSrPartials);
    const int per_block = (int)((S + n_partial - 1) / n_partial);
    hipLaunchKernelGGL(k_sr_partial, dim3(n_partial), dim3(kSrThreads), 0, st, (int)S, per_block, (const float *)density_term,
                       with_normal_loss ? (const float *)normal_term : (const float *)nullptr, partial);
    DM4D_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_sr_final, dim3(1), dim3(kSrThreads), 0, st, (int)S, n_partial, (const double *)partial, (float *)losses);
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

int dm4d_sr_backward(int64_t N, int32_t K, int64_t S, const void *xyz, const void *scales, const void *quats, const void *opac,
                     const void *knn_idx, const void *sample_idx, const void *order, const void *eps, float sampling_scale,
                     float density_factor, int32_t with_normal_loss, const void *upstream, const void *seg_ptr, const void *chunk_ptr,
                     const void *rev_ptr, const void *rev_pos, void *scratch, int64_t scratch_bytes, void *d_xyz, void *d_scales,
                     void *d_quats, void *d_opac, void *stream)
{
    const char *fn = "dm4d_sr_backward";
    if (sr_bad_sizes(fn, N, K, S) || sr_bad_scalars(fn, sampling_scale, density_factor, with_normal_loss)) return DM4D_ERR_INVALID;
    if (N == 0 || S == 0) return DM4D_OK;
    DM4D_REFUSE_NULL(!xyz || !scales || !quats || !opac || !knn_idx || !sample_idx || !order || !eps || !upstream || !seg_ptr || !chunk_ptr || !rev_ptr || !rev_pos)
    const SrLayout L = sr_layout(N, K, S);
    if (sr_bad_scratch(fn, scratch)) return DM4D_ERR_INVALID;
    if (short_scratch(fn, scratch_bytes, L.bytes)) return DM4D_ERR_CAPACITY;
    hipStream_t st = (hipStream_t)stream;
    float *rec = reinterpret_cast<float *>((char *)scratch + L.rec);
    float *slot = reinterpret_cast<float *>((char *)scratch + L.slot);
    float *own = reinterpret_cast<float *>((char *)scratch + L.own);
    hipLaunchKernelGGL(k_sr_prepare, dim3(blocks(N, kSrThreads)), dim3(kSrThreads), 0, st, (int)N, (const float *)xyz, (const float *)scales,
                       (const float *)quats, (const float *)opac, rec);
    DM4D_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_sr_backward, dim3(blocks(L.chunks, kSrThreads / kSrChunk)), dim3(kSrThreads), 0, st, (int)N,
                       (int)K, (int)S, (const float *)xyz, (const float *)scales, (const float *)quats, (const int32_t *)knn_idx,
                       (const int32_t *)sample_idx, (const int32_t *)order, (const float *)eps, sampling_scale, density_factor,
                       (int)with_normal_loss, (const float *)upstream, (const int32_t *)seg_ptr, (const int32_t *)chunk_ptr,
                       (const float *)rec, slot, own);
    DM4D_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_sr_gather, dim3(blocks(N, kSrThreads)), dim3(kSrThreads), 0, st, (int)N, (int)K, (const float *)scales,
                       (const float *)quats, (const int32_t *)chunk_ptr, (const int32_t *)rev_ptr, (const int32_t *)rev_pos,
                       (const float *)slot, (const float *)own, (float *)d_xyz, (float *)d_scales, (float *)d_quats, (float *)d_opac);
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

}  // extern "C"
