/*
 * dm4d_sugar_reg.h -- C ABI of the SuGaR density and normal regularisation of free Gaussians in libdm4d_hip.so
 * (csrc/sugar_reg.hip).  Same conventions as dm4d_density.h: plain pointers and sizes, every pointer marked [dev] is a DEVICE
 * pointer owned by the caller, every call is enqueued on the caller's hipStream_t, no call allocates device memory (scratch is
 * sized by dm4d_sr_scratch_bytes), return >= 0 success / < 0 one of the DM4D_ERR_* codes of dm4d.h with dm4d_last_error()
 * describing it.  Every argument check that needs no device data is made on the host before anything is launched, and N == 0 or
 * S == 0 is a success that launches nothing.
 *
 * Replaces SuGaRRegularizer.coarse_density_regulation (C/utils/sugar_utils.py:476-759 with get_field_values :278-353,
 * get_covariance :256-262, get_smallest_axis :355-372, get_beta :420-423 and the sample point of :226-228): per-sample gathers of
 * the K tracked neighbours as [S,K,3], [S,K,3,3] and [S,K] tensors, batched products over them and their autograd.  The semantics
 * are stated in DESIGN.md, "SuGaR density and normal regularisation"; the caller is dreammesh4d_amd/sugar_reg.py.
 *
 * The CONTENTS of knn_idx, sample_idx, order, seg_ptr, chunk_ptr, rev_ptr and rev_pos are the caller's contract (the host cannot
 * see them): dreammesh4d_amd/sugar_reg.py checks the two index arrays on the device and derives the tables itself.
 *
 * This header has a version of its own so that dm4d.h (and DM4D_ABI_VERSION) stay as they are.
 */
#ifndef DM4D_SUGAR_REG_H
#define DM4D_SUGAR_REG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DM4D_SR_ABI_VERSION 1
#define DM4D_SR_MAX_K 32                /* tracked neighbours per Gaussian, 1 .. 32 */
#define DM4D_SR_MAX_POINTS 33554432     /* 2^25 Gaussians: N * K stays below 2^31 */
#define DM4D_SR_MAX_SAMPLES 536870912   /* 2^29 samples */
#define DM4D_SR_CHUNK 16                /* samples of one Gaussian a group of 16 lanes sums in the backward */
#define DM4D_SR_RECORD_FLOATS 18        /* prepared record of a Gaussian: centre 3, M 9, opacity, m, n 3, argmin axis (int bits) */
#define DM4D_SR_SLOT_FLOATS 17          /* gradient record of a (chunk, neighbour slot): centre 3, M 9, opacity, m, n 3 */
#define DM4D_SR_OWN_FLOATS 13           /* gradient record of a chunk's own Gaussian: xyz 3, scales 3, quaternion 4, n 3 */

int dm4d_sr_version(void);

/* Bytes of scratch dm4d_sr_forward and dm4d_sr_backward need for these sizes (one buffer serves both); < 0: DM4D_ERR_INVALID. */
int64_t dm4d_sr_scratch_bytes(int64_t N, int32_t K, int64_t S);

/* Forward.  For sample i with g = sample_idx[i] and neighbours j_k = knn_idx[g,k] (float32, no contraction, sums over k ascending):
 *   x = xyz_g + q_g (0, sampling_scale * s_g * eps_i) conj(q_g)                    (two raw quaternion products)
 *   M_j[r,c] = R(q_j)[r,c] / max(s_j[c], 1e-8), R = quaternion_to_matrix with two_s = 2 / (q.q)
 *   m_j = min_c s_j[c] (lowest axis on ties), n_j = R(q_j)[:, argmin]
 *   u_k = M_j^T (x - xyz_j);  w_k = density_factor * opac_j * expf(-0.5 * clamp(u_k.u_k, 0, 1e8));  density = sum_k w_k
 *   beta = (sum_k m_j) / K;   sdf = (x - xyz_g).n_g;   density_term = |density - expf(-0.5 * sdf^2 / beta^2)|
 *   with_normal_loss: c_k = n_j * sign(n_j.n_g);  v_k = w_k |(x - xyz_j).c_k| / max(m_j, 1e-6)^2;  v_k /= max(sum_k v_k, 1e-6);
 *                     normal_term = |n_g - sum_k v_k c_k|^2
 * losses[0] = mean(density_term), losses[1] = mean(normal_term) (0 without the normal loss), summed in a fixed order.
 * order[S]: a permutation of 0 .. S-1 that groups the samples by Gaussian (the stable sort of sample_idx); it only decides which
 * lane handles which sample.  normal_term may be NULL without the normal loss. */
int dm4d_sr_forward(int64_t N, int32_t K, int64_t S, const void *xyz /*[dev] N*3 f32*/, const void *scales /*[dev] N*3 f32*/,
                    const void *quats /*[dev] N*4 f32*/, const void *opac /*[dev] N f32*/, const void *knn_idx /*[dev] N*K i32*/,
                    const void *sample_idx /*[dev] S i32*/, const void *order /*[dev] S i32*/, const void *eps /*[dev] S*3 f32*/,
                    float sampling_scale, float density_factor, int32_t with_normal_loss, void *scratch /*[dev]*/,
                    int64_t scratch_bytes, void *density /*[dev] S f32*/, void *beta /*[dev] S f32*/,
                    void *density_term /*[dev] S f32*/, void *normal_term /*[dev] S f32 or NULL*/, void *losses /*[dev] 2 f32*/,
                    void *stream);

/* Backward of the two means; the forward is recomputed, nothing of size S * K is kept between the calls.
 *   upstream[2] (device floats): dL/d losses[0], dL/d losses[1]
 *   seg_ptr[N+1]:   samples order[seg_ptr[g] .. seg_ptr[g+1]) belong to Gaussian g
 *   chunk_ptr[N+1]: exclusive scan of ceil((seg_ptr[g+1] - seg_ptr[g]) / DM4D_SR_CHUNK)
 *   rev_ptr[N+1], rev_pos[N*K]: the reverse of knn_idx -- rev_pos[rev_ptr[j] .. rev_ptr[j+1]) are the flat positions g * K + k
 *   with knn_idx[g,k] == j, ascending.
 * Writes every element of d_xyz, d_scales, d_quats, d_opac (any of them may be NULL: not wanted).  No atomics: a group of
 * DM4D_SR_CHUNK lanes sums the records of its chunk in a fixed lane order, one lane per Gaussian then adds its own chunks and the
 * chunks of every (g,k) that lists it in ascending (g, k, chunk) and chains to the inputs. */
int dm4d_sr_backward(int64_t N, int32_t K, int64_t S, const void *xyz, const void *scales, const void *quats, const void *opac,
                     const void *knn_idx, const void *sample_idx, const void *order, const void *eps, float sampling_scale,
                     float density_factor, int32_t with_normal_loss, const void *upstream /*[dev] 2 f32*/,
                     const void *seg_ptr /*[dev] N+1 i32*/, const void *chunk_ptr /*[dev] N+1 i32*/,
                     const void *rev_ptr /*[dev] N+1 i32*/, const void *rev_pos /*[dev] N*K i32*/, void *scratch /*[dev]*/,
                     int64_t scratch_bytes, void *d_xyz /*[dev] N*3 f32*/, void *d_scales /*[dev] N*3 f32*/,
                     void *d_quats /*[dev] N*4 f32*/, void *d_opac /*[dev] N f32*/, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* DM4D_SUGAR_REG_H */
