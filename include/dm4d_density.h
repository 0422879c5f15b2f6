/*
 * dm4d_density.h -- C ABI of the adaptive-density-control entry points of libdm4d_hip.so (csrc/density_control.hip): the
 * densification statistics of free Gaussians, their classification into keep / drop / clone / split, the plan of the output rows
 * and the one row move that applies it to every parameter and Adam moment.  Same conventions as dm4d.h: plain pointers and sizes,
 * every pointer marked [dev] is a DEVICE pointer owned by the caller, every call is enqueued on the caller's hipStream_t, no call
 * allocates device memory, return >= 0 success / < 0 one of the DM4D_ERR_* codes of dm4d.h with dm4d_last_error() describing it.
 * Every argument check that needs no device data is made on the host before anything is launched, and N == 0 (or M == 0) is a
 * success that launches nothing.
 *
 * Replaces the density control of GaussianBaseModel (C/geometry/gaussian_base.py:575-579, 606-870: boolean-mask indexing, repeat,
 * cat and bmm per tensor, and a rebuild of the optimiser state).  The semantics are stated in DESIGN.md, "Adaptive density
 * control"; the callers are dreammesh4d_amd/density_control.py and gaussian_model.py.
 *
 * This header has a version of its own so that dm4d.h (and DM4D_ABI_VERSION) stay as they are.
 */
#ifndef DM4D_DENSITY_H
#define DM4D_DENSITY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DM4D_DC_ABI_VERSION 1
#define DM4D_DC_MAX_ROWS 268435456     /* 2^31 / 8: with 8 children per split every output row index stays below 2^31 */
#define DM4D_DC_MAX_CHILDREN 8         /* S, the children per split source, lies in 1 .. 8 */
#define DM4D_DC_MAX_ARRAYS 24          /* arrays of one dm4d_dc_move call */
#define DM4D_DC_MAX_VIEWS 4096

/* kind[i] & 3.  A caller's boolean mask is a valid kind as it stands (true = DROP). */
#define DM4D_DC_KEEP 0
#define DM4D_DC_DROP 1
#define DM4D_DC_CLONE 2                /* the source stays AND one copy is appended */
#define DM4D_DC_SPLIT 3                /* the source goes, S children are appended */

/* role[j] of an output row: the kept original, the clone, or child k = role - DM4D_DC_ROLE_CHILD of its source */
#define DM4D_DC_ROLE_KEPT 0
#define DM4D_DC_ROLE_CLONE 1
#define DM4D_DC_ROLE_CHILD 2

/* flags of an array of the move */
#define DM4D_DC_ZERO_NEW 1             /* every row that is not a kept original is written as zeros (the Adam moments) */
#define DM4D_DC_SKIP_CHILDREN 2        /* child rows are not written: dm4d_dc_split_children computes them (xyz, _scaling) */

int dm4d_dc_version(void);

/* Densification statistics of one step, all B views in one launch (add_densification_stats and the max_radii2D update,
 * gaussian_base.py:816-820, 846-852).  One thread owns a Gaussian: for b ascending, when radii[b,i] > 0:
 *   accum[i] += sqrtf(gx * gx + gy * gy) (float32, no contraction; gx, gy = grad2d[b,i,0..1]);  denom[i] += 1;
 * and for every view, visible or not, max_radii[i] = max(max_radii[i], (float)radii[b,i]).  No atomics. */
int dm4d_dc_accumulate_stats(int32_t B, int64_t N, const void *grad2d /*[dev] B*N*3 f32*/, const void *radii /*[dev] B*N i32*/,
                             void *accum /*[dev] N f32*/, void *denom /*[dev] N f32*/, void *max_radii /*[dev] N f32*/,
                             void *stream);

/* kind[i] = CLONE / SPLIT / KEEP (densify, densify_and_clone, densify_and_split: gaussian_base.py:720-805):
 *   g = denom == 0 ? 0 : accum / denom;  s = expf(scaling) per axis, or with `sphere` the expf of the float32 mean
 *   ((a + b + c) / 3) of the three log-scales on all axes;  nrm = sqrtf(sx^2 + sy^2 + sz^2);
 *   g >= grad_threshold: CLONE when nrm <= split_thresh, SPLIT when nrm > split_thresh;  otherwise KEEP.
 * grad_threshold > 0 is required (a clone's padded gradient is 0: that makes the reference's clone-then-split one pass). */
int dm4d_dc_classify_densify(int64_t N, const void *accum /*[dev]*/, const void *denom /*[dev]*/,
                             const void *scaling /*[dev] N*3 f32, log-scales*/, float grad_threshold, float split_thresh,
                             int32_t sphere, void *kind /*[dev] N u8*/, void *stream);

/* kind[i] = DROP when 1 / (1 + expf(-opacity[i])) < min_opacity, or (radius_limit != NULL) max_radii[i] > *radius_limit;
 * otherwise KEEP (prune, gaussian_base.py:807-812).  radius_limit is a device float the caller fills (3 * mean(max_radii)),
 * so nothing waits for the host; max_radii may be NULL when radius_limit is. */
int dm4d_dc_classify_prune(int64_t N, const void *opacity /*[dev] N f32, logits*/, float min_opacity,
                           const void *max_radii /*[dev] or NULL*/, const void *radius_limit /*[dev] 1 f32 or NULL*/,
                           void *kind /*[dev] N u8*/, void *stream);

/* The plan: a reduce-then-scan of the three ranks (kept = KEEP or CLONE, clone, split) in separate launches -- workgroup totals,
 * one scan of the totals by a single workgroup, then the apply pass.  No kernel waits on another workgroup.
 *   plan_count: scratch <- the scanned workgroup totals;  totals[4] (int64) <- the number of KEEP, DROP, CLONE, SPLIT rows.
 *   [caller: reads totals once, M = KEEP + 2 * CLONE + S * SPLIT, allocates M rows]
 *   plan_rows:  src[M] (int32) and role[M] (uint8) in the reference's order: the kept originals (KEEP and CLONE sources) by
 *               ascending index, then the clones by ascending source, then child 0 of every SPLIT source by ascending index,
 *               then child 1, ...   `scratch` is the one plan_count filled for the same kind and N. */
int64_t dm4d_dc_plan_scratch_bytes(int64_t N);   /* < 0: DM4D_ERR_INVALID */
int dm4d_dc_plan_count(int64_t N, const void *kind /*[dev] N u8*/, void *scratch /*[dev]*/, int64_t scratch_bytes,
                       void *totals /*[dev] 4 i64*/, void *stream);
int dm4d_dc_plan_rows(int64_t N, const void *kind /*[dev]*/, int32_t S, const void *scratch /*[dev]*/, int64_t scratch_bytes,
                      const void *totals /*[dev] 4 i64, as plan_count wrote them*/, int64_t M, void *src /*[dev] M i32*/,
                      void *role /*[dev] M u8*/, void *stream);

/* The row move, one launch for all arrays: out[j] = in[src[j]], rows of `width` floats, a bit copy; 16-byte accesses when
 * width % 4 == 0 and both pointers are 16-byte aligned.  ZERO_NEW: rows with role != KEPT are zeros.  SKIP_CHILDREN: rows with
 * role >= CHILD are left unwritten.  in and out must not overlap. */
typedef struct dm4d_dc_arrays {
    int32_t count;                                  /* 1 .. DM4D_DC_MAX_ARRAYS */
    const void *in[DM4D_DC_MAX_ARRAYS];             /* [dev] N * width f32 */
    void *out[DM4D_DC_MAX_ARRAYS];                  /* [dev] M * width f32 */
    int32_t width[DM4D_DC_MAX_ARRAYS];              /* > 0, floats per row */
    int32_t flags[DM4D_DC_MAX_ARRAYS];
} dm4d_dc_arrays;
int dm4d_dc_move(int64_t N, int64_t M, const void *src /*[dev]*/, const void *role /*[dev]*/, const dm4d_dc_arrays *arrays,
                 void *stream);

/* The rows first_child .. M - 1 (first_child = KEEP + 2 * CLONE), child k of source i = src[j] (gaussian_base.py:732-741):
 *   s = expf(scaling_in[i]) (with `sphere` the common value, as in classify_densify);  q = rotation[i] / |rotation[i]|;
 *   xyz_out[j] = xyz_in[i] + R(q) (noise[k,i] * (s / S))      R as build_rotation (w, x, y, z), float32, no contraction;
 *   scaling_out[j] = logf(s / (0.8f * S)) per axis.
 * noise: [S,N,3] standard normal, indexed by copy and SOURCE index. */
int dm4d_dc_split_children(int64_t N, int64_t M, int64_t first_child, int32_t S, int32_t sphere, const void *src /*[dev]*/,
                           const void *role /*[dev]*/, const void *xyz_in /*[dev] N*3*/, const void *scaling_in /*[dev] N*3*/,
                           const void *rotation_in /*[dev] N*4*/, const void *noise /*[dev] S*N*3*/, void *xyz_out /*[dev] M*3*/,
                           void *scaling_out /*[dev] M*3*/, void *stream);

/* In place: opacity = logit(sigmoid(opacity) * 0.9f), logit(x) = logf(x / (1 - x)); both moments (NULL: none) <- 0
 * (reset_opacity, gaussian_base.py:575-579). */
int dm4d_dc_reset_opacity(int64_t N, void *opacity /*[dev] N f32*/, void *exp_avg /*[dev] or NULL*/,
                          void *exp_avg_sq /*[dev] or NULL*/, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* DM4D_DENSITY_H */
