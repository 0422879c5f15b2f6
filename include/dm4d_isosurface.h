/*
 * dm4d_isosurface.h -- C ABI of the mesh-extraction entry points of libdm4d_hip.so (csrc/isosurface.hip): the occupancy field of
 * a set of Gaussians and marching cubes on it.  Same conventions as dm4d.h: plain pointers and sizes, every pointer marked
 * [dev] is a DEVICE pointer owned by the caller, every call is enqueued on the caller's hipStream_t, no call allocates device
 * memory, return >= 0 success / < 0 one of the DM4D_ERR_* codes of dm4d.h with dm4d_last_error() describing it.
 *
 * Replaces GaussianIO.extract_fields / extract_mesh (C/geometry/gaussian_io.py:174-291; gaussian_3d_coeff,
 * C/geometry/gaussian_base.py:63-96; mcubes.marching_cubes, an un-vendored CPU package).  The semantics are stated in
 * DESIGN.md, "Mesh extraction from Gaussians"; the caller is dreammesh4d_amd/isosurface.py.
 *
 * This header has a version of its own so that dm4d.h (and DM4D_ABI_VERSION) stay as they are.
 */
#ifndef DM4D_ISOSURFACE_H
#define DM4D_ISOSURFACE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DM4D_ISO_ABI_VERSION 1
#define DM4D_ISO_RECORD_FLOATS 16      /* floats per Gaussian record (below) */
#define DM4D_ISO_MAX_RESOLUTION 512    /* 3 * R^3 edge slots stay below 2^31 */

int dm4d_iso_version(void);

/* Per kept Gaussian g (already normalised by the caller: centre (x - center) * scale, standard deviations s * scale, float32):
 *   records[g] = { cx, cy, cz, opacity,  ia, ib, ic, id,  ie, if, 0, 0,  r, g, b, 0 }   (rgb 0 when `rgb` is NULL)
 * with (ia .. if) the inverse of cov = R diag(s^2) R^T (R from the normalised quaternion (w, x, y, z)) by gaussian_3d_coeff's
 * cofactor formula (+ 1e-24 in the determinant), evaluated in float64 and rounded once to float32;
 *   box[g] = { bx0, bx1, by0, by1, bz0, bz1 }: per axis the first and last block b with vmin[b] < centre < vmax[b] (strict),
 *            first > last when there is none;  count[g] = the number of blocks in the box (0 when any axis has none).
 * vmin / vmax: [num_blocks] float32 each, the same bounds on all three axes. */
int dm4d_iso_gaussian_records(int64_t N, const void *xyzn /*[dev] N*3 f32*/, const void *stdn /*[dev] N*3 f32*/,
                              const void *rotation /*[dev] N*4 f32*/, const void *opacity /*[dev] N f32*/,
                              const void *rgb /*[dev] N*3 f32 or NULL*/, int32_t num_blocks, const void *vmin /*[dev]*/,
                              const void *vmax /*[dev]*/, void *records /*[dev] N*16 f32*/, void *box /*[dev] N*6 i32*/,
                              void *count /*[dev] N i64*/, void *stream);

/* keys[offset[g] + j] = block * N + g for the j-th block of g's box, blocks in ascending linear index
 * block = (bx * num_blocks + by) * num_blocks + bz.  offset: [N] int64, the exclusive prefix sum of count; P = the total. */
int dm4d_iso_pair_keys(int64_t N, int64_t P, int32_t num_blocks, const void *box /*[dev]*/, const void *offset /*[dev] N i64*/,
                       void *keys /*[dev] P i64*/, void *stream);

/* occ[R,R,R] (and csum[R,R,R,3] unless NULL) from the SORTED keys: block b owns keys[block_start[b] .. block_start[b + 1]),
 * ascending, so a voxel adds its Gaussians in ascending index.  Per pair, float32, no contraction:
 *   d = p - c;  power = -0.5 * (dx^2 ia + dy^2 id + dz^2 if) - dx dy ib - dx dz ic - dy dz ie;
 *   w = 0 when power > 0 or power < -86 (exp(-86) = 4.5e-38, the edge of float32's normal range), else exp(power);  occ += opacity * w,
 *   csum += opacity * w * rgb -- accumulated per voxel in float64, rounded once to float32.  No atomics.
 * coords: [R] float32 grid coordinates (torch.linspace(-1, 1, R)); block_start: [num_blocks^3 + 1] int64. */
int dm4d_iso_density_field(int64_t N, int64_t P, int32_t R, int32_t num_blocks, const void *coords /*[dev]*/,
                           const void *records /*[dev]*/, const void *keys /*[dev]*/, const void *block_start /*[dev]*/,
                           void *occ /*[dev]*/, void *csum /*[dev] or NULL*/, void *stream);

/* Marching cubes on f[R0,R1,R2] float32; a grid point is inside when f >= threshold.  Voxel n = (i * R1 + j) * R2 + k.
 *   classify: code[n] = case | flags << 8 (case: bit c set when corner (i + (c >> 2 & 1), j + (c >> 1 & 1), k + (c & 1)) is
 *             inside, 0 for a voxel without a cube; flags bit a: the voxel's +axis-a edge exists and is crossed),
 *             n_tris[n], n_verts[n] int32 (the caller scans them into exclusive int64 prefix sums tri_start / vert_start).
 *   vertices: vertex vert_start[n] + (number of lower crossed axes of n) per crossed edge: position a + t along the axis with
 *             t = (threshold - f_a) / (f_b - f_a) in float64, colour (csum_a + t (csum_b - csum_a)) / (f_a + t (f_b - f_a)),
 *             each rounded once to float32; edge_vertex[3 n + axis] = the vertex id (int32; other slots are not written).
 *   faces:    faces[tri_start[n] + t] = the t-th triangle of the cube's case (csrc/mc_table.h) through edge_vertex, int64. */
int dm4d_iso_mc_classify(int32_t R0, int32_t R1, int32_t R2, const void *f /*[dev]*/, double threshold, void *code /*[dev] i32*/,
                         void *n_tris /*[dev] i32*/, void *n_verts /*[dev] i32*/, void *stream);
int dm4d_iso_mc_vertices(int32_t R0, int32_t R1, int32_t R2, const void *f /*[dev]*/, const void *csum /*[dev] or NULL*/,
                         double threshold, const void *code /*[dev]*/, const void *vert_start /*[dev] i64*/, int64_t V,
                         void *verts /*[dev] V*3 f32*/, void *colors /*[dev] V*3 f32 or NULL*/, void *edge_vertex /*[dev] i32*/,
                         void *stream);
int dm4d_iso_mc_faces(int32_t R0, int32_t R1, int32_t R2, const void *code /*[dev]*/, const void *tri_start /*[dev] i64*/,
                      const void *edge_vertex /*[dev]*/, int64_t F, void *faces /*[dev] F*3 i64*/, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* DM4D_ISOSURFACE_H */
