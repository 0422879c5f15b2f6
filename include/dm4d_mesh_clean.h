/*
 * dm4d_mesh_clean.h -- C ABI of the mesh-cleaning entry points of libdm4d_hip.so (csrc/mesh_clean.hip): null and duplicate
 * faces, connected components by union-find, per-component statistics, the keep masks and the compaction.  Same conventions as
 * dm4d_isosurface.h: plain pointers and sizes, every pointer marked [dev] is a DEVICE pointer owned by the caller, every call is
 * enqueued on the caller's hipStream_t, no call allocates device memory, return >= 0 success / < 0 one of the DM4D_ERR_* codes
 * of dm4d.h with dm4d_last_error() describing it.
 *
 * Replaces the first half of clean_mesh (C/geometry/mesh_utils.py:90-128; pymeshlab, an un-vendored CPU package) as called by
 * GaussianIO.extract_mesh (C/geometry/gaussian_io.py:267-291).  The semantics are stated in DESIGN.md, "Mesh cleaning"; the
 * caller is dreammesh4d_amd/mesh_clean.py.
 *
 * Every entry point refuses, before any launch and by the argument's name: a size outside [0, 2^31 - 1], a null pointer to an
 * array that has elements, and a pointer that is not aligned to its element (4 bytes for f32 / i32 / u32, 8 for i64 and
 * `state`).  Face indices outside [0, V) never index anything: such a face counts as null and joins nothing.
 *
 * This header has a version of its own so that dm4d.h (and DM4D_ABI_VERSION) stay as they are.
 */
#ifndef DM4D_MESH_CLEAN_H
#define DM4D_MESH_CLEAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DM4D_MCL_ABI_VERSION 1

/* `state`: 16 uint32 words on the device, 8-byte aligned, shared by the calls of one cleaning:
 *   [0..2] / [3..5]  order-preserving image of the per-axis float32 min / max over the vertices any face names
 *                    (image(x) = bits ^ 0x80000000 for a clear sign bit, ~bits for a set one; 0xFFFFFFFF / 0 while empty)
 *   [6]   incomplete: some surviving face still has corners with different labels (run another round)
 *   [7]   n_null   [8] n_duplicate   [9] n_components (distinct labels)   [10] n_small
 *   [12..13]  one uint64: the largest kept component, face_count << 32 | (0xFFFFFFFF - label); 0 when there is none */
#define DM4D_MCL_STATE_WORDS 16
#define DM4D_MCL_STATE_LO 0
#define DM4D_MCL_STATE_HI 3
#define DM4D_MCL_STATE_INCOMPLETE 6
#define DM4D_MCL_STATE_N_NULL 7
#define DM4D_MCL_STATE_N_DUPLICATE 8
#define DM4D_MCL_STATE_N_COMPONENTS 9
#define DM4D_MCL_STATE_N_SMALL 10
#define DM4D_MCL_STATE_BEST 12

int dm4d_mcl_version(void);

/* Initialises `state`, then per face f = (a, b, c):
 *   null_face[f] = 1 when an index lies outside [0, V), when two indices are equal, or when the float64 cross product
 *                  (vb - va) x (vc - va) of the float32 corners is exactly (0, 0, 0) (differences, products and their
 *                  differences each one IEEE float64 operation); n_null counts them;
 *   key_hi[f] = s0, key_lo[f] = s1 << 31 | s2 with s0 <= s1 <= s2 the sorted indices (each below 2^31, so the pair holds for
 *               every V up to 2^31 - 1); both -1 for a null face.  Equal pairs <=> equal sorted triples.
 * The bounds of `state` cover the corners of every face whose indices are in range, null or not. */
int dm4d_mcl_face_flags(int64_t F, int64_t V, const void *verts /*[dev] V*3 f32*/, const void *faces /*[dev] F*3 i32*/,
                        void *null_face /*[dev] F u8*/, void *key_hi /*[dev] F i64*/, void *key_lo /*[dev] F i64*/,
                        void *state /*[dev]*/, void *stream);

/* perm: the faces in ascending (key_hi, key_lo), equal keys in input order (two stable sorts by the caller).
 * alive[f] = 1 for a face that is not null and is the first of its run of equal keys; n_duplicate counts the others that are
 * not null. */
int dm4d_mcl_face_first(int64_t F, const void *perm /*[dev] F i64*/, const void *key_hi /*[dev]*/, const void *key_lo /*[dev]*/,
                        const void *null_face /*[dev]*/, void *alive /*[dev] F u8*/, void *state /*[dev]*/, void *stream);

/* One round of union-find over the faces with alive[f] != 0 (every face when `alive` is NULL): parent[v] = v first when
 * `first_round`, then every face hooks its corners together (the larger root under the smaller, 32-bit atomicMin, path
 * halving), then parent[v] = root(v) for every v.  parent[v] <= v throughout.  The caller runs dm4d_mcl_component_stats next
 * and repeats the round while it reports `incomplete`. */
int dm4d_mcl_components_round(int64_t F, int64_t V, const void *faces /*[dev] F*3 i32*/, const void *alive /*[dev] F u8 or NULL*/,
                              int32_t first_round, void *parent /*[dev] V i32*/, void *stream);

/* From flattened labels (labels[v] = the root of v): n_components = the number of v with labels[v] == v; `incomplete` set when
 * a surviving face has corners with different labels; otherwise face_count[l] = the surviving faces of component l and, when
 * `box` is given, box[6 l ..] = the image (as in `state`) of the float32 min / max over the vertices with label l.
 * Integer atomics only. */
int dm4d_mcl_component_stats(int64_t F, int64_t V, const void *verts /*[dev] V*3 f32, NULL with box NULL*/,
                             const void *faces /*[dev]*/, const void *alive /*[dev] or NULL*/, const void *labels /*[dev] V i32*/,
                             void *face_count /*[dev] V i32*/, void *box /*[dev] V*6 u32 or NULL*/, void *state /*[dev]*/,
                             void *stream);

/* A component with faces is dropped when use_d and d2 < thr2 (d2 = dx dx + dy dy + dz dz in float64 of its float32 box, no
 * contraction), else when min_f > 0 and face_count < min_f; n_small counts the dropped.  With `largest` only the kept component
 * with the most faces stays (ties: the smallest label).  keep_vertex[v] = 1 when v's component stays and has faces,
 * keep_face[f] = alive[f] and the component of its first corner stays.  comp_keep: V bytes of scratch. */
int dm4d_mcl_keep(int64_t F, int64_t V, const void *faces /*[dev]*/, const void *alive /*[dev]*/, const void *labels /*[dev]*/,
                  const void *face_count /*[dev]*/, const void *box /*[dev]*/, double thr2, int32_t use_d, int64_t min_f,
                  int32_t largest, void *comp_keep /*[dev] V u8*/, void *keep_vertex /*[dev] V u8*/, void *keep_face /*[dev] F u8*/,
                  void *state /*[dev]*/, void *stream);

/* vert_end / face_end: the inclusive int64 prefix sums of keep_vertex / keep_face; Vo / Fo their totals.
 *   vertex_map[v] = vert_end[v] - 1 for a kept vertex, else -1; out_verts / out_colors rows copied bit for bit;
 *   out_faces[face_end[f] - 1] = vertex_map of f's corners, face_map[face_end[f] - 1] = f for a kept face.
 * A position outside [0, Vo) / [0, Fo) is not written. */
int dm4d_mcl_compact(int64_t F, int64_t V, int64_t Fo, int64_t Vo, const void *verts /*[dev]*/, const void *colors /*[dev] or NULL*/,
                     const void *faces /*[dev]*/, const void *keep_vertex /*[dev]*/, const void *vert_end /*[dev] V i64*/,
                     const void *keep_face /*[dev]*/, const void *face_end /*[dev] F i64*/, void *out_verts /*[dev] Vo*3 f32*/,
                     void *out_colors /*[dev] Vo*3 f32 or NULL*/, void *out_faces /*[dev] Fo*3 i64*/, void *vertex_map /*[dev] V i64*/,
                     void *face_map /*[dev] Fo i64*/, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* DM4D_MESH_CLEAN_H */
