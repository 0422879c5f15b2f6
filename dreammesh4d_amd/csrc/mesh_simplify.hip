// mesh_simplify.hip -- mesh simplification by vertex clustering (gfx950): the kernels behind
// dreammesh4d_amd/mesh_simplify.py.
//
// Reference: TriangleMesh.simplify_vertex_clustering(voxel_size, contraction = Average) as called by
// custom/threestudio-dreammesh4d/scripts/mesh_simplification.py:22-26 (open3d, CPU; un-vendored).  The result here is a
// function of the input alone (DESIGN.md "Mesh simplification"): clusters are numbered by ascending cell key, a cluster's
// position is the float64 sum of its members in ascending vertex index divided once and rounded once, faces keep their
// input order.  Nothing below uses a floating-point atomic, so two runs give the same bytes.
//
//   k_simplify_vertex_keys      vertex -> int64 key of its grid cell                          (streaming, one lane per vertex)
//   [caller: stable sort of the keys -> order, first position of every run of equal keys -> run_start]
//   k_simplify_cluster_average  run of a cluster -> its mean position (and colour), vertex_cluster  (one WAVE per cluster)
//   k_simplify_face_remap       face -> cluster ids, degenerate flag, rotation to smallest-first    (streaming + 3 gathers)
//   [caller: stable sort of the canonical triples -> perm]
//   k_simplify_face_first       sorted position -> keep flag of the first of every run of equal triples
//
// The average is a gather over runs of very uneven length (at scale 8 one cell of a million-vertex mesh holds thousands of
// vertices, at scale 128 about ten).  Its cost is the latency of the two dependent loads per member, order[i] then
// verts[order[i]]; the sum itself must be serial to fix its order.  One lane per cluster would walk its run one dependent
// load pair at a time and hold 63 other lanes for the longest run of the wave; one wave per cluster issues the loads of 64
// members at once (order[] is read coalesced), parks them in LDS, and the lanes 0..NC-1 add their component of the members in
// index order -- NC independent serial chains, one ds_read_b32 + cvt + v_add_f64 per member, the reads independent of the sums.
#include "common.h"
#include "hostcheck.h"
#include "../../include/dm4d.h"

namespace dm4d {

constexpr int kSimThreads = 256;
constexpr int kSimWaves = kSimThreads / 64;

__global__ __launch_bounds__(kSimThreads) void k_simplify_vertex_keys(const int64_t V, const float *__restrict__ verts, const double ox,
                                                                      const double oy, const double oz, const double voxel,
                                                                      const int64_t nx, const int64_t ny, int64_t *__restrict__ keys)
{
    const int64_t v = (int64_t)blockIdx.x * kSimThreads + threadIdx.x;
    if (v >= V) return;
    // IEEE float64 subtract, divide, floor: the same three operations as the float64 statement of the semantics
    const int64_t ix = (int64_t)floor(((double)verts[3 * v] - ox) / voxel);
    const int64_t iy = (int64_t)floor(((double)verts[3 * v + 1] - oy) / voxel);
    const int64_t iz = (int64_t)floor(((double)verts[3 * v + 2] - oz) / voxel);
    keys[v] = (iz * ny + iy) * nx + ix;
}

// orders a wave's LDS writes before the reads other lanes of the SAME wave make of them (a wave's DS operations execute in
// order; the fences keep the compiler from moving them across)
__device__ __forceinline__ void simplify_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// NC = 3 (positions) or 6 (positions and colours).  Cluster c owns order[run_start[c] .. run_start[c + 1]) (.. V for the last).
// Values read from order / run_start are range-checked before they index anything.
template <int NC>
__global__ __launch_bounds__(kSimThreads) void k_simplify_cluster_average(const int64_t V, const int64_t C, const int64_t *__restrict__ order,
                                                                          const int64_t *__restrict__ run_start,
                                                                          const float *__restrict__ verts, const float *__restrict__ colors,
                                                                          float *__restrict__ out_verts, float *__restrict__ out_colors,
                                                                          int64_t *__restrict__ vertex_cluster)
{
    constexpr int LP = NC | 1;                       // odd row stride: the 64 lanes' rows start on different banks
    __shared__ float s_tile[kSimWaves][64 * LP];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t c = (int64_t)blockIdx.x * kSimWaves + wv;
    if (c >= C) return;                              // wave-uniform
    int64_t s = run_start[c], e = c + 1 < C ? run_start[c + 1] : V;
    s = s < 0 ? 0 : (s > V ? V : s);
    e = e < s ? s : (e > V ? V : e);
    float *tile = s_tile[wv];
    double acc = 0.0;
    for (int64_t base = s; base < e; base += 64) {
        const int n = e - base < 64 ? (int)(e - base) : 64;
        if (lane < n) {
            const int64_t i = order[base + lane];
            float m[NC];
#pragma unroll
            for (int k = 0; k < NC; ++k) m[k] = 0.f;
            if ((uint64_t)i < (uint64_t)V) {
                vertex_cluster[i] = c;
#pragma unroll
                for (int k = 0; k < 3; ++k) m[k] = verts[3 * i + k];
                if constexpr (NC == 6) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) m[3 + k] = colors[3 * i + k];
                }
            }
#pragma unroll
            for (int k = 0; k < NC; ++k) tile[lane * LP + k] = m[k];
        }
        simplify_wave_sync();
        if (lane < NC) {
#pragma unroll 8
            for (int j = 0; j < n; ++j) acc = acc + (double)tile[j * LP + lane];     // ascending input vertex index
        }
        simplify_wave_sync();                        // the next chunk overwrites the tile
    }
    if (lane < NC && e > s) {
        const float mean = (float)(acc / (double)(e - s));                           // one division, one rounding to float32
        if (lane < 3) out_verts[3 * c + lane] = mean;
        else out_colors[3 * c + (lane - 3)] = mean;
    }
}

// canon[f] = the face's cluster ids rotated so that the smallest comes first (orientation kept), or (-1, -1, -1) for a face
// that collapses (two corners in one cluster) or names a vertex outside [0, V).  key_bc[f] = canon[f][1] * C + canon[f][2]
// (-1 for a dropped face): with canon[f][0] the two stable sort keys of the lexicographic order of the triples.
__global__ __launch_bounds__(kSimThreads) void k_simplify_face_remap(const int64_t F, const int64_t V, const int64_t C,
                                                                     const int64_t *__restrict__ faces,
                                                                     const int64_t *__restrict__ vertex_cluster,
                                                                     int64_t *__restrict__ canon, int64_t *__restrict__ key_bc)
{
    const int64_t f = (int64_t)blockIdx.x * kSimThreads + threadIdx.x;
    if (f >= F) return;
    const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    int64_t a = -1, b = -1, c = -1;
    if ((uint64_t)i0 < (uint64_t)V && (uint64_t)i1 < (uint64_t)V && (uint64_t)i2 < (uint64_t)V) {
        a = vertex_cluster[i0];
        b = vertex_cluster[i1];
        c = vertex_cluster[i2];
    }
    const bool in_range = (uint64_t)a < (uint64_t)C && (uint64_t)b < (uint64_t)C && (uint64_t)c < (uint64_t)C;
    if (!in_range || a == b || b == c || a == c) {
        canon[3 * f] = canon[3 * f + 1] = canon[3 * f + 2] = -1;
        key_bc[f] = -1;
        return;
    }
    if (b < a && b < c) {                            // (a, b, c) -> (b, c, a)
        const int64_t t = a;
        a = b; b = c; c = t;
    } else if (c < a && c < b) {                     // (a, b, c) -> (c, a, b)
        const int64_t t = c;
        c = b; b = a; a = t;
    }
    canon[3 * f] = a;
    canon[3 * f + 1] = b;
    canon[3 * f + 2] = c;
    key_bc[f] = b * C + c;
}

// perm: the faces in lexicographic order of canon, equal triples in input order (a stable sort).  keep[f] = 1 for a surviving
// face that is the first of its run of equal triples -- the occurrence with the lowest input index.
__global__ __launch_bounds__(kSimThreads) void k_simplify_face_first(const int64_t F, const int64_t *__restrict__ perm,
                                                                     const int64_t *__restrict__ canon, uint8_t *__restrict__ keep)
{
    const int64_t i = (int64_t)blockIdx.x * kSimThreads + threadIdx.x;
    if (i >= F) return;
    const int64_t f = perm[i];
    if ((uint64_t)f >= (uint64_t)F) return;
    const int64_t a = canon[3 * f], b = canon[3 * f + 1], c = canon[3 * f + 2];
    bool first = true;
    if (i > 0) {
        const int64_t g = perm[i - 1];
        if ((uint64_t)g < (uint64_t)F) first = canon[3 * g] != a || canon[3 * g + 1] != b || canon[3 * g + 2] != c;
    }
    keep[f] = (a >= 0 && first) ? 1 : 0;
}

}  // namespace dm4d

using namespace dm4d;

extern "C" {

int dm4d_simplify_vertex_keys(int64_t V, const float *verts, double origin_x, double origin_y, double origin_z, double voxel,
                              int64_t nx, int64_t ny, int64_t nz, int64_t *keys, dm4d_stream_t stream)
{
    const char *fn = "dm4d_simplify_vertex_keys";
    if (bad_count(fn, "V", V)) return DM4D_ERR_INVALID;
    if (!(voxel > 0.0) || !(voxel <= 1.7976931348623157e308) || !(origin_x == origin_x) || !(origin_y == origin_y) || !(origin_z == origin_z)) {
        set_error("%s: voxel size %g must be positive and finite (a mesh with no extent cannot be clustered)", fn, voxel);
        return DM4D_ERR_INVALID;
    }
    if (nx < 1 || ny < 1 || nz < 1) { set_error("%s: grid %lld x %lld x %lld", fn, (long long)nx, (long long)ny, (long long)nz); return DM4D_ERR_INVALID; }
    const unsigned __int128 cells = (unsigned __int128)nx * (unsigned __int128)ny;
    if (cells >> 62 || (cells * (unsigned __int128)nz) >> 62) {
        set_error("%s: the cell keys of a %lld x %lld x %lld grid do not fit in 62 bits", fn, (long long)nx, (long long)ny, (long long)nz);
        return DM4D_ERR_UNSUPPORTED;
    }
    if (V == 0) return DM4D_OK;
    DM4D_REFUSE_NULL(!verts || !keys)
    hipLaunchKernelGGL(k_simplify_vertex_keys, dim3(blocks(V, kSimThreads)), dim3(kSimThreads), 0, (hipStream_t)stream,
                       V, verts, origin_x, origin_y, origin_z, voxel, nx, ny, keys);
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

int dm4d_simplify_cluster_average(int64_t V, int64_t C, const int64_t *order, const int64_t *run_start, const float *verts,
                                  const float *colors, float *out_verts, float *out_colors, int64_t *vertex_cluster, dm4d_stream_t stream)
{
    const char *fn = "dm4d_simplify_cluster_average";
    if (bad_count(fn, "V", V) || bad_count(fn, "C", C)) return DM4D_ERR_INVALID;
    if (C > V || (V > 0 && C == 0)) { set_error("%s: %lld clusters of %lld vertices", fn, (long long)C, (long long)V); return DM4D_ERR_INVALID; }
    if ((colors != nullptr) != (out_colors != nullptr)) { set_error("%s: colors and out_colors go together", fn); return DM4D_ERR_INVALID; }
    if (V == 0) return DM4D_OK;
    DM4D_REFUSE_NULL(!order || !run_start || !verts || !out_verts || !vertex_cluster)
    const dim3 grid(blocks(C, kSimWaves)), block(kSimThreads);
    if (colors)
        hipLaunchKernelGGL(k_simplify_cluster_average<6>, grid, block, 0, (hipStream_t)stream, V, C, order, run_start, verts, colors, out_verts,
                           out_colors, vertex_cluster);
    else
        hipLaunchKernelGGL(k_simplify_cluster_average<3>, grid, block, 0, (hipStream_t)stream, V, C, order, run_start, verts, colors, out_verts,
                           out_colors, vertex_cluster);
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

int dm4d_simplify_face_remap(int64_t F, int64_t V, int64_t C, const int64_t *faces, const int64_t *vertex_cluster, int64_t *canon,
                             int64_t *key_bc, dm4d_stream_t stream)
{
    const char *fn = "dm4d_simplify_face_remap";
    if (bad_count(fn, "F", F) || bad_count(fn, "V", V) || bad_count(fn, "C", C)) return DM4D_ERR_INVALID;
    if (C > V) { set_error("%s: %lld clusters of %lld vertices", fn, (long long)C, (long long)V); return DM4D_ERR_INVALID; }
    if (F == 0) return DM4D_OK;
    DM4D_REFUSE_NULL(!faces || !vertex_cluster || !canon || !key_bc)
    hipLaunchKernelGGL(k_simplify_face_remap, dim3(blocks(F, kSimThreads)), dim3(kSimThreads), 0, (hipStream_t)stream,
                       F, V, C, faces, vertex_cluster, canon, key_bc);
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

int dm4d_simplify_face_first(int64_t F, const int64_t *perm, const int64_t *canon, uint8_t *keep, dm4d_stream_t stream)
{
    const char *fn = "dm4d_simplify_face_first";
    if (bad_count(fn, "F", F)) return DM4D_ERR_INVALID;
    if (F == 0) return DM4D_OK;
    DM4D_REFUSE_NULL(!perm || !canon || !keep)
    hipLaunchKernelGGL(k_simplify_face_first, dim3(blocks(F, kSimThreads)), dim3(kSimThreads), 0, (hipStream_t)stream,
                       F, perm, canon, keep);
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

}  // extern "C"
