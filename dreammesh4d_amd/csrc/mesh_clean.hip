// mesh_clean.hip -- mesh cleaning after marching cubes (gfx950, wave64): the kernels behind dreammesh4d_amd/mesh_clean.py.
//
// Reference: clean_mesh (custom/threestudio-dreammesh4d/geometry/mesh_utils.py:90-128; pymeshlab, CPU, un-vendored) up to, but
// not including, its repair and remeshing filters.  The result here is a function of the input alone (DESIGN.md "Mesh
// cleaning").  Nothing below uses a floating-point atomic, so two runs give the same bytes.
//
//   k_mcl_face_flags        face -> null flag, the two sort keys of its sorted index triple, the mesh bounds  (streaming + 3 gathers)
//   [caller: two stable sorts of the keys -> perm]
//   k_mcl_face_first        sorted position -> alive flag of the first of every run of equal keys
//   k_mcl_init_parent / k_mcl_hook / k_mcl_flatten      one round of union-find over the alive faces
//   k_mcl_stats_init / k_mcl_stats_vertices / k_mcl_stats_faces   roots, per-component boxes and face counts, the check of the round
//   [caller: reads `incomplete`, repeats the round while it is set]
//   k_mcl_comp_keep / k_mcl_keep_masks                  which components stay -> per-vertex and per-face keep flags
//   [caller: inclusive prefix sums of the two flag arrays]
//   k_mcl_compact_vertices / k_mcl_compact_faces        rows moved, faces remapped
//
// Union-find.  parent[v] <= v always, with equality exactly at roots, so every path descends strictly and ends.  Every write
// to parent[] during the hook kernel is a 32-bit atomicMin of a vertex that a chain of alive faces and parent links connects
// to the written one, so a tree never spans two components (safety) and a parent never increases.  No thread waits for another:
// find() only reads and lowers, and the retry of unite() happens only after some thread strictly lowered a parent between
// this thread's read and its atomicMin; a parent can be lowered at most v times, so retries are bounded.  Whether a round joined
// everything is CHECKED, not assumed: k_mcl_stats_faces sets `incomplete` when an alive face still has two labels and the
// caller runs another round, which then strictly lowers at least one parent.  When no face has two labels each component has one
// root, and its smallest vertex m is a root (parent[m] <= m lies in m's component), so label = m whatever the schedule was.
//
// Contention.  Most faces and vertices of a marching-cubes mesh belong to one large component, so the per-component counters
// and boxes would take one atomic per face / vertex on the same few addresses.  A wave whose active lanes all name the same
// component reduces in registers (DPP) and issues one atomic per counter; a mixed wave falls back to one atomic per lane.
#include "common.h"
#include "hostcheck.h"
#include "../../include/dm4d.h"
#include "../../include/dm4d_mesh_clean.h"

namespace dm4d {

constexpr int kMclThreads = 256;

// order-preserving image of a float: a < b (as floats, -0 < +0) <=> image(a) < image(b) (as unsigned)
__device__ __forceinline__ uint32_t mcl_image(float x)
{
    const uint32_t u = as_u(x);
    return u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
}
__device__ __forceinline__ float mcl_unimage(uint32_t k) { return as_f((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// the corners of face f; false when an index lies outside [0, V)
__device__ __forceinline__ bool mcl_load_face(const int32_t *__restrict__ faces, int64_t f, uint32_t V, uint32_t &a, uint32_t &b, uint32_t &c)
{
    a = (uint32_t)faces[3 * f];
    b = (uint32_t)faces[3 * f + 1];
    c = (uint32_t)faces[3 * f + 2];
    return a < V && b < V && c < V;
}

// *ctr += the number of lanes with `pred`: one atomic per wave
__device__ __forceinline__ void mcl_wave_count(bool pred, uint32_t *ctr)
{
    const uint64_t m = __ballot(pred);
    if (m && lane_id() == __ffsll((long long)m) - 1) atomicAdd(ctr, (uint32_t)__popcll(m));
}

__device__ __forceinline__ int32_t mcl_load(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ void k_mcl_state_init(uint32_t *__restrict__ state)
{
    const int i = threadIdx.x;
    if (i < DM4D_MCL_STATE_WORDS) state[i] = i < DM4D_MCL_STATE_HI ? 0xFFFFFFFFu : 0u;
}

// every lane of every wave stays to the end: the wave reductions below need all 64
__global__ __launch_bounds__(kMclThreads) void k_mcl_face_flags(const int64_t F, const uint32_t V, const float *__restrict__ verts,
                                                                const int32_t *__restrict__ faces, uint8_t *__restrict__ null_face,
                                                                int64_t *__restrict__ key_hi, int64_t *__restrict__ key_lo,
                                                                uint32_t *__restrict__ state)
{
    const int64_t f = (int64_t)blockIdx.x * kMclThreads + threadIdx.x;
    uint32_t mn[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[3] = {0u, 0u, 0u};
    bool is_null = false;
    if (f < F) {
        uint32_t a, b, c;
        is_null = true;
        int64_t hi = -1, lo = -1;
        if (mcl_load_face(faces, f, V, a, b, c)) {
            float p[3][3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                p[0][k] = verts[3 * (int64_t)a + k];
                p[1][k] = verts[3 * (int64_t)b + k];
                p[2][k] = verts[3 * (int64_t)c + k];
                const uint32_t i0 = mcl_image(p[0][k]), i1 = mcl_image(p[1][k]), i2 = mcl_image(p[2][k]);
                mn[k] = op_min_u32(i0, op_min_u32(i1, i2));
                mx[k] = op_max_u32(i0, op_max_u32(i1, i2));
            }
            if (a != b && b != c && a != c) {
                const double ux = (double)p[1][0] - (double)p[0][0], uy = (double)p[1][1] - (double)p[0][1], uz = (double)p[1][2] - (double)p[0][2];
                const double vx = (double)p[2][0] - (double)p[0][0], vy = (double)p[2][1] - (double)p[0][1], vz = (double)p[2][2] - (double)p[0][2];
                const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
                is_null = nx == 0.0 && ny == 0.0 && nz == 0.0;
            }
            if (!is_null) {
                const uint32_t s0 = op_min_u32(a, op_min_u32(b, c)), s2 = op_max_u32(a, op_max_u32(b, c));
                const uint32_t s1 = a ^ b ^ c ^ s0 ^ s2;
                hi = (int64_t)s0;
                lo = (int64_t)(((uint64_t)s1 << 31) | (uint64_t)s2);
            }
        }
        null_face[f] = is_null ? 1 : 0;
        key_hi[f] = hi;
        key_lo[f] = lo;
    }
    mcl_wave_count(is_null, state + DM4D_MCL_STATE_N_NULL);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        mn[k] = wave_min_u32(mn[k]);
        mx[k] = wave_max_u32(mx[k]);
    }
    if (lane_id() == 0 && mn[0] <= mx[0]) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            atomicMin(state + DM4D_MCL_STATE_LO + k, mn[k]);
            atomicMax(state + DM4D_MCL_STATE_HI + k, mx[k]);
        }
    }
}

__global__ __launch_bounds__(kMclThreads) void k_mcl_face_first(const int64_t F, const int64_t *__restrict__ perm,
                                                                const int64_t *__restrict__ key_hi, const int64_t *__restrict__ key_lo,
                                                                const uint8_t *__restrict__ null_face, uint8_t *__restrict__ alive,
                                                                uint32_t *__restrict__ state)
{
    const int64_t i = (int64_t)blockIdx.x * kMclThreads + threadIdx.x;
    bool duplicate = false;
    if (i < F) {
        const int64_t f = perm[i];
        if ((uint64_t)f < (uint64_t)F) {
            const bool nul = null_face[f] != 0;
            bool first = true;
            if (i > 0) {
                const int64_t g = perm[i - 1];
                if ((uint64_t)g < (uint64_t)F) first = key_hi[g] != key_hi[f] || key_lo[g] != key_lo[f];
            }
            duplicate = !nul && !first;
            alive[f] = (!nul && first) ? 1 : 0;
        }
    }
    mcl_wave_count(duplicate, state + DM4D_MCL_STATE_N_DUPLICATE);
}

__global__ __launch_bounds__(kMclThreads) void k_mcl_init_parent(const int64_t V, int32_t *__restrict__ parent)
{
    const int64_t v = (int64_t)blockIdx.x * kMclThreads + threadIdx.x;
    if (v < V) parent[v] = (int32_t)v;
}

// a root above x, lowering parent[] along the way (path halving): reads, and atomicMin of an ancestor
__device__ __forceinline__ int32_t mcl_find(int32_t *parent, int32_t x)
{
    for (;;) {
        const int32_t p = mcl_load(parent + x);
        if ((uint32_t)p >= (uint32_t)x) return x;        // p == x: a root (a value outside [0, x] cannot arise; it also ends the walk)
        const int32_t g = mcl_load(parent + p);
        if ((uint32_t)g >= (uint32_t)p) return p;
        atomicMin(parent + x, g);
        x = g;
    }
}

__device__ __forceinline__ void mcl_unite(int32_t *parent, int32_t a, int32_t b)
{
    for (;;) {
        a = mcl_find(parent, a);
        b = mcl_find(parent, b);
        if (a == b) return;
        if (a < b) {
            const int32_t t = a;
            a = b;
            b = t;
        }
        const int32_t old = atomicMin(parent + a, b);    // a > b
        if (old == a) return;                            // a was a root and now hangs under b
        // another thread lowered parent[a] first (to old < a).  parent[a] is now min(old, b); either way old and b belong
        // together and nothing but this thread may know it
        a = old;
    }
}

__global__ __launch_bounds__(kMclThreads) void k_mcl_hook(const int64_t F, const uint32_t V, const int32_t *__restrict__ faces,
                                                          const uint8_t *__restrict__ alive, int32_t *parent)
{
    const int64_t f = (int64_t)blockIdx.x * kMclThreads + threadIdx.x;
    if (f >= F || (alive && !alive[f])) return;
    uint32_t a, b, c;
    if (!mcl_load_face(faces, f, V, a, b, c)) return;
    if (a != b) mcl_unite(parent, (int32_t)a, (int32_t)b);
    if (b != c) mcl_unite(parent, (int32_t)b, (int32_t)c);
}

// no hook runs beside this kernel, so root(v) is fixed; the plain store of a root over an ancestor keeps every path valid
__global__ __launch_bounds__(kMclThreads) void k_mcl_flatten(const int64_t V, int32_t *parent)
{
    const int64_t v = (int64_t)blockIdx.x * kMclThreads + threadIdx.x;
    if (v >= V) return;
    int32_t x = (int32_t)v;
    for (;;) {
        const int32_t p = mcl_load(parent + x);
        if ((uint32_t)p >= (uint32_t)x) break;
        x = p;
    }
    __hip_atomic_store(parent + v, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void k_mcl_round_reset(uint32_t *__restrict__ state)
{
    if (threadIdx.x == 0) {
        state[DM4D_MCL_STATE_INCOMPLETE] = 0u;
        state[DM4D_MCL_STATE_N_COMPONENTS] = 0u;
    }
}

__global__ __launch_bounds__(kMclThreads) void k_mcl_stats_init(const int64_t V, const int32_t *__restrict__ labels,
                                                                int32_t *__restrict__ face_count, uint32_t *__restrict__ box,
                                                                uint32_t *__restrict__ state)
{
    const int64_t v = (int64_t)blockIdx.x * kMclThreads + threadIdx.x;
    bool root = false;
    if (v < V) {
        root = labels[v] == (int32_t)v;
        face_count[v] = 0;
        if (box) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                box[6 * v + k] = 0xFFFFFFFFu;
                box[6 * v + 3 + k] = 0u;
            }
        }
    }
    mcl_wave_count(root, state + DM4D_MCL_STATE_N_COMPONENTS);
}

// the first active lane and whether every active lane names the same label (wave-uniform results; all 64 lanes call)
__device__ __forceinline__ bool mcl_wave_same_label(bool active, uint32_t label, int &lead, uint32_t &l0, uint64_t &mask)
{
    mask = __ballot(active);
    lead = mask ? __ffsll((long long)mask) - 1 : 0;
    l0 = (uint32_t)__shfl((int)label, lead);
    return __ballot(active && label != l0) == 0;
}

__global__ __launch_bounds__(kMclThreads) void k_mcl_stats_vertices(const int64_t V, const float *__restrict__ verts,
                                                                    const int32_t *__restrict__ labels, uint32_t *box)
{
    const int64_t v = (int64_t)blockIdx.x * kMclThreads + threadIdx.x;
    uint32_t label = 0, im[3] = {0u, 0u, 0u};
    bool active = false;
    if (v < V) {
        label = (uint32_t)labels[v];
        active = label < (uint32_t)V;
        if (active) {
#pragma unroll
            for (int k = 0; k < 3; ++k) im[k] = mcl_image(verts[3 * v + k]);
        }
    }
    int lead;
    uint32_t l0;
    uint64_t mask;
    const bool same = mcl_wave_same_label(active, label, lead, l0, mask);
    if (mask == 0) return;                               // wave-uniform
    if (same) {
        uint32_t mn[3], mx[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            mn[k] = wave_min_u32(active ? im[k] : 0xFFFFFFFFu);
            mx[k] = wave_max_u32(active ? im[k] : 0u);
        }
        if (lane_id() == lead) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                atomicMin(box + 6 * (int64_t)l0 + k, mn[k]);
                atomicMax(box + 6 * (int64_t)l0 + 3 + k, mx[k]);
            }
        }
    } else if (active) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            atomicMin(box + 6 * (int64_t)label + k, im[k]);
            atomicMax(box + 6 * (int64_t)label + 3 + k, im[k]);
        }
    }
}

__global__ __launch_bounds__(kMclThreads) void k_mcl_stats_faces(const int64_t F, const uint32_t V, const int32_t *__restrict__ faces,
                                                                 const uint8_t *__restrict__ alive, const int32_t *__restrict__ labels,
                                                                 int32_t *face_count, uint32_t *state)
{
    const int64_t f = (int64_t)blockIdx.x * kMclThreads + threadIdx.x;
    uint32_t label = 0;
    bool active = false, split = false;
    if (f < F && (!alive || alive[f])) {
        uint32_t a, b, c;
        if (mcl_load_face(faces, f, V, a, b, c)) {
            label = (uint32_t)labels[a];
            const uint32_t lb = (uint32_t)labels[b], lc = (uint32_t)labels[c];
            split = label != lb || label != lc;
            active = !split && label < V;
        }
    }
    if (split) state[DM4D_MCL_STATE_INCOMPLETE] = 1u;                           // every writer stores the same word
    int lead;
    uint32_t l0;
    uint64_t mask;
    const bool same = mcl_wave_same_label(active, label, lead, l0, mask);
    if (mask == 0) return;
    if (same) {
        if (lane_id() == lead) atomicAdd(face_count + l0, (int32_t)__popcll(mask));
    } else if (active) {
        atomicAdd(face_count + label, 1);
    }
}

__global__ void k_mcl_keep_reset(uint32_t *__restrict__ state)
{
    if (threadIdx.x == 0) {
        state[DM4D_MCL_STATE_N_SMALL] = 0u;
        state[DM4D_MCL_STATE_BEST] = 0u;
        state[DM4D_MCL_STATE_BEST + 1] = 0u;
    }
}

__global__ __launch_bounds__(kMclThreads) void k_mcl_comp_keep(const int64_t V, const int32_t *__restrict__ labels,
                                                               const int32_t *__restrict__ face_count, const uint32_t *__restrict__ box,
                                                               const double thr2, const int use_d, const int64_t min_f, const int largest,
                                                               uint8_t *__restrict__ comp_keep, uint32_t *state)
{
    const int64_t v = (int64_t)blockIdx.x * kMclThreads + threadIdx.x;
    bool small = false;
    if (v < V) {
        bool keep = false;
        const int32_t cnt = face_count[v];
        if (labels[v] == (int32_t)v && cnt > 0) {
            bool small_d = false;
            if (use_d) {
                const double dx = (double)mcl_unimage(box[6 * v + 3]) - (double)mcl_unimage(box[6 * v]);
                const double dy = (double)mcl_unimage(box[6 * v + 4]) - (double)mcl_unimage(box[6 * v + 1]);
                const double dz = (double)mcl_unimage(box[6 * v + 5]) - (double)mcl_unimage(box[6 * v + 2]);
                const double d2 = dx * dx + dy * dy + dz * dz;
                small_d = d2 < thr2;
            }
            small = small_d || (min_f > 0 && (int64_t)cnt < min_f);
            keep = !small;
            if (keep && largest)
                atomicMax((unsigned long long *)(state + DM4D_MCL_STATE_BEST),
                          ((unsigned long long)(uint32_t)cnt << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)v));
        }
        comp_keep[v] = keep ? 1 : 0;
    }
    mcl_wave_count(small, state + DM4D_MCL_STATE_N_SMALL);
}

__global__ __launch_bounds__(kMclThreads) void k_mcl_keep_masks(const int64_t F, const int64_t V, const int32_t *__restrict__ faces,
                                                                const uint8_t *__restrict__ alive, const int32_t *__restrict__ labels,
                                                                const uint8_t *__restrict__ comp_keep, const int largest,
                                                                const uint32_t *__restrict__ state, uint8_t *__restrict__ keep_vertex,
                                                                uint8_t *__restrict__ keep_face)
{
    const int64_t i = (int64_t)blockIdx.x * kMclThreads + threadIdx.x;
    const unsigned long long best = *(const unsigned long long *)(state + DM4D_MCL_STATE_BEST);
    const uint32_t winner = 0xFFFFFFFFu - (uint32_t)best;
    auto stays = [&](uint32_t l) { return l < (uint32_t)V && comp_keep[l] != 0 && (!largest || (best != 0ull && l == winner)); };
    if (i < V) keep_vertex[i] = stays((uint32_t)labels[i]) ? 1 : 0;
    if (i < F) {
        uint32_t a, b, c;
        bool keep = false;
        if (alive[i] && mcl_load_face(faces, i, (uint32_t)V, a, b, c)) keep = stays((uint32_t)labels[a]);
        keep_face[i] = keep ? 1 : 0;
    }
}

__global__ __launch_bounds__(kMclThreads) void k_mcl_compact_vertices(const int64_t V, const int64_t Vo, const float *__restrict__ verts,
                                                                      const float *__restrict__ colors, const uint8_t *__restrict__ keep_vertex,
                                                                      const int64_t *__restrict__ vert_end, float *__restrict__ out_verts,
                                                                      float *__restrict__ out_colors, int64_t *__restrict__ vertex_map)
{
    const int64_t v = (int64_t)blockIdx.x * kMclThreads + threadIdx.x;
    if (v >= V) return;
    const int64_t o = keep_vertex[v] ? vert_end[v] - 1 : -1;
    if ((uint64_t)o >= (uint64_t)Vo) {
        vertex_map[v] = -1;
        return;
    }
    vertex_map[v] = o;
#pragma unroll
    for (int k = 0; k < 3; ++k) out_verts[3 * o + k] = verts[3 * v + k];
    if (colors) {
#pragma unroll
        for (int k = 0; k < 3; ++k) out_colors[3 * o + k] = colors[3 * v + k];
    }
}

__global__ __launch_bounds__(kMclThreads) void k_mcl_compact_faces(const int64_t F, const int64_t V, const int64_t Fo, const int64_t Vo,
                                                                   const int32_t *__restrict__ faces, const uint8_t *__restrict__ keep_vertex,
                                                                   const int64_t *__restrict__ vert_end, const uint8_t *__restrict__ keep_face,
                                                                   const int64_t *__restrict__ face_end, int64_t *__restrict__ out_faces,
                                                                   int64_t *__restrict__ face_map)
{
    const int64_t f = (int64_t)blockIdx.x * kMclThreads + threadIdx.x;
    if (f >= F || !keep_face[f]) return;
    const int64_t o = face_end[f] - 1;
    uint32_t idx[3];
    if ((uint64_t)o >= (uint64_t)Fo || !mcl_load_face(faces, f, (uint32_t)V, idx[0], idx[1], idx[2])) return;
    face_map[o] = f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int64_t n = keep_vertex[idx[k]] ? vert_end[idx[k]] - 1 : -1;
        out_faces[3 * o + k] = (uint64_t)n < (uint64_t)Vo ? n : -1;
    }
}

}  // namespace dm4d

using namespace dm4d;

extern "C" {

int dm4d_mcl_version(void) { return DM4D_MCL_ABI_VERSION; }

int dm4d_mcl_face_flags(int64_t F, int64_t V, const void *verts, const void *faces, void *null_face, void *key_hi, void *key_lo, void *state,
                        void *stream)
{
    const char *fn = "dm4d_mcl_face_flags";
    if (bad_count(fn, "F", F) || bad_count(fn, "V", V)) return DM4D_ERR_INVALID;
    const Arg args[] = {{"verts", verts, 4, F ? V : 0}, {"faces", faces, 4, F}, {"null_face", null_face, 1, F}, {"key_hi", key_hi, 8, F},
                           {"key_lo", key_lo, 8, F}, {"state", state, 8, 1}};
    if (bad_args(fn, args)) return DM4D_ERR_INVALID;
    hipLaunchKernelGGL(k_mcl_state_init, dim3(1), dim3(64), 0, (hipStream_t)stream, (uint32_t *)state);
    if (F > 0)
        hipLaunchKernelGGL(k_mcl_face_flags, dim3(blocks(F, kMclThreads)), dim3(kMclThreads), 0, (hipStream_t)stream, F, (uint32_t)V, (const float *)verts,
                           (const int32_t *)faces, (uint8_t *)null_face, (int64_t *)key_hi, (int64_t *)key_lo, (uint32_t *)state);
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

int dm4d_mcl_face_first(int64_t F, const void *perm, const void *key_hi, const void *key_lo, const void *null_face, void *alive, void *state,
                        void *stream)
{
    const char *fn = "dm4d_mcl_face_first";
    if (bad_count(fn, "F", F)) return DM4D_ERR_INVALID;
    const Arg args[] = {{"perm", perm, 8, F}, {"key_hi", key_hi, 8, F}, {"key_lo", key_lo, 8, F}, {"null_face", null_face, 1, F},
                           {"alive", alive, 1, F}, {"state", state, 8, 1}};
    if (bad_args(fn, args)) return DM4D_ERR_INVALID;
    if (F == 0) return DM4D_OK;
    hipLaunchKernelGGL(k_mcl_face_first, dim3(blocks(F, kMclThreads)), dim3(kMclThreads), 0, (hipStream_t)stream, F, (const int64_t *)perm, (const int64_t *)key_hi,
                       (const int64_t *)key_lo, (const uint8_t *)null_face, (uint8_t *)alive, (uint32_t *)state);
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

int dm4d_mcl_components_round(int64_t F, int64_t V, const void *faces, const void *alive, int32_t first_round, void *parent, void *stream)
{
    const char *fn = "dm4d_mcl_components_round";
    if (bad_count(fn, "F", F) || bad_count(fn, "V", V)) return DM4D_ERR_INVALID;
    const Arg args[] = {{"faces", faces, 4, F}, {"alive", alive, 1, 0}, {"parent", parent, 4, V}};
    if (bad_args(fn, args)) return DM4D_ERR_INVALID;
    if (V == 0) return DM4D_OK;
    hipStream_t st = (hipStream_t)stream;
    if (first_round) hipLaunchKernelGGL(k_mcl_init_parent, dim3(blocks(V, kMclThreads)), dim3(kMclThreads), 0, st, V, (int32_t *)parent);
    if (F > 0) {
        hipLaunchKernelGGL(k_mcl_hook, dim3(blocks(F, kMclThreads)), dim3(kMclThreads), 0, st, F, (uint32_t)V, (const int32_t *)faces, (const uint8_t *)alive,
                           (int32_t *)parent);
        hipLaunchKernelGGL(k_mcl_flatten, dim3(blocks(V, kMclThreads)), dim3(kMclThreads), 0, st, V, (int32_t *)parent);
    }
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

int dm4d_mcl_component_stats(int64_t F, int64_t V, const void *verts, const void *faces, const void *alive, const void *labels, void *face_count,
                             void *box, void *state, void *stream)
{
    const char *fn = "dm4d_mcl_component_stats";
    if (bad_count(fn, "F", F) || bad_count(fn, "V", V)) return DM4D_ERR_INVALID;
    if ((verts != nullptr) != (box != nullptr) && V > 0) { set_error("%s: verts and box go together", fn); return DM4D_ERR_INVALID; }
    const Arg args[] = {{"verts", verts, 4, 0}, {"faces", faces, 4, F}, {"alive", alive, 1, 0}, {"labels", labels, 4, V},
                           {"face_count", face_count, 4, V}, {"box", box, 4, 0}, {"state", state, 8, 1}};
    if (bad_args(fn, args)) return DM4D_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_mcl_round_reset, dim3(1), dim3(64), 0, st, (uint32_t *)state);
    if (V > 0) {
        hipLaunchKernelGGL(k_mcl_stats_init, dim3(blocks(V, kMclThreads)), dim3(kMclThreads), 0, st, V, (const int32_t *)labels, (int32_t *)face_count,
                           (uint32_t *)box, (uint32_t *)state);
        if (box)
            hipLaunchKernelGGL(k_mcl_stats_vertices, dim3(blocks(V, kMclThreads)), dim3(kMclThreads), 0, st, V, (const float *)verts, (const int32_t *)labels,
                               (uint32_t *)box);
        if (F > 0)
            hipLaunchKernelGGL(k_mcl_stats_faces, dim3(blocks(F, kMclThreads)), dim3(kMclThreads), 0, st, F, (uint32_t)V, (const int32_t *)faces,
                               (const uint8_t *)alive, (const int32_t *)labels, (int32_t *)face_count, (uint32_t *)state);
    }
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

int dm4d_mcl_keep(int64_t F, int64_t V, const void *faces, const void *alive, const void *labels, const void *face_count, const void *box,
                  double thr2, int32_t use_d, int64_t min_f, int32_t largest, void *comp_keep, void *keep_vertex, void *keep_face, void *state,
                  void *stream)
{
    const char *fn = "dm4d_mcl_keep";
    if (bad_count(fn, "F", F) || bad_count(fn, "V", V) || bad_count(fn, "min_f", min_f)) return DM4D_ERR_INVALID;
    if (!(thr2 >= 0.0) || (use_d != 0 && use_d != 1) || (largest != 0 && largest != 1)) {
        set_error("%s: thr2 = %g must be a number >= 0, use_d = %d and largest = %d flags 0 or 1", fn, thr2, use_d, largest);
        return DM4D_ERR_INVALID;
    }
    const Arg args[] = {{"faces", faces, 4, V ? F : 0}, {"alive", alive, 1, V ? F : 0}, {"labels", labels, 4, V}, {"face_count", face_count, 4, V},
                           {"box", box, 4, use_d ? V : 0}, {"comp_keep", comp_keep, 1, V}, {"keep_vertex", keep_vertex, 1, V},
                           {"keep_face", keep_face, 1, V ? F : 0}, {"state", state, 8, 1}};
    if (bad_args(fn, args)) return DM4D_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_mcl_keep_reset, dim3(1), dim3(64), 0, st, (uint32_t *)state);
    if (V > 0) {
        hipLaunchKernelGGL(k_mcl_comp_keep, dim3(blocks(V, kMclThreads)), dim3(kMclThreads), 0, st, V, (const int32_t *)labels, (const int32_t *)face_count,
                           (const uint32_t *)box, thr2, (int)use_d, min_f, (int)largest, (uint8_t *)comp_keep, (uint32_t *)state);
        hipLaunchKernelGGL(k_mcl_keep_masks, dim3(blocks(V > F ? V : F, kMclThreads)), dim3(kMclThreads), 0, st, F, V, (const int32_t *)faces, (const uint8_t *)alive,
                           (const int32_t *)labels, (const uint8_t *)comp_keep, (int)largest, (const uint32_t *)state, (uint8_t *)keep_vertex,
                           (uint8_t *)keep_face);
    }
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

int dm4d_mcl_compact(int64_t F, int64_t V, int64_t Fo, int64_t Vo, const void *verts, const void *colors, const void *faces, const void *keep_vertex,
                     const void *vert_end, const void *keep_face, const void *face_end, void *out_verts, void *out_colors, void *out_faces,
                     void *vertex_map, void *face_map, void *stream)
{
    const char *fn = "dm4d_mcl_compact";
    if (bad_count(fn, "F", F) || bad_count(fn, "V", V) || bad_count(fn, "Fo", Fo) || bad_count(fn, "Vo", Vo)) return DM4D_ERR_INVALID;
    if (Fo > F || Vo > V) { set_error("%s: Fo = %lld of F = %lld faces, Vo = %lld of V = %lld vertices", fn, (long long)Fo, (long long)F, (long long)Vo, (long long)V); return DM4D_ERR_INVALID; }
    if ((colors != nullptr) != (out_colors != nullptr) && Vo > 0) { set_error("%s: colors and out_colors go together", fn); return DM4D_ERR_INVALID; }
    const Arg args[] = {{"verts", verts, 4, V}, {"colors", colors, 4, 0}, {"faces", faces, 4, V ? F : 0}, {"keep_vertex", keep_vertex, 1, V},
                           {"vert_end", vert_end, 8, V}, {"keep_face", keep_face, 1, V ? F : 0}, {"face_end", face_end, 8, V ? F : 0},
                           {"out_verts", out_verts, 4, Vo}, {"out_colors", out_colors, 4, 0}, {"out_faces", out_faces, 8, Fo},
                           {"vertex_map", vertex_map, 8, V}, {"face_map", face_map, 8, Fo}};
    if (bad_args(fn, args)) return DM4D_ERR_INVALID;
    if (V == 0) return DM4D_OK;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_mcl_compact_vertices, dim3(blocks(V, kMclThreads)), dim3(kMclThreads), 0, st, V, Vo, (const float *)verts,
                       Vo > 0 ? (const float *)colors : nullptr, (const uint8_t *)keep_vertex, (const int64_t *)vert_end, (float *)out_verts,
                       (float *)out_colors, (int64_t *)vertex_map);
    if (F > 0 && Fo > 0)
        hipLaunchKernelGGL(k_mcl_compact_faces, dim3(blocks(F, kMclThreads)), dim3(kMclThreads), 0, st, F, V, Fo, Vo, (const int32_t *)faces,
                           (const uint8_t *)keep_vertex, (const int64_t *)vert_end, (const uint8_t *)keep_face, (const int64_t *)face_end,
                           (int64_t *)out_faces, (int64_t *)face_map);
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

}  // extern "C"
