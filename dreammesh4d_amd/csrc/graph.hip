// graph.hip -- deformation-graph construction: K nearest graph nodes of every mesh vertex in GEODESIC distance and
// their skinning weights (gfx950).
//
// Reference: DynamicSuGaRModel.build_deformation_graph(mode="geodisc")
// (custom/threestudio-dreammesh4d/geometry/dynamic_sugar.py:745-861): for every one of the V vertices one heat-method
// solve (potpourri3d, CPU) gives its geodesic distance to the M nodes' nearest vertices; the K nearest nodes are kept
// and weighted (1 - d_k / d_{K+1})^2 with EUCLIDEAN distances to the node positions, rows normalised (:845,859-861) --
// V sequential sparse solves, minutes of start-up at 16k vertices.
//
// Here distance is symmetric, so the M nodes are the sources: one [M, V] distance table relaxed in place over the
// mesh edges (thread = (node, vertex), d[v] = min(d[v], d[u] + |uv|) over the one-ring; values only decrease, the
// fixed point is the shortest edge path from the node's vertex whatever the update order -- deterministic), then one
// thread per vertex selects the K + 1 smallest of its M distances (ties towards the lower node index, as a stable
// argsort does).  Shortest edge paths over-estimate the smooth geodesic distance the heat method approximates by a
// bounded factor; the reference's own solver is not in the tree, so the choice of neighbours is pinned against an
// exact Dijkstra on the same edge graph (oracle/graph.py), not against potpourri3d: parity unpinned.
#include "common.h"
#include "../../include/dm4d.h"

namespace dm4d {

constexpr int kGeoMaxK = 16;
// a ranks strictly before b in numpy's sort order: NaN last (after +inf), NaN beside NaN a tie
__device__ __forceinline__ bool geo_ranks_before(float a, float b) { return a < b || (b != b && a == a); }

__global__ __launch_bounds__(256) void k_geo_init(int V, int M, const int32_t *__restrict__ src, float *__restrict__ d)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const int m = blockIdx.y;
    d[(size_t)m * V + v] = (src[m] == v) ? 0.0f : 3.0e38f;
}

__global__ __launch_bounds__(256) void k_geo_relax(int V, int M, const int32_t *__restrict__ off, const int32_t *__restrict__ nbr,
                                                   const float *__restrict__ len, float *d, int32_t *__restrict__ changed)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    float *row = d + (size_t)blockIdx.y * V;
    const float old = row[v];
    float best = old;
    for (int e = off[v]; e < off[v + 1]; ++e) best = fminf(best, __builtin_nontemporal_load(row + nbr[e]) + len[e]);
    if (best < old) {
        row[v] = best;
        *changed = 1;
    }
}

__global__ __launch_bounds__(256) void k_geo_select(int V, int M, int K, const float *__restrict__ d, const float *__restrict__ verts,
                                                    const float *__restrict__ node_xyz, int64_t *__restrict__ idx,
                                                    float *__restrict__ weights)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    // (as k_graph_select of heat.hip: the first K + 1 nodes always enter, so no index outside [0, M) can be written)
    float bd[kGeoMaxK + 1];
    int bi[kGeoMaxK + 1];
    const int K1 = K + 1;
    for (int m = 0; m < M; ++m) {
        const float dm = d[(size_t)m * V + v];
        if (m < K1 || geo_ranks_before(dm, bd[K1 - 1])) {                   // strict: an equal distance keeps the earlier (lower) index ahead
            int k = m < K1 ? m : K1 - 1;
            while (k > 0 && geo_ranks_before(dm, bd[k - 1])) { bd[k] = bd[k - 1]; bi[k] = bi[k - 1]; --k; }
            bd[k] = dm;
            bi[k] = m;
        }
    }
    const float px = verts[3 * (size_t)v], py = verts[3 * (size_t)v + 1], pz = verts[3 * (size_t)v + 2];
    float e[kGeoMaxK + 1];
    for (int k = 0; k < K1; ++k) {
        const int m = bi[k];
        const float dx = px - node_xyz[3 * (size_t)m], dy = py - node_xyz[3 * (size_t)m + 1], dz = pz - node_xyz[3 * (size_t)m + 2];
        e[k] = sqrtf((dx * dx + dy * dy) + dz * dz);
    }
    float w[kGeoMaxK], sum = 0.f;
    for (int k = 0; k < K; ++k) {
        const float t = 1.0f - e[k] / e[K];
        w[k] = t * t;
        sum += w[k];
    }
    // all K + 1 nodes equidistant or on the vertex: the uniform row where the reference's formula gives NaN
    const bool ok = e[K] > 0.f && sum > 0.f && sum <= 3.4028234e38f;
    const float uniform = 1.0f / (float)K;
    for (int k = 0; k < K; ++k) {
        idx[(size_t)v * K + k] = bi[k];
        weights[(size_t)v * K + k] = ok ? w[k] / sum : uniform;
    }
}

}  // namespace dm4d

using namespace dm4d;

extern "C" {

size_t dm4d_graph_geodesic_scratch_bytes(int32_t V, int32_t M) { return (size_t)(V > 0 ? V : 1) * (M > 0 ? M : 1) * 4 + 256; }

int dm4d_graph_geodesic_knn(int32_t V, int32_t M, int32_t K, const int32_t *csr_offsets, const int32_t *neighbors,
                            const float *edge_lengths, const float *verts, const float *node_xyz, const int32_t *node_vertex,
                            void *scratch, int64_t *neighbor_idx, float *neighbor_weights, dm4d_stream_t stream)
{
    if (V <= 0 || M <= 0 || K <= 0 || K > kGeoMaxK || K + 1 > M) {
        set_error("graph: need V > 0, M > K > 0, K <= %d (V %d, M %d, K %d)", kGeoMaxK, V, M, K);
        return DM4D_ERR_INVALID;
    }
    if (!csr_offsets || !neighbors || !edge_lengths || !verts || !node_xyz || !node_vertex || !scratch || !neighbor_idx || !neighbor_weights) {
        set_error("graph: null tensor");
        return DM4D_ERR_INVALID;
    }
    hipStream_t st = (hipStream_t)stream;
    float *d = (float *)scratch;
    int32_t *flag = (int32_t *)((char *)scratch + (size_t)V * M * 4);
    const dim3 grid((V + 255) / 256, M);
    hipLaunchKernelGGL(k_geo_init, grid, dim3(256), 0, st, V, M, node_vertex, d);
    DM4D_HIP_CHECK(hipGetLastError());
    // relax until a whole batch of sweeps changes nothing (a sweep moves information at least one edge; in-place
    // updates usually much further)
    const int kBatch = 16;
    for (int it = 0; it < V + kBatch; it += kBatch) {
        DM4D_HIP_CHECK(hipMemsetAsync(flag, 0, 4, st));
        for (int s = 0; s < kBatch; ++s) {
            hipLaunchKernelGGL(k_geo_relax, grid, dim3(256), 0, st, V, M, csr_offsets, neighbors, edge_lengths, d, flag);
            DM4D_HIP_CHECK(hipGetLastError());
        }
        int32_t h = 0;
        DM4D_HIP_CHECK(hipMemcpyAsync(&h, flag, 4, hipMemcpyDeviceToHost, st));
        DM4D_HIP_CHECK(hipStreamSynchronize(st));
        if (!h) break;
    }
    hipLaunchKernelGGL(k_geo_select, dim3((V + 255) / 256), dim3(256), 0, st, V, M, K, (const float *)d, verts, node_xyz, neighbor_idx,
                       neighbor_weights);
    DM4D_HIP_CHECK(hipGetLastError());
    return DM4D_OK;
}

}  // extern "C"
