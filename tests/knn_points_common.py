"""The contract of knn_points restated in numpy, for the CPU and GPU tests (written from the contract, not from the kernel):

    d2 = (dx*dx + dy*dy) + dz*dz      float32, elementwise, in this order, dx = q.x - p.x
    a query's results = the first K candidates under np.lexsort((index, d2)): ascending d2, ties to the lower index
    exclude_self: candidate j is no candidate of query i when j == i (a duplicate of the point still is one)
"""
import numpy as np


def dist2_matrix(query, points):
    """[Nq,Np] float32: every operation is one float32 numpy ufunc call, so nothing is contracted into an FMA."""
    q, p = np.ascontiguousarray(query, np.float32), np.ascontiguousarray(points, np.float32)
    dx = q[:, None, 0] - p[None, :, 0]
    dy = q[:, None, 1] - p[None, :, 1]
    dz = q[:, None, 2] - p[None, :, 2]
    d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == np.float32
    return d2


def knn_reference(query, points, K, exclude_self=False):
    """-> (dist2 [Nq,K] float32, idx [Nq,K] int64)."""
    d2 = dist2_matrix(query, points)
    nq, npts = d2.shape
    index = np.arange(npts, dtype=np.int64)
    out_d, out_i = np.empty((nq, K), np.float32), np.empty((nq, K), np.int64)
    for i in range(nq):
        cand = index[index != i] if exclude_self else index
        row = d2[i, cand]
        first = np.lexsort((cand, row))[:K]
        assert len(first) == K, "K exceeds the number of candidates"
        out_d[i], out_i[i] = row[first], cand[first]
    return out_d, out_i


def lattice(n):
    """n x n x n integer lattice with spacing 1, float32 [n^3,3]; index = (x * n + y) * n + z."""
    g = np.arange(n, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
