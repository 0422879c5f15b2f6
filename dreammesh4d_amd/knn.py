"""Exact k-nearest-neighbour search with indices on the HIP device (csrc/knn.hip, C ABI ``dm4d_knn_points``): the reference's
``pytorch3d.ops.knn_points`` (geometry/sugar.py:636, system/base.py:349, utils/sugar_utils.py) and open3d's
``KDTreeFlann.search_knn_vector_3d`` (utils/arap_utils.py:46-70, geometry/dynamic_sugar.py:762-812).

The result is unique: ``d2 = (dx*dx + dy*dy) + dz*dz`` in float32, the K smallest under the order (d2, index), ascending -- ties go
to the lower index (pytorch3d and FLANN leave the tie order open).  Two searches return the same bytes: an exhaustive one, and
Morton-ordered boxes of 1024 points with the queries sorted by the same key.  No CPU path.
"""
from collections import namedtuple

import torch

from . import _lib

KNN = namedtuple("KNN", ["dists", "idx"])        # pytorch3d's field names (its third field, `knn`, needs return_nn: not offered)

K_MAX = 32
# "auto": exhaustive up to this many (query, point) pairs, boxes above.  Measured on an MI355X (tools/knn_timing.py; DESIGN.md, kNN
# with indices): self searches cross over between 4 k and 16 k points at K = 16 and at 16 k points at K = 8; 12,000^2 lies between.
BRUTE_FORCE_MAX_PAIRS = 12000 * 12000
_METHODS = {"brute": 0, "boxes": 1}


def _knn_one(L, q, p, K, exclude, method, dists, idx32):
    dev = q.device
    nq, np_ = int(q.shape[0]), int(p.shape[0])
    with torch.cuda.device(dev):
        st = _lib.stream(dev)
        nbytes = int(L.dm4d_knn_points_scratch_bytes(nq, np_, K, method))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
        _lib.call("dm4d_knn_points", nq, np_, K, q.data_ptr(), p.data_ptr(), 1 if exclude else 0, method,
                  None if scratch is None else scratch.data_ptr(), nbytes, dists.data_ptr(), idx32.data_ptr(), st)


def knn_points(p1, p2, K, exclude_self=False, method="auto"):
    """For every point of ``p1`` its K nearest points of ``p2``: ``KNN(dists, idx)`` with ``dists`` float32 ``[..., N1, K]`` (SQUARED
    distances, ascending) and ``idx`` int64 ``[..., N1, K]`` into ``p2``.  ``p1`` / ``p2``: ``[N,3]``, or ``[B,N,3]`` with equal B (the
    reference's ``knn_points(x[None], x[None], K=k)``); ``lengths1`` / ``lengths2`` are not supported.  ``exclude_self``: candidate j
    is skipped for query i when j == i (a cloud searched in itself).  Outputs are detached.  ``method``: "auto" | "brute" | "boxes"."""
    if not (torch.is_tensor(p1) and torch.is_tensor(p2)):
        raise ValueError("knn_points: p1 and p2 must be tensors")
    if p1.dim() not in (2, 3) or p1.dim() != p2.dim() or p1.shape[-1] != 3 or p2.shape[-1] != 3:
        raise ValueError(f"knn_points: p1 and p2 must both be [N,3] or both [B,N,3], got {tuple(p1.shape)} and {tuple(p2.shape)}")
    if p1.dim() == 3 and p1.shape[0] != p2.shape[0]:
        raise ValueError(f"knn_points: batch sizes differ: {p1.shape[0]} and {p2.shape[0]}")
    if method != "auto" and method not in _METHODS:
        raise ValueError(f"knn_points: method must be 'auto', 'brute' or 'boxes', got {method!r}")
    K = int(K)
    n1, n2 = int(p1.shape[-2]), int(p2.shape[-2])
    candidates = n2 - (1 if exclude_self else 0)
    if not 1 <= K <= K_MAX or K > candidates:
        raise ValueError(f"knn_points: K = {K} outside 1 .. min({K_MAX}, {max(candidates, 0)} candidates); no padding convention is offered")
    if not (p1.is_cuda and p2.is_cuda):
        raise _lib.Dm4dError("knn_points runs on the HIP device (no CPU fallback in the product)")
    if p1.device != p2.device:
        raise ValueError(f"knn_points: p1 on {p1.device}, p2 on {p2.device}")
    L = _lib.lib()
    m = _METHODS[method] if method != "auto" else (0 if n1 * n2 <= BRUTE_FORCE_MAX_PAIRS else 1)
    same = p1 is p2 or (p1.data_ptr() == p2.data_ptr() and p1.shape == p2.shape and p1.stride() == p2.stride() and p1.dtype == p2.dtype)
    q = p1.detach().to(torch.float32).contiguous()
    p = q if same else p2.detach().to(torch.float32).contiguous()       # one array: the boxes method sorts it once
    batched = q.dim() == 3
    qb, pb = (q, p) if batched else (q[None], p[None])
    B = int(qb.shape[0])
    dists = torch.empty(B, n1, K, dtype=torch.float32, device=q.device)
    idx32 = torch.empty(B, n1, K, dtype=torch.int32, device=q.device)
    for b in range(B):
        _knn_one(L, qb[b], pb[b], K, exclude_self, m, dists[b], idx32[b])
    idx = idx32.to(torch.int64)
    return KNN(dists, idx) if batched else KNN(dists[0], idx[0])
