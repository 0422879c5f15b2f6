"""dm4d_knn_points / dreammesh4d_amd.knn.knn_points on the device against the numpy restatement of its contract
(tests/knn_points_common.py): every comparison is exact, on distances and indices, for the exhaustive search and for the box
search separately."""
import functools

import numpy as np
import pytest
import torch

from tests import knn_points_common as kc

pytestmark = pytest.mark.gpu
METHODS = ("brute", "boxes")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _run(query, points, K, method, exclude_self=False, same=False):
    from dreammesh4d_amd.knn import knn_points

    p = torch.from_numpy(np.ascontiguousarray(points, np.float32)).to("cuda:0")
    q = p if same else torch.from_numpy(np.ascontiguousarray(query, np.float32)).to("cuda:0")
    out = knn_points(q, p, K, exclude_self=exclude_self, method=method)
    return out.dists.cpu().numpy(), out.idx.cpu().numpy()


def _assert_same(got, want, what):
    (gd, gi), (wd, wi) = got, want
    assert gd.dtype == np.float32 and gi.dtype == np.int64
    bad = np.flatnonzero((gi != wi).any(axis=1) | (gd.view(np.uint32) != wd.view(np.uint32)).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} rows differ, first {bad[0]}: got {gi[bad[0]]} {gd[bad[0]]}, want {wi[bad[0]]} {wd[bad[0]]}"
    assert np.array_equal(gi, wi) and np.array_equal(gd, wd)


# ------------------------------------------------------------------------------------------------ random clouds
@functools.lru_cache(maxsize=None)
def _random_case():
    rng = np.random.default_rng(11)
    pts = rng.normal(size=(3000, 3)).astype(np.float32)
    query = rng.normal(size=(1000, 3)).astype(np.float32)
    query[::7] *= 6.0                                  # well outside the cloud
    query[3::50] += np.float32(40.0)                   # and far outside its bounding box
    return query, pts, kc.knn_reference(query, pts, 32)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("K", [1, 3, 8, 16, 32])
def test_random_clouds(K, method):
    _need_gpu()
    query, pts, (wd, wi) = _random_case()
    _assert_same(_run(query, pts, K, method), (wd[:, :K].copy(), wi[:, :K].copy()), f"K={K} {method}")


# ------------------------------------------------------------------------------------------------ self search
@functools.lru_cache(maxsize=None)
def _self_case(N):
    pts = np.random.default_rng(100 + N).random((N, 3)).astype(np.float32)
    return pts, kc.knn_reference(pts, pts, 8, exclude_self=True)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("N", [63, 64, 65, 1023, 1024, 1025, 2049])
def test_self_search_at_wave_and_box_edges(N, method):
    _need_gpu()
    pts, want = _self_case(N)
    _assert_same(_run(None, pts, 8, method, exclude_self=True, same=True), want, f"N={N} {method}")
    # the same cloud as two arrays: the queries are sorted on their own
    _assert_same(_run(pts, pts, 8, method, exclude_self=True), want, f"N={N} {method}, separate arrays")


# ------------------------------------------------------------------------------------------------ exact ties
@functools.lru_cache(maxsize=None)
def _lattice_case(shuffled):
    pts = kc.lattice(12)
    if shuffled:
        pts = pts[np.random.default_rng(5).permutation(len(pts))]
    return pts, kc.knn_reference(pts, pts, 27, exclude_self=True)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("K", [7, 27])
def test_integer_lattice(K, shuffled, method):
    """Ties everywhere: the 7th neighbour of an inner point is one of 12 at d2 = 2, and which one is the index rule's to say.
    A box pruned at `bound >= k-th best` instead of `>` loses the lower index here."""
    _need_gpu()
    pts, (wd, wi) = _lattice_case(shuffled)
    _assert_same(_run(None, pts, K, method, exclude_self=True, same=True), (wd[:, :K].copy(), wi[:, :K].copy()), f"K={K} {method}")


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("low_side", [-1.0, 1.0])
@pytest.mark.parametrize("K", [1, 3])
def test_tie_between_two_boxes(K, low_side, method):
    """Two slabs of 1024 points at z = -1 and z = +1 (z's top bit leads the Morton key: each slab is exactly one box), queries at
    the origin.  Each slab holds `K` copies of (0, 0, z) at d2 = 1, the rest is farther; both boxes' lower bound is exactly 1.
    Whichever box a wave searches first leaves its K-th best at exactly 1, the other box's bound EQUALS it, and the copies with
    the lower indices sit in one slab or the other (`low_side`): a search that skips a box at `bound >= best` returns the
    wrong indices for one of the two sides."""
    _need_gpu()
    rng = np.random.default_rng(17)

    def slab(z):
        xy = rng.uniform(0.25, 0.5, size=(1024, 2)) * rng.choice([-1.0, 1.0], size=(1024, 2))
        xy[:K] = 0.0
        return np.concatenate([xy, np.full((1024, 1), z)], axis=1).astype(np.float32)

    pts = np.concatenate([slab(low_side), slab(-low_side)])
    query = np.zeros((3, 3), np.float32)
    want = kc.knn_reference(query, pts, K)
    assert want[1][0].tolist() == list(range(K)) and (want[0] == 1.0).all()
    _assert_same(_run(query, pts, K, method), want, f"K={K} low indices at z={low_side} {method}")


@pytest.mark.parametrize("method", METHODS)
def test_duplicates(method):
    _need_gpu()
    half = np.random.default_rng(3).random((700, 3)).astype(np.float32)
    pts = np.concatenate([half, half])
    d, i = _run(None, pts, 1, method, exclude_self=True, same=True)
    assert np.array_equal(i[:, 0], (np.arange(1400) + 700) % 1400) and np.array_equal(d, np.zeros((1400, 1), np.float32))


@pytest.mark.parametrize("method", METHODS)
def test_degenerate_clouds(method):
    _need_gpu()
    same = np.tile(np.asarray([[0.25, -1.5, 3.0]], np.float32), (300, 1))          # zero-extent bounds
    _assert_same(_run(None, same, 5, method, exclude_self=True, same=True), kc.knn_reference(same, same, 5, exclude_self=True), "identical")
    _assert_same(_run(same[:10], same, 5, method), kc.knn_reference(same[:10], same, 5), "identical, queries")
    rng = np.random.default_rng(8)
    cluster = (1e-3 * rng.normal(size=(1500, 3))).astype(np.float32)
    far = np.concatenate([cluster[:700], np.asarray([[1e4, 0, 0]], np.float32), cluster[700:]])
    want = kc.knn_reference(far, far, 8, exclude_self=True)
    assert want[0][700].min() > 9e7                                                  # the far point's neighbours are the cluster
    _assert_same(_run(None, far, 8, method, exclude_self=True, same=True), want, "cluster and a far point")


@pytest.mark.parametrize("method", METHODS)
def test_k_at_the_limit(method):
    _need_gpu()
    rng = np.random.default_rng(9)
    pts, query = rng.random((20, 3)).astype(np.float32), rng.random((50, 3)).astype(np.float32)
    _assert_same(_run(query, pts, 20, method), kc.knn_reference(query, pts, 20), "K == Np")
    _assert_same(_run(None, pts, 19, method, exclude_self=True, same=True), kc.knn_reference(pts, pts, 19, exclude_self=True), "K == Np - 1")
    pts32 = rng.random((33, 3)).astype(np.float32)
    _assert_same(_run(None, pts32, 32, method, exclude_self=True, same=True), kc.knn_reference(pts32, pts32, 32, exclude_self=True), "K == 32 == Np - 1")


def test_methods_agree_and_repeat():
    _need_gpu()
    from dreammesh4d_amd.knn import knn_points

    g = torch.Generator().manual_seed(2)
    p = torch.randn(5000, 3, generator=g).to("cuda:0")
    q = torch.randn(777, 3, generator=g).to("cuda:0")
    for a1, a2, kw in ((q, p, {}), (p, p, dict(exclude_self=True))):
        b1, x1, x2 = knn_points(a1, a2, 16, method="brute", **kw), knn_points(a1, a2, 16, method="boxes", **kw), knn_points(a1, a2, 16, method="boxes", **kw)
        b2 = knn_points(a1, a2, 16, method="brute", **kw)
        assert torch.equal(b1.dists, x1.dists) and torch.equal(b1.idx, x1.idx)
        assert torch.equal(x1.dists, x2.dists) and torch.equal(x1.idx, x2.idx)
        assert torch.equal(b1.dists, b2.dists) and torch.equal(b1.idx, b2.idx)


def test_shapes_fields_and_auto():
    _need_gpu()
    from dreammesh4d_amd import knn

    query, pts, (wd, wi) = _random_case()
    q, p = torch.from_numpy(query).to("cuda:0"), torch.from_numpy(pts).to("cuda:0")
    flat = knn.knn_points(q, p, 8, method="brute")
    assert isinstance(flat, knn.KNN) and flat._fields == ("dists", "idx")
    assert flat.dists.shape == (1000, 8) and flat.idx.shape == (1000, 8) and flat.idx.dtype == torch.int64 and flat.dists.dtype == torch.float32
    assert not flat.dists.requires_grad
    one = knn.knn_points(q[None].requires_grad_(True), p[None], 8)               # the reference's call form; "auto"
    assert one.dists.shape == (1, 1000, 8) and one.idx.shape == (1, 1000, 8) and not one.dists.requires_grad
    for m in METHODS:
        forced = knn.knn_points(q[None], p[None], 8, method=m)
        assert torch.equal(one.dists, forced.dists) and torch.equal(one.idx, forced.idx)
    assert np.array_equal(one.dists[0].cpu().numpy(), wd[:, :8]) and np.array_equal(one.idx[0].cpu().numpy(), wi[:, :8])
    # a batch of two different clouds, and the reference's self call x[None], x[None]
    two_q, two_p = torch.stack([q, q.flip(0)]), torch.stack([p, p * 2.0])
    two = knn.knn_points(two_q, two_p, 3, method="boxes")
    second = knn.knn_points(q.flip(0), p * 2.0, 3, method="brute")
    assert torch.equal(two.dists[0], flat.dists[:, :3]) and torch.equal(two.idx[1], second.idx) and torch.equal(two.dists[1], second.dists)
    x = p[None]
    s = knn.knn_points(x, x, K=4)
    assert torch.equal(s.idx[0, :, 0].cpu(), torch.arange(3000)) and float(s.dists[0, :, 0].abs().max()) == 0.0
    # auto crosses over by the number of pairs: force the boxes side at a small size
    old = knn.BRUTE_FORCE_MAX_PAIRS
    try:
        knn.BRUTE_FORCE_MAX_PAIRS = 1000
        auto = knn.knn_points(q, p, 8)
    finally:
        knn.BRUTE_FORCE_MAX_PAIRS = old
    assert torch.equal(auto.dists, flat.dists) and torch.equal(auto.idx, flat.idx)


def test_errors():
    _need_gpu()
    from dreammesh4d_amd import _lib
    from dreammesh4d_amd.knn import knn_points

    p = torch.rand(40, 3, device="cuda:0")
    q = torch.rand(10, 3, device="cuda:0")
    for bad_k in (0, 33, 41):
        with pytest.raises(ValueError):
            knn_points(q, p, bad_k)
    with pytest.raises(ValueError):
        knn_points(p, p, 40, exclude_self=True)                 # 39 candidates
    knn_points(p, p, 32, exclude_self=True)
    with pytest.raises(_lib.Dm4dError):
        knn_points(q.cpu(), p.cpu(), 3)
    with pytest.raises(_lib.Dm4dError):
        knn_points(q, p.cpu(), 3)
    for a, b in ((q[:, :2], p), (q, p[None]), (q[None], torch.stack([p, p])), (q.reshape(-1), p), (q[None, None], p[None, None])):
        with pytest.raises(ValueError):
            knn_points(a, b, 3)
    with pytest.raises(ValueError):
        knn_points(q, p, 3, method="kdtree")
    # the C call refuses the same K's and writes nothing
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    for method in (0, 1):
        nbytes = L.dm4d_knn_points_scratch_bytes(10, 40, 8, method)
        assert (nbytes == 0) == (method == 0)
        scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda:0")
        for K, excl, n_pts in ((0, 0, 40), (33, 0, 40), (-1, 0, 40), (9, 0, 8), (8, 1, 8)):
            d = torch.full((10, 33), -7.0, device="cuda:0")
            i = torch.full((10, 33), -7, dtype=torch.int32, device="cuda:0")
            rc = L.dm4d_knn_points(10, n_pts, K, q.data_ptr(), p.data_ptr(), excl, method, scratch.data_ptr(), nbytes, d.data_ptr(), i.data_ptr(), st)
            torch.cuda.synchronize()
            assert rc == -1, (K, excl, n_pts, method)                       # DM4D_ERR_INVALID
            assert bool((d == -7.0).all()) and bool((i == -7).all())
    with pytest.raises(_lib.Dm4dError):
        _lib.call("dm4d_knn_points", 10, 40, 8, q.data_ptr(), p.data_ptr(), 0, 2, None, 0, d.data_ptr(), i.data_ptr(), st)
    rc = L.dm4d_knn_points(10, 40, 8, q.data_ptr(), p.data_ptr(), 0, 1, None, 0, d.data_ptr(), i.data_ptr(), st)
    assert rc == -3 and bool((i == -7).all())                                # DM4D_ERR_CAPACITY: no scratch given
