"""The numpy restatement of knn_points (tests/knn_points_common.py) against scipy's cKDTree in float64, and one case worked by
hand.  No device."""
import numpy as np

from tests import knn_points_common as kc

K = 8
SEED = 0
EPS = 2.0 ** -24
# |float32 d2 - exact d2| <= D2_ROUNDING * d2: (1 + e)^2 on each difference, one rounding per square, two per sum -- at most
# 5 roundings of relative size EPS on a sum of non-negative terms; 8 leaves room for the second-order terms
D2_ROUNDING = 8 * EPS


def _compare(query, points, exclude_self):
    from scipy.spatial import cKDTree

    got_d, got_i = kc.knn_reference(query, points, K, exclude_self=exclude_self)
    q64, p64 = query.astype(np.float64), points.astype(np.float64)
    extra = 2 if exclude_self else 1                    # the query itself comes back first, at distance 0
    _, nn = cKDTree(p64).query(q64, k=K + extra)
    if exclude_self:
        rows = np.arange(len(q64))
        assert np.array_equal(nn[:, 0], rows)           # no duplicates in a uniform cloud
        nn = nn[:, 1:]
    d64 = ((q64[:, None, :] - p64[nn]) ** 2).sum(-1)    # exact differences of float32 values, [Nq, K + 1], ascending
    # a row is decided when neighbouring distances differ by more than both can be off in float32 (tests/test_oracle_raster.py
    # guards its decision boundaries the same way)
    decided = (np.diff(d64, axis=1) > 2 * D2_ROUNDING * d64[:, 1:]).all(axis=1)
    left_out = int((~decided).sum())
    print(f"knn restatement vs cKDTree: {left_out} of {len(q64)} rows within float32 rounding of a tie (left out)")
    assert left_out <= 0.01 * len(q64)
    assert np.array_equal(got_i[decided], nn[decided, :K])
    assert (np.abs(got_d[decided].astype(np.float64) - d64[decided, :K]) <= D2_ROUNDING * d64[decided, :K]).all()
    assert (np.diff(got_d.astype(np.float64), axis=1) >= 0).all()


def test_restatement_matches_ckdtree_self_search():
    pts = np.random.default_rng(SEED).random((2000, 3)).astype(np.float32)
    _compare(pts, pts, exclude_self=True)


def test_restatement_matches_ckdtree_other_queries():
    rng = np.random.default_rng(SEED + 1)
    pts = rng.random((2000, 3)).astype(np.float32)
    query = (rng.random((500, 3)) * 1.4 - 0.2).astype(np.float32)        # some outside the cloud's bounds
    _compare(query, pts, exclude_self=False)


def test_unit_lattice_centre_by_hand():
    """3 x 3 x 3 unit lattice, index = 9 x + 3 y + z, query at the centre (1, 1, 1) = index 13: itself at d2 = 0, the 6 face
    neighbours at d2 = 1 by ascending index, then the 12 edge neighbours at d2 = 2 by ascending index."""
    pts = kc.lattice(3)
    assert np.array_equal(pts[13], [1, 1, 1])
    faces = [4, 10, 12, 14, 16, 22]
    edges = [1, 3, 5, 7, 9, 11, 15, 17, 19, 21, 23, 25]
    d, i = kc.knn_reference(pts[13:14], pts, 19)
    assert i[0].tolist() == [13] + faces + edges
    assert d[0].tolist() == [0.0] + [1.0] * 6 + [2.0] * 12
    d, i = kc.knn_reference(pts, pts, 18, exclude_self=True)
    assert i[13].tolist() == faces + edges
    assert d[13].tolist() == [1.0] * 6 + [2.0] * 12
    # a corner: 3 face, 3 edge neighbours, then the body diagonal
    assert i[0, :7].tolist() == [1, 3, 9, 4, 10, 12, 13] and d[0, :7].tolist() == [1, 1, 1, 2, 2, 2, 3]
