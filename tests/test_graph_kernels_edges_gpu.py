"""GPU: the graph-build kernels (csrc/heat.hip: k_cg_*, k_heat_face_dirs, k_graph_select; csrc/graph.hip: k_geo_*) one entry point
at a time against the restatements of tests/graph_kernels_edges.py (pinned on the CPU by test_graph_kernels_edges_cpu.py).

* dm4d_cg_batched_f64: X, the iteration count and final_rel_residual BIT FOR BIT against the float64 restatement in the kernels'
  own summation order, at max_iter 1, 7, 25 with check_every 1, 10; V = 1 ... 130 (partial 32-row blocks), S = 1 ... 257 (partial
  64-column blocks, two workgroups of k_cg_reduce / k_cg_roll); zero, finished, early-converged and warm-started columns; columns
  solved alone; converged runs judged by their TRUE residual; the refusals.
* dm4d_heat_face_directions: per component within 4 x 2^-53 (sum |u_k| |g_k|) / |grad| + 4 x 2^-52 of a longdouble reference, the
  far field (1e-300 ... 1) included, exact zeros for a constant, the bytes around the output untouched.
* dm4d_graph_select_knn: the stable argsort on EVERY row (ties, NaN, inf, >= 1e300, ld > S, first_vertex > 0), weights within
  4 x WEIGHT_YARD + 4 x 2^-23 |ref|, degenerate rows uniform, never an index outside [0, M) or a non-finite weight.
* dm4d_graph_geodesic_knn: the [M][V] distance table BIT FOR BIT against the float32 fixed point; indices and weights as above.
Every test prints its worst error / bound.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import graph_kernels_edges as ec

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _dev(a, dev, dtype):
    return torch.as_tensor(np.array(a, order="C"), dtype=dtype, device=dev).contiguous()        # (a copy: the cases are read-only)


# ------------------------------------------------------------------------------------------------ conjugate gradients
def _cg(dev, inp, max_iter, tol, check_every, columns=None, raw=False, B=None):
    """-> (X numpy, return value, final_rel_residual); raw: the bare return code, no exception."""
    from dreammesh4d_amd import _lib

    Bn = inp["B"] if B is None else B
    X0 = inp["X0"]
    if columns is not None:
        Bn, X0 = Bn[:, columns], X0[:, columns]
    V, S = Bn.shape
    off, col = _dev(inp["off"], dev, torch.int32), _dev(inp["col"], dev, torch.int32)
    val, dinv = _dev(inp["val"], dev, torch.float64), _dev(inp["dinv"], dev, torch.float64)
    Bt, X = _dev(Bn, dev, torch.float64), _dev(X0, dev, torch.float64).clone()
    L = _lib.lib()
    scratch = torch.empty(L.dm4d_cg_batched_scratch_bytes(V, S), dtype=torch.uint8, device=dev)
    rel = C.c_double(-1.0)
    args = (V, S, off.data_ptr(), col.data_ptr(), val.data_ptr(), dinv.data_ptr(), Bt.data_ptr(), X.data_ptr(), scratch.data_ptr(), max_iter, tol,
            check_every, C.byref(rel), _lib.stream(dev))
    it = L.dm4d_cg_batched_f64(*args) if raw else _lib.call("dm4d_cg_batched_f64", *args)
    torch.cuda.synchronize()
    return X.cpu().numpy(), it, rel.value


@pytest.mark.parametrize("name", [c.name for c in ec.CG_CASES])
def test_cg_fixed_iteration_counts_bit_for_bit(name):
    dev = _need_gpu()
    inp = ec.cg_inputs(name)
    msgs = []
    for n, ce in ec.CG_FIXED:
        X, it, rel = _cg(dev, inp, n, ec.CG_FIXED_TOL, ce)
        msgs += ec.compare_cg_fixed(name, n, ce, X, it, rel)
        ref = ec.cg_fixed_reference(name, n, ce)
        assert it == n or (ec.CG_BY_NAME[name].V == 1 and ref.iters == it)        # max_iter binds (1 x 1: solved exactly, stops at a look)
        X2, it2, rel2 = _cg(dev, inp, n, ec.CG_FIXED_TOL, ce)                     # determinism
        assert ec.same_bits(X, X2) and it == it2 and rel == rel2
        for s, kind in enumerate(inp["kinds"]):
            if kind == "zero":
                assert not X[:, s].any()
            if kind == "exact":
                assert np.array_equal(X[:, s], inp["X0"][:, s])
    print(f"{name}: {len(ec.CG_FIXED)} fixed runs, {len(msgs)} complaints")
    assert not msgs, "\n".join(msgs)


def test_cg_columns_are_independent_of_their_neighbours():
    dev = _need_gpu()
    name = "spd-V130-S130"
    inp = ec.cg_inputs(name)
    full, it, _ = _cg(dev, inp, 25, ec.CG_FIXED_TOL, 10)
    assert it == 25
    for s in (0, 1, 2, 3, 4, 63, 64, 129):
        alone, it1, _ = _cg(dev, inp, 25, ec.CG_FIXED_TOL, 10, columns=[s])
        assert ec.same_bits(alone[:, 0], full[:, s]), f"column {s} ({inp['kinds'][s]})"


@pytest.mark.parametrize("name", [c.name for c in ec.CG_CASES])
def test_cg_converged_runs_by_their_true_residual(name):
    dev = _need_gpu()
    inp = ec.cg_inputs(name)
    msgs, worst = [], -np.inf
    for tol, ce in ec.CG_CONVERGED:
        X, it, rel = _cg(dev, inp, ec.CG_CONVERGED_MAX_ITER, tol, ce)
        m, over = ec.compare_cg_converged(name, tol, ce, X, it, rel)
        msgs += m
        worst = max(worst, over)
        ref = ec.cg_converged_reference(name, tol, ce)
        print(f"{name} tol={tol}: {it} iterations (restatement {ref.iters}), |r|/|b| {rel:.3e}, worst (true residual - tol) / R {over:.3f}, "
              f"same bits as the restatement: {ec.same_bits(X, ref.X)}")
    assert not msgs, "\n".join(msgs)
    assert worst <= 1.0


def test_cg_refusals_and_the_nan_message():
    dev = _need_gpu()
    from dreammesh4d_amd import _lib

    L = _lib.lib()
    inp = ec.cg_inputs("spd-V33-S65")
    V, S = inp["B"].shape
    # more than 65,536 right-hand sides: unsupported, with a message, nothing launched
    one = ec.cg_inputs("spd-V1-S1")
    wide = dict(one, B=np.ones((1, 65537)), X0=np.zeros((1, 65537)))
    X, rc, _ = _cg(dev, wide, 5, 1e-10, 1, raw=True)
    assert rc == _lib.DM4D_ERR_UNSUPPORTED and b"65536" in L.dm4d_last_error() and not X.any()
    X, rc, _ = _cg(dev, dict(one, B=np.ones((1, 65536)), X0=np.zeros((1, 65536))), 5, 1e-10, 1, raw=True)
    assert rc >= 1 and np.abs(X * one["A"][0, 0] - 1.0).max() < 1e-15
    # max_iter = 0, tol = 0, check_every = 0, null pointers: invalid
    for n, tol, ce in ((0, 1e-10, 1), (5, 0.0, 1), (5, float("nan"), 1), (5, 1e-10, 0)):
        assert _cg(dev, inp, n, tol, ce, raw=True)[1] == _lib.DM4D_ERR_INVALID and L.dm4d_last_error()
    t = torch.zeros(V * S + 64, dtype=torch.float64, device=dev)
    good = [V, S, t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), 5, 1e-10, 1, None, _lib.stream(dev)]
    for k in range(2, 9):
        args = list(good)
        args[k] = None
        assert L.dm4d_cg_batched_f64(*args) == _lib.DM4D_ERR_INVALID and b"null" in L.dm4d_last_error()
    assert L.dm4d_cg_batched_f64(0, S, *good[2:]) == _lib.DM4D_ERR_INVALID and L.dm4d_cg_batched_f64(V, 0, *good[2:]) == _lib.DM4D_ERR_INVALID
    # a NaN in B: invalid, and the message says NaN -- wherever the column sits (its workgroup's maximum must not drop it)
    for s in (0, 40, 64):
        B = inp["B"].copy()
        B[5, s] = np.nan
        _, rc, _ = _cg(dev, inp, 20, 1e-10, 5, raw=True, B=B)
        assert rc == _lib.DM4D_ERR_INVALID and b"NaN" in L.dm4d_last_error(), (s, rc)
    X, it, rel = _cg(dev, inp, 20, 1e-10, 5)                    # ... and the library is as usable as before
    assert not ec.compare_cg_fixed("spd-V33-S65", 7, 10, *_cg(dev, inp, 7, ec.CG_FIXED_TOL, 10))


# ------------------------------------------------------------------------------------------------ face directions
@pytest.mark.parametrize("name", [c.name for c in ec.DIR_CASES])
def test_face_directions_against_longdouble(name):
    dev = _need_gpu()
    from dreammesh4d_amd import _lib

    c, inp = ec.DIR_BY_NAME[name], ec.dir_inputs(name)
    faces, G, U = _dev(inp["faces"], dev, torch.int32), _dev(inp["G"], dev, torch.float64), _dev(inp["U"], dev, torch.float64)
    buf = torch.full((2 * ec.DIR_PAD + 3 * c.F * c.S,), ec.DIR_SENTINEL, dtype=torch.float64, device=dev)
    out = buf[ec.DIR_PAD:]
    _lib.call("dm4d_heat_face_directions", c.F, c.S, faces.data_ptr(), G.data_ptr(), U.data_ptr(), out.data_ptr(), _lib.stream(dev))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    msgs, worst = ec.compare_dirs(name, got)
    print(f"{name}: worst |error| / bound {worst:.4f}; same bits as the float64 restatement: {ec.same_bits(got, ec.dir_restatement(name))}")
    assert not msgs, "\n".join(msgs)
    L = _lib.lib()
    for F_, S_ in ((0, c.S), (c.F, 0), (-1, c.S)):
        assert L.dm4d_heat_face_directions(F_, S_, faces.data_ptr(), G.data_ptr(), U.data_ptr(), out.data_ptr(), _lib.stream(dev)) == _lib.DM4D_ERR_INVALID
    assert L.dm4d_heat_face_directions(c.F, c.S, faces.data_ptr(), None, U.data_ptr(), out.data_ptr(), _lib.stream(dev)) == _lib.DM4D_ERR_INVALID


# ------------------------------------------------------------------------------------------------ selection and weights
def _select(dev, name):
    from dreammesh4d_amd import _lib

    c, inp = ec.SEL_BY_NAME[name], ec.sel_inputs(name)
    score = _dev(inp["score"], dev, torch.float64)
    verts, nodes = _dev(inp["verts"], dev, torch.float32), _dev(inp["nodes"], dev, torch.float32)
    idx = torch.full((c.Vtot, c.K), ec.SENT_IDX, dtype=torch.int64, device=dev)
    w = torch.full((c.Vtot, c.K), ec.SENT_W, dtype=torch.float32, device=dev)
    _lib.call("dm4d_graph_select_knn", c.S, c.M, c.K, score.data_ptr(), c.ld, c.v0, verts.data_ptr(), nodes.data_ptr(), idx.data_ptr(), w.data_ptr(),
              _lib.stream(dev))
    torch.cuda.synchronize()
    return idx.cpu().numpy(), w.cpu().numpy()


@pytest.mark.parametrize("name", [c.name for c in ec.SEL_CASES])
def test_select_knn_is_the_stable_argsort_on_every_row(name):
    dev = _need_gpu()
    idx, w = _select(dev, name)
    msgs, worst = ec.compare_select(name, idx, w)
    print(f"{name}: worst weight |error| / bound {worst:.4f}")
    assert not msgs, "\n".join(msgs)
    idx2, w2 = _select(dev, name)
    assert np.array_equal(idx, idx2) and ec.same_bits(w, w2)


def test_select_knn_refusals():
    dev = _need_gpu()
    from dreammesh4d_amd import _lib

    L = _lib.lib()
    t = torch.zeros(4096, dtype=torch.float64, device=dev)
    p, st = t.data_ptr(), _lib.stream(dev)
    call = lambda S, M, K, ld, v0, score=p: L.dm4d_graph_select_knn(S, M, K, score, ld, v0, p, p, p, p, st)
    for bad in ((0, 5, 4, 8, 0), (8, 4, 4, 8, 0), (8, 18, 17, 8, 0), (8, 5, 0, 8, 0), (8, 5, 4, 7, 0), (8, 5, 4, 8, -1)):
        assert call(*bad) == _lib.DM4D_ERR_INVALID and L.dm4d_last_error(), bad
    assert call(8, 5, 4, 8, 0, None) == _lib.DM4D_ERR_INVALID


# ------------------------------------------------------------------------------------------------ edge paths
def _geodesic(dev, g, K=None, M=None, raw=False):
    from dreammesh4d_amd import _lib

    L = _lib.lib()
    V, M, K = g["V"], g["M"] if M is None else M, g["K"] if K is None else K
    off, nbr, ln = _dev(g["off"], dev, torch.int32), _dev(g["nbr"], dev, torch.int32), _dev(g["len"], dev, torch.float32)
    verts, nodes, nv = _dev(g["verts"], dev, torch.float32), _dev(g["nodes"], dev, torch.float32), _dev(g["node_vertex"], dev, torch.int32)
    scratch = torch.zeros(L.dm4d_graph_geodesic_scratch_bytes(V, M), dtype=torch.uint8, device=dev)
    idx = torch.full((V, max(K, 1)), ec.SENT_IDX, dtype=torch.int64, device=dev)
    w = torch.full((V, max(K, 1)), ec.SENT_W, dtype=torch.float32, device=dev)
    args = (V, M, K, off.data_ptr(), nbr.data_ptr(), ln.data_ptr(), verts.data_ptr(), nodes.data_ptr(), nv.data_ptr(), scratch.data_ptr(), idx.data_ptr(),
            w.data_ptr(), _lib.stream(dev))
    rc = L.dm4d_graph_geodesic_knn(*args) if raw else _lib.call("dm4d_graph_geodesic_knn", *args)
    torch.cuda.synchronize()
    table = scratch[:V * M * 4].view(torch.float32).reshape(M, V).cpu().numpy()
    return rc, table, idx.cpu().numpy(), w.cpu().numpy()


@pytest.mark.parametrize("name", [c.name for c in ec.GEO_CASES])
def test_geodesic_table_bit_for_bit_and_its_selection(name):
    dev = _need_gpu()
    g = ec.geo_inputs(name)
    _, table, idx, w = _geodesic(dev, g)
    msgs, worst = ec.compare_geo(name, table, idx, w)
    print(f"{name}: table bit-identical {ec.same_bits(table, ec.relax_fixed_point(name)[0])}, worst weight |error| / bound {worst:.4f}")
    assert not msgs, "\n".join(msgs)
    _, table2, idx2, w2 = _geodesic(dev, g)
    assert ec.same_bits(table, table2) and np.array_equal(idx, idx2) and ec.same_bits(w, w2)


def test_geodesic_refusals_write_nothing():
    dev = _need_gpu()
    from dreammesh4d_amd import _lib

    g = ec.geo_inputs("geo-K16-M17")
    for K, M in ((17, 17), (16, 16), (0, 17), (4, 4)):          # K = 17; M == K
        rc, table, idx, w = _geodesic(dev, g, K=K, M=M, raw=True)
        assert rc == _lib.DM4D_ERR_INVALID and _lib.lib().dm4d_last_error()
        assert not table.any() and (idx == ec.SENT_IDX).all() and (w == np.float32(ec.SENT_W)).all()
