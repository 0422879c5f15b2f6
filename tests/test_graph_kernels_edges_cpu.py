"""Pins the restatements, the cases and the constants that tests/test_graph_kernels_edges_gpu.py judges the graph-build kernels by
(CPU only, no library call).

* The conjugate-gradient restatement (the kernels' own summation order) against np.linalg.solve and, for the singular path
  Laplacian, the pseudo-inverse; its two-stage dot product against a plain sum; columns solved alone give the same bits.
* The float32 relaxation fixed point against an exact float64 Dijkstra within V 2^-24 relative; unreachable entries stay 3.0e38.
* The float64 face-direction and float32 weight restatements against the longdouble / float64 references, through the very
  comparison functions the GPU test uses; CG_GAP and WEIGHT_YARD re-measured: 0.5 x constant <= measured <= constant.
* The case lists hold every class the kernels branch on.
* One-token mutants of the restatements, fed to those comparison functions in place of the device output: each is rejected.
"""
import numpy as np
import pytest

from tests import graph_kernels_edges as ec

CG_NAMES = [c.name for c in ec.CG_CASES]


# ------------------------------------------------------------------------------------------------ conjugate gradients
@pytest.mark.parametrize("name", CG_NAMES)
def test_cg_restatement_converges_to_the_direct_solution(name):
    inp = ec.cg_inputs(name)
    A = inp["A"]
    assert np.array_equal(A, A.T) and (np.diag(A) > 0).all()
    lam = np.linalg.eigvalsh(A)
    if inp["singular"]:
        assert abs(lam[0]) < 1e-12 and lam[1] > 1e-3 and np.abs(inp["B"].sum(0)).max() == 0.0      # consistent right-hand sides
        assert np.abs(ec.pinv_solution(name).astype(np.float64) - np.linalg.pinv(A) @ inp["B"]).max() < 1e-10
    else:
        assert lam[0] > 0 and lam[-1] / lam[0] < 1.5e3
    for tol, ce in ec.CG_CONVERGED:
        ref = ec.cg_converged_reference(name, tol, ce)
        msgs, over = ec.compare_cg_converged(name, tol, ce, ref.X, ref.iters, ref.rel)
        assert not msgs, "\n".join(msgs)
        assert ref.iters < ec.CG_CONVERGED_MAX_ITER and ref.rel <= tol
        if not inp["singular"]:
            want = np.linalg.solve(A, inp["B"])
            r = np.linalg.norm(inp["B"] - A @ ref.X, axis=0)
            assert (np.linalg.norm(ref.X - want, axis=0) <= r / lam[0] + 1e-14 * np.linalg.norm(want, axis=0)).all()
    # the eigenvector column is done after ONE step (to the float32 rounding of the vector), long before its neighbours
    if "eig" in inp["kinds"]:
        one = ec.cg_fixed_reference(name, 1, 1)
        res = ec.true_residual(inp, one.X)
        s = inp["kinds"].index("eig")
        assert res[s] < 1e-6 and np.median(res[[k == "random" for k in inp["kinds"]]]) > 1e-2


def test_cg_fixed_runs_bind_at_max_iter_and_restate_themselves():
    for name in CG_NAMES:
        for n, ce in ec.CG_FIXED:
            ref = ec.cg_fixed_reference(name, n, ce)
            # (the 1 x 1 system is solved exactly by the first step: a zero residual stops it at the next look)
            assert ref.iters == n or (ec.CG_BY_NAME[name].V == 1 and ref.rel == 0.0 and ref.iters == min(n, ce)), (name, n, ce, ref.iters)
            assert not ec.compare_cg_fixed(name, n, ce, ref.X.copy(), ref.iters, ref.rel)
            assert np.isfinite(ref.X).all()
    # check_every does not change the arithmetic
    assert ec.same_bits(ec.cg_fixed_reference("spd-V33-S65", 25, 1).X, ec.cg_fixed_reference("spd-V33-S65", 25, 10).X)


def test_cg_two_stage_dot_equals_a_plain_sum_and_columns_are_independent():
    rng = np.random.default_rng(0)
    for V in (1, 31, 32, 33, 65, 130):
        T = rng.normal(size=(V, 5))
        got = ec._col_dot(T, V)
        assert np.abs(got - T.sum(0)).max() <= 1e-14 * np.abs(T).sum(0).max()
    name = "spd-V130-S130"
    inp, full = ec.cg_inputs(name), ec.cg_fixed_reference(name, 25, 10)
    for s in (0, 1, 2, 3, 4, 64, 129):
        alone = ec.cg_restatement(inp, 25, ec.CG_FIXED_TOL, 10, columns=[s])
        assert ec.same_bits(alone.X[:, 0], full.X[:, s]), s


def test_cg_gap_is_remeasured():
    worst, where = 0.0, None
    for name in CG_NAMES:
        inp = ec.cg_inputs(name)
        for tol, ce in ec.CG_CONVERGED:
            ref = ec.cg_converged_reference(name, tol, ce)
            with np.errstate(divide="ignore", invalid="ignore"):
                rec = np.sqrt(np.where(ref.bb > 0, ref.rr / ref.bb, 0.0))
            gap = np.abs(ec.true_residual(inp, ref.X) - rec)
            if gap.max() > worst:
                worst, where = float(gap.max()), (name, tol, int(np.argmax(gap)), inp["kinds"][int(np.argmax(gap))])
    print(f"CG_GAP measured {worst:.4g} at {where}")
    assert 0.5 * ec.CG_GAP <= worst <= ec.CG_GAP and ec.CG_R == 4.0 * ec.CG_GAP


# ------------------------------------------------------------------------------------------------ edge paths
@pytest.mark.parametrize("name", [c.name for c in ec.GEO_CASES])
def test_relaxation_fixed_point_equals_float64_dijkstra(name):
    g = ec.geo_inputs(name)
    table, sweeps = ec.relax_fixed_point(name)
    exact = ec.dijkstra_float64(name)
    reach = np.isfinite(exact)
    assert np.array_equal(~reach, table == ec.UNREACHED) and table.dtype == np.float32
    assert (np.abs(table[reach] - exact[reach]) <= g["V"] * 2.0 ** -24 * exact[reach]).all()
    assert (table[np.arange(g["M"]), g["node_vertex"]] == 0).all()
    t2, idx, w = ec.geo_restatement(name)
    msgs, worst = ec.compare_geo(name, t2, idx, w)
    assert not msgs and worst <= 1.0 and np.isfinite(w).all() and idx.min() >= 0 and idx.max() < g["M"]


# ------------------------------------------------------------------------------------------------ face directions, weights
def test_face_direction_restatement_within_the_bound_of_the_longdouble_reference():
    assert np.finfo(np.longdouble).nmant >= 63 and np.finfo(np.longdouble).maxexp > 1024      # more digits AND more range
    for c in ec.DIR_CASES:
        msgs, worst = ec.compare_dirs(c.name, ec.dir_restatement(c.name))
        assert not msgs and worst <= 1.0, msgs
        ref, bound, zero = ec.dir_reference(c.name)
        n = np.sqrt((ref.reshape(c.F, 3, c.S) ** 2).sum(1)).astype(np.float64)
        assert (np.abs(n - 1.0)[~zero.reshape(c.F, 3, c.S)[:, 0]] < 1e-15).all()             # unit vectors, the far field included
        kinds = ec.dir_inputs(c.name)["kinds"]
        for s, k in enumerate(kinds):
            if k.startswith("const"):
                assert zero[:3, s].all()
            if k == "far":
                assert not zero[:, s].any()
    # the far field is there: gradients whose squares underflow in float64
    inp = ec.dir_inputs("dirs-F5-S65")
    far = [s for s, k in enumerate(inp["kinds"]) if k == "far"]
    assert inp["U"][:, far].min() == 1e-300 and inp["U"][:, far].max() == 1.0
    assert all(any(inp["U"][f][:, s].max() < 1e-160 for f in inp["faces"]) for s in far)


def _weight_errors():
    out = {}
    for c in ec.SEL_CASES:
        inp = ec.sel_inputs(c.name)
        sel = ec.stable_topk(inp["score"][:, :c.S], c.K + 1)
        rows = slice(c.v0, c.v0 + c.S)
        out[c.name] = (ec.weights_float32(inp["verts"][rows], inp["nodes"], sel), *ec.weights_reference(inp["verts"][rows], inp["nodes"], sel))
    for c in ec.GEO_CASES:
        g = ec.geo_inputs(c.name)
        sel = ec.stable_topk(ec.relax_fixed_point(c.name)[0].astype(np.float64), c.K + 1)
        out[c.name] = (ec.weights_float32(g["verts"], g["nodes"], sel), *ec.weights_reference(g["verts"], g["nodes"], sel))
    return out


def test_weight_yardstick_is_remeasured_and_the_restatements_pass_their_own_comparison():
    errs = {k: float(np.abs(w32 - ref).max()) for k, (w32, ref, _) in _weight_errors().items()}
    worst = max(errs, key=errs.get)
    print(f"WEIGHT_YARD measured {errs[worst]:.4g} at {worst}")
    assert 0.5 * ec.WEIGHT_YARD <= errs[worst] <= ec.WEIGHT_YARD
    for c in ec.SEL_CASES:
        idx, w = ec.select_restatement(c.name)
        msgs, ratio = ec.compare_select(c.name, idx, w)
        assert not msgs and ratio <= 1.0, msgs
        assert np.isfinite(w).all()


# ------------------------------------------------------------------------------------------------ coverage
def test_case_lists_cover_what_the_kernels_branch_on():
    assert {c.V for c in ec.CG_CASES} >= {1, 31, 32, 33, 65, 130} and {c.S for c in ec.CG_CASES} >= {1, 63, 64, 65, 257, 130}
    assert any(c.V % ec.CG_ROWS and c.V > ec.CG_ROWS for c in ec.CG_CASES)                   # partial row block after a full one
    assert any(c.S % ec.CG_COLS and c.S > ec.CG_COLS for c in ec.CG_CASES)                   # partial column block
    assert any(c.S > 256 for c in ec.CG_CASES)                                                # k_cg_reduce / k_cg_roll: two workgroups
    assert {c.matrix for c in ec.CG_CASES} == {"spd", "cot", "path"}
    kinds = set().union(*(ec.cg_inputs(c.name)["kinds"] for c in ec.CG_CASES))
    assert kinds == set(ec.COLUMN_KINDS)
    exact = ec.cg_inputs("spd-V33-S65")
    s = exact["kinds"].index("exact")
    assert not (exact["B"][:, s] - exact["A"] @ exact["X0"][:, s]).any()                      # rz == 0 and pAp == 0 from the start
    assert {(n, ce) for n, ce in ec.CG_FIXED} == {(n, ce) for n in (1, 7, 25) for ce in (1, 10)}      # 7 and 25: no multiples of 10
    assert {c.F for c in ec.DIR_CASES} == {1, 3, 4, 5} and {c.S for c in ec.DIR_CASES} == {1, 64, 65}
    sel = ec.SEL_CASES
    assert {c.K for c in sel} == {1, 4, 16} and {c.S for c in sel} >= {1, 255, 256, 257}
    assert {c.M - c.K for c in sel} >= {1, 2} and any(c.M == 40 for c in sel)
    assert any(c.ld > c.S for c in sel) and any(c.v0 > 0 and c.Vtot > c.v0 + c.S for c in sel)
    sk = set().union(*(ec.sel_inputs(c.name)["kinds"] for c in sel))
    assert {"ties", "all_equal", "descending", "ascending", "some_inf", "some_nan", "all_nan", "many_1e300", "twins", "equidistant"} <= sk
    nonfinite = [c.name for c in sel if not np.isfinite(ec.sel_inputs(c.name)["score"][:, :c.S]).all() or (ec.sel_inputs(c.name)["score"][:, :c.S] >= 1e300).any()]
    assert nonfinite == [c.name for c in sel if c.flavour == "nonfinite"]
    w = _weight_errors()
    degenerate = [k for k, (_, _, deg) in w.items() if deg.any()]
    assert degenerate == [c.name for c in sel if c.flavour == "degenerate"] + ["geo-degenerate-sphere", "geo-degenerate-coincident"]
    # cancellation (e_k within 0.2 % of e_K) and e_k > e_K
    tw = ec.sel_inputs("select-twins-K4-M12-S64")
    c = ec.SEL_BY_NAME["select-twins-K4-M12-S64"]
    st = ec.stable_topk(tw["score"][:, :c.S], c.K + 1)
    e = np.linalg.norm(tw["verts"][c.v0:c.v0 + c.S, None].astype(np.float64) - tw["nodes"][st], axis=-1)
    assert (np.abs(e[:, c.K - 1] / e[:, c.K] - 1) < 2e-3).any() and (e[:, :c.K] > e[:, c.K:]).any()
    # edge paths
    geo = {c.name: ec.geo_inputs(c.name) for c in ec.GEO_CASES}
    assert {g["V"] for g in geo.values()} >= {40, 300, 255, 256, 257}
    assert ec.relax_fixed_point("geo-path40")[1] > 16 and ec.relax_fixed_point("geo-path300")[1] > 256          # second relax batch
    assert any(g["M"] == g["K"] + 1 for g in geo.values()) and any(g["K"] == 16 for g in geo.values())
    assert all(len(set(g["node_vertex"].tolist())) < g["M"] for g in (geo["geo-path40"], geo["geo-V256"], geo["geo-components"]))
    comp, table = geo["geo-components"], ec.relax_fixed_point("geo-components")[0]
    assert (table == ec.UNREACHED).any() and np.diff(comp["off"])[49] == 0 and (table[:, 49] == ec.UNREACHED).all()
    second = np.arange(30, 49)
    assert ((table[:, second] < ec.UNREACHED).sum(0) == 2).all() and comp["K"] + 1 > 2       # fewer than K + 1 nodes reach it
    assert (geo["geo-zero-edges"]["len"] == 0).any()
    ties = ec.relax_fixed_point("geo-grid-ties")[0]
    assert any(len(set(ties[:, v].tolist())) < ties.shape[0] for v in range(ties.shape[1]))  # exact float32 ties


# ------------------------------------------------------------------------------------------------ mutants
def _cg_rejects(mutant):
    hit = []
    for name in CG_NAMES:
        bad = ec.cg_restatement(ec.cg_inputs(name), 7, ec.CG_FIXED_TOL, 10, mutant=mutant)
        if ec.compare_cg_fixed(name, 7, 10, bad.X, bad.iters, bad.rel):
            hit.append(name)
    return hit


def test_every_mutant_is_rejected_by_the_comparison_functions():
    sel_hit = lambda m: [c.name for c in ec.SEL_CASES if ec.compare_select(c.name, *ec.select_restatement(c.name, mutant=m))[0]]
    geo_hit = lambda m: [c.name for c in ec.GEO_CASES if ec.compare_geo(c.name, *ec.geo_restatement(c.name, mutant=m))[0]]
    hits = {
        "tie towards the higher index": sel_hit("tie_high") + geo_hit("tie_high"),
        "normalised by the K-th distance": sel_hit("kth") + geo_hit("kth"),
        "rows of the last partial block dropped": _cg_rejects("drop_rows"),
        "columns >= 64 floor(S / 64) dropped": _cg_rejects("drop_cols"),
        "wave stride 3": _cg_rejects("wave_stride"),
        "first_vertex ignored": sel_hit("ignore_v0"),
        "ld taken as S": sel_hit("ld_is_S"),
        "beta guard removed": _cg_rejects("no_beta_guard"),
        "directions not transposed": [c.name for c in ec.DIR_CASES if ec.compare_dirs(c.name, ec.dir_restatement(c.name, transposed=False))[0]],
    }
    print({k: len(v) for k, v in hits.items()})
    assert all(hits.values()), {k: v for k, v in hits.items() if not v}
    assert any(n.startswith("geo") for n in hits["tie towards the higher index"]) and any(n.startswith("select") for n in hits["tie towards the higher index"])
    assert set(hits["rows of the last partial block dropped"]) == {c.name for c in ec.CG_CASES if c.V % ec.CG_ROWS}
    assert set(hits["columns >= 64 floor(S / 64) dropped"]) == {c.name for c in ec.CG_CASES if c.S % ec.CG_COLS}
    assert set(hits["first_vertex ignored"]) == {c.name for c in ec.SEL_CASES if c.v0 > 0}
    assert set(hits["ld taken as S"]) == {c.name for c in ec.SEL_CASES if c.ld > c.S}
    # the beta guard shows on the columns that are finished from the start (NaN), and nowhere else
    assert set(hits["beta guard removed"]) == {c.name for c in ec.CG_CASES if {"exact", "zero"} & set(ec.cg_inputs(c.name)["kinds"]) or c.V == 1}
    # a sentinel index or a NaN weight in place of the device output is rejected too
    idx, w = ec.select_restatement("select-nonfinite-K4-M6-S65")
    idx2, w2 = idx.copy(), w.copy()
    idx2[3, -1], w2[5, 0] = -1, np.nan
    assert ec.compare_select("select-nonfinite-K4-M6-S65", idx2, w)[0] and ec.compare_select("select-nonfinite-K4-M6-S65", idx, w2)[0]
