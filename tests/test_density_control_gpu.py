"""Adaptive density control on the device: the reference's golden stages through ``GaussianModel``, the branch points of every
decision, the sizes and layouts at which the plan and the move take another path, guard rows, and a small end-to-end run.

Bounds of computed values: per element ``|got - f64| <= 4 * err_ref``, err_ref = the reference's (for the golden cases) or the
mask-indexing restatement's (elsewhere; no less than half an ulp of the tensor's largest magnitude, see
``density_control_common.restatement_unit``) own float32 error against float64 on the same inputs -- never anything the code
under test produced.  The factor 4 allows the device's expf, logf, sqrtf and division 1-2 ulp each where the CPU's are near 0.5, over
a chain of three to four operations."""
import types

import numpy as np
import pytest
import torch

from dreammesh4d_amd import _lib, density_control as dc, gaussian_model as gm, isosurface as iso
from tests import density_control_common as cm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NEVER = 10 ** 9


@pytest.fixture(scope="module")
def z():
    return cm.golden()


def on_dev(state):
    return cm.cast(state, device=DEV)


def state_of(model):
    st = {"params": {}, "m1": {}, "m2": {}}
    for g in model.optimizer.param_groups:
        p = g["params"][0]
        s = model.optimizer.state.get(p)
        st["params"][g["name"]] = p.data
        st["m1"][g["name"]] = None if s is None else s["exp_avg"]
        st["m2"][g["name"]] = None if s is None else s["exp_avg_sq"]
    st.update(accum=model.xyz_gradient_accum, denom=model.denom, max_radii=model.max_radii2D)
    return st


def model_from_state(state, sh_degree, step=2, **cfg):
    """A GaussianModel holding `state` (float32, CPU), its Adam state injected where the state has moments."""
    m = gm.GaussianModel(dict({"init_num_pts": 0, "sh_degree": sh_degree, "pred_normal": "normal" in state["params"]}, **cfg))
    for name, v in state["params"].items():
        setattr(m, m._GROUPS[name], torch.nn.Parameter(v.to(DEV).clone()))
    m.training_setup()
    for g in m.optimizer.param_groups:
        name = g["name"]
        if state["m1"][name] is not None:
            m.optimizer.state[g["params"][0]] = {"step": torch.tensor(float(step)), "exp_avg": state["m1"][name].to(DEV).clone(),
                                                 "exp_avg_sq": state["m2"][name].to(DEV).clone()}
    m.xyz_gradient_accum, m.denom = state["accum"].to(DEV).clone(), state["denom"].to(DEV).clone()
    m.max_radii2D = state["max_radii"].to(DEV).clone()
    return m


def check_optimizer(model, names, step):
    groups = model.optimizer.param_groups
    assert [g["name"] for g in groups] == list(names)
    params = [g["params"][0] for g in groups]
    assert all(len(g["params"]) == 1 and isinstance(g["params"][0], torch.nn.Parameter) for g in groups)
    assert all(getattr(model, model._GROUPS[g["name"]]) is g["params"][0] for g in groups)
    assert set(model.optimizer.state.keys()) == set(params), "stale or missing optimiser state keys"
    for p in params:
        s = model.optimizer.state[p]
        assert float(s["step"]) == step and s["exp_avg"].shape == p.shape and s["exp_avg_sq"].shape == p.shape


@pytest.mark.parametrize("case", ["A", "B"])
def test_golden_stages_through_the_model(z, case):
    want = {w["stage"]: w for w in cm.golden_stages(z, case)}
    gt, mo = float(z["grad_threshold"]), float(z["min_opacity"])
    m = model_from_state(cm.golden_inputs(z, "A"), 1, sphere=case == "B", split_thresh=float(z["split_thresh"]), prune_big_points=True,
                         densify_grad_threshold=gt, min_opac_prune=mo, sugar_prune_threshold=float(z["sugar_threshold"]), max_num=NEVER,
                         prune_from_iter=0, prune_until_iter=NEVER, prune_interval=NEVER, opacity_reset_interval=NEVER, densify_from_iter=0,
                         densify_until_iter=NEVER, densification_interval=NEVER)
    T = lambda a: torch.from_numpy(a).to(DEV)
    views = lambda g: [types.SimpleNamespace(grad=x) for x in T(g)]
    ratios, before = {}, [cm.cast(state_of(m))]

    def after(stage):
        n = len(want[stage]["src"])
        assert m._xyz.shape[0] == n, f"{stage}: {m._xyz.shape[0]} rows, the reference has {n}"
        for k, v in cm.compare_state(state_of(m), want[stage], f"case {case} {stage}", factor=4.0, prev=before[0]).items():
            ratios[f"{stage}/{k}"] = v
        check_optimizer(m, cm.NAMES, 2)
        before[0] = cm.cast(state_of(m))

    m.update_states(1, None, T(z["A/in/radii_0"]), views(z["A/in/grad2d_0"]))
    assert not m.pruned_or_densified
    after("stats")
    kinds = cm.kinds_densify(want["stats"]["state"], gt, float(z["split_thresh"]), case == "B").numpy()
    counts = m.densify(gt, noise=T(z[f"{case}/noise"]))
    assert counts == {"keep": int((kinds == 0).sum()), "drop": 0, "clone": int((kinds == 2).sum()), "split": int((kinds == 3).sum()),
                      "M": len(want["densify"]["src"])}
    after("densify")
    m.cfg.prune_interval, m.cfg.densify_until_iter = 200, 0
    m.update_states(200, None, list(T(z[f"{case}/radii_1"])), views(z[f"{case}/grad2d_1"]))
    assert m.pruned_or_densified
    m.cfg.prune_interval = NEVER
    after("prune")
    m.reset_opacity()
    after("reset")
    m.cfg.max_num = int(z["max_num"])
    m.update_states(201, None, None, None, generator=torch.Generator().manual_seed(int(z["perm_seed"])))
    m.cfg.max_num = NEVER
    after("cap")
    m.cfg.sugar_prune_at = 202
    m.update_states(202, None, None, None)
    after("sugar")
    print(f"case {case}: error / err_ref of the computed tensors {({k: round(v, 3) for k, v in ratios.items()})}")
    for g in m.optimizer.param_groups:
        g["lr"] = 1e-3
        g["params"][0].grad = torch.ones_like(g["params"][0])
    m.optimizer.step()
    check_optimizer(m, cm.NAMES, 3)
    assert all(torch.isfinite(g["params"][0]).all() for g in m.optimizer.param_groups)


# ------------------------------------------------------------------------------------------------ branch points
def f32(*v):
    return torch.tensor(v, dtype=torch.float32, device=DEV)


def test_branch_points_of_densify():
    below = float(np.nextafter(np.float32(0.046875), np.float32(0)))
    accum, denom = f32(0.046875, below, 0.046875, 1.0), f32(3, 3, 0, 1)
    assert np.float32(0.046875) / np.float32(3) == np.float32(0.015625)
    small = torch.full((4, 3), -20.0, device=DEV)
    kind = dc.classify_densify(accum, denom, small, 0.015625, 1.0)
    assert kind.tolist() == [dc.CLONE, dc.KEEP, dc.KEEP, dc.CLONE]          # >= selects; the float below does not; denom 0 keeps
    inf = float("inf")
    scaling = torch.tensor([[0.0, -inf, -inf], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.1, -inf, -inf]], device=DEV)
    hot_a, hot_d = f32(1, 1, 1, 1), f32(1, 1, 1, 1)
    assert dc.classify_densify(hot_a, hot_d, scaling, 0.5, 1.0).tolist() == [dc.CLONE, dc.SPLIT, dc.SPLIT, dc.SPLIT]   # nrm == 1: clone
    root3 = float(np.sqrt(np.float32(3)))
    k = dc.classify_densify(hot_a[:2].contiguous(), hot_d[:2].contiguous(), scaling[1:3].contiguous(), 0.5, root3)
    assert k.tolist() == [dc.CLONE, dc.CLONE]                               # nrm == float32(sqrt(3)) == the threshold: clone
    sph = torch.tensor([[0.3, -0.3, 0.0], [3.0, -3.0, 0.0]], device=DEV)     # mean 0 -> s = 1 on all axes, nrm = sqrt(3)
    assert dc.classify_densify(hot_a[:2].contiguous(), hot_d[:2].contiguous(), sph, 0.5, root3, sphere=True).tolist() == [dc.CLONE, dc.CLONE]
    assert dc.classify_densify(hot_a[:2].contiguous(), hot_d[:2].contiguous(), sph, 0.5, root3).tolist() == [dc.SPLIT, dc.SPLIT]
    with pytest.raises(_lib.Dm4dError, match="grad_threshold"):
        dc.classify_densify(hot_a, hot_d, scaling, 0.0, 1.0)


def test_branch_points_of_prune():
    below = float(np.nextafter(np.float32(0), np.float32(-1)))
    opacity = f32(0.0, below, -1e-3, 5.0).reshape(4, 1)
    assert dc.classify_prune(opacity, 0.5).tolist() == [dc.KEEP, dc.KEEP, dc.DROP, dc.KEEP]     # sigmoid(0) = 0.5 is not < 0.5
    radii = f32(7.0, float(np.nextafter(np.float32(7), np.float32(8))), 6.0, 100.0)
    limit = f32(7.0)
    assert dc.classify_prune(f32(5, 5, 5, 5), 0.5, radii, limit).tolist() == [dc.KEEP, dc.DROP, dc.KEEP, dc.DROP]   # == the limit keeps
    assert dc.classify_prune(f32(5, 5, -5, 5), 0.5, radii, limit).tolist() == [dc.KEEP, dc.DROP, dc.DROP, dc.DROP]
    assert dc.classify_prune(f32(5, 5, 5, 5), 0.5, radii, None).tolist() == [dc.KEEP] * 4


def test_branch_points_of_stats():
    g = torch.tensor([[[3.0, 4.0, 9.0], [3.0, 4.0, 9.0], [3.0, 4.0, 9.0], [0.0, 0.0, 9.0]],
                      [[0.5, 0.0, 9.0], [0.5, 0.0, 9.0], [0.5, 0.0, 9.0], [0.5, 0.0, 9.0]]], device=DEV)
    radii = torch.tensor([[2, 0, -3, 1], [9, 4, 0, 0]], dtype=torch.int32, device=DEV)
    accum, denom, mr = f32(1, 1, 1, 1).reshape(4, 1), f32(0, 1, 2, 3).reshape(4, 1), f32(5, 5, 5, 0.5)
    dc.accumulate_stats(g, radii, accum, denom, mr)
    assert accum.reshape(-1).tolist() == [6.5, 1.5, 1.0, 1.0]               # radii 0 and negative radii are not visible
    assert denom.reshape(-1).tolist() == [2.0, 2.0, 2.0, 4.0]
    assert mr.tolist() == [9.0, 5.0, 5.0, 1.0]                              # the max is taken in every view, visible or not


def test_reset_opacity_values_and_null_moments():
    st = cm.random_state(777, 0, 5)
    x = st["params"]["opacity"]
    want = cm.reset_opacity(cm.cast(st, torch.float64))["params"]["opacity"]
    err_ref = cm.restatement_unit(cm.reset_opacity(st)["params"]["opacity"], want)
    o, m1, m2 = x.to(DEV).clone(), st["m1"]["opacity"].to(DEV).clone(), st["m2"]["opacity"].to(DEV).clone()
    dc.reset_opacity(o, m1, m2)
    cm.assert_within(o, want, err_ref, "reset_opacity")
    assert not m1.any() and not m2.any()
    o2 = x.to(DEV).clone()
    dc.reset_opacity(o2)
    cm.assert_bit_equal(o2, o, "reset_opacity without moments")


# ------------------------------------------------------------------------------------------------ sizes and layouts
def run_apply(state, kind, S=2, sphere=False, seed=0, check_children=True):
    """dc.apply on `state` (CPU float32) with `kind` (numpy uint8) against the mask-indexing expectation: counts, row order, bit
    copies, zero moments of new rows, the children within 4 x the restatement's float32 error.  Everything is compared on the
    device, all rows."""
    n = len(kind)
    noise = torch.from_numpy(np.random.default_rng(seed).standard_normal((S, n, 3)).astype(np.float32))
    d = on_dev(state)
    moments = {k: (None if d["m1"][k] is None else (d["m1"][k], d["m2"][k])) for k in d["params"]}
    before = {k: v.clone() for k, v in d["params"].items()}
    new, new_m, counts = dc.apply(torch.from_numpy(kind).to(DEV), d["params"], moments, noise=noise.to(DEV), S=S, sphere=sphere)
    src, role = cm.expected_rows(kind, S)
    k2 = kind & 3
    assert counts == {"keep": int((k2 == 0).sum()), "drop": int((k2 == 1).sum()), "clone": int((k2 == 2).sum()),
                      "split": int((k2 == 3).sum()), "M": len(src)}
    s_dev, child, fresh = torch.from_numpy(src.astype(np.int64)).to(DEV), torch.from_numpy(role >= 2).to(DEV), torch.from_numpy(role > 0).to(DEV)
    as_bits = lambda t: t.contiguous().view(torch.int32)
    for name, p in d["params"].items():
        assert torch.equal(as_bits(p), as_bits(before[name])), f"{name}: the input was modified"
        out = new[name]
        assert out.shape == (len(src),) + tuple(p.shape[1:]) and out.dtype == torch.float32
        rows = ~child if name in ("xyz", "scaling") else torch.ones_like(child)
        assert torch.equal(as_bits(out)[rows], as_bits(p[s_dev])[rows]), f"{name}: copied rows differ in their bits"
        if moments[name] is None:
            assert new_m[name] is None
            continue
        for q in range(2):
            want = moments[name][q][s_dev].clone()
            want[fresh] = 0
            assert torch.equal(as_bits(new_m[name][q]), as_bits(want)), f"moment {q} of {name}"
    if check_children and counts["split"]:
        sources = np.flatnonzero(k2 == 3)
        x32, s32 = cm.children(state["params"], sources, noise, S, sphere)
        x64, s64 = cm.children(cm.cast(state, torch.float64)["params"], sources, noise, S, sphere)
        for name, got, w32, w64 in (("xyz", new["xyz"], x32, x64), ("scaling", new["scaling"], s32, s64)):
            cm.assert_within(got[child], w64, cm.restatement_unit(w32, w64), f"children's {name} (N = {n}, S = {S})")
    return new, new_m, counts


def random_kind(n, seed, p=(0.4, 0.2, 0.2, 0.2)):
    return np.random.default_rng(seed).choice(np.arange(4, dtype=np.uint8), n, p=p)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099])
@pytest.mark.parametrize("sh_degree", [0, 3])
def test_sizes(n, sh_degree):
    """4099 = one scan tile and three rows; widths 1, 3, 4 and 45 (sh_degree 3), f_rest without columns at sh_degree 0."""
    run_apply(cm.random_state(n, sh_degree, n), random_kind(n, n + 1), sphere=bool(n % 2))
    if n == 1:
        for k in range(4):
            run_apply(cm.random_state(1, sh_degree, 9), np.array([k], np.uint8))


def test_a_million_rows():
    """N = 1,000,003 at sh_degree 0: 245 scan tiles, rows past 2^16 in every rank."""
    n = 1_000_003
    rng = np.random.default_rng(3)
    params = {name: torch.from_numpy(rng.standard_normal((n,) + tail, dtype=np.float32)) for name, tail in cm.param_shapes(0, False).items()}
    st = {"params": params, "m1": {k: v * 0.5 for k, v in params.items()}, "m2": {k: v * v for k, v in params.items()}}
    run_apply(st, random_kind(n, 4, (0.7, 0.1, 0.1, 0.1)))


def test_plan_where_the_scan_of_the_totals_loops():
    """The totals are scanned by ONE workgroup of 1024 lanes, a lane owning ceil(G / 1024) consecutive totals; G = 1025 tiles of
    4096 rows (N = 4,194,309) is the smallest size at which a lane owns two.  The plan alone: 4 MB of kinds."""
    n = 4096 * 1024 + 5
    kind = random_kind(n, 11, (0.5, 0.2, 0.2, 0.1))
    src, role, counts = dc.plan(torch.from_numpy(kind).to(DEV), 2)
    es, er = cm.expected_rows(kind, 2)
    assert counts["M"] == len(es)
    assert torch.equal(src.cpu(), torch.from_numpy(es)) and torch.equal(role.cpu(), torch.from_numpy(er))


def test_all_keep_all_drop():
    st = cm.random_state(300, 1, 2)
    new, new_m, counts = run_apply(st, np.zeros(300, np.uint8))
    assert counts["M"] == 300
    for name, v in st["params"].items():
        cm.assert_bit_equal(new[name], v, name)
        cm.assert_bit_equal(new_m[name][0], st["m1"][name], f"m1/{name}")
    new, new_m, counts = run_apply(st, np.ones(300, np.uint8))
    assert counts == {"keep": 0, "drop": 300, "clone": 0, "split": 0, "M": 0}
    assert all(v.shape[0] == 0 and v.shape[1:] == st["params"][k].shape[1:] for k, v in new.items())
    assert all(m[0].shape[0] == 0 for m in new_m.values())
    # a boolean mask is a kind: True drops
    mask = torch.from_numpy(np.arange(300) % 3 == 0)
    new, _, counts = dc.apply(mask.to(DEV), on_dev(st)["params"], None)
    assert counts["M"] == 200
    cm.assert_bit_equal(new["rotation"], st["params"]["rotation"][~mask], "rotation under a boolean mask")


@pytest.mark.parametrize("S", [1, 2, 8])
def test_all_split(S):
    run_apply(cm.random_state(130, 1, S), np.full(130, 3, np.uint8), S=S, sphere=S == 8)


def test_alternating_kinds_and_high_bits():
    n = 1000
    per_element = (np.arange(n) % 4).astype(np.uint8)
    per_block = ((np.arange(n) // 64) % 4).astype(np.uint8)
    st = cm.random_state(n, 0, 6)
    run_apply(st, per_element)
    run_apply(st, per_block)
    new_a, _, _ = run_apply(st, per_element | np.uint8(0xFC))               # the kernels read kind & 3
    new_b, _, _ = run_apply(st, per_element)
    cm.assert_bit_equal(new_a["xyz"], new_b["xyz"], "kind & 3")


def test_unnormalised_quaternion_gives_the_same_children():
    st = cm.random_state(200, 0, 8)
    kind = np.full(200, 3, np.uint8)
    q = st["params"]["rotation"]
    st["params"]["rotation"] = q / q.norm(dim=1, keepdim=True)
    a, _, _ = run_apply(st, kind)
    st2 = cm.cast(st)
    st2["params"]["rotation"] = st["params"]["rotation"] * 2
    b, _, _ = run_apply(st2, kind)                                          # both within the bound of the same float64 children
    x64, _ = cm.children(cm.cast(st, torch.float64)["params"], np.arange(200), torch.from_numpy(
        np.random.default_rng(0).standard_normal((2, 200, 3)).astype(np.float32)), 2, False)
    x32, _ = cm.children(st["params"], np.arange(200), torch.from_numpy(
        np.random.default_rng(0).standard_normal((2, 200, 3)).astype(np.float32)), 2, False)
    cm.assert_within(b["xyz"], x64, cm.restatement_unit(x32, x64), "children of 2 x the unit quaternion")


def test_table_of_24_arrays_and_a_group_without_state():
    n = 500
    rng = np.random.default_rng(12)
    widths = [1, 3, 4, 9, 24, 45, 2, 8]
    params = {f"a{i}": torch.from_numpy(rng.standard_normal((n, w), dtype=np.float32)) for i, w in enumerate(widths)}
    st = {"params": params, "m1": {k: v + 1 for k, v in params.items()}, "m2": {k: v * v for k, v in params.items()}}
    kind = random_kind(n, 13, (0.5, 0.3, 0.2, 0.0))
    run_apply(st, kind)                                                     # 8 arrays with both moments: 24 table entries
    st["m1"]["a3"] = st["m2"]["a3"] = None                                  # a group that has not stepped yet
    new, new_m, _ = run_apply(st, kind)
    assert new_m["a3"] is None and new["a3"].shape[0] == new["a0"].shape[0]
    many = {f"b{i}": torch.from_numpy(rng.standard_normal((n, 1 + i % 5), dtype=np.float32)) for i in range(30)}
    run_apply({"params": many, "m1": {k: None for k in many}, "m2": {k: None for k in many}}, kind)   # two launches of the move


def test_guard_rows_stay_untouched():
    """The C entry points on views into sentinel-filled buffers: inputs, scratch, plan and outputs keep their guards; the kinds
    and the arrays start at odd offsets (the byte-wise and 4-byte paths)."""
    n, S, G = 5000, 2, 64
    kind_np = random_kind(n, 21)
    src_np, role_np = cm.expected_rows(kind_np, S)
    M = len(src_np)
    L, st = _lib.lib(), _lib.stream(DEV)

    def guarded(count, dtype, fill, front=G):
        buf = torch.full((front + count + G,), fill, dtype=dtype, device=DEV)
        return buf, buf[front:front + count]

    kbuf, kind = guarded(n, torch.uint8, 0xEE, front=3)
    kind.copy_(torch.from_numpy(kind_np))
    nbytes = L.dm4d_dc_plan_scratch_bytes(n)
    sbuf, scratch = guarded(nbytes // 4, torch.int32, -7)
    tbuf, totals = guarded(4, torch.int64, -7)
    srcbuf, src = guarded(M, torch.int32, -7)
    rolebuf, role = guarded(M, torch.uint8, 0xEE)
    widths = [3, 4, 45]
    ins, outs = [], []
    for w in widths:
        ibuf, i = guarded(n * w, torch.float32, -7.0, front=w)             # one guard row in front: 12 bytes for width 3
        i.copy_(torch.from_numpy(np.random.default_rng(w).standard_normal(n * w).astype(np.float32)))
        ins.append((ibuf, i))
        outs.append(guarded(M * w, torch.float32, -7.0, front=w))
    _lib.call("dm4d_dc_plan_count", n, kind.data_ptr(), scratch.data_ptr(), nbytes, totals.data_ptr(), st)
    _lib.call("dm4d_dc_plan_rows", n, kind.data_ptr(), S, scratch.data_ptr(), nbytes, totals.data_ptr(), M, src.data_ptr(), role.data_ptr(), st)
    A = _lib.DcArrays()
    A.count = len(widths)
    for a, w in enumerate(widths):
        getattr(A, "in")[a], A.out[a], A.width[a], A.flags[a] = ins[a][1].data_ptr(), outs[a][1].data_ptr(), w, _lib.DM4D_DC_ZERO_NEW if a == 1 else 0
    import ctypes
    _lib.call("dm4d_dc_move", n, M, src.data_ptr(), role.data_ptr(), ctypes.byref(A), st)
    torch.cuda.synchronize()
    assert torch.equal(src.cpu(), torch.from_numpy(src_np)) and torch.equal(role.cpu(), torch.from_numpy(role_np))
    k2 = kind_np & 3
    assert totals.tolist() == [int((k2 == q).sum()) for q in range(4)]
    for a, w in enumerate(widths):
        want = ins[a][1].reshape(n, w)[torch.from_numpy(src_np.astype(np.int64)).to(DEV)].clone()
        if a == 1:
            want[torch.from_numpy(role_np > 0).to(DEV)] = 0
        cm.assert_bit_equal(outs[a][1].reshape(M, w), want, f"width {w}")
    for name, buf, view, front, fill in [("kind", kbuf, kind, 3, 0xEE), ("scratch", sbuf, scratch, G, -7), ("totals", tbuf, totals, G, -7),
                                         ("src", srcbuf, src, G, -7), ("role", rolebuf, role, G, 0xEE)] + \
            [(f"in{w}", ins[a][0], ins[a][1], w, -7.0) for a, w in enumerate(widths)] + \
            [(f"out{w}", outs[a][0], outs[a][1], w, -7.0) for a, w in enumerate(widths)]:
        assert bool((buf[:front] == fill).all()) and bool((buf[front + view.numel():] == fill).all()), f"{name}: a guard was written"
    assert torch.equal(kind.cpu(), torch.from_numpy(kind_np))


# ------------------------------------------------------------------------------------------------ end to end
def test_end_to_end_small(tmp_path):
    rng = np.random.default_rng(0)
    pts = rng.standard_normal((100, 3))
    pts = 0.5 * pts / np.linalg.norm(pts, axis=1, keepdims=True)
    cfg = {"init_num_pts": 0, "sh_degree": 0, "prune_from_iter": 0, "prune_until_iter": 3, "prune_interval": 2, "densify_from_iter": 0,
           "densify_until_iter": 10, "densification_interval": 3, "densify_grad_threshold": 0.01, "split_thresh": 0.1, "min_opac_prune": 0.3,
           "opacity_init": 0.5}
    m = gm.GaussianModel(cfg)
    m.create_from_pcd(gm.BasicPointCloud(points=pts, colors=rng.random((100, 3)), normals=np.zeros((100, 3))), 10)
    m.training_setup()
    assert m._xyz.shape == (100, 3) and m._features_rest.shape == (100, 0, 3) and bool((m._rotation[:, 0] == 1).all())
    with torch.no_grad():
        m._opacity[::4] = -3.0                                              # a quarter below min_opac_prune
        m._scaling[::2] += 1.5                                              # half of them large enough to split
    sizes = []
    for it in range(1, 6):
        n = m._xyz.shape[0]
        for g in m.optimizer.param_groups:
            g["params"][0].grad = torch.from_numpy(rng.standard_normal(tuple(g["params"][0].shape)).astype(np.float32) * 1e-3).to(DEV)
        m.optimizer.step()
        grads = [types.SimpleNamespace(grad=torch.from_numpy((rng.standard_normal((n, 3)) * 0.02).astype(np.float32)).to(DEV)) for _ in range(2)]
        radii = torch.from_numpy(rng.integers(0, 30, (2, n)).astype(np.int32)).to(DEV)
        m.update_states(it, None, radii, grads, noise=None)
        assert m.pruned_or_densified == (it in (2, 3))
        sizes.append(m._xyz.shape[0])
        check_optimizer(m, ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"), it)
        assert m.xyz_gradient_accum.shape == (sizes[-1], 1) and m.max_radii2D.shape == (sizes[-1],)
    assert sizes[0] == 100 and sizes[1] == 75 and sizes[2] > sizes[1] and sizes[3] == sizes[2], sizes
    path = str(tmp_path / "gaussians.ply")
    m.save_ply(path)
    m2 = gm.GaussianModel({"init_num_pts": 0, "sh_degree": 0})
    m2.load_ply(path)
    for attr in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
        cm.assert_bit_equal(getattr(m2, attr).data, getattr(m, attr).data, attr)
    mesh = iso.extract_mesh(m, density_thresh=0.05, resolution=32, num_blocks=4)
    assert mesh["n_kept"] > 0 and mesh["verts"].shape[1] == 3 and mesh["colors"] is not None
