"""Pins the float64 reference, the cases and the bounds that tests/test_static_kernels_edges_gpu.py judges csrc/sugar_attr.hip and
csrc/statichead.hip by (CPU only, no library call).

* The closed-form reference (tests/static_kernels_edges.py) against float64 torch autograd through the project's own compositions --
  `SuGaR._attributes_fn` (the geometry functions) for the attributes; `renderer._where_detached`, `static_stage.tv_loss`,
  `F.mse_loss` and `F.interpolate` for the head -- on every case, every value and gradient element within 64 float64 roundings of
  its scale.  torch runs with the inputs' float32 decisions: F.normalize's eps is float32(1e-12) (what the kernels compare against;
  the double 1e-12 lies ABOVE it and would switch the equality cases to the clamped branch), the opacity mask is taken on the
  float32 opacities.
* |x| == eps: torch's float32 F.normalize itself gives the projected gradient there, and so does the reference.
* float32 restatement and float64 reference take identical branches on every case, and the cases cover every branch value.
* The yardsticks cover the float32 restatement and are not padded: 0.8 x constant <= measured <= constant.
* Eight one-token mutants of the float32 restatement each exceed their bound in at least one case.
"""
import functools
from unittest import mock

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import static_kernels_edges as ec

ATTR = [c.name for c in ec.ATTR_CASES]
HEAD = [c.name for c in ec.HEAD_CASES]
R64 = 64 * 2.0 ** -53


def _pinned(got, ref, what):
    got = np.asarray(got, np.float64).reshape(ref.v.shape)
    bad = np.abs(got - ref.v) > R64 * ref.s
    i = np.unravel_index(int(np.abs(got - ref.v).argmax()), got.shape) if got.size else ()
    assert not bad.any(), f"{what}: {int(bad.sum())} of {got.size} elements; e.g. {i}: torch {got[i]!r}, closed form {ref.v[i]!r}, scale {ref.s[i]:.3g}"


def _eps32():
    """The project's compositions with F.normalize's eps = float32(1e-12)."""
    from dreammesh4d_amd import geometry as geo

    return mock.patch.object(geo.F, "normalize", functools.partial(F.normalize, eps=ec.EPS))


# every case with all five upstream gradients; the cases with `variants` also with each gradient alone and with none
ATTR_PINS = [(c.name, w) for c in ec.ATTR_CASES for w in ([ec.UPSTREAM] + ([(k,) for k in ec.UPSTREAM] + [()] if c.variants else []))]


@pytest.mark.parametrize("name,which", ATTR_PINS, ids=[f"{n}-{'+'.join(k[2:] for k in w) or 'none'}" for n, w in ATTR_PINS])
def test_attribute_reference_equals_float64_autograd_through_the_torch_properties(name, which):
    from dreammesh4d_amd import sugar

    case, inp = ec.ATTR_BY_NAME[name], ec.attr_inputs(name)
    ref = ec.attr_case_reference(name, which)
    g = sugar.SuGaR(inp["points"], inp["faces"], n_gaussians_per_surface_triangle=case.G, device="cpu")
    assert np.array_equal(g._bary.numpy().reshape(-1, 3), inp["bary"])                     # SuGaR's own table
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)
    params = [t64(inp["points"]), t64(inp["cx"]), t64(inp["log_scales"]), t64(inp["densities"][:, None]), t64(inp["sh_dc"][:, None])]
    with _eps32():
        xyz, op, sc, rot, rgb, nrm = g._attributes_fn(inp["thickness"])(*params, torch.tensor(float(np.float32(inp["clip"])), dtype=torch.float64))
    N = len(inp["cx"])
    _pinned(xyz.detach(), ref["means"], "means")
    _pinned(rot.detach(), ref["rots"], "rotations")
    _pinned(sc.detach(), ref["scales"], "scales")
    _pinned(op.detach().reshape(N), ref["opac"], "opacities")
    _pinned(torch.cat([rgb, nrm], 1).detach(), ref["colors"], "colors")
    up = {k: torch.tensor(inp[k].astype(np.float64)) for k in which}
    zero = xyz.sum() * 0
    loss = zero + sum((out * up[k].reshape(out.shape)).sum() for k, out in (("g_means", xyz), ("g_rots", rot), ("g_scales", sc), ("g_opac", op)) if k in up)
    if "g_colors" in up:
        loss = loss + (torch.cat([rgb, nrm], 1) * up["g_colors"]).sum()
    grads = torch.autograd.grad(loss, params, allow_unused=True)
    for kind, gr, p in zip(("g_points", "g_cx", "g_ls", "g_den", "g_sh"), grads, params):
        gr = torch.zeros_like(p) if gr is None else gr
        assert bool(torch.isfinite(gr).all()), kind
        _pinned(gr.reshape(ref[kind].v.shape), ref[kind], kind)


def _head_composition(inp, dtype):
    """The torch operators static_head replaces (tests/test_static_stage_gpu.py), for any assignment of the views."""
    from dreammesh4d_amd.renderer import _where_detached
    from dreammesh4d_amd.static_stage import tv_loss

    t = lambda a: torch.tensor(np.asarray(a).astype(np.float64 if dtype == torch.float64 else np.float32))
    c, d, a = (t(inp[k]).requires_grad_(True) for k in ("color", "depth", "alpha"))
    B, _, H, W = c.shape
    n_ref, n_rnd = inp["n_ref"], inp["n_rnd"]
    mask = torch.tensor(inp["alpha"] > ec.A99)                                           # on the float32 opacities
    rgb = c[:, :3].clamp(0, 1)
    n_map = _where_detached(F.normalize(c[:, 3:], dim=1, eps=ec.EPS) * 0.5 * a + 0.5, mask.expand(B, 3, H, W))
    dd = _where_detached(d, mask)
    ref_v = [(int(r), v) for v, r in enumerate(inp["ref_pos"]) if 0 <= r < n_ref]
    rnd_v = [v for _, v in sorted((int(n), v) for v, n in enumerate(inp["rnd_pos"]) if 0 <= n < n_rnd)]
    zero = c.sum() * 0
    terms = [zero] * 5
    if ref_v:        # F.mse_loss over the n_ref reference views: each view against the reference image fidx_ref[its position]
        assert sorted(r for r, _ in ref_v) == list(range(n_ref))
        gt = torch.stack([t(inp["ref_images"][int(inp["fidx_ref"][r])]) for r, _ in ref_v])
        m = torch.stack([t(inp["ref_masks"][int(inp["fidx_ref"][r])]) for r, _ in ref_v])
        vs = [v for _, v in ref_v]
        terms[0] = F.mse_loss(gt * m, rgb[vs].permute(0, 2, 3, 1) * m)
        terms[1] = F.mse_loss(m, a[vs].permute(0, 2, 3, 1))
    half = torch.zeros(0, H // 2, W // 2, 3, dtype=c.dtype)
    if rnd_v:
        assert len(rnd_v) == n_rnd
        terms[2:] = [tv_loss(rgb[rnd_v]), tv_loss(dd[rnd_v]), tv_loss(n_map[rnd_v])]
        half = F.interpolate(rgb[rnd_v], (H // 2, W // 2), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    t5 = torch.stack(terms)
    loss = (t5 * t(inp["g_terms"])).sum() + zero
    if inp["g_half"] is not None:
        loss = loss + (half * t(inp["g_half"])).sum()
    grads = torch.autograd.grad(loss, (c, d, a), allow_unused=True)
    return t5.detach(), half.detach(), [torch.zeros_like(p) if g is None else g for g, p in zip(grads, (c, d, a))]


@pytest.mark.parametrize("name", HEAD)
def test_head_reference_equals_float64_autograd_through_the_torch_composition(name):
    case = ec.HEAD_BY_NAME[name]
    variants = [(True, True)] if name == ec.BIG else [(True, True), (True, False), (False, True)]
    for g_terms, g_half in variants:
        if not g_half and not case.with_half:
            continue
        inp, ref = ec.head_inputs(name, g_terms, g_half), ec.head_case_reference(name, g_terms, g_half)
        t5, half, (gc, gd, ga) = _head_composition(inp, torch.float64)
        _pinned(t5, ref["terms"], f"{name} terms")
        _pinned(half, ref["half"], f"{name} half")
        for kind, got in (("g_color", gc), ("g_depth", gd), ("g_alpha", ga)):
            assert bool(torch.isfinite(got).all())
            _pinned(got, ref[kind], f"{name} {kind} (g_terms {g_terms}, g_half {g_half})")
        # the partial sums add up to the terms' sums, and a view that is neither kind of view has none and receives nothing
        assert ref["partial"].v.shape == (case.B, ec.head_blocks(case.H, case.W), 8)
        for v in range(case.B):
            if not ref["branches"]["is_ref"][v] and not ref["branches"]["is_rnd"][v]:
                for k in ("partial", "g_color", "g_depth", "g_alpha"):
                    assert not ref[k].v[v].any() and not ref[k].s[v].any()
        thin = ~ref["branches"]["solid"].reshape(case.B, 1, case.H, case.W)
        assert not ref["g_depth"].s[thin].any() and not ref["g_color"].s[:, 3:][np.broadcast_to(thin, (case.B, 3, case.H, case.W))].any()


def test_at_norm_equal_eps_torch_takes_the_projected_gradient_and_so_does_the_reference():
    eps32 = np.float32(1e-12)
    assert np.sqrt(eps32 * eps32) == eps32 and float(eps32) == ec.EPS and ec.EPS < 1e-12
    for x, up, want in (([eps32, 0], [1, 1], [0, 1e12]), ([0, eps32, 0], [1, 1, 1], [1e12, 0, 1e12])):
        t = torch.tensor(np.asarray(x, np.float32), requires_grad=True)
        F.normalize(t, dim=0).backward(torch.tensor(np.asarray(up, np.float32)))           # torch's own float32 path, its own eps
        assert np.allclose(t.grad.numpy(), want, rtol=1e-6), t.grad
    # the reference at the planted equality points: a complex number, a face edge with its normal, a pixel normal
    inp = ec.attr_inputs("attr-special-G3")
    for f in (np.float64, np.float32):
        with np.errstate(all="ignore"):
            r = ec.attr_reference(inp, f)
        b = r["branches"]
        assert b["eq_c"].sum() >= 2 and b["live_c"][b["eq_c"]].all() and b["eq_1"].sum() == 1 and np.array_equal(b["eq_1"], b["eq_n"])
        i = np.flatnonzero(b["eq_c"] & (inp["cx"][:, 1] == 0))                              # (EPS, 0): no gradient along itself
        assert not r["g_cx"].v[i, 0].any() and np.abs(r["g_cx"].v[i, 1]).max() > 1e9
    for name in ec.HEAD_BY_NAME:
        if name != ec.BIG:
            b = ec.head_case_reference(name)["branches"]
            hit = b["eq"] & b["solid"] & b["is_rnd"][:, None]
            assert b["live"][b["eq"]].all()
            assert hit.any() or not b["is_rnd"].any(), name


@pytest.mark.parametrize("name", ATTR + HEAD)
def test_float32_and_float64_take_identical_branches(name):
    if name in ec.ATTR_BY_NAME:
        a, b = ec.attr_case_reference(name)["branches"], ec.attr_float32(name)["branches"]
    else:
        a, b = ec.head_case_reference(name)["branches"], ec.head_float32(name)["branches"]
    assert a.keys() == b.keys()
    for k in a:
        if k != "second":
            assert np.array_equal(a[k], b[k]), (name, k)


def test_the_cases_cover_every_branch_value_and_every_size():
    both = lambda m: bool(m.any() and not m.all())
    seen = {k: [] for k in ("best", "flip", "live_n", "live_1", "live_2", "live_c", "inside", "above", "w_zero", "ties4")}
    pairs, sizes = set(), set()
    for c in ec.ATTR_CASES:
        inp, b = ec.attr_inputs(c.name), ec.attr_case_reference(c.name)["branches"]
        for k in seen:
            seen[k].append(b[k].reshape(-1))
        tie = b["tie"] & ~b["ties4"]
        pairs |= {tuple(sorted(p)) for p in zip(b["best"][tie].tolist(), b["second"][tie].tolist())}
        sizes.add((len(inp["faces"]), c.G))
        assert len(inp["faces"]) <= 300 and inp["densities"].min() == -30 and inp["densities"].max() == 30
        assert inp["log_scales"].min() == -20 and inp["log_scales"].max() == 10
    seen = {k: np.concatenate(v) for k, v in seen.items()}
    assert set(seen["best"].tolist()) == {0, 1, 2, 3}
    assert all(both(seen[k]) for k in ("flip", "live_n", "live_1", "live_2", "live_c", "inside", "above", "w_zero", "ties4"))
    assert pairs == {(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)}                        # every two-way tie
    cube = ec.attr_case_reference("attr-cube-G1")["branches"]
    assert (cube["w_zero"] & (cube["best"] != 0)).any() and not cube["flip"][cube["w_zero"]].any()        # 180 degree turns: no flip
    assert {c.G for c in ec.ATTR_CASES} == {1, 3, 4, 6} and {c.clip for c in ec.ATTR_CASES} == {0.0, 1.2, 2.5}
    assert {1, 127, 128, 129, 300} <= {f for f, _ in sizes} and {255, 256, 257, 258} <= {f * g for f, g in sizes}
    for clip, reach in ((2.5, True), (1.2, False), (0.0, False)):
        ab = np.concatenate([ec.attr_case_reference(c.name)["branches"]["above"].reshape(-1) for c in ec.ATTR_CASES if c.clip == clip])
        assert both(ab) == reach
    for c in ec.ATTR_CASES:                                     # sh at the clip and one float beyond it, on both sides
        sh, clip = ec.attr_inputs(c.name)["sh_dc"], np.float32(c.clip)
        if sh.size >= 10:
            for v in (clip, -clip, np.nextafter(clip, np.float32(np.inf)), np.nextafter(-clip, np.float32(-np.inf))):
                assert (sh == v).any(), (c.name, v)
    # the special mesh: unreferenced vertices in the middle and at V - 1 with an exact zero gradient, a repeated index, a fan of 300
    inp, ref = ec.attr_inputs("attr-special-G3"), ec.attr_case_reference("attr-special-G3")
    V = len(inp["points"])
    lonely = sorted(set(range(V)) - set(inp["faces"].reshape(-1).tolist()))
    assert V - 1 in lonely and any(0 < v < V - 1 for v in lonely) and not ref["g_points"].s[lonely].any()
    assert (inp["faces"][:, 0] == inp["faces"][:, 1]).any()
    assert np.bincount(ec.attr_inputs("attr-fan300-G1")["faces"].reshape(-1))[0] == 300
    n = ref["colors"].v[ec.SPECIAL["collinear"][0] * 3, 3:]
    assert not n.any() and np.isfinite(ref["g_points"].v).all() and np.abs(ref["g_points"].v).max() > 1e12
    # the head
    shapes = {(c.H, c.W) for c in ec.HEAD_CASES}
    assert shapes == {(2, 2), (2, 64), (64, 2), (6, 10), (30, 34), (32, 32), (32, 34), (516, 512)}
    assert [ec.head_blocks(*s) for s in ((30, 34), (32, 32), (32, 34), (516, 512))] == [1, 1, 2, 256] and 516 * 512 > 4 * 256 * 256
    kinds = set()
    for c in ec.HEAD_CASES:
        inp = ec.head_inputs(c.name)
        b = ec.head_case_reference(c.name)["branches"] if c.name != ec.BIG else None
        kinds |= {(bool(0 <= r < c.n_ref), bool(0 <= n < c.n_rnd)) for r, n in zip(c.ref_pos, c.rnd_pos)}
        for v in ec.PLANT_ALPHA:
            assert (inp["alpha"] == v).any(), (c.name, v)
        for v in ec.PLANT_RGB[:5] if c.H * c.W == 4 else ec.PLANT_RGB:                      # (four pixels hold 12 colours)
            assert (inp["color"][:, :3] == v).any() and (np.signbit(inp["color"][:, :3]) & (inp["color"][:, :3] == 0)).any(), (c.name, v)
        if b is not None:
            assert both(b["solid"]) and both(b["lo"]) and both(b["hi"]) and both(b["live"]) and b["eq"].any()
            big = np.linalg.norm(inp["color"][:, 3:].astype(np.float64), axis=1)
            assert c.H * c.W == 4 or ((big > 9e17).any() and (big == 0).any() and ((big > 4e-13) & (big < 6e-13)).any())
    assert kinds == {(True, False), (False, True), (True, True), (False, False)}
    assert any(c.n_ref == 0 for c in ec.HEAD_CASES) and any(c.n_rnd == 0 for c in ec.HEAD_CASES) and any(c.B == 1 for c in ec.HEAD_CASES)
    assert any(c.n_ref == 2 and c.L == 4 and c.fidx == (3, 1) for c in ec.HEAD_CASES) and any(max(c.ref_pos) >= c.n_ref > 0 for c in ec.HEAD_CASES)
    assert any((ec.head_inputs(c.name)["ref_masks"] == np.float32(0.3)).any() for c in ec.HEAD_CASES)
    assert any(0.0 in c.g_terms and min(c.g_terms) < 0 for c in ec.HEAD_CASES) and any(not c.with_half and c.n_rnd for c in ec.HEAD_CASES)


def test_yardsticks_cover_the_float32_restatement_and_are_not_padded():
    worst, at = {}, {}
    for name in ATTR + HEAD:
        for k, v in ec.float32_ratios(name).items():
            if v > worst.get(k, -1.0):
                worst[k], at[k] = v, name
    print({k: (round(v, 4), at[k]) for k, v in worst.items()})
    assert worst.keys() == ec.YARD.keys()
    for k, v in worst.items():
        assert 0.8 * ec.YARD[k] <= v <= ec.YARD[k], (k, v, at[k], ec.YARD[k])


@pytest.mark.parametrize("mutant", ec.MUTANTS)
def test_a_one_token_mutant_of_the_float32_restatement_exceeds_its_bound(mutant):
    """The bounds are tight enough to catch what they exist to catch: each mutation is off by more than FACTOR x yardstick somewhere."""
    names = [n for n in ATTR + HEAD if n != ec.BIG]
    caught = {}
    for name in names:
        r = {k: v for k, v in ec.float32_ratios(name, (mutant,), ec.YARD).items() if v > 1.0}
        if r:
            caught[name] = r
    print(mutant, {n: {k: (v if np.isinf(v) else round(v, 1)) for k, v in r.items()} for n, r in list(caught.items())[:3]})
    assert caught, mutant
    clean = max(max(ec.float32_ratios(n, (), ec.YARD).values()) for n in names)
    assert clean <= 1.0 / ec.FACTOR + 1e-9
