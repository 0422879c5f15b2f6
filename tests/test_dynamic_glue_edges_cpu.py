"""Pins the references, the cases and the bounds that tests/test_dynamic_glue_edges_gpu.py judges csrc/imagehead.hip, csrc/dscale.hip and
csrc/sds_glue.hip by (CPU only, no library call).

* The closed-form references (tests/dynamic_glue_edges.py) against float64 torch autograd through the compositions the project keeps:
  `F.mse_loss` and `F.interpolate(mode="bilinear", align_corners=False)` for the image head, `oracle.skinning.vertex_scales` and
  `gaussian_scales` for d_scale -- every value and gradient element within 64 float64 roundings of its scale.  Two constants reach
  the kernels as float32 and the torch compositions as doubles; both are accounted for in closed form, not by a tolerance: the means'
  normalisation factor (the reference's mean is torch's times float32(1 / d) d) and the hybrid clamp's 0.4 (the oracle's diagonal is
  the reference's plus 0.4 - 0.4f wherever the clamp is not active; the margins make float64 decide every clamp the same way, and at
  the equality vertices the oracle is 6e-9 below the bound: the gradient passes there too).
* float32 restatement and float64 reference take identical branches; every margin and equality assertion of the cases holds in both.
* The yardsticks cover the float32 restatement and are not padded: 0.8 x constant <= measured <= constant.
* The SDS restatement against torch float16 autograd on the CPU: latents bit-identical, d_moments within the two caps on every case.
"""
from unittest import mock

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dynamic_glue_edges as ec

R64 = 64 * 2.0 ** -53
HEAD_PINS = [(c.name, v) for c in ec.HEAD_CASES for v in ec.head_variants(c.name)]
DS_PINS = [(c.name, m) for c in ec.DS_CASES for m in ec.DS_METHODS]


def _pinned(got, ref, what):
    got = np.asarray(got, np.float64).reshape(ref.v.shape)
    bad = np.abs(got - ref.v) > R64 * ref.s
    i = np.unravel_index(int(np.abs(got - ref.v).argmax()), got.shape) if got.size else ()
    assert not bad.any(), f"{what}: {int(bad.sum())} of {got.size} elements; e.g. {i}: torch {got[i]!r}, closed form {ref.v[i]!r}, scale {ref.s[i]:.3g}"


@pytest.mark.parametrize("name,var", HEAD_PINS, ids=[f"{n}-{''.join('rmh'[i] for i in range(3) if v[i]) or 'none'}" for n, v in HEAD_PINS])
def test_head_reference_equals_float64_autograd_through_mse_loss_and_interpolate(name, var):
    case, inp, ref = ec.HEAD_BY_NAME[name], ec.head_inputs(name, *var), ec.head_case_reference(name, *var)
    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    c, a = t(inp["color"]).requires_grad_(True), t(inp["alpha"]).requires_grad_(True)
    B, C, H, W = c.shape
    n_ref, n_rnd = case.n_ref, case.n_rnd
    rgb = c[:, :3].clamp(0, 1)
    ref_v = sorted((int(r), v) for v, r in enumerate(inp["ref_pos"]) if 0 <= r < n_ref)
    rnd_v = [v for _, v in sorted((int(n), v) for v, n in enumerate(inp["rnd_pos"]) if 0 <= n < n_rnd)]
    assert [r for r, _ in ref_v] == list(range(n_ref)) and len(rnd_v) == n_rnd
    loss, mse = c.sum() * 0 + a.sum() * 0, [torch.zeros((), dtype=torch.float64)] * 2
    if ref_v:
        vs = [v for _, v in ref_v]
        gt = torch.stack([t(inp["ref_images"][int(inp["fidx_ref"][r])]) for r, _ in ref_v])
        gm = torch.stack([t(inp["ref_masks"][int(inp["fidx_ref"][r])]) for r, _ in ref_v])
        mse = [F.mse_loss(gt, rgb[vs].permute(0, 2, 3, 1)), F.mse_loss(a[vs].permute(0, 2, 3, 1), gm)]
        for g, m in zip((inp["g_rgb"], inp["g_mask"]), mse):
            if g is not None:
                loss = loss + float(g) * m
    half = torch.zeros(0, H // 2, W // 2, 3, dtype=torch.float64)
    if rnd_v:
        half = F.interpolate(rgb[rnd_v], (H // 2, W // 2), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
        if inp["g_half"] is not None:
            loss = loss + (half * t(inp["g_half"])).sum()
    gc, ga = torch.autograd.grad(loss, (c, a))
    d = float(max(n_ref, 1) * H * W)
    m_rgb, m_mask = ec.head_matrix(n_ref, H, W)
    _pinned(torch.stack([mse[0] * (float(m_rgb) * 3.0 * d), mse[1] * (float(m_mask) * d)]).detach(), ref["means"], "means")
    _pinned(half.detach(), ref["half"], "half")
    _pinned(gc, ref["g_color"], "g_color")
    _pinned(ga, ref["g_alpha"], "g_alpha")
    # the partial sums are the means' sums, workgroup by workgroup
    assert ref["partial"].v.shape == (B, ec.head_blocks(H, W), 2)
    assert np.allclose(ref["partial"].v.sum((0, 1)) * [float(m_rgb), float(m_mask)], ref["means"].v, rtol=1e-12, atol=0)
    for v, (is_ref, is_rnd) in enumerate(ref["roles"]):
        if not is_ref:
            assert not ref["partial"].v[v].any() and not ref["partial"].s[v].any() and not ref["g_alpha"].s[v].any()
        if not is_ref and not is_rnd:
            assert not ref["g_color"].v[v].any() and not ref["g_color"].s[v].any()
    assert not ref["g_color"].s[:, 3:].any() and not ref["g_color"].v[:, 3:].any()
    if not var[1]:
        assert not ref["g_alpha"].v.any() and not ref["g_alpha"].s.any()                # null g_mask: exactly 0
    if not var[0] and not (var[2] and n_rnd):
        assert not ref["g_color"].s.any()
    out = (inp["color"][:, :3] < 0) | (inp["color"][:, :3] > 1)
    assert not ref["g_color"].s[:, :3][out].any()                                        # one float outside [0, 1]: exactly 0


def test_the_head_cases_cover_every_role_size_and_branch_value():
    roles = set()
    for c in ec.HEAD_CASES:
        assert c.B <= 6 and c.C in (3, 6)
        inp = ec.head_inputs(c.name)
        roles |= {tuple(r) for r in ec.head_case_reference(c.name)["roles"].tolist()}
        col = inp["color"][:, :3]
        for v in ec.PLANT_RGB[:5] if c.H * c.W == 4 else ec.PLANT_RGB:
            assert (col == v).any(), (c.name, v)
        rnd = [v for v, n in enumerate(c.rnd_pos) if 0 <= n < c.n_rnd]
        if rnd and c.H * c.W > 4:                                   # the same colours inside the 2 x 2 blocks of random views
            for v in ec.PLANT_RGB:
                assert (col[rnd] == v).any(), (c.name, v)
    assert roles == {(True, False), (False, True), (True, True), (False, False)}
    assert {(c.H, c.W) for c in ec.HEAD_CASES} == {(2, 2), (30, 34), (64, 2), (516, 512)} and {c.C for c in ec.HEAD_CASES} == {3, 6}
    assert sum(c.name == ec.BIG for c in ec.HEAD_CASES) == 1 and len(ec.head_variants(ec.BIG)) == 1
    assert [ec.head_blocks(*s) for s in ((2, 2), (30, 34), (64, 2), (516, 512))] == [1, 1, 1, 256] and (516 * 512 + 1023) // 1024 > 256
    assert (30 * 34) % 256 and (15 * 17) % 256 and (516 * 512) % (256 * 256)
    assert any(c.n_ref == 0 for c in ec.HEAD_CASES) and any(c.n_rnd == 0 for c in ec.HEAD_CASES)
    assert any(max(c.ref_pos) >= c.n_ref > 0 for c in ec.HEAD_CASES) and any(len(set(c.fidx)) < len(c.fidx) for c in ec.HEAD_CASES)


def test_loss_sum_references():
    from dreammesh4d_amd.loss_sum import weighted_sum

    assert {n for n, _, _ in ec.PSUM_CASES} == {0, 1, 255, 256, 257, 1000} and {k for _, k, _ in ec.PSUM_CASES} == {1, 3, 8} == {m for _, _, m in ec.PSUM_CASES}
    for n, k, m in ec.PSUM_CASES:
        partial, mat = ec.psum_inputs(n, k, m)
        ref = ec.psum_reference(n, k, m)
        _pinned((torch.tensor(partial.astype(np.float64)).sum(0) @ torch.tensor(mat.astype(np.float64))).numpy(), ref, f"psum {n} {k} {m}")
        assert k * m == 1 or ((mat == 0).any() and (mat < 0).any())
        assert n or (not ref.v.any() and not ref.s.any())
    for name, pairs in ec.wsum_cases().items():                     # the product's CPU path IS the torch float32 expression
        want, gw = ec.wsum_reference(pairs, 1.3)
        terms = [torch.tensor(t, requires_grad=True) for _, t in pairs]
        out = weighted_sum([(w, t) for (w, _), t in zip(pairs, terms)])
        assert out.dtype == torch.float32 and out.item() == float(want), name
        out.backward(torch.tensor(np.float32(1.3)))
        assert np.array_equal(np.concatenate([t.grad.numpy().reshape(-1) for t in terms]), gw), name
        assert len(gw) == {"n1": 1, "n16": 16}[name]
    w16 = [w for wi, _ in ec.wsum_cases()["n16"] for w in np.atleast_1d(wi)]
    assert 0.0 in w16 and min(w16) < 0


@pytest.mark.parametrize("name,method", DS_PINS, ids=[f"{n}-{m}" for n, m in DS_PINS])
def test_d_scale_reference_equals_float64_autograd_through_the_oracle(name, method):
    from oracle import skinning as sk

    case, inp, ref = ec.DS_BY_NAME[name], ec.ds_inputs(name, method), ec.ds_case_reference(name, method)
    D = torch.float64
    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    idx, w, faces = torch.tensor(inp["idx"]), t(inp["w"]), torch.tensor(inp["faces"])
    ds, do = t(inp["ds"]).requires_grad_(True), t(inp["dop"]).requires_grad_(True)
    NF, M = case.NF, case.M
    Sv = []
    for f in range(NF):
        _, _, Sm, op = sk.node_attributes(torch.zeros(M, 3, dtype=D), torch.zeros(M, 4, dtype=D), ds[f], do[f].reshape(M, 1))
        Sv.append(sk.vertex_scales(idx, w, Sm, op, method))
    Sv = torch.stack(Sv)
    g_ds, g_do = torch.autograd.grad((Sv * t(inp["g_Sv"])).sum(), (ds, do), allow_unused=True)
    shift = np.zeros(Sv.shape)
    if method == "hybrid":                                           # the oracle adds the double 0.4, the kernels 0.4f
        shift = (0.4 - float(ec.C04)) * ref["unclamped"][..., None, None] * np.eye(3)
        lw = ref["lw"]
        assert ((lw > 1 + 1e-4) | (lw < 1 - 1e-4) | (lw == 1)).all()
    _pinned(Sv.detach().numpy() + shift, ref["Sv"], "Sv")
    _pinned(g_ds, ref["g_ds"], "g_ds")
    _pinned(torch.zeros_like(do) if g_do is None else g_do, ref["g_dop"], "g_dop")
    sv_in, scaling = t(inp["sv_in"]).requires_grad_(True), t(inp["scaling"]).requires_grad_(True)
    with mock.patch.object(sk, "bary_table", lambda n, dtype=D: t(inp["bary"]).to(dtype)):           # the float32 table the kernels read
        gs = torch.stack([sk.gaussian_scales(faces, case.G, sv_in[f], scaling) for f in range(NF)])
    g_sv, g_sc = torch.autograd.grad((gs * t(inp["g_gs"])).sum(), (sv_in, scaling))
    _pinned(gs.detach(), ref["gscales"], "gscales")
    _pinned(g_sv, ref["g_sv"], "g_sv")
    _pinned(g_sc, ref["g_scaling"], "g_scaling")


def test_clamp_equality_is_exact_in_both_precisions_and_torch_passes_the_gradient_there():
    w, c04 = ec.W_EQ, ec.C04
    assert float(w) == 3355443 * 2.0 ** -24 and float(c04) * 2 ** 25 == 13421773
    assert (0.5 * 1.0 + 0.5 * float(w)) + float(c04) == 1.0                                           # float64 on the widened inputs
    h = np.float32(0.5)
    assert np.float32(np.float32(h * np.float32(1)) + np.float32(h * w)) + c04 == np.float32(1.0)      # float32, the kernel's order
    x = torch.tensor(np.float32(0.6), requires_grad=True)
    y = torch.clamp(x + 0.4, max=1.0)
    y.backward()
    assert y.item() == 1.0 and x.grad.item() == 1.0
    seen = {"below": 0, "above": 0, "equal": 0}
    for c in ec.DS_CASES:
        a, b = ec.ds_case_reference(c.name, "hybrid"), ec.ds_float32(c.name, "hybrid")       # (both assert the margins and the equality)
        inp = ec.ds_inputs(c.name, "hybrid")
        assert np.array_equal(a["unclamped"], b["unclamped"]), c.name
        eq = inp["eq_vertices"]
        assert (a["lw"][:, eq] == 1).all() and (b["lw"][:, eq] == 1).all() and a["unclamped"][:, eq].all()
        assert len(eq) == (2 if c.K >= 2 else 0)
        seen["below"] += int((a["lw"] < 1).sum())
        seen["above"] += int((a["lw"] > 1).sum())
        seen["equal"] += int((a["lw"] == 1).sum())
    assert all(v >= 8 for v in seen.values()), seen


def test_the_d_scale_cases_cover_the_adjacency_and_the_other_edges():
    assert {c.K for c in ec.DS_CASES} == {1, 2, 4} and {c.G for c in ec.DS_CASES} == {1, 6} and {c.NF for c in ec.DS_CASES} == {1, 3}
    assert max(c.M for c in ec.DS_CASES) <= 12
    assert sorted(ec.ds_mesh(c.mesh)[0] for c in ec.DS_CASES).count(257) == 1
    assert sorted(len(ec.ds_mesh(c.mesh)[1]) * c.G for c in ec.DS_CASES).count(258) == 1
    valences = set()
    for c in ec.DS_CASES:
        V, faces = ec.ds_mesh(c.mesh)
        val = np.bincount(faces.reshape(-1), minlength=V)
        valences |= set(val.tolist())
        for method in ec.DS_METHODS:
            inp, ref = ec.ds_inputs(c.name, method), ec.ds_case_reference(c.name, method)
            refd = np.bincount(inp["idx"].reshape(-1), minlength=c.M)
            assert refd[c.M - 1] == 0 and not ref["g_ds"].s[:, c.M - 1].any() and not ref["g_dop"].s[:, c.M - 1].any()      # an empty CSR row
            lonely = np.flatnonzero(val == 0)
            assert not ref["g_sv"].s[:, lonely].any() and not ref["g_sv"].v[:, lonely].any()
            if c.mesh in ("patch", "fan43"):
                assert len(lonely) == 1
            if c.K >= 2:
                assert refd[0] >= V and (inp["idx"][1, 0] == inp["idx"][1, 1])                 # a hub node; one node in two slots
            if method == "hybrid" and c.M > 3:
                assert (inp["dop"][:, 2] == 20).all() and (inp["dop"][:, 3] == -20).all()
                f32 = ec.ds_float32(c.name, method)
                assert not f32["g_dop"].v[:, 2].any() and (refd[3] == 0 or f32["g_dop"].v[:, 3].any())
                clamped = ~ref["unclamped"]
                assert clamped.any() or c.mesh == "tiny"
            if method == "lbs" and c.NF == 3:                          # no strain, weights that add up to exactly 1: exactly I
                rows = [4, 5] if c.K >= 2 else [0, 1]
                assert np.array_equal(ref["Sv"].v[2, rows], np.broadcast_to(np.eye(3), (2, 3, 3)))
                assert np.array_equal(ec.ds_float32(c.name, method)["Sv"].v[2, rows], np.broadcast_to(np.eye(3, dtype=np.float32), (2, 3, 3)))
    assert 1 in valences and 43 in valences and 0 in valences


def test_yardsticks_cover_the_float32_restatement_and_are_not_padded():
    worst = ec.float32_ratios()
    print({k: (round(float(v), 4), at) for k, (v, at) in worst.items()})
    assert worst.keys() == ec.YARD.keys()
    for k, (v, at) in worst.items():
        assert 0.8 * ec.YARD[k] <= v <= ec.YARD[k], (k, v, at, ec.YARD[k])


def _torch_half_graph(inp):
    """The torch float16 operators the glue kernels replace (zero123's op-by-op step), with autograd, on the CPU."""
    B = inp["moments"].shape[0]
    moments = torch.tensor(inp["moments"]).requires_grad_(True)
    post, noise, pred = torch.tensor(inp["post"]), torch.tensor(inp["noise"]), torch.tensor(inp["pred"])
    alphas, t = torch.tensor(inp["alphas"]), torch.tensor(inp["t"])
    mean, logvar = moments.chunk(2, dim=1)
    latents = (inp["scale_factor"] * (mean + torch.exp(0.5 * logvar.clamp(-30.0, 20.0)) * post)).to(torch.float32)
    with torch.no_grad():
        ac = alphas[t].view(-1, 1, 1, 1)
        noisy = ac.sqrt() * latents + (1 - ac).sqrt() * noise
        unc, cnd = pred.float().chunk(2)
        grad = torch.nan_to_num((1 - ac) * ((unc + inp["guidance_scale"] * (cnd - unc)) - noise))
        if inp["clip"] is not None:
            grad = grad.clamp(-inp["clip"], inp["clip"])
        target = latents - grad
    loss = 0.5 * F.mse_loss(latents, target, reduction="sum") / B
    (dm,) = torch.autograd.grad(loss, moments)
    return latents.detach().numpy(), noisy.half().numpy(), dm.numpy(), float(loss.detach()), float(grad.norm())


@pytest.mark.parametrize("name", [c.name for c in ec.SDS_CASES])
def test_sds_restatement_against_torch_float16_autograd_on_the_cpu(name):
    case, inp, rs = ec.SDS_BY_NAME[name], ec.sds_inputs(name), ec.sds_case_restatement(name)
    B = case.B
    assert ec.logvar_is_safe(inp["moments"][:, 4:]).all()
    lat, noisy, dm, loss, gnorm = _torch_half_graph(inp)
    assert np.array_equal(lat, rs["latents"]) and np.isfinite(lat).all()
    assert np.array_equal(noisy, rs["x_in"][:B, :4]) and np.array_equal(noisy, rs["x_in"][B:, :4])
    assert not rs["x_in"][:B, 4:].any() and np.array_equal(rs["x_in"][B:, 4:], inp["c_concat"][inp["fidx"]])
    share, ulps = ec.half_mismatch(dm, rs["d_moments"])
    print(name, "d_moments: share", share, "ulps", ulps)
    assert share <= 1e-3 and ulps <= 2.0, (share, ulps)
    lv = inp["moments"][:, 4:].astype(np.float32)
    out = (lv < -30) | (lv > 20)
    assert np.array_equal(~out, rs["inside"]) and not rs["d_moments"][:, 4:][out].any() and not dm[:, 4:][out].any()
    l64, n64 = ec.sds_sums(rs, B)
    l32, _ = ec.sds_sums(rs, B, np.float32)
    if np.isfinite(l32):
        assert abs(loss - l64) <= ec.FACTOR * ec.YARD["sds_loss"] * ec.U * l64 and abs(gnorm - n64) <= ec.FACTOR * ec.YARD["sds_norm"] * ec.U * n64
    else:
        assert case.clip is None and case.special == "nonfinite" and np.isinf(loss) and np.isinf(gnorm)


def test_the_sds_cases_cover_the_shapes_values_and_layouts():
    assert {(c.B, c.H, c.W) for c in ec.SDS_CASES} == {(1, 1, 1), (3, 4, 6), (2, 6, 4), (3, 32, 32)}
    assert any(c.clip is None for c in ec.SDS_CASES) and any(len(set(c.fidx)) < len(c.fidx) for c in ec.SDS_CASES)
    seen_lv = set()
    for i, c in enumerate(ec.SDS_CASES):
        inp, rs = ec.sds_inputs(c.name), ec.sds_case_restatement(c.name)
        seen_lv |= {v for v in ec.LV_PLANTED if (inp["moments"][:, 4:] == v).any()}
        if c.B * c.H * c.W > 1:
            assert 0 in c.t or ec.T_STEPS - 1 in c.t
            assert {ec.sds_layout(i, t) for t in ec.SDS_TENSORS} == set(ec.LAYOUTS)
        if c.special == "nonfinite":
            p = inp["pred"].astype(np.float32)
            assert np.isnan(p).any() and (p == np.inf).any() and (p == -np.inf).any()
            assert (np.abs(rs["g"]) == (ec.FLT_MAX if inp["clip"] is None else np.float32(inp["clip"]))).any()
        if c.clip == "element":
            g = np.abs(rs["g"])
            assert (g == np.float32(inp["clip"])).sum() > 10 and (g < np.float32(inp["clip"])).sum() > 10
            unclipped = np.abs(ec.sds_restate(dict(inp, clip=None))["g"])
            assert (unclipped == np.float32(inp["clip"])).any()                              # |g| == clip exactly, before the clip
    assert seen_lv == set(ec.LV_PLANTED)
    assert {c.t[j] for c in ec.SDS_CASES for j in range(c.B)} >= {0, ec.T_STEPS - 1}
    for t in ec.SDS_TENSORS:
        assert {ec.sds_layout(i, t) for i in range(len(ec.SDS_CASES))} == set(ec.LAYOUTS), t
