"""Pins the float64 reference that tests/test_skinning_edges_gpu.py judges the skinning kernels by (CPU only).

* oracle/skinning.py's so3_log, so3_exp and the left-Jacobian coefficients in float64 against 50-digit arithmetic (mpmath)
  from |v| = 1e-12 to pi - 1e-6, exact 0 and both signs of w: 1e-12 relative.
* "exact" mode: float64 autograd against central differences, every magnitude class (rows with dr == 0 included).
* "pypose" mode: the hand-written SO3_Log / so3_Exp / SO3_Act rules are the left-perturbation derivatives they claim to be,
  at every magnitude class (near the identity, near pi, w < 0), not only at generic rotations.
* the float32 error floor (tests/skinning_edge_cases.py::F32_FLOOR) the kernels' bound is 8 x of, re-measured.
"""
import numpy as np
import pytest
import torch

from oracle import skinning as sk
from tests import skinning_edge_cases as ec

D = torch.float64


def _sweep():
    t = np.concatenate([[0.0], np.exp(np.linspace(np.log(1e-12), np.log(np.pi - 1e-6), 400)),
                        [1.19e-7, 1.2e-7, 9.99e-5, 1.01e-4, 9.99e-4, 1.001e-3, 0.0999, 0.1001, 0.2999, 0.3001, 3.0, 3.14, np.pi - 1e-6]])
    rng = np.random.default_rng(0)
    ax = rng.normal(size=(len(t), 3))
    return t, ax / np.linalg.norm(ax, axis=1, keepdims=True)


def test_oracle_log_exp_and_jacobians_against_50_digit_arithmetic():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    t, ax = _sweep()
    mpv = lambda row: [mp.mpf(float(c)) for c in row]
    rel = lambda got, want: max(abs(mp.mpf(float(g)) - w) for g, w in zip(got, want)) / max(max(abs(w) for w in want), mp.mpf(10) ** -300)
    worst = {"log": 0, "exp": 0, "c1": 0, "c2": 0, "c2inv": 0, "Jl": 0, "Jl_inv": 0}
    # Log on unit quaternions (sin(t/2) a, +-cos(t/2)): 2 atan(|v| / w) / |v| v of the float64 components as they are
    for sgn in (1.0, -1.0):
        q = torch.tensor(np.concatenate([np.sin(0.5 * t)[:, None] * ax, sgn * np.cos(0.5 * t)[:, None]], 1), dtype=D)
        out = sk.so3_log(q)
        assert torch.isfinite(out).all()
        for i in range(len(t)):
            x, y, z, w = mpv(q[i])
            u = mp.sqrt(x * x + y * y + z * z)
            f = 2 * mp.atan(u / w) / u if u > 0 else 2 / w
            worst["log"] = max(worst["log"], rel(out[i], [f * x, f * y, f * z])) if u > 0 else worst["log"]
            if u == 0:
                assert not out[i].any()
    x = torch.tensor(t[:, None] * ax, dtype=D)
    g = torch.tensor(np.random.default_rng(1).normal(size=(len(t), 3)), dtype=D)
    qe, jl, jli = sk.so3_exp(x), sk._row_times_Jl(x, g), sk._row_times_Jl_inv(x, g)
    t2 = (x * x).sum(-1, keepdim=True)
    (c1, c2), c2i = sk._jl_coeffs(t2), sk._jl_inv_coeff(t2)
    cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    for i in range(len(t)):
        xv, gv = mpv(x[i]), mpv(g[i])
        tt = mp.sqrt(mp.mpf(float(t2[i, 0])))                     # the coefficients are functions of the float64 t^2 handed in
        if tt == 0:
            assert torch.equal(qe[i], torch.tensor([0, 0, 0, 1.0], dtype=D)) and float(c1[i]) == 0.5
            assert torch.equal(jl[i], g[i]) and torch.equal(jli[i], g[i])
            continue
        tn = mp.sqrt(sum(c * c for c in xv))
        worst["exp"] = max(worst["exp"], rel(qe[i], [mp.sin(tn / 2) / tn * c for c in xv] + [mp.cos(tn / 2)]))
        m1, m2 = (1 - mp.cos(tt)) / tt ** 2, (tt - mp.sin(tt)) / tt ** 3
        mi = (1 - (tt / 2) * mp.cot(tt / 2)) / tt ** 2
        worst["c1"] = max(worst["c1"], abs(mp.mpf(float(c1[i])) / m1 - 1))
        worst["c2"] = max(worst["c2"], abs(mp.mpf(float(c2[i])) / m2 - 1))
        worst["c2inv"] = max(worst["c2inv"], abs(mp.mpf(float(c2i[i])) / mi - 1))
        n1, n2 = (1 - mp.cos(tn)) / tn ** 2, (tn - mp.sin(tn)) / tn ** 3
        ni = (1 - (tn / 2) * mp.cot(tn / 2)) / tn ** 2
        gk = cross(gv, xv)
        gkk = cross(gk, xv)
        worst["Jl"] = max(worst["Jl"], rel(jl[i], [a + n1 * b + n2 * c for a, b, c in zip(gv, gk, gkk)]))
        worst["Jl_inv"] = max(worst["Jl_inv"], rel(jli[i], [a - b / 2 + ni * c for a, b, c in zip(gv, gk, gkk)]))
    print({k: float(v) for k, v in worst.items()})
    assert all(v < 1e-12 for v in worst.values()), {k: float(v) for k, v in worst.items()}


def _loss(sc, method, mode, gx, gr, dr):
    t = lambda a: torch.tensor(a, dtype=D)
    trans, q, S, op = sk.node_attributes(t(sc["dx"]), dr, t(sc["ds"]), t(sc["do"])[:, None])
    xyz, rot = sk.skin_vertices(t(sc["verts"]), torch.tensor(sc["nbr_idx"]), t(sc["nbr_w"]), trans, q, S, op, method, grad_mode=mode)
    return (xyz * gx.to(D)).sum() + (rot * gr.to(D)).sum()


@pytest.mark.parametrize("cls", ec.CLASSES)
def test_exact_mode_autograd_against_central_differences(cls):
    """dL/d(dr) of a dozen nodes of one class.  Vertices within 1e-3 of the hybrid clamp are left out (a finite difference
    across the kink measures nothing); the step 1e-6 stays inside w's sign in the w ~ 0 class (|w| >= 1e-5)."""
    sc = ec.skin_scene([cls], 3, 30, M=12 + ec.N_UNREF, seed=3)
    h = 1e-6
    for method in ec.METHODS:
        gx, gr, _ = ec.skin_upstream(sc, method, clamp_margin=1e-3)
        dr = torch.tensor(sc["dr"], dtype=D).requires_grad_(True)
        _loss(sc, method, "exact", gx, gr, dr).backward()
        assert torch.isfinite(dr.grad).all(), (cls, method)                       # dr == 0: no NaN from norm() at zero
        fd = torch.zeros_like(dr)
        with torch.no_grad():
            for m in range(12):
                for c in range(4):
                    e = torch.zeros_like(dr)
                    e[m, c] = h
                    fd[m, c] = (_loss(sc, method, "exact", gx, gr, dr + e) - _loss(sc, method, "exact", gx, gr, dr - e)) / (2 * h)
        scale = float(dr.grad.abs().max())
        assert float((dr.grad - fd).abs().max()) < 1e-7 * scale + 1e-8, (cls, method, float((dr.grad - fd).abs().max()), scale)
        assert not dr.grad[12:].any()


@pytest.mark.parametrize("cls", ec.CLASSES)
def test_pypose_rules_are_left_perturbation_derivatives_at_every_magnitude(cls):
    """d/de <h, f(Exp(e) X)> at e = 0 by float64 central differences equals the rule's output, for SO3_Log and SO3_Act at
    rotations X of the class; so3_Exp reads its incoming storage gradient as the left-tangent gradient of its output, so
    Log's rule after Exp's hands a tangent gradient back unchanged (g Jl Jl^-1 = g) at rotation vectors of the class."""
    rng = np.random.default_rng(5)
    n = 24
    q = torch.tensor(ec.class_rows(cls, n, rng), dtype=D)
    q[:, 3] += 1.0
    q = torch.nn.functional.normalize(q, dim=-1)
    p, h = torch.tensor(rng.normal(size=(n, 3))), torch.tensor(rng.normal(size=(n, 3)))
    eps = 1e-6

    def pert(i, sgn):
        phi = torch.zeros(n, 3, dtype=D)
        phi[:, i] = sgn * eps
        return sk.quat_mul(sk.so3_exp(phi), q)

    qa = q.clone().requires_grad_(True)
    (sk._ActPP.apply(qa, p) * h).sum().backward()
    fd = torch.stack([((sk.quat_act(pert(i, +1), p) - sk.quat_act(pert(i, -1), p)) * h).sum(-1) / (2 * eps) for i in range(3)], -1)
    assert torch.allclose(qa.grad[:, :3], fd, rtol=0, atol=1e-8) and not qa.grad[:, 3].any()
    ql = q.clone().requires_grad_(True)
    (sk._LogPP.apply(ql) * h).sum().backward()
    fd = torch.stack([((sk.so3_log(pert(i, +1)) - sk.so3_log(pert(i, -1))) * h).sum(-1) / (2 * eps) for i in range(3)], -1)
    assert torch.isfinite(ql.grad).all()
    assert torch.allclose(ql.grad[:, :3], fd, rtol=0, atol=2e-8) and not ql.grad[:, 3].any()
    x = sk.so3_log(q).detach().requires_grad_(True)
    (sk._LogPP.apply(sk._ExpPP.apply(x)) * h).sum().backward()
    assert torch.allclose(x.grad, h, rtol=0, atol=1e-9)
    # and Exp's rule on its own: the left-tangent derivative of Exp at x is Jl(x): Exp(x + d) = Exp(Jl d) Exp(x) + O(d^2)
    d = torch.tensor(rng.normal(size=(n, 3)))
    xd = x.detach()
    lhs = sk.so3_log(sk.quat_mul(sk.so3_exp(xd + eps * d), sk.quat_conj(sk.so3_exp(xd)))) - \
        sk.so3_log(sk.quat_mul(sk.so3_exp(xd - eps * d), sk.quat_conj(sk.so3_exp(xd))))
    e3 = torch.eye(3, dtype=D)
    Jl = torch.stack([sk._row_times_Jl(xd, e3[j].expand(n, 3)) for j in range(3)], 1)      # row j = e_j Jl
    assert torch.allclose(lhs / (2 * eps), torch.einsum("nij,nj->ni", Jl, d), rtol=0, atol=1e-8)


def test_hybrid_scenes_straddle_the_clamp_and_exclude_next_to_nothing():
    for label, sc in ec.skin_cases("all"):
        if sc["V"] < 1000:
            continue
        ec.skin_upstream(sc, "hybrid")
        d = sc["eta"] - 1.0
        assert (np.abs(d) < ec.CLAMP_EXCLUDE).mean() <= 0.005, label
        assert (d > 1e-3).sum() > 100 and (d < -1e-3).sum() > 100, label
        assert ((d > 0) & (d < 1e-3)).sum() >= 10 and ((d < 0) & (d > -1e-3)).sum() >= 10, label


def test_clamp_equality_vertices_sit_exactly_at_the_clamp_and_keep_their_gradient():
    """eta + 0.4f == 1 exactly, in float64 on the widened inputs and in float32 in the kernels' order of additions; such a vertex is
    NOT left out (only 0 < |eta + 0.4f - 1| < 1e-6 is), torch.clamp passes the gradient there, and the float64 oracle (whose double
    0.4 puts it 6e-9 below the bound) passes it too: dL/d(d_opacity) of the two nodes carries the vertices' x_lbs - x_dqs term."""
    x = torch.tensor(np.float32(0.6), requires_grad=True)
    torch.clamp(x + 0.4, max=1.0).backward()
    assert x.grad.item() == 1.0
    for K in (2, 4):
        sc = ec.clamp_equality_scene(K)
        eq = sc["eq_vertices"]
        gx, gr, keep = ec.skin_upstream(sc, "hybrid")
        assert (sc["eta"][eq] == 1.0).all() and keep[eq].all() and float(gx[eq].abs().min()) > 0
        near = (np.abs(sc["eta"] - 1.0) < ec.CLAMP_EXCLUDE) & (sc["eta"] != 1.0)
        assert not keep[near].any()
        h, c04 = np.float32(0.5), np.float32(0.4)
        assert (sc["do"][:2] == 0).all() and 1.0 / (1.0 + np.exp(-np.float32(0))) == 0.5
        for v in eq:
            w = sc["nbr_w"][v]
            acc = np.float32(0)
            for k in range(K):                                   # skinning.hip: eta += w * o, slot by slot; quad_sum adds the same two
                acc = np.float32(acc + np.float32(w[k] * h))     # non-zero terms
            assert np.float32(acc + c04) == np.float32(1.0) and not w[2:].any()
        # the gradient the `<` form dropped: with the equality vertices' upstream gradient alone, dL/d(d_opacity) of nodes 0 and 1
        only = torch.zeros_like(gx)
        only[eq] = gx[eq]
        _, _, g = ec.skin_reference(sc, "hybrid", "exact", only, torch.zeros_like(gr))
        s = ec.skin_row_scale(sc, only, torch.zeros_like(gr))
        assert (np.abs(g["do"][:2, 0]) > 100 * ec.KERNEL_BOUND * s[:2]).all(), (g["do"][:2, 0], s[:2])


def _floor_cases():
    for which in ["all"] + ec.CLASSES:
        yield from ((which, "skin", l, s) for l, s in ec.skin_cases(which))
        yield from ((which, "face", l, s) for l, s in ec.face_cases(which))


def test_float32_floor_of_the_oracle_formulas():
    """Measures ec.F32_FLOOR: the oracle's formulas evaluated in float32 against their float64 evaluation, worst per-element
    ratio over every case the GPU test runs.  Also: the float64 reference is finite everywhere."""
    worst = {}
    for which, kind, label, sc in _floor_cases():
        for mode in ec.MODES:
            if kind == "skin":
                for method in ec.METHODS:
                    gx, gr, _ = ec.skin_upstream(sc, method)
                    s = ec.skin_row_scale(sc, gx, gr)
                    x64, r64, g64 = ec.skin_reference(sc, method, mode, gx, gr)
                    _, _, g32 = ec.skin_reference(sc, method, mode, gx, gr, torch.float32)
                    assert np.isfinite(x64).all() and np.isfinite(r64).all() and all(np.isfinite(v).all() for v in g64.values())
                    r = max(ec.skin_ratios(sc, method, g32, g64, s).values())
                    worst[(which, mode)] = max(worst.get((which, mode), 0.0), r)
            else:
                gm, gq, gn = ec.face_upstream(sc)
                sx, sr = ec.face_row_scales(sc, gm, gq, gn)
                a, b = ec.face_reference(sc, mode, gm, gq, gn), ec.face_reference(sc, mode, gm, gq, gn, torch.float32)
                assert all(np.isfinite(v).all() for v in a)
                V0 = sc["V0"]
                r = max(ec.worst_ratio(b[3][:V0], a[3][:V0], sx[:V0]), ec.worst_ratio(b[4], a[4], sr))
                worst[(which, mode)] = max(worst.get((which, mode), 0.0), r)
    print({f"{k[0]}/{k[1]}": f"{v:.2e}" for k, v in worst.items()})
    top = max(worst.values())
    assert top <= ec.F32_FLOOR, (top, worst)
    assert top >= ec.F32_FLOOR / 2, "F32_FLOOR is stale: re-measure it (the bound must follow the reference, not drift above it)"
    assert ec.KERNEL_BOUND == 8 * ec.F32_FLOOR
