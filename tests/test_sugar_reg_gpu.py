"""SuGaR density and normal regularisation on the device, judged element by element: |got - f64| <= 4 * unit, where unit is the
reference's own float32 error for that tensor (``err_ref`` of the golden fixture; elsewhere the error of the reference's
expressions in float32 torch on the CPU), never less than half an ulp of the tensor's largest magnitude."""
import types

import numpy as np
import pytest
import torch

from dreammesh4d_amd import gaussian_model as gm, sugar_reg as sr
from tests import sugar_reg_common as cm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FACTOR = 4.0
KEYS = cm.PER_SAMPLE + ("loss_d", "loss_n") + cm.GRADS


@pytest.fixture(scope="module")
def z():
    return cm.golden()


def device_run(inp, with_normal, upstream=(1.0, 1.0), grad=(True, True, True, True), **kw):
    """The operator on `inp` -> the keys of cm.restate as float32 numpy arrays (a gradient that was not asked for is None)."""
    leaves = [torch.from_numpy(np.ascontiguousarray(inp[k])).to(DEV).requires_grad_(g) for k, g in zip(cm.INPUTS[:4], grad)]
    rest = [torch.from_numpy(np.ascontiguousarray(inp[k])).to(DEV) for k in cm.INPUTS[4:]]
    out = sr.sugar_density_reg(*leaves, *rest, with_normal_loss=with_normal, **kw)
    assert out.density_regulation.ndim == 0 and (out.normal_regulation is None) == (not with_normal)
    assert not out.density.requires_grad and not out.density_term.requires_grad
    total = upstream[0] * out.density_regulation + (upstream[1] * out.normal_regulation if with_normal else 0.0)
    total.backward()
    torch.cuda.synchronize()
    f = lambda t: None if t is None else t.detach().cpu().numpy()
    got = {"density": f(out.density), "beta": f(out.beta), "density_term": f(out.density_term), "loss_d": f(out.density_regulation),
           "normal_term": f(out.normal_term) if with_normal else np.zeros(len(inp["sample_idx"]), np.float32),
           "loss_n": f(out.normal_regulation) if with_normal else np.zeros((), np.float32)}
    for name, t in zip(cm.GRADS, leaves):
        got[name] = f(t.grad)
    return got


def within(got, f64, unit, what):
    """Per element |got - f64| <= FACTOR * unit; prints and returns the largest ratio."""
    g, w = np.asarray(got, np.float64), np.asarray(f64, np.float64).reshape(np.shape(got))
    assert np.isfinite(g).all(), f"{what}: non-finite values"
    err = float(np.abs(g - w).max()) if g.size else 0.0
    ratio = err / unit
    print(f"{what}: max |got - f64| = {err:.3e}, unit = {unit:.3e}, ratio = {ratio:.3f} (bound {FACTOR})")
    assert ratio <= FACTOR, f"{what}: max error {err:.3e} is {ratio:.2f} x unit = {unit:.3e} (bound {FACTOR})"
    return ratio


def check(inp, with_normal, what, upstream=(1.0, 1.0), grad=(True, True, True, True)):
    """The device against the restatement, the unit from the reference's expressions in float32 on the CPU."""
    f64 = cm.restate(inp, with_normal, upstream, bounds=cm.F32_BOUNDS)
    ref32 = cm.torch_expressions(inp, with_normal, upstream, torch.float32)
    got = device_run(inp, with_normal, upstream, grad)
    for k in KEYS:
        if got[k] is None:
            continue
        within(got[k], f64[k], cm.unit_of(ref32, f64, k), f"{what} {k}")
    return got, f64


# ------------------------------------------------------------------------------------------------ the golden case
@pytest.fixture(scope="module")
def golden_runs(z):
    """The device's results for the golden inputs, computed once: with the normal loss per upstream, and without it."""
    inp = cm.golden_inputs(z)
    runs = {tag: device_run(inp, True, up) for tag, up in cm.UPSTREAMS.items()}
    runs["plain"] = device_run(inp, False, (1.0, 0.0))
    return runs


def half_ulp(a):
    return 0.5 * float(np.spacing(np.float32(np.abs(a).max())))


@pytest.mark.parametrize("tag", ["d", "n", "dn", "plain"])
def test_golden_case(z, golden_runs, tag):
    got = golden_runs[tag]
    gtag = "d" if tag == "plain" else tag
    for k in cm.PER_SAMPLE + ("loss_d", "loss_n"):
        if tag == "plain" and k in ("normal_term", "loss_n"):
            assert not np.any(got[k])
            continue
        within(got[k], z[k], max(float(z[k + "_err_ref"]), half_ulp(z[k])), f"golden {tag} {k}")
    for k in cm.GRADS:
        key = f"{gtag}/{k}"
        within(got[k], z[key], max(float(z[key + "_err_ref"]), half_ulp(z[key])), f"golden {tag} {k}")


def test_golden_zero_upstream_leaves_the_other_term_alone(z, golden_runs):
    """With the normal term's upstream at 0 the gradients are the density term's, bit for bit those of the call without the
    normal loss; with the density term's at 0 only quaternions receive anything."""
    for k in cm.GRADS:
        assert np.array_equal(golden_runs["d"][k], golden_runs["plain"][k]), k
    for k in ("d_xyz", "d_scales", "d_opac"):
        assert not np.any(golden_runs["n"][k]), k
    assert np.any(golden_runs["n"]["d_quats"])
    for k in cm.PER_SAMPLE[:3] + ("loss_d",):
        assert np.array_equal(golden_runs["dn"][k].view(np.uint32), golden_runs["plain"][k].view(np.uint32)), k


def test_golden_two_calls_are_bit_equal(z, golden_runs):
    again = device_run(cm.golden_inputs(z), True, cm.UPSTREAMS["dn"])
    for k in KEYS:
        assert np.array_equal(again[k].view(np.uint32), golden_runs["dn"][k].view(np.uint32)), k


def test_golden_permuted_samples(z, golden_runs):
    """sample_idx permuted together with eps: the per-sample arrays are permuted bit for bit."""
    inp = dict(cm.golden_inputs(z))
    perm = np.random.default_rng(5).permutation(len(inp["sample_idx"]))
    inp["sample_idx"], inp["eps"] = inp["sample_idx"][perm], inp["eps"][perm]
    got = device_run(inp, True, cm.UPSTREAMS["dn"])
    for k in cm.PER_SAMPLE:
        assert np.array_equal(got[k].view(np.uint32), golden_runs["dn"][k][perm].view(np.uint32)), k


# ------------------------------------------------------------------------------------------------ the smallest shapes
def _self_only(n, s, seed):
    inp = cm.random_case(n, 1, s, seed)
    inp["knn_idx"] = np.arange(n, dtype=np.int32)[:, None]
    return inp


def _one_gaussian(seed):
    inp = cm.random_case(50, 8, 1000, seed)
    inp["sample_idx"][:] = 7
    return inp


def _hub(seed):
    inp = cm.random_case(1100, 4, 2200, seed, knn="random")
    inp["knn_idx"][:, 1] = 0
    return inp


def _listed_by_itself(seed):
    inp = cm.random_case(40, 6, 300, seed, knn="random")
    t = inp["knn_idx"]
    t[t == 5] = 6
    t[5, 0] = 5
    inp["sample_idx"][:20] = 5
    return inp


def _repeated_row(seed):
    inp = cm.random_case(40, 6, 300, seed)
    inp["knn_idx"][3, :] = 7
    inp["knn_idx"][9, 1:] = 9
    inp["sample_idx"][:30] = 3
    inp["sample_idx"][30:50] = 9
    return inp


SHAPES = {
    "K = 1, self only": lambda: _self_only(20, 50, 1),
    "K = 32, N = 33": lambda: cm.random_case(33, 32, 100, 2),
    "N = 17, K = 16": lambda: cm.random_case(17, 16, 100, 3),
    "S = 1": lambda: cm.random_case(30, 8, 1, 4),
    "S = 1000 in one Gaussian": lambda: _one_gaussian(5),
    "hub of in-degree 1100": lambda: _hub(6),
    "listed by nobody but itself": lambda: _listed_by_itself(7),
    "a row repeating one neighbour": lambda: _repeated_row(8),
    "N = 257, S = 257": lambda: cm.random_case(257, 3, 257, 9, knn="random"),
    "N K = 258, S = 4097": lambda: cm.random_case(129, 2, 4097, 10, knn="random"),
    "S = 17: one chunk and one sample": lambda: dict(cm.random_case(5, 5, 17, 11), sample_idx=np.full(17, 2, np.int32)),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes(name):
    inp = SHAPES[name]()
    check(inp, True, name)


def test_empty_segments_get_exactly_zero():
    """S = 70 among N = 400: a Gaussian that holds no sample and is listed by no sampled Gaussian receives exactly zero."""
    inp = cm.random_case(400, 16, 70, 12)
    got, _ = check(inp, True, "S = 70, N = 400")
    touched = np.zeros(400, bool)
    touched[inp["sample_idx"]] = True
    touched[inp["knn_idx"][inp["sample_idx"]].reshape(-1)] = True
    assert (~touched).sum() > 20
    for k in cm.GRADS:
        assert not np.any(got[k][~touched]), k
    check(inp, False, "S = 70, N = 400, no normal loss", upstream=(1.0, 0.0))


# ------------------------------------------------------------------------------------------------ branch points
B8 = np.float32(1e-8)


def _clamp_case(special):
    """Gaussian 0 at the origin with the scales `special`; it holds a third of the samples and every row lists it."""
    inp = cm.random_case(12, 4, 90, 20)
    inp["xyz"][0] = 0.0
    inp["scales"][0] = np.asarray(special, np.float32)
    inp["knn_idx"] = cm.exact_knn(inp["xyz"], 4).astype(np.int32)
    inp["knn_idx"][1:, 3] = 0
    inp["sample_idx"][::3] = 0
    return inp


@pytest.mark.parametrize("special", [(1e-9, np.nextafter(B8, np.float32(0)), B8), (np.nextafter(B8, np.float32(1)), 3e-9, 0.05), (0.04, B8, 1e-9)],
                         ids=["1e-9, below, at", "above, 3e-9, 0.05", "0.04, at, 1e-9"])
def test_scale_clamp_at_1e_8(special):
    inp = _clamp_case(special)
    got, f64 = check(inp, True, f"scales {special}")
    s0 = inp["scales"][0]
    # below the bound the inverse scale is constant: the axis receives its gradient only through the sample point and the minimum
    below = s0 < B8
    assert below.any() and np.isfinite(got["d_scales"]).all()
    assert np.any(f64["d_scales"][0] != 0)


def test_equal_smallest_scales_take_the_lowest_axis():
    inp = cm.random_case(30, 6, 200, 21)
    s = inp["scales"]
    s[:10, 1] = s[:10, 0] = np.minimum(s[:10, 0], s[:10, 2]) * np.float32(0.5)         # axes 0 and 1 tie below axis 2
    s[10:20, 2] = s[10:20, 1] = np.minimum(s[10:20, 0], s[10:20, 1]) * np.float32(0.5)  # axes 1 and 2 tie below axis 0
    s[20:] = s[20:, :1]                                                                  # all three equal
    got, f64 = check(inp, True, "tied scales")
    # the minimum's gradient goes to the lowest axis only: with three equal scales and beta the only asymmetric path it differs
    assert np.any(f64["d_scales"][20:, 0] != f64["d_scales"][20:, 1])


def test_tiny_smallest_scale_in_the_normal_weights():
    inp = cm.random_case(30, 6, 200, 22)
    inp["scales"][::3, 1] = np.float32(5e-7)
    inp["scales"][1::3, 2] = np.nextafter(np.float32(1e-6), np.float32(0))
    check(inp, True, "m < 1e-6")


def test_all_neighbours_far():
    """Rows that do not list their own Gaussian: sum_k v_k falls below 1e-6 for some samples (and to exactly 0 for others), and
    the squared warped distance passes 1e8 for the thinnest neighbours."""
    inp = cm.random_case(60, 3, 400, 23, knn="random")
    t = inp["knn_idx"]
    own = t == np.arange(60)[:, None]
    t[own] = (t[own] + 1) % 60
    inp["scales"][:30] *= np.float32(0.3)
    inp["scales"][:6] = np.float32(1e-5)
    got, f64 = check(inp, True, "far neighbours")
    V, uu = f64["_V"], f64["_uu"]
    assert (V < 1e-6).sum() > 10 and ((V > 0) & (V < 1e-6)).sum() > 0 and (V > 1e-6).sum() > 10
    assert (uu > 1e8).sum() > 10 and np.isfinite(got["normal_term"]).all()


def test_orthogonal_neighbour_normal_is_dropped():
    """Unit quaternions (1,0,0,0): n is an exact axis, so n_j . n_g is exactly 0 between Gaussians whose thin axes differ."""
    inp = cm.random_case(24, 5, 200, 24)
    inp["quats"][:] = np.array([1, 0, 0, 0], np.float32)
    for axis in range(3):
        rows = slice(axis, 24, 3)
        inp["scales"][rows, axis] = inp["scales"][rows].min(1) * np.float32(0.5)
    got, f64 = check(inp, True, "orthogonal normals")
    assert np.any(f64["d_quats"] != 0)


def test_density_equal_to_target_gives_zero_gradient():
    """K = 1 (self), eps = 0, opac = 1: density = exp(0) = 1 = target exactly, |.| has derivative 0 there."""
    inp = _self_only(9, 40, 25)
    inp["eps"][:] = 0.0
    inp["opac"][:] = 1.0
    got = device_run(inp, False, (1.0, 0.0))
    assert np.array_equal(got["density"], np.ones(40, np.float32)) and not np.any(got["density_term"]) and float(got["loss_d"]) == 0.0
    for k in cm.GRADS:
        assert not np.any(got[k]), k
    check(inp, True, "density == target")


def test_opacity_that_does_not_require_grad():
    inp = cm.random_case(30, 6, 200, 26)
    got, _ = check(inp, True, "opac without grad", grad=(True, True, True, False))
    assert got["d_opac"] is None and got["d_xyz"] is not None
    got, _ = check(inp, False, "only scales with grad", upstream=(1.0, 0.0), grad=(False, True, False, False))
    assert got["d_xyz"] is None and got["d_quats"] is None and got["d_scales"] is not None


def test_contents_of_the_index_arrays_are_checked_on_the_device():
    inp = cm.random_case(10, 3, 20, 27)
    for key, value in (("knn_idx", 10), ("knn_idx", -1), ("sample_idx", 10), ("sample_idx", -2)):
        bad = {k: v.copy() for k, v in inp.items()}
        bad[key].reshape(-1)[3] = value
        with pytest.raises(ValueError, match=key):
            device_run(bad, False, (1.0, 0.0))
    with pytest.raises(ValueError, match="on cpu"):
        a = [torch.from_numpy(inp[k]).to(DEV) for k in cm.INPUTS]
        a[6] = a[6].cpu()
        sr.sugar_density_reg(*a)


# ------------------------------------------------------------------------------------------------ end to end
def _model(n, seed, **cfg):
    rng = np.random.default_rng(seed)
    pts = rng.standard_normal((n, 3))
    pts = 0.5 * pts / np.linalg.norm(pts, axis=1, keepdims=True) * np.cbrt(rng.random((n, 1)))
    m = gm.GaussianModel(dict({"init_num_pts": 0, "sh_degree": 0, "opacity_init": 0.5, "split_thresh": 0.1}, **cfg))
    m.create_from_pcd(gm.BasicPointCloud(points=pts, colors=rng.random((n, 3)), normals=np.zeros((n, 3))), 10)
    m.training_setup()
    with torch.no_grad():
        m._scaling += torch.from_numpy(rng.uniform(-1.5, 0.5, (n, 3)).astype(np.float32)).to(DEV)
        m._rotation += torch.from_numpy(rng.standard_normal((n, 4)).astype(np.float32)).to(DEV)
        m._opacity += torch.from_numpy(rng.standard_normal((n, 1)).astype(np.float32)).to(DEV)
    for g in m.optimizer.param_groups:
        g["lr"] = 1e-3
    return m


def _model_inputs(m, reg, sample_idx, eps):
    f = lambda t: t.detach().cpu().numpy()
    return {"xyz": f(m.get_xyz), "scales": f(m.get_scaling), "quats": f(m.get_rotation), "opac": f(m.get_opacity)[:, 0],
            "knn_idx": f(reg.knn_idx).astype(np.int32), "sample_idx": f(sample_idx).astype(np.int32), "eps": f(eps)}


@pytest.mark.parametrize("sphere", [False, True], ids=["anisotropic", "sphere"])
def test_end_to_end(sphere):
    m = _model(300, 30, sphere=sphere)
    reg = sr.SuGaRRegularizer(m, keep_track_of_knn=True, knn_to_track=16)
    reg.reset_neighbors()
    assert reg.knn_idx.shape == (300, 16) and reg.knn_dists.shape == (300, 16) and bool((reg.knn_idx[:, 0] == torch.arange(300, device=DEV)).all())
    args = types.SimpleNamespace(n_samples_for_sdf_regularization=2000, use_sdf_better_normal_loss=True)
    gen = torch.Generator(device=DEV).manual_seed(3)
    # the first step's loss against the restatement, on the samples the generator yields
    state = gen.get_state()
    weights = reg.sampling_weights(probabilities_proportional_to_volume=False)
    idx = torch.multinomial(weights, num_samples=2000, replacement=True, generator=gen)
    eps = torch.randn(2000, 3, device=DEV, generator=gen)
    gen.set_state(state)
    inp = _model_inputs(m, reg, idx, eps)
    f64, ref32 = cm.restate(inp, True, bounds=cm.F32_BOUNDS), cm.torch_expressions(inp, True, dtype=torch.float32)

    def step():
        m.optimizer.zero_grad(set_to_none=True)
        loss = reg.coarse_density_regulation(args, generator=gen)
        total = loss["density_regulation"] + loss["normal_regulation"]
        total.backward()
        for name in ("_xyz", "_scaling", "_rotation", "_opacity"):
            grad = getattr(m, name).grad
            assert grad is not None and bool(torch.isfinite(grad).all()) and bool((grad != 0).any()), name
        m.optimizer.step()
        assert bool(torch.isfinite(total))
        return loss

    first = step()
    within(first["density_regulation"].item(), f64["loss_d"], cm.unit_of(ref32, f64, "loss_d"), "end to end loss_d")
    within(first["normal_regulation"].item(), f64["loss_n"], cm.unit_of(ref32, f64, "loss_n"), "end to end loss_n")
    if sphere:
        g = m._scaling.grad
        assert bool((g[:, 0] == g[:, 1]).all()) and bool((g[:, 1] == g[:, 2]).all())      # through mean and repeat
        assert bool((reg.get_smallest_axis(return_idx=True)[1] == 0).all())
    step()
    # densify, then new neighbours
    m.xyz_gradient_accum = torch.full((300, 1), 1.0, device=DEV)
    m.denom = torch.ones(300, 1, device=DEV)
    counts = m.densify(0.5, generator=gen)
    n = m._xyz.shape[0]
    assert n == counts["M"] > 300
    with pytest.raises(RuntimeError, match="reset_neighbors"):
        reg.coarse_density_regulation(args, generator=gen)
    reg.reset_neighbors()
    assert reg.knn_idx.shape == (n, 16)
    plain = reg.coarse_density_regulation(types.SimpleNamespace(n_samples_for_sdf_regularization=500, use_sdf_better_normal_loss=False), generator=gen)
    assert plain["normal_regulation"] == 0 and bool(torch.isfinite(plain["density_regulation"]))
    step()
    assert m._xyz.shape[0] == n
