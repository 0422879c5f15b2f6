"""SuGaR density and normal regularisation without a device: the float64 restatement reproduces what the reference computed for
the golden case, the library exports what include/dm4d_sugar_reg.h declares, the host-side argument checks refuse before any
launch, the API refuses CPU tensors and the modes it does not offer, the sampler keeps the reference's cumulative weights."""
import types

import numpy as np
import pytest
import torch

from dreammesh4d_amd import _lib, sugar_reg as sr
from tests import sugar_reg_common as cm


@pytest.fixture(scope="module")
def z():
    return cm.golden()


@pytest.mark.parametrize("tag", sorted(cm.UPSTREAMS))
def test_restatement_reproduces_the_golden_case(z, tag):
    """Forward and closed-form gradients against the reference's float64 run and its autograd: 1e-12 of the tensor's largest value."""
    got = cm.restate(cm.golden_inputs(z), True, cm.UPSTREAMS[tag], float(z["sampling_scale"]), float(z["density_factor"]))
    for k in cm.PER_SAMPLE + ("loss_d", "loss_n"):
        assert np.abs(got[k] - z[k]).max() <= 1e-12 * np.abs(z[k]).max(), k
    for k in cm.GRADS:
        want = z[f"{tag}/{k}"].reshape(got[k].shape)
        assert np.abs(got[k] - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300), f"{tag}/{k}"


def test_golden_case_is_the_one_the_issue_sets(z):
    inp = cm.golden_inputs(z)
    assert inp["knn_idx"].shape == (400, 16) and inp["sample_idx"].shape == (3000,) and inp["eps"].shape == (3000, 3)
    assert np.array_equal(inp["knn_idx"], cm.exact_knn(inp["xyz"], 16))
    s = inp["scales"]
    assert s.max() / s.min() > 50 and 0.05 < inp["opac"].min() and inp["opac"].max() < 0.99
    assert np.abs((inp["quats"].astype(np.float64) ** 2).sum(1) - 1).max() > 0          # normalised in float32: not exactly unit
    for k in cm.PER_SAMPLE + ("loss_d", "loss_n") + tuple(f"{t}/{g}" for t in cm.UPSTREAMS for g in cm.GRADS):
        assert float(z[k + "_err_ref"]) >= 0 and z[k].dtype == np.float64


def test_torch_expressions_agree_with_the_restatement():
    inp = cm.random_case(40, 5, 90, 3)
    a, b = cm.restate(inp, True), cm.torch_expressions(inp, True, dtype=torch.float64)
    for k in b:
        assert np.abs(a[k] - b[k]).max() <= 1e-12 * max(np.abs(a[k]).max(), 1e-300), k


def test_library_exports_the_header():
    L = _lib.lib()
    names = _lib.declared_symbols("sr")
    assert names == ["dm4d_sr_backward", "dm4d_sr_forward", "dm4d_sr_scratch_bytes", "dm4d_sr_version"]
    assert [n for n in names if not hasattr(L, n)] == []
    assert L.dm4d_sr_version() == _lib.abi_version("sr") == 1
    assert _lib.abi_version() == 107 and _lib.abi_version("dc") == 1 and _lib.abi_version("iso") >= 1     # the others keep their numbers
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(ln.split()[-1] for ln in out.splitlines() if " T dm4d_sr_" in ln) == names


P = 0x1000                                               # a non-null, 16-byte aligned pointer no refused call ever follows
BIG = 1 << 40


def _fwd(N=4, K=2, S=8, ss=1.5, df=1.0, normal=0, scratch=P, nbytes=BIG, null=None, nterm=P):
    a = [N, K, S, P, P, P, P, P, P, P, P, ss, df, normal, scratch, nbytes, P, P, P, nterm, P, None]
    if null is not None:
        a[null] = None
    return ("dm4d_sr_forward", tuple(a))


def _bwd(N=4, K=2, S=8, ss=1.5, df=1.0, normal=0, scratch=P, nbytes=BIG, null=None):
    a = [N, K, S, P, P, P, P, P, P, P, P, ss, df, normal, P, P, P, P, P, scratch, nbytes, P, P, P, P, None]
    if null is not None:
        a[null] = None
    return ("dm4d_sr_backward", tuple(a))


REFUSED = {
    "scratch N < 0": ("dm4d_sr_scratch_bytes", (-1, 16, 8)),
    "scratch N too large": ("dm4d_sr_scratch_bytes", (_lib.DM4D_SR_MAX_POINTS + 1, 16, 8)),
    "scratch K = 0": ("dm4d_sr_scratch_bytes", (4, 0, 8)),
    "scratch K = 33": ("dm4d_sr_scratch_bytes", (4, 33, 8)),
    "scratch S < 0": ("dm4d_sr_scratch_bytes", (4, 16, -1)),
    "scratch S too large": ("dm4d_sr_scratch_bytes", (4, 16, _lib.DM4D_SR_MAX_SAMPLES + 1)),
    "forward N < 0": _fwd(N=-1),
    "forward K = 0": _fwd(K=0),
    "forward K = 33": _fwd(K=33),
    "forward S too large": _fwd(S=_lib.DM4D_SR_MAX_SAMPLES + 1),
    "forward sampling_scale nan": _fwd(ss=float("nan")),
    "forward density_factor inf": _fwd(df=float("inf")),
    "forward flag 2": _fwd(normal=2),
    "forward null xyz": _fwd(null=3),
    "forward null knn_idx": _fwd(null=7),
    "forward null order": _fwd(null=9),
    "forward null losses": _fwd(null=20),
    "forward null normal_term with the normal loss": _fwd(normal=1, nterm=None),
    "forward null scratch": _fwd(scratch=None),
    "forward misaligned scratch": _fwd(scratch=P + 4),
    "backward N too large": _bwd(N=_lib.DM4D_SR_MAX_POINTS + 1),
    "backward K = 0": _bwd(K=0),
    "backward S < 0": _bwd(S=-3),
    "backward sampling_scale inf": _bwd(ss=float("inf")),
    "backward flag -1": _bwd(normal=-1),
    "backward null upstream": _bwd(null=14),
    "backward null seg_ptr": _bwd(null=15),
    "backward null chunk_ptr": _bwd(null=16),
    "backward null rev_ptr": _bwd(null=17),
    "backward null rev_pos": _bwd(null=18),
    "backward null scratch": _bwd(scratch=None),
    "backward misaligned scratch": _bwd(scratch=P + 8),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_host_validation_refuses_without_a_device(name):
    fn, args = REFUSED[name]
    rc = getattr(_lib.lib(), fn)(*args)
    assert rc == _lib.DM4D_ERR_INVALID, f"{fn}{args} returned {rc}"
    assert fn.encode() in _lib.lib().dm4d_last_error()


def test_scratch_size_and_nothing_to_do():
    L = _lib.lib()
    need = L.dm4d_sr_scratch_bytes(400, 16, 3000)
    chunks = (3000 + 15) // 16 + 400
    assert need >= 400 * 18 * 4 + chunks * (16 * 17 + 13) * 4 and need % 256 == 0
    assert L.dm4d_sr_scratch_bytes(100000, 16, 500000) < 160 << 20
    fn, args = _fwd(N=400, K=16, S=3000, nbytes=need - 1)
    assert getattr(L, fn)(*args) == _lib.DM4D_ERR_CAPACITY
    fn, args = _bwd(N=400, K=16, S=3000, nbytes=need - 1)
    assert getattr(L, fn)(*args) == _lib.DM4D_ERR_CAPACITY
    # N == 0 or S == 0 is a success that launches nothing
    none = (None,) * 8
    assert L.dm4d_sr_forward(0, 16, 8, *none, 1.5, 1.0, 0, None, 0, None, None, None, None, None, None) == 0
    assert L.dm4d_sr_forward(4, 16, 0, *none, 1.5, 1.0, 1, None, 0, None, None, None, None, None, None) == 0
    assert L.dm4d_sr_backward(4, 16, 0, *none, 1.5, 1.0, 1, None, None, None, None, None, None, 0, None, None, None, None, None) == 0


def _cpu_case(n=6, k=3, s=10):
    inp = cm.random_case(n, k, s, 0)
    return [torch.from_numpy(inp[name]) for name in cm.INPUTS]


def test_api_refuses_cpu_tensors():
    with pytest.raises(_lib.Dm4dError, match="no CPU fallback"):
        sr.sugar_density_reg(*_cpu_case())
    with pytest.raises(_lib.Dm4dError, match="no CPU fallback"):
        sr.sugar_density_reg(*_cpu_case(), with_normal_loss=True)


def test_api_refuses_bad_arguments_before_the_library():
    def bad(i, t, **kw):
        a = _cpu_case()
        a[i] = t(a[i])
        with pytest.raises(ValueError):
            sr.sugar_density_reg(*a, **kw)

    bad(0, lambda t: t[:, :2])
    bad(0, lambda t: t.double())
    bad(1, lambda t: t[:-1])
    bad(2, lambda t: t[:, :3])
    bad(3, lambda t: t[:, None, None])
    bad(3, lambda t: t.half())
    bad(4, lambda t: t[:, :0])
    bad(4, lambda t: t.float())
    bad(4, lambda t: torch.zeros(6, 33, dtype=torch.int32))
    bad(5, lambda t: t[:, None])
    bad(5, lambda t: t.float())
    bad(5, lambda t: t[:0])
    bad(6, lambda t: t[:-1])
    bad(6, lambda t: t.double())
    bad(0, lambda t: t.numpy())
    with pytest.raises(ValueError, match="not finite"):
        sr.sugar_density_reg(*_cpu_case(), sampling_scale=float("nan"))


class _Model:
    """What SuGaRRegularizer reads of a GaussianModel."""

    def __init__(self, n=5, seed=0):
        inp = cm.random_case(n, 2, 4, seed)
        self.get_xyz, self.get_scaling = torch.from_numpy(inp["xyz"]), torch.from_numpy(inp["scales"])
        self.get_rotation, self.get_opacity = torch.from_numpy(inp["quats"]), torch.from_numpy(inp["opac"])[:, None]


def test_the_four_refusals_by_name():
    with pytest.raises(NotImplementedError, match="learnable"):
        sr.SuGaRRegularizer(_Model(), beta_mode="learnable")
    with pytest.raises(NotImplementedError, match="weighted_average"):
        sr.SuGaRRegularizer(_Model(), beta_mode="weighted_average")
    with pytest.raises(NotImplementedError, match="surface_mesh_to_bind"):
        sr.SuGaRRegularizer(_Model(), surface_mesh_to_bind=object())
    with pytest.raises(NotImplementedError, match="estimate_from_points"):
        sr.SuGaRRegularizer(_Model()).get_normals(estimate_from_points=True)
    with pytest.raises(ValueError):
        sr.SuGaRRegularizer(_Model(), beta_mode="median")
    reg = sr.SuGaRRegularizer(_Model(), keep_track_of_knn=True, knn_to_track=8)
    assert reg.knn_to_track == 8 and reg.keep_track_of_knn and reg.beta_mode == "average" and reg.n_points == 5
    with pytest.raises(RuntimeError, match="reset_neighbors"):
        reg.coarse_density_regulation(types.SimpleNamespace(n_samples_for_sdf_regularization=4, use_sdf_better_normal_loss=False))


def test_sampler_keeps_the_cumulative_quirk():
    """5 Gaussians: the weights handed to multinomial are cumsum(areas) / sum(areas), as sugar_utils.py:214-218 is written."""
    m = _Model(5)
    reg = sr.SuGaRRegularizer(m)
    s, o = m.get_scaling.double(), m.get_opacity.double().view(-1)
    vol = (s[:, 0] * s[:, 1] * s[:, 2]).abs()
    for by_opacity, by_volume, areas in ((False, True, vol), (False, False, torch.ones(5, dtype=torch.float64)), (True, True, vol * o)):
        got = reg.sampling_weights(None, by_opacity, by_volume).double()
        want = areas.cumsum(0) / areas.sum()
        assert torch.allclose(got, want, rtol=1e-6, atol=0), (by_opacity, by_volume)
        assert abs(float(got[-1]) - 1) < 1e-6 and bool((got[1:] >= got[:-1]).all())
    assert torch.equal(reg.sampling_weights(probabilities_proportional_to_volume=False), torch.arange(1, 6).float() / 5)
    mask = torch.tensor([True, False, True, True, False])
    assert reg.sampling_weights(mask, False, False).tolist() == pytest.approx([1 / 3, 2 / 3, 1.0])
    g = torch.Generator().manual_seed(1)
    pts, idx = reg.sample_points_in_gaussians(64, 1.5, mask, False, False, generator=g)
    assert pts.shape == (64, 3) and set(idx.tolist()) <= {0, 2, 3}
    pts2, idx2 = reg.sample_points_in_gaussians(64, 1.5, mask, False, False, generator=torch.Generator().manual_seed(1))
    assert torch.equal(pts, pts2) and torch.equal(idx, idx2)


def test_smallest_axis_takes_the_lowest_index_on_ties():
    m = _Model(4)
    m.get_scaling = torch.tensor([[0.2, 0.1, 0.1], [0.1, 0.1, 0.1], [0.3, 0.2, 0.1], [0.1, 0.2, 0.1]])
    reg = sr.SuGaRRegularizer(m)
    axis, idx = reg.get_smallest_axis(return_idx=True)
    assert idx.tolist() == [1, 0, 2, 0]
    R = cm.quaternion_to_matrix(m.get_rotation)
    assert torch.equal(axis, torch.stack([R[i, :, c] for i, c in enumerate(idx.tolist())]))
    assert torch.equal(reg.get_normals(), axis)
    assert idx.tolist() == cm.lowest_argmin(m.get_scaling).tolist()
