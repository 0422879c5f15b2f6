"""CPU-side checks of the spherical-harmonics colour (degree 1-3): the fixture against a restatement of the basis, the comparison
helpers the GPU tests use, the host-side validation of the new degrees, the geometry's sh_levels plumbing and the ABI."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import sh_eval_common as shc


def test_fixture_matches_the_basis_formulae():
    """tests/golden/eval_sh.npz (the reference's eval_sh in float64) is reproduced to 1e-12 by the basis written out from the
    formulae in tests/sh_eval_common.py: pins the constants and signs the kernel must use.  Both branches of the clamp are covered."""
    fx = shc.load()
    assert fx["points"].dtype == np.float32 and fx["sh"].dtype == np.float32 and fx["sh"].shape[1:] == (16, 3)
    for deg in range(4):
        for c in range(2):
            v = shc.eval_v(fx["points"], fx["sh"], fx["campos"][c], deg)
            assert np.abs(v - fx[f"v_d{deg}_c{c}"]).max() <= 1e-12, (deg, c)
            B = shc.sh_basis(shc.directions(fx["points"], fx["campos"][c]), deg)
            A = 0.5 + (np.abs(B)[:, :, None] * np.abs(fx["sh"].astype(np.float64)[:, :(deg + 1) ** 2])).sum(axis=1)
            assert np.abs(A - fx[f"A_d{deg}_c{c}"]).max() <= 1e-6 * A.max()          # stored as float32
            # autograd's coefficient gradient is B_k * grad where not clamped
            NG = fx[f"dsh_d{deg}_c{c}"].shape[0]
            want = B[:NG, :, None] * (fx["grad"][:NG].astype(np.float64) * (v[:NG] >= 0))[:, None, :]
            assert np.abs(want - fx[f"dsh_d{deg}_c{c}"]).max() <= 1e-6 * np.abs(want).max()
            frac = float((v < 0).mean())
            assert 0.01 < frac < 0.5, (deg, c, frac)


def test_comparison_helpers_catch_a_planted_error():
    """The forward comparison fails on an error of 4x the bar planted in ONE element and passes at 0.5x; the gradient comparison
    likewise; a flipped clamp flag away from the clamp is counted."""
    fx = shc.load()
    v, A = fx["v_d3_c0"], fx["A_d3_c0"]
    rgb = np.maximum(v, 0.0)
    flags = v < 0
    i = np.unravel_index(np.argmax(v), v.shape)                # an unclamped element
    bar = shc.K_FORWARD * shc.U * float(A[i])
    for scale, ok in ((0.5, True), (4.0, False)):
        bad = rgb.copy()
        bad[i] += scale * bar
        ratio, wrong, near = shc.forward_excess(bad, flags, v, A)
        assert (ratio <= 1.0) == ok and abs(ratio - scale) < 1e-3 and wrong == 0 and near < 0.01
        if ok:
            shc.assert_forward(bad, flags, v, A)
        else:
            with pytest.raises(AssertionError):
                shc.assert_forward(bad, flags, v, A)
    f2 = flags.copy()
    f2[i] = True
    assert shc.forward_excess(rgb, f2, v, A)[1] == 1
    g = fx["dpoints_d3_c0"]
    j = np.unravel_index(np.argmax(np.abs(g)), g.shape)
    gbar = shc.GRAD_RTOL * abs(g[j]) + shc.GRAD_ATOL * np.abs(g).max()
    for scale, ok in ((0.5, True), (4.0, False)):
        bad = g.copy()
        bad[j] += scale * gbar
        assert (shc.grad_excess(bad, g) <= 1.0) == ok
    z = np.zeros((4, 3))
    assert shc.grad_excess(z, z) == 0.0 and shc.grad_excess(z + 1e-30, z) == np.inf       # a zero reference wants an exact zero


def test_sh_degree_validation_is_host_side():
    """Degrees 0 to 3 with enough coefficients pass the rasterizer's and the new entry points' validation (the call then stops at
    the next host-side check, the workspace size: nothing is launched); degree 4, a negative degree and too few coefficients are
    refused with both numbers in the message; shs with 6 channels stay refused."""
    from dreammesh4d_amd import _lib

    L = _lib.lib()
    dummy = (C.c_float * 64)()
    p = C.cast(dummy, C.c_void_p)

    def prepare(degree, M, channels=3):
        s = _lib.RasterSettings(64, 64, 0.2, 0.2, 1.0, degree, 0, 0, p, p, p, p)
        i = _lib.RasterInputs(4, M, channels, p, p, None, p, p, p, None)
        return L.dm4d_rasterize_prepare(C.byref(s), C.byref(i), p, p, 64, None), L.dm4d_last_error()

    for degree, M in ((3, 16), (3, 20), (2, 9), (1, 4), (1, 16), (0, 1), (0, 16)):
        rc, msg = prepare(degree, M)
        assert rc == -3 and b"geom workspace too small" in msg, (degree, M, rc, msg)      # DM4D_ERR_CAPACITY: validation passed
    rc, msg = prepare(4, 25)
    assert rc == -4 and b"sh_degree 4" in msg and b"25 coefficients" in msg, (rc, msg)    # DM4D_ERR_UNSUPPORTED
    rc, msg = prepare(-1, 16)
    assert rc == -4 and b"sh_degree -1" in msg and b"16 coefficients" in msg, (rc, msg)
    rc, msg = prepare(1, 3)
    assert rc == -1 and b"sh_degree 1 needs 4 coefficients" in msg and b"has 3" in msg, (rc, msg)
    rc, msg = prepare(3, 15)
    assert rc == -1 and b"needs 16" in msg and b"has 15" in msg, (rc, msg)
    rc, msg = prepare(2, 9, channels=6)
    assert rc == -1 and b"6 channels" in msg and b"sh_degree 2" in msg and b"9 coefficients" in msg, (rc, msg)
    # degree > 0 reads the camera centre
    s = _lib.RasterSettings(64, 64, 0.2, 0.2, 1.0, 2, 0, 0, p, p, p, None)
    i = _lib.RasterInputs(4, 9, 3, p, p, None, p, p, p, None)
    assert L.dm4d_rasterize_prepare(C.byref(s), C.byref(i), p, p, 64, None) == -1 and b"campos" in L.dm4d_last_error()
    # the entry points of their own: same rules, and N = 0 is a no-op that launches nothing
    assert L.dm4d_sh_eval_forward(4, 4, 25, p, p, p, p, p, None) == -4 and b"sh_degree 4" in L.dm4d_last_error()
    assert L.dm4d_sh_eval_forward(4, 2, 8, p, p, p, p, p, None) == -1 and b"needs 9 coefficients" in L.dm4d_last_error()
    assert L.dm4d_sh_eval_forward(4, 3, 16, p, p, None, p, p, None) == -1 and b"null" in L.dm4d_last_error()
    assert L.dm4d_sh_eval_backward(4, -1, 16, p, p, p, p, p, p, p, None) == -4
    assert L.dm4d_sh_eval_backward(4, 3, 16, p, p, p, p, p, None, p, None) == -1
    assert L.dm4d_sh_eval_forward(0, 3, 16, None, None, None, None, None, None) == 0
    assert L.dm4d_sh_eval_backward(0, 3, 16, None, None, None, None, None, None, None, None) == 0


def test_abi_version_and_symbols():
    from dreammesh4d_amd import _lib

    L = _lib.lib()
    assert L.dm4d_version() == 107 and _lib.abi_version() == 107
    for name in ("dm4d_sh_eval_forward", "dm4d_sh_eval_backward"):
        assert name in _lib.declared_symbols() and name in _lib._SIGNATURES and hasattr(L, name)


def _mesh():
    from dreammesh4d_amd import synthetic as syn

    return syn.uv_sphere(48)


class _Mesh:
    def __init__(self, verts, faces):
        self.vertices, self.triangles, self.vertex_colors = verts, faces, np.zeros((0, 3))


def test_sugar_model_sh_levels(tmp_path):
    """`sh_levels` of the geometry config sizes `_sh_coordinates_rest` as the reference does (sugar.py:231), get_points_rgb follows
    sugar.py:640-661 (ValueError without camera centres above level 1), and a checkpoint round trip keeps the wider tensor."""
    from dreammesh4d_amd import threestudio_host as host
    from dreammesh4d_amd import wire_formats as wf

    verts, faces = _mesh()
    mesh = _Mesh(np.asarray(verts, np.float64), np.asarray(faces, np.int64))
    g1 = host.SuGaRModel({"n_gaussians_per_surface_triangle": 1}, o3d_mesh=mesh)
    N = g1.n_gaussians
    assert tuple(g1._sh_coordinates_rest.shape) == (N, 0, 3) and g1.sh_levels == 1 and g1.active_sh_degree == 0
    assert tuple(g1.get_points_rgb().shape) == (N, 3)
    assert torch.equal(g1.get_points_rgb(torch.zeros(1, 3)), g1.get_points_rgb())            # level 1 ignores the argument
    g3 = host.SuGaRModel({"n_gaussians_per_surface_triangle": 1, "sh_levels": 3}, o3d_mesh=mesh)
    assert tuple(g3._sh_coordinates_rest.shape) == (N, 8, 3) and g3.sh_levels == 3 and g3.active_sh_degree == 2
    assert float(g3._sh_coordinates_rest.detach().abs().max()) == 0.0 and g3._sh_coordinates_rest.requires_grad
    assert tuple(g3.get_features.shape) == (N, 9, 3)
    assert "f_rest" in g3.optimize_params
    with pytest.raises(ValueError, match="camera_centers must be provided."):
        g3.get_points_rgb()
    with pytest.raises(ValueError, match="sh_levels"):
        host.SuGaRModel({"n_gaussians_per_surface_triangle": 1, "sh_levels": 5}, o3d_mesh=mesh)
    # checkpoint round trip under the reference's key names
    with torch.no_grad():
        g3._sh_coordinates_rest.copy_(torch.randn(N, 8, 3, generator=torch.Generator().manual_seed(3)))
    path = str(tmp_path / "ckpt.pt")
    wf.save_checkpoint(path, {"geometry": g3}, epoch=1, global_step=7)
    sd, _, step = wf.load_module_weights(path, module_name="geometry")
    assert step == 7 and tuple(sd["_sh_coordinates_rest"].shape) == (N, 8, 3) and "_sh_coordinates_dc" in sd
    h3 = host.SuGaRModel({"n_gaussians_per_surface_triangle": 1, "sh_levels": 3}, o3d_mesh=mesh)
    missing, unexpected, _, _ = wf.load_geometry(h3, path)
    assert not missing and not unexpected
    assert torch.equal(h3._sh_coordinates_rest.detach().cpu(), g3._sh_coordinates_rest.detach().cpu())
    with pytest.raises(RuntimeError, match="_sh_coordinates_rest"):                          # a level-1 model cannot take it
        wf.load_geometry(g1, path)


def test_batched_paths_refuse_sh_levels_by_name():
    from dreammesh4d_amd import geometry as geo
    from dreammesh4d_amd import sugar

    verts, faces = _mesh()
    g = sugar.SuGaR(verts, faces, n_gaussians_per_surface_triangle=1, sh_levels=2, device="cpu")
    with pytest.raises(NotImplementedError, match="sh_levels = 2"):
        geo.require_sh_levels_1(g, "somewhere")
    with pytest.raises(NotImplementedError, match="sh_levels"):
        geo.reject_sh_coefficients(torch.zeros(5, 4, 3), "somewhere")
    geo.reject_sh_coefficients(torch.zeros(5, 6), "somewhere")
    geo.require_sh_levels_1(sugar.SuGaR(verts, faces, n_gaussians_per_surface_triangle=1, device="cpu"), "somewhere")
    with pytest.raises(ValueError, match="camera_centers must be provided."):
        geo.points_rgb_sh(torch.zeros(5, 4, 3), torch.zeros(5, 3), None, 2)
    assert torch.equal(geo.points_rgb_sh(torch.ones(5, 4, 3), torch.zeros(5, 3), None, 1), geo.points_rgb(torch.ones(5, 1, 3)))
