"""GPU tests of the spherical-harmonics colour of degree 1-3: the HIP kernels against the reference's float64 eval_sh
(tests/golden/eval_sh.npz), the rasterizer's sh_degree > 0 against its own colors_precomp path (which the oracle tests pin),
degree 0 untouched, and the Python layer (points_rgb_sh, the single-view renderer, the batched paths' refusal)."""
import math

import numpy as np
import pytest
import torch

from dreammesh4d_amd import synthetic as syn
from tests import sh_eval_common as shc

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _dev():
    return torch.device("cuda:0")


def _t(a, dtype=np.float32):
    return torch.tensor(np.ascontiguousarray(np.asarray(a, dtype)), device=_dev())


def _sh_forward(points, campos, sh, degree):
    """dm4d_sh_eval_forward -> (rgb, clamped) as device tensors."""
    from dreammesh4d_amd import _lib

    N, M = int(sh.shape[0]), int(sh.shape[1])
    rgb = torch.full((N, 3), float("nan"), device=_dev())
    cl = torch.full((N, 3), 7, dtype=torch.uint8, device=_dev())
    _lib.call("dm4d_sh_eval_forward", N, degree, M, points.data_ptr(), campos.data_ptr(), sh.data_ptr(), rgb.data_ptr(), cl.data_ptr(),
              torch.cuda.current_stream(_dev()).cuda_stream)
    torch.cuda.synchronize()
    return rgb, cl


def _sh_backward(points, campos, sh, degree, clamped, g):
    from dreammesh4d_amd import _lib

    N, M = int(sh.shape[0]), int(sh.shape[1])
    dsh = torch.full((N, M, 3), float("nan"), device=_dev())
    dp = torch.full((N, 3), float("nan"), device=_dev())
    _lib.call("dm4d_sh_eval_backward", N, degree, M, points.data_ptr(), campos.data_ptr(), sh.data_ptr(), clamped.data_ptr(), g.data_ptr(),
              dsh.data_ptr(), dp.data_ptr(), torch.cuda.current_stream(_dev()).cuda_stream)
    torch.cuda.synchronize()
    return dsh, dp


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_kernel_forward_against_reference(degree):
    """dm4d_sh_eval_forward on the fixture, both cameras, with M = 16 stored coefficients (rows of 192 bytes of which the first
    12 (degree + 1)^2 are read) and with M = (degree + 1)^2 (one contiguous block per wave): per element
    |hip - ref| <= K 2^-24 A, K = 41 from the rounding count written out in tests/sh_eval_common.py (direction 5.5, a cubic
    in it 16.5 + 7 of its own, product 1, 16 additions), A = 0.5 + sum_k |B_k| |sh_k| from the fixture; `clamped` equals
    ref < 0 wherever |v_ref| exceeds that bar, and at most 1 % of the elements may be nearer the clamp than that.  An odd N
    (partial last wave) gives the same rows.
    Observed on an MI355X: max |hip - ref| / bar = 0.047 / 0.054 / 0.074 / 0.095 at degree 0 / 1 / 2 / 3; the
    gradients of the next test reach at most 0.04 of their bar."""
    _need_gpu()
    fx = shc.load()
    K = (degree + 1) ** 2
    pts = _t(fx["points"])
    for c in range(2):
        cam = _t(fx["campos"][c])
        v_ref, A = fx[f"v_d{degree}_c{c}"], fx[f"A_d{degree}_c{c}"]
        outs = []
        for M in sorted({16, K}):
            rgb, cl = _sh_forward(pts, cam, _t(fx["sh"][:, :M]), degree)
            assert set(np.unique(cl.cpu().numpy())) <= {0, 1}
            shc.assert_forward(rgb.cpu().numpy(), cl.cpu().numpy(), v_ref, A, what=f"degree {degree} camera {c} M {M}")
            outs.append((rgb, cl))
        assert torch.equal(outs[0][0], outs[-1][0]) and torch.equal(outs[0][1], outs[-1][1])       # M does not change a bit
        n = 1024 - 77                                                                              # partial wave, unaligned tail
        rgb, cl = _sh_forward(pts[:n].contiguous(), cam, _t(fx["sh"][:n]), degree)
        assert torch.equal(rgb, outs[-1][0][:n]) and torch.equal(cl, outs[-1][1][:n])
        # a coefficient tensor that is only 4-byte aligned takes the dword path: same bits
        buf = torch.zeros(1024 * 16 * 3 + 1, device=_dev())
        buf[1:] = _t(fx["sh"]).reshape(-1)
        rgb, cl = _sh_forward(pts, cam, buf[1:].view(1024, 16, 3), degree)
        assert torch.equal(rgb, outs[-1][0]) and torch.equal(cl, outs[-1][1])


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_kernel_backward_against_reference(degree):
    """dm4d_sh_eval_backward against the fixture's autograd (first NG points), per element within the project's gradient bar
    GRAD_RTOL |ref| + GRAD_ATOL max|ref| (1e-4, 5e-6); elements whose forward value lies within the forward bar of the clamp are
    left out (their flag may legitimately differ).  Exact zeros for clamped channels and for the coefficients beyond the degree;
    two runs are bit-identical; M = 16 and M = (degree + 1)^2 agree bit for bit."""
    _need_gpu()
    fx = shc.load()
    K = (degree + 1) ** 2
    pts, g = _t(fx["points"]), _t(fx["grad"])
    for c in range(2):
        cam = _t(fx["campos"][c])
        v_ref, A = fx[f"v_d{degree}_c{c}"], fx[f"A_d{degree}_c{c}"]
        sh16 = _t(fx["sh"])
        rgb, cl = _sh_forward(pts, cam, sh16, degree)
        dsh, dp = _sh_backward(pts, cam, sh16, degree, cl, g)
        dsh2, dp2 = _sh_backward(pts, cam, sh16, degree, cl, g)
        assert torch.equal(dsh, dsh2) and torch.equal(dp, dp2)
        dsh_n, dp_n, cl_n = dsh.cpu().numpy(), dp.cpu().numpy(), cl.cpu().numpy().astype(bool)
        assert np.isfinite(dsh_n).all() and np.isfinite(dp_n).all()
        assert not dsh_n[:, K:].any()                                           # beyond the degree: exact zeros
        assert not dsh_n[:, :K][np.broadcast_to(cl_n[:, None, :], dsh_n[:, :K].shape)].any()       # clamped channels: exact zeros
        shK = _t(fx["sh"][:, :K])
        dshK, dpK = _sh_backward(pts, cam, shK, degree, cl, g)
        assert torch.equal(dshK, dsh[:, :K]) and torch.equal(dpK, dp)
        NG = fx[f"dsh_d{degree}_c{c}"].shape[0]
        far = (np.abs(v_ref) > shc.K_FORWARD * shc.U * A)[:NG]                  # [NG,3]
        assert far.mean() >= 0.99
        r_sh = shc.grad_excess(dsh_n[:NG, :K], fx[f"dsh_d{degree}_c{c}"], keep=np.broadcast_to(far[:, None, :], (NG, K, 3)))
        r_p = shc.grad_excess(dp_n[:NG], fx[f"dpoints_d{degree}_c{c}"], keep=np.broadcast_to(far.all(axis=1)[:, None], (NG, 3)))
        print(f"degree {degree} camera {c}: dL_dsh error / bar {r_sh:.4f}, dL_dmeans3D error / bar {r_p:.4f}")
        assert r_sh <= 1.0 and r_p <= 1.0, (r_sh, r_p)


def test_point_on_the_camera_centre_gives_zeros():
    """A mean equal to campos has no direction: the forward is the DC colour, dL_dmeans3D an exact zero row, everything finite."""
    _need_gpu()
    fx = shc.load()
    pts = fx["points"][:130].copy()
    pts[[0, 64, 129]] = fx["campos"][0]
    sh, g = fx["sh"][:130], fx["grad"][:130]
    for degree in (1, 2, 3):
        rgb, cl = _sh_forward(_t(pts), _t(fx["campos"][0]), _t(sh), degree)
        dsh, dp = _sh_backward(_t(pts), _t(fx["campos"][0]), _t(sh), degree, cl, _t(g))
        rgb, cl, dsh, dp = (a.cpu().numpy() for a in (rgb, cl, dsh, dp))
        assert np.isfinite(rgb).all() and np.isfinite(dsh).all() and np.isfinite(dp).all()
        for i in (0, 64, 129):
            dc = np.float32(0.28209479177387814) * sh[i, 0] + np.float32(0.5)
            assert np.array_equal(rgb[i], np.maximum(dc, 0)) and np.array_equal(cl[i] != 0, dc < 0)
            assert not dp[i].any() and not dsh[i, 1:].any()
            assert np.array_equal(dsh[i, 0], np.where(dc < 0, 0, np.float32(0.28209479177387814) * g[i]).astype(np.float32))


# ------------------------------------------------------------------------------------------------ rasterizer composition
def _raster(cam, sh_degree):
    """tests/hip_raster.HipRaster with the settings' sh_degree set (its forward writes 0)."""
    from dreammesh4d_amd import _lib
    from tests.hip_raster import HipRaster

    class ShRaster(HipRaster):
        def forward(self, *a, **kw):
            real = _lib.RasterSettings

            def settings(*args):
                args = list(args)
                args[5] = sh_degree
                return real(*args)

            _lib.RasterSettings = settings
            try:
                return super().forward(*a, **kw)
            finally:
                _lib.RasterSettings = real

    return ShRaster(cam)


def _scene(cam, n=6000, seed=5):
    sc = syn.random_splat_scene(n, seed=seed, log_scale_mean=math.log(0.02), log_scale_std=0.5)
    sc["means3D"][::97] += (1.5 * np.asarray(cam.campos, np.float32))[None]       # some Gaussians behind the camera: culled, radius 0
    sc["sh"] = (np.random.default_rng(seed + 1).standard_normal((n, 16, 3)) * 0.6).astype(np.float32)
    return sc


@pytest.mark.parametrize("degree", [1, 2, 3])
@pytest.mark.parametrize("full_rows", [True, False])
def test_rasterizer_sh_equals_precomputed_colour(degree, full_rows):
    """forward(shs, sh_degree = d) equals forward(colors_precomp = dm4d_sh_eval_forward(...)) bit for bit (image, depth, alpha,
    radii), and so do dL_dmeans2D / dL_dopacity / dL_dscales / dL_drots; dL_dsh and the extra dL_dmeans3D equal
    dm4d_sh_eval_backward of the precomp call's dL_dcolors within the gradient bar; culled Gaussians have all-zero rows.
    M = 16 (full_rows) or M = (d + 1)^2."""
    _need_gpu()
    H = W = 128
    cam = syn.make_camera(H, W, elev_deg=20.0, azim_deg=35.0)
    sc = _scene(cam)
    M = 16 if full_rows else (degree + 1) ** 2
    sh = np.ascontiguousarray(sc["sh"][:, :M])
    rng = np.random.default_rng(11)
    gC, gD, gA = (rng.standard_normal(s).astype(np.float32) for s in ((3, H, W), (H, W), (H, W)))
    a = _raster(cam, degree)
    ca, ra, da, aa = a.forward(sc["means3D"], sc["opacities"], shs=sh, scales=sc["scales"], rotations=sc["rotations"])
    ga = a.backward(gC, gD, gA)
    rgb, cl = _sh_forward(_t(sc["means3D"]), _t(cam.campos), _t(sh), degree)
    b = _raster(cam, 0)
    cb, rb, db, ab = b.forward(sc["means3D"], sc["opacities"], colors=rgb.cpu().numpy(), scales=sc["scales"], rotations=sc["rotations"])
    gb = b.backward(gC, gD, gA)
    assert (ra > 0).sum() > 1000 and (ra == 0).sum() > 10
    for x, y in ((ca, cb), (ra, rb), (da, db), (aa, ab)):
        assert np.array_equal(x, y)
    for k in ("dL_dmeans2D", "dL_dopacity", "dL_dscales", "dL_drots"):
        assert np.array_equal(ga[k], gb[k]), k
    assert np.array_equal(ga["dL_dcolors"], gb["dL_dcolors"])            # dL/drgb, as documented in include/dm4d.h
    # what the SH backward makes of the precomp call's dL_dcolors (culled rows carry zeros already)
    dsh, dp = _sh_backward(_t(sc["means3D"]), _t(cam.campos), _t(sh), degree, cl, _t(gb["dL_dcolors"]))
    dsh, dp = dsh.cpu().numpy(), dp.cpu().numpy()
    assert np.isfinite(ga["dL_dsh"]).all() and np.isfinite(ga["dL_dmeans3D"]).all()
    assert shc.grad_excess(ga["dL_dsh"], dsh) <= 1.0
    extra = ga["dL_dmeans3D"].astype(np.float64) - gb["dL_dmeans3D"].astype(np.float64)
    # the sum is rounded once more to float32: half an ulp of the sum on top of the bar
    ulp = np.abs(ga["dL_dmeans3D"]).astype(np.float64) * shc.U
    err = np.abs(extra - dp)
    bar = shc.GRAD_RTOL * np.abs(dp) + shc.GRAD_ATOL * np.abs(dp).max() + ulp
    assert (err <= bar).all(), float((err / bar).max())
    assert np.abs(dp).max() > 0 and np.abs(dsh[:, 1:]).max() > 0
    culled = ra == 0
    for k in ("dL_dsh", "dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dcolors"):
        assert not ga[k][culled].any(), k


def test_degree_zero_is_untouched():
    """sh_degree = 0 with M = 16 random coefficients gives the bytes of M = 1 holding the first coefficient, forward and every
    gradient, with exact zeros in dL_dsh[:, 1:]."""
    _need_gpu()
    H = W = 128
    cam = syn.make_camera(H, W, elev_deg=20.0, azim_deg=35.0)
    sc = _scene(cam)
    rng = np.random.default_rng(12)
    gC = rng.standard_normal((3, H, W)).astype(np.float32)
    res = []
    for M in (16, 1):
        r = _raster(cam, 0)
        out = r.forward(sc["means3D"], sc["opacities"], shs=np.ascontiguousarray(sc["sh"][:, :M]), scales=sc["scales"],
                        rotations=sc["rotations"])
        res.append((out, r.backward(gC)))
    for x, y in zip(res[0][0], res[1][0]):
        assert np.array_equal(x, y)
    for k in ("dL_dmeans2D", "dL_dmeans3D", "dL_dopacity", "dL_dscales", "dL_drots"):
        assert np.array_equal(res[0][1][k], res[1][1][k]), k
    assert np.array_equal(res[0][1]["dL_dsh"][:, :1], res[1][1]["dL_dsh"])
    assert not res[0][1]["dL_dsh"][:, 1:].any() and np.abs(res[0][1]["dL_dsh"][:, 0]).max() > 0


# ------------------------------------------------------------------------------------------------ Python layer
def _settings(cam, degree, H, W):
    import dreammesh4d_amd.diff_gaussian_rasterization as dgr

    return dgr.GaussianRasterizationSettings(H, W, cam.tanfov, cam.tanfov, _t(np.ones(3)), 1.0, _t(cam.viewmatrix), _t(cam.projmatrix),
                                             degree, _t(cam.campos), False, False)


@pytest.mark.parametrize("degree", [1, 3])
def test_operator_sh_degree_matches_precomputed_colour(degree):
    """GaussianRasterizer(shs, sh_degree = d): the image equals the operator fed with points_rgb_sh's colours bit for bit, and
    autograd returns the full dL_dsh and the dL_dmeans3D that includes the direction term (equal to the precomputed-colour graph,
    where autograd adds points_rgb_sh's backward, within the gradient bar)."""
    _need_gpu()
    import dreammesh4d_amd.diff_gaussian_rasterization as dgr
    from dreammesh4d_amd import geometry as geo

    H = W = 96
    cam = syn.make_camera(H, W, elev_deg=10.0, azim_deg=-50.0)
    sc = _scene(cam, 4000, seed=8)
    M = (degree + 1) ** 2
    gC = _t(np.random.default_rng(2).standard_normal((3, H, W)))
    grads = []
    for mode in ("shs", "precomp"):
        m3, op = _t(sc["means3D"]).requires_grad_(), _t(sc["opacities"][:, None]).requires_grad_()
        scl, rot, sh = _t(sc["scales"]).requires_grad_(), _t(sc["rotations"]).requires_grad_(), _t(sc["sh"][:, :M]).requires_grad_()
        m2 = torch.zeros_like(m3, requires_grad=True)
        if mode == "shs":
            out = dgr.GaussianRasterizer(_settings(cam, degree, H, W))(means3D=m3, means2D=m2, opacities=op, shs=sh, scales=scl, rotations=rot)
        else:
            col = geo.points_rgb_sh(sh, m3, _t(cam.campos), degree + 1)
            out = dgr.GaussianRasterizer(_settings(cam, 0, H, W))(means3D=m3, means2D=m2, opacities=op, colors_precomp=col, scales=scl,
                                                                  rotations=rot)
        (out[0] * gC).sum().backward()
        grads.append((out, dict(m3=m3.grad, m2=m2.grad, op=op.grad, scl=scl.grad, rot=rot.grad, sh=sh.grad)))
    (oa, ga), (ob, gb) = grads
    for x, y in zip(oa, ob):
        assert torch.equal(x, y)
    for k in ("m2", "op", "scl", "rot"):
        assert torch.equal(ga[k], gb[k]), k
    assert tuple(ga["sh"].shape) == (4000, M, 3) and float(ga["sh"][:, 1:].abs().max()) > 0
    assert shc.grad_excess(ga["sh"].cpu().numpy(), gb["sh"].cpu().numpy()) <= 1.0
    assert shc.grad_excess(ga["m3"].cpu().numpy(), gb["m3"].cpu().numpy()) <= 1.0


def test_points_rgb_sh_against_fixture():
    """geometry.points_rgb_sh (the autograd Function over the two entry points): forward within the forward bar, autograd's
    gradients within the gradient bar of the fixture's, sh_levels 2 to 4."""
    _need_gpu()
    from dreammesh4d_amd import geometry as geo

    fx = shc.load()
    for levels in (2, 3, 4):
        d = levels - 1
        K = levels ** 2
        for c in range(2):
            sh, pts = _t(fx["sh"]).requires_grad_(), _t(fx["points"]).requires_grad_()
            rgb = geo.points_rgb_sh(sh, pts, _t(fx["campos"][c])[None], levels)
            (rgb * _t(fx["grad"])).sum().backward()
            v_ref, A = fx[f"v_d{d}_c{c}"], fx[f"A_d{d}_c{c}"]
            got = rgb.detach().cpu().numpy()
            assert shc.forward_excess(got, v_ref < 0, v_ref, A)[0] <= 1.0
            NG = fx[f"dsh_d{d}_c{c}"].shape[0]
            far = (np.abs(v_ref) > shc.K_FORWARD * shc.U * A)[:NG]
            assert shc.grad_excess(sh.grad.cpu().numpy()[:NG, :K], fx[f"dsh_d{d}_c{c}"], keep=np.broadcast_to(far[:, None, :], (NG, K, 3))) <= 1.0
            assert shc.grad_excess(pts.grad.cpu().numpy()[:NG], fx[f"dpoints_d{d}_c{c}"],
                                   keep=np.broadcast_to(far.all(axis=1)[:, None], (NG, 3))) <= 1.0
            assert not sh.grad[:, K:].any()


def _static_geometry(sh_levels):
    from dreammesh4d_amd import sugar

    verts, faces = syn.uv_sphere(1200)
    g = sugar.SuGaR(verts, faces, n_gaussians_per_surface_triangle=1, vertex_colors=np.full((len(verts), 3), 0.6), sh_levels=sh_levels,
                    device=_dev())
    return g


def _view(azim, H=96, W=96):
    from dreammesh4d_amd import renderer as R

    cam = syn.make_camera(H, W, elev_deg=10.0, azim_deg=azim)
    fov = torch.tensor(cam.fovy, device=_dev())
    return R.Camera(FoVx=fov, FoVy=fov, camera_center=_t(cam.campos), image_width=W, image_height=H,
                    world_view_transform=_t(cam.viewmatrix), full_proj_transform=_t(cam.projmatrix))


def test_single_view_renderer_with_sh_levels():
    """The static single-view renderer with sh_levels = 3: with zero higher bands it renders the sh_levels = 1 image bit for bit;
    with a constant DC term and a non-zero degree-1 band two azimuths of a (symmetric) sphere give different images, and the
    higher bands receive a gradient."""
    _need_gpu()
    from dreammesh4d_amd import renderer as R

    g1, g3 = _static_geometry(1), _static_geometry(3)
    r1, r3 = R.DiffSuGaRNormal(g1, training=False), R.DiffSuGaRNormal(g3, training=False)
    a1, a3 = r1.forward(_view(0.0))["render"], r3.forward(_view(0.0))["render"]
    assert torch.equal(a1, a3) and float(a1.detach().std()) > 0
    b1 = r1.forward(_view(90.0))["render"]
    assert float((a1 - b1).abs().max()) < 2e-2                    # constant colour on a sphere: the two views look alike
    with torch.no_grad():
        g3._sh_coordinates_rest[:, 2, :] = torch.tensor([1.2, -0.8, 0.5], device=_dev())     # B_3 = -k1 x: colour varies with azimuth
    a = r3.forward(_view(0.0))["render"]
    b = r3.forward(_view(90.0))["render"]
    assert float((a - b).abs().max()) > 0.1
    assert float((a - a3).abs().max()) > 0.05
    a.sum().backward()
    gr = g3._sh_coordinates_rest.grad
    assert gr is not None and torch.isfinite(gr).all() and float(gr[:, :3].abs().max()) > 0 and g3._points.grad is not None


def test_batched_paths_refuse_sh_levels():
    _need_gpu()
    from dreammesh4d_amd import gviews, static_stage, texture_export
    from dreammesh4d_amd import renderer as R

    g3 = _static_geometry(2)
    with pytest.raises(NotImplementedError, match="sh_levels"):
        static_stage.StaticStage(g3, R.DiffSuGaRNormal(g3), None, None, 64, 64)
    with pytest.raises(NotImplementedError, match="sh_levels"):
        texture_export.canonical_gaussians(g3)
    gv = gviews.GaussianViews(g3.n_gaussians, 64, 64, 0.2, _dev())
    cam = syn.make_camera(64, 64)
    with pytest.raises(NotImplementedError, match="sh_levels"):
        gviews.render_gaussian_views(gv, g3.get_xyz, g3.get_rotation, g3.get_scaling, g3.get_opacity.reshape(-1), g3.get_features,
                                     _t(cam.viewmatrix)[None], _t(cam.projmatrix)[None], _t(np.ones(6)))
