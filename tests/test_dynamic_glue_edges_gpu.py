"""GPU: the small fused kernels between the renderer, the guidance and the optimiser -- csrc/imagehead.hip (image head, partial sums,
weighted sum), csrc/dscale.hip, csrc/sds_glue.hip -- at their edges, element by element, through the C ABI (null pointers, strides and
NaN-filled output buffers included), against the references of tests/dynamic_glue_edges.py.

Image head, loss sums, d_scale: every element within FACTOR x YARD[kind] x 2^-24 x scale of the float64 closed form; elements of scale 0
(a view without a role, channels 3.., a null upstream gradient, one float outside [0, 1], an unreferenced node, a vertex in no face)
exactly 0; the weighted sum and its backward bit-identical to the float32 expression.  SDS glue: latents, x_in, t2 and the clamp mask
bit-identical to the float16 restatement, loss and |grad| under the scale bound, d_moments within 0.1 % / 2 float16 ulps, the padding
of sliced outputs untouched.  What each case reaches is listed where it is defined; the CPU file pins the references themselves.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import dynamic_glue_edges as ec

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _p(t):
    return 0 if t is None else t.data_ptr()


def _np(t):
    return t.detach().cpu().numpy()


def _judge(msgs, kind, got, ref, what):
    got = _np(got) if torch.is_tensor(got) else got
    worst, msg = ec.compare(kind, got, ref, what)
    print(f"{what}: worst error / bound {worst:.3f}", flush=True)
    if msg:
        msgs.append(msg)


# ------------------------------------------------------------------------------------------------ image head
@pytest.mark.parametrize("name", [c.name for c in ec.HEAD_CASES])
def test_image_head_kernels_against_the_closed_form(name):
    dev = _need_gpu()
    from dreammesh4d_amd import _lib
    from dreammesh4d_amd.loss_sum import partial_sums

    c = ec.HEAD_BY_NAME[name]
    B, Cn, H, W, n_ref, n_rnd = c.B, c.C, c.H, c.W, c.n_ref, c.n_rnd
    nb = _lib.lib().dm4d_image_head_blocks(H, W)
    assert nb == ec.head_blocks(H, W)
    T = lambda a: None if a is None else torch.tensor(a, device=dev)
    full = ec.head_inputs(name)
    color, alpha, ref_pos, rnd_pos = T(full["color"]), T(full["alpha"]), T(full["ref_pos"]), T(full["rnd_pos"])
    ref_images, ref_masks = T(full["ref_images"]), T(full["ref_masks"])
    fidx = T(full["fidx_ref"]) if n_ref else None
    head = (B, H, W, Cn, _p(color), _p(alpha), _p(ref_pos), _p(rnd_pos), _p(ref_images), _p(ref_masks), _p(fidx), n_ref, n_rnd)
    s = _lib.stream(dev)
    msgs = []
    ref = ec.head_case_reference(name)
    partial = torch.full((B, nb, 2), NAN, device=dev)
    half = torch.full((n_rnd, H // 2, W // 2, 3), NAN, device=dev) if n_rnd else None          # n_rnd = 0: a null half_rgb
    _lib.call("dm4d_image_head_forward", *head, _p(partial), _p(half), s)
    d = float(max(n_ref, 1) * H * W)
    means = partial_sums(partial.view(-1, 2), [[1.0 / (3.0 * d), 0.0], [0.0, 1.0 / d]])       # as image_head.py calls it
    _judge(msgs, "partial", partial, ref["partial"], f"{name} partial")
    _judge(msgs, "means", means, ref["means"], f"{name} means")
    if n_rnd:
        _judge(msgs, "half", half, ref["half"], f"{name} half")
    for var in ec.head_variants(name):
        inp, ref = ec.head_inputs(name, *var), ec.head_case_reference(name, *var)
        g_rgb, g_mask, g_half = T(inp["g_rgb"]), T(inp["g_mask"]), T(inp["g_half"])
        gc, ga = torch.full((B, Cn, H, W), NAN, device=dev), torch.full((B, 1, H, W), NAN, device=dev)
        _lib.call("dm4d_image_head_backward", *head, _p(g_rgb), _p(g_mask), _p(g_half), _p(gc), _p(ga), s)
        tag = f"{name} (g_rgb {var[0]}, g_mask {var[1]}, g_half {var[2]})"
        _judge(msgs, "g_color", gc, ref["g_color"], f"{tag} g_color")
        _judge(msgs, "g_alpha", ga, ref["g_alpha"], f"{tag} g_alpha")
    assert not msgs, "\n".join(msgs)


def test_partial_sums_at_every_size():
    dev = _need_gpu()
    from dreammesh4d_amd.loss_sum import partial_sums

    msgs = []
    for n, k, m in ec.PSUM_CASES:
        partial, mat = ec.psum_inputs(n, k, m)
        out = partial_sums(torch.tensor(partial, device=dev), [[float(v) for v in row] for row in mat])
        assert out.shape == (m,)
        worst, msg = ec.compare("psum", _np(out), ec.psum_reference(n, k, m), f"partial_sums n {n} k {k} m {m}")
        if msg:
            msgs.append(msg)
    assert not msgs, "\n".join(msgs)


def test_weighted_sum_is_the_float32_expression_bit_for_bit():
    dev = _need_gpu()
    from dreammesh4d_amd.loss_sum import weighted_sum

    for name, pairs in ec.wsum_cases().items():
        want, gw = ec.wsum_reference(pairs, 1.3)
        terms = [torch.tensor(t, device=dev, requires_grad=True) for _, t in pairs]
        out = weighted_sum([(w, t) for (w, _), t in zip(pairs, terms)])
        assert out.is_cuda and np.array_equal(_np(out).view(np.uint32), np.asarray(want).view(np.uint32)), (name, float(out), float(want))
        out.backward(torch.tensor(np.float32(1.3), device=dev))
        got = np.concatenate([_np(t.grad).reshape(-1) for t in terms])
        assert np.array_equal(got.view(np.uint32), gw.view(np.uint32)), (name, got, gw)


# ------------------------------------------------------------------------------------------------ d_scale
@pytest.mark.parametrize("method", ec.DS_METHODS)
@pytest.mark.parametrize("name", [c.name for c in ec.DS_CASES])
def test_d_scale_kernels_against_the_closed_form(name, method):
    dev = _need_gpu()
    from dreammesh4d_amd import _lib
    from dreammesh4d_amd.ops import METHODS

    c, inp, ref = ec.DS_BY_NAME[name], ec.ds_inputs(name, method), ec.ds_case_reference(name, method)
    V, K = inp["idx"].shape
    NF, M, G, F = c.NF, c.M, c.G, len(inp["faces"])
    N, hybrid = F * G, method == "hybrid"
    T = lambda a, dt=None: torch.tensor(np.ascontiguousarray(a if dt is None else a.astype(dt)), device=dev)
    nan = lambda *shape: torch.full(shape, NAN, device=dev)
    idx, w, ds, dop = T(inp["idx"], np.int32), T(inp["w"]), T(inp["ds"]), (T(inp["dop"]) if hybrid else None)
    assert inp["idx"].min() >= 0 and inp["idx"].max() < M and inp["faces"].min() >= 0 and inp["faces"].max() < V
    s, m, msgs = _lib.stream(dev), METHODS[method], []
    Sv = nan(NF, V, 3, 3)
    _lib.call("dm4d_vertex_scales_forward", m, NF, V, M, K, _p(idx), _p(w), _p(ds), _p(dop), _p(Sv), s)
    _judge(msgs, "Sv", Sv, ref["Sv"], f"{name} {method} Sv")
    if not hybrid and NF == 3:                                        # no strain, weights that add up to exactly 1
        rows = [4, 5] if K >= 2 else [0, 1]
        assert np.array_equal(_np(Sv)[2, rows], np.broadcast_to(np.eye(3, dtype=np.float32), (2, 3, 3)))
    off, items = ec.csr(inp["idx"], M)
    assert off[-1] == V * K and len(items) == V * K
    off, items, g_Sv = T(off), T(items), T(inp["g_Sv"])
    for with_dop in ((True, False) if hybrid else (False,)):          # (a null dL/dd_opacity: dL/dds is written all the same)
        g_ds, g_dop = nan(NF, M, 6), (nan(NF, M) if with_dop else None)
        _lib.call("dm4d_vertex_scales_backward", m, NF, V, M, K, _p(idx), _p(w), _p(ds), _p(dop), _p(off), _p(items), _p(g_Sv), _p(g_ds), _p(g_dop), s)
        _judge(msgs, "g_ds", g_ds, ref["g_ds"], f"{name} {method} g_ds")
        if with_dop:
            _judge(msgs, "g_dop", g_dop, ref["g_dop"], f"{name} {method} g_dop")
            if M > 3:
                assert not _np(g_dop)[:, 2].any(), "saturated opacity: o (1 - o) == 0 exactly"
    # ---- the Gaussians' scales from the float32 vertex matrices of the case
    faces, bary, sv_in, scaling, g_gs = T(inp["faces"], np.int32), T(inp["bary"]), T(inp["sv_in"]), T(inp["scaling"]), T(inp["g_gs"])
    gs = nan(NF, N, 3)
    _lib.call("dm4d_gaussian_scales_forward", NF, F, G, V, _p(faces), _p(bary), _p(sv_in), _p(scaling), _p(gs), s)
    _judge(msgs, "gscales", gs, ref["gscales"], f"{name} {method} gscales")
    off, items = ec.csr(inp["faces"], V)
    assert off[-1] == 3 * F and len(items) == 3 * F
    off, items = T(off), T(items)
    for want_sv, want_sc in ((True, True), (False, True), (True, False)):
        g_sv, g_sc = (nan(NF, V, 3, 3) if want_sv else None), (nan(N, 3) if want_sc else None)
        _lib.call("dm4d_gaussian_scales_backward", NF, F, G, V, _p(faces), _p(bary), _p(sv_in), _p(scaling), _p(off), _p(items), _p(g_gs), _p(g_sv),
                  _p(g_sc), s)
        if want_sv:
            _judge(msgs, "g_sv", g_sv, ref["g_sv"], f"{name} {method} g_sv (g_scaling {want_sc})")
        if want_sc:
            _judge(msgs, "g_scaling", g_sc, ref["g_scaling"], f"{name} {method} g_scaling (g_sv {want_sv})")
    assert not msgs, "\n".join(msgs)


def test_d_scale_equality_vertices_pass_the_gradient():
    """The hybrid clamp at lw + 0.4f == 1 exactly: torch.clamp passes the gradient there, so the -w tr g term of the (1 - lw) I
    diagonal reaches dL/dd_opacity of the equality vertices' nodes.  Named on its own so that a `<` for a `<=` reads as what it is."""
    dev = _need_gpu()
    from dreammesh4d_amd import _lib

    name, method = "patch-K2-G1-T1", "hybrid"
    c, inp, ref = ec.DS_BY_NAME[name], ec.ds_inputs(name, method), ec.ds_case_reference(name, method)
    V, K = inp["idx"].shape
    assert len(inp["eq_vertices"]) == 2 and (ref["lw"][:, inp["eq_vertices"]] == 1).all()
    T = lambda a, dt=None: torch.tensor(np.ascontiguousarray(a if dt is None else a.astype(dt)), device=dev)
    off, items = ec.csr(inp["idx"], c.M)
    idx, w, ds, dop, off, items, g_Sv = T(inp["idx"], np.int32), T(inp["w"]), T(inp["ds"]), T(inp["dop"]), T(off), T(items), T(inp["g_Sv"])
    g_ds, g_dop = torch.full((c.NF, c.M, 6), NAN, device=dev), torch.full((c.NF, c.M), NAN, device=dev)
    _lib.call("dm4d_vertex_scales_backward", 2, c.NF, V, c.M, K, _p(idx), _p(w), _p(ds), _p(dop), _p(off), _p(items), _p(g_Sv), _p(g_ds), _p(g_dop),
              _lib.stream(dev))
    nodes = sorted(set(inp["idx"][inp["eq_vertices"], :2].reshape(-1).tolist()))
    worst, msg = ec.compare("g_dop", _np(g_dop)[:, nodes], ec.S(ref["g_dop"].v[:, nodes], ref["g_dop"].s[:, nodes]), f"g_dop of nodes {nodes}")
    assert msg is None, msg


# ------------------------------------------------------------------------------------------------ SDS glue
def _laid_out(a, layout, dev, fill=None):
    """(tensor of a's shape in `layout` on the device, the buffer it lives in): holding `a`, or `fill` everywhere when a is a shape."""
    shape = a if isinstance(a, tuple) else a.shape
    dtype = fill[1] if isinstance(a, tuple) else torch.tensor(a[:0]).dtype
    B, Cn, H, W = shape
    pad = NAN if isinstance(a, tuple) else 0
    if layout == "slice":
        big = torch.full((B + 1, Cn + 2, H + 1, W + 3), pad, dtype=dtype, device=dev)
        view = big[:B, 1:Cn + 1, :H, 2:W + 2]
    elif layout == "channels_last":
        big = torch.full((B, H, W, Cn), pad, dtype=dtype, device=dev)
        view = big.permute(0, 3, 1, 2)
    else:
        big = torch.full(shape, pad, dtype=dtype, device=dev)
        view = big
    if not isinstance(a, tuple):
        view.copy_(torch.tensor(a))
    assert tuple(view.shape) == tuple(shape)
    return view, big


def _padding_untouched(view, big, layout):
    if layout != "slice":
        return True
    B, Cn, H, W = view.shape
    m = torch.ones(big.shape, dtype=torch.bool)
    m[:B, 1:Cn + 1, :H, 2:W + 2] = False
    return bool(torch.isnan(big.cpu().float()[m]).all())


@pytest.mark.parametrize("name", [c.name for c in ec.SDS_CASES])
def test_sds_glue_kernels_against_the_float16_restatement(name):
    dev = _need_gpu()
    from dreammesh4d_amd import _lib

    i = [c.name for c in ec.SDS_CASES].index(name)
    c, inp, rs = ec.SDS_BY_NAME[name], ec.sds_inputs(name), ec.sds_case_restatement(name)
    B, H, W = c.B, c.H, c.W
    assert inp["t"].min() >= 0 and inp["t"].max() < len(inp["alphas"]) and inp["fidx"].min() >= 0 and inp["fidx"].max() < c.L
    lay = {t: ec.sds_layout(i, t) for t in ec.SDS_TENSORS}
    moments, _ = _laid_out(inp["moments"], lay["moments"], dev)
    post, _ = _laid_out(inp["post"], lay["post"], dev)
    noise, _ = _laid_out(inp["noise"], lay["noise"], dev)
    cc, _ = _laid_out(inp["c_concat"], lay["c_concat"], dev)
    pred, _ = _laid_out(inp["pred"], lay["pred"], dev)
    latents, latents_big = _laid_out((B, 4, H, W), lay["latents"], dev, (NAN, torch.float32))
    x_in, x_in_big = _laid_out((2 * B, 8, H, W), lay["x_in"], dev, (NAN, torch.float16))
    d_mom, d_mom_big = _laid_out((B, 8, H, W), lay["d_moments"], dev, (NAN, torch.float16))
    t, fidx, alphas = torch.tensor(inp["t"], device=dev), torch.tensor(inp["fidx"], device=dev), torch.tensor(inp["alphas"], device=dev)
    t2 = torch.full((2 * B,), -1, dtype=torch.long, device=dev)
    loss, gnorm = torch.full((), NAN, device=dev), torch.full((), NAN, device=dev)
    clip = None if inp["clip"] is None else torch.tensor(np.float32(inp["clip"]), device=dev)
    ptr = lambda v: C.c_void_p(v.data_ptr())
    st = lambda v: (C.c_int64 * 4)(*v.stride())
    s = _lib.stream(dev)
    sf, gsc = float(inp["scale_factor"]), float(inp["guidance_scale"])
    _lib.call("dm4d_sds_prepare", B, H, W, sf, ptr(moments), st(moments), ptr(post), st(post), ptr(noise), st(noise), ptr(latents), st(latents),
              ptr(t), ptr(alphas), ptr(cc), st(cc), ptr(fidx), ptr(x_in), st(x_in), ptr(t2), s)
    _lib.call("dm4d_sds_finish", B, H, W, sf, gsc, ptr(pred), st(pred), ptr(latents), st(latents), ptr(noise), st(noise), ptr(t), ptr(alphas),
              None if clip is None else ptr(clip), ptr(moments), st(moments), ptr(post), st(post), ptr(d_mom), st(d_mom), ptr(loss), ptr(gnorm), s)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint16)
    lat, xi, dm = _np(latents), _np(x_in), _np(d_mom)
    assert np.array_equal(bits(lat), bits(rs["latents"])), f"latents: {int((bits(lat) != bits(rs['latents'])).sum())} of {lat.size} elements differ"
    assert np.array_equal(bits(xi), bits(rs["x_in"])), f"x_in: {int((bits(xi) != bits(rs['x_in'])).sum())} of {xi.size} elements differ"
    assert np.array_equal(_np(t2), rs["t2"])
    for what, view, big in (("latents", latents, latents_big), ("x_in", x_in, x_in_big), ("d_moments", d_mom, d_mom_big)):
        assert _padding_untouched(view, big, lay[what]), f"{what}: the padding of the sliced output was written"
    assert not bits(dm[:, 4:])[~rs["inside"]].any(), "the clamp's mask: d_moments[:, 4:] must be exactly 0 outside [-30, 20]"
    share, ulps = ec.half_mismatch(dm, rs["d_moments"])
    print(name, "d_moments: share of differing elements", share, "worst float16 ulps", ulps, flush=True)
    for j in list(zip(*np.nonzero(bits(dm) != bits(rs["d_moments"]))))[:8]:
        b, ch, y, x = (int(v) for v in j)
        print("   ", j, "got", dm[j], "restatement", rs["d_moments"][j], "logvar", inp["moments"][b, 4 + ch % 4, y, x], "post", inp["post"][b, ch % 4, y, x],
              "g", rs["g"][b, ch % 4, y, x], flush=True)
    assert share <= 1e-3 and ulps <= 2.0, (share, ulps)
    (l64, n64), (l32, _) = ec.sds_sums(rs, B), ec.sds_sums(rs, B, np.float32)
    got_l, got_n = float(loss), float(gnorm)
    print(name, "loss", got_l, l64, "|grad|", got_n, n64, flush=True)
    if np.isfinite(l32):
        assert abs(got_l - l64) <= ec.FACTOR * ec.YARD["sds_loss"] * ec.U * l64, (got_l, l64)
        assert abs(got_n - n64) <= ec.FACTOR * ec.YARD["sds_norm"] * ec.U * n64, (got_n, n64)
    else:
        assert got_l == np.inf and got_n == np.inf, (got_l, got_n)
