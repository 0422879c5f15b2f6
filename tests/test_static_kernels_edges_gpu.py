"""GPU: the two fused kernels of a static-stage iteration (csrc/sugar_attr.hip: k_sugar_attr_fwd / _bwd; csrc/statichead.hip:
k_static_head_fwd / _bwd) at their branch points, element by element against the float64 reference of tests/static_kernels_edges.py.

Attributes, through the C ABI into NaN-filled buffers with guard rows: G = 1, 3, 4, 6; F = 1, 127, 128, 129; N = 255 .. 258; a fan whose
centre lies in 300 faces; unreferenced vertices; a repeated index; the 24 rotations of the cube times five exact complex numbers
(every `best`, the four-way tie, every two-way tie, w an exact 0, flips); zero-area, coincident and needle faces; a face edge, a
face normal and complex numbers of exactly float32(1e-12); sh at and one float beyond +-clip and on both sides of the zero clamp;
densities and log scales at the ends of their ranges; every upstream gradient alone, none, every output alone; F = 0; the refusals
of sa_check; the public class with a loss on one attribute and with frozen points.

Head: 2x2 to 32x34 and 516x512 (above the 256-workgroup cap, launched once each way); every kind of view, n_ref = 0, n_rnd = 0,
n_ref = 2 of L = 4 with fidx_ref = [3, 1]; planted opacities, colours and normals at the corners and the workgroup seam; zero and
negative weights, g_half absent, g_terms absent.

Asserted per element: |hip - float64| <= 4 x yardstick x 2^-24 x scale (tests/test_static_kernels_edges_cpu.py re-measures the
yardsticks and pins the reference); exact zeros exactly; plain stores bit-identical between calls; dL/dpoints (float atomics) within
its bound on every call.  Every test prints its worst error / bound per tensor kind.
"""
import numpy as np
import pytest
import torch

from tests import static_kernels_edges as ec

pytestmark = pytest.mark.gpu
GUARD = 3
OUT5 = ("g_points", "g_cx", "g_ls", "g_den", "g_sh")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _report(tag, checks):
    """checks: (kind, got, reference S).  Prints the worst error / bound per kind, then asserts all of them."""
    worst, msgs = {}, []
    for kind, got, ref in checks:
        w, msg = ec.compare(kind, got.detach().cpu().numpy() if torch.is_tensor(got) else got, ref, f"{tag} {kind}")
        worst[kind] = max(worst.get(kind, 0.0), w)
        msgs.append(msg)
    print(f"{tag}: worst |error| / bound", {k: round(v, 4) for k, v in worst.items()})
    msgs = [m for m in msgs if m]
    assert not msgs, "\n".join(msgs)


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.detach().contiguous().view(torch.int32), b.detach().contiguous().view(torch.int32))


def _dev(a, dev, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=dev).contiguous()


# ------------------------------------------------------------------------------------------------ SuGaR attributes
class _Attr:
    """The device tensors of a case and the two C-ABI calls, every output NaN-filled with GUARD rows past its end."""

    def __init__(self, name, dev):
        from dreammesh4d_amd import _lib

        self.lib, self.dev, self.inp = _lib, dev, ec.attr_inputs(name)
        inp = self.inp
        self.F, self.G, self.V = len(inp["faces"]), inp["G"], len(inp["points"])
        self.N = self.F * self.G
        self.t = {k: _dev(inp[k], dev) for k in ("points", "bary", "cx", "log_scales", "densities", "sh_dc") + ec.UPSTREAM}
        self.t["faces"] = _dev(inp["faces"], dev, torch.int64)
        self.head = [self.t[k].data_ptr() for k in ("points", "faces", "bary", "cx", "log_scales", "densities", "sh_dc")] + [inp["thickness"], inp["clip"]]

    def _checked(self, bufs, rows):
        torch.cuda.synchronize()
        out = []
        for b, n in zip(bufs, rows):
            if b is None:
                out.append(None)
                continue
            assert bool(torch.isfinite(b[:n]).all()) and bool(torch.isnan(b[n:]).all())       # written to the end, and not past it
            out.append(b[:n])
        return out

    def forward(self):
        N, d = self.N, self.dev
        bufs = [_nan(d, N + GUARD, 3), _nan(d, N + GUARD, 4), _nan(d, N + GUARD, 3), _nan(d, N + GUARD), _nan(d, N + GUARD, 6)]
        self.lib.call("dm4d_sugar_attributes_forward", self.F, self.G, self.V, *self.head, *[b.data_ptr() for b in bufs], self.lib.stream(d))
        self.fwd = self._checked(bufs, [N] * 5)
        return self.fwd

    def backward(self, which=ec.UPSTREAM, want=OUT5):
        N, d = self.N, self.dev
        rows = [self.V, N, N, N, N]
        bufs = [_nan(d, r + GUARD, *s) if k in want else None for k, r, s in zip(OUT5, rows, ((3,), (2,), (2,), (), (3,)))]
        ups = [self.t[k].data_ptr() if k in which else None for k in ec.UPSTREAM]
        self.lib.call("dm4d_sugar_attributes_backward", self.F, self.G, self.V, *self.head, self.fwd[2].data_ptr(), self.fwd[3].data_ptr(), *ups,
                      *[self.lib.ptr(b) for b in bufs], self.lib.stream(d))
        return dict(zip(OUT5, self._checked(bufs, rows)))


@pytest.mark.parametrize("name", [c.name for c in ec.ATTR_CASES])
def test_sugar_attributes_and_their_gradients_element_by_element(name):
    dev = _need_gpu()
    case, ref = ec.ATTR_BY_NAME[name], ec.attr_case_reference(name)
    a = _Attr(name, dev)
    fwd = a.forward()
    got = a.backward()
    _report(name, [(k, t, ref[k]) for k, t in zip(ec.ATTR_KINDS[:5], fwd)] + [(k, got[k], ref[k]) for k in OUT5])
    # plain stores: a repeated call gives the same bits; dL/dpoints (atomics) stays within its bound
    again, fwd2 = a.backward(), _Attr(name, dev).forward()
    assert all(_same_bits(x, y) for x, y in zip(fwd, fwd2)) and all(_same_bits(again[k], got[k]) for k in OUT5[1:])
    _report(f"{name} repeated", [("g_points", again["g_points"], ref["g_points"])])
    inp, br = a.inp, ref["branches"]
    assert bool((fwd[2][:, 0] == inp["thickness"]).all())
    sat = torch.as_tensor(inp["densities"] == 30.0, device=dev)
    assert bool(sat.any()) and bool((fwd[3][sat] == 1.0).all()) and not got["g_den"][sat].any()       # 1 + exp(-30) == 1 in float32
    lonely = sorted(set(range(a.V)) - set(inp["faces"].reshape(-1).tolist()))
    assert not got["g_points"][lonely].any()
    w = fwd[1][:, 0].cpu().numpy()
    assert (w >= 0).all() and (w[br["w_zero"]] == 0).all()
    if case.mesh == "special":
        for what in ("collinear", "coincident", "repeated"):
            f = ec.SPECIAL[what][0]
            assert not fwd[4][f * a.G:(f + 1) * a.G, 3:].any(), what                                    # n an exact zero


@pytest.mark.parametrize("name", [c.name for c in ec.ATTR_CASES if c.variants])
def test_sugar_attributes_with_absent_upstream_gradients_and_absent_outputs(name):
    dev = _need_gpu()
    a = _Attr(name, dev)
    a.forward()
    full = a.backward()
    for which in [(k,) for k in ec.UPSTREAM] + [()]:
        ref, got = ec.attr_case_reference(name, which), a.backward(which)
        _report(f"{name} upstream {which or 'none'}", [(k, got[k], ref[k]) for k in OUT5])
        if not which:
            assert all(not got[k].any() for k in OUT5)
    for k in OUT5:                                               # each output alone
        got = a.backward(ec.UPSTREAM, (k,))
        if k == "g_points":
            _report(f"{name} only {k}", [(k, got[k], ec.attr_case_reference(name)[k])])
        else:
            assert _same_bits(got[k], full[k]), k


@pytest.mark.parametrize("name", [c.name for c in ec.ATTR_CASES if c.variants])
def test_render_attributes_of_the_public_class_equal_the_c_abi_calls(name):
    dev = _need_gpu()
    from dreammesh4d_amd import sugar

    case = ec.ATTR_BY_NAME[name]
    a = _Attr(name, dev)
    fwd = a.forward()
    inp = a.inp

    def model(learn_positions=True):
        g = sugar.SuGaR(inp["points"], inp["faces"], n_gaussians_per_surface_triangle=case.G, color_clip=case.clip, learn_positions=learn_positions,
                        device=dev)
        with torch.no_grad():
            g._quaternions.copy_(a.t["cx"])
            g._scales.copy_(a.t["log_scales"])
            g.all_densities.copy_(a.t["densities"][:, None])
            g._sh_coordinates_dc.copy_(a.t["sh_dc"][:, None])
        assert g.fused_attributes and float(np.float32(3.8 / 1_000_000)) == inp["thickness"]
        return g, [g._points, g._quaternions, g._scales, g.all_densities, g._sh_coordinates_dc]

    for key, up in (("xyz", "g_means"), ("rotation", "g_rots")):
        g, params = model()
        out = g.render_attributes()
        assert all(_same_bits(out[k].reshape(t.shape), t) for k, t in (("xyz", fwd[0]), ("rotation", fwd[1]), ("scaling", fwd[2]), ("opacity", fwd[3]), ("colors6", fwd[4])))
        (out[key] * a.t[up]).sum().backward()
        want = a.backward((up,))
        for k, p in zip(OUT5[1:], params[1:]):
            assert _same_bits(p.grad.reshape(want[k].shape), want[k]), (key, k)
        _report(f"{name} class, loss on {key}", [("g_points", params[0].grad, ec.attr_case_reference(name, (up,))["g_points"])])
    g, params = model(learn_positions=False)                     # dL/dpoints not wanted: a null pointer
    out = g.render_attributes()
    sum((out[k].reshape(a.t[u].shape) * a.t[u]).sum() for k, u in (("xyz", "g_means"), ("rotation", "g_rots"), ("scaling", "g_scales"), ("opacity", "g_opac"),
                                                                    ("colors6", "g_colors"))).backward()
    want = a.backward()
    assert params[0].grad is None and all(_same_bits(p.grad.reshape(want[k].shape), want[k]) for k, p in zip(OUT5[1:], params[1:]))


def test_sugar_attributes_without_faces_and_argument_checks_write_nothing():
    dev = _need_gpu()
    a = _Attr("attr-F1-G4", dev)
    L, st, N = a.lib.lib(), a.lib.stream(dev), a.N
    outs = [_nan(dev, N, 3), _nan(dev, N, 4), _nan(dev, N, 3), _nan(dev, N), _nan(dev, N, 6)]
    grads = [_nan(dev, a.V, 3), _nan(dev, N, 2), _nan(dev, N, 2), _nan(dev, N), _nan(dev, N, 3)]
    ups = [a.t[k].data_ptr() for k in ec.UPSTREAM]
    po, pg = [t.data_ptr() for t in outs], [t.data_ptr() for t in grads]
    fwd = lambda F, G, V, o=po: L.dm4d_sugar_attributes_forward(F, G, V, *a.head, *o, st)
    bwd = lambda F, G, V, s=po[2], o=po[3]: L.dm4d_sugar_attributes_backward(F, G, V, *a.head, s, o, *ups, *pg, st)
    assert fwd(0, a.G, a.V) == a.lib.OK and bwd(0, a.G, a.V) == a.lib.OK                              # F = 0: nothing to do
    for G in (0, 2, 7):
        assert fwd(a.F, G, a.V) == bwd(a.F, G, a.V) == a.lib.DM4D_ERR_INVALID
    assert fwd(a.F, a.G, 0) == bwd(a.F, a.G, 0) == fwd(-1, a.G, a.V) == a.lib.DM4D_ERR_INVALID
    for k in range(5):
        assert fwd(a.F, a.G, a.V, po[:k] + [None] + po[k + 1:]) == a.lib.DM4D_ERR_INVALID and b"null output" in L.dm4d_last_error()
    assert bwd(a.F, a.G, a.V, s=None) == bwd(a.F, a.G, a.V, o=None) == a.lib.DM4D_ERR_INVALID
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in outs + grads)
    assert fwd(a.F, a.G, a.V) == a.lib.OK and bwd(a.F, a.G, a.V) == a.lib.OK                          # ... and the library is as usable as before
    torch.cuda.synchronize()
    ref = ec.attr_case_reference("attr-F1-G4")
    _report("attr-F1-G4 after the refusals", [(k, t, ref[k]) for k, t in zip(ec.ATTR_KINDS, outs + grads)])


# ------------------------------------------------------------------------------------------------ static head
class _Head:
    def __init__(self, name, dev):
        from dreammesh4d_amd import _lib

        self.lib, self.dev, self.case, inp = _lib, dev, ec.HEAD_BY_NAME[name], ec.head_inputs(name)
        self.t = {k: _dev(inp[k], dev) for k in ("color", "depth", "alpha", "ref_images", "ref_masks", "g_terms")}
        self.t["g_half"] = None if inp["g_half"] is None else _dev(inp["g_half"], dev)
        self.t.update(ref_pos=_dev(inp["ref_pos"], dev, torch.int32), rnd_pos=_dev(inp["rnd_pos"], dev, torch.int32), fidx_ref=_dev(inp["fidx_ref"], dev, torch.int64))
        c = self.case
        self.args = [c.B, c.H, c.W] + [self.t[k].data_ptr() for k in ("color", "depth", "alpha", "ref_pos", "rnd_pos", "ref_images", "ref_masks", "fidx_ref")] + \
            [c.n_ref, c.n_rnd]
        self.nb = _lib.lib().dm4d_static_head_blocks(c.H, c.W)

    def forward(self):
        c, d = self.case, self.dev
        partial, half = _nan(d, c.B, self.nb, 8), _nan(d, c.n_rnd, c.H // 2, c.W // 2, 3)
        self.lib.call("dm4d_static_head_forward", *self.args, partial.data_ptr(), half.data_ptr() if c.n_rnd else None, self.lib.stream(d))
        return partial, half

    def backward(self, g_terms, g_half):
        c, d = self.case, self.dev
        out = [_nan(d, c.B, 6, c.H, c.W), _nan(d, c.B, 1, c.H, c.W), _nan(d, c.B, 1, c.H, c.W)]
        self.lib.call("dm4d_static_head_backward", *self.args, g_terms.data_ptr(), self.lib.ptr(g_half), *[t.data_ptr() for t in out], self.lib.stream(d))
        return out

    def terms(self, partial):
        from dreammesh4d_amd.loss_sum import partial_sums
        from dreammesh4d_amd.static_head import _norm_matrix

        c = self.case
        return partial_sums(partial.reshape(c.B * self.nb, 8), _norm_matrix(c.H, c.W, c.n_ref, c.n_rnd, self.dev))


def _head_checks(ref, gc, gd, ga):
    return [("g_color", gc, ref["g_color"]), ("g_depth", gd, ref["g_depth"]), ("g_alpha", ga, ref["g_alpha"])]


@pytest.mark.parametrize("name", [c.name for c in ec.HEAD_CASES])
def test_static_head_sums_terms_and_gradients_element_by_element(name):
    dev = _need_gpu()
    from dreammesh4d_amd.static_head import static_head

    case, ref = ec.HEAD_BY_NAME[name], ec.head_case_reference(name)
    h = _Head(name, dev)
    assert h.nb == ec.head_blocks(case.H, case.W)
    partial, half = h.forward()
    grads = h.backward(h.t["g_terms"], h.t["g_half"])
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in (partial, half, *grads))
    terms = h.terms(partial)
    _report(name, [("partial", partial, ref["partial"]), ("terms", terms, ref["terms"]), ("half", half, ref["half"])] + _head_checks(ref, *grads))
    thin = h.t["alpha"] <= float(ec.A99)
    assert not grads[1][thin].any() and not grads[0][:, 3:][thin.expand(-1, 3, -1, -1)].any()
    if name == ec.BIG:                                           # launched once each way
        return
    # a repeated call: the same bits
    p2, h2 = h.forward()
    assert _same_bits(p2, partial) and _same_bits(h2, half) and all(_same_bits(x, y) for x, y in zip(h.backward(h.t["g_terms"], h.t["g_half"]), grads))
    # the public operator: the same kernels behind autograd
    leaves = [h.t[k].clone().requires_grad_(True) for k in ("color", "depth", "alpha")]
    views = [h.t[k] for k in ("ref_pos", "rnd_pos", "ref_images", "ref_masks", "fidx_ref")]
    t5, hf = static_head(*leaves, *views, case.n_ref, case.n_rnd)
    assert _same_bits(t5, terms) and _same_bits(hf, half)
    loss = (t5 * h.t["g_terms"]).sum() + (0 if h.t["g_half"] is None else (hf * h.t["g_half"]).sum())
    loss.backward()
    assert all(_same_bits(leaf.grad, g) for leaf, g in zip(leaves, grads))
    if h.t["g_half"] is not None:
        # g_half absent (a null pointer) ...
        _report(f"{name} without g_half", _head_checks(ec.head_case_reference(name, True, False), *h.backward(h.t["g_terms"], None)))
        # ... and g_terms absent: only half_rgb in the loss, the wrapper's zeros
        leaves = [h.t[k].clone().requires_grad_(True) for k in ("color", "depth", "alpha")]
        (static_head(*leaves, *views, case.n_ref, case.n_rnd)[1] * h.t["g_half"]).sum().backward()
        _report(f"{name} without g_terms", _head_checks(ec.head_case_reference(name, False, True), *[leaf.grad for leaf in leaves]))
