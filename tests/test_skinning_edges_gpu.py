"""GPU: the HIP skinning and face -> Gaussian kernels (through ops.skin_vertices / ops.face_gaussians, so through the C ABI)
at their branch points, element by element, against the float64 oracle on the same float32 inputs.

Inputs (tests/skinning_edge_cases.py): node / vertex rotations in one magnitude class each -- exactly zero; around the
1.19e-7, 1e-4 and 1e-3 series switches; right above 1e-3; the usual 0.15; angles up to pi with w < 0; w ~ 0 -- all classes in
one call and each class alone; K in {1, 2, 3, 4, 5, 8}; K = 4 with V in {1, 63, 64, 65, 1001, 1500} (partial last block of the
DPP-quad kernel); unreferenced nodes (gradient exactly 0), a node referenced by every vertex, zero weights; the hybrid blend
on both sides of and next to its clamp; upstream gradients absent (null pointers); zero-area faces.
Left out, because the REFERENCE is singular there: vertices whose blended real dual-quaternion part sum_k w_k q_k has norm
< 0.25 (antipodal neighbours nearly cancel), vertices with 0 < |eta + 0.4f - 1| < 1e-6 (at most 0.5 % of a scene, asserted on
the CPU; a vertex EXACTLY at the clamp is decidable and takes part: torch.clamp passes the gradient there, and so must the
kernels -- `clamp-eq/K2` and `clamp-eq/K4`), the zero-area faces' normal gradient (1e12-scale through the 1e-12 clamp; it lands on vertices of their own).

Asserted: everything finite; forward per element 2e-6 absolute (quaternions as stored: the reference's sign); backward per
element |hip - ref| <= B (|ref| + s), s = the row's summed upstream-gradient norms, B = 8 x the float32 floor of the oracle's
own formulas (F32_FLOOR = 5.4e-7 measured on the CPU, so B = 4.3e-6); bit-identical re-runs.

Measured on an MI355X, worst |hip - ref| / (|ref| + s), class alone, exact / pypose convention (float32 floor 5.4e-7, bar
4.3e-6; DESIGN.md "Skinning kernels at their branch points" has the full table):
    skinning  zero 5.5e-8 / 6.5e-8   eps 6.7e-8 / 7.7e-8   1e-4 7.7e-8 / 9.6e-8   1e-3 1.5e-7 / 1.1e-7   above_1e-3 1.1e-7 / 1.4e-7
              0.15 2.0e-7 / 1.2e-7   1 1.5e-7 / 1.1e-7     3 1.0e-7 / 9.0e-8      w0 5.1e-7 / 6.0e-7     all 2.2e-7 / 2.4e-7
    face      every class 8.1e-8 / 8.1e-8, all classes in one call 9.6e-8 / 9.6e-8
Before row_times_Jl took 1 - cos t as 2 sin^2(t / 2) and row_times_Jl_inv took cot(t / 2) of the half angle, the pypose
column read 1.0e-5 (1e-3), 1.6e-5 (above_1e-3), 1.6e-4 (w0), 7.1e-5 (all) for skinning and up to 2.9e-5 (w0) for the face
kernels; the exact column was the same as now.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import skinning_edge_cases as ec

pytestmark = pytest.mark.gpu
FWD_ATOL = 2e-6


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _poison(dev, sizes):
    """The operators allocate their outputs uninitialised; leave NaN in freed blocks of the sizes the next backward asks the
    caching allocator for, so that a row the kernel does not write reads as NaN rather than as the zero of an earlier call."""
    for _ in range(2):
        junk = [torch.full((n,), float("nan"), device=dev) for n in sizes for _ in range(3)]
        del junk


def _skin_hip(sc, graph, method, mode, gx, gr):
    from dreammesh4d_amd import ops

    dev = graph.device
    leaves = {k: torch.tensor(sc[k], device=dev).requires_grad_(True) for k in ("dx", "dr", "ds", "do")}
    xyz, rot = ops.skin_vertices(graph, leaves["dx"], leaves["dr"], leaves["ds"], leaves["do"], method=method, grad_mode=mode)
    gxd, grd = gx.to(dev), gr.to(dev)
    _poison(dev, [sc["M"] * c for c in (3, 4, 6, 1)])
    torch.autograd.backward([xyz, rot], [gxd, grd])
    grads = {k: (np.zeros(v.shape) if v.grad is None else _np(v.grad)).reshape(sc["M"], -1) for k, v in leaves.items()}
    return _np(xyz), _np(rot), grads


def _skin_case(sc, label, method, mode, report):
    """One forward + backward of one scene; asserts the forward, returns nothing, adds the worst ratios to `report`."""
    from dreammesh4d_amd import ops

    dev = torch.device("cuda:0")
    graph = ops.DeformGraph(sc["verts"], sc["nbr_idx"], sc["nbr_w"], sc["M"], dev)
    gx, gr, keep = ec.skin_upstream(sc, method)
    s = ec.skin_row_scale(sc, gx, gr)
    oxyz, orot, og = ec.skin_reference(sc, method, mode, gx, gr)
    xyz, rot, g = _skin_hip(sc, graph, method, mode, gx, gr)
    tag = f"{label}/{method}/{mode}"
    assert np.isfinite(xyz).all() and np.isfinite(rot).all() and all(np.isfinite(v).all() for v in g.values()), tag
    fx = float(np.abs(xyz - oxyz)[keep].max()) if keep.any() else 0.0
    fr = float(np.abs(rot - orot).max())
    r = ec.skin_ratios(sc, method, g, og, s)
    for k in ("dx", "dr", "ds", "do"):                     # nodes no vertex references: exactly 0, in every gradient
        assert not g[k][sc["M"] - ec.N_UNREF:].any(), (tag, k)
    report[tag] = {"fwd_xyz": fx, "fwd_rot": fr, **r}
    print(tag, {k: f"{v:.2e}" for k, v in report[tag].items()}, flush=True)
    # bit-identical re-run
    xyz2, rot2, g2 = _skin_hip(sc, graph, method, mode, gx, gr)
    assert np.array_equal(xyz, xyz2) and np.array_equal(rot, rot2) and all(np.array_equal(g[k], g2[k]) for k in g), tag
    return graph, gx, gr, s, og, g


def _judge(report):
    bad = {t: {k: f"{v:.2e}" for k, v in r.items()} for t, r in report.items()
           if max(r["fwd_xyz"], r["fwd_rot"]) > FWD_ATOL or max(v for k, v in r.items() if not k.startswith("fwd")) > ec.KERNEL_BOUND}
    worst = max(max(v for k, v in r.items() if not k.startswith("fwd")) for r in report.values())
    assert not bad, f"forward bar {FWD_ATOL}, gradient bar {ec.KERNEL_BOUND:.2e} (worst ratio here {worst:.2e}); over the bar: {bad}"


@pytest.mark.parametrize("mode", ec.MODES)
@pytest.mark.parametrize("which", ["all"] + ec.CLASSES)
def test_skin_vertices_at_branch_points(which, mode):
    """`which` = "all": every class in one call, K in {1, 2, 3, 4, 5, 8}, the K = 4 block edges, the hub graph; otherwise that
    class alone (K = 1 and 4), so a failure names its band.  Every method.  The failure message lists every case over the bar
    with its worst ratio per gradient."""
    _need_gpu()
    report = {}
    for label, sc in ec.skin_cases(which):
        for method in ec.METHODS:
            _skin_case(sc, label, method, mode, report)
    _judge(report)


@pytest.mark.parametrize("K", [2, 4])
def test_hybrid_clamp_equality_vertices_pass_the_gradient(K):
    """Two vertices with eta + 0.4f == 1 exactly (tests/skinning_edge_cases.py::clamp_equality_scene), in the generic (K = 2) and the
    DPP-quad (K = 4) backward, with the upstream gradient on those two vertices alone: dL/d(d_opacity) of their nodes is the
    x_lbs - x_dqs term that torch.clamp's backward passes at the bound."""
    _need_gpu()
    from dreammesh4d_amd import ops

    sc = ec.clamp_equality_scene(K)
    graph = ops.DeformGraph(sc["verts"], sc["nbr_idx"], sc["nbr_w"], sc["M"], torch.device("cuda:0"))
    gx, gr, keep = ec.skin_upstream(sc, "hybrid")
    assert keep[sc["eq_vertices"]].all()
    only = torch.zeros_like(gx)
    only[sc["eq_vertices"]] = gx[sc["eq_vertices"]]
    gr = torch.zeros_like(gr)
    s = ec.skin_row_scale(sc, only, gr)
    for mode in ec.MODES:
        _, _, og = ec.skin_reference(sc, "hybrid", mode, only, gr)
        _, _, g = _skin_hip(sc, graph, "hybrid", mode, only, gr)
        r = ec.skin_ratios(sc, "hybrid", g, og, s)
        print(f"clamp-eq/K{K}/{mode}", {k: f"{v:.2e}" for k, v in r.items()}, "d_opacity of nodes 0, 1: hip", g["do"][:2, 0], "float64", og["do"][:2, 0], flush=True)
        assert max(r.values()) <= ec.KERNEL_BOUND, (mode, r, g["do"][:2, 0], og["do"][:2, 0])


@pytest.mark.parametrize("mode", ec.MODES)
@pytest.mark.parametrize("K", [4, 5])
def test_skin_backward_with_one_upstream_gradient_absent(K, mode):
    """g_xyz only and g_rot only: the backward entry point is handed a null pointer for the other (autograd would hand it
    zeros), for both vertex kernels; the reference gets zeros."""
    dev = _need_gpu()
    from dreammesh4d_amd import ops

    sc = ec.skin_scene(ec.CLASSES, K, 700, seed=40 + K)
    graph = ops.DeformGraph(sc["verts"], sc["nbr_idx"], sc["nbr_w"], sc["M"], dev)
    report = {}
    for method in ec.METHODS:
        gx, gr, _ = ec.skin_upstream(sc, method)
        for absent in ("rot", "xyz"):
            hx, hr = (gx, None) if absent == "rot" else (None, gr)
            zx, zr = (gx, torch.zeros_like(gr)) if absent == "rot" else (torch.zeros_like(gx), gr)
            s = ec.skin_row_scale(sc, zx, zr)
            _, _, og = ec.skin_reference(sc, method, mode, zx, zr)
            names = ["dx", "dr"] + (["ds"] if method != "dqs" else []) + (["do"] if method == "hybrid" else [])
            t = {k: torch.tensor(sc[k], device=dev) for k in names}
            ctx = SimpleNamespace(graph=graph, method=ops.METHODS[method] | ops.GRAD_MODES[mode], saved_tensors=tuple(t[k] for k in names),
                                  has=("ds" in names, "do" in names), shapes=tuple(t[k].shape if k in names else None for k in ("dx", "dr", "ds", "do")))
            out = ops._SkinVertices.backward(ctx, None if hx is None else hx.to(dev), None if hr is None else hr.to(dev))[2:]
            g = {k: _np(o).reshape(sc["M"], -1) for k, o in zip(("dx", "dr", "ds", "do"), out) if o is not None}
            assert all(np.isfinite(v).all() for v in g.values())
            tag = f"K{K}/{method}/{mode}/no_g_{absent}"
            report[tag] = {"fwd_xyz": 0.0, "fwd_rot": 0.0, **ec.skin_ratios(sc, method, g, og, s)}
            print(tag, {k: f"{v:.2e}" for k, v in report[tag].items()}, flush=True)
    _judge(report)


def _face_hip(sc, topo, mode, gm, gq, gn):
    from dreammesh4d_amd import ops

    dev = topo.device
    x, r = torch.tensor(sc["vxyz"], device=dev).requires_grad_(True), torch.tensor(sc["vrot"], device=dev).requires_grad_(True)
    m, q, n = ops.face_gaussians(topo, x, r, torch.tensor(sc["qs"], device=dev), grad_mode=mode)
    torch.autograd.backward([m, q, n], [gm.to(dev), gq.to(dev), gn.to(dev)])
    return _np(m), _np(q), _np(n), _np(x.grad), _np(r.grad)


@pytest.mark.parametrize("mode", ec.MODES)
@pytest.mark.parametrize("which", ["all"] + ec.CLASSES)
def test_face_gaussians_at_branch_points(which, mode):
    """Vertex rotations from the magnitude classes (exact identity and w < 0 among them), G in {1, 3, 4, 6} ("all") or {1, 6}
    (a class alone), F * G not a multiple of a workgroup's faces, three zero-area faces: their normals are exactly the 0 of
    the clamped formula, their normal gradients are finite and stay on their own vertices."""
    dev = _need_gpu()
    from dreammesh4d_amd import ops

    report = {}
    for label, sc in ec.face_cases(which):
        G, F, V0 = sc["G"], sc["F"], sc["V0"]
        assert (F * G) % 256 and F % (256 // G)
        topo = ops.MeshTopology(sc["faces"], sc["V"], G, dev)
        gm, gq, gn = ec.face_upstream(sc)
        sx, sr = ec.face_row_scales(sc, gm, gq, gn)
        om, oq, on, ogx, ogr = ec.face_reference(sc, mode, gm, gq, gn)
        m, q, n, gx, gr = _face_hip(sc, topo, mode, gm, gq, gn)
        tag = f"{label}/{mode}"
        assert all(np.isfinite(a).all() for a in (m, q, n, gx, gr)), tag
        assert not n[-3 * G:].any() and not on[-3 * G:].any(), tag
        assert np.abs(m - om).max() < FWD_ATOL and np.abs(q - oq).max() < FWD_ATOL and np.abs(n - on).max() < 1e-5, \
            (tag, np.abs(m - om).max(), np.abs(q - oq).max(), np.abs(n - on).max())
        report[tag] = {"fwd_xyz": float(np.abs(m - om).max()), "fwd_rot": float(np.abs(q - oq).max()),
                       "vxyz": ec.worst_ratio(gx[:V0], ogx[:V0], sx[:V0]), "vrot": ec.worst_ratio(gr, ogr, sr)}
        print(tag, {k: f"{v:.2e}" for k, v in report[tag].items()}, flush=True)
        m2, q2, n2, gx2, gr2 = _face_hip(sc, topo, mode, gm, gq, gn)
        assert np.array_equal(gx, gx2) and np.array_equal(gr, gr2) and np.array_equal(q, q2), tag
    _judge(report)


@pytest.mark.parametrize("mode", ec.MODES)
def test_face_backward_with_upstream_gradients_absent(mode):
    """Means only, rotations only, normals only: null pointers for the others."""
    dev = _need_gpu()
    from dreammesh4d_amd import ops

    report = {}
    for G in (1, 6):
        sc = ec.face_scene(ec.CLASSES, G, seed=50 + G)
        V0 = sc["V0"]
        topo = ops.MeshTopology(sc["faces"], sc["V"], G, dev)
        ups = ec.face_upstream(sc)
        t = lambda a: torch.tensor(a, device=dev)
        ctx = SimpleNamespace(topo=topo, flags=ops.GRAD_MODES[mode], saved_tensors=(t(sc["vxyz"]), t(sc["vrot"]), t(sc["qs"])))
        for only in range(3):
            sel = [u if i == only else None for i, u in enumerate(ups)]
            sx, sr = ec.face_row_scales(sc, *sel)
            ref = ec.face_reference(sc, mode, *sel)
            out = ops._FaceGaussians.backward(ctx, *[None if u is None else u.to(dev) for u in sel])
            gx, gr = _np(out[1]), _np(out[2])
            assert np.isfinite(gx).all() and np.isfinite(gr).all()
            tag = f"G{G}/{mode}/only_{('means', 'rots', 'normals')[only]}"
            report[tag] = {"fwd_xyz": 0.0, "fwd_rot": 0.0, "vxyz": ec.worst_ratio(gx[:V0], ref[3][:V0], sx[:V0]), "vrot": ec.worst_ratio(gr, ref[4], sr)}
            print(tag, {k: f"{v:.2e}" for k, v in report[tag].items()}, flush=True)
    _judge(report)
