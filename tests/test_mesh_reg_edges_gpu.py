"""GPU: the mesh regularisers (csrc/meshreg.hip: k_arap_*, k_nc_*, k_lap_*, k_quat_matrix_*) at their branch points, element by
element against the float64 reference of tests/mesh_reg_edges.py.

Cases: fans whose centre has valence 3, 7, 8, 9, 15, 16, 17, 33, 300 (every remainder of the 8-lane loop), open fans, isolated
vertices in the middle and at V - 1, a hand-built CSR with valence 1 and zero-weight reverse edges (ARAP, through the C ABI);
V = 1, 31, 32, 33 and P = 1, 255, 256, 257; T = 1, 2, 5 with a zero and a negative upstream weight; the rest pose (exact zeros),
deformations of 1e-4 of an edge, rotations that are not orthonormal; flat, folded, non-manifold, duplicated, zero-area and sliver
face pairs; a vertex at the centroid of its ring; unit and other quaternions.

Asserted per element: |hip - float64| <= 4 x yardstick x 2^-24 x scale, the yardstick being the worst error of the reference's
own float32 restatement in those units (tests/test_mesh_reg_edges_cpu.py re-measures it); exact zeros exactly; the optional
outputs, the two scratch forms and repeated calls bit-identical.  Every test prints its worst error / bound per tensor kind.

Argument checks: negative sizes and empty calls on every entry point; `T = 65536` on the ARAP entry points only, because only
they refuse it (`arap_check`).  The normal-consistency and Laplacian entry points hand T to the grid unchecked, where more than
65535 meshes end in a launch error of the runtime and not in DM4D_ERR_INVALID; that is not called here.
"""
import numpy as np
import pytest
import torch

from tests import mesh_reg_edges as ec

pytestmark = pytest.mark.gpu
BY_KIND = {k: [c.name for c in ec.CASES if c.kind == k] for k in ec.KINDS}


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


def _dev(a, dev, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=dev).contiguous()


# ------------------------------------------------------------------------------------------------ ARAP
def _arap_tables(case, dev):
    """(coach or None, device tensors off nbr rev w e) of a case: the coach's own, or the hand-built CSR."""
    from dreammesh4d_amd.mesh_reg import ARAPCoach

    tab = ec.host_tables(case.mesh)
    csr = tab["csr"]
    if case.mesh == "hand":
        return None, [_dev(a, dev, dt) for a, dt in zip(csr, (torch.int32,) * 3 + (torch.float32,) * 2)]
    coach = ARAPCoach(tab["verts"], tab["faces"], dev)
    E = len(csr.nbr)
    assert np.abs(coach._w.cpu().numpy()[:E] - csr.w).max(initial=0.0) <= 1e-4 * np.abs(csr.w).max(initial=0.0)
    coach._w[:E] = _dev(csr.w, dev, torch.float32)         # the cases' weights: the same bits on every host (mesh_reg_edges: INPUTS)
    mine = [coach._off, coach._nbr, coach._rev, coach._w, coach._e]
    for got, want in zip(mine, csr):                       # the tables the reference read are the tables the kernel reads
        assert np.array_equal(got.cpu().numpy()[:len(want)] if got.dim() == 1 else got.cpu().numpy()[:E], want)
    return coach, mine


@pytest.mark.parametrize("name", BY_KIND["arap"])
def test_arap_energy_and_gradients_element_by_element(name):
    dev = _need_gpu()
    from dreammesh4d_amd import _lib

    case, inp, ref = ec.CASE_BY_NAME[name], ec.case_inputs(name), ec.case_reference(name)
    coach, tables = _arap_tables(case, dev)
    T, V = inp["x"].shape[:2]
    x, R, g = _dev(inp["x"], dev, torch.float32), _dev(inp["R"], dev, torch.float32), _dev(inp["g"], dev, torch.float32)
    ptrs = [t.data_ptr() for t in tables]
    st = _lib.stream(dev)

    def backward(want_x, want_r):
        gx, gr = (_nan(dev, T, V, 3) if want_x else None), (_nan(dev, T, V, 3, 3) if want_r else None)
        _lib.call("dm4d_arap_energy_backward", T, V, *ptrs, x.data_ptr(), R.data_ptr(), g.data_ptr(), _lib.ptr(gx), _lib.ptr(gr), st)
        return gx, gr

    ev = _nan(dev, T, V)
    _lib.call("dm4d_arap_energy_forward", T, V, *ptrs, x.data_ptr(), R.data_ptr(), ev.data_ptr(), st)
    gx, gr = backward(True, True)
    _report(name, [("arap_energy", ev, ref["arap_energy"]), ("arap_g_xyz", gx, ref["arap_g_xyz"]), ("arap_g_rot", gr, ref["arap_g_rot"])])
    # each optional output alone, and a repeated call: the same bits
    assert _same_bits(backward(True, False)[0], gx) and _same_bits(backward(False, True)[1], gr)
    gx2, gr2 = backward(True, True)
    ev2 = _nan(dev, T, V)
    _lib.call("dm4d_arap_energy_forward", T, V, *ptrs, x.data_ptr(), R.data_ptr(), ev2.data_ptr(), st)
    assert _same_bits(gx2, gx) and _same_bits(gr2, gr) and _same_bits(ev2, ev)
    if "rest" in name:
        assert not ev.any() and not gx.any() and not gr.any()
    if coach is not None:                                   # the public class: the same kernels behind autograd
        xg, Rg = x.clone().requires_grad_(True), R.clone().requires_grad_(True)
        E = coach.compute_arap_energy(xg, Rg)
        assert _same_bits(E, ev.sum(dim=1))
        (E * g).sum().backward()
        assert _same_bits(xg.grad, gx) and _same_bits(Rg.grad, gr)
        xo = x.clone().requires_grad_(True)                 # needs_input_grad of the rotations off: g_rot is a null pointer
        (coach.compute_arap_energy(xo, R) * g).sum().backward()
        assert _same_bits(xo.grad, gx)


def test_arap_argument_checks_launch_nothing():
    dev = _need_gpu()
    from dreammesh4d_amd import _lib

    case = ec.CASE_BY_NAME["arap-fan33-T1"]
    inp = ec.case_inputs(case.name)
    _, tables = _arap_tables(case, dev)
    ptrs = [t.data_ptr() for t in tables]
    V = inp["x"].shape[1]
    x, R, g = _dev(inp["x"], dev, torch.float32), _dev(inp["R"], dev, torch.float32), _dev(inp["g"], dev, torch.float32)
    ev, gx, gr = _nan(dev, 1, V), _nan(dev, 1, V, 3), _nan(dev, 1, V, 3, 3)
    L, st = _lib.lib(), _lib.stream(dev)
    fwd = lambda T, V_: L.dm4d_arap_energy_forward(T, V_, *ptrs, x.data_ptr(), R.data_ptr(), ev.data_ptr(), st)
    bwd = lambda T, V_: L.dm4d_arap_energy_backward(T, V_, *ptrs, x.data_ptr(), R.data_ptr(), g.data_ptr(), gx.data_ptr(), gr.data_ptr(), st)
    for call in (fwd, bwd):
        assert call(65536, V) == _lib.DM4D_ERR_INVALID and b"65535" in L.dm4d_last_error()
        assert call(-1, V) == _lib.DM4D_ERR_INVALID and call(1, -1) == _lib.DM4D_ERR_INVALID
        assert call(0, V) == _lib.OK and call(1, 0) == _lib.OK
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (ev, gx, gr))
    assert fwd(1, V) == _lib.OK and bwd(1, V) == _lib.OK       # ... and the library is as usable as before
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in (ev, gx, gr))


# ------------------------------------------------------------------------------------------------ normal consistency
def _nc_on_device(name, dev):
    from dreammesh4d_amd.mesh_reg import MeshNormalConsistency

    case, inp = ec.CASE_BY_NAME[name], ec.case_inputs(name)
    tab = ec.host_tables(case.mesh)
    nc = MeshNormalConsistency(tab["faces"], len(tab["verts"]), dev)
    assert nc.n_pairs == len(tab["pairs"]) and np.array_equal(nc._pairs.cpu().numpy()[:nc.n_pairs], tab["pairs"])
    return nc, _dev(inp["x"], dev, torch.float32), _dev(inp["g"], dev, torch.float32)


def _nc_backward(nc, x, g, scratch):
    """g_xyz of the C ABI, into a buffer full of NaN: with the caller's scratch, or (scratch None) the library's own."""
    from dreammesh4d_amd import _lib

    T, V = int(x.shape[0]), nc.n_verts
    gx = _nan(x.device, T, V, 3)
    args = (T, V, nc.n_pairs, nc._pairs.data_ptr(), nc._off.data_ptr(), nc._items.data_ptr(), x.data_ptr(), g.data_ptr(), gx.data_ptr())
    if scratch is None:
        _lib.call("dm4d_normal_consistency_backward", *args, _lib.stream(x.device))
    else:
        _lib.call("dm4d_normal_consistency_backward_scratch", *args, scratch.data_ptr(), _lib.stream(x.device))
    return gx


@pytest.mark.parametrize("name", BY_KIND["nc"])
def test_normal_consistency_terms_and_gradient_element_by_element(name):
    dev = _need_gpu()
    from dreammesh4d_amd import _lib, mesh_reg

    ref = ec.case_reference(name)
    nc, x, g = _nc_on_device(name, dev)
    T, P = int(x.shape[0]), nc.n_pairs
    terms = _nan(dev, T, P)
    _lib.call("dm4d_normal_consistency_forward", T, nc.n_verts, P, nc._pairs.data_ptr(), x.data_ptr(), terms.data_ptr(), _lib.stream(dev))
    xg = x.clone().requires_grad_(True)
    loss = mesh_reg._NormalConsistency.apply(nc, xg)          # [T]: the mean over the pairs of every mesh
    assert _same_bits(loss, terms.sum(dim=1) / float(P))
    (loss * g).sum().backward()
    _report(name, [("nc_term", terms, ref["nc_term"]), ("nc_grad", xg.grad, ref["nc_grad"])])
    gx = _nc_backward(nc, x, g, _nan(dev, T, P, 12))
    assert _same_bits(gx, xg.grad) and _same_bits(_nc_backward(nc, x, g, _nan(dev, T, P, 12)), gx)
    assert abs(float(nc(x)) - float(ref["nc_term"].v.mean())) <= 1e-6          # the public call: mean over meshes and pairs
    if name == "nc-special-T2":
        pairs = nc._pairs.cpu().numpy()
        row = lambda what: int(np.flatnonzero((pairs == np.asarray(ec.SPECIAL[what])).all(1))[0])
        t = terms.cpu().numpy()
        assert (t[:, [row("zero_first"), row("zero_both")]] == 1.0).all() and (t[:, row("flat")] == 0.0).all()
        assert (t[:, row("folded")] == 2.0).all()
        assert bool(torch.isfinite(xg.grad).all()) and float(xg.grad[:, ec.SPECIAL["zero_first"][2]].abs().max()) > 1e7
        assert not xg.grad[:, ec.SPECIAL["no_pair"][0]].any()


def test_normal_consistency_library_scratch_grows_and_equals_the_callers():
    """`dm4d_normal_consistency_backward` owns its scratch: without pairs (nothing to allocate), with the smallest case, then
    with one that makes it grow -- unless an earlier test of the process already enlarged it: the growth depends on the order
    of the tests, the equality with the caller's scratch does not."""
    dev = _need_gpu()
    from dreammesh4d_amd.mesh_reg import MeshNormalConsistency

    none = MeshNormalConsistency(np.asarray([[0, 1, 2]]), 4, dev)
    assert none.n_pairs == 0
    gx = _nc_backward(none, torch.randn(2, 4, 3, device=dev), torch.tensor([1.0, -2.0], device=dev), None)
    assert gx.shape == (2, 4, 3) and not gx.any()
    for name in ("nc-strip1-T2", "nc-strip257-T2"):
        nc, x, g = _nc_on_device(name, dev)
        own = _nc_backward(nc, x, g, None)
        assert _same_bits(own, _nc_backward(nc, x, g, _nan(dev, int(x.shape[0]), nc.n_pairs, 12))), name
        _report(f"{name} library scratch", [("nc_grad", own, ec.case_reference(name)["nc_grad"])])


def test_normal_consistency_without_pairs_and_with_a_misaligned_scratch():
    dev = _need_gpu()
    from dreammesh4d_amd import _lib
    from dreammesh4d_amd.mesh_reg import MeshNormalConsistency

    # P == 0 (a single triangle): every vertex gets an exact zero
    nc = MeshNormalConsistency(np.asarray([[0, 1, 2]]), 4, dev)
    assert nc.n_pairs == 0
    x, g = torch.randn(2, 4, 3, device=dev), torch.tensor([1.0, -2.0], device=dev)
    gx = _nc_backward(nc, x, g, _nan(dev, 16))
    assert gx.shape == (2, 4, 3) and not gx.any()
    terms = _nan(dev, 2, 1)
    _lib.call("dm4d_normal_consistency_forward", 2, 4, 0, nc._pairs.data_ptr(), x.data_ptr(), terms.data_ptr(), _lib.stream(dev))
    torch.cuda.synchronize()
    assert bool(torch.isnan(terms).all())
    # a scratch that is not 16-byte aligned is refused before anything is launched; so are negative sizes
    nc, x, g = _nc_on_device("nc-strip1-T2", dev)
    T, V = int(x.shape[0]), nc.n_verts
    gx, scratch = _nan(dev, T, V, 3), _nan(dev, T * 12 + 4)
    L = _lib.lib()
    call = lambda T_, V_, P_, s: L.dm4d_normal_consistency_backward_scratch(T_, V_, P_, nc._pairs.data_ptr(), nc._off.data_ptr(), nc._items.data_ptr(),
                                                                             x.data_ptr(), g.data_ptr(), gx.data_ptr(), s, _lib.stream(dev))
    assert scratch.data_ptr() % 16 == 0
    assert call(T, V, 1, scratch.data_ptr() + 4) == _lib.DM4D_ERR_INVALID and b"16-byte" in L.dm4d_last_error()
    assert call(T, V, 1, None) == _lib.DM4D_ERR_INVALID
    assert call(-1, V, 1, scratch.data_ptr()) == call(T, -1, 1, scratch.data_ptr()) == call(T, V, -1, scratch.data_ptr()) == _lib.DM4D_ERR_INVALID
    assert call(0, V, 1, scratch.data_ptr()) == _lib.OK and call(T, 0, 1, scratch.data_ptr()) == _lib.OK
    torch.cuda.synchronize()
    assert bool(torch.isnan(gx).all()) and bool(torch.isnan(scratch).all())
    assert call(T, V, 1, scratch.data_ptr()) == _lib.OK
    _report("nc-strip1-T2 after the refusals", [("nc_grad", gx, ec.case_reference("nc-strip1-T2")["nc_grad"])])


# ------------------------------------------------------------------------------------------------ Laplacian
@pytest.mark.parametrize("name", BY_KIND["lap"])
def test_laplacian_terms_units_and_gradient_element_by_element(name):
    dev = _need_gpu()
    from dreammesh4d_amd import _lib, mesh_reg

    case, inp, ref = ec.CASE_BY_NAME[name], ec.case_inputs(name), ec.case_reference(name)
    tab = ec.host_tables(case.mesh)
    V = len(tab["verts"])
    ls = mesh_reg.MeshLaplacianSmoothing(tab["faces"], V, dev)
    assert np.array_equal(ls._off.cpu().numpy(), tab["lap_off"]) and np.array_equal(ls._nbr.cpu().numpy()[:len(tab["lap_nbr"])], tab["lap_nbr"])
    x, g = _dev(inp["x"], dev, torch.float32), _dev(inp["g"], dev, torch.float32)
    T = int(x.shape[0])
    terms, unit = _nan(dev, T, V), _nan(dev, T, V, 3)
    _lib.call("dm4d_laplacian_smoothing_forward", T, V, ls._off.data_ptr(), ls._nbr.data_ptr(), x.data_ptr(), terms.data_ptr(), unit.data_ptr(),
              _lib.stream(dev))
    xg = x.clone().requires_grad_(True)
    loss = mesh_reg._LaplacianSmoothing.apply(ls, xg)         # [T]: the mean over the vertices of every mesh
    assert _same_bits(loss, terms.sum(dim=1) / float(V))
    (loss * g).sum().backward()
    _report(name, [("lap_term", terms, ref["lap_term"]), ("lap_unit", unit, ref["lap_unit"]), ("lap_grad", xg.grad, ref["lap_grad"])])
    assert abs(float(ls(x)) - float(ref["lap_term"].v.mean())) <= 1e-6
    x2 = x.clone().requires_grad_(True)
    (mesh_reg._LaplacianSmoothing.apply(ls, x2) * g).sum().backward()
    assert _same_bits(x2.grad, xg.grad)
    zero = np.flatnonzero(np.diff(tab["lap_off"]) == 0).tolist() + ([0] if case.mesh == "square" else [])     # isolated, centroid
    assert case.mesh in ("fan-31", "fan-32", "fan-33") or zero
    assert not terms[:, zero].any() and not unit[:, zero].any()
    # argument checks that launch nothing
    L, junk = _lib.lib(), _nan(dev, T, V, 3)
    fwd = lambda T_, V_: L.dm4d_laplacian_smoothing_forward(T_, V_, ls._off.data_ptr(), ls._nbr.data_ptr(), x.data_ptr(), junk.data_ptr(), junk.data_ptr(), _lib.stream(dev))
    bwd = lambda T_, V_: L.dm4d_laplacian_smoothing_backward(T_, V_, ls._off.data_ptr(), ls._nbr.data_ptr(), unit.data_ptr(), g.data_ptr(), junk.data_ptr(), _lib.stream(dev))
    for call in (fwd, bwd):
        assert call(-1, V) == call(T, -1) == _lib.DM4D_ERR_INVALID and call(0, V) == call(T, 0) == _lib.OK
    torch.cuda.synchronize()
    assert bool(torch.isnan(junk).all())


# ------------------------------------------------------------------------------------------------ quaternions
@pytest.mark.parametrize("name", BY_KIND["quat"])
def test_quaternion_matrix_bitwise_and_its_backward_element_by_element(name):
    dev = _need_gpu()
    from dreammesh4d_amd import ops

    inp, ref = ec.case_inputs(name), ec.reference(name)
    q, G = torch.tensor(inp["q"]), torch.tensor(inp["G"])
    qd = q.to(dev).requires_grad_(True)
    Rd = ops.quat_xyzw_to_matrix(qd, "pypose")
    Rd.backward(G.to(dev))
    assert _same_bits(Rd.detach().cpu(), ops.quat_xyzw_to_matrix(q, "pypose"))     # the same float32 operations in the same order
    _report(name, [("quat_grad", qd.grad, ref["quat_grad"])])
    assert not qd.grad[:, 3].any()
