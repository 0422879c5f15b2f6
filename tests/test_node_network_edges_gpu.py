"""GPU: the node network (csrc/hexplane.hip + deform_mlp.hip, and the one-operator form csrc/nodenet.hip, through
`DeformationNetwork.node_outputs`) at its edges, element by element against the float64 reference of tests/node_network_edges.py.

Cases: every node class (interior; on a texel along 1, 2, 3 axes; on the lower / upper border; just outside and 1e6 outside the
box; 1, 7, 8, 9, 17, 40 nodes in one cell; two identical nodes; M = 1; all of them at once) and every timestamp set (t = 0, t = 1,
both, all five time rows, a repeated value, unsorted, outside [0, 1], 16 distinct, 16 equal) in both plane layouts; in_dim 64, 128,
192, 256 with B = 16 and with P = B M < 16; heads `all` and `pos+rot`.  Each case runs the fused operator and the two-operator path.

Asserted per element: |hip - float64| <= 4 x yardstick + 4 * 2^-23 |float64|, the yardstick being the worst error of the torch
float32 CPU path of the same module over the same cases (outputs 4.2e-8, spatial planes 4.3e-7, time planes 2.3e-7, MLP 1.7e-5;
tests/test_node_network_edges_cpu.py re-measures them); plane elements outside the reference's touched set exactly 0.0, also with
`grads_in_place` over two steps whose timestamps differ; heads without an upstream gradient; B = 17; nodes that move.

Measured on an MI355X, worst |error| / bound over all cases (1 = the bound; DESIGN.md "The node network at its edges"):
outputs 0.44 (all nodes at the five time rows), spatial planes 0.12, time planes 0.07, MLP 0.24 -- the same for the fused and the
two-operator path.  Before `build_plan` keyed its plan on the node tensor's version counter, the moved-nodes tests read
spatial 1.2e5, time 4.9e4 with correct outputs (new positions, old texel lists), and 1.8e5 on the outputs themselves for a
float64 node tensor replaced by another at the same address.
"""
import numpy as np
import pytest
import torch

from tests import node_network_edges as ec

pytestmark = pytest.mark.gpu
HEADS = ("dx", "dr", "ds", "do")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _device_net(cpu_net, layout, dev):
    import copy

    net = copy.deepcopy(cpu_net).to(dev)
    planes = [p for grid in net.deformation_net.grid.grids for p in grid]
    assert all(p.is_contiguous(memory_format=torch.channels_last) for p in planes)
    if layout == "contiguous":
        for p in planes:
            p.data = p.data.contiguous()
    return net


def _poison(net, dev):
    """The operators allocate their gradients uninitialised; leave NaN in freed blocks of those sizes, so that an element the
    kernels do not write reads as NaN and not as the zero of an earlier call."""
    for _ in range(2):
        junk = [torch.full((p.numel(),), float("nan"), device=dev) for n, p in ec.used_parameters(net)]
        del junk


def _run(net, nodes, ts, upstream):
    """One forward + backward of sum_k <out_k, upstream_k> -> (outputs, gradients) as float64 numpy in logical layout."""
    dev = ts.device
    out = net.node_outputs(nodes, ts)
    outs = {k: v for k, v in zip(HEADS, out) if v is not None}
    loss = sum((outs[k] * torch.tensor(w, dtype=torch.float32).to(dev).reshape(outs[k].shape)).sum() for k, w in upstream.items())
    _poison(net, dev)
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: (None if p.grad is None else p.grad.detach().cpu().double().numpy()) for n, p in ec.used_parameters(net)}
    B, M = int(ts.shape[0]), int(nodes.shape[0])
    return {k: v.detach().cpu().double().numpy().reshape(B, M, -1) for k, v in outs.items()}, grads


def _check(tag, outs, grads, ref):
    """Outputs, every gradient element and the exact zeros outside the touched set; prints the worst error / bound per kind."""
    msgs, worst = [], {k: 0.0 for k in ec.YARD}
    assert outs.keys() == ref.outs.keys(), tag
    for k in outs:
        worst["out"] = max(worst["out"], ec.worst_ratio("out", outs[k], ref.outs[k]))
        msgs.append(ec.compare("out", outs[k], ref.outs[k], f"{tag} output {k}"))
    assert grads.keys() == ref.grads.keys(), tag
    for n, g in grads.items():
        kind = ec.kind_of(n)
        if g is None:
            msgs.append(f"{tag} {n}: no gradient")
            continue
        worst[kind] = max(worst[kind], ec.worst_ratio(kind, g, ref.grads[n]))
        msgs.append(ec.compare(kind, g, ref.grads[n], f"{tag} gradient {n}"))
        if n in ref.touched:
            outside = g[0][:, ~ref.touched[n]]
            if not (outside == 0.0).all():           # (NaN included)
                msgs.append(f"{tag} gradient {n}: {int((outside != 0.0).sum())} elements outside the touched set are not exactly 0")
    print(f"{tag}: worst |error| / bound", {k: round(v, 4) for k, v in worst.items()})
    msgs = [m for m in msgs if m]
    assert not msgs, "\n".join(msgs)


def _case_on_device(name, dev):
    case = ec.CASE_BY_NAME[name]
    nodes, ts = ec.case_inputs(case)
    net = _device_net(ec.case_net(case), case.layout, dev)
    return case, net, torch.tensor(nodes).to(dev), torch.tensor(ts).to(dev)


@pytest.mark.parametrize("name", [c.name for c in ec.CASES])
def test_outputs_and_every_gradient_element_match_float64(name):
    dev = _need_gpu()
    case, net, nodes, ts = _case_on_device(name, dev)
    ref = ec.case_reference(name)
    for fuse in (True, False):
        net.fuse_node_network = fuse
        net.zero_grad(set_to_none=True)
        outs, grads = _run(net, nodes, ts, ref.upstream)
        _check(f"{name} {'fused' if fuse else 'two operators'}", outs, grads, ref)


@pytest.mark.parametrize("name", ["times-t1-contiguous", "times-t0-channels_last", "times-b16eq-channels_last", "times-repeat-contiguous",
                                  "width-256-P14", "width-192-P14"])
def test_in_place_gradient_planes_over_two_steps_with_other_timestamps(name):
    """`grads_in_place`: the persistent gradient planes keep their spatial texels and clear the time planes every step.  Step 1
    runs at other timestamps than step 2 (other time rows), step 2 must leave exact zeros in step 1's rows."""
    dev = _need_gpu()
    case, net, nodes, ts2 = _case_on_device(name, dev)
    ts1 = ec.timestamps("unsorted")
    ref1 = ec.reference(ec.case_net(case), case.multires, case.heads, nodes.cpu().numpy(), ts1, case.seed + 100)
    ref2 = ec.case_reference(name)
    assert any((ref1.touched[n] & ~ref2.touched[n]).any() for n in ref1.touched if ec.kind_of(n) == "time")
    net.grads_in_place = True
    planes = [p for grid in net.deformation_net.grid.grids for p in grid]
    for fuse in (True, False):
        net.fuse_node_network = fuse
        for step, (ts, ref) in enumerate(((torch.tensor(ts1).to(dev), ref1), (ts2, ref2))):
            net.zero_grad(set_to_none=True)
            outs, grads = _run(net, nodes, ts, ref.upstream)
            assert all(p.grad is b for p, b in zip(planes, net._hex_plan.grad_buffers))      # it really was the in-place path
            _check(f"{name} in place, {'fused' if fuse else 'two operators'}, step {step + 1}", outs, grads, ref)


@pytest.mark.parametrize("name,use", [("width-192-B16", ("dx",)), ("width-192-B16", ("ds",)), ("width-192-B16", ("do",)),
                                      ("width-64-P14", ("dx",)), ("width-128-P14", ("dr",)), ("nodes-cluster_17-channels_last", ("dr",))])
def test_heads_without_an_upstream_gradient(name, use):
    """A loss built from one head alone: the other heads' upstream gradients are None (null pointers in the C call); their
    parameters get exact zeros, everything else the float64 gradients."""
    dev = _need_gpu()
    case, net, nodes, ts = _case_on_device(name, dev)
    assert set(use) < set(ec.present_heads(case.heads))
    ref = ec.case_reference(name, use)
    assert ref.upstream.keys() == set(use)
    for fuse in (True, False):
        net.fuse_node_network = fuse
        net.zero_grad(set_to_none=True)
        outs, grads = _run(net, nodes, ts, ref.upstream)
        _check(f"{name} {'fused' if fuse else 'two operators'}, loss of {use[0]} alone", outs, grads, ref)
        for k in ec.present_heads(case.heads):
            if k not in use:
                mine = [n for n in grads if ec.HEAD_MODULES[k] in n]
                assert len(mine) == 4 and all(grads[n] is not None and not grads[n].any() and not ref.grads[n].any() for n in mine), k


def test_seventeen_frames_raise_the_library_error_naming_the_frame_limit():
    """kHexMaxFrames = 16: `node_outputs` leaves the fused operator for `hexplane_features`, whose C call refuses B = 17 in its
    argument check (before it launches anything) -- the caller sees Dm4dError with the limit in its message."""
    dev = _need_gpu()
    from dreammesh4d_amd._lib import Dm4dError

    case, net, nodes, _ = _case_on_device("nodes-interior-channels_last", dev)
    ts = torch.linspace(0, 1, 17).to(dev)
    for fuse in (True, False):
        net.fuse_node_network = fuse
        with pytest.raises(Dm4dError, match=r"dm4d_hexplane_forward failed.*B <= 16"):
            net.node_outputs(nodes, ts)
    torch.cuda.synchronize()
    assert all(p.grad is None for p in net.parameters())
    # and the network is as usable as before: 16 of the 17 frames
    ref = ec.reference(ec.case_net(case), case.multires, case.heads, nodes.cpu().numpy(), ts[:16].cpu().numpy(), case.seed)
    outs, grads = _run(net, nodes, ts[:16].contiguous(), ref.upstream)
    _check("16 frames after the refusal", outs, grads, ref)


def _moved_reference(case, nodes, ts):
    return ec.reference(ec.case_net(case), case.multires, case.heads, nodes, ts, case.seed)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("fuse", [True, False])
def test_nodes_moved_in_place_get_a_new_plan(fuse, in_place):
    """The plan (texel and column lists of the backward) belongs to node POSITIONS: after `nodes.copy_(...)` outputs and
    gradients are those of the new positions."""
    dev = _need_gpu()
    case, net, nodes, ts = _case_on_device("times-unsorted-channels_last", dev)
    net.fuse_node_network, net.grads_in_place = fuse, in_place
    first, second = ec.node_class("all", case.seed), ec.node_class("all", case.seed + 1)
    assert first.shape == second.shape and np.array_equal(first, nodes.cpu().numpy()) and not np.array_equal(first, second)
    for step, pos in enumerate((first, second)):
        if step:
            with torch.no_grad():
                nodes.copy_(torch.tensor(pos))
        ref = _moved_reference(case, pos, ts.cpu().numpy())
        net.zero_grad(set_to_none=True)
        outs, grads = _run(net, nodes, ts, ref.upstream)
        _check(f"nodes {'moved in place' if step else 'as built'}", outs, grads, ref)


@pytest.mark.parametrize("fuse", [True, False])
def test_node_tensors_the_plan_has_to_copy(fuse):
    """Node tensors that are not float32-contiguous (the plan holds a converted copy): a float64 tensor that is freed and
    replaced by another of the same length (the allocator may hand out the same address), and a strided float32 view whose
    base is overwritten."""
    dev = _need_gpu()
    case, net, _, ts = _case_on_device("times-repeat-contiguous", dev)
    net.fuse_node_network = fuse
    pos = [ec.node_class("all", case.seed + i) for i in range(4)]
    refs = [_moved_reference(case, p, ts.cpu().numpy()) for p in pos]

    def step(i, nodes, what):
        net.zero_grad(set_to_none=True)
        outs, grads = _run(net, nodes, ts, refs[i].upstream)
        _check(what, outs, grads, refs[i])

    n64 = torch.tensor(pos[0]).double().to(dev)
    step(0, n64, "float64 nodes")
    address = n64.data_ptr()
    del n64
    n64 = torch.tensor(pos[1]).double().to(dev)
    step(1, n64, f"another float64 tensor of the same length ({'the same' if n64.data_ptr() == address else 'another'} address)")
    base = torch.zeros(len(pos[2]), 4, device=dev)
    base[:, :3] = torch.tensor(pos[2]).to(dev)
    view = base[:, :3]
    assert not view.is_contiguous()
    step(2, view, "strided float32 view")
    base[:, :3] = torch.tensor(pos[3]).to(dev)
    step(3, base[:, :3], "the view's base overwritten")
