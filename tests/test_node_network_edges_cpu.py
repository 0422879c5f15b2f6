"""Pins the float64 reference and the bounds that tests/test_node_network_edges_gpu.py judges the node network by (CPU only).

* The reference (tests/node_network_edges.py: plain indexing, no F.grid_sample) against the module's own CPU path in float64
  (F.grid_sample + nn.Linear, pinned to the original by tests/test_deformation_golden.py), outputs and every gradient, on every
  case, with the coordinates in float64 on both sides: one function, 1e-12.  (With the kernels' float32 texel coordinates -- the
  form the GPU test uses -- only (i0, w1) change, by up to half an ulp of a texel index < 72, i.e. 4e-6 of a texel: more than the
  float32 arithmetic behind it costs, which is why the reference shares that step with the kernels.  That the float32 step is
  the module's is what the yardsticks show: the module's float32 path, which rounds its coordinates the same way, stays within
  4.2e-8 of this reference on every output.)
* The reference's touched set per plane is the support of its gradient, up to corners whose weight is exactly 0.
* The yardsticks (YARD_*) still cover the float32 CPU path on every case, and are not padded: the worst case reaches 80 % of each.
* The ReLU rule leaves out at most 2 % of the rows of every case.
"""
import numpy as np
import pytest
import torch

from tests import node_network_edges as ec

CASE_NAMES = [c.name for c in ec.CASES]


def test_case_list_covers_what_the_kernels_branch_on():
    for layout in ("channels_last", "contiguous"):
        mine = [c for c in ec.CASES if c.layout == layout]
        assert {c.nodes for c in mine} == set(ec.NODE_CLASSES)
        assert {c.times for c in mine} == set(ec.TIME_SETS)
    for in_dim, mr in ec.MULTIRES.items():
        assert in_dim == 32 * len(mr)
        shapes = [(len(ec.timestamps(c.times)), len(ec.node_class(c.nodes, c.seed))) for c in ec.CASES if c.multires == mr]
        assert any(B == 16 for B, M in shapes) and any(B * M < 16 for B, M in shapes)
    assert {c.heads for c in ec.CASES} == {"all", "pos+rot"}
    assert len(ec.node_class("all")) <= 150 and len(ec.node_class("single")) == 1
    a = ec.node_class("identical")
    assert len(a) == 2 and np.array_equal(a[0], a[1])
    # the classes are what their names say, in the kernels' own float32 arithmetic
    for name, want in (("border_lo", 0), ("border_hi", 8)):
        x = ec.query_coords(ec.node_class(name), [0.0])[:, :3]
        i0, w1 = ec.texel_coord(x, 9)
        assert ((i0 == want) & (w1 == 0)).any(1).all() and ((i0[3] == want) & (w1[3] == 0)).all()
    for k in (1, 2, 3):
        i0, w1 = ec.texel_coord(ec.query_coords(ec.node_class(f"on_texel_{k}"), [0.0])[:, :3], 9)
        assert ((w1 == 0).sum(1) >= k).all()
    i0, w1 = ec.texel_coord(ec.query_coords(ec.node_class("on_texel_fine"), [0.0])[:, :3], 18)
    assert (w1 == 0).all() and ((i0 > 0) & (i0 < 17)).all()
    for n in (1, 7, 8, 9, 17, 40):
        i0, _ = ec.texel_coord(ec.query_coords(ec.node_class(f"cluster_{n}"), [0.0])[:, :3], 9)
        assert len(i0) == n and (i0 == i0[0]).all()
    i0, w1 = ec.texel_coord(ec.query_coords(ec.node_class("interior")[:1], ec.timestamps("rows"))[:, 3], 5)
    assert i0.tolist() == [0, 1, 2, 3, 4] and not w1.any()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_reference_equals_the_float64_module(name):
    case = ec.CASE_BY_NAME[name]
    nodes, ts = ec.case_inputs(case)
    net = ec.case_net(case)
    # coordinates in float64 on both sides: the same function, to rounding
    r64 = ec.reference(net, case.multires, case.heads, nodes, ts, case.seed, coord_dtype=np.float64)
    outs, grads = ec.module_cpu(net, nodes, ts, r64.upstream, torch.float64)
    assert outs.keys() == r64.outs.keys() == set(ec.present_heads(case.heads))
    for k in outs:
        assert np.abs(outs[k] - r64.outs[k]).max() <= 1e-13 * max(1.0, np.abs(r64.outs[k]).max()), k
    assert grads.keys() == r64.grads.keys()
    for n, g in grads.items():
        assert np.abs(g - r64.grads[n]).max() <= 1e-12 * max(1.0, np.abs(g).max()), n


@pytest.mark.parametrize("name", CASE_NAMES)
def test_touched_set_is_the_support_of_the_gradient(name):
    ref = ec.case_reference(name)
    n_planes = 6 * len(ec.CASE_BY_NAME[name].multires)
    assert len(ref.touched) == n_planes
    for n, touched in ref.touched.items():
        support = (ref.grads[n][0] != 0).any(0)                   # [H, W]: some channel got gradient
        assert not (support & ~touched).any(), n
        assert np.array_equal(support, ref.touched_w[n]), n       # missing from the support: only corners of weight exactly 0
        assert not (ref.touched_w[n] & ~touched).any() and touched.any()


def test_relu_rule_leaves_out_at_most_two_percent_of_every_case():
    assert ec.RELU_MARGIN == ec.FACTOR * ec.YARD_OUT
    total = 0
    for c in ec.CASES:
        ref = ec.case_reference(c.name)
        total += int(ref.excluded.sum())
        assert ref.excluded.mean() <= ec.MAX_EXCLUDED, (c.name, int(ref.excluded.sum()), len(ref.excluded))
        for w in ref.upstream.values():
            w = w.reshape(len(ref.excluded), -1)
            assert not w[ref.excluded].any() and (w[~ref.excluded] != 0).all()
    assert total > 0      # the rule is exercised


def test_yardsticks_cover_the_float32_cpu_path():
    worst = {k: 0.0 for k in ec.YARD}
    for c in ec.CASES:
        for k, v in ec.float32_path_errors(c).items():
            worst[k] = max(worst[k], v)
    print("float32 CPU path, worst |error| per kind:", {k: f"{v:.3g}" for k, v in worst.items()})
    assert ec.YARD == {"out": ec.YARD_OUT, "spatial": ec.YARD_SPATIAL, "time": ec.YARD_TIME, "mlp": ec.YARD_MLP}
    for k, v in worst.items():
        assert 0.8 * ec.YARD[k] <= v <= ec.YARD[k], (k, v, ec.YARD[k])
