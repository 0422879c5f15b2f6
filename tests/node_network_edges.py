"""Cases, a plain float64 reference and the error bounds of tests/test_node_network_edges_{cpu,gpu}.py (TEST INFRASTRUCTURE).

The node network (dreammesh4d_amd/csrc/hexplane.hip, deform_mlp.hip, nodenet.hip behind `DeformationNetwork.node_outputs`) is
judged element by element against `reference()` below: six planes per scale, bilinear sampling (align_corners=True, border
clamp), the product over the planes, the scales side by side, then Linear -> relu -> residual Linear -> Linear per head; the
gradients of every plane and every MLP parameter by float64 autograd through plain indexing (no F.grid_sample anywhere).

Only one thing is float32 in the reference: the lower texel index and the upper weight (i0, w1) of every coordinate, computed
with the arithmetic of `texel_coord` / `node_coords` of hexplane.hip (x_n = (p - lo) * inv - 1, 2 t - 1, ((x_n + 1) * 0.5) *
(n - 1), clamp, floor).  WHICH texel a query touches is then a fact the kernel and the reference share and not a rounding race;
everything behind (the four weights, the samples, the products, the MLP) is float64.  `coord_dtype=np.float64` moves that
step to float64 as well: the form in which the reference equals the module's own float64 CPU path to rounding (the CPU test).

Grid: base resolution (9, 9, 9, 5), bounds 1 -- n - 1 is a power of two on every axis of the coarsest scale, so its texels, the
five time rows and both borders of EVERY scale are exact float32 coordinates (the aabb is [[+1], [-1]]: x_n = -p).  Texels of
the scale with 18 = 2 * 9 texels are not exact; the "on_texel_fine" class searches float32 positions whose float32 arithmetic
lands on one (w1 == 0).

Bounds (measured, not guessed).  The yardstick of a tensor kind is the worst elementwise error of the torch float32 CPU path of
the same module against the reference over ALL cases below; a kernel may be off by 4 x that plus 4 * 2^-23 |ref| per element
(another fixed summation order: gather lists, 8 lane partials, the MFMA's K order -- not another algorithm).

ReLU rule.  A (frame, node) row in which some float64 ReLU input |h| is below the forward bound could take the other branch in
float32 on either side; such a row gets a ZERO upstream gradient (it is left out of the gradient comparison, never of the
forward one), and at most 2 % of a case's rows may be left out (checked on the CPU for every case).
"""
import functools
from collections import namedtuple

import numpy as np
import torch

from dreammesh4d_amd.deformation import PLANE_AXES, DeformationNetwork

# ---- yardsticks: worst |float32 CPU path - reference| over all CASES, per tensor kind, rounded up to two digits
#      (test_node_network_edges_cpu.py re-measures them and asserts that these constants still cover the float32 path) ----
YARD_OUT = 4.2e-8        # measured 4.19e-08   outputs dx / dr / ds / do                 (|out| up to 0.22)
YARD_SPATIAL = 4.3e-7    # measured 4.22e-07   gradients of the (x,y) (x,z) (y,z) planes (|grad| up to 0.57)
YARD_TIME = 2.3e-7       # measured 2.26e-07   gradients of the (x,t) (y,t) (z,t) planes (|grad| up to 0.22)
YARD_MLP = 1.7e-5        # measured 1.56e-05 with 1 CPU thread, 1.68e-05 with 8 and 16 (the sgemm splits its sums): W0, b0, heads (|grad| up to 127)
FACTOR = 4.0
RTOL = 4.0 * 2.0 ** -23
YARD = {"out": YARD_OUT, "spatial": YARD_SPATIAL, "time": YARD_TIME, "mlp": YARD_MLP}
RELU_MARGIN = FACTOR * YARD_OUT          # the forward bound's absolute term
MAX_EXCLUDED = 0.02                      # share of a case's rows the ReLU rule may leave out

RESOLUTION = (9, 9, 9, 5)
BOUNDS = 1.0
SPATIAL, TIME = (0, 1, 3), (2, 4, 5)
HEAD_MODULES = {"dx": "pos_deform", "dr": "rotations_deform", "ds": "scales_deform", "do": "opacity_deform"}
HEAD_DIMS = {"dx": 3, "dr": 4, "ds": 6, "do": 1}
MULTIRES = {64: (1, 2), 128: (1, 2, 4, 8), 192: (1, 2, 3, 4, 6, 8), 256: (1, 2, 3, 4, 5, 6, 7, 8)}     # by in_dim = 32 * len

Case = namedtuple("Case", "name multires heads layout nodes times seed")


def present_heads(heads):
    return ("dx", "dr", "ds", "do") if heads == "all" else ("dx", "dr")


def kind_of(name):
    """Tensor kind of a parameter name: "spatial", "time", "mlp", or None (timenet: never used by the query)."""
    if name.startswith("timenet"):
        return None
    if ".grid.grids." in name:
        return "spatial" if int(name.rsplit(".", 1)[1]) in SPATIAL else "time"
    return None if name.endswith("grid.aabb") else "mlp"


def bound(kind, ref):
    return FACTOR * YARD[kind] + RTOL * np.abs(ref)


# ------------------------------------------------------------------------------------------------ coordinates
def texel_coord(xn, n, f=np.float32):
    """hexplane.hip::texel_coord in dtype f: (index of the lower texel, weight of the upper one)."""
    xn = np.asarray(xn, f)
    ix = ((xn + f(1)) * f(0.5)) * f(n - 1)
    ix = np.minimum(f(n - 1), np.maximum(ix, f(0)))
    fl = np.floor(ix)
    return fl.astype(np.int64), (ix - fl).astype(f)


def query_coords(nodes, ts, f=np.float32):
    """hexplane.hip::node_coords for every (frame, node) row: [B * M, 4] normalised (x, y, z, t) in dtype f.  nodes [M, 3] and
    ts [B] (timestamps in [0, 1]) are float32 VALUES; 2 t - 1 is rounded in float32 for either f (the module is handed that)."""
    nodes, ts = np.asarray(nodes, np.float32), np.asarray(ts, np.float32)
    lo, hi = f(np.float32(BOUNDS)), f(np.float32(-BOUNDS))
    x = (nodes.astype(f) - lo) * (f(2) / (hi - lo)) - f(1)
    t = (ts * np.float32(2) - np.float32(1)).astype(f)
    B, M = len(ts), len(nodes)
    return np.concatenate([np.broadcast_to(x[None], (B, M, 3)), np.broadcast_to(t[:, None, None], (B, M, 1))], 2).reshape(B * M, 4)


# ------------------------------------------------------------------------------------------------ node classes
def _tex(k):          # position of texel k of the coarsest scale along an axis (x_n = -p, texel k at x_n = -1 + k / 4)
    return 1.0 - k / 4.0


def _on_texel_fine(rng, n):
    """float32 positions whose float32 arithmetic lands exactly on a texel of the 18-texel scale, on every axis."""
    good = []
    for k in range(1, 17):
        p0 = np.float32(1.0 - 2.0 * k / 17.0)
        for c in (p0, np.nextafter(p0, np.float32(2)), np.nextafter(p0, np.float32(-2))):
            i0, w1 = texel_coord((np.float32(c) - np.float32(1)) * np.float32(-1) - np.float32(1), 18)
            if w1 == 0 and i0 == k:
                good.append(c)
                break
    assert len(good) >= 8
    return rng.choice(np.asarray(good, np.float32), size=(n, 3))


def node_class(name, seed=0):
    """float32 [M, 3] node positions of one class."""
    rng = np.random.default_rng([seed, sum(map(ord, name))])
    U = lambda n: rng.uniform(-0.9, 0.9, size=(n, 3))
    if name == "interior":
        x = U(22)
    elif name in ("on_texel_1", "on_texel_2", "on_texel_3"):      # on a texel of the coarsest scale along 1, 2, 3 axes: w1 == 0 there
        k = int(name[-1])
        x = U(6 if k < 3 else 4)
        for i in range(len(x)):
            for a in rng.permutation(3)[:k]:
                x[i, a] = _tex(rng.integers(1, 8))
    elif name == "on_texel_fine":
        x = _on_texel_fine(rng, 6)
    elif name in ("border_lo", "border_hi"):                       # x_n = -1 (texel 0) / x_n = +1 (x1 == x0: two corners, one texel)
        v = 1.0 if name == "border_lo" else -1.0
        x = U(4)
        for a in range(3):
            x[a, a] = v
        x[3] = v                                                   # the box's corner
    elif name in ("outside_near", "outside_far"):
        x = U(6)
        for a in range(3):
            for j, sgn in enumerate((1.0, -1.0)):
                x[2 * a + j, a] = sgn * (1e6 if name == "outside_far" else (float(np.nextafter(np.float32(1), np.float32(2))), 1.01)[a % 2])
    elif name.startswith("cluster_"):                              # n nodes inside ONE cell of the coarsest scale
        n = int(name.split("_")[1])
        cell = {1: (0, 0, 0), 7: (7, 7, 7), 8: (2, 5, 3), 9: (5, 1, 6), 17: (3, 3, 1), 40: (6, 4, 4)}[n]
        x = np.stack([_tex(c) - rng.uniform(0.02, 0.98, size=n) / 4.0 for c in cell], 1)
    elif name == "identical":
        x = np.repeat(U(1), 2, 0)
    elif name == "single":
        x = U(1)
    elif name == "all":
        x = np.concatenate([node_class(c, seed) for c in NODE_CLASSES if c != "all"], 0)
    else:
        raise ValueError(name)
    return np.ascontiguousarray(x, np.float32)


NODE_CLASSES = ["interior", "on_texel_1", "on_texel_2", "on_texel_3", "on_texel_fine", "border_lo", "border_hi", "outside_near",
                "outside_far", "cluster_1", "cluster_7", "cluster_8", "cluster_9", "cluster_17", "cluster_40", "identical", "single", "all"]

TIME_SETS = {"t0": [0.0], "t1": [1.0], "t01": [0.0, 1.0],
             "rows": [0.0, 0.25, 0.5, 0.75, 1.0],                  # all five time rows exactly
             "repeat": [0.3, 0.7, 0.3],                             # two frames, one timestamp: their slots in s_rows merge
             "unsorted": [0.9, 0.1, 0.6, 0.35],
             "outside": [-0.1, 1.2],
             "b16": [0.0, 1.0, 0.5, 0.03, 0.97, 0.26, 0.24, 0.75, 0.61, 0.12, 0.44, 0.88, 0.33, 0.07, 0.69, 0.52],
             "b16eq": [0.4] * 16}


def timestamps(name):
    return np.asarray(TIME_SETS[name], np.float32)


def _cases():
    out = []
    layouts, heads = ("channels_last", "contiguous"), ("all", "pos+rot")
    tnames = list(TIME_SETS)
    # every node class, per layout (the timestamp sets rotate)
    for li, layout in enumerate(layouts):
        for i, nc in enumerate(NODE_CLASSES):
            out.append(Case(f"nodes-{nc}-{layout}", MULTIRES[64], heads[(i + li) % 2], layout, nc, tnames[(i + 3 * li) % len(tnames)], 10 + i))
    # every timestamp set on all node classes at once, per layout
    for li, layout in enumerate(layouts):
        for i, tn in enumerate(tnames):
            out.append(Case(f"times-{tn}-{layout}", MULTIRES[128] if li == 0 else MULTIRES[64], heads[(i + li + 1) % 2], layout, "all", tn, 40 + i))
    # every MLP input width with B = 16 and with one partial row tile (P < 16)
    for i, (in_dim, mr) in enumerate(MULTIRES.items()):
        out.append(Case(f"width-{in_dim}-B16", mr, heads[i % 2], layouts[i % 2], "all", "b16", 60 + i))
        out.append(Case(f"width-{in_dim}-P14", mr, heads[(i + 1) % 2], layouts[(i + 1) % 2], "cluster_7", "t01", 70 + i))
        out.append(Case(f"width-{in_dim}-P1", mr, heads[i % 2], layouts[i % 2], "single", "t1" if i % 2 else "t0", 80 + i))
    return out


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


# ------------------------------------------------------------------------------------------------ the module under test
def make_net(multires, heads, seed):
    """float32 CPU module with every parameter the query uses away from its initial value: the zero-initialised heads get
    weights, the time planes (all ones at initialisation: the features would not depend on t) get a random field."""
    full = heads == "all"
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        net = DeformationNetwork(resolution=RESOLUTION, bounds=BOUNDS, multires=tuple(multires), no_ds=not full, no_dr=False, no_do=not full)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if "_deform" in name:
                p.add_(0.05 * torch.randn(p.shape, generator=g))
            elif kind_of(name) == "time":
                p.copy_(0.6 + 0.8 * torch.rand(p.shape, generator=g))
    return net


def case_net(case):
    return make_net(case.multires, case.heads, case.seed)


def case_inputs(case):
    return node_class(case.nodes, case.seed), timestamps(case.times)


def used_parameters(net):
    """(name, parameter) of everything the query of this module reads: the planes, feature_out and the heads it has (a module
    built without the scales / opacity heads still owns their parameters; they never get a gradient)."""
    d = net.deformation_net
    absent = [HEAD_MODULES[k] for k, off in (("ds", d.no_ds), ("dr", d.no_dr), ("do", d.no_do)) if off]
    return [(n, p) for n, p in net.named_parameters() if kind_of(n) and not any(m in n for m in absent)]


def state64(net):
    """name -> float64 leaf for every parameter the query uses."""
    return {n: p.detach().double().contiguous().clone().requires_grad_(True) for n, p in used_parameters(net)}


def module_cpu(net, nodes, ts, upstream, dtype):
    """The module's own torch-op path on the CPU (F.grid_sample, nn.Linear) in `dtype`, through `forward_dynamic_delta` in float32;
    in float64 through the same layers in the same order, because forward_dynamic_delta casts the hidden layer `.float()`.
    -> (outputs name -> [B, M, k] float64 numpy, gradients name -> float64 numpy)."""
    import copy

    net = copy.deepcopy(net).to(dtype)
    net.zero_grad(set_to_none=True)
    B, M = len(ts), len(nodes)
    xn = query_coords(nodes, ts, np.float32)
    pts = torch.tensor(np.broadcast_to(np.asarray(nodes, np.float32)[None], (B, M, 3)).reshape(-1, 3).copy()).to(dtype)
    t = torch.tensor(xn[:, 3:4].copy()).to(dtype)
    d = net.deformation_net
    if dtype == torch.float32:
        dx, dr, ds, do = net.forward_dynamic_delta(pts, t)
    else:
        h = d.feature_out(d.grid(pts, t))
        dx, dr = d.pos_deform(h), d.rotations_deform(h)
        ds = None if d.no_ds else d.scales_deform(h)
        do = None if d.no_do else d.opacity_deform(h)
    outs = {k: v for k, v in zip(("dx", "dr", "ds", "do"), (dx, dr, ds, do)) if v is not None}
    loss = sum((outs[k] * torch.tensor(w).to(dtype).reshape(outs[k].shape)).sum() for k, w in upstream.items())
    loss.backward()
    grads = {n: (np.zeros(tuple(p.shape)) if p.grad is None else p.grad.double().numpy()) for n, p in used_parameters(net)}
    return {k: v.detach().double().numpy().reshape(B, M, -1) for k, v in outs.items()}, grads


# ------------------------------------------------------------------------------------------------ the reference
Ref = namedtuple("Ref", "outs grads touched touched_w h excluded upstream")


def _ref_forward(P, multires, xn, heads, f):
    """-> (outputs name -> [rows, k] float64 tensors, h [rows, 64], per plane name the four corner indices and weights)."""
    feats, corners = [], {}
    for s, mult in enumerate(multires):
        res = [RESOLUTION[0] * mult, RESOLUTION[1] * mult, RESOLUTION[2] * mult, RESOLUTION[3]]
        acc = None
        for p, (a0, a1) in enumerate(PLANE_AXES):
            name = f"deformation_net.grid.grids.{s}.{p}"
            W, H = res[a0], res[a1]
            plane = P[name]
            assert tuple(plane.shape) == (1, 32, H, W)
            flat = plane.reshape(32, H * W)
            x0, wx = texel_coord(xn[:, a0], W, f)
            y0, wy = texel_coord(xn[:, a1], H, f)
            x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)          # clamped duplicates carry weight 0
            wx, wy = wx.astype(np.float64), wy.astype(np.float64)
            idx = [y0 * W + x0, y0 * W + x1, y1 * W + x0, y1 * W + x1]
            wts = [(1 - wx) * (1 - wy), wx * (1 - wy), (1 - wx) * wy, wx * wy]
            v = sum(flat[:, torch.from_numpy(i)] * torch.from_numpy(w) for i, w in zip(idx, wts))      # [32, rows]
            acc = v if acc is None else acc * v
            corners[name] = (idx, wts, (H, W))
        feats.append(acc.t())
    feat = torch.cat(feats, 1)
    pre = "deformation_net."
    h = feat @ P[pre + "feature_out.0.weight"].t() + P[pre + "feature_out.0.bias"]
    x = torch.relu(h)
    outs = {}
    for k in present_heads(heads):
        m = pre + HEAD_MODULES[k] + ".feature_out."
        y = x + x @ P[m + "0.main_stream.weight"].t() + P[m + "0.main_stream.bias"]
        outs[k] = y @ P[m + "1.weight"].t() + P[m + "1.bias"]
    return outs, h, corners


def make_upstream(B, M, heads, seed, use=None):
    """name -> float32-valued [B, M, k] upstream gradients of the heads in `use` (default: all present ones)."""
    g = np.random.default_rng([seed, 7])
    up = {k: g.normal(size=(B, M, HEAD_DIMS[k])).astype(np.float32).astype(np.float64) for k in present_heads(heads)}
    return {k: v for k, v in up.items() if use is None or k in use}


def reference(net, multires, heads, nodes, ts, seed, use=None, coord_dtype=np.float32, relu_margin=None):
    """float64 outputs and gradients of the query of `nodes` [M, 3] at timestamps `ts` [B] for the loss
    sum_k <out_k, upstream_k> over the heads in `use`, the upstream rows zeroed by the ReLU rule."""
    B, M = len(ts), len(nodes)
    P = state64(net)
    xn = query_coords(nodes, ts, coord_dtype)
    outs, h, corners = _ref_forward(P, multires, xn, heads, coord_dtype)
    margin = RELU_MARGIN if relu_margin is None else relu_margin
    excluded = (h.detach().abs() < margin).any(1).numpy()
    upstream = make_upstream(B, M, heads, seed, use)
    for w in upstream.values():
        w.reshape(B * M, -1)[excluded] = 0.0
    loss = sum((outs[k] * torch.from_numpy(w.reshape(B * M, -1))).sum() for k, w in upstream.items())
    names = list(P)
    got = torch.autograd.grad(loss, [P[n] for n in names], allow_unused=True)
    grads = {n: (np.zeros(tuple(P[n].shape)) if g is None else g.numpy()) for n, g in zip(names, got)}
    active = ~excluded
    touched, touched_w = {}, {}
    for name, (idx, wts, (H, W)) in corners.items():
        t, tw = np.zeros(H * W, bool), np.zeros(H * W, bool)
        for i, w in zip(idx, wts):
            t[i] = True
            tw[i[(w != 0) & active]] = True
        touched[name], touched_w[name] = t.reshape(H, W), tw.reshape(H, W)
    return Ref({k: v.detach().numpy().reshape(B, M, -1) for k, v in outs.items()}, grads, touched, touched_w, h.detach().numpy(), excluded, upstream)


@functools.lru_cache(maxsize=None)
def case_reference(name, use=None):
    """The reference of a case, computed once per process and shared (callers must not modify it)."""
    case = CASE_BY_NAME[name]
    nodes, ts = case_inputs(case)
    return reference(case_net(case), case.multires, case.heads, nodes, ts, case.seed, use=use)


def float32_path_errors(case):
    """Worst elementwise |torch float32 CPU path - reference| of one case, per tensor kind (what the yardsticks are made of)."""
    ref = case_reference(case.name)
    nodes, ts = case_inputs(case)
    outs, grads = module_cpu(case_net(case), nodes, ts, ref.upstream, torch.float32)
    worst = {"out": max(float(np.abs(outs[k] - ref.outs[k]).max()) for k in ref.outs), "spatial": 0.0, "time": 0.0, "mlp": 0.0}
    for n, g in grads.items():
        worst[kind_of(n)] = max(worst[kind_of(n)], float(np.abs(g - ref.grads[n]).max()))
    return worst


def worst_ratio(kind, got, ref):
    """max over the elements of |got - ref| / bound (inf if `got` is not finite everywhere)."""
    got, ref = np.asarray(got, np.float64).reshape(np.shape(ref)), np.asarray(ref)
    return float((np.abs(got - ref) / bound(kind, ref)).max()) if np.isfinite(got).all() else float("inf")


def compare(kind, got, ref, what):
    """None, or a message naming the worst element of `got` against `ref` under the bound of `kind`."""
    got, ref = np.asarray(got, np.float64).reshape(np.shape(ref)), np.asarray(ref)
    if not np.isfinite(got).all():
        return f"{what}: non-finite values"
    err, bd = np.abs(got - ref), bound(kind, ref)
    ratio = err / bd
    if ratio.max() <= 1.0:
        return None
    i = np.unravel_index(int(ratio.argmax()), ratio.shape)
    return (f"{what}: {int((ratio > 1).sum())} of {ratio.size} elements off; worst at {tuple(int(j) for j in i)}: got {got[i]:.9g}, "
            f"float64 {ref[i]:.9g}, |diff| {err[i]:.3g} > bound {bd[i]:.3g} (yardstick {YARD[kind]:.3g} x {FACTOR:g})")
