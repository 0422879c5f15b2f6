"""The backward tail of the batched `views` operators at the sizes where its two memory kernels can go wrong: the record gather
(csrc/raster_preprocess.hip gather_gaussian, inside k_gather_face_bwd / k_gather_bwd) and the vertex sum of the per-view corner
records (csrc/skinning.hip k_face_bwd_vertex).

Both kernels only add float32 numbers in a fixed order, so they are restated here in NumPy float32, addition by addition:

* the gather: a Gaussian's records [rec0, rec0 + rec_touched) are added in record order.  The renderer exposes the record buffer
  (its backward scratch), the per-view geometry workspace (rec_touched, rec0, conic_opacity: the layout of csrc/raster.h
  geom_layout is restated below and checked against the record counter) and, of the sums, dL/dmean2D on every path (the two
  moment sums through the conic, three roundings) and the raw colour / opacity sums wherever the per-view gradients are
  materialised (the two-kernel path and the learnable static appearance).  The conic and depth sums are not exposed unprocessed:
  they are covered by the comparison of the fused path with the two-kernel path.
* the vertex sum: eight lanes per vertex, lane c adds the corners c, c + 8, ... of the vertex for each view of the frame in view
  order, then lane ^ 1, lane ^ 2 and the other quad are added; the external vertex gradient comes last.  The position half of
  the vertex gradient is that sum itself; the rotation half goes through the Log's backward and is compared with the two-kernel
  path only.

Meshes: the first F faces of a 268-face UV sphere (67 meridians: the pole has valence 67 once F >= 67; a cut-open fan leaves
vertices of valence 1).  F = 41 / 42 / 43 / 85 x 6 Gaussians: one face short of a full workgroup of 252 live lanes, exactly one,
one over, and two workgroups with a partial tail."""
import math

import numpy as np
import pytest
import torch

from dreammesh4d_amd import synthetic as syn

pytestmark = pytest.mark.gpu

GREC = 128          # records per LDS window of a wave (csrc/raster_preprocess.hip DM4D_GREC; 32- and 48-byte records)
LANES = 252         # live lanes of a 256-thread workgroup with 6 Gaussians per face
SPHERE_FACES = 268  # 2 * 67 * (3 - 1): synthetic.uv_sphere picks 3 latitudes x 67 meridians
MODES = {"lean32": (8, (5, 6, 7)), "lean48": (12, (6, 7, 8)), "full64": (16, (7, 8, 9, 10, 11, 12))}     # floats per record, colour columns


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _geom_offsets(N, H, W):
    """Byte offsets of the arrays of a view's geometry workspace that the gather reads (csrc/raster.h geom_layout)."""
    T = ((W + 15) // 16) * ((H + 15) // 16)
    n = max(N, 1)
    sizes = [("counters", 256), ("tile_count", T * 4), ("tile_start", (T + 1) * 4), ("ccount", T * 64), ("cdone", T * 64), ("order", T * 4),
             ("longlist", T * 64), ("earlylist", T * 64), ("cflag", T * 64), ("xy", n * 8), ("depth", n * 4), ("conic_opacity", n * 16),
             ("rgb", n * 12), ("tiles_touched", n * 4), ("rec_touched", n * 4), ("rec0", n * 4)]
    off, o = {}, 0
    for name, b in sizes:
        off[name] = o
        o = (o + b + 255) // 256 * 256
    return off


_SCENES = {}


def _scene(F, dev):
    """Static part of the scene, built once per face count and left unchanged."""
    if F not in _SCENES:
        from dreammesh4d_amd import geometry as geo, ops

        M = 24
        sc = syn.mesh_bound_scene(SPHERE_FACES, n_nodes=M, k=4, seed=3)
        assert len(sc["faces"]) == SPHERE_FACES
        faces = sc["faces"][:F]
        N = 6 * F
        T = lambda a: torch.tensor(a, device=dev)
        graph = ops.DeformGraph(sc["verts"], sc["nbr_idx"], sc["nbr_w"], M, dev)
        topo = ops.MeshTopology(faces, len(sc["verts"]), 6, dev)
        verts, tf = T(sc["verts"]), T(faces)
        # the fan's slivers would make sub-pixel splats: four times the SuGaR initial size gives every Gaussian a few cells
        _SCENES[F] = dict(F=F, N=N, M=M, graph=graph, topo=topo, faces=faces, qs=geo.quaternions(verts, tf, T(sc["complex"][:N]), 6),
                          scales=geo.scaling(T(sc["log_scales"][:N] + np.float32(math.log(4.0))), syn.THICKNESS),
                          opac=geo.strengths(T(sc["densities"][:N])), rgb=geo.points_rgb(T(sc["sh_dc"][:N])))
    return _SCENES[F]


def _motion(M, n_frames, dev):
    _, motion = syn.node_motion(M, n_frames, seed=1)
    return {k: torch.stack([torch.tensor(m[k], device=dev) for m in motion]) for k in ("trans", "d_rot", "strain", "d_opacity")}


def _cams(H, W, specs):
    cams = [syn.make_camera(H, W, elev_deg=e, azim_deg=a, dist=d) for e, a, d in specs]
    dev = torch.device("cuda:0")
    return cams, torch.stack([torch.tensor(c.viewmatrix, device=dev) for c in cams]), torch.stack([torch.tensor(c.projmatrix, device=dev) for c in cams])


DEFAULT_CAMS = [(70.0, 10.0, 3.8), (50.0, 100.0, 2.2), (85.0, -60.0, 1.2), (30.0, 200.0, 3.0), (60.0, -150.0, 0.9), (75.0, 40.0, 1.6)]


def _view_geometry(r, B, N, H, W):
    """Per view: rec_touched, rec0, conic_opacity, record counter of the LAST forward of renderer `r`."""
    vs, ws = r.last
    geom = ws["geom"].view(B, -1).cpu().numpy()
    off = _geom_offsets(N, H, W)
    take = lambda b, name, dt, cnt: geom[b, off[name]:off[name] + cnt * np.dtype(dt).itemsize].copy().view(dt)
    out = []
    for b in range(B):
        g = dict(cnt=take(b, "rec_touched", np.uint32, N), rec0=take(b, "rec0", np.uint32, N),
                 conic=take(b, "conic_opacity", np.float32, 4 * N).reshape(N, 4), total=int(take(b, "counters", np.uint32, 4)[2]))
        out.append(g)
    return out


def _wave_ranges(g, radii):
    """Per wave of 64 consecutive Gaussians of a workgroup (252 live lanes each): records it streams, and whether one of its
    Gaussians' blocks straddles a window boundary."""
    N = len(radii)
    has = (radii > 0) & (g["cnt"] > 0)
    res = []
    for wg0 in range(0, N, LANES):
        for w0 in range(wg0, min(wg0 + LANES, N), 64):
            idx = np.arange(w0, min(w0 + 64, wg0 + LANES, N))
            idx = idx[has[idx]]
            if len(idx) == 0:
                res.append((0, False))
                continue
            r0 = g["rec0"][idx].astype(np.int64)
            r1 = r0 + g["cnt"][idx]
            R0 = r0.min()
            res.append((int(r1.max() - R0), bool((((r0 - R0) // GREC) != ((r1 - 1 - R0) // GREC)).any())))
    return res


def _run(sc, H, W, specs, fidx, mode, fuse, dev, want_m2=True, record_capacity=None, seed=0):
    """One forward + backward; returns everything the restatements need, on the host."""
    from dreammesh4d_amd import views

    cams, vm, pm = _cams(H, W, specs)
    B = len(specs)
    NF = B if fidx is None else int(max(fidx)) + 1
    r = views.ViewRenderer(sc["graph"], sc["topo"], H, W, cams[0].tanfov, method="hybrid")
    r.fuse_face_backward = fuse
    if record_capacity is not None:
        r.record_capacity, r.calibrated = record_capacity, True
    raw = _motion(sc["M"], NF, dev)
    leaves = {k: v.clone().requires_grad_(True) for k, v in raw.items()}
    static = mode == "full64"
    scales, opac, rgb = [t.clone().requires_grad_(static) for t in (sc["scales"], sc["opac"], sc["rgb"])]
    m2 = torch.zeros(B, sc["N"], 3, device=dev, requires_grad=True) if want_m2 else None
    tf = None if fidx is None else torch.tensor(fidx, device=dev, dtype=torch.int32)
    out = views.render_views(r, leaves["trans"], leaves["d_rot"], leaves["strain"], leaves["d_opacity"].squeeze(-1), sc["qs"], scales, opac,
                             rgb, vm, pm, torch.ones(6, device=dev), frame_index=tf, means2D=m2)
    gen = torch.Generator().manual_seed(seed)
    gC = torch.randn(B, 6, H, W, generator=gen).to(dev)
    gD = (0.1 * torch.randn(B, 1, H, W, generator=gen)).to(dev)
    gA = torch.randn(B, 1, H, W, generator=gen).to(dev)
    gV = (0.01 * torch.randn(NF, sc["graph"].V, 3, generator=gen)).to(dev)
    if mode == "lean32":
        torch.autograd.backward([out["color"], out["alpha"], out["vxyz"]], [gC, gA, gV])
    else:
        torch.autograd.backward([out["color"], out["depth"], out["alpha"], out["vxyz"]], [gC, gD, gA, gV])
    torch.cuda.synchronize()
    scr = next(iter(r._scratch.values()))
    cap = r.last[0].record_capacity
    recs = scr["grad"].view(B, -1).cpu().numpy().view(np.float32)[:, :cap * 16]
    lg = r.last_grads
    res = dict(r=r, B=B, NF=NF, radii=out["radii"].cpu().numpy(), geom=_view_geometry(r, B, sc["N"], H, W), cap=cap,
               recs=[recs[b, :cap * MODES[mode][0]].reshape(cap, MODES[mode][0]) for b in range(B)],
               corner=scr["face"].view(torch.float32).cpu().numpy(), gV=gV.cpu().numpy(), opac=opac.detach().cpu().numpy().reshape(-1),
               vx=lg["vx"].cpu().numpy(), vr=lg["vr"].cpu().numpy(), m2=None if m2 is None else m2.grad.cpu().numpy(),
               col=None if lg["col"] is None else lg["col"].cpu().numpy(), op=None if lg["op"] is None else lg["op"].cpu().numpy(),
               node={k: v.grad.cpu().numpy() for k, v in leaves.items()})
    return res


def _record_sums(res, b, cols):
    """float32 sums of the columns `cols` of every Gaussian's records of view b, in record order (zeros where the gather adds nothing)."""
    g, radii, rec = res["geom"][b], res["radii"][b], res["recs"][b]
    N = len(radii)
    has = (radii > 0) & (g["cnt"] > 0)
    rec0 = g["rec0"].astype(np.int64)
    end = np.minimum(rec0 + g["cnt"], np.maximum(rec0, res["cap"]))
    acc = np.zeros((N, len(cols)), np.float32)
    k = 0
    while True:
        m = has & (rec0 + k < end)
        if not m.any():
            break
        acc[m] = acc[m] + rec[np.ix_(rec0[m] + k, list(cols))]
        k += 1
    return acc


def _assert_gather_restated(res, mode, H, W):
    for b in range(res["B"]):
        g, radii = res["geom"][b], res["radii"][b]
        assert g["total"] == int(g["cnt"].sum()), "the restated workspace layout is off: record counter != sum of rec_touched"
        assert g["total"] <= res["cap"]
        mom = _record_sums(res, b, (0, 1))
        co = np.where((radii > 0)[:, None], g["conic"], np.float32(0)).astype(np.float32)
        want = np.zeros((len(radii), 3), np.float32)
        want[:, 0] = -(co[:, 0] * mom[:, 0] + co[:, 1] * mom[:, 1]) * np.float32(0.5 * W)
        want[:, 1] = -(co[:, 1] * mom[:, 0] + co[:, 2] * mom[:, 1]) * np.float32(0.5 * H)
        assert float(np.abs(want).max()) > 0
        assert np.array_equal(res["m2"][b].view(np.uint32), want.view(np.uint32)), (mode, b, "dL/dmean2D")
        if res["col"] is not None:
            cols = MODES[mode][1]
            s = _record_sums(res, b, cols)
            got = res["col"][b][:, 6 - len(cols):]
            assert float(np.abs(s).max()) > 0
            assert np.array_equal(got.view(np.uint32), s.view(np.uint32)), (mode, b, "colour sums")
        if res["op"] is not None:
            s = _record_sums(res, b, (5,))[:, 0]
            ok = (radii > 0) & (res["opac"] > 0)
            want_op = np.where(ok, s / np.where(ok, res["opac"], np.float32(1)), np.float32(0)).astype(np.float32)
            assert np.array_equal(res["op"][b].view(np.uint32), want_op.view(np.uint32)), (mode, b, "opacity sums")


def _assert_vertex_restated(res, sc, fidx):
    """vx == the eight-lane sum of the per-view corner records in the kernel's order + the external vertex gradient."""
    topo = sc["topo"]
    off, item = topo.csr_off.cpu().numpy().astype(np.int64), topo.csr_items.cpu().numpy().astype(np.int64)
    V, F, B = topo.V, sc["F"], res["B"]
    corner = res["corner"][:B * F * 18].reshape(B, F * 3, 6)
    val = off[1:] - off[:-1]
    for fr in range(res["NF"]):
        vb = [b for b in range(B) if (b if fidx is None else fidx[b]) == fr]
        a = np.zeros((8, V, 6), np.float32)
        for c in range(8):
            for b in vb:
                for k in range(int(val.max() + 7) // 8):
                    e = off[:-1] + c + 8 * k
                    m = e < off[1:]
                    if m.any():
                        a[c][m] = a[c][m] + corner[b][item[e[m]]]
        s1 = [a[c] + a[c ^ 1] for c in range(8)]
        s2 = [s1[c] + s1[c ^ 2] for c in range(8)]
        tot = s2[0] + s2[7]
        want = (tot[:, :3] + res["gV"][fr]).astype(np.float32)
        assert float(np.abs(tot).max()) > 0
        assert np.array_equal(res["vx"][fr].view(np.uint32), want.view(np.uint32)), ("vertex sum", fr)


def _assert_fused_equals_unfused(fu, un, shared):
    for k in ("vx", "vr"):
        a, b = fu[k], un[k]
        assert float(np.abs(b).max()) > 0, k
        if shared:      # the views of a frame are added in another place: tests/test_views_gpu.py's bound for this pair
            assert float(np.abs(a - b).max()) <= 2e-6 * float(np.abs(b).max()), (k, float(np.abs(a - b).max()), float(np.abs(b).max()))
        else:
            assert np.array_equal(a, b), k
    for k in fu["node"]:
        a, b = fu["node"][k], un["node"][k]
        if shared:
            assert float(np.abs(a - b).max()) <= 2e-6 * float(np.abs(b).max()), k
        else:
            assert np.array_equal(a, b), k
    assert np.array_equal(fu["m2"], un["m2"])


@pytest.mark.parametrize("mode", ["lean32", "lean48", "full64"])
@pytest.mark.parametrize("F,H,W", [(41, 64, 64), (42, 64, 64), (43, 128, 128), (85, 64, 64), (85, 128, 128)])
def test_two_frames_three_views_restated_in_float32(F, H, W, mode):
    _need_gpu()
    dev = torch.device("cuda:0")
    sc = _scene(F, dev)
    fidx = [0, 1, 1, 0, 1, 0]
    un = _run(sc, H, W, DEFAULT_CAMS, fidx, mode, False, dev)
    _assert_gather_restated(un, mode, H, W)
    if mode == "full64":
        return      # a learnable static appearance materialises the per-view gradients: the two-kernel path whatever `fuse` says
    fu = _run(sc, H, W, DEFAULT_CAMS, fidx, mode, True, dev)
    assert fu["col"] is None
    _assert_gather_restated(fu, mode, H, W)
    _assert_vertex_restated(fu, sc, fidx)
    _assert_fused_equals_unfused(fu, un, True)


@pytest.mark.parametrize("mode", ["lean32", "lean48", "full64"])
@pytest.mark.parametrize("F", [41, 85])
def test_one_frame_one_view_without_frame_index(F, mode):
    _need_gpu()
    dev = torch.device("cuda:0")
    sc = _scene(F, dev)
    un = _run(sc, 64, 64, DEFAULT_CAMS[1:2], None, mode, False, dev)
    _assert_gather_restated(un, mode, 64, 64)
    if mode == "full64":
        return
    fu = _run(sc, 64, 64, DEFAULT_CAMS[1:2], None, mode, True, dev)
    _assert_gather_restated(fu, mode, 64, 64)
    _assert_vertex_restated(fu, sc, None)
    _assert_fused_equals_unfused(fu, un, False)


def test_mesh_has_a_vertex_of_valence_1_and_a_pole_of_at_least_65():
    _need_gpu()
    sc = _scene(85, torch.device("cuda:0"))
    off = sc["topo"].csr_off.cpu().numpy()
    val = off[1:] - off[:-1]
    assert (val == 1).any() and val.max() >= 65, sorted(set(val.tolist()))


def test_every_length_of_a_wave_s_record_range_occurs_and_is_restated():
    """Cameras are searched (one forward over a sweep of distances and elevations) for waves whose record range is empty (every
    Gaussian culled), shorter than a window, exactly one window, one window + 1 and longer than three windows, and for a Gaussian
    whose block straddles a window boundary; the views found are then run through the fused backward and restated."""
    _need_gpu()
    from dreammesh4d_amd import views

    dev = torch.device("cuda:0")
    F, H, W = 85, 64, 64
    sc = _scene(F, dev)
    sweep = [(e, 25.0 * i, 0.75 + 0.0125 * i) for e in (80.0, 55.0) for i in range(260)]
    cases = {"empty": lambda n: n == 0, "short": lambda n: 0 < n < GREC, "one window": lambda n: n == GREC,
             "one window + 1": lambda n: n == GREC + 1, "more than three windows": lambda n: n > 3 * GREC}
    found, straddle = {}, None
    for s0 in range(0, len(sweep), 52):
        specs = sweep[s0:s0 + 52]
        cams, vm, pm = _cams(H, W, specs)
        B = len(specs)
        r = views.ViewRenderer(sc["graph"], sc["topo"], H, W, cams[0].tanfov, method="hybrid")
        raw = _motion(sc["M"], 1, dev)
        out = views.render_views(r, raw["trans"], raw["d_rot"], raw["strain"], raw["d_opacity"].squeeze(-1), sc["qs"], sc["scales"], sc["opac"],
                                 sc["rgb"], vm, pm, torch.ones(6, device=dev), frame_index=torch.zeros(B, device=dev, dtype=torch.int32))
        radii = out["radii"].cpu().numpy()
        for b, g in enumerate(_view_geometry(r, B, sc["N"], H, W)):
            waves = _wave_ranges(g, radii[b])
            for name, hit in cases.items():
                if name not in found and any(hit(n) for n, _ in waves):
                    found[name] = specs[b]
            if straddle is None and any(st for _, st in waves):
                straddle = specs[b]
        if len(found) == len(cases) and straddle is not None:
            break
    assert sorted(found) == sorted(cases) and straddle is not None, f"no camera of the sweep gives: {sorted(set(cases) - set(found))}, straddle {straddle}"
    specs = list(dict.fromkeys(list(found.values()) + [straddle]))
    fidx = [0] * len(specs)      # one frame, as in the sweep: the same node motion, so the same records
    for mode in ("lean32", "lean48"):
        fu = _run(sc, H, W, specs, fidx, mode, True, dev)
        seen = [n for b in range(fu["B"]) for n, _ in _wave_ranges(fu["geom"][b], fu["radii"][b])]
        for name, hit in cases.items():
            assert any(hit(n) for n in seen), (name, sorted(seen))
        assert any(st for b in range(fu["B"]) for _, st in _wave_ranges(fu["geom"][b], fu["radii"][b]))
        _assert_gather_restated(fu, mode, H, W)
        _assert_vertex_restated(fu, sc, fidx)
        un = _run(sc, H, W, specs, fidx, mode, False, dev)
        _assert_gather_restated(un, mode, H, W)
        _assert_fused_equals_unfused(fu, un, True)


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("mode", ["lean32", "lean48", "full64"])
def test_record_capacity_below_the_need_reports_overflow_and_does_not_fault(mode, fuse):
    """The operator's record capacity argument set below the records of the views: the backward's gather clamps every range to the
    capacity (`end = min(rec0 + cnt, max(rec0, rec_cap))`), the call returns, and check() reports the overflow and raises the capacity."""
    _need_gpu()
    from dreammesh4d_amd import _lib

    dev = torch.device("cuda:0")
    sc = _scene(85, dev)
    fidx = [0, 1, 1]
    full = _run(sc, 64, 64, DEFAULT_CAMS[:3], fidx, mode, fuse, dev)
    need = [g["total"] for g in full["geom"]]
    cap = min(need) // 2 + 37          # inside a wave's range in every view
    assert 0 < cap < min(need)
    res = _run(sc, 64, 64, DEFAULT_CAMS[:3], fidx, mode, fuse, dev, record_capacity=cap)
    r = res["r"]
    assert r.last[0].record_capacity == cap
    with pytest.raises(_lib.Dm4dError):
        r.check()
    assert r.record_capacity >= max(need)
    assert [g["total"] for g in res["geom"]] == need      # the records are counted exactly even when they overflow
