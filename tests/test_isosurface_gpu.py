"""Device tests of mesh extraction from Gaussians (csrc/isosurface.hip through dreammesh4d_amd/isosurface.py): the occupancy field
against the reference's own grids (tests/golden/gaussian_field.npz) and against the float64 restatement, marching cubes against
the numpy restatement bit for bit, and the pipeline end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from dreammesh4d_amd import isosurface as iso, wire_formats as wf
from tests import isosurface_common as ic

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS32 = 2.0 ** -24


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def field(g, rgb=None, **kw):
    return iso.gaussian_density_field(dev(g["xyz"]), dev(g["scaling"]), dev(g["rotation"]), dev(g["opacity"]), rgb=dev(rgb), **kw)


@pytest.fixture(scope="module")
def golden():
    return np.load(ic.GOLDEN)


# ------------------------------------------------------------------------------------------------------------- the field
@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_field_matches_the_reference_grids(golden, case):
    """max|hip - occ_f64| <= 4 * err_ref * max(occ_f64) + 1e-9, err_ref being the reference's own float32 error against the same
    functions run in float64 (it sits at 1 by construction; 4 covers another exp and another rounding of `power`)."""
    gc = ic.golden_case(golden, case)
    g = {k: gc[k] for k in ("xyz", "scaling", "rotation", "opacity")}
    nb = gc["num_blocks"]
    out = field(g, resolution=32, num_blocks=nb)
    occ = out["occ"].cpu().numpy()
    ref64, ref32, err_ref = gc["occ_f64"], gc["occ"], gc["err_ref"]
    err = float(np.abs(occ.astype(np.float64) - ref64).max())
    bound = 4 * err_ref * float(ref64.max()) + 1e-9
    print(f"case {case}: max|hip - occ_f64| = {err:.3e}, bound {bound:.3e} (err_ref {err_ref:.3e}, the reference's float32 grid: "
          f"{float(np.abs(ref32 - ref64).max()):.3e})")
    assert occ.dtype == np.float32 and occ.shape == (32, 32, 32) and out["csum"] is None
    assert np.array_equal(out["center"].cpu().numpy(), gc["center"]) and out["scale"] == gc["scale"]
    assert out["n_kept"] == 300
    assert err <= bound
    assert (ref32 == 0).sum() > 1000 and not occ[ref32 == 0].any()
    if case == "C":                                                   # the filtered Gaussians change nothing, bit for bit
        b = ic.golden_case(golden, "B")
        kept = g["opacity"] > np.float32(0.005)
        assert kept.sum() == 300 and len(kept) == 340 and sorted(map(tuple, g["xyz"][kept])) == sorted(map(tuple, b["xyz"]))
        only = {k: v[kept] for k, v in g.items()}
        assert np.array_equal(field(only, resolution=32, num_blocks=nb)["occ"].cpu().numpy(), occ)


def test_hard_cutoff_of_one_wide_gaussian():
    """One wide Gaussian (sigma 0.3 after normalisation, two tiny far ones fix the bounding box) at R = 32, num_blocks = 16:
    blocks whose window excludes its centre are exactly 0 although the Gaussian is far from 0 there; the others match the
    float64 restatement.  Bound: `power` is ~20 float32 operations on terms of its own size and w |power| <= 1 / e, the
    exponential is within 1.4 ulp and the inverse entries carry one rounding: 32 * 2^-24 * opacity covers them."""
    g = {"xyz": np.array([[0.1, -0.05, 0.02], [-1, -1, -1], [1, 1, 1]], np.float32),
         "scaling": np.array([[0.33, 0.3, 0.27], [1e-3] * 3, [1e-3] * 3], np.float32),
         "rotation": np.array([[0.9, 0.1, -0.3, 0.2], [1, 0, 0, 0], [1, 0, 0, 0]], np.float32),
         "opacity": np.array([0.8, 0.5, 0.5], np.float32)}
    ref = ic.field_reference(**g, resolution=32, num_blocks=16)
    out = field(g, resolution=32, num_blocks=16)
    occ = out["occ"].cpu().numpy()
    hit = np.repeat(np.repeat(np.repeat(ref["hit"], 2, 0), 2, 1), 2, 2)
    assert 20 < ref["hit"].sum() < 16 ** 3 / 2 and out["n_pairs"] == ref["n_pairs"] and out["scale"] == ref["scale"]
    wide = ref["hit"].copy()                                          # the blocks of the wide Gaussian: not those at the corners
    for ax in range(3):
        wide[tuple(slice(None) if a != ax else [0, 1, 2, 13, 14, 15] for a in range(3))] = False
    wide = np.repeat(np.repeat(np.repeat(wide, 2, 0), 2, 1), 2, 2)
    rim = wide & ~np.roll(wide, 2, 0) | wide & ~np.roll(wide, -2, 0)   # its outermost blocks along x: the cut is abrupt
    assert not occ[~hit].any() and wide.sum() >= 27 * 8 and ref["occ"][rim].min() > 0.05
    err = float(np.abs(occ.astype(np.float64) - ref["occ"]).max())
    print(f"cut-off: {int(ref['hit'].sum())} blocks hit, max error {err:.3e}, bound {32 * EPS32 * 0.8:.3e}")
    assert err <= 32 * EPS32 * 0.8


def test_centre_exactly_on_a_bound_is_excluded():
    """x is chosen so that the normalised centre equals vmax[5] in float32: block 5 is excluded on x (strict), block 6 is not."""
    coords, vmin, vmax = ic.block_bounds(32, 16)
    # bounding box [-1, 1]^3 by two tiny Gaussians: center 0, scale fl32(0.9), so x = vmax[5] / fl32(0.9) must round back exactly
    target = vmax[5]
    x = np.float32(target / np.float32(0.9))
    cand = [c for c in (np.nextafter(x, np.float32(-9)), x, np.nextafter(x, np.float32(9))) if np.float32(c * np.float32(0.9)) == target]
    assert cand, "no float32 x normalises onto the bound"
    g = {"xyz": np.array([[cand[0], 0.0, 0.0], [-1, -1, -1], [1, 1, 1]], np.float32),
         "scaling": np.array([[0.05] * 3, [1e-3] * 3, [1e-3] * 3], np.float32),
         "rotation": np.tile(np.array([1, 0, 0, 0], np.float32), (3, 1)), "opacity": np.array([0.9, 0.5, 0.5], np.float32)}
    ref = ic.field_reference(**g, resolution=32, num_blocks=16)
    assert ref["scale"] == 0.9 and np.float32((g["xyz"][0, 0] - ref["center"][0]) * np.float32(0.9)) == target
    assert not ref["hit"][5].any() and ref["hit"][6].any() and vmin[6] < target
    out = field(g, resolution=32, num_blocks=16)
    occ = out["occ"].cpu().numpy()
    assert out["n_pairs"] == ref["n_pairs"]
    mid = slice(14, 18)
    assert not occ[10:12, mid, mid].any() and occ[12:14, mid, mid].min() > 0     # block 5 (x index 10, 11) cut, block 6 not
    assert np.abs(occ - ref["occ"]).max() <= 32 * EPS32 * 0.9


def test_colour_sum():
    g = ic.random_gaussians(200, seed=7, sigma=(0.01, 0.02))
    colour = np.array([0.25, 0.5, 0.875], np.float32)
    out = field(g, rgb=np.tile(colour, (200, 1)), resolution=32, num_blocks=4)
    occ, csum = out["occ"].cpu().numpy().astype(np.float64), out["csum"].cpu().numpy().astype(np.float64)
    assert csum.shape == (32, 32, 32, 3) and out["csum"].dtype == torch.float32
    solid = occ > 1e-6
    assert solid.sum() > 1000 and np.abs(csum[solid] / occ[solid][:, None] - colour).max() <= 1e-6
    assert field(g, resolution=32, num_blocks=4)["csum"] is None
    assert np.array_equal(field(g, resolution=32, num_blocks=4)["occ"].cpu().numpy(), out["occ"].cpu().numpy())
    # varying colours against the float64 restatement
    ref = ic.field_reference(g["xyz"], g["scaling"], g["rotation"], g["opacity"], g["rgb"], resolution=32, num_blocks=4)
    got = field(g, rgb=g["rgb"], resolution=32, num_blocks=4)
    bound = 32 * EPS32 * float(ref["occ"].max())
    assert np.abs(got["csum"].cpu().numpy() - ref["csum"]).max() <= bound and np.abs(got["occ"].cpu().numpy() - ref["occ"]).max() <= bound


def test_two_runs_give_the_same_bytes_and_order_only_moves_the_last_bits():
    g = ic.random_gaussians(500, seed=11, sigma=(0.01, 0.02))
    a = field(g, rgb=g["rgb"], resolution=40, num_blocks=5)
    b = field(g, rgb=g["rgb"], resolution=40, num_blocks=5)
    assert torch.equal(a["occ"], b["occ"]) and torch.equal(a["csum"], b["csum"]) and a["n_pairs"] == b["n_pairs"]
    perm = np.random.default_rng(0).permutation(500)
    p = field({k: v[perm] for k, v in g.items()}, resolution=40, num_blocks=5)
    assert p["n_pairs"] == a["n_pairs"] and p["n_kept"] == a["n_kept"] and p["scale"] == a["scale"]
    # the float64 sum of <= 500 terms moves by <= 500 * 2^-53 relative: invisible after the rounding to float32 except where
    # the sum sits within that of a rounding boundary -- then by one float32 ulp
    occ_a, occ_p = a["occ"].cpu().numpy(), p["occ"].cpu().numpy()
    assert np.abs(occ_a.astype(np.float64) - occ_p).max() <= 2 * EPS32 * float(occ_a.max())
    assert (occ_a != occ_p).mean() < 1e-3


def test_chunked_blocks_and_partial_chunks():
    """s^3 > 512 (several workgroups per block) with a partial last chunk (s = 10: 1000 voxels) and s = 1 (one voxel per block)."""
    g = ic.random_gaussians(60, seed=13, sigma=(0.02, 0.04))
    for R, nb in ((20, 2), (12, 12)):
        ref = ic.field_reference(g["xyz"], g["scaling"], g["rotation"], g["opacity"], resolution=R, num_blocks=nb)
        out = field(g, resolution=R, num_blocks=nb)
        assert out["n_pairs"] == ref["n_pairs"]
        assert np.abs(out["occ"].cpu().numpy() - ref["occ"]).max() <= 32 * EPS32 * float(ref["occ"].max())


# ------------------------------------------------------------------------------------------------------- marching cubes
@pytest.mark.parametrize("name", ["random_sign", "noncubic", "on_threshold", "all_outside", "boundary"])
def test_marching_cubes_equals_the_restatement_bit_for_bit(name):
    f, threshold, csum = ic.mesh_fields()[name]
    ref = ic.marching_cubes_reference(f, threshold, csum)
    out = iso.marching_cubes(dev(f), threshold, dev(csum))
    verts, faces = out["verts"].cpu().numpy(), out["faces"].cpu().numpy()
    assert verts.dtype == np.float32 and faces.dtype == np.int64
    assert verts.shape == ref["verts"].shape and faces.shape == ref["faces"].shape
    assert verts.tobytes() == ref["verts"].tobytes() and np.array_equal(faces, ref["faces"])
    if csum is None:
        assert out["colors"] is None
    else:
        assert out["colors"].cpu().numpy().tobytes() == ref["colors"].tobytes()
    if name == "random_sign":
        assert ref["cases"] == set(range(256)) and ic.manifold_defects(faces) == (0, 0)
    if name == "on_threshold":
        assert (f == threshold).sum() > 50 and len(verts) > 100       # samples equal to the threshold are inside
    if name == "all_outside":
        assert len(verts) == 0 and len(faces) == 0
    if name == "boundary":
        assert len(faces) > 100 and ic.manifold_defects(faces)[0] == 0 and ic.manifold_defects(faces)[1] > 0    # open: border edges
    if len(verts):
        assert verts.min() >= 0 and (verts.max(0) <= np.array(f.shape) - 1).all()


# --------------------------------------------------------------------------------------------------------- end to end
def test_sphere_of_gaussians_end_to_end(tmp_path):
    g = ic.sphere_gaussians()
    mesh = iso.extract_mesh({k: dev(v) for k, v in g.items()}, density_thresh=0.8, resolution=64, num_blocks=16)
    v, f, c = mesh["verts"].cpu().numpy().astype(np.float64), mesh["faces"].cpu().numpy(), mesh["colors"].cpu().numpy()
    assert len(f) > 2000 and ic.manifold_defects(f) == (0, 0)
    lo, hi = g["xyz"].min(0), g["xyz"].max(0)
    assert (v >= lo - 0.1 * (hi - lo)).all() and (v <= hi + 0.1 * (hi - lo)).all()
    r = np.linalg.norm(v, axis=1)
    assert 0.3 < r.min() and r.max() < 0.7                             # a shell around the sphere of radius 0.5
    up, down = v[:, 2] > 0.35, v[:, 2] < -0.35
    assert up.sum() > 50 and down.sum() > 50
    assert np.abs(c[up] - np.array(ic.COLOR_UP)).max() <= 0.02 and np.abs(c[down] - np.array(ic.COLOR_DOWN)).max() <= 0.02

    # the same through the command line on a written .ply, then on into mesh_simplify
    n = len(g["xyz"])
    ply = str(tmp_path / "sphere.ply")
    logit = np.log(g["opacity"] / (1 - g["opacity"]))
    wf.write_gaussian_ply(ply, g["xyz"], (g["rgb"] - 0.5) / wf.SH_C0, np.zeros((n, 0)), logit, np.log(g["scaling"]), g["rotation"])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = subprocess.run([sys.executable, "-m", "dreammesh4d_amd.isosurface", "--ply", ply, "--resolution", "64", "--output",
                          str(tmp_path / "out")], cwd=root, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert f"{n} kept" in run.stdout and "vertices" in run.stdout and "pairs" in run.stdout
    back = wf.read_mesh(str(tmp_path / "out" / "sphere_mc.ply"))
    assert abs(len(back["verts"]) - len(v)) <= 0.02 * len(v) and ic.manifold_defects(back["faces"]) == (0, 0)
    assert back["colors"] is not None and np.abs(back["verts"] - v.mean(0)).max() < 0.7
    from dreammesh4d_amd.mesh_simplify import simplify_vertex_clustering

    res = simplify_vertex_clustering(dev(back["verts"].astype(np.float32)), dev(back["faces"]), dev(back["colors"].astype(np.float32)), scale=16)
    assert 8 < res["n_vertices"] < len(back["verts"]) and res["n_faces"] > 0


def test_extract_mesh_reads_a_geometry_object():
    """The object path: `get_*` as properties (the SuGaR classes) or as methods, colour from `get_points_rgb()` only when
    `sh_levels == 1` (absent counts as 1), against the dict path bit for bit."""
    import types

    g = {k: dev(v) for k, v in ic.sphere_gaussians(600).items()}
    kw = dict(density_thresh=0.3, resolution=32, num_blocks=8)
    ref = iso.extract_mesh(g, **kw)
    assert len(ref["faces"]) > 500 and ref["colors"] is not None
    props = dict(get_xyz=g["xyz"], get_scaling=g["scaling"], get_rotation=g["rotation"], get_opacity=g["opacity"][:, None],
                 get_points_rgb=lambda: g["rgb"])
    same = lambda a, b: all(torch.equal(a[k], b[k]) for k in ("verts", "faces"))
    for levels in (None, 1):
        obj = types.SimpleNamespace(**props) if levels is None else types.SimpleNamespace(sh_levels=levels, **props)
        out = iso.extract_mesh(obj, **kw)
        assert same(out, ref) and torch.equal(out["colors"], ref["colors"])
    out = iso.extract_mesh(types.SimpleNamespace(sh_levels=2, **props), **kw)
    assert same(out, ref) and out["colors"] is None
    methods = types.SimpleNamespace(sh_levels=1, **{k: (lambda v=v: v) for k, v in props.items() if k != "get_points_rgb"})
    out = iso.extract_mesh(methods, **kw)                              # no get_points_rgb at all: no colour
    assert same(out, ref) and out["colors"] is None
