"""CPU-side tests of mesh extraction from Gaussians: the generated marching-cubes table and the meshes the numpy restatement
(tests/isosurface_common.py) draws with it, the new header and its binding, the operator's refusals (no device is touched) and
the Gaussian PLY layout."""
import os

import numpy as np
import pytest
import torch

from dreammesh4d_amd import _lib, isosurface as iso, wire_formats as wf
from tests import isosurface_common as ic

GEN = ic.GEN


# ------------------------------------------------------------------------------------------------------------- the table
def test_regenerating_the_table_reproduces_the_committed_header():
    with open(GEN.HEADER_PATH) as fh:
        assert fh.read() == GEN.render_header()
    assert GEN.main(["--check"]) == 0


def test_every_case_uses_every_crossed_edge_in_closed_loops():
    count, tris, max_tris = GEN.build_table()
    assert max_tris == 5 and count.max() == 5 and count[0] == 0 and count[255] == 0          # the header's DM4D_MC_MAX_TRIS
    with open(GEN.HEADER_PATH) as fh:
        assert "#define DM4D_MC_MAX_TRIS 5\n" in fh.read()
    moved = 0
    for case in range(256):
        crossed = {e for e in range(12) if (case >> GEN.edge_corners(e)[0] & 1) != (case >> GEN.edge_corners(e)[1] & 1)}
        loops = GEN.case_loops(case)                                  # asserts: one segment in, one out per crossed edge; closed
        assert sorted(e for l in loops for e in l) == sorted(crossed), case
        assert all(len(l) >= 3 and l[0] == min(l) for l in loops) and [l[0] for l in loops] == sorted(l[0] for l in loops)
        t = [tuple(x) for x in tris[case, :count[case]]]
        assert count[case] == sum(len(l) - 2 for l in loops) <= 5 and {e for tri in t for e in tri} == crossed
        assert (tris[case, count[case]:] == -1).all()
        # within the cube every directed loop edge is used once: fans add interior diagonals in both directions
        d = [(tri[a], tri[(a + 1) % 3]) for tri in t for a in range(3)]
        assert len(set(d)) == len(d)
        loop_edges = {(l[a], l[(a + 1) % len(l)]) for l in loops for a in range(len(l))}
        assert {e for e in d if (e[1], e[0]) not in d} == loop_edges, case
        # a diagonal never lies in a cube face (the neighbouring cube could draw it too: four triangles on one edge); the fan
        # starts at the loop's smallest edge unless that fan has such a diagonal
        assert all(not (GEN.EDGE_FACES[a] & GEN.EDGE_FACES[b]) for a, b in d if (a, b) not in loop_edges), case
        first = [tri[0] for tri in t]
        moved += sum(GEN.fan_apex(l) != 0 for l in loops)
        assert all(l[GEN.fan_apex(l)] in first for l in loops)
    assert moved == 18


def test_ambiguous_faces_separate_the_inside_corners():
    """Corners 0 and 3 (offsets (0,0,0) and (0,1,1)) are the inside diagonal of the face i = 0: two triangles, none joining them;
    the complement joins the OUTSIDE corners instead (one loop around both)."""
    assert len(GEN.case_loops(0b00001001)) == 2 and len(GEN.case_loops(0b11110110)) == 1
    assert len(GEN.case_loops(0b01101001)) == 4                       # four inside corners, no two adjacent: four triangles


@pytest.fixture(scope="module")
def random_mesh():
    f, csum = ic.random_sign_field()
    return f, csum, ic.marching_cubes_reference(f, 0.0, csum)


def test_random_sign_field_gives_a_closed_oriented_manifold_and_all_cases(random_mesh):
    f, _, m = random_mesh
    assert m["cases"] == set(range(256))
    assert ic.manifold_defects(m["faces"]) == (0, 0)
    assert len(m["verts"]) == len(np.unique(m["verts"], axis=0)) and m["faces"].max() == len(m["verts"]) - 1      # welded, all used
    inside = f.astype(np.float64) >= 0.0
    crossed = sum(int((np.diff(inside.astype(np.int8), axis=a) != 0).sum()) for a in range(3))
    assert len(m["verts"]) == crossed


def test_sphere_mesh_is_a_sphere_with_outward_normals():
    f = ic.sphere_field(24)
    m = ic.marching_cubes_reference(f, 0.0)
    v, fc = m["verts"].astype(np.float64), m["faces"]
    assert ic.manifold_defects(fc) == (0, 0) and ic.euler_characteristic(len(v), fc) == 2
    n = np.cross(v[fc[:, 1]] - v[fc[:, 0]], v[fc[:, 2]] - v[fc[:, 0]])
    area = np.linalg.norm(n, axis=1) / 2
    big = area > 1e-4 * area.mean()
    assert (~big).mean() <= 0.01
    centre = v[fc].mean(1) / (24 - 1) * 2 - 1                          # grad f = -p / |p|
    assert ((n * -centre).sum(1)[big] < 0).all()
    r = np.linalg.norm(v / 23 * 2 - 1, axis=1)
    assert np.abs(r - 0.6).max() < 0.01                                # linear interpolation of a distance field


def test_vertex_and_face_order_follow_the_rule(random_mesh):
    """Vertex ids ascend with 3 * voxel + axis (recovered from the positions); faces ascend with their cube's voxel index."""
    f, _, m = random_mesh
    v = m["verts"].astype(np.float64)
    base = np.floor(v).astype(np.int64)
    frac = v - base
    axis = np.argmax(frac > 0, axis=1)                                 # t in (0, 1]: t == 1 only when f_b == threshold, absent here
    assert ((frac > 0).sum(1) == 1).all()
    key = 3 * ((base[:, 0] * f.shape[1] + base[:, 1]) * f.shape[2] + base[:, 2]) + axis
    assert (np.diff(key) > 0).all()
    cube = np.floor(v[m["faces"]].min(1)).astype(np.int64)
    lin = (cube[:, 0] * f.shape[1] + cube[:, 1]) * f.shape[2] + cube[:, 2]
    assert (np.diff(lin) >= 0).all()


# ------------------------------------------------------------------------------------------------------- header, binding
def test_new_header_parses_and_the_library_exports_it():
    names = _lib.declared_symbols("iso")
    assert names == sorted(_lib._PARSED["iso"][2]) and len(names) == 7 and all(n.startswith("dm4d_iso_") for n in names)
    L = _lib.lib()
    for n in names:
        assert hasattr(L, n), n
    assert L.dm4d_iso_version() == _lib.abi_version("iso") == _lib._PARSED["iso"][0]["DM4D_ISO_ABI_VERSION"] == 1
    assert len(_lib._SIGNATURES) == 127 and not set(names) & set(_lib._SIGNATURES) and _lib.abi_version() == 107
    assert _lib._PARSED["iso"][1] == {}


def test_entry_points_validate_before_any_launch():
    import ctypes as C

    L = _lib.lib()
    p = C.cast((C.c_double * 64)(), C.c_void_p)
    assert L.dm4d_iso_density_field(4, 4, 1, 1, p, p, p, p, p, None, None) == -1 and b"resolution" in L.dm4d_last_error()
    assert L.dm4d_iso_density_field(4, 4, 513, 1, p, p, p, p, p, None, None) == -1
    assert L.dm4d_iso_density_field(4, 4, 32, 5, p, p, p, p, p, None, None) == -1
    assert L.dm4d_iso_density_field(4, 4, 32, 4, p, None, p, p, p, None, None) == -1 and b"null" in L.dm4d_last_error()
    assert L.dm4d_iso_gaussian_records(-1, p, p, p, p, None, 4, p, p, p, p, p, None) == -1
    assert L.dm4d_iso_gaussian_records(4, p, p, p, p, None, 0, p, p, p, p, p, None) == -1
    assert L.dm4d_iso_gaussian_records(0, None, None, None, None, None, 4, None, None, None, None, None, None) == 0
    assert L.dm4d_iso_pair_keys(4, -1, 4, p, p, p, None) == -1 and L.dm4d_iso_pair_keys(4, 0, 4, None, None, None, None) == 0
    assert L.dm4d_iso_mc_classify(0, 4, 4, p, 0.0, p, p, p, None) == -1 and b"grid" in L.dm4d_last_error()
    assert L.dm4d_iso_mc_classify(1024, 1024, 1024, p, 0.0, p, p, p, None) == -1
    assert L.dm4d_iso_mc_classify(4, 4, 4, p, float("nan"), p, p, p, None) == -1
    assert L.dm4d_iso_mc_vertices(4, 4, 4, p, p, 0.0, p, p, 5, p, None, p, None) == -1 and b"go together" in L.dm4d_last_error()
    assert L.dm4d_iso_mc_vertices(4, 4, 4, None, None, 0.0, None, None, 0, None, None, None, None) == 0
    assert L.dm4d_iso_mc_faces(4, 4, 4, p, None, p, 3, p, None) == -1 and L.dm4d_iso_mc_faces(4, 4, 4, None, None, None, 0, None, None) == 0


# --------------------------------------------------------------------------------------------------------------- refusals
def _scene(n=12):
    g = ic.random_gaussians(n, seed=1)
    return {k: torch.from_numpy(v) for k, v in g.items()}


def _field(g, **kw):
    return iso.gaussian_density_field(g["xyz"], g["scaling"], g["rotation"], g["opacity"], **kw)


def test_field_refuses_bad_arguments_and_has_no_cpu_path():
    g = _scene()
    for R, nb in ((1, 1), (513, 1), (1024, 16), (32, 5), (30, 4)):
        with pytest.raises(ValueError, match="resolution"):
            _field(g, resolution=R, num_blocks=nb)
    with pytest.raises(ValueError, match="N == 0"):
        _field({k: v[:0] for k, v in g.items()})
    with pytest.raises(ValueError, match="opacity > 0.005"):
        _field(dict(g, opacity=torch.full((12,), 0.005)))             # the filter is strict
    one = {k: v[:1] for k, v in g.items()}
    with pytest.raises(ValueError, match="no extent"):
        _field(one)
    with pytest.raises(ValueError, match="no extent"):                # only the kept Gaussians count
        _field(dict(g, opacity=torch.tensor([0.9] + [0.001] * 11)))
    for key in ("xyz", "scaling", "rotation", "opacity"):
        for bad in (float("nan"), float("inf")):
            t = g[key].clone()
            t.view(-1)[3] = bad
            with pytest.raises(ValueError, match="not all finite"):
                _field(dict(g, **{key: t}))
    with pytest.raises(ValueError, match="not all finite"):
        _field(g, rgb=torch.full((12, 3), float("nan")))
    with pytest.raises(ValueError, match="float32"):
        _field(dict(g, xyz=g["xyz"].double()))
    with pytest.raises(ValueError, match="rotation must be"):
        _field(dict(g, rotation=g["rotation"][:, :3]))
    with pytest.raises(TypeError):
        _field(dict(g, xyz=g["xyz"].numpy()))
    with pytest.raises(_lib.Dm4dError, match="no CPU path"):
        _field(g)
    with pytest.raises(_lib.Dm4dError, match="no CPU path"):
        _field(dict(g, opacity=g["opacity"][:, None]), rgb=g["rgb"], resolution=32, num_blocks=4)


def test_marching_cubes_and_extract_mesh_refuse_on_the_host():
    f = torch.zeros(4, 5, 6)
    with pytest.raises(_lib.Dm4dError, match="no CPU path"):
        iso.marching_cubes(f, 0.5)
    with pytest.raises(ValueError, match="occ must be"):
        iso.marching_cubes(f.double(), 0.5)
    with pytest.raises(ValueError, match="occ must be"):
        iso.marching_cubes(f[0], 0.5)
    with pytest.raises(ValueError, match="csum must be"):
        iso.marching_cubes(f, 0.5, csum=torch.zeros(4, 5, 6))
    with pytest.raises(ValueError, match="not a number"):
        iso.marching_cubes(f, float("nan"))
    with pytest.raises(ValueError, match="lacks"):
        iso.extract_mesh({"xyz": torch.zeros(3, 3)})
    with pytest.raises(_lib.Dm4dError, match="no CPU path"):
        iso.extract_mesh(_scene(), resolution=32, num_blocks=4)


def test_block_bounds_are_the_reference_float32_operations():
    coords, vmin, vmax = iso.block_bounds(32, 16)
    x = torch.linspace(-1, 1, 32)
    assert torch.equal(coords, x) and coords.dtype == torch.float32 and vmin.shape == vmax.shape == (16,)
    for b, xs in enumerate(x.split(2)):                                # the reference's per-block amin / amax, then -= / +=
        lo, hi = xs.amin(), xs.amax()
        lo -= (2 / 16) * 1.5
        hi += (2 / 16) * 1.5
        assert lo == vmin[b] and hi == vmax[b]
    assert (vmin[1:] > vmin[:-1]).all() and (vmax[1:] > vmax[:-1]).all()


def test_cli_arguments_and_output_name():
    p = iso._parser()
    a = p.parse_args(["--ply", "in/point_cloud.ply", "--output", "out"])
    assert (a.ply, a.resolution, a.num_blocks, a.density_thresh, a.output) == ("in/point_cloud.ply", 128, 16, 0.8, "out")
    for argv in (["--ply", "g.ply"], ["--output", "o"], ["--ply", "g.ply", "--output", "o", "--resolution", "x"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
    assert iso.output_path("some/dir/last.v2.ply", "out") == os.path.join("out", "last_mc.ply")


# ------------------------------------------------------------------------------------------------------------ file format
def test_gaussian_ply_round_trip_is_bit_exact_and_applies_the_activations(tmp_path):
    rng = np.random.default_rng(2)
    n = 23
    cols = {"xyz": rng.normal(size=(n, 3)), "f_dc": rng.normal(size=(n, 3)), "f_rest": rng.normal(size=(n, 45)),
            "opacity_raw": rng.normal(size=n) * 4, "scale_raw": rng.normal(size=(n, 3)) - 4, "rotation": rng.normal(size=(n, 4))}
    cols = {k: v.astype(np.float32) for k, v in cols.items()}
    path = str(tmp_path / "g.ply")
    wf.write_gaussian_ply(path, cols["xyz"], cols["f_dc"], cols["f_rest"], cols["opacity_raw"], cols["scale_raw"], cols["rotation"])
    with open(path, "rb") as fh:
        head = fh.read().split(b"end_header\n")[0].decode().splitlines()
    names = [l.split()[2] for l in head if l.startswith("property")]
    assert all(l.split()[1] == "float" for l in head if l.startswith("property")) and head[1] == "format binary_little_endian 1.0"
    assert names == ["x", "y", "z", "nx", "ny", "nz"] + [f"f_dc_{i}" for i in range(3)] + [f"f_rest_{i}" for i in range(45)] \
        + ["opacity"] + [f"scale_{i}" for i in range(3)] + [f"rot_{i}" for i in range(4)]
    g = wf.read_gaussian_ply(path)
    for k, v in cols.items():
        assert g[k].dtype == np.float32 and g[k].tobytes() == v.tobytes(), k
    t = lambda k: torch.from_numpy(cols[k])
    assert np.allclose(g["opacity"], torch.sigmoid(t("opacity_raw")).numpy(), rtol=3e-7, atol=0)
    assert np.allclose(g["scaling"], torch.exp(t("scale_raw")).numpy(), rtol=3e-7, atol=0)
    assert np.array_equal(g["rgb"], cols["f_dc"] * np.float32(0.28209479177387814) + np.float32(0.5))
    assert g["opacity"].shape == (n,) and g["scaling"].shape == (n, 3) and g["rgb"].shape == (n, 3)
    # degree 0: no f_rest columns at all
    wf.write_gaussian_ply(path, cols["xyz"], cols["f_dc"], np.zeros((n, 0)), cols["opacity_raw"][:, None], cols["scale_raw"], cols["rotation"])
    g0 = wf.read_gaussian_ply(path)
    assert g0["f_rest"].shape == (n, 0) and g0["opacity_raw"].tobytes() == cols["opacity_raw"].tobytes()
    mesh = str(tmp_path / "m.ply")
    wf.write_ply(mesh, np.zeros((3, 3)), np.array([[0, 1, 2]]))
    with pytest.raises(ValueError, match="expected 3 columns for f_dc"):
        wf.read_gaussian_ply(mesh)
