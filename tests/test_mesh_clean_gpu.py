"""Device tests of mesh cleaning (csrc/mesh_clean.hip through dreammesh4d_amd/mesh_clean.py): connected components and every field
of ``clean_mesh`` against the numpy restatement of tests/mesh_clean_common.py, bit for bit -- integers and copied floats need no
tolerance -- then the blob-plus-floaters field end to end, ``extract_mesh`` with and without cleaning, and the two CLIs."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from dreammesh4d_amd import isosurface as iso, mesh_clean as mc, wire_formats as wf
from tests import isosurface_common as ic, mesh_clean_common as cm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPONENT_CASES = cm.component_cases()
CLEAN_CASES = cm.clean_cases()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(res):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in res.items()}


@pytest.mark.parametrize("name", sorted(COMPONENT_CASES))
def test_components_equal_the_restatement(name):
    faces, V = COMPONENT_CASES[name]
    want, n_want = cm.labels_scipy(faces, V)
    for f in (dev(faces), dev(faces.astype(np.int32))):
        labels, n = mc.connected_components(f, V)
        assert labels.dtype == torch.int32 and labels.device == f.device and tuple(labels.shape) == (V,)
        assert np.array_equal(labels.cpu().numpy(), want) and n == n_want


def test_components_refuse_an_index_out_of_range():
    with pytest.raises(ValueError, match=r"face indices span \[0, 3\], the mesh has 3 vertices"):
        mc.connected_components(dev(np.array([[0, 1, 3]], np.int64)), 3)
    with pytest.raises(ValueError, match=r"face indices span \[-1, 2\]"):
        mc.clean_mesh(dev(np.zeros((3, 3), np.float32)), dev(np.array([[0, -1, 2]], np.int64)))
    with pytest.raises(ValueError, match="not all finite"):
        mc.clean_mesh(dev(np.array([[0, 0, 0], [1, 0, 0], [0, np.inf, 0]], np.float32)), dev(np.array([[0, 1, 2]], np.int64)))


@pytest.mark.parametrize("name", sorted(CLEAN_CASES))
def test_clean_mesh_equals_the_restatement(name):
    v, f, c, kw = CLEAN_CASES[name]
    if "int32" in name:
        f = f.astype(np.int32)
    want = cm.restate(v, f, c, **kw)
    got = host(mc.clean_mesh(dev(v), dev(f), dev(c), **kw))
    assert sorted(got) == sorted(cm.FIELDS)
    assert cm.differences(got, want) == []
    assert got["faces"].dtype == np.int64 and got["labels"].dtype == np.int32 and got["verts"].dtype == np.float32


def test_unreferenced_non_finite_vertices_do_not_matter():
    v, f, c = cm.tie()
    v = np.concatenate([v, np.array([[np.nan, 0, 0], [np.inf, -np.inf, 1]], np.float32)])
    c = np.concatenate([c, np.zeros((2, 3), np.float32)])
    got = host(mc.clean_mesh(dev(v), dev(f), dev(c), min_f=75, min_d=1.0))
    assert cm.differences(got, cm.restate(v, f, c, min_f=75, min_d=1.0)) == [] and len(got["faces"]) == 160


@pytest.fixture(scope="module")
def blob():
    return iso.marching_cubes(dev(cm.blob_field(32)), 0.0)


def test_blob_plus_floaters(blob):
    """One large ball and six floaters at R = 32 through marching cubes on the device, cleaned with the defaults: equal to the
    restatement, exactly one component survives, and prune_isolated_points has nothing left to remove."""
    from dreammesh4d_amd.threestudio_host import prune_isolated_points

    v, f = blob["verts"].cpu().numpy(), blob["faces"].cpu().numpy()
    want = cm.restate(v, f, None)
    got = host(mc.clean_mesh(blob["verts"], blob["faces"], None))
    assert cm.differences(got, want) == []
    assert (want["face_count"] > 0).sum() == 7 and got["n_small"] == 6 and got["n_components"] >= 7
    survivors = np.unique(got["labels"][got["vertex_map"] >= 0])
    assert len(survivors) == 1 and 1000 < len(got["faces"]) < len(f) and ic.manifold_defects(got["faces"])[0] == 0
    assert np.array_equal(mc.connected_components(dev(got["faces"]), len(got["verts"]))[0].cpu().numpy(), np.zeros(len(got["verts"]), np.int32))
    pv, pf, pc = prune_isolated_points(got["verts"].astype(np.float64), got["faces"], np.ones_like(got["verts"], dtype=np.float64))
    assert np.array_equal(pv, got["verts"].astype(np.float64)) and np.array_equal(pf, got["faces"]) and len(pc) == len(pv)


def test_two_runs_give_the_same_bytes():
    """The largest case here: the R = 64 blob-plus-floaters mesh with colours, every output compared as bytes."""
    mesh = iso.marching_cubes(dev(cm.blob_field(64)), 0.0)
    colors = torch.rand(mesh["verts"].shape, device=DEV)
    a = host(mc.clean_mesh(mesh["verts"], mesh["faces"], colors, keep="largest"))
    b = host(mc.clean_mesh(mesh["verts"], mesh["faces"], colors, keep="largest"))
    assert len(a["faces"]) > 10000 and cm.differences(a, b) == []
    la, na = mc.connected_components(mesh["faces"], len(mesh["verts"]))
    lb, nb = mc.connected_components(mesh["faces"], len(mesh["verts"]))
    assert torch.equal(la, lb) and na == nb == 7


def _gaussians():
    g = ic.sphere_gaussians(600)
    far = ic.sphere_gaussians(40, radius=0.04)                          # a floater well outside the sphere
    far["xyz"] = far["xyz"] + np.float32([0.9, 0.9, 0.9])
    far["scaling"] = np.full_like(far["scaling"], 0.02)
    return {k: np.concatenate([g[k], far[k]]) for k in g}


def test_extract_mesh_default_is_unchanged_and_clean_is_clean_mesh():
    g = {k: dev(v) for k, v in _gaussians().items()}
    kw = dict(density_thresh=0.3, resolution=48, num_blocks=8)
    plain = iso.extract_mesh(g, **kw)
    fld = iso.gaussian_density_field(g["xyz"], g["scaling"], g["rotation"], g["opacity"], g["rgb"], resolution=48, num_blocks=8)
    mesh = iso.marching_cubes(fld["occ"], 0.3, fld["csum"])
    world = (mesh["verts"] / (48 - 1.0) * 2 - 1) / fld["scale"] + fld["center"]
    assert sorted(plain) == ["center", "colors", "faces", "n_kept", "n_pairs", "scale", "verts"]
    assert torch.equal(plain["verts"], world) and torch.equal(plain["faces"], mesh["faces"]) and torch.equal(plain["colors"], mesh["colors"])
    assert mc.connected_components(plain["faces"], len(plain["verts"]))[1] >= 2
    for ckw in (dict(), dict(min_f=10, min_d=0.0, keep="largest")):
        cleaned = iso.extract_mesh(g, clean=True, **kw, **ckw)
        want = mc.clean_mesh(plain["verts"], plain["faces"], plain["colors"], **ckw)
        assert cm.differences(host(cleaned), host(want)) == []
        assert cleaned["n_kept"] == plain["n_kept"] and 0 < len(cleaned["faces"]) < len(plain["faces"])
        assert len(np.unique(cleaned["labels"].cpu().numpy()[cleaned["vertex_map"].cpu().numpy() >= 0])) == 1


def test_mesh_clean_cli_round_trips_a_ply(tmp_path):
    v, f, c = cm.tie()
    src = str(tmp_path / "tie.ply")
    wf.write_ply(src, v, f, colors=c)
    run = subprocess.run([sys.executable, "-m", "dreammesh4d_amd.mesh_clean", "--mesh_path", src, "--output", str(tmp_path / "out"), "--min_f", "75",
                          "--min_d", "0", "--keep", "largest"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert "Cleaned mesh has 82 vertices and 80 triangles" in run.stdout and "1 of them small" in run.stdout
    back = wf.read_mesh(str(tmp_path / "out" / "tie_clean.ply"))
    mesh = wf.read_mesh(src)
    want = cm.restate(mesh["verts"].astype(np.float32), mesh["faces"], mesh["colors"].astype(np.float32), min_f=75, min_d=0, keep="largest")
    assert np.array_equal(back["faces"], want["faces"]) and np.array_equal(back["verts"].astype(np.float32), want["verts"])
    assert np.array_equal(back["colors"].astype(np.float32), want["colors"])


def test_isosurface_cli_cleans_on_request(tmp_path):
    """`--clean` writes what the restatement makes of the mesh the same command line extracts without it (here: extract_mesh on
    the Gaussians as the CLI reads them)."""
    g = _gaussians()
    n = len(g["xyz"])
    ply = str(tmp_path / "gauss.ply")
    logit = np.log(g["opacity"] / (1 - g["opacity"]))
    wf.write_gaussian_ply(ply, g["xyz"], (g["rgb"] - 0.5) / wf.SH_C0, np.zeros((n, 0)), logit, np.log(g["scaling"]), g["rotation"])
    run = subprocess.run([sys.executable, "-m", "dreammesh4d_amd.isosurface", "--ply", ply, "--resolution", "48", "--num_blocks", "8",
                          "--density_thresh", "0.3", "--output", str(tmp_path / "c"), "--clean", "--min_f", "10", "--min_d", "0", "--keep", "largest"],
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert "duplicate faces, 2 components, 0 of them small" in run.stdout
    cleaned = wf.read_mesh(str(tmp_path / "c" / "gauss_mc.ply"))
    read = wf.read_gaussian_ply(ply)
    plain = iso.extract_mesh({k: dev(np.ascontiguousarray(read[k], np.float32)) for k in ("xyz", "scaling", "rotation", "opacity", "rgb")},
                             density_thresh=0.3, resolution=48, num_blocks=8)
    pv, pf = plain["verts"].cpu().numpy(), plain["faces"].cpu().numpy()
    assert cm.labels_scipy(pf, len(pv))[1] == 2 and cm.labels_scipy(cleaned["faces"], len(cleaned["verts"]))[1] == 1
    again = cm.restate(pv, pf, None, min_f=10, min_d=0, keep="largest")
    assert np.array_equal(cleaned["faces"], again["faces"]) and np.array_equal(cleaned["verts"].astype(np.float32), again["verts"])
    assert cleaned["colors"] is not None and len(cleaned["faces"]) < len(pf)
