"""CPU-side tests of mesh simplification by vertex clustering: the float64 restatement (tests/mesh_simplify_common.py) on cases
worked by hand, the host-side validation of the operator and of its C entry points (no device is touched), the command line,
and the presence of the new symbols in the cross-compiled library."""
import ctypes as C

import numpy as np
import pytest
import torch

from dreammesh4d_amd import _lib, mesh_simplify as ms
from tests import mesh_simplify_common as mc

SYMBOLS = ("dm4d_simplify_vertex_keys", "dm4d_simplify_cluster_average", "dm4d_simplify_face_remap", "dm4d_simplify_face_first")


# ------------------------------------------------------------------------------------------------ the restatement, by hand
def test_restatement_on_a_3x3_grid_of_quads():
    """4 x 4 vertices at integer coordinates, scale 2: voxel 1.5, origin -0.75, so coordinate 0 -> cell 0, 1 and 2 -> cell 1,
    3 -> cell 2 on both axes and everything in cell 0 along z: 3 x 3 x 1 cells, all occupied, key = 3 iy + ix.  Cluster
    coordinates are the means 0, 1.5, 3.  Of the 9 quads only the 4 that cross a boundary on BOTH axes survive (the corner
    quads); each triangle is given starting at a corner that is not its smallest cluster, so the rotation is exercised."""
    verts = np.array([[j, i, 0] for i in range(4) for j in range(4)], np.float32)
    faces = []
    for i in range(3):
        for j in range(3):
            v00 = 4 * i + j
            v01, v10, v11 = v00 + 1, v00 + 4, v00 + 5
            faces += [(v11, v00, v01), (v10, v00, v11)]
    ref = mc.simplify_reference(verts, np.array(faces), scale=2)
    assert ref["voxel_size"] == 1.5 and ref["origin"].tolist() == [-0.75, -0.75, -0.75] and ref["grid"] == (3, 3, 1)
    group = [0, 1, 1, 2]
    assert ref["vertex_cluster"].tolist() == [3 * group[i] + group[j] for i in range(4) for j in range(4)]
    mean = [0.0, 1.5, 3.0]
    assert ref["verts"].dtype == np.float32 and ref["verts"].tolist() == [[mean[c % 3], mean[c // 3], 0.0] for c in range(9)]
    assert ref["faces"].tolist() == [[0, 1, 4], [0, 4, 3], [1, 2, 5], [1, 5, 4], [3, 4, 7], [3, 7, 6], [4, 5, 8], [4, 8, 7]]
    assert (ref["n_vertices"], ref["n_faces"], ref["n_degenerate"], ref["n_duplicate"]) == (9, 8, 10, 0)


def test_restatement_puts_a_vertex_on_a_cell_boundary_into_the_upper_cell():
    """x = 0..4, scale 2: voxel 2, origin -1, cell boundaries at 1 and 3.  (1 + 1) / 2 = 1 and (3 + 1) / 2 = 2 exactly: floor
    sends the boundary vertices up.  Clusters {0}, {1, 2}, {3, 4}."""
    verts = np.array([[x, 0, 0] for x in range(5)], np.float32)
    ref = mc.simplify_reference(verts, np.array([[4, 0, 2], [0, 1, 2], [3, 4, 0]]), scale=2)
    assert ref["grid"] == (3, 1, 1) and ref["vertex_cluster"].tolist() == [0, 1, 1, 2, 2]
    assert ref["verts"].tolist() == [[0, 0, 0], [1.5, 0, 0], [3.5, 0, 0]]
    assert ref["faces"].tolist() == [[0, 1, 2]] and ref["n_degenerate"] == 2 and ref["n_duplicate"] == 0
    # the grid scene of the device tests is built the same way
    v, _, _ = mc.grid_scene()
    r = mc.simplify_reference(v, np.zeros((0, 3), np.int64), scale=4)
    assert r["voxel_size"] == 2.0 and r["origin"].tolist()[:2] == [-1.0, -1.0]
    on_boundary = (v[:, 0] % 2 == 1)
    assert on_boundary.sum() > 100 and np.array_equal((r["vertex_cluster"] % 5)[on_boundary], ((v[:, 0] + 1) // 2)[on_boundary])


def test_restatement_duplicates_and_orientation():
    """A, A' share a cell; B, C are far away.  (A, B, C) and (A', B, C) collapse to one triple: the first is kept.  (B, C, A') is
    the same triple again after the rotation.  (A, C, B) has the opposite orientation: it is a different face and survives."""
    verts = np.array([[0, 0, 0], [0.25, 0, 0], [4, 0, 0], [0, 4, 0]], np.float32)           # A, A', B, C
    ref = mc.simplify_reference(verts, np.array([[0, 2, 3], [1, 2, 3], [2, 3, 1], [0, 3, 2], [3, 2, 1], [0, 1, 2]]), scale=2)
    assert ref["vertex_cluster"].tolist() == [0, 0, 1, 2] and ref["verts"].tolist() == [[0.125, 0, 0], [4, 0, 0], [0, 4, 0]]
    assert ref["faces"].tolist() == [[0, 1, 2], [0, 2, 1]]
    assert (ref["n_faces"], ref["n_degenerate"], ref["n_duplicate"]) == (2, 1, 3) and mc.opposite_pairs(ref["faces"]) == 2


def test_restatement_sums_serially_in_vertex_order():
    """np.add.at is the serial sum of the semantics: bit-equal to an explicit loop on a crowded clustering, where a pairwise sum
    (np.sum over the members) differs in the last bit for some cluster."""
    rng = np.random.default_rng(0)
    v = (rng.normal(size=(6000, 3)) * np.array([1.0, 1e-3, 1e3])).astype(np.float32)
    col = rng.random((6000, 3)).astype(np.float32)
    ref = mc.simplify_reference(v, np.zeros((0, 3), np.int64), col, scale=3)
    assert ref["max_cluster_size"] > 500
    assert np.array_equal(ref["verts"], mc.serial_means(v, ref["vertex_cluster"], ref["n_vertices"]))
    assert np.array_equal(ref["colors"], mc.serial_means(col, ref["vertex_cluster"], ref["n_vertices"]))


def test_small_scenes_take_every_branch():
    """The scenes of the device tests (the million-vertex one is checked there) satisfy, on the restatement alone: output vertex
    count strictly between 1 and V, a degenerate face dropped, a duplicate removed, an opposite-orientation pair kept."""
    for name, (build, scale) in mc.SCENES.items():
        if name.startswith("million"):
            continue
        v, f, c = build()
        ref = mc.simplify_reference(v, f, c, scale=scale)
        mc.check_branches(ref, len(v))
        if name == "crowded_cell":
            assert ref["max_cluster_size"] > 4096


# ------------------------------------------------------------------------------------------------ host-side validation
def test_grid_parameters_and_their_refusals():
    voxel, origin, dims = ms.grid_parameters([0, 0, 0], [3, 3, 0], scale=2)
    assert voxel == 1.5 and origin == [-0.75, -0.75, -0.75] and dims == (3, 3, 1)
    assert ms.grid_parameters([0, 0, 0], [3, 3, 0], voxel_size=1.5) == (voxel, origin, dims)
    for bad in (0, -4, 2.5, True):
        with pytest.raises(ValueError, match="scale must be an integer greater than 0"):
            ms.grid_parameters([0, 0, 0], [1, 1, 1], scale=bad)
    with pytest.raises(ValueError, match="degenerate mesh"):                                   # a flat mesh: no extent on any axis
        ms.grid_parameters([1, 2, 3], [1, 2, 3], scale=64)
    with pytest.raises(ValueError, match="voxel_size must be positive"):
        ms.grid_parameters([0, 0, 0], [1, 1, 1], voxel_size=0.0)
    with pytest.raises(ValueError, match="not all finite"):
        ms.grid_parameters([0, 0, 0], [1, float("nan"), 1], scale=8)
    with pytest.raises(ValueError, match="do not fit in 62 bits"):                             # 1e7^3 cells
        ms.grid_parameters([0, 0, 0], [1, 1, 1], voxel_size=1e-7)
    with pytest.raises(ValueError, match="do not fit in 62 bits"):                             # quotient overflows float64
        ms.grid_parameters([0, 0, 0], [1e30, 1, 1], voxel_size=1e-300)
    assert ms.grid_parameters([0, 0, 0], [1, 1, 1], scale=1 << 20)[2] == ((1 << 20) + 1,) * 3    # 2^60.00..: still fits


def test_operator_validates_on_the_host_and_has_no_cpu_path():
    v = torch.rand(10, 3)
    f = torch.tensor([[0, 1, 2], [3, 4, 5]])
    for bad in (0, -1):
        with pytest.raises(ValueError, match="scale must be an integer greater than 0"):
            ms.simplify_vertex_clustering(v, f, scale=bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ms.simplify_vertex_clustering(v, f)
    with pytest.raises(ValueError, match="float32"):
        ms.simplify_vertex_clustering(v.double(), f)
    with pytest.raises(ValueError, match="faces must be"):
        ms.simplify_vertex_clustering(v, f.float())
    with pytest.raises(ValueError, match="colors must be"):
        ms.simplify_vertex_clustering(v, f, colors=torch.rand(9, 3))
    with pytest.raises(TypeError):
        ms.simplify_vertex_clustering(v.numpy(), f)
    ms.check_face_range(0, 9, 10)
    for lo, hi in ((0, 10), (-1, 9)):
        with pytest.raises(ValueError, match="face indices span"):
            ms.check_face_range(lo, hi, 10)


def test_entry_points_validate_before_any_launch():
    L = _lib.lib()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    keys = lambda V, voxel, nx, ny, nz, verts=p: L.dm4d_simplify_vertex_keys(V, verts, 0.0, 0.0, 0.0, voxel, nx, ny, nz, p, None)
    assert keys(4, 1.0, 1 << 21, 1 << 21, 1 << 20) == -4 and b"do not fit in 62 bits" in L.dm4d_last_error()
    assert keys(4, 1.0, 1 << 40, 1 << 40, 1) == -4
    assert keys(4, 0.0, 2, 2, 2) == -1 and b"voxel size" in L.dm4d_last_error()
    assert keys(4, float("nan"), 2, 2, 2) == -1 and keys(4, float("inf"), 2, 2, 2) == -1
    assert keys(4, 1.0, 0, 2, 2) == -1 and keys(-1, 1.0, 2, 2, 2) == -1 and keys(1 << 31, 1.0, 2, 2, 2) == -1
    assert keys(4, 1.0, 2, 2, 2, verts=None) == -1 and b"null" in L.dm4d_last_error()
    assert keys(0, 1.0, 2, 2, 2, verts=None) == 0
    avg = L.dm4d_simplify_cluster_average
    assert avg(4, 5, p, p, p, None, p, None, p, None) == -1 and b"5 clusters of 4 vertices" in L.dm4d_last_error()
    assert avg(4, 0, p, p, p, None, p, None, p, None) == -1
    assert avg(4, 2, p, p, p, p, p, None, p, None) == -1 and b"go together" in L.dm4d_last_error()
    assert avg(4, 2, p, None, p, None, p, None, p, None) == -1 and avg(0, 0, None, None, None, None, None, None, None, None) == 0
    remap = L.dm4d_simplify_face_remap
    assert remap(-2, 4, 2, p, p, p, p, None) == -1 and remap(3, 4, 5, p, p, p, p, None) == -1
    assert remap(3, 4, 2, p, None, p, p, None) == -1 and remap(0, 4, 2, None, None, None, None, None) == 0
    first = L.dm4d_simplify_face_first
    assert first(1 << 31, p, p, p, None) == -1 and first(3, p, p, None, None) == -1 and first(0, None, None, None, None) == 0


# ------------------------------------------------------------------------------------------------ command line, file formats
def test_cli_arguments_and_output_name():
    p = ms._parser()
    a = p.parse_args(["--mesh_path", "in/mesh.ply", "--output", "out"])
    assert (a.mesh_path, a.scale, a.output) == ("in/mesh.ply", 64, "out")
    assert p.parse_args(["--mesh_path", "m.obj", "--scale", "128", "--output", "o"]).scale == 128
    for argv in (["--mesh_path", "m.ply"], ["--output", "o"], ["--mesh_path", "m.ply", "--output", "o", "--scale", "x"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
    import os

    assert ms.output_path("some/dir/exported_mesh.ply", 64, 8123, "out") == os.path.join("out", "exported_mesh_64_8123.ply")
    assert ms.output_path("it5000-export.v2.obj", 8, 17, "d") == os.path.join("d", "it5000-export_8_17.ply")    # up to the FIRST dot


def test_read_mesh_reads_ply_and_plain_obj(tmp_path):
    from dreammesh4d_amd import wire_formats as wf

    obj = tmp_path / "m.obj"
    obj.write_text("# comment\nv 0 0 0 1 0 0\nv 1 0 0 0 1 0\nv 1 1 0 0 0 1\nv 0 1 0 0.5 0.5 0.5\nvt 0 0\nvn 0 0 1\n"
                   "f 1 2 3 4\nf 1/1 2/1 3/1\nf 1//1 3//1 4//1\nf -4/1/1 -2/1/1 -1/1/1\n")
    m = wf.read_mesh(str(obj))
    assert m["verts"].tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]]
    assert m["faces"].tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 3], [0, 2, 3]]
    assert m["colors"].tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.5, 0.5]]
    bare = tmp_path / "bare.OBJ"
    bare.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    assert wf.read_mesh(str(bare))["colors"] is None
    ply = tmp_path / "m.ply"
    wf.write_ply(str(ply), m["verts"], m["faces"], colors=m["colors"])
    back = wf.read_mesh(str(ply))
    assert np.array_equal(back["verts"], m["verts"]) and np.array_equal(back["faces"], m["faces"])
    with pytest.raises(ValueError, match="only .ply and .obj"):
        wf.read_mesh(str(tmp_path / "m.stl"))


# ------------------------------------------------------------------------------------------------ ABI
def test_library_exports_the_simplification_entry_points():
    L = _lib.lib()
    declared = _lib.declared_symbols()
    for s in SYMBOLS:
        assert s in declared and s in _lib._SIGNATURES and hasattr(L, s), s
