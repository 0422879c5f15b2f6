"""Mesh cleaning without a device: the numpy restatement's components against an independent BFS, the cases the device tests
rely on really exercise what they are named for, the library exports what include/dm4d_mesh_clean.h declares, the C entry points
refuse bad sizes and pointers before any launch, the API refuses what it does not take, by name."""
import subprocess

import numpy as np
import pytest
import torch

from dreammesh4d_amd import _lib, mesh_clean as mc
from tests import mesh_clean_common as cm

COMPONENT_CASES = cm.component_cases()
CLEAN_CASES = cm.clean_cases()


@pytest.mark.parametrize("name", sorted(COMPONENT_CASES))
def test_restatement_labels_equal_a_bfs(name):
    faces, V = COMPONENT_CASES[name]
    labels, n = cm.labels_scipy(faces, V)
    bfs = cm.labels_bfs(faces, V)
    assert labels.dtype == np.int32 and np.array_equal(labels, bfs) and n == len(np.unique(bfs))
    assert (labels <= np.arange(V)).all() and np.array_equal(labels[labels], labels)


def test_component_cases_are_what_they_are_named():
    n = {k: cm.labels_scipy(*v)[1] for k, v in COMPONENT_CASES.items()}
    assert n["empty V=0"] == 0 and n["empty V=5"] == 5 and n["one triangle"] == 1
    assert n["65 vertices"] == 3 + 5 and n["4097 vertices"] == 3 + 5 + (4097 - 5) % 3
    assert n["strip 4096 ascending"] == n["strip 4096 descending"] == n["strip 4096 random"] == 1
    assert n["1000 tetrahedra interleaved"] == 1000 and n["two blobs share a vertex"] == 1
    assert n["isolated between used"] == 1 + 2 * 202 and n["hubs low"] == n["hubs high"] == 1
    f, V = COMPONENT_CASES["1000 tetrahedra interleaved"]
    assert np.array_equal(cm.labels_scipy(f, V)[0], np.arange(V) % 1000)
    assert len(COMPONENT_CASES["hubs low"][0]) > 4 * 256


def test_clean_cases_are_what_they_are_named():
    zv, zf, _ = cm.zoo()
    r = cm.restate(zv, zf, None, min_f=0, min_d=0)
    assert r["n_null"] == 4 and r["n_duplicate"] == 8 and r["n_small"] == 0          # 2 repeated, 1 collinear, 1 coincident; 6 + 2
    assert len(r["faces"]) == len(zf) - 12 and len(r["verts"]) == len(zv) - 8        # 6 orphans, 2 never named
    assert sorted(r["face_count"][r["face_count"] > 0].tolist()) == [1, 1, 5, 10, 63, 64, 100, 300]
    assert (r["labels"][r["vertex_map"] < 0] == np.nonzero(r["vertex_map"] < 0)[0]).all()
    by_f = cm.restate(zv, zf, None, min_f=64, min_d=0)
    assert sorted(by_f["face_count"][by_f["kept"]].tolist()) == [64, 100, 300] and by_f["n_small"] == 5
    by_d = cm.restate(zv, zf, None, min_f=0, min_d=20.0)
    assert sorted(by_d["face_count"][by_d["kept"]].tolist()) == [10, 63, 64, 300] and by_d["n_small"] == 4      # 100 tiny faces go, 10 long stay
    both = cm.restate(zv, zf, None)
    assert sorted(both["face_count"][both["kept"]].tolist()) == [64, 300] and both["n_small"] == 6
    ov, of_, _, kw = CLEAN_CASES["64 and 63 faces"]
    r = cm.restate(ov, of_, None, **kw)
    assert r["face_count"][r["kept"]].tolist() == [64] and r["n_small"] == 1 and len(r["faces"]) == 64
    tv, tf, _, kw = CLEAN_CASES["tie largest"]
    r = cm.restate(tv, tf, None, **kw)
    tied = np.nonzero(r["face_count"] == 80)[0]
    assert len(tied) == 2 and np.nonzero(r["kept"])[0].tolist() == [tied.min()] and r["n_small"] == 0 and len(r["faces"]) == 80
    order = cm.restate(tv, tf, None, min_f=0, min_d=0)
    assert (np.diff(order["face_map"]) > 0).all() and (np.diff(order["vertex_map"][order["vertex_map"] >= 0]) == 1).all()
    r = cm.restate(*CLEAN_CASES["all dropped, largest"][:3], **CLEAN_CASES["all dropped, largest"][3])
    assert len(r["faces"]) == 0 and len(r["verts"]) == 0 and r["n_small"] == 3


def test_blob_field_floaters_fall_under_the_defaults():
    """The R = 32 field of the device test, through the numpy marching cubes: seven components, the six small ones under min_d or
    min_f, the large one holds every surviving vertex (so the 75 % rule downstream has nothing to remove)."""
    from tests import isosurface_common as ic

    m = ic.marching_cubes_reference(cm.blob_field(32), 0.0)
    v, f = m["verts"], m["faces"]
    r = cm.restate(v, f, None)
    has = r["face_count"] > 0
    assert has.sum() == 7 and r["kept"].sum() == 1 and r["n_small"] == 6 and r["n_duplicate"] == 0
    assert 0 < r["n_null"] < 50                                        # marching cubes leaves a few triangles without area
    small = has & ~r["kept"]
    thr2 = 0.2 ** 2 * r["D2"]
    assert ((r["d2"][small] < thr2) | (r["face_count"][small] < 64)).all() and r["d2"][r["kept"]][0] > thr2
    assert r["face_count"][small].min() >= 24 and r["face_count"][r["kept"]][0] > 1000
    assert len(r["verts"]) == (r["labels"] == np.nonzero(r["kept"])[0][0]).sum()


def test_library_exports_the_header():
    L = _lib.lib()
    names = _lib.declared_symbols("mcl")
    assert names == ["dm4d_mcl_compact", "dm4d_mcl_component_stats", "dm4d_mcl_components_round", "dm4d_mcl_face_first",
                     "dm4d_mcl_face_flags", "dm4d_mcl_keep", "dm4d_mcl_version"]
    assert [n for n in names if not hasattr(L, n)] == []
    assert L.dm4d_mcl_version() == _lib.abi_version("mcl") == 1
    assert _lib.abi_version() == 107 and _lib.abi_version("dc") == 1 and _lib.abi_version("iso") == 1 and _lib.abi_version("sr") == 1
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(ln.split()[-1] for ln in out.splitlines() if " T dm4d_mcl_" in ln) == names
    assert _lib.DM4D_MCL_STATE_WORDS == 16 and _lib.DM4D_MCL_STATE_BEST % 2 == 0


P = 0x1000                                               # a non-null, aligned pointer no refused call ever follows


def _call(fn, args, **change):
    """`args`: list of (name, value); `change` replaces values by name."""
    return fn, tuple(change.get(k, v) for k, v in args)


FLAGS = [("F", 4), ("V", 6), ("verts", P), ("faces", P), ("null_face", P), ("key_hi", P), ("key_lo", P), ("state", P), ("stream", None)]
FIRST = [("F", 4), ("perm", P), ("key_hi", P), ("key_lo", P), ("null_face", P), ("alive", P), ("state", P), ("stream", None)]
ROUND = [("F", 4), ("V", 6), ("faces", P), ("alive", None), ("first_round", 1), ("parent", P), ("stream", None)]
STATS = [("F", 4), ("V", 6), ("verts", P), ("faces", P), ("alive", P), ("labels", P), ("face_count", P), ("box", P), ("state", P), ("stream", None)]
KEEP = [("F", 4), ("V", 6), ("faces", P), ("alive", P), ("labels", P), ("face_count", P), ("box", P), ("thr2", 1.0), ("use_d", 1), ("min_f", 64),
        ("largest", 0), ("comp_keep", P), ("keep_vertex", P), ("keep_face", P), ("state", P), ("stream", None)]
COMPACT = [("F", 4), ("V", 6), ("Fo", 2), ("Vo", 3), ("verts", P), ("colors", P), ("faces", P), ("keep_vertex", P), ("vert_end", P), ("keep_face", P),
           ("face_end", P), ("out_verts", P), ("out_colors", P), ("out_faces", P), ("vertex_map", P), ("face_map", P), ("stream", None)]
TOO_MANY = 1 << 31

REFUSED = {
    "flags F < 0": (_call("dm4d_mcl_face_flags", FLAGS, F=-1), "F"),
    "flags V too large": (_call("dm4d_mcl_face_flags", FLAGS, V=TOO_MANY), "V"),
    "flags null verts": (_call("dm4d_mcl_face_flags", FLAGS, verts=None), "verts is null"),
    "flags null faces": (_call("dm4d_mcl_face_flags", FLAGS, faces=None), "faces is null"),
    "flags null state with nothing to do": (_call("dm4d_mcl_face_flags", FLAGS, F=0, state=None), "state is null"),
    "flags misaligned verts": (_call("dm4d_mcl_face_flags", FLAGS, verts=P + 2), "verts is not 4-byte aligned"),
    "flags misaligned key_lo": (_call("dm4d_mcl_face_flags", FLAGS, key_lo=P + 4), "key_lo is not 8-byte aligned"),
    "flags misaligned state": (_call("dm4d_mcl_face_flags", FLAGS, state=P + 4), "state is not 8-byte aligned"),
    "first F too large": (_call("dm4d_mcl_face_first", FIRST, F=TOO_MANY), "F"),
    "first null perm": (_call("dm4d_mcl_face_first", FIRST, perm=None), "perm is null"),
    "first null alive": (_call("dm4d_mcl_face_first", FIRST, alive=None), "alive is null"),
    "first misaligned perm": (_call("dm4d_mcl_face_first", FIRST, perm=P + 4), "perm is not 8-byte aligned"),
    "round V < 0": (_call("dm4d_mcl_components_round", ROUND, V=-2), "V"),
    "round null parent": (_call("dm4d_mcl_components_round", ROUND, parent=None), "parent is null"),
    "round null faces": (_call("dm4d_mcl_components_round", ROUND, faces=None), "faces is null"),
    "round misaligned parent": (_call("dm4d_mcl_components_round", ROUND, parent=P + 1), "parent is not 4-byte aligned"),
    "stats F < 0": (_call("dm4d_mcl_component_stats", STATS, F=-1), "F"),
    "stats box without verts": (_call("dm4d_mcl_component_stats", STATS, verts=None), "verts and box go together"),
    "stats null labels": (_call("dm4d_mcl_component_stats", STATS, labels=None), "labels is null"),
    "stats null face_count": (_call("dm4d_mcl_component_stats", STATS, face_count=None), "face_count is null"),
    "stats misaligned box": (_call("dm4d_mcl_component_stats", STATS, box=P + 2), "box is not 4-byte aligned"),
    "keep min_f < 0": (_call("dm4d_mcl_keep", KEEP, min_f=-1), "min_f"),
    "keep thr2 nan": (_call("dm4d_mcl_keep", KEEP, thr2=float("nan")), "thr2"),
    "keep thr2 < 0": (_call("dm4d_mcl_keep", KEEP, thr2=-1.0), "thr2"),
    "keep flag 2": (_call("dm4d_mcl_keep", KEEP, largest=2), "largest"),
    "keep null box with the diameter test": (_call("dm4d_mcl_keep", KEEP, box=None), "box is null"),
    "keep null keep_face": (_call("dm4d_mcl_keep", KEEP, keep_face=None), "keep_face is null"),
    "keep misaligned labels": (_call("dm4d_mcl_keep", KEEP, labels=P + 2), "labels is not 4-byte aligned"),
    "compact Vo > V": (_call("dm4d_mcl_compact", COMPACT, Vo=7), "Vo"),
    "compact Fo < 0": (_call("dm4d_mcl_compact", COMPACT, Fo=-1), "Fo"),
    "compact colors without out_colors": (_call("dm4d_mcl_compact", COMPACT, out_colors=None), "colors and out_colors go together"),
    "compact null vert_end": (_call("dm4d_mcl_compact", COMPACT, vert_end=None), "vert_end is null"),
    "compact null face_map": (_call("dm4d_mcl_compact", COMPACT, face_map=None), "face_map is null"),
    "compact misaligned out_faces": (_call("dm4d_mcl_compact", COMPACT, out_faces=P + 4), "out_faces is not 8-byte aligned"),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_host_validation_refuses_without_a_device(name):
    (fn, args), words = REFUSED[name]
    rc = getattr(_lib.lib(), fn)(*args)
    assert rc == _lib.DM4D_ERR_INVALID, f"{fn}{args} returned {rc}"
    msg = _lib.lib().dm4d_last_error().decode()
    assert msg.startswith(fn + ":") and words in msg, msg


def _mesh(n=4):
    v, f = cm.strip_mesh(n)
    return torch.from_numpy(v), torch.from_numpy(f), torch.rand(len(v), 3)


def test_api_refuses_cpu_tensors():
    v, f, c = _mesh()
    with pytest.raises(_lib.Dm4dError, match="clean_mesh: .*no CPU path"):
        mc.clean_mesh(v, f, c)
    with pytest.raises(_lib.Dm4dError, match="clean_mesh: .*no CPU path"):
        mc.clean_mesh(v, f.int())
    with pytest.raises(_lib.Dm4dError, match="connected_components: .*no CPU path"):
        mc.connected_components(f, len(v))


def test_api_refuses_bad_arguments_by_name():
    v, f, c = _mesh()
    for bad, word in ((v[:, :2], "verts"), (v.double(), "verts"), (v.reshape(-1), "verts")):
        with pytest.raises(ValueError, match=f"clean_mesh: {word} must be"):
            mc.clean_mesh(bad, f, None)
    for bad in (f[:, :2], f.float(), f.to(torch.int16), f.reshape(-1)):
        with pytest.raises(ValueError, match="clean_mesh: faces must be"):
            mc.clean_mesh(v, bad, c)
        with pytest.raises(ValueError, match="connected_components: faces must be"):
            mc.connected_components(bad, len(v))
    for bad in (c[:-1], c.double(), c[:, :2]):
        with pytest.raises(ValueError, match="clean_mesh: colors must be"):
            mc.clean_mesh(v, f, bad)
    for bad in (v.numpy(), None):
        with pytest.raises(TypeError, match="clean_mesh: verts and colors"):
            mc.clean_mesh(bad, f, c)
    with pytest.raises(TypeError, match="clean_mesh: faces must be a torch tensor"):
        mc.clean_mesh(v, f.numpy(), c)
    for bad in ("biggest", None, 1, "ALL"):
        with pytest.raises(ValueError, match="clean_mesh: keep must be one of"):
            mc.clean_mesh(v, f, c, keep=bad)
    for bad in (-1, 1.5, True, None, 1 << 31):
        with pytest.raises(ValueError, match="clean_mesh: min_f must be"):
            mc.clean_mesh(v, f, c, min_f=bad)
    for bad in (-0.5, float("nan"), float("inf"), "20", None, True):
        with pytest.raises(ValueError, match="clean_mesh: min_d must be"):
            mc.clean_mesh(v, f, c, min_d=bad)
    for bad in (-1, 2.0, None, True, 1 << 31):
        with pytest.raises(ValueError, match="connected_components: n_verts must be"):
            mc.connected_components(f, bad)


def test_host_helpers():
    x = np.array([0.0, -0.0, 1.5, -2.25, 3e38, -3e38, 1e-45, np.inf, -np.inf], np.float32)
    u = x.view(np.uint32)
    image = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    assert np.array_equal(mc.unimage(image).view(np.uint32), u)
    order = np.argsort(image, kind="stable")
    assert (np.diff(x[order].astype(np.float64)) >= 0).all() and image[1] < image[0]
    assert mc.diagonal2(np.float32([0, 1, 2]), np.float32([3, 5, 14])) == 9 + 16 + 144 == cm.diagonal2([0, 1, 2], [3, 5, 14])
    assert mc.output_path("/a/b/blob_mc.v2.ply", "out") == "out/blob_mc_clean.ply"
    args = mc._parser().parse_args(["--mesh_path", "m.ply", "--output", "o"])
    assert (args.min_f, args.min_d, args.keep) == (64, 20.0, "all")
    from dreammesh4d_amd import isosurface as iso

    args = iso._parser().parse_args(["--ply", "g.ply", "--output", "o"])
    assert args.clean is False and (args.min_f, args.min_d, args.keep) == (64, 20.0, "all")
    args = iso._parser().parse_args(["--ply", "g.ply", "--output", "o", "--clean", "--min_f", "8", "--min_d", "2.5", "--keep", "largest"])
    assert args.clean is True and (args.min_f, args.min_d, args.keep) == (8, 2.5, "largest")
