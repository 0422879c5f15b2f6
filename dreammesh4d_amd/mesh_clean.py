"""Mesh cleaning on the HIP device: the step between marching cubes and ``mesh_simplify`` that removes what a floater in the
occupancy field leaves behind -- and the package's connected-component primitive.

Replaces the first half of ``clean_mesh`` (custom/threestudio-dreammesh4d/geometry/mesh_utils.py:90-128: pymeshlab's
``meshing_remove_unreferenced_vertices``, ``meshing_remove_duplicate_faces``, ``meshing_remove_null_faces``,
``meshing_remove_connected_component_by_diameter`` and ``..._by_face_number``, CPU) with the kernels of ``csrc/mesh_clean.hip``.
The result is a function of the input alone ("Mesh cleaning"):

1. a vertex is referenced when any input face names it; ``lo, hi`` = the per-axis float32 min / max over the referenced vertices,
   ``D2 = dx*dx + dy*dy + dz*dz`` in float64 on the host;
2. a face is null when it repeats an index or the float64 cross product ``(b - a) x (c - a)`` of its float32 corners is exactly zero;
3. two non-null faces are duplicates when their sorted index triples are equal; the one with the smallest input position stays;
4. components over the surviving faces, two vertices connected when a surviving face names both (the one-ring graph of
   ``threestudio_host.prune_isolated_points``, not meshlab's edge adjacency); ``labels[v]`` = the smallest vertex index of v's
   component, ``labels[v] = v`` for an unreferenced or orphaned vertex;
5. per component a face count and a float32 bounding box, ``d2`` from it as in 1;
6. a component is dropped when ``min_d > 0`` and ``d2 < (min_d / 100) ** 2 * D2``, else when ``min_f > 0`` and it has fewer than
   ``min_f`` faces; ``keep="largest"`` then keeps only the surviving component with the most faces (ties: the smallest label);
7. surviving faces keep their input order with indices remapped, vertices named by a surviving face keep theirs, rows of
   ``verts`` and ``colors`` are copied bit for bit.

Not restated: ``meshing_merge_close_vertices`` (marching cubes here is already welded, and ``mesh_simplify`` is the merge step),
``meshing_repair_non_manifold_edges`` / ``_vertices``, ``meshing_isotropic_explicit_remeshing`` and ``decimate_mesh``.  Parity
with pymeshlab is unpinned (the package is not available where this is built).

The two stable sorts of the face keys and the two prefix sums of the keep flags are torch calls on the device; everything else is
HIP.  There is no CPU path.

    python -m dreammesh4d_amd.mesh_clean --mesh_path in.ply --output out_dir [--min_f 64 --min_d 20 --keep all|largest]
"""
import argparse
import math
import os

import numpy as np
import torch

from . import _args

KEEP_MODES = ("all", "largest")
MAX_COUNT = (1 << 31) - 1
MAX_ROUNDS = 64


def _checked_faces(what, faces):
    if not torch.is_tensor(faces):
        raise TypeError(f"{what}: faces must be a torch tensor")
    _args.check_face_tensor(what, faces)
    if faces.shape[0] > MAX_COUNT:
        raise ValueError(f"{what}: {faces.shape[0]} faces, more than {MAX_COUNT}")


def unimage(words):
    """float32 values of their order-preserving uint32 images (include/dm4d_mesh_clean.h, ``state``)."""
    k = np.asarray(words, np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def diagonal2(lo, hi):
    """``dx*dx + dy*dy + dz*dz`` in float64 from six float32 bounds."""
    dx, dy, dz = (float(h) - float(l) for l, h in zip(lo, hi))
    return dx * dx + dy * dy + dz * dz


def _components(_lib, st, F, V, faces32, alive, verts, face_count, box, state):
    """Rounds of union-find until the check of ``dm4d_mcl_component_stats`` finds no face with two labels ("Mesh
    cleaning": one round is the rule; every further round strictly lowers a parent).  -> (labels [V] int32, state on the host)."""
    parent = torch.empty(V, dtype=torch.int32, device=faces32.device)
    for rnd in range(MAX_ROUNDS):
        _lib.call("dm4d_mcl_components_round", F, V, faces32.data_ptr(), _lib.ptr(alive), int(rnd == 0), parent.data_ptr(), st)
        _lib.call("dm4d_mcl_component_stats", F, V, _lib.ptr(verts) if box is not None else None, faces32.data_ptr(), _lib.ptr(alive),
                  parent.data_ptr(), face_count.data_ptr(), _lib.ptr(box), state.data_ptr(), st)
        host = state.cpu().numpy().view(np.uint32)
        if not host[_lib.DM4D_MCL_STATE_INCOMPLETE]:
            return parent, host
    raise _lib.Dm4dError(f"connected components: still incomplete after {MAX_ROUNDS} rounds")


def connected_components(faces, n_verts):
    """faces [F,3] int32 / int64 on a HIP device, n_verts the number of vertices -> (labels [n_verts] int32, n_components).

    Two vertices are connected when a face names both; ``labels[v]`` is the smallest vertex index of v's component and
    ``labels[v] = v`` for a vertex no face names; ``n_components`` counts the distinct labels.  Raises ValueError for a face index
    outside [0, n_verts), ``_lib.Dm4dError`` for a CPU tensor."""
    from . import _lib

    what = "connected_components"
    _checked_faces(what, faces)
    if isinstance(n_verts, bool) or not isinstance(n_verts, (int, np.integer)) or not 0 <= n_verts <= MAX_COUNT:
        raise ValueError(f"{what}: n_verts must be an integer in [0, {MAX_COUNT}] (got {n_verts!r})")
    dev = faces.device
    if dev.type != "cuda":
        raise _args.no_cpu_path(what)
    V, F = int(n_verts), int(faces.shape[0])
    with torch.cuda.device(dev):
        if F:
            _args.check_index_range(what, _args.FACE_INDICES, faces, V)
        faces32 = faces.detach().to(torch.int32).contiguous()
        state = torch.zeros(_lib.DM4D_MCL_STATE_WORDS, dtype=torch.int32, device=dev)
        face_count = torch.empty(V, dtype=torch.int32, device=dev)
        labels, host = _components(_lib, _lib.stream(dev), F, V, faces32, None, None, face_count, None, state)
    return labels, int(host[_lib.DM4D_MCL_STATE_N_COMPONENTS])


def clean_mesh(verts, faces, colors=None, min_f=64, min_d=20.0, keep="all"):
    """verts [V,3] float32, faces [F,3] int32 / int64, colors [V,3] float32 or None -- tensors on one HIP device; ``min_f`` a face
    count (0: no test), ``min_d`` a percentage of the mesh diagonal (0: no test), ``keep`` "all" or "largest".  The defaults are
    the reference's.  Steps 1-7 of the module docstring.

    -> dict(verts [V',3] float32, faces [F',3] int64, colors [V',3] float32 or None, vertex_map [V] int64 (the output vertex of
    every input vertex, -1 = dropped), face_map [F'] int64 (the input position of every output face), labels [V] int32 (step 4),
    n_components (distinct labels, orphans and unreferenced vertices included), n_null, n_duplicate (faces removed by steps 2 and
    3), n_small (components with faces that the two tests of step 6 drop; what ``keep="largest"`` drops is not counted)).

    Not restated: ``meshing_merge_close_vertices``, the two non-manifold repairs, isotropic remeshing and ``decimate_mesh``.

    Raises TypeError / ValueError for arguments of the wrong kind, shape, dtype or range (a face index outside [0, V), vertices
    named by a face that are not finite), ``_lib.Dm4dError`` for CPU tensors."""
    from . import _lib

    what = "clean_mesh"
    if not torch.is_tensor(verts) or (colors is not None and not torch.is_tensor(colors)):
        raise TypeError(f"{what}: verts and colors must be torch tensors")
    _checked_faces(what, faces)
    if verts.ndim != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32 or verts.shape[0] > MAX_COUNT:
        raise ValueError(f"{what}: verts must be float32 [V,3] with V <= {MAX_COUNT} (got {verts.dtype} {tuple(verts.shape)})")
    if colors is not None and (colors.shape != verts.shape or colors.dtype != torch.float32):
        raise ValueError(f"{what}: colors must be float32 {tuple(verts.shape)} (got {colors.dtype} {tuple(colors.shape)})")
    if keep not in KEEP_MODES:
        raise ValueError(f"{what}: keep must be one of {KEEP_MODES} (got {keep!r})")
    if isinstance(min_f, bool) or not isinstance(min_f, (int, np.integer)) or not 0 <= min_f <= MAX_COUNT:
        raise ValueError(f"{what}: min_f must be an integer in [0, {MAX_COUNT}] (got {min_f!r})")
    if isinstance(min_d, bool) or not isinstance(min_d, (int, float, np.integer, np.floating)) or not (0 <= min_d and math.isfinite(min_d)):
        raise ValueError(f"{what}: min_d must be a finite number >= 0 (got {min_d!r})")
    dev = verts.device
    if dev.type != "cuda" or faces.device != dev or (colors is not None and colors.device != dev):
        raise _args.no_cpu_path(what)
    V, F = int(verts.shape[0]), int(faces.shape[0])
    min_f, min_d = int(min_f), float(min_d)
    verts = verts.detach().contiguous()
    colors = None if colors is None else colors.detach().contiguous()
    u8, i32, i64 = (dict(dtype=t, device=dev) for t in (torch.uint8, torch.int32, torch.int64))
    with torch.cuda.device(dev):
        st = _lib.stream(dev)
        if F:
            _args.check_index_range(what, _args.FACE_INDICES, faces, V)
        faces32 = faces.detach().to(torch.int32).contiguous()
        state = torch.empty(_lib.DM4D_MCL_STATE_WORDS, **i32)
        null_face, alive = torch.empty(F, **u8), torch.empty(F, **u8)
        key_hi, key_lo = torch.empty(F, **i64), torch.empty(F, **i64)
        _lib.call("dm4d_mcl_face_flags", F, V, verts.data_ptr(), faces32.data_ptr(), null_face.data_ptr(), key_hi.data_ptr(), key_lo.data_ptr(),
                  state.data_ptr(), st)
        # lexicographic order of the sorted triples, equal triples in input order: stable sort by (s1, s2), then by s0
        p1 = torch.sort(key_lo, stable=True).indices
        perm = p1[torch.sort(key_hi[p1], stable=True).indices].contiguous()
        _lib.call("dm4d_mcl_face_first", F, perm.data_ptr(), key_hi.data_ptr(), key_lo.data_ptr(), null_face.data_ptr(), alive.data_ptr(),
                  state.data_ptr(), st)
        face_count, box = torch.empty(V, **i32), torch.empty(V, 6, **i32)
        labels, host = _components(_lib, st, F, V, faces32, alive, verts, face_count, box, state)
        D2 = 0.0
        if F:
            D2 = diagonal2(unimage(host[_lib.DM4D_MCL_STATE_LO:_lib.DM4D_MCL_STATE_LO + 3]), unimage(host[_lib.DM4D_MCL_STATE_HI:_lib.DM4D_MCL_STATE_HI + 3]))
            if not math.isfinite(D2):
                raise ValueError(f"{what}: the vertices the faces name are not all finite")
        thr2 = (min_d / 100.0) ** 2 * D2
        comp_keep, keep_vertex, keep_face = torch.empty(V, **u8), torch.empty(V, **u8), torch.empty(F, **u8)
        _lib.call("dm4d_mcl_keep", F, V, faces32.data_ptr(), alive.data_ptr(), labels.data_ptr(), face_count.data_ptr(), box.data_ptr(), thr2,
                  int(min_d > 0), min_f, int(keep == "largest"), comp_keep.data_ptr(), keep_vertex.data_ptr(), keep_face.data_ptr(),
                  state.data_ptr(), st)
        vert_end = torch.cumsum(keep_vertex, 0, dtype=torch.int64)
        face_end = torch.cumsum(keep_face, 0, dtype=torch.int64)
        zero = torch.zeros(1, **i64)
        totals = torch.cat([vert_end[-1:] if V else zero, face_end[-1:] if F else zero, state.to(torch.int64)]).cpu().tolist()
        Vo, Fo, words = int(totals[0]), int(totals[1]), [int(w) & 0xFFFFFFFF for w in totals[2:]]
        out_verts = torch.empty(Vo, 3, dtype=torch.float32, device=dev)
        out_colors = None if colors is None else torch.empty(Vo, 3, dtype=torch.float32, device=dev)
        out_faces, face_map, vertex_map = torch.empty(Fo, 3, **i64), torch.empty(Fo, **i64), torch.empty(V, **i64)
        _lib.call("dm4d_mcl_compact", F, V, Fo, Vo, verts.data_ptr(), _lib.ptr(colors), faces32.data_ptr(), keep_vertex.data_ptr(), vert_end.data_ptr(),
                  keep_face.data_ptr(), face_end.data_ptr(), out_verts.data_ptr(), _lib.ptr(out_colors), out_faces.data_ptr(), vertex_map.data_ptr(),
                  face_map.data_ptr(), st)
    return {"verts": out_verts, "faces": out_faces, "colors": out_colors, "vertex_map": vertex_map, "face_map": face_map, "labels": labels,
            "n_components": words[_lib.DM4D_MCL_STATE_N_COMPONENTS], "n_null": words[_lib.DM4D_MCL_STATE_N_NULL],
            "n_duplicate": words[_lib.DM4D_MCL_STATE_N_DUPLICATE], "n_small": words[_lib.DM4D_MCL_STATE_N_SMALL]}


def output_path(mesh_path, output):
    """``{output}/{stem}_clean.ply``, stem = the file name up to its first dot."""
    return os.path.join(output, os.path.basename(mesh_path).split(".")[0] + "_clean.ply")


def add_arguments(p):
    """The three options of the cleaning, shared with the isosurface CLI."""
    p.add_argument("--min_f", default=64, type=int, help="drop components with fewer faces (0: keep them)")
    p.add_argument("--min_d", default=20.0, type=float, help="drop components whose diagonal is below this percentage of the mesh's (0: keep them)")
    p.add_argument("--keep", default="all", choices=KEEP_MODES, help="'largest' keeps only the surviving component with the most faces")


def _parser():
    p = argparse.ArgumentParser(prog="python -m dreammesh4d_amd.mesh_clean", description=__doc__.split("\n")[0])
    p.add_argument("--mesh_path", required=True, help="path to input mesh")
    p.add_argument("--output", required=True, help="directory of the output mesh")
    add_arguments(p)
    return p


def main(argv=None):
    from . import wire_formats as wf

    args = _parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise _args.no_cpu_path("mesh_clean")
    mesh = wf.read_mesh(args.mesh_path)
    print(f"Input mesh has {len(mesh['verts'])} vertices and {len(mesh['faces'])} triangles")
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    colors = mesh.get("colors")
    res = clean_mesh(t(mesh["verts"], np.float32), t(mesh["faces"], np.int64), None if colors is None else t(colors, np.float32),
                     min_f=args.min_f, min_d=args.min_d, keep=args.keep)
    print(f"{res['n_null']} null and {res['n_duplicate']} duplicate faces, {res['n_components']} components, {res['n_small']} of them small")
    print(f"Cleaned mesh has {len(res['verts'])} vertices and {len(res['faces'])} triangles")
    os.makedirs(args.output, exist_ok=True)
    path = output_path(args.mesh_path, args.output)
    wf.write_ply(path, res["verts"].cpu().numpy(), res["faces"].cpu().numpy(), colors=None if res["colors"] is None else res["colors"].cpu().numpy())
    return path


if __name__ == "__main__":
    main()
