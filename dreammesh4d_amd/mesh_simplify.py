"""Mesh simplification by vertex clustering on the HIP device: the step between the coarse mesh and the static refine stage.

Replaces ``custom/threestudio-dreammesh4d/scripts/mesh_simplification.py`` (open3d's
``TriangleMesh.simplify_vertex_clustering(voxel_size, contraction=Average)``, CPU) with the kernels of
``csrc/mesh_simplify.hip``.  open3d numbers clusters and faces in the iteration order of its hash maps; here the result is a
function of the input alone ("Mesh simplification"):

* ``lo, hi`` = per-axis min / max of the float32 vertices; ``voxel = max(hi - lo) / scale`` (or ``voxel_size``),
  ``origin = lo - voxel / 2``, the cell of a vertex ``floor((v - origin) / voxel)`` per axis, the grid
  ``n = floor((hi - origin) / voxel) + 1`` per axis, ``key = (iz * ny + iy) * nx + ix`` -- all in float64 / int64;
* output vertex ``c`` is the cluster with the c-th smallest key: the float64 sum of its members in ascending vertex index,
  divided by their number in float64, rounded once to float32 (colours likewise);
* a face is mapped corner by corner, dropped when two corners share a cluster, rotated (not sorted) to start at its
  smallest id, and dropped when the same triple occurred earlier; surviving faces keep their input order.

The two stable sorts, the run boundaries and the compactions are torch calls on the device; everything else is HIP.  There is
no CPU path.  Vertex normals are not carried: the loader of the bind mesh (``threestudio_host._load_mesh``) does not read them.

    python -m dreammesh4d_amd.mesh_simplify --mesh_path coarse.ply --scale 64 --output out_dir
"""
import argparse
import math
import os

import numpy as np
import torch

from . import _args

KEY_BITS = 62


def _checked_scale(scale):
    if isinstance(scale, bool) or not isinstance(scale, (int, np.integer)) or scale <= 0:
        raise ValueError(f"simplify_vertex_clustering: scale must be an integer greater than 0 (got {scale!r})")
    return int(scale)


def grid_parameters(lo, hi, scale=64, voxel_size=None):
    """Host side of the semantics, in float64: (voxel, origin [3], (nx, ny, nz)) from the per-axis bounds.  Raises ValueError for
    ``scale <= 0``, a mesh without extent (``voxel == 0``), non-finite bounds, and a grid whose keys need more than 62 bits."""
    lo = [float(x) for x in lo]
    hi = [float(x) for x in hi]
    if not all(math.isfinite(x) for x in lo + hi):
        raise ValueError("simplify_vertex_clustering: the vertices are not all finite")
    if voxel_size is None:
        voxel = max(h - l for l, h in zip(lo, hi)) / _checked_scale(scale)
    else:
        voxel = float(voxel_size)
        if not (voxel > 0.0 and math.isfinite(voxel)):
            raise ValueError(f"simplify_vertex_clustering: voxel_size must be positive and finite (got {voxel_size!r})")
    if voxel == 0.0:
        raise ValueError("simplify_vertex_clustering: degenerate mesh, all vertices coincide (voxel size 0)")
    origin = [l - 0.5 * voxel for l in lo]
    cells = [(h - o) / voxel for h, o in zip(hi, origin)]
    dims = tuple(int(math.floor(q)) + 1 if math.isfinite(q) else 1 << KEY_BITS for q in cells)
    if dims[0] * dims[1] * dims[2] >= 1 << KEY_BITS:
        raise ValueError(f"simplify_vertex_clustering: the cell keys of a {cells[0]:.6g} x {cells[1]:.6g} x {cells[2]:.6g} grid do not "
                         f"fit in {KEY_BITS} bits (voxel size {voxel:e})")
    return voxel, origin, dims


def check_face_range(fmin, fmax, n_verts):
    """Raises ValueError unless every face index lies in [0, n_verts)."""
    _args.check_span("simplify_vertex_clustering", _args.FACE_INDICES, fmin, fmax, n_verts)


def simplify_vertex_clustering(verts, faces, colors=None, scale=64, voxel_size=None):
    """verts [V,3] float32, faces [F,3] int32 / int64, colors [V,3] float32 or None -- tensors on one HIP device.

    -> dict(verts [C,3] float32, faces [F',3] int64, colors [C,3] float32 or None, vertex_cluster [V] int64 (the output vertex
    every input vertex went to), voxel_size, origin, grid (host floats / ints), n_vertices, n_faces, n_degenerate (faces dropped
    because two corners share a cluster), n_duplicate (faces dropped because the same triple occurred earlier))."""
    from . import _lib

    if not torch.is_tensor(verts) or not torch.is_tensor(faces) or (colors is not None and not torch.is_tensor(colors)):
        raise TypeError("simplify_vertex_clustering: verts, faces and colors must be torch tensors")
    if verts.ndim != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32 or verts.shape[0] == 0:
        raise ValueError(f"simplify_vertex_clustering: verts must be float32 [V,3] with V > 0 (got {verts.dtype} {tuple(verts.shape)})")
    _args.check_face_tensor("simplify_vertex_clustering", faces)
    if colors is not None and (colors.shape != verts.shape or colors.dtype != torch.float32):
        raise ValueError(f"simplify_vertex_clustering: colors must be float32 {tuple(verts.shape)} (got {colors.dtype} {tuple(colors.shape)})")
    if voxel_size is None:
        _checked_scale(scale)
    dev = verts.device
    if dev.type != "cuda" or faces.device != dev or (colors is not None and colors.device != dev):
        raise RuntimeError("simplify_vertex_clustering: tensors must live on one HIP device; there is no CPU path")
    V, F = int(verts.shape[0]), int(faces.shape[0])
    verts = verts.detach().contiguous()
    faces = faces.detach().to(torch.int64).contiguous()
    colors = None if colors is None else colors.detach().contiguous()
    i64 = dict(dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        st = _lib.stream(dev)
        # the only values that visit the host: six bounds, the two extreme face indices, and the counts
        bounds = torch.cat([verts.amin(0), verts.amax(0)]).double().cpu().tolist()
        if F:
            _args.check_index_range("simplify_vertex_clustering", _args.FACE_INDICES, faces, V)
        voxel, origin, dims = grid_parameters(bounds[:3], bounds[3:], scale, voxel_size)
        keys = torch.empty(V, **i64)
        _lib.call("dm4d_simplify_vertex_keys", V, verts.data_ptr(), origin[0], origin[1], origin[2], voxel, dims[0], dims[1], dims[2],
                  keys.data_ptr(), st)
        sorted_keys, order = torch.sort(keys, stable=True)
        head = torch.ones(V, dtype=torch.bool, device=dev)
        head[1:] = sorted_keys[1:] != sorted_keys[:-1]
        run_start = head.nonzero().flatten()
        C = int(run_start.shape[0])
        out_verts = torch.empty(C, 3, dtype=torch.float32, device=dev)
        out_colors = None if colors is None else torch.empty(C, 3, dtype=torch.float32, device=dev)
        vertex_cluster = torch.empty(V, **i64)
        _lib.call("dm4d_simplify_cluster_average", V, C, order.data_ptr(), run_start.data_ptr(), verts.data_ptr(),
                  None if colors is None else colors.data_ptr(), out_verts.data_ptr(), None if colors is None else out_colors.data_ptr(),
                  vertex_cluster.data_ptr(), st)
        canon = torch.empty(F, 3, **i64)
        key_bc = torch.empty(F, **i64)
        _lib.call("dm4d_simplify_face_remap", F, V, C, faces.data_ptr(), vertex_cluster.data_ptr(), canon.data_ptr(), key_bc.data_ptr(), st)
        # lexicographic order of the triples, equal triples in input order: stable sort by (b, c), then by a
        p1 = torch.sort(key_bc, stable=True).indices
        perm = p1[torch.sort(canon[:, 0][p1], stable=True).indices].contiguous()
        keep = torch.zeros(F, dtype=torch.uint8, device=dev)
        _lib.call("dm4d_simplify_face_first", F, perm.data_ptr(), canon.data_ptr(), keep.data_ptr(), st)
        kept = keep.nonzero().flatten()                     # ascending: the input order of the first occurrences
        out_faces = canon[kept]
        n_degenerate = int((canon[:, 0] < 0).sum())
    n_faces = int(out_faces.shape[0])
    return {"verts": out_verts, "faces": out_faces, "colors": out_colors, "vertex_cluster": vertex_cluster, "voxel_size": voxel,
            "origin": origin, "grid": dims, "n_vertices": C, "n_faces": n_faces, "n_degenerate": n_degenerate,
            "n_duplicate": F - n_degenerate - n_faces}


def output_path(mesh_path, scale, n_vertices, output):
    """``{output}/{stem}_{scale}_{n_vertices}.ply``, stem = the file name up to its first dot (the reference script's name)."""
    stem = os.path.basename(mesh_path).split(".")[0]
    return os.path.join(output, f"{stem}_{scale}_{n_vertices}.ply")


def _parser():
    p = argparse.ArgumentParser(prog="python -m dreammesh4d_amd.mesh_simplify", description=__doc__.split("\n")[0])
    p.add_argument("--mesh_path", required=True, help="path to input mesh")
    p.add_argument("--scale", default=64, type=int, help="large value for more vertices in simplification model")
    p.add_argument("--output", required=True, help="path to output mesh")
    return p


def main(argv=None):
    from . import wire_formats as wf

    args = _parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("mesh_simplify: no HIP device; there is no CPU path")
    mesh = wf.read_mesh(args.mesh_path)
    print(f"Input mesh has {len(mesh['verts'])} vertices and {len(mesh['faces'])} triangles")
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    colors = mesh.get("colors")
    res = simplify_vertex_clustering(t(mesh["verts"], np.float32), t(mesh["faces"], np.int64),
                                     None if colors is None else t(colors, np.float32), scale=args.scale)
    print(f"voxel_size = {res['voxel_size']:e}")
    print(f"Simplified mesh has {res['n_vertices']} vertices and {res['n_faces']} triangles")
    os.makedirs(args.output, exist_ok=True)
    path = output_path(args.mesh_path, args.scale, res["n_vertices"], args.output)
    wf.write_ply(path, res["verts"].cpu().numpy(), res["faces"].cpu().numpy(),
                 colors=None if res["colors"] is None else res["colors"].cpu().numpy())
    return path


if __name__ == "__main__":
    main()
