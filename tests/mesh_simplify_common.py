"""Shared by tests/test_mesh_simplify_cpu.py and tests/test_mesh_simplify_gpu.py: a numpy float64 restatement of the
vertex-clustering semantics (written from their statement, not from open3d) and the scenes the device is compared on.

Semantics.  lo, hi = per-axis min / max of the float32 vertices.  voxel = max(hi - lo) / scale, origin = lo - voxel / 2,
cell = floor((v - origin) / voxel) per axis, grid n = floor((hi - origin) / voxel) + 1 per axis, key = (iz ny + iy) nx + ix --
float64 and int64 throughout.  Output vertex c is the cluster with the c-th smallest key; its position (colour) is the sum of
its members in float64 IN ASCENDING VERTEX INDEX, divided by their number in float64, rounded once to float32.  A face is mapped
corner by corner to cluster ids, dropped when two ids are equal, rotated (not sorted) so that its smallest id comes first,
dropped when an earlier face gave the same triple; the survivors keep their input order.

The sums use np.add.at, which applies its additions one at a time in index order; np.sum adds pairwise and would differ from a
serial sum in the last bit.  ``serial_means`` is the same thing as an explicit loop (small inputs only)."""
import numpy as np


def simplify_reference(verts, faces, colors=None, scale=64, voxel_size=None):
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    voxel = float(np.max(hi - lo)) / int(scale) if voxel_size is None else float(voxel_size)
    assert voxel > 0.0
    origin = lo - 0.5 * voxel
    cell = np.floor((v - origin) / voxel).astype(np.int64)
    n = np.floor((hi - origin) / voxel).astype(np.int64) + 1
    assert int(n[0]) * int(n[1]) * int(n[2]) < 2 ** 62
    key = (cell[:, 2] * n[1] + cell[:, 1]) * n[0] + cell[:, 0]
    _, vc = np.unique(key, return_inverse=True)                  # cluster ids in ascending key order
    vc = vc.reshape(-1).astype(np.int64)
    C = int(vc.max()) + 1
    count = np.bincount(vc, minlength=C)

    def means(x):
        s = np.zeros((C, 3), np.float64)
        np.add.at(s, vc, x)                                      # one addition at a time, in ascending vertex index
        return (s / count[:, None].astype(np.float64)).astype(np.float32)

    out = {"verts": means(v), "colors": None if colors is None else means(np.asarray(colors, np.float32).astype(np.float64)),
           "vertex_cluster": vc, "voxel_size": voxel, "origin": origin, "grid": tuple(int(x) for x in n), "n_vertices": C,
           "max_cluster_size": int(count.max())}
    t = vc[f]
    degenerate = (t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 0] == t[:, 2])
    k = np.argmin(t, axis=1)                                     # unique for a face that is not degenerate
    rot = np.take_along_axis(t, (k[:, None] + np.arange(3)[None]) % 3, axis=1)
    alive = np.nonzero(~degenerate)[0]
    if len(alive):
        _, first = np.unique(rot[alive], axis=0, return_index=True)      # index of the FIRST occurrence of every distinct triple
        kept = np.sort(alive[first])
    else:
        kept = alive
    out.update(faces=rot[kept], n_faces=len(kept), n_degenerate=int(degenerate.sum()), n_duplicate=len(alive) - len(kept))
    return out


def serial_means(values, vertex_cluster, n_clusters):
    """The cluster means as an explicit serial loop in vertex order (float64 sum, one division, one rounding)."""
    s = np.zeros((n_clusters, values.shape[1]), np.float64)
    cnt = np.zeros(n_clusters, np.int64)
    x = np.asarray(values, np.float32).astype(np.float64)
    for i, c in enumerate(vertex_cluster):
        s[c] = s[c] + x[i]
        cnt[c] += 1
    return (s / cnt[:, None].astype(np.float64)).astype(np.float32)


def opposite_pairs(faces):
    """Number of faces (a, b, c) of a canonical face list whose mirror image (a, c, b) is in the list too."""
    have = {tuple(r) for r in np.asarray(faces).tolist()}
    return sum((a, c, b) in have for a, b, c in have)


# ------------------------------------------------------------------------------------------------------------ scenes
def with_branch_faces(verts, faces):
    """Appends four faces (no vertices: the bounds and the grid stay what they were) that take every branch of the face stage
    whatever the clustering does to the rest of the mesh.  p, q, r = the vertices with the smallest, the largest and the most
    central coordinate along the axis of largest extent: for every scale >= 2 they lie in three different cells (cells 0, scale
    and one strictly between), so (p, q, r) survives.  Appended: (p, q, r); its rotation (q, r, p), a duplicate once rotated back,
    to be removed; its mirror image (p, r, q), same vertices in the opposite orientation, to be KEPT; and (p, p, q), which
    collapses under every clustering."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ax = int(np.argmax(v.max(axis=0) - v.min(axis=0)))
    x = v[:, ax]
    p, q, r = int(np.argmin(x)), int(np.argmax(x)), int(np.argmin(np.abs(x - 0.5 * (x.min() + x.max()))))
    return np.concatenate([f, np.array([[p, q, r], [q, r, p], [p, r, q], [p, p, q]], np.int64)])


def sphere_scene(n_faces=40_000):
    """The sphere of synthetic.mesh_bound_scene (a closed UV sphere: its pole fans fall into few cells)."""
    from dreammesh4d_amd import synthetic as syn

    sc = syn.mesh_bound_scene(n_faces, n_nodes=16, k=4, seed=0)
    return np.asarray(sc["verts"], np.float32), with_branch_faces(sc["verts"], sc["faces"]), None


def grid_scene(n=33, extent=8.0):
    """n x n vertices at multiples of extent / (n - 1) over [0, extent]^2, heights on a coarse lattice: with extent 8, n = 33 and
    scale 4 the cells are 2 wide from origin -1, so every vertex with an odd integer coordinate lies EXACTLY on a cell boundary
    (and goes to the upper cell: floor).  All coordinates are small dyadic rationals, exact in float32."""
    h = extent / (n - 1)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    z = 0.5 * ((i * 7 + j * 3) % 5)                                     # 0, 0.5, ..., 2: folds the sheet inside the cells
    verts = np.stack([i * h, j * h, z], -1).reshape(-1, 3).astype(np.float32)
    a = (i[:-1, :-1] * n + j[:-1, :-1]).reshape(-1)
    faces = np.concatenate([np.stack([a, a + n, a + n + 1], 1), np.stack([a, a + n + 1, a + 1], 1)])
    return verts, with_branch_faces(verts, faces), None


def colored_scene(n_faces=30_000, seed=1):
    """A bumpy sphere (radial noise, so that cells cut the surface irregularly) with random vertex colours."""
    from dreammesh4d_amd import synthetic as syn

    rng = np.random.default_rng(seed)
    v, f = syn.uv_sphere(n_faces, radius=0.6)
    v = np.asarray(v, np.float64)
    v = (v * (1.0 + 0.05 * rng.normal(size=(len(v), 1)))).astype(np.float32)
    return v, with_branch_faces(v, f), rng.random((len(v), 3)).astype(np.float32)


def crowded_scene(n_faces=120_000):
    """A sphere dense enough that at scale 2 single cells hold far more than 4096 vertices (64 chunks of the wave-per-cluster
    average kernel and more)."""
    from dreammesh4d_amd import synthetic as syn

    v, f = syn.uv_sphere(n_faces, radius=0.6)
    v = np.asarray(v, np.float32)
    return v, with_branch_faces(v, f), None


def million_scene(seed=2):
    """About a million vertices: the size of a dense coarse mesh before simplification."""
    from dreammesh4d_amd import synthetic as syn

    rng = np.random.default_rng(seed)
    v, f = syn.uv_sphere(2_000_000, radius=0.6)
    v = np.asarray(v, np.float64)
    v = (v * (1.0 + 0.01 * rng.normal(size=(len(v), 1)))).astype(np.float32)
    return v, with_branch_faces(v, f), rng.random((len(v), 3)).astype(np.float32)


# name -> (builder, scale)
SCENES = {
    "sphere_scale8": (sphere_scene, 8),
    "sphere_scale16": (sphere_scene, 16),
    "sphere_scale64": (sphere_scene, 64),
    "grid_on_boundaries": (grid_scene, 4),
    "colored": (colored_scene, 24),
    "crowded_cell": (crowded_scene, 2),
    "million_scale128": (million_scene, 128),
}


def check_branches(ref, n_input_verts):
    """Every branch is taken on this scene, judged on the restatement alone."""
    assert 1 < ref["n_vertices"] < n_input_verts, (ref["n_vertices"], n_input_verts)
    assert ref["n_degenerate"] >= 1 and ref["n_duplicate"] >= 1, (ref["n_degenerate"], ref["n_duplicate"])
    assert opposite_pairs(ref["faces"]) >= 2, "no opposite-orientation pair survived"
