"""What the mesh-cleaning tests share: a numpy restatement of steps 1-7 of dreammesh4d_amd/mesh_clean.py (components through
scipy.sparse.csgraph, mapped to the smallest index per label), an independent pure-Python BFS, and the case builders."""
import numpy as np

FIELDS = ("verts", "faces", "colors", "vertex_map", "face_map", "labels", "n_components", "n_null", "n_duplicate", "n_small")


# ------------------------------------------------------------------------------------------------------ the restatement
def labels_scipy(faces, n_verts):
    """(labels [V] int32, n_components): one-ring graph of `faces`, every label the smallest vertex index of its component."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components

    V = int(n_verts)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    if V == 0:
        return np.zeros(0, np.int32), 0
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    g = sp.coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(V, V))
    n, lab = connected_components(g, directed=False)
    mins = np.full(n, V, np.int64)
    np.minimum.at(mins, lab, np.arange(V))
    return mins[lab].astype(np.int32), int(n)


def labels_bfs(faces, n_verts):
    """The same labels by a breadth-first search over adjacency lists: seeds in ascending index, so a seed is its component's
    smallest vertex."""
    adj = [[] for _ in range(n_verts)]
    for a, b, c in np.asarray(faces, np.int64).reshape(-1, 3).tolist():
        adj[a] += [b, c]
        adj[b] += [a, c]
        adj[c] += [a, b]
    lab = [-1] * n_verts
    for s in range(n_verts):
        if lab[s] >= 0:
            continue
        lab[s] = s
        queue = [s]
        while queue:
            nxt = []
            for v in queue:
                for w in adj[v]:
                    if lab[w] < 0:
                        lab[w] = s
                        nxt.append(w)
            queue = nxt
    return np.asarray(lab, np.int32).reshape(n_verts)


def diagonal2(lo, hi):
    d = np.asarray(hi, np.float32).astype(np.float64) - np.asarray(lo, np.float32).astype(np.float64)
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def restate(verts, faces, colors=None, min_f=64, min_d=20.0, keep="all"):
    """Steps 1-7 in numpy -> the dict of ``clean_mesh`` plus what the tests look at: alive, face_count, d2 (per label), D2, kept
    (per label)."""
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    V, F = len(verts), len(faces)
    # 1
    D2 = float(diagonal2(verts[faces.ravel()].min(0), verts[faces.ravel()].max(0))) if F else 0.0
    # 2
    a, b, c = faces[:, 0], faces[:, 1], faces[:, 2]
    p = verts.astype(np.float64)
    u, w = p[b] - p[a], p[c] - p[a]
    nx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
    ny = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
    nz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    null = (a == b) | (b == c) | (a == c) | ((nx == 0) & (ny == 0) & (nz == 0))
    # 3
    alive = np.zeros(F, bool)
    live = np.nonzero(~null)[0]
    if len(live):
        first = np.unique(np.sort(faces[live], 1), axis=0, return_index=True)[1]
        alive[live[first]] = True
    # 4
    labels, n_components = labels_scipy(faces[alive], V)
    # 5
    face_count = np.bincount(labels[faces[alive, 0]], minlength=V).astype(np.int64) if V else np.zeros(0, np.int64)
    blo, bhi = np.full((V, 3), np.inf, np.float32), np.full((V, 3), -np.inf, np.float32)
    np.minimum.at(blo, labels, verts)
    np.maximum.at(bhi, labels, verts)
    has = face_count > 0
    d2 = np.where(has, diagonal2(np.where(has[:, None], blo, 0), np.where(has[:, None], bhi, 0)), 0.0)
    # 6
    thr2 = (float(min_d) / 100.0) ** 2 * D2
    small_d = has & (min_d > 0) & (d2 < thr2)
    small_f = has & ~small_d & (min_f > 0) & (face_count < min_f)
    kept = has & ~small_d & ~small_f
    n_small = int((small_d | small_f).sum())
    if keep == "largest" and kept.any():
        best = max(np.nonzero(kept)[0].tolist(), key=lambda l: (face_count[l], -l))
        kept = np.zeros(V, bool)
        kept[best] = True
    # 7
    keep_face = alive & kept[labels[faces[:, 0]]] if F else np.zeros(0, bool)
    keep_vertex = kept[labels] if V else np.zeros(0, bool)
    vertex_map = np.where(keep_vertex, np.cumsum(keep_vertex) - 1, -1).astype(np.int64)
    face_map = np.nonzero(keep_face)[0].astype(np.int64)
    return {"verts": verts[keep_vertex], "faces": vertex_map[faces[keep_face]].reshape(-1, 3), "colors": None if colors is None else
            np.ascontiguousarray(colors, np.float32)[keep_vertex], "vertex_map": vertex_map, "face_map": face_map, "labels": labels,
            "n_components": n_components, "n_null": int(null.sum()), "n_duplicate": int((~null).sum() - alive.sum()), "n_small": n_small,
            "alive": alive, "face_count": face_count, "d2": d2, "D2": D2, "kept": kept}


def differences(got, want):
    """Names of the fields of ``clean_mesh``'s dict (numpy values) that differ from the restatement's, bit for bit."""
    bad = []
    for k in FIELDS:
        g, w = got[k], want[k]
        if w is None or g is None:
            same = g is None and w is None
        elif isinstance(w, np.ndarray):
            g = np.asarray(g)
            same = g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()
        else:
            same = int(g) == int(w)
        if not same:
            bad.append(k)
    return bad


# ------------------------------------------------------------------------------------------------- component cases (faces only)
def strip_faces(n_tris):
    i = np.arange(n_tris, dtype=np.int64)
    return np.stack([i, i + 1, i + 2], 1)


def renumbered(faces, n_verts, order, seed=0):
    """The faces with vertex i renamed: "ascending" keeps it, "descending" reverses, "random" permutes (fixed seed)."""
    new = {"ascending": np.arange(n_verts), "descending": np.arange(n_verts)[::-1],
           "random": np.random.default_rng(seed).permutation(n_verts)}[order].astype(np.int64)
    return new[faces]


TET = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int64)
OCTA = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int64)


def component_cases():
    """name -> (faces [F,3] int64, V)."""
    cases = {"empty V=0": (np.zeros((0, 3), np.int64), 0), "empty V=5": (np.zeros((0, 3), np.int64), 5),
             "one triangle": (np.array([[2, 0, 1]], np.int64), 3)}
    for V in (65, 4097):                                               # no multiple of 64 or 256: three strips and a few loose vertices
        third = (V - 5) // 3
        parts = [strip_faces(third - 2) + k * third for k in range(3)]
        cases[f"{V} vertices"] = (renumbered(np.concatenate(parts), V, "random", seed=V), V)
    for order in ("ascending", "descending", "random"):
        cases[f"strip 4096 {order}"] = (renumbered(strip_faces(4096), 4098, order, seed=1), 4098)
    n = 1000
    cases["1000 tetrahedra interleaved"] = ((TET[None] * n + np.arange(n)[:, None, None]).reshape(-1, 3), 4 * n)
    second = OCTA + 5
    cases["two blobs share a vertex"] = (np.concatenate([OCTA, second]), 11)         # vertex 5 is in both
    cases["isolated between used"] = (strip_faces(200) * 3 + 1, 3 * 202)
    F = 3000                                                           # a dozen workgroups, all on the same two hubs
    third = np.arange(F, dtype=np.int64)
    cases["hubs low"] = (np.stack([np.zeros(F, np.int64), np.ones(F, np.int64), third + 2], 1), F + 2)
    cases["hubs high"] = (np.stack([np.full(F, F + 1), np.full(F, F), third], 1), F + 2)
    return cases


# ------------------------------------------------------------------------------------------------------ mesh cases
def strip_mesh(n_tris, origin=(0.0, 0.0, 0.0), step=0.5):
    """A zigzag strip of n_tris triangles in the plane z = origin z: n_tris + 2 vertices, `step` apart along x."""
    i = np.arange(n_tris + 2)
    v = np.stack([i * step * 0.5, (i % 2) * step, np.zeros(len(i))], 1) + np.asarray(origin)
    return v.astype(np.float32), strip_faces(n_tris)


def compose(parts, extra_verts=(), extra_faces=(), seed=0, shuffle=True):
    """Meshes side by side, then `extra_verts` (indices continue) and `extra_faces` (global indices); vertices and faces randomly
    renumbered / reordered when `shuffle`.  -> verts, faces, colors."""
    vs, fs, base = [], [], 0
    for v, f in parts:
        vs.append(v)
        fs.append(f + base)
        base += len(v)
    verts = np.concatenate(vs + [np.asarray(extra_verts, np.float32).reshape(-1, 3)]).astype(np.float32)
    faces = np.concatenate(fs + [np.asarray(extra_faces, np.int64).reshape(-1, 3)])
    rng = np.random.default_rng(seed)
    if shuffle:
        new = rng.permutation(len(verts))
        out = np.empty_like(verts)
        out[new] = verts
        verts, faces = out, new[faces][rng.permutation(len(faces))]
    return verts, faces, rng.uniform(0, 1, verts.shape).astype(np.float32)


PERMS6 = [(0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2)]


def zoo(shuffle=True):
    """One long strip of 300 faces (it sets the mesh diagonal), around it: 100 faces in a tiny strip (many faces, small), 10 faces
    in a long one (few faces, large), 5 tiny, strips of exactly 64 and 63 faces, a face in all six index orders, null faces of the
    three kinds and one almost-null face, a component made of null faces only, and vertices no face names."""
    parts = [strip_mesh(300, (0, 0, 0), 0.5), strip_mesh(100, (5, 20, 1), 0.001), strip_mesh(10, (0, 40, 2), 8.0),
             strip_mesh(5, (30, 20, 3), 0.001), strip_mesh(64, (0, 60, 4), 2.0), strip_mesh(63, (0, 80, 5), 2.0)]
    n = sum(len(v) for v, _ in parts)
    ev = [[0, 100, 0], [1, 101, 1], [2, 102, 2],                       # n .. n+2: collinear
          [7, 100, 0], [7, 100, 0], [8, 100, 0],                       # n+3, n+4 coincide
          [0, 0, -10], [1, 0, -10], [2, 1e-30, -10],                   # n+6 .. n+8: cross product (0, 0, 1e-30), not null
          [0, 120, 0], [1, 120, 0], [2, 120 + 1e-3, 0],                # n+9 .. n+11: a sliver, not null
          [50, 50, 50], [51, 51, 51]]                                  # n+12, n+13: never named
    ef = [[n, n + 1, n + 2], [n + 3, n + 4, n + 5], [n + 6, n + 7, n + 8], [n + 9, n + 10, n + 11], [5, 5, 6], [7, 8, 7]]
    ef += [[(3, 4, 5)[i] for i in p] for p in PERMS6] + [[12, 11, 10], [10, 11, 12]]
    return compose(parts, ev, ef, seed=3, shuffle=shuffle)


def tie():
    """Strips of 80, 80 and 70 faces, renumbered: `keep="largest"` has to break a tie by label."""
    return compose([strip_mesh(80, (0, 0, 0)), strip_mesh(70, (0, 5, 0)), strip_mesh(80, (0, 10, 0))], seed=5)


def clean_cases():
    """name -> (verts, faces, colors or None, kwargs of clean_mesh)."""
    zv, zf, zc = zoo()
    tv, tf, tc = tie()
    ov, of_, oc = compose([strip_mesh(64, (0, 0, 0)), strip_mesh(63, (0, 5, 0))], seed=7)
    return {
        "zoo defaults": (zv, zf, zc, {}),
        "zoo nothing small": (zv, zf, zc, dict(min_f=0, min_d=0)),
        "zoo min_f alone": (zv, zf, zc, dict(min_f=64, min_d=0)),
        "zoo min_d alone": (zv, zf, zc, dict(min_f=0, min_d=20.0)),
        "zoo both, largest": (zv, zf, zc, dict(min_f=11, min_d=5.0, keep="largest")),
        "zoo no colours": (zv, zf, None, dict(min_f=64, min_d=1.0)),
        "zoo int32 faces in order": zoo(shuffle=False)[:2] + (None, dict(min_f=6, min_d=0.5)),
        "64 and 63 faces": (ov, of_, oc, dict(min_f=64, min_d=0)),
        "tie all": (tv, tf, tc, dict(min_f=64, min_d=0)),
        "tie largest": (tv, tf, tc, dict(min_f=64, min_d=0, keep="largest")),
        "all dropped, largest": (tv, tf, tc, dict(min_f=100, min_d=0, keep="largest")),
        "no faces": (zv, np.zeros((0, 3), np.int64), zc, {}),
        "nothing": (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), None, {}),
    }


# ------------------------------------------------------------------------------------------------- blob plus floaters
BALLS = [((13.2, 16.1, 15.7), 9.3), ((27.3, 5.2, 5.4), 2.1), ((27.1, 26.6, 5.3), 2.2), ((26.8, 5.4, 26.9), 2.0), ((27.2, 27.1, 26.7), 2.3),
         ((4.3, 4.4, 27.6), 2.1), ((27.4, 16.2, 16.3), 1.9)]


def blob_field(R=32):
    """occ [R,R,R] float32: max over the balls of ``radius - distance`` (index coordinates of R = 32, scaled with R); the surface
    is the level 0.  One large ball and six of about 2 voxels radius, apart from each other."""
    s = R / 32.0
    ax = np.arange(R, dtype=np.float64)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    occ = np.full((R, R, R), -np.inf)
    for (cx, cy, cz), r in BALLS:
        occ = np.maximum(occ, r * s - np.sqrt((x - cx * s) ** 2 + (y - cy * s) ** 2 + (z - cz * s) ** 2))
    return occ.astype(np.float32)
