"""Pins the float64 reference, the cases and the bounds that tests/test_mesh_reg_edges_gpu.py judges the mesh regularisers by
(CPU only, no library call).

* The closed-form reference (tests/mesh_reg_edges.py: scatters over edges and pairs, no autograd) against float64 autograd
  through oracle/mesh_reg.py on every case, values and every gradient element within 1e-12 max(1, |ref|): the ARAP energy summed
  per source vertex, the normal-consistency term of every pair (the oracle on the pair's two faces), the Laplacian (the
  oracle's total, and a dense L v for the per-vertex view); the degenerate pairs and the zero-norm vertex included.  The
  quaternion reference against the float64 CPU path of ops.quat_xyzw_to_matrix.
* The case list covers what the kernels branch on, and float32 and float64 take the same branches.
* The yardsticks still cover the float32 restatement and are not padded: 0.8 x constant <= measured <= constant.
* The host tables of MeshNormalConsistency and ARAPCoach against a brute-force restatement, the coach's float32 cotangent
  weights against the float64 ones the cases carry.
"""
import numpy as np
import pytest
import torch

from oracle import mesh_reg as M
from tests import mesh_reg_edges as ec

BY_KIND = {k: [c.name for c in ec.CASES if c.kind == k] for k in ec.KINDS}


def _close(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    bad = np.abs(got - want) > 1e-12 * np.maximum(1.0, np.abs(want))
    assert not bad.any(), f"{what}: {int(bad.sum())} elements, worst {np.abs(got - want).max():.3g}"


@pytest.mark.parametrize("name", BY_KIND["arap"])
def test_arap_reference_equals_float64_autograd_through_the_oracle(name):
    case, inp, ref = ec.CASE_BY_NAME[name], ec.case_inputs(name), ec.case_reference(name)
    csr = ec.host_tables(case.mesh)["csr"]
    V = len(csr.off) - 1
    src = np.repeat(np.arange(V), np.diff(csr.off))
    x = torch.tensor(inp["x"], dtype=torch.float64, requires_grad=True)
    R = torch.tensor(inp["R"], dtype=torch.float64, requires_grad=True)
    adj = {"src": src, "nbr": csr.nbr, "w": csr.w, "e": csr.e}
    total = sum(float(g) * M.arap_energy(adj, x[t], R[t]) for t, g in enumerate(inp["g"]))
    total.backward()
    _close(ref["arap_g_xyz"].v, x.grad.numpy(), "g_xyz")
    _close(ref["arap_g_rot"].v, R.grad.numpy(), "g_rot")
    per_vertex = np.zeros((case.T, V))
    with torch.no_grad():
        for i in range(V):
            k = slice(int(csr.off[i]), int(csr.off[i + 1]))
            own = {"src": src[k], "nbr": csr.nbr[k], "w": csr.w[k], "e": csr.e[k]}
            per_vertex[:, i] = [float(M.arap_energy(own, x[t], R[t])) for t in range(case.T)]
    _close(ref["arap_energy"].v, per_vertex, "vertex energy")


@pytest.mark.parametrize("name", BY_KIND["nc"])
def test_normal_consistency_reference_equals_float64_autograd_through_the_oracle(name):
    case, inp, ref = ec.CASE_BY_NAME[name], ec.case_inputs(name), ec.case_reference(name)
    tab = ec.host_tables(case.mesh)
    x = torch.tensor(inp["x"], dtype=torch.float64, requires_grad=True)
    total = sum(float(g) * M.normal_consistency(x[t:t + 1], tab["faces"]) for t, g in enumerate(inp["g"]))
    total.backward()
    _close(ref["nc_grad"].v, x.grad.numpy(), "g_xyz")
    terms = np.zeros((case.T, len(tab["pairs"])))
    with torch.no_grad():
        for p, (v0, v1, a, b) in enumerate(tab["pairs"].tolist()):
            # (a face listed twice pairs up on all three of its edges: three times the same two normals, their mean)
            mine = M.normal_consistency_pairs([(v0, v1, a), (v1, v0, b)]).tolist()
            assert [v0, v1, a, b] in mine and len(mine) == (3 if a == b else 1)
            terms[:, p] = [float(M.normal_consistency(x[t:t + 1], [(v0, v1, a), (v1, v0, b)])) for t in range(case.T)]
    _close(ref["nc_term"].v, terms, "terms")
    assert np.isfinite(ref["nc_grad"].v).all()


@pytest.mark.parametrize("name", BY_KIND["lap"])
def test_laplacian_reference_equals_float64_autograd_through_the_oracle(name):
    case, inp, ref = ec.CASE_BY_NAME[name], ec.case_inputs(name), ec.case_reference(name)
    tab = ec.host_tables(case.mesh)
    V = len(tab["verts"])
    x = torch.tensor(inp["x"], dtype=torch.float64, requires_grad=True)
    faces = tab["faces"] if len(tab["faces"]) else np.zeros((0, 3), np.int64)
    losses = [M.laplacian_smoothing(x[t:t + 1], faces) for t in range(case.T)]
    sum(float(g) * l for g, l in zip(inp["g"], losses)).backward()
    _close(ref["lap_grad"].v, x.grad.numpy(), "g_xyz")
    _close(ref["lap_term"].v.sum(1) / V, [float(l.detach()) for l in losses], "mean term")
    # per vertex: a dense uniform Laplacian, rows of isolated vertices zero
    L = np.zeros((V, V))
    for f in faces:
        for a, b in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0])):
            L[a, b] = L[b, a] = 1.0
    deg = L.sum(1)
    L = L / np.maximum(deg, 1)[:, None] - np.diag((deg > 0).astype(np.float64))
    d = np.einsum("ij,tjk->tik", L, inp["x"].astype(np.float64))
    n = np.linalg.norm(d, axis=-1)
    _close(ref["lap_term"].v, n, "terms")
    _close(ref["lap_unit"].v, np.where(n[..., None] > 0, d / np.where(n > 0, n, 1)[..., None], 0.0), "unit")


@pytest.mark.parametrize("name", BY_KIND["quat"])
def test_quaternion_reference_equals_the_float64_cpu_path(name):
    from dreammesh4d_amd import ops

    inp, ref = ec.case_inputs(name), ec.reference(name)
    q = torch.tensor(inp["q"], dtype=torch.float64, requires_grad=True)
    R = ops.quat_xyzw_to_matrix(q, "pypose")
    R.backward(torch.tensor(inp["G"], dtype=torch.float64))
    _close(ref["quat_R"].v, R.detach().numpy(), "R")
    _close(ref["quat_grad"].v, q.grad.numpy(), "g_quat")
    assert not ref["quat_grad"].v[:, 3].any()


def _pair_row(pairs, row):
    hit = np.flatnonzero((pairs == np.asarray(row)).all(1))
    assert len(hit) >= 1, row
    return int(hit[0])


def test_case_list_covers_what_the_kernels_branch_on():
    sizes = {k: [] for k in ec.KINDS}
    for c in ec.CASES:
        if c.kind == "quat":
            sizes["quat"].append((c.mesh[0], c.mesh[1]))
            continue
        tab = ec.host_tables(c.mesh)
        assert len(tab["verts"]) <= 2000
        sizes[c.kind].append((c.T, len(tab["pairs"]) if c.kind == "nc" else len(tab["verts"])))
    for kind in ("arap", "nc", "lap"):
        assert {T for T, _ in sizes[kind]} == {1, 2, 5}
    assert {1, 31, 32, 33} <= {n for _, n in sizes["arap"]} and {1, 31, 32, 33} <= {n for _, n in sizes["lap"]}
    assert {1, 255, 256, 257} <= {n for _, n in sizes["nc"]}
    assert set(sizes["quat"]) == {(n, u) for n in (1, 255, 256, 257) for u in (True, False)}
    assert all(0.0 in g and min(g) < 0 for T, g in ec.UPSTREAM.items() if T == 5) and min(ec.UPSTREAM[2]) < 0
    # valences of the fan mesh: every class of the lane loop, isolated vertices in the middle and at V - 1
    tab = ec.host_tables("fans")
    V = len(tab["verts"])
    for off in (tab["csr"].off, tab["lap_off"]):
        deg = np.diff(off)
        assert set(deg % 8) == set(range(8))
        assert {0, 2, 3, 5, 6} | set(ec.FAN_VALENCES) == set(deg)
        assert deg[V - 1] == 0 and (deg[1:V - 1] == 0).sum() == 1
    items = np.diff(tab["nc_off"])                                  # (pair, role) items per vertex: what k_nc_bwd's lanes walk
    assert set(ec.FAN_VALENCES) <= set(items) and items[V - 1] == 0
    # the hand-built graph: valence 1, a symmetric pattern, one-way edges whose reverse has weight 0
    _, csr = ec.hand_csr()
    assert 1 in np.diff(csr.off) and np.array_equal(csr.rev[csr.rev], np.arange(len(csr.rev)))
    assert ((csr.w != 0) & (csr.w[csr.rev] == 0)).any() and (csr.w < 0).any()
    src = np.repeat(np.arange(len(csr.off) - 1), np.diff(csr.off))
    assert np.array_equal(csr.nbr[csr.rev], src) and np.array_equal(src[csr.rev], csr.nbr)
    assert ec.host_tables("lone")["csr"].off.tolist() == [0, 0] and len(ec.host_tables("lone")["lap_nbr"]) == 0


def test_special_pairs_are_what_their_names_say_in_float32_and_float64():
    tab, inp = ec.host_tables("special"), ec.case_inputs("nc-special-T2")
    pairs, ref, r32 = tab["pairs"], ec.case_reference("nc-special-T2"), ec.reference("nc-special-T2", np.float32)
    n32, m32 = ec.nc_normals(pairs, inp["x"], np.float32)
    n64, m64 = ec.nc_normals(pairs, inp["x"], np.float64)
    zf, zb = _pair_row(pairs, ec.SPECIAL["zero_first"]), _pair_row(pairs, ec.SPECIAL["zero_both"])
    for n0, m in ((n32, m32), (n64, m64)):
        assert (n0[:, zf] == 0).all() and (m[:, zf] > 1).all() and (n0[:, zb] == 0).all() and (m[:, zb] == 0).all()
    for r in (ref, r32):
        assert (r["nc_term"].v[:, [zf, zb]] == 1.0).all() and np.isfinite(r["nc_grad"].v).all()
        assert (r["nc_term"].v[:, _pair_row(pairs, ec.SPECIAL["flat"])] == 0.0).all()
        assert (r["nc_term"].v[:, _pair_row(pairs, ec.SPECIAL["folded"])] == 2.0).all()
        dup = np.flatnonzero(pairs[:, 2] == pairs[:, 3])
        assert len(dup) == 3 and set(pairs[dup, 2]) == set(ec.SPECIAL["duplicate"])       # one pair per edge of the face listed twice
        assert np.abs(r["nc_term"].v[:, dup] - 2.0).max() < 1e-6
    assert np.abs(ref["nc_grad"].v[:, ec.SPECIAL["zero_first"][2]]).max() > 1e7            # the oracle's 1 / 1e-8
    for what, count in (("three_faces", 3), ("four_faces", 6)):
        assert int((pairs[:, :2] == np.asarray(ec.SPECIAL[what])).all(1).sum()) == count
    (v,) = ec.SPECIAL["four_roles"]
    assert all((pairs[:, k] == v).any() for k in range(4))
    assert not (pairs == ec.SPECIAL["no_pair"][0]).any()
    s = _pair_row(pairs, ec.SPECIAL["slivers"])
    edge = np.linalg.norm(inp["x"][0, pairs[s, 1]].astype(np.float64) - inp["x"][0, pairs[s, 0]])
    assert 0.9e-3 < n64[0, s] / edge ** 2 < 1.1e-3 and 0.9e-3 < m64[0, s] / edge ** 2 < 1.1e-3
    # the clamp decides alike in float32 and float64 on every normal-consistency case
    for name in BY_KIND["nc"]:
        p, x = ec.host_tables(ec.CASE_BY_NAME[name].mesh)["pairs"], ec.case_inputs(name)["x"]
        for a32, a64 in zip(ec.nc_normals(p, x, np.float32), ec.nc_normals(p, x, np.float64)):
            assert np.array_equal(a32 > np.float32(ec.NC_EPS), a64 > ec.NC_EPS), name


def test_exact_zeros_of_the_laplacian_and_of_the_rest_pose_in_float32_and_float64():
    for f in (np.float32, np.float64):
        r = ec.reference("lap-square-T2", f)
        assert (r["lap_term"].v[:, 0] == 0).all() and (r["lap_unit"].v[:, 0] == 0).all()           # the centroid vertex
        assert (r["lap_term"].v[:, 1:5] > 0.5).all() and (np.abs(r["lap_grad"].v[:, 1:5]).max(-1) > 0).all()
        V = r["lap_term"].v.shape[1]
        assert (r["lap_term"].v[:, V - 1] == 0).all() and (r["lap_grad"].v[:, V - 1] == 0).all()    # the isolated one
        for name in ("arap-fans-rest-T2", "arap-hand-rest-T2"):
            r = ec.reference(name, f)
            assert all(not r[k].v.any() for k in ec.KINDS["arap"]), name
            assert all(r[k].s.any() for k in ec.KINDS["arap"]), name                               # ... by cancellation, not by absence
    for name in BY_KIND["lap"]:                                      # n > 0 decides alike
        assert np.array_equal(ec.reference(name, np.float32)["lap_term"].v > 0, ec.case_reference(name)["lap_term"].v > 0), name
    fans = ec.case_reference("lap-fans-T5")
    iso = np.flatnonzero(np.diff(ec.host_tables("fans")["lap_off"]) == 0)
    assert len(iso) == 2 and not fans["lap_term"].v[:, iso].any() and not fans["lap_unit"].s[:, iso].any()


def test_yardsticks_cover_the_float32_restatement_and_are_not_padded():
    worst = {}
    for c in ec.CASES:
        for k, v in ec.float32_ratios(c.name).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print({k: round(v, 4) for k, v in worst.items()})
    assert worst.keys() == ec.YARD.keys()
    for k, v in worst.items():
        assert 0.8 * ec.YARD[k] <= v <= ec.YARD[k], (k, v, ec.YARD[k])


@pytest.mark.parametrize("mesh", ["fans", "strip-257", "special"])
def test_host_tables_against_a_brute_force_restatement(mesh):
    tab = ec.host_tables(mesh)
    faces, V = tab["faces"], len(tab["verts"])
    # pytorch3d's enumeration: edges in lexicographic order, their faces in face order, every i < j
    opposite = {}
    for face in faces.tolist():
        for k in range(3):
            a, b = face[(k + 1) % 3], face[(k + 2) % 3]
            opposite.setdefault((min(a, b), max(a, b)), []).append(face[k])
    rows = [(u, v, o[i], o[j]) for (u, v), o in sorted(opposite.items()) for i in range(len(o)) for j in range(i + 1, len(o))]
    assert np.array_equal(tab["pairs"], np.asarray(rows, np.int64).reshape(-1, 4))
    assert np.array_equal(tab["pairs"], M.normal_consistency_pairs(faces))
    # the item CSR lists every (pair, role) exactly once, under the vertex that has that role
    off, items = tab["nc_off"], tab["nc_items"]
    assert off[0] == 0 and off[-1] == len(items) == 4 * len(rows) and np.array_equal(np.sort(items), np.arange(4 * len(rows)))
    owner = np.repeat(np.arange(V), np.diff(off))
    assert np.array_equal(tab["pairs"].reshape(-1)[items], owner)
    # ARAP: sorted one-rings, rev an involution onto the opposite edge, rest edges the float32 differences
    csr = tab["csr"]
    src = np.repeat(np.arange(V), np.diff(csr.off))
    ring = [set() for _ in range(V)]
    for a, b, c in faces.tolist():
        for u, v in ((a, b), (b, c), (c, a)):
            if u != v:
                ring[u].add(v)
                ring[v].add(u)
    assert csr.nbr.tolist() == [j for s in ring for j in sorted(s)]
    assert np.array_equal(csr.rev[csr.rev], np.arange(len(csr.rev)))
    assert np.array_equal(csr.nbr[csr.rev], src) and np.array_equal(src[csr.rev], csr.nbr)
    assert np.array_equal(csr.e, tab["verts"][src] - tab["verts"][csr.nbr])
    assert np.array_equal(tab["lap_off"], csr.off) and np.array_equal(tab["lap_nbr"], csr.nbr)
    if mesh != "special":        # (its zero-area faces sit on Heron's clamp) the coach's float32 weights against the cases' float64 ones
        from dreammesh4d_amd.mesh_reg import ARAPCoach

        own = ARAPCoach(tab["verts"], faces, "cpu")._w.numpy()
        assert own.shape == csr.w.shape and np.abs(own - csr.w).max() <= 1e-4 * np.abs(csr.w).max()
