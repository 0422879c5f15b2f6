"""Cases, restatements, bounds and comparison functions of tests/test_graph_kernels_edges_{cpu,gpu}.py (TEST INFRASTRUCTURE).

The deformation-graph construction (dreammesh4d_amd/csrc/heat.hip and csrc/graph.hip) is judged one entry point at a time:

* dm4d_cg_batched_f64 against `cg_restatement`: Jacobi-preconditioned conjugate gradients in numpy float64 IN THE KERNEL'S OWN
  ORDER (CSR rows summed in entry order; per 32-row block and column, wave w sums its rows w, w + 4, ... in order; the four
  wave partials as ((p0 + p1) + p2) + p3; blocks in block order; alpha = rz / pAp if pAp > 0 else 0, beta = rz_new / rz if
  rz > 0 else 0).  Only +, * and / in float64 are involved and the library is built with -ffp-contract=off, so the device result
  is compared BIT FOR BIT.  The restatement also restates the host loop (a look at the residual every `check_every` iterations).
* dm4d_heat_face_directions against an np.longdouble evaluation that carries a scale beside every gradient component.
* dm4d_graph_select_knn and k_geo_select: the indices against numpy's stable argsort on EVERY row, the weights against a float64
  evaluation of (1 - e_k / e_K)^2 from the float32 positions, bound 4 x WEIGHT_YARD + 4 x 2^-23 |ref|.
* dm4d_graph_geodesic_knn's distance table against `relax_fixed_point`: float32 Jacobi relaxation run to its fixed point.  The
  operator is monotone and only decreases values, so the device's in-place relaxation reaches the same fixed point whatever
  its update order: BIT FOR BIT.

Degenerate weight rows (e_K == 0, or a row sum that is 0 or not finite: all K + 1 chosen nodes equidistant from the vertex, or
on it) are the uniform row 1 / K in kernel and reference alike; the original formula yields NaN there.

INPUTS are seeded numpy or constructed, rounded so that every host sees the same bits.  Nothing here is measured against the
kernels: CG_GAP and WEIGHT_YARD are measured on the restatements (tests/test_graph_kernels_edges_cpu.py re-measures them), and
that file feeds one-token mutants of the restatements to the comparison functions below, which must reject each.
"""
import functools
import heapq
from collections import namedtuple

import numpy as np

# ---- measured constants (test_graph_kernels_edges_cpu.py re-measures them: 0.5 x constant <= measured <= constant) ----
CG_GAP = 3.6e-14          # worst |recursive - true| relative residual of the restatement at termination; measured 3.526e-14
                          # (path-V33-S64, tol 1e-10, random column 38: the singular matrix lets x drift along the constants)
CG_R = 4.0 * CG_GAP       # what the true residual of a converged column may exceed `tol` by
WEIGHT_YARD = 5.4e-7      # worst |float32 restatement - float64 reference| of a weight over all cases; measured 5.317e-7
                          # (geo-V257)
FACTOR = 4.0
U32 = 2.0 ** -23
CG_ROWS, CG_COLS, CG_WAVES = 32, 64, 4
UNREACHED = np.float32(3.0e38)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


# ================================================================================================ 1. conjugate gradients
CgCase = namedtuple("CgCase", "name matrix V S")
CG_CASES = [
    CgCase("spd-V1-S1", "spd", 1, 1),
    CgCase("spd-V31-S63", "spd", 31, 63),
    CgCase("spd-V32-S64", "spd", 32, 64),
    CgCase("spd-V33-S65", "spd", 33, 65),
    CgCase("spd-V65-S257", "spd", 65, 257),
    CgCase("spd-V130-S130", "spd", 130, 130),
    CgCase("cot-V130-S65", "cot", 130, 65),
    CgCase("path-V33-S64", "path", 33, 64),
]
CG_BY_NAME = {c.name: c for c in CG_CASES}
CG_FIXED = [(n, ce) for n in (1, 7, 25) for ce in (1, 10)]        # (max_iter, check_every) with tol out of reach
CG_FIXED_TOL = 1e-150                                            # tol^2 = 1e-300: only an exactly zero residual stops early
CG_CONVERGED = [(1e-10, 10), (1e-13, 3)]                         # (tol, check_every)
CG_CONVERGED_MAX_ITER = 2000
COLUMN_KINDS = ("random", "zero", "eig", "exact", "x0")         # columns 0..4 where S >= 5; the last column is "x0" again


def grid_patch(nx, ny, seed, jitter=0.35):
    """An OPEN patch of nx x ny vertices, unit spacing, jittered in the plane and lifted a little; coordinates are multiples of
    2^-10 (the same bits everywhere).  Two triangles per cell, the diagonal alternating.  -> (verts float32 [V,3], faces [F,3])."""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), indexing="ij")
    p = np.stack([gx, gy, np.zeros_like(gx)], -1).reshape(-1, 3)
    p[:, :2] += rng.uniform(-jitter, jitter, size=(len(p), 2))
    p[:, 2] = 0.3 * rng.uniform(-1, 1, size=len(p))
    p = np.round(p * 1024.0) / 1024.0
    faces = []
    for i in range(nx - 1):
        for j in range(ny - 1):
            a, b, c, d = i * ny + j, (i + 1) * ny + j, (i + 1) * ny + j + 1, i * ny + j + 1
            faces += [(a, b, c), (a, c, d)] if (i + j) % 2 == 0 else [(a, b, d), (b, c, d)]
    return p.astype(np.float32), np.asarray(faces, np.int64)


def _csr_from_dense(A):
    """Row-major CSR with sorted columns of the non-zeros of A (the diagonal is always kept)."""
    V = len(A)
    off, col, val = [0], [], []
    for i in range(V):
        for j in range(V):
            if A[i, j] != 0.0 or i == j:
                col.append(j)
                val.append(A[i, j])
        off.append(len(col))
    return np.asarray(off, np.int32), np.asarray(col, np.int32), np.asarray(val, np.float64)


def _cg_matrix(case):
    rng = np.random.default_rng(1000 + case.V)
    V = case.V
    if case.matrix == "spd":            # sparse, symmetric, strictly diagonally dominant, every entry a multiple of 1/8
        A = np.zeros((V, V))
        for i in range(V):
            for j in rng.choice(V, size=min(3, V), replace=False):
                if j != i:
                    A[i, j] = A[j, i] = float(rng.choice([-8, -5, -3, -1, 1, 2, 4, 7])) / 8.0
        A[np.arange(V), np.arange(V)] = np.abs(A).sum(1) + 0.125
    elif case.matrix == "path":         # singular: the graph Laplacian of a path with integer edge weights
        w = rng.integers(1, 4, size=V - 1).astype(np.float64)
        A = np.zeros((V, V))
        for i, wi in enumerate(w):
            A[i, i] += wi; A[i + 1, i + 1] += wi
            A[i, i + 1] -= wi; A[i + 1, i] -= wi
    else:                               # cotangent A + t L of a jittered open patch (obtuse triangles included)
        from dreammesh4d_amd.graph_build import heat_operators

        verts, faces = grid_patch(13, 10, seed=5)
        assert len(verts) == V
        L, _, area, t, _, _ = heat_operators(verts, faces)
        A = np.diag(area) + float(np.float32(t)) * L.toarray()
        A = 0.5 * (A + A.T)
    return A


@functools.lru_cache(maxsize=None)
def cg_inputs(name):
    """-> dict(A dense, off col val dinv, B [V,S], X0 [V,S], kinds [S], exact [V,S] or None per column via `sol`)."""
    case = CG_BY_NAME[name]
    V, S = case.V, case.S
    A = _cg_matrix(case)
    off, col, val = _csr_from_dense(A)
    diag = np.diag(A).copy()
    rng = np.random.default_rng(7 + 31 * V + S)
    kinds = ["random"] * S
    if S >= 5:
        kinds[:5] = COLUMN_KINDS
        kinds[S - 1] = "x0"
        if case.matrix == "cot":                                        # A xi is not exact there: no column starts AT its solution
            kinds[3] = "random"
    B = np.round(rng.normal(size=(V, S)) * 4096.0) / 4096.0
    X0 = np.zeros((V, S))
    # an eigenvector of D^-1 A (its largest eigenvalue), rounded to float32 and signed by its largest component
    dh = 1.0 / np.sqrt(diag)
    lam, Y = np.linalg.eigh(dh[:, None] * A * dh[None, :])
    v = dh * Y[:, -1]
    v = v / v[np.argmax(np.abs(v))]
    v = v.astype(np.float32).astype(np.float64)
    xi = rng.integers(-4, 5, size=V).astype(np.float64)                 # the exact start: small integers
    for s, kind in enumerate(kinds):
        if kind == "zero":
            B[:, s] = 0.0
        elif kind == "eig":
            B[:, s] = A @ v
        elif kind == "exact":
            B[:, s] = A @ xi                                            # exact for spd and path (multiples of 1/8, integers)
            X0[:, s] = xi
        elif kind == "x0":
            X0[:, s] = np.round(rng.normal(size=V) * 256.0) / 256.0
    if case.matrix == "path":                                           # consistent right-hand sides: zero mean
        for s, kind in enumerate(kinds):
            if kind in ("random", "x0"):
                B[:, s] -= B[:, s].sum() / V
                B[:, s] = np.round(B[:, s] * 2.0 ** 20) / 2.0 ** 20
                B[0, s] -= B[:, s].sum()
    out = dict(A=A, off=off, col=col, val=val, dinv=1.0 / diag, B=B, X0=X0, kinds=kinds, singular=case.matrix == "path")
    if case.matrix == "path":
        out["lam_min_plus"] = float(np.sort(np.linalg.eigvalsh(A))[1])
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _spmm(off, col, val, X):
    """A X, every row's entries added in entry order (the kernel's `ax += val[e] * x[col[e]]`)."""
    V = len(off) - 1
    out = np.zeros((V, X.shape[1]))
    nnz = np.diff(off)
    for j in range(int(nnz.max(initial=0))):
        rows = np.flatnonzero(nnz > j)
        e = off[rows] + j
        out[rows] = out[rows] + val[e, None] * X[col[e]]
    return out


def _col_dot(T, V, stride=CG_WAVES, drop_partial_block=False):
    """Column sums of T [V,S] in the kernels' two stages: block_rows_reduce, then k_cg_reduce over the row blocks."""
    S = T.shape[1]
    nb = (V + CG_ROWS - 1) // CG_ROWS
    P = np.zeros((nb * CG_ROWS, S))
    P[:V] = T
    P = P.reshape(nb, CG_ROWS, S)
    waves = []
    for w in range(CG_WAVES):
        acc = np.zeros((nb, S))
        for r in range(w, CG_ROWS, stride):
            acc = acc + P[:, r]
        waves.append(acc)
    part = ((waves[0] + waves[1]) + waves[2]) + waves[3]
    total = np.zeros(S)
    for k in range(nb - 1 if (drop_partial_block and V % CG_ROWS) else nb):
        total = total + part[k]
    return total


CgResult = namedtuple("CgResult", "X iters rel rr bb")


def cg_restatement(inp, max_iter, tol, check_every, mutant=None, columns=None):
    """dm4d_cg_batched_f64 restated (module docstring) -> CgResult(X, iterations run, final_rel_residual, rr [S], bb [S]).
    `columns`: solve only these columns (the same right-hand sides alone).  `mutant`: one deliberate defect
    (test_graph_kernels_edges_cpu.py): "wave_stride", "drop_rows", "drop_cols", "no_beta_guard"."""
    off, col, val, dinv = inp["off"], inp["col"], inp["val"], inp["dinv"][:, None]
    B, X = inp["B"], inp["X0"].copy()
    if columns is not None:
        B, X = B[:, columns], X[:, columns]
    V, S = B.shape
    live = slice(0, S // CG_COLS * CG_COLS) if mutant == "drop_cols" else slice(0, S)
    dot = functools.partial(_col_dot, V=V, stride=3 if mutant == "wave_stride" else CG_WAVES, drop_partial_block=mutant == "drop_rows")
    x0 = X.copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        r = B - _spmm(off, col, val, X)
        z = r * dinv
        p = z.copy()
        rz, bb = dot(r * z), dot(B * B)
        it, rel2, rr = 0, 1.0, np.zeros(S)
        while it < max_iter:
            for _ in range(check_every):
                if it >= max_iter:
                    break
                Ap = _spmm(off, col, val, p)
                pAp = dot(p * Ap)
                alpha = np.where(pAp > 0.0, rz / pAp, 0.0)
                X = X + alpha * p
                r = r - alpha * Ap
                z = r * dinv
                rz_new, rr = dot(r * z), dot(r * r)
                beta = rz_new / rz if mutant == "no_beta_guard" else np.where(rz > 0.0, rz_new / rz, 0.0)
                p = z + beta * p
                rz = rz_new
                it += 1
            rel = np.where(bb > 0.0, rr / bb, np.where(bb == 0.0, 0.0, np.nan))[live]
            rel2 = float(np.max(rel, initial=0.0)) if not np.isnan(rel).any() else float("nan")
            if rel2 != rel2 or rel2 <= tol * tol:
                break
    X[:, live.stop:] = x0[:, live.stop:]
    return CgResult(X, it, float(np.sqrt(rel2)), rr, bb)


@functools.lru_cache(maxsize=None)
def cg_fixed_reference(name, max_iter, check_every):
    return cg_restatement(cg_inputs(name), max_iter, CG_FIXED_TOL, check_every)


@functools.lru_cache(maxsize=None)
def cg_converged_reference(name, tol, check_every):
    return cg_restatement(cg_inputs(name), CG_CONVERGED_MAX_ITER, tol, check_every)


def true_residual(inp, X, columns=None):
    """|b - A x|_2 / |b|_2 per column (0 where b = 0 and the residual is 0 too)."""
    B = inp["B"] if columns is None else inp["B"][:, columns]
    r = np.linalg.norm(B - inp["A"] @ X, axis=0)
    b = np.linalg.norm(B, axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(b > 0, r / b, np.where(r == 0, 0.0, np.inf))


@functools.lru_cache(maxsize=None)
def pinv_solution(name):
    """A^+ B of a singular case in longdouble: (A + 1 1^T / 32) x = b for the zero-mean b (1 / 32: exact beside the integer
    entries), three rounds of iterative refinement."""
    inp = cg_inputs(name)
    ld = np.longdouble
    V = len(inp["A"])
    aug = inp["A"] + 1.0 / 32.0
    augl, Bl = aug.astype(ld), inp["B"].astype(ld)
    x = np.linalg.solve(aug, inp["B"]).astype(ld)
    for _ in range(3):
        x = x + np.linalg.solve(aug, (Bl - augl @ x).astype(np.float64)).astype(ld)
    return x - x.sum(0) / ld(V)


def compare_cg_fixed(name, max_iter, check_every, X, iters, rel):
    """The device result of a fixed-iteration run against the restatement: every bit.  -> list of complaints."""
    ref = cg_fixed_reference(name, max_iter, check_every)
    msgs = []
    if iters != ref.iters:
        msgs.append(f"{name} n={max_iter} ce={check_every}: returned {iters} iterations, restatement {ref.iters}")
    if not same_bits(np.float64(rel), np.float64(ref.rel)):
        msgs.append(f"{name} n={max_iter} ce={check_every}: final_rel_residual {rel!r} != {ref.rel!r}")
    X = np.asarray(X)
    if not same_bits(X, ref.X):
        bad = _bits(X) != _bits(ref.X) if X.shape == ref.X.shape else None
        if bad is None:
            msgs.append(f"{name}: shape {X.shape} != {ref.X.shape}")
        else:
            with np.errstate(invalid="ignore", divide="ignore"):
                worst = np.nanmax(np.abs(X - ref.X) / np.maximum(np.abs(ref.X), 1e-300))
            rows, cols = np.nonzero(bad)
            msgs.append(f"{name} n={max_iter} ce={check_every}: X differs in {int(bad.sum())} elements (rows {sorted(set(rows.tolist()))[:6]}, "
                        f"columns {sorted(set(cols.tolist()))[:6]}), worst relative {worst:.3g}, non-finite {int((~np.isfinite(X)).sum())}")
    return msgs


def compare_cg_converged(name, tol, check_every, X, iters, rel):
    """A converged run judged on its own (no restatement of the iterates needed).  -> (complaints, worst (true - tol) / R)."""
    inp = cg_inputs(name)
    msgs = []
    X = np.asarray(X)
    if not (iters % check_every == 0 or iters == CG_CONVERGED_MAX_ITER) or iters <= 0:
        msgs.append(f"{name} tol={tol}: {iters} iterations is no multiple of {check_every}")
    if not rel <= tol:
        msgs.append(f"{name} tol={tol}: final_rel_residual {rel}")
    if not np.isfinite(X).all():
        msgs.append(f"{name} tol={tol}: {int((~np.isfinite(X)).sum())} non-finite values")
        return msgs, np.inf
    true = true_residual(inp, X)
    over = (true - tol) / CG_R
    if (true > tol + CG_R).any():
        s = int(np.argmax(true))
        msgs.append(f"{name} tol={tol}: true residual {true[s]:.3e} of column {s} ({inp['kinds'][s]}) > tol + {CG_R:.1e}")
    for s, kind in enumerate(inp["kinds"]):
        if kind == "zero" and X[:, s].any():
            msgs.append(f"{name}: the zero column {s} came back non-zero")
        if kind == "exact" and not np.array_equal(X[:, s], inp["X0"][:, s]):
            msgs.append(f"{name}: the column started at its exact solution moved by {np.abs(X[:, s] - inp['X0'][:, s]).max():.3g}")
    if inp["singular"]:
        ld = np.longdouble
        star, Xl = pinv_solution(name), X.astype(ld)
        R = inp["B"].astype(ld) - inp["A"].astype(ld) @ Xl                  # (longdouble: the bound below is sharp)
        for s in range(X.shape[1]):
            want = star[:, s]
            got = Xl[:, s] - Xl[:, s].sum() / ld(len(Xl))
            rn = float(np.sqrt((R[:, s] * R[:, s]).sum()))
            dist = float(np.sqrt(((got - want) * (got - want)).sum()))
            # (+ what float64 cannot hold of the solution itself: 4 x 2^-53 sqrt(V) max|x|)
            if dist > rn / inp["lam_min_plus"] + FACTOR * 2.0 ** -53 * np.sqrt(len(Xl)) * float(np.abs(want).max(initial=1.0)):
                msgs.append(f"{name} tol={tol}: column {s} ({inp['kinds'][s]}) is {dist:.3g} from the pseudo-inverse solution, |r| / lambda = {rn / inp['lam_min_plus']:.3g}")
    return msgs, float(np.max(over))


# ================================================================================================ 2. face directions
DirCase = namedtuple("DirCase", "name F S")
DIR_CASES = [DirCase("dirs-F1-S1", 1, 1), DirCase("dirs-F3-S64", 3, 64), DirCase("dirs-F4-S65", 4, 65), DirCase("dirs-F5-S65", 5, 65),
             DirCase("dirs-F5-S1", 5, 1)]
DIR_BY_NAME = {c.name: c for c in DIR_CASES}
DIR_PAD = 37                                            # sentinel doubles in front of and behind the output
DIR_SENTINEL = -12345.678


@functools.lru_cache(maxsize=None)
def dir_inputs(name):
    """faces [F,3] int32, G [F,3,3] float64 (heat_operators on a jittered patch, the third row closed so that the three rows add up
    to exactly zero: the gradient of a constant is then an exact 0), U [V,S] float64; kinds [S]."""
    from dreammesh4d_amd.graph_build import heat_operators

    case = DIR_BY_NAME[name]
    verts, faces = grid_patch(3, 3, seed=11)
    faces = faces[:case.F]
    G = heat_operators(verts, faces)[4].copy()
    G = np.round(G * 2.0 ** 30) / 2.0 ** 30
    G[:, 2] = -(G[:, 0] + G[:, 1])
    rng = np.random.default_rng(100 + 7 * case.F + case.S)
    V, S = len(verts), case.S
    U = np.round(rng.normal(size=(V, S)) * 2.0 ** 20) / 2.0 ** 20
    kinds = ["random"] * S
    if S >= 8:
        kinds[1], kinds[2], kinds[3], kinds[S - 1], kinds[S - 2] = "const_half", "const_zero", "far", "far", "const_half"
    else:
        kinds[0] = "far" if case.F == 5 else "const_half"
    for s, kind in enumerate(kinds):
        if kind == "const_half":
            U[faces[0], s] = 0.5                        # a power of two: u g is exact, and (g0 + g1) + g2 == 0 exactly
        elif kind == "const_zero":
            U[faces[0], s] = 0.0
        elif kind == "far":                             # the far field of a heat solution: 1e-300 ... 1
            U[:, s] = 10.0 ** (-300.0 * rng.uniform(size=V))
            if case.F > 1:                              # one face whose gradient underflows when squared
                U[faces[1], s] = (1e-170, 1e-200, 1e-290)
            hot = [v for v in faces[-1] if case.F == 1 or v not in faces[1]][-1]
            U[hot, s], U[faces[0][0], s] = 1.0, 1e-300
    U.setflags(write=False)
    return dict(faces=faces.astype(np.int32), G=G, U=U, kinds=kinds, V=V)


@functools.lru_cache(maxsize=None)
def dir_reference(name):
    """(XT [3F,S] longdouble, bound [3F,S] float64, zero [3F,S] bool: must be an exact zero)."""
    inp = dir_inputs(name)
    ld = np.longdouble
    f, G, U = inp["faces"], inp["G"].astype(ld), inp["U"].astype(ld)
    F, S = len(f), U.shape[1]
    u = U[f]                                            # [F,3,S]
    grad = np.einsum("fks,fkc->fcs", u, G)              # [F,3,S]
    scale = np.einsum("fks,fk->fs", np.abs(u), np.sqrt((G * G).sum(-1)))       # sum_k |u_k| |g_k|
    m = np.abs(grad).max(axis=1, keepdims=True)
    safe = np.where(m > 0, m, ld(1))
    gn = grad / safe
    n = np.sqrt((gn * gn).sum(axis=1, keepdims=True)) * safe
    zero = np.broadcast_to(m == 0, grad.shape)
    XT = np.where(zero, ld(0), -grad / np.where(n > 0, n, ld(1)))
    bound = np.where(zero, 0.0, FACTOR * 2.0 ** -53 * (scale[:, None, :] / np.where(n > 0, n, ld(1))).astype(np.float64) + FACTOR * 2.0 ** -52)
    return XT.reshape(3 * F, S), bound.reshape(3 * F, S), zero.reshape(3 * F, S).copy()


def dir_restatement(name, transposed=True):
    """The kernel's expression in float64 -> the flat sentinel buffer the GPU test reads back (`transposed=False`: the mutant
    that writes [S][3F])."""
    inp = dir_inputs(name)
    f, G, U = inp["faces"], inp["G"], inp["U"]
    u = U[f]
    g = [(u[:, 0] * G[:, 0, c, None] + u[:, 1] * G[:, 1, c, None]) + u[:, 2] * G[:, 2, c, None] for c in range(3)]
    m = np.maximum(np.maximum(np.abs(g[0]), np.abs(g[1])), np.abs(g[2]))
    ex = np.where(m > 0, np.frexp(m)[1], 0)
    g = [np.ldexp(c, -ex) for c in g]
    n = np.maximum(np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]), 1e-300)
    XT = np.stack([-c / n for c in g], 1).reshape(3 * len(f), -1)
    buf = np.full(2 * DIR_PAD + XT.size, DIR_SENTINEL)
    buf[DIR_PAD:DIR_PAD + XT.size] = (XT if transposed else XT.T).reshape(-1)
    return buf


def compare_dirs(name, buf):
    """buf: the flat buffer (DIR_PAD sentinels, [3F][S], DIR_PAD sentinels).  -> (complaints, worst error / bound)."""
    ref, bound, zero = dir_reference(name)
    buf = np.asarray(buf)
    msgs = []
    if not (buf[:DIR_PAD] == DIR_SENTINEL).all() or not (buf[DIR_PAD + ref.size:] == DIR_SENTINEL).all():
        msgs.append(f"{name}: the doubles around the output were written")
    got = buf[DIR_PAD:DIR_PAD + ref.size].reshape(ref.shape)
    if not np.isfinite(got).all():
        msgs.append(f"{name}: {int((~np.isfinite(got)).sum())} non-finite directions")
    if (got[zero] != 0).any():
        msgs.append(f"{name}: the gradient of a constant is not an exact zero")
    err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(zero, 0.0, err / np.where(zero, 1.0, bound))
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    if (ratio > 1.0).any():
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        msgs.append(f"{name}: {int((ratio > 1).sum())} components off, worst at row {i[0]} column {i[1]} ({dir_inputs(name)['kinds'][i[1]]}): "
                    f"got {got[i]!r}, reference {float(ref[i])!r}, error / bound {ratio[i]:.3g}")
    return msgs, float(ratio.max())


# ================================================================================================ 3. selection and weights
SENT_IDX, SENT_W = -777, -55.5                          # what rows outside [v0, v0 + S) of idx / weights must keep


def stable_topk(score, K1):
    """[M,S] scores -> [S,K1] node indices: numpy's stable argsort (NaN last, ties towards the lower index)."""
    return np.argsort(score, axis=0, kind="stable")[:K1].T.astype(np.int64)


def weights_reference(verts, nodes, sel):
    """float64 (1 - e_k / e_K)^2, row-normalised, from float32 positions; sel [S,K+1] node indices of vertices 0..S-1.  Degenerate
    rows (e_K == 0, row sum 0 or not finite) are uniform.  -> (weights [S,K] float64, degenerate [S] bool)."""
    v, n = np.asarray(verts, np.float32).astype(np.float64), np.asarray(nodes, np.float32).astype(np.float64)
    d = v[:, None, :] - n[sel]
    e = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    K = sel.shape[1] - 1
    with np.errstate(divide="ignore", invalid="ignore"):
        t = 1.0 - e[:, :K] / e[:, K:]
        w = t * t
        tot = w.sum(1)
        deg = ~((e[:, K] > 0) & (tot > 0) & np.isfinite(tot))
        out = np.where(deg[:, None], 1.0 / K, w / tot[:, None])
    return out, deg


def weights_float32(verts, nodes, sel, mutant=None):
    """The kernels' expression in np.float32, in their order.  mutant "kth": normalise by the K-th instead of the (K + 1)-th."""
    f = np.float32
    v, n = np.asarray(verts, f), np.asarray(nodes, f)
    d = v[:, None, :] - n[sel]
    e = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    K = sel.shape[1] - 1
    eK = e[:, K - 1 if mutant == "kth" else K]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        tot = np.zeros(len(v), f)
        w = np.zeros((len(v), K), f)
        for k in range(K):
            t = f(1.0) - e[:, k] / eK
            w[:, k] = t * t
            tot = tot + w[:, k]
        ok = (eK > 0) & (tot > 0) & np.isfinite(tot)
        out = np.where(ok[:, None], w / tot[:, None], f(1.0) / f(K))
    return out.astype(f)


SelCase = namedtuple("SelCase", "name K M S ld v0 Vtot flavour")
SEL_CASES = [
    SelCase("select-K1-M2-S1", 1, 2, 1, 1, 0, 1, "plain"),
    SelCase("select-K4-M5-S255", 4, 5, 255, 255, 0, 255, "plain"),
    SelCase("select-K4-M6-S256-ld300", 4, 6, 256, 300, 0, 256, "plain"),
    SelCase("select-K4-M40-S257-v7", 4, 40, 257, 257, 7, 300, "plain"),
    SelCase("select-K16-M17-S257-ld260-v3", 16, 17, 257, 260, 3, 261, "plain"),
    SelCase("select-K16-M18-S255", 16, 18, 255, 255, 0, 255, "plain"),
    SelCase("select-K16-M40-S256-v44-ld400", 16, 40, 256, 400, 44, 300, "plain"),
    SelCase("select-K1-M40-S257", 1, 40, 257, 257, 0, 257, "plain"),
    SelCase("select-twins-K4-M12-S64", 4, 12, 64, 70, 5, 80, "twins"),
    SelCase("select-nonfinite-K4-M6-S65", 4, 6, 65, 65, 0, 65, "nonfinite"),
    SelCase("select-nonfinite-K16-M17-S257-v2", 16, 17, 257, 259, 2, 260, "nonfinite"),
    SelCase("select-nonfinite-K1-M40-S64", 1, 40, 64, 64, 0, 64, "nonfinite"),
    SelCase("select-degenerate-K4-M12-S40", 4, 12, 40, 48, 3, 50, "degenerate"),
    SelCase("select-degenerate-K1-M2-S3", 1, 2, 3, 3, 0, 3, "degenerate"),
]
SEL_BY_NAME = {c.name: c for c in SEL_CASES}
SPHERE_3 = [(1, 2, 2), (2, 1, 2), (2, 2, 1), (-1, 2, 2), (2, -1, 2), (2, 2, -1), (1, -2, 2), (-2, 1, 2), (3, 0, 0), (0, 3, 0), (0, 0, 3),
            (-3, 0, 0)]                                  # |p| = 3 exactly, in float32 and float64


@functools.lru_cache(maxsize=None)
def sel_inputs(name):
    """score [M,ld] float64 (columns >= S hold NaN: never to be read into a result), verts [Vtot,3], nodes [M,3] float32."""
    c = SEL_BY_NAME[name]
    rng = np.random.default_rng(17 * c.K + 1009 * c.M + c.S + 3 * c.ld + c.v0)
    score = np.full((c.M, c.ld), np.nan)
    body = rng.normal(size=(c.M, c.S))
    kinds = ["random"] * c.S
    for s in range(c.S):
        k = s % 8 if c.S >= 8 else 0
        if k == 1:
            body[:, s], kinds[s] = rng.integers(0, 3, size=c.M), "ties"
        elif k == 2:
            body[:, s], kinds[s] = 0.25, "all_equal"
        elif k == 3:
            body[:, s], kinds[s] = -np.arange(c.M, dtype=np.float64), "descending"
        elif k == 4:
            body[:, s], kinds[s] = np.arange(c.M, dtype=np.float64), "ascending"
        elif k == 5:
            body[:, s], kinds[s] = np.repeat(rng.normal(size=(c.M + 1) // 2), 2)[:c.M], "pair_ties"
    if c.flavour == "nonfinite":
        for s in range(c.S):
            k = s % 8
            col = body[:, s]
            pick = rng.permutation(c.M)
            if k == 0:
                col[pick[:max(1, c.M // 2)]], kinds[s] = np.inf, "some_inf"
            elif k == 1:
                col[pick[:max(1, c.M // 2)]], kinds[s] = np.nan, "some_nan"
            elif k == 2:
                col[pick[:c.M - 1]], kinds[s] = 1.0e300, "many_1e300"
            elif k == 3:
                col[:], kinds[s] = np.nan, "all_nan"
            elif k == 4:
                col[:], kinds[s] = np.inf, "all_inf"
            elif k == 5:
                col[pick[:c.M // 3 + 1]] = np.nan
                col[pick[c.M // 3 + 1:2 * (c.M // 3) + 2]] = np.inf
                col[pick[-1]], kinds[s] = 1.5e300, "nan_inf_1e300"
            elif k == 6:
                col[:], kinds[s] = rng.choice([1.0e300, 1.0e305, np.inf, np.nan], size=c.M), "all_huge"
            else:
                col[pick[:c.M - 1]], kinds[s] = -np.inf, "minus_inf"
    score[:, :c.S] = body
    verts = (np.round(rng.uniform(-2, 2, size=(c.Vtot, 3)) * 1024.0) / 1024.0).astype(np.float32)
    nodes = (np.round(rng.uniform(-2, 2, size=(c.M, 3)) * 1024.0) / 1024.0).astype(np.float32)
    if c.flavour == "twins":
        # nodes on shells around the origin, two by two on nearly the same shell (e_k ~ e_K: cancellation); vertices near the origin
        dirs = rng.normal(size=(c.M, 3))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        radius = 1.0 + 0.5 * (np.arange(c.M) // 2) + 1e-3 * (np.arange(c.M) % 2)
        nodes = (np.round(dirs * radius[:, None] * 2.0 ** 16) / 2.0 ** 16).astype(np.float32)
        verts = (np.round(rng.uniform(-0.01, 0.01, size=(c.Vtot, 3)) * 2.0 ** 16) / 2.0 ** 16).astype(np.float32)
        for s in range(c.S):                            # the ranking is by distance from the origin, from a rotating start
            score[:, s] = np.roll(np.arange(c.M, dtype=np.float64), s % c.M)
            kinds[s] = "twins"
    if c.flavour == "degenerate":
        centre = np.asarray([0.5, -1.0, 0.25])
        nodes = (np.asarray(SPHERE_3[:c.M], np.float64) + centre).astype(np.float32)
        if c.M >= 12:
            nodes[6:] = nodes[6]                        # nodes 6.. share one position
        for s in range(c.S):
            v = c.v0 + s
            k = s % 4
            if k == 0:
                verts[v], kinds[s] = centre, "equidistant"                 # every node at distance 3: the row sum is 0
            elif k == 1:
                verts[v], kinds[s] = nodes[-1], "on_the_nodes"             # e_K == 0 where the (K + 1)-th is one of the shared nodes
                score[:, s] = -np.arange(c.M, dtype=np.float64)            # the shared nodes rank first
            elif k == 2:
                verts[v], kinds[s] = nodes[-1], "on_the_last"              # e_k > 0 = e_K: an infinite ratio
                score[:, s] = np.arange(c.M, dtype=np.float64)
                score[c.M - 1, s] = c.K - 0.5                              # the node under the vertex ranks (K + 1)-th
    for a in (score, verts, nodes):
        a.setflags(write=False)
    return dict(score=score, verts=verts, nodes=nodes, kinds=kinds)


def select_restatement(name, mutant=None):
    """What dm4d_graph_select_knn must leave in sentinel-filled idx [Vtot,K] / weights [Vtot,K].  Mutants: "tie_high" (ties towards
    the higher index), "ignore_v0", "ld_is_S", "kth"."""
    c, inp = SEL_BY_NAME[name], sel_inputs(name)
    score = inp["score"]
    table = score.reshape(-1)[:c.M * c.S].reshape(c.M, c.S) if mutant == "ld_is_S" else score[:, :c.S]
    if mutant == "tie_high":
        sel = (c.M - 1 - stable_topk(table[::-1], c.K + 1))
    else:
        sel = stable_topk(table, c.K + 1)
    v0 = 0 if mutant == "ignore_v0" else c.v0
    idx = np.full((c.Vtot, c.K), SENT_IDX, np.int64)
    w = np.full((c.Vtot, c.K), SENT_W, np.float32)
    idx[v0:v0 + c.S] = sel[:, :c.K]
    w[v0:v0 + c.S] = weights_float32(inp["verts"][v0:v0 + c.S], inp["nodes"], sel, mutant="kth" if mutant == "kth" else None)
    return idx, w


def _compare_rows(tag, idx, w, want_sel, verts, nodes, M):
    """Rows of idx [n,K] / w [n,K] against the wanted selection [n,K+1].  -> (complaints, worst weight error / bound)."""
    K = want_sel.shape[1] - 1
    msgs = []
    idx, w = np.asarray(idx), np.asarray(w)
    if idx.min(initial=0) < 0 or idx.max(initial=0) >= M:
        msgs.append(f"{tag}: neighbour indices outside [0, {M}): min {idx.min()}, max {idx.max()}")
    bad = (idx != want_sel[:, :K]).any(1)
    if bad.any():
        r = int(np.flatnonzero(bad)[0])
        msgs.append(f"{tag}: {int(bad.sum())} rows differ from the stable argsort, first row {r}: {idx[r].tolist()} != {want_sel[r, :K].tolist()}")
    if not np.isfinite(w).all():
        msgs.append(f"{tag}: {int((~np.isfinite(w)).sum())} non-finite weights in rows {np.flatnonzero(~np.isfinite(w).all(1))[:8].tolist()}")
    ref, _ = weights_reference(verts, nodes, want_sel)
    bound = FACTOR * WEIGHT_YARD + FACTOR * U32 * np.abs(ref)
    ratio = np.abs(w.astype(np.float64) - ref) / bound
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    if (ratio > 1).any():
        r = int(np.argmax(ratio.max(1)))
        msgs.append(f"{tag}: weights off in {int((ratio > 1).any(1).sum())} rows, worst row {r}: {w[r].tolist()} != {ref[r].tolist()} (error / bound {ratio[r].max():.3g})")
    return msgs, float(ratio.max(initial=0.0))


def compare_select(name, idx, w):
    """idx [Vtot,K] int64 / w [Vtot,K] float32 as the entry point left them (sentinel-filled before the call)."""
    c, inp = SEL_BY_NAME[name], sel_inputs(name)
    idx, w = np.asarray(idx), np.asarray(w)
    want = stable_topk(inp["score"][:, :c.S], c.K + 1)
    rows = slice(c.v0, c.v0 + c.S)
    msgs, worst = _compare_rows(name, idx[rows], w[rows], want, inp["verts"][rows], inp["nodes"], c.M)
    outside = np.ones(c.Vtot, bool)
    outside[rows] = False
    if (idx[outside] != SENT_IDX).any() or (w[outside] != np.float32(SENT_W)).any():
        msgs.append(f"{name}: rows outside [{c.v0}, {c.v0 + c.S}) were written")
    return msgs, worst


# ================================================================================================ 4. edge-path distances
GeoCase = namedtuple("GeoCase", "name K")
GEO_CASES = [GeoCase("geo-path40", 4), GeoCase("geo-path300", 4), GeoCase("geo-V255", 4), GeoCase("geo-V256", 4), GeoCase("geo-V257", 4),
             GeoCase("geo-grid-ties", 4), GeoCase("geo-zero-edges", 4), GeoCase("geo-components", 4), GeoCase("geo-K16-M17", 16),
             GeoCase("geo-K1", 1), GeoCase("geo-degenerate-sphere", 4), GeoCase("geo-degenerate-coincident", 4)]
GEO_BY_NAME = {c.name: c for c in GEO_CASES}


def _csr_from_edges(V, edges):
    """Undirected (u, v, length) triples -> one-ring CSR (offsets int32 [V+1], neighbours int32, lengths float32), sorted."""
    both = sorted({(u, v): l for u, v, l in edges}.items())
    both = sorted([(u, v, l) for (u, v), l in both] + [(v, u, l) for (u, v), l in both])
    off = np.zeros(V + 1, np.int32)
    for u, _, _ in both:
        off[u + 1] += 1
    return np.cumsum(off).astype(np.int32), np.asarray([v for _, v, _ in both], np.int32), np.asarray([l for _, _, l in both], np.float32)


@functools.lru_cache(maxsize=None)
def geo_inputs(name):
    """off nbr len (CSR), verts [V,3] float32, nodes [M,3] float32, node_vertex [M] int32."""
    K = GEO_BY_NAME[name].K
    rng = np.random.default_rng(sum(map(ord, name)))
    q = lambda a, b=1024.0: np.round(np.asarray(a, np.float64) * b) / b
    rand_len = lambda: float(q(rng.uniform(0.05, 1.0)))
    if name in ("geo-path40", "geo-path300"):
        V = 40 if name == "geo-path40" else 300
        edges = [(i, i + 1, rand_len()) for i in range(V - 1)]
        node_vertex = [0, V - 1, V // 2, V // 3, V - 1] + ([7] if V == 300 else [])     # two nodes on the last vertex; M == K + 1 at 40
    elif name in ("geo-V255", "geo-V256", "geo-V257", "geo-K16-M17", "geo-K1", "geo-zero-edges"):
        V = {"geo-V255": 255, "geo-V256": 256, "geo-V257": 257, "geo-K16-M17": 64, "geo-K1": 33, "geo-zero-edges": 48}[name]
        edges = [(i, i + 1, rand_len()) for i in range(V - 1)] + [(V - 1, 0, rand_len())]
        for _ in range(V):
            u, v = (int(x) for x in rng.choice(V, 2, replace=False))
            edges.append((min(u, v), max(u, v), rand_len()))
        if name == "geo-zero-edges":
            edges = [(u, v, 0.0 if i % 3 == 0 else l) for i, (u, v, l) in enumerate(edges)]
        M = {"geo-K16-M17": 17, "geo-K1": 2}.get(name, 20)
        node_vertex = rng.choice(V, M, replace=False).tolist()
        if M >= 20:
            node_vertex[5] = node_vertex[11]                                          # two nodes on one vertex
            node_vertex[3] = V - 1
    elif name == "geo-grid-ties":
        n = 9
        V = n * n
        edges = [(i * n + j, i * n + j + 1, 1.0 + ((i + j) % 3 == 0)) for i in range(n) for j in range(n - 1)]
        edges += [(i * n + j, (i + 1) * n + j, 1.0) for i in range(n - 1) for j in range(n)]
        node_vertex = [0, n - 1, V - 1, V - n, V // 2, 4, 4 * n]
    elif name == "geo-components":
        V = 50                                                                        # 0..29, 30..48, and the isolated 49
        edges = [(i, i + 1, rand_len()) for i in range(29)] + [(i, i + 1, rand_len()) for i in range(30, 48)] + [(30, 40, rand_len())]
        node_vertex = [3, 35, 17, 28, 44, 17, 9]                                      # only nodes 1 and 4 live in the second component
    else:
        V = 12
        edges = [(i, i + 1, rand_len()) for i in range(V - 1)] + [(0, 6, rand_len())]
        node_vertex = [0, 3, 5, 8, 11]                                                # M == K + 1: every node is chosen on every row
    M = len(node_vertex)
    assert M >= K + 1
    off, nbr, ln = _csr_from_edges(V, edges)
    verts = q(rng.uniform(-2, 2, size=(V, 3))).astype(np.float32)
    nodes = q(verts[node_vertex].astype(np.float64) + rng.uniform(-0.05, 0.05, size=(M, 3))).astype(np.float32)
    if name == "geo-degenerate-sphere":
        verts[4] = (0.5, -1.0, 0.25)
        nodes = (np.asarray(SPHERE_3[:M], np.float64) + verts[4].astype(np.float64)).astype(np.float32)      # vertex 4: all at distance 3
        last = int(np.argsort(_relax(off, nbr, ln, np.asarray(node_vertex))[0][:, 9], kind="stable")[K])
        verts[9] = nodes[last]                                                        # vertex 9 sits on its (K + 1)-th node: e_K == 0
    if name == "geo-degenerate-coincident":
        nodes[:] = verts[6]                                                           # every node in one place: every row degenerate
    out = dict(off=off, nbr=nbr, len=ln, verts=verts, nodes=nodes, node_vertex=np.asarray(node_vertex, np.int32), V=V, M=M, K=K)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _relax(off, nbr, ln, node_vertex):
    V, M = len(off) - 1, len(node_vertex)
    d = np.full((M, V), UNREACHED, np.float32)
    d[np.arange(M), node_vertex] = 0.0
    src = np.repeat(np.arange(V), np.diff(off))
    sweeps = 0
    while True:
        new = d.copy()
        if len(src):
            cand = (d[:, nbr] + ln[None, :]).astype(np.float32)
            np.minimum.at(new.T, src, cand.T)
        if np.array_equal(new, d):
            return d, sweeps
        d, sweeps = new, sweeps + 1


@functools.lru_cache(maxsize=None)
def relax_fixed_point(name):
    """float32 Jacobi relaxation d[v] = min(d[v], min_u fl32(d[u] + len)) from k_geo_init's table, run until nothing changes.
    -> (table [M,V] float32, sweeps that changed something)."""
    g = geo_inputs(name)
    return _relax(g["off"], g["nbr"], g["len"], g["node_vertex"])


def dijkstra_float64(name):
    """Exact shortest edge paths in float64 (a heap; unreachable: inf) -> [M,V]."""
    g = geo_inputs(name)
    out = np.full((g["M"], g["V"]), np.inf)
    for m, s in enumerate(g["node_vertex"].tolist()):
        dist, heap = out[m], [(0.0, s)]
        dist[s] = 0.0
        while heap:
            du, u = heapq.heappop(heap)
            if du > dist[u]:
                continue
            for e in range(g["off"][u], g["off"][u + 1]):
                v, dv = int(g["nbr"][e]), du + float(g["len"][e])
                if dv < dist[v]:
                    dist[v] = dv
                    heapq.heappush(heap, (dv, v))
    return out


def geo_restatement(name, mutant=None):
    """(table, idx [V,K], weights [V,K]) as dm4d_graph_geodesic_knn must leave them."""
    g = geo_inputs(name)
    table, _ = relax_fixed_point(name)
    K = g["K"]
    if mutant == "tie_high":
        sel = g["M"] - 1 - stable_topk(table[::-1].astype(np.float64), K + 1)
    else:
        sel = stable_topk(table.astype(np.float64), K + 1)
    return table, sel[:, :K].copy(), weights_float32(g["verts"], g["nodes"], sel, mutant="kth" if mutant == "kth" else None)


def compare_geo(name, table, idx, w):
    g = geo_inputs(name)
    want, _ = relax_fixed_point(name)
    table = np.asarray(table)
    msgs = []
    if not same_bits(table, want):
        bad = _bits(table) != _bits(want)
        msgs.append(f"{name}: the distance table differs in {int(bad.sum())} entries, first {tuple(np.argwhere(bad)[0])}: "
                    f"{table[bad][0]!r} != {want[bad][0]!r}")
    sel = stable_topk(want.astype(np.float64), g["K"] + 1)
    more, worst = _compare_rows(name, idx, w, sel, g["verts"], g["nodes"], g["M"])
    return msgs + more, worst
