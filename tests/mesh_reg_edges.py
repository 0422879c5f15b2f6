"""Cases, a plain float64 reference and the error bounds of tests/test_mesh_reg_edges_{cpu,gpu}.py (TEST INFRASTRUCTURE).

The mesh regularisers (dreammesh4d_amd/csrc/meshreg.hip behind dreammesh4d_amd/mesh_reg.py and ops.quat_xyzw_to_matrix) are
judged element by element: ARAP per-vertex energy [T,V], dE/dx' and dE/dR; normal-consistency terms [T,P] and vertex gradient;
Laplacian terms, unit vectors and vertex gradient; the pypose backward of quaternion -> matrix.  The reference states every
gradient in closed form over edges and pairs (`np.add.at` scatters; no autograd, no code of oracle/mesh_reg.py) and reads the
float32 tables the kernels read (the coach's `_off _nbr _rev _e`, the weights of INPUTS below, `MeshNormalConsistency._pairs`),
widened to float64: only the arithmetic differs.  tests/test_mesh_reg_edges_cpu.py pins it to float64 autograd through the oracle.

Scale.  Every number the reference computes travels with a SCALE (class `S`): what its rounding error is proportional to.
An input's scale is its magnitude; a sum or difference adds the scales of its terms (so a sum's scale is the sum of the
absolute values it adds up, and a cancelled difference keeps the size of what cancelled); products, quotients and square roots
propagate to first order (|a| s_b + |b| s_a, plus the second-order term 2^-24 s_a s_b so that an exact zero does not hide the
error of what cancelled to it); a branch taken on an exact value (the 1e-8 norm clamp, the Laplacian's n > 0, an isolated
vertex) yields a constant of scale 0.  An element of scale 0 must be reproduced exactly.

Bounds (measured, not guessed).  The yardstick of a tensor kind is the worst, over all elements of all CASES, of
|float32 restatement - float64 reference| / (2^-24 scale), the float32 restatement being this same reference run in np.float32
on the CPU.  A kernel element may differ from the float64 reference by FACTOR x yardstick x 2^-24 x scale (another fixed
summation order: 8 lane partials, then a butterfly -- not another algorithm).  Nothing is measured against the kernels.

Exact facts.  The cases are built so that float32 and float64 take the same branches: zero-area faces and the centroid vertex
have small integer coordinates, every mesh vertex is a multiple of 2^-12 (so the rest pose translated by (0.5, -2, 8) has
exactly the rest edges), and the rest-pose residual is the very float32 difference the kernel forms.

INPUTS.  Every input of every case is the same bits on every machine (numpy's seeded generator, float64 arithmetic, one
rounding to float32).  That includes the ARAP edge weights: the coach computes its cotangent weights with torch's float32
`norm`, whose last bit differs between CPUs, and a yardstick is a maximum over elements, which such a bit moves by percents.
The cases therefore carry `cot_weights` (the coach's formula in float64 numpy, rounded once), the GPU test writes them into the
coach's `_w` before it calls anything, and the CPU test pins the coach's own float32 weights to them (to 1e-4 of the mesh's largest weight:
Heron's formula in float32 loses 1e-5 of the area of the needle faces of the valence-300 fan, whose weights are the largest).  Offsets, neighbours, reverse edges and rest edges are the
coach's.  Kernel and reference read the same tables: only the arithmetic differs.

Open question, not decided here: kernel and oracle give an ISOLATED vertex a zero Laplacian row (term 0, no gradient).
pytorch3d is neither installed nor vendored, so which convention it follows is unpinned; these tests pin kernel = oracle.
"""
import functools
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
FACTOR = 4.0                 # the project's factor (tests/node_network_edges.py)
NC_EPS = 1e-8                # torch.cosine_similarity's clamp of the norms

# ---- yardsticks: worst |float32 restatement - float64 reference| / (2^-24 scale) over all CASES, per tensor kind, rounded up
#      to two digits (test_mesh_reg_edges_cpu.py re-measures them: 0.8 x constant <= measured <= constant) ----
YARD = {
    "arap_energy": 0.70,     # measured 0.6961  (arap-fan32-T5)
    "arap_g_xyz": 1.3,       # measured 1.2640  (arap-fans-T5)
    "arap_g_rot": 1.7,       # measured 1.6722  (arap-fans-T5)
    "nc_term": 0.23,         # measured 0.2258  (nc-fans-T5)
    "nc_grad": 0.20,         # measured 0.1916  (nc-strip1-T2)
    "lap_term": 5.0,         # measured 4.9192  (lap-fans-T5: 300 neighbours added one by one)
    "lap_unit": 4.7,         # measured 4.6096  (lap-fans-T5)
    "lap_grad": 2.6,         # measured 2.5587  (lap-fans-T5)
    "quat_grad": 0.85,       # measured 0.8457  (quat-256-free)
}


# ------------------------------------------------------------------------------------------------ value + scale arithmetic
class S:
    """A numpy array `v` and the scale `s` of each of its elements (module docstring)."""
    __slots__ = ("v", "s")

    def __init__(self, v, s=None):
        self.v = v
        self.s = np.abs(v) if s is None else s

    def __getitem__(self, k):
        return S(self.v[k], self.s[k])

    def __neg__(self):
        return S(-self.v, self.s)

    def __add__(self, o):
        return S(self.v + o.v, self.s + o.s)

    def __sub__(self, o):
        return S(self.v - o.v, self.s + o.s)

    def __mul__(self, o):
        return S(self.v * o.v, np.abs(self.v) * o.s + np.abs(o.v) * self.s + U * self.s * o.s)

    def __truediv__(self, o):
        return S(self.v / o.v, self.s / np.abs(o.v) + np.abs(self.v) * o.s / (o.v * o.v))

    def times(self, c):
        """By an exact constant (or array of constants)."""
        return S(self.v * c, self.s * np.abs(c))

    def sum(self, axis):
        """Over the last axis, left to right (np.sum picks its order by the CPU's vector width: not the same on every machine)."""
        assert axis == -1
        out = self[..., 0]
        for k in range(1, self.v.shape[-1]):
            out = out + self[..., k]
        return out

    def sqrt(self):
        """Of a non-negative number: first order where that is finite, never more than sqrt(scale)."""
        r = np.sqrt(self.v)
        with np.errstate(divide="ignore", invalid="ignore"):
            first = np.where(r > 0, self.s / (2 * r), np.inf)
        return S(r, np.minimum(first, np.sqrt(self.s)).astype(r.dtype))

    def where(self, cond, other=None):
        """self where `cond` (an exact decision), else `other` (default: the constant 0 of scale 0)."""
        z = np.zeros((), self.v.dtype)
        return S(np.where(cond, self.v, z if other is None else other.v), np.where(cond, self.s, z if other is None else other.s))


def stack(parts):
    return S(np.stack([p.v for p in parts], -1), np.stack([p.s for p in parts], -1))


def cross(a, b):
    (a0, a1, a2), (b0, b1, b2) = (a[..., k] for k in range(3)), (b[..., k] for k in range(3))
    return stack([a1 * b2 - a2 * b1, a2 * b0 - a0 * b2, a0 * b1 - a1 * b0])


def dot(a, b):
    return (a * b).sum(-1)


def col(a):
    """[n] -> [n,1], to broadcast a per-row number over the 3 components."""
    return S(a.v[..., None], a.s[..., None])


def scatter(idx, a, n):
    """out[idx[k]] += a[k] over the first axis (np.add.at: one addition per entry, in order)."""
    out = S(np.zeros((n,) + a.v.shape[1:], a.v.dtype), np.zeros((n,) + a.v.shape[1:], a.v.dtype))
    np.add.at(out.v, idx, a.v)
    np.add.at(out.s, idx, a.s)
    return out


def _over_t(fn, T):
    """Run fn(t) -> tuple of S for every timestamp and stack each output along a new first axis."""
    rows = [fn(t) for t in range(T)]
    return tuple(S(np.stack([r[k].v for r in rows]), np.stack([r[k].s for r in rows])) for k in range(len(rows[0])))


# ------------------------------------------------------------------------------------------------ the reference
Csr = namedtuple("Csr", "off nbr rev w e")      # int64 [V+1], int64 [E], int64 [E], float32 [E], float32 [E,3]


def arap_reference(csr, x, R, g, f=np.float64):
    """E_t = sum_i sum_j w_ij |(x'_i - x'_j) - R_i e_ij|^2 per source vertex, and the gradients of sum_t g_t E_t:
    -> (energy [T,V], g_xyz [T,V,3], g_rot [T,V,3,3]) as S."""
    V = len(csr.off) - 1
    src = np.repeat(np.arange(V), np.diff(csr.off))
    nbr, W, E = csr.nbr, S(csr.w.astype(f)), S(csr.e.astype(f))

    def one(t):
        X, Rt = S(x[t].astype(f)), S(R[t].astype(f))
        s = (X[src] - X[nbr]) - (Rt[src] * S(E.v[:, None, :], E.s[:, None, :])).sum(-1)      # residual of every edge [E,3]
        ws = col(W) * s
        two_g = f(2) * f(g[t])
        energy = scatter(src, W * dot(s, s), V)
        gx = (scatter(src, ws, V) - scatter(nbr, ws, V)).times(two_g)                       # +2 w s to the source, -2 w s to the target
        gR = -scatter(src, S(ws.v[:, :, None], ws.s[:, :, None]) * S(E.v[:, None, :], E.s[:, None, :]), V).times(two_g)
        return energy, gx, gR

    return _over_t(one, len(x))


def nc_reference(pairs, V, x, g, f=np.float64):
    """Per pair (v0, v1, a, b): n0 = (v1 - v0) x (a - v0), m = (b - v0) x (v1 - v0), term = 1 - n0.m / (max(|n0|, eps) max(|m|, eps)),
    and the gradient of sum_t g_t mean_p term: -> (terms [T,P], g_xyz [T,V,3]) as S."""
    P = len(pairs)
    eps = f(NC_EPS)

    def one(t):
        X = S(x[t].astype(f))
        p0, p1, pa, pb = (X[pairs[:, k]] for k in range(4))
        e, a, b = p1 - p0, pa - p0, pb - p0
        n0, m = cross(e, a), cross(b, e)
        r0, r1 = dot(n0, n0).sqrt(), dot(m, m).sqrt()
        big0, big1 = r0.v > eps, r1.v > eps
        const = S(np.full(P, eps, f), np.zeros(P, f))
        l0, l1 = r0.where(big0, const), r1.where(big1, const)
        c = dot(n0, m) / (l0 * l1)
        term = S(np.ones(P, f)) - c
        inv01 = S(np.ones(P, f), np.zeros(P, f)) / (l0 * l1)
        c00, c11 = (c / (l0 * l0)).where(big0), (c / (l1 * l1)).where(big1)      # a clamped norm is a constant: no second term
        g0 = -(m * col(inv01) - n0 * col(c00))                                   # d term / d n0
        g1 = -(n0 * col(inv01) - m * col(c11))                                   # d term / d m
        dE, dA, dB = cross(a, g0) + cross(g1, b), cross(g0, e), cross(e, g1)
        d0 = -((dE + dA) + dB)
        gx = ((scatter(pairs[:, 0], d0, V) + scatter(pairs[:, 1], dE, V)) + scatter(pairs[:, 2], dA, V)) + scatter(pairs[:, 3], dB, V)
        return term, gx.times(f(g[t]) / f(P))

    return _over_t(one, len(x))


def nc_normals(pairs, x, f=np.float32):
    """(|n0|, |m|) [T,P] of every pair in dtype f, unclamped: what the clamp decides on."""
    X = np.asarray(x, f)
    p0, p1, pa, pb = (X[:, pairs[:, k]] for k in range(4))
    n0, m = np.cross(p1 - p0, pa - p0), np.cross(pb - p0, p1 - p0)
    return np.sqrt((n0 * n0).sum(-1)), np.sqrt((m * m).sum(-1))


def lap_reference(off, nbr, x, g, f=np.float64):
    """d_i = mean_{j in N(i)} v_j - v_i (0 for an isolated vertex), term = |d|, unit = d / |d| (0 where |d| == 0), and the
    gradient of sum_t g_t mean_i term_i = (sum_{j in N(i)} unit_j / deg_j - unit_i) g_t / V:
    -> (terms [T,V], unit [T,V,3], g_xyz [T,V,3]) as S."""
    V = len(off) - 1
    deg = np.diff(off)
    src = np.repeat(np.arange(V), deg)
    degf = np.maximum(deg, 1).astype(f)

    def one(t):
        X = S(x[t].astype(f))
        d = (scatter(src, X[nbr], V).times(1 / degf[:, None]) - X).where((deg > 0)[:, None])
        n = dot(d, d).sqrt()
        unit = (d / col(S(np.where(n.v > 0, n.v, 1).astype(f), n.s))).where((n.v > 0)[:, None])
        gx = (scatter(src, unit[nbr].times(1 / degf[nbr][:, None]), V) - unit).times(f(g[t]) / f(V))
        return n, unit, gx

    return _over_t(one, len(x))


def quat_reference(q, G, f=np.float64):
    """R(q) of pypose's SO3.matrix() for q = (x, y, z, w) (not normalised), and pypose's backward
    (sum_c R[:, c] x G[:, c], 0): -> (R [n,3,3], g_quat [n,4]) as S."""
    Q = S(q.astype(f))
    x, y, z, w = (Q[:, k] for k in range(4))
    one = S(np.ones(len(q), f))
    R = [one - (y * y + z * z).times(f(2)), (x * y - z * w).times(f(2)), (x * z + y * w).times(f(2)),
         (x * y + z * w).times(f(2)), one - (x * x + z * z).times(f(2)), (y * z - x * w).times(f(2)),
         (x * z - y * w).times(f(2)), (y * z + x * w).times(f(2)), one - (x * x + y * y).times(f(2))]
    Gs = S(G.astype(f))
    t = None
    for c in range(3):
        o = cross(stack([R[c], R[3 + c], R[6 + c]]), Gs[:, :, c])
        t = o if t is None else t + o
    zero = np.zeros((len(q), 1), f)
    Rm = stack(R)
    return S(Rm.v.reshape(-1, 3, 3), Rm.s.reshape(-1, 3, 3)), S(np.concatenate([t.v, zero], 1), np.concatenate([t.s, zero], 1))


# ------------------------------------------------------------------------------------------------ meshes
def _grid(v):
    """float32 vertices on the 2^-12 grid."""
    return np.ascontiguousarray(np.round(np.asarray(v, np.float64) * 4096.0) / 4096.0, np.float32)


def _fan(n, closed, centre, height=0.5, radius=1.0, phase=0.3):
    """A cone: centre vertex first, then n rim vertices; faces (centre, rim k, rim k+1)."""
    ang = phase + 2 * np.pi * np.arange(n) / (n if closed else 2 * n)
    rim = np.stack([radius * np.cos(ang), radius * np.sin(ang), np.zeros(n)], 1)
    v = np.concatenate([[[0.0, 0.0, height]], rim]) + np.asarray(centre, np.float64)
    k = np.arange(n if closed else n - 1)
    return v, np.stack([np.zeros_like(k), 1 + k, 1 + (k + 1) % n], 1)


def _join(parts):
    """Disjoint union of (verts, faces) components; a component without faces is a set of isolated vertices."""
    vs, fs, base = [], [], 0
    for v, f in parts:
        vs.append(np.asarray(v, np.float64).reshape(-1, 3))
        fs.append(np.asarray(f, np.int64).reshape(-1, 3) + base)
        base += len(vs[-1])
    return _grid(np.concatenate(vs)), np.concatenate(fs)


NO_FACES = np.zeros((0, 3), np.int64)
FAN_VALENCES = (3, 7, 8, 9, 15, 16, 17, 33, 300)
OPEN_FANS = (5, 6)           # rim vertices = valence of the centre; the two end vertices of the rim have valence 2


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(verts float32 [V,3], faces int64 [F,3]) of a named mesh."""
    if name == "fans":       # closed fans of every valence class, two open fans, an isolated vertex in the middle and one at V - 1
        parts = [_fan(n, True, (2.5 * (i % 4), 2.5 * (i // 4), 0.25 * i)) for i, n in enumerate(FAN_VALENCES)]
        parts.insert(4, ([[1.25, 1.25, -0.5]], NO_FACES))
        parts += [_fan(n, False, (2.5 * i, -2.5, 0.5)) for i, n in enumerate(OPEN_FANS)]
        parts.append(([[-1.5, 0.75, 0.25]], NO_FACES))
        return _join(parts)
    if name.startswith("fan-"):                                   # one closed fan: V = n + 1 vertices, P = n pairs
        return _join([_fan(int(name[4:]) - 1, True, (0.25, -0.5, 0.125))])
    if name == "lone":                                            # V = 1: one isolated vertex
        return _join([([[0.25, -0.5, 1.0]], NO_FACES)])
    if name.startswith("strip-"):                                 # triangle strip with P interior edges: P + 1 faces, P + 3 vertices
        P = int(name[6:])
        k = np.arange(P + 3)
        v = np.stack([0.25 * k, (k % 2) * 0.5 + 0.03 * np.sin(0.7 * k), 0.1 * np.cos(0.4 * k)], 1)
        j = np.arange(P + 1)
        return _join([(v, np.where((j % 2 == 0)[:, None], np.stack([j, j + 1, j + 2], 1), np.stack([j + 1, j, j + 2], 1)))])
    if name == "square":     # a vertex exactly at the centroid of its ring, a fan of valence 8 beside it, an isolated vertex
        sq = ([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0]], [[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1]])
        return _join([sq, _fan(8, True, (3.0, 0.5, 0.25)), ([[5.0, 5.0, 5.0]], NO_FACES)])
    if name == "special":
        return _special()
    raise ValueError(name)


SPECIAL = {}                 # what -> vertex indices (v0, v1, a, b) of the pair the special mesh builds for it


def _special():
    """The normal-consistency edge cases, one component each (integer coordinates where an exact zero is wanted)."""
    v, f = [], []

    def add(points, faces):
        base = len(v)
        v.extend(points)
        f.extend([[base + i for i in face] for face in faces])
        return base

    b = add([(0, 0, 0), (2, 0, 0), (0, 3, 0), (1, -2, 0)], [(0, 1, 2), (1, 0, 3)])
    SPECIAL["flat"] = (b, b + 1, b + 2, b + 3)                                              # coplanar: term 0
    b = add([(0, 0, 2), (2, 0, 2), (1, 2, 2), (1, 2, 2)], [(0, 1, 2), (1, 0, 3)])
    SPECIAL["folded"] = (b, b + 1, b + 2, b + 3)                                            # folded onto itself: cos = -1, term 2
    b = add([(0, 0, 4), (1, 0, 4), (0.3, 0.9, 4.2), (0.6, -0.8, 4.5), (0.4, 0.1, 3.1)], [(0, 1, 2), (1, 0, 3), (0, 1, 4)])
    SPECIAL["three_faces"] = (b, b + 1)                                                     # 3 faces on one edge: 3 pairs
    b = add([(3, 0, 4), (4, 0, 4), (3.3, 0.9, 4.2), (3.6, -0.8, 4.5), (3.4, 0.1, 3.1), (3.5, 0.7, 3.4)],
            [(0, 1, 2), (1, 0, 3), (0, 1, 4), (1, 0, 5)])
    SPECIAL["four_faces"] = (b, b + 1)                                                      # 4 faces on one edge: 6 pairs
    b = add([(0, 3, 1), (1.1, 3.2, 1.3), (0.4, 4.1, 0.8)], [(0, 1, 2), (0, 1, 2)])
    SPECIAL["duplicate"] = (b, b + 1, b + 2, b + 2)                                         # a face twice: a == b, term 2
    b = add([(0, 0, 6), (4, 0, 6), (2, 0, 6), (1, 3, 6)], [(0, 1, 2), (1, 0, 3)])
    SPECIAL["zero_first"] = (b, b + 1, b + 2, b + 3)                                        # first face collinear: |n0| = 0 exactly
    b = add([(0, 0, 7), (6, 0, 7), (2, 0, 7), (3, 0, 7)], [(0, 1, 2), (1, 0, 3)])
    SPECIAL["zero_both"] = (b, b + 1, b + 2, b + 3)                                         # both faces collinear
    b = add([(0.1, 0.2, 5.3), (1.1, 0.2, 5.3), (0.6, 0.201, 5.3), (0.55, 0.1993, 5.3007)], [(0, 1, 2), (1, 0, 3)])
    SPECIAL["slivers"] = (b, b + 1, b + 2, b + 3)                                           # height 1e-3 of the shared edge
    k = np.arange(8)
    b = add([(4 + 0.5 * i, 3 + 0.5 * (i % 2), 0.1 * i * i) for i in k], [(j, j + 1, j + 2) if j % 2 == 0 else (j + 1, j, j + 2) for j in range(6)])
    SPECIAL["four_roles"] = (b + 3,)                                                        # a strip's inner vertex: v0, v1, a and b
    b = add([(7, 7, 7)], [])
    SPECIAL["no_pair"] = (b,)
    # NOT on the 2^-12 grid: the slivers need their 1e-3; float32 values all the same
    return np.ascontiguousarray(np.asarray(v, np.float64), np.float32), np.asarray(f, np.int64)


def hand_csr():
    """A symmetric CSR no triangle mesh has (ARAP only): a star whose 9 leaves have valence 1, a two-vertex chain, a vertex of
    valence 4 with asymmetric weights, and zero-weight reverse edges as the kNN coach makes them.
    -> (rest vertices float32 [V,3], Csr)."""
    rng = np.random.default_rng(77)
    edges = [(0, j) for j in range(1, 10)] + [(10, 11)] + [(12, 13), (12, 14), (12, 15), (12, 16), (13, 14)]
    V = 17
    verts = _grid(rng.uniform(-1, 1, size=(V, 3)) + [0.5, -1.0, 2.0])
    w = {}
    for n, (a, b) in enumerate(edges):
        w[(a, b)] = float(np.float32(rng.uniform(0.1, 1.0)))
        w[(b, a)] = 0.0 if n % 3 == 0 else float(np.float32(rng.normal()))                  # one-way edges, asymmetric and negative weights
    keys = sorted(w)
    src, nbr = np.asarray([k[0] for k in keys]), np.asarray([k[1] for k in keys])
    off = np.zeros(V + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(src, minlength=V))
    pos = {k: i for i, k in enumerate(keys)}
    rev = np.asarray([pos[(b, a)] for a, b in keys], np.int64)
    return verts, Csr(off, nbr.astype(np.int64), rev, np.asarray([w[k] for k in keys], np.float32), (verts[src] - verts[nbr]).astype(np.float32))


# ------------------------------------------------------------------------------------------------ cases
Case = namedtuple("Case", "name kind mesh T seed")
UPSTREAM = {1: [1.0], 2: [-1.5, 0.75], 5: [1.0, 0.0, -0.5, 2.0, 0.25]}      # per timestamp: a zero and a negative weight
AMPLITUDE = {1: [0.05], 2: [0.02, 0.3], 5: [0.3, 0.01, 0.1, 0.03, 0.2]}    # per timestamp

CASES = [
    # ARAP: the modes of a timestamp are (deformation, rotation); see _arap_inputs
    Case("arap-fans-T5", "arap", "fans", 5, 1), Case("arap-fans-rest-T2", "arap", "fans", 2, 2),
    Case("arap-lone-T1", "arap", "lone", 1, 3), Case("arap-fan31-T2", "arap", "fan-31", 2, 4),
    Case("arap-fan32-T5", "arap", "fan-32", 5, 5), Case("arap-fan33-T1", "arap", "fan-33", 1, 6),
    Case("arap-hand-T2", "arap", "hand", 2, 7), Case("arap-hand-rest-T2", "arap", "hand", 2, 8),
    Case("nc-fans-T5", "nc", "fans", 5, 11), Case("nc-special-T2", "nc", "special", 2, 12),
    Case("nc-strip1-T2", "nc", "strip-1", 2, 13), Case("nc-strip255-T1", "nc", "strip-255", 1, 14),
    Case("nc-strip256-T5", "nc", "strip-256", 5, 15), Case("nc-strip257-T2", "nc", "strip-257", 2, 16),
    Case("lap-fans-T5", "lap", "fans", 5, 21), Case("lap-square-T2", "lap", "square", 2, 22),
    Case("lap-lone-T1", "lap", "lone", 1, 23), Case("lap-fan31-T1", "lap", "fan-31", 1, 24),
    Case("lap-fan32-T2", "lap", "fan-32", 2, 25), Case("lap-fan33-T5", "lap", "fan-33", 5, 26),
] + [Case(f"quat-{n}-{'unit' if unit else 'free'}", "quat", (n, unit), 1, 30 + n) for n in (1, 255, 256, 257) for unit in (True, False)]
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
KINDS = {"arap": ("arap_energy", "arap_g_xyz", "arap_g_rot"), "nc": ("nc_term", "nc_grad"),
         "lap": ("lap_term", "lap_unit", "lap_grad"), "quat": ("quat_grad",)}
ARAP_MODES = {   # case -> per timestamp (deformation, rotation)
    "arap-fans-T5": [("small", "small"), ("large", "random"), ("mid", "random"), ("large", "general"), ("small", "identity")],
    "arap-fans-rest-T2": [("rest", "identity"), ("translated", "identity")],
    "arap-lone-T1": [("large", "general")],
    "arap-fan31-T2": [("mid", "random"), ("small", "small")],
    "arap-fan32-T5": [("large", "general"), ("small", "small"), ("mid", "random"), ("large", "random"), ("mid", "general")],
    "arap-fan33-T1": [("mid", "random")],
    "arap-hand-T2": [("large", "general"), ("small", "small")],
    "arap-hand-rest-T2": [("rest", "identity"), ("translated", "identity")],
}
TRANSLATION = (0.5, -2.0, 8.0)


def _quat_matrix(q):
    x, y, z, w = (q[..., k] for k in range(4))
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                     2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(q.shape[:-1] + (3, 3))


def host_tables(mesh_name):
    """The float32 / int tables the kernels read for a mesh, built by the product's host code on the CPU:
    -> dict(verts, faces, csr (ARAP), pairs, nc_off, nc_items (normal consistency), lap_off, lap_nbr (Laplacian))."""
    return dict(_host_tables(mesh_name))


@functools.lru_cache(maxsize=None)
def _host_tables(mesh_name):
    from dreammesh4d_amd.mesh_reg import ARAPCoach, MeshLaplacianSmoothing, MeshNormalConsistency

    if mesh_name == "hand":
        verts, csr = hand_csr()
        return (("verts", verts), ("faces", None), ("csr", csr))
    verts, faces = mesh(mesh_name)
    V = len(verts)
    i64 = lambda t: t.numpy().astype(np.int64)
    coach = ARAPCoach(verts, faces, "cpu")
    E = int(coach._off[-1])
    csr = Csr(i64(coach._off), i64(coach._nbr)[:E], i64(coach._rev)[:E], cot_weights(verts, faces, i64(coach._off), i64(coach._nbr)[:E]),
              coach._e.numpy()[:E].copy())
    nc = MeshNormalConsistency(faces, V, "cpu")
    ls = MeshLaplacianSmoothing(faces, V, "cpu")
    return (("verts", verts), ("faces", faces), ("csr", csr), ("pairs", i64(nc._pairs)[:nc.n_pairs]), ("nc_off", i64(nc._off)),
            ("nc_items", i64(nc._items)[:4 * nc.n_pairs]), ("lap_off", i64(ls._off)), ("lap_nbr", i64(ls._nbr)[:int(ls._off[-1])]))


def cot_weights(verts, faces, off, nbr):
    """The coach's edge weights (Heron's area clamped at 1e-12, 0.5 cot / 4 assigned per directed edge with later faces winning,
    then W + W^T) in float64 numpy from the float32 vertices, rounded once to float32 [E]: the same bits on every machine."""
    v = np.asarray(verts, np.float64)
    directed = {}
    for f in np.asarray(faces).tolist():
        p = v[f]
        A, B, C = (float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])) for d in (p[1] - p[2], p[0] - p[2], p[0] - p[1]))
        s = 0.5 * (A + B + C)
        area = np.sqrt(max(s * (s - A) * (s - B) * (s - C), 1e-12))
        cot = [(B * B + C * C - A * A) / area / 4.0, (A * A + C * C - B * B) / area / 4.0, (A * A + B * B - C * C) / area / 4.0]
        for k in range(3):
            directed[(f[k], f[(k + 1) % 3])] = 0.5 * cot[k]
    src = np.repeat(np.arange(len(off) - 1), np.diff(off))
    return np.asarray([directed.get((a, b), 0.0) + directed.get((b, a), 0.0) for a, b in zip(src.tolist(), nbr.tolist())], np.float64).astype(np.float32)


def _shortest_edge(verts, csr):
    """Per vertex, the length of its shortest incident edge (1 for a vertex without edges)."""
    V = len(verts)
    out = np.full(V, np.inf)
    src = np.repeat(np.arange(V), np.diff(csr.off))
    np.minimum.at(out, src, np.linalg.norm(csr.e.astype(np.float64), axis=1))
    return np.where(np.isfinite(out), out, 1.0)


@functools.lru_cache(maxsize=None)
def _case_inputs(name):
    case = CASE_BY_NAME[name]
    rng = np.random.default_rng([case.seed, 5])
    g = np.asarray(UPSTREAM[case.T], np.float32)
    if case.kind == "quat":
        n, unit = case.mesh
        q = rng.normal(size=(n, 4))
        q = q / np.linalg.norm(q, axis=1, keepdims=True) if unit else q * rng.uniform(0.2, 3.0, size=(n, 1))
        return (("q", q.astype(np.float32)), ("G", rng.normal(size=(n, 3, 3)).astype(np.float32)))
    tab = host_tables(case.mesh)
    verts = tab["verts"]
    V = len(verts)
    if case.kind == "arap":
        short = _shortest_edge(verts, tab["csr"])[:, None]
        x, R = [], []
        for dmode, rmode in ARAP_MODES[name]:
            noise = rng.normal(size=(V, 3))
            if dmode == "rest":
                x.append(verts)
            elif dmode == "translated":
                x.append(verts + np.asarray(TRANSLATION, np.float32))
            else:
                amp = {"small": 1e-4 * short, "mid": 0.05, "large": 0.5}[dmode]
                x.append((verts.astype(np.float64) + amp * noise).astype(np.float32))
            if rmode == "identity":
                R.append(np.broadcast_to(np.eye(3, dtype=np.float32), (V, 3, 3)))
            elif rmode == "general":                                # not orthonormal: the kernel must not assume it
                R.append(rng.normal(size=(V, 3, 3)).astype(np.float32))
            else:
                q = np.concatenate([(1e-4 if rmode == "small" else 1.0) * rng.normal(size=(V, 3)), np.ones((V, 1))], 1)
                R.append(_quat_matrix(q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32))
        return (("x", np.ascontiguousarray(np.stack(x), np.float32)), ("R", np.ascontiguousarray(np.stack(R), np.float32)), ("g", g))
    if case.mesh == "special":          # t = 0 as built; t = 1 an integer shear of it (collinear stays collinear, exactly)
        v64 = verts.astype(np.float64)
        shear = np.stack([v64[:, 0] + 2 * v64[:, 1], v64[:, 1] - v64[:, 2], v64[:, 2] * 2], 1)
        return (("x", np.ascontiguousarray(np.stack([v64, shear]), np.float32)), ("g", g))
    if case.mesh == "square":           # the centroid component stays as it is (t = 1: doubled), the rest is deformed
        amp = np.asarray(AMPLITUDE[case.T])[:, None, None] * rng.normal(size=(case.T, V, 3))
        amp[:, :5] = 0.0
        x = verts.astype(np.float64)[None] * np.asarray([1.0, 2.0])[:, None, None] + amp
        return (("x", np.ascontiguousarray(x, np.float32)), ("g", g))
    x = verts.astype(np.float64)[None] + np.asarray(AMPLITUDE[case.T])[:, None, None] * rng.normal(size=(case.T, V, 3))
    return (("x", np.ascontiguousarray(x, np.float32)), ("g", g))


def case_inputs(name):
    """float32 inputs of a case (shared, do not modify): x [T,V,3] and g [T] (+ R [T,V,3,3] for ARAP); q [n,4] and G [n,3,3]."""
    return dict(_case_inputs(name))


def reference(name, f=np.float64):
    """kind -> S of every tensor kind of a case, in dtype f."""
    case, inp = CASE_BY_NAME[name], case_inputs(name)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if case.kind == "quat":
            return {"quat_R": (out := quat_reference(inp["q"], inp["G"], f))[0], "quat_grad": out[1]}
        tab = host_tables(case.mesh)
        if case.kind == "arap":
            out = arap_reference(tab["csr"], inp["x"], inp["R"], inp["g"], f)
        elif case.kind == "nc":
            out = nc_reference(tab["pairs"], len(tab["verts"]), inp["x"], inp["g"], f)
        else:
            out = lap_reference(tab["lap_off"], tab["lap_nbr"], inp["x"], inp["g"], f)
    return dict(zip(KINDS[case.kind], out))


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """The float64 reference of a case, computed once per process and shared (callers must not modify it)."""
    return reference(name, np.float64)


def ratio(got, ref, yard=1.0):
    """Elementwise |got - ref.v| / (yard 2^-24 ref.s); where the scale is 0: 0 if exact, else inf.  Non-finite `got` -> inf."""
    got = np.asarray(got, np.float64).reshape(ref.v.shape)
    err, bd = np.abs(got - ref.v.astype(np.float64)), yard * U * ref.s.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, np.where(bd > 0, err / bd, np.inf))
    return np.where(np.isfinite(got), r, np.inf)


def float32_ratios(name):
    """kind -> worst ratio of the float32 restatement of one case against its float64 reference (what the yardsticks are made of)."""
    r64, r32 = case_reference(name), reference(name, np.float32)
    return {k: float(ratio(r32[k].v, r64[k]).max(initial=0.0)) for k in KINDS[CASE_BY_NAME[name].kind]}


def compare(kind, got, ref, what):
    """(worst error / bound, None or a message naming the worst element) of `got` against the S `ref` under the bound of `kind`."""
    r = ratio(got, ref, FACTOR * YARD[kind])
    worst = float(r.max(initial=0.0))
    if worst <= 1.0:
        return worst, None
    i = np.unravel_index(int(r.argmax()), r.shape)
    g = np.asarray(got, np.float64).reshape(ref.v.shape)
    return worst, (f"{what}: {int((r > 1).sum())} of {r.size} elements off; worst at {tuple(int(j) for j in i)}: got {g[i]:.9g}, float64 "
                   f"{ref.v[i]:.9g}, |diff| {abs(g[i] - ref.v[i]):.3g} > {FACTOR:g} x {YARD[kind]:g} x 2^-24 x scale {ref.s[i]:.3g}")
