"""Cases, plain references and the error bounds of tests/test_dynamic_glue_edges_{cpu,gpu}.py (TEST INFRASTRUCTURE).

The small fused kernels a dynamic-stage iteration runs between the renderer, the guidance and the optimiser, judged element by element:
  * dreammesh4d_amd/csrc/imagehead.hip: k_head_fwd / k_head_bwd (dm4d_image_head_*: per-workgroup partial sums, the two means, the
    half-size image, dL/dcolor, dL/dalpha), k_partial_sums, k_weighted_sum, k_weighted_sum_bwd;
  * dreammesh4d_amd/csrc/dscale.hip: k_vscale_fwd / _bwd, k_gscale_fwd / _bwd_vertex / _bwd_scaling (Sv, g_ds, g_dop, gscales, g_sv,
    g_scaling);
  * dreammesh4d_amd/csrc/sds_glue.hip: k_sds_prepare / k_sds_finish.

Image head, loss sums, d_scale.  The reference states every value and gradient in closed form in numpy (`np.add.at` scatters; no
autograd, no code of image_head.py, loss_sum.py, ops.py, dynamic_stage.py or oracle/) and reads the float32 inputs the kernels read,
widened to float64 -- the constant 0.4f of the hybrid clamp and the float32 normalisation factors of the means included.  Scale and
bound are those of tests/mesh_reg_edges.py (class `S`, imported): a kernel element may differ from the float64 reference by
FACTOR x YARD[kind] x 2^-24 x scale, YARD[kind] being the worst error of this same reference run in np.float32 over all cases; an
element decided by a branch on exact data has scale 0 and must match exactly.  exp is carried as tests/static_kernels_edges.py carries
it (scale exp(x) (1 + |x|); the float32 restatement takes it in float64 and rounds once).  Nothing is measured against the kernels.
tests/test_dynamic_glue_edges_cpu.py pins the reference to float64 autograd through the torch compositions the project keeps.

The hybrid clamp  lw = min(sum_k w o + 0.4f, 1).  torch.clamp passes the gradient where x <= max, the bound included.  The equality
vertices have dop = 0 on both their nodes (o = 0.5 exactly) and w = (1.0f, 3355443 x 2^-24): 0.5 + 3355443 x 2^-25 + 13421773 x 2^-25
is exactly 1 in float64, and float32 rounds both of its additions to 1.0f.  The reference asserts that, in both precisions, for every
equality vertex, and a margin of 1e-4 from the clamp for every other vertex.

SDS glue.  The kernels' contract is "the torch float16 graph's roundings", so their reference is that expression restated in numpy
with one explicit rounding per torch operator (`sds_restate`), on the CPU, with none of the project's code.  Bit-identical: latents,
x_in, t2, the clamp mask.  loss and |grad| against the float64 sum of the restatement's terms under the scale bound.  d_moments may
differ from the restatement in at most 0.1 % of a case's elements by at most 2 float16 ulps (expf's last bit carried through two
float16 roundings): conditions, not measurements.  So that `latents` can be bit-identical at all, every log-variance of every case is
one whose float16(exp(lv / 2)) does not hinge on the last bits of expf: exp lies at least 8 float32 ulps from a float16 rounding
midpoint (`_safe_logvar`; the CPU test asserts it).

UNREACHABLE, therefore unpinned:
  * imagehead.hip `half_rgb == nullptr` with a view whose rnd_pos < n_rnd: dm4d_image_head_forward refuses a null half_rgb unless
    n_rnd == 0, and then no view satisfies n < n_rnd (`head_reference` asserts `is_rnd` is False everywhere when n_rnd == 0).
  * dscale.hip: sigmoid(-20) is an ordinary number (2.06e-9), only the upper end saturates (1 + exp(-20) == 1.0f): `vscale_reference`
    asserts o(1 - o) == 0 in float32 exactly on the nodes with dop = 20 and > 0 on those with dop = -20.
  * sds_glue.hip: after nan_to_num `g` is never NaN, so fminf / fmaxf of the clip never see one (`sds_restate` asserts it).
"""
import functools
from collections import namedtuple

import numpy as np

from tests.mesh_reg_edges import FACTOR, S, U, col, ratio, scatter, stack
from tests.static_kernels_edges import _const, _exp, _num, _zero

C04 = np.float32(0.4)                               # the kernels' 0.4f
W_EQ = np.float32(3355443 * 2.0 ** -24)             # with w = (1, W_EQ) and o = 0.5 twice: lw + 0.4f == 1 in both precisions
FLT_MAX = np.float32(3.4028234663852886e38)

# ---- yardsticks: worst |float32 restatement - float64 reference| / (2^-24 scale) over all cases, per tensor kind, rounded up to two
#      digits (test_dynamic_glue_edges_cpu.py re-measures them: 0.8 x constant <= measured <= constant) ----
YARD = {
    "partial": 7.5,          # measured 7.4451  (head-516x512: ~1030 pixels of a workgroup added one by one)
    "means": 2.0,            # measured 1.9628  (head-516x512)
    "half": 1.9,             # measured 1.8800  (head-516x512)
    "g_color": 1.1,          # measured 1.0844  (head-516x512)
    "g_alpha": 1.2,          # measured 1.1882  (head-30x34)
    "psum": 1.4,             # measured 1.3797  (n256-k3-m8)
    "Sv": 1.7,               # measured 1.6250  (patch-K4-G6-T3-lbs)
    "g_ds": 1.4,             # measured 1.3601  (patch-K4-G6-T3-lbs)
    "g_dop": 0.47,           # measured 0.4640  (patch-K2-G1-T1-hybrid)   expf
    "gscales": 1.1,          # measured 1.0335  (patch-K2-G1-T1-lbs)
    "g_sv": 0.89,            # measured 0.8897  (patch-K4-G6-T3-lbs)
    "g_scaling": 0.97,       # measured 0.9601  (patch-K2-G1-T1-lbs)
    "sds_loss": 110.0,       # measured 101.2709 (sds-3x32x32: 12288 terms added one by one)
    "sds_norm": 51.0,        # measured 50.5859  (sds-3x32x32)
}
HEAD_KINDS = ("partial", "means", "half", "g_color", "g_alpha")
VS_KINDS = ("Sv", "g_ds", "g_dop")
GS_KINDS = ("gscales", "g_sv", "g_scaling")


def _join(parts):
    return S(np.stack([p.v for p in parts]), np.stack([p.s for p in parts]))


def _sum1(a):
    """Over axis 1, left to right."""
    out = a[:, 0]
    for k in range(1, a.v.shape[1]):
        out = out + a[:, k]
    return out


# ------------------------------------------------------------------------------------------------ image head: the reference
def head_blocks(H, W):
    """dm4d_image_head_blocks, taken as a fact: workgroups per view; pixel p belongs to workgroup (p / 256) mod blocks."""
    return max(1, min(256, (H * W + 1023) // 1024))


def head_reference(inp, f=np.float64):
    """kind -> S: partial [B,blocks,2], means [2], half [n_rnd,H/2,W/2,3], g_color [B,C,H,W], g_alpha [B,1,H,W]; "roles" [B,2]."""
    color, alpha = inp["color"], inp["alpha"]
    B, C, H, W = color.shape
    HW, nb = H * W, head_blocks(H, W)
    n_ref, n_rnd = inp["n_ref"], inp["n_rnd"]
    block = (np.arange(HW) // 256) % nb
    yy, xx = np.divmod(np.arange(HW), W)
    half = _zero((n_rnd, H // 2, W // 2, 3), f)
    part, gcol, galp, roles = [], [], [], []

    def scalar(g, den):              # g[0] * 2.0f / den, den an exact product of sizes
        assert den < 2 ** 24
        return S(np.full((), g, f)).times(f(2)) / _const(f(den), (), f)

    for v in range(B):
        r, n = int(inp["ref_pos"][v]), int(inp["rnd_pos"][v])
        is_ref, is_rnd = 0 <= r < n_ref, 0 <= n < n_rnd
        assert n_rnd > 0 or not is_rnd
        roles.append((is_ref, is_rnd))
        c32 = color[v, :3].reshape(3, HW).T                                             # [HW,3]
        lo, hi = c32 < 0, c32 > 1                                                       # on the float32 input
        rgb = S(c32.astype(f)).where(~(lo | hi), _num(1.0, (HW, 3), f).where(hi))       # (a 1 that enters sums: scale 1)
        A = S(alpha[v].reshape(HW).astype(f))
        sums = _zero((HW, 2), f)
        if is_ref:
            fi = int(inp["fidx_ref"][r])
            gt, gm = S(inp["ref_images"][fi].reshape(HW, 3).astype(f)), S(inp["ref_masks"][fi].reshape(HW).astype(f))
            d, dm = gt - rgb, A - gm
            sums = stack([(d * d).sum(-1), dm * dm])
        part.append(scatter(block, sums, nb))
        if is_rnd:
            R4 = S(rgb.v.reshape(H // 2, 2, W // 2, 2, 3), rgb.s.reshape(H // 2, 2, W // 2, 2, 3))
            h0 = R4[:, 0, :, 0].times(f(0.5)) + R4[:, 0, :, 1].times(f(0.5))
            h1 = R4[:, 1, :, 0].times(f(0.5)) + R4[:, 1, :, 1].times(f(0.5))
            hv = h0.times(f(0.5)) + h1.times(f(0.5))
            half.v[n], half.s[n] = hv.v, hv.s
        # ---- backward
        gk = _zero((HW, 3), f)
        if is_ref and inp["g_rgb"] is not None:
            k = scalar(inp["g_rgb"], n_ref * HW * 3)
            gk = S(np.full((HW, 3), k.v, f), np.full((HW, 3), k.s, f)) * (rgb - gt)
        if is_rnd and inp["g_half"] is not None:
            gk = gk + S(inp["g_half"][n].astype(f))[yy >> 1, xx >> 1].times(f(0.25))
        gk = gk.where((c32 >= 0) & (c32 <= 1))                                          # torch.clamp passes on [0, 1], bounds included
        ga = _zero(HW, f)
        if is_ref and inp["g_mask"] is not None:
            k = scalar(inp["g_mask"], n_ref * HW)
            ga = S(np.full(HW, k.v, f), np.full(HW, k.s, f)) * (A - gm)
        rest = np.zeros((C - 3, H, W), f)
        gcol.append(S(np.concatenate([gk.v.T.reshape(3, H, W), rest]), np.concatenate([gk.s.T.reshape(3, H, W), rest])))
        galp.append(S(ga.v.reshape(1, H, W), ga.s.reshape(1, H, W)))
    partial = _join(part)
    flat = S(partial.v.reshape(B * nb, 2).T, partial.s.reshape(B * nb, 2).T).sum(-1)        # the workgroups in order
    m_rgb, m_mask = head_matrix(n_ref, H, W)
    means = stack([flat[0].times(f(m_rgb)), flat[1].times(f(m_mask))])
    return dict(partial=partial, means=means, half=half, g_color=_join(gcol), g_alpha=_join(galp), roles=np.asarray(roles))


def head_matrix(n_ref, H, W):
    """The float32 factors F.mse_loss's normalisation reaches dm4d_partial_sums as."""
    d = float(max(n_ref, 1) * H * W)
    return np.float32(1.0 / (3.0 * d)), np.float32(1.0 / d)


# ------------------------------------------------------------------------------------------------ image head: the cases
HeadCase = namedtuple("HeadCase", "name B C H W ref_pos rnd_pos n_ref n_rnd L fidx seed")
HEAD_CASES = [
    # one workgroup with 252 idle lanes, one half-size pixel; reference only, random only, both, neither
    HeadCase("head-2x2", 4, 3, 2, 2, (1, -1, 0, -1), (-1, 1, 0, -1), 2, 2, 2, (1, 0), 1),
    # 1020 pixels, 255 half-size pixels: ragged tails; every role, ref_pos >= n_ref, rnd_pos >= n_rnd, two views on frame 2; C = 6
    HeadCase("head-30x34", 6, 6, 30, 34, (0, -1, 1, -1, 5, 2), (-1, 0, 1, -1, -1, 7), 3, 2, 3, (2, 0, 2), 2),
    HeadCase("head-64x2", 3, 3, 64, 2, (0, -1, -1), (-1, 1, 0), 1, 2, 1, (0,), 3),               # Wh = 1
    HeadCase("head-30x34-noref", 2, 3, 30, 34, (0, -1), (0, 1), 0, 2, 0, (), 4),                 # n_ref = 0: null reference tensors
    HeadCase("head-64x2-nornd", 2, 6, 64, 2, (0, 1), (-1, 0), 2, 0, 2, (1, 1), 5),               # n_rnd = 0: null half_rgb and g_half
    HeadCase("head-516x512", 2, 3, 516, 512, (0, -1), (-1, 0), 1, 1, 1, (0,), 6),                # 258 workgroups asked for, 256 given
]
HEAD_BY_NAME = {c.name: c for c in HEAD_CASES}
BIG = "head-516x512"
_F0, _F1 = np.float32(0), np.float32(1)
PLANT_RGB = (np.float32(-0.0), _F0, _F1, np.nextafter(_F0, -_F1), np.nextafter(_F1, np.float32(2)), np.nextafter(_F0, _F1),
             np.nextafter(_F1, _F0), np.float32(-0.3), np.float32(1.3))
HEAD_VARIANTS = ((True, True, True), (False, True, True), (True, False, True), (True, True, False))     # g_rgb, g_mask, g_half present


def head_planted(H, W):
    """Flat pixel positions that carry planted colours: the corners, the seams between workgroups and rounds, a few inner pixels."""
    HW = H * W
    pos = [0, W - 1, HW - W, HW - 1] + [p for p in (255, 256, 1019, 1023, 1024, 65535, 65536, 262143, 262144) if p < HW]
    return sorted(set(pos + [p for p in (W + 1, HW // 2, HW // 2 + 1) if p < HW]))


@functools.lru_cache(maxsize=None)
def _head_inputs(name):
    c = HEAD_BY_NAME[name]
    B, H, W = c.B, c.H, c.W
    rng = np.random.default_rng([c.seed, 41])
    color = rng.uniform(-0.3, 1.3, size=(B, c.C, H, W)).astype(np.float32)
    alpha = rng.uniform(0, 1, size=(B, 1, H, W)).astype(np.float32)
    for v in range(B):
        cf = color[v].reshape(c.C, -1)
        for j, p in enumerate(head_planted(H, W)):
            for k in range(3):
                cf[k, p] = PLANT_RGB[(j + v + 3 * k) % len(PLANT_RGB)]
    ref_images = rng.uniform(size=(c.L, H, W, 3)).astype(np.float32) if c.L else None
    ref_masks = (rng.uniform(size=(c.L, H, W, 1)) > 0.4).astype(np.float32) if c.L else None
    if c.L:
        ref_masks[rng.uniform(size=ref_masks.shape) > 0.8] = np.float32(0.3)
    g_half = rng.normal(size=(c.n_rnd, H // 2, W // 2, 3)).astype(np.float32) if c.n_rnd else None
    return tuple(dict(color=color, alpha=alpha, ref_pos=np.asarray(c.ref_pos, np.int32), rnd_pos=np.asarray(c.rnd_pos, np.int32),
                      ref_images=ref_images, ref_masks=ref_masks, fidx_ref=np.asarray(c.fidx, np.int64), n_ref=c.n_ref, n_rnd=c.n_rnd,
                      g_rgb=np.float32(1.25), g_mask=np.float32(-0.75), g_half=g_half).items())


def head_inputs(name, g_rgb=True, g_mask=True, g_half=True):
    """float32 inputs of a head case (shared, do not modify); a False flag: that upstream gradient is absent (a null pointer)."""
    inp = dict(_head_inputs(name))
    for k, keep in (("g_rgb", g_rgb), ("g_mask", g_mask), ("g_half", g_half)):
        if not keep:
            inp[k] = None
    return inp


@functools.lru_cache(maxsize=None)
def head_case_reference(name, g_rgb=True, g_mask=True, g_half=True):
    with np.errstate(all="ignore"):
        return head_reference(head_inputs(name, g_rgb, g_mask, g_half), np.float64)


def head_variants(name):
    c = HEAD_BY_NAME[name]
    return [v for v in (HEAD_VARIANTS[:1] if name == BIG else HEAD_VARIANTS) if v[2] or c.n_rnd]


# ------------------------------------------------------------------------------------------------ loss sums
PSUM_N = (0, 1, 255, 256, 257, 1000)
PSUM_KM = ((1, 1), (1, 3), (1, 8), (3, 1), (3, 3), (3, 8), (8, 1), (8, 3), (8, 8))
PSUM_CASES = [(n, k, m) for n in PSUM_N for k, m in PSUM_KM]


@functools.lru_cache(maxsize=None)
def psum_inputs(n, k, m):
    """(partial [n,k], matrix [k,m]) float32; the matrix has zero and negative entries wherever it has more than one entry."""
    rng = np.random.default_rng([n, k, m, 43])
    partial = (rng.normal(size=(n, k)) * np.exp(rng.uniform(-3, 3, size=(n, 1)))).astype(np.float32)
    mat = rng.uniform(0.1, 2.0, size=(k, m)).astype(np.float32)
    flat = mat.reshape(-1)
    flat[1::3] = 0.0
    flat[2::3] *= -1.0
    return partial, mat


def psum_reference(n, k, m, f=np.float64):
    """out[j] = sum_c mat[c][j] (sum_i partial[i][c]) -> S [m]."""
    partial, mat = psum_inputs(n, k, m)
    colsum = S(partial.T.astype(f)).sum(-1) if n else _zero(k, f)
    terms = S(mat.T.astype(f)) * S(colsum.v[None, :], colsum.s[None, :])                   # [m,k]
    return terms.sum(-1)


def wsum_cases():
    """name -> pairs [(weight, term)] as loss_sum.weighted_sum takes them (numpy float32 terms): n = 1; n = 16 with a vector term
    between scalars, a zero weight and a negative weight."""
    rng = np.random.default_rng(47)
    t = lambda *shape: (rng.normal(size=shape) * 3).astype(np.float32)
    one = [(1.75, t())]
    sixteen = [(0.5, t()), (-2.0, t()), (0.0, t()), (1e-3, t()), (3.0, t()), ((1.0, 0.0, -0.25, 2.0, 1e4, 1e-4, -1.0, 0.5), t(8)),
               (7.0, t()), (-0.125, t()), (1.0, t())]
    return {"n1": one, "n16": sixteen}


def wsum_reference(pairs, g):
    """(the float32 left-to-right expression, g x w_i per flattened term): bit-exact expectations."""
    acc, w = np.float32(0.0), []
    for wi, ti in pairs:
        for wj, tj in zip(np.atleast_1d(np.asarray(wi, np.float32)), np.atleast_1d(ti)):
            acc = np.float32(acc + np.float32(wj * tj))
            w.append(wj)
    return acc, np.float32(g) * np.asarray(w, np.float32)


# ------------------------------------------------------------------------------------------------ d_scale: the reference
def vscale_reference(inp, f=np.float64):
    """kind -> S: Sv [NF,V,3,3], g_ds [NF,M,6], g_dop [NF,M] (zeros under lbs); "lw" [NF,V] and "unclamped" [NF,V] under hybrid."""
    idx, NF, M = inp["idx"], inp["ds"].shape[0], inp["ds"].shape[1]
    V, K = idx.shape
    hybrid = inp["method"] == "hybrid"
    Wt = S(inp["w"].astype(f))
    fv, fm = np.repeat(np.arange(V), K), idx.reshape(-1)                                 # the records (v, k) in the CSR's order
    Wr = S(Wt.v.reshape(-1), Wt.s.reshape(-1))
    out = {k: [] for k in VS_KINDS}
    lws, uncl = [], []
    for fr in range(NF):
        Dn = S(inp["ds"][fr].astype(f))                                                  # [M,6]
        o = None
        if hybrid:
            o = _num(1.0, M, f) / (_num(1.0, M, f) + _exp(-S(inp["dop"][fr].astype(f)), f))
            c = Wt * o[idx]
        else:
            c = Wt
        c0 = c.sum(-1)
        s6 = _sum1(S(c.v[..., None], c.s[..., None]) * Dn[idx])                          # [V,6]
        un = np.ones(V, bool)
        if hybrid:
            lw = c0 + _num(C04, V, f)
            un = lw.v <= 1                                                               # clamp(max = 1): not clamped, the bound included
            eq = np.zeros(V, bool)
            eq[inp["eq_vertices"]] = True
            assert (lw.v[eq] == 1).all(), "an equality vertex is not at lw + 0.4f == 1"
            assert (np.abs(lw.v[~eq].astype(np.float64) - 1) >= 1e-4).all(), "a vertex within 1e-4 of the clamp that is not an equality vertex"
            c0 = c0 + (_num(1.0, V, f) - lw).where(un)
            lws.append(lw.v)
            uncl.append(un)
            sat, low = inp["dop"][fr] == 20, inp["dop"][fr] == -20
            if f == np.float32:
                assert not (o.v * (1 - o.v))[sat].any() and (o.v[sat] == 1).all()
            assert ((o.v * (1 - o.v))[low] > 0).all()
        out["Sv"].append(stack([c0 + s6[:, 0], s6[:, 3], s6[:, 4], s6[:, 3], c0 + s6[:, 1], s6[:, 5], s6[:, 4], s6[:, 5], c0 + s6[:, 2]]))
        # ---- backward: per node, over the (vertex, k) records that name it
        G = S(inp["g_Sv"][fr].reshape(V, 9).astype(f))
        tr = (G[:, 0] + G[:, 4]) + G[:, 8]
        sym = stack([G[:, 0], G[:, 4], G[:, 8], G[:, 1] + G[:, 3], G[:, 2] + G[:, 6], G[:, 5] + G[:, 7]])
        cw = Wr * o[fm] if hybrid else Wr
        out["g_ds"].append(scatter(fm, col(cw) * sym[fv], M))
        if hybrid:
            dot, d = tr[fv], Dn[fm]
            for j in range(6):
                dot = dot + sym[fv][:, j] * d[:, j]
            go = scatter(fm, Wr * (dot - tr[fv].where(un[fv])), M)                       # the (1 - lw) I term passes -w tr g while not clamped
            out["g_dop"].append((go * o) * (_num(1.0, M, f) - o))
        else:
            out["g_dop"].append(_zero(M, f))
    res = {k: _join(v) for k, v in out.items()}
    res["Sv"] = S(res["Sv"].v.reshape(NF, V, 3, 3), res["Sv"].s.reshape(NF, V, 3, 3))
    if hybrid:
        res["lw"], res["unclamped"] = np.stack(lws), np.stack(uncl)
    return res


def gscale_reference(inp, f=np.float64):
    """kind -> S: gscales [NF,N,3], g_sv [NF,V,3,3], g_scaling [N,3] from the float32 vertex matrices `sv_in`."""
    faces, NF = inp["faces"], inp["sv_in"].shape[0]
    V, F, G = inp["sv_in"].shape[1], len(inp["faces"]), len(inp["bary"])
    N = F * G
    face_of, g_of = np.repeat(np.arange(F), G), np.tile(np.arange(G), F)
    Bw, Sc = S(inp["bary"].astype(f)), S(inp["scaling"].astype(f))
    # the records (face, corner, g) in the order the vertex gather walks them
    rf, rc, rg = np.repeat(np.arange(F), 3 * G), np.tile(np.repeat(np.arange(3), G), F), np.tile(np.arange(G), 3 * F)
    ri = rf * G + rg
    outs, gsv, gsc = [], [], None
    for fr in range(NF):
        SV = S(inp["sv_in"][fr].reshape(V, 9).astype(f))
        D = None
        for c in range(3):
            term = col(Bw[g_of, c]) * SV[faces[face_of, c]]
            D = term if D is None else D + term
        outs.append(stack([(D[:, 3 * r] * Sc[:, 0] + D[:, 3 * r + 1] * Sc[:, 1]) + D[:, 3 * r + 2] * Sc[:, 2] for r in range(3)]))
        GO = S(inp["g_gs"][fr].astype(f))                                                # [N,3]
        bg = col(Bw[rg, rc]) * GO[ri]                                                    # [R,3]: b go[r]
        val = S(bg.v[:, :, None], bg.s[:, :, None]) * S(Sc.v[ri][:, None, :], Sc.s[ri][:, None, :])
        gsv.append(scatter(faces[rf, rc], S(val.v.reshape(-1, 9), val.s.reshape(-1, 9)), V))
        acc = stack([(D[:, j] * GO[:, 0] + D[:, 3 + j] * GO[:, 1]) + D[:, 6 + j] * GO[:, 2] for j in range(3)])
        gsc = acc if gsc is None else gsc + acc
    g_sv = _join(gsv)
    return dict(gscales=_join(outs), g_sv=S(g_sv.v.reshape(NF, V, 3, 3), g_sv.s.reshape(NF, V, 3, 3)), g_scaling=gsc)


# ------------------------------------------------------------------------------------------------ d_scale: the cases
DsCase = namedtuple("DsCase", "name mesh K G NF M seed")
DS_CASES = [
    DsCase("patch-K4-G6-T3", "patch", 4, 6, 3, 12, 1),         # F x G = 300: two workgroups
    DsCase("patch-K2-G1-T1", "patch", 2, 1, 1, 5, 2),          # the K = 2 equality vertices
    DsCase("fan43-K4-G6-T3", "fan43", 4, 6, 3, 12, 3),         # valence 43; F x G = 258
    DsCase("line257-K1-G1-T1", "line257", 1, 1, 1, 12, 4),     # V = 257
    DsCase("tiny-K1-G1-T3", "tiny", 1, 1, 3, 2, 5),
]
DS_BY_NAME = {c.name: c for c in DS_CASES}
DS_METHODS = ("lbs", "hybrid")
DOP_SET = (-1.5, -0.5, 0.9, 2.0, 3.0)


@functools.lru_cache(maxsize=None)
def ds_mesh(name):
    """(V, faces int64 [F,3]).  patch: a 6 x 6 grid (two corners of valence 1) and a last vertex in no face; fan43: a closed fan, its
    centre in 43 faces, and a vertex in no face in the middle of the numbering; line257: three faces among 257 vertices, vertex 256 in
    two of them; tiny: one face."""
    if name == "patch":
        q = np.asarray([(r * 6 + c_, r * 6 + c_ + 1, r * 6 + c_ + 6, r * 6 + c_ + 7) for r in range(5) for c_ in range(5)])
        return 37, np.concatenate([q[:, [0, 1, 2]], q[:, [1, 3, 2]]]).astype(np.int64)
    if name == "fan43":
        k = np.arange(43)
        rim = 1 + k + (k >= 20)                                 # vertex 21 is in no face
        return 45, np.stack([np.zeros(43, np.int64), rim, np.roll(rim, -1)], 1).astype(np.int64)
    if name == "line257":
        return 257, np.asarray([[0, 1, 2], [255, 256, 254], [256, 3, 4]], np.int64)
    if name == "tiny":
        return 3, np.asarray([[2, 0, 1]], np.int64)
    raise ValueError(name)


@functools.lru_cache(maxsize=None)
def _ds_inputs(name, method):
    from dreammesh4d_amd import geometry as geo

    c = DS_BY_NAME[name]
    V, faces = ds_mesh(c.mesh)
    K, G, NF, M = c.K, c.G, c.NF, c.M
    rng = np.random.default_rng([c.seed, 53])
    idx = rng.integers(0, M - 1, size=(V, K))                  # node M - 1: referenced by no vertex
    w = rng.random((V, K)) + 0.05
    w = w / w.sum(1, keepdims=True) * np.where(np.arange(V) % 3 == 0, 1.6, 1.0)[:, None]      # every third vertex leans above the clamp
    dop = (rng.choice(DOP_SET, size=(NF, M)) + 0.1 * rng.normal(size=(NF, M))).astype(np.float32)
    dop[:, :2] = 0.0                                           # o = 0.5 exactly
    if M > 3:
        dop[:, 2], dop[:, 3] = 20.0, -20.0                     # saturated; an ordinary small number
    eq = []
    if K >= 2:
        idx[:, 0] = 0                                          # one node referenced by every vertex
        idx[1, 1] = 0                                          # the same node in two slots
        eq = [2, V - 2]
        for v in eq:
            idx[v, :2], w[v] = (0, 1), 0.0
            w[v, 0], w[v, 1] = 1.0, W_EQ
        dy = np.asarray([0.5, 0.25, 0.125, 0.125] if K == 4 else [0.5, 0.5])
        idx[4:6, 1:] = rng.integers(3, M - 1, size=(2, K - 1)) if M > 4 else 1
        w[4:6] = dy                                            # weights that add up to exactly 1
    else:
        w[:2] = 1.0
    w = w.astype(np.float32)
    ds = (0.2 * rng.normal(size=(NF, M, 6))).astype(np.float32)
    ds[NF - 1] = 0.0 if NF > 1 else ds[NF - 1]                 # the last of three frames has no strain
    if method == "hybrid":                                     # every vertex but the equality vertices: 1e-3 from the clamp or further
        for _ in range(8):
            o = 1.0 / (1.0 + np.exp(-dop.astype(np.float64)))
            lw = (w.astype(np.float64)[None] * o[:, idx]).sum(-1) + float(C04)
            near = (np.abs(lw - 1) < 1e-3).any(0)
            near[eq] = False
            if not near.any():
                break
            w[near] *= np.float32(0.75)
    out = dict(method=method, idx=idx.astype(np.int64), w=w, ds=ds, dop=dop, eq_vertices=np.asarray(eq if method == "hybrid" else [], np.int64),
               faces=faces, bary=geo.bary_coords(G, None)[..., 0].numpy().astype(np.float32),
               scaling=np.exp(0.5 * rng.normal(size=(len(faces) * G, 3)) - 3.0).astype(np.float32),
               g_Sv=rng.normal(size=(NF, V, 3, 3)).astype(np.float32), g_gs=rng.normal(size=(NF, len(faces) * G, 3)).astype(np.float32))
    with np.errstate(all="ignore"):
        out["sv_in"] = vscale_reference(out, np.float64)["Sv"].v.astype(np.float32)       # what the Gaussian kernels read: rounded once
    return tuple(out.items())


def ds_inputs(name, method):
    """The inputs of a d_scale case (shared, do not modify)."""
    return dict(_ds_inputs(name, method))


@functools.lru_cache(maxsize=None)
def ds_case_reference(name, method):
    inp = ds_inputs(name, method)
    with np.errstate(all="ignore"):
        return {**vscale_reference(inp, np.float64), **gscale_reference(inp, np.float64)}


def ds_float32(name, method):
    inp = ds_inputs(name, method)
    with np.errstate(all="ignore"):
        return {**vscale_reference(inp, np.float32), **gscale_reference(inp, np.float32)}


def csr(keys, n_keys):
    """(offsets int32 [n_keys+1], items int32) of the records sorted by key, stable: the adjacency the gather backwards walk."""
    keys = np.asarray(keys).reshape(-1)
    off = np.zeros(n_keys + 1, np.int64)
    np.cumsum(np.bincount(keys, minlength=n_keys), out=off[1:])
    return off.astype(np.int32), np.argsort(keys, kind="stable").astype(np.int32)


# ------------------------------------------------------------------------------------------------ SDS glue: the restatement
def _h(a):
    """One float16 rounding of a float32 array, back in float32."""
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def _std(lv):
    """std = float16(exp(float16(0.5 float16(clamp(logvar))))) and the clamp's gradient mask."""
    inside = (lv >= -30) & (lv <= 20)
    half_lv = _h(np.float32(0.5) * _h(np.clip(lv, np.float32(-30), np.float32(20))))
    return _h(np.exp(half_lv.astype(np.float64)).astype(np.float32)), inside


def sds_restate(inp):
    """The two glue kernels' expressions with the torch float16 graph's roundings, one per torch operator."""
    f32 = np.float32
    B = inp["moments"].shape[0]
    sf, gs = f32(inp["scale_factor"]), f32(inp["guidance_scale"])
    m, post, noise = inp["moments"].astype(f32), inp["post"].astype(f32), inp["noise"]
    with np.errstate(all="ignore"):
        sd, inside = _std(m[:, 4:])
        lat = _h(sf * _h(m[:, :4] + _h(sd * post)))
        ac = inp["alphas"][inp["t"]].reshape(B, 1, 1, 1)
        noisy = np.sqrt(ac) * lat + np.sqrt(f32(1) - ac) * noise
        x_in = np.zeros((2 * B, 8) + m.shape[2:], np.float16)
        x_in[:B, :4] = x_in[B:, :4] = noisy.astype(np.float16)
        x_in[B:, 4:] = inp["c_concat"][inp["fidx"]]
        pred = inp["pred"].astype(f32)
        unc, cnd = pred[:B], pred[B:]
        g = (f32(1) - ac) * ((unc + gs * (cnd - unc)) - noise)
        g = np.where(np.isnan(g), f32(0), np.where(g == np.inf, FLT_MAX, np.where(g == -np.inf, -FLT_MAX, g))).astype(f32)
        assert not np.isnan(g).any()
        if inp["clip"] is not None:
            g = np.minimum(np.maximum(g, -f32(inp["clip"])), f32(inp["clip"]))
        diff = lat - (lat - g)
        cmul = (f32(1) / f32(B)) * f32(0.5)
        d_sum = _h(_h((f32(2) * diff) * cmul) * sf)
        d_lv = _h(_h(_h(d_sum * post) * sd) * f32(0.5))
        d_mom = np.concatenate([d_sum, np.where(inside, d_lv, f32(0))], 1).astype(np.float16)
    return dict(latents=lat, x_in=x_in, t2=np.concatenate([inp["t"], inp["t"]]), d_moments=d_mom, inside=inside, g=g, diff=diff)


def sds_sums(rs, B, f=np.float64):
    """(loss, |grad|) from the restatement's per-element terms, added up one by one in dtype f."""
    with np.errstate(all="ignore"):
        d, g = rs["diff"].reshape(-1).astype(f), rs["g"].reshape(-1).astype(f)
        return (f(0.5) * np.cumsum(d * d, dtype=f)[-1]) / f(B), np.sqrt(np.cumsum(g * g, dtype=f)[-1])


def half_mismatch(got, want):
    """(share of elements that differ, worst difference in float16 ulps) of two float16 arrays; NaN equals NaN, an infinity only itself."""
    a, b = np.asarray(got, np.float16).astype(np.float64), np.asarray(want, np.float16).astype(np.float64)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    if same.all():
        return 0.0, 0.0
    with np.errstate(all="ignore"):
        big = np.maximum(np.maximum(np.abs(a), np.abs(b)), 2.0 ** -14)                     # (subnormals: the spacing of 2^-14)
        ulps = np.where(same, 0.0, np.abs(a - b) / np.exp2(np.floor(np.log2(big)) - 10))
    return float((~same).mean()), float(np.nan_to_num(ulps, nan=np.inf).max())


# ------------------------------------------------------------------------------------------------ SDS glue: the cases
SdsCase = namedtuple("SdsCase", "name B H W clip special t fidx L seed")
T_STEPS = 1000
SDS_CASES = [
    SdsCase("sds-1x1x1", 1, 1, 1, None, "nan", (0,), (1,), 2, 1),                          # t2 is written for i < 2 B although n = 1
    SdsCase("sds-3x4x6-clip", 3, 4, 6, 0.25, "nonfinite", (0, T_STEPS - 1, 500), (2, 0, 2), 3, 2),
    SdsCase("sds-2x6x4", 2, 6, 4, None, None, (T_STEPS - 1, 17), (0, 0), 1, 3),
    SdsCase("sds-2x6x4-nonfinite", 2, 6, 4, None, "nonfinite", (300, 0), (1, 0), 2, 4),     # no clip: +-FLT_MAX reaches the sums
    SdsCase("sds-3x32x32", 3, 32, 32, "element", "nonfinite", (20, 979, T_STEPS - 1), (4, 4, 1), 5, 5),
]
SDS_BY_NAME = {c.name: c for c in SDS_CASES}
H16 = lambda v: np.float16(v)
LV_PLANTED = (H16(-30), H16(20), np.nextafter(H16(-30), H16(-40)), np.nextafter(H16(20), H16(30)), H16(-60), H16(24),
              np.nextafter(H16(-30), H16(0)), np.nextafter(H16(20), H16(0)))
LAYOUTS = ("contiguous", "channels_last", "slice")
SDS_TENSORS = ("moments", "post", "noise", "latents", "c_concat", "x_in", "pred", "d_moments")


def logvar_is_safe(lv16):
    """Whether float16(exp(lv / 2)) is the same for every expf within 8 float32 ulps of the exact one."""
    lv = np.asarray(lv16, np.float16).astype(np.float32)
    half_lv = _h(np.float32(0.5) * _h(np.clip(lv, np.float32(-30), np.float32(20)))).astype(np.float64)
    x = np.exp(half_lv)
    q = np.exp2(np.maximum(np.floor(np.log2(x)), -14.0) - 10)                             # float16 spacing at x
    away = np.abs((x / q) % 1.0 - 0.5) * q                                                # distance to the nearest rounding midpoint
    return away >= 8 * np.exp2(np.floor(np.log2(x)) - 23)


def _safe_logvar(lv16):
    lv16 = np.asarray(lv16, np.float16).copy()
    for _ in range(64):
        bad = ~logvar_is_safe(lv16)
        if not bad.any():
            return lv16
        lv16[bad] = np.nextafter(lv16[bad], np.float16(0))
    raise AssertionError("no safe log-variance found")


def sds_layout(case_index, tensor):
    """Which layout a tensor takes in a case: every tensor gets every layout over the cases, not all the same in one case."""
    return LAYOUTS[(case_index + SDS_TENSORS.index(tensor) + SDS_TENSORS.index(tensor) // 3) % 3]


@functools.lru_cache(maxsize=None)
def _sds_inputs(name):
    c = SDS_BY_NAME[name]
    B, H, W = c.B, c.H, c.W
    rng = np.random.default_rng([c.seed, 59])
    moments = rng.normal(size=(B, 8, H, W))
    moments[:, 4:] = rng.uniform(-36, 12, size=(B, 4, H, W))
    lv = moments[:, 4:].astype(np.float16)
    flat = lv.reshape(-1)
    n_plant = min(len(LV_PLANTED), flat.size)
    flat[:: max(1, flat.size // n_plant)][:n_plant] = LV_PLANTED[:n_plant]
    lv = _safe_logvar(lv)
    assert all((lv == v).any() for v in LV_PLANTED[:n_plant])
    moments = moments.astype(np.float16)
    moments[:, 4:] = lv
    post = rng.normal(size=(B, 4, H, W))
    post[lv.astype(np.float32) > 8] *= 2.0 ** -7              # std up to exp(10): nothing overflows float16
    noise = rng.normal(size=(B, 4, H, W)).astype(np.float32)
    pred = rng.normal(size=(2 * B, 4, H, W)).astype(np.float16)
    pf = pred.reshape(-1)
    if c.special == "nan":
        pf[1] = np.nan
    elif c.special == "nonfinite":
        for j, v in enumerate((np.nan, np.inf, -np.inf, np.inf, -np.inf, np.nan)):      # in the unconditional and the conditional half
            pf[(7 + j * (pf.size // 6 + 1)) % pf.size] = v
    betas = np.linspace(0.00085 ** 0.5, 0.0120 ** 0.5, T_STEPS, dtype=np.float64) ** 2
    inp = dict(moments=moments, post=post.astype(np.float16), noise=noise, pred=pred, t=np.asarray(c.t, np.int64),
               alphas=np.cumprod(1.0 - betas).astype(np.float32), c_concat=rng.normal(size=(c.L, 4, H, W)).astype(np.float16),
               fidx=np.asarray(c.fidx, np.int64), scale_factor=0.18215, guidance_scale=3.0, clip=c.clip)
    if c.clip == "element":                                    # the clip IS one element's |g|: |g| == clip exactly there
        g = np.abs(sds_restate(dict(inp, clip=None))["g"]).reshape(-1)
        inp["clip"] = float(np.sort(g[g < 1e30])[int(0.7 * g.size)])
    return tuple(inp.items())


def sds_inputs(name):
    """The inputs of an SDS case (shared, do not modify): float16 moments, post, pred, c_concat; float32 noise, alphas; int64 t, fidx."""
    return dict(_sds_inputs(name))


@functools.lru_cache(maxsize=None)
def sds_case_restatement(name):
    return sds_restate(sds_inputs(name))


# ------------------------------------------------------------------------------------------------ judging
def float32_ratios():
    """kind -> (worst ratio of the float32 restatement against the float64 reference in units of 2^-24 scale, the case that set it)."""
    worst = {}

    def note(kind, r, where):
        if r > worst.get(kind, (-1.0, None))[0]:
            worst[kind] = (r, where)

    for c in HEAD_CASES:
        for var in head_variants(c.name):
            r64 = head_case_reference(c.name, *var)
            with np.errstate(all="ignore"):
                r32 = head_reference(head_inputs(c.name, *var), np.float32)
            for k in HEAD_KINDS:
                note(k, float(ratio(r32[k].v, r64[k]).max(initial=0.0)), c.name)
    for n, k, m in PSUM_CASES:
        note("psum", float(ratio(psum_reference(n, k, m, np.float32).v, psum_reference(n, k, m)).max(initial=0.0)), f"n{n}-k{k}-m{m}")
    for c in DS_CASES:
        for method in DS_METHODS:
            r64, r32 = ds_case_reference(c.name, method), ds_float32(c.name, method)
            for k in VS_KINDS + GS_KINDS:
                note(k, float(ratio(r32[k].v, r64[k]).max(initial=0.0)), f"{c.name}-{method}")
    for c in SDS_CASES:
        rs = sds_case_restatement(c.name)
        (l64, n64), (l32, n32) = sds_sums(rs, c.B), sds_sums(rs, c.B, np.float32)
        if np.isfinite(l32):                                  # (+-FLT_MAX squared overflows float32: the kernels must return inf there)
            note("sds_loss", abs(float(l32) - l64) / (U * l64), c.name)
            note("sds_norm", abs(float(n32) - n64) / (U * n64), c.name)
    return worst


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
