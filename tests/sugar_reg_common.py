"""Yardsticks of the SuGaR density and normal regularisation tests ("SuGaR density and normal regularisation").

``restate``          the semantics in float64 numpy, forward and CLOSED-FORM gradients (no autograd): what the device is judged by
``torch_expressions`` the reference's expressions written in torch (any dtype, autograd): in float32 on the CPU its distance to
                     ``restate`` is the ``unit`` of a case that is not in the golden fixture
``golden``           tests/golden/sugar_reg.npz: what the reference's own methods computed (make_golden_sugar_reg.py)
and the builders of the edge cases.
"""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sugar_reg.npz")
INPUTS = ("xyz", "scales", "quats", "opac", "knn_idx", "sample_idx", "eps")
PER_SAMPLE = ("density", "beta", "density_term", "normal_term")
GRADS = ("d_xyz", "d_scales", "d_quats", "d_opac")
UPSTREAMS = {"d": (1.0, 0.0), "n": (0.0, 1.0), "dn": (1.0, 1.0)}
# the two lower bounds as float32 holds them (torch casts the scalar of ``clamp(min=...)`` to the tensor's dtype): a float32 scale
# that equals float32(1e-8) is AT the bound, although it is below the double 1e-8
F32_BOUNDS = (float(np.float32(1e-8)), float(np.float32(1e-6)))


def golden():
    return np.load(GOLDEN)


def golden_inputs(z):
    return {k: z[f"in/{k}"] for k in INPUTS}


# ------------------------------------------------------------------------------------------------ float64 numpy, closed form
def _rotation(q):
    r, i, j, k = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    two_s = 2.0 / (q * q).sum(-1)
    R = np.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                  two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                  two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1)
    return R.reshape(-1, 3, 3)


def _rotation_backward(q, dR):
    """dq of R = I + two_s B(q), two_s = 2 / (q.q)."""
    r, i, j, k = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    d = dR.reshape(-1, 9).T
    qq = (q * q).sum(-1)
    T = 2.0 / qq
    dT = (d[0] * -(j * j + k * k) + d[1] * (i * j - k * r) + d[2] * (i * k + j * r) + d[3] * (i * j + k * r) + d[4] * -(i * i + k * k)
          + d[5] * (j * k - i * r) + d[6] * (i * k - j * r) + d[7] * (j * k + i * r) + d[8] * -(i * i + j * j))
    dq = np.stack((T * (-k * d[1] + j * d[2] + k * d[3] - i * d[5] - j * d[6] + i * d[7]),
                   T * (-2 * i * d[4] - 2 * i * d[8] + j * d[1] + k * d[2] + j * d[3] - r * d[5] + k * d[6] + r * d[7]),
                   T * (-2 * j * d[0] - 2 * j * d[8] + i * d[1] + r * d[2] + i * d[3] + k * d[5] - r * d[6] + k * d[7]),
                   T * (-2 * k * d[0] - 2 * k * d[4] - r * d[1] + i * d[2] + r * d[3] + j * d[5] + i * d[6] + j * d[7])), -1)
    return dq + 2.0 * q * (-2.0 / (qq * qq) * dT)[:, None]


def restate(inp, with_normal, upstream=(1.0, 1.0), sampling_scale=1.5, density_factor=1.0, bounds=(1e-8, 1e-6)):
    """dict of the four per-sample arrays, the two losses and the four gradients of ``upstream[0] * density_regulation +
    upstream[1] * normal_regulation``, all float64.  ``normal_term`` and its loss are zeros without ``with_normal``.
    ``bounds``: the two lower clamps; the doubles of the reference's float64 run by default, ``F32_BOUNDS`` for a case whose float32
    inputs sit exactly at a bound."""
    B8, B6 = bounds
    xyz, s, q, op = (np.asarray(inp[k], np.float64) for k in INPUTS[:4])
    op = op.reshape(-1)
    knn, g = np.asarray(inp["knn_idx"], np.int64), np.asarray(inp["sample_idx"], np.int64)
    eps = np.asarray(inp["eps"], np.float64)
    N, K, S = knn.shape[0], knn.shape[1], g.shape[0]
    ar = np.arange(N)
    R = _rotation(q)
    a = 1.0 / np.maximum(s, B8)
    M = R * a[:, None, :]
    cs = np.argmin(s, axis=1)                              # the first (lowest) axis on ties
    m, n = s[ar, cs], R[ar, :, cs]
    # the sample point: q (0,v) conj(q) = (w^2 - |u|^2) v + 2 (u.v) u + 2 w (u x v)
    v = sampling_scale * s[g] * eps
    w_, u_ = q[g, 0:1], q[g, 1:]
    ww_uu = w_ * w_ - (u_ * u_).sum(-1, keepdims=True)
    p = ww_uu * v + 2 * (u_ * v).sum(-1, keepdims=True) * u_ + 2 * w_ * np.cross(u_, v)
    x = xyz[g] + p
    J = knn[g]
    sh = x[:, None] - xyz[J]
    u = np.einsum("skrc,skr->skc", M[J], sh)
    uu = (u * u).sum(-1)
    e = np.exp(-0.5 * np.clip(uu, 0.0, 1e8))
    w = density_factor * op[J] * e
    density = w.sum(1)
    beta = m[J].sum(1) / K
    d, ng = x - xyz[g], n[g]
    sdf = (d * ng).sum(1)
    target = np.exp(-0.5 * sdf ** 2 / beta ** 2)
    out = {"density": density, "beta": beta, "density_term": np.abs(density - target), "normal_term": np.zeros(S), "_uu": uu}
    gd, gn = upstream[0] / S, (upstream[1] / S if with_normal else 0.0)
    r = np.zeros((S, 3))
    if with_normal:
        sg = np.sign((n[J] * ng[:, None]).sum(-1))
        c = n[J] * sg[..., None]
        vk = w * np.abs((sh * c).sum(-1)) / np.maximum(m[J], B6) ** 2
        vn = vk / np.maximum(vk.sum(1), B6)[:, None]
        out["_V"] = vk.sum(1)
        r = ng - (vn[..., None] * c).sum(1)
        out["normal_term"] = (r * r).sum(1)
    out["loss_d"], out["loss_n"] = out["density_term"].mean(), out["normal_term"].mean()
    # ---- backward
    sD = gd * np.sign(density - target)
    dsdf = -sD * target * (-sdf / beta ** 2)
    dbeta = -sD * target * (sdf ** 2 / beta ** 3)
    dm2 = np.where((uu >= 0) & (uu <= 1e8), sD[:, None] * w * -0.5, 0.0)
    du = 2 * u * dm2[..., None]
    dsh = np.einsum("skrc,skc->skr", M[J], du)
    d_xyz, d_s, d_q, d_op = np.zeros((N, 3)), np.zeros((N, 3)), np.zeros((N, 4)), np.zeros(N)
    dM, dm, dn = np.zeros((N, 3, 3)), np.zeros(N), np.zeros((N, 3))
    np.add.at(dM, J, sh[..., :, None] * du[..., None, :])
    np.add.at(d_xyz, J, -dsh)
    np.add.at(d_op, J, sD[:, None] * density_factor * e)
    np.add.at(dm, J, np.broadcast_to((dbeta / K)[:, None], J.shape))
    dr = 2 * r * gn
    np.add.at(dn, g, dsdf[:, None] * d + dr)
    if with_normal:
        np.add.at(dn, J, -(vn * sg)[..., None] * dr[:, None, :])
    dx = dsh.sum(1)
    np.add.at(d_xyz, g, dx)
    dp = dx + dsdf[:, None] * ng
    udp, vdp, uv = ((a_ * b_).sum(-1, keepdims=True) for a_, b_ in ((u_, dp), (v, dp), (u_, v)))
    dv = ww_uu * dp + 2 * udp * u_ - 2 * w_ * np.cross(u_, dp)
    np.add.at(d_s, g, dv * sampling_scale * eps)
    dqg = np.concatenate((2 * w_ * vdp + 2 * (np.cross(u_, v) * dp).sum(-1, keepdims=True),
                          -2 * vdp * u_ + 2 * uv * dp + 2 * udp * v + 2 * w_ * np.cross(v, dp)), -1)
    np.add.at(d_q, g, dqg)
    # ---- the chain through M, m, n and R
    dR = dM * a[:, None, :]
    da = (dM * R).sum(1)
    d_s += np.where(s >= B8, -da * a * a, 0.0)
    d_s[ar, cs] += dm
    dR[ar, :, cs] += dn
    d_q += _rotation_backward(q, dR)
    out.update(d_xyz=d_xyz, d_scales=d_s, d_quats=d_q, d_opac=d_op)
    return out


# ------------------------------------------------------------------------------------------------ the expressions in torch
def quaternion_to_matrix(q):
    """pytorch3d.transforms.quaternion_to_matrix, from its documented formula."""
    r, i, j, k = torch.unbind(q, -1)
    two_s = 2.0 / (q * q).sum(-1)
    o = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1)
    return o.reshape(q.shape[:-1] + (3, 3))


def quaternion_raw_multiply(a, b):
    aw, ax, ay, az = torch.unbind(a, -1)
    bw, bx, by, bz = torch.unbind(b, -1)
    return torch.stack((aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw), -1)


def quaternion_apply(q, point):
    """pytorch3d.transforms.quaternion_apply: q (0, point) conj(q)."""
    real = point.new_zeros(point.shape[:-1] + (1,))
    out = quaternion_raw_multiply(quaternion_raw_multiply(q, torch.cat((real, point), -1)), q * q.new_tensor([1, -1, -1, -1]))
    return out[..., 1:]


def lowest_argmin(s):
    idx = torch.zeros(s.shape[0], dtype=torch.int64)
    idx = torch.where(s[:, 1] < s[:, 0], torch.ones_like(idx), idx)
    return torch.where(s[:, 2] < torch.minimum(s[:, 0], s[:, 1]), torch.full_like(idx, 2), idx)


def torch_expressions(inp, with_normal, upstream=(1.0, 1.0), dtype=torch.float32, sampling_scale=1.5, density_factor=1.0):
    """The expressions of sugar_utils.py:226-228, 256-262, 305-311, 355-372, 420-423, 708-757 in torch on the CPU, gradients by
    autograd; same keys as ``restate`` (numpy float64 copies of whatever dtype computed them)."""
    xyz, s, q, op = (torch.tensor(np.asarray(inp[k]), dtype=dtype, requires_grad=True) for k in INPUTS[:4])
    knn, g = torch.tensor(np.asarray(inp["knn_idx"]), dtype=torch.int64), torch.tensor(np.asarray(inp["sample_idx"]), dtype=torch.int64)
    eps = torch.tensor(np.asarray(inp["eps"]), dtype=dtype)
    x = xyz[g] + quaternion_apply(q[g], sampling_scale * s[g] * eps)
    M = quaternion_to_matrix(q) * (1.0 / s.clamp(min=1e-8))[:, None]
    J = knn[g]
    shift = x[:, None] - xyz[J]
    warped = M[J].transpose(-1, -2) @ shift[..., None]
    m2 = (warped[..., 0] * warped[..., 0]).sum(dim=-1).clamp(min=0.0, max=1e8)
    w = density_factor * op.reshape(-1, 1)[J][..., 0] * torch.exp(-1.0 / 2 * m2)
    density = w.sum(dim=-1)
    cs = lowest_argmin(s)
    m = s.gather(1, cs[:, None])[:, 0]
    n = quaternion_to_matrix(q).gather(2, cs[:, None, None].expand(-1, 3, -1)).squeeze(2)
    beta = m[J].mean(dim=1)
    ng = n[g]
    sdf = ((x - xyz[g]) * ng).sum(dim=-1)
    target = torch.exp(-0.5 * sdf.pow(2) / beta.pow(2))
    dterm = (density - target).abs()
    loss_d = dterm.mean()
    nterm, loss_n = torch.zeros_like(dterm), dterm.sum() * 0
    if with_normal:
        cn = n[J]
        cn = cn * torch.sign((cn * ng[:, None]).sum(dim=-1, keepdim=True)).detach()
        nw = ((x[:, None] - xyz[J]) * cn).sum(dim=-1).abs().detach()
        nw = w.detach() * nw / m[J].detach().clamp(min=1e-6) ** 2
        nw = nw / nw.sum(dim=-1).detach().unsqueeze(-1).clamp(min=1e-6)
        nterm = (ng - (nw[..., None] * cn).sum(dim=-2)).pow(2).sum(dim=-1)
        loss_n = nterm.mean()
    (upstream[0] * loss_d + upstream[1] * loss_n).backward()
    f = lambda t: t.detach().double().numpy()
    out = {"density": f(density), "beta": f(beta), "density_term": f(dterm), "normal_term": f(nterm), "loss_d": f(loss_d), "loss_n": f(loss_n)}
    for name, t in zip(GRADS, (xyz, s, q, op)):
        out[name] = f(t.grad if t.grad is not None else torch.zeros_like(t)).reshape(t.shape)
    return out


def unit_of(ref32, f64, name):
    """The unit of a tensor's bound: the float32 error of the reference's expressions, at least half an ulp of its largest value."""
    big = float(np.abs(f64[name]).max()) if np.size(f64[name]) else 0.0
    half_ulp = 0.5 * float(np.spacing(np.float32(big)))
    return max(float(np.abs(ref32[name] - f64[name]).max()), half_ulp)


# ------------------------------------------------------------------------------------------------ builders
def exact_knn(xyz, K):
    """[N,K] int64: the K nearest points of every point (itself included) by an exhaustive float64 search, ties to the lower index."""
    x = np.asarray(xyz, np.float64)
    d2 = ((x[:, None] - x[None]) ** 2).sum(-1)
    return np.argsort(d2, axis=1, kind="stable")[:, :K].astype(np.int64)


def random_case(N, K, S, seed, spread=0.8, knn="exact"):
    """Seeded inputs: points in a ball, anisotropic scales over two decades around the point spacing, quaternions normalised in
    float32 (so not exactly unit), opacities in (0.05, 0.99)."""
    rng = np.random.default_rng(seed)
    xyz = rng.standard_normal((N, 3))
    xyz = (xyz / np.linalg.norm(xyz, axis=1, keepdims=True) * spread * np.cbrt(rng.random((N, 1)))).astype(np.float32)
    spacing = spread * (4.0 / max(N, 2)) ** (1.0 / 3.0)
    scales = (spacing * 10.0 ** rng.uniform(-1.7, 0.3, (N, 3))).astype(np.float32)
    q = rng.standard_normal((N, 4)).astype(np.float32)
    q = (q / np.sqrt((q * q).sum(1, keepdims=True, dtype=np.float32))).astype(np.float32)
    opac = rng.uniform(0.05, 0.99, N).astype(np.float32)
    table = exact_knn(xyz, K) if knn == "exact" else rng.integers(0, N, (N, K))
    return {"xyz": xyz, "scales": scales, "quats": q, "opac": opac, "knn_idx": table.astype(np.int32),
            "sample_idx": rng.integers(0, N, S).astype(np.int32), "eps": rng.standard_normal((S, 3)).astype(np.float32)}
