"""Shared by tests/test_arap_fit_cpu.py and tests/test_arap_fit_gpu.py: a torch restatement of the reference's fitted-rotation
branch (custom/threestudio-dreammesh4d/utils/arap_utils.py:195-214) over a CSR edge list, in the dtype of its inputs.  It is
test infrastructure: tests/test_arap_fit_cpu.py pins it to tests/golden/arap_fit.npz (the reference's own class in float64) to
1e-10, and the GPU tests then use it in float64 as the yardstick and in float32 as the measure of what float32 LAPACK achieves.
It keeps the reference's operations -- covariance, torch.svd, R = W U^T, flip of the smallest singular value's column where
det <= 0, the "unchanged" rule -- and does NOT share the kernel's method (no quaternion, no eigenvector)."""
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "arap_fit.npz")
EPS32 = float(np.finfo(np.float32).eps)
R_BAR_FACTOR = 4.0          # HIP's max_i |dR_i| gap_i may be this many times the float32 torch.svd fit's (the issue's bar)
SIGN_RATIO = 1e-3           # the determinant-flip flag is compared where sig3 / sig1 exceeds this


def load():
    z = np.load(GOLD)
    return {k: z[k] for k in z.files}


def adjacency(verts, faces, dtype=torch.float64):
    """src [E], nbr [E], w [E], e [E,3] with the reference's dense-branch cotangent weights (arap_utils.py:100-151) evaluated
    in `dtype` (oracle/mesh_reg.py::build is the same in float32, the product's precision)."""
    verts = torch.as_tensor(np.asarray(verts), dtype=dtype)
    faces_t = torch.as_tensor(np.asarray(faces), dtype=torch.long)
    V = verts.shape[0]
    nb = [set() for _ in range(V)]
    for f in np.asarray(faces):
        for j in range(3):
            nb[int(f[j])].update((int(f[(j + 1) % 3]), int(f[(j + 2) % 3])))
    src = torch.as_tensor(np.concatenate([np.full(len(n), i, np.int64) for i, n in enumerate(nb)]))
    nbr = torch.as_tensor(np.concatenate([np.asarray(sorted(n), np.int64) for n in nb]))
    v0, v1, v2 = verts[faces_t].unbind(1)
    A, B, C = (v1 - v2).norm(dim=1), (v0 - v2).norm(dim=1), (v0 - v1).norm(dim=1)
    s = 0.5 * (A + B + C)
    area = (s * (s - A) * (s - B) * (s - C)).clamp_(min=1e-12).sqrt()
    A2, B2, C2 = A * A, B * B, C * C
    cot = torch.stack([(B2 + C2 - A2) / area, (A2 + C2 - B2) / area, (A2 + B2 - C2) / area], dim=1) / 4.0
    W = torch.zeros(V, V, dtype=dtype)
    W[faces_t[:, [0, 1, 2]].flatten(), faces_t[:, [1, 2, 0]].flatten()] = 0.5 * cot.flatten()
    W = W + W.T
    return src, nbr, W[src, nbr], verts[src] - verts[nbr]


def fit(src, nbr, w, e, xp):
    """xp [V,3] -> R [V,3,3], sig [V,3], flip [V] bool, unchanged [V] bool; differentiable in xp like the reference."""
    V = xp.shape[0]
    ep = xp[src] - xp[nbr]
    S = torch.zeros(V, 3, 3, dtype=xp.dtype).index_add(0, src, w[:, None, None] * e[:, :, None] * ep[:, None, :])
    # (P == P_prime).all(dim=1) over the neighbours, then torch.where(...)[0]: unchanged on AT LEAST ONE axis
    differs = torch.zeros(V, 3, dtype=torch.long).index_add(0, src, (ep.detach() != e).long())
    unchanged = (differs == 0).any(dim=1)
    S = torch.where(unchanged[:, None, None], torch.zeros_like(S), S)
    U, sig, W = torch.svd(S)
    R = W @ U.transpose(1, 2)
    flip = torch.det(R.detach()) <= 0
    sgn = torch.ones(V, 3, dtype=xp.dtype)
    sgn[flip, torch.argmin(sig.detach(), dim=1)[flip]] = -1
    R = W @ (U * sgn[:, None, :]).transpose(1, 2)
    return R, sig.detach(), flip, unchanged


def energy(src, nbr, w, e, xp, R):
    ep = xp[src] - xp[nbr]
    return (w * (ep - torch.einsum("vab,vb->va", R[src], e)).square().sum(-1)).sum()


def gap(sig, flip):
    """(sig2 + d sig3) / sig1, d = -1 where the flip is taken: the conditioning of R (0 where S = 0)."""
    d = torch.where(flip, -1.0, 1.0).to(sig.dtype)
    return torch.where(sig[:, 0] > 0, (sig[:, 1] + d * sig[:, 2]) / sig[:, 0].clamp_min(1e-300), torch.zeros_like(sig[:, 0]))


def r_error(R, R64, gap64):
    """max_i max|R_i - R64_i| gap_i and the plain max|dR|."""
    d = (R.double() - R64).abs().amax((1, 2))
    return float((d * gap64).max()), float(d.max())


def orthogonality(R):
    """max |R^T R - I| and min det over a [..., 3, 3] float32 tensor, evaluated in float64."""
    R = R.double().reshape(-1, 3, 3)
    return float((R.transpose(1, 2) @ R - torch.eye(3, dtype=torch.float64)).abs().max()), float(torch.det(R).min())
