"""Shared by tests/test_sh_eval_cpu.py and tests/test_sh_eval_gpu.py: the fixture of tests/golden/make_golden_sh.py, a float64
numpy restatement of the real SH basis of degree 0..3 written from the formulae (the constants the kernel must use), and the
comparison helpers -- kept here so that the CPU suite can test the helpers the GPU suite relies on."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_sh.npz")
U = 2.0 ** -24          # unit roundoff of float32

# Rounding count of csrc/sh.h + csrc/sh_eval.hip (one rounding per written float32 operation, no contraction), in units of U,
# relative to 0.5 + sum_k |B_k| |sh_k|:
#   direction      d = p - c (1); |d|^2 = (dx dx + dy dy) + dz dz: 2 from d, 1 per square, 2 additions -> 5; sqrt halves it and
#                  rounds (3.5); x = dx / |d|: 1 + 3.5 + 1 = 5.5 per component
#   basis          a polynomial of degree <= 3 in (x, y, z) inherits 3 x 5.5 = 16.5; its own evaluation is at most 7 roundings on a
#                  path (B12 = (k z) ((2 zz - 3 xx) - 3 yy): square, scale, subtract, square-scale, subtract, rounded constant
#                  times z, final product) -> 23.5
#   accumulation   B_k sh_k (1), and a term passes through at most 15 additions of the running sum plus the + 0.5 (16)
#   K = 23.5 + 1 + 16 = 40.5 -> 41
# This is a worst-case (every rounding aligned) count per monomial.  Strictly it is relative to the sum of the ABSOLUTE monomials
# of each B_k (xx + yy where B_8 has xx - yy), which is >= |B_k|; the bar uses |B_k| (the fixture's A).
K_FORWARD = 41.0

GRAD_RTOL = 1e-4        # the project's gradient bar (tests/test_raster_gpu.py:17-18): per element
GRAD_ATOL = 5e-6        # x max|reference gradient| of the tensor


def load():
    return dict(np.load(GOLDEN))


def sh_basis(dirs, degree):
    """B_k(dir), k < (degree + 1)^2, float64 [N, K]: the real spherical harmonics in the sign convention of the published 3D
    Gaussian Splatting colour model."""
    d = np.asarray(dirs, np.float64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    pi = np.pi
    B = [np.full_like(x, 0.5 * np.sqrt(1.0 / pi))]
    if degree >= 1:
        k1 = np.sqrt(3.0 / (4.0 * pi))
        B += [-k1 * y, k1 * z, -k1 * x]
    if degree >= 2:
        k2a, k2b, k2c = 0.5 * np.sqrt(15.0 / pi), 0.25 * np.sqrt(5.0 / pi), 0.25 * np.sqrt(15.0 / pi)
        B += [k2a * x * y, -k2a * y * z, k2b * (2 * z * z - x * x - y * y), -k2a * x * z, k2c * (x * x - y * y)]
    if degree >= 3:
        k3a, k3b, k3c = 0.25 * np.sqrt(35.0 / (2.0 * pi)), 0.5 * np.sqrt(105.0 / pi), 0.25 * np.sqrt(21.0 / (2.0 * pi))
        k3d, k3e = 0.25 * np.sqrt(7.0 / pi), 0.25 * np.sqrt(105.0 / pi)
        q = 4 * z * z - x * x - y * y
        B += [-k3a * y * (3 * x * x - y * y), k3b * x * y * z, -k3c * y * q, k3d * z * (2 * z * z - 3 * x * x - 3 * y * y),
              -k3c * x * q, k3e * z * (x * x - y * y), -k3a * x * (x * x - 3 * y * y)]
    return np.stack(B, axis=1)


def directions(points, campos):
    d = np.asarray(points, np.float64) - np.asarray(campos, np.float64)[None]
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def eval_v(points, sh, campos, degree):
    """sum_k B_k sh_k + 0.5 in float64, [N,3]."""
    K = (degree + 1) ** 2
    B = sh_basis(directions(points, campos), degree)
    return (B[:, :, None] * np.asarray(sh, np.float64)[:, :K]).sum(axis=1) + 0.5


def forward_excess(rgb, clamped, v_ref, A, k=K_FORWARD):
    """Compares a float32 forward with the float64 reference.  Returns (worst |rgb - max(v_ref, 0)| / bar, number of clamp flags
    that differ among the elements farther from the clamp than the bar, fraction of elements within the bar of the clamp)."""
    bar = k * U * np.asarray(A, np.float64)
    ref = np.maximum(v_ref, 0.0)
    ratio = float((np.abs(np.asarray(rgb, np.float64) - ref) / bar).max())
    far = np.abs(v_ref) > bar
    wrong = int(((np.asarray(clamped) != 0) != (v_ref < 0))[far].sum())
    return ratio, wrong, float(1.0 - far.mean())


def assert_forward(rgb, clamped, v_ref, A, what=""):
    ratio, wrong, near = forward_excess(rgb, clamped, v_ref, A)
    print(f"{what}: max |hip - ref| / bar = {ratio:.4f}, flags wrong {wrong}, near-clamp fraction {near:.2e}")
    assert ratio <= 1.0, f"{what}: |hip - ref| reaches {ratio:.3f} x the bar of {K_FORWARD} * 2^-24 * A"
    assert wrong == 0, f"{what}: {wrong} clamp flags differ away from the clamp"
    assert near <= 0.01, f"{what}: {near:.3%} of the elements lie within the bar of the clamp"


def grad_excess(got, ref, keep=None):
    """max over the kept elements of |got - ref| / (GRAD_RTOL |ref| + GRAD_ATOL max|ref|); an element whose bar is 0 must match exactly."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bar = GRAD_RTOL * np.abs(ref) + GRAD_ATOL * np.abs(ref).max()
    err = np.abs(got - ref)
    if keep is not None:
        err, bar = err[keep], bar[keep]
    if err.size == 0:
        return 0.0
    r = np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max())
