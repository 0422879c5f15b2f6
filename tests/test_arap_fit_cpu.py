"""CPU-side checks of the fitted-rotation ARAP path (ARAPCoach.compute_arap_energy(xyz_prime) with the reference's default
vert_rotations=None): the C ABI of the new entry point and its host-side argument checks, the float64 restatement the GPU tests
measure against pinned to the reference's own class (tests/golden/arap_fit.npz), and the fact the backward rests on."""
import ctypes as C
import os
import re

import numpy as np
import torch

from tests import arap_fit_common as afc

CASES = ("mid", "noisy", "rigid", "smooth", "yz")


def test_fit_entry_point_is_exported_and_checks_its_arguments_on_the_host():
    """dm4d_arap_fit_rotations is in the cross-compiled library, in include/dm4d.h and in the ctypes table; the ABI number is
    unchanged (the addition is a new symbol); negative sizes, null tensors, a null output and more timestamps than a grid's y
    extent are refused before anything is launched, with arap_check's messages; empty problems are no-ops."""
    from dreammesh4d_amd import _lib

    L = _lib.lib()
    name = "dm4d_arap_fit_rotations"
    assert hasattr(L, name) and name in _lib.declared_symbols() and name in _lib._SIGNATURES
    assert L.dm4d_version() == _lib.abi_version() == 107
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dm4d.h")
    assert re.search(r"107 gained dm4d_arap_fit_rotations", open(header).read())
    dummy = (C.c_float * 64)()
    p = C.cast(dummy, C.c_void_p)
    fit = L.dm4d_arap_fit_rotations
    assert fit(-1, 4, p, p, p, p, p, p, p, None) == -1 and b"negative T/V" in L.dm4d_last_error()
    assert fit(2, -4, p, p, p, p, p, p, p, None) == -1 and b"negative T/V" in L.dm4d_last_error()
    assert fit(65536, 4, p, p, p, p, p, p, p, None) == -1 and b"65535 timestamps" in L.dm4d_last_error()
    for k in range(5):                                           # each of the five inputs in turn
        args = [p] * 5
        args[k] = None
        assert fit(2, 4, *args, p, p, None) == -1 and b"null tensor" in L.dm4d_last_error(), k
    assert fit(2, 4, p, p, p, p, p, None, p, None) == -1 and b"null output" in L.dm4d_last_error()
    assert fit(0, 4, None, None, None, None, None, None, None, None) == 0
    assert fit(3, 0, None, None, None, None, None, None, None, None) == 0


def test_restatement_reproduces_the_reference_fixture():
    """tests/arap_fit_common.py::fit / energy in float64 give the reference's R, singular values, flip decisions, energy and
    autograd gradient (through torch.svd) of every fixture case to 1e-10: the yardstick of the GPU tests is the reference's code,
    not a formula of ours.  The fixture covers both flip outcomes (noisy) and the "unchanged" rule (yz: R = I everywhere)."""
    fx = afc.load()
    assert tuple(fx["cases"]) == CASES and fx["verts"].dtype == np.float32
    src, nbr, w, e = afc.adjacency(fx["verts"], fx["faces"], torch.float64)
    V = len(fx["verts"])
    for name in CASES:
        xp = torch.tensor(fx[f"{name}_xyz_prime"], requires_grad=True)
        assert xp.dtype == torch.float64 and np.array_equal(fx[f"{name}_xyz_prime"], fx[f"{name}_xyz_prime"].astype(np.float32))
        R, sig, flip, unchanged = afc.fit(src, nbr, w, e, xp)
        E = afc.energy(src, nbr, w, e, xp, R)
        (g,) = torch.autograd.grad(E, xp)
        gw, Ew = fx[f"{name}_g_xyz"], float(fx[f"{name}_energy"])
        print(f"{name}: |dR| {float((R.detach() - torch.tensor(fx[f'{name}_R'])).abs().max()):.2e} |dsig| "
              f"{np.abs(sig.numpy() - fx[f'{name}_sig']).max():.2e} dE {abs(E.item() - Ew):.2e} |dg| {np.abs(g.numpy() - gw).max():.2e}")
        assert np.abs(R.detach().numpy() - fx[f"{name}_R"]).max() <= 1e-10
        assert np.abs(sig.numpy() - fx[f"{name}_sig"]).max() <= 1e-10
        assert np.array_equal(flip.numpy(), fx[f"{name}_flip"])
        assert np.array_equal(unchanged.numpy(), fx[f"{name}_sig"][:, 0] == 0)
        assert abs(E.item() - Ew) <= 1e-10 * max(1.0, abs(Ew))
        assert np.abs(g.numpy() - gw).max() <= 1e-10 * max(1.0, np.abs(gw).max())
    assert 0.1 * V < fx["noisy_flip"].sum() < 0.9 * V
    assert (fx["yz_sig"] == 0).all() and np.array_equal(fx["yz_R"], np.broadcast_to(np.eye(3), (V, 3, 3)))
    assert not (fx["noisy_sig"][:, 0] == 0).any()
    assert np.abs(fx["rigid_R"] - fx["rigid_Q"]).max() <= 1e-5 and abs(float(fx["rigid_energy"])) <= 1e-10


def test_gradient_with_the_rotations_held_fixed_is_the_reference_autograd_gradient():
    """The fitted R is a stationary point of the energy over SO(3) (after the determinant flip too, and an "unchanged" vertex's
    R is a constant), so dE/dxyz_prime with R held fixed -- what k_arap_bwd computes, no SVD derivative -- equals the reference's
    autograd gradient through torch.svd: to 1e-10 on every fixture case."""
    fx = afc.load()
    src, nbr, w, e = afc.adjacency(fx["verts"], fx["faces"], torch.float64)
    for name in CASES:
        xp = torch.tensor(fx[f"{name}_xyz_prime"], requires_grad=True)
        R = torch.tensor(fx[f"{name}_R"])
        (g,) = torch.autograd.grad(afc.energy(src, nbr, w, e, xp, R), xp)
        gw = fx[f"{name}_g_xyz"]
        print(f"{name}: |g_fixedR - g_autograd| {np.abs(g.numpy() - gw).max():.2e} of |g|max {np.abs(gw).max():.2e}")
        assert np.abs(g.numpy() - gw).max() <= 1e-10 * max(1.0, np.abs(gw).max())
