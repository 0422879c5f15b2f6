"""Adaptive density control without a device: the mask-indexing restatement reproduces the reference's golden stages, the library
exports what include/dm4d_density.h declares, the host-side argument checks refuse before any launch, the API refuses CPU tensors."""
import ctypes

import numpy as np
import pytest
import torch

from dreammesh4d_amd import _lib, density_control as dc, gaussian_model as gm, threestudio_host as host
from tests import density_control_common as cm


@pytest.fixture(scope="module")
def z():
    return cm.golden()


@pytest.mark.parametrize("case", ["A", "B"])
def test_restatement_reproduces_the_golden_stages(z, case):
    """float32: row order, counts and every copied row exactly; float64: the computed values to 1e-12."""
    want = cm.golden_stages(z, case)
    for dtype in (torch.float32, torch.float64):
        got = cm.replay(z, case, dtype)
        assert [g[0] for g in got] == list(cm.STAGES)
        for (stage, state, src, new), w in zip(got, want):
            what = f"case {case} {stage} {dtype}"
            assert state["params"]["xyz"].shape[0] == len(w["src"]), what
            assert np.array_equal(src.numpy(), w["src"]), f"{what}: row order"
            if stage == "densify":
                assert np.array_equal(new.numpy(), w["new"]), f"{what}: new rows"
            if dtype == torch.float32:
                cm.compare_state(state, w, what, factor=4.0)
            else:
                cm.compare_state(state, w, what, atol=1e-12)


def test_golden_has_every_kind(z):
    for case in ("A", "B"):
        st = cm.replay(z, case, torch.float32)[0][1]
        kinds = cm.kinds_densify(st, float(z["grad_threshold"]), float(z["split_thresh"]), case == "B").numpy()
        assert min((kinds == k).sum() for k in (0, 2, 3)) >= 30
        n_before, n_after = len(z[f"{case}/densify/src"]), len(z[f"{case}/prune/src"])
        assert n_before - n_after >= 30


def test_expected_rows_is_the_reference_order():
    kind = np.array([0, 2, 3, 1, 3, 2, 0], np.uint8)
    src, role = cm.expected_rows(kind, 2)
    assert src.tolist() == [0, 1, 5, 6, 1, 5, 2, 4, 2, 4]
    assert role.tolist() == [0, 0, 0, 0, 1, 1, 2, 2, 3, 3]


def test_library_exports_the_header():
    L = _lib.lib()
    names = _lib.declared_symbols("dc")
    assert {"dm4d_dc_version", "dm4d_dc_accumulate_stats", "dm4d_dc_classify_densify", "dm4d_dc_classify_prune", "dm4d_dc_plan_count",
            "dm4d_dc_plan_rows", "dm4d_dc_move", "dm4d_dc_reset_opacity"} <= set(names)
    assert [n for n in names if not hasattr(L, n)] == []
    assert L.dm4d_dc_version() == _lib.abi_version("dc") == 1
    assert _lib.abi_version() == 107                    # include/dm4d.h keeps its number
    assert (dc.KEEP, dc.DROP, dc.CLONE, dc.SPLIT) == (0, 1, 2, 3)


def test_registered_as_gaussian_splatting():
    assert host.find("gaussian-splatting") is gm.GaussianModel
    m = gm.GaussianModel({"init_num_pts": 0, "sh_degree": 2, "pred_normal": True})
    assert m.max_sh_degree == 2 and m.optimizer is None and m._xyz.numel() == 0
    with pytest.raises(KeyError):
        gm.GaussianModel({"init_num_pts": 0, "no_such_key": 1})


P = 0x1000                                               # a non-null pointer no refused call ever follows
TOO_MANY = _lib.DM4D_DC_MAX_ROWS + 1


def _table(count, width=3, flags=0, null=False):
    A = _lib.DcArrays()
    A.count = count
    for a in range(min(max(count, 0), _lib.DM4D_DC_MAX_ARRAYS)):
        getattr(A, "in")[a], A.out[a], A.width[a], A.flags[a] = (None if null else P), P, width, flags
    return ctypes.byref(A)


REFUSED = {
    "stats N < 0": ("dm4d_dc_accumulate_stats", (1, -1, P, P, P, P, P, None)),
    "stats N too large": ("dm4d_dc_accumulate_stats", (1, TOO_MANY, P, P, P, P, P, None)),
    "stats B < 0": ("dm4d_dc_accumulate_stats", (-1, 4, P, P, P, P, P, None)),
    "stats null": ("dm4d_dc_accumulate_stats", (1, 4, P, None, P, P, P, None)),
    "densify N < 0": ("dm4d_dc_classify_densify", (-1, P, P, P, 0.1, 0.1, 0, P, None)),
    "densify N too large": ("dm4d_dc_classify_densify", (TOO_MANY, P, P, P, 0.1, 0.1, 0, P, None)),
    "densify threshold 0": ("dm4d_dc_classify_densify", (4, P, P, P, 0.0, 0.1, 0, P, None)),
    "densify threshold nan": ("dm4d_dc_classify_densify", (4, P, P, P, float("nan"), 0.1, 0, P, None)),
    "densify null": ("dm4d_dc_classify_densify", (4, P, P, None, 0.1, 0.1, 0, P, None)),
    "prune N < 0": ("dm4d_dc_classify_prune", (-1, P, 0.1, None, None, P, None)),
    "prune null": ("dm4d_dc_classify_prune", (4, None, 0.1, None, None, P, None)),
    "prune limit without radii": ("dm4d_dc_classify_prune", (4, P, 0.1, None, P, P, None)),
    "scratch N < 0": ("dm4d_dc_plan_scratch_bytes", (-1,)),
    "scratch N too large": ("dm4d_dc_plan_scratch_bytes", (TOO_MANY,)),
    "count N too large": ("dm4d_dc_plan_count", (TOO_MANY, P, P, 1 << 30, P, None)),
    "count null": ("dm4d_dc_plan_count", (4, None, P, 16, P, None)),
    "rows S = 0": ("dm4d_dc_plan_rows", (4, P, 0, P, 16, P, 4, P, P, None)),
    "rows S = 9": ("dm4d_dc_plan_rows", (4, P, 9, P, 16, P, 4, P, P, None)),
    "rows N < 0": ("dm4d_dc_plan_rows", (-4, P, 2, P, 16, P, 4, P, P, None)),
    "rows M too large": ("dm4d_dc_plan_rows", (4, P, 2, P, 16, P, 9, P, P, None)),
    "rows null": ("dm4d_dc_plan_rows", (4, P, 2, P, 16, P, 4, None, P, None)),
    "move N too large": ("dm4d_dc_move", (TOO_MANY, 4, P, P, _table(1), None)),
    "move M < 0": ("dm4d_dc_move", (4, -1, P, P, _table(1), None)),
    "move no table": ("dm4d_dc_move", (4, 4, P, P, None, None)),
    "move 25 arrays": ("dm4d_dc_move", (4, 4, P, P, _table(25), None)),
    "move -1 arrays": ("dm4d_dc_move", (4, 4, P, P, _table(-1), None)),
    "move width 0": ("dm4d_dc_move", (4, 4, P, P, _table(2, width=0), None)),
    "move width < 0": ("dm4d_dc_move", (4, 4, P, P, _table(2, width=-3), None)),
    "move unknown flag": ("dm4d_dc_move", (4, 4, P, P, _table(2, flags=8), None)),
    "move null array": ("dm4d_dc_move", (4, 4, P, P, _table(2, null=True), None)),
    "move null src": ("dm4d_dc_move", (4, 4, None, P, _table(2), None)),
    "children S = 0": ("dm4d_dc_split_children", (4, 8, 4, 0, 0, P, P, P, P, P, P, P, P, None)),
    "children S = 9": ("dm4d_dc_split_children", (4, 8, 4, 9, 0, P, P, P, P, P, P, P, P, None)),
    "children first > M": ("dm4d_dc_split_children", (4, 8, 9, 2, 0, P, P, P, P, P, P, P, P, None)),
    "children null": ("dm4d_dc_split_children", (4, 8, 4, 2, 0, P, P, P, P, P, None, P, P, None)),
    "reset N < 0": ("dm4d_dc_reset_opacity", (-1, P, None, None, None)),
    "reset null": ("dm4d_dc_reset_opacity", (4, None, None, None, None)),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_host_validation_refuses_without_a_device(name):
    fn, args = REFUSED[name]
    rc = getattr(_lib.lib(), fn)(*args)
    assert rc == _lib.DM4D_ERR_INVALID, f"{fn}{args} returned {rc}"
    assert fn.encode() in _lib.lib().dm4d_last_error()


def test_scratch_size_and_capacity():
    L = _lib.lib()
    assert L.dm4d_dc_plan_scratch_bytes(0) == 16 and L.dm4d_dc_plan_scratch_bytes(4096) == 16 and L.dm4d_dc_plan_scratch_bytes(4097) == 32
    assert L.dm4d_dc_plan_scratch_bytes(_lib.DM4D_DC_MAX_ROWS) == 16 * 65536
    assert L.dm4d_dc_plan_count(5000, P, P, 16, P, None) == _lib.DM4D_ERR_CAPACITY
    # nothing to do is a success that launches nothing
    assert L.dm4d_dc_accumulate_stats(3, 0, None, None, None, None, None, None) == 0
    assert L.dm4d_dc_move(4, 0, None, None, _table(2), None) == 0
    assert L.dm4d_dc_reset_opacity(0, None, None, None, None) == 0


def test_move_refuses_more_workgroups_than_a_launch_holds():
    """2^31 output rows of 24 arrays of 2^20 floats: refused by name on the host, nothing is launched."""
    L = _lib.lib()
    n = _lib.DM4D_DC_MAX_ROWS
    assert L.dm4d_dc_move(n, 8 * n, P, P, _table(24, width=1 << 20), None) == _lib.DM4D_ERR_UNSUPPORTED
    assert b"several calls" in L.dm4d_last_error()
    # 2^24 workgroups of 256 threads are one too many for a launch: 2^24 * 1024 units of a width-1 array
    assert L.dm4d_dc_move(n, 64 * n, P, P, _table(1, width=1), None) == _lib.DM4D_ERR_INVALID       # M > 8 N is refused first
    assert L.dm4d_dc_move(n, 8 * n, P, P, _table(8, width=1), None) == _lib.DM4D_ERR_UNSUPPORTED    # 8 x 2^21 workgroups


def test_model_can_be_moved_and_cast_like_any_module():
    """``.to()`` / ``.float()`` go through ``nn.Module._apply``, which the model must not shadow -- alone and inside a parent."""
    m = gm.GaussianModel({"init_num_pts": 0})
    assert m.to("cpu") is m and m.float() is m
    parent = torch.nn.Module()
    parent.geometry = m
    parent.head = torch.nn.Linear(2, 2)
    assert parent.to("cpu") is parent and parent.double().head.weight.dtype == torch.float64
    m2 = gm.GaussianModel({"init_num_pts": 0, "pred_normal": True})
    st = cm.random_state(5, 0, 1)
    for name, v in st["params"].items():
        setattr(m2, m2._GROUPS[name], torch.nn.Parameter(v.clone()))
    m2.training_setup()
    m2.to("cpu")
    assert m2.double()._xyz.dtype == torch.float64 and m2.float()._xyz.dtype == torch.float32
    assert torch.equal(m2._xyz.data, st["params"]["xyz"])


def test_registry_keeps_outside_classes_beside_its_own():
    assert "gaussian-splatting" in host.__extensions__ and "gaussian-splatting" not in host.__modules__
    assert set(host.registered()) == set(host.__modules__) | {"gaussian-splatting"}
    with pytest.raises(ValueError):
        host.register("gaussian-splatting")(object)


def test_api_refuses_cpu_tensors():
    n = 8
    st = cm.random_state(n, 0, 0)
    f = torch.zeros(n)
    with pytest.raises(_lib.Dm4dError, match="no CPU path"):
        dc.accumulate_stats(torch.zeros(1, n, 3), torch.zeros(1, n, dtype=torch.int32), f.clone(), f.clone(), f.clone())
    with pytest.raises(_lib.Dm4dError, match="no CPU path"):
        dc.classify_densify(f, f, st["params"]["scaling"], 0.1, 0.1)
    with pytest.raises(_lib.Dm4dError, match="no CPU path"):
        dc.classify_prune(st["params"]["opacity"], 0.1)
    with pytest.raises(_lib.Dm4dError, match="no CPU path"):
        dc.apply(torch.zeros(n, dtype=torch.uint8), st["params"], None)
    with pytest.raises(_lib.Dm4dError, match="no CPU path"):
        dc.reset_opacity(st["params"]["opacity"])
