"""The refusal contract of the entry points whose host checks are open-coded (dm4d_simplify_*, dm4d_iso_*, dm4d_dc_*, dm4d_sr_*):
for every call below the return code and the text left in dm4d_last_error() are pinned as literals, recorded from the library
before its host checks moved into csrc/hostcheck.h.  Every call is refused before any launch, so nothing here needs a device.
(The tabled checks of dm4d_mcl_* are pinned by tests/test_mesh_clean_cpu.py.)"""
import pytest

from dreammesh4d_amd import _lib

P = 0x1000                                               # a non-null, 16-byte aligned pointer no refused call ever follows


def _call(fn, args, **change):
    """`args`: list of (name, value); `change` replaces values by name."""
    return fn, tuple(change.get(k, v) for k, v in args)


KEYS = [("V", 8), ("verts", P), ("ox", 0.0), ("oy", 0.0), ("oz", 0.0), ("voxel", 1.0), ("nx", 2), ("ny", 2), ("nz", 2), ("keys", P), ("stream", None)]
AVERAGE = [("V", 8), ("C", 4), ("order", P), ("run_start", P), ("verts", P), ("colors", P), ("out_verts", P), ("out_colors", P),
           ("vertex_cluster", P), ("stream", None)]
REMAP = [("F", 4), ("V", 8), ("C", 4), ("faces", P), ("vertex_cluster", P), ("canon", P), ("key_bc", P), ("stream", None)]
FIRST = [("F", 4), ("perm", P), ("canon", P), ("keep", P), ("stream", None)]

RECORDS = [("N", 8), ("xyzn", P), ("stdn", P), ("rotation", P), ("opacity", P), ("rgb", P), ("num_blocks", 2), ("vmin", P), ("vmax", P),
           ("records", P), ("box", P), ("count", P), ("stream", None)]
PAIRS = [("N", 8), ("P", 16), ("num_blocks", 2), ("box", P), ("offset", P), ("keys", P), ("stream", None)]
CLASSIFY = [("R0", 4), ("R1", 4), ("R2", 4), ("f", P), ("threshold", 0.0), ("code", P), ("n_tris", P), ("n_verts", P), ("stream", None)]
VERTICES = [("R0", 4), ("R1", 4), ("R2", 4), ("f", P), ("csum", P), ("threshold", 0.0), ("code", P), ("vert_start", P), ("V", 8), ("verts", P),
            ("colors", P), ("edge_vertex", P), ("stream", None)]

STATS = [("B", 2), ("N", 8), ("grad2d", P), ("radii", P), ("accum", P), ("denom", P), ("max_radii", P), ("stream", None)]
COUNT = [("N", 8), ("kind", P), ("scratch", P), ("scratch_bytes", 1 << 20), ("totals", P), ("stream", None)]
ROWS = [("N", 8), ("kind", P), ("S", 2), ("scratch", P), ("scratch_bytes", 1 << 20), ("totals", P), ("M", 8), ("src", P), ("role", P),
        ("stream", None)]

FORWARD = [("N", 8), ("K", 4), ("S", 16), ("xyz", P), ("scales", P), ("quats", P), ("opac", P), ("knn_idx", P), ("sample_idx", P), ("order", P),
           ("eps", P), ("sampling_scale", 1.0), ("density_factor", 1.0), ("with_normal_loss", 1), ("scratch", P), ("scratch_bytes", 1 << 30),
           ("density", P), ("beta", P), ("density_term", P), ("normal_term", P), ("losses", P), ("stream", None)]
BACKWARD = [("N", 8), ("K", 4), ("S", 16), ("xyz", P), ("scales", P), ("quats", P), ("opac", P), ("knn_idx", P), ("sample_idx", P), ("order", P),
            ("eps", P), ("sampling_scale", 1.0), ("density_factor", 1.0), ("with_normal_loss", 1), ("upstream", P), ("seg_ptr", P),
            ("chunk_ptr", P), ("rev_ptr", P), ("rev_pos", P), ("scratch", P), ("scratch_bytes", 1 << 30), ("d_xyz", P), ("d_scales", P),
            ("d_quats", P), ("d_opac", P), ("stream", None)]

# name -> ((function, arguments), (return code, dm4d_last_error()) of the library at the commit before csrc/hostcheck.h)
REFUSED = {
    "simplify keys V < 0": (_call("dm4d_simplify_vertex_keys", KEYS, V=-1),
        (-1, 'dm4d_simplify_vertex_keys: V = -1 is outside [0, 2147483647]')),
    "simplify first null perm": (_call("dm4d_simplify_face_first", FIRST, perm=None),
        (-1, 'dm4d_simplify_face_first: null argument')),
    "simplify average colors alone": (_call("dm4d_simplify_cluster_average", AVERAGE, out_colors=None),
        (-1, 'dm4d_simplify_cluster_average: colors and out_colors go together')),
    "simplify remap F too large and null faces": (_call("dm4d_simplify_face_remap", REMAP, F=1 << 31, faces=None),
        (-1, 'dm4d_simplify_face_remap: F = 2147483648 is outside [0, 2147483647]')),
    "iso records N too large": (_call("dm4d_iso_gaussian_records", RECORDS, N=1 << 31),
        (-1, 'dm4d_iso_gaussian_records: N = 2147483648 is outside [0, 2147483647]')),
    "iso pairs P too large": (_call("dm4d_iso_pair_keys", PAIRS, P=1 << 62),
        (-1, 'dm4d_iso_pair_keys: P = 4611686018427387904 is outside [0, 4611686018427387903]')),
    "iso classify null f": (_call("dm4d_iso_mc_classify", CLASSIFY, f=None),
        (-1, 'dm4d_iso_mc_classify: null argument')),
    "iso vertices csum alone": (_call("dm4d_iso_mc_vertices", VERTICES, colors=None),
        (-1, 'dm4d_iso_mc_vertices: csum and colors go together')),
    "iso vertices V < 0 and null verts": (_call("dm4d_iso_mc_vertices", VERTICES, V=-1, verts=None),
        (-1, 'dm4d_iso_mc_vertices: V = -1 is outside [0, 2147483647]')),
    "dc stats N too large": (_call("dm4d_dc_accumulate_stats", STATS, N=_lib.DM4D_DC_MAX_ROWS + 1),
        (-1, 'dm4d_dc_accumulate_stats: N = 268435457 is outside [0, 268435456]')),
    "dc count null totals": (_call("dm4d_dc_plan_count", COUNT, totals=None),
        (-1, 'dm4d_dc_plan_count: null argument')),
    "dc count short scratch": (_call("dm4d_dc_plan_count", COUNT, scratch_bytes=8),
        (-3, 'dm4d_dc_plan_count: scratch of 8 bytes, 16 needed')),
    "dc count misaligned totals": (_call("dm4d_dc_plan_count", COUNT, totals=P + 4),
        (-1, 'dm4d_dc_plan_count: scratch must be 16-byte, totals 8-byte aligned')),
    "dc rows misaligned scratch": (_call("dm4d_dc_plan_rows", ROWS, scratch=P + 8),
        (-1, 'dm4d_dc_plan_rows: scratch must be 16-byte, totals 8-byte, src 4-byte aligned')),
    "dc rows M too large": (_call("dm4d_dc_plan_rows", ROWS, M=17),
        (-1, 'dm4d_dc_plan_rows: M = 17 is outside [0, 16]')),
    "dc count N < 0 and null scratch": (_call("dm4d_dc_plan_count", COUNT, N=-1, scratch=None),
        (-1, 'dm4d_dc_plan_count: N = -1 is outside [0, 268435456]')),
    "sr forward N < 0": (_call("dm4d_sr_forward", FORWARD, N=-1),
        (-1, 'dm4d_sr_forward: N = -1 is outside [0, 33554432]')),
    "sr forward K = 0": (_call("dm4d_sr_forward", FORWARD, K=0),
        (-1, 'dm4d_sr_forward: K = 0 is outside [1, 32]')),
    "sr forward null xyz": (_call("dm4d_sr_forward", FORWARD, xyz=None),
        (-1, 'dm4d_sr_forward: null argument')),
    "sr forward null scratch": (_call("dm4d_sr_forward", FORWARD, scratch=None),
        (-1, 'dm4d_sr_forward: null argument')),
    "sr forward misaligned scratch": (_call("dm4d_sr_forward", FORWARD, scratch=P + 8),
        (-1, 'dm4d_sr_forward: scratch must be 16-byte aligned')),
    "sr backward short scratch": (_call("dm4d_sr_backward", BACKWARD, scratch_bytes=256),
        (-3, 'dm4d_sr_backward: scratch of 256 bytes, 20224 needed')),
    "sr backward S too large and null upstream": (_call("dm4d_sr_backward", BACKWARD, S=_lib.DM4D_SR_MAX_SAMPLES + 1, upstream=None),
        (-1, 'dm4d_sr_backward: S = 536870913 is outside [0, 536870912]')),
}


def refusal(fn, args):
    """(return code, dm4d_last_error()) of one call."""
    L = _lib.lib()
    rc = getattr(L, fn)(*args)
    return rc, L.dm4d_last_error().decode()


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusal_is_what_it_was(name):
    (fn, args), recorded = REFUSED[name]
    assert refusal(fn, args) == recorded
