"""ctypes binding of libdm4d_hip.so, derived from the headers of its C ABI under include/ (the table ``HEADERS`` below).

The product path has NO fallback: if the HIP library is missing or fails to load,
importing an operator raises.  (The CPU restatements under oracle/ are test
infrastructure and are never imported from here.)
"""
import ctypes as C
import os
import re
import subprocess
from collections import namedtuple

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "libdm4d_hip.so")
_LIB = None

c_f = C.POINTER(C.c_float)
c_i32 = C.POINTER(C.c_int32)
c_u32 = C.POINTER(C.c_uint32)
c_u64 = C.POINTER(C.c_uint64)
c_u8 = C.POINTER(C.c_uint8)


class Dm4dError(RuntimeError):
    pass


# the one function-pointer typedef of the header; the parser refuses any other
ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_int, C.c_size_t)

_SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "char": C.c_char, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
            "int32_t": C.c_int32, "int64_t": C.c_int64, "uint8_t": C.c_uint8, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
_DECLARATOR = re.compile(r"(?:(?P<type>\w[\w\s]*?)(?=[\s*])\s*)?(?P<stars>(?:\*\s*(?:const\b\s*)?)*)(?P<name>\w+)(?:\[(?P<bound>\w+)\])?")


def parse_header(text, fn_typedefs=None):
    """(constants, structs, signatures) of a C header written the way include/dm4d.h is: `#define NAME <integer>`, `typedef struct
    tag { fields } name;` and `ret name(args);`.  constants: name -> int.  structs: C name -> ctypes.Structure, fields in
    declaration order (fixed-width scalars, c_void_p for every pointer, `type * N` for arrays, earlier structs by value).
    signatures: name -> (restype, argtypes); an argument that points to one of the structs is POINTER(struct), a function-pointer
    typedef is looked up in `fn_typedefs`, every other pointer is c_void_p (device pointers arrive as ints), a returned pointer is
    c_void_p too, or c_char_p for `char *`.  Anything else raises ValueError naming the text: nothing is skipped."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#[ \t]*ifdef[ \t]+__cplusplus\b.*?^[ \t]*#[ \t]*endif\b[^\n]*", "", text, flags=re.S | re.M)   # C, not C++
    constants, structs, signatures = {}, {}, {}
    known = dict(_SCALARS, void=None)       # every type name a declaration may use -> what it is by value (None: only behind a pointer)
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\S[^\n]*?)[ \t]*$", text, flags=re.M):
        try:
            constants[name] = int(value, 0)
        except ValueError:
            raise ValueError(f"#define {name} {value}: not an integer literal") from None
    text = re.sub(r"^[ \t]*#[^\n]*", "", text, flags=re.M)

    def declarator(decl, base=None, struct_pointers=False):
        """ctype and name of `[type] [*...] name [[N]]`; `base` is the type of a second declarator (`float *a, *b`)."""
        m = _DECLARATOR.fullmatch(decl.strip())
        words = [w for w in ((m and m["type"]) or base or "").split() if w not in ("const", "struct")]
        if not m or (m["type"] and base) or len(words) != 1:
            raise ValueError(f"cannot parse declaration '{decl.strip()}'")
        if words[0] not in known:
            raise ValueError(f"unknown type '{words[0]}' in '{decl.strip()}'")
        stars, t = m["stars"].count("*"), known[words[0]]
        if stars:
            t = C.POINTER(t) if struct_pointers and stars == 1 and words[0] in structs else C.c_void_p
        elif t is None:
            raise ValueError(f"'{words[0]}' by value in '{decl.strip()}'")
        if m["bound"]:
            if not m["bound"].isdigit() and m["bound"] not in constants:
                raise ValueError(f"unknown array bound '{m['bound']}' in '{decl.strip()}'")
            t = t * (int(m["bound"]) if m["bound"].isdigit() else constants[m["bound"]])
        return t, m["name"], m["type"] or base

    depth, begin, statements = 0, 0, []
    for i, ch in enumerate(text):
        depth += (ch == "{") - (ch == "}")
        if ch == ";" and depth == 0:
            statements.append(" ".join(text[begin:i].split()))
            begin = i + 1
    if depth or text[begin:].strip():
        raise ValueError(f"cannot parse declaration '{' '.join(text[begin:].split())[:200]}'")

    for st in statements:
        if m := re.fullmatch(r"typedef struct (\w+) \{(.*)\} (\w+)", st):
            fields = []
            for field in filter(None, (f.strip() for f in m[2].split(";"))):
                base = None
                for decl in field.split(","):
                    t, name, base = declarator(decl, base)
                    fields.append((name, t))
            known[m[3]] = structs[m[3]] = type(m[3], (C.Structure,), {"_fields_": fields, "__doc__": f"{m[3]} (include/dm4d.h)."})
        elif m := re.fullmatch(r"typedef struct (\w+) (\w+)", st):          # opaque handle: only ever behind a pointer
            known[m[2]] = None
        elif m := re.fullmatch(r"typedef [^()]*\(\s*\*\s*(\w+)\s*\)\s*\(.*\)", st):
            if m[1] not in (fn_typedefs or {}):
                raise ValueError(f"unknown function-pointer typedef '{m[1]}' in '{st}'")
            known[m[1]] = fn_typedefs[m[1]]
        elif st.startswith("typedef "):
            t, name, _ = declarator(st[len("typedef "):])
            known[name] = t
        elif m := re.fullmatch(r"([\w\s*]+?)\b(\w+) ?\((.*)\)", st):
            ret = m[1].replace("const", " ").replace("*", " * ").split()
            if not ret or ret[0] not in known or ret[1:] != ["*"] * (len(ret) - 1):
                raise ValueError(f"unknown return type '{m[1].strip()}' in '{st}'")
            res = (C.c_char_p if ret[0] == "char" else C.c_void_p) if len(ret) > 1 else known[ret[0]]
            args = [] if m[3].strip() == "void" else [declarator(a, struct_pointers=True)[0] for a in m[3].split(",")]
            signatures[m[2]] = (res, args)
        else:
            raise ValueError(f"cannot parse declaration '{st}'")
    return constants, structs, signatures


# One row per header of the C ABI: file under include/, key, the library's version function, the header's version macro, which
# constants become names of this module (None: all, a tuple of prefixes, or a dict {module name: constant}), and the structs that
# get a module-level alias {module name: C name}.  Every header keeps its own functions and its own version number.  Adding a
# header is adding a row.
Header = namedtuple("Header", "file key version_fn version_macro constants structs")
HEADERS = tuple(Header(*row) for row in (
    ("dm4d.h", "dm4d", "dm4d_version", "DM4D_ABI_VERSION", None,
     {"RasterSettings": "dm4d_raster_settings", "RasterInputs": "dm4d_raster_inputs", "ViewsStruct": "dm4d_views",
      "ViewsGrads": "dm4d_views_grads", "GViewsStruct": "dm4d_gviews", "GViewsGrads": "dm4d_gviews_grads",
      "MlpWeights": "dm4d_mlp_weights", "MlpWeightsGrad": "dm4d_mlp_weights_grad", "StepDesc": "dm4d_step_desc",
      "GradSegments": "dm4d_grad_segments", "AdamwArgs": "dm4d_adamw_args", "AdamwStepArgs": "dm4d_adamw_step_args"}),
    ("dm4d_isosurface.h", "iso", "dm4d_iso_version", "DM4D_ISO_ABI_VERSION",
     {"ISO_RECORD_FLOATS": "DM4D_ISO_RECORD_FLOATS", "ISO_MAX_RESOLUTION": "DM4D_ISO_MAX_RESOLUTION"}, {}),
    ("dm4d_density.h", "dc", "dm4d_dc_version", "DM4D_DC_ABI_VERSION", ("DM4D_DC_",), {"DcArrays": "dm4d_dc_arrays"}),
    ("dm4d_sugar_reg.h", "sr", "dm4d_sr_version", "DM4D_SR_ABI_VERSION", ("DM4D_SR_",), {}),
    ("dm4d_mesh_clean.h", "mcl", "dm4d_mcl_version", "DM4D_MCL_ABI_VERSION", ("DM4D_MCL_",), {}),
))
_PARSED = {}                            # key -> (constants, structs, signatures)
for _h in HEADERS:
    with open(os.path.join(os.path.dirname(_HERE), "include", _h.file)) as _f:
        _c, _s, _ = _PARSED[_h.key] = parse_header(_f.read(), {"dm4d_alloc_fn": ALLOC_FN})
    if isinstance(_h.constants, dict):
        globals().update({k: _c[v] for k, v in _h.constants.items()})                           # _lib.ISO_RECORD_FLOATS
    else:
        globals().update({k: v for k, v in _c.items() if _h.constants is None or k.startswith(_h.constants)})     # _lib.DM4D_DC_SPLIT
    globals().update({k: _s[v] for k, v in _h.structs.items()})                                 # _lib.RasterSettings
_CONSTANTS, _STRUCTS, _SIGNATURES = _PARSED["dm4d"]
OK = _CONSTANTS["DM4D_OK"]
MAX_GRAD_SEGMENTS = _CONSTANTS["DM4D_MAX_GRAD_SEGMENTS"]


def declared_symbols(header="dm4d"):
    """Every function the header with key `header` declares."""
    return sorted(_PARSED[header][2])


def abi_version(header="dm4d") -> int:
    """The version macro of the header with key `header` (the header the binding is derived from)."""
    return _PARSED[header][0][next(h.version_macro for h in HEADERS if h.key == header)]


def all_declared_symbols():
    """Every function any header of the table declares."""
    return sorted(name for _, _, signatures in _PARSED.values() for name in signatures)


def build(force: bool = False) -> str:
    """Compile libdm4d_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    csrc = os.path.join(_HERE, "csrc")
    cmd = ["make", "-s", "-C", csrc, "-j8"]
    if force:
        cmd.append("-B")
    subprocess.check_call(cmd)
    return SO_PATH


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        if not os.path.exists(SO_PATH):
            raise ImportError(
                f"{SO_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  dreammesh4d_amd has no CPU fallback.")
        L = C.CDLL(SO_PATH)
        for h in HEADERS:
            for name, (res, args) in _PARSED[h.key][2].items():
                fn = getattr(L, name)
                fn.restype = res
                fn.argtypes = args
            have, want = getattr(L, h.version_fn)(), abi_version(h.key)
            if have != want:
                raise ImportError(f"{SO_PATH} has ABI version {have} of include/{h.file}, the header declares {want}: rebuild it "
                                  "(`python -c 'import __graft_entry__ as g; g.build()'`)")
        _LIB = L
    return _LIB


def check(rc, what=""):
    if rc is not None and rc < 0:
        msg = lib().dm4d_last_error()
        raise Dm4dError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
    return rc


def call(name, *args):
    """Call entry point `name` and raise Dm4dError (with the name and the library's message) on a negative return."""
    return check(getattr(lib(), name)(*args), name)


def ptr(t):
    return None if t is None else t.data_ptr()


def stream(dev):
    """Handle of torch's current stream on `dev`."""
    import torch

    return torch.cuda.current_stream(dev).cuda_stream
