"""The table of headers the ctypes binding is derived from (_lib.HEADERS): every row parses, the union of the declared functions
is what all_declared_symbols() returns, the built library exports every one of them and answers every header's version."""
from dreammesh4d_amd import _lib

KEYS = ["dm4d", "iso", "dc", "sr", "mcl"]


def test_every_header_of_the_table_parses():
    assert [h.key for h in _lib.HEADERS] == KEYS == list(_lib._PARSED)
    for h in _lib.HEADERS:
        constants, structs, signatures = _lib._PARSED[h.key]
        assert signatures and h.version_fn in signatures and h.version_macro in constants, h.file
        assert _lib.declared_symbols(h.key) == sorted(signatures) and _lib.abi_version(h.key) == constants[h.version_macro]
    assert (_lib._CONSTANTS, _lib._STRUCTS, _lib._SIGNATURES) == _lib._PARSED["dm4d"]
    assert _lib.declared_symbols() == _lib.declared_symbols("dm4d") and _lib.abi_version() == _lib.abi_version("dm4d") == 107


def test_all_declared_symbols_is_the_union_without_duplicates():
    per_header = [name for key in KEYS for name in _lib.declared_symbols(key)]
    assert len(per_header) == len(set(per_header)) == 127 + 7 + 10 + 4 + 7
    assert _lib.all_declared_symbols() == sorted(per_header)


def test_the_library_exports_every_symbol_and_answers_every_version():
    L = _lib.lib()
    assert [name for name in _lib.all_declared_symbols() if not hasattr(L, name)] == []
    for h in _lib.HEADERS:
        assert getattr(L, h.version_fn)() == _lib.abi_version(h.key), h.file
    assert [_lib.abi_version(key) for key in KEYS] == [107, 1, 1, 1, 1]
