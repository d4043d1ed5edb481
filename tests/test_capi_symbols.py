"""CPU: libegtr_hip.so builds for gfx950, loads, and exports every symbol include/egtr_hip.h declares.
No compute calls (there is no GPU here)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib_path():
    path = os.path.join(ROOT, "egtr_amd", "libegtr_hip.so")
    if not os.path.exists(path):
        subprocess.run(["make", "-C", os.path.join(ROOT, "egtr_amd", "csrc"), "-j", "4"], check=True)
    return path


def _declared(headers=("egtr_hip.h", "egtr_hip_test.h")):
    """Every entry point declared under include/ (the drop-in boundary + the test-only variant selectors)."""
    names = set()
    for h in headers:
        src = open(os.path.join(ROOT, "include", h)).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        names |= set(re.findall(r"\b(egtr_[a-z0-9_]+)\s*\(", src))
    return sorted(names)


def test_variant_selectors_are_not_part_of_the_public_boundary():
    public = _declared(("egtr_hip.h",))
    assert not [n for n in public if n.endswith("_variant")]
    assert [n for n in _declared(("egtr_hip_test.h",)) if n.endswith("_variant")]


def test_header_declares_the_expected_entry_points():
    names = _declared()
    for n in ("egtr_msda_forward_f32", "egtr_msda_backward_f32", "egtr_msda_forward_bf16",
              "egtr_self_attn_forward_f32", "egtr_self_attn_backward_f32", "egtr_rel_head_forward_save_f32",
              "egtr_abi_version", "egtr_status_string", "egtr_last_hip_error"):
        assert n in names


def test_library_exports_every_declared_symbol(lib_path):
    h = ctypes.CDLL(lib_path)
    for n in _declared():
        assert hasattr(h, n), f"{n} declared in include/egtr_hip.h but not exported"
    h.egtr_abi_version.restype = ctypes.c_int
    assert h.egtr_abi_version() == 7
    h.egtr_status_string.restype = ctypes.c_char_p
    assert b"ok" == h.egtr_status_string(0)


def test_ctypes_binding_covers_the_header(lib_path):
    """The product binding (egtr_amd/_lib.py) is exactly the public boundary; the test-only selectors of egtr_hip_test.h
    are bound by tests/hip_test_abi.py alone."""
    from egtr_amd import _lib
    import hip_test_abi
    assert sorted(_lib.SIGNATURES) == _declared(("egtr_hip.h",))
    assert sorted(hip_test_abi.SIGNATURES) == _declared(("egtr_hip_test.h",))
    assert not set(_lib.SIGNATURES) & set(hip_test_abi.SIGNATURES)
    _lib.lib()  # resolves every symbol with its argtypes
    hip_test_abi._handle()


_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "long long": ctypes.c_longlong}


def _prototypes(header):
    """name -> (restype, argtypes) for every prototype of include/<header>: pointers and egtr_stream_t are c_void_p (a returned
    ``const char*`` is c_char_p), int / float / double / long long their ctypes types.  Anything else raises."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)      # preprocessor lines

    def ctype(decl, returned=False):
        words = [w for w in decl.replace("*", " * ").split() if w != "const"]
        if "*" in words:
            return ctypes.c_char_p if returned and words[0] == "char" else ctypes.c_void_p
        if not returned:
            assert len(words) >= 2 and re.fullmatch(r"[A-Za-z_]\w*", words[-1]), f"{header}: unnamed parameter {decl!r}"
            words = words[:-1]
        if words == ["egtr_stream_t"]:
            return ctypes.c_void_p
        assert " ".join(words) in _SCALARS, f"{header}: no ctypes type for {decl!r}"
        return _SCALARS[" ".join(words)]

    out = {}
    for ret, name, args in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(egtr_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
        assert name not in out, f"{header}: {name} declared twice"
        args = [a.strip() for a in args.split(",")] if args.strip() not in ("", "void") else []
        out[name] = (ctype(ret.strip(), returned=True), [ctype(a) for a in args])
    return out


def test_ctypes_tables_equal_the_headers_prototypes(lib_path):
    """argtypes and restype of every bound entry, as the tables state them and as the loaded functions carry them, equal what
    the headers declare: a c_int for a long long or a float would load and then corrupt a call."""
    from egtr_amd import _lib
    import hip_test_abi
    for header, table, handle in (("egtr_hip.h", _lib.SIGNATURES, _lib.lib()),
                                  ("egtr_hip_test.h", hip_test_abi.SIGNATURES, hip_test_abi._handle())):
        protos = _prototypes(header)
        assert sorted(protos) == _declared((header,)), f"{header}: a prototype the parser could not read"
        assert sorted(table) == sorted(protos)
        for name, (restype, argtypes) in protos.items():
            fn = getattr(handle, name)
            assert list(table[name]) == argtypes, f"{name}: table {table[name]}, header {argtypes}"
            assert list(fn.argtypes) == argtypes and fn.restype is restype, f"{name}: bound as {fn.restype} {fn.argtypes}"
            if table is _lib.SIGNATURES:
                assert _lib._RESTYPES.get(name, ctypes.c_int) is restype, f"{name}: _RESTYPES vs header {restype}"
    assert not set(_lib._RESTYPES) - set(_lib.SIGNATURES)


@pytest.mark.parametrize("terms", [0, 3, 7, 6, 1])
def test_split_gemm_entries_validate_terms_without_a_gpu(lib_path, terms):
    """``terms`` other than 6 / 1 is EGTR_E_ARG (the workspace query: 0) with otherwise plausible non-NULL arguments; 6 / 1 with a
    NULL operand is EGTR_E_ARG as before.  Both answers come before any HIP call."""
    from egtr_amd import _lib
    h = _lib.lib()
    good = terms in (6, 1)
    # for a bad `terms` every operand is plausible, so that `terms` is the ONLY reason for EGTR_E_ARG: `p` a 16-byte aligned host
    # address, `pa` a one-entry host array holding it (the pointer-array arguments: their entries are looked at too), `ia` a
    # one-entry int array of 128 (row strides, N, K, pos_rows, split_rows: 128 x 128 problems).  For a valid `terms`: all NULL.
    raw = ctypes.create_string_buffer(64 + 16)
    addr = (ctypes.addressof(raw) + 15) & ~15
    ptrs, ints = (ctypes.c_void_p * 1)(addr), (ctypes.c_int * 1)(128)
    p, pa, ia = (None, None, None) if good else (addr, ctypes.addressof(ptrs), ctypes.addressof(ints))
    E_ARG = -1
    assert h.egtr_linear_split_bf16_ex_f32(None, 1, pa, ia, pa, pa, pa, ia, ia, ia, 128, 128, pa, ia, pa, pa, ia, pa, pa, ia, pa,
                                           terms) == E_ARG
    assert h.egtr_linear_split_bf16_wgrad_ex_f32(None, p, 128, p, 128, p, p, 128, 128, 128, p, 1, p, terms) == E_ARG
    assert h.egtr_gemm_split_tile_weights_f32(None, p, 128, 0, 128, 128, p, terms) == E_ARG
    assert h.egtr_gemm_split_tile_weights_pair_f32(None, p, 128, 128, 128, p, terms) == E_ARG
    assert h.egtr_gemm_split_tile_weights_multi_f32(None, 1, pa, ia, pa, ia, ia, ia, ia, pa, terms) == E_ARG
    floats = h.egtr_linear_split_bf16_wgrad_workspace_floats(128, 128, 128, terms)
    assert (floats > 0) if good else (floats == 0)
    assert h.egtr_linear_split_bf16_wgrad_workspace_floats(128, 128, 100, terms) == 0


def test_null_arguments_are_rejected_without_a_gpu(lib_path):
    """Argument validation happens before any HIP call, so it is checkable on a CPU-only box."""
    from egtr_amd import _lib
    h = _lib.lib()
    st = h.egtr_msda_forward_f32(None, None, None, None, None, None, 1, 1, 8, 32, 4, 1, 4, None)
    assert st == -1
    st = h.egtr_self_attn_forward_f32(None, None, None, None, 1, 1, 8, 32, None, None, None, None)
    assert st == -1
    assert b"invalid" in h.egtr_status_string(-1)
    with pytest.raises(_lib.EgtrHipError):
        _lib.check(st, "x")


def test_usable_cpus_respects_affinity_and_is_applied_to_torch():
    """tests/conftest.py sizes torch's intra-op pool to the CPUs this process may use (the GPU boxes show 256 cores behind
    a 16-CPU quota; the default 128 threads made the oracle passes several times slower)."""
    import os

    import torch

    import conftest
    n = conftest.usable_cpus()
    assert 1 <= n <= (os.cpu_count() or 1)
    assert n <= len(os.sched_getaffinity(0))
    assert torch.get_num_threads() == max(1, min(n, 16))
