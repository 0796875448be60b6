"""Ledger of csrc/stil_read.h (stil_tta_amd._lib.READ_HEADERS), in the style of tests/test_bnmemory_abi_ledger_cpu.py: every
prototype names the tests that check it directly, the library exports it and _lib binds it; the header lives beside its kernels, not
in include/ (whose file list is closed), its names collide with no other header's, and the library version stays 106."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

from test_abi_ledger_cpu import _test_functions  # noqa: E402

_GPU, _CPU = "test_gpu_read.py", "test_read_cpu.py"
LEDGER = {"stil_read_rows": [f"{_GPU}::test_read_rows_against_float64", f"{_GPU}::test_read_rows_rejects_bad_arguments_with_nothing_written",
                             f"{_CPU}::test_closed_form_gradient_is_float64_autograd", f"{_CPU}::test_fp32_aten_read_meets_tol"]}


def _protos():
    from stil_tta_amd._lib import READ_HEADERS, parse_header
    (path,) = READ_HEADERS
    assert os.path.basename(path) == "stil_read.h" and os.path.exists(path)
    return parse_header(path)


def test_the_prototypes_of_the_header_are_the_ledgers_keys():
    assert set(_protos()) == set(LEDGER), (sorted(_protos()), sorted(LEDGER))


def test_the_prototype_is_the_one_the_binding_calls():
    (restype, args), = _protos().values()
    assert restype is ctypes.c_int
    assert [n for _, n in args] == ["Z", "ld", "rows", "K", "grad_scale", "gamma", "div_weight", "eps", "lse", "p", "ldp", "yhat", "conf",
                                    "f", "pbar", "dZ", "ldd", "out", "ws", "stream"]
    kinds = {"Z": ctypes.c_void_p, "ld": ctypes.c_int, "grad_scale": ctypes.c_float, "gamma": ctypes.c_float, "ws": ctypes.c_void_p}
    assert all(dict((n, t) for t, n in args)[n] is t for n, t in kinds.items())


def test_every_entry_point_names_direct_tests_that_exist():
    for name, refs in LEDGER.items():
        assert refs, name
        for ref in refs:
            fname, func = ref.split("::")
            assert func in _test_functions(fname), f"{name}: {ref} does not exist"


def test_library_exports_and_binds_every_prototype_at_version_106():
    import __graft_entry__ as G
    G.build()
    from stil_tta_amd._lib import LIB_PATH, lib
    dll = ctypes.CDLL(LIB_PATH)
    for name in _protos():
        assert hasattr(dll, name), f"{name} declared in csrc/stil_read.h but not exported"
    assert set(_protos()) <= set(lib().protos)
    assert lib().version() == 106


def test_the_header_stays_out_of_include_and_collides_with_nothing():
    from stil_tta_amd._lib import HEADER, MEMORY_HEADERS, READ_HEADERS, TTA_HEADERS, parse_header
    include = os.path.dirname(HEADER)
    assert all(os.path.dirname(p) != include for p in READ_HEADERS)
    assert not set(READ_HEADERS) & (set(TTA_HEADERS) | set(MEMORY_HEADERS)) and len(MEMORY_HEADERS) == 1
    mine = set(_protos())
    for path in (HEADER,) + tuple(TTA_HEADERS) + tuple(MEMORY_HEADERS):
        assert not mine & set(parse_header(path)), path
