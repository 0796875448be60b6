"""Ledger of csrc/stil_cgpl.h (stil_tta_amd._lib.CGPL_HEADERS), in the style of tests/test_read_abi_ledger_cpu.py: every prototype
names the tests that check it directly, the library exports it and _lib binds it; the header lives beside its kernels, not in
include/ (whose file list is closed), its names collide with no other header's, and the library version stays 106."""
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

_GPU, _CPU = "test_gpu_cgpl.py", "test_cgpl_cpu.py"
LEDGER = {"stil_cgpl_rows": [f"{_GPU}::test_cgpl_rows_against_float64", f"{_GPU}::test_cgpl_rows_rejects_bad_arguments_with_nothing_written",
                             f"{_CPU}::test_closed_form_gradient_is_float64_autograd", f"{_CPU}::test_fp32_aten_cgpl_meets_tol_on_well_posed_inputs",
                             f"{_CPU}::test_the_restatement_reproduces_the_oracles_training_step"]}


def _protos():
    from stil_tta_amd._lib import CGPL_HEADERS, parse_header
    (path,) = CGPL_HEADERS
    assert os.path.basename(path) == "stil_cgpl.h" and os.path.exists(path)
    return parse_header(path)


def test_the_prototypes_of_the_header_are_the_ledgers_keys():
    assert set(_protos()) == set(LEDGER), (sorted(_protos()), sorted(LEDGER))


def test_the_prototype_is_the_one_the_binding_calls():
    (restype, args), = _protos().values()
    assert restype is ctypes.c_int
    assert [n for _, n in args] == ["Zm", "Zi", "Zt", "ld", "feat", "protos", "coin", "rows", "K", "Dp", "T", "rate", "th", "grad_scale", "lse3",
                                    "p", "q", "ldp", "conf", "flags", "ce3", "dZm", "dZi", "dZt", "ldd", "counts", "out", "active", "gate",
                                    "n_tensors", "ws", "stream"]
    kinds = {"Zm": ctypes.c_void_p, "ld": ctypes.c_int, "coin": ctypes.c_void_p, "Dp": ctypes.c_int, "T": ctypes.c_float, "rate": ctypes.c_float,
             "th": ctypes.c_float, "grad_scale": ctypes.c_float, "lse3": ctypes.c_void_p, "ldd": ctypes.c_int, "n_tensors": ctypes.c_int,
             "ws": ctypes.c_void_p, "stream": ctypes.c_void_p}
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
        assert hasattr(dll, name), f"{name} declared in csrc/stil_cgpl.h but not exported"
    assert set(_protos()) <= set(lib().protos)
    assert lib().version() == 106


def test_the_header_stays_out_of_include_and_collides_with_nothing():
    from stil_tta_amd._lib import CGPL_HEADERS, HEADER, MEMORY_HEADERS, READ_HEADERS, TTA_HEADERS, parse_header
    include = os.path.dirname(HEADER)
    assert all(os.path.dirname(p) != include for p in CGPL_HEADERS)
    others = tuple(TTA_HEADERS) + tuple(MEMORY_HEADERS) + tuple(READ_HEADERS)
    assert not set(CGPL_HEADERS) & set(others) and len(MEMORY_HEADERS) == 1 and len(READ_HEADERS) == 1
    mine = set(_protos())
    for path in (HEADER,) + others:
        assert not mine & set(parse_header(path)), path
