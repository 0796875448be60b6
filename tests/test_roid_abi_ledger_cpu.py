"""Ledger of csrc/stil_roid.h (stil_tta_amd._lib.ROID_HEADERS), in the style of tests/test_cgpl_abi_ledger_cpu.py: every prototype
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

_GPU, _CPU = "test_gpu_roid.py", "test_roid_cpu.py"
LEDGER = {
    "stil_roid_rows": [f"{_GPU}::test_roid_rows_against_float64", f"{_GPU}::test_entry_points_reject_bad_arguments_with_nothing_written",
                       f"{_CPU}::test_closed_form_gradient_is_float64_autograd", f"{_CPU}::test_the_cases_are_well_posed"],
    "stil_roid_ensemble": [f"{_GPU}::test_roid_ensemble_against_float64", f"{_GPU}::test_entry_points_reject_bad_arguments_with_nothing_written",
                           f"{_CPU}::test_momentum_one_makes_the_ensemble_the_identity"],
}

ARGS = {
    "stil_roid_rows": ["Z", "ld", "rows", "K", "ema", "tau", "clip", "eps", "momentum", "grad_scale", "correct", "lse", "p", "ldp", "H", "cos",
                       "slr", "dn", "cn", "w", "keep", "pbar", "prior", "scores", "lds", "dZ", "ldd", "counts", "loss", "ws", "stream"],
    "stil_roid_ensemble": ["params", "theta0", "achunks", "n_achunks", "chunk2tensor", "active", "n_tensors", "n", "momentum", "stream"],
}
KINDS = {
    "stil_roid_rows": {"Z": ctypes.c_void_p, "ld": ctypes.c_int, "rows": ctypes.c_int, "K": ctypes.c_int, "ema": ctypes.c_void_p,
                       "tau": ctypes.c_float, "clip": ctypes.c_float, "eps": ctypes.c_float, "momentum": ctypes.c_float,
                       "grad_scale": ctypes.c_float, "correct": ctypes.c_int, "lse": ctypes.c_void_p, "ldp": ctypes.c_int,
                       "keep": ctypes.c_void_p, "lds": ctypes.c_int, "ldd": ctypes.c_int, "counts": ctypes.c_void_p, "ws": ctypes.c_void_p,
                       "stream": ctypes.c_void_p},
    "stil_roid_ensemble": {"params": ctypes.c_void_p, "theta0": ctypes.c_void_p, "n_achunks": ctypes.c_int, "n_tensors": ctypes.c_int,
                           "n": ctypes.c_long, "momentum": ctypes.c_float, "stream": ctypes.c_void_p},
}


def _protos():
    from stil_tta_amd._lib import ROID_HEADERS, parse_header
    (path,) = ROID_HEADERS
    assert os.path.basename(path) == "stil_roid.h" and os.path.exists(path)
    return parse_header(path)


def test_the_prototypes_of_the_header_are_the_ledgers_keys():
    assert set(_protos()) == set(LEDGER), (sorted(_protos()), sorted(LEDGER))


def test_the_prototypes_are_the_ones_the_binding_calls():
    protos = _protos()
    for name, (restype, args) in protos.items():
        assert restype is ctypes.c_int, name
        assert [n for _, n in args] == ARGS[name], name
        assert all(dict((n, t) for t, n in args)[n] is t for n, t in KINDS[name].items()), name
    # the slab arguments of the ensemble are stil_sar_restore's, in its order
    from stil_tta_amd._lib import TTA_HEADERS, parse_header
    sar = next(parse_header(p)["stil_sar_restore"] for p in TTA_HEADERS if os.path.basename(p) == "stil_sar.h")
    assert [n for _, n in sar[1]][2:8] == ARGS["stil_roid_ensemble"][2:8]


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
        assert hasattr(dll, name), f"{name} declared in csrc/stil_roid.h but not exported"
    assert set(_protos()) <= set(lib().protos)
    assert lib().version() == 106


def test_the_header_stays_out_of_include_and_collides_with_nothing():
    from stil_tta_amd._lib import CGPL_HEADERS, HEADER, MEMORY_HEADERS, READ_HEADERS, ROID_HEADERS, SHIFT_HEADERS, TTA_HEADERS, parse_header
    include = os.path.dirname(HEADER)
    assert all(os.path.dirname(p) != include for p in ROID_HEADERS)
    assert sorted(os.listdir(include)) == sorted(os.path.basename(p) for p in (HEADER,) + tuple(TTA_HEADERS))
    others = tuple(TTA_HEADERS) + tuple(MEMORY_HEADERS) + tuple(READ_HEADERS) + tuple(CGPL_HEADERS) + tuple(SHIFT_HEADERS)
    assert not set(ROID_HEADERS) & set(others) and len(ROID_HEADERS) == 1
    mine = set(_protos())
    for path in (HEADER,) + others:
        assert not mine & set(parse_header(path)), path
