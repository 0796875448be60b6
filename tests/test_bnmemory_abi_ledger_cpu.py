"""Ledger of csrc/stil_bnmemory.h (stil_tta_amd._lib.MEMORY_HEADERS), in the style of tests/test_tta_abi_ledger_cpu.py: every
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

_GPU, _CPU = "test_gpu_bnmemory.py", "test_bnmemory_cpu.py"
_DIRECT = [f"{_GPU}::test_entry_points_against_float64", f"{_GPU}::test_null_outputs_are_the_prior_entry_points_bit_for_bit",
           f"{_GPU}::test_rho_one_is_the_training_entry_points_bit_for_bit_and_still_updates",
           f"{_GPU}::test_bad_arguments_are_refused_with_nothing_written",
           f"{_CPU}::test_the_c_abi_refuses_bad_memory_arguments_before_any_launch"]
LEDGER = {"stil_bn_memory_fwd": _DIRECT, "stil_bn_memory_fwd_tiles": _DIRECT}


def _protos():
    from stil_tta_amd._lib import MEMORY_HEADERS, parse_header
    (path,) = MEMORY_HEADERS
    assert os.path.basename(path) == "stil_bnmemory.h" and os.path.exists(path)
    return parse_header(path)


def test_the_prototypes_of_the_header_are_the_ledgers_keys():
    assert set(_protos()) == set(LEDGER), (sorted(_protos()), sorted(LEDGER))


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
        assert hasattr(dll, name), f"{name} declared in csrc/stil_bnmemory.h but not exported"
    assert set(_protos()) <= set(lib().protos)
    assert lib().version() == 106


def test_the_header_stays_out_of_include_and_collides_with_nothing():
    from stil_tta_amd._lib import HEADER, MEMORY_HEADERS, TTA_HEADERS, parse_header
    include = os.path.dirname(HEADER)
    assert all(os.path.dirname(p) != include for p in MEMORY_HEADERS) and not set(MEMORY_HEADERS) & set(TTA_HEADERS)
    mine = set(_protos())
    for path in (HEADER,) + tuple(TTA_HEADERS):
        assert not mine & set(parse_header(path)), path
