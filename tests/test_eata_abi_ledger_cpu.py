"""Ledger of include/stil_eata.h, the EATA test-time adaptation C ABI: every prototype names the tests that check it directly,
the library exports it, and neither include/stil_hip.h's set (tests/test_abi_ledger_cpu.py) nor include/stil_tta.h's
(tests/test_tta_abi_ledger_cpu.py) lists it."""
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

_EATA = "test_gpu_eata.py"
LEDGER = {
    "stil_eata_rows": [f"{_EATA}::test_eata_rows_against_float64", f"{_EATA}::test_eata_rows_rejects_bad_arguments"],
    "stil_eata_anchor": [f"{_EATA}::test_slab_kernels_against_float64"],
    "stil_eata_fisher_accum": [f"{_EATA}::test_slab_kernels_against_float64"],
}


def _eata_protos():
    from stil_tta_amd._lib import EATA_HEADER, parse_header
    return parse_header(EATA_HEADER)


def test_every_eata_entry_point_names_a_direct_test_that_exists():
    protos = _eata_protos()
    assert set(protos) == set(LEDGER), (sorted(protos), sorted(LEDGER))
    for name, refs in LEDGER.items():
        assert refs, name
        for ref in refs:
            fname, func = ref.split("::")
            assert func in _test_functions(fname), f"{name}: {ref} does not exist"


def test_library_exports_every_eata_prototype():
    import __graft_entry__ as G
    G.build()
    from stil_tta_amd._lib import LIB_PATH, lib
    dll = ctypes.CDLL(LIB_PATH)
    for name in _eata_protos():
        assert hasattr(dll, name), f"{name} declared in include/stil_eata.h but not exported"
    assert set(_eata_protos()) <= set(lib().protos)   # bound by _lib next to the other two headers
    assert lib().version() == 106


def test_the_other_two_headers_do_not_list_them():
    from stil_tta_amd._lib import TTA_HEADER, parse_header
    assert not set(parse_header()) & set(_eata_protos())
    assert not set(parse_header(TTA_HEADER)) & set(_eata_protos())
