"""Ledger of include/stil_tta.h, the test-time adaptation C ABI: every prototype names the test that checks it directly,
the library exports it, and include/stil_hip.h's own set (parse_header() with no argument, tests/test_abi_ledger_cpu.py)
does not list it."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
TESTS = os.path.dirname(os.path.abspath(__file__))

from test_abi_ledger_cpu import _test_functions  # noqa: E402

_TTA = "test_gpu_tta.py"
LEDGER = {
    "stil_entropy_rows": [f"{_TTA}::test_entropy_rows_against_float64", f"{_TTA}::test_entropy_rows_rejects_bad_arguments"],
}


def _tta_protos():
    from stil_tta_amd._lib import TTA_HEADER, parse_header
    return parse_header(TTA_HEADER)


def test_every_tta_entry_point_names_a_direct_test_that_exists():
    protos = _tta_protos()
    assert set(protos) == set(LEDGER), (sorted(protos), sorted(LEDGER))
    for name, refs in LEDGER.items():
        assert refs, name
        for ref in refs:
            fname, func = ref.split("::")
            assert func in _test_functions(fname), f"{name}: {ref} does not exist"


def test_every_tta_prototype_cites_tent_and_the_reference_hook():
    from stil_tta_amd._lib import TTA_HEADER
    src = open(TTA_HEADER).read()
    assert "Wang et al., ICLR 2021" in src and "STiLModel.py:523-524" in src


def test_library_exports_every_tta_prototype():
    import __graft_entry__ as G
    G.build()
    from stil_tta_amd._lib import LIB_PATH, lib
    dll = ctypes.CDLL(LIB_PATH)
    for name in _tta_protos():
        assert hasattr(dll, name), f"{name} declared in include/stil_tta.h but not exported"
    assert set(_tta_protos()) <= set(lib().protos)   # bound by _lib next to stil_hip.h's entry points
    assert lib().version() == 106


def test_stil_hip_header_set_does_not_list_them():
    from stil_tta_amd._lib import parse_header
    assert not set(parse_header()) & set(_tta_protos())
