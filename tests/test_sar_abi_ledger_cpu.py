"""Ledger of include/stil_sar.h, the C ABI of SAR's row loss, ascent step, restore and model recovery: every prototype names the
tests that check it directly, the library exports it, and none of include/stil_hip.h (tests/test_abi_ledger_cpu.py),
include/stil_tta.h (tests/test_tta_abi_ledger_cpu.py), include/stil_eata.h (tests/test_eata_abi_ledger_cpu.py),
include/stil_bnprior.h (tests/test_bnprior_abi_ledger_cpu.py), include/stil_infomax.h (tests/test_shot_abi_ledger_cpu.py),
include/stil_margent.h (tests/test_margent_abi_ledger_cpu.py) and include/stil_deyo.h (tests/test_deyo_abi_ledger_cpu.py) lists it."""
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

_G = "test_gpu_sar.py"
LEDGER = {
    "stil_sar_rows": [f"{_G}::test_sar_rows_against_float64", f"{_G}::test_sar_rows_that_select_every_row_give_the_gradient_of_entropy_rows",
                      f"{_G}::test_sar_rows_rejects_bad_arguments"],
    "stil_sar_perturb": [f"{_G}::test_perturb_and_restore_against_float64", f"{_G}::test_slab_kernels_reject_bad_arguments"],
    "stil_sar_restore": [f"{_G}::test_perturb_and_restore_against_float64", f"{_G}::test_slab_kernels_reject_bad_arguments"],
    "stil_sar_recover": [f"{_G}::test_recover_writes_exactly_a_when_flagged_and_nothing_otherwise", f"{_G}::test_slab_kernels_reject_bad_arguments"],
}


def _protos():
    from stil_tta_amd._lib import SAR_HEADER, parse_header
    return parse_header(SAR_HEADER)


def test_every_sar_entry_point_names_a_direct_test_that_exists():
    protos = _protos()
    assert set(protos) == set(LEDGER), (sorted(protos), sorted(LEDGER))
    for name, refs in LEDGER.items():
        assert refs, name
        for ref in refs:
            fname, func = ref.split("::")
            assert func in _test_functions(fname), f"{name}: {ref} does not exist"


def test_library_exports_every_sar_prototype():
    import __graft_entry__ as G
    G.build()
    from stil_tta_amd._lib import LIB_PATH, lib
    dll = ctypes.CDLL(LIB_PATH)
    for name in _protos():
        assert hasattr(dll, name), f"{name} declared in include/stil_sar.h but not exported"
    assert set(_protos()) <= set(lib().protos)   # bound by _lib next to the other seven headers
    assert lib().version() == 106


def test_the_other_seven_headers_do_not_list_them():
    from stil_tta_amd._lib import BNPRIOR_HEADER, DEYO_HEADER, EATA_HEADER, INFOMAX_HEADER, MARGENT_HEADER, TTA_HEADER, parse_header
    for other in (None, TTA_HEADER, EATA_HEADER, BNPRIOR_HEADER, INFOMAX_HEADER, MARGENT_HEADER, DEYO_HEADER):
        assert not set(parse_header(*([other] if other else []))) & set(_protos())
