"""Ledger of include/stil_deyo.h, the C ABI of DeYO's patch shuffle and row loss: every prototype names the tests that check
it directly, the library exports it, and none of include/stil_hip.h (tests/test_abi_ledger_cpu.py), include/stil_tta.h
(tests/test_tta_abi_ledger_cpu.py), include/stil_eata.h (tests/test_eata_abi_ledger_cpu.py), include/stil_bnprior.h
(tests/test_bnprior_abi_ledger_cpu.py), include/stil_infomax.h (tests/test_shot_abi_ledger_cpu.py) and include/stil_margent.h
(tests/test_margent_abi_ledger_cpu.py) lists it."""
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

_G = "test_gpu_deyo.py"
LEDGER = {
    "stil_patch_shuffle": [f"{_G}::test_patch_shuffle_is_the_gather_bit_for_bit", f"{_G}::test_patch_shuffle_takes_the_scalar_path_on_a_misaligned_view",
                           f"{_G}::test_patch_shuffle_rejects_bad_arguments"],
    "stil_deyo_rows": [f"{_G}::test_deyo_rows_against_float64", f"{_G}::test_entropy_only_deyo_rows_is_eata_rows_bit_for_bit",
                       f"{_G}::test_deyo_rows_rejects_bad_arguments"],
}


def _protos():
    from stil_tta_amd._lib import DEYO_HEADER, parse_header
    return parse_header(DEYO_HEADER)


def test_every_deyo_entry_point_names_a_direct_test_that_exists():
    protos = _protos()
    assert set(protos) == set(LEDGER), (sorted(protos), sorted(LEDGER))
    for name, refs in LEDGER.items():
        assert refs, name
        for ref in refs:
            fname, func = ref.split("::")
            assert func in _test_functions(fname), f"{name}: {ref} does not exist"


def test_library_exports_every_deyo_prototype():
    import __graft_entry__ as G
    G.build()
    from stil_tta_amd._lib import LIB_PATH, lib
    dll = ctypes.CDLL(LIB_PATH)
    for name in _protos():
        assert hasattr(dll, name), f"{name} declared in include/stil_deyo.h but not exported"
    assert set(_protos()) <= set(lib().protos)   # bound by _lib next to the other six headers
    assert lib().version() == 106


def test_the_other_six_headers_do_not_list_them():
    from stil_tta_amd._lib import BNPRIOR_HEADER, EATA_HEADER, INFOMAX_HEADER, MARGENT_HEADER, TTA_HEADER, parse_header
    for other in (None, TTA_HEADER, EATA_HEADER, BNPRIOR_HEADER, INFOMAX_HEADER, MARGENT_HEADER):
        assert not set(parse_header(*([other] if other else []))) & set(_protos())
