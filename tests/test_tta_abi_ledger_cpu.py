"""Ledgers of the test-time adaptation C ABI, one per header of stil_tta_amd._lib.TTA_HEADERS: every prototype names the tests
that check it directly, the library exports it and _lib binds it; TTA_HEADERS is exactly what include/ holds beside stil_hip.h
(whose own ledger is tests/test_abi_ledger_cpu.py), and no two of the eight headers declare the same name."""
import ctypes
import itertools
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

from test_abi_ledger_cpu import _test_functions  # noqa: E402

_TTA, _EATA, _SHOT, _MARGENT, _DEYO, _SAR = (f"test_gpu_{n}.py" for n in ("tta", "eata", "shot", "margent", "deyo", "sar"))
_BN_F64 = "test_gpu_bnprior.py::test_entry_points_against_float64"
_BN_RHO1 = "test_gpu_bnprior.py::test_rho_one_is_the_existing_entry_points_bit_for_bit"
_BN_BAD = "test_gpu_bnprior.py::test_bad_arguments_are_refused"
LEDGERS = {
    "stil_tta.h": {
        "stil_entropy_rows": [f"{_TTA}::test_entropy_rows_against_float64", f"{_TTA}::test_entropy_rows_rejects_bad_arguments"],
    },
    "stil_eata.h": {
        "stil_eata_rows": [f"{_EATA}::test_eata_rows_against_float64", f"{_EATA}::test_eata_rows_rejects_bad_arguments"],
        "stil_eata_anchor": [f"{_EATA}::test_slab_kernels_against_float64"],
        "stil_eata_fisher_accum": [f"{_EATA}::test_slab_kernels_against_float64"],
    },
    "stil_bnprior.h": {
        "stil_bn_prior_fwd": [_BN_F64, _BN_RHO1, _BN_BAD],
        "stil_bn_prior_fwd_tiles": [_BN_F64, _BN_RHO1, _BN_BAD],
        "stil_bn_prior_bwd": [_BN_F64, _BN_RHO1, _BN_BAD, "test_gpu_bnprior.py::test_scalar_backward_final_against_float64"],
        "stil_bn_prior_bwd_tiles": [_BN_F64, _BN_RHO1, _BN_BAD],
    },
    "stil_infomax.h": {
        "stil_infomax_rows": [f"{_SHOT}::test_infomax_rows_against_float64", f"{_SHOT}::test_zero_weight_is_entropy_rows_bit_for_bit",
                              f"{_SHOT}::test_infomax_rows_rejects_bad_arguments"],
    },
    "stil_margent.h": {
        "stil_marginal_entropy_groups": [f"{_MARGENT}::test_marginal_entropy_groups_against_float64",
                                         f"{_MARGENT}::test_marginal_entropy_groups_rejects_bad_arguments"],
    },
    "stil_deyo.h": {
        "stil_patch_shuffle": [f"{_DEYO}::test_patch_shuffle_is_the_gather_bit_for_bit",
                               f"{_DEYO}::test_patch_shuffle_takes_the_scalar_path_on_a_misaligned_view",
                               f"{_DEYO}::test_patch_shuffle_rejects_bad_arguments"],
        "stil_deyo_rows": [f"{_DEYO}::test_deyo_rows_against_float64", f"{_DEYO}::test_entropy_only_deyo_rows_is_eata_rows_bit_for_bit",
                           f"{_DEYO}::test_deyo_rows_rejects_bad_arguments"],
    },
    "stil_sar.h": {
        "stil_sar_rows": [f"{_SAR}::test_sar_rows_against_float64",
                          f"{_SAR}::test_sar_rows_that_select_every_row_give_the_gradient_of_entropy_rows",
                          f"{_SAR}::test_sar_rows_rejects_bad_arguments"],
        "stil_sar_perturb": [f"{_SAR}::test_perturb_and_restore_against_float64", f"{_SAR}::test_slab_kernels_reject_bad_arguments"],
        "stil_sar_restore": [f"{_SAR}::test_perturb_and_restore_against_float64", f"{_SAR}::test_slab_kernels_reject_bad_arguments"],
        "stil_sar_recover": [f"{_SAR}::test_recover_writes_exactly_a_when_flagged_and_nothing_otherwise",
                             f"{_SAR}::test_slab_kernels_reject_bad_arguments"],
    },
}
per_header = pytest.mark.parametrize("header", sorted(LEDGERS))


def _protos(header=None):
    """the prototypes of include/<header>; None: of include/stil_hip.h"""
    from stil_tta_amd._lib import TTA_HEADERS, parse_header
    if header is None:
        return parse_header()
    (path,) = [p for p in TTA_HEADERS if os.path.basename(p) == header]
    return parse_header(path)


@per_header
def test_the_prototypes_of_a_header_are_its_ledgers_keys(header):
    assert set(_protos(header)) == set(LEDGERS[header]), (sorted(_protos(header)), sorted(LEDGERS[header]))


@per_header
def test_every_entry_point_names_a_direct_test_that_exists(header):
    for name, refs in LEDGERS[header].items():
        assert refs, name
        for ref in refs:
            fname, func = ref.split("::")
            assert func in _test_functions(fname), f"{name}: {ref} does not exist"


@per_header
def test_library_exports_and_binds_every_prototype(header):
    import __graft_entry__ as G
    G.build()
    from stil_tta_amd._lib import LIB_PATH, lib
    dll = ctypes.CDLL(LIB_PATH)
    for name in _protos(header):
        assert hasattr(dll, name), f"{name} declared in include/{header} but not exported"
    assert set(_protos(header)) <= set(lib().protos)   # bound by _lib next to stil_hip.h's entry points


def test_library_version():
    import __graft_entry__ as G
    G.build()
    from stil_tta_amd._lib import lib
    assert lib().version() == 106


def test_every_tta_prototype_cites_tent_and_the_reference_hook():
    from stil_tta_amd._lib import TTA_HEADERS
    (path,) = [p for p in TTA_HEADERS if os.path.basename(p) == "stil_tta.h"]
    src = open(path).read()
    assert "Wang et al., ICLR 2021" in src and "STiLModel.py:523-524" in src


def test_tta_headers_are_what_include_holds_beside_stil_hip_h():
    from stil_tta_amd._lib import HEADER, TTA_HEADERS
    include = os.path.dirname(HEADER)
    assert all(os.path.dirname(p) == include and os.path.exists(p) for p in TTA_HEADERS)
    names = [os.path.basename(p) for p in TTA_HEADERS]
    assert sorted(names) == sorted(set(os.listdir(include)) - {"stil_hip.h"}) == sorted(LEDGERS)


def test_no_two_of_the_eight_headers_declare_the_same_name():
    sets = {h: set(_protos(h)) for h in [None] + sorted(LEDGERS)}
    assert len(sets) == 8 and all(sets.values())
    for a, b in itertools.combinations(sets, 2):
        assert not sets[a] & sets[b], (a, b, sorted(sets[a] & sets[b]))
