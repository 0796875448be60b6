"""Ledger of csrc/stil_rotta.h (stil_tta_amd._lib.ROTTA_HEADERS), in the style of tests/test_roid_abi_ledger_cpu.py: every prototype
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

_GPU, _CPU = "test_gpu_rotta.py", "test_rotta_cpu.py"
_REFUSE = f"{_GPU}::test_entry_points_reject_bad_arguments_with_nothing_written"
LEDGER = {
    "stil_rotta_bank_update": [f"{_GPU}::test_bank_update_against_the_restatement", f"{_GPU}::test_one_call_equals_one_call_per_sample",
                               f"{_GPU}::test_a_one_class_stream_is_held_to_its_share", _REFUSE,
                               f"{_CPU}::test_the_banks_decisions_are_well_conditioned"],
    "stil_rotta_bank_store": [f"{_GPU}::test_bank_store_is_a_bit_exact_gather", _REFUSE],
    "stil_rotta_rows": [f"{_GPU}::test_rotta_rows_against_float64", f"{_GPU}::test_rotta_rows_on_an_empty_bank", _REFUSE,
                        f"{_CPU}::test_fp32_aten_meets_the_loss_kernels_bars"],
    "stil_rotta_exchange": [f"{_GPU}::test_exchange_and_teacher_against_float64", _REFUSE],
    "stil_rotta_teacher": [f"{_GPU}::test_exchange_and_teacher_against_float64", _REFUSE,
                           f"{_CPU}::test_an_empty_bank_has_no_loss_and_the_teacher_average_has_its_ends"],
}

_SLAB = ["achunks", "n_achunks", "chunk2tensor", "active", "n_tensors", "n"]
ARGS = {
    "stil_rotta_bank_update": ["Zt", "ld", "B", "K", "N", "lambda_t", "lambda_u", "label", "unc", "age", "occ", "n", "owner", "lse", "p", "ldp",
                               "H", "yhat", "accepted", "slot_of", "counts", "stream"],
    "stil_rotta_bank_store": ["x_img", "x_tab", "owner", "N", "B", "img_floats", "tab_floats", "bank_img", "bank_tab", "stream"],
    "stil_rotta_rows": ["Zs", "lds", "Zt", "ldt", "label", "age", "rows", "K", "grad_scale", "ce", "w", "dZ", "ldd", "counts", "loss", "active",
                        "active_out", "n_tensors", "ws", "stream"],
    "stil_rotta_exchange": ["params", "teacher"] + _SLAB + ["stream"],
    "stil_rotta_teacher": ["params", "teacher"] + _SLAB + ["nu", "stream"],
}
_I, _F, _P = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
KINDS = {
    "stil_rotta_bank_update": {"Zt": _P, "ld": _I, "B": _I, "K": _I, "N": _I, "lambda_t": _F, "lambda_u": _F, "n": _P, "ldp": _I, "accepted": _P,
                               "counts": _P, "stream": _P},
    "stil_rotta_bank_store": {"owner": _P, "N": _I, "B": _I, "img_floats": ctypes.c_long, "tab_floats": _I, "stream": _P},
    "stil_rotta_rows": {"lds": _I, "ldt": _I, "rows": _I, "K": _I, "grad_scale": _F, "ldd": _I, "active": _P, "n_tensors": _I, "ws": _P, "stream": _P},
    "stil_rotta_exchange": {"params": _P, "teacher": _P, "n_achunks": _I, "n_tensors": _I, "n": ctypes.c_long, "stream": _P},
    "stil_rotta_teacher": {"params": _P, "teacher": _P, "n_achunks": _I, "n_tensors": _I, "n": ctypes.c_long, "nu": _F, "stream": _P},
}


def _protos():
    from stil_tta_amd._lib import ROTTA_HEADERS, parse_header
    (path,) = ROTTA_HEADERS
    assert os.path.basename(path) == "stil_rotta.h" and os.path.exists(path)
    return parse_header(path)


def test_the_prototypes_of_the_header_are_the_ledgers_keys():
    assert set(_protos()) == set(LEDGER), (sorted(_protos()), sorted(LEDGER))


def test_the_prototypes_are_the_ones_the_binding_calls():
    protos = _protos()
    for name, (restype, args) in protos.items():
        assert restype is ctypes.c_int, name
        assert [n for _, n in args] == ARGS[name], name
        assert all(dict((n, t) for t, n in args)[n] is t for n, t in KINDS[name].items()), name
        assert args[-1] == (ctypes.c_void_p, "stream"), f"{name}: the stream comes last"
    # the slab arguments of the teacher's two entry points are stil_sar_restore's, in its order
    from stil_tta_amd._lib import TTA_HEADERS, parse_header
    sar = next(parse_header(p)["stil_sar_restore"] for p in TTA_HEADERS if os.path.basename(p) == "stil_sar.h")
    for name in ("stil_rotta_exchange", "stil_rotta_teacher"):
        assert [n for _, n in sar[1]][2:8] == ARGS[name][2:8] == _SLAB


def test_the_bounds_of_the_header_are_the_ones_the_host_checks():
    import re
    from stil_tta_amd import tta
    from stil_tta_amd._lib import ROTTA_HEADERS
    src = open(ROTTA_HEADERS[0]).read()
    assert int(re.search(r"#define STIL_ROTTA_MAX_SLOTS (\d+)", src).group(1)) == tta.ROTTA_MAX_SLOTS
    assert int(re.search(r"#define STIL_ROTTA_MAX_CLASSES (\d+)", src).group(1)) >= 1000


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
        assert hasattr(dll, name), f"{name} declared in csrc/stil_rotta.h but not exported"
    assert set(_protos()) <= set(lib().protos)
    assert lib().version() == 106


def test_the_header_stays_out_of_include_and_collides_with_nothing():
    from stil_tta_amd._lib import (CGPL_HEADERS, HEADER, MEMORY_HEADERS, READ_HEADERS, ROID_HEADERS, ROTTA_HEADERS, SHIFT_HEADERS, TTA_HEADERS,
                                   parse_header)
    include = os.path.dirname(HEADER)
    assert all(os.path.dirname(p) != include for p in ROTTA_HEADERS)
    assert sorted(os.listdir(include)) == sorted(os.path.basename(p) for p in (HEADER,) + tuple(TTA_HEADERS))
    others = tuple(TTA_HEADERS) + tuple(MEMORY_HEADERS) + tuple(READ_HEADERS) + tuple(CGPL_HEADERS) + tuple(SHIFT_HEADERS) + tuple(ROID_HEADERS)
    assert not set(ROTTA_HEADERS) & set(others) and len(ROTTA_HEADERS) == 1
    mine = set(_protos())
    for path in (HEADER,) + others:
        assert not mine & set(parse_header(path)), path
