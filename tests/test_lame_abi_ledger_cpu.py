"""Ledger of csrc/stil_lame.h (stil_tta_amd._lib.LAME_HEADERS), in the style of tests/test_rotta_abi_ledger_cpu.py: every prototype
names the tests that check it directly, the library exports it and _lib binds it; the header lives beside its kernels, not in
include/ (whose file list is closed), its names collide with no other header's, and the library version stays 106."""
import ctypes
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

from test_abi_ledger_cpu import _test_functions  # noqa: E402

_GPU, _CPU = "test_gpu_lame.py", "test_lame_cpu.py"
_REFUSE = f"{_GPU}::test_entry_points_reject_bad_arguments_with_nothing_written"
LEDGER = {
    "stil_lame_affinity": [f"{_GPU}::test_affinity_against_the_restatement", _REFUSE, f"{_GPU}::test_the_property_on_the_device",
                           f"{_CPU}::test_no_neighbour_decision_hangs_on_a_small_gap"],
    "stil_lame_rows": [f"{_GPU}::test_rows_against_the_restatement", _REFUSE, f"{_GPU}::test_the_property_on_the_device",
                       f"{_CPU}::test_the_iteration_is_well_conditioned"],
}

ARGS = {
    "stil_lame_affinity": ["F", "ldf", "rows", "D", "k", "kind", "nbr", "wts", "dk", "ws", "stream"],
    "stil_lame_rows": ["Z", "ld", "rows", "K", "nbr", "wts", "k", "lambda", "max_steps", "tol", "lse", "p", "ldp", "Y", "ldy", "energy", "steps",
                       "ws", "stream"],
}
_I, _F, _P = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
KINDS = {
    "stil_lame_affinity": {"F": _P, "ldf": _I, "rows": _I, "D": _I, "k": _I, "kind": _I, "nbr": _P, "wts": _P, "dk": _P, "ws": _P, "stream": _P},
    "stil_lame_rows": {"Z": _P, "ld": _I, "rows": _I, "K": _I, "nbr": _P, "wts": _P, "k": _I, "lambda": _F, "max_steps": _I, "tol": _F, "lse": _P,
                       "p": _P, "ldp": _I, "Y": _P, "ldy": _I, "energy": _P, "steps": _P, "ws": _P, "stream": _P},
}


def _protos():
    from stil_tta_amd._lib import LAME_HEADERS, parse_header
    (path,) = LAME_HEADERS
    assert os.path.basename(path) == "stil_lame.h" and os.path.exists(path)
    return parse_header(path)


def test_the_prototypes_of_the_header_are_the_ledgers_keys():
    assert set(_protos()) == set(LEDGER), (sorted(_protos()), sorted(LEDGER))


def test_the_prototypes_are_the_ones_the_binding_calls():
    protos = _protos()
    for name, (restype, args) in protos.items():
        assert restype is ctypes.c_int, name
        assert [n for _, n in args] == ARGS[name], name
        assert set(KINDS[name]) == set(ARGS[name]), name
        assert all(dict((n, t) for t, n in args)[n] is t for n, t in KINDS[name].items()), name
        assert args[-1] == (ctypes.c_void_p, "stream"), f"{name}: the stream comes last"


def test_the_bounds_of_the_header_are_the_ones_the_host_checks():
    from stil_tta_amd import tta
    from stil_tta_amd._lib import LAME_HEADERS
    src = open(LAME_HEADERS[0]).read()
    assert int(re.search(r"#define STIL_LAME_MAX_ROWS (\d+)", src).group(1)) == tta.LAME_MAX_ROWS
    kinds = {n.lower(): int(v) for n, v in re.findall(r"#define STIL_LAME_(KNN|RBF) (\d+)", src)}
    assert kinds == {n: i for i, n in enumerate(tta.LAME_AFFINITIES)}, "the kind stil_lame_affinity takes is the index in LAME_AFFINITIES"
    assert "unpinned" in src   # the header says that the definition is recalled, not pinned


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
        assert hasattr(dll, name), f"{name} declared in csrc/stil_lame.h but not exported"
    assert set(_protos()) <= set(lib().protos)
    assert lib().version() == 106


def test_the_header_stays_out_of_include_and_collides_with_nothing():
    from stil_tta_amd._lib import (CGPL_HEADERS, HEADER, LAME_HEADERS, MEMORY_HEADERS, READ_HEADERS, ROID_HEADERS, ROTTA_HEADERS, SHIFT_HEADERS,
                                   TTA_HEADERS, parse_header)
    include = os.path.dirname(HEADER)
    assert all(os.path.dirname(p) != include for p in LAME_HEADERS)
    assert sorted(os.listdir(include)) == sorted(os.path.basename(p) for p in (HEADER,) + tuple(TTA_HEADERS))
    others = (tuple(TTA_HEADERS) + tuple(MEMORY_HEADERS) + tuple(READ_HEADERS) + tuple(CGPL_HEADERS) + tuple(SHIFT_HEADERS) + tuple(ROID_HEADERS)
              + tuple(ROTTA_HEADERS))
    assert not set(LAME_HEADERS) & set(others) and len(LAME_HEADERS) == 1
    mine = set(_protos())
    for path in (HEADER,) + others:
        assert not mine & set(parse_header(path)), path
