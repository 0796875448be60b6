"""Ledger of csrc/stil_shift.h (stil_tta_amd._lib.SHIFT_HEADERS), in the style of tests/test_cgpl_abi_ledger_cpu.py: every prototype
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

_GPU, _CPU = "test_gpu_shift.py", "test_shift_cpu.py"
_REFUSALS = [f"{_GPU}::test_refusals_leave_out_untouched", f"{_CPU}::test_c_abi_rejects_bad_arguments_without_a_gpu"]
_YARDSTICK = f"{_CPU}::test_float32_numpy_stays_within_a_quarter_of_tol_of_the_float64_model"
LEDGER = {
    "stil_shift_noise": [f"{_GPU}::test_noise_against_the_model", f"{_GPU}::test_one_call_on_three_samples_is_a_call_on_one_then_on_two",
                         f"{_GPU}::test_noise_of_strength_zero_without_clipping_is_a_copy", f"{_CPU}::test_model_moments_over_2_to_the_20_draws",
                         _YARDSTICK] + _REFUSALS,
    "stil_shift_contrast": [f"{_GPU}::test_contrast_against_float64", _YARDSTICK] + _REFUSALS,
    "stil_shift_brightness": [f"{_GPU}::test_brightness_against_float64_at_its_edges", _YARDSTICK] + _REFUSALS,
    "stil_shift_pixelate": [f"{_GPU}::test_pixelate_against_float64", _YARDSTICK] + _REFUSALS,
    "stil_shift_tab": [f"{_GPU}::test_tabular_shifts_against_the_model", f"{_GPU}::test_a_table_of_257_rows_is_one_row_then_256",
                       f"{_CPU}::test_model_moments_over_2_to_the_20_draws", _YARDSTICK] + _REFUSALS,
}


def _protos():
    from stil_tta_amd._lib import SHIFT_HEADERS, parse_header
    (path,) = SHIFT_HEADERS
    assert os.path.basename(path) == "stil_shift.h" and os.path.exists(path)
    return parse_header(path)


def test_the_prototypes_of_the_header_are_the_ledgers_keys():
    assert set(_protos()) == set(LEDGER), (sorted(_protos()), sorted(LEDGER))


def test_the_prototypes_are_the_ones_the_binding_calls():
    names = {name: [n for _, n in args] for name, (_, args) in _protos().items()}
    assert all(restype is ctypes.c_int for restype, _ in _protos().values())
    assert all(n[-1] == "stream" and n[:2] == ["x", "out"] for n in names.values())
    assert names["stil_shift_noise"] == ["x", "out", "n", "kind", "strength", "lo", "hi", "seed", "offset", "stream"]
    assert names["stil_shift_contrast"] == ["x", "out", "B", "C", "HW", "factor", "lo", "hi", "mean_ws", "stream"]
    assert names["stil_shift_brightness"] == ["x", "out", "B", "C", "HW", "delta", "lo", "hi", "stream"]
    assert names["stil_shift_pixelate"] == ["x", "out", "B", "C", "H", "W", "s", "stream"]
    assert names["stil_shift_tab"] == ["x", "out", "B", "n_cols", "num_cat", "cat_len", "col_on", "col_std", "col_fill", "kind", "strength", "seed",
                                       "offset", "stream"]
    kinds = dict((n, t) for t, n in _protos()["stil_shift_noise"][1])
    assert kinds["n"] is ctypes.c_long and kinds["strength"] is ctypes.c_float and kinds["seed"] is ctypes.c_ulonglong
    assert kinds["offset"] is ctypes.c_ulonglong and kinds["x"] is ctypes.c_void_p and kinds["kind"] is ctypes.c_int
    kinds = dict((n, t) for t, n in _protos()["stil_shift_tab"][1])
    assert kinds["cat_len"] is ctypes.c_void_p and kinds["offset"] is ctypes.c_ulonglong and kinds["num_cat"] is ctypes.c_int


def test_every_entry_point_names_direct_tests_that_exist():
    for name, refs in LEDGER.items():
        assert refs, name
        assert any(r.startswith(_GPU) for r in refs) and any(r.startswith(_CPU) for r in refs), name
        for ref in refs:
            fname, func = ref.split("::")
            assert func in _test_functions(fname), f"{name}: {ref} does not exist"


def test_library_exports_and_binds_every_prototype_at_version_106():
    import __graft_entry__ as G
    G.build()
    from stil_tta_amd._lib import LIB_PATH, lib
    dll = ctypes.CDLL(LIB_PATH)
    for name in _protos():
        assert hasattr(dll, name), f"{name} declared in csrc/stil_shift.h but not exported"
    assert set(_protos()) <= set(lib().protos)
    assert lib().version() == 106


def test_the_header_stays_out_of_include_and_collides_with_nothing():
    from stil_tta_amd._lib import CGPL_HEADERS, HEADER, MEMORY_HEADERS, READ_HEADERS, SHIFT_HEADERS, TTA_HEADERS, parse_header
    include = os.path.dirname(HEADER)
    assert all(os.path.dirname(p) != include for p in SHIFT_HEADERS)
    assert not os.path.exists(os.path.join(include, "stil_shift.h"))
    others = tuple(TTA_HEADERS) + tuple(MEMORY_HEADERS) + tuple(READ_HEADERS) + tuple(CGPL_HEADERS)
    assert not set(SHIFT_HEADERS) & set(others) and len(SHIFT_HEADERS) == 1
    mine = set(_protos())
    for path in (HEADER,) + others:
        assert not mine & set(parse_header(path)), path
