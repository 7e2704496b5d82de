"""The ledger of include/egopack_lamb.h, in the form tests/test_cabi.py holds the headers of ``_lib.HEADERS`` to: the header is bound
from a second table (``_lib.EXTRA_HEADERS``) because the first ledger pins the keys of ``HEADERS``; its names are pinned and sorted,
each is exported and bound with the parsed types, none is declared by a ledgered header, one signature is pinned by hand, and every
entry point has a guard-band case in tests/test_gpu_bounds_lamb.py or the reason "writes no device memory".  No GPU."""
import ctypes

from egopack_amd import _lib
from tests import cabi_common as CC
from tests import test_gpu_bounds_lamb as BL

NAMES = ["egk_lamb_apply", "egk_lamb_moments", "egk_lamb_trust", "egk_lamb_tune"]
EXEMPT = {"egk_lamb_tune": "knob: writes no device memory"}
vp, i32, i64, f32, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_double


def test_the_second_table_holds_the_header_and_the_first_is_as_it_was():
    assert list(_lib.EXTRA_HEADERS) == ["lamb"] and _lib.EXTRA_HEADERS["lamb"].name == "egopack_lamb.h"
    assert "lamb" not in _lib.HEADERS and list(_lib.HEADERS) == list(CC.NAMES)
    assert list(_lib.signatures()) == list(_lib.HEADERS) and not set(NAMES) & set(_lib.declared())
    assert f'#include "{_lib.EXTRA_HEADERS["lamb"].name}"' in _lib.HEADERS["hip"].read_text()  # (a C user includes one file)
    assert "typedef struct" not in _lib.strip_c(_lib.EXTRA_HEADERS["lamb"].read_text())  # (scalars and pointers only: STRUCTS as ledgered)


def test_every_symbol_of_the_header_is_exported_and_bound():
    lib, sigs = _lib.load(), _lib.extra_signatures()["lamb"]
    assert sorted(sigs) == NAMES == sorted(NAMES)
    for name in NAMES:
        assert hasattr(lib, name), f"{name} declared in include/egopack_lamb.h but not exported"
        fn, (restype, argtypes) = getattr(lib, name), sigs[name]
        assert fn.restype == restype and list(fn.argtypes) == argtypes, name


def test_no_name_is_declared_by_a_ledgered_header():
    ledgered = {name for names in CC.NAMES.values() for name in names}
    assert not ledgered & set(NAMES)
    for key in _lib.HEADERS:
        assert not set(_lib.declared(key)) & set(NAMES), key


def test_a_name_of_a_ledgered_header_in_the_second_table_is_refused(tmp_path, monkeypatch):
    twice = tmp_path / "egopack_twice.h"
    twice.write_text("int egk_version(void);\n")
    monkeypatch.setattr(_lib, "EXTRA_HEADERS", {"twice": twice})
    _lib.extra_signatures.cache_clear()
    try:
        try:
            _lib.extra_signatures()
            raise AssertionError("a name declared twice was bound")
        except RuntimeError as e:
            assert "egk_version is declared in egopack_twice.h and again under the key 'hip'" in str(e)
    finally:
        monkeypatch.undo()
        _lib.extra_signatures.cache_clear()
    assert sorted(_lib.extra_signatures()["lamb"]) == NAMES


def test_the_hand_pinned_signature_is_what_the_parser_reads():
    want = (ctypes.c_int, [vp, vp, vp, vp, i32, vp, i32, i32, i32, vp, vp, vp])
    text = """int egk_lamb_trust(egk_stream_t s, const double* part, const int32_t* slot_piece0, const int32_t* slot_group, int32_t n_slots,
                   const float* group_hyper, int32_t n_groups, int32_t trust_clip, int32_t always_adapt, float* trust, double* norms,
                   const int32_t* gate);"""
    assert _lib.parse_prototypes(text) == {"egk_lamb_trust": want}
    assert _lib.extra_signatures()["lamb"]["egk_lamb_trust"] == want
    assert _lib.extra_signatures()["lamb"]["egk_lamb_tune"] == (ctypes.c_int, [i32, i32])
    mom = _lib.extra_signatures()["lamb"]["egk_lamb_moments"]
    assert mom == (ctypes.c_int, [vp, vp, vp, i32, vp, vp, i64, i64, i32, i32, i32, vp, vp, vp, i32, vp, i32, vp, f64, f64, f32, vp, vp, vp, i64])


def test_every_entry_point_has_a_bounds_case_or_writes_no_device_memory():
    covered = set(BL.covered())
    assert covered <= set(NAMES) and set(EXEMPT) <= set(NAMES) and not covered & set(EXEMPT)
    assert covered | set(EXEMPT) == set(NAMES), sorted(set(NAMES) - covered - set(EXEMPT))
    assert all("writes no device memory" in why for why in EXEMPT.values())
    assert len({c[0] for c in BL.CASES}) == len(BL.CASES), "case ids must be unique"
    for name, fn, variant, covers, plain in BL.CASES:
        assert covers and all(c.startswith("egk_lamb_") for c in covers), name
    for key in _lib.HEADERS:  # no entry point is covered from two modules
        assert BL.CASES is not CC.bounds(key).CASES and not covered & set(CC.bounds(key).covered()), key
