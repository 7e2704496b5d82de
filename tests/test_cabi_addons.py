"""The ONE ledger of ``_lib.ADDON_HEADERS``, the open third table of the C ABI, parametrized over its keys: what tests/test_cabi.py
asserts for a header of ``_lib.HEADERS``, asserted for every add-on header.  What is pinned per key lives in
tests/cabi_addon_<key>.py -- ``NAMES`` (sorted), ``EXEMPT`` (the only admissible reason: "writes no device memory"), ``BOUNDS`` (the
module with the guard-band cases) and ``PINNED`` (hand-written signatures) -- so a later header adds a key to the table and files
here, and changes none.  No GPU."""
import importlib

import pytest

from egopack_amd import _lib
from tests import cabi_common as CC

KEYS = list(_lib.ADDON_HEADERS)


def pins(key):
    return importlib.import_module(f"tests.cabi_addon_{key}")


def bounds(key):
    return importlib.import_module(pins(key).BOUNDS)


def test_the_third_table_is_open_and_the_first_two_are_as_they_were():
    assert "calibrate" in KEYS and all(_lib.ADDON_HEADERS[k].name == f"egopack_{k}.h" for k in KEYS)
    assert list(_lib.HEADERS) == list(CC.NAMES) and list(_lib.EXTRA_HEADERS) == ["lamb"]
    assert not set(KEYS) & (set(_lib.HEADERS) | set(_lib.EXTRA_HEADERS))
    assert list(_lib.signatures()) == list(_lib.HEADERS) and list(_lib.addon_signatures()) == KEYS
    for key in KEYS:  # every key has its pin file, in full
        P = pins(key)
        assert P.NAMES == sorted(P.NAMES) and isinstance(P.EXEMPT, dict) and isinstance(P.BOUNDS, str) and P.PINNED


@pytest.mark.parametrize("key", KEYS)
def test_every_header_symbol_is_exported_and_bound(key):
    """The names of a header are the pinned ones, each is exported and bound with the types its prototype declares, a C user gets
    them from the one file, and the header declares no struct (STRUCTS stays the set the first ledger pins)."""
    lib, header, sigs = _lib.load(), _lib.ADDON_HEADERS[key].name, _lib.addon_signatures()[key]
    assert sorted(sigs) == pins(key).NAMES, sorted(set(sigs) ^ set(pins(key).NAMES))
    for name in sigs:
        assert hasattr(lib, name), f"{name} declared in include/{header} but not exported"
        fn, (restype, argtypes) = getattr(lib, name), sigs[name]
        assert fn.restype == restype and list(fn.argtypes) == argtypes, name
    assert f'#include "{header}"' in _lib.HEADERS["hip"].read_text()
    assert "typedef struct" not in _lib.strip_c(_lib.ADDON_HEADERS[key].read_text())


@pytest.mark.parametrize("key", KEYS)
def test_no_entry_point_is_declared_by_another_header(key):
    mine = set(_lib.addon_signatures()[key])
    ledgered = {name for names in CC.NAMES.values() for name in names}
    assert not mine & ledgered and not mine & set(_lib.declared())
    for other, table in _lib.extra_signatures().items():
        assert not mine & set(table), other
    for other, table in _lib.addon_signatures().items():
        assert other == key or not mine & set(table), other


@pytest.mark.parametrize("where, text, needle", [
    ("a header of HEADERS", "int egk_version(void);\n", "egk_version is declared in egopack_twice.h and again under the key 'hip'"),
    ("a header of EXTRA_HEADERS", "int egk_lamb_tune(int32_t key, int32_t value);\n",
     "egk_lamb_tune is declared in egopack_twice.h and again under the key 'lamb'"),
    ("another add-on", "int egk_temp_newton(egk_stream_t s);\n", "egk_temp_newton is declared in egopack_twice.h and again under the key 'calibrate'"),
])
def test_a_name_another_table_declares_is_refused(tmp_path, monkeypatch, where, text, needle):
    twice = tmp_path / "egopack_twice.h"
    twice.write_text(text)
    monkeypatch.setattr(_lib, "ADDON_HEADERS", {**_lib.ADDON_HEADERS, "twice": twice})
    _lib.addon_signatures.cache_clear()
    try:
        with pytest.raises(RuntimeError) as e:
            _lib.addon_signatures()
        assert needle in str(e.value), (where, str(e.value))
        monkeypatch.setattr(_lib, "ADDON_HEADERS", {"absent": tmp_path / "egopack_absent.h"})
        _lib.addon_signatures.cache_clear()
        with pytest.raises(RuntimeError, match="egopack_absent.h is missing.*'absent'"):
            _lib.addon_signatures()
    finally:
        monkeypatch.undo()
        _lib.addon_signatures.cache_clear()
    assert list(_lib.addon_signatures()) == KEYS


@pytest.mark.parametrize("key", KEYS)
def test_the_hand_pinned_signatures_are_what_the_parser_reads(key):
    for name, (text, want) in pins(key).PINNED.items():
        assert _lib.parse_prototypes(text) == {name: want}, name
        assert _lib.addon_signatures()[key][name] == want, name


@pytest.mark.parametrize("key", KEYS)
def test_every_entry_point_has_a_bounds_case_or_writes_no_device_memory(key):
    """A kernel added to a header later fails here until it gets a case in the header's bounds module."""
    B, exempt, declared = bounds(key), pins(key).EXEMPT, set(_lib.addon_signatures()[key])  # (importable without a GPU)
    covered = set(B.covered())
    assert covered <= declared, f"cases name entry points the header does not declare: {sorted(covered - declared)}"
    assert set(exempt) <= declared, f"exemptions of entry points the header does not declare: {sorted(set(exempt) - declared)}"
    assert not covered & set(exempt), f"in exactly one of the two places: {sorted(covered & set(exempt))}"
    missing = declared - covered - set(exempt)
    assert not missing, f"entry points with neither a bounds case nor an exemption: {sorted(missing)}"
    assert all("writes no device memory" in why for why in exempt.values())
    for name, fn, variant, covers, plain in B.CASES:
        assert covers and all(c.startswith("egk_") for c in covers), name
    assert len({c[0] for c in B.CASES}) == len(B.CASES), "case ids must be unique"
    others = [CC.bounds(k) for k in _lib.HEADERS] + [bounds(k) for k in KEYS if k != key]
    for other in others:  # the cases live in their own list, and no entry point is covered from two modules
        assert B.CASES is not other.CASES and not covered & set(other.covered()), other.__name__
