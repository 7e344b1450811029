"""The tuning options (uvx_set_option / uvx_get_option): defaults, key range, the header's enum against its Python mirror, and the
set-and-restore helper _lib.option.  Host code only: the library is loaded without a device."""
import os
import re
import subprocess
import sys

import pytest

from ultravox_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# uvx_get_option(k), k = 1 .. 31, in a process that has set nothing (recorded before the keys had names)
DEFAULTS = [2, 0, 1, 1, 0, 1, 1, 0, 1, 0, 1, 1, 1, 1, 0, 1, 1] + [0] * 14


def test_defaults_in_a_fresh_process():
    code = "from ultravox_amd import _lib; L = _lib.lib(); print(*[L.uvx_get_option(k) for k in range(1, 32)])"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert [int(x) for x in out.stdout.split()] == DEFAULTS
    assert len(DEFAULTS) == 31


def test_every_key_round_trips():
    L = _lib.lib()
    for k in range(1, 32):
        first = L.uvx_get_option(k)
        try:
            assert L.uvx_set_option(k, 1000 + k) == 0
            assert L.uvx_get_option(k) == 1000 + k
        finally:
            assert L.uvx_set_option(k, first) == 0
        assert L.uvx_get_option(k) == first


@pytest.mark.parametrize("key", [0, 32, -1])
def test_keys_outside_the_table_are_rejected(key):
    L = _lib.lib()
    L.uvx_gemm_pick_variant(128, 128, 128, 1)          # (any call that leaves no message of its own)
    assert L.uvx_set_option(key, 1) == -1              # UVX_ERR_INVALID
    assert f"unknown key {key}".encode() in L.uvx_last_error()
    assert L.uvx_get_option(key) == -1
    with pytest.raises(ValueError):
        with _lib.option(key, 1):
            pass


def test_header_enum_equals_the_python_mirror():
    src = open(os.path.join(ROOT, "include", "uvx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    body = re.search(r"typedef enum \{([^}]*)\} uvx_option_t;", src).group(1)
    entries = [e.strip() for e in body.split(",") if e.strip()]
    pairs = [re.fullmatch(r"UVX_OPT_([A-Z0-9_]+)\s*=\s*(\d+)", e) for e in entries]
    assert all(pairs), entries
    header = [(m.group(1), int(m.group(2))) for m in pairs]
    assert sorted(v for _, v in header) == list(range(1, 27))           # exactly keys 1 .. 26, each once
    assert len({n for n, _ in header}) == 26
    assert header == [(m.name, int(m)) for m in _lib.Option]            # member for member, in the header's order
    assert len(_lib.Option.__members__) == 26                            # (no aliases hiding behind the iteration)


def test_option_restores_the_entry_value():
    L = _lib.lib()
    key = _lib.Option.RMSNORM_TWO_PASS
    assert L.uvx_set_option(key, 7) == 0                # an entry value that is not the default
    try:
        with _lib.option(key, 1):
            assert L.uvx_get_option(key) == 1
        assert L.uvx_get_option(key) == 7
        with pytest.raises(KeyError):
            with _lib.option(key, 2):
                assert L.uvx_get_option(key) == 2
                raise KeyError("from the body")
        assert L.uvx_get_option(key) == 7
        with _lib.option(key, 3):                       # nested uses of one key unwind in order
            with _lib.option(18, 4):                    # (a plain number is the same key)
                assert L.uvx_get_option(key) == 4
                with pytest.raises(KeyError):
                    with _lib.option(key, 5):
                        assert L.uvx_get_option(key) == 5
                        raise KeyError("from the body")
                assert L.uvx_get_option(key) == 4
            assert L.uvx_get_option(key) == 3
        assert L.uvx_get_option(key) == 7
    finally:
        L.uvx_set_option(key, 0)
    assert L.uvx_get_option(key) == 0
