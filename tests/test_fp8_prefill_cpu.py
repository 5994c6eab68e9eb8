"""CPU: the two C entries behind the drafter's FP8 prompt prefill -- lantern_linear_rows_packed_fmt (lantern_linear_rows_packed with the packed weight's
format as an argument) and lantern_drafter_fc_packed (the input stage on the packed weight at any row count): present, declared, bound, and every
argument check answered on the host before anything is launched.  What the kernels compute: tests/test_gpu_prefill_fp8.py."""
import ctypes as C
import os
import re

from lantern_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lantern_linear_rows_packed_fmt", "lantern_drafter_fc_packed")
INVALID = -1          # LANTERN_E_INVALID


def test_both_symbols_are_exported_declared_and_bound():
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "lantern_hip.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name
        assert re.search(r"^int " + name + r"\(", hdr, re.M), name
    assert L.lantern_version() == 200          # additive: the ABI version stays


def test_linear_rows_packed_fmt_validates_without_gpu():
    """The checks of lantern_linear_rows_packed, plus the format: packed = 0 is no packed weight.  Both formats answer alike; nothing is dereferenced or
    launched before a check fails (the addresses are not memory)."""
    L = _lib.lib()
    one = C.c_void_p(0x1000)
    f = L.lantern_linear_rows_packed_fmt
    assert f(one, one, None, 64, 128, 32, one, 32, 0, None, 0, 0, 0, None) == INVALID and b"packed = 0" in L.lantern_last_error()
    assert f(one, one, None, 64, 128, 32, one, 32, 0, None, 0, 0, 3, None) == INVALID and b"packed = 3" in L.lantern_last_error()          # no third format read as bf16
    for packed in (1, 2):
        assert f(None, one, None, 64, 128, 32, one, 32, 0, None, 0, 0, packed, None) == INVALID and b"null buffer" in L.lantern_last_error()
        assert f(one, one, None, 64, 100, 32, one, 32, 0, None, 0, 0, packed, None) == INVALID and b"multiple of 64" in L.lantern_last_error()
        assert f(one, one, None, 64, 128, 32, one, 16, 0, None, 0, 0, packed, None) == INVALID          # out rows shorter than n_rows
        assert f(one, one, None, 64, 128, 32, one, 32, 7, None, 0, 0, packed, None) == INVALID and b"epilogue 7" in L.lantern_last_error()
        assert f(one, one, None, 64, 128, 32, one, 32, 1, None, 0, 0, packed, None) == INVALID and b"residual" in L.lantern_last_error()
        assert f(one, one, None, 64, 128, 32, one, 32, 2, None, 0, 0, packed, None) == INVALID and b"pair_rows" in L.lantern_last_error()
        assert f(one, one, None, 0, 128, 32, one, 32, 0, None, 0, 0, packed, None) == 0                  # no rows: nothing to do
        assert f(one, one, None, 64, 128, 0, one, 32, 0, None, 0, 0, packed, None) == 0                  # no columns either
    assert f(one, one, None, 64, 100, 32, one, 32, 0, None, 0, 0, 2, None) == INVALID and b"linear_rows_packed_fmt" in L.lantern_last_error()


def test_drafter_fc_packed_validates_without_gpu():
    L = _lib.lib()
    one = C.c_void_p(0x1000)
    f = L.lantern_drafter_fc_packed
    scale = C.c_float(1.0)
    assert f(one, one, one, one, None, 200, 128, 512, scale, one, 0, None) == INVALID and b"packed = 0" in L.lantern_last_error()
    assert f(one, one, one, one, None, 200, 128, 512, scale, one, 3, None) == INVALID and b"packed = 3" in L.lantern_last_error()
    for packed in (1, 2):
        assert f(None, one, one, one, None, 200, 128, 512, scale, one, packed, None) == INVALID and b"null buffer" in L.lantern_last_error()
        assert f(one, one, one, one, None, 200, 96, 512, scale, one, packed, None) == INVALID and b"multiple of 64" in L.lantern_last_error()      # H % 64
        assert f(one, one, one, one, None, 200, 48, 512, scale, one, packed, None) == INVALID                                                     # (% 16 is not enough)
        assert f(one, one, one, one, None, -1, 128, 512, scale, one, packed, None) == INVALID
        assert f(one, one, one, one, None, 200, 128, 0, scale, one, packed, None) == INVALID                                                      # an empty vocabulary
        assert f(one, one, one, one, None, 0, 128, 512, scale, one, packed, None) == 0                                                            # no rows
