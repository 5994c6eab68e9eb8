"""CPU: the FP8 KV-cache entries of the C ABI -- declared, exported, row size, refusals in front of any launch -- and the scale rule of the
format (include/lantern_hip.h, "FP8 KV cache"): the frexp form the header states picks the smallest e with amax <= 448 * 2^e for every
positive finite bf16 value."""
import ctypes as C
import os
import re

import torch

from lantern_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["lantern_kv8_row_bytes", "lantern_kv8_append", "lantern_kv8_dequantize", "lantern_tree_attention_kv8"]
E_INVALID, E_UNSUPPORTED = -1, -3          # include/lantern_hip.h


def _err():
    return (_lib.lib().lantern_last_error() or b"").decode()


def test_header_declares_and_library_exports_the_four_entries():
    hdr = open(os.path.join(ROOT, "include", "lantern_hip.h")).read()
    declared = set(re.findall(r"\b(lantern_[a-z_0-9]+)\s*\(", hdr))
    L = _lib.lib()
    for name in ENTRIES:
        assert name in declared, f"{name} not declared in lantern_hip.h"
        assert hasattr(L, name), f"{name} not exported"
        assert name in _lib.EXPORTS
    assert re.search(r"LANTERN_E_INVALID = -1\b", hdr) and re.search(r"LANTERN_E_UNSUPPORTED = -3\b", hdr)
    assert L.lantern_version() == 200


def test_row_bytes():
    L = _lib.lib()
    assert L.lantern_kv8_row_bytes(64) == 80
    assert L.lantern_kv8_row_bytes(128) == 144
    assert L.lantern_kv8_row_bytes(96) == 0


def _append(L, k_new=0x1000, v_new=0x2000, k_cache=0x3000, v_cache=0x4000, B=2, Hkv=2, T=5, d=128, nsb=None, nsh=None, nst=None, sb=None, sh=None,
            pos=None, pos0=0, S_max=64):
    row = d + 16
    nsb = Hkv * T * d if nsb is None else nsb
    nsh = T * d if nsh is None else nsh
    nst = d if nst is None else nst
    sh = S_max * row if sh is None else sh
    sb = Hkv * sh if sb is None else sb
    return L.lantern_kv8_append(C.c_void_p(k_new), C.c_void_p(v_new), C.c_void_p(k_cache), C.c_void_p(v_cache), B, Hkv, T, d, C.c_int64(nsb),
                                C.c_int64(nsh), C.c_int64(nst), C.c_int64(sb), C.c_int64(sh), C.c_void_p(pos), C.c_int64(pos0), C.c_int64(S_max), None)


def test_append_refusals_without_a_device():
    """Every check runs on the host in front of the launch: the (fake) pointers are never touched."""
    L = _lib.lib()
    assert _append(L, k_new=None, v_new=None, k_cache=None, v_cache=None) == E_INVALID and "null" in _err()
    assert _append(L, k_cache=None) == E_INVALID and "null" in _err()                  # a new-rows pointer without its cache
    assert _append(L, v_new=None) == E_INVALID
    assert _append(L, d=96) in (E_INVALID, E_UNSUPPORTED) and "96" in _err()
    assert _append(L, sh=64 * 144 + 8) == E_INVALID and "16" in _err()                 # a byte stride that is no multiple of 16
    assert _append(L, sb=2 * 64 * 144 + 4) == E_INVALID
    assert _append(L, sh=63 * 144) == E_INVALID and "kv_stride_h_bytes" in _err()      # rows of one head would overlap the next head's
    assert _append(L, nst=100) == E_INVALID
    assert _append(L, k_new=0x1008) == E_INVALID and "aligned" in _err()
    assert _append(L, pos0=-1) == E_INVALID
    assert _append(L, T=0) == 0 and _append(L, B=0) == 0                               # nothing to do: no launch


def test_dequantize_refusals_without_a_device():
    L = _lib.lib()
    assert L.lantern_kv8_dequantize(None, None, C.c_int64(4), 128, None) == E_INVALID and "null" in _err()
    assert L.lantern_kv8_dequantize(C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_int64(4), 96, None) in (E_INVALID, E_UNSUPPORTED)
    assert L.lantern_kv8_dequantize(C.c_void_p(0x1004), C.c_void_p(0x2000), C.c_int64(4), 128, None) == E_INVALID
    assert L.lantern_kv8_dequantize(None, None, C.c_int64(0), 128, None) == 0


def _attn(L, q=0x1000, k=0x2000, v=0x3000, out=0x4000, bits=0x5000, B=1, Hq=4, Hkv=4, N=26, d=128, S=256, sb=None, sh=None, ws=None, ws_bytes=0):
    row = d + 16
    sh = S * row if sh is None else sh
    sb = Hkv * sh if sb is None else sb
    return L.lantern_tree_attention_kv8(C.c_void_p(q), C.c_void_p(k), C.c_void_p(v), C.c_void_p(out), B, Hq, Hkv, N, d, C.c_int64(N * Hq * d),
                                        C.c_int64(Hq * d), C.c_int64(d), C.c_int64(sb), C.c_int64(sh), C.c_int64(N * Hq * d), C.c_int64(Hq * d),
                                        None, None, C.c_int64(S), C.c_void_p(bits), 0, C.c_float(d ** -0.5), C.c_void_p(ws), C.c_size_t(ws_bytes), None)


def test_attention_refusals_without_a_device():
    L = _lib.lib()
    assert _attn(L, k=None) == E_INVALID and "null" in _err()
    assert _attn(L, q=None) == E_INVALID
    assert _attn(L, bits=None) == E_INVALID
    assert _attn(L, d=96) in (E_INVALID, E_UNSUPPORTED) and "96" in _err()
    assert _attn(L, sh=256 * 144 + 8) == E_INVALID and "16" in _err()
    assert _attn(L, sb=4 * 256 * 144 + 8) == E_INVALID
    assert _attn(L, sh=256 * 144 - 16) == E_INVALID and "kv_stride_h" in _err()        # kv_stride_h < max_kv_len * (d + 16)
    assert _attn(L, sh=256 * 128) == E_INVALID                                         # the bf16 entry's element count is too small here
    assert _attn(L, N=65) == E_INVALID and "65" in _err()
    assert _attn(L, Hq=4, Hkv=3) == E_INVALID
    assert _attn(L, B=0) == 0
    # the split path asks for the same workspace as the bf16 entry
    need = L.lantern_tree_attention_workspace(1, 2, 59, 128, C.c_int64(4096))
    assert need > 0 and _attn(L, Hq=2, Hkv=2, N=59, S=4096) == E_INVALID and "workspace" in _err()


def test_frexp_rule_is_the_smallest_scale_exponent_for_every_bf16_value():
    """e = p - 9 + (m > 0.875) with (m, p) = frexp(amax) against brute force: 448 * 2^e >= amax > 448 * 2^(e - 1), all positive finite bf16."""
    bits = torch.arange(1, 0x7f80, dtype=torch.int32).to(torch.int16)                  # subnormals included, inf / NaN excluded
    amax = bits.view(torch.bfloat16).double()
    assert amax.numel() == 0x7f7f and bool(torch.isfinite(amax).all()) and bool((amax > 0).all())
    m, p = torch.frexp(amax.float())
    e = p.to(torch.int64) - 9 + (m > 0.875).to(torch.int64)
    cap = 448.0 * torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double())        # exact in f64 over this range
    assert bool((amax <= cap).all()), "the scale does not cover the row maximum"
    assert bool((amax > cap / 2).all()), "a smaller exponent would have covered it"
    # the integer form of the same rule on the bf16 bit pattern (what the device computes), normal values
    normal = bits.to(torch.int64) >= 0x80
    e_bits = (bits.to(torch.int64) >> 7) - 135 + ((bits.to(torch.int64) & 0x7f) > 0x60).to(torch.int64)
    assert torch.equal(e[normal], e_bits[normal])
    assert bool((e[~normal] < -64).all()) and bool((e_bits[~normal] < -64).all())    # subnormal maxima: both clamp to -64


def test_python_mirror_refuses_other_dtypes_and_formats():
    import types
    import pytest
    from lantern_amd.drafters.kv_cache import initialize_past_key_values
    fake = types.SimpleNamespace(config=types.SimpleNamespace(num_hidden_layers=1, num_key_value_heads=2, max_position_embeddings=32,
                                                              hidden_size=2 * 128, num_attention_heads=2),
                                 parameters=lambda: iter([torch.zeros(1)]), dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        initialize_past_key_values(fake, 1, kv_format="int4")
    pkv, slabs, cur = initialize_past_key_values(fake, 2, kv_format="fp8")             # allocation alone needs no device
    assert slabs[0].shape == (2, 2, 2, 32, 144) and slabs[0].dtype == torch.uint8 and not slabs[0].any()
    assert pkv[0][0].shape == (2, 2, 0, 128)
    fake.config.hidden_size = 2 * 96
    with pytest.raises(ValueError):
        initialize_past_key_values(fake, 1, kv_format="fp8")
