"""CPU: the arithmetic of the FP8 (OCP e4m3fn) weight format the drafter's stream-K GEMMs can stream (include/lantern_hip.h, "FP8 weight streaming"),
the size of its buffer, and the presence of its entry points in the built library.  What the kernels do with it: tests/test_gpu_drafter_fp8.py."""
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_finite_e4m3fn_code_is_a_bf16_value():
    """The kernel expands codes to bf16 operands without a scale: that is exact only if e4m3fn (4 exponent bits, 3 mantissa bits, subnormals down to
    2^-9) embeds in bf16 (8 exponent bits, 7 mantissa bits) -- every finite code -> f32 -> bf16 -> f32 is the identity; 254 finite codes, max 448."""
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    f = codes.view(torch.float8_e4m3fn).float()
    finite = torch.isfinite(f)
    assert int(finite.sum()) == 254 and not bool(finite[0x7f]) and not bool(finite[0xff])
    assert torch.equal(f[finite].to(torch.bfloat16).float(), f[finite])
    assert f[finite].abs().max().item() == 448.0 and f[0x7e].item() == 448.0 and f[0xfe].item() == -448.0
    assert f[0x01].item() == 2.0 ** -9 and f[0x08].item() == 2.0 ** -6          # smallest subnormal / smallest normal
    # and back: the round trip through torch's own conversion returns the code (the conversion the pack kernel is held against on the GPU)
    back = f[finite].to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(back, codes[finite])


def test_fp8_buffer_size_follows_the_bf16_brick_geometry():
    """Bricks in half the bytes of lantern_pack_linear_weight_bytes, plus 4 bytes (one f32 scale) per padded row of every set."""
    from lantern_amd import _lib
    L = _lib.lib()
    for n_rows, K, pair in ((33, 64, 0), (1, 64, 0), (48, 512, 48), (35, 832, 35), (1000, 1024, 0), (4096, 4096, 0), (11008, 4096, 11008), (8192, 4096, 0)):
        bf = int(L.lantern_pack_linear_weight_bytes(n_rows, K, pair))
        n_pad = (n_rows + 31) // 32 * 32
        sets = 2 if pair else 1
        assert bf == n_pad * K * 2 * sets
        assert int(L.lantern_pack_linear_weight_fp8_bytes(n_rows, K, pair)) == bf // 2 + 4 * n_pad * sets, (n_rows, K, pair)
    assert int(L.lantern_pack_linear_weight_fp8_bytes(32, 80, 0)) == 0 and int(L.lantern_pack_linear_weight_fp8_bytes(0, 64, 0)) == 0          # like the bf16 one


def test_fp8_entry_points_and_defines_exist():
    from lantern_amd import _lib
    L = _lib.lib()
    for name in ("lantern_pack_linear_weight_fp8_bytes", "lantern_pack_linear_weight_fp8", "lantern_unpack_linear_weight_fp8"):
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    hdr = open(os.path.join(ROOT, "include", "lantern_hip.h")).read()
    assert re.search(r"^#define LANTERN_PACKED_BF16 1$", hdr, re.M) and re.search(r"^#define LANTERN_PACKED_FP8 2$", hdr, re.M)
    for name in ("lantern_pack_linear_weight_fp8_bytes", "lantern_pack_linear_weight_fp8", "lantern_unpack_linear_weight_fp8"):
        assert re.search(r"\b" + name + r"\(", hdr), name
    from lantern_amd import ops
    assert (ops.PACKED_BF16, ops.PACKED_FP8) == (1, 2)
    assert L.lantern_version() == 200          # additive: the ABI version stays


def test_fp8_refusals_without_a_device():
    """Host-side argument checks: a CPU tensor or a non-bf16 source weight raises LanternError before anything is launched; the pack entry point
    refuses K % 64 != 0 as unsupported, with a message."""
    import ctypes as C

    import pytest
    from lantern_amd import _lib, ops
    with pytest.raises(_lib.LanternError):
        ops.pack_linear_weight(torch.zeros(32, 64, dtype=torch.bfloat16), fmt="fp8")
    with pytest.raises(_lib.LanternError):
        ops.pack_linear_weight(torch.zeros(32, 64, dtype=torch.bfloat16), fmt="int4")
    with pytest.raises(_lib.LanternError):
        ops.unpack_linear_weight_fp8(ops.PackedLinearWeight(torch.zeros(8), 32, 64, 0))          # a bf16 packed weight has no codes
    L = _lib.lib()
    buf = (C.c_char * 65536)()
    rc = L.lantern_pack_linear_weight_fp8(C.c_void_p(C.addressof(buf)), 32, 80, 0, C.c_void_p(C.addressof(buf)), None)
    assert rc == -3 and b"multiple of 64" in L.lantern_last_error()          # LANTERN_E_UNSUPPORTED
