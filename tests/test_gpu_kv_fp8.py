"""The FP8 KV cache end to end (include/lantern_hip.h, "FP8 KV cache"): the hardware conversion the format leans on, the quantising append against a
torch restatement of the format's rule (bit-exact), `lantern_tree_attention_kv8` against the references of tests/test_gpu_tree_attention.py on the
dequantised caches (same bars: ATOL = RTOL = 2e-2, and no further from f64 than the reference's own pipeline + 2e-2) and against the bf16 kernel on
those caches (bit-identical: the fp8 instance keeps the bf16 instance's assignment of d-columns to MFMA operand slots), the commit kernels on the
byte rows, and the `KVCache` mirror."""
import math
import types

import numpy as np
import pytest
import torch

from lantern_amd import _lib, ops
from lantern_amd.drafters.kv_cache import initialize_past_key_values

pytestmark = pytest.mark.gpu
ATOL, RTOL = 2e-2, 2e-2


# ------------------------------------------------------------------------------------------------ the format, restated in torch on the CPU

def ref_quantize(x):
    """bf16 [..., d] (CPU) -> uint8 [..., d + 16]: frexp rule, exact division, clamp to +-448, torch's RNE cast to float8_e4m3fn."""
    xf = x.float()
    amax = xf.abs().amax(-1)
    m, p = torch.frexp(amax)
    e = (p.to(torch.int64) - 9 + (m > 0.875).to(torch.int64)).clamp(-64, 64)
    e[amax == 0] = 0
    s = torch.ldexp(torch.ones_like(amax), e.to(torch.int32))
    codes = (xf / s[..., None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    tail = torch.zeros(x.shape[:-1] + (16,), dtype=torch.uint8)
    tail[..., :4] = s.contiguous().view(torch.uint8).reshape(x.shape[:-1] + (4,))
    return torch.cat((codes, tail), dim=-1)


def special_rows(n, d, seed):
    """n bf16 rows of d elements that walk through the cases of the format's rule (kind = row % 8)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    rows = []
    for i in range(n):
        kind = i % 8
        x = (torch.randn(d, generator=g) * 50.0).to(torch.bfloat16)
        j = int(torch.randint(0, d, (1,), generator=g))
        if kind == 0:      # amax exactly 448 * 2^3
            x[j] = -3584.0
        elif kind == 1:    # the next bf16 above it: the exponent steps up
            x[j] = torch.tensor([0x4560 + 1], dtype=torch.int16).view(torch.bfloat16)[0]          # 0x4560 = 3584.0
            assert float(x[j]) == 3600.0
        elif kind == 2:
            x = torch.zeros(d, dtype=torch.bfloat16)
        elif kind == 3:    # lower clamp: e = -64, every code 0
            x = torch.full((d,), 1e-30, dtype=torch.bfloat16)
        elif kind == 4:    # upper clamp: e = 64, every code saturates
            x = torch.full((d,), 1e25, dtype=torch.bfloat16)
            x[::2] = -x[::2]
        elif kind == 5:    # scale 1: exact halves between two e4m3 values (normal and subnormal range), both signs
            ties = torch.tensor([1.0625, 1.1875, 17.0, 19.0, 2.0 ** -10, 1.5 * 2.0 ** -9, 2.5 * 2.0 ** -9, 7.5 * 2.0 ** -9, 232.0, 440.0, 0.0166015625])
            x = torch.cat([ties, -ties] * (d // 22 + 1))[:d].to(torch.bfloat16)
            x[j] = 448.0
        elif kind == 6:    # scale 1: the code's subnormal range, on and between its 2^-9 steps
            steps = torch.cat([torch.arange(0, 9).float(), torch.tensor([0.3, 0.7, 1.25, 2.75, 6.6, 7.9])]) * 2.0 ** -9
            x = torch.cat([steps, -steps] * (d // 30 + 1))[:d].to(torch.bfloat16)
            x[j] = -448.0
        rows.append(x)
    return torch.stack(rows)


# ------------------------------------------------------------------------------------------------ (a) the conversion

@pytest.mark.parametrize("d", [64, 128])
def test_conversion_is_exact_for_every_code_and_scale(d):
    """The hardware assumption of the format: v_cvt_scalef32_pk_bf16_fp8 with a scale 2^e returns code * 2^e exactly."""
    exps = [-64, -9, 0, 7, 64]
    codes = ((torch.arange(256)[:, None] + torch.arange(d)[None, :]) % 256).to(torch.uint8)          # every code at every byte position
    slab = torch.zeros(len(exps), 256, d + 16, dtype=torch.uint8)
    want = torch.empty(len(exps), 256, d, dtype=torch.float32)
    for i, e in enumerate(exps):
        s = torch.ldexp(torch.ones(1), torch.tensor([e], dtype=torch.int32))
        slab[i, :, :d] = codes
        slab[i, :, d:d + 4] = s.view(torch.uint8)
        want[i] = codes.view(torch.float8_e4m3fn).float() * s
    got = ops.kv8_dequantize(slab.cuda()).float().cpu()
    ok = (codes & 0x7f) != 0x7f                                                                        # the two NaN codes
    assert torch.isfinite(want[:, ok]).all()
    assert torch.equal(got[:, ok], want[:, ok])


# ------------------------------------------------------------------------------------------------ (b) the quantiser

@pytest.mark.parametrize("pos_kind", ["array", "scalar"])
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("d", [64, 128])
def test_append_is_bit_exact_and_touches_only_its_rows(d, T, pos_kind):
    B, Hkv, S_max = 2, 2, 16
    n = B * Hkv * T
    k_rows, v_rows = special_rows(n, d, seed=d + T), special_rows(n + 4, d, seed=2 * d + T)[4:]      # V starts at kind 4: all 8 kinds even at T = 1
    k_new = k_rows.reshape(B, T, Hkv, d).cuda()                                                       # [B, T, Hkv, d]: passed as the transposed view
    v_new = v_rows.reshape(B, T, Hkv, d).cuda()
    k_slab = torch.full((B, Hkv, S_max, d + 16), 0xA5, dtype=torch.uint8, device="cuda")
    v_slab = k_slab.clone()
    if pos_kind == "array":
        pos = [3, S_max - 2] if T > 1 else [S_max - 1, S_max]       # batch row 1: rows from position S_max on are skipped
        ops.kv8_append(k_new.transpose(1, 2), v_new.transpose(1, 2), k_slab, v_slab, torch.tensor(pos, dtype=torch.int64, device="cuda"))
    else:
        pos = [7, 7]
        ops.kv8_append(k_new.transpose(1, 2), v_new.transpose(1, 2), k_slab, v_slab, 7)
    torch.cuda.synchronize()
    written = 0
    for new, slab in ((k_new, k_slab), (v_new, v_slab)):
        want = torch.full((B, Hkv, S_max, d + 16), 0xA5, dtype=torch.uint8)
        q = ref_quantize(new.cpu())                                                                   # [B, T, Hkv, d + 16]
        for b in range(B):
            for t in range(T):
                if pos[b] + t < S_max:
                    want[b, :, pos[b] + t] = q[b, t]
                    written += 1
        got = slab.cpu()
        assert torch.equal(got[..., :d], want[..., :d]), "codes (or bytes outside the written rows)"
        assert torch.equal(got[..., d:], want[..., d:]), "tail bytes"
    assert written == (2 * (2 * T if pos_kind == "scalar" else (T + 2 if T > 1 else 1)))


def test_append_one_pair_alone_and_dequantise_round_trip():
    """K without V (what `KVCache.cat` does), and the read-back equals codes * scale of the restated format."""
    B, Hkv, T, d, S_max = 1, 3, 7, 128, 8
    x = special_rows(B * Hkv * T, d, seed=9).reshape(B, Hkv, T, d)
    slab = torch.zeros(B, Hkv, S_max, d + 16, dtype=torch.uint8, device="cuda")
    ops.kv8_append(None, x.cuda(), None, slab, 1)
    want = ref_quantize(x)
    assert torch.equal(slab[:, :, 1:8].cpu(), want) and not slab[:, :, 0].any()
    deq = ops.kv8_dequantize(slab[:, :, 1:8].contiguous()).float().cpu()
    scale = want[..., d:d + 4].contiguous().view(torch.float32)
    assert torch.equal(deq, want[..., :d].view(torch.float8_e4m3fn).float() * scale)
    with pytest.raises(_lib.LanternError):
        ops.kv8_append(x.cuda(), None, None, slab, 0)                        # new rows without their cache
    with pytest.raises(_lib.LanternError):
        ops.kv8_append(x.cuda().float(), None, slab, None, 0)


# ------------------------------------------------------------------------------------------------ (c) attention
# the two references and the case maker of tests/test_gpu_tree_attention.py, restated

def reference_attention(q, k_cache, v_cache, tree_mask, kv_len, kv_start, scale):
    B, N, Hq, d = q.shape
    Hkv = k_cache.shape[1]
    outs = []
    fmin = torch.finfo(torch.float32).min
    for b in range(B):
        L, st = int(kv_len[b]), int(kv_start[b])
        k = k_cache[b, :, :L].repeat_interleave(Hq // Hkv, dim=0)
        v = v_cache[b, :, :L].repeat_interleave(Hq // Hkv, dim=0)
        w = torch.matmul(q[b].transpose(0, 1), k.transpose(1, 2)).float() * scale
        mask = torch.zeros(N, L, dtype=torch.float32, device=q.device)
        mask[:, :st] = fmin
        tm = tree_mask if tree_mask.dim() == 2 else tree_mask[b]
        mask[:, L - N:][tm == 0] = fmin
        p = torch.softmax(w + mask, dim=-1).to(torch.bfloat16)
        outs.append(torch.matmul(p, v).transpose(0, 1).reshape(N, Hq * d))
    return torch.stack(outs)


def exact_attention(q, k_cache, v_cache, tree_mask, kv_len, kv_start, scale):
    B, N, Hq, d = q.shape
    Hkv = k_cache.shape[1]
    outs = []
    for b in range(B):
        L, st = int(kv_len[b]), int(kv_start[b])
        k = k_cache[b, :, :L].repeat_interleave(Hq // Hkv, dim=0).double()
        v = v_cache[b, :, :L].repeat_interleave(Hq // Hkv, dim=0).double()
        w = torch.matmul(q[b].transpose(0, 1).double(), k.transpose(1, 2)) * scale
        vis = torch.ones(N, L, dtype=torch.bool, device=q.device)
        vis[:, :st] = False
        tm = tree_mask if tree_mask.dim() == 2 else tree_mask[b]
        vis[:, L - N:] = tm != 0
        p = torch.softmax(w.masked_fill(~vis, -math.inf), dim=-1)
        outs.append(torch.matmul(p, v).transpose(0, 1).reshape(N, Hq * d))
    return torch.stack(outs)


def make_case(B, Hq, Hkv, N, d, S_max, lens, starts, seed, tree_mask=None):
    """q, the two fp8 slabs (quantised by the append kernel; rows past the end hold NaN codes and a NaN scale), their dequantised bf16 images, and
    the same slabs with clean zero rows past the end."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    q = torch.randn(B, N, Hq, d, generator=g).to(torch.bfloat16).cuda()
    k = torch.randn(B, Hkv, S_max, d, generator=g).to(torch.bfloat16).cuda()
    v = torch.randn(B, Hkv, S_max, d, generator=g).to(torch.bfloat16).cuda()
    k8 = torch.empty(B, Hkv, S_max, d + 16, dtype=torch.uint8, device="cuda")
    v8 = torch.empty_like(k8)
    ops.kv8_append(k, v, k8, v8, 0)
    k8z, v8z = k8.clone(), v8.clone()
    for b in range(B):
        k8[b, :, lens[b]:, :d], v8[b, :, lens[b]:, :d] = 0x7F, 0xFF
        k8[b, :, lens[b]:, d:], v8[b, :, lens[b]:, d:] = 0xFF, 0xFF
        k8z[b, :, lens[b]:], v8z[b, :, lens[b]:] = 0, 0
    if tree_mask is None:
        tree_mask = torch.tril(torch.ones(N, N))
        tree_mask[torch.rand(N, N, generator=g) < 0.5] = 0
        tree_mask = torch.tril(tree_mask)
        tree_mask.fill_diagonal_(1)
        tree_mask[:, 0] = 1
    kd, vd = ops.kv8_dequantize(k8), ops.kv8_dequantize(v8)
    dev = lambda x: torch.tensor(x, dtype=torch.int64).cuda()          # noqa: E731
    return dict(q=q, k8=k8, v8=v8, k8z=k8z, v8z=v8z, kd=kd, vd=vd, tm=tree_mask.cuda(), lens=dev(lens), starts=dev(starts))


def check(c, max_kv_len=None, q=None):
    q = c["q"] if q is None else q
    d = q.shape[-1]
    bits = ops.tree_mask_bits(c["tm"])
    kw = dict(kv_len=c["lens"], kv_start=c["starts"], max_kv_len=max_kv_len)
    out = ops.tree_attention(q, c["k8"], c["v8"], bits, **kw)
    out_clean = ops.tree_attention(q, c["k8z"], c["v8z"], bits, **kw)
    out_bf16 = ops.tree_attention(q, c["kd"], c["vd"], bits, **kw)
    torch.cuda.synchronize()
    got = out.float()
    assert torch.isfinite(got).all()
    assert torch.equal(out, out_clean), "rows past kv_len leaked into the output"
    # (i) the bars of tests/test_gpu_tree_attention.py against both references on the dequantised caches
    qc = q.contiguous()
    ref = reference_attention(qc, c["kd"], c["vd"], c["tm"], c["lens"], c["starts"], d ** -0.5).float()
    exact = exact_attention(qc, c["kd"], c["vd"], c["tm"], c["lens"], c["starts"], d ** -0.5).float()
    err = (got - ref).abs()
    print(f"max |fp8 - ref| = {float(err.max()):.3e}   max |fp8 - f64| = {float((got - exact).abs().max()):.3e}   "
          f"max |ref - f64| = {float((ref - exact).abs().max()):.3e}   differing elements vs bf16 kernel = {int((out != out_bf16).sum())}")
    assert (err <= ATOL + RTOL * ref.abs()).all(), float(err.max())
    assert float((got - exact).abs().max()) <= float((ref - exact).abs().max()) + 2e-2
    # (ii) the bf16 kernel on the dequantised caches: the same d-column -> MFMA slot assignment, so the same bits
    assert torch.equal(out, out_bf16)
    return out


def test_attention_lumina_head_shape():
    check(make_case(2, 4, 4, 26, 128, 256, [126, 100], [0, 37], seed=1))


@pytest.mark.parametrize("N", [1, 33, 64])
def test_attention_tree_sizes(N):
    check(make_case(1, 4, 4, N, 128, 192, [100 + N], [0], seed=10 + N))


def test_attention_d64_gqa():
    check(make_case(2, 8, 2, 59, 64, 384, [200, 384], [0, 11], seed=3))


@pytest.mark.parametrize("prev", [0, 31, 32, 33])
def test_attention_prefix_lengths_around_tile_edges(prev):
    check(make_case(1, 2, 2, 26, 128, 96, [prev + 26], [0], seed=20 + prev))


def test_attention_per_row_tree_bits_and_transposed_q():
    B, Hq, N, d = 3, 4, 40, 128
    g = torch.Generator(device="cpu").manual_seed(5)
    tms = []
    for b in range(B):
        tm = torch.tril((torch.rand(N, N, generator=g) < 0.4).float())
        tm.fill_diagonal_(1)
        tms.append(tm)
    c = make_case(B, Hq, Hq, N, d, 320, [150, 320, 41], [0, 5, 0], seed=6, tree_mask=torch.stack(tms))
    got = check(c)
    qt = c["q"].permute(0, 2, 1, 3).contiguous()                      # [B,Hq,N,d] as after .transpose(1, 2) in the reference
    got_t = check(c, q=qt.permute(0, 2, 1, 3))
    assert torch.equal(got, got_t)


def test_attention_split_keys_path():
    need = _lib.lib().lantern_tree_attention_workspace(1, 2, 59, 128, 4096)
    assert need > 0                                                   # this shape does take the split path (the workspace serves both formats)
    check(make_case(1, 2, 2, 59, 128, 4096, [3900], [17], seed=8))


def test_attention_argument_errors():
    c = make_case(1, 2, 2, 8, 128, 64, [40], [0], seed=11)
    bits = ops.tree_mask_bits(c["tm"])
    with pytest.raises(_lib.LanternError):
        ops.tree_attention(c["q"], c["k8"], c["vd"], bits)                       # mixed formats
    with pytest.raises(_lib.LanternError):
        ops.tree_attention(c["q"], c["k8"][..., :128], c["v8"][..., :128], bits)     # uint8 rows that are not d + 16
    with pytest.raises(_lib.LanternError):
        ops.tree_attention(c["q"], c["k8"].to(torch.int8), c["v8"].to(torch.int8), bits)
    with pytest.raises(_lib.LanternError):
        ops.tree_attention(c["q"][..., :64], c["k8"], c["v8"], bits)            # d = 64 queries on d = 128 rows


# ------------------------------------------------------------------------------------------------ (d) the commit on byte rows

def _commit_case():
    from lantern_amd.drafters import choices
    tb = ops.tree_static_build(choices.mc_sim_7b_63)
    ret = torch.from_numpy(np.ascontiguousarray(tb["retrieve_indices"])).cuda()          # [P, D], -1 padded
    lens = (ret >= 0).sum(-1)
    cands = [p for p in range(ret.shape[0]) if int(lens[p]) >= 3 and int(ret[p, 1]) != 1]
    pth = max(cands, key=lambda p: int(lens[p]))                                         # a path whose nodes are not in place
    return ret, pth, int(lens[pth]), int(ret.max()) + 1


def test_commit_moves_fp8_rows_byte_for_byte():
    """lantern_kv_gather on rows of 144 bytes (9 16-byte chunks; 5 at d = 64): codes and tails move together, nothing else changes."""
    ret, pth, n, N = _commit_case()
    for d in (128, 64):
        S, prev = 96, 37
        g = torch.Generator(device="cpu").manual_seed(d)
        k8 = torch.zeros(4, S, d + 16, dtype=torch.uint8, device="cuda")
        v8 = torch.zeros_like(k8)
        new = [(torch.randn(1, 4, prev + N, d, generator=g) * (1 + torch.arange(prev + N)[:, None])).to(torch.bfloat16).cuda() for _ in range(2)]
        ops.kv8_append(new[0], new[1], k8[None], v8[None], 0)                             # a different scale per position
        before = [k8.clone(), v8.clone()]
        assert len({bytes(r) for r in before[0][0, :prev + N, d:d + 4].cpu().numpy()}) > 4
        best = torch.tensor([pth], dtype=torch.int32, device="cuda")
        alen = torch.tensor([n - 1], dtype=torch.int32, device="cuda")
        nl = ops.kv_gather([k8, v8], torch.zeros(2, dtype=torch.int32, device="cuda"), torch.full((2,), prev, dtype=torch.int64, device="cuda"),
                           ret, best, alen)
        assert nl.tolist() == [prev + n, prev + n]
        src = ret[pth, :n] + prev
        for s, b0 in zip((k8, v8), before):
            assert torch.equal(s[:, prev:prev + n], b0[:, src])                           # moved rows, tails included
            keep = torch.ones(S, dtype=torch.bool, device="cuda")
            keep[prev:prev + n] = False
            assert torch.equal(s[:, keep], b0[:, keep])


def _fake_model(L, Hq, Hkv, d, S_max):
    lin = types.SimpleNamespace(weight=torch.zeros(1, device="cuda"))
    return types.SimpleNamespace(config=types.SimpleNamespace(num_hidden_layers=L, num_key_value_heads=Hkv, max_position_embeddings=S_max,
                                                              hidden_size=Hq * d, num_attention_heads=Hq),
                                 model=types.SimpleNamespace(layers=[types.SimpleNamespace(self_attn=types.SimpleNamespace(q_proj=lin))]),
                                 dtype=torch.bfloat16)


def test_commit_through_kvcache_copy():
    ret, pth, n, N = _commit_case()
    prev, d = 21, 128
    pkv, slabs, cur = initialize_past_key_values(_fake_model(1, 4, 4, d, 96), 1, kv_format="fp8")
    kc = pkv[0][0]
    g = torch.Generator(device="cpu").manual_seed(4)
    kc.cat((torch.randn(1, 4, prev + N, d, generator=g) * (1 + torch.arange(prev + N)[:, None])).to(torch.bfloat16).cuda())
    before = kc.data.clone()
    idx = ret[pth, :n] + prev
    kc.copy(idx, prev)
    assert int(cur[0]) == prev + n and kc.shape == (1, 4, prev + n, d)
    assert torch.equal(kc.data[:, :, prev:prev + n], before[:, :, idx])
    keep = torch.ones(96, dtype=torch.bool, device="cuda")
    keep[prev:prev + n] = False
    assert torch.equal(kc.data[:, :, keep], before[:, :, keep])
    assert not slabs[0][1].any()                                                          # the V slab of the layer was not touched


# ------------------------------------------------------------------------------------------------ (e) the mirror API

def test_kvcache_fp8_mirror_equals_the_direct_path():
    B, Hq, Hkv, d, S_max, prev, N = 2, 4, 2, 128, 160, 45, 26
    pkv, slabs, cur = initialize_past_key_values(_fake_model(2, Hq, Hkv, d, S_max), B, kv_format="fp8")
    assert len(slabs) == 1 and slabs[0].shape == (4, B, Hkv, S_max, d + 16) and slabs[0].dtype == torch.uint8
    assert cur.shape == (4,) and cur.dtype == torch.long and not cur.is_cuda
    g = torch.Generator(device="cpu").manual_seed(12)
    rnd = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).cuda()               # noqa: E731
    k0, v0, k1, v1, q = rnd(B, Hkv, prev, d), rnd(B, Hkv, prev, d), rnd(B, Hkv, N, d), rnd(B, Hkv, N, d), rnd(B, N, Hq, d)
    kc, vc = pkv[1]                                                                        # second layer: a non-zero slab offset
    kc.cat(k0); vc.cat(v0)
    k_all, v_all = kc.cat(k1), vc.cat(v1)
    assert k_all.shape == (B, Hkv, prev + N, d + 16) and k_all.dtype == torch.uint8 and kc.shape == (B, Hkv, prev + N, d)
    assert int(cur[2]) == int(cur[3]) == prev + N and int(cur[0]) == 0
    tm = torch.tril(torch.ones(N, N)).cuda()
    bits = ops.tree_mask_bits(tm)
    lens = torch.tensor([prev + N] * B, dtype=torch.int64, device="cuda")
    out = ops.tree_attention(q, kc.data, vc.data, bits, kv_len=lens, max_kv_len=prev + N)
    # the direct path: the C-ABI wrappers on slabs of one's own
    k8 = torch.zeros(B, Hkv, S_max, d + 16, dtype=torch.uint8, device="cuda")
    v8 = torch.zeros_like(k8)
    ops.kv8_append(k0, v0, k8, v8, 0)
    ops.kv8_append(k1, v1, k8, v8, torch.full((B,), prev, dtype=torch.int64, device="cuda"))
    assert torch.equal(k8, kc.data) and torch.equal(v8, vc.data)
    want = ops.tree_attention(q, k8, v8, bits, kv_len=lens, max_kv_len=prev + N)
    assert torch.equal(out, want) and torch.isfinite(out.float()).all()
    with pytest.raises(ValueError):
        kc.cat(rnd(B, Hkv, S_max, d))                                                      # does not fit


def test_default_kv_format_is_unchanged():
    fake = _fake_model(2, 4, 4, 128, 64)
    a = initialize_past_key_values(fake, 2)
    b = initialize_past_key_values(fake, batch_size=2, kv_format="bf16")
    for pkv, slabs, cur in (a, b):
        assert slabs[0].shape == (4, 2, 4, 64, 128) and slabs[0].dtype == torch.bfloat16 and cur.shape == (4,)
        x = torch.randn(2, 4, 5, 128, device="cuda").to(torch.bfloat16)
        got = pkv[1][0].cat(x)
        assert torch.equal(got, x) and pkv[1][0].shape == (2, 4, 5, 128) and torch.equal(slabs[0][2, :, :, :5], x)
