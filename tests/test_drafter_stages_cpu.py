"""The tolerances tests/test_gpu_drafter_stages.py holds the drafter's norm, head-stage and split-K kernels to, checked on the CPU (no GPU, no
library): they hold for correct arithmetic -- the f32 / bf16 emulation of each kernel stays inside them at every case the GPU file runs -- and
they bite -- every deliberately wrong oracle (tests/stage_oracles.py, `mutate=`) leaves twice the band on at least a tenth of the elements."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import stage_oracles as SO  # noqa: E402

TEETH = 0.10          # share of elements a mutation must move out of TWICE the tolerance


def _norm_rope_args(cfg):
    d, nq, nk, mp, B, T = cfg
    i = SO.head_inputs(cfg)
    cos, sin = SO.rotary_tables(d)
    return (i["qkv"], B, T, nq, nk, d, i["qw"], i["qb"], i["kw"], i["kb"], cos, sin), i["pos"]


def _pairs_args(cfg, table):
    d, nq, nk, mp, B, T = cfg
    i = SO.head_inputs(cfg)
    freqs = SO.pair_tables(d)[table]
    return (i["qkv"], B, T, nq, nk, d, freqs), SO.pair_positions(i["pos"], table, freqs.shape[0])


def _applicable(mutations):
    """(config, mutation) pairs: 'shard' needs a second shard (mp >= 2), 'shared_pos' a second batch row"""
    return [pytest.param(c, m, id=f"{c}-{m}") for c in SO.HEAD_CONFIGS for m in mutations
            if not (m == "shard" and c[3] < 2) and not (m == "shared_pos" and c[4] < 2)]


# ----------------------------------------------------------------------------- the bounds hold for correct arithmetic
def test_rmsnorm_emulation_stays_inside_the_bound():
    """Every (H, M) the GPU file runs: the emulation's worst |emulated - f64| / tol is 0.926 (H = 11008, M = 5; 0.33 at H = 8, 0.87 from
    H = 2048 on: the more elements, the nearer some pair of roundings comes to two half ulps); the all-zero row gives exact zeros."""
    worst = 0.0
    for H in SO.RMS_H:
        for M in SO.RMS_M:
            x, w = SO.rmsnorm_case(H, M)
            ref = SO.rmsnorm_ref(x, w, SO.RMS_EPS)
            emu = SO.rmsnorm_emulated(x, w, SO.RMS_EPS)
            r = SO.worst_ratio(emu, ref, SO.rmsnorm_tol(ref))
            print(f"rmsnorm emulated H={H} M={M}: {r:.3f}")
            worst = max(worst, r)
            if M == 5:
                assert bool((emu[2] == 0).all()) and bool((ref[2] == 0).all())
    print(f"rmsnorm emulated worst: {worst:.3f}")
    assert 0.5 < worst <= 1.0          # inside, and not by a margin that would make the bound vacuous


@pytest.mark.parametrize("cfg", SO.HEAD_CONFIGS, ids=str)
def test_qk_norm_rope_emulation_stays_inside_the_bound(cfg):
    """Worst |emulated - f64| / tol over q and k: 0.592, 0.554, 0.760 for the three configs (six roundings rarely all push one way); v is the input."""
    args, pos = _norm_rope_args(cfg)
    q, k, v, aux = SO.qk_norm_rope_ref(*args, pos)
    eq, ek, ev = SO.qk_norm_rope_emulated(*args, pos)
    rq, rk = SO.worst_ratio(eq, q, SO.qk_norm_rope_tol(q, aux["q"])), SO.worst_ratio(ek, k, SO.qk_norm_rope_tol(k, aux["k"]))
    print(f"qk_norm_rope emulated {cfg}: q {rq:.3f} k {rk:.3f}")
    assert 0.3 < max(rq, rk) <= 1.0
    assert torch.equal(ev, v) and v.dtype == torch.bfloat16


@pytest.mark.parametrize("table", ["grid", "random"])
@pytest.mark.parametrize("cfg", SO.HEAD_CONFIGS, ids=str)
def test_qk_rope_pairs_emulation_stays_inside_the_bound(cfg, table):
    """Worst |emulated - f64| / tol over q and k, the three configs and both tables: 0.890 (one rounding: at most 1 / 1.1 = 0.909)."""
    args, pos = _pairs_args(cfg, table)
    d, nq, nk = cfg[:3]
    q, k, v = SO.qk_rope_pairs_ref(*args, pos)
    eq, ek, ev = SO.qk_rope_pairs_emulated(*args, pos)
    xq, xk, _ = (t.permute(0, 2, 1, 3) for t in SO._split_heads(args[0], cfg[4], cfg[5], nq, nk, d))
    rq, rk = SO.worst_ratio(eq, q, SO.qk_rope_pairs_tol(q, xq)), SO.worst_ratio(ek, k, SO.qk_rope_pairs_tol(k, xk))
    print(f"qk_rope_pairs emulated {cfg} {table}: q {rq:.3f} k {rk:.3f}")
    assert 0.5 < max(rq, rk) <= 1.0
    assert torch.equal(ev, v)


@pytest.mark.parametrize("epilogue", ["plain", "bias", "residual", "bias_residual"])
@pytest.mark.parametrize("shape", SO.SPLITK_SMALL + SO.SPLITK_7B, ids=str)
def test_splitk_emulation_stays_inside_the_bound(shape, epilogue):
    """K <= 1024: worst |emulated - f64| / tol 0.983 ((32, 48, 33, 3) with bias: at small K the band is the roundings alone; 0.78 at K = 1024).
    The two 7B shapes are held to 2e-2 * max|want|, the project's convention for its GEMMs: the emulation uses 0.19 of that."""
    M, K, N, ksplit = shape
    x, w, b, res = SO.splitk_case(M, K, N)
    b = b if "bias" in epilogue else None
    res = res if "residual" in epilogue else None
    lin, want = SO.splitk_ref(x, w, b, res)
    emu = SO.splitk_emulated(x, w, b, res)
    if K <= 1024:
        tol = SO.splitk_tol(x, w, lin, want, res)
        r = SO.worst_ratio(emu, want, tol)
        # the accumulation term: K^1.5 * 2^-23 * 2 / pi for unit-variance rows (2.5e-3 at K = 1024) against a lost k-step's 4 / sqrt(K) = 0.125
        assert float((tol - SO.U * lin.abs() - (SO.U * want.abs() if res is not None else 0.0)).max()) < 4e-3
    else:
        r = float((emu.double() - want).abs().max() / (2e-2 * want.abs().max()))
    print(f"splitk emulated {shape} {epilogue}: {r:.3f}")
    assert r <= 1.0


# ----------------------------------------------------------------------------- the bounds have teeth
@pytest.mark.parametrize("mutation", SO.RMS_MUTATIONS)
@pytest.mark.parametrize("H", [100, 4096])
def test_rmsnorm_bound_catches_the_mutation(H, mutation):
    """Share of elements outside twice the band (M = 5; the zero row, a fifth of the elements, cannot move): 'mean' 0.800 at both sizes,
    'no_weight' 0.776 (H = 100) and 0.766 (H = 4096)."""
    x, w = SO.rmsnorm_case(H, 5)
    ref = SO.rmsnorm_ref(x, w, SO.RMS_EPS)
    f = SO.frac_outside(SO.rmsnorm_ref(x, w, SO.RMS_EPS, mutate=mutation), ref, SO.rmsnorm_tol(ref))
    print(f"rmsnorm {mutation} H={H}: {f:.3f}")
    assert f >= TEETH


@pytest.mark.parametrize("cfg,mutation", _applicable(SO.NORM_ROPE_MUTATIONS))
def test_qk_norm_rope_bound_catches_the_mutation(cfg, mutation):
    """Share of q and of k elements each mutation moves out of twice the band, lowest of the three configs: 'sign' 0.585, 'pairs' 0.557,
    'swap' 0.959, 'pos' 0.223 (the slow frequencies barely turn in one position), 'shard' 0.933, 'shared_pos' 0.398."""
    args, pos = _norm_rope_args(cfg)
    q, k, v, aux = SO.qk_norm_rope_ref(*args, pos)
    mq, mk, mv, _ = SO.qk_norm_rope_ref(*args, pos, mutate=mutation)
    fq, fk = SO.frac_outside(mq, q, SO.qk_norm_rope_tol(q, aux["q"])), SO.frac_outside(mk, k, SO.qk_norm_rope_tol(k, aux["k"]))
    print(f"qk_norm_rope {mutation} {cfg}: q {fq:.3f} k {fk:.3f}")
    assert fq >= TEETH and fk >= TEETH
    assert torch.equal(mv, v)


@pytest.mark.parametrize("table", ["grid", "random"])
@pytest.mark.parametrize("cfg,mutation", _applicable(SO.ROPE_PAIRS_MUTATIONS))
def test_qk_rope_pairs_bound_catches_the_mutation(cfg, mutation, table):
    """Share of q and of k elements each mutation moves out of twice the band, lowest of the three configs -- 2-D grid table / random table:
    'sign' 0.503 / 0.989, 'halves' 0.490 / 0.983, 'swap' 0.990 / 0.986, 'pos' 0.273 / 0.660, 'shared_pos' 0.302 / 0.498."""
    args, pos = _pairs_args(cfg, table)
    d, nq, nk = cfg[:3]
    q, k, v = SO.qk_rope_pairs_ref(*args, pos)
    mq, mk, _ = SO.qk_rope_pairs_ref(*args, pos, mutate=mutation)
    xq, xk, _ = (t.permute(0, 2, 1, 3) for t in SO._split_heads(args[0], cfg[4], cfg[5], nq, nk, d))
    fq, fk = SO.frac_outside(mq, q, SO.qk_rope_pairs_tol(q, xq)), SO.frac_outside(mk, k, SO.qk_rope_pairs_tol(k, xk))
    print(f"qk_rope_pairs {mutation} {cfg} {table}: q {fq:.3f} k {fk:.3f}")
    assert fq >= TEETH and fk >= TEETH


@pytest.mark.parametrize("epilogue", ["plain", "bias_residual"])
@pytest.mark.parametrize("shape", SO.SPLITK_SMALL, ids=str)
def test_splitk_bound_catches_a_lost_kstep(shape, epilogue):
    """The f64 product with the 16-wide k-step at the seam of the middle K slice zeroed leaves the bound on at least one element of EVERY output row."""
    M, K, N, ksplit = shape
    x, w, b, res = SO.splitk_case(M, K, N)
    b, res = (b, res) if epilogue == "bias_residual" else (None, None)
    lin, want = SO.splitk_ref(x, w, b, res)
    _, lost = SO.splitk_ref(x, w, b, res, drop_kstep=SO.splitk_seam(K, ksplit or SO.splitk_auto(N)))
    outside = (lost - want).abs() > SO.splitk_tol(x, w, lin, want, res)
    print(f"splitk lost k-step {shape} {epilogue}: rows caught {int(outside.any(1).sum())}/{M}, elements {float(outside.double().mean()):.3f}")
    assert bool(outside.any(dim=1).all())


# ----------------------------------------------------------------------------- the oracles against the layer's torch path
@pytest.mark.parametrize("cfg", SO.HEAD_CONFIGS, ids=str)
def test_qk_norm_rope_oracle_matches_the_layers_torch_path(cfg):
    """The f32 oracle against the formulas of decoder_layer.Attention.forward (HeadLayerNorm, cos / sin gathered by position, _rotate_half)."""
    from lantern_amd.drafters.decoder_layer import HeadLayerNorm, _rotate_half
    d, nq, nk, mp, B, T = cfg
    args, pos = _norm_rope_args(cfg)
    qkv, qw, qb, kw, kb, cos, sin = (t.float() for t in (args[0],) + args[6:])
    got = SO.qk_norm_rope_ref(qkv, B, T, nq, nk, d, qw, qb, kw, kb, cos, sin, pos, dtype=torch.float32)
    x = qkv.reshape(B * T, nq + 2 * nk, d)
    want = []
    for heads, lo, w, b in ((nq, 0, qw, qb), (nk, nq, kw, kb)):
        norm = HeadLayerNorm(d, mp, heads // mp)
        norm.load_state_dict(dict(weight=w, bias=b))
        with torch.no_grad():
            n = norm(x[:, lo:lo + heads]).reshape(B, T, heads, d).transpose(1, 2)
        c, s = cos[pos].unsqueeze(1), sin[pos].unsqueeze(1)
        want.append(n * c + _rotate_half(n) * s)
    want.append(x[:, nq + nk:].reshape(B, T, nk, d).transpose(1, 2))
    for g, wnt in zip(got[:3], want):
        torch.testing.assert_close(g, wnt, rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("cfg", SO.HEAD_CONFIGS, ids=str)
def test_qk_rope_pairs_oracle_matches_the_layers_torch_path(cfg):
    """The f32 oracle against decoder_layer.apply_rotary_pairs (one batch row at a time: it takes the gathered [T, d/2, 2] rows)."""
    from lantern_amd.drafters.decoder_layer import apply_rotary_pairs
    d, nq, nk, mp, B, T = cfg
    args, pos = _pairs_args(cfg, "random")
    qkv, freqs = args[0].float(), args[6]
    q, k, v = SO.qk_rope_pairs_ref(qkv, B, T, nq, nk, d, freqs, pos, dtype=torch.float32)
    xq, xk, _ = SO._split_heads(qkv, B, T, nq, nk, d)
    for b in range(B):
        torch.testing.assert_close(q[b], apply_rotary_pairs(xq[b:b + 1], freqs[pos[b]])[0].transpose(0, 1), rtol=2e-5, atol=2e-5)
        torch.testing.assert_close(k[b], apply_rotary_pairs(xk[b:b + 1], freqs[pos[b]])[0].transpose(0, 1), rtol=2e-5, atol=2e-5)


def test_positions_are_clamped_and_a_shared_row_is_expanded():
    """[T] positions equal their [B, T] expansion; positions beyond either end of the table equal the ends."""
    cfg = SO.HEAD_CONFIGS[0]
    d, nq, nk, mp, B, T = cfg
    args, pos = _norm_rope_args(cfg)
    a = SO.qk_norm_rope_ref(*args, pos[0])
    b = SO.qk_norm_rope_ref(*args, pos[0].expand(B, T))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    far = pos.clone()
    far[0, 0], far[-1, -1] = -3, SO.TABLE_ROWS + 7
    c, e = SO.qk_norm_rope_ref(*args, far), SO.qk_norm_rope_ref(*args, pos)
    assert torch.equal(c[0], e[0]) and torch.equal(c[1], e[1])


# ----------------------------------------------------------------------------- what the layer tests can see of a head-stage error
def test_what_the_layer_tests_see_of_a_flipped_rotate_half():
    """Computed here on the CPU from tests/golden/layer.npz and the f64 oracle (which reproduces the recorded k0 at 2e-5), on the `hd128` case's own
    first-call inputs and positions 0 .. 8: the 'sign' mutation moves k by at most 7.05 -- far outside test_drafter_layer.py's 4e-2 + 4e-2 |k| band,
    so the layer tests DO see a flipped rotate_half, through the fast frequencies.  What they cannot see is most of head_dim: 66% of k's elements stay
    inside that band under 'sign' and 76% under 'pos' (max move 3.24), where the derived bound puts 42% and 34% outside TWICE its width."""
    import test_drafter_layer as TL
    layer = TL.build("hd128", "cpu", torch.float32)
    at = layer.self_attn
    x0, pos0 = TL.g("hd128", "x0", "cpu"), TL.g("hd128", "pos0", "cpu")
    B, T, _ = x0.shape
    with torch.no_grad():
        xn = layer.input_layernorm(x0)
        qkv = torch.cat([at.q_proj(xn), at.k_proj(xn), at.v_proj(xn)], dim=-1).reshape(B * T, -1).double()
    d, nq, nk = at.head_dim, at.num_heads, at.num_key_value_heads
    assert d == 128
    args = (qkv, B, T, nq, nk, d, *(t.detach().double() for t in (at.q_norm.weight, at.q_norm.bias, at.k_norm.weight, at.k_norm.bias)),
            at.rotary_emb.cos_cached.double(), at.rotary_emb.sin_cached.double(), pos0)
    _, k, _, aux = SO.qk_norm_rope_ref(*args)
    np.testing.assert_allclose(k.numpy(), TL.GOLD["hd128.k0"], rtol=2e-5, atol=2e-5)          # the oracle IS the recorded layer's head stage
    band, tol = 4e-2 + 4e-2 * k.abs(), SO.qk_norm_rope_tol(k, aux["k"])
    for m in ("sign", "pos"):
        mk = SO.qk_norm_rope_ref(*args, mutate=m)[1]
        move, blind, caught = float((mk - k).abs().max()), 1.0 - SO.frac_outside(mk, k, band, 1.0), SO.frac_outside(mk, k, tol)
        print(f"hd128 golden positions, {m}: max |dk| {move:.3g}, inside the 4e-2 band {blind:.3f}, outside twice the derived bound {caught:.3f}")
        assert move > 4e-2 and blind > 0.5 and caught > 1.0 - blind
