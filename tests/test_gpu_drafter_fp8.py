"""GPU (-m gpu): FP8 (OCP e4m3fn, weight-only, one f32 scale per output row) weight streaming for the drafter's stream-K GEMMs.
  * the device pack is held against torch's own float8_e4m3fn conversion on the CPU, bit for bit;
  * on weights that ARE e4m3 codes times a power of two the fp8 kernel must return the bits of the bf16 packed kernel (same bricks, same wave -> brick
    assignment, same MFMA sequence; a scale of 2^j commutes with every f32 rounding) -- every epilogue, the input stage's gather form, the head's CFG form;
  * on arbitrary weights it meets the f64 product of the DEQUANTISED weights at the bf16 kernel's own tolerance (the quantisation error is not the
    kernel's: the reference holds the same quantised weights);
  * layers, the one-call depth, and what the feature promises end to end: greedy speculative decoding emits the target's tokens whatever the drafter
    proposes, so the fp8 drafter's stream equals the bf16 drafter's."""
import random
import types

import numpy as np
import pytest
import torch

import cases as CS
from lantern_amd import _lib, ops
from lantern_amd._lib import LanternError

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F8 = torch.float8_e4m3fn


def _deq(q):          # uint8 codes -> f32 values
    return q.view(F8).float()


def _cpu_quant(W):
    """The format's definition, on the CPU with torch's conversion: s = max|row| / 448 (1 for a zero row), q = e4m3fn_rne(f32(W) / s)."""
    Wf = W.detach().float().cpu()
    s = Wf.abs().amax(dim=1) / 448.0
    s[s == 0] = 1.0
    return (Wf / s[:, None]).to(F8).view(torch.uint8), s


# ----------------------------------------------------------------------------------------------------------------- 2. pack
@pytest.mark.parametrize("N,K,pair", [(33, 64, 0), (1, 64, 0), (96, 512, 48), (70, 832, 35), (1000, 1024, 0)])
def test_fp8_pack_is_bit_exact_against_torchs_conversion(N, K, pair):
    """Codes compare as dequantised values (so +0 / -0 do not matter), scales bit for bit.  Rows on purpose: all zero; holding +max and -max; one large
    entry over entries that land in e4m3's subnormal range (|q| < 2^-6) and below half its smallest subnormal (-> 0)."""
    g = torch.Generator().manual_seed(N * 7 + K)
    W = torch.randn(N, K, generator=g) * torch.logspace(-3, 2, N)[:, None]
    if N > 4:
        W[1] = 0.0
        W[2, 5], W[2, 9] = W[2].abs().max() * 2, -W[2].abs().max() * 2
        W[3] = torch.randn(K, generator=g) * 3e-5
        W[3, 7] = 1.0          # s = 1 / 448: entries of 3e-5 become |q| ~ 0.013 (subnormal), many below 2^-10 (-> 0)
        W[N - 1] = torch.randn(K, generator=g) * 1e-6
        W[N - 1, 0] = -2.0
    W = W.to(BF)
    pk = ops.pack_linear_weight(W.cuda(), pair_rows=pair, fmt="fp8")
    assert pk.fmt == "fp8" and pk.code == 2 and pk.K == K and pk.n_rows == (pair or N) and pk.data.dtype == torch.uint8
    assert pk.data.numel() == int(_lib.lib().lantern_pack_linear_weight_fp8_bytes(pk.n_rows, K, pair))
    q, s = ops.unpack_linear_weight_fp8(pk)
    assert q.shape == (N, K) and q.dtype == torch.uint8 and s.shape == (N,) and s.dtype == torch.float32
    q_want, s_want = _cpu_quant(W)
    assert torch.equal(s.cpu().view(torch.int32), s_want.view(torch.int32))
    got, want = _deq(q.cpu()), _deq(q_want)
    assert bool(torch.isfinite(got).all())          # no NaN code
    assert torch.equal(got, want), (got - want).abs().max()
    if N > 4:
        assert float(s[1]) == 1.0 and not bool(q[1].cpu().bitwise_and(0x7f).any())
        assert (got[3] != 0).sum() > 1 and ((got[3].abs() > 0) & (got[3].abs() < 2.0 ** -6)).any()          # the subnormal range is really used


# ----------------------------------------------------------------------------------------------------------------- 3. bit-exact GEMM
def _code_weight(rows, K, gen):
    """W = q * 2^j per row, q drawn from the finite e4m3 codes without 0x80 (-0), one |q| = 448 per row: exact in bf16, and the pack recovers (q, 2^j)."""
    codes = torch.tensor([c for c in range(256) if (c & 0x7f) != 0x7f and c != 0x80], dtype=torch.uint8)
    q = codes[torch.randint(0, codes.numel(), (rows, K), generator=gen)]
    q[torch.arange(rows), torch.randint(0, K, (rows,), generator=gen)] = torch.where(torch.rand(rows, generator=gen) < 0.5, 0x7e, 0xfe).to(torch.uint8)
    s = torch.pow(2.0, torch.randint(-12, 4, (rows,), generator=gen).float())
    W = _deq(q) * s[:, None]
    assert torch.equal(W.to(BF).float(), W)
    return W.to(BF).cuda(), q, s


GEMM_SHAPES = [(1, 512, 96, 0), (32, 320, 40, 1), (7, 1024, 1000, 2), (32, 64, 33, 0), (9, 832, 70, 2), (32, 64, 1, 1), (20, 16384, 64, 0), (20, 4096, 4096, 1)]


def _gemm_inputs(M, K, N, epi, gen):
    dev = torch.device("cuda")
    x = torch.randn(M, K, generator=gen).to(BF).to(dev)
    b = (0.1 * torch.randn(2 * N if epi == 2 else N, generator=gen)).to(BF).to(dev)
    res = torch.randn(M, N, generator=gen).to(BF).to(dev)
    kw = dict(residual=res) if epi == 1 else {}
    return x, b, res, kw


@pytest.fixture
def whole_tiles_off():
    """Small matrices get whole tiles per workgroup by default (no partial tiles): with the rule off, the (tile, K) space is cut into equal shares and
    several workgroups meet in the workspace on every tile."""
    before = _lib.get_tuning("sk_whole_mb")
    _lib.set_tuning("sk_whole_mb", 0)
    yield
    _lib.set_tuning("sk_whole_mb", before)


def _bit_exact_gemm(M, K, N, epi):
    gen = torch.Generator().manual_seed(M * 131 + K + N + epi)
    rows = 2 * N if epi == 2 else N
    W, q, s = _code_weight(rows, K, gen)
    x, b, res, kw = _gemm_inputs(M, K, N, epi, gen)
    pair = N if epi == 2 else 0
    p16, p8 = ops.pack_linear_weight(W, pair), ops.pack_linear_weight(W, pair, fmt="fp8")
    q_got, s_got = ops.unpack_linear_weight_fp8(p8)
    assert torch.equal(_deq(q_got.cpu()), _deq(q)) and torch.equal(s_got.cpu(), s)
    want = ops.linear_rows_streamk(x, p16, epi, bias=b, **kw)
    got = ops.linear_rows_streamk(x, p8, epi, bias=b, **kw)
    again = ops.linear_rows_streamk(x, p8, epi, bias=b, **kw)          # same workspace: the counters came back to zero
    assert got.shape == (M, N) and torch.equal(got, want), (got.float() - want.float()).abs().max()
    assert torch.equal(again, got)


@pytest.mark.parametrize("M,K,N,epi", GEMM_SHAPES)
def test_fp8_gemm_is_bit_exact_against_the_bf16_kernel_on_power_of_two_scales(M, K, N, epi):
    _bit_exact_gemm(M, K, N, epi)


@pytest.mark.parametrize("M,K,N,epi", [(20, 16384, 64, 0), (9, 832, 70, 2), (7, 1024, 1000, 2), (32, 320, 40, 1)])
def test_fp8_gemm_is_bit_exact_when_workgroups_share_tiles(M, K, N, epi, whole_tiles_off):
    """The workspace path: 2 tiles x 64 K chunks over 128 workgroups for (20, 16384, 64) -- every output is the sum of partial tiles."""
    _bit_exact_gemm(M, K, N, epi)


@pytest.mark.parametrize("embed_scale", [1.0, 8.0])
def test_fp8_input_stage_is_bit_exact(embed_scale):
    """drafter_fc (the GATHER form: embedding rows scaled and re-rounded in the A fragment), 20 rows and a 70-row prefill in 32-row blocks."""
    H, vocab = 128, 512
    gen = torch.Generator().manual_seed(int(embed_scale) + 3)
    W, _, _ = _code_weight(H, 2 * H, gen)
    embed = torch.randn(vocab, H, generator=gen).to(BF).cuda()
    bias = (0.1 * torch.randn(H, generator=gen)).to(BF).cuda()
    p16, p8 = ops.pack_linear_weight(W), ops.pack_linear_weight(W, fmt="fp8")
    for M in (20, 70):
        ids = torch.randint(0, vocab, (M,), generator=gen).cuda()
        hid = torch.randn(M, H, generator=gen).to(BF).cuda()
        got = ops.drafter_fc(ids, hid, embed, W, bias, embed_scale=embed_scale, packed=p8)
        want = torch.cat([ops.drafter_fc(ids[m:m + 32], hid[m:m + 32], embed, W, bias, embed_scale=embed_scale, packed=p16) for m in range(0, M, 32)])
        assert got.shape == (M, H) and torch.equal(got, want)


def test_fp8_head_cfg_epilogue_is_bit_exact():
    """The head's window GEMM with the CFG epilogue (both rows scaled before its bf16 steps): head_expand's top-k lists and head_sample's distributions
    (injected draws) equal the bf16 packed weight's, bit for bit."""
    V, K, n, k = 1024, 256, 5, 10
    gen = torch.Generator().manual_seed(11)
    W, _, _ = _code_weight(V, K, gen)
    W = (W.float() * 2.0 ** -8).to(BF)          # (still codes times powers of two; logits of a few units: a softmax with more than one live entry)
    A = (0.5 * torch.randn(2 * n, K, generator=gen)).to(BF).cuda()
    bias = (0.1 * torch.randn(V, generator=gen)).to(BF).cuda()
    p16, p8 = ops.pack_linear_weight(W), ops.pack_linear_weight(W, fmt="fp8")
    scores = torch.randn(n, generator=gen).cuda()
    e16 = ops.head_expand(A, W, 0, V, 3.0, bias=bias, model=ops.MODEL_PLAIN, top_k_filter=300, scores_in=scores, top_k=k, packed=p16)
    e8 = ops.head_expand(A, W, 0, V, 3.0, bias=bias, model=ops.MODEL_PLAIN, top_k_filter=300, scores_in=scores, top_k=k, packed=p8)
    for a, b in zip(e16, e8):
        assert torch.equal(a, b)
    inj = torch.stack([torch.randperm(V, generator=gen)[:k] for _ in range(n)]).cuda()
    s16 = ops.head_sample(A, W, 0, V, 3.0, bias=bias, model=ops.MODEL_PLAIN, top_k_filter=300, n_draw=k, draw_idx=inj, packed=p16)
    s8 = ops.head_sample(A, W, 0, V, 3.0, bias=bias, model=ops.MODEL_PLAIN, top_k_filter=300, n_draw=k, draw_idx=inj, packed=p8)
    for a, b in zip(s16, s8):
        assert torch.equal(a, b)
    assert torch.equal(s8[1], inj)


# ----------------------------------------------------------------------------------------------------------------- 4. / 5. f64
def _f64_reference(x, q, s, b, res, N, epi):
    xd, wd, bd = x.double().cpu(), _deq(q).double() * s.double()[:, None], b.double().cpu()
    if epi == 0:
        return xd @ wd.T + bd
    if epi == 1:
        return (xd @ wd.T + bd) + res.double().cpu()
    gate, up = xd @ wd[:N].T + bd[:N], xd @ wd[N:].T + bd[N:]
    return torch.nn.functional.silu(gate) * up


@pytest.mark.parametrize("M,K,N,epi", GEMM_SHAPES)
def test_fp8_gemm_matches_f64_on_arbitrary_scales(M, K, N, epi):
    """W ~ N(0, 1 / K) as in test_streamk_gemm_matches_f64_and_the_per_tile_kernels, the reference on the dequantised weights (exact there), that test's
    tolerance: 2e-2 of the row scale -- bf16 activations, f32 accumulation in another order, bf16 output roundings."""
    gen = torch.Generator().manual_seed(M * 131 + K + N + epi + 1)
    rows = 2 * N if epi == 2 else N
    W = (torch.randn(rows, K, generator=gen) / K ** 0.5).to(BF).cuda()
    x, b, res, kw = _gemm_inputs(M, K, N, epi, gen)
    p8 = ops.pack_linear_weight(W, N if epi == 2 else 0, fmt="fp8")
    q, s = ops.unpack_linear_weight_fp8(p8)
    want = _f64_reference(x, q.cpu(), s.cpu(), b, res, N, epi)
    scale = want.abs().max().item()
    for _ in range(2):
        got = ops.linear_rows_streamk(x, p8, epi, bias=b, **kw)
        err = (got.double().cpu() - want).abs().max().item()
        print(f"fp8 gemm {(M, K, N, epi)}: max err {err:.3e} of scale {scale:.3e}")
        assert got.shape == (M, N) and err <= 2e-2 * scale


@pytest.mark.parametrize("K,N,epi", [(512, 96, 0), (320, 40, 1), (832, 70, 2)])
def test_fp8_more_than_32_rows_go_in_blocks_through_the_streamk_kernel(K, N, epi, monkeypatch):
    """ops.linear_rows_packed (the prefill path) on an fp8 weight: 70 rows = the concatenation of the <= 32-row stream-K calls, within the f64 bound."""
    M = 70
    gen = torch.Generator().manual_seed(K + N + epi)
    rows = 2 * N if epi == 2 else N
    W = (torch.randn(rows, K, generator=gen) / K ** 0.5).to(BF).cuda()
    x, b, res, kw = _gemm_inputs(M, K, N, epi, gen)
    p8 = ops.pack_linear_weight(W, N if epi == 2 else 0, fmt="fp8")
    parts = [ops.linear_rows_streamk(x[m:m + 32], p8, epi, bias=b, **({"residual": res[m:m + 32]} if epi == 1 else {})) for m in range(0, M, 32)]
    calls = []
    real = ops.linear_rows_streamk
    monkeypatch.setattr(ops, "linear_rows_streamk", lambda *a, **k_: (calls.append(a[0].shape[0]), real(*a, **k_))[1])
    got = ops.linear_rows_packed(x, p8, epi, bias=b, **kw)
    assert calls == [32, 32, 6] and got.shape == (M, N) and torch.equal(got, torch.cat(parts))
    q, s = ops.unpack_linear_weight_fp8(p8)
    want = _f64_reference(x, q.cpu(), s.cpu(), b, res, N, epi)
    assert (got.double().cpu() - want).abs().max().item() <= 2e-2 * want.abs().max().item()


# ----------------------------------------------------------------------------------------------------------------- 6. layers, one-call depth
def _dequantised_f32_copy(layer_bf16, builder, name, dev):
    """The same layer in f32 on torch's ops (fused = False) with every nn.Linear weight replaced by its dequantised value q * s."""
    ref = builder(name, dev, torch.float32)
    ref.load_state_dict({k: v.float() for k, v in layer_bf16.state_dict().items()})
    for m in ref.modules():
        if isinstance(m, torch.nn.Linear):
            q, s = _cpu_quant(m.weight.data)
            m.weight.data = (_deq(q) * s[:, None]).to(dev)
    ref.fused = False
    return ref


@pytest.mark.parametrize("name", ["hd128", "hd64_gqa", "an_hd128", "an_hd64", "lg_hd128", "lg_hd64", "lg_hd64_idx1"])
def test_layers_run_with_fp8_weights(name, monkeypatch):
    """DecoderLayer (Lumina / Anole fixtures) and LlamaDecoderLayer with weight_format = "fp8" on the fixture weights and inputs (a 2 x 9 call, then a
    2 x 5 call behind its cache) against the layer's own torch composition in f32 on the dequantised weights, at the tolerance tests/test_drafter_layer.py
    uses for the fused bf16 layer against its f32 golden (rtol = atol = 4e-2: bf16 activations and per-projection bf16 roundings on one side only)."""
    import test_drafter_layer as TL
    dev = torch.device("cuda")
    lg, an = name.startswith("lg_"), name.startswith("an_")
    builder, gg = (TL.build_lg, TL.gl) if lg else ((TL.build_an, TL.gl) if an else (TL.build, TL.g))
    layer = builder(name, dev, BF)
    assert layer.weight_format == "bf16"
    calls = []
    real = ops.linear_rows_streamk
    monkeypatch.setattr(ops, "linear_rows_streamk", lambda A, w, *a, **k_: (calls.append(getattr(w, "fmt", None)), real(A, w, *a, **k_))[1])
    kw0 = dict(freqs_cis=gg(name, "f0", dev)) if lg else {}
    kw1 = dict(freqs_cis=gg(name, "f1", dev)) if lg else {}
    with torch.no_grad():
        layer(gg(name, "x0", dev, BF), attention_mask=gg(name, "m0", dev), position_ids=gg(name, "pos0", dev), use_cache=True, **kw0)
        assert calls == ["bf16"] * 4 and len(layer._packed_weights) == 4
        layer.weight_format = "fp8"
        assert "_packed_weights" not in layer.__dict__          # changing the format drops the packed copies
        calls.clear()
        y0, kv0 = layer(gg(name, "x0", dev, BF), attention_mask=gg(name, "m0", dev), position_ids=gg(name, "pos0", dev), use_cache=True, **kw0)
        y1, kv1 = layer(gg(name, "x1", dev, BF), attention_mask=gg(name, "m1", dev), position_ids=gg(name, "pos1", dev), past_key_value=kv0, use_cache=True, **kw1)
        assert calls == ["fp8"] * 8
        ref = _dequantised_f32_copy(layer, builder, name, dev)
        f32 = lambda key: gg(name, key, dev, BF).float()          # (the bf16 inputs the fp8 layer saw)
        r0, rkv0 = ref(f32("x0"), attention_mask=gg(name, "m0", dev), position_ids=gg(name, "pos0", dev), use_cache=True, **kw0)
        r1, rkv1 = ref(f32("x1"), attention_mask=gg(name, "m1", dev), position_ids=gg(name, "pos1", dev), past_key_value=rkv0, use_cache=True, **kw1)
    for got, want in ((y0, r0), (y1, r1), (kv1[0], rkv1[0]), (kv1[1], rkv1[1])):
        np.testing.assert_allclose(got.float().cpu().numpy(), want.float().cpu().numpy(), rtol=4e-2, atol=4e-2)
    with pytest.raises(ValueError):
        layer.weight_format = "int8"


def _drafter(model_type, V, H, heads, depth=4, seed=11):
    cfg = types.SimpleNamespace(vocab_size=V, hidden_size=H, pad_token_id=None, num_hidden_layers=1, num_attention_heads=heads, num_key_value_heads=heads,
                                intermediate_size=2 * H, max_position_embeddings=512, rms_norm_eps=1e-5, model_parallel_size=1, input_type="t2i")
    from lantern_amd.drafters import cnets
    torch.manual_seed(seed)
    return cnets.Model(cfg, total_tokens=40, depth=depth, top_k=CS.TOPK, model_type=model_type).to("cuda").to(BF)


@pytest.mark.parametrize("model_type,V,H,heads,depth", [("llamagen", 16384, 128, 2, 4), ("lumina_mgpt", 65536, 256, 2, 5)])
def test_fp8_depth_plan_equals_the_python_depth_loop(model_type, V, H, heads, depth, monkeypatch):
    """lantern_draft_depth with fc_packed = layer_packed = head_packed = 2 against the per-kernel module path on the same fp8 weights: the same drafted
    tree over two consecutive drafting calls (the comparison tests/test_gpu_drafter.py makes for bf16)."""
    from transformers.generation.logits_process import LogitsProcessorList, TopKLogitsWarper
    from lantern_amd.drafters import cnets
    dev = torch.device("cuda")
    mdl = _drafter(model_type, V, H, heads, depth)
    mdl.init_tree()
    assert mdl.set_weight_format("fp8") is mdl and mdl.weight_format == "fp8" and mdl.layers[0].weight_format == "fp8"
    head = torch.nn.Linear(H, V, bias=False).to(dev).to(BF)
    proc = LogitsProcessorList([TopKLogitsWarper(300)])
    lum = [None, types.SimpleNamespace(image_top_k=300)]
    codes = []
    orig_run = cnets.DraftPlan.run
    monkeypatch.setattr(cnets.DraftPlan, "run", lambda self, i: (codes.append((self.args.fc_packed, self.args.layer_packed, self.args.head_packed)), orig_run(self, i))[1])
    fmts = []
    for fn in ("linear_rows_streamk", "drafter_fc", "head_expand"):
        real = getattr(ops, fn)
        pick = (lambda a, k_: a[1]) if fn == "linear_rows_streamk" else (lambda a, k_: k_.get("packed"))
        monkeypatch.setattr(ops, fn, (lambda real, pick: (lambda *a, **k_: (fmts.append(getattr(pick(a, k_), "fmt", None)), real(*a, **k_))[1]))(real, pick))

    def run(plan_on):
        mdl.use_depth_plan = plan_on
        mdl.reset_kv()
        outs, total = [], 7
        g = torch.Generator(device="cuda").manual_seed(5)
        for c in range(2):
            n_new = total if c == 0 else 2
            hid = torch.randn(2, n_new, H, device=dev, dtype=BF, generator=g)
            ids = torch.randint(4, 8000, (2, total + 1), device=dev, generator=g)
            if model_type == "lumina_mgpt":
                am = torch.ones(2, total, dtype=torch.bool, device=dev)
                am[1, :2] = False
                out = mdl.topK_generate(hid[:1], hid[1:], ids[:1], head, lum, attention_mask=am, tree_type="dynamic")
            else:
                out = mdl.topK_genrate(hid, ids, head, proc, 3.0)
            outs.append([t.clone() for t in out])
            total += 2
        return outs
    py = run(False)
    assert fmts and set(fmts) == {"fp8"}, set(fmts)          # every GEMM of the module path read fp8 bricks: input stage, layer, head window
    pl = run(True)
    assert len(codes) == 2 * depth and set(codes) == {(2, 2, 2)}, codes
    for c, (a, b) in enumerate(zip(py, pl)):
        for x, y in zip(a, b):
            assert x.shape == y.shape and torch.equal(x, y), (c, x, y)
    mdl.set_weight_format("bf16")
    assert mdl.layers[0].weight_format == "bf16" and "_packed_weights" not in mdl.__dict__ and "_plan" not in mdl.__dict__


def test_fp8_static_plan_streams_fp8_at_every_level():
    """Static trees (StaticDraftPlan: lantern_head_sample for the root row, one lantern_draft_depth per level) on an fp8 drafter: every C call carries
    packed = 2 for the input stage, the layer and the head window; the levels' distributions are distributions over the image window, the draws distinct
    tokens with mass."""
    from lantern_amd.drafters import choices, cnets
    dev, V, H = torch.device("cuda"), 65536, 256
    mdl = _drafter("lumina_mgpt", V, H, 2, depth=4, seed=13).set_weight_format("fp8")
    mdl.init_tree(choices.mc_sim_7b_63)
    levels = [len(t) for t in mdl.tree_buffer["tree_indices"]]
    head = torch.nn.Linear(H, V, bias=False).to(dev).to(BF)
    lum = [None, types.SimpleNamespace(image_top_k=300)]
    g = torch.Generator(device="cuda").manual_seed(5)
    ug = torch.Generator(device="cuda").manual_seed(77)
    mdl.static_draw_uniforms = lambda R, kk: torch.rand((R, kk), dtype=torch.float64, device=dev, generator=ug)
    hid = torch.randn(2, 7, H, device=dev, dtype=BF, generator=g)
    ids = torch.randint(4, 8000, (2, 8), device=dev, generator=g)
    am = torch.ones(2, 7, dtype=torch.bool, device=dev)
    am[1, :2] = False
    tok, prob, ol = mdl.topK_generate(hid[:1], hid[1:], ids[:1], head, lum, attention_mask=am, tree_type="static")
    plan = mdl.__dict__["_splan"][1]
    assert isinstance(plan, cnets.StaticDraftPlan)
    assert (plan.args.fc_packed, plan.args.layer_packed, plan.args.head_packed) == (2, 2, 2)
    R, k = 1 + sum(levels), CS.TOPK
    full = torch.cat(ol)
    assert tok.shape == (R, k) and full.shape == (R, V)
    assert torch.allclose(full.sum(-1), torch.ones(R, device=dev), atol=1e-5) and float(full[:, :4].sum()) == 0.0 and float(full[:, 8197:8803].sum()) == 0.0 and float(full[:, 8804:].sum()) == 0.0
    assert (full.gather(1, tok) > 0).all() and all(len(set(r)) == k for r in tok.tolist())


# ----------------------------------------------------------------------------------------------------------------- 7. end to end
HT, HKV, DH, SMAX, MT = 128, 2, 32, 512, 97


class _Head:
    """Scripted lm_head (tests/test_gpu_generate.py): the logits row is looked up from the (token, position) digits the target writes into its hidden state."""

    def __init__(self, dev, V):
        g = torch.Generator(device="cpu").manual_seed(5)
        self.weight = torch.zeros(V, HT, device=dev, dtype=BF)
        self.table = (3.0 * torch.randn(MT, V, generator=g)).to(BF).to(dev)

    def __call__(self, hidden):
        tok, pos = _decode(hidden)
        return self.table[(tok * 7 + pos * 13) % MT]


def _decode(h):
    return (h[..., 0].float() + 128 * h[..., 2].float()).long(), (h[..., 1].float() + 128 * h[..., 3].float()).long()


class _Inner:
    """Scripted target: hidden state and K/V rows carry (token, position); LlamaGen's prefill comes as `cond_idx`."""

    def __init__(self, dev, n_layers=2):
        lin = types.SimpleNamespace(weight=torch.zeros(1, device=dev))
        self.layers = [types.SimpleNamespace(self_attn=types.SimpleNamespace(q_proj=lin)) for _ in range(n_layers)]
        self.tree_mask, self.tree_mode, self.dev = None, None, dev

    def __call__(self, cond_idx=None, input_ids=None, attention_mask=None, past_key_values=None, position_ids=None, **kw):
        if cond_idx is not None:
            B, T = cond_idx.shape[:2]
            input_ids = torch.zeros(B, T, dtype=torch.long, device=self.dev)
        B, T = input_ids.shape
        cur = int(past_key_values[0][0].current_length)
        if position_ids is None:
            position_ids = torch.arange(cur, cur + T, device=self.dev)[None].expand(B, T)
        position_ids = position_ids.reshape(-1, T).expand(B, T)
        hidden = torch.zeros(B, T, HT, device=self.dev, dtype=BF)
        hidden[..., 0] = (input_ids % 128).to(BF)
        hidden[..., 2] = (input_ids // 128).to(BF)
        hidden[..., 1] = (position_ids % 128).to(BF)
        hidden[..., 3] = (position_ids // 128).to(BF)
        kv = hidden[:, None, :, :DH].expand(B, HKV, T, DH).contiguous()
        for layer in past_key_values:
            for c in layer:
                c.cat(kv, dim=2)
        return (hidden,)


def _base(dev, V, llamagen):
    cfg = types.SimpleNamespace(num_hidden_layers=2, num_key_value_heads=HKV, max_position_embeddings=SMAX, hidden_size=HKV * DH, num_attention_heads=HKV)
    base = types.SimpleNamespace(model=_Inner(dev), lm_head=_Head(dev, V), config=cfg, dtype=BF)
    if llamagen:
        base.encode_prompt = lambda prompt, cfg_: (torch.zeros(2, 120, HT, device=dev, dtype=BF), None)
    return base


def test_greedy_decoding_emits_the_same_tokens_with_an_fp8_drafter():
    """Exact-match speculative decoding (greedy, LANTERN off) returns the target's greedy sequence whatever the drafter proposes: the LlamaGen mirror's
    token stream with drafter_weight_format = "fp8" equals the stream with "bf16", token for token; the accept lengths may differ (printed).  The
    drafter fits the HIP layer (hidden 128, head_dim 64): its input stage and its layer's four GEMMs really stream fp8 bricks."""
    from lantern_amd.ea_model_llamagen import EaModel
    dev, Vl = torch.device("cuda"), 4096
    g = torch.Generator(device="cpu").manual_seed(1)
    table = ops.build_vq_table(torch.randn(Vl, 8, generator=g).to(dev))
    streams, means, seen = {}, {}, {}
    real = ops.linear_rows_streamk
    for fmt in ("bf16", "fp8"):
        random.seed(7)
        torch.manual_seed(2)
        drafter = _drafter("llamagen", Vl, HT, 2, depth=4, seed=21)
        drafter.init_tree()
        ref = types.SimpleNamespace(base_model=_base(dev, Vl, True), ea_layer=drafter, nearest_latents=table)
        mdl = EaModel.from_reference(ref, drafter_weight_format=fmt)
        assert drafter.weight_format == fmt and drafter.layers[0].weight_format == fmt
        mdl.uniform_window = 256
        fm = seen[fmt] = set()
        ops.linear_rows_streamk = lambda A, w, *a, _fm=fm, **k_: (_fm.add(getattr(w, "fmt", "row-major")), real(A, w, *a, **k_))[1]
        try:
            tokens, mean_accept, _ = mdl.generate(prompt=["a photo"], max_length=40, temperature=0.0, top_k=300, top_p=1.0, cfg=4.0, lantern=False,
                                                  lantern_k=100, lantern_delta=0.2, static_tree=False)
        finally:
            ops.linear_rows_streamk = real
        streams[fmt], means[fmt] = tokens[0].tolist(), mean_accept
    print(f"mean accept length: bf16 drafter {means['bf16']:.3f}, fp8 drafter {means['fp8']:.3f}")
    assert seen["bf16"] == {"bf16"} and seen["fp8"] == {"fp8"}, seen
    assert len(streams["fp8"]) == 40 and streams["fp8"] == streams["bf16"]


def test_sampled_lumina_run_completes_with_an_fp8_drafter():
    """EaLumina_mGPT.eagenerate with sampling and LANTERN on top of an fp8 drafter (static tree: the accept test reads the drafter's own distributions):
    every step's status is 0 (a non-zero status raises), the emitted ids are image ids, and the target's K/V rows spell the emitted sequence."""
    from lantern_amd.drafters.choices import mc_sim_7b_63
    from lantern_amd.ea_model_lumina_mgpt import EaLumina_mGPT
    dev, V = torch.device("cuda"), 16384
    random.seed(4321)
    torch.manual_seed(1)
    drafter = _drafter("lumina_mgpt", V, HT, 2, depth=4, seed=22)
    g = torch.Generator(device="cpu").manual_seed(1)
    table = ops.build_vq_table(torch.randn(8192, 8, generator=g).to(dev))
    ref = types.SimpleNamespace(base_model=_base(dev, V, False), ea_layer=drafter, nearest_latents=table)
    mdl = EaLumina_mGPT.from_reference(ref, drafter_weight_format="fp8", cfg_mode="parallel", eagle_version=1)
    assert drafter.weight_format == "fp8"
    mdl.uniform_window = 256
    prompt = torch.randint(9000, 12000, (1, 7), device=dev)
    out_ids, accept = mdl.eagenerate(prompt, max_new_tokens=24, cfg_scale=3.0, top_k=200, lantern=True, lantern_k=100, lantern_delta=0.1, tree_choices=mc_sim_7b_63)
    ids = out_ids[0]
    L0 = prompt.shape[1] + 3
    assert ids.shape[0] == L0 + sum(accept) and sum(accept) >= 24 and all(1 <= a <= 7 for a in accept)
    new = ids[L0 + 1:]
    assert ((new >= 4) & (new < 8196) | (new == 8803) | (new == 8196)).all()
    data, n_valid = mdl.past_key_values_data[0], int(mdl.current_length_data[0])
    tok, pos = _decode(data[0, 0, 0, :n_valid].float())
    assert n_valid == ids.shape[0] and tok.tolist() == ids.tolist() and pos.tolist() == list(range(n_valid))
    assert {w.fmt for _, w, *_ in drafter.layers[0]._packed_weights.values()} == {"fp8"}


# ----------------------------------------------------------------------------------------------------------------- 8. refusals
def test_fp8_refusals():
    """packed = 2 with K % 64 != 0 has no kernel: LANTERN_E_UNSUPPORTED (-3) with a message, nothing launched; a CPU tensor or a non-bf16 source weight
    raises LanternError; so do a layer or drafter that cannot read fp8."""
    import ctypes as C
    L = _lib.lib()
    dev = torch.device("cuda")
    M, K, N = 4, 80, 32
    x = torch.zeros(M, K, dtype=BF, device=dev)
    w = torch.zeros(N * K + 4 * N, dtype=torch.uint8, device=dev)
    out = torch.zeros(M, N, dtype=BF, device=dev)
    ws = ops._sk_workspace(dev)
    rc = L.lantern_linear_rows_streamk(C.c_void_p(x.data_ptr()), C.c_void_p(w.data_ptr()), None, M, K, 0, N, C.c_void_p(out.data_ptr()), N, 0, 0, None, 0, 0, 2,
                                       C.c_void_p(ws.data_ptr()), C.c_size_t(ws.numel()), None)
    assert rc == -3 and b"K % 64" in L.lantern_last_error(), (rc, L.lantern_last_error())
    rc = L.lantern_pack_linear_weight_fp8(C.c_void_p(x.data_ptr()), N, K, 0, C.c_void_p(w.data_ptr()), None)
    assert rc == -3 and b"multiple of 64" in L.lantern_last_error()
    with pytest.raises(LanternError):
        ops.pack_linear_weight(torch.zeros(32, 64, dtype=BF), fmt="fp8")                       # a CPU tensor
    with pytest.raises(LanternError):
        ops.pack_linear_weight(torch.zeros(32, 64, dtype=torch.float16, device=dev), fmt="fp8")   # not bf16
    with pytest.raises(LanternError):
        ops.pack_linear_weight(torch.zeros(32, 80, dtype=BF, device=dev), fmt="fp8")              # K % 64
    with pytest.raises(LanternError):
        ops.unpack_linear_weight_fp8(ops.pack_linear_weight(torch.zeros(32, 64, dtype=BF, device=dev)))
    p8 = ops.pack_linear_weight(torch.zeros(32, 64, dtype=BF, device=dev), fmt="fp8")
    with pytest.raises(LanternError):
        ops.linear_rows_streamk(torch.zeros(4, 128, dtype=BF, device=dev), p8)                    # K of the call != K of the weight
    with pytest.raises(LanternError, match="drafter"):
        from lantern_amd.verify import MirrorBase
        m = MirrorBase()
        m.ea_layer = types.SimpleNamespace()
        m.set_drafter_weight_format("fp8")                                                        # a drafter that is not this package's
