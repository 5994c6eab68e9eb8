"""GPU (-m gpu): FP8 (e4m3fn, one f32 scale per output row) drafter weights in the prompt prefill -- the tiled GEMM's fp8 instances
(lantern_linear_rows_packed_fmt) and the input stage's gather form on the packed weight (lantern_drafter_fc_packed).
  * on weights that ARE e4m3 codes times a power of two per row the fp8 tiled kernel returns the bits of the bf16 tiled kernel: same bricks, same MFMA
    sequence, and a 2^j scale commutes with the f32 roundings;
  * on arbitrary weights it meets the f64 product of the DEQUANTISED weights at the bound the stream-K fp8 and the bf16 kernels are held to on the same
    inputs (2e-2 of max |reference|);
  * routing: from "gemm_tiled_from" rows (129) an fp8 weight takes one tiled launch, below that the 32-row stream-K blocks as before; the C entry itself
    runs the tiled fp8 kernel at any row count;
  * the gather form is the same kernel with another A addressing: bit-equal to the plain GEMM on the concatenated rows;
  * layers of both families and cnets.Model on a 2 x 80 prefill.
The constructions (_code_weight, _gemm_inputs, _f64_reference) are those of tests/test_gpu_drafter_fp8.py."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import cases as CS
from lantern_amd import _lib, ops

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F8 = torch.float8_e4m3fn

# (M, K, N, epilogue): the smallest shapes that reach every edge of the tile loop -- a second row block of one row, one K block, a last tile one column
# wide, surplus tiles; an odd number of K blocks; a gate / up pair over 13 K blocks and three row blocks; ...
SHAPES = [(129, 64, 33, 0), (130, 192, 1, 1), (257, 832, 70, 2), (200, 320, 40, 1), (129, 1024, 1000, 2), (384, 512, 96, 0)]


def _deq(q):          # uint8 codes -> f32 values
    return q.view(F8).float()


def _cpu_quant(W):
    """The format's definition, on the CPU with torch's conversion: s = max|row| / 448 (1 for a zero row), q = e4m3fn_rne(f32(W) / s)."""
    Wf = W.detach().float().cpu()
    s = Wf.abs().amax(dim=1) / 448.0
    s[s == 0] = 1.0
    return (Wf / s[:, None]).to(F8).view(torch.uint8), s


def _code_weight(rows, K, gen):
    """W = q * 2^j per row, q drawn from the finite e4m3 codes without 0x80 (-0), one |q| = 448 per row: exact in bf16, and the pack recovers (q, 2^j)."""
    codes = torch.tensor([c for c in range(256) if (c & 0x7f) != 0x7f and c != 0x80], dtype=torch.uint8)
    q = codes[torch.randint(0, codes.numel(), (rows, K), generator=gen)]
    q[torch.arange(rows), torch.randint(0, K, (rows,), generator=gen)] = torch.where(torch.rand(rows, generator=gen) < 0.5, 0x7e, 0xfe).to(torch.uint8)
    s = torch.pow(2.0, torch.randint(-12, 4, (rows,), generator=gen).float())
    W = _deq(q) * s[:, None]
    assert torch.equal(W.to(BF).float(), W)
    return W.to(BF).cuda(), q, s


def _gemm_inputs(M, K, N, epi, gen):
    dev = torch.device("cuda")
    x = torch.randn(M, K, generator=gen).to(BF).to(dev)
    b = (0.1 * torch.randn(2 * N if epi == 2 else N, generator=gen)).to(BF).to(dev)
    res = torch.randn(M, N, generator=gen).to(BF).to(dev)
    kw = dict(residual=res) if epi == 1 else {}
    return x, b, res, kw


def _f64_reference(x, q, s, b, res, N, epi):
    xd, wd, bd = x.double().cpu(), _deq(q).double() * s.double()[:, None], b.double().cpu()
    if epi == 0:
        return xd @ wd.T + bd
    if epi == 1:
        return (xd @ wd.T + bd) + res.double().cpu()
    gate, up = xd @ wd[:N].T + bd[:N], xd @ wd[N:].T + bd[N:]
    return torch.nn.functional.silu(gate) * up


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _c_linear_rows_packed_fmt(x, pk, epi, bias, res, code):
    """lantern_linear_rows_packed_fmt itself, with `code` as its `packed` argument"""
    M, K = x.shape
    out = torch.full((M, pk.n_rows), float("nan"), dtype=BF, device=x.device)
    rc = _lib.lib().lantern_linear_rows_packed_fmt(_ptr(x), _ptr(pk.data), _ptr(bias), M, K, pk.n_rows, _ptr(out), pk.n_rows, epi, _ptr(res if epi == 1 else None),
                                                   res.shape[1] if epi == 1 else 0, pk.pair_rows, code, ops._stream())
    assert rc == 0, _lib.lib().lantern_last_error()
    return out


def _c_drafter_fc_packed(ids, hid, embed, pk, bias, scale, code):
    M, H = hid.shape
    out = torch.full((M, H), float("nan"), dtype=BF, device=hid.device)
    rc = _lib.lib().lantern_drafter_fc_packed(_ptr(ids), _ptr(hid), _ptr(embed), _ptr(pk.data), _ptr(bias), M, H, embed.shape[0], C.c_float(scale), _ptr(out), code,
                                              ops._stream())
    assert rc == 0, _lib.lib().lantern_last_error()
    return out


# ----------------------------------------------------------------------------------------------------------------- 1. bit-exact
@pytest.mark.parametrize("M,K,N,epi", SHAPES)
def test_fp8_tiled_gemm_is_bit_exact_against_the_bf16_tiled_kernel_on_power_of_two_scales(M, K, N, epi):
    gen = torch.Generator().manual_seed(M * 131 + K + N + epi)
    rows = 2 * N if epi == 2 else N
    W, q, s = _code_weight(rows, K, gen)
    x, b, res, kw = _gemm_inputs(M, K, N, epi, gen)
    pair = N if epi == 2 else 0
    p16, p8 = ops.pack_linear_weight(W, pair), ops.pack_linear_weight(W, pair, fmt="fp8")
    q_got, s_got = ops.unpack_linear_weight_fp8(p8)
    assert torch.equal(_deq(q_got.cpu()), _deq(q)) and torch.equal(s_got.cpu(), s)
    assert M >= _lib.get_tuning("gemm_tiled_from")          # both sides are the tiled kernel
    want = ops.linear_rows_packed(x, p16, epi, bias=b, **kw)
    got = ops.linear_rows_packed(x, p8, epi, bias=b, **kw)
    again = ops.linear_rows_packed(x, p8, epi, bias=b, **kw)
    assert got.shape == (M, N) and torch.equal(got, want), (got.float() - want.float()).abs().max()
    assert torch.equal(again, got)


# ----------------------------------------------------------------------------------------------------------------- 2. f64
@pytest.mark.parametrize("M,K,N,epi", SHAPES)
def test_fp8_tiled_gemm_matches_f64_on_arbitrary_scales(M, K, N, epi):
    """W ~ N(0, 1 / K), the reference on the dequantised weights (exact there); 2e-2 of max |reference|: bf16 activations, f32 accumulation in another
    order, bf16 output roundings -- the bound of test_fp8_gemm_matches_f64_on_arbitrary_scales and of the bf16 kernels' tests on these inputs."""
    gen = torch.Generator().manual_seed(M * 131 + K + N + epi + 1)
    rows = 2 * N if epi == 2 else N
    W = (torch.randn(rows, K, generator=gen) / K ** 0.5).to(BF).cuda()
    x, b, res, kw = _gemm_inputs(M, K, N, epi, gen)
    p8 = ops.pack_linear_weight(W, N if epi == 2 else 0, fmt="fp8")
    q, s = ops.unpack_linear_weight_fp8(p8)
    want = _f64_reference(x, q.cpu(), s.cpu(), b, res, N, epi)
    scale = want.abs().max().item()
    got = ops.linear_rows_packed(x, p8, epi, bias=b, **kw)
    err = (got.double().cpu() - want).abs().max().item()
    print(f"fp8 tiled gemm {(M, K, N, epi)}: max err {err:.3e} of scale {scale:.3e}")
    assert got.shape == (M, N) and err <= 2e-2 * scale


# ----------------------------------------------------------------------------------------------------------------- 3. routing
def test_fp8_prefill_rows_take_one_tiled_launch_and_fewer_rows_keep_the_streamk_blocks(monkeypatch):
    K, N = 320, 40
    gen = torch.Generator().manual_seed(5)
    W = (torch.randn(N, K, generator=gen) / K ** 0.5).to(BF).cuda()
    p8 = ops.pack_linear_weight(W, fmt="fp8")
    calls = []
    real = ops.linear_rows_streamk
    monkeypatch.setattr(ops, "linear_rows_streamk", lambda *a, **k_: (calls.append(a[0].shape[0]), real(*a, **k_))[1])
    x, b, res, kw = _gemm_inputs(200, K, N, 1, gen)
    got = ops.linear_rows_packed(x, p8, 1, bias=b, **kw)
    assert calls == [] and got.shape == (200, N)
    ops.linear_rows_packed(x[:70], p8, 1, bias=b, residual=res[:70])
    assert calls == [32, 32, 6]
    assert _lib.get_tuning("gemm_tiled_from") == 129
    calls.clear()
    ops.linear_rows_packed(x[:129], p8, 1, bias=b, residual=res[:129])          # the threshold itself is tiled, one row less is not
    assert calls == []
    ops.linear_rows_packed(x[:128], p8, 1, bias=b, residual=res[:128])
    assert calls == [32, 32, 32, 32]


# ----------------------------------------------------------------------------------------------------------------- 4. the C entry
@pytest.mark.parametrize("M", [5, 40])
@pytest.mark.parametrize("K,N,epi", [(320, 40, 1), (832, 70, 2), (64, 33, 0)])
def test_the_c_entry_runs_the_tiled_fp8_kernel_at_any_row_count(M, K, N, epi):
    """packed = 2 below the bf16 kernels' threshold: no fallback to the row-blocked kernel (it would read the fp8 bricks as bf16 and miss the bound by
    orders of magnitude), no refusal."""
    gen = torch.Generator().manual_seed(M + K + N + epi)
    rows = 2 * N if epi == 2 else N
    W = (torch.randn(rows, K, generator=gen) / K ** 0.5).to(BF).cuda()
    x, b, res, kw = _gemm_inputs(M, K, N, epi, gen)
    p8 = ops.pack_linear_weight(W, N if epi == 2 else 0, fmt="fp8")
    q, s = ops.unpack_linear_weight_fp8(p8)
    want = _f64_reference(x, q.cpu(), s.cpu(), b, res, N, epi)
    got = _c_linear_rows_packed_fmt(x, p8, epi, b, res, 2)
    err = (got.double().cpu() - want).abs().max().item()
    print(f"fp8 tiled gemm through the C entry {(M, K, N, epi)}: max err {err:.3e} of scale {want.abs().max().item():.3e}")
    assert err <= 2e-2 * want.abs().max().item()
    # packed = 1 is lantern_linear_rows_packed itself
    p16 = ops.pack_linear_weight(W, N if epi == 2 else 0)
    assert torch.equal(_c_linear_rows_packed_fmt(x, p16, epi, b, res, 1), ops.linear_rows_packed(x, p16, epi, bias=b, **kw))


# ----------------------------------------------------------------------------------------------------------------- 5. gather form
@pytest.mark.parametrize("embed_scale", [1.0, 8.0])
@pytest.mark.parametrize("M", [129, 200])
def test_fp8_input_stage_prefill_equals_the_gemm_on_the_concatenated_rows(M, embed_scale):
    """ops.drafter_fc on an fp8 packed weight at prefill row counts = the tiled kernel's gather form: the bits of ops.linear_rows_packed on
    cat(bf16(embed[ids] * scale), hidden) -- the same kernel, only the A addressing differs (ids outside the vocabulary are clamped, as in the stream-K form)."""
    H, vocab = 128, 512
    gen = torch.Generator().manual_seed(int(embed_scale) * 1000 + M)
    Wc, _, _ = _code_weight(H, 2 * H, gen)
    Wr = (torch.randn(H, 2 * H, generator=gen) / (2 * H) ** 0.5).to(BF).cuda()
    embed = torch.randn(vocab, H, generator=gen).to(BF).cuda()
    bias = (0.1 * torch.randn(H, generator=gen)).to(BF).cuda()
    ids = torch.randint(0, vocab, (M,), generator=gen)
    ids[3], ids[M - 1] = -7, vocab + 5
    ids = ids.cuda()
    hid = torch.randn(M, H, generator=gen).to(BF).cuda()
    e = embed[ids.clamp(0, vocab - 1)]
    if embed_scale > 1.0:
        e = (e.float() * embed_scale).to(BF)          # one f32 product, rounded to nearest even: the kernel's f32_to_bf16_rne
    cat = torch.cat((e, hid), dim=1).contiguous()
    for W in (Wc, Wr):
        p16, p8 = ops.pack_linear_weight(W), ops.pack_linear_weight(W, fmt="fp8")
        got8 = ops.drafter_fc(ids, hid, embed, W, bias, embed_scale=embed_scale, packed=p8)
        assert got8.shape == (M, H) and torch.equal(got8, ops.linear_rows_packed(cat, p8, bias=bias))
        assert torch.equal(got8, _c_drafter_fc_packed(ids, hid, embed, p8, bias, embed_scale, 2))
        got16 = _c_drafter_fc_packed(ids, hid, embed, p16, bias, embed_scale, 1)
        assert torch.equal(got16, ops.linear_rows_packed(cat, p16, bias=bias))
        if W is Wc:
            assert torch.equal(got8, got16)          # codes times powers of two: fp8 = bf16, bit for bit
    p8 = ops.pack_linear_weight(Wr, fmt="fp8")          # and without a bias
    assert torch.equal(ops.drafter_fc(ids, hid, embed, Wr, None, embed_scale=embed_scale, packed=p8), ops.linear_rows_packed(cat, p8))


# ----------------------------------------------------------------------------------------------------------------- 6. layer, drafter
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


@pytest.mark.parametrize("name", ["hd128", "lg_hd64"])
def test_layer_prefill_runs_tiled_with_fp8_weights(name, monkeypatch):
    """A causal prefill of 2 x 80 rows (160 >= 129; the second row left-padded by 3) through a fixture layer of each family with weight_format = "fp8":
    its four GEMMs are one ops.linear_rows_packed call each and none of them falls into stream-K blocks; against the layer's torch composition in f32
    on the dequantised weights at rtol = atol = 4e-2 (test_layers_run_with_fp8_weights' tolerance) on every row that is not padding."""
    import test_drafter_layer as TL
    from lantern_amd.drafters.decoder_layer import precompute_freqs_cis_2d
    dev = torch.device("cuda")
    lg = name.startswith("lg_")
    builder = TL.build_lg if lg else TL.build
    layer = builder(name, dev, BF)
    layer.weight_format = "fp8"
    H, d = layer.self_attn.hidden_size, layer.self_attn.head_dim
    T0, starts = 80, [0, 3]
    gen = torch.Generator(device="cuda").manual_seed(len(name) + T0)
    x0 = torch.randn(2, T0, H, device=dev, generator=gen).to(BF)
    if lg:
        pos0 = torch.arange(T0, device=dev)[None]
        kw0 = dict(freqs_cis=precompute_freqs_cis_2d(16, d, 10000, 20).to(dev)[pos0[0]])
    else:
        pos0 = (torch.arange(T0, device=dev)[None] - torch.tensor(starts, device=dev)[:, None]).clamp(min=0)
        kw0 = {}
    calls = []
    for fn in ("linear_rows_packed", "linear_rows_streamk"):
        real = getattr(ops, fn)
        monkeypatch.setattr(ops, fn, (lambda real, fn: (lambda A, w, *a, **k_: (calls.append((fn, A.shape[0], getattr(w, "fmt", None))), real(A, w, *a, **k_))[1]))(real, fn))
    ks = torch.tensor(starts, dtype=torch.int64, device=dev)
    m0 = TL._causal_additive(T0, 0, starts, dev)
    with torch.no_grad():
        y0, kv0 = layer(x0, attention_mask=m0, position_ids=pos0, use_cache=True, causal=True, kv_start=ks, **kw0)
        assert calls == [("linear_rows_packed", 160, "fp8")] * 4, calls
        ref = _dequantised_f32_copy(layer, builder, name, dev)
        r0, rkv0 = ref(x0.float(), attention_mask=m0, position_ids=pos0, use_cache=True, **kw0)
    for b, st in enumerate(starts):
        np.testing.assert_allclose(y0[b, st:].float().cpu().numpy(), r0[b, st:].cpu().numpy(), rtol=4e-2, atol=4e-2)
        for got, want in zip(kv0, rkv0):
            np.testing.assert_allclose(got[b, :, st:].float().cpu().numpy(), want[b, :, st:].cpu().numpy(), rtol=4e-2, atol=4e-2)


def test_fp8_drafter_prefill_runs_the_input_stage_in_one_call(monkeypatch):
    """cnets.Model.forward on a 2 x 80 prefill with fp8 weights: ops.drafter_fc once, with all 160 rows and the fp8 packed fc weight (a bf16 drafter
    slices by 128 rows, and keeps doing so); the layer's GEMMs never reach the stream-K kernel."""
    from lantern_amd.drafters import cnets
    dev, V, H, T = torch.device("cuda"), 16384, 128, 80
    cfg = types.SimpleNamespace(vocab_size=V, hidden_size=H, pad_token_id=None, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=2,
                                intermediate_size=2 * H, max_position_embeddings=512, rms_norm_eps=1e-5, model_parallel_size=1, input_type="t2i")
    torch.manual_seed(3)
    mdl = cnets.Model(cfg, total_tokens=40, depth=4, top_k=CS.TOPK, model_type="lumina_mgpt").to(dev).to(BF)
    mdl.init_tree()
    gen = torch.Generator(device="cuda").manual_seed(9)
    x = torch.randn(2, T, H, device=dev, generator=gen).to(BF)
    ids = torch.randint(4, 8000, (2, T), device=dev, generator=gen)
    am = torch.ones(2, T, dtype=torch.bool, device=dev)
    am[1, :3] = False
    fc_calls, sk_calls = [], []
    real_fc, real_sk = ops.drafter_fc, ops.linear_rows_streamk
    monkeypatch.setattr(ops, "drafter_fc", lambda ids_, hid_, *a, **k_: (fc_calls.append((hid_.shape[0], getattr(k_.get("packed"), "fmt", None))), real_fc(ids_, hid_, *a, **k_))[1])
    monkeypatch.setattr(ops, "linear_rows_streamk", lambda A, *a, **k_: (sk_calls.append(A.shape[0]), real_sk(A, *a, **k_))[1])

    def run():
        mdl.reset_kv()
        mdl.tree_mask = None
        with torch.no_grad():
            return mdl(x, ids, attention_mask=am, use_cache=True)[0]
    y16 = run()
    assert fc_calls == [(128, None), (32, None)] and sk_calls == []
    fc_calls.clear()
    mdl.set_weight_format("fp8")
    y8 = run()
    assert fc_calls == [(160, "fp8")] and sk_calls == []
    assert y8.shape == (2, T, H) and bool(torch.isfinite(y8.float()).all())
    # The fp8 drafter's hidden states stay near the bf16 drafter's on the rows that are not padding.  Bound: e4m3 keeps 3 mantissa bits, a relative error
    # of at most 2^-4 per weight; over the six products of input stage + layer (random signs, sums of 128 - 256 terms) the recorded difference of the
    # random-weight fixtures is 3-4 % of the range (EXPERIMENTS.md "FP8 weight streaming", agreement): 2^-4 * 2 = 12.5 % of max |bf16| is what a wrong
    # scale, brick or row order would miss by a factor of several.
    d = (y8.float() - y16.float())[:, 3:].abs().max().item()
    assert d <= 0.125 * y16.float()[:, 3:].abs().max().item(), d


# ----------------------------------------------------------------------------------------------------------------- 7. the route, piece by piece
def _c_drafter_fc(ids, hid, embed, W, bias, scale):
    """lantern_drafter_fc itself: the per-tile kernel on the row-major weight"""
    M, H = hid.shape
    out = torch.full((M, H), float("nan"), dtype=BF, device=hid.device)
    rc = _lib.lib().lantern_drafter_fc(_ptr(ids), _ptr(hid), _ptr(embed), _ptr(W), _ptr(bias), M, H, embed.shape[0], C.c_float(scale), _ptr(out), ops._stream())
    assert rc == 0, _lib.lib().lantern_last_error()
    return out


def _c_drafter_fc_streamk(ids, hid, embed, wt, bias, scale, code):
    """lantern_drafter_fc_streamk itself on `wt`: the row-major weight (code 0) or a packed weight's bricks (code 1 / 2)"""
    M, H = hid.shape
    out = torch.full((M, H), float("nan"), dtype=BF, device=hid.device)
    ws = ops._sk_workspace(hid.device)
    rc = _lib.lib().lantern_drafter_fc_streamk(_ptr(ids), _ptr(hid), _ptr(embed), _ptr(wt), _ptr(bias), M, H, embed.shape[0], C.c_float(scale), _ptr(out), code,
                                               _ptr(ws), C.c_size_t(ws.numel()), ops._stream())
    assert rc == 0, _lib.lib().lantern_last_error()
    return out


def _fc_inputs(M, H=128, vocab=512):
    gen = torch.Generator().manual_seed(1000 + M)
    W = (torch.randn(H, 2 * H, generator=gen) / (2 * H) ** 0.5).to(BF).cuda()
    embed = torch.randn(vocab, H, generator=gen).to(BF).cuda()
    bias = (0.1 * torch.randn(H, generator=gen)).to(BF).cuda()
    ids = torch.randint(0, vocab, (M,), generator=gen).cuda()
    hid = torch.randn(M, H, generator=gen).to(BF).cuda()
    return ids, hid, embed, W, bias


@pytest.mark.parametrize("M", [20, 40, 150])
def test_bf16_input_stage_equals_the_kernels_its_route_names(M, monkeypatch):
    """ops.drafter_input_stage / ops.drafter_fc at any row count = the single-kernel calls of ops.drafter_gemm_route("input"), issued by hand through the C
    entries, bit for bit: 20 rows stream-K on the packed weight; 40 rows lantern_drafter_fc; 150 rows 128 on lantern_drafter_fc and the 22-row tail on
    stream-K with the ROW-MAJOR weight (the oddity the route's docstring records)."""
    ids, hid, embed, W, bias = _fc_inputs(M)
    p16 = ops.pack_linear_weight(W)
    scale = 2.0
    if M == 20:
        want = _c_drafter_fc_streamk(ids, hid, embed, p16.data, bias, scale, 1)
    elif M == 40:
        want = _c_drafter_fc(ids, hid, embed, W, bias, scale)
    else:
        want = torch.cat([_c_drafter_fc(ids[:128], hid[:128], embed, W, bias, scale), _c_drafter_fc_streamk(ids[128:], hid[128:], embed, W, bias, scale, 0)])
    assert ops.drafter_gemm_route("input", 150, ops.W_PACKED, True, _lib.get_tuning("gemm_tiled_from")) == [("drafter_fc", 0, 128), ("drafter_fc_streamk/row-major", 128, 22)]
    pieces = []
    real = ops.drafter_fc
    monkeypatch.setattr(ops, "drafter_fc", lambda ids_, hid_, *a, **k_: (pieces.append((hid_.shape[0], getattr(k_.get("packed"), "fmt", None))), real(ids_, hid_, *a, **k_))[1])
    got = ops.drafter_input_stage(ids, hid, embed, W, bias, scale, p16)
    assert pieces == {20: [(20, "bf16")], 40: [(40, None)], 150: [(128, None), (22, None)]}[M]
    assert got.shape == want.shape and torch.equal(got, want)
    assert torch.equal(real(ids, hid, embed, W, bias, embed_scale=scale, packed=p16), want)          # ops.drafter_fc takes any row count too
    assert torch.equal(real(ids, hid, embed, W, bias, embed_scale=scale), want if M != 20 else _c_drafter_fc_streamk(ids, hid, embed, W, bias, scale, 0))


@pytest.mark.parametrize("M", [40, 128, 129])
def test_fp8_input_stage_equals_the_kernels_its_route_names(M):
    """The same for an fp8 packed weight: below "gemm_tiled_from" (129) stream-K blocks of 32 rows on the packed weight, from there one lantern_drafter_fc_packed."""
    assert _lib.get_tuning("gemm_tiled_from") == 129
    ids, hid, embed, W, bias = _fc_inputs(M)
    p8 = ops.pack_linear_weight(W, fmt="fp8")
    if M >= 129:
        want = _c_drafter_fc_packed(ids, hid, embed, p8, bias, 2.0, 2)
    else:
        want = torch.cat([_c_drafter_fc_streamk(ids[m:m + 32], hid[m:m + 32], embed, p8.data, bias, 2.0, 2) for m in range(0, M, 32)])
    for fn in (ops.drafter_input_stage, ops.drafter_fc):
        got = fn(ids, hid, embed, W, bias, 2.0, p8)
        assert got.shape == (M, 128) and torch.equal(got, want)


@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
@pytest.mark.parametrize("M", [32, 33, 129])
def test_layer_gemm_equals_the_kernels_its_route_names(M, fmt):
    """ops.drafter_linear (the decoder layer's GEMM) at K = 320, N = 40 with the residual epilogue: 32 rows one stream-K call; 33 rows bf16 one
    lantern_linear_rows_packed, fp8 stream-K blocks of 32 + 1 rows; 129 rows bf16 lantern_linear_rows_packed, fp8 one lantern_linear_rows_packed_fmt."""
    K, N = 320, 40
    gen = torch.Generator().manual_seed(5 + M)
    W = (torch.randn(N, K, generator=gen) / K ** 0.5).to(BF).cuda()
    pk = ops.pack_linear_weight(W, fmt=fmt)
    x, b, res, kw = _gemm_inputs(M, K, N, 1, gen)
    if M <= 32:
        want = ops.linear_rows_streamk(x, pk, 1, bias=b, residual=res)
    elif fmt == "bf16":
        want = torch.full((M, N), float("nan"), dtype=BF, device=x.device)
        rc = _lib.lib().lantern_linear_rows_packed(_ptr(x), _ptr(pk.data), _ptr(b), M, K, N, _ptr(want), N, 1, _ptr(res), N, 0, ops._stream())
        assert rc == 0, _lib.lib().lantern_last_error()
    elif M < 129:
        want = torch.cat([ops.linear_rows_streamk(x[m:m + 32], pk, 1, bias=b, residual=res[m:m + 32]) for m in range(0, M, 32)])
    else:
        want = _c_linear_rows_packed_fmt(x, pk, 1, b, res, 2)
    got = ops.drafter_linear(x, pk, 1, bias=b, residual=res)
    assert got.shape == (M, N) and torch.equal(got, want)
    assert torch.equal(ops.drafter_linear(x, pk, 1, bias=b, residual=res), got)
