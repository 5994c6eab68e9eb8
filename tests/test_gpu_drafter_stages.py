"""The kernels the drafter's fused layer body launches besides its stream-K GEMMs -- lantern_rmsnorm_rows, lantern_qk_norm_rope,
lantern_qk_rope_pairs -- and lantern_linear_rows_splitk, each called directly and compared elementwise with its f64 oracle
(tests/stage_oracles.py) inside the derived tolerance tests/test_drafter_stages_cpu.py shows to hold and to bite; rows that are only copied
(V, the slab rows outside [row0, row0 + T)) bit for bit.  Every test prints its worst |got - ref| / tol (EXPERIMENTS.md records them)."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import stage_oracles as SO  # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _dev(*ts):
    return tuple(t.cuda() for t in ts)


# ----------------------------------------------------------------------------- rmsnorm_rows
@pytest.mark.parametrize("M", SO.RMS_M)
@pytest.mark.parametrize("H", SO.RMS_H)
def test_rmsnorm_rows_matches_f64(H, M):
    """Both paths of rmsnorm_rows_kernel: the vector one (H % 8 == 0 up to 8192: 8, 24, 2048 -- one chunk per thread --, 2056, 4096, 8192) and the
    scalar one (100; 8200 and 11008 beyond the vector limit); row scales over 1e-2 .. 1e2, the all-zero row gives exact zeros."""
    from lantern_amd import ops
    x, w = SO.rmsnorm_case(H, M)
    got = ops.rmsnorm_rows(x.cuda(), w.cuda(), SO.RMS_EPS).cpu()
    ref = SO.rmsnorm_ref(x, w, SO.RMS_EPS)
    assert got.shape == (M, H) and got.dtype == BF and bool(torch.isfinite(got.float()).all())
    r = SO.worst_ratio(got, ref, SO.rmsnorm_tol(ref))
    print(f"ratio rmsnorm_rows H={H} M={M}: {r:.3f}")
    assert r <= 1.0
    if M == 5:
        assert bool((got[2] == 0).all())          # (a zero of either sign: the weight's sign carries over)


def test_rmsnorm_rows_misaligned_input_takes_the_scalar_path_to_the_same_bits():
    """H = 4096 rows that start one element into a larger buffer: still contiguous, so the wrapper hands the 2-byte-aligned pointer through and the
    kernel leaves its 16-byte vector path; same values, same bits as the aligned call, and inside the tolerance."""
    from lantern_amd import ops
    H, M = 4096, 5
    x, w = SO.rmsnorm_case(H, M)
    xd, wd = _dev(x, w)
    buf = torch.zeros(M * H + 8, dtype=BF, device="cuda")
    view = buf[1:1 + M * H].view(M, H)
    view.copy_(xd)
    assert view.is_contiguous() and view.data_ptr() % 16 == 2 and xd.data_ptr() % 16 == 0
    aligned, shifted = ops.rmsnorm_rows(xd, wd, SO.RMS_EPS), ops.rmsnorm_rows(view, wd, SO.RMS_EPS)
    ref = SO.rmsnorm_ref(x, w, SO.RMS_EPS)
    r = SO.worst_ratio(shifted.cpu(), ref, SO.rmsnorm_tol(ref))
    print(f"ratio rmsnorm_rows misaligned H={H}: {r:.3f}, elements that differ from the aligned call: {int((_bits(aligned) != _bits(shifted)).sum())}")
    assert r <= 1.0
    assert _same_bits(aligned, shifted)


def test_rmsnorm_rows_of_no_rows():
    from lantern_amd import ops
    out = ops.rmsnorm_rows(torch.empty(0, 64, dtype=BF, device="cuda"), torch.ones(64, dtype=BF, device="cuda"), SO.RMS_EPS)
    torch.cuda.synchronize()
    assert out.shape == (0, 64)


# ----------------------------------------------------------------------------- the head stages
def _pattern(shape):
    """a recognisable bf16 fill: no value the kernels would produce by accident, different in every row"""
    n = 1
    for s in shape:
        n *= s
    return ((torch.arange(n, device="cuda") % 509).float() * 0.25 - 70.0).to(BF).reshape(shape)


def _check_slab_form(call, B, T, nk, d, q, k, v):
    """call(k_slab, v_slab, row0) writes rows [4, 4 + T) of [B, nk, T + 7, d] slabs: those rows as the freshly allocated form, the others untouched"""
    row0, rows = 4, T + 7
    k_slab, v_slab = _pattern((B, nk, rows, d)), _pattern((B, nk, rows, d)).flip(2).contiguous()
    k0, v0 = k_slab.clone(), v_slab.clone()
    q2, k2, v2 = call(k_slab, v_slab, row0)
    assert k2.data_ptr() == k_slab.data_ptr() and v2.data_ptr() == v_slab.data_ptr()
    assert _same_bits(q2, q) and _same_bits(k_slab[:, :, row0:row0 + T], k) and _same_bits(v_slab[:, :, row0:row0 + T], v)
    for slab, before in ((k_slab, k0), (v_slab, v0)):
        assert _same_bits(slab[:, :, :row0], before[:, :, :row0]) and _same_bits(slab[:, :, row0 + T:], before[:, :, row0 + T:])


def _far_positions(pos, rows):
    """positions beyond both ends of the table, and the ends they must be clamped to"""
    far, ends = pos.clone(), pos.clone()
    far.view(-1)[0], far.view(-1)[-1] = -3, rows + 7
    ends.view(-1)[0], ends.view(-1)[-1] = 0, rows - 1
    return far, ends


@pytest.mark.parametrize("cfg", SO.HEAD_CONFIGS, ids=str)
def test_qk_norm_rope_matches_f64(cfg):
    """Head dims 128 and 64, one and two gamma / beta shards, per-row positions over a 300-row table (0, the last row, batch rows that differ at
    every t): q and k inside the six-rounding tolerance of the f64 oracle, v the input bits; [T] positions as their [B, T] expansion; positions
    beyond the table as its ends; the slab form at row0 = 4 writes its T rows and nothing else."""
    from lantern_amd import ops
    d, nq, nk, mp, B, T = cfg
    i = SO.head_inputs(cfg)
    cos, sin = SO.rotary_tables(d)
    host = (i["qkv"], B, T, nq, nk, d, i["qw"], i["qb"], i["kw"], i["kb"], cos, sin)
    qkv, qw, qb, kw, kb, cosd, sind = _dev(i["qkv"], i["qw"], i["qb"], i["kw"], i["kb"], cos, sin)

    def run(pos, **kw_):
        return ops.qk_norm_rope(qkv, B, T, nq, nk, d, qw, qb, kw, kb, cosd, sind, pos.cuda(), **kw_)
    q, k, v = run(i["pos"])
    rq, rk, rv, aux = SO.qk_norm_rope_ref(*host, i["pos"])
    assert q.shape == (B, nq, T, d) and k.shape == v.shape == (B, nk, T, d)
    ratio_q, ratio_k = SO.worst_ratio(q.cpu(), rq, SO.qk_norm_rope_tol(rq, aux["q"])), SO.worst_ratio(k.cpu(), rk, SO.qk_norm_rope_tol(rk, aux["k"]))
    print(f"ratio qk_norm_rope {cfg}: q {ratio_q:.3f} k {ratio_k:.3f}")
    assert ratio_q <= 1.0 and ratio_k <= 1.0
    assert _same_bits(v.cpu(), rv)
    if B > 1:          # one row of positions shared by the batch rows
        shared = run(i["pos"][1])
        expanded = run(i["pos"][1].expand(B, T).contiguous())
        sq, sk, _, saux = SO.qk_norm_rope_ref(*host, i["pos"][1])
        assert SO.worst_ratio(shared[1].cpu(), sk, SO.qk_norm_rope_tol(sk, saux["k"])) <= 1.0
        assert all(_same_bits(a, b) for a, b in zip(shared, expanded))
    far, ends = _far_positions(i["pos"], cos.shape[0])
    assert all(_same_bits(a, b) for a, b in zip(run(far), run(ends)))
    assert _same_bits(run(ends)[1], k)          # (the config's positions already hold both ends)
    _check_slab_form(lambda ks, vs, r0: run(i["pos"], k_slab=ks, v_slab=vs, row0=r0), B, T, nk, d, q, k, v)


def test_qk_norm_rope_refuses_another_head_dim():
    from lantern_amd import ops
    from lantern_amd._lib import LanternError
    B, T, nq, nk, d = 1, 2, 2, 2, 32
    z = torch.zeros
    with pytest.raises(LanternError, match="head_dim 32"):
        ops.qk_norm_rope(z(B * T, (nq + 2 * nk) * d, dtype=BF, device="cuda"), B, T, nq, nk, d, *(z(1, d, dtype=BF, device="cuda") for _ in range(4)),
                         z(8, d, dtype=BF, device="cuda"), z(8, d, dtype=BF, device="cuda"), torch.arange(T, device="cuda"))


@pytest.mark.parametrize("table", ["grid", "random"])
@pytest.mark.parametrize("cfg", SO.HEAD_CONFIGS, ids=str)
def test_qk_rope_pairs_matches_f64(cfg, table):
    """The same geometries without norms, on LlamaGen's 2-D table and on a random one (cos and sin untied): per-row [B, T] positions and one
    shared [T] row against the f64 oracle inside one rounding; v the input bits; the clamp at both ends; the slab form."""
    from lantern_amd import ops
    d, nq, nk, mp, B, T = cfg
    i = SO.head_inputs(cfg)
    freqs = SO.pair_tables(d)[table]
    pos = SO.pair_positions(i["pos"], table, freqs.shape[0])
    host = (i["qkv"], B, T, nq, nk, d, freqs)
    qkv, fd = _dev(i["qkv"], freqs)
    xq, xk, _ = (t.permute(0, 2, 1, 3) for t in SO._split_heads(i["qkv"], B, T, nq, nk, d))

    def run(p, **kw_):
        return ops.qk_rope_pairs(qkv, B, T, nq, nk, d, fd, p.cuda(), **kw_)

    def ratios(got, p):
        rq, rk, rv = SO.qk_rope_pairs_ref(*host, p)
        assert _same_bits(got[2].cpu(), rv)
        return SO.worst_ratio(got[0].cpu(), rq, SO.qk_rope_pairs_tol(rq, xq)), SO.worst_ratio(got[1].cpu(), rk, SO.qk_rope_pairs_tol(rk, xk))
    q, k, v = run(pos)
    assert q.shape == (B, nq, T, d) and k.shape == v.shape == (B, nk, T, d)
    per_row, shared = ratios((q, k, v), pos), ratios(run(pos[-1]), pos[-1])          # [B, T], then one [T] row for every batch row
    print(f"ratio qk_rope_pairs {cfg} {table}: [B,T] q {per_row[0]:.3f} k {per_row[1]:.3f}, [T] q {shared[0]:.3f} k {shared[1]:.3f}")
    assert max(per_row + shared) <= 1.0
    assert all(_same_bits(a, b) for a, b in zip(run(pos[-1]), run(pos[-1].expand(B, T).contiguous())))
    far, ends = _far_positions(pos, freqs.shape[0])
    clamped = run(far)
    assert all(_same_bits(a, b) for a, b in zip(clamped, run(ends)))
    assert max(ratios(clamped, ends)) <= 1.0
    _check_slab_form(lambda ks, vs, r0: run(pos, k_slab=ks, v_slab=vs, row0=r0), B, T, nk, d, q, k, v)


def test_qk_rope_pairs_refuses_a_table_of_another_shape():
    from lantern_amd import ops
    from lantern_amd._lib import LanternError
    B, T, nq, nk, d = 1, 2, 2, 2, 64
    qkv = torch.zeros(B * T, (nq + 2 * nk) * d, dtype=BF, device="cuda")
    for shape in ((16, d, 2), (16, d // 2), (16, d // 2, 1)):
        with pytest.raises(LanternError, match="freqs must be"):
            ops.qk_rope_pairs(qkv, B, T, nq, nk, d, torch.zeros(shape, device="cuda"), torch.arange(T, device="cuda"))


# ----------------------------------------------------------------------------- linear_rows_splitk
@pytest.mark.parametrize("epilogue", ["plain", "bias", "residual", "bias_residual"])
@pytest.mark.parametrize("shape", SO.SPLITK_SMALL + SO.SPLITK_7B, ids=str)
def test_linear_rows_splitk_matches_f64(shape, epilogue):
    """One K slice, uneven slices, as many slices as k-steps, the automatic split; ragged column tiles, one row, 32 rows.  K <= 1024: inside
    one bf16 rounding per epilogue step plus the worst-case f32 accumulation error, elementwise (a lost k-step leaves that bound on every row:
    test_drafter_stages_cpu.py); the two 7B shapes: 2e-2 * max|want|, as the stream-K kernel's test.  Also: the per-tile kernels within
    2e-2 * scale, the same bits on a second call, and the same bits from a workspace that held NaN."""
    from lantern_amd import ops, _lib
    M, K, N, ksplit = shape
    x, w, b, res = SO.splitk_case(M, K, N)
    b = b if "bias" in epilogue else None
    res = res if "residual" in epilogue else None
    xd, wd = _dev(x, w)
    bd, rd = (None if t is None else t.cuda() for t in (b, res))
    got = ops.linear_rows_splitk(xd, wd, bias=bd, residual=rd, ksplit=ksplit)
    lin, want = SO.splitk_ref(x, w, b, res)
    assert got.shape == (M, N) and got.dtype == BF
    scale = float(want.abs().max())
    if K <= 1024:
        r = SO.worst_ratio(got.cpu(), want, SO.splitk_tol(x, w, lin, want, res))
    else:
        r = float((got.cpu().double() - want).abs().max()) / (2e-2 * scale)
    print(f"ratio linear_rows_splitk {shape} {epilogue}: {r:.3f}")
    assert r <= 1.0
    old = ops.linear_rows_epilogue(xd, wd, ops.EPI_RESIDUAL, bias=bd, residual=rd) if res is not None else ops.linear_rows(xd, wd, 0, N, bias=bd)
    assert float((got.float() - old.float()).abs().max()) <= 2e-2 * scale
    assert _same_bits(ops.linear_rows_splitk(xd, wd, bias=bd, residual=rd, ksplit=ksplit), got)
    # the C entry on a workspace full of NaN: every slot the finishing pass reads has been written by this launch
    ks = ksplit or SO.splitk_auto(N)
    ws = torch.full((ks, M, N), float("nan"), dtype=torch.float32, device="cuda")
    out = torch.full((M, N), float("nan"), dtype=BF, device="cuda")
    ptr = lambda t: C.c_void_p(None if t is None else t.data_ptr())          # noqa: E731
    _lib.check(_lib.lib().lantern_linear_rows_splitk(ptr(xd), ptr(wd), ptr(bd), M, K, N, ptr(out), N, ptr(rd), 0 if rd is None else N, ks, ptr(ws),
                                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)), "linear_rows_splitk")
    assert _same_bits(out, got)


@pytest.mark.parametrize("M,K,N,ksplit", [(33, 64, 8, 1), (4, 24, 8, 1), (4, 512, 8, 17), (4, 32, 8, 3)],
                         ids=["33_rows", "K_not_a_multiple_of_16", "17_slices", "more_slices_than_ksteps"])
def test_linear_rows_splitk_refuses_what_it_cannot_run(M, K, N, ksplit):
    """The argument check answers (its message names M, K and ksplit) before anything is launched."""
    from lantern_amd import ops
    from lantern_amd._lib import LanternError
    x, w = torch.zeros(M, K, dtype=BF, device="cuda"), torch.zeros(N, K, dtype=BF, device="cuda")
    with pytest.raises(LanternError, match=r"linear_rows_splitk: M=\d+ <= 32, K=\d+ % 16 == 0, 1 <= ksplit=\d+ <= 16"):
        ops.linear_rows_splitk(x, w, ksplit=ksplit)
    torch.cuda.synchronize()
