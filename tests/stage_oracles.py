"""Plain-torch oracles of the kernels the drafter's fused layer body launches besides its stream-K GEMMs -- lantern_rmsnorm_rows,
lantern_qk_norm_rope, lantern_qk_rope_pairs, lantern_linear_rows_splitk -- with the tolerances they are held to and the test cases, shared by
tests/test_drafter_stages_cpu.py (is the tolerance right, and does it bite?) and tests/test_gpu_drafter_stages.py (the kernels).

Three families, all on the CPU:
  *_ref       the operation in `dtype` (float64 for the kernel comparisons), on the bf16 inputs as they are.  `mutate=` gives a deliberately WRONG
              variant (a flipped sign, the other kernel's pairing, a position off by one ...): what a subtly broken kernel would compute.
  *_emulated  the same arithmetic in f32, rounded to bf16 exactly where the kernel comments (csrc/drafter_fc.hip) say the kernel rounds.
  *_tol       the elementwise bound |kernel - ref| must keep: roundings propagated to first order, u = 2^-8 the unit roundoff of bf16.
"""
import torch

U = 2.0 ** -8          # bf16: 8 significant bits, round to nearest even -> relative error of one rounding <= 2^-8
BF = torch.bfloat16


def _r(x):
    """one bf16 rounding of an f32 value, carried on in f32 (f32_to_bf16_rne then bf16_bits_to_f32 in the kernels)"""
    return x.to(BF).to(torch.float32)


# ----------------------------------------------------------------------------- rmsnorm_rows
RMS_MUTATIONS = ("mean", "no_weight")


def rmsnorm_ref(x, w, eps, dtype=torch.float64, mutate=None):
    """w * x * rsqrt(mean(x^2) + eps) over the last axis."""
    x, w = x.to(dtype), w.to(dtype)
    if mutate == "mean":
        var = (x - x.mean(-1, keepdim=True)).pow(2).mean(-1, keepdim=True)
    else:
        assert mutate in (None, "no_weight"), mutate
        var = x.pow(2).mean(-1, keepdim=True)
    y = x * torch.rsqrt(var + eps)
    return y if mutate == "no_weight" else w * y


def rmsnorm_emulated(x, w, eps):
    """rmsnorm_rows_kernel: f32 statistics, x * rstd rounded to bf16, times the bf16 weight, rounded again."""
    xf = x.to(torch.float32)
    rstd = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + torch.tensor(eps, dtype=torch.float32))
    return (w.to(torch.float32) * _r(xf * rstd)).to(BF)


def rmsnorm_tol(ref):
    """two roundings: (1 + u)^2 - 1 = 2^-7 (1 + 2^-9); the 1.01 leaves 6e-5 relative for the f32 statistics"""
    return 1.01 * 2.0 ** -7 * ref.abs() + 1e-30


RMS_H = (8, 24, 100, 2048, 2056, 4096, 8192, 8200, 11008)
RMS_M = (1, 5)
RMS_EPS = 1e-5
_RMS_SCALES = (1.0, 1e-2, 0.0, 1e2, 0.3)          # row 2 of a 5-row case is all zeros


def rmsnorm_case(H, M):
    """x [M, H] bf16 (row scales over 1e-2 .. 1e2, one all-zero row where M = 5; a mean of half the spread, so that the 'mean' mutation shows),
    w [H] bf16 = 1 + 0.3 randn."""
    g = torch.Generator().manual_seed(1000 * H + M)
    x = (torch.randn(M, H, generator=g) + 0.5) * torch.tensor(_RMS_SCALES[:M])[:, None]
    w = 1.0 + 0.3 * torch.randn(H, generator=g)
    return x.to(BF), w.to(BF)


# ----------------------------------------------------------------------------- the head stages
HEAD_CONFIGS = ((128, 4, 2, 2, 2, 5), (64, 4, 4, 1, 1, 3), (64, 8, 2, 2, 3, 1))          # (d, nq, nk, mp, B, T)
TABLE_ROWS = 300
NORM_ROPE_MUTATIONS = ("sign", "pairs", "swap", "pos", "shard", "shared_pos")
ROPE_PAIRS_MUTATIONS = ("sign", "halves", "swap", "pos", "shared_pos")


def _positions(pos, B, T, rows, mutate):
    pos = torch.as_tensor(pos).to(torch.int64).cpu()
    pos = pos.reshape(1, T).expand(B, T) if pos.numel() == T else pos.reshape(B, T)
    if mutate == "shared_pos":
        pos = pos[:1].expand(B, T)
    if mutate == "pos":
        pos = pos + 1
    return pos.clamp(0, rows - 1)          # the kernels' documented behaviour: never read outside the table


def _rot_halves(n):
    h = n.shape[-1] // 2
    return torch.cat((-n[..., h:], n[..., :h]), dim=-1)


def _rot_pairs(n):
    return torch.stack((-n[..., 1::2], n[..., 0::2]), dim=-1).flatten(-2)


def _split_heads(qkv, B, T, nq, nk, d):
    x = qkv.reshape(B, T, nq + 2 * nk, d)
    return x[:, :, :nq], x[:, :, nq:nq + nk], x[:, :, nq + nk:]


def _head_norm(xh, w, b, mutate, rnd):
    """[B, T, heads, d] -> (sc = ln * gamma, n = sc + beta): layer norm over d (eps 1e-5), gamma / beta row head // (heads / mp)."""
    heads, mp = xh.shape[2], w.shape[0]
    idx = torch.arange(heads) // (heads // mp)
    if mutate == "shard":
        idx = (idx + 1) % mp
    mean = xh.mean(-1, keepdim=True)
    var = (xh - mean).pow(2).mean(-1, keepdim=True)
    ln = rnd((xh - mean) * torch.rsqrt(var + 1e-5))
    sc = rnd(ln * w.to(xh.dtype)[idx])
    return sc, rnd(sc + b.to(xh.dtype)[idx])


def _norm_rope(qkv, B, T, nq, nk, d, qw, qb, kw, kb, cos, sin, pos, dtype, mutate, rnd):
    assert mutate is None or mutate in NORM_ROPE_MUTATIONS, mutate
    q, k, v = _split_heads(qkv, B, T, nq, nk, d)
    p = _positions(pos, B, T, cos.shape[0], mutate)
    c, s = cos.cpu().to(dtype)[p][:, :, None], sin.cpu().to(dtype)[p][:, :, None]          # [B, T, 1, d]: the bf16 table values as given
    if mutate == "swap":
        c, s = s, c
    out, aux = [], {}
    for name, xh, w, b in (("q", q, qw, qb), ("k", k, kw, kb)):
        sc, n = _head_norm(xh.to(dtype), w.cpu(), b.cpu(), mutate, rnd)
        rot = _rot_pairs(n) if mutate == "pairs" else _rot_halves(n)
        if mutate == "sign":
            rot = -rot
        out.append(rnd(rnd(n * c) + rnd(rot * s)).permute(0, 2, 1, 3))
        aux[name] = tuple(t.permute(0, 2, 1, 3) for t in (sc, n, c, s))
    return out[0], out[1], v.permute(0, 2, 1, 3), aux


def qk_norm_rope_ref(qkv, B, T, nq, nk, d, qw, qb, kw, kb, cos, sin, pos, dtype=torch.float64, mutate=None):
    """qkv [B*T, (nq + 2 nk) d] -> q [B,nq,T,d], k [B,nk,T,d] in `dtype`, v [B,nk,T,d] (the input values, untouched), and
    aux = {"q" | "k": (sc, n, cos, sin)}: the intermediates qk_norm_rope_tol needs, laid out like the outputs (cos / sin broadcast over heads)."""
    return _norm_rope(qkv.cpu(), B, T, nq, nk, d, qw, qb, kw, kb, cos, sin, pos, dtype, mutate, lambda t: t)


def qk_norm_rope_emulated(qkv, B, T, nq, nk, d, qw, qb, kw, kb, cos, sin, pos):
    """qk_norm_rope_kernel: f32 statistics; bf16 roundings of ln, ln * gamma, + beta, n * cos, rotate_half(n) * sin and the sum (six)."""
    q, k, v, _ = _norm_rope(qkv.cpu(), B, T, nq, nk, d, qw, qb, kw, kb, cos, sin, pos, torch.float32, None, _r)
    return q.to(BF), k.to(BF), v


def qk_norm_rope_tol(ref, aux):
    """Six roundings to first order, p the rotation partner (i + d/2) mod d: ln and sc each reach the output through cos (own element) and sin
    (partner) -- 2 u |sc| --, n likewise -- u |n| --, then the two products and the sum."""
    sc, n, c, s = aux
    h = ref.shape[-1] // 2
    scp, npt = torch.roll(sc, h, -1), torch.roll(n, h, -1)
    return 1.1 * U * (c.abs() * (2 * sc.abs() + n.abs()) + s.abs() * (2 * scp.abs() + npt.abs()) + (n * c).abs() + (npt * s).abs() + ref.abs()) + 1e-6


def _rope_pairs(qkv, B, T, nq, nk, d, freqs, pos, dtype, mutate):
    assert mutate is None or mutate in ROPE_PAIRS_MUTATIONS, mutate
    q, k, v = _split_heads(qkv, B, T, nq, nk, d)
    p = _positions(pos, B, T, freqs.shape[0], mutate)
    f = freqs.cpu().to(dtype)[p]                                           # [B, T, d/2, 2]
    c, s = (f[..., j].repeat_interleave(2, dim=-1)[:, :, None] for j in (0, 1))          # element i uses freqs[p][i // 2]
    if mutate == "swap":
        c, s = s, c
    out = []
    for xh in (q, k):
        x = xh.to(dtype)
        rot = _rot_halves(x) if mutate == "halves" else _rot_pairs(x)          # pairs: (x0 c - x1 s, x1 c + x0 s)
        if mutate == "sign":
            rot = -rot
        out.append((x * c + rot * s).permute(0, 2, 1, 3))
    return out[0], out[1], v.permute(0, 2, 1, 3)


def qk_rope_pairs_ref(qkv, B, T, nq, nk, d, freqs, pos, dtype=torch.float64, mutate=None):
    """qkv [B*T, (nq + 2 nk) d], freqs [rows, d/2, 2] f32 (cos, sin) -> q [B,nq,T,d], k [B,nk,T,d] in `dtype`, v [B,nk,T,d] (the input values)."""
    return _rope_pairs(qkv.cpu(), B, T, nq, nk, d, freqs, pos, dtype, mutate)


def qk_rope_pairs_emulated(qkv, B, T, nq, nk, d, freqs, pos):
    """qk_rope_pairs_kernel: everything in f32 on the bf16 inputs, one rounding to bf16."""
    q, k, v = _rope_pairs(qkv.cpu(), B, T, nq, nk, d, freqs, pos, torch.float32, None)
    return q.to(BF), k.to(BF), v


def qk_rope_pairs_tol(ref, x):
    """one rounding of an f32 result; `x`: the stage's input laid out like ref (|x0| + |x1| is the pair's magnitude at either element)"""
    xa = x.abs().to(ref.dtype)
    pair = xa + _rot_pairs(xa).abs()
    return 1.1 * U * ref.abs() + 1e-6 * pair


def head_inputs(cfg):
    """The inputs of one head-stage config: qkv = 1.5 randn + 0.3 (the mean subtraction matters), gamma = 1 + 0.3 randn and beta = 0.3 randn,
    distinct per shard; positions [B, T] over the whole table with position 0, position rows - 1 and -- B > 1 -- batch rows that differ at every t."""
    d, nq, nk, mp, B, T = cfg
    g = torch.Generator().manual_seed(d * 1000 + nq * 100 + B * 10 + T)
    qkv = (1.5 * torch.randn(B * T, (nq + 2 * nk) * d, generator=g) + 0.3).to(BF)
    qw, kw = ((1.0 + 0.3 * torch.randn(mp, d, generator=g)).to(BF) for _ in range(2))
    qb, kb = ((0.3 * torch.randn(mp, d, generator=g)).to(BF) for _ in range(2))
    pos = torch.randint(1, TABLE_ROWS - 1, (B * T,), generator=g)
    pos[0], pos[-1] = 0, TABLE_ROWS - 1
    pos = pos.reshape(B, T)
    assert B == 1 or bool((pos[0] != pos[1]).all())
    return dict(qkv=qkv, qw=qw, qb=qb, kw=kw, kb=kb, pos=pos)


def rotary_tables(d, rows=TABLE_ROWS):
    """cos / sin [rows, d] bf16, built the way the layer builds them (Rotary.tables_bf16)."""
    from lantern_amd.drafters.decoder_layer import Rotary
    return Rotary(d, rows).tables_bf16(torch.device("cpu"), rows)


def pair_tables(d, rows=TABLE_ROWS):
    """{"grid": LlamaGen's 2-D table (4 condition rows, a 16 x 16 grid, ten zero rows = 270 rows), "random": [rows, d/2, 2] f32 with cos and sin untied}"""
    from lantern_amd.drafters.decoder_layer import precompute_freqs_cis_2d
    g = torch.Generator().manual_seed(77 + d)
    return {"grid": precompute_freqs_cis_2d(16, d, cls_token_num=GRID_CLS).contiguous(), "random": torch.randn(rows, d // 2, 2, generator=g)}


GRID_CLS, GRID_CELLS = 4, 256


def pair_positions(pos, table, rows):
    """The config's positions for one of pair_tables: "random" -- folded into the table's rows, first and last row kept; "grid" -- spread over
    the grid cells only (its condition rows and its tail are zeros: a token there comes out as zeros whatever the kernel does; the clamp
    checks and the random table go there)."""
    if table == "grid":
        p = GRID_CLS + (pos * 7) % GRID_CELLS
    else:
        p = pos % rows
        p.view(-1)[0], p.view(-1)[-1] = 0, rows - 1
    assert p.shape[0] == 1 or bool((p[0] != p[1]).all())
    return p


# ----------------------------------------------------------------------------- linear_rows_splitk
SPLITK_SMALL = ((1, 16, 1, 1), (32, 48, 33, 3), (20, 256, 40, 16), (7, 272, 96, 5), (32, 1024, 70, 0))          # (M, K, N, ksplit); K <= 1024
SPLITK_7B = ((20, 4096, 4096, 0), (20, 11008, 4096, 0))


def splitk_auto(N):
    """the wrapper's choice for ksplit = 0: enough K slices to fill 256 CUs with 32-column tiles, at most 8"""
    return max(1, min(8, -(-256 // (-(-N // 32)))))


def splitk_case(M, K, N):
    g = torch.Generator().manual_seed(M * 131 + K + N)
    x = torch.randn(M, K, generator=g).to(BF)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(BF)
    b = (0.1 * torch.randn(N, generator=g)).to(BF)
    res = torch.randn(M, N, generator=g).to(BF)
    return x, w, b, res


def splitk_ref(x, w, bias=None, residual=None, dtype=torch.float64, drop_kstep=None):
    """(lin, want): lin = x @ w.T (+ bias), want = lin (+ residual).  drop_kstep = s: the WRONG product that loses the 16-wide k-step s."""
    x, w = x.cpu().to(dtype), w.cpu().to(dtype)
    if drop_kstep is not None:
        x = x.clone()
        x[:, 16 * drop_kstep:16 * drop_kstep + 16] = 0
    lin = x @ w.T
    if bias is not None:
        lin = lin + bias.cpu().to(dtype)
    return lin, (lin if residual is None else lin + residual.cpu().to(dtype))


def splitk_emulated(x, w, bias=None, residual=None):
    """linear_rows_splitk: f32 accumulation (in another order than the kernel's: inside the bound's last term), + bias, one rounding, + residual, one more"""
    v = x.to(torch.float32) @ w.to(torch.float32).T
    if bias is not None:
        v = v + bias.to(torch.float32)
    o = _r(v)
    return (o if residual is None else o + residual.to(torch.float32)).to(BF)


def splitk_tol(x, w, lin, want, residual):
    """one bf16 rounding per epilogue step, plus the worst case of a K-term f32 accumulation"""
    K = x.shape[1]
    acc = K * 2.0 ** -23 * (x.cpu().double().abs() @ w.cpu().double().abs().T)
    return U * lin.abs() + (U * want.abs() if residual is not None else 0.0) + acc


def splitk_seam(K, ksplit):
    """the first k-step of the middle K slice (slice y starts at k-step (K / 16) * y / ksplit, as the kernel divides them)"""
    return (K // 16) * (ksplit // 2) // ksplit


def worst_ratio(got, ref, tol):
    return float(((got.to(ref.dtype) - ref).abs() / tol).max())


def frac_outside(mut, ref, tol, factor=2.0):
    """share of elements a mutated oracle moves out of `factor` times the tolerance band"""
    return float(((mut - ref).abs() > factor * tol).double().mean())
