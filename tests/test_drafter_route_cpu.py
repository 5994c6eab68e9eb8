"""CPU: ops.drafter_gemm_route, the one statement of which kernel runs a GEMM of the drafter on M rows, against the routing table spelled out here
(what the drafter launched before the table existed, at "gemm_tiled_from" = 129, and the same rules at 65)."""
import pytest

from lantern_amd import ops

ROWS, PACKED, FP8 = ops.W_ROWS, ops.W_PACKED, ops.W_FP8
MS = [0, 1, 32, 33, 64, 128, 129, 130, 150, 300]
SK, RP, RPF = "linear_rows_streamk", "linear_rows_packed", "linear_rows_packed_fmt"
FC, FC_SK, FC_SK_ROWS, FC_PACKED = "drafter_fc", "drafter_fc_streamk", "drafter_fc_streamk/row-major", "drafter_fc_packed"


def _blocks(kernel, M, size):
    out, r = [], 0
    while r < M:
        out.append((kernel, r, min(size, M - r)))
        r += size
    return out


def _expected(stage, M, weight, aligned, tf):
    """The table, row by row; None where a combination does not exist."""
    if weight != ROWS and not aligned:
        return None                                            # a weight is packed only where K % 64 == 0
    if stage == "layer":
        if M <= 32:
            return [(SK, 0, M)]                                # one stream-K call, any weight form, M = 0 included
        if weight != FP8:
            return [(RP, 0, M)]                                # the C side picks row-blocked or tiled (ops.linear_rows_packed refuses a row-major weight)
        return _blocks(SK, M, 32) if M < tf else [(RPF, 0, M)]
    if stage == "packed":                                      # ops.linear_rows_packed called by itself
        if weight != FP8:
            return [(RP, 0, M)]
        return _blocks(SK, M, 32) if M < tf else [(RPF, 0, M)]          # (M = 0: no piece, no launch)
    if M <= 32:
        if not aligned:
            return [(FC, 0, M)]
        return [(FC_SK_ROWS if weight == ROWS else FC_SK, 0, M)]
    if weight == FP8:
        return _blocks(FC_SK, M, 32) if M < tf else [(FC_PACKED, 0, M)]
    return [(FC_SK_ROWS if n <= 32 and aligned else FC, r, n) for _, r, n in _blocks("", M, 128)]


@pytest.mark.parametrize("tf", [129, 65])
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("weight", [ROWS, PACKED, FP8])
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("stage", ["layer", "packed", "input"])
def test_route_is_the_table_and_tiles_the_rows(stage, M, weight, aligned, tf):
    want = _expected(stage, M, weight, aligned, tf)
    if want is None:
        with pytest.raises(ValueError, match="drafter_gemm_route"):
            ops.drafter_gemm_route(stage, M, weight, aligned, tf)
        return
    got = ops.drafter_gemm_route(stage, M, weight, aligned, tf)
    assert got == want
    at = 0
    for _, r0, n in got:                                       # no gap, no overlap, nothing behind M
        assert r0 == at and (n > 0 or M == 0)
        at += n
    assert at == M


def test_route_examples_written_out():
    r = ops.drafter_gemm_route
    assert r("layer", 70, FP8, True, 129) == [(SK, 0, 32), (SK, 32, 32), (SK, 64, 6)]
    assert r("packed", 70, FP8, True, 129) == [(SK, 0, 32), (SK, 32, 32), (SK, 64, 6)]
    assert r("packed", 0, FP8, True, 129) == [] and r("layer", 0, FP8, True, 129) == [(SK, 0, 0)]
    assert r("packed", 20, PACKED, True, 129) == [(RP, 0, 20)] and r("layer", 20, PACKED, True, 129) == [(SK, 0, 20)]
    assert r("layer", 128, FP8, True, 129) == [(SK, 0, 32), (SK, 32, 32), (SK, 64, 32), (SK, 96, 32)] and r("layer", 129, FP8, True, 129) == [(RPF, 0, 129)]
    assert r("layer", 70, FP8, True, 65) == [(RPF, 0, 70)] and r("layer", 64, FP8, True, 65) == [(SK, 0, 32), (SK, 32, 32)]
    # the input stage; a bf16 prefill never reads the packed copy, and its short tail runs on stream-K with the row-major weight (the known oddity)
    for w in (ROWS, PACKED):
        assert r("input", 150, w, True, 129) == [(FC, 0, 128), (FC_SK_ROWS, 128, 22)]
        assert r("input", 300, w, True, 129) == [(FC, 0, 128), (FC, 128, 128), (FC, 256, 44)]
        assert r("input", 130, w, True, 65) == [(FC, 0, 128), (FC_SK_ROWS, 128, 2)]          # bf16 does not read the tuning value
    assert r("input", 150, ROWS, False, 129) == [(FC, 0, 128), (FC, 128, 22)]
    assert r("input", 20, PACKED, True, 129) == [(FC_SK, 0, 20)] and r("input", 20, ROWS, True, 129) == [(FC_SK_ROWS, 0, 20)] and r("input", 20, ROWS, False, 129) == [(FC, 0, 20)]
    assert r("input", 70, FP8, True, 129) == [(FC_SK, 0, 32), (FC_SK, 32, 32), (FC_SK, 64, 6)]
    assert r("input", 128, FP8, True, 129) == _blocks(FC_SK, 128, 32) and r("input", 129, FP8, True, 129) == [(FC_PACKED, 0, 129)]
    assert r("input", 70, FP8, True, 65) == [(FC_PACKED, 0, 70)]
    # more rows of the table, literally: M = 33, 64, 300 for every weight form
    for stage in ("layer", "packed"):
        for M in (33, 64, 300):
            assert r(stage, M, PACKED, True, 129) == [(RP, 0, M)] and r(stage, M, ROWS, True, 129) == [(RP, 0, M)] and r(stage, M, ROWS, False, 129) == [(RP, 0, M)]
        assert r(stage, 33, FP8, True, 129) == [(SK, 0, 32), (SK, 32, 1)] and r(stage, 64, FP8, True, 129) == [(SK, 0, 32), (SK, 32, 32)]
        assert r(stage, 300, FP8, True, 129) == [(RPF, 0, 300)] and r(stage, 300, FP8, True, 65) == [(RPF, 0, 300)]
    assert r("layer", 32, ROWS, False, 129) == [(SK, 0, 32)] and r("layer", 1, FP8, True, 129) == [(SK, 0, 1)] and r("packed", 1, FP8, True, 129) == [(SK, 0, 1)]
    assert r("packed", 32, FP8, True, 16) == [(RPF, 0, 32)] and r("layer", 32, FP8, True, 16) == [(SK, 0, 32)]          # <= 32 rows: the layer never reads the tuning value
    for w in (ROWS, PACKED):
        assert r("input", 33, w, True, 129) == [(FC, 0, 33)] and r("input", 64, w, True, 129) == [(FC, 0, 64)] and r("input", 128, w, True, 129) == [(FC, 0, 128)]
        assert r("input", 129, w, True, 129) == [(FC, 0, 128), (FC_SK_ROWS, 128, 1)] and r("input", 160, w, True, 129) == [(FC, 0, 128), (FC_SK_ROWS, 128, 32)]
        assert r("input", 161, w, True, 129) == [(FC, 0, 128), (FC, 128, 33)]
    assert r("input", 33, FP8, True, 129) == [(FC_SK, 0, 32), (FC_SK, 32, 1)] and r("input", 64, FP8, True, 129) == [(FC_SK, 0, 32), (FC_SK, 32, 32)]
    assert r("input", 300, FP8, True, 129) == [(FC_PACKED, 0, 300)] and r("input", 0, PACKED, True, 129) == [(FC_SK, 0, 0)] and r("input", 0, ROWS, False, 129) == [(FC, 0, 0)]
    # the tuning value may come as a function: read only where the route depends on it
    reads = []
    tf = lambda: (reads.append(1), 129)[1]
    for stage, M, w in (("layer", 20, FP8), ("layer", 32, PACKED), ("layer", 150, PACKED), ("packed", 150, PACKED), ("input", 20, FP8), ("input", 20, PACKED), ("input", 150, PACKED), ("input", 150, ROWS)):
        assert r(stage, M, w, True, tf) == r(stage, M, w, True, 129)
    assert reads == []
    assert r("layer", 70, FP8, True, tf) == r("layer", 70, FP8, True, 129) and r("input", 129, FP8, True, tf) == [(FC_PACKED, 0, 129)] and len(reads) == 2
    with pytest.raises(ValueError):
        r("prefill", 5, PACKED, True, 129)
    with pytest.raises(ValueError):
        r("layer", -1, PACKED, True, 129)
