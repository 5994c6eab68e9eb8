#!/usr/bin/env python3
"""lantern_tree_attention on a bf16 cache against lantern_tree_attention_kv8 on the FP8 form of the same cache, at the shapes of tools/ta_profile.py,
in one process: the K/V values are quantised once (lantern_kv8_append), the bf16 cache is the dequantised image of the FP8 one, so both launches see
the same numbers and their outputs are compared bit for bit before anything is timed.  Timing: HIP events around 30 launches, after a warm-up of
both formats; the two formats alternate, five repetitions each; median and spread (max - min) of the per-launch time.  Bytes = K and V rows read once
+ q + out.  Then the append kernel alone for T = 26 and 59 new rows per (batch row, head), K and V in one launch.
Usage: python tools/ta_kv8_bench.py [--json out.json] [--shapes substring]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lantern_amd import ops  # noqa: E402

SHAPES = [("lumina_1seq_N26", 2, 32, 32, 26, 128, 2400), ("lumina_1seq_N59", 2, 32, 32, 59, 128, 2400),
          ("lumina_8seq_N26", 16, 32, 32, 26, 128, 2400), ("lumina_48seq_N26", 96, 32, 32, 26, 128, 2400),
          ("lumina_48seq_N59", 96, 32, 32, 59, 128, 2400), ("llamagen_1seq_N59", 2, 20, 20, 59, 64, 400),
          ("llamagen_48seq_N59", 96, 20, 20, 59, 64, 400)]
ITERS, REPS, WARMUP = 30, 5, 5


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS * 1e3      # us per launch


def alternate(fns):
    for fn in fns:
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(REPS):
        for i, fn in enumerate(fns):
            t[i].append(timed(fn))
    return t


def stats(ts):
    return round(statistics.median(ts), 2), round(max(ts) - min(ts), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--shapes", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ta_kv8_bench: no GPU (nothing is measured without one)")
    rows = []
    for label, B, Hq, Hkv, N, d, S in SHAPES:
        if args.shapes not in label:
            continue
        g = torch.Generator(device="cuda").manual_seed(0)
        q = torch.randn(B, N, Hq, d, generator=g, device="cuda").to(torch.bfloat16)
        k8 = torch.empty(B, Hkv, S, d + 16, dtype=torch.uint8, device="cuda")
        v8 = torch.empty_like(k8)
        for slab in (k8, v8):          # one of K / V at a time keeps the peak footprint down
            x = torch.randn(B, Hkv, S, d, generator=g, device="cuda").to(torch.bfloat16)
            ops.kv8_append(x if slab is k8 else None, x if slab is v8 else None, k8 if slab is k8 else None, v8 if slab is v8 else None, 0)
            del x
        k, v = ops.kv8_dequantize(k8), ops.kv8_dequantize(v8)
        bits = ops.tree_mask_bits(torch.tril(torch.ones(N, N, device="cuda")))
        lens = torch.full((B,), S, dtype=torch.int64, device="cuda")
        out16 = torch.empty(B, N, Hq * d, dtype=torch.bfloat16, device="cuda")
        out8 = torch.empty_like(out16)
        run16 = lambda: ops.tree_attention(q, k, v, bits, kv_len=lens, max_kv_len=S, out=out16)      # noqa: E731
        run8 = lambda: ops.tree_attention(q, k8, v8, bits, kv_len=lens, max_kv_len=S, out=out8)      # noqa: E731
        run16(), run8()
        torch.cuda.synchronize()
        same = bool(torch.equal(out16, out8))
        t16, t8 = alternate([run16, run8])
        io = 2 * B * N * Hq * d * 2
        b16, b8 = 2 * B * Hkv * S * d * 2 + io, 2 * B * Hkv * S * (d + 16) + io
        (m16, s16), (m8, s8) = stats(t16), stats(t8)
        row = {"shape": label, "B": B, "Hq": Hq, "N": N, "d": d, "S": S, "outputs_equal": same,
               "bf16_us": m16, "bf16_spread_us": s16, "bf16_raw_us": [round(x, 2) for x in t16], "bf16_bytes": b16, "bf16_GBps": round(b16 / m16 / 1e3, 1),
               "fp8_us": m8, "fp8_spread_us": s8, "fp8_raw_us": [round(x, 2) for x in t8], "fp8_bytes": b8, "fp8_GBps": round(b8 / m8 / 1e3, 1),
               "byte_ratio": round(b8 / b16, 4), "time_ratio": round(m8 / m16, 4), "fp8_faster_beyond_spread": bool(m16 - m8 > max(s16, s8))}
        del k, v
        for T in (26, 59):             # the append: T new rows per (batch row, head), K and V in one launch, behind S - T cached rows
            kn = torch.randn(B, Hkv, T, d, generator=g, device="cuda").to(torch.bfloat16)
            vn = torch.randn(B, Hkv, T, d, generator=g, device="cuda").to(torch.bfloat16)
            pos = torch.full((B,), S - T, dtype=torch.int64, device="cuda")
            (ta,) = alternate([lambda: ops.kv8_append(kn, vn, k8, v8, pos)])
            row[f"append_T{T}_us"], row[f"append_T{T}_spread_us"] = stats(ta)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del k8, v8
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
