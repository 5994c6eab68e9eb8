"""The drafter's six weight-streaming products at the drafting shape (20 rows) and the 7B sizes, one stream-K launch each: microseconds per call and the
achieved weight TB/s, for bf16 or fp8 packed weights.  Every product rotates over enough packed copies of its weight that a call never finds its
bricks in the 256 MB Infinity Cache (the state a drafting pass leaves for the next one is a matter of the whole pass: tools/draft_bench.py); medians of
`batches` x copies kernel-only timings (lantern_profile_next_launch) after a warm-up.
usage: streamk_bench.py [--weight-format bf16|fp8] [rows=20] [batches=7]      (LANTERN_<TUNING NAME>=<int> in the environment: lantern_tuning_set)"""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from lantern_amd import ops
from lantern_amd import _lib as _L

fmt = "bf16"
if "--weight-format" in sys.argv:
    i = sys.argv.index("--weight-format")
    fmt = sys.argv[i + 1]
    del sys.argv[i:i + 2]
M = int(sys.argv[1]) if len(sys.argv) > 1 else 20
batches = int(sys.argv[2]) if len(sys.argv) > 2 else 7
knobs = _L.tuning_from_env()
dev, bf = torch.device("cuda"), torch.bfloat16
H, I = 4096, 11008
# (name, K, N, epilogue): the layer's four, the input stage (gather form, K = 2H), the head window (8192 image ids; plain epilogue -- the CFG form differs in its tail only)
products = [("qkv", H, 3 * H, 0), ("o", H, H, 1), ("gate_up", H, I, 2), ("down", I, H, 1), ("fc", 2 * H, H, "fc"), ("head_window", H, 8192, 0)]
pack = (lambda w, pair: ops.pack_linear_weight(w, pair, fmt="fp8")) if fmt == "fp8" else (lambda w, pair: ops.pack_linear_weight(w, pair))
out = []
for name, K, N, epi in products:
    rows = 2 * N if epi == 2 else N
    nbytes = rows * K * (1 if fmt == "fp8" else 2)
    copies = max(2, -(-600_000_000 // nbytes) + 1)
    w = (torch.randn(rows, K, device=dev) / K ** 0.5).to(bf)
    pks = []
    for c in range(copies):
        pks.append(pack(w if c == 0 else w.roll(c, 0), N if epi == 2 else 0))
    res = torch.randn(M, N, device=dev, dtype=bf)
    if epi == "fc":
        embed = torch.randn(8192, H, device=dev, dtype=bf)
        ids = torch.randint(0, 8192, (M,), device=dev)
        x = torch.randn(M, H, device=dev, dtype=bf)
        call = lambda pk: ops.drafter_fc(ids, x, embed, w, None, packed=pk)
    else:
        x = torch.randn(M, K, device=dev, dtype=bf)
        kw = dict(residual=res) if epi == 1 else {}
        call = lambda pk: ops.linear_rows_streamk(x, pk, epi, **kw)
    for _ in range(2):
        for pk in pks:
            call(pk)
    torch.cuda.synchronize()
    # kernel-only durations: the launch itself records the event pair at kernel begin / end (lantern_profile_next_launch), so the Python call overhead
    # between launches (more than the kernel's own time for the small products) is not in the figure
    import ctypes as C
    evs = []
    for _ in range(batches):
        for pk in pks:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); e1.record()          # (torch creates the hipEvent_t handles on the first record)
            _L.check(_L.lib().lantern_profile_next_launch(C.c_void_p(e0.cuda_event), C.c_void_p(e1.cuda_event)), "profile_next_launch")
            call(pk)
            evs.append((e0, e1))
    torch.cuda.synchronize()
    times = [1e3 * e0.elapsed_time(e1) for e0, e1 in evs]
    us = statistics.median(times)
    out.append(dict(product=name, weight_format=fmt, rows=M, K=K, N=rows, weight_MB=round(nbytes / 1e6, 1), copies=copies, us=round(us, 2),
                    us_min=round(min(times), 2), us_max=round(max(times), 2), weight_TBps=round(nbytes / us / 1e6, 2)))
    print(out[-1], flush=True)
    del pks, w
print(json.dumps({"tuning": knobs, "products": out}))
