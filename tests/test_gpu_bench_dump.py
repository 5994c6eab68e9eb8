"""GPU (-m gpu): `bench.py --dump-outputs DIR` on the headline's kernel path at a small size (16 sequences in 4 stream groups, the chain kernel on
raw rows with its prepare stage inside the launch, commit turn-taking).  Two runs with the same arguments write the same arrays; the arrays are
what the last timed step computed, and agree with each other (the accepted tokens are the best candidate path, the KV lengths of a sequence's
two slabs differ by the prompt)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

ARGS = ["--gpus", "1", "--steps", "4", "--warmup", "2", "--seqs-per-gpu", "16", "--groups", "4", "--ep", "chain", "--kv-smax", "1024",
        "--pool-steps", "4", "--spin-up", "0", "--extras-out", ""]


def _run(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + ["--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.timeout(1300)
def test_bench_dump_outputs_are_the_last_step_and_repeat(tmp_path):
    line = _run(tmp_path / "a")
    assert line["steps"] == 4 and line["ms_per_step"] > 0 and "roofline" not in line and "cpu_baseline" not in line
    _run(tmp_path / "b")
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(n + ".npy" for n in ("best", "accept_len", "bonus_token", "counters", "candidates", "accepted_tokens",
                                                "accepted_hidden", "kv_lengths"))
    assert sorted(os.listdir(tmp_path / "b")) == names
    a = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    b = {n[:-4]: np.load(tmp_path / "b" / n) for n in names}
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    for n in a:
        assert a[n].dtype in (np.float32, np.float64), n
        assert np.array_equal(a[n], b[n]), n
    B = 16
    best, alen, cand = a["best"].astype(np.int64), a["accept_len"].astype(np.int64), a["candidates"].astype(np.int64)
    P, D = cand.shape[1:]
    assert best.shape == alen.shape == (B,) and ((best >= 0) & (best < P)).all() and ((alen >= 0) & (alen < D)).all()
    assert (a["counters"][:, 5] == 0).all()                                   # evaluate_posterior status: ok
    acc = a["accepted_tokens"].astype(np.int64)
    for s in range(B):
        assert np.array_equal(acc[s, :alen[s] + 1], cand[s, best[s], :alen[s] + 1])
        assert (acc[s, alen[s] + 1:] == -1).all() and not a["accepted_hidden"][s, :, alen[s] + 1:].any()
    assert a["accepted_hidden"].shape == (B, 2, D, 4096) and a["accepted_hidden"][:, :, 0].any()
    kv = a["kv_lengths"]
    assert kv.shape == (B, 2) and (kv[:, 0] - kv[:, 1] == 64).all() and (kv[:, 1] >= 3 + 6).all()   # cond = uncond + prompt; 6 steps behind them
