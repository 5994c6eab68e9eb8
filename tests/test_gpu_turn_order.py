"""GPU: commit turn-taking (lantern_step_group.turn) must not depend on how streams map to hardware queues.  lantern_verify_step enqueues the launches
that wait in ticket order, so groups that share a queue -- here, deterministically, a stream -- never wait for a launch enqueued behind them; the wait
is bounded by time and says so in turn[1] when it gave up; the harness places group streams on distinct hardware queues."""
import functools
import time

import pytest
import torch

GEOM = dict(kv_layers=2, kv_heads=4, kv_smax=512)
STEPS = 12


def _run(groups, steps, fused, **over):
    from lantern_amd import harness as HN
    cfg = HN.WorkloadConfig(n_seq=4 * groups, pool_steps=4, max_steps=steps + 4, sigma=5.0, n_groups=groups, ep_kernel="chain", fuse_o7=True, spec_rows=3,
                            fused_prepare=fused, **GEOM, **over)
    wl = HN.LuminaVerifyWorkload(cfg, torch.device("cuda"))
    assert wl.fused_prepare == fused
    return wl


def _results(wl, steps):
    """Every logged verdict, token and counter, the lengths and every KV slab, on the host."""
    wl.check_status(0, steps)
    return [x.cpu() for x in (wl.log_best[:steps], wl.log_alen[:steps], wl.log_token[:steps], wl.log_cnt[:steps], wl.lens[steps & 1], torch.stack(list(wl.slabs)))]


@functools.lru_cache(maxsize=None)
def _free_running(groups, steps, fused):
    """The reference: the same loop with the groups running free (commit_window = 0), each on its own stream.  Computed once per shape, never modified."""
    wl = _run(groups, steps, fused, commit_window=0)
    for _ in range(steps):
        wl.step()
    return _results(wl, steps)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("groups", [2, 4])
def test_turns_on_one_stream_never_wait(groups, fused):
    """Every group on ONE stream, the stand-in for a shared hardware queue: each walk's turn has been released by the time the walk runs, because the commit
    it waits for was enqueued in front of it.  Same results as the free-running loop, every commit counted once, and not one wait that gave up."""
    wl = _run(groups, STEPS, fused, commit_window=1, shared_stream=True)
    assert len({s.cuda_stream for s in wl.streams}) == 1
    for _ in range(STEPS):
        wl.step()
    got = _results(wl, STEPS)
    for a, b in zip(got, _free_running(groups, STEPS, fused)):
        assert torch.equal(a, b)
    t = wl._turn.cpu()
    assert int(t[0]) == STEPS * groups
    assert wl.turn_timeouts() == 0 and not t[1:].any()


@pytest.mark.gpu
def test_a_turn_nobody_releases_times_out_in_milliseconds_and_is_counted():
    """One step whose every walk waits for one commit more than will have completed (the turn block starts one behind the tickets): each walk gives up after
    2 ms, the step's results are the free-running step's, turn[1] counts the workgroups that gave up, and the step is over in a few milliseconds --
    the bound used to be ~104 ms per waiting launch.  (A bounded wait by design: run once.)"""
    from lantern_amd import _lib
    groups = 2
    ref = _free_running(groups, 1, False)          # (also loads every kernel the timed step uses)
    wl = _run(groups, 1, False, commit_window=1)
    wl._turn = torch.zeros(_lib.TURN_WORDS(groups), dtype=torch.int64, device="cuda")
    wl._turn[0] = -1
    wl._turn_step = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    wl.step()
    wl.sync()
    dt = time.perf_counter() - t0
    print(f"step with {groups} walks that wait out their bound: {dt * 1e3:.2f} ms; turn[:2] = {wl._turn[:2].tolist()}")
    assert dt < 0.050
    n = wl.turn_timeouts()
    assert 0 < n <= 4 * groups          # one count per sequence workgroup that gave up
    assert int(wl._turn[0]) == groups - 1          # both commits ran and released their turn
    for a, b in zip(_results(wl, 1), ref):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_queue_probe_and_group_stream_choice():
    """lantern_streams_share_queue: a stream shares a queue with itself; and when group_streams reports four distinct queues, no two of its streams do."""
    from lantern_amd import harness as HN
    dev = torch.device("cuda")
    streams = HN.group_streams(dev, 4)
    rep = HN.group_streams_report(dev)
    print("group streams:", rep)
    assert len(streams) == 4 and len({s.cuda_stream for s in streams}) == 4 and rep["requested"] == 4
    assert HN.streams_share_queue(streams[0], streams[0])
    if rep["distinct_queues"]:
        for i in range(4):
            for j in range(4):
                if i != j:
                    assert not HN.streams_share_queue(streams[i], streams[j]), (i, j)
    else:          # fewer than four hardware queues in this environment: the harness said so
        assert rep["queues_found"] < 4
