"""CPU: lantern_verify_step refuses two groups of one call that would count into the same completion counters of a commit turn
(lantern_step_group.turn), before anything is launched."""
import ctypes as C

from lantern_amd import _lib

E_INVALID = -1


def _turn_groups(n):
    """n groups that pass the turn checks of their own (a turn block, KV slabs, turn_group in range); nothing else is filled in, and the pointers
    are never dereferenced: validation comes first."""
    arr = (_lib.StepGroup * n)()
    for g in range(n):
        s = arr[g]
        s.turn, s.slab_ptrs = 4096, 8192
        s.turn_group, s.turn_groups, s.turn_wait = g, n, g
    return arr


def test_duplicate_turn_group_under_one_turn_is_refused_before_any_launch():
    L = _lib.lib()
    arr = _turn_groups(3)
    arr[2].turn_group = 0
    assert L.lantern_verify_step(arr, 3) == E_INVALID
    msg = L.lantern_last_error()
    assert msg.startswith(b"verify_step: group 2, turn: ") and b"groups 0 and 2 share `turn` and turn_group 0" in msg, msg


def test_distinct_turn_groups_and_distinct_turn_blocks_pass_the_turn_check():
    """The same groups with distinct turn_group, or with equal turn_group under different turn blocks, get past the turn check: the call then fails at the
    first stage of the empty group 0, not at "turn".  Sharing a stream (all streams are 0 here) is legal."""
    L = _lib.lib()
    arr = _turn_groups(3)
    assert L.lantern_verify_step(arr, 3) == E_INVALID and L.lantern_last_error().startswith(b"verify_step: group 0, gather_candidates: ")
    arr[2].turn_group, arr[2].turn = 0, 3 * 4096
    assert L.lantern_verify_step(arr, 3) == E_INVALID and L.lantern_last_error().startswith(b"verify_step: group 0, gather_candidates: ")
