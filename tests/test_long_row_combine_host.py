"""Sizes behind the group-wise combine of long rows (csrc/agg_kernel.hpp), without a GPU: the workspace holds the
(group sum, residual) pairs behind the segment partials, the counter tensor the group tickets behind the row tickets.

Pair slots are cut on the global segment index — the group that starts at segment gs of a row that starts at s0 takes
slot 2 (gs // 16) + (gs == s0) — so the count depends on n_seg alone: 2 ((n_seg - 1) // 16) + 2 once a row CAN have two
groups (n_seg > 16), none before.  The same rule is checked here to give every group of every multi-group row a slot
of its own, inside that count, on random segment layouts."""
import numpy as np
import pytest

GROUP = 16


def _pair_slots(n_seg):
    return 2 * ((n_seg - 1) // GROUP) + 2 if n_seg > GROUP else 0


@pytest.mark.parametrize("in_norm", [0, 1])
@pytest.mark.parametrize("n_seg", [0, 16, 17, 33, 257])
def test_workspace_holds_partials_and_group_pairs(n_seg, in_norm):
    from stag_amd import _lib
    lib = _lib.lib()
    for D in (4, 128, 512, 3 * 128):           # (3 D: the derivative outputs ride in the same rows)
        stride = D * (2 if in_norm else 1)
        want = (n_seg + 2 * _pair_slots(n_seg)) * stride * 4
        assert lib.stag_plan_workspace_bytes(n_seg, D, in_norm) == want, (n_seg, D, in_norm)
    assert [_pair_slots(n) for n in (0, 16, 17, 33)] == [0, 0, 4, 6]


@pytest.mark.parametrize("n_seg", [0, 16, 17, 33])
def test_counter_count_holds_row_and_group_tickets(n_seg):
    from stag_amd import ops
    assert ops._COMBINE_GROUP == GROUP
    for tiles in (1, 2):
        for n_long in ((0,) if n_seg == 0 else (1, 3)):
            got = ops._counter_count(n_long, n_seg, tiles)
            assert got >= max(n_long, 1) * tiles                       # the row counters, [tiles][n_long]
            if n_seg > GROUP:                                          # a group counter at every segment index, per tile
                assert got == tiles * n_long + tiles * n_seg
                # the last group counter a kernel can address: tile tiles - 1, a group that starts at the last segment
                assert tiles * n_long + (tiles - 1) * n_seg + (n_seg - 1) < got
            else:
                assert got == max(n_long, 1) * tiles                   # no row has two groups: as before


def test_pair_slots_are_disjoint():
    rng = np.random.default_rng(3)
    for _ in range(200):
        lens = rng.integers(2, 60, rng.integers(1, 12))                # segments per long row, rows back to back
        ptr = np.concatenate([[0], np.cumsum(lens)])
        n_seg, used = int(ptr[-1]), set()
        for s0, s1 in zip(ptr[:-1], ptr[1:]):
            if s1 - s0 <= GROUP:
                continue                                               # one group: no pair
            for gs in range(s0, s1, GROUP):
                slot = 2 * (gs // GROUP) + (1 if gs == s0 else 0)
                assert slot not in used and slot < _pair_slots(n_seg)
                used.add(slot)
