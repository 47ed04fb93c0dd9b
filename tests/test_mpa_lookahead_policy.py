"""pathfit.mpa.lookahead_depth: how many iterations the next MPA sweep covers, as a pure function of the acceptance history, the
"mpa_lookahead" cap and the iterations left (no GPU, no library)."""
import pytest


def _mpa():
    from pathfit import mpa
    return mpa


def test_off_means_the_plain_sweep():
    m = _mpa()
    for hist in ([], [0], [5, 0, 0], [0, m.STALE]):
        assert m.lookahead_depth(hist, 0, 10) == 0
        assert m.lookahead_depth(hist, 0, 10, always=True) == 0


def test_only_after_a_quiet_iteration():
    m = _mpa()
    assert m.lookahead_depth([], 8, 20) == 1                   # nothing is known before the first iteration
    assert m.lookahead_depth([953], 8, 19) == 1
    assert m.lookahead_depth([953, 0, 3], 8, 17) == 1          # an earlier quiet iteration does not count
    assert m.lookahead_depth([953, 3, 0], 8, 17) == 8
    assert m.lookahead_depth([0], 8, 19) == 8


@pytest.mark.parametrize("cap,left,want", [(8, 20, 8), (8, 8, 8), (8, 7, 7), (8, 2, 2), (8, 1, 1), (3, 20, 3), (1, 20, 1), (16, 6, 6)])
def test_depth_is_the_cap_but_never_past_the_end(cap, left, want):
    m = _mpa()
    assert m.lookahead_depth([4, 0], cap, left) == want
    assert m.lookahead_depth([4, 7], cap, left, always=True) == want


def test_back_to_single_sweeps_after_a_stale_level():
    m = _mpa()
    h = [4, 0, 0, 1]                                            # ... the level after the accepting iteration is stale
    assert m.lookahead_depth(h + [m.STALE], 8, 10) == 1
    assert m.lookahead_depth(h + [m.STALE], 8, 10, always=True) == 1
    assert m.lookahead_depth(h + [m.STALE, 6], 8, 9) == 1       # until the next quiet iteration
    assert m.lookahead_depth(h + [m.STALE, 6, 0], 8, 8) == 8
    assert m.lookahead_depth(h + [m.STALE, 6], 8, 9, always=True) == 8


def test_a_whole_run_never_sweeps_past_k():
    """Replay the policy over a run of K iterations with a given acceptance sequence, as MPA._sweep does: the iterations
    covered by the sweeps and the served levels are exactly 1 .. K, in order, each once."""
    m = _mpa()
    K = 20
    acc = [9, 8, 7, 0, 0, 2, 5, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    for cap, always in ((8, False), (3, False), (16, False), (3, True), (1, False)):
        hist, waiting, swept, served = [], 0, [], []
        for it in range(1, K + 1):
            took = False
            if waiting:
                if [a for a in hist if a != m.STALE][-1] == 0:     # the level is current: the iteration before accepted nothing
                    took, waiting = True, waiting - 1
                    served.append(it)
                else:
                    waiting = 0
                    hist.append(m.STALE)
            if not took:
                d = m.lookahead_depth(hist, cap, K - it + 1, always)
                assert 1 <= d <= min(cap, K - it + 1)
                swept.append((it, d))
                waiting = d - 1
            hist.append(acc[it - 1])
        assert sorted(served + [it for it, _ in swept]) == list(range(1, K + 1))
        assert all(it + d - 1 <= K for it, d in swept)
        if cap == 8 and not always:                                # sweeps at 5 (stale at 7), 9 (stale at 10), 11 (8 levels), 19 (2 left)
            assert [s for s in swept if s[1] > 1] == [(5, 8), (9, 8), (11, 8), (19, 2)] and served == [6] + list(range(12, 19)) + [20]
        if cap == 1:
            assert served == [] and len(swept) == K
