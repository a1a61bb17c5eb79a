"""core.ring_plan: how a persistent launch of K steps from step0 runs on a metric ring of R slots.  The kernels fold all of a
launch's steps into slot step0 % R and clear slot (step0 + K) % R for the launch after; the plan must never hand the C ABI a
launch it refuses (K a multiple of R), and must leave no stale counts in the slots the run passes through."""
import pytest

from wheeledlab_amd.core import ring_plan

STALE = "stale"


def _run(step0, K, R):
    """the ring after the planned launches, modelled slot by slot: a set of the steps booked there, or STALE (an earlier pass)"""
    segments, zero = ring_plan(step0, K, R)
    ring = [STALE] * R
    ring[step0 % R] = set()      # the launch's own slot was cleared by its predecessor
    for z in zero:
        ring[z] = set()
    for k0, k in segments:
        s = step0 + k0
        assert not (R > 1 and k > 0 and k % R == 0), "a launch the C ABI refuses (ring slot aliasing)"
        if k > 0:
            assert ring[s % R] is not STALE
            ring[s % R] |= set(range(k0, k0 + k))
        ring[(s + k) % R] = set()
    return segments, ring


@pytest.mark.parametrize("R", [1, 2, 3, 4, 7])
def test_ring_plan_over_a_grid(R):
    for step0 in range(0, 3 * R + 2):
        for K in range(0, 4 * R + 3):
            segments, zero = ring_plan(step0, K, R)
            assert zero == sorted(set(zero)) and all(0 <= z < R for z in zero)
            assert [k0 for k0, _ in segments] == [sum(k for _, k in segments[:i]) for i in range(len(segments))]
            assert sum(k for _, k in segments) == K
            split = R > 1 and K > 1 and K % R == 0
            assert segments == ([(0, 1), (1, K - 1)] if split else [(0, K)])
            if R == 1:
                assert zero == []
                continue
            _, ring = _run(step0, K, R)
            # every slot the run passes through (its steps' and the one after them) holds no stale counts
            for i in range(min(K + 1, R)):
                assert ring[(step0 + i) % R] is not STALE, (step0, K, R, i)
            booked = sorted(s for slot in ring if slot is not STALE for s in slot)
            if split:            # the second launch clears the first one's slot: the ring keeps steps 1 .. K - 1
                assert booked == list(range(1, K)), (step0, K, R)
            else:
                assert booked == list(range(K)) and (K == 0 or ring[step0 % R] == set(range(K))), (step0, K, R)


def test_ring_plan_examples():
    assert ring_plan(5, 3, 4) == ([(0, 3)], [2, 3])
    assert ring_plan(5, 8, 4) == ([(0, 1), (1, 7)], [0, 1, 2, 3])
    assert ring_plan(0, 8, 8) == ([(0, 1), (1, 7)], [2, 3, 4, 5, 6, 7])
    assert ring_plan(3, 1, 4) == ([(0, 1)], [])
    assert ring_plan(7, 5, 1) == ([(0, 5)], [])
    assert ring_plan(2, 0, 4) == ([(0, 0)], [])
