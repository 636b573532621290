"""A host model of the paired dense final hop's double row reservation (CPU).

`finalBodyDense2` (nebula_amd/csrc/final_kernels.h) serves two queries per workgroup. Each query is a
reservation stream of its own (its counters, its block table, its physical rows), and lane 0 of wave 0 takes
both reservations in the kernel's order of steps:

  1. resvTake(a), resvTake(b)        the chunk's virtual rows from its group's counter, per stream
  2. resvPublish(a), resvPublish(b)  every block the chunk owes is allocated and published
  3. resvAwait(a), resvAwait(b)      the block its first row lies in, when another chunk owes it

The model runs the workgroups as state machines under a random scheduler with a bounded number of resident
workgroups (dispatch order, any completion order) and asserts, per stream: every row is placed exactly once,
the close (tests/test_resv_model.py, the single-stream model's) fills the holes, and no workgroup ever waits
on a block whose publisher has not yet reserved — so a waiter's publisher is resident and publishes without
waiting (no cycle). A schedule in which nobody can move fails the test.
"""
import random

import pytest

from tests.test_resv_model import close

TAKE_A, TAKE_B, PUB_A, PUB_B, WAIT_A, WAIT_B, WRITE, DONE = range(8)


class Stream:
    def __init__(self, G, shift):
        self.G, self.shift, self.B = G, shift, 1 << shift
        self.counters = [0] * G
        self.phys = 0
        self.table = {}                            # (g, virtual block) -> physical block
        self.owed = set()                          # blocks some workgroup has reserved the first row of
        self.placed = {}

    def take(self, wg, n):
        g = wg % self.G
        if n == 0:
            return None                            # (the kernel takes nothing for an empty chunk)
        v = self.counters[g]
        self.counters[g] += n
        k0, k1 = v >> self.shift, (v + n - 1) >> self.shift
        if v & (self.B - 1) == 0:
            self.owed.add((g, k0))
        if k1 != k0:
            self.owed.add((g, k1))
        return g, v, n, k0, k1

    def alloc(self, g, k):
        assert (g, k) not in self.table            # each virtual block is allocated exactly once
        self.table[(g, k)] = self.phys >> self.shift
        self.phys += self.B

    def publish(self, t):
        if t is None:
            return
        g, v, n, k0, k1 = t
        if v & (self.B - 1) == 0:
            self.alloc(g, k0)
        if k1 != k0:
            self.alloc(g, k1)

    def ready(self, t):
        """Step 3 can complete. A block that is not there yet must be owed by a workgroup that has reserved."""
        if t is None:
            return True
        g, v, n, k0, k1 = t
        if (g, k0) in self.table:
            return True
        assert v & (self.B - 1) != 0               # its own blocks were published in step 2
        assert (g, k0) in self.owed, "waits on a block whose publisher has not reserved"
        return False

    def write(self, wg, t):
        if t is None:
            return
        g, v, n, k0, k1 = t
        first = (self.table[(g, k0)] << self.shift) + (v & (self.B - 1))
        split = ((k0 + 1) << self.shift) - v
        second = (self.table[(g, k1)] << self.shift) if k1 != k0 else 0
        for j in range(n):
            o = first + j if j < split else second + j - split
            assert o not in self.placed
            self.placed[o] = (wg, j)


def run_pair(rows_a, rows_b, G, shift, resident, rng):
    n = len(rows_a)
    sa, sb = Stream(G, shift), Stream(G, shift)
    state = [TAKE_A] * n
    takes = [[None, None] for _ in range(n)]
    started, live = 0, []
    while started < n or live:
        while started < n and len(live) < resident:     # dispatch order
            live.append(started)
            started += 1
        movable = []
        for wg in live:
            st = state[wg]
            if st == WAIT_A and not sa.ready(takes[wg][0]):
                continue
            if st == WAIT_B and not sb.ready(takes[wg][1]):
                continue
            movable.append(wg)
        assert movable, "every resident workgroup waits: a cycle"
        wg = rng.choice(movable)
        st = state[wg]
        if st == TAKE_A:
            takes[wg][0] = sa.take(wg, rows_a[wg])
        elif st == TAKE_B:
            takes[wg][1] = sb.take(wg, rows_b[wg])
        elif st == PUB_A:
            sa.publish(takes[wg][0])
        elif st == PUB_B:
            sb.publish(takes[wg][1])
        elif st == WRITE:
            sa.write(wg, takes[wg][0])
            sb.write(wg, takes[wg][1])
        state[wg] = st + 1
        if state[wg] == DONE:
            live.remove(wg)
    return sa, sb


def check_stream(s, rows, G, shift):
    B = 1 << shift
    assert s.phys % B == 0 and s.phys <= sum(rows) + G * B         # resvSlack: G partial blocks at most
    out, R = close(s.placed, s.counters, s.phys, s.table, G, shift)
    assert R == sum(rows)
    assert sorted(out) == list(range(R))                           # the close filled the holes: dense [0, R)
    assert sorted(out.values()) == sorted((w, j) for w, n in enumerate(rows) for j in range(n))


def rows_with_total(n_wg, total, B, rng, zero_every):
    """n_wg row counts (each <= B: a chunk's rows fit a block) that sum to `total`, some of them zero."""
    rows = [0] * n_wg
    idx = [i for i in range(n_wg) if zero_every == 0 or i % zero_every != 0] or [0]
    left = total
    while left:
        i = rng.choice(idx)
        add = min(left, B - rows[i], rng.choice([1, 2, B // 7 + 1, B // 2, B]))
        rows[i] += add
        left -= add
        if all(rows[k] == B for k in idx):
            break
    assert sum(rows) == total, "the workgroups cannot hold the total"
    return rows


@pytest.mark.parametrize("G", [4, 8, 16])
@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("seed", range(4))
def test_pair_reservation_around_one_block(G, delta, seed):
    """Row totals of 2^shift - 1, 2^shift and 2^shift + 1 per stream (and a multiple of it for the other), some
    workgroups without rows for one stream or for both."""
    rng = random.Random(7919 * G + 31 * seed + delta)
    shift = rng.choice([5, 6, 8])
    B = 1 << shift
    n_wg = rng.choice([3 * G + 1, 40, 97])
    rows_a = rows_with_total(n_wg, B + delta, B, rng, zero_every=3)
    rows_b = rows_with_total(n_wg, rng.choice([1, 3]) * B + delta, B, rng, zero_every=2)
    # workgroup 0 has rows for neither stream, 3 none for the first, 2 none for the second
    assert rows_a[0] == 0 and rows_b[0] == 0 and rows_a[3] == 0 and rows_b[2] == 0
    sa, sb = run_pair(rows_a, rows_b, G, shift, resident=rng.choice([1, 2, G, 2 * G + 1]), rng=rng)
    check_stream(sa, rows_a, G, shift)
    check_stream(sb, rows_b, G, shift)


@pytest.mark.parametrize("G", [4, 8, 16])
@pytest.mark.parametrize("seed", range(6))
def test_pair_reservation_random(G, seed):
    """Many blocks per group in both streams, independent row counts, random completion orders."""
    rng = random.Random(104729 * G + seed)
    shift = rng.choice([5, 6, 8])
    B = 1 << shift
    n_wg = rng.choice([5, 64, 300])
    pick = lambda: rng.choice([0, 0, 1, B // 3, B - 1, B, rng.randrange(B + 1)])
    rows_a = [pick() for _ in range(n_wg)]
    rows_b = [pick() for _ in range(n_wg)]
    sa, sb = run_pair(rows_a, rows_b, G, shift, resident=rng.choice([1, 3, 16, 64]), rng=rng)
    check_stream(sa, rows_a, G, shift)
    check_stream(sb, rows_b, G, shift)
