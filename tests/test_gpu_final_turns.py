"""A batch's final-hop launches take turns on its two final streams (flag batch_final_turns, engine.cpp
FinalStreamScope).

With the flag at 1 every final-hop launch of a pipelined ngx_go_batch (a single hop, a pair, a held hop that
is flushed) goes to the final stream the launch before it did not use; with 0 query i's launch is on final
stream i & 1, so with pairing on every pair kernel (launched by its odd query) is on the second stream. The
read-only counters final_launches_s0 / final_launches_s1 count the launches enqueued per stream. Every case
compares every query's code, rows, scanned edges and row digest with ngx_go of the same plan.

The graph is RmatDataset(12) with in-edges and pull_factor 1 (tests/test_gpu_batch_pair.py), so hop 2 of a
3-step query pulls and its final hop is dense.
"""
import pytest

from nebula_amd import engine, ngql
from tests import fixtures
from tests.test_gpu_batch_pair import Q, Q_ONE_STEP, SCALE, _alone, _prep, _seeds, _text

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rmat():
    ds = fixtures.RmatDataset(SCALE, with_in=True)
    e = engine.Engine(0)
    ds.load_engine(e)
    e.set_flag("pull_factor", 1)
    yield ds, e
    e.close()


def _run(e, preps, want):
    """One batch: every query as alone; the launches it enqueued on final stream 0 and 1, its paired launches."""
    s0, s1, p0 = e.get_flag("final_launches_s0"), e.get_flag("final_launches_s1"), e.get_flag("paired_finals")
    got = e.go_batch(preps, digests=True)
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g[0], g[1], g[2], tuple(g[3])) == w, (i, g, w)
    return (e.get_flag("final_launches_s0") - s0, e.get_flag("final_launches_s1") - s1,
            e.get_flag("paired_finals") - p0)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8])
def test_seeds_only(rmat, n):
    """Plans that differ in their seeds only: n // 2 pair launches and the odd tail's single one. Twice per flag
    value in one context (lanes, pending closes and the turn carry over from batch to batch)."""
    ds, e = rmat
    assert e.get_flag("batch_final_turns") == 1          # the default
    preps = [_prep(e, ds.space, _text(Q, _seeds(100 + i))) for i in range(n)]
    want = _alone(e, ds.space, preps)
    try:
        for flag in (1, 0):
            e.set_flag("batch_final_turns", flag)
            assert e.get_flag("batch_final_turns") == flag
            for _ in range(2):
                s0, s1, paired = _run(e, preps, want)
                assert paired == n // 2
                if n == 1:
                    assert (s0, s1) == (0, 0)                         # one plan is not pipelined: no final stream
                    continue
                assert s0 + s1 == n // 2 + n % 2, (flag, s0, s1)
                if flag:
                    assert abs(s0 - s1) <= 1 and s0 >= s1, (s0, s1)   # n = 8: 2 and 2
                else:
                    # the parent's rule: a pair is launched by its odd query on stream 1, the odd tail on stream 0
                    assert (s0, s1) == (n % 2, n // 2), (s0, s1)
    finally:
        e.set_flag("batch_final_turns", 1)


@pytest.fixture(scope="module")
def mixed(rmat):
    """Pairable plans, another literal, 1-step plans and a query that exits on an empty frontier, interleaved:
    (0, 1) pair; 2 holds and 3 has another literal (flush, then single); 4 holds and 5 is not dense (flush, then
    single); 6 holds and 7 never reaches a final hop (the batch loop flushes); 8, 9 single; 10 the odd tail."""
    ds, e = rmat
    nowhere = None
    for v in (4095, 4094, 4093, 4091, 4087, (1 << SCALE) + 12345):
        r = e.go(ds.space, ngql.parse_go(f"GO FROM {v} OVER e YIELD e._dst"))
        if r.ok and not r.rows:
            nowhere = [v]
            break
    assert nowhere is not None
    texts = [_text(Q, _seeds(120)), _text(Q, _seeds(121)), _text(Q, _seeds(122), 30), _text(Q, _seeds(123)),
             _text(Q, _seeds(124)), _text(Q_ONE_STEP, _seeds(125)), _text(Q, _seeds(126)), _text(Q, nowhere),
             _text(Q_ONE_STEP, _seeds(128)), _text(Q, _seeds(129)), _text(Q, _seeds(130))]
    preps = [_prep(e, ds.space, t) for t in texts]
    return preps, _alone(e, ds.space, preps)


@pytest.mark.parametrize("flag", [1, 0])
def test_mixed_batch(rmat, mixed, flag):
    """Every prefix of the mixed batch: results as alone, and with the flag the two streams' launch counts never
    differ by more than one whatever kind of launch came last (strict alternation per launch)."""
    ds, e = rmat
    preps, want = mixed
    e.set_flag("batch_final_turns", flag)
    try:
        for n in range(2, len(preps) + 1):
            s0, s1, paired = _run(e, preps[:n], want[:n])
            assert paired == 1, (n, paired)                              # only (0, 1) pairs
            # every query but the one that exits launches one final hop; the pair's two share a launch
            assert s0 + s1 == n - 1 - (1 if n > 7 else 0), (n, s0, s1)
            if flag:
                assert s0 - s1 in (0, 1), (n, s0, s1)                    # stream 0 first, then in turns
    finally:
        e.set_flag("batch_final_turns", 1)


@pytest.fixture(scope="module")
def five(rmat):
    ds, e = rmat
    preps = [_prep(e, ds.space, _text(Q, _seeds(140 + i))) for i in range(5)]
    return preps, _alone(e, ds.space, preps)


@pytest.mark.parametrize("name,value,default", [("batch_finals", 1, 2), ("batch_lanes", 2, 4), ("batch_lanes", 3, 4),
                                                ("batch_lanes", 4, 4), ("resv_groups", 4, 8)])
@pytest.mark.parametrize("flag", [1, 0])
def test_configurations(rmat, five, name, value, default, flag):
    """One final stream (nothing alternates: every launch on it), 2 to 4 lanes (a lane's next final hop waits for
    its last close, on whichever stream that ran), 4 reservation groups."""
    ds, e = rmat
    preps, want = five
    e.set_flag(name, value)
    e.set_flag("batch_final_turns", flag)
    try:
        for _ in range(2):
            s0, s1, paired = _run(e, preps, want)
            assert paired == 2
            if name == "batch_finals":
                assert (s0, s1) == (3, 0)
            elif flag:
                assert (s0, s1) == (2, 1)
            else:
                assert (s0, s1) == (1, 2)
    finally:
        e.set_flag(name, default)
        e.set_flag("batch_final_turns", 1)


def test_poisoned_scratch():
    """Five plans on an engine whose scratch buffers are filled with 0xA5 (flag poison_buffers), with the flag
    at 1 and at 0: no launch reads a word that its own stream's waits did not order behind its writer."""
    ds = fixtures.RmatDataset(SCALE, with_in=True)
    e = engine.Engine(0)
    try:
        e.set_flag("poison_buffers", 1)
        ds.load_engine(e)
        e.set_flag("pull_factor", 1)
        preps = [_prep(e, ds.space, _text(Q, _seeds(160 + i))) for i in range(5)]
        want = _alone(e, ds.space, preps)
        for flag in (1, 0):
            e.set_flag("batch_final_turns", flag)
            s0, s1, paired = _run(e, preps, want)
            assert paired == 2 and s0 + s1 == 3
    finally:
        e.set_flag("poison_buffers", 0)
        e.close()
