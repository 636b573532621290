"""Two batch queries' dense final hops in one launch (flag batch_pair_finals, final_kernels.h finalBodyDense2).

ngx_go_batch holds the dense, loads-first final hop of query 2k and launches it together with query 2k + 1's
when the two differ in their seeds only; anything else makes the held hop run alone, as without the flag.
Every case runs its batch with the flag at 1 and at 0 and compares every query's code, rows, scanned edges
and row digest with ngx_go of the same plan; the read-only counters paired_finals and dense_early_finals
say which launches ran.

The graph is RmatDataset(12) with in-edges and pull_factor 1 (tests/test_gpu_dense_early.py,
tests/test_gpu_pull.py::test_dense_final_hop), so hop 2 of a 3-step query pulls and its final hop is dense.
"""
import pytest

from nebula_amd import datagen, engine, ngql
from tests import fixtures
from tests.test_gpu_dense_early import SPACE as CSR_SPACE, CsrGraph

pytestmark = pytest.mark.gpu

Q = "GO 3 STEPS FROM {S} OVER e WHERE e.p0 < {K} YIELD e._dst, e._rank, e.p0, e.p1"
Q_OTHER_YIELD = "GO 3 STEPS FROM {S} OVER e WHERE e.p0 < {K} YIELD e._dst, e.p1"
Q_ONE_STEP = "GO FROM {S} OVER e WHERE e.p0 < {K} YIELD e._dst, e._rank, e.p0, e.p1"
SCALE = 12


def _text(q, seeds, k=50):
    return q.replace("{S}", ", ".join(str(int(v)) for v in seeds)).replace("{K}", str(k))


def _seeds(i, n=30):
    return datagen.rmat_seeds(SCALE, n, 16, 42, 300 + i)


@pytest.fixture(scope="module")
def rmat():
    ds = fixtures.RmatDataset(SCALE, with_in=True)
    e = engine.Engine(0)
    ds.load_engine(e)
    e.set_flag("pull_factor", 1)
    yield ds, e
    e.close()


def _prep(e, space, text):
    return e.prepare_go(space, ngql.parse_go(text), on_device=True, compact=True, yield_only=True)


def _alone(e, space, preps):
    """Each plan through ngx_go: (code, rows, edges, digest) as go_batch reports them."""
    out = []
    for p in preps:
        r = e.go(space, p, rows=False, device_digest=True)
        assert r.ok
        assert len(r.hop_edges) == len(r.hop_frontier)
        out.append((0, r.nrows, sum(r.hop_edges), tuple(r.device_digest)))
    return out


def _batch(e, space, preps, pairs, early, want=None, times=1):
    """The batch with the flag at 1 and at 0, `times` times each: every query as alone; `pairs` paired launches
    with the flag (none without), `early` loads-first final hops either way."""
    want = want or _alone(e, space, preps)
    try:
        for flag in (1, 0):
            e.set_flag("batch_pair_finals", flag)
            assert e.get_flag("batch_pair_finals") == flag
            for _ in range(times):
                p0, x0 = e.get_flag("paired_finals"), e.get_flag("dense_early_finals")
                got = e.go_batch(preps, digests=True)
                paired, ran_early = e.get_flag("paired_finals") - p0, e.get_flag("dense_early_finals") - x0
                for i, (g, w) in enumerate(zip(got, want)):
                    assert (g[0], g[1], g[2], tuple(g[3])) == w, (flag, i, g, w)
                assert paired == (pairs if flag else 0), (flag, paired)
                assert ran_early == early, (flag, ran_early)
    finally:
        e.set_flag("batch_pair_finals", 1)              # the default
    return want


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_seeds_only(rmat, n):
    """Plans that differ in their seeds only pair two by two; the last of an odd batch runs single. Twice in
    one context: the lanes, their pending closes and the reservation tags carry over from batch to batch."""
    ds, e = rmat
    preps = [_prep(e, ds.space, _text(Q, _seeds(i))) for i in range(n)]
    _batch(e, ds.space, preps, pairs=n // 2, early=n, times=2)
    if n == 5:
        # no fewer waves per SIMD than the single kernel's 8 (512 / 8 registers), as DESIGN §6.1 states
        assert 0 < e.get_flag("jit_dense2_vgprs") <= 64
        assert e.get_flag("jit_dense2_scratch") == 0


def test_other_yield_is_another_module(rmat):
    ds, e = rmat
    preps = [_prep(e, ds.space, _text(Q_OTHER_YIELD if i & 1 else Q, _seeds(10 + i))) for i in range(4)]
    _batch(e, ds.space, preps, pairs=0, early=4)


def test_other_literal_same_module(rmat):
    """e.p0 < 50 and e.p0 < 30 share the generated module (the literal travels in the arguments): no pair."""
    ds, e = rmat
    c0 = e.get_flag("jit_compiled")
    preps = [_prep(e, ds.space, _text(Q, _seeds(20 + i), 30 if i & 1 else 50)) for i in range(4)]
    want = _batch(e, ds.space, preps, pairs=0, early=4)
    assert e.get_flag("jit_compiled") - c0 <= 1
    assert want[0][1] != want[1][1]


def test_second_query_exits_early(rmat):
    """Query 2k + 1 starts from a vertex without out-edges: no frontier from hop 1 on (GO_EXIT), it never reaches
    its final hop, and the held hop of query 2k runs alone."""
    ds, e = rmat
    # (RMAT leaves its highest vertices without out-edges; failing those, a vid the space does not hold)
    nowhere = None
    for v in (4095, 4094, 4093, 4091, 4087, (1 << SCALE) + 12345):
        r = e.go(ds.space, ngql.parse_go(f"GO FROM {v} OVER e YIELD e._dst"))
        if r.ok and not r.rows:
            nowhere = [v]
            break
    assert nowhere is not None
    preps = [_prep(e, ds.space, _text(Q, nowhere if i & 1 else _seeds(30 + i))) for i in range(4)]
    want = _batch(e, ds.space, preps, pairs=0, early=2)
    assert want[1][1] == 0 and want[0][1] > 0


def test_second_query_not_dense(rmat):
    """Query 2k + 1 is a 1-step plan: its final hop is not dense, so the held hop is flushed first."""
    ds, e = rmat
    preps = [_prep(e, ds.space, _text(Q_ONE_STEP if i & 1 else Q, _seeds(40 + i))) for i in range(5)]
    _batch(e, ds.space, preps, pairs=0, early=3)


@pytest.fixture(scope="module")
def five(rmat):
    ds, e = rmat
    preps = [_prep(e, ds.space, _text(Q, _seeds(50 + i))) for i in range(5)]
    return preps, _alone(e, ds.space, preps)


@pytest.mark.parametrize("flag,value,default", [("resv_groups", 4, 8), ("resv_groups", 8, 8), ("batch_finals", 1, 2),
                                                ("batch_finals", 2, 2), ("batch_lanes", 2, 4), ("batch_lanes", 3, 4),
                                                ("batch_lanes", 4, 4)])
def test_configurations(rmat, five, flag, value, default):
    """Reservation groups, one or two final streams (one: the closes on the close stream), 2 to 4 lanes (the
    held query keeps its lane until its pair has run)."""
    ds, e = rmat
    preps, want = five
    e.set_flag(flag, value)
    try:
        _batch(e, ds.space, preps, pairs=2, early=5, want=want)
    finally:
        e.set_flag(flag, default)


def test_rows_around_one_block():
    """Results of 2^16 - 1, 2^16 and 2^16 + 1 rows (one reservation block, kargs.h kResvShift) on a hand-built
    slot: seed rows point at 256 rows of degree 256 (or 255 of them and one of degree 255 or 257), GO 2 STEPS
    without a WHERE returns every edge of those rows."""
    V = 600
    adj = [[] for _ in range(V)]
    for r in range(1, 257):
        adj[r] = [(r * 7 + k) % 590 for k in range(256)]
    adj[257] = list(range(255))
    adj[258] = list(range(257))
    adj[590] = list(range(1, 256)) + [257]                 # 2^16 - 1 rows
    adj[591] = list(range(1, 257))                         # 2^16
    adj[592] = list(range(1, 256)) + [258]                 # 2^16 + 1
    adj[593] = list(range(2, 257))                         # another frontier for the second of a pair
    g = CsrGraph(adj)
    with engine.Engine(0) as e:
        g.load_engine(e)
        e.set_flag("pull_factor", 1)
        q = "GO 2 STEPS FROM {S} OVER e YIELD e._dst, e.p1"
        preps = [_prep(e, CSR_SPACE, q.replace("{S}", str(r + 1))) for r in (590, 591, 592, 593, 591, 590)]
        want = _batch(e, CSR_SPACE, preps, pairs=3, early=6)
        assert [w[1] for w in want[:3]] == [(1 << 16) - 1, 1 << 16, (1 << 16) + 1]


def test_poisoned_scratch():
    """A pair on an engine whose scratch buffers are filled with 0xA5 (flag poison_buffers): the paired kernel
    reads no word that nothing wrote."""
    ds = fixtures.RmatDataset(SCALE, with_in=True)
    e = engine.Engine(0)
    try:
        e.set_flag("poison_buffers", 1)
        ds.load_engine(e)
        e.set_flag("pull_factor", 1)
        preps = [_prep(e, ds.space, _text(Q, _seeds(60 + i))) for i in range(3)]
        _batch(e, ds.space, preps, pairs=1, early=3)
    finally:
        e.set_flag("poison_buffers", 0)
        e.close()
