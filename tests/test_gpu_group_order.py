"""`GO ... | GROUP BY ... | ORDER BY ... | LIMIT ...` and `GO ... | GROUP BY ... | LIMIT ...` with grouping and
selection on the device in one call (ngx_go_group_order_by) against the same text run on the oracle through the
host restatements (nebula_amd/groupby.py, orderby.py).

Groups equal on every factor come out in no fixed order on either side, so a window is compared with
tests/test_gpu_orderby.py::same_window against the oracle's full set of group rows; where the factors hold every
key the rows are equal. Compared columns are integers, strings and double MAX / MIN (exact in any arrival order).
Every device case asserts that group_order_device rose by one and that group_by_device and order_by_device did
not move, so a silent fall-back to the two-step path fails."""
import ctypes

import pytest

from nebula_amd import datagen, engine, pipeline
from oracle import oracle
from tests import fixtures
from tests.test_gpu_orderby import same_window

pytestmark = pytest.mark.gpu
EDGES = ["serve", "like", "teammate"]
COLS = ("e._dst AS d, e.p0 AS a, e.p1 AS b, (double)(0 - e.p0 * 0.5) AS x, $$.vt.name AS s, (int)(e.p0 % 7) AS k, "
        "e._rank AS r")                                           # the casts give the columns a static type
GO = "GO 2 STEPS FROM {S} OVER e YIELD " + COLS
COUNTERS = ("group_order_device", "group_by_device", "order_by_device")


@pytest.fixture(scope="module")
def rmat():
    ds = fixtures.RmatDataset(11, with_in=True, with_tag=True)
    o = oracle.Oracle()
    o.set_flags(threads=8)
    ds.load_oracle(o)
    e = engine.Engine(0)
    ds.load_engine(e)
    seeds = ", ".join(str(int(v)) for v in datagen.sample_vids(91, 1 << ds.scale, 6))
    yield ds, o, e, seeds
    e.close()
    o.close()


@pytest.fixture(scope="module")
def nba():
    ds = fixtures.nba()
    o = oracle.Oracle()
    ds.load_oracle(o)
    e = engine.Engine(0)
    ds.load_engine(e)
    yield ds, o, e
    e.close()
    o.close()


_HOST = {}


def host(o, ds, text, **kw):
    """The oracle's answer through the host path, computed once per text and left unchanged."""
    key = (id(o), text)
    if key not in _HOST:
        out = pipeline.run(o, ds.space, text, order_limit=True, **kw)
        assert out.ok, out.error
        _HOST[key] = out
    return _HOST[key]


def device(e, ds, text, **kw):
    before = [e.get_flag(f) for f in COUNTERS]
    out = pipeline.run(e, ds.space, text, order_limit=True, **kw)
    assert out.ok, out.error
    return out, [e.get_flag(f) - b for f, b in zip(COUNTERS, before)]


def check(o, e, ds, go, gb, factors, offset, count, rose=(1, 0, 0), total=False, **kw):
    """factors: (GROUP BY column name, desc) pairs; none: LIMIT alone."""
    groups = host(o, ds, go + " | " + gb)
    ob = "ORDER BY " + ", ".join("$-.%s%s" % (n, " DESC" if d else "") for n, d in factors) + " | " if factors else ""
    text = go + " | " + gb + " | " + ob + ("LIMIT %d, %d" % (offset, count) if offset else "LIMIT %d" % count)
    want = host(o, ds, text)
    got, moved = device(e, ds, text, **kw)
    assert moved == list(rose)
    assert got.names == want.names == groups.names
    assert list(got.col_types) == list(want.col_types)
    idx = [(groups.names.index(n), d) for n, d in factors]
    same_window(got.rows, groups.rows, idx, offset, count)
    same_window(want.rows, groups.rows, idx, offset, count)
    if total:
        assert got.rows == want.rows
    return got, want


PLANS = {
    "count_desc": ("GROUP BY $-.d YIELD $-.d AS d, COUNT(*) AS c", [("c", True)], 0, 10, False),
    "sum_then_keys": ("GROUP BY $-.k, $-.a YIELD $-.k AS k, $-.a AS a, SUM($-.b) AS sb, MAX($-.x) AS mx",
                      [("sb", False), ("k", False), ("a", True)], 0, 25, True),
    "sum_then_keys_offset": ("GROUP BY $-.k, $-.a YIELD $-.k AS k, $-.a AS a, SUM($-.b) AS sb, MAX($-.x) AS mx",
                             [("sb", True), ("a", False), ("k", False)], 3, 20, True),
    "string_key_desc": ("GROUP BY $-.s YIELD $-.s AS name, COUNT(*) AS c, MIN($-.x) AS mx, COUNT_DISTINCT($-.a) AS da",
                        [("name", True)], 0, 15, True),
    "double_max_then_key": ("GROUP BY $-.d YIELD $-.d AS d, MAX($-.x) AS mx, COUNT(*) AS c", [("mx", False), ("d", True)], 5, 40, True),
    "limit_alone": ("GROUP BY $-.d YIELD $-.d AS d, COUNT(*) AS c, SUM($-.b) AS sb", [], 3, 20, False),
    "limit_alone_few": ("GROUP BY $-.k YIELD $-.k AS k, COUNT(*) AS c", [], 3, 20, False),
    "count_past_the_groups": ("GROUP BY $-.k YIELD $-.k AS k, COUNT(*) AS c, AVG($-.a) AS av", [("c", True), ("k", False)], 2, 20, True),
}


@pytest.mark.parametrize("plan", list(PLANS))
def test_device_equals_oracle(rmat, plan):
    ds, o, e, seeds = rmat
    gb, factors, offset, count, total = PLANS[plan]
    got, want = check(o, e, ds, GO.replace("{S}", seeds), gb, factors, offset, count, total=total)
    assert got.rows


def test_the_plans_reach_what_they_name(rmat):
    ds, o, e, seeds = rmat
    go = GO.replace("{S}", seeds)
    assert len(host(o, ds, go + " | " + PLANS["count_desc"][0]).rows) > 300      # a select over many groups
    assert len(host(o, ds, go + " | " + PLANS["limit_alone_few"][0]).rows) == 7  # the window ends past the groups


def test_zero_rows(rmat):
    ds, o, e, seeds = rmat
    go = "GO FROM %s OVER e WHERE e.p0 < 0 YIELD e._dst AS d, e.p0 AS a" % seeds
    got, want = check(o, e, ds, go, "GROUP BY $-.d YIELD $-.d AS d, SUM($-.a) AS sa", [("sa", True)], 0, 5)
    assert got.rows == [] and list(got.col_types) == []


def test_known_answer_on_the_nba_fixture(nba):
    ds, o, e = nba
    text = fixtures.nba_query("GO FROM {P:Tim Duncan}, {P:Tony Parker}, {P:Manu Ginobili}, {P:LaMarcus Aldridge} OVER like "
                              "YIELD $$.player.name AS name | GROUP BY $-.name YIELD $-.name AS name, COUNT(*) AS c "
                              "| ORDER BY $-.c DESC, $-.name | LIMIT 2")
    want = pipeline.run(o, ds.space, text, EDGES, order_limit=True)
    assert want.ok and len(want.rows) == 2 and want.rows[0][1][1] >= want.rows[1][1][1]
    got, moved = device(e, ds, text, edge_names=EDGES)
    assert moved == [1, 0, 0]
    assert (got.names, list(got.col_types), got.rows) == (want.names, list(want.col_types), want.rows)


# ----------------------------------------------------------------------------- fallbacks
class CountingGo:
    """Counts the backend's go calls (each is one ngx_go) for the length of a with block."""

    def __init__(self, e):
        self.e, self.calls = e, 0

    def __enter__(self):
        inner = self.e.go

        def go(*a, **kw):
            self.calls += 1
            return inner(*a, **kw)
        self.e.go = go
        return self

    def __exit__(self, *exc):
        del self.e.go


TOTAL_TAIL = [("c", True), ("k", False)]


def test_a_function_key_is_never_sent(rmat):
    ds, o, e, seeds = rmat
    gb = "GROUP BY $-.k, abs(5) YIELD $-.k AS k, COUNT(*) AS c"
    with CountingGo(e) as n:
        check(o, e, ds, GO.replace("{S}", seeds), gb, TOTAL_TAIL, 0, 3, rose=(0, 0, 0), total=True)
    assert n.calls == 1


def test_an_uncast_key_is_refused_by_the_group_stage(rmat):
    """`e.p0 % 7` without a cast is UNKNOWN-typed: sent, refused with `group by:`, answered by the plain host path
    without a try at the device GROUP BY (which would refuse again): two traversals."""
    ds, o, e, seeds = rmat
    go = "GO 2 STEPS FROM %s OVER e YIELD e.p0 %% 7 AS k, e.p1 AS b" % seeds
    gb = "GROUP BY $-.k YIELD $-.k AS k, COUNT(*) AS c"
    p = pipeline.Pipeline(e, ds.space, order_limit=True)
    s, g, gspec, ospec = p._group_order_spec(go, gb, "ORDER BY $-.c DESC, $-.k", "LIMIT 3")
    r = e.go(ds.space, s, group_by=gspec, order_by=ospec, yield_only=True, compact=True)
    assert not r.ok and r.code == engine.E_UNSUPPORTED and r.error.startswith("group by: UNKNOWN-typed")
    with CountingGo(e) as n:
        check(o, e, ds, go, gb, TOTAL_TAIL, 0, 3, rose=(0, 0, 0), total=True)
    assert n.calls == 2


def test_order_k_max_below_k_groups_on_the_device_and_orders_on_the_host(rmat):
    ds, o, e, seeds = rmat
    go = GO.replace("{S}", seeds)
    gb = "GROUP BY $-.k YIELD $-.k AS k, COUNT(*) AS c"
    kmax = e.get_flag("order_k_max")
    e.set_flag("order_k_max", 2)
    try:
        p = pipeline.Pipeline(e, ds.space, order_limit=True)
        s, g, gspec, ospec = p._group_order_spec(go, gb, "ORDER BY $-.c DESC, $-.k", "LIMIT 3")
        r = e.go(ds.space, s, group_by=gspec, order_by=ospec, yield_only=True, compact=True)
        assert not r.ok and r.code == engine.E_UNSUPPORTED and r.error.startswith("order by: offset + count above order_k_max")
        with CountingGo(e) as n:
            check(o, e, ds, go, gb, TOTAL_TAIL, 0, 3, rose=(0, 1, 0), total=True)
        assert n.calls == 2
        check(o, e, ds, go, gb, TOTAL_TAIL, 0, 2, total=True)     # K = 2: on the device
    finally:
        e.set_flag("order_k_max", kmax)


def test_the_switch_gives_the_two_step_path(rmat):
    ds, o, e, seeds = rmat
    go = GO.replace("{S}", seeds)
    gb = "GROUP BY $-.k YIELD $-.k AS k, COUNT(*) AS c"
    check(o, e, ds, go, gb, TOTAL_TAIL, 0, 3, rose=(0, 1, 0), total=True, device_group_order=False)
    check(o, e, ds, go, gb, [], 0, 3, rose=(0, 1, 0), device_group_order=False)
    check(o, e, ds, go, gb, TOTAL_TAIL, 0, 3, rose=(0, 0, 0), total=True, device_group_by=False)
    check(o, e, ds, go, gb, TOTAL_TAIL, 0, 3, rose=(0, 1, 0), total=True, device_order_by=False)


def test_order_by_without_limit_is_not_sent(rmat):
    ds, o, e, seeds = rmat
    text = GO.replace("{S}", seeds) + " | GROUP BY $-.k YIELD $-.k AS k, COUNT(*) AS c | ORDER BY $-.c DESC, $-.k"
    got, moved = device(e, ds, text)
    assert moved == [0, 1, 0] and got.rows == host(o, ds, text).rows and len(got.rows) == 7


def test_the_default_still_refuses_limit(rmat):
    ds, o, e, seeds = rmat
    text = GO.replace("{S}", seeds) + " | GROUP BY $-.k YIELD $-.k AS k, COUNT(*) AS c | LIMIT 3"
    before = [e.get_flag(f) for f in COUNTERS]
    with pytest.raises(pipeline.PipelineError, match="only GO sentences run in this path"):
        pipeline.run(e, ds.space, text)
    assert [e.get_flag(f) for f in COUNTERS] == [before[0], before[1] + 1, before[2]]    # grouped as before, then refused


def test_world_2_is_refused():
    """A shard of a two-shard world: the shards' group states would have to merge (a later step)."""
    def fn(user, op, send, recv, nbytes):
        if op == engine.XCHG_ALLGATHER:                           # commit: the peer (rank 1) holds no vertices
            ctypes.memmove(recv, send, nbytes)
            ctypes.memset(recv + nbytes, 0, nbytes)
            return 0
        return 1

    cb = engine.ExchangeFn(fn)
    e = engine.Engine(0, 0, 2, exchange=cb)
    try:
        rows = datagen.rmat(10, 8, 42, 100, False, False)
        e.add_space(datagen.RMAT_SPACE, 100)
        for is_edge, sid, name, fields in datagen.rmat_schemas():
            e.add_schema(datagen.RMAT_SPACE, is_edge, sid, name, fields)
        e.load_kv(datagen.RMAT_SPACE, *rows.arrays())
        e.commit(datagen.RMAT_SPACE)
        seeds = ", ".join(str(int(v)) for v in datagen.sample_vids(3, 1 << 10, 20))
        r = e.go(datagen.RMAT_SPACE, "GO FROM %s OVER e YIELD e._dst AS d, e.p0 AS a" % seeds,   # one hop: no exchange
                 group_by=engine.GroupBySpec([1], [("", 1, None), ("COUNT", -1, "*")]),
                 order_by=engine.OrderBySpec([(1, True)], 0, 10))
        assert not r.ok and r.code == engine.E_UNSUPPORTED and r.error.startswith("group by: world > 1") and r.go_nrows > 0
        assert [e.get_flag(f) for f in COUNTERS] == [0, 0, 0]
    finally:
        e.close()
