"""`GO ... | GROUP BY ... YIELD <aggregates>` with the grouping on the device (ngx_go_group_by) against the
host restatement of GroupByExecutor (nebula_amd/groupby.py) over the oracle's rows, and the reference's
GroupByLimitTest answers through the Engine backend.

Integers, keys, counts and types must match exactly. Double SUM / AVG: for a group with values x1..xn,
|device - host| <= (n - 1) * 2^-52 * sum|xi| (two summation orders, each within gamma_(n-1) * sum|x|), for
AVG that bound / n + 2^-52 * |avg|; computed per group from the oracle's rows. Every query must raise the
counter flag group_by_device by one, so a silent fall-back to the host fails, and runs under group_lds_max = 0
(global atomics) and a value past every group count (LDS aggregation where the state fits a workgroup's LDS);
the counter flag group_by_lds shows which path ran."""
import ctypes

import pytest

from nebula_amd import datagen, engine, groupby, kvfmt, ngql, pipeline
from oracle import oracle
from tests import fixtures
from tests.golden.groupby_cases import CASES

pytestmark = pytest.mark.gpu
EDGES = ["serve", "like", "teammate"]
EPS = 2.0 ** -52
LDS = pytest.mark.parametrize("lds_max", [0, 1 << 20], ids=["global", "lds"])
LDS_BYTES = 64 * 1024                                             # kernels.h kGroupLdsBytes

GO = ("GO 2 STEPS FROM {S} OVER e YIELD e._dst AS d, e.p0 AS a, e.p1 AS b, (double)(e.p0 * 0.5) AS x, "
      "$$.vt.name AS s, (int)(e.p0 % 7) AS k, e._rank AS r")   # the casts give the columns a static type
GROUPS = {
    "low": "GROUP BY $-.k YIELD $-.k, COUNT(*), SUM($-.a), AVG($-.a), MAX($-.b), MIN($-.b), BIT_AND($-.a), "
           "BIT_OR($-.a), BIT_XOR($-.b), COUNT_DISTINCT($-.a), SUM($-.d), MAX($-.d), MIN($-.d), COUNT($-.s)",
    "high": "GROUP BY $-.d YIELD $-.d AS d, COUNT(*), SUM($-.b), COUNT_DISTINCT($-.a), MAX($-.a)",
    "two": "GROUP BY $-.k, $-.a YIELD $-.k, $-.a, COUNT(*), SUM($-.b), COUNT_DISTINCT($-.d)",
    "string": "GROUP BY $-.s YIELD $-.s AS name, COUNT($-.s), MIN($-.a), SUM($-.b), COUNT_DISTINCT($-.s)",
    "const": "GROUP BY $-.r YIELD $-.r, COUNT(*), SUM($-.a), COUNT_DISTINCT($-.k)",
    "double": "GROUP BY $-.k YIELD $-.k, SUM($-.x), AVG($-.x), MAX($-.x), MIN($-.x), COUNT_DISTINCT($-.x), "
              "BIT_OR($-.x), SUM(1.5), SUM(3), AVG(2), BIT_XOR(3), COUNT(1), 1+1 AS cal, COUNT_DISTINCT(*)",
}
# which yield columns are double sums / averages of which input column (name) in GROUPS["double"]
DOUBLE_COLS = {1: ("sum", "x"), 2: ("avg", "x"), 7: ("sum", 1.5)}


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


def wide_dataset():
    """650 out-edges `w`(val INT, cnt INT) of 5 vertices: vids past 2^15 and val in +-1.2 M (9 values, some
    negative), so compact results hold e._dst and val at 4 bytes; cnt at 1."""
    nparts, etype = 3, 11
    b = kvfmt.KVBatch()
    for i in range(5):
        for j in range(130):
            src, dst = 70001 + i, 100000 + 7 * j
            val = ((i * 131 + j * 977) % 9) * 300007 - 1200000
            b.put(kvfmt.edge_key(src % nparts + 1, src, etype, 0, dst), kvfmt.encode_row([kvfmt.INT, kvfmt.INT], [val, j % 5]))
    schemas = [fixtures.SchemaDef(True, etype, "w", [("val", kvfmt.INT), ("cnt", kvfmt.INT)])]
    return fixtures.Dataset(space=1, num_parts=nparts, schemas=schemas, batch=b)


@pytest.fixture(scope="module")
def wide():
    ds = wide_dataset()
    o = oracle.Oracle()
    ds.load_oracle(o)
    e = engine.Engine(0)
    ds.load_engine(e)
    yield ds, o, e
    e.close()
    o.close()


_HOST = {}


def host(o, ds, text):
    """The host restatement over the oracle's rows, computed once per query text."""
    if text not in _HOST:
        out = pipeline.run(o, ds.space, text)
        assert out.ok, out.error
        _HOST[text] = out
    return _HOST[text]


def device(e, ds, text, lds_max=-1, **kw):
    before = e.get_flag("group_by_device"), e.get_flag("group_by_lds")
    e.set_flag("group_lds_max", lds_max)
    try:
        out = pipeline.run(e, ds.space, text, **kw)
    finally:
        e.set_flag("group_lds_max", -1)
    assert out.ok, out.error
    return out, e.get_flag("group_by_device") - before[0], e.get_flag("group_by_lds") - before[1]


def same(got, want, nkeys, doubles=None, bounds=None):
    assert got.names == want.names
    assert list(got.col_types) == list(want.col_types)
    g, w = sorted(got.rows, key=lambda r: repr(r[:nkeys])), sorted(want.rows, key=lambda r: repr(r[:nkeys]))
    assert len(g) == len(w)
    for rg, rw in zip(g, w):
        for c, (cg, cw) in enumerate(zip(rg, rw)):
            if doubles and c in doubles:
                assert cg[0] == cw[0] == "double"
                assert abs(cg[1] - cw[1]) <= bounds[(rw[:nkeys], c)], (c, rw[:nkeys], cg[1], cw[1], bounds[(rw[:nkeys], c)])
            else:
                assert cg == cw, (c, rg, rw)


def nkeys_of(gb):
    return len(ngql.parse_group_by(gb).groups)


def lds_expected(lds_max, ngroups, nslots):
    """group_by_lds rises when the threshold admits the groups and the state words fit a workgroup's LDS."""
    return int(lds_max >= ngroups and 0 < ngroups * nslots * 8 <= LDS_BYTES)


def double_bounds(o, ds, go):
    """Per (group key k, yield column of GROUPS["double"]): the bound of the module docstring from the oracle's rows."""
    xs = {}
    for r in host(o, ds, go).rows:                                # per group (k): the x values
        xs.setdefault((r[5],), []).append(r[3][1])
    bounds = {}
    for key, v in xs.items():
        n = len(v)
        for c, (what, col) in DOUBLE_COLS.items():
            vals = v if col == "x" else [col] * n
            b = (n - 1) * EPS * sum(abs(t) for t in vals)
            if what == "avg":
                b = b / n + EPS * abs(sum(vals) / n)
            bounds[(key, c)] = b
    return bounds


@LDS
@pytest.mark.parametrize("name", ["low", "high", "two", "string", "const"])
def test_device_equals_host(rmat, name, lds_max):
    ds, o, e, seeds = rmat
    text = GO.replace("{S}", seeds) + " | " + GROUPS[name]
    want = host(o, ds, text)
    got, calls, lds = device(e, ds, text, lds_max)
    assert calls == 1
    assert len(host(o, ds, GO.replace("{S}", seeds)).rows) > 0
    assert len(want.rows) == 1 if name == "const" else len(want.rows) >= 2
    same(got, want, nkeys_of(GROUPS[name]))
    if lds_max == 0:
        assert lds == 0
    elif name in ("low", "const"):                                # a few groups: the state fits a workgroup's LDS
        assert lds == 1


@LDS
def test_double_columns_and_constants(rmat, lds_max):
    ds, o, e, seeds = rmat
    go = GO.replace("{S}", seeds)
    text = go + " | " + GROUPS["double"]
    want = host(o, ds, text)
    bounds = double_bounds(o, ds, go)
    got, calls, lds = device(e, ds, text, lds_max)
    assert calls == 1 and lds == (1 if lds_max else 0) and len(want.rows) >= 2
    same(got, want, 1, DOUBLE_COLS, bounds)


def _spec_run(e, ds, go_text, gb_text, compact, yield_only=True):
    s, g, spec = pipeline.Pipeline(e, ds.space)._device_spec(go_text, gb_text)
    return g, e.go(ds.space, s, group_by=spec, yield_only=yield_only, compact=compact)


WIDE_GO = "GO FROM 70001, 70002, 70003, 70004, 70005 OVER w YIELD w._dst AS d, w.val AS v, w.cnt AS c"


@LDS
@pytest.mark.parametrize("gb,nslots", [
    ("GROUP BY $-.v YIELD $-.v, COUNT(*), SUM($-.d), MIN($-.v), MAX($-.d), COUNT_DISTINCT($-.d), BIT_XOR($-.c)", 6),
    ("GROUP BY $-.d YIELD $-.d, SUM($-.v), BIT_AND($-.v), MIN($-.v), AVG($-.v)", 5),
    ("GROUP BY $-.c, $-.v YIELD $-.v, $-.c, COUNT(*), MAX($-.v)", 2),
], ids=["key4", "value4", "two"])
def test_four_byte_columns(wide, gb, nslots, lds_max):
    """Width 4: keys and values read as int32 and sign-extended (val is negative in 4 of its 9 values)."""
    ds, o, e = wide
    want = host(o, ds, WIDE_GO + " | " + gb)
    nrows = len(host(o, ds, WIDE_GO).rows)
    assert nrows == 650 and len(want.rows) >= 2
    assert any(c[1] < 0 for r in host(o, ds, WIDE_GO).rows for c in r[1:2])
    lds0 = e.get_flag("group_by_lds")
    e.set_flag("group_lds_max", lds_max)
    try:
        g, r = _spec_run(e, ds, WIDE_GO, gb, True)
    finally:
        e.set_flag("group_lds_max", -1)
    assert r.ok and r.go_nrows == nrows
    assert list(r.dev_widths[1]) == [4, 4, 1]
    assert e.get_flag("group_by_lds") - lds0 == lds_expected(lds_max, len(want.rows), nslots)
    assert sorted(r.rows, key=repr) == sorted(want.rows, key=repr)
    assert list(r.col_types) == list(want.col_types)


def test_compact_on_and_off_cover_every_width(rmat):
    """compact: e._dst at 2 bytes, e.p0 at 1, e._rank a constant (width 0), computed columns at 8; without it
    every column at 8. Width 4 is test_four_byte_columns' (a scale-11 graph has no 4-byte column)."""
    ds, o, e, seeds = rmat
    go = GO.replace("{S}", seeds)
    want = host(o, ds, go + " | " + GROUPS["low"])
    widths = set()
    for compact, yo in ((True, True), (False, True), (False, False)):
        g, r = _spec_run(e, ds, go, GROUPS["low"], compact, yo)
        assert r.ok and r.go_nrows == len(host(o, ds, go).rows)
        widths |= set(r.dev_widths[1])
        assert sorted(r.rows, key=repr) == sorted(want.rows, key=repr)
        assert list(r.col_types) == list(want.col_types)
    assert {0, 1, 2, 8} <= widths


@LDS
@pytest.mark.parametrize("go", [
    "GO 1 TO 3 STEPS FROM {S} OVER e BIDIRECT WHERE e.p0 > 60 YIELD e._dst AS d, e.p0 AS a, e.p1 AS b",
    "GO 2 STEPS FROM {S} OVER e REVERSELY YIELD e._dst AS d, e.p0 AS a, e.p1 AS b",
    "GO 2 STEPS FROM {S} OVER e WHERE e.p1 % 1000 < 613 YIELD e._dst AS d, e.p0 AS a, e.p1 AS b",
    "GO 2 STEPS FROM {S} OVER e WHERE e.p1 % 1000 < 614 YIELD e._dst AS d, e.p0 AS a, e.p1 AS b",
], ids=["m_to_n_bidirect", "reversely", "where613", "where614"])
def test_directions_and_record_hops(rmat, go, lds_max):
    ds, o, e, seeds = rmat
    for gb, nslots in (("GROUP BY $-.a YIELD $-.a, COUNT(*), SUM($-.b), MAX($-.d)", 3),
                       ("GROUP BY $-.d YIELD $-.d, COUNT(*), BIT_XOR($-.a)", 2)):
        text = go.replace("{S}", seeds) + " | " + gb
        want = host(o, ds, text)
        got, calls, lds = device(e, ds, text, lds_max)
        assert calls == 1 and len(want.rows) >= 2
        assert lds == lds_expected(lds_max, len(want.rows), nslots)
        same(got, want, 1)


def test_a_row_count_off_the_block_size(rmat):
    ds, o, e, seeds = rmat
    ns = [len(host(o, ds, "GO 2 STEPS FROM %s OVER e WHERE e.p1 %% 1000 < %d YIELD e._dst AS d, e.p0 AS a, e.p1 AS b"
                   % (seeds, t)).rows) for t in (613, 614)]
    assert any(n % 256 for n in ns) and all(n > 256 for n in ns)


@LDS
def test_zero_rows(rmat, lds_max):
    ds, o, e, seeds = rmat
    text = "GO FROM %s OVER e WHERE e.p0 < 0 YIELD e._dst AS d, e.p0 AS a | GROUP BY $-.d YIELD $-.d, COUNT(*), SUM($-.a) AS t" % seeds
    got, calls, lds = device(e, ds, text, lds_max)
    assert calls == 1 and lds == 0                                # no row, no kernel
    assert got.rows == [] and got.names == ["$-.d", "COUNT(*)", "t"] and list(got.col_types) == []


@LDS
@pytest.mark.parametrize("case", CASES, ids=[f"L{c['line']}" for c in CASES])
def test_known_answers_through_engine(nba, case, lds_max):
    ds, o, e = nba
    before = e.get_flag("group_by_device"), e.get_flag("group_by_lds")
    e.set_flag("group_lds_max", lds_max)
    try:
        out = pipeline.run(e, ds.space, fixtures.nba_query(case["query"]), EDGES)
    finally:
        e.set_flag("group_lds_max", -1)
    assert out.ok, out.error
    assert e.get_flag("group_by_device") - before[0] == (1 if case["device"] else 0)
    # the device-eligible cases all have aggregates over a handful of groups: their state fits the LDS
    assert e.get_flag("group_by_lds") - before[1] == (1 if case["device"] and lds_max else 0)
    if "names" in case:
        assert out.names == case["names"]
    got = fixtures.normalize_cells(out.rows)
    assert got == ([] if case.get("empty") else fixtures.nba_expected(case["rows"]))


def test_lifetime_and_hygiene(rmat):
    """Two group-bys in a row with different specs, then a plain GO on the same context; device_group_by=False
    and the unsupported specs answer from the host path."""
    ds, o, e, seeds = rmat
    go = GO.replace("{S}", seeds)
    for name in ("two", "low", "string"):
        got, calls, _ = device(e, ds, go + " | " + GROUPS[name])
        assert calls == 1
        same(got, host(o, ds, go + " | " + GROUPS[name]), nkeys_of(GROUPS[name]))
    plain = e.go(ds.space, go)
    assert sorted(plain.rows, key=repr) == sorted(host(o, ds, go).rows, key=repr)
    got, calls, _ = device(e, ds, go + " | " + GROUPS["low"], device_group_by=False)
    assert calls == 0
    same(got, host(o, ds, go + " | " + GROUPS["low"]), 1)
    # STD on the host runs over the engine's rows, whose order is not the oracle's: its sum of n squares (all
    # >= 0, so each order is within gamma_n of the exact sum; the mean is an exact integer sum / n) and the
    # square root leave |a - b| <= (n + 2) * 2^-52 * value
    gb = "GROUP BY $-.k YIELD $-.k, STD($-.a), COUNT(*)"
    got, calls, _ = device(e, ds, go + " | " + gb)
    want = host(o, ds, go + " | " + gb)
    assert calls == 0
    same(got, want, 1, {1: "std"}, {(r[:1], 1): (r[2][1] + 2) * EPS * r[1][1] for r in want.rows})
    for gb in ("GROUP BY $-.k, abs(5) YIELD $-.k, COUNT(*)",       # a function key
               "GROUP BY $-.x YIELD $-.x, COUNT(*)",               # a DOUBLE key: E_UNSUPPORTED from the library
               "GROUP BY $-.k YIELD $-.k, AVG($-.d)"):             # AVG of a VID column
        got, calls, _ = device(e, ds, go + " | " + gb)
        assert calls == 0
        same(got, host(o, ds, go + " | " + gb), nkeys_of(gb))


@pytest.mark.parametrize("gb,reason", [
    ("GROUP BY $-.x YIELD $-.x, COUNT(*)", "DOUBLE key"),
    ("GROUP BY $-.k YIELD $-.k, AVG($-.d)", "AVG of a VID"),
    ("GROUP BY $-.k YIELD $-.k, MAX($-.s)", "MAX / MIN of a BOOL or STRING"),
    ("GROUP BY $-.d, $-.a, $-.b, $-.k, $-.r YIELD COUNT(*)", None),   # five keys: refused before the library
])
def test_unsupported_specs_name_their_reason(rmat, gb, reason):
    ds, o, e, seeds = rmat
    go = GO.replace("{S}", seeds)
    plan = pipeline.Pipeline(e, ds.space)._device_spec(go, gb)
    if reason is None:
        assert plan is None
        return
    s, g, spec = plan
    r = e.go(ds.space, s, group_by=spec, yield_only=True, compact=True)
    assert not r.ok and r.code == engine.E_UNSUPPORTED and reason in r.error


UNCAST_GO = "GO 2 STEPS FROM {S} OVER e YIELD e.p0 % 7 AS u, e.p1 AS b"   # u: a per-row (UNKNOWN) type
COUNT_STAR = ("COUNT", -1, "*")


@pytest.mark.parametrize("go,spec,reason", [
    # plans Pipeline never sends (_device_spec stops them first), built by hand for the library's own checks;
    # GO's columns: d 0, a 1, b 2, x 3, s 4, k 5, r 6
    (GO, engine.GroupBySpec([5], [("", 5, None), ("STD", 1, None)]), "STD"),
    (GO, engine.GroupBySpec([0, 1, 2, 5, 6], [COUNT_STAR]), "more than 4 keys"),
    (GO, engine.GroupBySpec([5], [COUNT_STAR] * 65), "more than 64 yields"),
    (GO, engine.GroupBySpec([3], [COUNT_STAR]), "DOUBLE key"),
    (UNCAST_GO, engine.GroupBySpec([0], [("", 0, None), COUNT_STAR]), "UNKNOWN-typed"),
    (UNCAST_GO, engine.GroupBySpec([1], [("SUM", 0, None)]), "UNKNOWN-typed"),
], ids=["std", "five_keys", "65_yields", "double_key", "unknown_key", "unknown_value"])
def test_the_library_refuses_with_a_reason(rmat, go, spec, reason):
    ds, o, e, seeds = rmat
    before = e.get_flag("group_by_device")
    r = e.go(ds.space, go.replace("{S}", seeds), group_by=spec, yield_only=True, compact=True)
    assert not r.ok and r.code == engine.E_UNSUPPORTED and reason in r.error
    assert e.get_flag("group_by_device") == before
    plain = "GO FROM %s OVER e YIELD e._dst AS d" % seeds        # the context answers the next query
    assert sorted(e.go(ds.space, plain).rows) == sorted(host(o, ds, plain).rows)


def test_an_uncast_key_answers_from_the_host(rmat):
    """`e.p0 % 7` without a cast is UNKNOWN-typed: Pipeline sends it, the library refuses, the host groups."""
    ds, o, e, seeds = rmat
    text = UNCAST_GO.replace("{S}", seeds) + " | GROUP BY $-.u YIELD $-.u, COUNT(*), SUM($-.b), MAX($-.b)"
    assert pipeline.Pipeline(e, ds.space)._device_spec(*text.split(" | ")) is not None
    got, calls, _ = device(e, ds, text)
    want = host(o, ds, text)
    assert calls == 0 and len(want.rows) == 7
    same(got, want, 1)


def test_world_2_is_refused():
    """A shard of a two-shard world: group states of the shards would have to merge (a later step)."""
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
                 group_by=engine.GroupBySpec([1], [("", 1, None), COUNT_STAR]))
        assert not r.ok and r.code == engine.E_UNSUPPORTED and "world > 1" in r.error and r.go_nrows > 0
        assert e.get_flag("group_by_device") == 0
    finally:
        e.close()


def test_poisoned_scratch_gives_the_same_rows(rmat):
    """Fresh scratch filled with a poison byte (flag poison_buffers): nothing is read before it is written."""
    ds, o, _, seeds = rmat
    go = GO.replace("{S}", seeds)
    e = engine.Engine(0)
    try:
        e.set_flag("poison_buffers", 1)
        ds.load_engine(e)
        for name in ("low", "string", "double"):
            got, calls, _ = device(e, ds, go + " | " + GROUPS[name])
            assert calls == 1
            if name == "double":
                same(got, host(o, ds, go + " | " + GROUPS[name]), 1, DOUBLE_COLS, double_bounds(o, ds, go))
            else:
                same(got, host(o, ds, go + " | " + GROUPS[name]), nkeys_of(GROUPS[name]))
    finally:
        e.set_flag("poison_buffers", 0)
        e.close()
