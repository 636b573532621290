"""`GO ... | ORDER BY ... | LIMIT ...` and `GO ... | LIMIT ...` with the selection on the device
(ngx_go_order_by) against the host restatement of OrderByExecutor / LimitExecutor (nebula_amd/orderby.py)
over the oracle's rows, and the reference's OrderByTest / GroupByLimitTest answers through the Engine backend.

Rows equal on every factor come out in no fixed order (std::sort in the reference; the row index as last key
on the device), so a window is compared with same_window: the sequence of factor tuples is the host window's
(that is determined), a tuple whose rows all lie inside the window brings exactly those rows, a tuple cut by
a window edge brings the right number of that tuple's rows. All values compare exactly (the double column is
computed alike on both sides: one multiplication and one subtraction of exactly representable values).
Every device case asserts that the counter flag order_by_device rose by one, so a silent fall-back to the
host fails."""
import collections
import ctypes

import pytest

from nebula_amd import datagen, engine, kvfmt, ngql, orderby, pipeline
from oracle import oracle
from tests import fixtures
from tests.golden.orderby_cases import CASES
from tests.test_orderby_host import check_golden, golden_query

pytestmark = pytest.mark.gpu
EDGES = ["serve", "like", "teammate"]

COLS = ("e._dst AS d, e.p0 AS a, e.p1 AS b, (double)(0 - e.p0 * 0.5) AS x, $$.vt.name AS s, (int)(e.p0 % 7) AS k, "
        "e._rank AS r")                                           # the casts give the columns a static type
NAMES = ["d", "a", "b", "x", "s", "k", "r"]
GO = "GO 2 STEPS FROM {S} OVER e YIELD " + COLS


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


# values that differ only in their top byte, only in their bottom byte, and in their sign, all within 4 bytes
WIDE_VALS = [-1200000, -0x1000000 + 5, -0x2000000 + 5, -2, -1, 0, 1, 2, 255, 256, 0x1000000 + 5, 0x1000000 + 6,
             0x2000000 + 5, 1200000]


def wide_dataset():
    """650 out-edges `w`(val INT, cnt INT) of 5 vertices, as test_gpu_groupby.wide_dataset: vids past 2^15 and
    val of WIDE_VALS, so compact results hold w._dst and val at 4 bytes; cnt at 1."""
    nparts, etype = 3, 11
    b = kvfmt.KVBatch()
    for i in range(5):
        for j in range(130):
            src, dst = 70001 + i, 100000 + 7 * j
            val = WIDE_VALS[(i * 131 + j * 977) % len(WIDE_VALS)]
            b.put(kvfmt.edge_key(src % nparts + 1, src, etype, 0, dst), kvfmt.encode_row([kvfmt.INT, kvfmt.INT], [val, j % 5]))
    schemas = [fixtures.SchemaDef(True, etype, "w", [("val", kvfmt.INT), ("cnt", kvfmt.INT)])]
    return fixtures.Dataset(space=1, num_parts=nparts, schemas=schemas, batch=b)


PREFIX = "twenty-bytes-of-text"                                   # 20 bytes: the difference lies in the third word


def string_names():
    """300 names behind a common 20-byte prefix, of lengths 20 .. 43: the bare prefix (a proper prefix of every
    other), pairs equal through byte 16 and beyond (they differ past the second word), repeats."""
    assert len(PREFIX) == 20
    tails = ["", "a", "b", "ab", "abcd", "abcdefgh", "abcdefghi", "abcdefghijklmnopqrstuvw", "abce", "\xe9", "B", "aB"]
    return [PREFIX + tails[(7 * i + i // 12) % len(tails)] + ("" if i % 5 else str(i % 3)) for i in range(300)]


def string_dataset():
    """300 out-edges `t`(n INT) of 3 vertices to 300 vertices tagged `nm`(name STRING, big STRING): name of
    string_names(); big is short but for one vertex's 300 bytes (past the factor length cap)."""
    nparts, etype, tag = 2, 7, 3
    b = kvfmt.KVBatch()
    for i, name in enumerate(string_names()):
        dst = 5000 + i
        b.put(kvfmt.vertex_key(dst % nparts + 1, dst, tag), kvfmt.encode_row([kvfmt.STRING, kvfmt.STRING],
                                                                              [name, "q" * 300 if i == 17 else "q%d" % (i % 4)]))
        src = 9001 + i % 3
        b.put(kvfmt.edge_key(src % nparts + 1, src, etype, 0, dst), kvfmt.encode_row([kvfmt.INT], [(i * 37) % 11 - 5]))
    schemas = [fixtures.SchemaDef(False, tag, "nm", [("name", kvfmt.STRING), ("big", kvfmt.STRING)]),
               fixtures.SchemaDef(True, etype, "t", [("n", kvfmt.INT)])]
    return fixtures.Dataset(space=1, num_parts=nparts, schemas=schemas, batch=b)


def _small(build):
    ds = build()
    o = oracle.Oracle()
    ds.load_oracle(o)
    e = engine.Engine(0)
    ds.load_engine(e)
    return ds, o, e


@pytest.fixture(scope="module")
def wide():
    ds, o, e = _small(wide_dataset)
    yield ds, o, e
    e.close()
    o.close()


@pytest.fixture(scope="module")
def strings():
    ds, o, e = _small(string_dataset)
    yield ds, o, e
    e.close()
    o.close()


_HOST = {}


def host(o, ds, go_text):
    """The GO's rows from the oracle, computed once per text and left unchanged."""
    key = (id(o), go_text)
    if key not in _HOST:
        out = pipeline.run(o, ds.space, go_text)
        assert out.ok, out.error
        _HOST[key] = out
    return _HOST[key]


def device(e, ds, text, **kw):
    before = e.get_flag("order_by_device")
    out = pipeline.run(e, ds.space, text, order_limit=True, **kw)
    assert out.ok, out.error
    return out, e.get_flag("order_by_device") - before


def tail(factors, names, offset, count):
    ob = "ORDER BY " + ", ".join("$-.%s%s" % (names[i], " DESC" if desc else "") for i, desc in factors) + " | " if factors else ""
    return " | " + ob + ("LIMIT %d, %d" % (offset, count) if offset else "LIMIT %d" % count)


_ORDERED = {}


def same_window(got_rows, all_rows, factors, offset, count):
    """got_rows is a valid window [offset, offset + count) of all_rows ordered by factors ((column, desc)
    pairs; none: LIMIT alone, any rows of the input in the right number)."""
    allc = collections.Counter(all_rows)
    gotc = collections.Counter(got_rows)
    if not factors:
        assert len(got_rows) == max(0, min(len(all_rows), offset + count) - offset)
        assert not gotc - allc
        return
    if not all_rows:
        assert got_rows == []
        return
    key = (id(all_rows), tuple(factors))                          # all_rows is one of host()'s lists: kept, unchanged
    if key not in _ORDERED:
        names = ["c%d" % i for i in range(len(all_rows[0]))]
        s = ngql.OrderBySentence([(names[i], desc) for i, desc in factors])
        _ORDERED[key] = orderby.order_by(s, names, [0] * len(names), all_rows)[2]
    window = _ORDERED[key][offset:offset + count]

    def tup(r):
        return tuple(orderby._key(r[i]) for i, _ in factors)
    assert [tup(r) for r in got_rows] == [tup(r) for r in window]          # 2: determined by the order
    in_all, in_win, by_tup = collections.Counter(map(tup, all_rows)), collections.Counter(map(tup, window)), {}
    for r in all_rows:
        by_tup.setdefault(tup(r), collections.Counter())[r] += 1
    got_by = {}
    for r in got_rows:
        got_by.setdefault(tup(r), collections.Counter())[r] += 1
    for t, n in in_win.items():
        if n == in_all[t]:
            assert got_by[t] == by_tup[t], t                                # 3: the whole tie lies inside
        else:
            assert sum(got_by[t].values()) == n and not got_by[t] - by_tup[t], t   # 4: cut by a window edge


def check(o, e, ds, go_text, factors, offset, count, names=NAMES, calls=1, **kw):
    want = host(o, ds, go_text)
    got, rose = device(e, ds, go_text + tail(factors, names, offset, count), **kw)
    assert rose == calls
    assert got.names == want.names
    # the interim schema: an UNKNOWN column takes its first row's type; no rows, no schema
    assert list(got.col_types) == (pipeline.Interim.from_result(want.names, want.col_types, want.rows).types if got.rows else [])
    same_window(got.rows, want.rows, factors, offset, count)
    return got, want


D, A, B, X, S, K, R = range(7)
PLANS = {
    "d": [(D, False)], "d_desc": [(D, True)], "a": [(A, False)], "b_desc": [(B, True)], "x": [(X, False)],
    "x_desc": [(X, True)], "k": [(K, False)], "k_desc": [(K, True)], "r": [(R, False)], "s": [(S, False)],
    "s_desc": [(S, True)],
    "a_d": [(A, False), (D, True)], "k_b": [(K, True), (B, False)], "s_a": [(S, False), (A, True)], "r_k": [(R, False), (K, False)],
    "k_a_x_d": [(K, False), (A, True), (X, False), (D, False)], "r_s_b_d": [(R, True), (S, True), (B, False), (D, True)],
}


@pytest.mark.parametrize("plan", list(PLANS))
def test_factor_types_and_directions(rmat, plan):
    ds, o, e, seeds = rmat
    go = GO.replace("{S}", seeds)
    n = len(host(o, ds, go).rows)
    assert n > 2000
    check(o, e, ds, go, PLANS[plan], 0, 100)
    check(o, e, ds, go, PLANS[plan], 37, 300)                     # offset > 0; `k` (7 values) is cut in mid-tie


def test_the_low_cardinality_factor_is_cut_in_mid_tie(rmat):
    ds, o, e, seeds = rmat
    rows = host(o, ds, GO.replace("{S}", seeds)).rows
    ks = sorted(r[K][1] for r in rows)
    assert len(set(ks)) == 7 and ks[99] == ks[100] and ks[36] == ks[37]
    assert len({r[R] for r in rows}) == 1                         # e._rank: one value, a width-0 column when compact


def test_window_shapes(rmat):
    ds, o, e, seeds = rmat
    go = GO.replace("{S}", seeds)
    n = len(host(o, ds, go).rows)
    assert n % 256 and n > 256                                    # off the block size
    kmax = e.get_flag("order_k_max")
    e.set_flag("order_k_max", max(kmax, n + 10))
    try:
        for factors in (PLANS["b_desc"], PLANS["k_a_x_d"], []):
            for offset, count in ((0, 1), (0, n), (0, n + 5), (n - 3, 10), (n - 1, 1), (n, 4), (n + 7, 4), (5, 0), (0, n - 1)):
                got, _ = check(o, e, ds, go, factors, offset, count)
                assert len(got.rows) == max(0, min(n, offset + count) - offset) if count else got.rows == []
    finally:
        e.set_flag("order_k_max", kmax)


def test_zero_rows(rmat):
    ds, o, e, seeds = rmat
    go = "GO FROM %s OVER e WHERE e.p0 < 0 YIELD e._dst AS d, e.p0 AS a" % seeds
    for factors in ([(1, True)], []):
        got, want = check(o, e, ds, go, factors, 0, 10, names=["d", "a"])
        assert got.rows == [] and got.names == ["d", "a"] and list(got.col_types) == []


WIDE_GO = "GO FROM 70001, 70002, 70003, 70004, 70005 OVER w YIELD w._dst AS d, w.val AS v, w.cnt AS c"


@pytest.mark.parametrize("compact", [True, False], ids=["compact", "wide8"])
@pytest.mark.parametrize("factors", [[(1, False)], [(1, True)], [(2, True), (1, False)], [(1, True), (0, True)]],
                         ids=["v", "v_desc", "c_desc_v", "v_desc_d_desc"])
def test_stored_widths(wide, factors, compact):
    """val at 4 bytes, cnt at 1 (compact) or both at 8: signs, and values apart only in one byte."""
    ds, o, e = wide
    rows = host(o, ds, WIDE_GO).rows
    assert len(rows) == 650 and {r[1][1] for r in rows} == set(WIDE_VALS)
    for offset, count in ((0, 60), (200, 200)):
        s, spec = pipeline.Pipeline(e, ds.space, order_limit=True)._order_spec(
            WIDE_GO, "ORDER BY " + ", ".join("$-.%s%s" % ("dvc"[i], " DESC" if d else "") for i, d in factors),
            "LIMIT %d, %d" % (offset, count))
        before = e.get_flag("order_by_device")
        r = e.go(ds.space, s, order_by=spec, yield_only=True, compact=compact)
        assert r.ok and r.go_nrows == 650 and e.get_flag("order_by_device") == before + 1
        assert list(r.dev_widths[1]) == ([4, 4, 1] if compact else [8, 8, 8])
        same_window(r.rows, rows, factors, offset, count)


@pytest.mark.parametrize("compact,yield_only", [(True, True), (False, True), (False, False)])
def test_compact_on_and_off_cover_every_width(rmat, compact, yield_only):
    ds, o, e, seeds = rmat
    go = GO.replace("{S}", seeds)
    rows = host(o, ds, go).rows
    widths = set()
    for name in ("a_d", "r_k", "k_a_x_d"):
        s, spec = pipeline.Pipeline(e, ds.space, order_limit=True)._order_spec(
            go, tail(PLANS[name], NAMES, 0, 1).split(" | ")[1], "LIMIT 11, 500")
        r = e.go(ds.space, s, order_by=spec, yield_only=yield_only, compact=compact)
        assert r.ok and r.go_nrows == len(rows)
        widths |= set(r.dev_widths[1])
        same_window(r.rows, rows, PLANS[name], 11, 500)
    assert widths >= ({0, 1, 2, 8} if compact else {8})


STR_GO = "GO FROM 9001, 9002, 9003 OVER t YIELD $$.nm.name AS s, t.n AS n, t._dst AS d, $$.nm.big AS big"


@pytest.mark.parametrize("factors", [[(0, False)], [(0, True)], [(0, False), (1, True)], [(0, True), (1, False)],
                                     [(1, False), (0, False)]], ids=["s", "s_desc", "s_n_desc", "s_desc_n", "n_s"])
def test_multi_word_strings(strings, factors):
    ds, o, e = strings
    rows = host(o, ds, STR_GO).rows
    names = {r[0][1] for r in rows}
    assert len(rows) == 300 and PREFIX in names and PREFIX + "abcd" in names and PREFIX + "abce" in names
    assert max(len(s.encode()) for s in names) > 40 and len(names) < 300   # three words and a length; repeats
    for offset, count in ((0, 25), (90, 120), (0, 300)):
        check(o, e, ds, STR_GO, factors, offset, count, names=["s", "n", "d", "big"])


@pytest.mark.parametrize("go", [
    "GO 1 TO 2 STEPS FROM {S} OVER e YIELD " + COLS,
    "GO 2 STEPS FROM {S} OVER e REVERSELY YIELD " + COLS,
    "GO 1 TO 2 STEPS FROM {S} OVER e BIDIRECT WHERE e.p0 > 60 YIELD " + COLS,
], ids=["m_to_n", "reversely", "m_to_n_bidirect"])
def test_appended_results(rmat, go):
    ds, o, e, seeds = rmat
    go = go.replace("{S}", seeds)
    assert len(host(o, ds, go).rows) > 500
    for name in ("b_desc", "s_a", "k_a_x_d"):
        check(o, e, ds, go, PLANS[name], 3, 200)
    check(o, e, ds, go, [], 3, 200)


@pytest.mark.parametrize("case", CASES, ids=[f"{c['source']}{c['line']}" for c in CASES])
def test_known_answers_through_engine(nba, case):
    ds, o, e = nba
    before = e.get_flag("order_by_device")
    out = pipeline.run(e, ds.space, golden_query(case), EDGES, order_limit=True)
    assert e.get_flag("order_by_device") - before == (1 if case.get("device") else 0)
    check_golden(case, out)


def _spec_go(e, ds, go, spec, **kw):
    return e.go(ds.space, go, order_by=spec, yield_only=True, compact=True, **kw)


UNCAST_GO = "GO 2 STEPS FROM {S} OVER e YIELD e.p0 % 7 AS u, e.p1 AS b"   # u: a per-row (UNKNOWN) type


@pytest.mark.parametrize("go,spec,reason", [
    (GO, engine.OrderBySpec([(0, False)], 0, -1), "no LIMIT"),
    (GO, engine.OrderBySpec([(0, False)], 65536, 1), "order_k_max"),
    (GO, engine.OrderBySpec([(i % 7, False) for i in range(9)], 0, 10), "more than 8 factors"),
    (UNCAST_GO, engine.OrderBySpec([(0, False)], 0, 10), "UNKNOWN-typed factor"),
], ids=["no_limit", "k_max", "nine_factors", "unknown_factor"])
def test_the_library_refuses_with_a_reason(rmat, go, spec, reason):
    ds, o, e, seeds = rmat
    before = e.get_flag("order_by_device")
    r = _spec_go(e, ds, go.replace("{S}", seeds), spec)
    assert not r.ok and r.code == engine.E_UNSUPPORTED and reason in r.error
    assert e.get_flag("order_by_device") == before
    plain = "GO FROM %s OVER e YIELD e._dst AS d" % seeds        # the context answers the next query
    assert sorted(e.go(ds.space, plain).rows) == sorted(host(o, ds, plain).rows)


def test_a_long_factor_string_is_refused_and_answered_by_the_host(strings):
    ds, o, e = strings
    r = _spec_go(e, ds, STR_GO, engine.OrderBySpec([(3, False)], 0, 10))
    assert not r.ok and r.code == engine.E_UNSUPPORTED and "longer than 256 bytes" in r.error
    check(o, e, ds, STR_GO, [(3, True), (2, False)], 0, 10, names=["s", "n", "d", "big"], calls=0)
    check(o, e, ds, STR_GO, [(0, False)], 0, 10, names=["s", "n", "d", "big"])    # the long string crosses as a cell


def test_order_k_max_is_the_bound(rmat):
    ds, o, e, seeds = rmat
    go = GO.replace("{S}", seeds)
    kmax = e.get_flag("order_k_max")
    assert kmax == 65536
    e.set_flag("order_k_max", 64)
    try:
        check(o, e, ds, go, PLANS["b_desc"], 4, 60)               # K = 64: on the device
        check(o, e, ds, go, PLANS["b_desc"], 4, 61, calls=0)      # K = 65: refused, the host answers
        check(o, e, ds, go, [], 0, 65, calls=0)
    finally:
        e.set_flag("order_k_max", kmax)


def test_host_answers_what_the_device_path_does_not_take(rmat):
    ds, o, e, seeds = rmat
    go = GO.replace("{S}", seeds)
    check(o, e, ds, go, PLANS["k_b"], 0, 50, calls=0, device_order_by=False)
    uncast = UNCAST_GO.replace("{S}", seeds)                      # Pipeline sends it, the library refuses, the host orders
    assert pipeline.Pipeline(e, ds.space, order_limit=True)._order_spec(uncast, "ORDER BY $-.u", "LIMIT 20") is not None
    check(o, e, ds, uncast, [(0, True), (1, False)], 0, 20, names=["u", "b"], calls=0)
    check(o, e, ds, uncast, [(1, True)], 0, 20, names=["u", "b"])            # an UNKNOWN column that is no factor crosses
    before = e.get_flag("order_by_device")                       # ORDER BY without LIMIT: straight to the host
    out = pipeline.run(e, ds.space, go + " | ORDER BY $-.b DESC, $-.d, $-.a", order_limit=True)
    assert out.ok and e.get_flag("order_by_device") == before
    same_window(out.rows, host(o, ds, go).rows, [(B, True), (D, False), (A, False)], 0, len(out.rows))
    assert len(out.rows) == len(host(o, ds, go).rows)
    with pytest.raises(pipeline.PipelineError, match="only GO sentences run in this path"):
        pipeline.run(e, ds.space, go + " | LIMIT 3")              # the default stays off


def test_world_2_is_refused():
    """A shard of a two-shard world: the shards' winners would have to merge (a later step)."""
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
                 order_by=engine.OrderBySpec([(1, False)], 0, 10))
        assert not r.ok and r.code == engine.E_UNSUPPORTED and "world > 1" in r.error and r.go_nrows > 0
        assert e.get_flag("order_by_device") == 0
    finally:
        e.close()


def test_lifetime(rmat):
    """A result is freed before the next call; different plans in a row, then a plain GO on the same context."""
    ds, o, e, seeds = rmat
    go = GO.replace("{S}", seeds)
    for name in ("s_a", "b_desc", "s_a", "k_a_x_d"):
        check(o, e, ds, go, PLANS[name], 2, 150)
    plain = e.go(ds.space, go)
    assert sorted(plain.rows, key=repr) == sorted(host(o, ds, go).rows, key=repr)
    check(o, e, ds, go, PLANS["x_desc"], 0, 9)


def test_poisoned_scratch_gives_the_same_window(rmat):
    """Fresh scratch filled with a poison byte (flag poison_buffers): nothing is read before it is written."""
    ds, o, _, seeds = rmat
    go = GO.replace("{S}", seeds)
    e = engine.Engine(0)
    try:
        e.set_flag("poison_buffers", 1)
        ds.load_engine(e)
        for name in ("k_a_x_d", "s_desc", "b_desc"):
            check(o, e, ds, go, PLANS[name], 5, 400)
        check(o, e, ds, go, [], 5, 400)
    finally:
        e.set_flag("poison_buffers", 0)
        e.close()
