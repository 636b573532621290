"""LOOKUP through the Engine: the reference's LookupTest answers (tests/golden/lookup_cases.py) and a set of
sentences over the NBA fixture run through pipeline.run(..., lookup=True); rows (sorted: the device answers in
storage order, the reference in index key order per part) and names equal lookup.scan_model over the same rows. Then
the default refusal, and every "lookup: ..." refusal a small load can produce."""
import json
import os

import pytest

from nebula_amd import engine, kvfmt, lookup, ngql, pipeline
from tests import fixtures
from tests.golden import lookup_cases as G
from tests.test_lookup_host import check_case, indexes, model

pytestmark = pytest.mark.gpu

INT, STRING = 2, 6


def golden_dataset():
    b = kvfmt.KVBatch()
    ids = {n: (i, [t for _, t in f]) for _, i, n, f in G.SCHEMAS}

    def part(v):
        return v % G.PARTS + 1
    for tag, rows in G.VERTICES.items():
        for vid, vals in rows:
            b.put(kvfmt.vertex_key(part(vid), vid, ids[tag][0]), kvfmt.encode_row(ids[tag][1], vals))
    for edge, rows in G.EDGES.items():
        for src, dst, rank, vals in rows:                         # out under +type, in under -type, as InsertEdgeExecutor
            row = kvfmt.encode_row(ids[edge][1], vals)
            b.put(kvfmt.edge_key(part(src), src, ids[edge][0], rank, dst), row)
            b.put(kvfmt.edge_key(part(dst), dst, -ids[edge][0], rank, src), row)
    schemas = [fixtures.SchemaDef(e, i, n, f) for e, i, n, f in G.SCHEMAS]
    return fixtures.Dataset(space=1, num_parts=G.PARTS, schemas=schemas, batch=b)


@pytest.fixture(scope="module")
def golden():
    ds = golden_dataset()
    with engine.Engine() as e:
        ds.load_engine(e)
        yield ds, e


@pytest.mark.parametrize("case", G.CASES, ids=[c[0] for c in G.CASES])
def test_golden(golden, case):
    ds, e = golden
    before = e.get_flag("lookup_device")
    out = pipeline.run(e, ds.space, case[1], lookup=True, indexes=indexes())
    check_case(case, out)
    if isinstance(case[2], list):
        rows, names, _ = model(case[1])
        assert sorted(tuple(v for _, v in r) for r in out.rows) == sorted(rows) and out.names == names
        assert e.get_flag("lookup_device") - before == 1
    else:
        assert e.get_flag("lookup_device") == before


# ----------------------------------------------------------------------------- NBA
NBA_INDEXES = [lookup.Index(1, "player_age", "player", False, [("age", INT)]),
               lookup.Index(2, "player_name", "player", False, [("name", STRING)]),
               lookup.Index(3, "serve_years", "serve", True, [("start_year", INT), ("end_year", INT)])]
EDGE_NAMES = ["serve", "like", "teammate"]
NBA_QUERIES = [
    "LOOKUP ON player WHERE player.age > 40",
    "LOOKUP ON player WHERE player.age >= 30 && player.age < 34 YIELD player.name, player.age",
    "LOOKUP ON player WHERE player.age != 33 YIELD player.age",
    "LOOKUP ON player WHERE player.age < 0",
    'LOOKUP ON player WHERE player.name == "Tim Duncan" YIELD player.age',
    'LOOKUP ON player WHERE player.name == "Nobody"',
    "LOOKUP ON serve WHERE serve.start_year > 2010 YIELD serve.start_year, serve.end_year",
    "LOOKUP ON serve WHERE serve.start_year == 2003 && serve.end_year <= 2010 YIELD serve.end_year AS e",
    "LOOKUP ON serve WHERE serve.start_year >= 1990 && serve.end_year != 2016",
]


@pytest.fixture(scope="module")
def nba():
    ds = fixtures.nba()
    d = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "nba.json")))
    vid = ngql.nebula_hash
    tables = {"player": [(vid(n), {"name": n, "age": a}) for n, a in d["players"]],
              # an edge inserted twice under one (src, dst, rank) is one row: the later insert's
              "serve": list({(vid(p), vid(t), r): (vid(p), vid(t), r, {"start_year": s, "end_year": e})
                             for p, t, r, s, e in d["serve"]}.values())}
    with engine.Engine() as e:
        ds.load_engine(e)
        yield ds, e, tables


@pytest.mark.parametrize("q", NBA_QUERIES)
def test_nba_equals_the_model(nba, q):
    ds, e, tables = nba
    s = ngql.parse_lookup(q)
    plan = lookup.plan_of(e.catalog(ds.space), NBA_INDEXES, s)
    want = lookup.scan_model(tables[s.from_], plan, ds.num_parts)
    out = pipeline.run(e, ds.space, q, EDGE_NAMES, lookup=True, indexes=NBA_INDEXES)
    assert out.ok, out.error
    assert out.names == plan.names
    assert sorted(tuple(v for _, v in r) for r in out.rows) == sorted(want)
    if want:
        assert out.col_types == plan.types
    if "age > 40" in q or "start_year > 2010" in q:
        assert want                                               # the sentences are not all empty


def test_nba_pipes(nba):
    ds, e, tables = nba
    kw = dict(lookup=True, indexes=NBA_INDEXES, order_limit=True, fetch=True)
    look = "LOOKUP ON player WHERE player.age > 40 YIELD player.age AS age"
    old = sorted(v for v, p in tables["player"] if p["age"] > 40)
    assert old
    go = "GO FROM %s OVER serve YIELD serve._dst AS t, serve.start_year AS y" % ", ".join(map(str, old))
    want = pipeline.run(e, ds.space, go, EDGE_NAMES)
    got = pipeline.run(e, ds.space, look + " | GO FROM $-.VertexID OVER serve YIELD serve._dst AS t, serve.start_year AS y",
                       EDGE_NAMES, **kw)
    assert got.ok and want.ok and want.rows
    assert fixtures.normalize_cells(got.rows) == fixtures.normalize_cells(want.rows)
    got = pipeline.run(e, ds.space, "$v = " + look + "; GO FROM $v.VertexID OVER serve YIELD serve._dst AS t, "
                       "serve.start_year AS y", EDGE_NAMES, **kw)
    assert got.ok and fixtures.normalize_cells(got.rows) == fixtures.normalize_cells(want.rows)
    got = pipeline.run(e, ds.space, look + " | FETCH PROP ON player $-.VertexID YIELD player.name, player.age", EDGE_NAMES, **kw)
    assert got.ok, got.error
    assert sorted((r[0][1], r[2][1]) for r in got.rows) == sorted((v, p["age"]) for v, p in tables["player"] if p["age"] > 40)
    got = pipeline.run(e, ds.space, look + " | ORDER BY $-.age DESC | LIMIT 2", EDGE_NAMES, **kw)
    assert got.ok, got.error
    assert [r[1][1] for r in got.rows] == sorted((p["age"] for _, p in tables["player"] if p["age"] > 40), reverse=True)[:2]
    got = pipeline.run(e, ds.space, "GO FROM %d OVER serve YIELD serve._dst AS id | %s" % (old[0], look), EDGE_NAMES, **kw)
    alone = pipeline.run(e, ds.space, look, EDGE_NAMES, **kw)
    assert got.ok and got.rows == alone.rows and len(alone.rows) == len(old)


# ----------------------------------------------------------------------------- refusals
def test_default_refusal(nba):
    ds, e, _ = nba
    with pytest.raises(pipeline.PipelineError) as err:
        pipeline.run(e, ds.space, "LOOKUP ON player WHERE player.age > 40", EDGE_NAMES)
    assert str(err.value) == "only GO sentences run in this path: LOOKUP ON player WHERE player.age > 40"


def spec_of(cat, idx, q):
    return lookup.device_spec(lookup.plan_of(cat, idx, ngql.parse_lookup(q)))


def test_refusals():
    fields = [("a", INT), ("s", STRING)]
    many = [("f%d" % i, INT) for i in range(17)]
    with engine.Engine() as e:
        e.add_space(1, 1)
        e.add_schema(1, False, 2, "ttl", fields, ttl_col="a", ttl_dur=100)
        e.add_schema(1, True, 3, "ettl", fields, ttl_col="a", ttl_dur=100)
        e.add_schema(1, False, 4, "ver", [("a", INT)], ver=0)
        e.add_schema(1, False, 4, "ver", fields, ver=1)
        e.add_schema(1, False, 5, "wide", many)
        e.add_schema(1, True, 6, "bad", [("a", INT)])
        e.add_schema(1, False, 7, "ok", fields)
        b = kvfmt.KVBatch()
        b.put(kvfmt.vertex_key(1, 1, 2), kvfmt.encode_row([INT, STRING], [1, "x"]))
        b.put(kvfmt.vertex_key(1, 1, 4), kvfmt.encode_row([INT], [1], ver=0))          # the old version lacks `s`
        b.put(kvfmt.vertex_key(1, 2, 4), kvfmt.encode_row([INT, STRING], [2, "y"], ver=1))
        b.put(kvfmt.vertex_key(1, 1, 5), kvfmt.encode_row([INT] * 17, list(range(17))))
        b.put(kvfmt.vertex_key(1, 1, 7), kvfmt.encode_row([INT, STRING], [1, "x"]))
        b.put(kvfmt.vertex_key(1, 2, 7), kvfmt.encode_row([INT, STRING], [2, "y"]))
        b.put(kvfmt.edge_key(1, 1, 3, 0, 2), kvfmt.encode_row([INT, STRING], [1, "x"]))
        b.put(kvfmt.edge_key(1, 1, 6, 0, 2), b"")                                       # an empty value: EF_EMPTY_VALUE
        b.put(kvfmt.edge_key(1, 1, 6, 1, 2), kvfmt.encode_row([INT], [1]))
        e.load_batch(1, b)
        e.commit(1)
        cat = e.catalog(1)
        idx = [lookup.Index(1, "i1", "ttl", False, [("a", INT)]), lookup.Index(2, "i2", "ettl", True, [("a", INT)]),
               lookup.Index(3, "i3", "ver", False, fields), lookup.Index(4, "i4", "wide", False, many),
               lookup.Index(5, "i5", "bad", True, [("a", INT)]), lookup.Index(6, "i6", "ok", False, [("a", INT)]),
               lookup.Index(7, "i7", "ver", False, [("a", INT)])]

        def refused(q, text):
            before = e.get_flag("lookup_device")
            out = pipeline.run(e, 1, q, lookup=True, indexes=idx)
            assert not out.ok and out.error.startswith(text), out.error
            assert e.get_flag("lookup_device") == before
        refused("LOOKUP ON ttl WHERE ttl.a == 1", "lookup: a TTL tag schema")
        refused("LOOKUP ON ettl WHERE ettl.a == 1", "lookup: a TTL edge schema")
        refused("LOOKUP ON bad WHERE bad.a == 1", "lookup: edges with empty or unreadable values")
        refused('LOOKUP ON ver WHERE ver.a == 1 && ver.s == "y"', "lookup: field `s' is missing from some row's schema version")
        refused("LOOKUP ON ver WHERE ver.a == 1 YIELD ver.s", "lookup: field `s' is missing from some row's schema version")
        refused("LOOKUP ON wide WHERE " + " && ".join("wide.f%d == %d" % (i, i) for i in range(17)),
                "lookup: more than 16 scanned fields")
        refused("LOOKUP ON wide WHERE wide.f0 != 1 && " + " && ".join("wide.f%d == %d" % (i, i) for i in range(16)),
                "lookup: more than 16 residual terms")
        refused("LOOKUP ON wide WHERE wide.f0 == 0 YIELD " + ", ".join("wide.f%d" % i for i in range(16)),
                "lookup: more than 16 columns")
        ok = pipeline.run(e, 1, "LOOKUP ON ver WHERE ver.a >= 1", lookup=True, indexes=idx)      # `a` is in every version
        assert ok.ok and sorted(r[0][1] for r in ok.rows) == [1, 2]
        ok = pipeline.run(e, 1, "LOOKUP ON wide WHERE wide.f0 == 0 YIELD " + ", ".join("wide.f%d" % i for i in range(15)),
                          lookup=True, indexes=idx)
        assert ok.ok and [v for _, v in ok.rows[0]] == [1] + list(range(15))
        # lookup_rows_max: at the limit served, one row above it refused
        e.set_flag("lookup_rows_max", 2)
        ok = pipeline.run(e, 1, "LOOKUP ON ok WHERE ok.a >= 1", lookup=True, indexes=idx)
        assert ok.ok and len(ok.rows) == 2
        e.set_flag("lookup_rows_max", 1)
        refused("LOOKUP ON ok WHERE ok.a >= 1", "lookup: 2 rows, above lookup_rows_max")
        ok = pipeline.run(e, 1, "LOOKUP ON ok WHERE ok.a >= 2", lookup=True, indexes=idx)
        assert ok.ok and len(ok.rows) == 1
