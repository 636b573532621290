"""FETCH PROP ON through the Engine: the reference FetchVerticesTest / FetchEdgesTest answers
(tests/golden/fetch_cases.py) on the NBA fixture, on the device path where the sentence is eligible (the flag
fetch_device proves it ran) and through the refusal ("fetch: ...") and the host restatement over the Engine for the
rest; and an RMAT graph (scale 10, edge factor 4, tag rows for two vertices in three) where 20 seeded
`GO 2 STEPS ... | FETCH PROP ON ...` sentences of both kinds equal the host restatement over the oracle."""
import random

import numpy as np
import pytest

from nebula_amd import datagen, engine, fetch, kvfmt, pipeline
from oracle import oracle
from tests import fixtures
from tests.golden.fetch_cases import CASES
from tests.test_fetch_host import check_golden

pytestmark = pytest.mark.gpu

EDGES = ["serve", "like", "teammate"]
# refused by the device ("fetch: ..."): a YIELD expression, ON *, DISTINCT over device-resident edge keys
REFUSED = {"v_base_expr", "e_base_expr", "v_all", "v_all_pipe", "v_all_twice", "v_no_vertex_all", "e_distinct_pipe",
           "e_distinct_dst"}
# after the refusal of `GO | FETCH ... DISTINCT` the GO is delivered and the deduplicated keys go up: one device call
REFUSED_THEN_DEVICE = {"e_distinct_pipe", "e_distinct_dst"}
# never sent: reference errors (worded by the host's prepare stage), and inputs that end before the storage leg
HOST_ONLY = {c[0] for c in CASES if c[3] in ("syntax", "error")} | {"v_no_vertex_pipe"}


@pytest.fixture(scope="module")
def nba():
    ds = fixtures.nba()
    with engine.Engine() as e:
        ds.load_engine(e)
        yield ds, e, fetch.Catalog.of(ds.num_parts, ds.schemas)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_known_answers(nba, case):
    ds, e, cat = nba
    before = e.get_flag("fetch_device")
    p = pipeline.Pipeline(e, ds.space, EDGES, fetch=True, catalog=cat, order_limit=True)
    check_golden(case, p.run(fixtures.nba_query(case[1])))
    ran = e.get_flag("fetch_device") - before
    name = case[0]
    if name in HOST_ONLY:
        assert (ran, p.fetch_fallbacks) == (0, 0)
    elif name in REFUSED:
        assert p.fetch_fallbacks == 1 and p.fetch_refusal.startswith("fetch:")
        assert ran == (1 if name in REFUSED_THEN_DEVICE else 0)
    else:
        assert (ran, p.fetch_fallbacks) == (1, 0)
    off = pipeline.run(e, ds.space, fixtures.nba_query(case[1]), EDGES, fetch=True, catalog=cat, order_limit=True,
                       device_fetch=False)
    check_golden(case, off)
    assert e.get_flag("fetch_device") - before == ran


# ----------------------------------------------------------------------------- RMAT
SCALE, EF, PARTS = 10, 4, 100
VERTEX = "FETCH PROP ON vt $-.id YIELD vt.v0, vt.name, $-.s"
VERTEX_DROP = "FETCH PROP ON vt $-.id YIELD vt.name"
EDGE = "FETCH PROP ON e $-.id->$-.s@$-.r YIELD e.p0, e.p1, e._type"    # the edge back: there for some rows only


def tag_rows(n):
    """Tag rows beside the generated edges: two vertices in three have one."""
    b = kvfmt.KVBatch()
    types = [t for _, t in datagen.RMAT_TAG_FIELDS]
    for v in range(n):
        if v % 3:
            b.put(kvfmt.vertex_key(v % PARTS + 1, v, datagen.RMAT_TAG), kvfmt.encode_row(types, [v * 7, "n%d" % v]))
    return b


def sentences():
    rng = random.Random(20)
    out = []
    for i in range(20):
        seeds = ", ".join(str(rng.randrange(1 << SCALE)) for _ in range(rng.randint(1, 4)))
        go = "GO 2 STEPS FROM %s OVER e YIELD e._dst AS id, e._src AS s, e._rank AS r" % seeds
        out.append((go, (VERTEX, VERTEX_DROP, EDGE, EDGE)[i % 4]))
    return out


@pytest.fixture(scope="module")
def rmat():
    ds = fixtures.RmatDataset(SCALE, ef=EF, num_parts=PARTS, with_tag=False)
    ds.schemas.append(fixtures.SchemaDef(False, datagen.RMAT_TAG, datagen.RMAT_TAG_NAME, datagen.RMAT_TAG_FIELDS))
    extra = tag_rows(1 << SCALE)
    o = oracle.Oracle()
    o.add_space(ds.space, ds.num_parts)
    for s in ds.schemas:
        o.add_schema(ds.space, s.is_edge, s.sid, s.name, s.fields, s.ver, s.ttl_col, s.ttl_dur)
    o.put_kv(ds.space, *ds.rows.arrays())
    o.put_batch(ds.space, extra)
    o.finalize(8)
    with engine.Engine() as e:
        e.add_space(ds.space, ds.num_parts)
        for s in ds.schemas:
            e.add_schema(ds.space, s.is_edge, s.sid, s.name, s.fields, s.ver, s.ttl_col, s.ttl_dur)
        e.load_kv(ds.space, *ds.rows.arrays())
        e.load_batch(ds.space, extra)
        e.commit(ds.space)
        yield ds, o, e, fetch.Catalog.of(ds.num_parts, ds.schemas)


def test_rmat_draws_against_the_oracle(rmat):
    ds, o, e, cat = rmat
    refs, with_rows, with_miss = [], 0, 0
    for go, ft in sentences():                                    # the draws, judged on the oracle's results alone
        ref = pipeline.run(o, ds.space, go + " | " + ft, ["e"], fetch=True, catalog=cat)
        keys = pipeline.run(o, ds.space, go, ["e"])
        assert ref.ok and keys.ok, ref.error
        refs.append(ref)
        with_rows += bool(ref.rows)
        if ft is VERTEX:                                          # every key keeps its row: a miss is a row of defaults
            with_miss += any(r[2][1] == "" for r in ref.rows)
        else:
            with_miss += len(ref.rows) < len(keys.rows)
    assert with_rows >= 15 and with_miss >= 5
    for (go, ft), ref in zip(sentences(), refs):
        before = e.get_flag("fetch_device")
        p = pipeline.Pipeline(e, ds.space, ["e"], fetch=True, catalog=cat)
        got = p.run(go + " | " + ft)
        assert got.ok, got.error
        assert (e.get_flag("fetch_device") - before, p.fetch_fallbacks) == (1, 0)
        assert got.names == ref.names
        assert fixtures.normalize_cells(got.rows) == fixtures.normalize_cells(ref.rows)
        if ref.rows:
            assert got.col_types == ref.col_types
