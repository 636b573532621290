"""Closing an Engine gives back every device scratch buffer it grew: the process-wide gauge dbuf_live_bytes (bytes
held by the engine's growable device buffers, engine_ctx.h DBuf) read on a second Engine returns to where it was,
to the byte, after an Engine that ran one sentence of every kind on the NBA fixture is closed. Each sentence is
checked to have taken its device path (the call's counter rose), so the buffers of that path were allocated:
built-string arenas, the multi-root pipe walk and its input table, the group columns of GROUP BY | ORDER BY, FETCH
on a tag and on an edge, LOOKUP with a string column, a set operator (the second lane and its arenas), FIND
SHORTEST PATH, and a pipelined batch (the parked lanes). World 1: the buffers of the world > 1 exchanges are the
same kind of member and are freed by the same rule, not by this test."""
import pytest

from nebula_amd import engine, ngql, pipeline
from tests import fixtures
from tests.test_gpu_lookup import NBA_INDEXES

pytestmark = pytest.mark.gpu

EDGES = ["serve", "like", "teammate"]
FOUR = "{P:Tim Duncan}, {P:Tony Parker}, {P:Manu Ginobili}, {P:LaMarcus Aldridge}"
# (sentence, the counter that proves its device path)
SENTENCES = [
    ("GO FROM " + FOUR + " OVER like YIELD $$.player.name AS name, (string)like.likeness AS s", None),
    ("GO FROM {P:Tim Duncan} OVER like YIELD like._dst AS id, like.likeness AS w "
     "| GO FROM $-.id OVER like YIELD $-.w AS w, like._dst AS d, $$.player.name AS name", "pipe_walks"),
    ("GO FROM " + FOUR + " OVER like YIELD $$.player.name AS name | GROUP BY $-.name YIELD $-.name AS name, "
     "COUNT(*) AS c | ORDER BY $-.c DESC, $-.name | LIMIT 2", "group_order_device"),
    ("GO FROM {P:Boris Diaw} OVER like YIELD like._dst AS id | FETCH PROP ON player $-.id YIELD player.name, player.age",
     "fetch_device"),
    ("GO FROM {P:Boris Diaw} OVER serve YIELD serve._src AS s, serve._dst AS d "
     "| FETCH PROP ON serve $-.s->$-.d YIELD serve.start_year, serve.end_year", "fetch_device"),
    ("LOOKUP ON player WHERE player.age > 40 YIELD player.name, player.age", "lookup_device"),
    ("GO FROM {P:Tim Duncan} OVER like YIELD like._dst AS d, $$.player.name AS name UNION "
     "GO FROM {P:Tony Parker} OVER like YIELD like._dst AS d, $$.player.name AS name", "set_op_device"),
    ("FIND SHORTEST PATH FROM {P:Tiago Splitter} TO {P:LaMarcus Aldridge} OVER like UPTO 5 STEPS", "find_path_device"),
]


def test_close_returns_every_scratch_byte():
    ds = fixtures.nba()
    with engine.Engine() as a:
        base = a.get_flag("dbuf_live_bytes")
        with engine.Engine() as b:
            ds.load_engine(b)
            kw = dict(order_limit=True, set_ops=True, find_path=True, fetch=True, lookup=True, indexes=NBA_INDEXES)
            for text, counter in SENTENCES:
                before = b.get_flag(counter) if counter else 0
                out = pipeline.run(b, ds.space, fixtures.nba_query(text), EDGES, **kw)
                assert out.ok, (text, out.error)
                if counter:
                    assert b.get_flag(counter) > before, text
            go = ngql.parse_go(fixtures.nba_query("GO 2 STEPS FROM " + FOUR + " OVER like YIELD like._dst AS d, like.likeness AS w"))
            prep = b.prepare_go(ds.space, go, on_device=True, compact=True)
            overlaps = b.get_flag("batch_overlaps")
            assert [r[0] for r in b.go_batch([prep] * 4)] == [0] * 4
            assert b.get_flag("batch_overlaps") > overlaps             # the queries ran on rotating lanes
            held = a.get_flag("dbuf_live_bytes")
            assert held > base
        assert a.get_flag("dbuf_live_bytes") == base
