"""Which heads Pipeline sends to the fused device call (`GO | GROUP BY | [ORDER BY |] LIMIT`,
ngx_go_group_order_by), with which plan, and where a refusal leads. No GPU: the backend is a stub that records
its go calls, refuses or answers the device forms as the test scripts it, and hands plain GOs to the oracle."""
import os
import types

import pytest

from nebula_amd import engine, pipeline
from oracle import oracle
from tests import fixtures

EDGES = ["serve", "like", "teammate"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED = -1002


@pytest.fixture(scope="module")
def nba():
    ds = fixtures.nba()
    o = oracle.Oracle()
    ds.load_oracle(o)
    yield ds, o
    o.close()


class Stub:
    """fused / grouped: what a go(group_by=, order_by=) / go(group_by=) call gets: a refusal's reason, or an
    Outcome whose rows it answers with."""
    device_group_by = device_order_by = device_group_order = True

    def __init__(self, o, fused="group by: stub", grouped="group by: stub"):
        self.o, self.fused, self.grouped, self.calls = o, fused, grouped, []

    def go(self, space, s, input=None, group_by=None, order_by=None, **kw):
        self.calls.append((group_by, order_by))
        if group_by is None and order_by is None:
            return self.o.go(space, s, input=input)
        script = self.fused if group_by is not None and order_by is not None else self.grouped if order_by is None else "order by: stub"
        if isinstance(script, str):
            return types.SimpleNamespace(ok=False, code=UNSUPPORTED, error=script, col_types=[], rows=[])
        return types.SimpleNamespace(ok=True, code=0, error="", col_types=list(script.col_types), rows=list(script.rows))

    def kinds(self):
        return ["fused" if g is not None and o is not None else "group" if g is not None else "order" if o is not None else "plain"
                for g, o in self.calls]


def q(text):
    return fixtures.nba_query(text)


LIKE = "GO FROM {P:Tim Duncan}, {P:Tony Parker}, {P:Manu Ginobili} OVER like YIELD $$.player.name AS name, like.likeness AS l"
GB = "GROUP BY $-.name YIELD $-.name AS name, COUNT(*) AS c, SUM($-.l) AS sl"
GSPEC = engine.GroupBySpec([0], [("", 0, None), ("COUNT", -1, "*"), ("SUM", 1, None)])


def run(backend, ds, text, **kw):
    return pipeline.run(backend, ds.space, text, EDGES, order_limit=True, **kw)


def same(a, b):
    assert (a.ok, a.error, a.names, list(a.col_types), a.rows) == (b.ok, b.error, b.names, list(b.col_types), b.rows)


@pytest.mark.parametrize("tail,ospec", [
    ("ORDER BY $-.c DESC, $-.name | LIMIT 1, 2", engine.OrderBySpec([(1, True), (0, False)], 1, 2)),
    ("ORDER BY $-.sl | LIMIT 5", engine.OrderBySpec([(2, False)], 0, 5)),
    ("LIMIT 3", engine.OrderBySpec([], 0, 3)),
    ("LIMIT 2 OFFSET 1", engine.OrderBySpec([], 2, 1)),
])
def test_an_eligible_head_is_one_fused_call(nba, tail, ospec):
    ds, o = nba
    text = q(LIKE + " | " + GB + " | " + tail)
    want = run(o, ds, text)
    assert want.ok and want.rows
    stub = Stub(o, fused=want)
    got = run(stub, ds, text)
    assert stub.kinds() == ["fused"] and stub.calls[0] == (GSPEC, ospec)
    same(got, want)                                               # names are the GROUP BY's, types the interim's
    p = pipeline.Pipeline(stub, ds.space, EDGES, order_limit=True)
    parts = [t.strip() for t in text.split(" | ")]
    assert p._group_order_spec(parts[0], parts[1], parts[2] if len(parts) == 4 else None, parts[-1])[2:] == (GSPEC, ospec)


def test_a_fused_answer_feeds_the_next_sentence(nba):
    ds, o = nba
    head = q("GO FROM {P:Tim Duncan}, {P:Tony Parker} OVER like YIELD like._dst AS id | GROUP BY $-.id YIELD $-.id AS id, COUNT(*) AS c "
             "| ORDER BY $-.c DESC, $-.id | LIMIT 2")
    text = head + " | GO FROM $-.id OVER serve YIELD $-.c AS c, serve._dst AS t"
    stub = Stub(o, fused=run(o, ds, head))
    got = run(stub, ds, text)
    assert stub.kinds() == ["fused", "plain"]
    same(got, run(o, ds, text))


FIVE = "GO FROM {P:Tim Duncan} OVER serve YIELD serve._dst AS a, serve.start_year AS b, serve.end_year AS c, $^.player.age AS d, $^.player.name AS e"
INELIGIBLE = {
    "factor_is_no_group_column": LIKE + " | " + GB + " | ORDER BY $-.l | LIMIT 2",
    "duplicate_group_column_names": LIKE + " | GROUP BY $-.name YIELD $-.name AS c, COUNT(*) AS c | ORDER BY $-.c | LIMIT 2",
    "distinct_go": LIKE.replace("YIELD", "YIELD DISTINCT") + " | " + GB + " | ORDER BY $-.c | LIMIT 2",
    "go_reading_its_input": "GO FROM {P:Tim Duncan} OVER like YIELD like._dst AS id | GO FROM $-.id OVER like YIELD $$.player.name AS name, "
                            "like.likeness AS l | " + GB + " | ORDER BY $-.c DESC, $-.name | LIMIT 2",
    "function_key": LIKE + " | GROUP BY $-.name, abs(5) YIELD $-.name AS name, COUNT(*) AS c | ORDER BY $-.c DESC, $-.name | LIMIT 2",
    "five_keys": FIVE + " | GROUP BY $-.a, $-.b, $-.c, $-.d, $-.e YIELD $-.a AS a, COUNT(*) AS n | ORDER BY $-.a | LIMIT 2",
    "order_by_without_limit": LIKE + " | " + GB + " | ORDER BY $-.c DESC, $-.name",
}


@pytest.mark.parametrize("name", list(INELIGIBLE))
def test_an_ineligible_head_is_not_sent_and_the_host_answers(nba, name):
    ds, o = nba
    text = q(INELIGIBLE[name])
    stub = Stub(o)
    got = run(stub, ds, text)
    assert "fused" not in stub.kinds()
    same(got, run(o, ds, text))
    parts = [t.strip() for t in text.split(" | ")]
    i = max(j for j, t in enumerate(parts) if t.upper().startswith("GO"))
    rest = parts[i + 2:]
    ob = rest[0] if rest and rest[0].upper().startswith("ORDER") else None
    lim = rest[-1] if rest and rest[-1].upper().startswith("LIMIT") else None
    assert pipeline.Pipeline(stub, ds.space, EDGES, order_limit=True)._group_order_spec(parts[i], parts[i + 1], ob, lim) is None


def test_a_group_stage_refusal_goes_straight_to_the_host(nba):
    ds, o = nba
    text = q(LIKE + " | " + GB + " | ORDER BY $-.c DESC, $-.name | LIMIT 2")
    stub = Stub(o, fused="group by: UNKNOWN-typed column (per-row value types)")
    got = run(stub, ds, text)
    assert stub.kinds() == ["fused", "plain"]                     # no try at the device GROUP BY: it would refuse again
    same(got, run(o, ds, text))


def test_an_order_stage_refusal_groups_on_the_device_and_orders_on_the_host(nba):
    ds, o = nba
    text = q(LIKE + " | " + GB + " | ORDER BY $-.c DESC, $-.name | LIMIT 2")
    grouped = run(o, ds, q(LIKE + " | " + GB))
    stub = Stub(o, fused="order by: offset + count above order_k_max", grouped=grouped)
    got = run(stub, ds, text)
    assert stub.kinds() == ["fused", "group"] and stub.calls[1] == (GSPEC, None)
    same(got, run(o, ds, text))


def test_the_switches(nba):
    ds, o = nba
    text = q(LIKE + " | " + GB + " | ORDER BY $-.c DESC, $-.name | LIMIT 2")
    want = run(o, ds, text)
    grouped = run(o, ds, q(LIKE + " | " + GB))
    for kw, kinds in (({"device_group_order": False}, ["group"]), ({"device_order_by": False}, ["group"]),
                      ({"device_group_by": False}, ["plain"])):
        stub = Stub(o, fused="group by: must not be asked", grouped=grouped)
        same(run(stub, ds, text, **kw), want)
        assert stub.kinds() == kinds
    stub = Stub(o, grouped=grouped)
    stub.device_group_order = False                               # a backend without the call
    same(run(stub, ds, text), want)
    assert stub.kinds() == ["group"]
    stub = Stub(o, grouped=grouped)
    with pytest.raises(pipeline.PipelineError, match="only GO sentences run in this path"):
        pipeline.run(stub, ds.space, text, EDGES)                 # order_limit off: nothing changes
    assert stub.kinds() == ["group"]


def test_the_header_declares_the_call():
    with open(os.path.join(ROOT, "include", "nebula_gn.h")) as f:
        header = f.read()
    assert "int32_t ngx_go_group_order_by(ngx_ctx* ctx, const ngx_go_result* r, const ngx_group_plan* group," in header
    assert "ngx_go_group_order_by" in engine.SIGNATURES
    assert engine.Engine.device_group_order is True
