"""The YIELD sentence on the host: ngql.parse_yield, nebula_amd/yieldexec.py and Pipeline(yield_sentence=True) on
the oracle backend against the reference YieldTest answers (tests/golden/yield_cases.py), the Status texts, the
first-row typing rule, and tests/yieldref.py pinned to the restatement."""
import math

import numpy as np
import pytest

from nebula_amd import ngql, pipeline, yieldexec
from oracle import oracle
from tests import fixtures, yieldref
from tests.golden import yield_cases

EDGES = ["serve", "like", "teammate"]


@pytest.fixture(scope="module")
def nba():
    ds = fixtures.nba()
    o = oracle.Oracle()
    ds.load_oracle(o)
    yield ds, o
    o.close()


def interim(names, types, rows):
    kinds = {1: "bool", 2: "int", 3: "id", 5: "double", 6: "str", 21: "timestamp"}
    return pipeline.Interim(list(names), list(types), [tuple((kinds[t], v) for t, v in zip(types, r)) for r in rows])


def test_parser():
    s = ngql.parse_yield("YIELD $-.team AS t, COUNT(*), sum($-.a * 2) AS s, 1 + 1 WHERE $-.start > 2005 && $-.a != 3")
    assert [(y.fun, y.alias, y.expr.to_string()) for y in s.yields] == \
        [("", "t", "$-.team"), ("COUNT", "", "*"), ("SUM", "s", "($-.a*2)"), ("", "", "(1+1)")]
    assert s.where.to_string() == "(($-.start>2005)&&($-.a!=3))"
    assert s.column_names() == ["t", "*", "s", "(1+1)"]
    assert ngql.parse_yield("yield $var.*").yields[0].expr.kind == ngql.K_VAR_PROP
    assert ngql.parse_yield("YIELD 1").where is None
    assert ngql.is_yield("  yield 1") and not ngql.is_yield("GO FROM 1 OVER e YIELD e._dst")
    for bad in ("YIELD DISTINCT $-.a", "YIELD", "YIELD $-.a WHERE", "YIELD $-.a,", "YIELD $-.a LIMIT 3"):
        with pytest.raises(SyntaxError):
            ngql.parse_yield(bad)


@pytest.mark.parametrize("case", yield_cases.CASES, ids=[c["name"] for c in yield_cases.CASES])
def test_golden(nba, case):
    ds, o = nba
    out = pipeline.run(o, ds.space, fixtures.nba_query(case["query"]), EDGES, yield_sentence=True)
    if "error" in case:
        assert not out.ok
        assert case["error"] == "any" or out.error.startswith("SyntaxError") == (case["error"] == "syntax")
        if "text" in case:
            assert out.error == case["text"]
        return
    assert out.ok, out.error
    assert "names" not in case or out.names == case["names"]
    assert sorted(fixtures.normalize_cells(out.rows)) == sorted(fixtures.nba_expected(case["rows"]))


def test_default_arguments_still_refuse(nba):
    ds, o = nba
    q = fixtures.nba_query("GO FROM {P:Tim Duncan} OVER like YIELD like._dst AS id | YIELD COUNT(*)")
    with pytest.raises(pipeline.PipelineError, match="only GO sentences run in this path"):
        pipeline.run(o, ds.space, q, EDGES)
    assert pipeline.run(o, ds.space, q, EDGES, yield_sentence=True).rows == [(("int", 2),)]
    assert pipeline.run(o, ds.space, "YIELD 123 AS id", EDGES).rows == pipeline.run(
        o, ds.space, "YIELD 123 AS id", EDGES, yield_sentence=True).rows            # the constant form is kept


def test_status_texts():
    inp = interim(["a", "b"], [2, 2], [(1, 2)])
    run = lambda text, i=inp, v=None: yieldexec.run(ngql.parse_yield(text), i, v or {})
    for text, i, v, want in [
        ("YIELD $^.player.name", inp, None, "SyntaxError: Only support input and variable in yield sentence."),
        ("YIELD $v.a WHERE $-.b > 1", inp, {"v": inp}, "Not support both input and variable."),
        ("YIELD $v.a, $w.b", None, {"v": inp, "w": inp}, "Only one variable allowed to use."),
        ("YIELD $v.a", None, {}, "Variable `v' not defined."),
        ("YIELD $v.*", None, {}, "Variable `v' not defined."),
        ("YIELD $-.a", None, None, "Inputs nullptr."),
        ("YIELD $-.zz", inp, None, "column `zz' not exist in input."),
        ("YIELD $v.zz", None, {"v": inp}, "column `zz' not exist in variable."),
        ("YIELD $-.a", interim(["a", "a"], [2, 2], [(1, 2)]), None, "Duplicate column `a'"),
        ("YIELD $-.a, COUNT(*)", inp, None, "SyntaxError: Input columns without aggregation are not supported in YIELD "
                                           "statement without GROUP BY, near `$-.a'"),
        ("YIELD $-.a / 0", inp, None, "Division by zero"),
        ("YIELD MAX($-.a) WHERE $-.a > 5", inp, None, "Not Support: 0"),
        ("YIELD COUNT($-.t)", interim(["t"], [21], [(5,)]), None, "Wrong Type: 21"),
    ]:
        with pytest.raises(yieldexec.YieldError) as ei:
            run(text, i, v)
        assert str(ei.value) == want, text


def test_first_row_types_and_empty_forms():
    inp = interim(["a", "x", "id"], [2, 5, 3], [(1, 0.5, 7), (4, 2.0, 8), (9, 1.5, 9)])
    run = lambda text, i=inp: yieldexec.run(ngql.parse_yield(text), i, {})
    # the types are the first INPUT row's although WHERE drops it
    assert run("YIELD $-.a + $-.x AS v, $-.id, $-.a > 1 AS g WHERE $-.a > 1") == \
        (["v", "$-.id", "g"], [5, 3, 1], [(("double", 6.0), ("id", 8), ("bool", True)), (("double", 10.5), ("id", 9), ("bool", True))])
    # rows in, none kept: one aggregate row
    names, types, rows = run("YIELD COUNT(*), SUM($-.a), AVG($-.x), BIT_AND($-.a) WHERE $-.a > 100")
    assert types == [2, 2, 5, 2] and rows[0][:2] == (("int", 0), ("int", 0)) and math.isnan(rows[0][2][1]) and rows[0][3] == ("int", 0)
    assert run("YIELD $-.a WHERE $-.a > 100") == (["$-.a"], [2], [])
    # empty input: no rows at all, COUNT(*) included
    assert run("YIELD COUNT(*)", pipeline.Interim(["a"])) == (["*"], [], [])
    assert run("YIELD SUM($-.id), COUNT($-.x), 1 + 1") == (["$-.id", "$-.x", "(1+1)"], [3, 2, 2], [(("id", 24), ("int", 3), ("int", 2))])


def test_numpy_model_agrees_with_the_restatement():
    rng = np.random.default_rng(5)
    n = 300
    cols = {"a": rng.integers(-2 ** 62, 2 ** 62, n), "b": rng.integers(-50, 50, n), "x": rng.integers(-40, 40, n).astype(np.float64)}
    inp = interim(["a", "b", "x"], [2, 2, 5], list(zip(cols["a"].tolist(), cols["b"].tolist(), cols["x"].tolist())))
    mask = (cols["b"] > 0) & (cols["x"] + 1.0 >= 0.0)
    where = " WHERE $-.b > 0 && $-.x + 1.0 >= 0.0"
    _, _, rows = yieldexec.run(ngql.parse_yield("YIELD $-.a, $-.b * 2 + 1 AS e, $-.x / 4.0 AS q" + where), inp, {})
    assert [tuple(v for _, v in r) for r in rows] == yieldref.project(
        cols, mask, [lambda c: c["a"], lambda c: c["b"] * 2 + 1, lambda c: c["x"] / 4.0])
    _, _, rows = yieldexec.run(ngql.parse_yield(
        "YIELD COUNT(*), SUM($-.a), AVG($-.b), SUM($-.x), MAX($-.a), MIN($-.x), BIT_XOR($-.a), BIT_AND($-.b), BIT_OR($-.b), "
        "AVG($-.x)" + where), inp, {})
    assert tuple(v for _, v in rows[0]) == yieldref.aggregate(cols, mask, [
        ("COUNT", None), ("SUM", lambda c: c["a"]), ("AVG", lambda c: c["b"]), ("SUM", lambda c: c["x"]),
        ("MAX", lambda c: c["a"]), ("MIN", lambda c: c["x"]), ("BIT_XOR", lambda c: c["a"]), ("BIT_AND", lambda c: c["b"]),
        ("BIT_OR", lambda c: c["b"]), ("AVG", lambda c: c["x"])])
