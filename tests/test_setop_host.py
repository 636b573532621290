"""UNION / INTERSECT / MINUS, host path: the SetExecutor restatement (nebula_amd/setop.py) through
pipeline.run(..., set_ops=True) on the oracle backend against the reference SetTest answers
(tests/golden/set_cases.py), the set-sentence splitter, every error text and empty-side rule, casting, the
INTERSECT multiplicity rule and MINUS over duplicates."""
import math

import pytest

from nebula_amd import ngql, pipeline, setop
from oracle import oracle
from tests import fixtures
from tests.golden.set_cases import CASES

EDGES = ["serve", "like", "teammate"]
T_INT, T_VID, T_DOUBLE, T_STRING, T_BOOL, T_TS = pipeline.T_INT, pipeline.T_VID, pipeline.T_DOUBLE, pipeline.T_STRING, pipeline.T_BOOL, 21


@pytest.fixture(scope="module")
def nba():
    ds = fixtures.nba()
    o = oracle.Oracle()
    ds.load_oracle(o)
    return ds, o


def golden_query(case):
    nobody = ngql.nebula_hash("NON EXIST VERTEX ID")              # SetTest.cpp:616-626: no player has this vid
    return fixtures.nba_query(case["query"]).replace("{NOBODY}", str(nobody))


def check_golden(case, out):
    if case.get("error") == "syntax":
        assert not out.ok and out.error.startswith("SyntaxError: "), out.error
        return
    if case.get("error") == "execution":
        assert not out.ok and not out.error.startswith("SyntaxError"), out.error
        return
    assert out.ok, out.error
    assert out.names == case["names"]
    got = sorted(fixtures.normalize_cells(out.rows), key=repr)
    if case.get("empty"):
        assert got == []
    elif "cast_rows" in case:
        assert got == sorted(case["cast_rows"], key=repr)
    elif not case.get("names_only"):
        assert got == fixtures.nba_expected(case["rows"])


@pytest.mark.parametrize("case", CASES, ids=[f"set{c['line']}" for c in CASES])
def test_known_answers(nba, case):
    ds, o = nba
    check_golden(case, pipeline.run(o, ds.space, golden_query(case), EDGES, set_ops=True))


def test_default_still_refuses(nba):
    """set_ops=False: the text goes to the GO parser as before, which stops at the operator."""
    ds, o = nba
    q = golden_query(CASES[0])
    out = pipeline.run(o, ds.space, q, EDGES)
    assert not out.ok and out.error == "SyntaxError: expected eof, got 'UNION'"
    out = pipeline.run(o, ds.space, "(" + q + ")", EDGES)
    assert not out.ok and out.error.startswith("SyntaxError: ")
    assert pipeline.run(o, ds.space, q, EDGES, set_ops=True).ok


def test_splitter():
    ops = lambda t: ngql.split_set(t)
    assert ops("GO FROM 1 OVER e") == (["GO FROM 1 OVER e"], [])
    assert ops("A union B Union All C UNION DISTINCT D intersect E MINUS F") == \
        (["A ", " B ", " C ", " D ", " E ", " F"], ["UNION", "UNION ALL", "UNION", "INTERSECT", "MINUS"])
    # quotes, parentheses, and names that only contain a keyword
    assert ops('GO FROM 1 OVER e YIELD "x UNION y" AS s MINUS (A UNION B)')[1] == ["MINUS"]
    assert ops("GO FROM 1 OVER union_e YIELD e.minus, $-.union, $var.intersect")[1] == []
    assert ops("A | B UNION C | D") == (["A | B ", " C | D"], ["UNION"])               # looser than the pipe
    assert ngql.is_set("A MINUS B") and not ngql.is_set("(A MINUS B)") and not ngql.is_set("A | B")
    for bad in ("UNION A", "A UNION", "A UNION ALL", "A MINUS INTERSECT B"):
        with pytest.raises(SyntaxError):
            ngql.split_set(bad)


class Stub:
    """A backend that answers `GO FROM <k> ...` with canned interim results, and counts its traversals."""

    def __init__(self, results):
        self.results, self.calls = results, 0

    def go(self, space, s, input=None, **kw):
        self.calls += 1
        names, types, rows, err = self.results[s.vids[0]]
        return type("R", (), dict(ok=not err, error=err, code=-1 if err else 0, col_types=types, rows=rows))()


def in_order(rows):
    """fixtures.normalize_cells without its sort: the rows' plain values in the order they came."""
    return [fixtures.normalize_cells([r])[0] for r in rows]


def ints(*vals):
    return (["c"], [T_INT], [(("int", v),) for v in vals], "")


def run_stub(results, text):
    return pipeline.Pipeline(Stub(results), 1, set_ops=True).run(text)


G = "GO FROM %d OVER e YIELD e.c AS c"


def test_left_associative_and_parentheses():
    res = {1: ints(1, 2, 3), 2: ints(2), 3: ints(2, 9)}
    # (1 MINUS 2) UNION 3 = {1, 3} u {2, 9}; 1 MINUS (2 UNION 3) = {1, 3}
    flat = run_stub(res, (G % 1) + " MINUS " + (G % 2) + " UNION " + (G % 3))
    assert fixtures.normalize_cells(flat.rows) == [(1,), (2,), (3,), (9,)]
    nested = run_stub(res, (G % 1) + " MINUS (" + (G % 2) + " UNION " + (G % 3) + ")")
    assert fixtures.normalize_cells(nested.rows) == [(1,), (3,)]
    # a parenthesised set sentence heads a pipe; its result is the pipe's interim input
    piped = run_stub(res, "(" + (G % 1) + " INTERSECT " + (G % 3) + ") | GROUP BY $-.c YIELD $-.c AS c, COUNT(*) AS n")
    assert fixtures.normalize_cells(piped.rows) == [(2, 1)]
    assert piped.names == ["c", "n"]


def test_error_texts():
    ok, bad = ints(1), (["c"], [], [], "boom")
    out = run_stub({1: bad, 2: ok}, (G % 1) + " UNION " + (G % 2))
    assert not out.ok and out.error == "left subquery has error: boom"
    out = run_stub({1: ok, 2: bad}, (G % 1) + " MINUS " + (G % 2))
    assert not out.ok and out.error == "right subquery has error: boom"
    out = run_stub({1: bad, 2: bad}, (G % 1) + " INTERSECT " + (G % 2))
    assert out.error == "left subquery has error: boom"
    out = run_stub({1: bad, 2: ok, 3: ok}, (G % 1) + " UNION " + (G % 2) + " UNION " + (G % 3))
    assert out.error == "left subquery has error: left subquery has error: boom"
    two = "GO FROM 2 OVER e YIELD e.c AS c, e.d AS d"
    out = run_stub({1: ok, 2: (["c", "d"], [T_INT, T_INT], [(("int", 1), ("int", 2))], "")}, (G % 1) + " UNION ALL " + two)
    assert not out.ok and out.error == "Field count not match."
    out = run_stub({1: ok, 2: (["c", "d"], [], [], "")}, (G % 1) + " MINUS " + two)     # before the empty-side rules
    assert not out.ok and out.error == "Field count not match."
    # fed by a pipe: refused when the pipe is prepared (PipeExecutor.cpp:101-106), nothing runs
    st = Stub({1: ok, 2: ok})
    out = pipeline.Pipeline(st, 1, set_ops=True).run((G % 1) + " | (" + (G % 2) + " UNION " + (G % 2) + ")")
    assert not out.ok and out.error == "SyntaxError: Set op not support input." and st.calls == 0
    # ... and a set sentence that heads a fed pipe gets the input itself (SetExecutor::feedResult)
    out = run_stub({1: ok, 2: ok}, (G % 1) + " | ((" + (G % 2) + " UNION " + (G % 2) + ") | " + "GO FROM $-.c OVER e YIELD e.c AS c)")
    assert not out.ok and out.error == "Set operation not support input yet."
    with pytest.raises(setop.SetError, match="Unknown operator"):
        setop.apply("XOR", ["c"], [T_INT], [], ["c"], [T_INT], [])


def test_empty_side_rules():
    some = (["l"], [T_INT], [(("int", 4),), (("int", 4),)])
    other = (["r"], [T_STRING], [(("str", "x"),), (("str", "x"),)])
    none_l, none_r = (["l"], [], []), (["r"], [], [])
    for op in ("UNION ALL", "UNION", "INTERSECT", "MINUS"):
        assert setop.apply(op, *none_l, *none_r) == (["l"], [], [])
    # UNION hands the other side through as it is: not cast, not made distinct, under the left's names
    for op in ("UNION ALL", "UNION"):
        assert setop.apply(op, *none_l, *other) == (["l"], [T_STRING], other[2])
        assert setop.apply(op, *some, *none_r) == (["l"], [T_INT], some[2])
    assert setop.apply("INTERSECT", *some, *none_r) == (["l"], [], [])
    assert setop.apply("INTERSECT", *none_l, *other) == (["l"], [], [])
    assert setop.apply("MINUS", *none_l, *other) == (["l"], [], [])
    assert setop.apply("MINUS", *some, *none_r) == (["l"], [T_INT], some[2])


def test_casting():
    left = (["a"], [T_DOUBLE], [(("double", 2.0),), (("double", 2.5),)])
    right = (["b"], [T_INT], [(("int", 2),), (("int", 3),)])
    assert setop.apply("INTERSECT", *left, *right)[2] == [(("double", 2.0),)]
    assert setop.apply("MINUS", *left, *right) == (["a"], [T_DOUBLE], [(("double", 2.5),)])
    assert setop.apply("UNION ALL", *left, *right)[2] == left[2] + [(("double", 2.0),), (("double", 3.0),)]
    # the other way round the doubles are truncated to the left's INT
    assert setop.apply("INTERSECT", *right, *left)[2] == [(("int", 2),)]
    assert setop.apply("MINUS", *right, *left)[2] == [(("int", 3),)]
    # INT and VID are different variant types: cast, then equal
    vid = (["v"], [T_VID], [(("id", 2),)])
    assert setop.apply("INTERSECT", *vid, *right)[2] == [(("id", 2),)]
    # without differing schema types nothing is cast, and the variant types decide
    assert setop.apply("INTERSECT", ["v"], [T_INT], vid[2], *right)[2] == []
    strs = (["s"], [T_STRING], [(("str", " 2 "),), (("str", "x1"),)])
    with pytest.raises(setop.SetError) as e:
        setop.apply("UNION", *right, *strs)
    assert str(e.value) == "Casting from string `x1' to int failed."
    for t, text in ((T_VID, "Casting from string x1 to vid failed."), (T_TS, "Casting from string x1 to timestamp failed."),
                    (T_DOUBLE, "Casting from string x1 to double failed.")):
        with pytest.raises(setop.SetError) as e:
            setop.cast_to(("str", "x1"), t)
        assert str(e.value) == text
    assert setop.cast_to(("str", " 2 "), T_INT) == ("int", 2) and setop.cast_to(("str", "1e2"), T_DOUBLE) == ("double", 100.0)
    with pytest.raises(setop.SetError):
        setop.cast_to(("str", "9223372036854775808"), T_INT)
    assert setop.cast_to(("str", ""), T_BOOL) == ("bool", True) and setop.cast_to(("str", "true"), T_BOOL) == ("bool", False)
    assert setop.cast_to(("double", 0.0), T_BOOL) == ("bool", False) and setop.cast_to(("bool", True), T_STRING) == ("str", "1")
    assert [setop.cast_to(("double", d), T_STRING)[1] for d in (1.0, -0.5, 1e21, 1.5e-7, 123456.789, 1e20)] == \
        ["1", "-0.5", "1E21", "1.5E-7", "123456.789", "100000000000000000000"]
    assert setop.cast_to(("int", -7), T_STRING) == ("str", "-7") and setop.cast_to(("double", -2.9), T_INT) == ("int", -2)
    with pytest.raises(setop.SetError, match="Type not supported yet"):
        setop.cast_to(("int", 1), 4)                              # FLOAT: castTo's default branch


@pytest.mark.parametrize("cl", [1, 2, 3])
@pytest.mark.parametrize("cr", [1, 2, 3])
def test_intersect_multiplicity(cl, cr):
    left = ints(*([5] * cl + [6, 7, 6]))[:3]
    right = ints(*([6] + [5] * cr + [8]))[:3]
    rows = setop.apply("INTERSECT", *left, *right)[2]
    assert in_order(rows) == [(5,)] * min(cl, cr) + [(6,)]                              # in left order


def test_minus_keeps_unmatched_duplicates():
    left = ints(1, 2, 1, 3, 2, 1)[:3]
    right = ints(2, 2, 9)[:3]
    assert in_order(setop.apply("MINUS", *left, *right)[2]) == [(1,), (1,), (3,), (1,)]


def test_equality_and_distinct_order():
    nan = float("nan")
    left = (["d"], [T_DOUBLE], [(("double", -0.0),), (("double", nan),), (("double", 1.0),)])
    right = (["d"], [T_DOUBLE], [(("double", 0.0),), (("double", nan),)])
    assert len(setop.apply("INTERSECT", *left, *right)[2]) == 1                         # the zeros; a NaN equals nothing
    minus = setop.apply("MINUS", *left, *right)[2]
    assert len(minus) == 2 and math.isnan(minus[0][0][1]) and minus[1] == (("double", 1.0),)
    uni = setop.apply("UNION", *left, *right)[2]
    assert [r[0][1] for r in uni[:2]] == [-0.0, 1.0] and len(uni) == 4 and all(math.isnan(r[0][1]) for r in uni[2:])
    strs = lambda *v: (["s"], [T_STRING], [(("str", x),) for x in v])
    uni = setop.apply("UNION", *strs("b", "a", "ab"), *strs("a", "", "b"))[2]
    assert [r[0][1] for r in uni] == ["", "a", "ab", "b"]
    assert setop.row_key((("int", 1),)) != setop.row_key((("id", 1),))                  # the variant type counts
    assert setop.row_key((("empty", True),)) == setop.row_key((("bool", True),))
