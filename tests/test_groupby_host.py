"""GROUP BY in a pipe, host path: the GroupByExecutor restatement (nebula_amd/groupby.py) through
pipeline.run on the oracle backend against the reference GroupByLimitTest answers
(tests/golden/groupby_cases.py), the parser, each SyntaxError text, and the restatement against an
independent dict-of-lists computation over the oracle's rows of an RMAT GO."""
import math
import struct

import pytest

from nebula_amd import groupby, ngql, pipeline
from oracle import oracle
from tests import fixtures
from tests.golden.groupby_cases import CASES, ERROR_CASES

EDGES = ["serve", "like", "teammate"]


@pytest.fixture(scope="module")
def nba():
    ds = fixtures.nba()
    o = oracle.Oracle()
    ds.load_oracle(o)
    return ds, o


@pytest.fixture(scope="module")
def rmat_rows():
    ds = fixtures.RmatDataset(9, with_in=True, with_tag=True)
    o = oracle.Oracle()
    ds.load_oracle(o)
    q = ("GO 2 STEPS FROM 1,2,3,5,8,13 OVER e YIELD e._dst AS d, e.p0 AS a, e.p1 AS b, e.p0 * 0.5 AS x, "
         "$$.vt.name AS s, e.p0 % 5 AS k")
    out = pipeline.run(o, ds.space, q)
    assert out.ok and len(out.rows) > 500
    return ds, o, q, pipeline.Interim.from_result(out.names, out.col_types, out.rows)


@pytest.mark.parametrize("case", CASES, ids=[f"L{c['line']}" for c in CASES])
def test_known_answers(nba, case):
    ds, o = nba
    out = pipeline.run(o, ds.space, fixtures.nba_query(case["query"]), EDGES)
    assert out.ok, out.error
    if "names" in case:
        assert out.names == case["names"]
    got = fixtures.normalize_cells(out.rows)
    if case.get("empty"):
        assert got == []
        return
    assert got == fixtures.nba_expected(case["rows"])             # doubles exactly: the literals are exact


@pytest.mark.parametrize("case", ERROR_CASES, ids=[f"L{c['line']}" for c in ERROR_CASES])
def test_syntax_errors(nba, case):
    ds, o = nba
    out = pipeline.run(o, ds.space, fixtures.nba_query(case["query"]), EDGES)
    assert not out.ok
    assert out.error.startswith("SyntaxError: "), out.error


def test_parser_round_trip():
    s = ngql.parse_group_by("GROUP BY $-.a, teamName, abs(5) YIELD $-.a, count(*), COUNT_DISTINCT(*) AS cd, "
                            "Sum($-.w) as s, avg($-.w), MAX($-.start), min($-.w), STD($-.w), bit_and($-.w), "
                            "BIT_OR(2), bit_xor($-.w + 1), 1+1 AS cal")
    assert [g.to_string() for g in s.groups] == ["$-.a", "teamName", "abs(5)"]
    assert [y.fun for y in s.yields] == ["", "COUNT", "COUNT_DISTINCT", "SUM", "AVG", "MAX", "MIN", "STD", "BIT_AND",
                                         "BIT_OR", "BIT_XOR", ""]
    assert s.column_names() == ["$-.a", "COUNT(*)", "cd", "s", "AVG($-.w)", "MAX($-.start)", "MIN($-.w)",
                                "STD($-.w)", "BIT_AND($-.w)", "BIT_OR(2)", "BIT_XOR(($-.w+1))", "cal"]
    assert ngql.is_group_by("  group   by $-.a YIELD $-.a") and not ngql.is_group_by("GO FROM 1 OVER e")
    again = ngql.parse_group_by("GROUP BY " + ",".join(g.to_string() for g in s.groups) + " YIELD " +
                                ",".join(y.to_string() + (" AS " + y.alias if y.alias else "") for y in s.yields))
    assert again.column_names() == s.column_names()
    with pytest.raises(SyntaxError):
        ngql.parse_group_by("GROUP BY $-.a YIELD COUNT($-.a, $-.b)")
    with pytest.raises(SyntaxError):
        ngql.parse_group_by("GROUP BY $-.a YIELD COUNT($-.a) extra")


INTERIM = pipeline.Interim(["name", "id"], [pipeline.T_STRING, pipeline.T_VID],
                           [(("str", "a"), ("id", 1)), (("str", "b"), ("id", 2))])


@pytest.mark.parametrize("text,error", [
    ("GROUP BY $-.name", "SyntaxError: Yield cols is empty"),
    ("GROUP BY YIELD COUNT(*)", "SyntaxError: Group cols is empty"),
    ("GROUP BY $-.name YIELD SUM(*)", "SyntaxError: Syntax error: near `*'"),
    ("GROUP BY $-.name YIELD *", None),                            # no such column in the grammar
    ("GROUP BY $-.name, SUM($-.id) YIELD $-.name", "SyntaxError: Use invalid group function `SUM'"),
    ("GROUP BY $-.start_year YIELD COUNT($-.id)", "SyntaxError: Group `start_year' isn't in output fields"),
    ("GROUP BY $-.name YIELD COUNT($-.start_year)", "SyntaxError: Yield `start_year' isn't in output fields"),
    ("GROUP BY $-.name YIELD $-.id", "SyntaxError: Yield `id' isn't in group fields"),
    ("GROUP BY $-.name YIELD $v.id", "SyntaxError: Can't support variableExpression"),
    ("GROUP BY team YIELD COUNT($-.id), $-.name AS teamName", "SyntaxError: Group `team' isn't in output fields"),
    ("GROUP BY 1+1 YIELD COUNT(1)", "SyntaxError: Group `(1+1)' isn't in output fields"),
])
def test_error_texts(text, error):
    p = pipeline.Pipeline(None, 1)
    out = p._group_by(text, INTERIM)
    assert not out.ok
    if error is not None:
        assert out.error == error
    else:
        assert out.error.startswith("SyntaxError: ")


def test_errors_are_not_reached_on_empty_input():
    """execute() :182-202: an empty input answers with the column names before checkAll runs, but after
    prepare()."""
    p = pipeline.Pipeline(None, 1)
    out = p._group_by("GROUP BY $-.nope YIELD COUNT($-.missing) AS c, $-.other", pipeline.Interim(["id"]))
    assert out.ok and out.names == ["c", "$-.other"] and out.rows == [] and out.col_types == []
    assert not p._group_by("GROUP BY $-.nope YIELD SUM(*)", pipeline.Interim(["id"])).ok
    dup = pipeline.Interim(["a", "a"], [2, 2], [(("int", 1), ("int", 2))])
    out = p._group_by("GROUP BY $-.a YIELD $-.a", dup)             # DuplicateColumn (:606-622)
    assert not out.ok and out.error == "Duplicate column `a'"


def test_later_sentences_stay_refused(nba):
    ds, o = nba
    for tail in ("ORDER BY $-.name", "LIMIT 2", "YIELD COUNT(*)"):
        with pytest.raises(pipeline.PipelineError, match="only GO sentences run in this path"):
            pipeline.run(o, ds.space, fixtures.nba_query("GO FROM {P:Tim Duncan} OVER like YIELD like._dst AS name | " + tail), EDGES)


# ----------------------------------------------------------------------------- independent computation
def _i64(v):
    return ngql.to_i64(v)


def _independent(rows, names, key_cols, aggs):
    """Dict of lists: group the rows' cells by the key columns' cells, then fold each list. `aggs' is a
    list of (function, column name or a constant cell)."""
    idx = {n: i for i, n in enumerate(names)}
    lists = {}
    for r in rows:
        lists.setdefault(tuple(r[idx[k]] for k in key_cols), []).append(r)
    out = []
    for key, rs in lists.items():
        row = []
        for fn, col in aggs:
            cells = [r[idx[col]] if isinstance(col, str) else col for r in rs]
            first = next((c for c in cells if c[0] in ("int", "id", "timestamp", "double")), None)
            same = [c[1] for c in cells if first is not None and c[0] == first[0]]
            ints = [c[1] for c in cells if c[0] == "int"]
            if fn == "":
                row.append(cells[-1])
            elif fn == "COUNT":
                row.append(("int", len(cells)))
            elif fn == "COUNT_DISTINCT":
                row.append(("int", len({c for c in cells})))
            elif fn == "SUM":
                if first is None:
                    row.append(("int", 0))
                elif first[0] == "double":
                    acc = same[0]
                    for v in same[1:]:
                        acc += v
                    row.append(("double", acc))
                else:
                    row.append((first[0], _i64(sum(same))))
            elif fn == "AVG":
                if first is None:
                    row.append(("double", 0.0))
                elif first[0] == "double":
                    acc = same[0]
                    for v in same[1:]:
                        acc += v
                    row.append(("double", acc / len(cells)))
                elif first[0] == "int":
                    row.append(("double", float(_i64(sum(same))) / len(cells)))
                else:
                    row.append(("double", struct.unpack("<d", struct.pack("<q", _i64(sum(same))))[0] / len(cells)))
            elif fn in ("MAX", "MIN"):
                pick = max if fn == "MAX" else min
                row.append(pick(cells, key=lambda c: c[1]))
            elif fn == "STD":
                xs = [float(c[1]) for c in cells if c[0] in ("int", "double")]
                if not xs:
                    row.append(("int", 0))
                else:
                    if first[0] in ("int", "double"):
                        acc = same[0]
                        for v in same[1:]:
                            acc = acc + v if first[0] == "double" else _i64(acc + v)
                        avg = float(acc) / len(cells)
                    else:
                        avg = None
                    s2 = 0.0
                    for x in xs:
                        s2 += (x - avg) * (x - avg)
                    row.append(("double", math.sqrt(s2 / len(xs))))
            else:
                acc = None
                for v in ints:
                    acc = v if acc is None else (acc & v if fn == "BIT_AND" else acc | v if fn == "BIT_OR" else acc ^ v)
                row.append(("int", acc if acc is not None else 0))
        out.append(tuple(row))
    return sorted(out, key=repr)


ALL_FUNCS = ["COUNT", "COUNT_DISTINCT", "SUM", "AVG", "MAX", "MIN", "STD", "BIT_AND", "BIT_OR", "BIT_XOR"]


@pytest.mark.parametrize("keys", [["k"], ["d"], ["k", "s"], ["s"]])
@pytest.mark.parametrize("col", ["a", "x", "d"])
def test_restatement_equals_independent(rmat_rows, keys, col):
    """Every function over an INT (a), a DOUBLE (x) and a VID (d) column, by a low-cardinality key, a
    high-cardinality key, two keys and a string key."""
    _, _, _, it = rmat_rows
    text = "GROUP BY " + ", ".join("$-." + k for k in keys) + " YIELD " + \
        ", ".join("$-." + k for k in keys) + ", " + ", ".join(f"{f}($-.{col})" for f in ALL_FUNCS)
    names, types, rows = groupby.run(ngql.parse_group_by(text), it.names, it.types, it.rows)
    want = _independent(groupby.typed_rows(it.names, it.types, it.rows), it.names, keys,
                        [("", k) for k in keys] + [(f, col) for f in ALL_FUNCS])
    assert len(want) >= 2
    assert sorted(rows, key=repr) == want
    assert names[:len(keys)] == ["$-." + k for k in keys] and names[-1] == f"BIT_XOR($-.{col})"
    assert types == [{"int": 2, "id": 3, "double": 5, "str": 6}[k] for k, _ in rows[0]]
    if col == "d":                                                # VID sums keep their type; BIT_* ignore them
        assert rows[0][len(keys) + 2][0] == "id" and rows[0][-1] == ("int", 0)


def test_constants_star_and_wraparound(rmat_rows):
    _, _, _, it = rmat_rows
    text = ("GROUP BY $-.k YIELD $-.k AS k, COUNT(*), COUNT_DISTINCT(*), SUM(1.5), SUM(%d), AVG(2), MAX(7), "
            "BIT_XOR(3), 1+1 AS cal, STD(4)" % (2 ** 62))
    _, types, rows = groupby.run(ngql.parse_group_by(text), it.names, it.types, it.rows)
    counts = {}
    for r in groupby.typed_rows(it.names, it.types, it.rows):
        counts[r[5]] = counts.get(r[5], 0) + 1
    assert len(rows) == len(counts) >= 2
    for r in rows:
        n = counts[r[0]]
        acc = 0.0
        for _ in range(n):
            acc += 1.5
        assert r[1:] == (("int", n), ("int", 1), ("double", acc), ("int", _i64(n * 2 ** 62)), ("double", 2.0),
                         ("int", 7), ("int", 3 if n % 2 else 0), ("int", 2), ("double", 0.0))
    assert types == [2, 2, 2, 5, 2, 5, 2, 2, 2, 5]


def test_mixed_type_sum_and_group_keeps_last():
    """Sum takes the type of its first summable value and ignores the others; Avg still counts them;
    Group keeps the last value; MAX / MIN compare the union's type before its value."""
    it = pipeline.Interim(["k", "v"], [2, 0], [
        (("int", 1), ("str", "z")), (("int", 1), ("int", 5)), (("int", 1), ("double", 2.5)),
        (("int", 1), ("int", -7)), (("int", 2), ("double", 0.25)), (("int", 2), ("int", 1)),
        (("int", 2), ("double", 0.5)), (("int", 3), ("str", "q"))])
    s = ngql.parse_group_by("GROUP BY $-.k YIELD $-.k, SUM($-.v), AVG($-.v), COUNT($-.v), BIT_OR($-.v), "
                            "MAX($-.v), MIN($-.v), STD($-.v)")
    _, types, rows = groupby.run(s, it.names, it.types, it.rows)
    assert sorted(rows, key=repr) == sorted([
        (("int", 1), ("int", -2), ("double", -0.5), ("int", 4), ("int", 5 | -7), ("str", "z"), ("int", -7),
         ("double", math.sqrt(((5 + .5) ** 2 + (2.5 + .5) ** 2 + (-7 + .5) ** 2) / 3))),
        (("int", 2), ("double", 0.75), ("double", 0.25), ("int", 3), ("int", 1), ("double", 0.5), ("int", 1),
         ("double", math.sqrt(((0.25 - .25) ** 2 + (1 - .25) ** 2 + (.5 - .25) ** 2) / 3))),
        (("int", 3), ("int", 0), ("double", 0.0), ("int", 1), ("int", 0), ("str", "q"), ("str", "q"), ("int", 0)),
    ], key=repr)
    assert types[:4] == [2, 2, 5, 2]
    it2 = pipeline.Interim(["k", "v"], [2, 2], [(("int", 1), ("int", 5)), (("int", 1), ("int", 9))])
    _, _, rows = groupby.run(ngql.parse_group_by("GROUP BY k YIELD $-.k AS k, $-.k"), it2.names, it2.types, it2.rows)
    assert rows == [(("int", 1), ("int", 1))]


def test_empty_go_feeds_group_by(rmat_rows):
    ds, o, _, _ = rmat_rows
    out = pipeline.run(o, ds.space, "GO FROM 1 OVER e WHERE e.p0 < 0 YIELD e._dst AS d, e.p0 AS w "
                                    "| GROUP BY $-.d YIELD $-.d, COUNT(*), SUM($-.w) AS total")
    assert out.ok and out.names == ["$-.d", "COUNT(*)", "total"] and out.rows == []


def test_pipeline_equals_direct_run(rmat_rows):
    ds, o, q, it = rmat_rows
    tail = "GROUP BY $-.k YIELD $-.k, COUNT(*), SUM($-.b), MAX($-.d), COUNT_DISTINCT($-.a)"
    out = pipeline.run(o, ds.space, q + " | " + tail)
    _, types, rows = groupby.run(ngql.parse_group_by(tail), it.names, it.types, it.rows)
    assert out.ok and sorted(out.rows, key=repr) == sorted(rows, key=repr) and out.col_types == types
