"""FIND SHORTEST | ALL | NOLOOP PATH, host path: the parser's forms and errors, the FindPathExecutor restatement
(nebula_amd/findpath.py) through pipeline.run(..., find_path=True) on the oracle backend against the reference
FindPathTest answers (tests/golden/findpath_cases.py), the default's refusal, the vid-reference error texts, and the
enumeration of the device call's path DAG (findpath.paths_from_dag) on hand-made edge lists."""
import pytest

from nebula_amd import findpath, ngql, pipeline
from oracle import oracle
from tests import fixtures
from tests.golden.findpath_cases import CASES

EDGES = ["serve", "like", "teammate"]


@pytest.fixture(scope="module")
def nba():
    ds = fixtures.nba()
    o = oracle.Oracle()
    ds.load_oracle(o)
    return ds, o


def golden_text(text):
    for key, name in (("{NOBODY1}", "Nobody1"), ("{NOBODY2}", "Nobody2"), ("{NOBODY}", "Nobody"), ("{NONEXIST}", "NON EXIST VERTEX ID")):
        text = text.replace(key, str(ngql.nebula_hash(name)))
    return fixtures.nba_query(text)


def check_golden(case, out):
    if case.get("error") == "execution":
        assert not out.ok and not out.error.startswith("SyntaxError"), out.error
        return
    assert out.ok, out.error
    assert out.names == ["_path_"]
    assert all(len(r) == 1 and r[0][0] == "path" for r in out.rows)
    assert sorted(r[0][1] for r in out.rows) == sorted(golden_text(p) for p in case["paths"])


def test_golden_vids_are_the_suites():
    assert golden_text("{P:Tim Duncan}<like,0>{P:Tony Parker}") == "5662213458193308137<like,0>-7579316172763586624"
    assert golden_text("{T:Spurs}") == "7193291116733635180"


@pytest.mark.parametrize("case", CASES, ids=[f"path{c['line']}" for c in CASES])
def test_known_answers(nba, case):
    ds, o = nba
    check_golden(case, pipeline.run(o, ds.space, golden_text(case["query"]), EDGES, find_path=True))


def test_golden_covers_every_group():
    have = {(c["kind"], c["direction"], "," in c["query"].split("OVER")[-1] or "*" in c["query"].split("OVER")[-1]) for c in CASES}
    for kind in ngql.PATH_KINDS:
        for direction in ("", "REVERSELY", "BIDIRECT"):
            assert (kind, direction, False) in have                # SingleEdge x kind x direction
    assert ("SHORTEST", "", True) in have and ("ALL", "", True) in have   # MultiEdges
    assert sum(1 for c in CASES if c.get("piped")) == 3 and sum(1 for c in CASES if c.get("error")) == 2


def test_default_still_refuses(nba):
    ds, o = nba
    q = golden_text(CASES[0]["query"])
    with pytest.raises(pipeline.PipelineError) as e:
        pipeline.run(o, ds.space, q, EDGES)
    assert str(e.value) == "only GO sentences run in this path: " + q[:40]
    assert pipeline.run(o, ds.space, q, EDGES, find_path=True).ok


def test_parser_forms():
    s = ngql.parse_find_path("FIND SHORTEST PATH FROM 1, -2, hash(\"x\") TO 3 OVER like UPTO 4 STEPS")
    assert (s.kind, s.from_vids, s.to_vids, s.over, s.over_all, s.direction, s.upto) == \
        ("SHORTEST", [1, -2, ngql.nebula_hash("x")], [3], [("like", "")], False, ngql.FORWARD, 4)
    assert s.shortest and s.no_loop
    s = ngql.parse_find_path("find all path from $-.a to $v.b over like as l, serve reversely")
    assert (s.kind, s.from_type, s.from_col, s.to_type, s.to_var, s.to_col) == ("ALL", 1, "a", 2, "v", "b")
    assert s.over == [("like", "l"), ("serve", "")] and s.direction == ngql.REVERSELY and s.upto == 5
    assert not s.shortest and not s.no_loop
    s = ngql.parse_find_path("FIND NOLOOP PATH FROM 1 TO 2 OVER * BIDIRECT UPTO 0x10 STEPS")
    assert s.kind == "NOLOOP" and s.over_all and s.direction == ngql.BIDIRECT and s.upto == 16
    assert not s.shortest and s.no_loop
    assert ngql.is_find_path("  find shortest path from 1 to 2 over e") and not ngql.is_find_path("GO FROM 1 OVER find")
    # the new words are not keywords: GO texts that use them as names lex as before
    g = ngql.parse_go("GO FROM 1 OVER path YIELD path.upto AS shortest, path.find")
    assert g.over == [("path", "")] and g.column_names() == ["shortest", "path.find"]


@pytest.mark.parametrize("text", [
    "FIND PATH FROM 1 TO 2 OVER e",                               # no kind
    "FIND LONGEST PATH FROM 1 TO 2 OVER e",
    "FIND SHORTEST FROM 1 TO 2 OVER e",
    "FIND SHORTEST PATH TO 2 OVER e",
    "FIND SHORTEST PATH FROM 1 OVER e",
    "FIND SHORTEST PATH FROM 1 TO 2",
    "FIND SHORTEST PATH FROM 1 TO 2 OVER e UPTO STEPS",
    "FIND SHORTEST PATH FROM 1 TO 2 OVER e UPTO 3",
    "FIND SHORTEST PATH FROM 1 TO 2 OVER e UPTO -3 STEPS",
    "FIND SHORTEST PATH FROM 1 TO 2 OVER e UPTO 3 STEPS WHERE e.x > 1",   # where_clause is commented out of the grammar
    "FIND SHORTEST PATH FROM 1.5 TO 2 OVER e",
    "FIND SHORTEST PATH FROM \"a\" TO 2 OVER e",
    "FIND SHORTEST PATH FROM 1, $-.x TO 2 OVER e",
])
def test_parser_errors(nba, text):
    with pytest.raises((SyntaxError, ValueError)):
        ngql.parse_find_path(text)
    ds, o = nba
    out = pipeline.run(o, ds.space, text, EDGES, find_path=True)
    assert not out.ok and out.error.startswith("SyntaxError: ")


def test_reference_errors(nba):
    ds, o = nba
    tim = ngql.nebula_hash("Tim Duncan")
    run = lambda q: pipeline.run(o, ds.space, q, EDGES, find_path=True)
    out = run("FIND SHORTEST PATH FROM $nope.src TO %d OVER like" % tim)
    assert not out.ok and out.error == "Variable `nope' not defined"
    go = "GO FROM %d OVER like YIELD like._src AS src, like._dst AS dst" % tim
    out = run(go + " | FIND SHORTEST PATH FROM $-.src TO $-.nope OVER like")
    assert not out.ok and out.error == "Column `nope' not found"
    out = run("GO FROM %d OVER like YIELD like._src AS src, like._dst AS src | FIND ALL PATH FROM $-.src TO $-.src OVER like" % tim)
    assert not out.ok and out.error == "Duplicate column `src'"
    out = run("GO FROM %d OVER like YIELD like._src AS src | FIND ALL PATH FROM $-.src TO $-.src OVER like"
              % ngql.nebula_hash("NON EXIST VERTEX ID"))
    assert not out.ok and out.error == "Interim has no data."
    out = run("GO FROM %d OVER like YIELD $^.player.name AS src | FIND ALL PATH FROM $-.src TO 1 OVER like" % tim)
    assert not out.ok and out.error == "Column `src' not found"   # getVid of a string column
    out = run("FIND SHORTEST PATH FROM $-.src TO %d OVER like" % tim)         # no pipe: no vids, no rows, no error
    assert out.ok and out.rows == [] and out.names == ["_path_"]
    out = run("FIND SHORTEST PATH FROM %d TO %d OVER nosuchedge" % (tim, tim))
    assert not out.ok


def test_nothing_is_handed_on(nba):
    """FindPathExecutor never calls onResult_: the sentence behind the pipe runs without input."""
    ds, o = nba
    tim, tony = ngql.nebula_hash("Tim Duncan"), ngql.nebula_hash("Tony Parker")
    out = pipeline.run(o, ds.space, "FIND SHORTEST PATH FROM %d TO %d OVER like | GO FROM $-.id OVER like" % (tim, tony),
                       EDGES, find_path=True)
    assert out.ok and out.rows == []


def test_upto_bounds_the_length(nba):
    ds, o = nba
    run = lambda q: pipeline.run(o, ds.space, golden_text(q), EDGES, find_path=True)
    q = "FIND SHORTEST PATH FROM {P:Tiago Splitter} TO {P:LaMarcus Aldridge} OVER like UPTO %d STEPS"
    assert run(q % 2).rows == []                                  # the path has 3 edges
    assert len(run(q % 3).rows) == 1 and len(run(q % 4).rows) == 1


def test_paths_from_dag():
    names = {1: "e", 2: "f"}
    # two diamonds in a row, 1 -> {2, 3} -> 4 -> {5, 6} -> 7, to target 7 (bit 0); a second target 4 (bit 1) shares
    # the first diamond; the edge 9 -> 4 lies on no path from the source and is never reached
    E = [(1, 2, 1, 0, 3), (1, 3, 1, 0, 3), (2, 4, 1, 0, 3), (3, 4, 2, 5, 3), (4, 5, 1, 0, 1), (4, 6, 1, 0, 1), (5, 7, -1, 0, 1),
         (6, 7, 1, 0, 1), (9, 4, 1, 0, 2)]
    cols = list(zip(*E))
    rows = findpath.paths_from_dag([1], [7, 4], *cols, names)
    assert sorted(rows) == sorted([
        "1<e,0>2<e,0>4<e,0>5<-e,0>7", "1<e,0>2<e,0>4<e,0>6<e,0>7", "1<e,0>3<f,5>4<e,0>5<-e,0>7", "1<e,0>3<f,5>4<e,0>6<e,0>7",
        "1<e,0>2<e,0>4", "1<e,0>3<f,5>4"])
    assert findpath.paths_from_dag([1], [7], [], [], [], [], [], names) == []
