"""FETCH PROP ON tags / edges, host path: the FetchVerticesExecutor / FetchEdgesExecutor restatement
(nebula_amd/fetch.py) through pipeline.run(..., fetch=True) on the oracle backend against the reference answers
(tests/golden/fetch_cases.py), the parser's forms and syntax errors, every reference error text, empty inputs,
FETCH feeding a following GO, and the default that still refuses the sentence."""
import pytest

from nebula_amd import fetch, ngql, pipeline
from oracle import oracle
from tests import fixtures
from tests.golden.fetch_cases import CASES

EDGES = ["serve", "like", "teammate"]
P = ngql.nebula_hash


@pytest.fixture(scope="module")
def nba():
    ds = fixtures.nba()
    o = oracle.Oracle()
    ds.load_oracle(o)
    return ds, o, fetch.Catalog.of(ds.num_parts, ds.schemas)


def run(nba, q, **kw):
    ds, o, cat = nba
    return pipeline.run(o, ds.space, fixtures.nba_query(q), EDGES, fetch=True, catalog=cat, order_limit=True, **kw)


def check_golden(case, out):
    name, _, cols, want = case
    if want == "syntax":
        assert not out.ok and out.error.startswith("SyntaxError: "), out.error
        return
    if want == "error":
        assert not out.ok and not out.error.startswith("SyntaxError"), out.error
        return
    assert out.ok, out.error
    if cols is not None:
        assert out.names == cols
    if want == "empty":
        assert out.rows == []
    elif want is not None:
        assert fixtures.normalize_cells(out.rows) == fixtures.nba_expected(want)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_known_answers(nba, case):
    check_golden(case, run(nba, case[1]))


def test_default_still_refuses(nba):
    ds, o, cat = nba
    with pytest.raises(pipeline.PipelineError) as x:
        pipeline.run(o, ds.space, "FETCH PROP ON player 100", EDGES)
    assert str(x.value) == "only GO sentences run in this path: FETCH PROP ON player 100"
    with pytest.raises(pipeline.PipelineError):
        pipeline.run(o, ds.space, "GO FROM 1 OVER like | FETCH PROP ON player $-.id", EDGES, catalog=cat)


def test_schemas_are_asked_for_when_the_pipeline_is_built(nba):
    """A backend that cannot name its schemas needs catalog=: said at construction, not at the first FETCH."""
    ds, o, cat = nba
    with pytest.raises(pipeline.PipelineError, match="catalog"):
        pipeline.Pipeline(o, ds.space, EDGES, fetch=True)


# ----------------------------------------------------------------------------- parser
def test_parser_forms():
    s = ngql.parse_fetch('FETCH PROP ON player, team 1, -2, hash("x") YIELD DISTINCT player.name AS n, team.name')
    assert isinstance(s, ngql.FetchVerticesSentence) and s.tags == ["player", "team"] and s.distinct and s.has_yield
    assert [ngql.eval_const(e) for e in s.vids] == [1, -2, P("x")]
    assert [(y.alias, y.expr.to_string()) for y in s.yields] == [("n", "player.name"), ("", "team.name")]
    s = ngql.parse_fetch("fetch prop on * $-.id")
    assert s.tags == ["*"] and (s.from_type, s.from_col) == (1, "id") and not s.has_yield
    s = ngql.parse_fetch("FETCH PROP ON team $-")
    assert (s.from_type, s.from_col) == (1, "id")
    s = ngql.parse_fetch("FETCH PROP ON player $v.c YIELD player.age, $v.c")
    assert (s.from_type, s.from_var, s.from_col) == (2, "v", "c")
    s = ngql.parse_fetch('FETCH PROP ON serve 1->2, hash("a") -> 4@7, 5->6@-3 YIELD serve.start_year')
    assert isinstance(s, ngql.FetchEdgesSentence) and s.edges == ["serve"]
    assert [(ngql.eval_const(a), ngql.eval_const(b), r) for a, b, r in s.keys] == [(1, 2, 0), (P("a"), 4, 7), (5, 6, -3)]
    s = ngql.parse_fetch("FETCH PROP ON serve $-.s->$-.d@$-.r")
    assert s.from_type == 1 and (s.src_ref.prop, s.dst_ref.prop, s.rank_ref.prop) == ("s", "d", "r")
    s = ngql.parse_fetch("FETCH PROP ON serve $a.s -> $a.d YIELD DISTINCT serve._dst")
    assert s.from_type == 2 and s.rank_ref is None and s.distinct and s.ref_string() == "$a.s->$a.d"
    assert ngql.is_fetch("  fetch PROP ON x 1") and not ngql.is_fetch("GO FROM 1 OVER fetch")


@pytest.mark.parametrize("q", [
    "FETCH PROP player 1", "FETCH PROP ON 1", "FETCH PROP ON player", "FETCH PROP ON player 1 YIELD",
    "FETCH PROP ON player 1,", "FETCH PROP ON serve 1->", "FETCH PROP ON serve 1->2@x", "FETCH PROP ON * 1->2",
    "FETCH PROP ON serve $-.a->$v.b", "FETCH PROP ON player 1.5", 'FETCH PROP ON player "x"', "FETCH PROP ON player 1 2",
    "FETCH PROP ON serve $-.a->3"])
def test_syntax_errors(nba, q):
    with pytest.raises(SyntaxError):
        ngql.parse_fetch(q)
    out = run(nba, q)
    assert not out.ok and out.error.startswith("SyntaxError: ")
    out = run(nba, "GO FROM {P:Tim Duncan} OVER like | " + q)       # the whole text is parsed before anything runs
    assert not out.ok and out.error.startswith("SyntaxError: ")


# ----------------------------------------------------------------------------- error texts
GO_ID = "GO FROM {P:Boris Diaw} OVER like YIELD like._dst AS id"
GO_SD = "GO FROM {P:Boris Diaw} OVER serve YIELD serve._src AS s, serve._dst AS d, serve._rank AS r"


@pytest.mark.parametrize("q,text", [
    ("FETCH PROP ON player $v.id", "Variable `v' not defined"),
    (GO_ID + " | FETCH PROP ON player $-.*", "Cant not use `*' to reference a vertex id column."),
    (GO_ID + " | FETCH PROP ON player $-.nope", "Column `nope' not found"),
    (GO_ID + ", like.likeness AS id | FETCH PROP ON player $-.id", "Duplicate column `id'"),
    ("GO FROM {P:Boris Diaw} OVER like YIELD $$.player.name AS id | FETCH PROP ON player $-.id", "Column `id' not found"),
    ("FETCH PROP ON abc 1", "Unknown error(406): "),
    ("FETCH PROP ON player, player 1", "tag(player) was dup"),
    ("FETCH PROP ON player 1 YIELD COUNT(player.age)", "SyntaxError: Do not support aggregated query with fetch prop on."),
    ("FETCH PROP ON player 1 YIELD $^.player.name", "SyntaxError: tag.prop and edgetype.prop are supported in fetch sentence."),
    ("FETCH PROP ON player 1 YIELD team.name", "SyntaxError: Near [team.name], tag should be declared in `ON' clause first."),
    ("FETCH PROP ON player 1 YIELD player.name1", "`player' is not a prop of `name1'"),
    ("FETCH PROP ON serve, like 1->2", "fetch prop on edge support only one edge label now."),
    ("FETCH PROP ON abc 1->2", "Unknown error(407): "),
    (GO_SD + " | FETCH PROP ON serve $-.*->$-.d", "Can not use `*' to reference a vertex id column."),
    ("$a = " + GO_SD + "; $b = " + GO_SD + "; FETCH PROP ON serve $a.s->$b.d", "SyntaxError: Near $a.s->$b.d, Only support single data source."),
    ("FETCH PROP ON serve $a.s->$a.d", "Variable `a' not defined"),
    ("FETCH PROP ON serve 1->2 YIELD $$.team.name", "SyntaxError: tag.prop and edgetype.prop are supported in fetch sentence."),
    (GO_SD + " | FETCH PROP ON serve $-.s->$-.d YIELD $-.s", "SyntaxError: `$-' and `$variable' not supported in fetch yet."),
    ("FETCH PROP ON serve 1->2 YIELD like.likeness", "SyntaxError: Near [like.likeness], edge should be declared in `ON' clause first."),
    ("FETCH PROP ON serve 1->2 YIELD serve.nope", "`nope' is not a prop of `serve'"),
    (GO_SD + " | FETCH PROP ON serve $-.s->$-.nope", "Column `nope' not found"),
    (GO_SD + ", serve._dst AS d | FETCH PROP ON serve $-.s->$-.d", "Duplicate column `d'"),
])
def test_error_texts(nba, q, text):
    out = run(nba, q)
    assert not out.ok and out.error == text


# ----------------------------------------------------------------------------- semantics beyond the golden cases
def test_empty_inputs(nba):
    """onEmptyInputs: the column names and no rows, no types; `$-` without a pipe is no error."""
    out = run(nba, "FETCH PROP ON player $-.id YIELD player.name")
    assert out.ok and out.names == ["VertexID", "player.name"] and out.rows == [] and out.col_types == []
    out = run(nba, "FETCH PROP ON serve $-.s->$-.d")
    assert out.ok and out.names == ["serve._src", "serve._dst", "serve._rank", "serve.start_year", "serve.end_year"]
    assert out.rows == [] and out.col_types == []
    out = run(nba, "GO FROM {P:NON EXIST VERTEX ID} OVER like YIELD like._dst AS id | FETCH PROP ON player $-.id")
    assert out.ok and out.names == ["VertexID"] and out.rows == []


def test_default_row_rule(nba):
    """A vid without data gives no row, unless YIELD reads the input: then a row of default props."""
    q = "GO FROM {P:Boris Diaw} OVER like YIELD like._dst AS id | FETCH PROP ON team $-.id YIELD team.name"
    assert run(nba, q).rows == []
    out = run(nba, q + ", $-.id")
    assert out.names == ["VertexID", "team.name", "$-.id"]
    assert fixtures.normalize_cells(out.rows) == fixtures.nba_expected(
        [("P:Tony Parker", "", "P:Tony Parker"), ("P:Tim Duncan", "", "P:Tim Duncan")])
    # `$var.x' in YIELD is no input prop (expCtx_->hasInputProp()): the rows stay out
    out = run(nba, "$v = GO FROM {P:Boris Diaw} OVER like YIELD like._dst AS id; FETCH PROP ON team $v.id YIELD team.name, $v.id")
    assert out.ok and out.rows == []
    # a tag the vertex lacks among several: its props are defaults
    out = run(nba, "FETCH PROP ON player, team {P:Boris Diaw}, {T:Spurs} YIELD player.age, team.name")
    assert fixtures.normalize_cells(out.rows) == fixtures.nba_expected([("P:Boris Diaw", 36, ""), ("T:Spurs", 0, "Spurs")])


def test_rows_types_and_order(nba):
    """One row per input row in input order (a repeated vid repeats); the interim typed from the first record."""
    out = run(nba, "GO 2 STEPS FROM {P:Boris Diaw} OVER like YIELD like._dst AS id | FETCH PROP ON player $-.id YIELD player.age > 40, player.name")
    ref = run(nba, "GO 2 STEPS FROM {P:Boris Diaw} OVER like YIELD like._dst AS id")
    assert [r[0][1] for r in out.rows] == [r[0][1] for r in ref.rows] and len(out.rows) == 5
    assert out.col_types == [pipeline.T_VID, pipeline.T_BOOL, pipeline.T_STRING]
    assert [k for k, _ in out.rows[0]] == ["id", "bool", "str"]
    out = run(nba, "FETCH PROP ON serve {P:Marco Belinelli}->{T:Hornets}@1, {P:Marco Belinelli}->{T:Hornets}, {P:Marco Belinelli}->{T:Hornets}@2")
    assert out.col_types == [pipeline.T_VID, pipeline.T_VID, pipeline.T_INT, pipeline.T_INT, pipeline.T_INT]
    assert [tuple(v for _, v in r)[2:] for r in out.rows] == [(1, 2016, 2017), (0, 2010, 2012)]
    out = run(nba, "FETCH PROP ON serve {P:Boris Diaw}->{T:Hawks}, {P:Boris Diaw}->{T:Hawks} YIELD serve._type, serve.end_year - serve.start_year AS y")
    assert out.names[3:] == ["serve._type", "y"] and len(out.rows) == 2
    assert [v for _, v in out.rows[0]][3:] == [fixtures.nba().schemas[2].sid, 2]


def test_no_yield_columns_from_response(nba):
    """Without YIELD the columns are the tags seen in the response, in tag id order."""
    out = run(nba, "FETCH PROP ON team, player {P:Boris Diaw}")
    assert out.names == ["VertexID", "player.name", "player.age"]
    out = run(nba, "FETCH PROP ON team, player {P:Boris Diaw}, {T:Spurs}")
    assert out.names == ["VertexID", "player.name", "player.age", "team.name"]
    assert fixtures.normalize_cells(out.rows) == fixtures.nba_expected(
        [("P:Boris Diaw", "Boris Diaw", 36, ""), ("T:Spurs", "", 0, "Spurs")])


def test_fetch_feeds_go(nba):
    """FETCH calls onResult_: its interim is the input of the sentence behind it."""
    out = run(nba, "FETCH PROP ON player {P:Boris Diaw} YIELD player.name | GO FROM $-.VertexID OVER like YIELD like._dst AS id, $-.VertexID AS me")
    assert fixtures.normalize_cells(out.rows) == fixtures.nba_expected(
        [("P:Tony Parker", "P:Boris Diaw"), ("P:Tim Duncan", "P:Boris Diaw")])
    out = run(nba, GO_SD + " | FETCH PROP ON serve $-.s->$-.d@$-.r YIELD serve._dst AS team | FETCH PROP ON team $-.team")
    assert sorted(v for r in out.rows for k, v in r if k == "str") == ["Hawks", "Hornets", "Jazz", "Spurs", "Suns"]
    out = run(nba, "$f = FETCH PROP ON player {P:Boris Diaw}; GO FROM $f.VertexID OVER like")
    assert len(out.rows) == 2
