"""LOOKUP on the host: the parser, the reference's LookupTest answers (tests/golden/lookup_cases.py) through
lookup.py and scan_model, the index-key encoders against the reference's vectors and their arithmetic, the
truncating cast, and pipes over a table-backed fake backend that evaluates the device plan format in Python."""
import math
import struct
from types import SimpleNamespace as NS

import pytest

from nebula_amd import fetch, lookup, ngql, pipeline
from tests.golden import lookup_cases as G

INT, DOUBLE, BOOL, STRING = 2, 5, 1, 6


def catalog():
    return fetch.Catalog.of(G.PARTS, [NS(is_edge=e, sid=i, name=n, fields=f, ver=0) for e, i, n, f in G.SCHEMAS])


def indexes():
    types = {n: dict(f) for _, _, n, f in G.SCHEMAS}
    return [lookup.Index(i, n, s, e, [(f, types[s][f]) for f in fs]) for i, n, s, e, fs in G.INDEXES]


def table(name):
    """The golden rows of a tag / an edge type as scan_model takes them."""
    fields = next(f for _, _, n, f in G.SCHEMAS if n == name)
    if name in G.EDGES:
        return [(s, d, r, dict(zip([f for f, _ in fields], v))) for s, d, r, v in G.EDGES[name]]
    return [(v, dict(zip([f for f, _ in fields], vals))) for v, vals in G.VERTICES.get(name, [])]


def model(query):
    """(rows, names, index id) or the error text."""
    s = ngql.parse_lookup(query)
    plan = lookup.plan_of(catalog(), indexes(), s)
    return lookup.scan_model(table(s.from_), plan, G.PARTS), plan.names, plan.index.index_id


def check_case(case, outcome):
    """A pipeline Outcome against a golden case."""
    name, query, want, names = case
    if want == G.SYNTAX:
        assert not outcome.ok and outcome.error.startswith("SyntaxError"), outcome.error
    elif want == G.EXEC:
        assert not outcome.ok and not outcome.error.startswith("SyntaxError"), outcome.error
    else:
        assert outcome.ok, outcome.error
        assert sorted(tuple(v for _, v in r) for r in outcome.rows) == sorted(want)
        if names is not None:
            assert outcome.names == names


# ----------------------------------------------------------------------------- parser
def test_parser_round_trips():
    s = ngql.parse_lookup("LOOKUP ON player WHERE player.age > 40 && player.name != \"x\" YIELD player.name AS n, player.age")
    assert s.from_ == "player" and s.has_yield and [y.alias for y in s.yields] == ["n", ""]
    assert s.where.to_string() == "((player.age>40)&&(player.name!=x))"
    assert [y.expr.to_string() for y in s.yields] == ["player.name", "player.age"]
    assert ngql.parse_lookup("lookup on t where t.a == 1").yields == []
    assert ngql.parse_lookup("LOOKUP ON t").where is None         # the executor's "Where clause is required"
    assert ngql.is_lookup("  lookup on t where t.a == 1") and not ngql.is_lookup("GO FROM 1 OVER lookup")
    assert not ngql.is_lookup("lookups")


@pytest.mark.parametrize("text", ["LOOKUP ON t WHERE col1 == 200", "LOOKUP ON t WHERE t.a == 1 && b < 2",
                                  "LOOKUP t WHERE t.a == 1", "LOOKUP ON t WHERE t.a == 1 YIELD", "LOOKUP ON t WHERE",
                                  "LOOKUP ON t WHERE t.a == 1 extra"])
def test_parser_syntax_errors(text):
    with pytest.raises(SyntaxError):
        ngql.parse_lookup(text)


def test_go_texts_lex_as_before():
    s = ngql.parse_go("GO FROM 1 OVER lookup YIELD lookup._dst AS lookup")
    assert s.yields[0].alias == "lookup"


# ----------------------------------------------------------------------------- golden
@pytest.mark.parametrize("case", G.CASES, ids=[c[0] for c in G.CASES])
def test_golden_through_the_model(case):
    name, query, want, names = case
    try:
        rows, got_names, _ = model(query)
    except SyntaxError:
        assert want == G.SYNTAX
        return
    except lookup.LookupError as e:
        assert want in (G.SYNTAX, G.EXEC)
        assert str(e).startswith("SyntaxError") == (want == G.SYNTAX), str(e)
        return
    assert sorted(rows) == sorted(want)
    if names is not None:
        assert got_names == names


@pytest.mark.parametrize("query,text", [
    ("LOOKUP ON lookup_tag_1", "SyntaxError: Where clause is required"),
    ("LOOKUP ON nothing WHERE nothing.a == 1", "Tag or Edge was not found : nothing"),
    ("LOOKUP ON teacher WHERE teacher.age == 1", "Unknown error(411): "),
    ("LOOKUP ON lookup_tag_2 WHERE lookup_tag_2.col1 == true", "Unknown error(411): "),
    ("LOOKUP ON lookup_tag_2 WHERE lookup_tag_2.col2 == 1 OR lookup_tag_2.col2 == 2",
     "SyntaxError: OR and XOR are not supported in lookup where clause ：((lookup_tag_2.col2==1)||(lookup_tag_2.col2==2))"),
    ("LOOKUP ON lookup_tag_2 WHERE lookup_tag_2.col2 == 1 XOR lookup_tag_2.col2 == 2",
     "SyntaxError: OR and XOR are not supported in lookup where clause ：((lookup_tag_2.col2==1)XOR(lookup_tag_2.col2==2))"),
    ("LOOKUP ON tag_with_str WHERE tag_with_str.c2 CONTAINS \"a\"", "SyntaxError: Unsupported 'CONTAINS' in where clause"),
    ("LOOKUP ON lookup_tag_2 WHERE lookup_tag_2.col2 != lookup_tag_2.col3",
     "SyntaxError: Does not support left and right are both property"),
    ("LOOKUP ON lookup_tag_2 WHERE udf_is_in(lookup_tag_2.col2, 1)", "SyntaxError: Function expressions are not supported yet"),
    ("LOOKUP ON lookup_tag_2 WHERE 1 == 1", "SyntaxError: Unsupported expression ：(1==1)"),
    ("LOOKUP ON student WHERE teacher.number == 1", "SyntaxError: Edge or Tag name error : teacher "),
    ("LOOKUP ON student WHERE student.number == 1 YIELD teacher.age", "SyntaxError: Edge or Tag name error : teacher "),
    ("LOOKUP ON student WHERE student.number == 1 YIELD student.nothing", "Unknown column `nothing' in schema"),
    ("LOOKUP ON student WHERE student.number == 1 YIELD COUNT(student.age)", "SyntaxError: Not supported yet"),
    ("LOOKUP ON student WHERE student.number == 1 YIELD student.age + 1",
     "SyntaxError: Expressions other than AliasProp are not supported"),
    ("LOOKUP ON tag_with_str WHERE tag_with_str.c2 > \"a\" and tag_with_str.c3 == \"b\"",
     "SyntaxError: Data type of field c2 not support range scan"),
    ("LOOKUP ON lookup_tag_2 WHERE lookup_tag_2.col2 > (lookup_tag_2.col3 - 100)", "Lookup vertices failed"),
    ("LOOKUP ON lookup_tag_2 WHERE lookup_tag_2.col2 == 1 and lookup_tag_2.col2 == 2", "Lookup vertices failed"),
    ("LOOKUP ON lookup_tag_2 WHERE lookup_tag_2.col2 >= 1 and lookup_tag_2.col2 == 1", "Lookup vertices failed"),
])
def test_status_texts(query, text):
    with pytest.raises(lookup.LookupError) as e:
        model(query)
    assert str(e.value) == text


@pytest.mark.parametrize("case", G.OPTIMIZER, ids=[str(i) for i in range(len(G.OPTIMIZER))])
def test_optimizer_chooses(case):
    tag, filters, accept = case
    schema = next(f for _, _, n, f in G.SCHEMAS if n == tag)
    mine = [i for i in indexes() if i.schema_name == tag]
    if accept is None:
        with pytest.raises(lookup.LookupError) as e:
            lookup.find_optimal_index(mine, filters, schema)
        assert str(e.value) == lookup.INDEX_NOT_FOUND
    else:
        assert lookup.find_optimal_index(mine, filters, schema).name in accept


def test_chosen_index_of_a_sentence():
    assert model("LOOKUP ON lookup_tag_1 WHERE lookup_tag_1.col1 == 200")[2] == 1
    assert model("LOOKUP ON lookup_tag_1 WHERE lookup_tag_1.col2 == 200")[2] == 3
    assert model("LOOKUP ON lookup_tag_2 WHERE lookup_tag_2.col3 > 100.5")[2] == 4
    assert model("LOOKUP ON lookup_edge_1 WHERE lookup_edge_1.col2 == 201")[2] == 8
    # two indexes of one range hint count: the std::map keeps the last
    mine = [i for i in indexes() if i.schema_name == "t1"]
    schema = next(f for _, _, n, f in G.SCHEMAS if n == "t1")
    assert lookup.find_optimal_index(mine, [("c1", G.EQ), ("c2", G.GT)], schema).name == "i5"


def test_quirk_eq_then_greater_scans_for_the_greater():
    """`c == 100 and c > 101`: writeScanItem raises the begin value to 101 and keeps its relation EQ; the end stays
    (EQ, 100) and normalizes to 100 + 1: begin == end, a prefix scan for 101. With `c > 200` the range is empty."""
    def ranges(where):
        plan = lookup.plan_of(catalog(), indexes(), ngql.parse_lookup("LOOKUP ON lookup_tag_2 WHERE " + where))
        assert not plan.required_filter
        return plan.ranges()
    k = lambda v: struct.unpack(">Q", lookup.encode_int64(v))[0]
    assert ranges("lookup_tag_2.col2 == 100 and lookup_tag_2.col2 > 101") == [("col2", k(101), k(101))]
    assert ranges("lookup_tag_2.col2 == 100 and lookup_tag_2.col2 > 200") == [("col2", k(200), k(101))]


# ----------------------------------------------------------------------------- encoders
def test_int_key_vectors_and_order():
    for v, raw in G.INT_KEYS:
        assert lookup.encode_int64(v) == raw and lookup.decode_int64(raw) == v
    vals = [-(1 << 63), -(1 << 63) + 1, -1, 0, 1, (1 << 63) - 2, (1 << 63) - 1]
    keys = [lookup.encode_int64(v) for v in vals]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)


def test_round_trips():
    for v in G.ROUND_TRIP:
        t = DOUBLE if isinstance(v, float) else INT
        back = lookup.decode_variant(lookup.encode_variant(v), t)
        assert back == v and type(back) is type(v)


def u64(raw):
    return struct.unpack(">Q", raw)[0]


def test_double_keys_are_the_references_arithmetic():
    """encodeDouble: `if (v < 0) i = -(INT64_MAX + i)` over the bits, then byte 0 ^= 0x80, big-endian. With m the
    magnitude bits of a negative value, INT64_MAX + (2^63 + m) = m - 1 (mod 2^64), so the key is 2^63 - (m - 1).
    No NaN is in the data."""
    top = 1 << 63
    sub = struct.unpack("<d", struct.pack("<Q", 1))[0]            # the smallest subnormal
    inf_bits = 0x7FF0000000000000
    assert u64(lookup.encode_double(0.0)) == top
    assert u64(lookup.encode_double(-0.0)) == 0                   # not below zero: only the top bit flips
    assert u64(lookup.encode_double(sub)) == top + 1
    assert u64(lookup.encode_double(-sub)) == top                 # m = 1: shares +0.0's key
    assert u64(lookup.encode_double(math.inf)) == top + inf_bits
    assert u64(lookup.encode_double(-math.inf)) == top - (inf_bits - 1)
    assert u64(lookup.encode_double(-1.5)) == top - (struct.unpack("<Q", struct.pack("<d", 1.5))[0] - 1)
    vals = [-math.inf, -1e300, -2.5, -1.0, -1e-300, 0.0, 1e-300, 1.0, 2.5, 1e300, math.inf]
    keys = [lookup.encode_double(v) for v in vals]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert lookup.decode_double(lookup.encode_double(-sub)) == 0.0


def test_bound_addition_saturates():
    assert lookup.bound_addition(INT, 5) == lookup.encode_int64(6)
    assert lookup.bound_addition(INT, (1 << 63) - 1) == b"\xff" * 8
    assert lookup.bound_addition(INT, -1) == lookup.encode_int64(0)


# ----------------------------------------------------------------------------- stated deviations
def test_property_operand_under_and_is_an_error_at_every_depth():
    """The reference returns E_INVALID_FILTER for `a > (b - 100)` from the top-level expression only and drops such
    a term silently under an AND; here it is the error at every depth."""
    for where in ("lookup_tag_2.col2 > (lookup_tag_2.col3 - 100)",
                  "lookup_tag_2.col2 == 100 && lookup_tag_2.col3 > (lookup_tag_2.col2 - 100)"):
        with pytest.raises(lookup.LookupError) as e:
            model("LOOKUP ON lookup_tag_2 WHERE " + where)
        assert str(e.value) == lookup.INVALID_FILTER


def test_timestamp_bounds_take_the_int_branch():
    """boundVariant takes its double branch for every type but INT; a TIMESTAMP field's `>` / `<=` bound is an
    integer's here."""
    ts = [("at", 21)]
    cat = fetch.Catalog(1, tags={"t": (2, ts)})
    idx = [lookup.Index(1, "i", "t", False, ts)]
    plan = lookup.plan_of(cat, idx, ngql.parse_lookup("LOOKUP ON t WHERE t.at > 10 && t.at <= 20"))
    assert plan.ranges() == [("at", u64(lookup.encode_int64(11)), u64(lookup.encode_int64(21)))]
    rows = [(v, {"at": v}) for v in (10, 11, 20, 21)]
    assert sorted(lookup.scan_model(rows, plan)) == [(11,), (20,)]


# ----------------------------------------------------------------------------- the truncating cast
CAST_SCHEMA = [("a", INT), ("b", INT)]
CAST_ROWS = [(v, {"a": 1 if v != 3 else 2, "b": b}) for v, b in [(1, 99), (2, 100), (3, 100), (4, 101)]]


def cast_plan(where):
    cat = fetch.Catalog(1, tags={"t": (2, CAST_SCHEMA)})
    idx = [lookup.Index(1, "i", "t", False, CAST_SCHEMA)]
    return lookup.plan_of(cat, idx, ngql.parse_lookup("LOOKUP ON t WHERE " + where))


def test_accurate_scan_truncates_the_double():
    plan = cast_plan("t.a == 1 and t.b < 100.5")                  # end = encode(toInt(100.5)) = 100, exclusive
    assert not plan.required_filter
    assert sorted(lookup.scan_model(CAST_ROWS, plan)) == [(1,)]


def test_residual_term_compares_as_double():
    plan = cast_plan("t.a != 2 and t.b < 100.5")                  # `!=` on the first field: nothing scanned, all filtered
    assert plan.required_filter and plan.scan == []
    assert sorted(lookup.scan_model(CAST_ROWS, plan)) == [(1,), (2,)]


# ----------------------------------------------------------------------------- pipes over a fake backend
class TableBackend:
    """Rows in Python; lookup() evaluates the device plan format (key ranges, typed equalities, residual terms) the
    way csrc/lookup.hip does, go() records its input and answers a fixed row per input vid."""

    def __init__(self):
        self.go_inputs = []

    def catalog(self, space):
        return catalog()

    def lookup(self, space, spec):
        name = next(n for e, i, n, f in G.SCHEMAS if i == spec.schema_id and e == spec.is_edge)
        types = dict(next(f for _, _, n, f in G.SCHEMAS if n == name))
        rows = []
        for row in table(name):
            props, keep = row[-1], True
            for fld, kind, _, lo, hi, bits, sb in spec.fields:
                v = props[fld]
                if kind in (lookup.LK_INT, lookup.LK_DOUBLE):
                    k = u64(lookup.encode_variant(v))
                    keep &= (k == lo) if lo == hi else lo <= k < hi
                elif kind == lookup.LK_BOOL:
                    keep &= bool(v) == bool(bits)
                else:
                    keep &= v.encode() == sb
            for fld, kind, op, _, _, bits, sb in spec.terms:
                const = sb.decode() if kind == lookup.LK_STRING else bool(bits) if kind == lookup.LK_BOOL else \
                    struct.unpack("<d", struct.pack("<q", bits))[0] if kind == lookup.LK_DOUBLE else bits
                keep &= lookup.rel_eval(lookup.decode_variant(lookup.encode_variant(props[fld]), types[fld]), op, const)
            if keep:
                head = list(row[:-1])
                cells = [("id", h) for h in head[:2]] + [("int", h) for h in head[2:]]
                kinds = {INT: "int", DOUBLE: "double", BOOL: "bool", STRING: "str"}
                rows.append(tuple(cells + [(kinds[types[y]], props[y]) for y in spec.yields]))
        return NS(ok=True, error="", code=0, rows=rows, nrows=len(rows), col_types=[])

    def go(self, space, s, input=None, **kw):
        self.go_inputs.append(input)
        vids = [] if input is None else sorted({r[input.names.index(s.from_col)][1] for r in input.rows})
        return NS(ok=True, error="", col_types=[3], rows=[(("id", v + 1000),) for v in vids])


@pytest.mark.parametrize("case", G.CASES, ids=[c[0] for c in G.CASES])
def test_golden_through_the_plan_format(case):
    check_case(case, pipeline.run(TableBackend(), 1, case[1], lookup=True, indexes=indexes()))


def test_lookup_feeds_go():
    b = TableBackend()
    out = pipeline.run(b, 1, "LOOKUP ON lookup_tag_2 WHERE lookup_tag_2.col2 > 300 YIELD lookup_tag_2.col3 | "
                             "GO FROM $-.VertexID OVER e YIELD e._dst", ["e"], lookup=True, indexes=indexes())
    assert out.ok, out.error
    inp = b.go_inputs[0]
    assert inp.names == ["VertexID", "lookup_tag_2.col3"]
    assert sorted(r[0][1] for r in out.rows) == [1223, 1224, 1225]
    b = TableBackend()
    out = pipeline.run(b, 1, "$v = LOOKUP ON lookup_edge_2 WHERE lookup_edge_2.col2 == 100; "
                             "GO FROM $v.DstVID OVER e YIELD e._dst", ["e"], lookup=True, indexes=indexes())
    assert out.ok and [r[0][1] for r in out.rows] == [1221]
    assert b.go_inputs[0].names == ["SrcVID", "DstVID", "Ranking"]


def test_lookup_ignores_its_input():
    b = TableBackend()
    q = "LOOKUP ON lookup_tag_1 WHERE lookup_tag_1.col1 == 200"
    alone = pipeline.run(b, 1, q, lookup=True, indexes=indexes())
    piped = pipeline.run(b, 1, "GO FROM 1 OVER e YIELD e._dst AS id | " + q, ["e"], lookup=True, indexes=indexes())
    assert piped.ok and piped.rows == alone.rows and piped.names == alone.names == ["VertexID"]


def test_opt_in():
    with pytest.raises(pipeline.PipelineError) as e:
        pipeline.run(TableBackend(), 1, "LOOKUP ON lookup_tag_1 WHERE lookup_tag_1.col1 == 200")
    assert str(e.value) == "only GO sentences run in this path: LOOKUP ON lookup_tag_1 WHERE lookup_tag_"
    with pytest.raises(pipeline.PipelineError):                   # a backend without lookup()
        pipeline.Pipeline(NS(go=None), 1, lookup=True, indexes=indexes(), catalog=catalog())
    p = pipeline.Pipeline(TableBackend(), 1, lookup=True, indexes=indexes())
    assert p.run("LOOKUP ON lookup_tag_2 WHERE lookup_tag_2.col2 >= 100").ok and (p.lookups, p.lookup_rows) == (1, 6)
