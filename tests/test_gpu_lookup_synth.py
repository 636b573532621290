"""The LOOKUP kernels on synthetic tables loaded as KV rows, at the smallest shapes at which they can go wrong: row
counts around the 256-row chunk and over one grid turn, every stored width as scanned field, residual term and YIELD
column, bounds at and outside a narrowed column's range and at INT64_MAX, edges whose rows alternate between empty
adjacencies and 1 / 255 / 256 / 257 edges (the off[] upper-bound trap), order under grid max 1, 3 and the default,
and scratch reuse. The expectation is lookup.scan_model over the same rows; order is checked against storage order
(one part: the vertex table is sorted by vid, an adjacency by the KV key order of (rank, dst))."""
import pytest

from nebula_amd import engine, kvfmt, lookup, ngql, pipeline

pytestmark = pytest.mark.gpu

BOOL, INT, DOUBLE, STRING = 1, 2, 5, 6
I64MAX, I64MIN = (1 << 63) - 1, -(1 << 63)
# i1 .. i8 narrow to 1 / 2 / 4 / 8 bytes at export; d holds negatives and both zeros; s lengths 0, 1, 7, 8, 9, 300
FIELDS = [("i1", INT), ("i2", INT), ("i4", INT), ("i8", INT), ("d", DOUBLE), ("b", BOOL), ("s", STRING)]
STRS = ["", "a", "abcdefg", "abcdefgh", "abcdefghi", "x" * 300]
DBLS = [-2.5, -0.0, 0.0, 1.5, -1e300, 7.25]
I8 = [I64MIN, -1, 0, 1, I64MAX - 1, I64MAX]


def props(v):
    return {"i1": v % 256 - 128, "i2": (v * 7) % 65536 - 32768, "i4": (v * 100003) % (1 << 32) - (1 << 31),
            "i8": I8[v % 6], "d": DBLS[v % 6], "b": v % 3 == 0, "s": STRS[v % 6]}


def load(n, step=1):
    """n tag rows t on the vertices 0, step, 2 * step ...; the vertices between them hold tag u only (present 0)."""
    e = engine.Engine()
    e.add_space(1, 1)
    e.add_schema(1, False, 2, "t", FIELDS)
    e.add_schema(1, False, 3, "u", [("x", INT)])
    b = kvfmt.KVBatch()
    types = [t for _, t in FIELDS]
    rows = []
    for v in range(n * step):
        if v % step == 0:
            p = props(v)
            b.put(kvfmt.vertex_key(1, v, 2), kvfmt.encode_row(types, [p[f] for f, _ in FIELDS]))
            rows.append((v, p))
        else:
            b.put(kvfmt.vertex_key(1, v, 3), kvfmt.encode_row([INT], [v]))
    if n == 0:
        b.put(kvfmt.vertex_key(1, 0, 3), kvfmt.encode_row([INT], [0]))
    e.load_batch(1, b)
    e.commit(1)
    return e, rows


def index_on(*names, edge=False, schema="t", fields=FIELDS):
    t = dict(fields)
    return [lookup.Index(1, "i", schema, edge, [(n, t[n]) for n in names])]


def run(e, rows, q, idx):
    s = ngql.parse_lookup(q)
    plan = lookup.plan_of(e.catalog(1), idx, s)
    want = lookup.scan_model(rows, plan, 1)
    out = pipeline.run(e, 1, q, ["e"], lookup=True, indexes=idx)
    assert out.ok, out.error
    got = [tuple(v for _, v in r) for r in out.rows]
    assert sorted(got, key=repr) == sorted(want, key=repr), q
    return got, want


WHERE = {
    "all": ("i1", "t.i1 >= -128"),
    "none": ("i1", "t.i1 > 127"),
    "every_other": ("b", "t.b == true"),
    "i8_term": ("i1", "t.i1 != 100 && t.i8 < 0"),
}


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 65537])
@pytest.mark.parametrize("grid", [1, 3])
def test_row_counts(n, grid):
    e, rows = load(n, step=2 if n <= 257 else 1)
    with e:
        e.set_flag("lookup_grid_max", grid)
        for name, (field, where) in WHERE.items():
            got, _ = run(e, rows, "LOOKUP ON t WHERE " + where + " YIELD t.i2", index_on(field, "i8") if "i8" in where else index_on(field))
            assert [g[0] for g in got] == sorted(g[0] for g in got)      # storage order: by vid
        if n:
            last = rows[-1][0]
            only = "t.i4 == %d" % props(last)["i4"]
            got, _ = run(e, rows, "LOOKUP ON t WHERE " + only, index_on("i4"))
            assert (last,) in got
        if n >= 257:
            v = rows[256][0]
            got, _ = run(e, rows, "LOOKUP ON t WHERE t.i4 == %d YIELD t.s, t.d" % props(v)["i4"], index_on("i4"))
            assert got == [(v, props(v)["s"], props(v)["d"])]


@pytest.fixture(scope="module")
def table():
    e, rows = load(600, step=2)
    with e:
        yield e, rows


Y = " YIELD t.i1, t.i2, t.i4, t.i8, t.d, t.b, t.s"
STORAGE = [
    # every stored width as the scanned field, bounds at the column's own min / max and outside on both sides
    ("i1", "t.i1 >= -128 && t.i1 <= 127"), ("i1", "t.i1 > -128 && t.i1 < 127"), ("i1", "t.i1 < -128"), ("i1", "t.i1 > 127"),
    ("i1", "t.i1 >= -1000 && t.i1 <= 1000"), ("i1", "t.i1 == -128"), ("i1", "t.i1 > -3 && t.i1 <= 5"),
    ("i2", "t.i2 >= -32768 && t.i2 < 0"), ("i2", "t.i2 > 32767"), ("i2", "t.i2 < -32768"), ("i2", "t.i2 <= 70000"),
    ("i4", "t.i4 < 0"), ("i4", "t.i4 >= 2147483648"), ("i4", "t.i4 < -2147483648"), ("i4", "t.i4 > -5000000000"),
    ("i8", "t.i8 < 0"), ("i8", "t.i8 > %d" % I64MAX), ("i8", "t.i8 <= %d" % I64MAX), ("i8", "t.i8 >= %d" % I64MAX),
    ("i8", "t.i8 >= %d && t.i8 < %d" % (I64MIN, I64MAX)), ("i8", "t.i8 == %d" % I64MIN), ("i8", "t.i8 > %d" % (I64MAX - 1)),
    ("d", "t.d < 0.0"), ("d", "t.d >= 0.0"), ("d", "t.d == 0.0"), ("d", "t.d > -3.0 && t.d <= 1.5"), ("d", "t.d < -1000.5"),
    ("d", "t.d < 1"), ("d", "t.d >= 1"),
    ("b", "t.b == true"), ("b", "t.b == false"),
    ("s", 't.s == ""'), ("s", 't.s == "a"'), ("s", 't.s == "abcdefg"'), ("s", 't.s == "abcdefgh"'), ("s", 't.s == "abcdefghi"'),
    ("s", 't.s == "%s"' % ("x" * 300)), ("s", 't.s == "abcdefgX"'),
    # the same columns as residual terms behind a `!=` on the first field
    ("i1", "t.i1 != 0 && t.i2 < 0"), ("i1", "t.i1 != 0 && t.i4 >= 100.5"), ("i1", "t.i1 != 0 && t.i8 <= -1"),
    ("i1", "t.i1 != 0 && t.d < 0"), ("i1", "t.i1 != 0 && t.d == 0"), ("i1", "t.i1 != 0 && t.d != 1.5"),
    ("i1", "t.i1 != 0 && t.b != true"), ("i1", 't.i1 != 0 && t.s != "a"'), ("i1", 't.i1 != 0 && t.s == "abcdefghi"'),
    ("i1", "t.i1 != 0 && t.i1 < 5.5"), ("i1", "t.i1 != 0 && t.b == 1"), ("d", "t.d != 0.0"),
]


@pytest.mark.parametrize("field,where", STORAGE, ids=[w for _, w in STORAGE])
def test_storage_forms(table, field, where):
    e, rows = table
    others = [f for f, _ in FIELDS if f != field and ("t." + f + " ") in where]
    got, _ = run(e, rows, "LOOKUP ON t WHERE " + where + Y, index_on(field, *others))   # the index: exactly the fields named
    assert [g[0] for g in got] == sorted(g[0] for g in got)


def test_multi_field_prefix_and_range(table):
    e, rows = table
    _, want = run(e, rows, "LOOKUP ON t WHERE t.b == true && t.i8 == -9223372036854775808 && t.i1 >= -100 && t.i1 < 100" + Y, index_on("b", "i8", "i1"))
    assert want
    run(e, rows, "LOOKUP ON t WHERE t.i1 < 100.5 && t.b == true", index_on("b", "i1"))
    run(e, rows, "LOOKUP ON t WHERE t.i1 < 100.5 && t.b != false", index_on("b", "i1"))


def test_back_to_back_reuses_scratch(table):
    e, rows = table
    a1, _ = run(e, rows, "LOOKUP ON t WHERE t.i1 >= -128" + Y, index_on("i1"))
    b1, _ = run(e, rows, 'LOOKUP ON t WHERE t.s == "abcdefg" YIELD t.s', index_on("s"))
    a2, _ = run(e, rows, "LOOKUP ON t WHERE t.i1 >= -128" + Y, index_on("i1"))
    assert a1 == a2 and len(a1) == len(rows) and b1


def test_order_and_rows_max():
    e, rows = load(1000)
    with e:
        outs = []
        for grid in (1, 3, 0):
            e.set_flag("lookup_grid_max", grid)
            got, _ = run(e, rows, "LOOKUP ON t WHERE t.b == false YIELD t.s", index_on("b"))
            outs.append(got)
        assert outs[0] == outs[1] == outs[2] == [(v, p["s"]) for v, p in rows if not p["b"]]
        m = len(outs[0])
        e.set_flag("lookup_rows_max", m)
        assert pipeline.run(e, 1, "LOOKUP ON t WHERE t.b == false", lookup=True, indexes=index_on("b")).ok
        e.set_flag("lookup_rows_max", m - 1)
        out = pipeline.run(e, 1, "LOOKUP ON t WHERE t.b == false", lookup=True, indexes=index_on("b"))
        assert not out.ok and out.error == "lookup: %d rows, above lookup_rows_max" % m


# ----------------------------------------------------------------------------- edges
EFIELDS = [("w", INT), ("n", STRING)]


def kv_order(r, d):                                               # ranks and dsts little-endian in the key
    return (int.from_bytes((r % (1 << 64)).to_bytes(8, "little"), "big"), int.from_bytes((d % (1 << 64)).to_bytes(8, "little"), "big"))


def load_edges(degrees, wide_dst=False, ranks="const"):
    """Vertex v has degrees[v] out-edges of type e; the rows between hold none."""
    e = engine.Engine()
    e.add_space(1, 1)
    e.add_schema(1, True, 5, "e", EFIELDS)
    e.add_schema(1, False, 2, "u", [("x", INT)])
    b = kvfmt.KVBatch()
    rows = []
    nv = len(degrees)
    for v in range(nv):
        b.put(kvfmt.vertex_key(1, v, 2), kvfmt.encode_row([INT], [v]))
    for v, deg in enumerate(degrees):
        for k in range(deg):
            dst = 1000 * (v + 1) + k + ((1 << 40) if wide_dst and k % 2 else 0)     # one edge per (src, rank, dst)
            rank = 7 if ranks == "const" else k % 3 if ranks == "narrow" else (k % 3) * (1 << 40) - 5
            p = {"w": (v * 31 + k) % 200 - 100, "n": "e%d" % (k % 4)}
            b.put(kvfmt.edge_key(1, v, 5, rank, dst), kvfmt.encode_row([INT, STRING], [p["w"], p["n"]]))
            rows.append((v, dst, rank, p))
    e.load_batch(1, b)
    e.commit(1)
    return e, rows


SHAPES = {
    "alternating": [0, 1, 0, 255, 0, 0, 256, 0, 257, 0, 1, 0],
    "hub": [0, 0, 900, 0, 3, 0],
    "first_last_full": [2, 0, 0, 300, 0, 5],
}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("wide_dst,ranks", [(False, "const"), (True, "narrow"), (False, "wide")])
@pytest.mark.parametrize("grid", [1, 3, 0])
def test_edges(shape, wide_dst, ranks, grid):
    e, rows = load_edges(SHAPES[shape], wide_dst, ranks)
    idx = index_on("w", edge=True, schema="e", fields=EFIELDS)
    with e:
        e.set_flag("lookup_grid_max", grid)
        for where in ("e.w >= -100", "e.w < 0", "e.w == 5", "e.w > 1000", 'e.w != 3 && e.n == "e1"'):
            use = index_on("w", "n", edge=True, schema="e", fields=EFIELDS) if "e.n" in where else idx
            got, want = run(e, rows, "LOOKUP ON e WHERE " + where + " YIELD e.w, e.n", use)
            keyed = sorted(want, key=lambda r: (r[0],) + kv_order(r[2], r[1]))
            assert got == keyed                                   # storage order: by source row, then the KV key order
