"""ngx_fetch (FETCH PROP ON key lookup and gather in HBM) on a small hand-built space, with keys placed as a
synthetic device result (tests/devresult.py) or passed as host arrays, against plain Python dict lookups written
here (not nebula_amd/fetch.py).

The space: tags A (two schema versions: the older one lacks a_d and a_b) and B, edge types E and F with the same
(src, dst, rank) triples, one source per adjacency length 0, 1, 2, 63, 64, 65 and 1000 whose (rank, dst) pairs mix
-1, 0, 1, 255, 256, 257 so that the stored (KV key) order differs from the numeric one. Every case is a few
thousand keys at most."""
import ctypes
import itertools
import struct

import numpy as np
import pytest

from nebula_amd import engine, fetch, kvfmt, ngql, pipeline
from nebula_amd.kvfmt import BOOL, DOUBLE, INT, STRING
from tests import devresult as dr
from tests import fixtures

pytestmark = pytest.mark.gpu

SPACE, PARTS = 7, 3
TAG_A, TAG_B, EDGE_E, EDGE_F = 11, 12, 21, 22
A0 = [("a_i", INT), ("a_s", STRING)]
A1 = A0 + [("a_d", DOUBLE), ("a_b", BOOL)]
SMALL = [-1, 0, 1, 255, 256, 257]
DSTS = SMALL + [44] + list(range(1000, 1160))                     # 167 dsts x 6 ranks >= 1000 pairs
LENGTHS = [0, 1, 2, 63, 64, 65, 1000]
SRC0 = 5000                                                       # source of adjacency length LENGTHS[k]: SRC0 + k
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1025]
E_UNSUPPORTED, E_QUERY = -1002, -1003


def part(v):
    return (v % (1 << 64)) % PARTS + 1


def stored_key(rank, dst):
    """The bytes the KV key holds after (part, src, type): rank, then dst, little-endian."""
    return struct.pack("<q", rank) + struct.pack("<q", dst)


def build(ranks=SMALL, ttl=False, bad_edge=False):
    """(Dataset, tags {vid: {tag: values}}, edges {(type, src, dst, rank): (w, s)})"""
    schemas = [fixtures.SchemaDef(False, TAG_A, "A", A0, 0), fixtures.SchemaDef(False, TAG_A, "A", A1, 1),
               fixtures.SchemaDef(False, TAG_B, "B", [("b_i", INT)]),
               fixtures.SchemaDef(True, EDGE_E, "E", [("w", INT), ("s", STRING)]),
               fixtures.SchemaDef(True, EDGE_F, "F", [("w", INT), ("s", STRING)])]
    if ttl:
        schemas[2].ttl_col, schemas[2].ttl_dur = "b_i", 100
        schemas[3].ttl_col, schemas[3].ttl_dur = "w", 100
    b = kvfmt.KVBatch()
    tags, edges = {}, {}

    def tag_a(v, i, s, d, bl, ver=1):
        if ver == 1:
            b.put(kvfmt.vertex_key(part(v), v, TAG_A), kvfmt.encode_row([t for _, t in A1], [i, s, d, bl], 1))
            tags.setdefault(v, {})[TAG_A] = (i, s, d, bl)
        else:
            b.put(kvfmt.vertex_key(part(v), v, TAG_A), kvfmt.encode_row([t for _, t in A0], [i, s], 0))
            tags.setdefault(v, {})[TAG_A] = (i, s, 0.0, False)    # the fields the version lacks read as defaults

    tag_a(-5, -7, "", 1.5, True)                                  # a negative vid, an empty string
    tag_a(1, 300, "x", -0.25, False)
    tag_a(2, 1 << 40, "y" * 300, 2.0, True)
    tag_a(3, 9, "old", 0.0, False, ver=0)                         # written under the older schema version
    for v in range(10, 40):
        tag_a(v, v * 3, "s%d" % v, v / 4, v % 2 == 0)
    for v in (1, 50, 51):                                         # 1 has A and B; 50, 51 B only
        b.put(kvfmt.vertex_key(part(v), v, TAG_B), kvfmt.encode_row([INT], [v + 1000]))
        tags.setdefault(v, {})[TAG_B] = (v + 1000,)
    pairs = list(itertools.product(ranks, DSTS))
    for k, n in enumerate(LENGTHS):
        src = SRC0 + k                                            # edges, no tag
        for et in (EDGE_E, EDGE_F):
            for rank, dst in pairs[:n] if len(pairs) >= n else pairs:
                val = (rank % 1000 * 7 + dst + et, "e%d_%d" % (rank, dst))
                b.put(kvfmt.edge_key(part(src), src, et, rank, dst), kvfmt.encode_row([INT, STRING], list(val)))
                edges[(et, src, dst, rank)] = val
    if bad_edge:
        b.put(kvfmt.edge_key(part(SRC0), SRC0, EDGE_E, 0, 77), b"")   # an empty value: EF_EMPTY_VALUE
    return fixtures.Dataset(SPACE, PARTS, schemas, b), tags, edges


def load(ds, narrow=1):
    e = engine.Engine(0)
    e.set_flag("narrow_columns", narrow)
    ds.load_engine(e)
    return e


@pytest.fixture(scope="module")
def world():
    ds, tags, edges = build()
    e = load(ds)
    yield e, tags, edges, fetch.Catalog.of(PARTS, ds.schemas)
    e.close()


def vspec(tags, yields, keys=None, key_col=-1, keep_missing=False):
    names = ["VertexID"] + ["y%d" % i for i in range(len(yields))]
    return engine.FetchSpec(engine.FETCH_VERTEX, list(tags), 0, (key_col, -1, -1), keys, False, keep_missing, yields,
                            names, [0] * len(names), [], False, names)


def espec(etype, yields, keys=None, key_cols=(0, 1, 2), distinct=False):
    names = ["s", "d", "r"] + ["y%d" % i for i in range(len(yields))]
    return engine.FetchSpec(engine.FETCH_EDGE, [], etype, tuple(key_cols), keys, distinct, False, yields, names,
                            [0] * len(names), [], False, names)


A_YIELDS = [(engine.FY_TAG_PROP, TAG_A, f, 0, 0) for f, _ in A1]
AB_YIELDS = A_YIELDS + [(engine.FY_TAG_PROP, TAG_B, "b_i", 0, 0)]
E_YIELDS = [(engine.FY_EDGE_PROP, 0, "w", 0, 0), (engine.FY_EDGE_PROP, 0, "s", 0, 0)]


def expect_vertices(tags, vids, on, keep_missing, extra=None):
    """Plain lookup: a row per key that has a row of an ON tag (or every key under keep_missing)."""
    out = []
    for i, v in enumerate(vids):
        have = tags.get(int(v), {})
        if not any(t in have for t in on) and not keep_missing:
            continue
        row = [int(v)]
        for t in on:
            row += list(have.get(t, (0, "", 0.0, False) if t == TAG_A else (0,)))
        if extra is not None:
            row.append(extra[i])
        out.append(tuple(row))
    return out


def values(rows):
    return [tuple(v for _, v in r) for r in rows]


def vid_pool(n, seed):
    rng = np.random.default_rng(seed)
    pool = np.array([-5, 1, 2, 3, 50, 51, 7777, SRC0 + 3, -9] + list(range(10, 40)), dtype=np.int64)
    return pool[rng.integers(0, len(pool), n)]


@pytest.mark.parametrize("grid", [0, 1, 3])
@pytest.mark.parametrize("n", COUNTS)
def test_vertex_counts(world, n, grid):
    """Hits, misses, a negative vid, a vid with edges but no tag, A only under ON A, B: host key arrays."""
    e, tags, _, _ = world
    vids = vid_pool(n, n)
    e.set_flag("fetch_grid_max", grid)
    try:
        before = e.get_flag("fetch_device")
        r = e.fetch(SPACE, vspec([TAG_A, TAG_B], AB_YIELDS, [vids]))
        assert r.ok, r.error
        assert e.get_flag("fetch_device") == before + 1 and r.go_nrows == n
        assert values(r.rows) == expect_vertices(tags, vids, [TAG_A, TAG_B], False)
        assert r.col_types == [3, 2, 6, 5, 1, 2]
    finally:
        e.set_flag("fetch_grid_max", 0)


@pytest.mark.parametrize("width", [0, 1, 2, 4, 8])
@pytest.mark.parametrize("keep_missing", [False, True])
def test_vertex_device_keys(world, width, keep_missing):
    """Key columns of a device-resident result at every stored width and as a constant; an input column (a string)
    handed through; with keep_missing every key keeps a row of defaults."""
    e, tags, _, _ = world
    n = 257
    lim = {0: None, 1: 40, 2: 60, 4: 8000, 8: None}[width]
    vids = np.full(n, 2, np.int64) if width == 0 else np.array([v for v in vid_pool(4 * n, width) if lim is None or -100 < v < lim][:n])
    labels = [b"k%d" % i if i % 3 else b"" for i in range(len(vids))]
    res = dr.DevResult([(dr.T_STRING, 8, labels), (dr.T_VID, width, 2 if width == 0 else vids)])
    ys = A_YIELDS + [(engine.FY_INPUT_COL, 0, "", 0, 0)]
    r = e.fetch(SPACE, vspec([TAG_A], ys, None, key_col=1, keep_missing=keep_missing), result=res)
    assert r.ok, r.error
    assert values(r.rows) == expect_vertices(tags, vids, [TAG_A], keep_missing, [b.decode() for b in labels])


def test_vertex_all_miss_all_hit_repeat(world):
    e, tags, _, _ = world
    r = e.fetch(SPACE, vspec([TAG_A], A_YIELDS, [np.arange(100000, 100300, dtype=np.int64)]))
    assert r.ok and r.rows == [] and r.tags_seen == 0
    r = e.fetch(SPACE, vspec([TAG_A], A_YIELDS, [np.arange(10, 40, dtype=np.int64)]))
    assert values(r.rows) == expect_vertices(tags, range(10, 40), [TAG_A], False) and len(r.rows) == 30
    r = e.fetch(SPACE, vspec([TAG_B, TAG_A], A_YIELDS, [np.full(300, 2, np.int64)]))
    assert values(r.rows) == [(2, 1 << 40, "y" * 300, 2.0, True)] * 300 and r.tags_seen == 2
    r = e.fetch(SPACE, vspec([TAG_A], A_YIELDS, [np.array([3], dtype=np.int64)]))      # the older schema version
    assert values(r.rows) == [(3, 9, "old", 0.0, False)]


def test_eight_tags():
    """ON with the most tags the device takes: vertex v has tag k iff bit k of v is set, so every combination of
    hits occurs, the eighth tag's with and without the others; keep_missing keeps vertex 0 and an unknown vid."""
    ids = list(range(31, 39))
    schemas = [fixtures.SchemaDef(False, t, "T%d" % k, [("x", INT)]) for k, t in enumerate(ids)]
    b = kvfmt.KVBatch()
    b.put(kvfmt.vertex_key(part(0), 0, 99), kvfmt.encode_row([INT], [0]))      # vertex 0 has a row, of no ON tag
    schemas.append(fixtures.SchemaDef(False, 99, "other", [("x", INT)]))
    for v in range(1, 256):
        for k, t in enumerate(ids):
            if v >> k & 1:
                b.put(kvfmt.vertex_key(part(v), v, t), kvfmt.encode_row([INT], [v * 10 + k]))
    ys = [(engine.FY_TAG_PROP, t, "x", 0, 0) for t in ids]
    vids = np.arange(-1, 257, dtype=np.int64)
    with load(fixtures.Dataset(SPACE, PARTS, schemas, b)) as e:
        for keep_missing in (False, True):
            r = e.fetch(SPACE, vspec(ids, ys, [vids], keep_missing=keep_missing))
            assert r.ok, r.error
            want = [(int(v),) + tuple(v * 10 + k if 0 < v < 256 and v >> k & 1 else 0 for k in range(8))
                    for v in vids if keep_missing or 0 < v < 256]
            assert values(r.rows) == want and r.tags_seen == 255


def test_no_yield_column_set(world):
    """Through the pipeline: the columns of a FETCH without YIELD are those of the tags seen."""
    e, tags, _, cat = world
    out = pipeline.run(e, SPACE, "FETCH PROP ON B, A 10, 7777, 11", fetch=True, catalog=cat)
    assert out.ok and out.names == ["VertexID", "A.a_i", "A.a_s", "A.a_d", "A.a_b"]
    assert values(out.rows) == [(v,) + tags[v][TAG_A] for v in (10, 11)]
    out = pipeline.run(e, SPACE, "FETCH PROP ON B, A 50, 1", fetch=True, catalog=cat)
    assert out.names == ["VertexID", "A.a_i", "A.a_s", "A.a_d", "A.a_b", "B.b_i"]
    assert values(out.rows) == [(50, 0, "", 0.0, False, 1050), (1, 300, "x", -0.25, False, 1001)]
    assert e.get_flag("fetch_device") > 0


# ----------------------------------------------------------------------------- edges
def edge_keys(edges, etype, src, ranks, seed):
    """Keys around an adjacency: every stored edge's key, and for each a neighbour that misses (dst + 1 unless
    stored), keys below the first and above the last stored entry, a rank no edge has, a dst outside int8."""
    have = sorted(((r, d) for (t, s, d, r) in edges if t == etype and s == src), key=lambda k: stored_key(*k))
    keys = [(src, d, r) for r, d in have]
    keys += [(src, d + 1, r) for r, d in have[:50]]
    keys += [(src, -2, -1), (src, 1 << 50, 257), (src, 300, 0), (src, 44, 99), (src + 100, 0, 0), (src, 0, 1 << 40)]
    rng = np.random.default_rng(seed)
    return [keys[i] for i in rng.permutation(len(keys))]


def expect_edges(edges, etype, keys):
    return [(s, d, r) + edges[(etype, s, d, r)] for s, d, r in keys if (etype, s, d, r) in edges]


def test_stored_order_is_not_numeric():
    pairs = [(r, d) for r in SMALL for d in SMALL]
    by_bytes = sorted(pairs, key=lambda k: stored_key(*k))
    assert by_bytes != sorted(pairs)
    assert [r for r, _ in by_bytes][::6] == [0, 256, 1, 257, 255, -1]   # low byte first: 0x00.., 0x0001, 0x01, 0x0101, 0xff00, 0xff..ff


@pytest.mark.parametrize("grid", [0, 1])
@pytest.mark.parametrize("k", range(len(LENGTHS)))
def test_edge_adjacencies(world, k, grid):
    e, _, edges, _ = world
    keys = edge_keys(edges, EDGE_E, SRC0 + k, SMALL, k)
    arrays = [np.array([x[j] for x in keys], dtype=np.int64) for j in range(3)]
    e.set_flag("fetch_grid_max", grid)
    try:
        r = e.fetch(SPACE, espec(EDGE_E, E_YIELDS, arrays))
        assert r.ok, r.error
        assert values(r.rows) == expect_edges(edges, EDGE_E, keys)
        assert len(set(r.rows)) == LENGTHS[k]                     # every stored edge was found (a neighbour key may hit too)
        res = dr.DevResult([(dr.T_VID, 8, arrays[0]), (dr.T_VID, 8, arrays[1]), (dr.T_INT, 8, arrays[2])])
        r2 = e.fetch(SPACE, espec(EDGE_E, E_YIELDS, None), result=res)
        assert values(r2.rows) == values(r.rows)
    finally:
        e.set_flag("fetch_grid_max", 0)


def test_edge_two_types_key_props_duplicates(world):
    e, _, edges, _ = world
    src = SRC0 + 2
    keys = [(src, 0, -1), (src, 0, -1), (src, -1, -1), (src, 5, 5)]   # the two stored edges (one asked twice), and a miss
    arrays = [np.array([x[j] for x in keys], dtype=np.int64) for j in range(3)]
    ys = E_YIELDS + [(engine.FY_EDGE_KEY, 0, "", k, 0) for k in range(4)]
    for et in (EDGE_E, EDGE_F):
        r = e.fetch(SPACE, espec(et, ys, arrays))
        assert values(r.rows) == [x + (x[0], x[1], x[2], et) for x in expect_edges(edges, et, keys)] and len(r.rows) == 3
    # a rank column of -1: rank 0
    r = e.fetch(SPACE, espec(EDGE_E, E_YIELDS, arrays[:2] + [arrays[2]], key_cols=(0, 1, -1)))
    assert values(r.rows) == expect_edges(edges, EDGE_E, [(s, d, 0) for s, d, _ in keys])
    # DISTINCT through the pipeline: literal keys are deduplicated before they are uploaded
    cat = world[3]
    q = "FETCH PROP ON E %d->0@-1, %d->0@-1 YIELD %s E.w" % (src, src, "%s")
    assert len(pipeline.run(e, SPACE, q % "", fetch=True, catalog=cat).rows) == 2
    assert len(pipeline.run(e, SPACE, q % "DISTINCT", fetch=True, catalog=cat).rows) == 1


RANK_FORMS = {"const0": [0], "const5": [5], "int8": [-128, 127, 0], "int16": [-32768, 32767, 1], "int32": [-(1 << 31), (1 << 31) - 1, 255],
              "int64": [-(1 << 63), (1 << 63) - 1, 256, -1]}


@pytest.mark.parametrize("narrow", [1, 0])
@pytest.mark.parametrize("form", list(RANK_FORMS))
def test_rank_storage_forms(form, narrow):
    ranks = RANK_FORMS[form]
    ds, _, edges = build(ranks=ranks)
    with load(ds, narrow) as e:
        for k in (1, 3, 6):
            keys = edge_keys(edges, EDGE_E, SRC0 + k, ranks, k)
            keys += [(SRC0 + k, d, r + 1) for _, d, r in keys[:20] if r < (1 << 63) - 1]     # a rank beside the stored ones
            keys += [(SRC0 + k, 300, ranks[0]), (SRC0 + k, 44 + 256, ranks[0])]             # 300 against a column holding 44
            arrays = [np.array([x[j] for x in keys], dtype=np.int64) for j in range(3)]
            r = e.fetch(SPACE, espec(EDGE_E, E_YIELDS, arrays))
            assert r.ok, r.error
            assert values(r.rows) == expect_edges(edges, EDGE_E, keys)


def test_int8_dst_column_key_out_of_range():
    """An adjacency whose dsts fit int8 (one holds 44): a key dst of 300 (44 + 256) must miss, not wrap."""
    b = kvfmt.KVBatch()
    for d in (-3, 44, 100):
        b.put(kvfmt.edge_key(part(1), 1, EDGE_E, 0, d), kvfmt.encode_row([INT, STRING], [d, "z"]))
    ds = fixtures.Dataset(SPACE, PARTS, [fixtures.SchemaDef(True, EDGE_E, "E", [("w", INT), ("s", STRING)])], b)
    with load(ds) as e:
        keys = [np.array([1, 1, 1, 1], dtype=np.int64), np.array([300, 44, 44 - 256, -3], dtype=np.int64), np.zeros(4, np.int64)]
        r = e.fetch(SPACE, espec(EDGE_E, E_YIELDS, keys))
        assert values(r.rows) == [(1, 44, 0, 44, "z"), (1, -3, 0, -3, "z")]


# ----------------------------------------------------------------------------- refusals and the fallback
def test_refusals(world):
    e, tags, edges, cat = world
    one = [np.array([1], dtype=np.int64)]
    before = e.get_flag("fetch_device")

    def refused(spec, result=None, text="fetch:"):
        r = e.fetch(SPACE, spec, result=result)
        assert not r.ok and r.code == E_UNSUPPORTED and r.error.startswith(text), r.error
    refused(vspec([TAG_A], [(-1, 0, "", 0, 0)], one))             # a YIELD expression
    refused(vspec([], A_YIELDS[:0], one))                         # ON *
    refused(vspec([TAG_A] * 9, [], one), text="fetch: more than 8 tags")
    refused(vspec([TAG_A], A_YIELDS * 4, one), text="fetch: more than 16 columns")
    res = dr.DevResult([(dr.T_UNKNOWN, 8, [1, 2]), (dr.T_DOUBLE, 8, np.array([1.0, 2.0])), (dr.T_STRING, 8, [b"a", b"b"])])
    for col in (0, 1, 2):
        refused(vspec([TAG_A], A_YIELDS, None, key_col=col), result=res)
    res3 = dr.DevResult([(dr.T_VID, 8, np.array([1])), (dr.T_VID, 8, np.array([1])), (dr.T_INT, 8, np.array([0]))])
    refused(espec(EDGE_E, E_YIELDS, None, distinct=True), result=res3)
    r = e.fetch(SPACE, vspec([TAG_A, TAG_A], [], one))
    assert r.code == E_QUERY and r.error == "tag(A) was dup"
    r = e.fetch(SPACE, vspec([99], [], one))
    assert r.code == E_QUERY and r.error == "Unknown error(406): "
    r = e.fetch(SPACE, vspec([TAG_A], [(engine.FY_TAG_PROP, TAG_A, "nope", 0, 0)], one))
    assert r.code == E_QUERY and r.error == "`A' is not a prop of `nope'"
    r = e.fetch(SPACE, espec(EDGE_E, [(engine.FY_EDGE_PROP, 0, "nope", 0, 0)], one * 3))
    assert r.code == E_QUERY and r.error == "`nope' is not a prop of `E'"
    assert e.get_flag("fetch_device") == before
    # the pipeline falls back to the host restatement and counts it
    p = pipeline.Pipeline(e, SPACE, ["E", "F"], fetch=True, catalog=cat)
    out = p.run("FETCH PROP ON A 1, 2 YIELD A.a_i + 1 AS n")
    assert out.ok and values(out.rows) == [(1, 301), (2, (1 << 40) + 1)]
    assert p.fetch_fallbacks == 1 and p.fetch_refusal.startswith("fetch:")
    out = p.run("FETCH PROP ON * 1")
    assert out.ok and p.fetch_fallbacks == 2 and values(out.rows) == [(1, 300, "x", -0.25, False, 1001)]
    assert e.get_flag("fetch_device") == before


def test_refusals_through_the_pipeline(world):
    """Refusals that only a sentence's shape or its input decides, through Pipeline.run: each is counted once and the
    sentence is answered all the same."""
    e, tags, edges, cat = world
    before = e.get_flag("fetch_device")
    # an UNKNOWN-typed key column (an arithmetic YIELD of the GO): refused in HBM, answered once the rows are delivered
    p = pipeline.Pipeline(e, SPACE, ["E", "F"], fetch=True)
    out = p.run("GO FROM %d OVER E YIELD E.w - E.w + 10 AS id | FETCH PROP ON A $-.id YIELD A.a_i, A.a_s" % (SRC0 + 2))
    assert out.ok, out.error
    assert values(out.rows) == [(10, 30, "s10")] * 2
    assert p.fetch_fallbacks == 1 and p.fetch_refusal == "fetch: UNKNOWN-typed column (per-row value types)"
    # a string key column: the host path words the reference's error
    p = pipeline.Pipeline(e, SPACE, ["E", "F"], fetch=True)
    out = p.run("GO FROM %d OVER E YIELD E.s AS id | FETCH PROP ON A $-.id" % (SRC0 + 2))
    assert not out.ok and out.error == "Column `id' not found"
    assert p.fetch_fallbacks == 1 and p.fetch_refusal == "fetch: a non-integer key column"
    # more than 16 output columns
    p = pipeline.Pipeline(e, SPACE, ["E", "F"], fetch=True)
    out = p.run("FETCH PROP ON A 1 YIELD " + ", ".join(["A.a_i"] * 16))
    assert out.ok and values(out.rows) == [(1,) + (300,) * 16]
    assert p.fetch_fallbacks == 1 and p.fetch_refusal == "fetch: more than 16 columns"
    # DISTINCT over edge keys that are still in HBM: refused once, then the delivered keys go up deduplicated
    p = pipeline.Pipeline(e, SPACE, ["E", "F"], fetch=True)
    q = "GO FROM %d, %d OVER E YIELD E._src AS s, E._dst AS d, E._rank AS r | FETCH PROP ON F $-.s->$-.d@$-.r YIELD DISTINCT F.w"
    out = p.run(q % (SRC0 + 2, SRC0 + 1))
    assert out.ok and sorted(values(out.rows)) == sorted(
        (s_, d, r, w) for (t, s_, d, r), (w, _) in edges.items() if t == EDGE_F and s_ in (SRC0 + 1, SRC0 + 2))
    assert p.fetch_fallbacks == 1 and p.fetch_refusal == "fetch: DISTINCT over device-resident edge keys"
    # after a refusal of `GO | FETCH` the GO is delivered and the FETCH is tried again over the host keys: that call
    # ran for the first and the last sentence (integers by then, deduplicated by then), not for the other two
    assert e.get_flag("fetch_device") == before + 2


def test_two_to_the_31_keys_refused(world):
    """A result of 2^31 rows is refused from its row count alone, before any column is read or anything launched."""
    e = world[0]
    res = dr.DevResult([(dr.T_VID, 8, np.array([1, 2])), (dr.T_VID, 8, np.array([1, 2])), (dr.T_INT, 8, np.array([0, 0]))])
    res.struct.nrows = 1 << 31
    before = e.get_flag("fetch_device")
    for spec in (vspec([TAG_A], A_YIELDS, None, key_col=0), espec(EDGE_E, E_YIELDS, None)):
        r = e.fetch(SPACE, spec, result=res)
        assert not r.ok and r.code == E_UNSUPPORTED and r.error == "fetch: 2^31 keys or more"
    assert e.get_flag("fetch_device") == before


def test_world_2_is_refused():
    """A shard of a two-shard world: the keys would have to go to their owners (a later step). Both entry points
    refuse, and the pipeline answers through the host restatement."""
    def fn(user, op, send, recv, nbytes):
        if op == engine.XCHG_ALLGATHER:                           # commit: the peer (rank 1) holds no vertices
            ctypes.memmove(recv, send, nbytes)
            ctypes.memset(recv + nbytes, 0, nbytes)
            return 0
        return 1

    cb = engine.ExchangeFn(fn)
    ds, tags, edges = build()
    e = engine.Engine(0, 0, 2, exchange=cb)
    try:
        ds.load_engine(e)
        r = e.fetch(SPACE, vspec([TAG_A], A_YIELDS, [np.array([1], dtype=np.int64)]))
        assert not r.ok and r.code == E_UNSUPPORTED and r.error.startswith("fetch: world > 1")
        go = "GO FROM %d OVER E YIELD E._src AS s, E._dst AS d, E._rank AS r" % (SRC0 + 2)   # one hop: no exchange
        r = e.go_fetch(SPACE, go, espec(EDGE_F, E_YIELDS, None))
        assert not r.ok and r.code == E_UNSUPPORTED and r.error.startswith("fetch: world > 1")
        assert e.get_flag("fetch_device") == 0
    finally:
        e.close()


def test_refusals_of_the_space():
    """A TTL schema and a slot with an empty-valued edge are refused before any launch; the host path answers."""
    ds, tags, edges = build(ttl=True, bad_edge=True)
    with load(ds) as e:
        cat = fetch.Catalog.of(PARTS, ds.schemas)
        one = [np.array([50], dtype=np.int64)]
        r = e.fetch(SPACE, vspec([TAG_B], [], one))
        assert r.code == E_UNSUPPORTED and r.error == "fetch: a TTL tag schema"
        r = e.fetch(SPACE, espec(EDGE_E, E_YIELDS, [np.array([SRC0 + 1]), np.array([-1]), np.array([-1])]))
        assert r.code == E_UNSUPPORTED and r.error == "fetch: a TTL edge schema"
        r = e.fetch(SPACE, espec(EDGE_F, E_YIELDS, [np.array([SRC0 + 1]), np.array([-1]), np.array([-1])]))
        assert r.ok and values(r.rows) == [(SRC0 + 1, -1, -1) + edges[(EDGE_F, SRC0 + 1, -1, -1)]]
        # through the pipeline: the host restatement answers with the backend's TTL (b_i = 1050, 1051; duration 100)
        before = e.get_flag("fetch_device")
        for now, want in ((1100, [(50, 1050), (51, 1051)]), (1151, [(51, 1051)]), (5000, [])):
            p = pipeline.Pipeline(e, SPACE, ["E", "F"], fetch=True, now_sec=now)
            out = p.run("FETCH PROP ON B 50, 51, 7777 YIELD B.b_i")
            assert out.ok, out.error
            assert values(out.rows) == want
            assert p.fetch_fallbacks == 1 and p.fetch_refusal == "fetch: a TTL tag schema"
        assert e.get_flag("fetch_device") == before
    ds, tags, edges = build(bad_edge=True)
    with load(ds) as e:
        r = e.fetch(SPACE, espec(EDGE_E, E_YIELDS, [np.array([SRC0 + 1]), np.array([-1]), np.array([-1])]))
        assert r.code == E_UNSUPPORTED and r.error == "fetch: edges with empty or unreadable values"
        cat = fetch.Catalog.of(PARTS, ds.schemas)
        p = pipeline.Pipeline(e, SPACE, ["E", "F"], fetch=True, catalog=cat)
        out = p.run("FETCH PROP ON E %d->-1@-1" % (SRC0 + 1))
        assert out.ok and p.fetch_fallbacks == 1
        assert values(out.rows) == [(SRC0 + 1, -1, -1) + edges[(EDGE_E, SRC0 + 1, -1, -1)]]


def test_calls_around_a_go(world):
    """Two calls and a GO between them on one Engine: the same rows."""
    e, tags, edges, _ = world
    vids = vid_pool(300, 5)
    spec = vspec([TAG_A, TAG_B], AB_YIELDS, [vids])
    first = e.fetch(SPACE, spec)
    go = e.go(SPACE, "GO FROM %d OVER E YIELD E._dst AS d, E._rank AS r, E.w AS w" % (SRC0 + 4))
    assert go.ok and len(go.rows) == 64
    second = e.fetch(SPACE, spec)
    assert first.rows == second.rows and values(first.rows) == expect_vertices(tags, vids, [TAG_A, TAG_B], False)
    # GO | FETCH in one device call, both kinds
    cat = world[3]
    p = pipeline.Pipeline(e, SPACE, ["E", "F"], fetch=True, catalog=cat)
    before = e.get_flag("fetch_device")
    out = p.run("GO FROM %d OVER E YIELD E._src AS s, E._dst AS d, E._rank AS r | FETCH PROP ON F $-.s->$-.d@$-.r YIELD F.w" % (SRC0 + 5))
    assert out.ok and e.get_flag("fetch_device") == before + 1
    want = sorted((s, d, r, w) for (t, s, d, r), (w, _) in edges.items() if t == EDGE_F and s == SRC0 + 5)
    assert sorted(values(out.rows)) == want and len(want) == 65
