"""A model of GO that shares nothing with the code under test, the shaped graphs it is run on, and the loaders the
tests put those graphs into an Engine and into the oracle with.

The model is plain Python over an edge list `(src vid, dst vid, type, rank, (p0, p1, b))` plus optional tag rows
`{vid: x}`. It restates GoExecutor's rules (src/graph/GoExecutor.cpp of the reference):
  * an edge `a -> b` of type t and rank r is stored twice: the out row `(a, +t, r, b)` and the in row `(b, -t, r, a)`,
    both with the edge's properties. FORWARD a hop scans the `+t` rows of its frontier for every OVER type t,
    REVERSELY the `-t` rows, BIDIRECT both (stepOut, getStepOutProps);
  * the seeds are the FROM list as written: a vid listed twice is scanned twice, a vid without rows scans nothing; only
    YIELD DISTINCT makes the list a set (execute, :123-129);
  * a hop's next frontier is the set of the `dst` fields of the rows it scanned, whatever WHERE says
    (getDstIdsFromRespWithBackTrack); an empty next frontier ends the query (no further hop is counted);
  * `GO M TO N STEPS` records hops M .. N (plain `N STEPS`: hop N only); WHERE and YIELD are evaluated for the rows
    of the record hops only (processFinalResult);
  * for a scanned row `(v, s, r, w)`: `_src` is v, `_dst` is w, `_rank` is r, `_type` is the stored signed type s
    (so REVERSELY `_src` is the edge's destination and `_type` is negative);
  * with more than one OVER type, `x._dst` of a row of another type is 0, and every other `x.prop` of it is the
    column type's default, 0 for integers (getEdgeDstId, getAliasProp);
  * a pushed-down WHERE: FORWARD, on the last hop, storage evaluates the WHERE first, and there an alias of another
    type than the row's is an error that drops the row (QueryBaseProcessor.inl:539-601 of the reference: "Ignore this
    edge"), so with several OVER types only the rows of the type the WHERE names survive; REVERSELY, BIDIRECT, on earlier
    record hops and with pushdown off graphd alone evaluates it, with the defaults above;
  * `$^.t.x` / `$$.t.x` of a vertex without the tag is the default, 0, where graphd evaluates them (getSrcTagProp,
    getDstTagProp). That is the whole rule only for the one form here that reads tags: its YIELD reads no edge property
    but `_dst`, so the storage request is structure-only and storage never evaluates the pushed WHERE
    (QueryBaseProcessor.inl:520). With an edge property in the YIELD, a pushed WHERE that reads `$^.t.x` fails in
    storage for a source without the tag row ("Invalid Tag Filter", .inl:582-596) and drops the edge: the model does
    NOT restate that, so a new form of that kind needs the rule added first (the host test would show the difference).
The model parses and evaluates no nGQL: each query form of FORMS pairs the text with Python callables.

Cells are `(kind, value)` as the engine and the oracle hand them out: "id" for `_src` / `_dst`, "int" for `_rank`,
`_type` and INT properties.
"""
import random
import struct
from collections import namedtuple

import numpy as np

from nebula_amd import kvfmt
from tests import fixtures

# ----------------------------------------------------------------------------- constants of the kernels under test
# Mirrored from nebula_amd/csrc (tests/test_goref_host.py asserts each against the header it is named in, so a change
# of a constant moves the tests).
K_SEED_FUSE_MAX = 4096          # kernels.h   kSeedFuseMax
K_CHUNK = 2048                  # kargs.h     kChunk
K_WG = 256                      # final_kernels.h WG
K_SPARSE_SUB = K_CHUNK // K_WG  # kernels.hip kSparseSub = CE / WG (CE = kChunk): 8 slices of 256 edges
K_PULL_K = 16                   # kernels.h   kPullK
K_PULL_WINDOW = 2048            # kernels.h   kPullWindow
K_PULL_SEG = 1024               # kernels.h   kPullSeg
K_PULL_MAX_SLOTS = 4            # kernels.h   kPullMaxSlots
K_COMPACT_TILE = 4096           # kernels.h   kCompactTile
K_RESV_SHIFT = 16               # kargs.h     kResvShift
K_RESV_GROUPS = 8               # kargs.h     kResvGroups
K_XCHG_BLOCK = 256              # kernels.h   kXchgBlock (k_pack / k_merge rows per workgroup)
K_LIST_THREADS = 1024           # kernels.h   kListThreads (k_pack_list)
K_LIST_TILE = 4096              # kernels.h   kListTile (k_pack_list rows per workgroup)
K_XCHG_LIST_FACTOR = 32         # kernels.h   kXchgListFactor (lists iff 32 * E of the busiest shard < smallest shard)
K_MAX_WORLD = 64                # kernels.h   kMaxWorld
K_ROOT_BATCH = 64               # kernels.h   kRootBatch (roots of one multi-root walk: one bit of a row's set each)
K_TILE = 4096                   # kargs.h     kTile (the degree scan's tile, over a record hop's (row, input row) entries)
CONSTANTS = {
    "kernels.h": {"kSeedFuseMax": K_SEED_FUSE_MAX, "kPullK": K_PULL_K, "kPullWindow": K_PULL_WINDOW,
                  "kPullSeg": K_PULL_SEG, "kPullMaxSlots": K_PULL_MAX_SLOTS, "kCompactTile": K_COMPACT_TILE,
                  "kXchgBlock": K_XCHG_BLOCK, "kListThreads": K_LIST_THREADS, "kListTile": K_LIST_TILE,
                  "kXchgListFactor": K_XCHG_LIST_FACTOR, "kMaxWorld": K_MAX_WORLD, "kRootBatch": K_ROOT_BATCH},
    "kargs.h": {"kChunk": K_CHUNK, "kResvShift": K_RESV_SHIFT, "kResvGroups": K_RESV_GROUPS, "kTile": K_TILE},
    "final_kernels.h": {"WG": K_WG},
}

TYPE_OF = {"e": 1, "f": 2, "g": 3, "h": 4, "i": 5}
NAME_OF = {t: n for n, t in TYPE_OF.items()}
EDGE_FIELDS = [("p0", kvfmt.INT), ("p1", kvfmt.INT), ("b", kvfmt.INT)]
TAG_ID = 11
SCHEMA = [fixtures.SchemaDef(True, t, n, EDGE_FIELDS) for n, t in TYPE_OF.items()] + \
         [fixtures.SchemaDef(False, TAG_ID, "t", [("x", kvfmt.INT)])]
FORWARD, REVERSELY, BIDIRECT = 0, 1, 2
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


def default_props(a, b, t, r):
    """(p0 in 0 .. 99, p1 over the 62-bit range, b in -100 .. 99) from a hash of the edge's key."""
    h = (a * 2654435761 + b * 40503 + t * 97 + r * 31 + 17) & 0xFFFFFFFFFFFF
    return (h % 100, (h * 6364136223846793005 + 1442695040888963407) % (1 << 62) - (1 << 61), (h >> 9) % 200 - 100)


def edge(a, b, t=1, r=0, props=None):
    return (a, b, t, r, tuple(props) if props is not None else default_props(a, b, t, r))


class Graph:
    """vids: the vertex table (every endpoint of an edge is in it); edges: `edge()` tuples, no (src, dst, type, rank)
    twice; types: the edge types that get a slot pair (default: those with an edge); tags: {vid: x} or None."""

    def __init__(self, vids, edges, types=None, tags=None):
        self.vids = sorted(set(vids))
        self.edges = list(edges)
        self.types = sorted(types if types is not None else {x[2] for x in self.edges})
        self.tags = tags
        have = set(self.vids)
        keys = set()
        for a, b, t, r, _ in self.edges:
            assert a in have and b in have and t in self.types, (a, b, t)
            assert (a, b, t, r) not in keys, ("an edge twice", a, b, t, r)
            keys.add((a, b, t, r))
        self._rows = None

    def rows(self):
        """{(vertex, signed type): [(rank, other end, props)]}: the stored rows."""
        if self._rows is None:
            rows = {}
            for a, b, t, r, p in self.edges:
                rows.setdefault((a, t), []).append((r, b, p))
                rows.setdefault((b, -t), []).append((r, a, p))
            self._rows = rows
        return self._rows

    def out_degree(self, v, types):
        return sum(len(self.rows().get((v, t), ())) for t in types)


# ----------------------------------------------------------------------------- the model
Row = namedtuple("Row", "src dst st rank props g")           # one scanned row, st its stored signed type
Model = namedtuple("Model", "rows hop_edges hop_frontier")


def go(graph, seeds, over, direction, m, n, where, yields, distinct=False, pushed_type=None):
    """GO m TO n STEPS FROM seeds OVER over (type ids) in `direction`; where: Row -> bool or None; yields: one
    callable Row -> cell per column; pushed_type: the type of the alias a pushed-down WHERE reads (None: not pushed). Returns Model(rows as a list of cell tuples, hop_edges, hop_frontier)."""
    stored = graph.rows()
    scan = {FORWARD: list(over), REVERSELY: [-t for t in over], BIDIRECT: list(over) + [-t for t in over]}[direction]
    frontier = list(seeds)
    if distinct:
        frontier = list(dict.fromkeys(frontier))
    out, hop_edges, hop_frontier, seen = [], [], [], set()
    for hop in range(1, n + 1):
        hop_frontier.append(len(frontier))
        scanned = [Row(v, w, st, r, p, graph) for v in frontier for st in scan for r, w, p in stored.get((v, st), ())]
        hop_edges.append(len(scanned))
        if hop >= m:
            for row in scanned:
                if pushed_type is not None and direction == FORWARD and hop == n and abs(row.st) != pushed_type:
                    continue
                if where is not None and not where(row):
                    continue
                cells = tuple(y(row) for y in yields)
                if distinct:
                    if cells in seen:
                        continue
                    seen.add(cells)
                out.append(cells)
        frontier = list({row.dst for row in scanned})
        if not frontier:
            break
    return Model(out, hop_edges, hop_frontier)


def _of(row, t, name):
    """`alias.name` where the alias is edge type t."""
    if abs(row.st) != t:
        return 0
    if name == "_src":
        return row.src
    if name == "_dst":
        return row.dst
    if name == "_rank":
        return row.rank
    if name == "_type":
        return row.st
    return row.props[("p0", "p1", "b").index(name)]


def _cmod(a, b):
    """C++ `%`: the quotient truncates towards zero."""
    q = abs(a) // abs(b)
    if (a < 0) != (b < 0):
        q = -q
    return a - q * b


def _tag(row, vid):
    return (row.g.tags or {}).get(vid, 0)


def _col(kind, name, k=0):
    return lambda over: (lambda row: (kind, _of(row, over[k], name)))


# A form: the text after `OVER ... [direction]` with {a} / {b} for the first / second OVER alias, the predicate and the
# YIELD columns as functions of the OVER type ids, DISTINCT, and how many OVER types it needs at least.
# where_alias: the OVER alias an edge-reading WHERE names (what a pushed-down filter keeps), None if it reads no edge.
Form = namedtuple("Form", "name tail where yields distinct min_over tags where_alias")
FORMS = {f.name: f for f in [
    Form("bench", "WHERE {a}.p0 < 50 YIELD {a}._dst, {a}._rank, {a}.p0, {a}.p1",
         lambda over: (lambda row: _of(row, over[0], "p0") < 50),
         [_col("id", "_dst"), _col("int", "_rank"), _col("int", "p0"), _col("int", "p1")], False, 1, False, 0),
    Form("all", "YIELD {a}._dst, {a}.p1", None, [_col("id", "_dst"), _col("int", "p1")], False, 1, False, None),
    Form("keys", "YIELD {a}._src, {a}._dst, {a}._type, {a}._rank", None,
         [_col("id", "_src"), _col("id", "_dst"), _col("int", "_type"), _col("int", "_rank")], False, 1, False, None),
    Form("mod", "WHERE {a}.p1 % 7 == 1 YIELD {a}._dst, {a}.p1",
         lambda over: (lambda row: _cmod(_of(row, over[0], "p1"), 7) == 1),
         [_col("id", "_dst"), _col("int", "p1")], False, 1, False, 0),
    Form("signed", "WHERE {a}.b < 0 YIELD {a}._dst, {a}.b",
         lambda over: (lambda row: _of(row, over[0], "b") < 0),
         [_col("id", "_dst"), _col("int", "b")], False, 1, False, 0),
    Form("distinct", "YIELD DISTINCT {a}._dst", None, [_col("id", "_dst")], True, 1, False, None),
    Form("tags", "WHERE $^.t.x >= 0 YIELD {a}._dst, $^.t.x, $$.t.x",
         lambda over: (lambda row: _tag(row, row.src) >= 0),
         [_col("id", "_dst"), lambda over: (lambda row: ("int", _tag(row, row.src))),
          lambda over: (lambda row: ("int", _tag(row, row.dst)))], False, 1, True, None),
    Form("multi", "WHERE {a}.b < 50 YIELD {a}._dst, {b}._dst, {a}._rank, {b}._rank, {a}.b, {b}.b",
         lambda over: (lambda row: _of(row, over[0], "b") < 50),
         [_col("id", "_dst"), _col("id", "_dst", 1), _col("int", "_rank"), _col("int", "_rank", 1), _col("int", "b"),
          _col("int", "b", 1)], False, 2, False, 0),
    Form("multi_all", "YIELD {a}._dst, {b}._dst, {a}._rank, {b}._rank, {a}.b, {b}.b", None,
         [_col("id", "_dst"), _col("id", "_dst", 1), _col("int", "_rank"), _col("int", "_rank", 1), _col("int", "b"),
          _col("int", "b", 1)], False, 2, False, None),
]}
_DIR = {FORWARD: "", REVERSELY: " REVERSELY", BIDIRECT: " BIDIRECT"}
KIND_TYPE = {"id": kvfmt.VID, "int": kvfmt.INT}


def sentence(form, seeds, over, direction=FORWARD, m=None, n=1):
    """The nGQL text of a form; over: edge names."""
    f = FORMS[form]
    assert len(over) >= f.min_over
    steps = "%d STEPS" % n if m is None else "%d TO %d STEPS" % (m, n)
    tail = f.tail.replace("{a}", over[0]).replace("{b}", over[1] if len(over) > 1 else over[0])
    return "GO %s FROM %s OVER %s%s %s" % (steps, ", ".join(str(int(v)) for v in seeds), ", ".join(over), _DIR[direction], tail)


def model(graph, form, seeds, over, direction=FORWARD, m=None, n=1, pushdown=True):
    f = FORMS[form]
    types = [TYPE_OF[x] for x in over]
    return go(graph, seeds, types, direction, n if m is None else m, n, f.where(types) if f.where else None,
              [y(types) for y in f.yields], f.distinct,
              types[f.where_alias] if pushdown and f.where_alias is not None else None)


def column_kinds(form):
    return [y([1, 2])(Row(0, 0, 1, 0, (0, 0, 0), Graph([0], [])))[0] for y in FORMS[form].yields]


# ----------------------------------------------------------------------------- the comparator
def typed_cell(k, v):
    """A cell as the comparator sees it: a string exactly, a double by its bits, everything else as an integer."""
    if k == "str":
        assert isinstance(v, str), (k, v)
        return (k, v)
    if k in ("double", "float"):
        return (k, struct.unpack("<q", struct.pack("<d", v))[0])
    return (k, int(v))


def typed_rows(rows):
    return sorted(tuple(typed_cell(k, v) for k, v in r) for r in rows)


def assert_same(got, want, what=""):
    """got: an engine or oracle GoResult (or a Model); want: the Model. Sorted typed rows, the edges scanned per hop
    and the frontier per hop, all exact."""
    assert getattr(got, "ok", True), (what, getattr(got, "error", ""))
    edges = got.hop_edges if hasattr(got, "hop_edges") else got.hop_scanned
    assert [int(x) for x in edges] == list(want.hop_edges), (what, "hop_edges", list(edges), want.hop_edges)
    assert [int(x) for x in got.hop_frontier] == list(want.hop_frontier), (what, "hop_frontier", list(got.hop_frontier),
                                                                           want.hop_frontier)
    assert_rows(got.rows, want.rows, what)


def assert_rows(got, want, what=""):
    """Two lists of rows of typed cells are the same multiset."""
    a, b = typed_rows(got), typed_rows(want)
    if a != b:
        sa, sb = set(a), set(b)
        raise AssertionError((what, "rows", len(a), len(b), sorted(sa - sb)[:3], sorted(sb - sa)[:3]))


def columns(want, ncol):
    """The model's rows as int64 columns (for oracle.row_digest and for compact device results)."""
    return [np.array([r[c][1] for r in want.rows], dtype=np.int64) for c in range(ncol)]


# ----------------------------------------------------------------------------- loaders
def _key(x):
    return (x & (1 << 64) - 1).to_bytes(8, "little")


_space = [300]


def new_space():
    _space[0] += 1
    return _space[0]


def part_of(vid, num_parts):
    """ID_HASH: the part of a vid (the vid as an unsigned 64-bit number)."""
    return (vid & (1 << 64) - 1) % num_parts + 1


def shard_of(vid, num_parts, world):
    """The engine's placement: part = vid mod num_parts + 1, shard = part % world."""
    return part_of(vid, num_parts) % world


def shard_tables(graph, num_parts, world, vids=None):
    """(tables, shardBase): each shard's vertex list ordered by (part, vid), and the global row of each shard's first
    row (world + 1 entries; global rows are the tables concatenated in rank order). vids: the vertices that have a row
    (default: all of graph.vids, as ngx_load_csr is given them)."""
    tables = [[] for _ in range(world)]
    for v in sorted(graph.vids if vids is None else vids, key=lambda v: (part_of(v, num_parts), v)):
        tables[shard_of(v, num_parts, world)].append(v)
    base = [0]
    for t in tables:
        base.append(base[-1] + len(t))
    return tables, base


def kv_vertices(graph):
    """The vertices a KV load knows: those with an out row, an in row or a tag row."""
    have = set(graph.tags or {})
    for a, b, _, _, _ in graph.edges:
        have.add(a)
        have.add(b)
    return sorted(have)


def csr_slots(graph, rank=None, world=1, num_parts=1):
    """ngx_load_csr's arrays of a Graph: (vpart, vid, slots), a slot pair (+t, -t) per type of graph.types, the rows'
    edges in key order (rank, then dst, by their little-endian bytes). With a rank: that shard's rows only (the out slot
    their out-edges, the in slot their in-edges; dst holds vids of any shard) and their parts."""
    if rank is None:
        vids, vpart = graph.vids, np.ones(len(graph.vids), np.int32)
    else:
        vids = shard_tables(graph, num_parts, world)[0][rank]
        vpart = np.array([part_of(v, num_parts) for v in vids], np.int32)
    row = {v: i for i, v in enumerate(vids)}
    nv = len(vids)
    slots = []
    for t in graph.types:
        for sign in (1, -1):
            lists = [[] for _ in range(nv)]
            for a, b, tt, r, p in graph.edges:
                if tt == t and (a if sign > 0 else b) in row:
                    lists[row[a] if sign > 0 else row[b]].append((r, b if sign > 0 else a, p))
            off, dst, rank, cols = [0], [], [], ([], [], [])
            for lst in lists:
                for r, d, p in sorted(lst, key=lambda x: (_key(x[0]), _key(x[1]))):
                    dst.append(d)
                    rank.append(r)
                    for k in range(3):
                        cols[k].append(p[k])
                off.append(len(dst))
            slots.append((sign * t, np.array(off, np.uint64), np.array(dst, np.int64), [np.array(c, np.int64) for c in cols],
                          np.array(rank, np.int64)))
    return vpart, np.array(vids, np.int64), slots


def load_engine_csr(e, graph, space=None, arrays=None, num_parts=1):
    """The graph through ngx_load_csr (exact layout, exact mirrors, one part, no tag rows). Returns the space."""
    space = space or new_space()
    e.add_space(space, num_parts)
    for s in SCHEMA:
        e.add_schema(space, s.is_edge, s.sid, s.name, s.fields)
    e.load_csr(space, *(arrays or csr_slots(graph)))
    e.commit(space)
    return space


def kv_batch(graph, num_parts=1):
    """Every row of the graph, each key with the part of the vertex it is stored under (ngx_load_kv keeps the rows of
    its shard's parts)."""
    b = kvfmt.KVBatch()
    types = [t for _, t in EDGE_FIELDS]
    for a, d, t, r, p in graph.edges:
        row = kvfmt.encode_row(types, list(p))
        b.put(kvfmt.edge_key(part_of(a, num_parts), a, t, r, d), row)
        b.put(kvfmt.edge_key(part_of(d, num_parts), d, -t, r, a), row)
    for v, x in sorted((graph.tags or {}).items()):
        b.put(kvfmt.vertex_key(part_of(v, num_parts), v, TAG_ID), kvfmt.encode_row([kvfmt.INT], [x]))
    return b


def dataset(graph, space=None, num_parts=1):
    return fixtures.Dataset(space or new_space(), num_parts, SCHEMA, kv_batch(graph, num_parts))


def load_engine_kv(e, graph, space=None, num_parts=1):
    """The graph as KV rows (out and in row per edge, a tag row per entry of graph.tags). Returns the space."""
    ds = dataset(graph, space, num_parts)
    ds.load_engine(e)
    return ds.space


def load_oracle(o, graph, space=None, num_parts=1):
    ds = dataset(graph, space, num_parts)
    ds.load_oracle(o)
    return ds.space


# ----------------------------------------------------------------------------- shaped graphs
# Every generator returns (Graph, seeds). Unless said otherwise row r of the vertex table is vid r + 1 and the
# traversal is `GO 2 STEPS`: the seeds' out-edges (hop 1) select the frontier the hop under test expands.
def fan(frontier_rows, adj, nv, types=None, tags=None, extra=()):
    """Vertex nv + 1 (the seed, the last row) points over type 1 at `frontier_rows`; adj: {row: [(dst row, type, rank)
    or dst row]} the edges of the hop under test."""
    edges = [edge(nv + 1, r + 1, 1, 0) for r in sorted(set(frontier_rows))]
    for r, lst in adj.items():
        for x in lst:
            d, t, rk = x if isinstance(x, tuple) else (x, 1, 0)
            edges.append(edge(r + 1, d + 1, t, rk))
    edges += list(extra)
    return Graph(range(1, nv + 2), edges, types=types, tags=tags), [nv + 1]


def frontier_edges(n, seed=0):
    """A hop-2 frontier with exactly n edges: degrees drawn from {0, 1, 2, 3, 7, 19, 64, 300} until n are placed,
    the destinations spread over the rows; every row with edges is in the frontier, as are some without."""
    rnd = random.Random(1000 + n + seed)
    nv = max(n // 3, 8) + 40
    adj, left, r = {}, n, 0
    while left:
        d = min(left, rnd.choice([0, 0, 1, 2, 3, 7, 19, 64, 300]), nv)
        if d:
            adj[r] = rnd.sample(range(nv), d)
        left -= d
        r += 1
        assert r < nv
    g, seeds = fan(list(range(r)) + [nv - 1], adj, nv)
    assert sum(len(a) for a in adj.values()) == n
    return g, seeds


def supernode_midchunk():
    """Rows 0 .. 9 of degree 1, row 10 of degree 5000 (frontier positions 10 .. 5009: it starts mid-chunk and covers
    chunks 0, 1 and 2), rows 11 .. 20 of degree 1; all of them in the frontier."""
    nv = 5200
    adj = {r: [(r * 37) % 5000 + 21] for r in list(range(10)) + list(range(11, 21))}
    adj[10] = list(range(100, 5100))
    return fan(range(21), adj, nv)


def sparse_rows():
    """Degree-1 rows with runs of degree-0 rows between them: 703 entries (more than 256) share chunk 0 with a row of
    degree K_CHUNK - 351 = 1697, and a run of 300 degree-0 frontier rows straddles the boundary of chunks 0 and 1
    (positions 2047 | 2048 belong to the rows before and after the run). Both are asserted from the chunk map."""
    nv = 4000
    adj, r, pos = {}, 0, 0
    rnd = random.Random(3)
    for k in range(350):                                          # 350 degree-1 rows, each followed by a degree-0 row
        adj[r] = [rnd.randrange(nv)]
        r += 2
        pos += 1
    adj[r] = rnd.sample(range(nv), K_CHUNK - pos - 1)             # fills chunk 0 up to position 2046
    r += 1
    adj[r] = [rnd.randrange(nv)]                                  # position 2047, the last of chunk 0
    r += 301                                                      # the run of 300 empty rows
    adj[r] = [rnd.randrange(nv)]                                  # position 2048, the first of chunk 1
    r += 1
    for k in range(300):
        adj[r] = [rnd.randrange(nv)]
        r += 1 + k % 3
    assert r < nv
    g, seeds = fan(range(r), adj, nv)
    ends = chunk_ends(g, list(range(1, r + 1)), [1])
    (b0, _), (e0, _) = ends[0]
    (b1, _), _ = ends[1]
    assert b0 == 0 and e0 - b0 + 1 > 256 and b1 - e0 == 301, ends[:2]   # 703 entries in chunk 0; 300 empty rows between
    assert all(i not in adj for i in range(e0 + 1, b1)) and len(adj[700]) == K_CHUNK - 351
    return g, seeds


def chunk_ends(graph, frontier, over):
    """The chunk map of a hop over `frontier` (vids in row order): per K_CHUNK chunk of the hop's edges, the (frontier
    index, slot) of its first and of its last edge; the entries run vertex by vertex, slot by slot."""
    ends, pos = [], 0
    owner = []                                                    # (first position, count, index, slot) per entry
    for i, v in enumerate(frontier):
        for k, t in enumerate(over):
            n = len(graph.rows().get((v, t), ()))
            if n:
                owner.append((pos, n, i, k))
            pos += n
    at = 0
    for c in range((pos + K_CHUNK - 1) // K_CHUNK):
        lo, hi = c * K_CHUNK, min(pos, (c + 1) * K_CHUNK) - 1
        while owner[at][0] + owner[at][1] <= lo:
            at += 1
        j = at
        while owner[j][0] + owner[j][1] <= hi:
            j += 1
        ends.append((owner[at][2:], owner[j][2:]))
    return ends


SLOT_DEGREES = ((1, 500), (2, 700), (3, 300))


def interleaved_slots(empty_type=None):
    """Three OVER types (e, f, g) whose per-vertex entries interleave: each of 8 frontier rows has 500 edges of e, 700 of
    f and 300 of g (1500 a row), so the chunk boundaries fall in different slots: chunk 2 (positions 4096 .. 6143) begins
    in slot f (slot 1) of row 2 and ends in slot e (slot 0) of row 4, which is asserted here from the chunk map. With
    empty_type that type has a slot pair and no edge at all (the other slots' boundaries move; nothing is asserted of
    them)."""
    nv = 800
    rnd = random.Random(11)
    adj = {}
    for r in range(8):
        lst = []
        for t, n in SLOT_DEGREES:
            if t != empty_type:
                lst += [(d, t, 0) for d in rnd.sample(range(nv), n)]
        adj[r] = lst
    g, seeds = fan(range(8), adj, nv, types=[1, 2, 3])
    if empty_type is None:
        ends = chunk_ends(g, list(range(1, 9)), [1, 2, 3])
        assert ends[2] == ((2, 1), (4, 0)), ends                  # begins in slot 1 of one vertex, ends in slot 0 of another
        assert {b[1] for b, _ in ends} >= {0, 1} and len(ends) == 6
    return g, seeds


def seed_graph(nv=1500, types=(1,), seed=5):
    """nv vertices with scattered vids; degree 0 .. 2 per type, so that with several types some vertices have edges in
    no slot, some in one and some in all."""
    rnd = random.Random(seed)
    vids = sorted(rnd.sample(range(10, 20 * nv), nv))
    edges = []
    for i, v in enumerate(vids):
        for t in types:
            if (i + t) % 5 == 0 or i % 7 == 0:                    # i % 7 == 0: degree 0 in all slots
                continue
            for d in rnd.sample(vids, 1 + (i + t) % 2):
                edges.append(edge(v, d, t, 0))
    return Graph(vids, edges, types=list(types))


def vid_width_graph():
    """Vids that need 1, 2, 4 and 8 bytes, negative ones among them, each with a present neighbour in vid order and a
    missing vid next to it."""
    vids = [-(1 << 40), -70000, -300, -2, -1, 1, 2, 100, 127, 128, 300, 32767, 32768, 70000, (1 << 31) - 1, 1 << 31,
            (1 << 40) + 7, INT64_MAX - 1]
    rnd = random.Random(9)
    edges = []
    for v in vids:
        for d in rnd.sample(vids, 3):
            edges.append(edge(v, d, 1, 0))
    return Graph(vids, edges)


def sparse_graph(n, kind="spread"):
    """A hop of exactly n edges for the sparse kernel. spread: destinations at random; one: every edge to one row;
    distinct: every destination different (the next frontier equals the edges)."""
    rnd = random.Random(50 + n)
    nv = max(n, 16) + 64
    adj, left, r = {}, n, 0
    dsts = list(range(nv))
    rnd.shuffle(dsts)
    while left:
        d = min(left, rnd.choice([1, 1, 2, 5, 40, 200]))
        if kind == "one":
            d = 1
            adj[r] = [nv - 3]
        elif kind == "distinct":
            adj[r] = [dsts.pop() for _ in range(d)]
        else:
            adj[r] = rnd.sample(range(nv), d)
        left -= d
        r += 1
    return fan(range(r), adj, nv)


def sparse_repeats():
    """One destination (row 900) once in every 256-edge slice of chunk 0 and once in each of chunks 0, 1 and 2; every
    other destination distinct."""
    nv = 3 * K_CHUNK + 1100
    per = K_CHUNK // K_SPARSE_SUB
    adj = {}
    nxt = iter(range(1000, nv))
    for k in range(3 * K_SPARSE_SUB):                             # row k owns slice k: 256 edges
        hit = k < K_SPARSE_SUB or k % K_SPARSE_SUB == 3
        adj[k] = ([900] if hit else []) + [next(nxt) for _ in range(per - (1 if hit else 0))]
    return fan(range(3 * K_SPARSE_SUB), adj, nv)


def pull_degrees(frontier_share=2, seed=0):
    """Targets with in-degree 0, 1, 1, 15, 16, 17, 1023, 1024, 1025 and 3000 (rows 0 .. 9; the two of in-degree 1 differ
    in whether their source is in the frontier: row 10 is in it, row 11 is not, both asserted), the other sources drawn
    from rows 10 .. 3009; every target has two out-edges for the hop after the pull. The frontier is one source row in
    `frontier_share` (at least 2)."""
    rnd = random.Random(70 + seed)
    degs = [0, 1, 1, 15, 16, 17, K_PULL_SEG - 1, K_PULL_SEG, K_PULL_SEG + 1, 3000]
    pool = list(range(10, 3010))
    nv = 3040
    adj = {}
    for t, d in enumerate(degs):
        for s in (pool if d == len(pool) else [pool[t - 1]] if d == 1 else rnd.sample(pool, d)):
            adj.setdefault(s, []).append(t)
        adj[t] = [3010 + t, 3011 + t]
    front = [s for k, s in enumerate(pool) if k % frontier_share == 0]
    assert 1 in adj[pool[0]] and 2 in adj[pool[1]] and pool[0] in front and pool[1] not in front
    assert [sum(1 for lst in adj.values() if t in lst) for t in range(10)] == degs
    return fan(front, adj, nv)


PULL_WHICH = ("head_first", "head_last", "past_head", "segment_last", "segment_first")


def pull_single(which):
    """Row T (the last but the seed) of in-degree 2100 (three K_PULL_SEG segments) whose only in-neighbour in the
    frontier is, as the pull kernel orders the in-list, PULL_WHICH: the first head entry (the source with the largest
    out-degree), the last head entry (the smallest out-degree among the K_PULL_K largest), the first source past the head
    (the 17th by out-degree), or the source at position K_PULL_SEG - 1 / K_PULL_SEG of the stored in-list (key order:
    the source vids' little-endian bytes): the last entry of segment 0 / the first of segment 1. Head source k has
    out-degree 19 - k, the 17th has 3, every other source 1; the extra edges go to filler rows. Forty decoy rows with
    one edge each to fillers are in the frontier too, so that the hop has enough edges to be pulled.
    Returns (Graph, seeds, T's vid)."""
    D = 2100
    nv = D + 120
    T = nv - 1
    order = sorted(range(D), key=lambda r: _key(r + 1))            # the stored in-list of T
    seg_last, seg_first = order[K_PULL_SEG - 1], order[K_PULL_SEG]
    head = [r for r in range(100, 400, 17) if r not in (seg_last, seg_first)][:K_PULL_K]
    past = next(r for r in range(500, 600) if r not in (seg_last, seg_first))
    assert len(head) == K_PULL_K
    fill = list(range(D, D + 30))
    adj = {r: [T] for r in range(D)}
    for k, r in enumerate(head):
        adj[r] = fill[:18 - k] + [T]
    adj[past] = fill[:2] + [T]
    decoys = list(range(D + 40, D + 80))
    for k, r in enumerate(decoys):
        adj[r] = [fill[k % 30]]
    adj[T] = [fill[0], fill[1], fill[2]]
    chosen = {"head_first": head[0], "head_last": head[-1], "past_head": past, "segment_last": seg_last,
              "segment_first": seg_first}[which]
    g, seeds = fan([chosen] + decoys, adj, nv)
    return g, seeds, T + 1


def pull_ring(nv, types=(1,), seed=0):
    """nv rows, every one with an in-edge of every type (a ring per type, plus random chords); a third of the rows in
    the frontier. The seed row has no in-edge, so the pull's image holds exactly nv rows."""
    rnd = random.Random(90 + nv + seed)
    adj = {}
    for r in range(nv):
        for t in types:
            ds = {(r + t) % nv}
            if rnd.random() < 0.4:
                ds.add(rnd.randrange(nv))
            adj.setdefault(r, []).extend((d, t, 0) for d in sorted(ds))
    return fan(rnd.sample(range(nv), max(nv // 3, 2)), adj, nv, types=list(types))


COMPACT_REACHED = ("none", "all", "first", "last", "edges")


COMPACT_SEED_ROW = 5


def compaction_graph(nv, kind):
    """nv rows in all; the seed is row 5 (vid 6) and its out-edges reach exactly the rows COMPACT_REACHED names: none,
    all (itself too), row 0, the last row, or rows 1023, 1024, 4095 and 4096 (those the table has): the ends of a
    wave's 1024-row run and of a K_COMPACT_TILE tile. The compaction after hop 1 lists them. Up to four reached rows
    get 90 out-edges each, so that hop 2 has at least nv / 100 edges for every nv up to 9000 and can be pulled (it then
    reads the bitmap, whose last word's last bit is the last row); more reached rows get one or two. The seed gets no
    edge beyond those that reach."""
    seed = COMPACT_SEED_ROW
    reached = {"none": [], "all": list(range(nv)), "first": [0], "last": [nv - 1],
               "edges": [r for r in (1023, 1024, K_COMPACT_TILE - 1, K_COMPACT_TILE) if r < nv]}[kind]
    assert kind == "all" or seed not in reached
    edges = [edge(seed + 1, r + 1) for r in reached]
    for r in reached:
        ds = range(r + 1, r + 91) if len(reached) <= 4 else {(r * 13 + 1), (r * 29 + 5)}
        for d in sorted({x % nv for x in ds}):
            if r != seed:                                         # (the seed's own edges are the ones above)
                edges.append(edge(r + 1, d + 1))
    assert len(reached) > 4 or not reached or 90 * 100 >= nv
    return Graph(range(1, nv + 1), edges), [seed + 1]


RANK_FORMS = {
    "zero": [0], "five": [5], "minus1": [-1], "int8": [-128, 127, 0], "int16": [-32768, 32767, 0, 200],
    "int32": [-(1 << 31), (1 << 31) - 1, 0, 70000], "int64": [INT64_MIN, INT64_MAX, 0, 1 << 40],
}
B_SETS = {
    "i8": [-128, 127], "i8x": [-129, 128], "i32": [-(1 << 31), (1 << 31) - 1], "i32x": [-(1 << 31) - 1, 1 << 31],
    "i64": [INT64_MIN, INT64_MAX],
}


def storage_graph(rank_e, rank_f, b_set, seed=0):
    """Two OVER types in different storage forms. Type e: every dst vid fits int8 (rows 1 .. 100); type f: one dst vid
    is 2^31 + 5 (the last vertex), so its dst column stays wide. Ranks of e / f cycle through RANK_FORMS[rank_e / rank_f]
    with every value present; parallel edges that differ only in rank where the form has several values. Column b of
    both types holds exactly the values of B_SETS[b_set]. GO 2 STEPS from the hub (vid 120)."""
    rnd = random.Random(seed + 17)
    big = (1 << 31) + 5
    vids = list(range(1, 101)) + [120, big]
    edges = []
    re_, rf = RANK_FORMS[rank_e], RANK_FORMS[rank_f]
    bs = B_SETS[b_set]
    n = [0]

    have = set()

    def add(a, d, t, r):
        if (a, d, t, r) in have:
            return
        have.add((a, d, t, r))
        p = default_props(a, d, t, r)
        edges.append(edge(a, d, t, r, (p[0], p[1], bs[n[0] % len(bs)])))
        n[0] += 1

    front = list(range(1, 61))
    for k, v in enumerate(front):
        add(120, v, 1, re_[k % len(re_)])
    for k, v in enumerate(front):
        ds = rnd.sample(range(1, 101), 4)
        for j, d in enumerate(ds):
            add(v, d, 1, re_[(k + j) % len(re_)])
        if len(re_) > 1:                                          # parallel edges that differ only in rank
            for r in re_:
                add(v, ds[0], 1, r)
        for j, d in enumerate(rnd.sample(range(1, 101), 3) + ([big] if k % 9 == 0 else [])):
            add(v, d, 2, rf[(k + j) % len(rf)])
        if len(rf) > 1 and k % 4 == 0:
            d = 1 + (v * 7) % 100
            for r in rf:
                add(v, d, 2, r)
    g = Graph(vids, edges, types=[1, 2])
    for t, form in ((1, re_), (2, rf)):
        assert {x[3] for x in g.edges if x[2] == t} == set(form), (t, form)
    assert {x[4][2] for x in g.edges} == set(bs)
    return g, [120]


def resv_arrays(rows, nsuper=4):
    """The row-reservation CSR, built with numpy: `nsuper` supernodes (rows 0 .. nsuper - 1) with `rows` out-edges of
    type e in all, to rows spread over the table; the seed (the last row) points at the supernodes. A final hop from
    the supernodes returns exactly `rows` rows without WHERE; p0 is the CSR position's parity, so `p0 < 1` keeps every
    second row. Returns (vpart, vid, slots, model columns): the columns (dst, rank, p0, p1) of the final hop's rows."""
    nv = max(rows // nsuper + nsuper + 2, 64)
    per = [rows // nsuper + (1 if k < rows % nsuper else 0) for k in range(nsuper)]
    assert max(per) <= nv - 1
    off = np.zeros(nv + 1, np.uint64)
    off[1:nsuper + 1] = np.cumsum(per)
    off[nsuper + 1:nv] = rows
    off[nv] = rows + nsuper
    dst_rows = np.concatenate([np.arange(p, dtype=np.int64) for p in per] + [np.arange(nsuper, dtype=np.int64)])
    src_rows = np.concatenate([np.full(p, k, np.int64) for k, p in enumerate(per)] + [np.full(nsuper, nv - 1, np.int64)])
    # key order inside a row: by the dst vid's little-endian bytes
    dvid = dst_rows + 1
    key = dvid.astype(np.uint64).byteswap()
    order = np.lexsort((key, src_rows))
    src_rows, dst_rows, dvid = src_rows[order], dst_rows[order], dvid[order]
    pos = np.arange(len(dvid), dtype=np.int64)
    p0 = pos % 2
    p1 = (pos * 6364136223846793005 + 1442695040888963407) % (1 << 40) - (1 << 39)
    b = pos % 200 - 100
    out = (1, off, dvid, [p0, p1, b], np.zeros(len(dvid), np.int64))
    # the exact mirror: in-edges of every row, sources in key order
    skey = (src_rows + 1).astype(np.uint64).byteswap()
    iorder = np.lexsort((skey, dst_rows))
    ioff = np.zeros(nv + 1, np.uint64)
    ioff[1:] = np.cumsum(np.bincount(dst_rows, minlength=nv))
    inn = (-1, ioff, (src_rows + 1)[iorder], [p0[iorder], p1[iorder], b[iorder]], np.zeros(len(dvid), np.int64))
    final = slice(0, rows)                                        # the supernodes' edges: the final hop's rows
    cols = [dvid[final], np.zeros(rows, np.int64), p0[final], p1[final]]
    return np.ones(nv, np.int32), np.arange(1, nv + 1, dtype=np.int64), [out, inn], cols, nv


def resv_graph(rows, nsuper=4):
    """The same graph as a Graph (for the model and the oracle)."""
    vpart, vid, slots, cols, nv = resv_arrays(rows, nsuper)
    _, off, dvid, (p0, p1, b), _ = slots[0]
    src = np.repeat(np.arange(1, nv + 1), np.diff(off.astype(np.int64)))
    edges = [(int(s), int(d), 1, 0, (int(x), int(y), int(z))) for s, d, x, y, z in zip(src, dvid, p0, p1, b)]
    return Graph(range(1, nv + 1), edges), [nv]


# ----------------------------------------------------------------------------- the cases
# Shared by tests/test_gpu_go_shapes.py (which runs them on the device) and tests/test_goref_host.py (which shows the
# model equal to the oracle on every one of them). A case: a graph builder and the queries run on it.
Query = namedtuple("Query", "form over direction m n seeds pushdown")


def Q(form, over=("e",), direction=FORWARD, m=None, n=2, seeds=None, pushdown=True):
    return Query(form, tuple(over), direction, m, n, tuple(seeds) if seeds is not None else None, pushdown)


Case = namedtuple("Case", "build queries kv")
CASES = {}
_built = {}


def case(name, build, queries, kv=False):
    CASES[name] = Case(build, queries, kv)


def built(name):
    """(Graph, default seeds) of a case, built once."""
    if name not in _built:
        _built[name] = CASES[name].build()[:2]
    return _built[name]


_models = {}


def case_model(name, q):
    """The model of one query of a case, computed once and shared."""
    if (name, q) not in _models:
        g, seeds = built(name)
        _models[(name, q)] = model(g, q.form, q.seeds if q.seeds is not None else seeds, q.over, q.direction, q.m, q.n,
                                   q.pushdown)
    return _models[(name, q)]


def case_sentence(name, q):
    g, seeds = built(name)
    return sentence(q.form, q.seeds if q.seeds is not None else seeds, q.over, q.direction, q.m, q.n)


def _repeat(vids, n):
    return [vids[(k * 7) % len(vids)] for k in range(n)]


def _seed_case(types, counts, form):
    g = seed_graph(types=types)
    over = [NAME_OF[t] for t in types]
    qs = [Q(form, over, n=2, seeds=_repeat(g.vids, c)) for c in counts]
    qs.append(Q(form, over, n=1, seeds=list(g.vids)))                              # every vertex, the seed hop records
    missing = [v + d for v in g.vids[::50] for d in (-1, 1) if v + d not in set(g.vids)]
    qs.append(Q(form, over, n=2, seeds=[x for v in missing for x in (v, v + 1 if v + 1 in set(g.vids) else v - 1)]))
    qs.append(Q(form, over, n=2, seeds=[g.vids[3], g.vids[8], g.vids[3]]))         # the same seed twice
    qs.append(Q("distinct", over[:1], n=2, seeds=[g.vids[3], g.vids[8], g.vids[3]]))
    qs.append(Q(form, over, n=2, seeds=[g.vids[0], g.vids[7], g.vids[14]]))        # degree 0 in all slots
    qs.append(Q(form, over, m=1, n=3, seeds=g.vids[1:40]))
    return lambda: (g, [g.vids[1]]), qs


# seed hop: seeds x slots = 1, 4095, 4096, 4097 entries with one OVER type; 3, 4095 and 4098 with three (1365 and 1366
# seeds: 4096 is no multiple of 3)
case("seed1", *_seed_case((1,), [1, K_SEED_FUSE_MAX - 1, K_SEED_FUSE_MAX, K_SEED_FUSE_MAX + 1], "bench"))
case("seed3", *_seed_case((1, 2, 3), [1, (K_SEED_FUSE_MAX - 1) // 3, K_SEED_FUSE_MAX // 3 + 1], "multi_all"))


def _vid_case():
    g = vid_width_graph()
    have = set(g.vids)
    seeds = []
    for v in g.vids:
        seeds.append(v)
        seeds += [w for w in (v - 1, v + 1) if w not in have and INT64_MIN <= w <= INT64_MAX]
    return g, seeds


case("vids", _vid_case, [Q("keys", n=1), Q("keys", n=2), Q("bench", n=2), Q("keys", direction=REVERSELY, n=2),
                         Q("keys", direction=BIDIRECT, n=2), Q("keys", direction=BIDIRECT, m=1, n=2)])

CHUNK_SIZES = (1, K_CHUNK - 1, K_CHUNK, K_CHUNK + 1, 3 * K_CHUNK + 5)
for _n in CHUNK_SIZES:
    case("chunk%d" % _n, (lambda n: lambda: frontier_edges(n))(_n), [Q("bench", n=2), Q("all", n=2), Q("all", n=3)])
case("chunk_supernode", supernode_midchunk, [Q("bench", n=2), Q("all", n=3)])
case("chunk_sparse_rows", sparse_rows, [Q("bench", n=2), Q("keys", n=2), Q("all", n=3)])
case("chunk_slots", interleaved_slots, [Q("multi_all", "efg", n=2), Q("multi", "efg", n=2, pushdown=False),
                                        Q("multi_all", "efg", n=3)])
case("chunk_empty_slot", lambda: interleaved_slots(empty_type=3),
     [Q("multi_all", "efg", n=2), Q("multi_all", "gfe", n=2), Q("multi_all", "efg", n=3)])

SPARSE_SIZES = (255, 256, 257, K_CHUNK - 1, K_CHUNK, K_CHUNK + 1)
for _n in SPARSE_SIZES:
    case("sparse%d" % _n, (lambda n: lambda: sparse_graph(n))(_n), [Q("all", n=3), Q("distinct", n=4)])
case("sparse_one", lambda: sparse_graph(K_CHUNK + 1, "one"), [Q("all", n=3)])
case("sparse_distinct", lambda: sparse_graph(K_CHUNK + 1, "distinct"), [Q("all", n=3)])
case("sparse_repeats", sparse_repeats, [Q("all", n=3)])
case("sparse_empty", lambda: fan(range(40), {}, 100), [Q("all", n=3)])
case("sparse_after_pull", lambda: pull_ring(600), [Q("all", n=3), Q("bench", n=4)])

case("pull_degrees", lambda: pull_degrees(2), [Q("all", n=3), Q("bench", n=3)])
case("pull_degrees_thin", lambda: pull_degrees(60), [Q("all", n=3)])
for _w in PULL_WHICH:
    case("pull_" + _w, (lambda w: lambda: pull_single(w))(_w), [Q("all", n=3)])
PULL_V = (63, 64, 65, K_PULL_WINDOW - 1, K_PULL_WINDOW, K_PULL_WINDOW + 1)
for _n in PULL_V:
    case("pull_v%d" % _n, (lambda n: lambda: pull_ring(n))(_n), [Q("all", n=3)])
case("pull_4types", lambda: pull_ring(300, (1, 2, 3, 4)), [Q("multi_all", "efgh", n=3)])
case("pull_5types", lambda: pull_ring(300, (1, 2, 3, 4, 5)), [Q("multi_all", "efghi", n=3)])

COMPACT_V = (K_COMPACT_TILE - 1, K_COMPACT_TILE, K_COMPACT_TILE + 1, 2 * K_COMPACT_TILE + 1)
for _n in COMPACT_V:
    for _k in COMPACT_REACHED:
        case("compact%d_%s" % (_n, _k), (lambda n, k: lambda: compaction_graph(n, k))(_n, _k), [Q("all", n=3)])

STORAGE = (("zero", "int8", "i8"), ("five", "int16", "i8x"), ("minus1", "int32", "i32"), ("int64", "zero", "i32x"),
           ("int8", "int64", "i64"), ("int16", "five", "i64"))
for _c in STORAGE:
    case("storage_%s_%s_%s" % _c, (lambda c: lambda: storage_graph(*c))(_c),
         [Q("multi_all", "ef", n=2), Q("multi", "ef", n=2), Q("multi", "fe", n=2, pushdown=False), Q("signed", "e", n=2), Q("signed", "f", n=2), Q("keys", "e", n=2),
          Q("bench", "e", n=2)])


def _tag_case():
    g, seeds = frontier_edges(300, seed=4)
    g.tags = {v: (v * 37) % 1000 - 300 for v in g.vids if v % 3}           # a third of the vertices lack the tag
    return g, seeds


case("tags", _tag_case, [Q("tags", n=2), Q("tags", m=1, n=2)], kv=True)

RESV_ROWS = ((1 << K_RESV_SHIFT) - 1, 1 << K_RESV_SHIFT, (1 << K_RESV_SHIFT) + 1, K_RESV_GROUPS * (1 << K_RESV_SHIFT) + 1)


# ----------------------------------------------------------------------------- shaped shards (world > 1)
# Shared by tests/goshard_worker.py (one child process per rank rebuilds a case by name), tests/test_gpu_go_shards.py
# and tests/test_goshard_host.py. num_parts = world, so a residue class of vid is one part on one shard and a shard's
# rows are its vids in ascending order.
class Shards:
    """Vids such that shard q holds exactly counts[q] rows: local row i of shard q is `vid(q, i)`, global row
    `row(q, i)`."""

    def __init__(self, counts):
        self.world = self.num_parts = len(counts)
        self.counts = list(counts)
        assert 2 <= self.world <= K_MAX_WORLD
        self.base = [0]
        for n in counts:
            self.base.append(self.base[-1] + n)
        self.vglobal = self.base[-1]

    def vid(self, q, i):
        assert 0 <= i < self.counts[q], (q, i)
        return self.world * (i + 1) + (q - 1) % self.world

    def row(self, q, i):
        assert 0 <= i < self.counts[q], (q, i)
        return self.base[q] + i

    def vids(self):
        return [self.vid(q, i) for q in range(self.world) for i in range(self.counts[q])]

    def where(self, vid):
        """(shard, local row) of a vid."""
        q = shard_of(vid, self.num_parts, self.world)
        return q, vid // self.world - 1

    def check(self, graph, vids=None):
        """The placement rule gives this graph the tables the counts claim: a change of the rule fails here."""
        tables, base = shard_tables(graph, self.num_parts, self.world, vids)
        assert [len(t) for t in tables] == self.counts, ([len(t) for t in tables], self.counts)
        assert base == self.base
        for q, t in enumerate(tables):
            assert t == [self.vid(q, i) for i in range(self.counts[q])], q


def sharded(counts, base_mod=None, vglobal_mod=None):
    """A Shards of exactly these per-shard row counts (0 included); base_mod: {q: shardBase[q] & 63} and vglobal_mod:
    vglobal & 63, asserted where the case's name claims them."""
    sh = Shards(counts)
    for q, m in (base_mod or {}).items():
        assert sh.base[q] & 63 == m, (q, sh.base[q], m)
    assert vglobal_mod is None or sh.vglobal & 63 == vglobal_mod, (sh.vglobal, vglobal_mod)
    return sh


def marker_graph(sh, senders, decoys=(), seed0=None, dup=False, tags=None):
    """The graph of an exchange case. senders: {(q, i): [(q', i'), ...]}: the out-edges (rank 0; with dup a parallel edge
    of rank 1 too) whose marks the hop under test exchanges; decoys: the same for rows that are never in the frontier.
    seed0: a row with an edge to every sender (GO 3 STEPS from it: the senders are hop 2's frontier); without it the
    senders are the seeds of a GO 2 STEPS. Every other row t (the pool) has exactly one out-edge, to the next pool row in
    global row order (cyclic), whose p1 is t's global row: the hop after the one under test returns one row per reached
    vertex, and a further hop again one per vertex. Senders, decoys and seed0 are never targets.
    Returns (Graph, seeds)."""
    special = set(senders) | set(dict(decoys)) | ({seed0} if seed0 else set())
    pool = [(q, i) for q in range(sh.world) for i in range(sh.counts[q]) if (q, i) not in special]
    edges = []
    for k, (q, i) in enumerate(pool):
        nq, ni = pool[(k + 1) % len(pool)]
        edges.append(edge(sh.vid(q, i), sh.vid(nq, ni), 1, 0, (0, sh.row(q, i), 0)))
    for src, targets in list(senders.items()) + list(dict(decoys).items()):
        assert len(set(targets)) == len(targets) and not set(targets) & special, src
        for t in targets:
            edges.append(edge(sh.vid(*src), sh.vid(*t), 1, 0))
            if dup:
                edges.append(edge(sh.vid(*src), sh.vid(*t), 1, 1))
    if seed0:
        edges += [edge(sh.vid(*seed0), sh.vid(*s), 1, 0) for s in sorted(senders)]
    g = Graph(sh.vids(), edges, types=[1], tags=tags)
    sh.check(g)
    return g, [sh.vid(*seed0)] if seed0 else [sh.vid(*s) for s in sorted(senders)]


def hop_frontiers(graph, seeds, n):
    """FORWARD over type e: the frontier (vids) of hops 1 .. n, by the model's rule."""
    out, frontier = [], list(seeds)
    for _ in range(n):
        out.append(frontier)
        frontier = sorted({w for v in frontier for _, w, _ in graph.rows().get((v, 1), ())})
    return out


def rows_sent(graph, sh, seeds, hop, rank):
    """The rows of other shards that `rank` marks in hop `hop` (1-based) of a FORWARD GO over e."""
    mine = [v for v in hop_frontiers(graph, seeds, hop)[hop - 1] if sh.where(v)[0] == rank]
    return len({w for v in mine for _, w, _ in graph.rows().get((v, 1), ()) if sh.where(w)[0] != rank})


def xchg_bitmap_bytes(counts, rank):
    """exchangeFrontier's lastXchgBytes: a bitmap of every peer's rows, in 64-bit words."""
    return sum((n + 63) // 64 * 8 for q, n in enumerate(counts) if q != rank)


def xchg_list_bytes(world, sent):
    """exchangeFrontierList's lastXchgBytes: the all-gathered counts and 4 bytes per row sent."""
    return (world - 1) * world * 8 + 4 * sent


def xchg_pull_bytes(counts):
    """A pulled hop at world > 1: this shard's frontier bitmap, the largest shard's words long, to every peer."""
    return max((n + 63) // 64 for n in counts) * 8 * (len(counts) - 1)


def pulled(model_, q, pull_factor, vglobal):
    """The intermediate hops (1-based) every shard pulls: the hop's edges over all shards E > 0 and
    E * 100 >= pull_factor * vglobal (engine.cpp ngx_go, the pull gather)."""
    return [h for h, E in enumerate(model_.hop_edges, 1) if h < q.n and pull_factor > 0 and E > 0 and
            E * 100 >= pull_factor * vglobal]


# A query of a shard case: the Query, the engine flags (every rank alike), and what proves the path: `xchg` maps a hop
# (1-based) to "bitmap", "list" or "pull", `counters` the exact increase of the read-only counters on every rank.
SQ = namedtuple("SQ", "q flags xchg counters")
ShardCase = namedtuple("ShardCase", "world counts build queries kv")
SHARD_CASES = {}
_shard_built = {}
BITMAP = {"xchg_lists": 0, "pull_factor": 0}
LISTS = {"xchg_lists": 1, "pull_factor": 0}
AUTO = {"xchg_lists": -1, "pull_factor": 0}
SHARD_COUNTERS = ("pull_hops", "xchg_list_hops", "dense_finals", "dst_fetches")


def shard_case(name, counts, build, queries, kv=False):
    assert name not in SHARD_CASES
    SHARD_CASES[name] = ShardCase(len(counts), list(counts), build, queries, kv)


def shard_built(name):
    """(Graph, default seeds, Shards) of a shard case, built once."""
    if name not in _shard_built:
        _shard_built[name] = SHARD_CASES[name].build()
    return _shard_built[name]


def shard_seeds(name, sq):
    return list(sq.q.seeds) if sq.q.seeds is not None else shard_built(name)[1]


def shard_model(name, k):
    q = SHARD_CASES[name].queries[k].q
    if ("shard", name, k) not in _models:
        g = shard_built(name)[0]
        _models[("shard", name, k)] = model(g, q.form, shard_seeds(name, SHARD_CASES[name].queries[k]), q.over, q.direction,
                                            q.m, q.n, q.pushdown)
    return _models[("shard", name, k)]


def shard_sentence(name, k):
    sq = SHARD_CASES[name].queries[k]
    return sentence(sq.q.form, shard_seeds(name, sq), sq.q.over, sq.q.direction, sq.q.m, sq.q.n)


def shard_cases(world):
    return [n for n in SHARD_CASES if SHARD_CASES[n].world == world]


def assert_merged(shard_rows, shard_hop_edges, want, distinct=False, what=""):
    """shard_rows: per shard its rows as typed cells; shard_hop_edges: per shard its edges scanned per hop. The rows
    concatenated (for DISTINCT: their set, as graphd applies it to the merged responses) equal the model's as sorted
    typed rows, and the shards' edges sum to the model's per hop."""
    merged = [tuple(typed_cell(k, v) for k, v in r) for rows in shard_rows for r in rows]
    if distinct:
        merged = list(set(merged))
    a, b = sorted(merged), typed_rows(want.rows)
    if a != b:
        sa, sb = set(a), set(b)
        raise AssertionError((what, "rows", len(a), len(b), sorted(sa - sb)[:3], sorted(sb - sa)[:3]))
    hops = len(want.hop_edges)
    summed = [sum(int(e[h]) if h < len(e) else 0 for e in shard_hop_edges) for h in range(max([hops] + [len(e) for e in shard_hop_edges]))]
    assert summed == list(want.hop_edges), (what, "hop_edges", summed, want.hop_edges)


def _edge_rows(n):
    """The rows of an n-row range at a wave's, a k_pack block's and a k_pack_list run's and tile's ends."""
    return sorted({r for r in (0, 63, 64, K_XCHG_BLOCK - 1, K_XCHG_BLOCK, K_LIST_THREADS - 1, K_LIST_THREADS,
                               K_LIST_TILE - 1, K_LIST_TILE, n - 1) if 0 <= r < n})


def _w2_build(n):
    """World 2, counts [8, n]: five senders on shard 0 whose marks in shard 1's range are none (a row of shard 0
    instead), row 0, the last row, the edge rows (63 | 64, 255 | 256, 1023 | 1024, 4095 | 4096 where the range has
    them) and all n rows."""
    def build():
        sh = sharded([8, n])
        senders = {(0, 0): [(0, 7)], (0, 1): [(1, 0)], (0, 2): [(1, n - 1)], (0, 3): [(1, r) for r in _edge_rows(n)],
                   (0, 4): [(1, r) for r in range(n)]}
        g, seeds = marker_graph(sh, senders)
        return g, seeds, sh
    return build


def _w2_queries(n, flags, kind):
    v = lambda i: [2 * (i + 1) + 1]                                # Shards.vid(0, i) at world 2
    # in this order: the query that marks every row of the peer, then the one that marks only its last row, on buffers
    # the first one filled
    order = [0, 1, 3, 4, 2]
    qs = [SQ(Q("all", seeds=v(i)), flags, {1: kind}, {"xchg_list_hops": 1 if kind == "list" else 0, "pull_hops": 0})
          for i in order]
    return qs


BITMAP_N = (1, 63, 64, 65, K_XCHG_BLOCK - 1, K_XCHG_BLOCK, K_XCHG_BLOCK + 1, K_LIST_TILE + 1)
for _n in BITMAP_N:
    shard_case("bitmap_w2_%d" % _n, [8, _n], _w2_build(_n), _w2_queries(_n, BITMAP, "bitmap"))
LIST_N = (1, K_LIST_THREADS - 1, K_LIST_THREADS, K_LIST_THREADS + 1, K_LIST_TILE - 1, K_LIST_TILE, K_LIST_TILE + 1,
          2 * K_LIST_TILE + 1)
for _n in LIST_N:
    shard_case("list_w2_%d" % _n, [8, _n], _w2_build(_n), _w2_queries(_n, LISTS, "list"))


def _forms_build(counts):
    """Senders on every shard that has more than two rows, each marking the first and the last row of every other
    shard's pool: the graph of the DISTINCT and the REVERSELY query of a world."""
    def build():
        sh = sharded(counts)
        src = [(q, 1) for q in range(sh.world) if sh.counts[q] > 2]
        senders = {}
        for s in src:
            ts = []
            for q in range(sh.world):
                rows = [i for i in (0, sh.counts[q] - 1) if 0 <= i < sh.counts[q] and (q, i) not in src]
                ts += [(q, i) for i in sorted(set(rows))]
            senders[s] = ts
        g, seeds = marker_graph(sh, senders)
        return g, seeds, sh
    return build


def _forms_queries(sh_counts):
    sh = Shards(sh_counts)
    target = sh.vid(max(range(len(sh_counts)), key=lambda q: sh_counts[q]), 0)
    none = {"xchg_list_hops": 0, "pull_hops": 0}
    return [SQ(Q("all"), BITMAP, {1: "bitmap"}, none), SQ(Q("distinct"), BITMAP, {1: "bitmap"}, none),
            SQ(Q("all", n=3), BITMAP, {1: "bitmap", 2: "bitmap"}, none),
            SQ(Q("keys", direction=REVERSELY, seeds=[target]), BITMAP, {1: "bitmap"}, none),
            SQ(Q("all"), LISTS, {1: "list"}, {"xchg_list_hops": 1, "pull_hops": 0}),
            SQ(Q("distinct", n=3), LISTS, {1: "list", 2: "list"}, {"xchg_list_hops": 2, "pull_hops": 0})]


W8_COUNTS = [3, 1, 0, 58, 1, 64, 5, 70]      # global rows 0 .. 63: shards 0, 1, (2,) 3, 4 and the first row of 5
shard_case("forms_w2", [70, 129], _forms_build([70, 129]), _forms_queries([70, 129]))
shard_case("forms_w3_empty", [66, 0, 130], _forms_build([66, 0, 130]), _forms_queries([66, 0, 130]))
shard_case("forms_w8", W8_COUNTS, _forms_build(W8_COUNTS), _forms_queries(W8_COUNTS))


def _triple_build():
    """World 3: a sender on each shard, all three marking row 64 and row 0 of shard 1 (its owner's sender too), and the
    senders of shards 0 and 2 each one row of shard 1 the other does not."""
    sh = sharded([5, 66, 4])
    senders = {(0, 1): [(1, 64), (1, 0), (1, 63)], (1, 1): [(1, 64), (1, 0)], (2, 1): [(1, 64), (1, 0), (1, 65)]}
    g, seeds = marker_graph(sh, senders)
    return g, seeds, sh


shard_case("bitmap_w3_triple", [5, 66, 4], _triple_build,
           [SQ(Q("all"), BITMAP, {1: "bitmap"}, {"xchg_list_hops": 0, "pull_hops": 0}),
            SQ(Q("all"), LISTS, {1: "list"}, {"xchg_list_hops": 1, "pull_hops": 0})])


def _two_senders_build():
    """World 3, counts [6, 4097, 6]: the senders of shards 0 and 2 both list rows of shard 1: one of them 4000 rows
    (among them the tile's edge rows), the other 3 (one of them shared), while shard 1 sends nothing: the host
    collective pads every pair's list to 4000 entries."""
    sh = sharded([6, K_LIST_TILE + 1, 6])
    n = K_LIST_TILE + 1
    many, r = set(_edge_rows(n)), 50
    while len(many) < 4000:
        many.add(r)
        r += 1
    many = sorted(many)
    senders = {(0, 1): [(1, r) for r in many], (2, 1): [(1, 5), (1, 4095), (1, 4090)]}
    g, seeds = marker_graph(sh, senders)
    return g, seeds, sh


shard_case("list_w3_two_senders", [6, K_LIST_TILE + 1, 6], _two_senders_build,
           [SQ(Q("all"), LISTS, {1: "list"}, {"xchg_list_hops": 1, "pull_hops": 0}),
            SQ(Q("all"), BITMAP, {1: "bitmap"}, {"xchg_list_hops": 0, "pull_hops": 0})])

AUTO_E = 2


def _auto_build(smallest):
    """The hop's busiest shard scans AUTO_E edges; the smallest shard has `smallest` rows."""
    def build():
        sh = sharded([smallest, smallest + 6])
        g, seeds = marker_graph(sh, {(0, 1): [(1, 0), (1, smallest + 5)]})
        return g, seeds, sh
    return build


shard_case("auto_w2_bitmap", [K_XCHG_LIST_FACTOR * AUTO_E] * 1 + [K_XCHG_LIST_FACTOR * AUTO_E + 6],
           _auto_build(K_XCHG_LIST_FACTOR * AUTO_E), [SQ(Q("all"), AUTO, {1: "bitmap"}, {"xchg_list_hops": 0, "pull_hops": 0})])
shard_case("auto_w2_list", [K_XCHG_LIST_FACTOR * AUTO_E + 1] + [K_XCHG_LIST_FACTOR * AUTO_E + 7],
           _auto_build(K_XCHG_LIST_FACTOR * AUTO_E + 1), [SQ(Q("all"), AUTO, {1: "list"}, {"xchg_list_hops": 1, "pull_hops": 0})])


def _pull_build(counts, base_mod, vglobal_mod):
    """GO 3 STEPS from seed0: hop 2's frontier is the senders: rows 0, 1, 62 .. 65, n - 2 and n - 1 of every shard (those
    it has): the first and the last row, and the rows around a word's end, whose bits the repack takes from the next
    segment word. Rows 2, 61, 66 and n - 3 are decoys with out-edges but outside the frontier. Every sender and decoy
    has two parallel edges to one pool row of its own, so a lost frontier bit loses a row and a spurious one adds one."""
    def build():
        sh = sharded(counts, base_mod, vglobal_mod)
        big = max(range(sh.world), key=lambda q: sh.counts[q])
        seed0 = (big, 30)
        send, decoy = [], []
        for q in range(sh.world):
            n = sh.counts[q]
            s = sorted({i for i in (0, 1, 62, 63, 64, 65, n - 2, n - 1) if 0 <= i < n})
            send += [(q, i) for i in s]
            decoy += [(q, i) for i in sorted({2, 61, 66, n - 3}) if 0 <= i < n and i not in s and (q, i) != seed0 and n > 8]
        special = set(send) | set(decoy) | {seed0}
        pool = [(q, i) for q in range(sh.world) for i in range(sh.counts[q]) if (q, i) not in special]
        assert len(pool) >= len(send) + len(decoy), (len(pool), len(send), len(decoy))
        # the senders' targets spread over the whole pool (and so over every shard that has pool rows), each decoy's
        # target the pool row after a sender's
        at = [k * len(pool) // len(send) for k in range(len(send))]
        assert len(set(at)) == len(at) and all(b - a >= 2 for a, b in zip(at, at[1:])) and at[-1] + 1 < len(pool)
        senders = {s: [pool[at[k]]] for k, s in enumerate(send)}
        decoys = {d: [pool[at[k * len(send) // max(len(decoy), 1)] + 1]] for k, d in enumerate(decoy)}
        assert {q for ts in senders.values() for q, _ in ts} >= {q for q in range(sh.world) if sh.counts[q] >= 40}
        g, seeds = marker_graph(sh, senders, decoys, seed0=seed0, dup=True)
        assert (big, sh.counts[big] - 1) in senders
        return g, seeds, sh
    return build


def _pull_queries(counts):
    """pull_factor 1: hop 2 (and hop 1 where its edges suffice) is pulled, then the dense final hop, its totals sized
    on the device and on the host; then GO 4 STEPS with the pull_factor that hop 2's edges reach and hop 3's do not:
    a pulled hop followed by a pushed one. The expected counters come from the model (tests/test_gpu_go_shards.py)."""
    return [SQ(Q("all", n=3), {"pull_factor": 1, "xchg_lists": 0, "dense_world_dev": 1}, None, None),
            SQ(Q("all", n=3), {"pull_factor": 1, "xchg_lists": 0, "dense_world_dev": 0}, None, None),
            SQ(Q("all", n=4), {"pull_factor": "hop2", "xchg_lists": 0, "dense_world_dev": 1}, None, None)]


PULL_SHAPES = {
    "pull_w2_base0": ([64, 40], {1: 0}, 40),          # shardBase[1] & 63 == 0; vglobal no multiple of 64
    "pull_w2_base1": ([65, 63], {1: 1}, 0),           # == 1; vglobal == 128
    "pull_w2_base63": ([63, 128], {1: 63}, 63),       # == 63; the largest shard ends with its last word's last bit
    "pull_w3_empty": ([70, 0, 122], {1: 6, 2: 6}, 0),
    "pull_w8": (W8_COUNTS, {3: 4, 5: 63, 7: 4}, 10),   # output word 0 holds four shards with rows and part of a fifth
}
for _name, (_c, _b, _v) in PULL_SHAPES.items():
    shard_case(_name, _c, _pull_build(_c, _b, _v), _pull_queries(_c))


def pull_factor_hop2(name, k):
    """The pull_factor that pulls hop 2 of a GO 4 STEPS and pushes its hop 3: the largest with E2 * 100 >= pf * vglobal."""
    m = shard_model(name, k)
    sh = shard_built(name)[2]
    pf = m.hop_edges[1] * 100 // sh.vglobal
    assert pf >= 1 and m.hop_edges[2] * 100 < pf * sh.vglobal and m.hop_edges[0] * 100 < pf * sh.vglobal, (name, pf, m.hop_edges)
    return pf


def shard_flags(name, k):
    f = dict(SHARD_CASES[name].queries[k].flags)
    if f.get("pull_factor") == "hop2":
        f["pull_factor"] = pull_factor_hop2(name, k)
    return f


def _tags_build(counts, where):
    """GO 2 STEPS from seed0 (shard 0) over senders on every shard with rows to spare; the final hop's destinations are
    on the sender's own shard only (`self`), on the next shard only (`peer`), or on every shard (`all`). A third of the
    vertices have no tag row, a sender and a destination among them; negative x fails the WHERE. Every vertex has an
    edge, so a KV load knows every row."""
    def build():
        sh = sharded(counts)
        W = sh.world
        src = [(q, 1) for q in range(W) if sh.counts[q] > 3]
        seed0 = (src[0][0], 2)
        senders = {}
        for k, s in enumerate(src):
            q = s[0]
            owners = {"self": [q], "peer": [src[(k + 1) % len(src)][0]], "all": [p for p in range(W) if sh.counts[p]]}[where]
            senders[s] = [(p, i) for p in owners for i in sorted({0, sh.counts[p] - 1, 3 % sh.counts[p]})
                          if (p, i) not in src and (p, i) != seed0]
        g, seeds = marker_graph(sh, senders, seed0=seed0)
        tags = {}
        for n_, v in enumerate(g.vids):
            if n_ % 3 != 2:
                tags[v] = (v * 37) % 1000 - 200
        lacking = set(g.vids) - set(tags)
        ends = {sh.vid(*t) for ts in senders.values() for t in ts}
        tags.pop(sh.vid(*src[-1]), None)                          # a source without a tag row
        tags.pop(sorted(ends)[0], None)                           # a destination without one
        assert lacking and ends - set(tags) and ends & set(tags)
        g.tags = tags
        sh.check(g, kv_vertices(g))
        return g, seeds, sh
    return build


def _tags_queries():
    return [SQ(Q("tags"), {"dst_props": 0, "xchg_lists": 0, "pull_factor": 0}, {1: "bitmap"}, {"dst_fetches": 0}),
            SQ(Q("tags"), {"dst_props": 1, "xchg_lists": 0, "pull_factor": 0}, {1: "bitmap"}, {"dst_fetches": 1})]


shard_case("tags_w2_self", [9, 14], _tags_build([9, 14], "self"), _tags_queries(), kv=True)
shard_case("tags_w2_peer", [9, 14], _tags_build([9, 14], "peer"), _tags_queries(), kv=True)
shard_case("tags_w3_all", [7, 70, 12], _tags_build([7, 70, 12], "all"), _tags_queries(), kv=True)
shard_case("tags_w8_all", W8_COUNTS, _tags_build(W8_COUNTS, "all"), _tags_queries(), kv=True)


# ----------------------------------------------------------------------------- pipes: GO ... FROM $-.id / $var.id
# The reference rule (GoExecutor.cpp:471-509 setupStarts, :1317-1330 getRoots + rowsOfVids): an edge row is emitted once
# per input row whose vid is one of the row's roots, `$-.x` bound to that input row. Per root that is a GO from the root
# alone, so: per input row i with vid v_i the rows are exactly those of `GO ... FROM v_i`, `$-.x` bound to row i's
# cells; the result is the concatenation over the input rows; YIELD DISTINCT is one set over the whole result. An input
# vid that is no vertex, or has no edges, contributes nothing. `pipe` is that loop over `go`, nothing else: no root
# sets, no batches.
PIPE_COLS = ("id", "k", "w", "s", "d")                            # the vid column, two INT, a STRING, a DOUBLE
T_DOUBLE, T_STRING = 5, 6                                         # pipeline.T_DOUBLE / T_STRING (asserted by the host test)


def pipe_input(rows, vid_type=kvfmt.VID):
    """rows: (vid, k, w, s, d) tuples -> the Interim a pipe's right side reads. vid_type: the vid column as VID or INT."""
    from nebula_amd import pipeline
    kind = "id" if vid_type == kvfmt.VID else "int"
    return pipeline.Interim(list(PIPE_COLS), [vid_type, kvfmt.INT, kvfmt.INT, T_STRING, T_DOUBLE],
                            [((kind, v), ("int", k), ("int", w), ("str", s), ("double", d)) for v, k, w, s, d in rows])


def input_row(v, j, dup=0, w=None):
    """The input row of root j (its dup-th): k is j mod K_ROOT_BATCH (roots 0 and 64 share it), w differs per duplicate."""
    return (v, j % K_ROOT_BATCH, (j * 37 + dup * 11) % 100 if w is None else w, "r%d.%d" % (j, dup), j + dup / 4.0)


def _pe(kind, name, k=0):
    return lambda over: (lambda row, inp: (kind, _of(row, over[k], name)))


def _pin(name):
    return lambda over: (lambda row, inp: inp[name])


# A pipe form: as Form, but the callables also receive the input row ({column name: cell}); reads: WHERE or YIELD read
# the input (the device then keys entries by (frontier row, input row)); var: the sentence reads `$var` instead of `$-`.
PipeForm = namedtuple("PipeForm", "name tail where yields distinct min_over reads var")
PIPE_FORMS = {f.name: f for f in [
    PipeForm("all", "YIELD {a}._dst, {a}.p1", None, [_pe("id", "_dst"), _pe("int", "p1")], False, 1, False, None),
    PipeForm("all_d", "YIELD DISTINCT {a}._dst, {a}.p1", None, [_pe("id", "_dst"), _pe("int", "p1")], True, 1, False, None),
    PipeForm("keys", "YIELD {a}._src, {a}._dst, {a}._type", None,
             [_pe("id", "_src"), _pe("id", "_dst"), _pe("int", "_type")], False, 1, False, None),
    PipeForm("k", "YIELD $-.k, {a}._dst", None, [_pin("k"), _pe("id", "_dst")], False, 1, True, None),
    PipeForm("k_d", "YIELD DISTINCT $-.k, {a}._dst", None, [_pin("k"), _pe("id", "_dst")], True, 1, True, None),
    PipeForm("w", "WHERE {a}.p0 >= $-.w YIELD $-.w, $-.s, $-.d, {a}._dst, {a}.p0",
             lambda over: (lambda row, inp: _of(row, over[0], "p0") >= inp["w"][1]),
             [_pin("w"), _pin("s"), _pin("d"), _pe("id", "_dst"), _pe("int", "p0")], False, 1, True, None),
    PipeForm("two", "YIELD $-.k, {a}._dst, {b}._dst, {a}.p0, {b}.p0", None,
             [_pin("k"), _pe("id", "_dst"), _pe("id", "_dst", 1), _pe("int", "p0"), _pe("int", "p0", 1)], False, 2, True, None),
    PipeForm("var", "WHERE {a}.p0 >= $v.w YIELD $v.w, $v.s, {a}._dst",
             lambda over: (lambda row, inp: _of(row, over[0], "p0") >= inp["w"][1]),
             [_pin("w"), _pin("s"), _pe("id", "_dst")], False, 1, True, "v"),
]}


def pipe_sentence(form, over, direction=FORWARD, m=None, n=1):
    f = PIPE_FORMS[form]
    assert len(over) >= f.min_over
    steps = "%d STEPS" % n if m is None else "%d TO %d STEPS" % (m, n)
    tail = f.tail.replace("{a}", over[0]).replace("{b}", over[1] if len(over) > 1 else over[0])
    return "GO %s FROM %s.id OVER %s%s %s" % (steps, "$" + f.var if f.var else "$-", ", ".join(over), _DIR[direction], tail)


def pipe(graph, form, inp, over, direction=FORWARD, m=None, n=1):
    """The rows of the pipe form over the input `inp` (an Interim with a column `id`): see the section's comment."""
    f = PIPE_FORMS[form]
    types = [TYPE_OF[x] for x in over]
    where = f.where(types) if f.where else None
    ys = [y(types) for y in f.yields]
    at = inp.names.index("id")
    out = []
    for cells in inp.rows:
        env = dict(zip(inp.names, cells))
        out += go(graph, [cells[at][1]], types, direction, n if m is None else m, n,
                  (lambda row, env=env: where(row, env)) if where else None,
                  [(lambda row, y=y, env=env: y(row, env)) for y in ys]).rows
    if f.distinct:
        out = list(dict.fromkeys(out))
    return out


Plan = namedtuple("Plan", "walks hop_edges hop_frontier")


def pipe_plan(graph, form, inp, over, direction=FORWARD, m=None, n=1, fallback=False):
    """What the device plan scans (engine.cpp runPipe), for hop_edges / hop_frontier and the pipe_walks counter only:
    no input row: nothing; one step and no read of the input: one plain walk from the distinct vids (first-seen order);
    otherwise one walk per K_ROOT_BATCH distinct vids from their union; fallback (a storage mask: the walk cannot be
    keyed by root): one walk per distinct vid, or per input row where the input is read. The statistics add up."""
    f = PIPE_FORMS[form]
    types = [TYPE_OF[x] for x in over]
    at = inp.names.index("id")
    vids = list(dict.fromkeys(c[at][1] for c in inp.rows))
    if not vids:
        return Plan(0, [], [])
    if not f.reads and n == 1:
        starts = [vids]
    elif fallback:
        starts = [[c[at][1]] for c in inp.rows] if f.reads else [[v] for v in vids]
    else:
        starts = [vids[b:b + K_ROOT_BATCH] for b in range(0, len(vids), K_ROOT_BATCH)]
    he, hf = [], []
    for s in starts:
        r = go(graph, s, types, direction, n, n, None, [])
        for acc, x in ((he, r.hop_edges), (hf, r.hop_frontier)):
            acc += [0] * (len(x) - len(acc))
            for h, v in enumerate(x):
                acc[h] += v
    return Plan(len(starts), he, hf)


# ---- shaped graphs and inputs (every generator returns (Graph, {input name: Interim}))
def _rotated(n, by=5):
    return [(j + by) % n for j in range(n)]


def roots_graph(R, same_mid=None, vid_type=kvfmt.VID, rotate=5):
    """R roots (vid 1 + j), each with a private path root -> mid (10000 + j) -> leaf (20000 + j) whose edges carry
    p1 = j and p0 = j % 100; same_mid {j: i}: root j points at root i's mid instead (and has no mid of its own). One
    input row per root, in an order rotated by `rotate` so that a root's bit is not its row."""
    same_mid = same_mid or {}
    edges = []
    for j in range(R):
        mj = same_mid.get(j, j)
        edges.append(edge(1 + j, 10000 + mj, 1, 0, (j % 100, j, 0)))
        if mj == j:
            edges.append(edge(10000 + j, 20000 + j, 1, 0, (j % 100, j, -j)))
    vids = {v for e_ in edges for v in e_[:2]}
    return Graph(vids, edges), {"in": pipe_input([input_row(1 + j, j) for j in _rotated(R, rotate)], vid_type)}


CONVERGE_ROOTS = K_ROOT_BATCH
HUB, SIDE = 500, 501


def converge_mults(m_last):
    """Input rows per root: 1, 2, 3 in turn, the last root m_last."""
    return [1 + j % 3 for j in range(CONVERGE_ROOTS - 1)] + [m_last]


def converge_graph(m_last, D, flip=False, two=False):
    """K_ROOT_BATCH roots (vids 1 ..) of one batch that all reach HUB at hop 1; HUB has D out-edges (p0 = i % 20,
    p1 = i) to leaves 1000 + i. flip: every edge reversed (for REVERSELY). two: HUB also has D edges of type f to
    leaves 2000 + i, and every root also points (type e) at SIDE, which has two edges of type f and none of type e.
    The input rows of a root are spread over the input (by duplicate, then by root) and differ in w (0 .. 19)."""
    mk = (lambda a, b, t, p: edge(b, a, t, 0, p)) if flip else (lambda a, b, t, p: edge(a, b, t, 0, p))
    edges = [mk(1 + j, HUB, 1, (j % 100, j, 0)) for j in range(CONVERGE_ROOTS)]
    edges += [mk(HUB, 1000 + i, 1, (i % 20, i, 0)) for i in range(D)]
    if two:
        edges += [mk(HUB, 2000 + i, 2, (i % 20, 100 + i, 0)) for i in range(D)]
        edges += [mk(1 + j, SIDE, 1, (j % 100, j, 1)) for j in range(CONVERGE_ROOTS)]
        edges += [mk(SIDE, 3000 + i, 2, (5 * i, 200 + i, 0)) for i in range(2)]
    mults = converge_mults(m_last)
    order = sorted((dup, j) for j in range(CONVERGE_ROOTS) for dup in range(mults[j]))
    rows = [input_row(1 + j, j, dup, w=(j * 5 + dup * 3) % 20) for dup, j in order]
    vids = {v for e_ in edges for v in e_[:2]}
    return Graph(vids, edges, types=[1, 2] if two else [1]), {"in": pipe_input(rows)}


# (the last root's input rows, D): sum of the multiplicities x D = K_CHUNK - 1, K_CHUNK, K_CHUNK + 1 and 128 x 17 (a
# chunk boundary inside one entry's run of 17 edges); the host test asserts the products
CONVERGE_SHAPES = {"below": (K_CHUNK - 1 - 126, 1), "exact": (2, 16), "above": (683 - 126, 3), "inside": (2, 17)}


def entries_graph(N, deg):
    """One vid (7) in N input rows with w = the row's number; its `deg` out-edges have p0 = N // 2, N, 0."""
    edges = [edge(7, 100 + i, 1, 0, ((N // 2, N, 0)[i], i, 0)) for i in range(deg)]
    rows = [(7, r % 1000, r, "s%d" % r, r * 0.5) for r in range(N)]
    return Graph([7] + [100 + i for i in range(deg)], edges), {"in": pipe_input(rows)}


def ring_graph():
    """A directed ring 1 -> 2 -> ... -> 5 -> 1 (p1 = the source, p0 = 10 x the source). Inputs: every vertex a root (two
    rows for vertex 2); roots 1 and 3 only."""
    edges = [edge(i, i % 5 + 1, 1, 0, (10 * i, i, 0)) for i in range(1, 6)]
    five = [input_row(i, i - 1, 0, w=7 * i) for i in range(1, 6)] + [input_row(2, 1, 1, w=0)]
    two = [input_row(1, 0, 0, w=15), input_row(3, 2, 0, w=0)]
    return Graph(range(1, 6), edges), {"five": pipe_input(five), "two": pipe_input(two)}


def dying_graph():
    """A live chain 1 -> 2 -> 3 -> {4, 6} -> 5; C = 10 -> 11 and 11 has no out-edge (its walk ends at hop 1 of 3);
    B = 20 has no edge at all; 999 and 3000 .. 3031 are no vertices; 4000 .. 4031 are vertices without edges; 70 roots
    5000 + j -> 2 join the chain. Inputs, in the order the queries use them: `mixed` (a dead vid, B, C and the live
    root in one batch, C and the live root twice), `dead_live` (a first batch of 64 roots that all die at hop 1 with no
    edge scanned, then three live ones), `many` (71 roots), `one`."""
    edges = [edge(1, 2, 1, 0, (50, 1, 0)), edge(2, 3, 1, 0, (60, 2, 0)), edge(3, 4, 1, 0, (70, 3, 0)),
             edge(3, 6, 1, 0, (5, 33, 0)), edge(4, 5, 1, 0, (80, 4, 0)), edge(6, 5, 1, 0, (90, 6, 0)),
             edge(10, 11, 1, 0, (40, 10, 0))]
    edges += [edge(5000 + j, 2, 1, 0, (j, 5000 + j, 0)) for j in range(70)]
    vids = {v for e_ in edges for v in e_[:2]} | {20} | {4000 + i for i in range(32)}
    mixed = [input_row(999, 0), input_row(20, 1), input_row(10, 2), input_row(1, 3), input_row(10, 2, 1), input_row(1, 3, 1, w=0)]
    dead = [3000 + i for i in range(32)] + [4000 + i for i in range(32)]
    dead_live = [input_row(v, j) for j, v in enumerate(dead)] + [input_row(1, 64, 0, w=0), input_row(5000, 65), input_row(5001, 66)]
    many = [input_row(5000 + j, j, 0, w=j) for j in range(70)] + [input_row(1, 70, 0, w=55)]
    return Graph(vids, edges), {"mixed": pipe_input(mixed), "dead_live": pipe_input(dead_live), "many": pipe_input(many),
                                "one": pipe_input([input_row(1, 0, 0, w=60)])}


ONEWALK_V = K_SEED_FUSE_MAX + 1


def onewalk_graph():
    """K_SEED_FUSE_MAX + 1 vertices, every one in the input, once or three times; one or two out-edges each."""
    N = ONEWALK_V
    keys = set()
    for i in range(N):
        keys.add((i + 1, i * 7 % N + 1))
        if i % 3 == 0:
            keys.add((i + 1, (i * 11 + 1) % N + 1))
    edges = [edge(a, b) for a, b in sorted(keys)]
    rows = [input_row(1 + j, j, dup) for dup in range(3) for j in range(N) if dup == 0 or j % 2]
    return Graph(range(1, N + 1), edges), {"in": pipe_input(rows)}


LONG_S = "".join(chr(33 + i) for i in range(63)).replace('"', "x").replace("\\", "y")


def columns_graph():
    """Three private paths; the vid column typed VID and typed INT; w at INT64_MIN, -1, 0 and INT64_MAX; an empty and a
    63-byte string; -0.0 and 0.0 as doubles."""
    g, _ = roots_graph(3)
    rows = [(1, 0, INT64_MIN, "", -0.0), (1, 1, -1, LONG_S, 0.0), (2, 2, 0, "a", 1.5), (2, 3, INT64_MAX, "b", -2.25),
            (3, 4, 2, "", 1e300), (3, 5, 3, LONG_S, -0.0)]
    assert len(LONG_S.encode()) == 63
    return g, {"vid": pipe_input(rows, kvfmt.VID), "int": pipe_input(rows, kvfmt.INT)}


# ---- the cases (tests/test_gpu_pipe_shapes.py on the device, tests/test_pipe_shapes_host.py against the oracle)
PQ = namedtuple("PQ", "form over direction m n inp")


def P(form, over=("e",), direction=FORWARD, m=None, n=2, inp="in"):
    return PQ(form, tuple(over), direction, m, n, inp)


# cap: max_edge_returned_per_vertex of the engine (0: unset); a cap makes the walks fall back (pipe_plan's fallback)
PipeCase = namedtuple("PipeCase", "build queries cap")
PIPE_CASES = {}
_pipe_built = {}


def pipe_case(name, build, queries, cap=0):
    assert name not in PIPE_CASES
    PIPE_CASES[name] = PipeCase(build, queries, cap)


def pipe_built(name):
    if name not in _pipe_built:
        _pipe_built[name] = PIPE_CASES[name].build()
    return _pipe_built[name]


def pipe_case_sentence(name, k):
    q = PIPE_CASES[name].queries[k]
    return pipe_sentence(q.form, q.over, q.direction, q.m, q.n)


def pipe_case_model(name, k):
    """Model(rows of `pipe`, hop_edges and hop_frontier of `pipe_plan`) of query k, computed once, and the walks."""
    if ("pipe", name, k) not in _models:
        g, inputs = pipe_built(name)
        q = PIPE_CASES[name].queries[k]
        plan = pipe_plan(g, q.form, inputs[q.inp], q.over, q.direction, q.m, q.n, PIPE_CASES[name].cap > 0)
        _models[("pipe", name, k)] = (Model(pipe(g, q.form, inputs[q.inp], q.over, q.direction, q.m, q.n), plan.hop_edges,
                                            plan.hop_frontier), plan.walks)
    return _models[("pipe", name, k)]


ROOT_COUNTS = (1, K_ROOT_BATCH - 1, K_ROOT_BATCH, K_ROOT_BATCH + 1, 2 * K_ROOT_BATCH, 2 * K_ROOT_BATCH + 1)
for _n in ROOT_COUNTS:
    pipe_case("roots%d" % _n, (lambda n: lambda: roots_graph(n))(_n), [P("all"), P("k"), P("w"), P("var"), P("all", m=1, n=2)])
for _name, (_m, _d) in CONVERGE_SHAPES.items():
    pipe_case("converge_" + _name, (lambda m, d: lambda: converge_graph(m, d))(_m, _d), [P("all"), P("w"), P("k")])
pipe_case("converge_reversely", lambda: converge_graph(1, 5, flip=True),
          [P("keys", direction=REVERSELY), P("w", direction=REVERSELY), P("keys", direction=REVERSELY, m=1, n=2)])
pipe_case("converge_bidirect", lambda: converge_graph(1, 5),
          [P("keys", direction=BIDIRECT), P("w", direction=BIDIRECT), P("k", direction=BIDIRECT, m=1, n=2)])
pipe_case("converge_two_types", lambda: converge_graph(1, 5, two=True),
          [P("two", "ef"), P("two", "fe"), P("all", "ef"), P("two", "ef", m=1, n=2)])
ENTRY_ROWS = (K_TILE - 1, K_TILE, K_TILE + 1)
for _n in ENTRY_ROWS:
    for _d in (1, 3):
        pipe_case("entries%d_deg%d" % (_n, _d), (lambda n, d: lambda: entries_graph(n, d))(_n, _d), [P("w", n=1), P("k", n=1)])
pipe_case("ring", ring_graph, [P(f, m=1, n=4, inp=i) for i in ("five", "two") for f in ("all", "k", "w")] +
          [P("k", n=4, inp="five"), P("all", n=3, inp="two")])
pipe_case("dying", dying_graph, [P(f, m=m, n=3, inp=i) for i in ("mixed", "dead_live", "many", "one")
                                 for f, m in (("all", None), ("w", None), ("k", 1))])
pipe_case("distinct_across", lambda: roots_graph(K_ROOT_BATCH + 1, {K_ROOT_BATCH: 0}, rotate=0), [P("all_d"), P("all"), P("k_d"), P("k")])
pipe_case("onewalk", onewalk_graph, [P("all", n=1), P("keys", direction=REVERSELY, n=1), P("keys", direction=BIDIRECT, n=1),
                                     P("all_d", n=1)])
pipe_case("columns", columns_graph, [P(f, inp=i) for i in ("vid", "int") for f in ("w", "k", "all")] + [P("w", n=1, inp="int")])
FALLBACK_CAP = 1000
pipe_case("fallback_roots", lambda: roots_graph(K_ROOT_BATCH + 1), [P("all"), P("w"), P("all_d"), P("k", m=1, n=2)], cap=FALLBACK_CAP)
pipe_case("fallback_converge", lambda: converge_graph(1, 5), [P("all"), P("w")], cap=FALLBACK_CAP)


# ---- shaped shards (tests/goshard_worker.py runs them by name, tests/test_gpu_pipe_shards.py checks them)
PipeShardCase = namedtuple("PipeShardCase", "world counts build queries")
PIPE_SHARD_CASES = {}
_pipe_shard_built = {}


def pipe_shard_case(name, counts, build):
    qs = [P(f, n=n) for f in ("all", "w") for n in (2, 3)]
    PIPE_SHARD_CASES[name] = PipeShardCase(len(counts), list(counts), build, qs)


def pipe_shard_built(name):
    """(Graph, {input name: Interim}, Shards) of a pipe shard case, built once."""
    if name not in _pipe_shard_built:
        _pipe_shard_built[name] = PIPE_SHARD_CASES[name].build()
    return _pipe_shard_built[name]


def pipe_shard_cases(world):
    return [n for n in PIPE_SHARD_CASES if PIPE_SHARD_CASES[n].world == world]


def pipe_shard_model(name, k):
    if ("pipeshard", name, k) not in _models:
        g, inputs, _ = pipe_shard_built(name)
        q = PIPE_SHARD_CASES[name].queries[k]
        plan = pipe_plan(g, q.form, inputs[q.inp], q.over, q.direction, q.m, q.n)
        _models[("pipeshard", name, k)] = (Model(pipe(g, q.form, inputs[q.inp], q.over, q.direction, q.m, q.n),
                                                 plan.hop_edges, plan.hop_frontier), plan.walks)
    return _models[("pipeshard", name, k)]


def xchg_roots_bytes(counts, rank):
    """exchangeRoots' share of lastXchgBytes: a 64-bit root set per row of every peer."""
    return sum(n * 8 for q, n in enumerate(counts) if q != rank)


def _placed(sh, paths, roots):
    """The graph of (q, i) -> (q, i) edges `paths` over every row of sh (rows without an edge stay vertices), p0 = the
    edge's number x 9 mod 100 and p1 its number; the input: roots [(q, i)] with 1, 2, 3 input rows in turn."""
    edges = [edge(sh.vid(*a), sh.vid(*b), 1, 0, (k * 9 % 100, k, 0)) for k, (a, b) in enumerate(paths)]
    g = Graph(sh.vids(), edges, types=[1])
    sh.check(g)
    order = sorted((dup, j) for j in range(len(roots)) for dup in range(1 + j % 3))
    return g, {"in": pipe_input([input_row(sh.vid(*roots[j]), j, dup) for dup, j in order])}, sh


def _w2_pipe():
    """World 2, counts [5, 70] (the merge's stride is 70, shard 0 has 5 rows). Ten roots on shard 1 reach the hub (0, 0),
    whose shard holds none of them; X = (1, 60) is reached at hop 1 by a root of its own shard and by one of the peer;
    (0, 2) -> (0, 3) stays on shard 0. The hub points at rows 20, 21 and 69 (the last) of shard 1."""
    sh = sharded([5, 70])
    roots = [(1, i) for i in range(10)] + [(0, 1), (1, 10), (0, 2)]
    paths = [((1, i), (0, 0)) for i in range(10)] + [((0, 1), (1, 60)), ((1, 10), (1, 60)), ((0, 2), (0, 3)),
             ((0, 0), (1, 20)), ((0, 0), (1, 21)), ((0, 0), (1, 69)), ((1, 60), (1, 22)), ((1, 60), (0, 4)), ((0, 3), (1, 23)),
             ((1, 20), (1, 30)), ((1, 21), (1, 31)), ((1, 69), (0, 4)), ((0, 4), (1, 32)), ((1, 22), (1, 33)), ((1, 23), (1, 34))]
    return _placed(sh, paths, roots)


def _w3_empty_pipe():
    """World 3, counts [3, 0, 66]: shard 1 has no row. Root A = (0, 0) -> (2, 5) -> (0, 1) -> (2, 6): shard 0 scans an edge
    on hop 1 and none on hop 2 of 3 STEPS. Root B = (2, 0) -> (2, 7) -> (2, 5): row (2, 5) is expanded by hop 2 for A and by
    hop 3 for B alone (a root set that shard 0 left over from hop 1 would add A's rows to hop 3's).
    (2, 5) -> (0, 1) and (2, 5) -> (2, 8); (2, 8) -> (2, 9). A third root, the last row of shard 2, walks down its shard."""
    sh = sharded([3, 0, 66])
    roots = [(0, 0), (2, 0), (2, 65)]
    paths = [((0, 0), (2, 5)), ((2, 0), (2, 7)), ((2, 7), (2, 5)), ((2, 5), (0, 1)), ((2, 5), (2, 8)), ((0, 1), (2, 6)),
             ((2, 8), (2, 9)), ((2, 65), (2, 64)), ((2, 64), (2, 63)), ((2, 63), (2, 62))]
    return _placed(sh, paths, roots)


def _w3_peers_pipe():
    """World 3, counts [3, 4, 66]: Y = (2, 65) is reached at hop 1 by a root of shard 0 and by a root of shard 1 (its
    root sets arrive from two peers), and by none of its own shard; Z = (1, 3) by roots of shards 0 and 2."""
    sh = sharded([3, 4, 66])
    roots = [(0, 0), (1, 0), (2, 0), (0, 1)]
    paths = [((0, 0), (2, 65)), ((1, 0), (2, 65)), ((0, 1), (1, 3)), ((2, 0), (1, 3)), ((2, 65), (2, 10)), ((2, 65), (0, 2)),
             ((1, 3), (2, 11)), ((2, 10), (1, 2)), ((0, 2), (2, 12)), ((2, 11), (2, 13))]
    return _placed(sh, paths, roots)


pipe_shard_case("pipe_w2", [5, 70], _w2_pipe)
pipe_shard_case("pipe_w3_empty", [3, 0, 66], _w3_empty_pipe)
pipe_shard_case("pipe_w3_peers", [3, 4, 66], _w3_peers_pipe)
