"""The dense final hop with the edge-column loads first (final_kernels.h finalBodyDense, flag
dense_early_loads) against the oracle.

An eligible generated kernel (one OVER type, no src row read, single-load YIELD columns) computes its 8
CSR positions from blockIdx alone, issues every column load, and only then builds the chunk's frontier
bits from the rows' marks (dense_mask.h). Each case runs with the flag at 1 and at 0; the read-only
counter dense_early_finals proves which kernel ran, and rows, hop statistics and errors equal the oracle's.

The graphs are hand-built CSRs loaded through ngx_load_csr (out slot e, its exact mirror -e so hop 1 can be
pulled, one part), so slot sizes, chunk boundaries and row layouts are exact; the oracle gets the same
edges as KV rows. Row r is vid r + 1. Every query is GO 2 STEPS: hop 1 (pulled: pull_factor 1) marks the
frontier, the final hop covers every CSR position of slot e.
"""
import random

import numpy as np
import pytest

from nebula_amd import datagen, engine, kvfmt, ngql
from oracle import oracle
from tests import fixtures

pytestmark = pytest.mark.gpu

CE = 2048
SPACE = 7
SCHEMA = [fixtures.SchemaDef(True, 1, "e", [("p0", kvfmt.INT), ("p1", kvfmt.INT)])]


class CsrGraph:
    """adj[r] = sorted distinct dst rows of row r; props[(r, d)] = (p0, p1), default from a hash."""

    def __init__(self, adj, props=None):
        self.adj = [sorted(a) for a in adj]
        self.V = len(adj)
        self.props = props or {}

    def prop(self, r, d):
        if (r, d) in self.props:
            return self.props[(r, d)]
        h = (r * 2654435761 + d * 40503 + 17) & 0xFFFFFFFF
        return h % 100, (h * 6364136223846793005 + 1442695040888963407) % (1 << 62) - (1 << 61)

    def edges(self):
        return sum(len(a) for a in self.adj)

    def _slot(self, etype, lists, key):
        off, dst, p0, p1 = [0], [], [], []
        for r, a in enumerate(lists):
            # a row's edges in key order: by the little-endian bytes of the dst vid
            for d in sorted(a, key=lambda d: (d + 1).to_bytes(8, "little")):
                x = self.prop(*key(r, d))
                dst.append(d + 1)
                p0.append(x[0])
                p1.append(x[1])
            off.append(len(dst))
        return (etype, np.array(off, np.uint64), np.array(dst, np.int64),
                [np.array(p0, np.int64), np.array(p1, np.int64)])

    def load_engine(self, e):
        e.add_space(SPACE, 1)
        for s in SCHEMA:
            e.add_schema(SPACE, s.is_edge, s.sid, s.name, s.fields)
        rev = [[] for _ in range(self.V)]
        for r, a in enumerate(self.adj):
            for d in a:
                rev[d].append(r)
        out = self._slot(1, self.adj, lambda r, d: (r, d))
        inn = self._slot(-1, rev, lambda r, d: (d, r))
        e.load_csr(SPACE, np.ones(self.V, np.int32), np.arange(1, self.V + 1, dtype=np.int64), [out, inn])
        e.commit(SPACE)

    def load_oracle(self, o):
        b = kvfmt.KVBatch()
        for r, a in enumerate(self.adj):
            for d in a:
                row = kvfmt.encode_row([kvfmt.INT, kvfmt.INT], list(self.prop(r, d)))
                b.put(kvfmt.edge_key(1, r + 1, 1, 0, d + 1), row)
                b.put(kvfmt.edge_key(1, d + 1, -1, 0, r + 1), row)
        fixtures.Dataset(SPACE, 1, SCHEMA, b).load_oracle(o)


Q_BENCH = "GO 2 STEPS FROM {S} OVER e WHERE e.p0 < 50 YIELD e._dst, e._rank, e.p0, e.p1"
Q_ALL = "GO 2 STEPS FROM {S} OVER e YIELD e._dst, e.p1"
Q_MOD = "GO 2 STEPS FROM {S} OVER e WHERE e.p1 % e.p0 == 1 YIELD e._dst, e.p0"
Q_DIV0 = "GO 2 STEPS FROM {S} OVER e WHERE e.p1 % (e.p0 - e.p0) > 1 YIELD e._dst"
Q_SRC = "GO 2 STEPS FROM {S} OVER e WHERE e.p0 < 50 YIELD e._src, e._dst, e.p0"


def check(g, queries, seeds, early_expected=True, flags=(1, 0), engine_flags=None, expect_ok=None, pushdown=True,
          host_rows=False):
    """Each query with dense_early_loads 1 and 0 on one engine: the oracle's outcome, rows and statistics;
    the dense final hop ran, on the kernel the flag selects."""
    o = oracle.Oracle()
    g.load_oracle(o)
    e = engine.Engine(0)
    try:
        for k, v in (engine_flags or {}).items():
            e.set_flag(k, v)
        g.load_engine(e)
        assert e.info(SPACE).edges >= g.edges()
        e.set_flag("pull_factor", 1)
        assert e.get_flag("dense_early_loads") == 1                    # the default
        for q in queries:
            s = ngql.parse_go(q.replace("{S}", ", ".join(str(v + 1) for v in seeds)))
            ref = o.go(SPACE, s, pushdown=pushdown)
            if expect_ok is not None:
                assert ref.ok == expect_ok, (q, ref.error)
            # the YIELD columns alone are the device result (yield_only: no src row array, as the bench), every
            # column an integer: compared by the digest of the rows (src column: zeros)
            ncol = len(s.yields)
            want = oracle.row_digest([np.zeros(len(ref.rows), np.int64)] +
                                     [np.array([int(r[c][1]) for r in ref.rows], dtype=np.int64) for c in range(ncol)])
            prep = e.prepare_go(SPACE, s, pushdown=pushdown, on_device=True, yield_only=True,
                                compact=(queries.index(q) % 2 == 0))
            for flag in flags:
                e.set_flag("dense_early_loads", flag)
                d0, x0 = e.get_flag("dense_finals"), e.get_flag("dense_early_finals")
                # host_rows: the rows decoded on the host instead (with their src / dst / rank arrays)
                got = e.go(SPACE, s, pushdown=pushdown) if host_rows else e.go(SPACE, prep, rows=False, device_digest=True)
                dense, early = e.get_flag("dense_finals") - d0, e.get_flag("dense_early_finals") - x0
                assert dense == 1, (q, flag, e.jit_note())
                assert early == (1 if flag and early_expected else 0), (q, flag, e.jit_note())
                if early:
                    assert e.get_flag("jit_dense_scratch") == 0
                assert got.ok == ref.ok, (q, flag, got.error, ref.error)
                if not ref.ok:
                    continue
                assert got.hop_edges == ref.hop_scanned, (q, flag)
                assert got.hop_frontier == ref.hop_frontier, (q, flag)
                if host_rows:
                    assert fixtures.normalize_cells(got.rows) == fixtures.normalize_cells(ref.rows), (q, flag)
                else:
                    assert got.nrows == len(ref.rows) and tuple(got.device_digest) == tuple(want), (q, flag)
    finally:
        e.set_flag("poison_buffers", 0)
        e.close()
        o.close()


def slot_of(n, seed):
    """A slot of exactly n edges: row 0 (the seed) points at every other row among the first ones, the rest
    of the edges are spread over rows of random degrees."""
    rnd = random.Random(seed)
    if n == 1:
        return CsrGraph([[0], []]), [0]
    V = max(n // 6, 40)
    adj = [[] for _ in range(V)]
    adj[0] = list(range(0, min(V, 120), 2))[:n - 1]
    left = n - len(adj[0])
    r = 1
    while left:
        d = min(left, rnd.choice([0, 0, 1, 2, 3, 7, 19, 64, 300]), V)
        adj[r % V] = sorted(set(adj[r % V]) | set(rnd.sample(range(V), d)))
        left = n - sum(len(a) for a in adj)
        r += 1
    return CsrGraph(adj), [0]


@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 3 * 2048 + 5])
def test_slot_sizes(n):
    """(a) the last chunk holds 1, 2047, 2048 (none partial), 1 and 5 edges: no load leaves the slot."""
    g, seeds = slot_of(n, 31 + n)
    assert g.edges() == n
    check(g, [Q_BENCH, Q_ALL], seeds)


def supernode_graph(inside):
    """Rows 0-9 of degree 1, row 10 of degree 5000 (CSR positions 10 .. 5009: chunks 0, 1, 2), rows 11-20 of
    degree 1; the seed is the last row and points at degree-1 rows on both sides, zero-degree rows and,
    with `inside`, the supernode."""
    V = 5200
    adj = [[] for _ in range(V)]
    for r in list(range(10)) + list(range(11, 21)):
        adj[r] = [(r * 37) % 5000 + 21]
    adj[10] = list(range(100, 5100))
    front = [1, 3, 5, 8, 9, 11, 12, 15, 20] + list(range(5100, 5160))
    adj[V - 1] = sorted(front + ([10] if inside else []))
    return CsrGraph(adj), [V - 1]


@pytest.mark.parametrize("inside", [True, False])
def test_supernode_across_three_chunks(inside):
    """(b)"""
    g, seeds = supernode_graph(inside)
    check(g, [Q_BENCH, Q_ALL], seeds)


def test_supernode_with_poisoned_scratch():
    """(b) once more on an engine whose scratch buffers are filled with 0xA5 (tests/test_gpu_poison.py):
    the kernel reads no word that nothing wrote."""
    for inside in (True, False):
        g, seeds = supernode_graph(inside)
        check(g, [Q_BENCH], seeds, engine_flags={"poison_buffers": 1})


def test_many_small_rows():
    """(c) 3000 rows of degree 1 to 3 with 700 zero-degree rows in the middle: chunks of more than 256 rows
    (the strided row loop), every third row in the frontier."""
    rnd = random.Random(5)
    V = 3000 + 700 + 1
    adj = [[] for _ in range(V)]
    rows = list(range(1500)) + list(range(2200, 3700))
    for r in rows:
        adj[r] = rnd.sample(range(V - 1), rnd.randrange(1, 4))
    adj[V - 1] = rows[::3] + list(range(1500, 2200, 50))
    g = CsrGraph(adj)
    assert max(len(a) for a in adj[:V - 1]) <= 3 and g.edges() - len(adj[V - 1]) > 2 * CE
    check(g, [Q_BENCH, Q_ALL], [V - 1])


def error_graph(bad_inside):
    """200 rows of degree 30. Edges of the rows r % 4 == 0 have p0 = 0 (e.p1 % e.p0 fails on them), all
    others p0 in 1 .. 99; the frontier is the rows r % 4 == 1, plus with `bad_inside` two of the failing rows."""
    V = 201
    rnd = random.Random(77)
    adj = [rnd.sample(range(V - 1), 30) for _ in range(V - 1)] + [[]]
    props = {}
    for r in range(V - 1):
        for d in adj[r]:
            props[(r, d)] = (0 if r % 4 == 0 else 1 + (r * 7 + d) % 99, r * 1000 + d)
    adj[V - 1] = [r for r in range(V - 1) if r % 4 == 1] + ([8, 120] if bad_inside else [])
    for d in adj[V - 1]:
        props[(V - 1, d)] = (5, 11)
    return CsrGraph(adj, props), [V - 1]


def test_filter_error_outside_the_frontier():
    """(d) a WHERE that fails only on edges of rows outside the frontier: the query succeeds; with such rows
    inside the frontier it fails as the oracle's does. Without pushdown: graphd evaluates the WHERE (a pushed
    filter that fails on an edge only drops it)."""
    g, seeds = error_graph(False)
    check(g, [Q_MOD], seeds, expect_ok=True, pushdown=False)
    g, seeds = error_graph(True)
    check(g, [Q_MOD], seeds, expect_ok=False, pushdown=False)


def test_division_by_zero_everywhere():
    """(d) e.p1 % (e.p0 - e.p0) fails on every edge it is evaluated for: a frontier of rows without out-edges
    evaluates it for none (success, no rows), any other frontier fails (graphd's WHERE: no pushdown)."""
    V = 300
    adj = [[] for _ in range(V)]
    for r in range(100):
        adj[r] = [(r * 13 + k) % 100 for k in range(0, 40, 3)]
    adj[V - 1] = list(range(150, 160))                     # zero-degree rows only
    check(CsrGraph(adj), [Q_DIV0], [V - 1], expect_ok=True, pushdown=False)
    adj[V - 1] = list(range(150, 160)) + [42]
    check(CsrGraph(adj), [Q_DIV0], [V - 1], expect_ok=False, pushdown=False)


def test_ineligible_shape_keeps_the_generic_kernel():
    """(f) e._src, or host rows with their src array, need the src row: the module has no loads-first kernel,
    the counter does not move, the rows are the oracle's."""
    g, seeds = slot_of(2049, 9)
    check(g, [Q_SRC, Q_BENCH], seeds, early_expected=False, host_rows=True)


def test_bench_layout():
    """(e) the bench query on RmatDataset(12) with the bench's placement (on_device, compact, yield_only),
    compared by device digest, alone and through go_batch of 6 plans, flag on and off."""
    ds = fixtures.RmatDataset(12, with_in=True)
    o = oracle.Oracle()
    o.set_flags(threads=8)
    ds.load_oracle(o)
    seeds = datagen.sample_vids(1799, 1 << ds.scale, 60)
    s = ngql.parse_go(f"GO 3 STEPS FROM {', '.join(str(int(v)) for v in seeds)} OVER e WHERE e.p0 < 50 "
                      "YIELD e._dst, e._rank, e.p0, e.p1")
    ref = o.go(ds.space, s)
    o.close()
    cols = [np.array([int(r[c][1]) for r in ref.rows], dtype=np.int64) for c in range(4)]
    want = oracle.row_digest([np.zeros(len(ref.rows), np.int64)] + cols)
    with engine.Engine(0) as e:
        ds.load_engine(e)
        e.set_flag("pull_factor", 1)
        prep = e.prepare_go(ds.space, s, on_device=True, compact=True, yield_only=True)
        for flag in (1, 0):
            e.set_flag("dense_early_loads", flag)
            x0 = e.get_flag("dense_early_finals")
            r = e.go(ds.space, prep, rows=False, device_digest=True)
            assert r.ok and r.hop_edges == ref.hop_scanned and tuple(r.device_digest) == tuple(want), flag
            assert r.hop_frontier == ref.hop_frontier
            assert e.get_flag("dense_early_finals") - x0 == flag
            got = e.go_batch([prep] * 6, digests=True)
            assert all(g[0] == 0 and tuple(g[3]) == tuple(want) for g in got), flag
            assert e.get_flag("dense_early_finals") - x0 == 7 * flag
        # the loads-first kernel stays inside the generic kernel's register budget (5 waves per SIMD, no scratch)
        assert 0 < e.get_flag("jit_dense_vgprs") <= 96          # 512 / 5 waves, in granules of 8
        assert e.get_flag("jit_dense_scratch") == 0 and e.get_flag("jit_scratch") == 0
