"""The shard cases of tests/goref.py on the CPU: what tests/test_gpu_go_shards.py relies on.

For every shard case: the model equals the oracle on every query (the oracle is one process; the whole graph is loaded
with the case's num_parts); the shards' CSR arrays / KV batches partition the graph (every vid on exactly one shard, the
slots' edges together the edge list with its in-rows) at the counts and offsets the case claims. The merged-rows
comparator is shown to fail on a dropped row, a doubled row, a cell off by 1 and a hop_edges sum off by 1, and to pass
when a row moves to another shard. The hop_xchg formulas are checked on hand-computed values.
"""
import pytest

from nebula_amd import ngql
from oracle import oracle
from tests import goref

NAMES = sorted(goref.SHARD_CASES)


def test_placement_rule():
    assert [goref.part_of(v, 3) for v in (0, 1, 2, 3, 4)] == [1, 2, 3, 1, 2]
    assert [goref.shard_of(v, 3, 3) for v in (0, 1, 2, 3, 4)] == [1, 2, 0, 1, 2]
    assert goref.part_of(-1, 7) == ((1 << 64) - 1) % 7 + 1          # the vid as an unsigned number
    assert goref.shard_of(5, 100, 8) == (5 % 100 + 1) % 8
    sh = goref.sharded([3, 0, 2], {1: 3, 2: 3}, 5)
    assert sh.base == [0, 3, 3, 5] and sh.vglobal == 5
    assert [sh.vid(0, i) for i in range(3)] == [5, 8, 11] and [sh.vid(2, i) for i in range(2)] == [4, 7]
    assert all(goref.shard_of(sh.vid(q, i), 3, 3) == q and sh.where(sh.vid(q, i)) == (q, i)
               for q in range(3) for i in range(sh.counts[q]))
    with pytest.raises(AssertionError):
        goref.sharded([3, 0, 2], {2: 4})
    with pytest.raises(AssertionError):                             # a graph placed by another rule fails on the host
        goref.Shards([2, 2]).check(goref.Graph([2, 3, 4, 6], []))


@pytest.mark.parametrize("name", NAMES)
def test_model_equals_oracle(name):
    case = goref.SHARD_CASES[name]
    g, _, sh = goref.shard_built(name)
    o = oracle.Oracle()
    try:
        space = goref.load_oracle(o, g, num_parts=sh.num_parts)
        for k, sq in enumerate(case.queries):
            text = goref.shard_sentence(name, k)
            ref = o.go(space, ngql.parse_go(text), pushdown=sq.q.pushdown)
            assert ref.ok, (text[:200], ref.error)
            goref.assert_same(ref, goref.shard_model(name, k), (name, k, sq.q.form))
    finally:
        o.close()


@pytest.mark.parametrize("name", NAMES)
def test_shards_partition_the_graph(name):
    case = goref.SHARD_CASES[name]
    g, _, sh = goref.shard_built(name)
    assert sh.world == case.world and sh.counts == case.counts and sh.num_parts == sh.world
    tables, base = goref.shard_tables(g, sh.num_parts, sh.world, goref.kv_vertices(g) if case.kv else None)
    assert [len(t) for t in tables] == case.counts and base == sh.base
    assert sorted(v for t in tables for v in t) == g.vids           # every vid on exactly one shard
    want = sorted([(a, t, r, b, p) for a, b, t, r, p in g.edges] + [(b, -t, r, a, p) for a, b, t, r, p in g.edges])
    if case.kv:
        whole = goref.kv_batch(g, sh.num_parts)
        keys, ko, _, _ = whole.arrays()
        parts = [int.from_bytes(bytes(keys[ko[i]:ko[i] + 4]), "little", signed=True) >> 8 for i in range(len(ko) - 1)]
        assert len(parts) == 2 * len(g.edges) + len(g.tags) and set(parts) <= set(range(1, sh.num_parts + 1))
        per = [sum(1 for p in parts if p % sh.world == q) for q in range(sh.world)]
        rows = [sum(1 for a, b, _, _, _ in g.edges for v in (a, b) if sh.where(v)[0] == q) +
                sum(1 for v in g.tags if sh.where(v)[0] == q) for q in range(sh.world)]
        assert per == rows                                          # each shard keeps the rows of its own vertices
        return
    got = []
    for rank in range(sh.world):
        vpart, vid, slots = goref.csr_slots(g, rank, sh.world, sh.num_parts)
        assert vid.tolist() == tables[rank] and vpart.tolist() == [goref.part_of(v, sh.num_parts) for v in tables[rank]]
        assert all(p % sh.world == rank for p in vpart.tolist())
        assert [s[0] for s in slots] == [1, -1]
        for st, off, dst, cols, rk in slots:
            assert len(off) == len(vid) + 1 and off[0] == 0 and off[-1] == len(dst)
            for i, v in enumerate(vid.tolist()):
                for e in range(int(off[i]), int(off[i + 1])):
                    got.append((v, st, int(rk[e]), int(dst[e]), tuple(int(c[e]) for c in cols)))
    assert sorted(got) == want


def _merged_fixture():
    g, seeds, sh = goref.shard_built("forms_w2")
    m = goref.shard_model("forms_w2", 0)
    rows = [list(m.rows[:3]), list(m.rows[3:])]
    edges = [[5, 1], [3, 3]]
    assert len(m.rows) == 4 and m.hop_edges == [8, 4]
    return m, rows, edges


def test_merged_comparator_notices():
    m, rows, edges = _merged_fixture()
    goref.assert_merged(rows, edges, m)
    goref.assert_merged([rows[0][:-1], rows[1] + rows[0][-1:]], edges, m)          # a row on another shard: order-free
    goref.assert_merged([rows[1], rows[0]], [edges[1], edges[0]], m)
    goref.assert_merged([rows[0] + rows[0][:1], rows[1]], edges, m, distinct=True)  # DISTINCT applies to the merged rows
    cell = list(rows[1][0])
    cell[1] = (cell[1][0], cell[1][1] + 1)
    bad = [
        ([rows[0][:-1], rows[1]], edges),                                           # a dropped row
        ([rows[0], rows[1] + rows[0][:1]], edges),                                  # a doubled row, on another shard
        ([rows[0], [tuple(cell)] + rows[1][1:]], edges),                            # a cell off by 1
        (rows, [[5, 1], [3, 4]]),                                                   # a hop_edges sum off by 1
        (rows, [[5, 1], [2, 3]]),
        (rows, [[5, 1, 1], [3, 3]]),                                                # a hop the model does not have
    ]
    for r, e in bad:
        with pytest.raises(AssertionError):
            goref.assert_merged(r, e, m)
    with pytest.raises(AssertionError):
        goref.assert_merged([rows[0][:-1], rows[1]], edges, m, distinct=True)


def bitmap_bytes(counts, rank):
    """Σ over the peers q of ceil(rows_q / 64) * 8 (exchangeFrontier's lastXchgBytes)."""
    return sum(-(-n // 64) * 8 for q, n in enumerate(counts) if q != rank)


def list_bytes(world, sent):
    """(W - 1) * W * 8 + 4 * (rows this rank sent) (exchangeFrontierList's lastXchgBytes)."""
    return (world - 1) * world * 8 + 4 * sent


def test_xchg_formulas_by_hand():
    assert bitmap_bytes([8, 65], 0) == 16 and bitmap_bytes([8, 65], 1) == 8 and bitmap_bytes([8, 64], 0) == 8
    assert bitmap_bytes([3, 1, 0, 60, 1, 64, 5, 70], 0) == 8 + 0 + 8 + 8 + 8 + 8 + 16
    assert bitmap_bytes([3, 1, 0, 60, 1, 64, 5, 70], 7) == 8 + 8 + 0 + 8 + 8 + 8 + 8
    assert list_bytes(2, 0) == 16 and list_bytes(2, 4097) == 16 + 16388 and list_bytes(3, 3) == 48 + 12
    for counts in ([8, 65], [8, 64], [66, 0, 130], [3, 1, 0, 60, 1, 64, 5, 70]):
        for r in range(len(counts)):
            assert goref.xchg_bitmap_bytes(counts, r) == bitmap_bytes(counts, r)
    assert goref.xchg_list_bytes(3, 3) == 60 and goref.xchg_list_bytes(8, 0) == 448
    assert goref.xchg_pull_bytes([63, 128]) == 16 and goref.xchg_pull_bytes([3, 1, 0, 60, 1, 64, 5, 70]) == 2 * 8 * 7
    # rows_sent on a case computed by hand: the sender of shard 0 marks 3 rows of shard 1, the one of shard 2 three,
    # shard 1's own sender none outside its shard
    g, seeds, sh = goref.shard_built("bitmap_w3_triple")
    assert [goref.rows_sent(g, sh, seeds, 1, r) for r in range(3)] == [3, 0, 3]
    g, seeds, sh = goref.shard_built("list_w3_two_senders")
    assert [goref.rows_sent(g, sh, seeds, 1, r) for r in range(3)] == [4000, 0, 3]


def test_case_claims():
    """What the cases' names claim, asserted from the built graphs."""
    for n in goref.BITMAP_N:
        assert goref.SHARD_CASES["bitmap_w2_%d" % n].counts == [8, n]
    assert set(goref.BITMAP_N) == {1, 63, 64, 65, 255, 256, 257, 4097}
    assert set(goref.LIST_N) == {1, 1023, 1024, 1025, 4095, 4096, 4097, 2 * 4096 + 1}
    for n in goref.LIST_N:                                           # the `all` query fills the list up to cap
        g, _, sh = goref.shard_built("list_w2_%d" % n)
        assert goref.rows_sent(g, sh, [sh.vid(0, 4)], 1, 0) == n and (n < 8 or max(sh.counts) == n)
        assert goref.rows_sent(g, sh, [sh.vid(0, 0)], 1, 0) == 0
    E = goref.AUTO_E
    assert min(goref.SHARD_CASES["auto_w2_bitmap"].counts) == 32 * E and min(goref.SHARD_CASES["auto_w2_list"].counts) == 32 * E + 1
    for name in ("auto_w2_bitmap", "auto_w2_list"):
        assert goref.shard_model(name, 0).hop_edges[0] == E
    for name, (counts, base_mod, vmod) in goref.PULL_SHAPES.items():
        g, seeds, sh = goref.shard_built(name)
        front = {sh.where(v) for v in goref.hop_frontiers(g, seeds, 2)[1]}
        for q, n in enumerate(counts):                               # the first and the last row of every shard
            assert n == 0 or {(q, 0), (q, n - 1)} <= front, (name, q)
        for k in (0, 1):
            assert goref.pulled(goref.shard_model(name, k), goref.SHARD_CASES[name].queries[k].q, 1, sh.vglobal) == [1, 2]
        assert goref.pulled(goref.shard_model(name, 2), goref.SHARD_CASES[name].queries[2].q, goref.shard_flags(name, 2)["pull_factor"],
                            sh.vglobal) == [2]
    assert {b & 63 for name, (c, _, _) in goref.PULL_SHAPES.items() for b in goref.Shards(c).base[1:-1]} >= {0, 1, 63}
    sh = goref.Shards(goref.PULL_SHAPES["pull_w2_base63"][0])        # the largest shard's last row: last bit of its last word
    assert sh.counts[1] % 64 == 0 and sh.counts[1] == max(sh.counts) and sh.base[1] & 63
    sh = goref.Shards(goref.W8_COUNTS)                               # output word 0: shards 0, 1, (2,) 3, 4 and a row of 5
    assert [b for b in sh.base if b < 64] == [0, 3, 4, 4, 62, 63] and sh.base[6] > 64
