"""`goref.pipe` against the oracle, on the CPU: the model's authority for tests/test_gpu_pipe_shapes.py and
tests/test_gpu_pipe_shards.py.

For every graph, input and form the device tests use, at world 1 and for the shard cases' graphs, the model's rows
equal those of the oracle's back-tracker (Oracle.go(..., input=...)); the comparator, extended to strings and doubles,
fails on a dropped row, a doubled row, a cell off by 1 (a string one byte off, a double one bit off) and a hop count
off by 1; the new constants are read back from their headers; and the shapes the cases claim are asserted here, where
no GPU is needed: bits set at the hub, entries x D against kChunk, the rows per shard, the edges per shard and hop.
"""
import math
import os
import re

import pytest

from nebula_amd import ngql, pipeline
from oracle import oracle
from tests import goref

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nebula_amd", "csrc")


def _vs_oracle(g, inputs, queries, model_of, name):
    o = oracle.Oracle()
    try:
        space = goref.load_oracle(o, g)
        for k, q in enumerate(queries):
            text = goref.pipe_sentence(q.form, q.over, q.direction, q.m, q.n)
            ref = o.go(space, ngql.parse_go(text), input=inputs[q.inp])
            assert ref.ok, (name, text, ref.error)
            goref.assert_rows(ref.rows, model_of(k)[0].rows, (name, k, text, q.inp))
    finally:
        o.close()


@pytest.mark.parametrize("name", sorted(goref.PIPE_CASES))
def test_model_equals_oracle(name):
    g, inputs = goref.pipe_built(name)
    _vs_oracle(g, inputs, goref.PIPE_CASES[name].queries, lambda k: goref.pipe_case_model(name, k), name)


@pytest.mark.parametrize("name", sorted(goref.PIPE_SHARD_CASES))
def test_shard_model_equals_oracle(name):
    g, inputs, _ = goref.pipe_shard_built(name)
    _vs_oracle(g, inputs, goref.PIPE_SHARD_CASES[name].queries, lambda k: goref.pipe_shard_model(name, k), name)


def test_constants():
    assert (goref.K_ROOT_BATCH, goref.K_TILE) == (64, 4096)
    assert goref.CONSTANTS["kernels.h"]["kRootBatch"] == goref.K_ROOT_BATCH and goref.CONSTANTS["kargs.h"]["kTile"] == goref.K_TILE
    for header, k, v in (("kernels.h", "kRootBatch", goref.K_ROOT_BATCH), ("kargs.h", "kTile", goref.K_TILE)):
        m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)" % k, open(os.path.join(CSRC, header)).read())
        assert m and int(m.group(1)) == v, (header, k)
    eng = open(os.path.join(CSRC, "engine.cpp")).read()
    # runPipe batches by the named constant, and the (row, input row) entries' scan is tiled by kTile
    assert len(re.findall(r"b0 \+= kRootBatch\)", eng)) == 2 and not re.search(r"b0 \+= 64\b", eng)
    assert re.search(r"tileSums\.get<uint64_t>\(\(std::max<uint64_t>\(nEnt2, 1\) \+ kTile - 1\) / kTile \+ 1\)", eng)
    assert (goref.T_DOUBLE, goref.T_STRING) == (pipeline.T_DOUBLE, pipeline.T_STRING)


def test_comparator_notices():
    g, inputs = goref.pipe_built("columns")
    m = goref.Model(goref.pipe(g, "w", inputs["vid"], ["e"], n=2), [3, 3], [3, 3])
    assert len(m.rows) == 4 and {c[0] for r in m.rows for c in r} == {"int", "str", "double", "id"}
    goref.assert_same(m, m)
    goref.assert_same(goref.Model(list(reversed(m.rows)), m.hop_edges, m.hop_frontier), m)
    bad = [goref.Model(m.rows[:-1], m.hop_edges, m.hop_frontier),                  # one row dropped
           goref.Model(m.rows + [m.rows[1]], m.hop_edges, m.hop_frontier),         # one row twice
           goref.Model(m.rows, [3, 4], m.hop_frontier), goref.Model(m.rows, m.hop_edges, [3, 2])]   # a hop count off by 1
    for c, (kind, v) in enumerate(m.rows[2]):                                      # one cell of any column off by 1
        r = list(m.rows[2])
        r[c] = (kind, v + "x" if kind == "str" else math.nextafter(v, math.inf) if kind == "double" else v + 1)
        bad.append(goref.Model(m.rows[:2] + [tuple(r)] + m.rows[3:], m.hop_edges, m.hop_frontier))
    zero = [r for r in m.rows if r[2] == ("double", -0.0) and math.copysign(1, r[2][1]) < 0]
    assert zero                                                                    # -0.0 and 0.0 differ in their bits
    i = m.rows.index(zero[0])
    r = list(zero[0])
    r[2] = ("double", 0.0)
    bad.append(goref.Model(m.rows[:i] + [tuple(r)] + m.rows[i + 1:], m.hop_edges, m.hop_frontier))
    for b in bad:
        with pytest.raises(AssertionError):
            goref.assert_same(b, m)


def _masks(g, vids, hops):
    """{vertex: set of root indices} after `hops` FORWARD hops over e from vids[j] as root j, by the model's rule."""
    out = {}
    for j, v in enumerate(vids):
        for w in goref.hop_frontiers(g, [v], hops + 1)[hops]:
            out.setdefault(w, set()).add(j)
    return out


def _distinct(inp):
    return list(dict.fromkeys(r[0][1] for r in inp.rows))


def test_shapes_world1():
    for n in goref.ROOT_COUNTS:                                    # walks = ceil(R / 64), a root's bit is not its row
        g, inputs = goref.pipe_built("roots%d" % n)
        vids = _distinct(inputs["in"])
        assert len(vids) == n and goref.pipe_case_model("roots%d" % n, 0)[1] == (n + 63) // 64
        assert n < 6 or vids[0] == 6
        batch0 = vids[:64]
        assert all(len(s) == 1 for s in _masks(g, batch0, 2).values()) and (n < 64 or len(_masks(g, batch0, 1)) == 64)
    for name, (m_last, D) in goref.CONVERGE_SHAPES.items():
        g, inputs = goref.pipe_built("converge_" + name)
        vids = _distinct(inputs["in"])
        assert len(vids) == goref.K_ROOT_BATCH
        assert _masks(g, vids, 1) == {goref.HUB: set(range(64))}   # exactly 64 bits set at the hub
        entries = len(inputs["in"].rows)
        assert entries == sum(goref.converge_mults(m_last)) and g.out_degree(goref.HUB, [1]) == D
        assert entries * D == {"below": goref.K_CHUNK - 1, "exact": goref.K_CHUNK, "above": goref.K_CHUNK + 1,
                               "inside": goref.K_CHUNK + 128}[name]
        ws = {}
        for r in inputs["in"].rows:
            ws.setdefault(r[0][1], []).append(r[2][1])
        assert any(len(set(w)) > 1 for w in ws.values())           # duplicate vids carry different $-.w
        assert len(goref.pipe_case_model("converge_" + name, 0)[0].rows) == entries * D
    assert goref.K_CHUNK % 17 and (goref.K_CHUNK // 17) * 17 < goref.K_CHUNK < (goref.K_CHUNK // 17 + 1) * 17
    g, inputs = goref.pipe_built("converge_two_types")
    assert g.out_degree(goref.SIDE, [1]) == 0 and g.out_degree(goref.SIDE, [2]) == 2 and g.out_degree(goref.HUB, [2]) == 5
    for n in goref.ENTRY_ROWS:
        for d in (1, 3):
            g, inputs = goref.pipe_built("entries%d_deg%d" % (n, d))
            assert len(inputs["in"].rows) == n and _distinct(inputs["in"]) == [7] and g.out_degree(7, [1]) == d
            assert len({r[2][1] for r in inputs["in"].rows}) == n
    g, inputs = goref.pipe_built("ring")
    vids = _distinct(inputs["five"])
    for h in range(4):                                             # every hop: all five rows, one bit each, another each hop
        mk = _masks(g, vids, h)
        assert sorted(mk) == [1, 2, 3, 4, 5] and all(len(s) == 1 for s in mk.values())
        assert h == 0 or mk != _masks(g, vids, h - 1)
    assert [sorted(_masks(g, _distinct(inputs["two"]), h)) for h in range(3)] == [[1, 3], [2, 4], [3, 5]]
    g, inputs = goref.pipe_built("dying")
    dead = _distinct(inputs["dead_live"])[:64]
    assert len(dead) == 64 and all(g.out_degree(v, [1]) == 0 for v in dead) and sum(v in g.vids for v in dead) == 32
    assert 999 not in g.vids and 20 in g.vids and g.out_degree(20, [1]) == 0 and g.out_degree(11, [1]) == 0
    assert len(_distinct(inputs["many"])) == 71 and len(_distinct(inputs["one"])) == 1
    g, inputs = goref.pipe_built("distinct_across")
    vids = _distinct(inputs["in"])
    a, b = vids.index(1), vids.index(65)
    assert a // 64 != b // 64 and _masks(g, vids, 1)[10000] == {a, b}       # two batches, one hub
    rows = goref.pipe_case_model("distinct_across", 1)[0].rows
    assert rows.count((("id", 20000), ("int", 0))) == 2 and goref.pipe_case_model("distinct_across", 0)[0].rows.count(
        (("id", 20000), ("int", 0))) == 1
    g, inputs = goref.pipe_built("onewalk")
    assert len(_distinct(inputs["in"])) == goref.K_SEED_FUSE_MAX + 1 and len(inputs["in"].rows) > len(g.vids)
    assert all(goref.pipe_case_model("onewalk", k)[1] == 1 for k in range(4))
    g, inputs = goref.pipe_built("columns")
    assert {r[2][1] for r in inputs["vid"].rows} >= {goref.INT64_MIN, -1, 0, goref.INT64_MAX}
    assert {len(r[3][1]) for r in inputs["vid"].rows} >= {0, 63}
    assert inputs["vid"].types[0] != inputs["int"].types[0] and inputs["int"].rows[0][0][0] == "int"
    for name in ("fallback_roots", "fallback_converge"):           # the cap never binds; walks per vid / per input row
        g, inputs = goref.pipe_built(name)
        assert max(g.out_degree(v, [1]) for v in g.vids) < goref.PIPE_CASES[name].cap
        for k, q in enumerate(goref.PIPE_CASES[name].queries):
            n = len(inputs["in"].rows) if goref.PIPE_FORMS[q.form].reads else len(_distinct(inputs["in"]))
            assert goref.pipe_case_model(name, k)[1] == n


def test_shapes_shards():
    g, inputs, sh = goref.pipe_shard_built("pipe_w2")
    assert sh.counts == [5, 70]
    vids = _distinct(inputs["in"])
    m1 = _masks(g, vids, 1)
    hub, x = sh.vid(0, 0), sh.vid(1, 60)
    assert len(m1[hub]) == 10 and all(sh.where(vids[j])[0] == 1 for j in m1[hub])      # the hub's roots: all on the peer
    assert sorted(sh.where(vids[j])[0] for j in m1[x]) == [0, 1]                        # own | recv
    assert {sh.where(v)[0] for v in vids} == {0, 1}
    g, inputs, sh = goref.pipe_shard_built("pipe_w3_empty")
    assert sh.counts == [3, 0, 66] and sh.counts[1] == 0
    vids = _distinct(inputs["in"])
    fr = goref.hop_frontiers(g, vids, 3)
    per = [[sum(g.out_degree(v, [1]) for v in f if sh.where(v)[0] == q) for f in fr] for q in range(3)]
    assert per[0][0] > 0 and per[0][1] == 0 and per[0][2] > 0 and per[1] == [0, 0, 0]   # hop 2 has no edge on shard 0
    t = sh.vid(2, 5)
    assert _masks(g, vids, 1)[t] == {0} and _masks(g, vids, 2)[t] == {1}               # another root each time
    g, inputs, sh = goref.pipe_shard_built("pipe_w3_peers")
    vids = _distinct(inputs["in"])
    m1 = _masks(g, vids, 1)
    assert sorted(sh.where(vids[j])[0] for j in m1[sh.vid(2, 65)]) == [0, 1]            # from two peers, none of its own
    assert sorted(sh.where(vids[j])[0] for j in m1[sh.vid(1, 3)]) == [0, 2]
    assert goref.xchg_roots_bytes([5, 70], 0) == 560 and goref.xchg_roots_bytes([3, 0, 66], 2) == 24
