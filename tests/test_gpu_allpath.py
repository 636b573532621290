"""FIND ALL PATH and FIND NOLOOP PATH on the device (flag find_path_all; nebula_amd/csrc/findpath.hip k_path_walk,
op_findpath.cpp::findAllPaths) against the model of tests/allref.py, which shares nothing with them.

Every device case calls Engine.find_path(..., rows=False) and compares the (layer, src, dst, type, rank, mask) tuples
with the model's layered DAG as sets, asserts that none occurs twice, and compares `found`, `levels` and the stat
find_path_layers with the model. Where the model counts at most 5,000 walks the rendered rows of both kinds are
compared with the model's depth-first walks too. The reference's FindPathTest answers run through the pipeline with
the flag at 1 (device) and at 0 (the refusal and the host restatement, as before the flag existed).
"""
import random

import pytest

from nebula_amd import engine, pipeline
from oracle import oracle
from tests import allref as A
from tests import fixtures
from tests import pathref as P
from tests.golden.findpath_cases import CASES
from tests.test_findpath_host import check_golden, golden_text

pytestmark = pytest.mark.gpu

K_PATH_BUF = 1024                                                 # kernels.h: kPathBuf
MAX_ROWS = 5000
NBA_EDGES = ["serve", "like", "teammate"]
GOLDEN = [c for c in CASES if c["kind"] in ("ALL", "NOLOOP") and c["direction"] != "BIDIRECT" and not c.get("error")]


@pytest.fixture(scope="module")
def eng():
    with engine.Engine() as e:
        assert e.get_flag("find_path_all") == 0
        e.set_flag("find_path_all", 1)
        yield e


def device_layers(e, space, q):
    """({(layer, src, dst, type, rank, mask)}, found, levels, layers launched) of the sentence on the device."""
    before, layers = e.get_flag("find_path_device"), e.get_flag("find_path_layers")
    r = e.find_path(space, q, rows=False)
    assert r.ok, r.error
    assert e.get_flag("find_path_device") == before + 1
    src, dst, typ, rank, mask, layer = r.dev_cols
    assert len(src) == len(dst) == len(typ) == len(rank) == len(mask) == len(layer) == r.go_nrows
    tuples = [(int(layer[i]), int(src[i]), int(dst[i]), int(typ[i]), int(rank[i]), int(mask[i])) for i in range(len(src))]
    assert len({t[:5] for t in tuples}) == len(tuples), "a (layer, edge) pair was emitted twice"
    return set(tuples), r.path_found, r.hop_frontier[0], e.get_flag("find_path_layers") - layers


def device_rows(e, space, q):
    before = e.get_flag("find_path_device")
    r = e.find_path(space, q)
    assert r.ok, r.error
    assert e.get_flag("find_path_device") == before + 1 and r.nrows == len(r.rows)
    return sorted(row[0][1] for row in r.rows)


def check(e, space, edges, vids, sources, targets, over, reversely, upto, rows=True):
    """The ALL sentence's layered edge set (NOLOOP's is the same call) and both kinds' rows against the model."""
    types = [P.TYPE_OF[n] for n in over]
    dag = A.layered_dag(edges, sources, targets, types, reversely, upto, vids)
    depths, layers = A.levels(edges, sources, targets, types, reversely, upto, vids)
    q = A.sentence("ALL", sources, targets, over, reversely, upto)
    got, found, levels, launched = device_layers(e, space, q)
    want = {k + (m,) for k, m in dag.items()}
    assert got == want, (q, sorted(got - want)[:5], sorted(want - got)[:5])
    assert found == A.found(dag, targets), (q, bin(found))
    assert (levels, launched) == (depths + layers, layers), (q, levels, launched, depths, layers)
    if rows and A.count(dag, sources, targets) <= MAX_ROWS:
        for kind, simple in (("ALL", False), ("NOLOOP", True)):
            model = sorted(A.render(w, P.NAME_OF) for w in A.walks(edges, sources, targets, types, reversely, upto, simple, vids))
            assert device_rows(e, space, A.sentence(kind, sources, targets, over, reversely, upto)) == model, (kind, q)
    return dag


# ----------------------------------------------------------------------------- the reference's answers
@pytest.fixture(scope="module")
def nba():
    ds = fixtures.nba()
    with engine.Engine() as e:
        ds.load_engine(e)
        yield ds, e


@pytest.mark.parametrize("case", GOLDEN, ids=[f"path{c['line']}" for c in GOLDEN])
def test_known_answers_on_the_device(nba, case):
    ds, e = nba
    e.set_flag("find_path_all", 1)
    try:
        before = e.get_flag("find_path_device")
        p = pipeline.Pipeline(e, ds.space, NBA_EDGES, find_path=True)
        check_golden(case, p.run(golden_text(case["query"])))
        assert p.find_path_fallbacks == 0 and e.get_flag("find_path_device") == before + 1
    finally:
        e.set_flag("find_path_all", 0)


@pytest.mark.parametrize("case", GOLDEN, ids=[f"path{c['line']}" for c in GOLDEN])
def test_known_answers_with_the_flag_off(nba, case):
    ds, e = nba
    assert e.get_flag("find_path_all") == 0
    before = e.get_flag("find_path_device")
    p = pipeline.Pipeline(e, ds.space, NBA_EDGES, find_path=True)
    check_golden(case, p.run(golden_text(case["query"])))
    assert p.find_path_fallbacks == 1 and p.find_path_refusal == "find path: ALL and NOLOOP enumerate walks, not levels"
    assert e.get_flag("find_path_device") == before


def test_flag_range(eng):
    for bad in (-1, 2):
        with pytest.raises(engine.EngineError, match="find_path_all"):
            eng.set_flag("find_path_all", bad)
    assert eng.get_flag("find_path_all") == 1


# ----------------------------------------------------------------------------- seeded graphs
SEEDS = tuple(range(12))
NV = 150
UPTOS = (1, 2, 3, 4, 8)
_cases = {}


def seeded(seed):
    """allref.random_graph(seed, 150) with two out-edges a vertex on average, 1 .. 3 sources and 1 .. 64 targets
    (seeds 0 and 1: all 64, so bit 63 occurs). The first source is a of the graph's 3-cycle a -> b -> c -> a and the
    first targets are b and c, so either direction has walks that come back to a target. Odd seeds list a vid
    without a vertex on each side and are loaded into 7 parts."""
    if seed not in _cases:
        g = A.random_graph(seed, NV, fanout=(1, 2, 2, 2, 3))
        rng = random.Random(500 + seed)
        n_s = rng.randint(1, 3)
        n_t = 64 if seed < 2 else 1 if seed == 2 else rng.choice((2, 5, 9, 17, 33, 48))
        pool = [v for v in g.vids if v not in g.cycle]
        rng.shuffle(pool)
        pool = [g.cycle[0]] + pool[:n_s - 1] + [g.cycle[1], g.cycle[2]] + pool[n_s - 1:]
        miss = A.missing_vids(g, 2, seed) if seed % 2 else []
        sources = pool[:n_s - (1 if miss and n_s > 1 else 0)] + (miss[:1] if n_s > 1 else [])
        targets = pool[n_s:n_s + n_t - len(miss[1:])] + miss[1:]
        if n_t == 64:
            targets = targets[:1] + targets[2:] + targets[1:2]    # c of the cycle is target 63
        assert len(targets) == n_t and not set(sources) & set(targets)
        _cases[seed] = (g, sources, targets, 7 if seed % 2 else 1)
    return _cases[seed]


@pytest.fixture(scope="module")
def space_of(eng):
    spaces = {}

    def get(seed, e=eng):
        if (seed, id(e)) not in spaces:
            g, _, _, parts = seeded(seed)
            spaces[(seed, id(e))] = P.load(e, 0, g.edges, num_parts=parts, vids=g.vids)
        return spaces[(seed, id(e))]
    return get


def test_seeded_graphs_reach_what_they_are_for():
    """On the model alone: bit 63, a vertex in three layers or more, masks that shrink from layer to layer."""
    deep = bit63 = shrink = 0
    for seed in SEEDS:
        g, sources, targets, _ = seeded(seed)
        dag = A.layered_dag(g.edges, sources, targets, [1, 2], False, 8, g.vids)
        bit63 += any(m >> 63 for m in dag.values())
        per = {}
        for (i, u, v, _, _), m in dag.items():
            per.setdefault(v, {})[i] = m
        deep += any(len(x) >= 3 for x in per.values())
        shrink += any(len(set(x.values())) > 1 for x in per.values())
    assert bit63 >= 2 and deep >= 8 and shrink >= 8


@pytest.mark.parametrize("seed", SEEDS)
def test_seeded_graph(eng, space_of, seed):
    g, sources, targets, _ = seeded(seed)
    for reversely in (False, True):
        for upto in UPTOS:
            check(eng, space_of(seed), g.edges, g.vids, sources, targets, ("e", "f"), reversely, upto)


@pytest.mark.parametrize("grid", [1, 3])
def test_walk_layout(eng, space_of, grid):
    """The UPTO 8 sentences with every layer in `grid` workgroups: many (row, slot) rounds, the LDS count carried over."""
    eng.set_flag("path_grid_max", grid)
    try:
        widest = 0
        for seed in SEEDS:
            g, sources, targets, _ = seeded(seed)
            check(eng, space_of(seed), g.edges, g.vids, sources, targets, ("e", "f"), seed % 2 == 1, 8, rows=False)
            widest = max([widest] + A.layer_sizes(g.edges, sources, targets, [1, 2], seed % 2 == 1, 8, g.vids))
        assert 2 * widest > 4 * grid                              # entries of one layer: a workgroup takes 4 a round
    finally:
        eng.set_flag("path_grid_max", 0)


def test_poisoned_scratch(space_of):
    """The whole seeded set on a fresh Engine whose scratch allocations start as 0xA5 bytes."""
    with engine.Engine() as e:
        e.set_flag("poison_buffers", 1)
        try:
            e.set_flag("find_path_all", 1)
            for seed in SEEDS:
                g, sources, targets, _ = seeded(seed)
                for reversely in (False, True):
                    for upto in UPTOS:
                        check(e, space_of(seed, e), g.edges, g.vids, sources, targets, ("e", "f"), reversely, upto, rows=False)
        finally:
            e.set_flag("poison_buffers", 0)


def test_reuse_between_sentences(eng, space_of):
    """The largest sentence, the smallest, the largest again; then a SHORTEST sentence and a GO between two ALLs."""
    size = {s: len(A.layered_dag(seeded(s)[0].edges, seeded(s)[1], seeded(s)[2], [1, 2], False, 8, seeded(s)[0].vids)) for s in SEEDS}
    big = max(size, key=size.get)
    assert size[big] > 100 and len(seeded(2)[2]) == 1
    for seed, upto in ((big, 8), (2, 1), (big, 8)):
        g, sources, targets, _ = seeded(seed)
        check(eng, space_of(seed), g.edges, g.vids, sources, targets, ("e", "f"), False, upto, rows=False)
    g, sources, targets, _ = seeded(big)
    sp = space_of(big)
    go = "GO 2 STEPS FROM %d OVER e YIELD e._dst AS d, e._rank AS r" % sources[0]
    digest = eng.go(sp, go, on_device=True, device_digest=True).device_digest
    shortest = device_rows(eng, sp, P.sentence(sources, targets, ("e", "f"), False, 8))
    for _ in range(2):
        check(eng, sp, g.edges, g.vids, sources, targets, ("e", "f"), False, 4, rows=False)
        assert device_rows(eng, sp, P.sentence(sources, targets, ("e", "f"), False, 8)) == shortest
        assert eng.go(sp, go, on_device=True, device_digest=True).device_digest == digest


# ----------------------------------------------------------------------------- shapes
def test_one_vertex_in_three_layers(eng):
    """1 -> 2 <-> 3 beside the chain 2 -> 4 -> 5: row 2 is in layers 1, 3 and 5 (4 in 2, 4, 6); and the 3-cycle at UPTO 8."""
    edges = [(1, 2, 1, 0), (2, 3, 1, 0), (3, 2, 1, 0), (2, 4, 1, 0), (4, 5, 1, 0)]
    vids = [1, 2, 3, 4, 5]
    sp = P.load(eng, 0, edges, vids=vids)
    dag = check(eng, sp, edges, vids, [1], [5], ("e",), False, 8)
    assert {i for (i, u, _, _, _) in dag if u == 2} == {1, 3, 5} and {i for (i, u, _, _, _) in dag if u == 4} == {2, 4, 6}
    check(eng, sp, edges, vids, [5], [1], ("e",), True, 8)
    cyc = [(1, 2, 1, 0), (2, 3, 1, 0), (3, 1, 1, 0)]
    sp = P.load(eng, 0, cyc, vids=[1, 2, 3])
    dag = check(eng, sp, cyc, [1, 2, 3], [1], [3], ("e",), False, 8)
    assert sorted(k[0] for k in dag) == list(range(8))            # the third arrival takes all 8 edges
    assert len(device_rows(eng, sp, "FIND ALL PATH FROM 1 TO 3 OVER e UPTO 8 STEPS")) == 3
    assert device_rows(eng, sp, "FIND NOLOOP PATH FROM 1 TO 3 OVER e UPTO 8 STEPS") == ["1<e,0>2<e,0>3"]


def test_self_loops(eng):
    """A self-loop on the source and on the middle vertex: ALL walks round them, NOLOOP keeps the one plain path."""
    edges = [(1, 1, 1, 0), (1, 2, 1, 0), (2, 2, 2, 5), (2, 3, 1, 0)]
    sp = P.load(eng, 0, edges, vids=[1, 2, 3])
    check(eng, sp, edges, [1, 2, 3], [1], [3], ("e", "f"), False, 4)
    assert device_rows(eng, sp, "FIND NOLOOP PATH FROM 1 TO 3 OVER e, f UPTO 4 STEPS") == ["1<e,0>2<e,0>3"]
    assert len(device_rows(eng, sp, "FIND ALL PATH FROM 1 TO 3 OVER e, f UPTO 4 STEPS")) == 6   # 2 edges; 3: 2 ways; 4: 3 ways
    check(eng, sp, edges, [1, 2, 3], [3], [1], ("e", "f"), True, 4)


def test_through_one_target_to_another_and_back(eng):
    edges = [(1, 2, 1, 0), (2, 3, 1, 0), (3, 2, 1, 0)]
    sp = P.load(eng, 0, edges, vids=[1, 2, 3])
    check(eng, sp, edges, [1, 2, 3], [1], [2, 3], ("e",), False, 4)
    assert device_rows(eng, sp, "FIND ALL PATH FROM 1 TO 2, 3 OVER e UPTO 4 STEPS") == [
        "1<e,0>2", "1<e,0>2<e,0>3", "1<e,0>2<e,0>3<e,0>2", "1<e,0>2<e,0>3<e,0>2<e,0>3"]
    assert device_rows(eng, sp, "FIND NOLOOP PATH FROM 1 TO 2, 3 OVER e UPTO 4 STEPS") == ["1<e,0>2", "1<e,0>2<e,0>3"]


def test_parallel_edges(eng):
    """Two edges that differ in rank only and two that differ in type only are different steps."""
    edges = [(1, 2, 1, 0), (1, 2, 1, 9), (2, 3, 1, 4), (2, 3, 2, 4)]
    sp = P.load(eng, 0, edges, vids=[1, 2, 3])
    dag = check(eng, sp, edges, [1, 2, 3], [1], [3], ("e", "f"), False, 2)
    assert len(dag) == 4
    assert len(device_rows(eng, sp, "FIND NOLOOP PATH FROM 1 TO 3 OVER e, f UPTO 2 STEPS")) == 4
    check(eng, sp, edges, [1, 2, 3], [3], [1], ("e", "f"), True, 2)


@pytest.mark.parametrize("grid", [0, 1])
def test_unequal_waves_in_one_workgroup(eng, grid):
    """Layer 1 is five rows with 0, 1, 65, 130 and 64 out-edges, each into a middle of its own that leads to the
    target (the row without out-edges is a target itself, or nothing would list it): over `e, f` 10 (row, slot)
    entries with trip counts 0 .. 3 in a workgroup and two idle waves in the third."""
    degrees = [(0, 1), (1, 2), (65, 1), (130, 1), (64, 2)]        # (out-edges, their type)
    edges, nxt = [], 7
    target = 7 + sum(d for d, _ in degrees)
    for i, (d, t) in enumerate(degrees):
        edges.append((1, 2 + i, 1 + i % 2, i))
        for _ in range(d):
            edges += [(2 + i, nxt, t, -3), (nxt, target, 1, 0)]
            nxt += 1
    assert nxt == target
    vids = list(range(1, target + 1))
    sp = P.load(eng, 0, edges, vids=vids)
    eng.set_flag("path_grid_max", grid)
    try:
        dag = check(eng, sp, edges, vids, [1], [target, 2], ("e", "f"), False, 3)
        assert len(dag) == 5 + 2 * 260 and A.layer_sizes(edges, [1], [target, 2], [1, 2], False, 3, vids) == [1, 5, 260]
        check(eng, sp, edges, vids, [1], [target, 2], ("e", "f"), False, 4)
    finally:
        eng.set_flag("path_grid_max", 0)


def loop_flushes(n):
    """One layer row with n emitted edges: its wave adds 64 a trip (the last trip the rest); after a trip the
    workgroup flushes when it holds more than kPathBuf - 256. The flush after the kernel's last round is not counted."""
    have = flushes = 0
    while n:
        have += min(n, 64)
        n -= min(n, 64)
        if have > K_PATH_BUF - 256:
            flushes += 1
            have = 0
    return flushes


@pytest.mark.parametrize("n", [767, 768, 769, 1664])
def test_flush_at_exactly_the_bound(eng, n):
    """1 -> n middles -> the target, UPTO 2: layer 0 is one row whose n edges are all emitted in one workgroup; layer
    1 is n rows of one edge, four a workgroup, which never fill a buffer."""
    assert [loop_flushes(k) for k in (767, 768, 769, 1664)] == [0, 0, 1, 2]
    edges = [(1, 2 + i, 1, 0) for i in range(n)] + [(2 + i, n + 2, 1, 0) for i in range(n)]
    vids = list(range(1, n + 3))
    sp = P.load(eng, 0, edges, vids=vids)
    before = eng.get_flag("find_path_loop_flushes")
    dag = check(eng, sp, edges, vids, [1], [n + 2], ("e",), False, 2, rows=False)
    assert len(dag) == 2 * n
    assert eng.get_flag("find_path_loop_flushes") == before + loop_flushes(n)


RANKS = {"const 5": [5], "const -1": [-1], "int8": [-128, 127, 0], "int16": [-(1 << 15), (1 << 15) - 1, 1],
         "int32": [-(1 << 31), (1 << 31) - 1, -1], "int64": [-(1 << 63), (1 << 63) - 1, 0]}


@pytest.mark.parametrize("narrow", [1, 0])
@pytest.mark.parametrize("form", list(RANKS))
def test_rank_storage_forms(eng, form, narrow):
    ranks = RANKS[form]
    assert P.rank_form(ranks) == form.split()[0] and form.split()[0] in P.RANK_FORMS
    edges = [(a, a + 1, 1, r) for a in (1, 2, 3) for r in ranks]
    eng.set_flag("narrow_columns", narrow)
    try:
        sp = P.load(eng, 0, edges, vids=[1, 2, 3, 4])
    finally:
        eng.set_flag("narrow_columns", 1)
    dag = check(eng, sp, edges, [1, 2, 3, 4], [1], [4], ("e",), False, 3)
    assert {k[4] for k in dag} == set(ranks) and len(dag) == 3 * len(ranks)
    check(eng, sp, edges, [1, 2, 3, 4], [4], [1], ("e",), True, 3)


def test_chain_with_a_target_at_each_vertex(eng):
    edges = [(i, i + 1, 1, 0) for i in range(1, 9)]
    vids = list(range(1, 10))
    sp = P.load(eng, 0, edges, vids=vids)
    dag = check(eng, sp, edges, vids, [1], vids[1:], ("e",), False, 8)
    assert dag[(0, 1, 2, 1, 0)] == 0xFF and dag[(7, 8, 9, 1, 0)] == 0x80 and len(dag) == 8
    assert len(device_rows(eng, sp, A.sentence("NOLOOP", [1], vids[1:], ("e",), False, 8))) == 8
    dag = check(eng, sp, edges, vids, [1], vids[1:], ("e",), False, 7)
    assert len(dag) == 7 and A.found(dag, vids[1:]) == 0x7F
    check(eng, sp, edges, vids, [9], vids[:8], ("e",), True, 8)


def test_dead_ends(eng):
    """A source without a vertex, a source without edges, a target nothing reaches, and a to side that dies at depth 1
    while UPTO is 8 (the deeper layers read depth 1's sets)."""
    edges = [(1, 2, 1, 0), (2, 3, 1, 0), (3, 4, 1, 0), (5, 6, 1, 0), (4, 1, 1, 0)]
    vids = [1, 2, 3, 4, 5, 6, 7]
    sp = P.load(eng, 0, edges, vids=vids)
    assert check(eng, sp, edges, vids, [99], [4], ("e",), False, 8) == {}
    assert check(eng, sp, edges, vids, [7], [4], ("e",), False, 8) == {}
    dag = check(eng, sp, edges, vids, [1, 7, 99], [4, 5, 98], ("e",), False, 8)
    assert A.found(dag, [4, 5, 98]) == 1
    assert A.levels(edges, [1], [6], [1], False, 8, vids) == (2, 1)   # 6 <- 5 <- nothing: the depth-2 expansion finds no row
    assert check(eng, sp, edges, vids, [1], [6], ("e",), False, 8) == {}
    dag = check(eng, sp, edges, vids, [5, 1], [6], ("e",), False, 8)
    assert list(dag) == [(0, 5, 6, 1, 0)]


# ----------------------------------------------------------------------------- refusals
def test_refusals(eng):
    edges = [(0, 1, 1, 0), (1, 2, 2, 0), (0, 2, 2, 4)] + [(0, 3 + i, 1, 0) for i in range(10)] + [(3 + i, 2, 1, 0) for i in range(10)]
    sp = P.load(eng, 13, edges)
    ok = ["1<e,0>2<f,0>3", "1<f,4>3"] + ["1<e,0>%d<e,0>3" % (4 + i) for i in range(10)]
    assert device_rows(eng, sp, "FIND ALL PATH FROM 1 TO 3 OVER e, f UPTO 8 STEPS") == sorted(ok)
    assert P.refused(eng, sp, "FIND ALL PATH FROM 1 TO 3 OVER e, f UPTO 9 STEPS", "find path: UPTO above 8 for ALL and NOLOOP") == sorted(ok)
    P.refused(eng, sp, "FIND NOLOOP PATH FROM 1 TO 3 OVER e, f BIDIRECT UPTO 3 STEPS", "find path: BIDIRECT")
    many = ", ".join(str(100 + i) for i in range(64))
    assert P.refused(eng, sp, "FIND ALL PATH FROM 1 TO 3, %s OVER e, f UPTO 3 STEPS" % many, "find path: more than 64 targets") == sorted(ok)
    eng.set_flag("path_rows_max", 8)
    try:
        assert P.refused(eng, sp, "FIND ALL PATH FROM 1 TO 3 OVER e, f UPTO 3 STEPS", "find path: path edges above path_rows_max") == sorted(ok)
    finally:
        eng.set_flag("path_rows_max", 1 << 20)
    # the walks are counted on the host, after the device has answered: the device stat moves, the pipeline falls back
    q = "FIND ALL PATH FROM 1 TO 3 OVER e, f UPTO 3 STEPS"
    eng.path_paths_max = 10
    try:
        r = eng.find_path(sp, q)
        assert not r.ok and r.code == engine.E_UNSUPPORTED and r.error == "find path: more than 10 paths", r.error
        p = pipeline.Pipeline(eng, sp, P.EDGES, find_path=True)
        out = p.run(q)
        assert out.ok and p.find_path_fallbacks == 1 and p.find_path_refusal == "find path: more than 10 paths"
        assert sorted(x[0][1] for x in out.rows) == sorted(ok)
        assert eng.find_path(sp, q.replace("ALL", "NOLOOP")).error == "find path: more than 10 paths"
        eng.path_paths_max = 12                                   # twelve walks: the bound itself is allowed
        assert device_rows(eng, sp, q) == sorted(ok)
    finally:
        del eng.path_paths_max
    assert eng.path_paths_max == 1 << 20


# ----------------------------------------------------------------------------- RMAT
SCALE = 10
RMAT_DRAWS = (0, 1, 2, 10, 18, 19, 23, 35, 47, 48)            # draws whose ALL answer over the oracle has 7 .. 105 rows: far under both caps


def rmat_draw(draw):
    rng = random.Random(4200 + draw)
    ns, nt = rng.randint(1, 2), rng.randint(1, 8)
    vids = rng.sample(range(1 << SCALE), ns + nt)
    return ", ".join(map(str, vids[:ns])), ", ".join(map(str, vids[ns:]))


@pytest.fixture(scope="module")
def rmat():
    ds = fixtures.RmatDataset(SCALE, ef=4, with_in=True)
    o = oracle.Oracle()
    o.set_flags(threads=8)
    ds.load_oracle(o)
    with engine.Engine() as e:
        e.set_flag("find_path_all", 1)
        ds.load_engine(e)
        yield ds, o, e
    o.close()


@pytest.mark.parametrize("draw", RMAT_DRAWS)
def test_rmat_equals_the_host_restatement(rmat, draw):
    ds, o, e = rmat
    frm, to = rmat_draw(draw)
    for kind in ("ALL", "NOLOOP"):
        q = "FIND %s PATH FROM %s TO %s OVER e%s UPTO 3 STEPS" % (kind, frm, to, " REVERSELY" if draw % 2 else "")
        before = e.get_flag("find_path_device")
        p = pipeline.Pipeline(e, ds.space, ["e"], find_path=True)
        dev = p.run(q)
        assert dev.ok and p.find_path_fallbacks == 0 and e.get_flag("find_path_device") == before + 1, (dev.error, p.find_path_refusal)
        ref = pipeline.run(o, ds.space, q, ["e"], find_path=True)
        assert ref.ok, ref.error
        assert sorted(r[0][1] for r in dev.rows) == sorted(r[0][1] for r in ref.rows) and len(ref.rows) >= 6, q
