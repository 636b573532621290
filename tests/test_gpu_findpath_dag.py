"""The path DAG of ngx_find_path (nebula_amd/csrc/findpath.hip, op_findpath.cpp::findPath) against the breadth-first model
of tests/pathref.py, edge by edge and target bit by target bit, with the found mask and the levels expanded.

Every case calls Engine.find_path(..., rows=False), checks that the stat find_path_device rose by one, and compares
the (src, dst, type, rank, bit) tuples of the returned edge arrays with the model's. No tuple may occur twice: a
target is found at one meet (the odd meet masks with notFound, the even one with `had`), the sweeps after that meet
visit every (level row, slot, edge) once, and an edge u -> v lies in exactly one of the from side's levels, the odd
meet's edges and the to side's levels, by ds[u] alone. Where the model counts at most 5,000 paths the rendered rows
are compared too.

Seeded graphs of 300 vertices (pathref.gpu_case; tests/test_pathref_host.py asserts what they reach), the sweeps
under path_grid_max 1 and 3, the LDS buffer's flush at exactly its bound, a level whose waves have unequal trip
counts and a workgroup with idle waves, every rank storage form with and without narrow columns, the deepest legal
search (level 250 in a uint8_t), the refusals that had no test, and scratch that shrinks and grows between calls.
"""
import numpy as np
import pytest

from nebula_amd import engine, pipeline
from tests import fixtures
from tests import pathref as P

pytestmark = pytest.mark.gpu

K_PATH_BUF, K_PATH_GRID_MAX = 1024, 2048                          # kernels.h: kPathBuf, kPathGridMax
MAX_ROWS = 5000


@pytest.fixture(scope="module")
def eng():
    with engine.Engine() as e:
        yield e


@pytest.fixture(scope="module")
def space_of(eng):
    spaces = {}

    def get(seed):
        if seed not in spaces:
            c = P.gpu_case(seed)
            spaces[seed] = P.load(eng, 0, c.graph.edges, num_parts=c.num_parts, vids=c.graph.vids)
        return spaces[seed]
    return get


def device_dag(e, space, q):
    """({(src, dst, type, rank, bit)}, found, levels) of the sentence on the device; no tuple twice."""
    before = e.get_flag("find_path_device")
    r = e.find_path(space, q, rows=False)
    assert r.ok, r.error
    assert e.get_flag("find_path_device") == before + 1
    src, dst, typ, rank, mask = r.dev_cols
    assert len(src) == len(dst) == len(typ) == len(rank) == len(mask) == r.go_nrows
    tuples = []
    for i in range(len(src)):
        m = int(mask[i])
        assert m != 0
        key = (int(src[i]), int(dst[i]), int(typ[i]), int(rank[i]))
        tuples += [key + (j,) for j in range(64) if m >> j & 1]
    got = set(tuples)
    assert len(got) == len(tuples), "an (edge, target) pair was emitted twice"
    return got, r.path_found, r.hop_frontier[0]


def device_rows(e, space, q):
    before = e.get_flag("find_path_device")
    r = e.find_path(space, q)
    assert r.ok, r.error
    assert e.get_flag("find_path_device") == before + 1 and r.nrows == len(r.rows)
    return sorted(row[0][1] for row in r.rows)


def check(e, space, q, model, sources, targets, rows=True):
    got, found, levels = device_dag(e, space, q)
    want = P.dag_tuples(model.edges)
    assert got == want, (q, sorted(got - want)[:5], sorted(want - got)[:5])
    assert found == model.found, (q, bin(found), bin(model.found))
    assert levels == model.levels, (q, levels, model.levels)
    if rows and sum(P.count_paths(model.edges, sources, j) for j in range(len(targets))) <= MAX_ROWS:
        assert device_rows(e, space, q) == P.render_paths(model.edges, sources, targets, P.NAME_OF), q


def check_graph(e, space, edges, vertices, sources, targets, over, reversely, upto, rows=True):
    m = P.shortest_dag(edges, sources, targets, [P.TYPE_OF[n] for n in over], reversely, upto, vertices)
    check(e, space, P.sentence(sources, targets, over, reversely, upto), m, sources, targets, rows)
    return m


# ----------------------------------------------------------------------------- seeded graphs
@pytest.mark.parametrize("seed", P.GPU_SEEDS)
def test_random_graph(eng, space_of, seed):
    c = P.gpu_case(seed)
    sp = space_of(seed)
    for reversely, over, upto in P.gpu_queries(seed):
        check(eng, sp, P.sentence(c.sources, c.targets, over, reversely, upto), P.gpu_model(seed, reversely, over, upto),
              c.sources, c.targets)


@pytest.mark.parametrize("grid", [1, 3])
def test_sweep_layout(eng, space_of, grid):
    """The UPTO 8 sentences of every seed with the sweeps (and the odd meet) in `grid` workgroups: each goes through
    many (row, slot) rounds with the LDS count carried over, its waves on rows of unequal degree."""
    assert eng.get_flag("path_grid_max") == 0
    eng.set_flag("path_grid_max", grid)
    try:
        assert eng.get_flag("path_grid_max") == grid
        widest = 0
        for seed in P.GPU_SEEDS:
            c = P.gpu_case(seed)
            for reversely in (False, True):
                m = P.gpu_model(seed, reversely, ("e", "f"), 8)
                check(eng, space_of(seed), P.sentence(c.sources, c.targets, ("e", "f"), reversely, 8), m, c.sources, c.targets, rows=False)
                for length in {l for l in m.L if 1 <= l <= 8}:    # the from side's levels below the meet are swept
                    widest = max([widest] + [2 * m.from_sizes[d] for d in range((length + 1) // 2)])
        assert widest > 4 * grid                                  # entries of one sweep: a workgroup takes 4 a round
    finally:
        eng.set_flag("path_grid_max", 0)


def test_path_grid_max_range(eng):
    for bad in (-1, K_PATH_GRID_MAX + 1):
        with pytest.raises(engine.EngineError, match="path_grid_max"):
            eng.set_flag("path_grid_max", bad)
    assert eng.get_flag("path_grid_max") == 0


def test_scratch_shrinks_and_grows(eng, space_of):
    """The largest sentence, the smallest, the largest again on one Engine: the per-level lists are reused."""
    size = {s: len(P.gpu_model(s, False, ("e", "f"), 15).edges) for s in P.GPU_SEEDS}
    big, small = max(size, key=size.get), 6
    assert len(P.gpu_case(small).targets) == 1 and size[big] > 100
    for seed, upto in ((big, 15), (small, 1), (big, 15)):
        c = P.gpu_case(seed)
        check(eng, space_of(seed), P.sentence(c.sources, c.targets, ("e", "f"), False, upto), P.gpu_model(seed, False, ("e", "f"), upto),
              c.sources, c.targets, rows=False)


# ----------------------------------------------------------------------------- the flush inside the edge loop
def loop_flushes(n):
    """One sweep of one row with n kept edges: one wave is active and adds 64 edges a trip (the last trip the rest);
    after a trip the workgroup flushes when it holds more than kPathBuf - 256."""
    have = flushes = 0
    while n:
        have += min(n, 64)
        n -= min(n, 64)
        if have > K_PATH_BUF - 256:
            flushes += 1
            have = 0
    return flushes


@pytest.mark.parametrize("n", [767, 768, 769, 832, 833, 1664])
def test_flush_at_exactly_the_bound(eng, n):
    """1 -> n middles -> target, UPTO 2. Only loop flushes count (the flush after a kernel's last round does not), and
    only k_path_sweep counts them: the odd meet of step 1 walks the source's n edges and keeps none, the even meet
    finds the target at the middles, then the from side sweeps level 0 (the source's n edges, all kept) and the to
    side its level 0 (the target's n transposed edges, all kept): twice the flushes of one such row."""
    assert [loop_flushes(k) for k in (767, 768, 769, 832, 833, 1664)] == [0, 0, 1, 1, 1, 2]
    edges = [(1, 2 + i, 1, 0) for i in range(n)] + [(2 + i, n + 2, 1, 0) for i in range(n)]
    vids = list(range(1, n + 3))
    sp = P.load(eng, 0, edges, vids=vids)
    before = eng.get_flag("find_path_loop_flushes")
    m = check_graph(eng, sp, edges, vids, [1], [n + 2], ("e",), False, 2, rows=False)
    assert len(m.edges) == 2 * n
    assert eng.get_flag("find_path_loop_flushes") == before + 2 * loop_flushes(n)


# ----------------------------------------------------------------------------- unequal waves, idle waves
@pytest.mark.parametrize("grid", [0, 1])
def test_unequal_waves_in_one_workgroup(eng, grid):
    """Level 1 of the from side is five rows with 0, 1, 65, 130 and 64 out-edges, each into a middle of its own; every
    middle leads to target 1 (3 edges: the odd meet of step 2 walks the five rows) and through one more vertex to
    target 2 (4 edges: the even meet of step 2, then the sweep walks them). Over `e, f` that is 10 entries: trip
    counts 0 .. 3 within a workgroup, and two idle waves in the third."""
    degrees = [(0, 1), (1, 2), (65, 1), (130, 1), (64, 2)]        # (out-edges, their type)
    edges, nxt = [], 7
    t1 = 7 + sum(d for d, _ in degrees)
    x, t2 = t1 + 1, t1 + 2
    for i, (d, t) in enumerate(degrees):
        edges.append((1, 2 + i, 1 + i % 2, i))
        for _ in range(d):
            edges += [(2 + i, nxt, t, -3), (nxt, t1, 1, 0), (nxt, x, 2, 9)]
            nxt += 1
    edges.append((x, t2, 1, 0))
    assert nxt == t1
    vids = list(range(1, t2 + 1))
    sp = P.load(eng, 0, edges, vids=vids)
    eng.set_flag("path_grid_max", grid)
    try:
        m = check_graph(eng, sp, edges, vids, [1], [t1, t2], ("e", "f"), False, 4)
        assert m.from_sizes[1] == 5 and m.found == 3 and m.L == [3, 4]
        check_graph(eng, sp, edges, vids, [t1, t2], [1], ("e", "f"), True, 4)
    finally:
        eng.set_flag("path_grid_max", 0)


# ----------------------------------------------------------------------------- ranks
RANKS = {"const 5": [5], "const -1": [-1], "int8": [-128, 127, 0], "int16": [-(1 << 15), (1 << 15) - 1, 1],
         "int32": [-(1 << 31), (1 << 31) - 1, -1], "int64": [-(1 << 63), (1 << 63) - 1, 0]}


@pytest.mark.parametrize("narrow", [1, 0])
@pytest.mark.parametrize("form", list(RANKS))
def test_rank_storage_forms(eng, form, narrow):
    """1 -> 2 -> 3 -> 4 with every step once per rank: UPTO 3 reads the ranks in the from side's sweep, the odd meet
    and the to side's sweep. narrow_columns = 0 stores every form in 8 bytes and none as a constant."""
    ranks = RANKS[form]
    assert P.rank_form(ranks) == form.split()[0]
    edges = [(a, a + 1, 1, r) for a in (1, 2, 3) for r in ranks]
    vids = [1, 2, 3, 4]
    assert eng.get_flag("narrow_columns") == 1
    eng.set_flag("narrow_columns", narrow)
    try:
        sp = P.load(eng, 0, edges, vids=vids)
    finally:
        eng.set_flag("narrow_columns", 1)
    m = check_graph(eng, sp, edges, vids, [1], [4], ("e",), False, 3)
    assert {k[3] for k in m.edges} == set(ranks) and len(m.edges) == 3 * len(ranks)
    check_graph(eng, sp, edges, vids, [4], [1], ("e",), True, 3)


# ----------------------------------------------------------------------------- depth
@pytest.fixture(scope="module")
def chain(eng):
    edges = [(i, i + 1, 1, 0) for i in range(1, 501)]
    vids = list(range(1, 502))
    return P.load(eng, 0, edges, vids=vids), edges, vids


def test_deepest_search(eng, chain):
    sp, edges, vids = chain
    m = check_graph(eng, sp, edges, vids, [1], [501], ("e",), False, 500)
    assert m.found == 1 and len(m.edges) == 500 and m.levels == 500   # the even meet of step 250: level 250
    m = check_graph(eng, sp, edges, vids, [1], [501], ("e",), False, 499)
    assert m.found == 0 and not m.edges


def test_targets_at_64_depths(eng, chain):
    sp, edges, vids = chain
    targets = [1 + 7 * k for k in range(1, 65)]
    m = check_graph(eng, sp, edges, vids, [101], targets, ("e",), False, 500)
    assert m.found == sum(1 << (k - 1) for k in range(1, 65) if 7 * k > 100)      # the others lie behind the source
    assert m.found != 0 and m.found != (1 << 64) - 1


# ----------------------------------------------------------------------------- refusals
def refused_with_error(e, space, q, text, host_error):
    """As pathref.refused, for a sentence the host restatement answers with an error of its own."""
    r = e.find_path(space, q)
    assert not r.ok and r.code == engine.E_UNSUPPORTED and r.error == text, r.error
    before = e.get_flag("find_path_device")
    p = pipeline.Pipeline(e, space, P.EDGES, find_path=True)
    out = p.run(q)
    host = pipeline.run(e, space, q, P.EDGES, find_path=True, device_find_path=False)
    assert not out.ok and not host.ok and out.error == host.error == host_error, (out.error, host.error)
    assert p.find_path_fallbacks == 1 and p.find_path_refusal == text and e.get_flag("find_path_device") == before


def exactly(e, space, q, text):
    r = e.find_path(space, q)
    assert not r.ok and r.code == engine.E_UNSUPPORTED and r.error == text, r.error
    return P.refused(e, space, q, text)


def test_refusals(eng):
    edges = [(0, 1, 1, 0), (1, 2, 2, 0), (0, 2, 2, 4)]
    sp = P.load(eng, 3, edges)
    assert exactly(eng, sp, "FIND SHORTEST PATH FROM 1 TO 3 OVER e, f UPTO 501 STEPS", "find path: UPTO outside 1 .. 500") == ["1<f,4>3"]
    eng.set_flag("max_edge_returned_per_vertex", 1000)
    try:
        assert exactly(eng, sp, "FIND SHORTEST PATH FROM 1 TO 3 OVER *", "find path: max_edge_returned_per_vertex is set") == ["1<f,4>3"]
    finally:
        eng.set_flag("max_edge_returned_per_vertex", 0)
    assert device_rows(eng, sp, "FIND SHORTEST PATH FROM 1 TO 3 OVER *") == ["1<f,4>3"]
    exactly(eng, sp, "FIND SHORTEST PATH FROM 1 TO 2 OVER e AS a, e AS b", "find path: an edge listed twice")
    refused_with_error(eng, sp, "FIND SHORTEST PATH FROM 1 TO 3 OVER e, e", "find path: an edge alias listed twice", "edge alias(e) was dup")
    refused_with_error(eng, sp, "FIND SHORTEST PATH FROM 1 TO 3 OVER e AS a, f AS a", "find path: an edge alias listed twice",
                       "edge alias(a) was dup")
    ttl = [fixtures.SchemaDef(True, 1, "e", [("p0", P.kvfmt.INT)], ttl_col="p0", ttl_dur=1000), P.SCHEMA[1]]
    sp = P.load(eng, 3, edges, schema=ttl)
    exactly(eng, sp, "FIND SHORTEST PATH FROM 1 TO 3 OVER e, f", "find path: a TTL edge schema")
    assert device_rows(eng, sp, "FIND SHORTEST PATH FROM 1 TO 3 OVER f") == ["1<f,4>3"]       # f has no TTL
