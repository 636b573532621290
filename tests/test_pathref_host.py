"""The FIND SHORTEST PATH model (tests/pathref.py) against the host restatement (nebula_amd/findpath.py) over an
in-memory backend, through findpath.paths_from_dag, and the conditions that the device test's seeds and queries
(pathref.gpu_case / gpu_queries, run by tests/test_gpu_findpath_dag.py) must meet to be worth running. No GPU."""
import random
from types import SimpleNamespace

import numpy as np
import pytest

from nebula_amd import findpath, ngql
from tests import pathref as P


class MemBackend:
    """Answers the one-step GOs of findpath._neighbours from an edge list: one row of (kind, value) cells
    `_src, _dst, _type, _rank` per edge of the asked type at an asked vid, the type negated and the ends swapped
    for REVERSELY."""

    def __init__(self, graph):
        self.vertices = set(graph.vids)
        self.out, self.inn = {}, {}
        for a, b, t, r in graph.edges:
            self.out.setdefault((a, t), []).append((b, r))
            self.inn.setdefault((b, t), []).append((a, r))
        self.calls = 0

    def go(self, space, g):
        assert len(g.over) == 1 and g.direction in (ngql.FORWARD, ngql.REVERSELY) and len(g.yields) == 4
        self.calls += 1
        t = P.TYPE_OF[g.over[0][0]]
        table, sign = (self.out, 1) if g.direction == ngql.FORWARD else (self.inn, -1)
        rows = []
        for v in g.vids:
            if v in self.vertices:
                for d, r in table.get((v, t), ()):
                    rows.append((("int", v), ("int", d), ("int", sign * t), ("int", r)))
        return SimpleNamespace(ok=True, error="", rows=rows)


OVERS = (("e",), ("e", "f"), ("*",))


def small_cases():
    """240 cases: 40 graphs of 24 .. 40 vertices (hubs of 4 .. 8 edges: the host leg extends every walk) x 6 queries
    each, over both directions, the three OVER forms and UPTO 1 .. 6, with 1 .. 3 sources and 1 .. 8 targets, some
    of them vids without a vertex."""
    out = []
    for seed in range(40):
        g = P.random_graph(seed, 24 + seed % 17, hub_degrees=(4, 8), hubs=2)
        rng = random.Random(seed)
        for q in range(6):
            pool = g.vids + P.missing_vids(g, 2, seed + q)
            picked = rng.sample(pool, rng.randint(1, 3) + rng.randint(1, 8))
            n_s = rng.randint(1, min(3, len(picked) - 1))
            n_s = min(n_s, len(picked) - 1)
            out.append((g, picked[:n_s], picked[n_s:][:8], OVERS[(seed + q) % 3], (seed + q // 3) % 2 == 1, 1 + (seed + q) % 6))
    return out


def model_of(g, sources, targets, over, reversely, upto):
    types = [1, 2] if over == ("*",) else [P.TYPE_OF[n] for n in over]
    return P.shortest_dag(g.edges, sources, targets, types, reversely, upto, g.vids)


def test_model_equals_the_host_restatement():
    cases = small_cases()
    assert len(cases) >= 200
    nonempty = deep = 0
    for g, sources, targets, over, reversely, upto in cases:
        s = ngql.parse_find_path(P.sentence(sources, targets, over, reversely, upto))
        backend = MemBackend(g)
        host = findpath.find_path(backend, 1, s, sources, targets, P.EDGES)
        m = model_of(g, sources, targets, over, reversely, upto)
        want = P.render_paths(m.edges, sources, targets, P.NAME_OF)
        assert sorted(host) == want, (g.vids, g.edges, sources, targets, over, reversely, upto)
        assert len(want) == sum(P.count_paths(m.edges, sources, j) for j in range(len(targets)))
        nonempty += bool(want)
        deep += any(3 <= l <= upto for l in m.L)
    assert nonempty >= len(cases) // 3 and deep >= 20                 # the comparison is not one of empty lists


def test_model_through_paths_from_dag():
    for g, sources, targets, over, reversely, upto in small_cases():
        m = model_of(g, sources, targets, over, reversely, upto)
        keys = sorted(m.edges)
        cols = [np.array([k[i] for k in keys], np.int64) for i in range(4)]
        mask = np.array([m.edges[k] for k in keys], np.uint64)
        got = findpath.paths_from_dag(sources, targets, cols[0], cols[1], cols[2], cols[3], mask, P.NAME_OF)
        assert sorted(got) == P.render_paths(m.edges, sources, targets, P.NAME_OF)


def test_hand_checked_dags():
    """The model itself on graphs small enough to read: a diamond, a target one step past UPTO, a vid without a
    vertex, REVERSELY's orientation and sign, a vertex at two distances from two targets."""
    diamond = [(1, 2, 1, 0), (1, 3, 1, 7), (2, 4, 1, 0), (3, 4, 2, -1), (4, 5, 1, 0)]
    m = P.shortest_dag(diamond, [1], [4, 5, 9], [1, 2], False, 2)
    assert m.edges == {(1, 2, 1, 0): 1, (1, 3, 1, 7): 1, (2, 4, 1, 0): 1, (3, 4, 2, -1): 1} and m.found == 1
    assert m.L[:2] == [2, 3] and m.levels == 2                    # 5 is one past UPTO; 9 has no vertex
    assert P.count_paths(m.edges, [1], 0) == 2
    assert P.render_paths(m.edges, [1], [4, 5, 9], P.NAME_OF) == ["1<e,0>2<e,0>4", "1<e,7>3<f,-1>4"]
    m = P.shortest_dag(diamond, [1], [4, 5], [1], False, 3)
    assert m.edges == {(1, 2, 1, 0): 3, (2, 4, 1, 0): 3, (4, 5, 1, 0): 2} and m.found == 3 and m.levels == 2
    m = P.shortest_dag(diamond, [4], [1], [1, 2], True, 5)
    assert m.edges == {(4, 2, -1, 0): 1, (2, 1, -1, 0): 1, (4, 3, -2, -1): 1, (3, 1, -1, 7): 1}
    assert P.render_paths(m.edges, [4], [1], P.NAME_OF) == ["4<-e,0>2<-e,0>1", "4<-f,-1>3<-e,7>1"]
    two = [(1, 2, 1, 0), (2, 3, 1, 0), (3, 4, 1, 0), (4, 5, 1, 0), (4, 6, 1, 0), (6, 7, 1, 0)]
    m = P.shortest_dag(two, [1], [5, 7], [1], False, 5)
    assert m.edges[(3, 4, 1, 0)] == 3 and m.edges[(4, 5, 1, 0)] == 1 and m.edges[(4, 6, 1, 0)] == 2
    assert m.found == 3 and m.levels == 4                         # 4 edges at the even meet of step 2, 5 at the odd meet of step 3
    assert P.shortest_dag(two, [9], [5], [1], False, 5).levels == 0
    assert P.shortest_dag(two, [7], [1], [1], False, 5)[:3] == ({}, 0, 2)   # 7 leads nowhere: level 1 of the from side is empty


def test_random_graph_is_what_it_says():
    for seed in P.GPU_SEEDS:
        g = P.random_graph(seed, P.GPU_NV)
        assert g == P.random_graph(seed, P.GPU_NV) and len(set(g.edges)) == len(g.edges)
        deg, touched = {}, set()
        for a, b, t, r in g.edges:
            deg[a] = deg.get(a, 0) + 1
            touched |= {a, b}
        assert len(g.hubs) in (2, 3) and all(70 <= deg[h] <= 300 for h in g.hubs) and max(deg[h] for h in g.hubs) > 256
        rest = [d for v, d in deg.items() if v not in g.hubs]
        assert 1.2 <= sum(rest) / (P.GPU_NV - len(g.hubs)) <= 1.9
        assert len(g.isolated) == 3 and not touched & set(g.isolated)
        assert sum(1 for a, b, _, _ in g.edges if a == b) >= 3
        pairs = {}
        for a, b, t, r in g.edges:
            pairs.setdefault((a, b), []).append((t, r))
        assert any(len({t for t, _ in x}) == 2 for x in pairs.values())
        assert any(len(x) > len({t for t, _ in x}) for x in pairs.values())
    forms = {t: {P.random_graph(seed, P.GPU_NV).forms[t] for seed in P.GPU_SEEDS} for t in (1, 2)}
    assert forms[1] == forms[2] == set(P.RANK_FORMS)


def test_device_cases_reach_what_they_are_for():
    """Asserted on the model alone, over the seeds and queries tests/test_gpu_findpath_dag.py runs."""
    queries = found_one = three_lengths = odd_and_even = just_past = two_dt = 0
    longest = deepest = 0
    forms_on_dags = set()
    n_targets = []
    for seed in P.GPU_SEEDS:
        c = P.gpu_case(seed)
        n_targets.append(len(c.targets))
        assert 1 <= len(c.sources) <= 4 and 1 <= len(c.targets) <= 64
        for reversely, over, upto in P.gpu_queries(seed):
            m = P.gpu_model(seed, reversely, over, upto)
            d = P.gpu_dist(seed, reversely, over)
            lengths = {l for l in m.L if 1 <= l <= upto}
            queries += 1
            found_one += bool(lengths)
            three_lengths += len(lengths) >= 3
            odd_and_even += len({l % 2 for l in lengths}) == 2
            just_past += upto + 1 in m.L
            longest = max([longest] + list(lengths))
            deepest = max(deepest, m.levels // 2)
            for (u, v, t, r) in m.edges:
                forms_on_dags.add((abs(t), c.graph.forms[abs(t)]))
            on = {}                                               # vertex -> the dt at which it lies on some target's DAG
            for (u, v, t, r), mask in m.edges.items():
                for j in range(len(c.targets)):
                    if mask >> j & 1:
                        on.setdefault(v, set()).add(d.dt[j][v])
            two_dt += any(len(x) > 1 for x in on.values())
    assert queries == 384
    assert sum(1 for n in n_targets if n == 64) >= 4 and sum(1 for n in n_targets if n == 63) >= 2
    assert found_one >= 0.8 * queries, found_one
    assert three_lengths >= 0.25 * queries, three_lengths
    assert odd_and_even > 0 and just_past > 0 and two_dt > 0
    assert longest >= 9, longest
    assert forms_on_dags == {(t, f) for t in (1, 2) for f in P.RANK_FORMS}, forms_on_dags
    print("queries %d, one target found %.1f %%, three lengths %.1f %%, odd and even %d, L = upto + 1 in %d, "
          "two dt in %d, longest L %d, deepest level %d" % (queries, 100.0 * found_one / queries, 100.0 * three_lengths / queries,
                                                          odd_and_even, just_past, two_dt, longest, deepest))
    # path_grid_max = 1: some level of an UPTO 8 query holds more than 4 (row, slot) entries, so a workgroup loops
    assert max(max(P.gpu_model(s, rev, ("e", "f"), 8).from_sizes.values()) for s in P.GPU_SEEDS for rev in (False, True)) * 2 > 4
