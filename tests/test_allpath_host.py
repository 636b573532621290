"""FIND ALL PATH / FIND NOLOOP PATH without a GPU: the model of tests/allref.py (plain depth-first walks, plain
breadth-first layers) against the host restatement (nebula_amd/findpath.py) over the in-memory backend of
tests/test_pathref_host.py, and findpath.paths_from_layers / count_walks over the model's layered edge set against
the model's walks: on seeded graphs, on hand-checked graphs and on the reference's FindPathTest answers."""
import json
import os
import random

import numpy as np
import pytest

from nebula_amd import findpath, ngql
from tests import allref as A
from tests.golden.findpath_cases import CASES
from tests.test_findpath_host import golden_text
from tests.test_pathref_host import MemBackend

NAME_OF = {1: "e", 2: "f"}
OVERS = ((("e",), (1,)), (("e", "f"), (1, 2)), (("*",), (1, 2)))
MAX_WALKS = 20000
KINDS = (("ALL", False), ("NOLOOP", True))


sentence = A.sentence

def small_cases():
    """216 graphs of 12 .. 24 vertices (allref.random_graph: in- and out-degree at most 4) x 3 sentences: 1 .. 3
    sources, 1 .. 6 targets, both directions, the three OVER forms, UPTO 1 .. 6. The first sentence of a graph starts
    on its 3-cycle a -> b -> c -> a and lists b and c: b lies on a cycle through itself and on the walks to c. Odd
    sentences list a vid without a vertex on each side."""
    out = []
    for seed in range(216):
        g = A.random_graph(seed, 12 + seed % 13)
        rng = random.Random(seed)
        a, b, c = g.cycle
        for q in range(3):
            names, types = OVERS[(seed + q) % 3]
            reversely = (seed // 3 + q) % 2 == 1
            upto = 1 + (seed // 6 + q) % 6
            n_s, n_t = rng.randint(1, 3), rng.randint(1, 6)
            rest = [v for v in g.vids if v not in (a, b, c)]
            rng.shuffle(rest)
            if q == 0:
                sources = [a] + rest[:n_s - 1]
                targets = ([b, c] + rest[n_s:])[:max(n_t, 2)]
            else:
                pool = rest + [a, b, c]
                rng.shuffle(pool)
                sources, targets = pool[:n_s], pool[n_s:n_s + n_t]
            if (seed + q) % 2:
                miss = A.missing_vids(g, 2, seed + q)
                sources, targets = sources + miss[:1], targets + miss[1:]
            out.append((g, sources, targets, names, types, reversely, upto))
    return out


def as_columns(dag):
    keys = sorted(dag)
    cols = [np.array([k[i] for k in keys], np.int64) for i in range(5)]
    return cols + [np.array([dag[k] for k in keys], np.uint64)]


def rows_from_layers(dag, sources, targets, names, no_loop, max_paths=1 << 20):
    layer, src, dst, typ, rank, mask = as_columns(dag)
    return sorted(findpath.paths_from_layers(sources, targets, layer, src, dst, typ, rank, mask, names, no_loop, max_paths))


def test_model_equals_the_host_restatement_and_the_layers():
    cases = small_cases()
    assert len({id(c[0]) for c in cases}) >= 200
    nonempty = loops_dropped = through_itself = through_another = deep = 0
    for g, sources, targets, names, types, reversely, upto in cases:
        every = A.walks(g.edges, sources, targets, types, reversely, upto, False, g.vids)
        assert len(every) <= MAX_WALKS, (len(every), sources, targets, upto)
        dag = A.layered_dag(g.edges, sources, targets, types, reversely, upto, g.vids)
        layer, src, dst, typ, rank, mask = as_columns(dag)
        assert findpath.count_walks(sources, targets, layer, src, dst) == len(every) == A.count(dag, sources, targets)
        for kind, simple in KINDS:
            want = every if not simple else A.walks(g.edges, sources, targets, types, reversely, upto, True, g.vids)
            want = sorted(A.render(w, NAME_OF) for w in want)
            s = ngql.parse_find_path(sentence(kind, sources, targets, names, reversely, upto))
            host = findpath.find_path(MemBackend(g), 1, s, sources, targets, ["e", "f"])
            assert sorted(host) == want, (kind, g.vids, g.edges, sources, targets, names, reversely, upto)
            assert rows_from_layers(dag, sources, targets, NAME_OF, simple) == want, (kind, sources, targets, upto)
            if simple:
                assert all(len({w[0][0]} | {x[1] for x in w}) == len(w) + 1 for w in
                           A.walks(g.edges, sources, targets, types, reversely, upto, True, g.vids))
                loops_dropped += len(want) < len(every)
        nonempty += bool(every)
        deep += any(len(w) >= 5 for w in every)
        goal = set(targets)
        through_itself += any(w[-1][1] in {x[0] for x in w} for w in every)
        through_another += any(goal & ({x[0] for x in w[1:]} - {w[-1][1]}) for w in every)
    assert nonempty >= len(cases) // 3 and deep >= 30 and loops_dropped >= 100
    assert through_itself >= 50 and through_another >= 50


def test_max_paths_raises():
    g = A.random_graph(3, 20)
    a, b, c = g.cycle
    dag = A.layered_dag(g.edges, [a], [b, c], (1, 2), False, 6, g.vids)
    n = len(A.walks(g.edges, [a], [b, c], (1, 2), False, 6, False, g.vids))
    assert n >= 4
    assert len(rows_from_layers(dag, [a], [b, c], NAME_OF, False, max_paths=n)) == n
    for no_loop in (False, True):                                 # the bound is on the ALL walks for both kinds
        with pytest.raises(findpath.FindPathRefusal) as e:
            rows_from_layers(dag, [a], [b, c], NAME_OF, no_loop, max_paths=n - 1)
        assert str(e.value) == "find path: more than %d paths" % (n - 1)
    assert isinstance(e.value, findpath.FindPathError)


def test_hand_checked_dags():
    cyc = [(1, 2, 1, 0), (2, 3, 1, 0), (3, 1, 1, 0)]
    dag = A.layered_dag(cyc, [1], [3], [1], False, 7)
    # 3 is 2, 5 edges from 1 (and 8: past UPTO). Layer i holds the step i mod 3 of the cycle while 3 is still within
    # reach of its head: 6 - i edges left there. The 7th step 1 -> 2 leaves 2, two edges short of 3: not useful.
    assert dag == {(0, 1, 2, 1, 0): 1, (1, 2, 3, 1, 0): 1, (2, 3, 1, 1, 0): 1, (3, 1, 2, 1, 0): 1, (4, 2, 3, 1, 0): 1}
    # depth 3 of the to side reaches nothing new and ends it; layer 5 is launched from row 3 and emits nothing
    assert A.levels(cyc, [1], [3], [1], False, 7) == (3, 6)
    assert rows_from_layers(dag, [1], [3], NAME_OF, False) == ["1<e,0>2<e,0>3", "1<e,0>2<e,0>3<e,0>1<e,0>2<e,0>3"]
    assert rows_from_layers(dag, [1], [3], NAME_OF, True) == ["1<e,0>2<e,0>3"]
    assert A.found(dag, [3]) == 1
    diamond = [(1, 2, 1, 0), (1, 3, 1, 7), (2, 4, 1, 0), (3, 4, 2, -1), (4, 5, 1, 0)]
    dag = A.layered_dag(diamond, [1], [4, 5, 9], [1, 2], False, 3)
    assert dag == {(0, 1, 2, 1, 0): 3, (0, 1, 3, 1, 7): 3, (1, 2, 4, 1, 0): 3, (1, 3, 4, 2, -1): 3, (2, 4, 5, 1, 0): 2}
    assert A.found(dag, [4, 5, 9]) == 3 and A.levels(diamond, [1], [4, 5, 9], [1, 2], False, 3) == (2, 3)
    assert rows_from_layers(dag, [1], [4, 5, 9], NAME_OF, False) == [
        "1<e,0>2<e,0>4", "1<e,0>2<e,0>4<e,0>5", "1<e,7>3<f,-1>4", "1<e,7>3<f,-1>4<e,0>5"]
    dag = A.layered_dag(diamond, [1], [4, 5], [1, 2], False, 2)  # at UPTO 2 only 4 is within reach
    assert set(dag.values()) == {1} and len(dag) == 4
    dag = A.layered_dag(diamond, [4], [1], [1, 2], True, 2)
    assert dag == {(0, 4, 2, -1, 0): 1, (0, 4, 3, -2, -1): 1, (1, 2, 1, -1, 0): 1, (1, 3, 1, -1, 7): 1}
    assert rows_from_layers(dag, [4], [1], NAME_OF, True) == ["4<-e,0>2<-e,0>1", "4<-f,-1>3<-e,7>1"]
    assert A.layered_dag(diamond, [9], [4], [1], False, 3) == {} and A.levels(diamond, [9], [4], [1], False, 3) == (2, 0)
    assert A.levels(diamond, [1], [9], [1], False, 3) == (0, 1)  # no target row: layer 0 runs and emits nothing


# ----------------------------------------------------------------------------- the reference's answers
GOLDEN = [c for c in CASES if c["kind"] in ("ALL", "NOLOOP") and c["direction"] != "BIDIRECT" and not c.get("error")
          and not c.get("piped")]


def nba_edges():
    d = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "nba.json")))
    vid, types = ngql.nebula_hash, d["edge_types"]
    edges = [(vid(p), vid(t), types["serve"], rank) for p, t, rank, _, _ in d["serve"]]
    edges += [(vid(p), vid(o), types["like"], 0) for p, o, _ in d["like"]]
    edges += [(vid(p), vid(o), types["teammate"], 0) for p, o, _, _ in d["teammate"]]
    vertices = {vid(p) for p, _ in d["players"]} | {vid(t) for t in d["teams"]}
    return edges, vertices, types


@pytest.mark.parametrize("case", GOLDEN, ids=[f"path{c['line']}" for c in GOLDEN])
def test_known_answers_through_the_layers(case):
    edges, vertices, types = nba_edges()
    s = ngql.parse_find_path(golden_text(case["query"]))
    assert s.kind == case["kind"] and s.from_type == 0 and s.to_type == 0
    over = sorted(types.values()) if s.over_all else [types[n] for n, _ in s.over]
    dag = A.layered_dag(edges, s.from_vids, s.to_vids, over, s.direction == ngql.REVERSELY, s.upto, vertices)
    names = {t: n for n, t in types.items()}
    got = rows_from_layers(dag, s.from_vids, s.to_vids, names, case["kind"] == "NOLOOP")
    assert got == sorted(golden_text(p) for p in case["paths"])


def test_golden_cases_are_there():
    assert {(c["kind"], c["direction"]) for c in GOLDEN} == {(k, d) for k in ("ALL", "NOLOOP") for d in ("", "REVERSELY")}
