"""A model of FIND SHORTEST PATH that shares nothing with the code under test, the seeded graphs it is run on, and
the loader the device tests put those graphs into an Engine with.

The model is plain breadth-first search over an edge list `(src vid, dst vid, type, rank)`:
  ds[v]    the multi-source distance from the source set along the sentence's direction;
  dt_j[v]  per target j, the distance to it (a search from the target against that direction);
  L_j      ds[target j]. Target j is found iff 1 <= L_j <= UPTO.
A step `u -> v` of the sentence's direction lies on a shortest path to target j iff j is found and
ds[u] + 1 + dt_j[v] == L_j. FORWARD a step is the edge itself, `(src, dst, +type, rank)`; REVERSELY the stored edge
`a -> b` is the step `b -> a` and prints as `(b, a, -type, rank)`: the orientation and the sign of PathEdge.
Vids without a vertex take no part: they start no search and no edge is followed into them.
"""
import random
from collections import deque, namedtuple

import numpy as np

from nebula_amd import engine, kvfmt, pipeline
from tests import fixtures

INF = 1 << 30
Dist = namedtuple("Dist", "steps ds dt L sources targets")
Dag = namedtuple("Dag", "edges found levels L from_sizes to_sizes")


# ----------------------------------------------------------------------------- the model
def _bfs(adj, starts):
    dist = {}
    q = deque()
    for v in starts:
        if v not in dist:
            dist[v] = 0
            q.append(v)
    while q:
        u = q.popleft()
        for v in adj.get(u, ()):
            if v not in dist:
                dist[v] = dist[u] + 1
                q.append(v)
    return dist


def distances(edges, sources, targets, over_types, reversely, vertices=None):
    """The three distances of the module docstring, for every UPTO at once. vertices: the vids that have a vertex
    (default: every endpoint of an edge)."""
    if vertices is None:
        vertices = {x[0] for x in edges} | {x[1] for x in edges}
    vertices = set(vertices)
    over = set(over_types)
    steps = []
    for a, b, t, r in edges:
        if t in over and a in vertices and b in vertices:
            steps.append((b, a, -t, r) if reversely else (a, b, t, r))
    fwd, bwd = {}, {}
    for u, v, _, _ in steps:
        fwd.setdefault(u, []).append(v)
        bwd.setdefault(v, []).append(u)
    ds = _bfs(fwd, [s for s in sources if s in vertices])
    dt = [_bfs(bwd, [t] if t in vertices else []) for t in targets]
    L = [ds.get(t, INF) for t in targets]
    return Dist(steps, ds, dt, L, list(sources), list(targets))


def levels_expanded(dist, upto, found_at):
    """ngx_path_result.levels, from the driver's rule ("Levels"): step k = 1 .. ceil(UPTO / 2) ends the
    search before anything else when level k - 1 of either side is empty (the from side's level d is the vertices at
    ds == d, the to side's the vertices at dt_j == d for any target j, found or not: found targets are expanded on);
    then the odd meet finds the targets with L_j == 2k - 1; the search ends if every target (a vid without a vertex
    is one, and is never found) is found or 2k > UPTO; otherwise both sides expand one level (levels += 2) and the
    even meet finds the targets with L_j == 2k; the search ends if every target is found."""
    nf, nt = level_sizes(dist)
    n_targets = len(dist.targets)
    found, levels = set(), 0
    for k in range(1, upto // 2 + upto % 2 + 1):
        if nf.get(k - 1, 0) == 0 or nt.get(k - 1, 0) == 0:
            break
        found |= found_at.get(2 * k - 1, set())
        if len(found) == n_targets or 2 * k > upto:
            break
        levels += 2
        found |= found_at.get(2 * k, set())
        if len(found) == n_targets:
            break
    return levels


def level_sizes(dist):
    """({d: vertices at ds == d}, {d: vertices at dt_j == d for some j}) as counts."""
    nf, at = {}, {}
    for d in dist.ds.values():
        nf[d] = nf.get(d, 0) + 1
    for dt in dist.dt:
        for v, d in dt.items():
            at.setdefault(d, set()).add(v)
    return nf, {d: len(s) for d, s in at.items()}


def dag_from(dist, upto):
    """Dag of one UPTO: edges {(src, dst, signed type, rank): mask}, the found mask, levels expanded, L_j (INF: not
    reached), and the level sizes of both sides."""
    found_js = [j for j, l in enumerate(dist.L) if 1 <= l <= upto]
    edges = {}
    if found_js and dist.steps:
        index = {}
        for u, v, _, _ in dist.steps:
            index.setdefault(u, len(index))
            index.setdefault(v, len(index))
        ds = np.full(len(index), INF, np.int64)
        for v, d in dist.ds.items():
            if v in index:
                ds[index[v]] = d
        dt = np.full((len(found_js), len(index)), INF, np.int64)
        for k, j in enumerate(found_js):
            for v, d in dist.dt[j].items():
                if v in index:
                    dt[k, index[v]] = d
        U = np.array([index[s[0]] for s in dist.steps])
        V = np.array([index[s[1]] for s in dist.steps])
        want = np.array([dist.L[j] for j in found_js], np.int64)[:, None]
        on = (ds[U][None, :] + 1 + dt[:, V]) == want
        for k, i in zip(*np.nonzero(on)):
            key = dist.steps[i]
            edges[key] = edges.get(key, 0) | (1 << found_js[k])
    found = sum(1 << j for j in found_js)
    found_at = {}
    for j in found_js:
        found_at.setdefault(dist.L[j], set()).add(j)
    nf, nt = level_sizes(dist)
    return Dag(edges, found, levels_expanded(dist, upto, found_at), list(dist.L), nf, nt)


def shortest_dag(edges, sources, targets, over_types, reversely, upto, vertices=None):
    return dag_from(distances(edges, sources, targets, over_types, reversely, vertices), upto)


def dag_tuples(dag):
    """{(src, dst, type, rank, bit)} of a model's edges."""
    out = set()
    for key, mask in dag.items():
        j = 0
        while mask >> j:
            if mask >> j & 1:
                out.add(key + (j,))
            j += 1
    return out


def _adj(dag, j):
    adj = {}
    for (u, v, t, r), mask in dag.items():
        if mask >> j & 1:
            adj.setdefault(u, []).append((v, t, r))
    return adj


def count_paths(dag, sources, j):
    """Paths to target j: walks over its edges from a source to a vertex none of them leaves, counted per vertex."""
    adj = _adj(dag, j)
    memo = {}
    for s in set(sources):
        stack = [s] if s in adj else []
        while stack:                                              # depth first without recursion: 500 edges deep
            v = stack[-1]
            if v in memo and memo[v] >= 0:
                stack.pop()
                continue
            todo = [d for d, _, _ in adj[v] if d in adj and memo.get(d, -1) < 0]
            if todo:
                assert v not in memo, "a cycle in the model's DAG"
                memo[v] = -1
                stack += todo
            else:
                memo[v] = sum(memo[d] if d in adj else 1 for d, _, _ in adj[v])
                stack.pop()
    return sum(memo[s] for s in set(sources) if s in adj)


def render_paths(dag, sources, targets, names):
    """Every path as `vid<edge,rank>vid...` (`-edge` for a negative type), sorted. names: {type: edge name}."""
    out = []
    for j, target in enumerate(targets):
        adj = _adj(dag, j)
        stack = [(s, str(s)) for s in set(sources) if s in adj]
        while stack:
            v, text = stack.pop()
            if v == target:
                out.append(text)
                continue
            for d, t, r in adj.get(v, ()):
                stack.append((d, "%s<%s%s,%d>%d" % (text, "-" if t < 0 else "", names[abs(t)], r, d)))
    return sorted(out)


# ----------------------------------------------------------------------------- seeded graphs
RANK_FORMS = ("const", "int8", "int16", "int32", "int64")
_BITS = {"int8": 8, "int16": 16, "int32": 32, "int64": 64}
_CONSTS = (5, -1, 300, -70000, 1 << 40)

Graph = namedtuple("Graph", "vids edges forms hubs isolated")


def rank_form(ranks):
    """How a slot with these ranks is stored: one value for all, else the narrowest signed width that holds them."""
    ranks = list(ranks)
    if len(set(ranks)) == 1:
        return "const"
    lo, hi = min(ranks + [0]), max(ranks + [0])
    for form in RANK_FORMS[1:]:
        b = _BITS[form]
        if lo >= -(1 << (b - 1)) and hi < 1 << (b - 1):
            return form
    raise ValueError("rank outside int64")


def random_graph(seed, nv, hub_degrees=(70, 300), hubs=None):
    """Graph(vids, edges, forms, hubs, isolated): nv vertices with scattered vids; edges `(src vid, dst vid, type,
    rank)` of types 1 and 2, no two equal, mean out-degree about 1.5; `hubs` rows (2 or 3 by default) with between
    hub_degrees[0] and hub_degrees[1] out-edges of one type into six vertices each (parallel edges that differ in
    rank only, so the hubs shorten nothing); three self-loops; parallel edges that differ in type only or in rank
    only; three vertices without edges. forms[type] is the slot's rank storage form: type 1 takes
    RANK_FORMS[seed % 5], type 2 RANK_FORMS[(seed + 2) % 5], each with its extremes present."""
    rng = random.Random(seed * 7919 + nv)
    vids = sorted(rng.sample(range(1, 10 * nv + 1), nv))
    forms = {1: RANK_FORMS[seed % 5], 2: RANK_FORMS[(seed + 2) % 5]}
    const = {t: _CONSTS[(seed + t) % len(_CONSTS)] for t in (1, 2)}

    def span(t):
        b = _BITS[forms[t]]
        return -(1 << (b - 1)), (1 << (b - 1)) - 1

    palette = {}
    for t in (1, 2):
        if forms[t] == "const":
            palette[t] = [const[t]]
        else:
            lo, hi = span(t)
            palette[t] = [lo, hi, -1, 0, 1, lo // 2 - 1, hi // 2 + 1, rng.randrange(lo, hi + 1)]
    shuffled = vids[:]
    rng.shuffle(shuffled)
    isolated, live = shuffled[:3], shuffled[3:]
    edges = set()
    for u in live:
        for _ in range(rng.choice((0, 1, 1, 2, 2, 3))):
            t = rng.choice((1, 2))
            edges.add((u, rng.choice(live), t, rng.choice(palette[t])))
    for u in rng.sample(live, 3):                                 # self-loops
        t = rng.choice((1, 2))
        edges.add((u, u, t, rng.choice(palette[t])))
    for u, v, t, r in rng.sample(sorted(edges), min(10, len(edges))):
        edges.add((u, v, 3 - t, rng.choice(palette[3 - t])))      # the same pair over the other type
        if forms[t] != "const":
            edges.add((u, v, t, rng.choice([x for x in palette[t] if x != r])))
    wide = [t for t in (1, 2) if forms[t] != "const"]
    hub_rows = rng.sample(live, hubs if hubs is not None else rng.choice((2, 3)))
    for k, hub in enumerate(hub_rows):
        t = wide[k % len(wide)]
        lo, hi = span(t)
        deg = rng.randint(*hub_degrees) if k else hub_degrees[1]  # the first hub is the widest
        deg -= sum(1 for e in edges if e[0] == hub)
        pool = rng.sample(live, 6)
        per = [deg // 6 + (1 if i < deg % 6 else 0) for i in range(6)]
        for v, n in zip(pool, per):
            ranks = set()
            while len(ranks) < n:
                ranks.add(rng.randrange(lo, hi + 1))
            have = {r for a, b, tt, r in edges if (a, b, tt) == (hub, v, t)}
            for r in sorted(ranks - have):
                edges.add((hub, v, t, r))
    edges = sorted(edges)
    for t in (1, 2):                                              # each slot is stored as its form says
        assert rank_form([e[3] for e in edges if e[2] == t]) == forms[t], (seed, t)
        if forms[t] != "const":
            assert {span(t)[0], span(t)[1]} <= {e[3] for e in edges if e[2] == t}, (seed, t)
        else:
            assert const[t] != 0
    return Graph(vids, edges, forms, hub_rows, isolated)


def missing_vids(graph, n, seed=0):
    """n vids of the graph's range that have no vertex."""
    have = set(graph.vids)
    rng = random.Random(seed + 1)
    out = []
    while len(out) < n:
        v = rng.randrange(1, 10 * len(graph.vids) + 1)
        if v not in have and v not in out:
            out.append(v)
    return out


# ----------------------------------------------------------------------------- loading an Engine, shared helpers
EDGES = ["e", "f"]
SCHEMA = [fixtures.SchemaDef(True, 1, "e", [("p0", kvfmt.INT)]), fixtures.SchemaDef(True, 2, "f", [("p0", kvfmt.INT)])]
_space = [100]


def _key(x):
    return (x & (1 << 64) - 1).to_bytes(8, "little")


def load(e, nv, edges, num_parts=1, vpart=None, vids=None, schema=SCHEMA):
    """edges: (src row, dst row, type, rank), row r being vid r + 1; with `vids` (the vertex table's vids) a plain
    edge list (src vid, dst vid, type, rank) instead, and nv is not read. Every type is loaded with its exact
    transpose. vpart: the part of each entry of vids (default: vid % num_parts + 1, the space's own rule).
    Returns the space."""
    _space[0] += 1
    space = _space[0]
    e.add_space(space, num_parts)
    for s in schema:
        e.add_schema(space, s.is_edge, s.sid, s.name, s.fields, s.ver, s.ttl_col, s.ttl_dur)
    if vids is None:
        vids = list(range(1, nv + 1))
        edges = [(a + 1, b + 1, t, r) for a, b, t, r in edges]
    if vpart is None:
        vpart = [v % num_parts + 1 for v in vids]
    table = sorted(zip(vpart, vids))
    row = {v: i for i, (_, v) in enumerate(table)}
    nv = len(table)
    slots = []
    for t in sorted({x[2] for x in edges}):
        for sign in (1, -1):
            rows = [[] for _ in range(nv)]
            for a, b, tt, r in edges:
                if tt == t:
                    (rows[row[a]] if sign > 0 else rows[row[b]]).append((r, b if sign > 0 else a))
            off, dst, rank = [0], [], []
            for lst in rows:
                for r, d in sorted(lst, key=lambda x: (_key(x[0]), _key(x[1]))):
                    dst.append(d)
                    rank.append(r)
                off.append(len(dst))
            slots.append((sign * t, np.array(off, np.uint64), np.array(dst, np.int64), [np.zeros(len(dst), np.int64)],
                          np.array(rank, np.int64)))
    e.load_csr(space, np.array([p for p, _ in table], np.int32), np.array([v for _, v in table], np.int64), slots)
    e.commit(space)
    return space


def refused(e, space, q, reason):
    """The device call refuses with `reason`; the pipeline answers from the host restatement."""
    r = e.find_path(space, q)
    assert not r.ok and r.code == engine.E_UNSUPPORTED and r.error.startswith("find path:") and reason in r.error, r.error
    before = e.get_flag("find_path_device")
    p = pipeline.Pipeline(e, space, EDGES, find_path=True)
    out = p.run(q)
    assert out.ok and p.find_path_fallbacks == 1 and e.get_flag("find_path_device") == before
    host = pipeline.run(e, space, q, EDGES, find_path=True, device_find_path=False)
    assert sorted(out.rows) == sorted(host.rows)
    return sorted(r[0][1] for r in out.rows)


# ----------------------------------------------------------------------------- the device test's cases
# Shared by tests/test_gpu_findpath_dag.py (which runs them) and tests/test_pathref_host.py (which asserts on the
# model alone that they reach the depths, meets and rank forms they are there for).
GPU_SEEDS = tuple(range(24))
GPU_NV = 300
GPU_UPTOS = (1, 2, 3, 7, 8, 15)
TYPE_OF = {"e": 1, "f": 2}
NAME_OF = {1: "e", 2: "f"}
Case = namedtuple("Case", "seed graph sources targets num_parts")
_cases, _dists = {}, {}


def gpu_case(seed):
    """1 .. 4 sources and 1 .. 64 targets of random_graph(seed, 300): seeds 0 .. 3 with exactly 64 targets, 4 and 5
    with 63. The first two targets are one step from the first source, one along an edge and one against one, so
    that UPTO 1 finds something in either direction. Odd seeds list a vid without a vertex on both sides (inside the
    counts above). Even seeds are loaded into 1 part, odd seeds into 7."""
    if seed not in _cases:
        g = random_graph(seed, GPU_NV)
        rng = random.Random(1000 + seed)
        out = {}
        inn = {}
        for a, b, t, _ in g.edges:
            if a != b and t == 2:                                 # over f: found by `OVER f` and by `OVER e, f`
                out.setdefault(a, []).append(b)
                inn.setdefault(b, []).append(a)
        both = sorted(v for v in out if v in inn and set(out[v]) != set(inn[v]))
        n_s = 1 if seed % 4 == 0 else rng.randint(1, 4)
        n_t = 64 if seed < 4 else 63 if seed < 6 else 1 if seed == 6 else rng.choice((2, 5, 9, 17, 33, 48))
        first = rng.choice(both)
        near = [rng.choice(out[first])]
        near += [rng.choice([v for v in inn[first] if v != near[0]])]
        near = near[:n_t]
        missing = missing_vids(g, 2, seed) if seed % 2 else []
        n_miss = 1 if missing and n_t > 2 else 0
        rest = [v for v in g.vids if v != first and v not in near]
        rng.shuffle(rest)
        sources = [first] + rest[:n_s - 1 - (1 if missing and n_s > 1 else 0)]
        if missing and n_s > 1:
            sources.insert(1, missing[0])
        rest = rest[n_s:]
        targets = near + rest[:n_t - len(near) - n_miss]
        if n_miss:
            targets.insert(len(targets) // 2, missing[1])
        assert len(sources) == n_s and len(targets) == n_t and not set(sources) & set(targets)
        assert len(set(sources)) == n_s and len(set(targets)) == n_t
        _cases[seed] = Case(seed, g, sources, targets, 7 if seed % 2 else 1)
    return _cases[seed]


def gpu_queries(seed):
    """(reversely, OVER names, upto): both directions x GPU_UPTOS over `e, f`; every third seed over `f` alone too."""
    overs = [("e", "f")] + ([("f",)] if seed % 3 == 0 else [])
    return [(rev, over, upto) for over in overs for rev in (False, True) for upto in GPU_UPTOS]


def sentence(sources, targets, over, reversely, upto):
    return "FIND SHORTEST PATH FROM %s TO %s OVER %s%s UPTO %d STEPS" % (
        ", ".join(map(str, sources)), ", ".join(map(str, targets)), ", ".join(over), " REVERSELY" if reversely else "", upto)


def gpu_dist(seed, reversely, over):
    key = (seed, reversely, over)
    if key not in _dists:
        c = gpu_case(seed)
        _dists[key] = distances(c.graph.edges, c.sources, c.targets, [TYPE_OF[n] for n in over], reversely, c.graph.vids)
    return _dists[key]


def gpu_model(seed, reversely, over, upto):
    return dag_from(gpu_dist(seed, reversely, over), upto)
