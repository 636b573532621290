"""A model of FIND ALL PATH and FIND NOLOOP PATH that shares nothing with the kernels or with nebula_amd/findpath.py,
and the seeded graphs the tests run it on.

An edge list holds `(src vid, dst vid, type, rank)`. A step of the sentence's direction is, FORWARD, the edge itself
`(src, dst, +type, rank)`; REVERSELY the stored edge `a -> b` is the step `b -> a` and prints as `(b, a, -type, rank)`.
Only edges of the OVER types between vids that have a vertex make steps.

  walks        plain depth-first enumeration: every walk of 1 .. UPTO steps from a source to a target, each once; a
               walk may repeat vertices and steps and may pass through a target and go on. `simple` keeps the walks
               whose vertices are all distinct.
  layered_dag  from plain breadth-first distances dist(v, t_j): U_0 = the sources that are vertices; layer i holds
               every step u -> v with u in U_i and a non-empty m = {j : dist(v, t_j) <= UPTO - 1 - i}, as
               {(i, u, v, type, rank): m}; U_(i+1) = the heads of layer i's steps while i + 1 < UPTO.
  levels       (to-side depths expanded, from-side layers launched), the driver's rule.
"""
import random
from collections import deque, namedtuple

INF = 1 << 30


def steps_of(edges, over_types, reversely, vertices=None):
    if vertices is None:
        vertices = {x[0] for x in edges} | {x[1] for x in edges}
    vertices, over = set(vertices), set(over_types)
    out = []
    for a, b, t, r in edges:
        if t in over and a in vertices and b in vertices:
            out.append((b, a, -t, r) if reversely else (a, b, t, r))
    return out, vertices


def _adj(steps):
    adj = {}
    for u, v, t, r in steps:
        adj.setdefault(u, []).append((v, t, r))
    return adj


def walks(edges, sources, targets, over_types, reversely, upto, simple, vertices=None):
    """Every walk as a tuple of steps `(u, v, signed type, rank)`."""
    steps, vertices = steps_of(edges, over_types, reversely, vertices)
    adj = _adj(steps)
    goal = set(targets)
    out = []

    def extend(v, walk, on):
        if walk and v in goal:
            out.append(tuple(walk))
        if len(walk) == upto:
            return
        for w, t, r in adj.get(v, ()):
            if simple and w in on:
                continue
            walk.append((v, w, t, r))
            if simple:
                on.add(w)
            extend(w, walk, on)
            walk.pop()
            if simple:
                on.discard(w)

    for s in sources:
        if s in vertices:
            extend(s, [], {s})
    return out


def render(walk, names):
    """`vid<edge,rank>vid...`, `-edge` for a negative type. names: {type: edge name}."""
    text = str(walk[0][0])
    for _, v, t, r in walk:
        text += "<%s%s,%d>%d" % ("-" if t < 0 else "", names[abs(t)], r, v)
    return text


def _dist_to(steps, vertices, targets):
    """Per target j {v: dist(v, t_j)}: a breadth-first search from t_j against the steps."""
    back = {}
    for u, v, _, _ in steps:
        back.setdefault(v, []).append(u)
    out = []
    for t in targets:
        dist = {}
        if t in vertices:
            dist[t] = 0
            q = deque([t])
            while q:
                x = q.popleft()
                for y in back.get(x, ()):
                    if y not in dist:
                        dist[y] = dist[x] + 1
                        q.append(y)
        out.append(dist)
    return out


def _layers(edges, sources, targets, over_types, reversely, upto, vertices):
    steps, vertices = steps_of(edges, over_types, reversely, vertices)
    adj = _adj(steps)
    dist = _dist_to(steps, vertices, targets)
    dag, sizes = {}, []
    rows = {s for s in sources if s in vertices}
    for i in range(upto):
        if not rows:
            break
        sizes.append(len(rows))
        nxt = set()
        for u in rows:
            for v, t, r in adj.get(u, ()):
                m = sum(1 << j for j, d in enumerate(dist) if d.get(v, INF) <= upto - 1 - i)
                if m:
                    dag[(i, u, v, t, r)] = m
                    if i + 1 < upto:
                        nxt.add(v)
        rows = nxt
    return dag, sizes, dist


def layered_dag(edges, sources, targets, over_types, reversely, upto, vertices=None):
    return _layers(edges, sources, targets, over_types, reversely, upto, vertices)[0]


def levels(edges, sources, targets, over_types, reversely, upto, vertices=None):
    """The to side expands depth d = 1 .. UPTO - 1 while some (vertex, target) pair lies at distance exactly d - 1;
    the from side launches layer i = 0 .. UPTO - 1 while U_i is not empty."""
    _, sizes, dist = _layers(edges, sources, targets, over_types, reversely, upto, vertices)
    at = {d for per in dist for d in per.values()}
    depths = 0
    for d in range(1, upto):
        if d - 1 not in at:
            break
        depths += 1
    return depths, len(sizes)


def layer_sizes(edges, sources, targets, over_types, reversely, upto, vertices=None):
    return _layers(edges, sources, targets, over_types, reversely, upto, vertices)[1]


def count(dag, sources, targets):
    """The ALL walks of a layered DAG, by layers: walks ending at each vertex, summed where it is a target."""
    goal, ends, total = set(targets), {s: 1 for s in sources}, 0
    for i in range(max(k[0] for k in dag) + 1 if dag else 0):
        nxt = {}
        for (layer, u, v, _, _) in dag:
            if layer == i and u in ends:
                nxt[v] = nxt.get(v, 0) + ends[u]
        total += sum(n for v, n in nxt.items() if v in goal)
        ends = nxt
    return total


def sentence(kind, sources, targets, over, reversely, upto):
    return "FIND %s PATH FROM %s TO %s OVER %s%s UPTO %d STEPS" % (
        kind, ", ".join(map(str, sources)), ", ".join(map(str, targets)), ", ".join(over), " REVERSELY" if reversely else "", upto)


def found(dag, targets):
    """Bit j: some step of the DAG ends at targets[j]."""
    heads = {k[2] for k in dag}
    return sum(1 << j for j, t in enumerate(targets) if t in heads)


# ----------------------------------------------------------------------------- seeded graphs
Graph = namedtuple("Graph", "vids edges cycle isolated")
RANKS = (0, 0, 1, -1, 7, -(1 << 40))


def random_graph(seed, nv, degree=4, fanout=(0, 1, 1, 2, 2, 3)):
    """Graph(vids, edges, cycle, isolated): nv vertices with scattered vids, edges of types 1 and 2 with no vertex
    above `degree` out-edges or in-edges (so a sentence of UPTO n has at most degree + ... + degree^n walks a
    source); a 3-cycle `cycle` = (a, b, c) with a -> b -> c -> a over type 1 and a chord out of it; two self-loops;
    parallel edges that differ in rank only and in type only; two vertices without edges. fanout: what a vertex's
    number of random out-edges is drawn from."""
    rng = random.Random(seed * 104729 + nv)
    vids = sorted(rng.sample(range(1, 10 * nv + 1), nv))
    shuffled = vids[:]
    rng.shuffle(shuffled)
    isolated, live = shuffled[:2], shuffled[2:]
    edges, out, inn = set(), {}, {}

    def add(a, b, t, r):
        if (a, b, t, r) in edges or out.get(a, 0) >= degree or inn.get(b, 0) >= degree:
            return False
        edges.add((a, b, t, r))
        out[a] = out.get(a, 0) + 1
        inn[b] = inn.get(b, 0) + 1
        return True

    a, b, c = live[:3]
    for u, v in ((a, b), (b, c), (c, a)):
        add(u, v, 1, 0)
    add(b, live[3], 2, 1)
    for u in live:
        for _ in range(rng.choice(fanout)):
            add(u, rng.choice(live), rng.choice((1, 2)), rng.choice(RANKS))
    loops = 0
    for u in rng.sample(live, len(live)):
        if loops < 2 and add(u, u, rng.choice((1, 2)), rng.choice(RANKS)):
            loops += 1
    twins = 0
    for u, v, t, r in rng.sample(sorted(edges), len(edges)):
        if twins < 4 and u != v:
            twins += add(u, v, 3 - t, r) + add(u, v, t, r + 3)
    return Graph(vids, sorted(edges), (a, b, c), isolated)


def missing_vids(graph, n, seed=0):
    have = set(graph.vids)
    rng = random.Random(seed + 17)
    out = []
    while len(out) < n:
        v = rng.randrange(1, 10 * len(graph.vids) + 1)
        if v not in have and v not in out:
            out.append(v)
    return out
