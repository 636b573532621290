"""FIND SHORTEST | ALL | NOLOOP PATH: host-side restatement of graphd's FindPathExecutor
(src/graph/FindPathExecutor.cpp), as it is written.

  - setupVids / setupVidsFromRef (:492-537): FROM / TO read literal vids, the pipe's input (`$-.col`) or a
    variable (`$var.col`): `Variable `%s' not defined`, `Duplicate column `%s'` (checkIfDuplicateColumn on the
    pipe's input), getDistinctVIDs' `Interim has no data.` and `Column `%s' not found`. `$-` without a pipe is
    no error: no vids, no rows;
  - execute (:159-182): steps_ = N / 2 + N % 2; one empty walk per from vid in pathFrom_ and per to vid in
    pathTo_ (both std::multimap, kept as such: a vid listed twice starts two walks);
  - getNeighborsAndFindPath (:184-227): a side without vids ends the search; each step asks the neighbours of
    the from-side vids over the types getStepOutProps(false) gives and of the to-side vids over
    getStepOutProps(true) (:683-736; FORWARD: the edge types / the opposite ones, REVERSELY the other way round,
    BIDIRECT both for both), with `_dst`, `_type` and `_rank`. Here a side's neighbours are one-step GO
    sentences from its vids, one per OVER edge, yielding `_src`, `_dst`, `_type`, `_rank`: what the reference
    reads from storage, and it runs unchanged over the Engine and over the oracle;
  - findPath (:229-305): every kept walk is extended by every neighbour (updatePath under isPathAcceptable:
    BIDIRECT never steps back over the edge it came by, NOLOOP never revisits a vertex of the walk); a from-side
    neighbour inside the to-side's previous vid set meets an odd path (meetOddPath), the two new vid sets'
    intersection meets the even ones (meetEvenPath), each under its length check and ABA check;
  - SHORTEST (FindPathSentence(true, true): also NOLOOP): a path is skipped when finalPath_'s first entry for
    its target is shorter; the search ends once targetNotFound_ is empty;
  - setupResponse / buildPathRow (:751-843): one column `_path_`; a NOLOOP row that repeats a vertex is dropped;
    the steps after the turning point print their type negated.
A path is a cell ("path", text) with the reference's test rendering (TraverseTestBase.h buildPathString):
`vid<edge,rank>vid...`, a reverse edge as `-edge`.
FindPathExecutor hands no result on: it never calls onResult_ and finishes with doFinish(kNext), so the sentence
piped behind FIND PATH runs with inputs_ == nullptr. pipeline.py does the same: the next sentence gets no input.
These functions serve every backend and are the specification of the device path (ngx_find_path,
include/nebula_gn.h); paths_from_dag turns that call's path-DAG edges into the same rows for SHORTEST, and
paths_from_layers its layered edges for ALL and NOLOOP.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import ngql

T_PATH = 41                                                       # nebula::cpp2::SupportedType::PATH


class FindPathError(Exception):
    """A failed Status of the executor; str() is the outcome's error text."""


class FindPathRefusal(FindPathError):
    """The device answer is not turned into rows here (text `find path: ...`): the caller runs the restatement."""


# ----------------------------------------------------------------------------- FROM / TO
def _distinct_vids(interim, col: str) -> List[int]:
    """InterimResult::getDistinctVIDs (InterimResult.cpp:51-72)."""
    if not interim.rows:
        raise FindPathError("Interim has no data.")
    if col not in interim.names:
        raise FindPathError("Column `%s' not found" % col)
    i = interim.names.index(col)
    out, seen = [], set()
    for row in interim.rows:
        kind, v = row[i]
        if kind not in ("int", "id", "timestamp"):
            raise FindPathError("Column `%s' not found" % col)
        if v not in seen:
            seen.add(v)
            out.append(int(v))
    return out


def setup_vids(s: ngql.FindPathSentence, inp, variables: Dict[str, object]) -> Tuple[List[int], List[int]]:
    """(from vids, to vids) of the sentence; `inp` is the pipe's Interim or None."""
    out = []
    for vids, typ, var, col in ((s.from_vids, s.from_type, s.from_var, s.from_col), (s.to_vids, s.to_type, s.to_var, s.to_col)):
        if typ == 0:
            out.append(list(vids))
            continue
        if typ == 1:
            if inp is None:                                       # inputs_ == nullptr: Status::OK, no vids
                out.append([])
                continue
            src = inp
        else:
            if var not in variables:
                raise FindPathError("Variable `%s' not defined" % var)
            src = variables[var]
        if inp is not None:                                       # checkIfDuplicateColumn reads the pipe's input
            seen = set()
            for n in inp.names:
                if n in seen:
                    raise FindPathError("Duplicate column `%s'" % n)
                seen.add(n)
        out.append(_distinct_vids(src, col))
    return out[0], out[1]


# ----------------------------------------------------------------------------- neighbours
def _neighbours(backend, space: int, s: ngql.FindPathSentence, edge_names: Sequence[str], vids: Sequence[int],
                reversely: bool, names: Dict[int, str], go_kw) -> List[Tuple[int, List[Tuple[int, int, int]]]]:
    """Frontiers of one side: (vertex, [(dst, signed type, rank)]) per vertex and edge type, from one-step GOs."""
    direction = s.direction
    if direction != ngql.BIDIRECT and reversely:
        direction = ngql.REVERSELY if direction == ngql.FORWARD else ngql.FORWARD
    over = [(n, "") for n in edge_names] if s.over_all else [(n, "") for n, _ in s.over]
    seen = set()
    for n, a in (s.over if not s.over_all else []):               # prepareOver: expCtx_->addEdge(alias or name)
        key = a or n
        if key in seen:
            raise FindPathError("edge alias(%s) was dup" % key)
        seen.add(key)
    frontiers: Dict[Tuple[int, int], List[Tuple[int, int, int]]] = {}
    order = []
    for name, _ in over:
        g = ngql.GoSentence(vids=list(vids), over=[(name, "")], direction=direction)
        g.yields = [ngql.YieldCol(ngql.Prop(k, "", name, p)) for k, p in
                    ((ngql.K_EDGE_SRC, "_src"), (ngql.K_EDGE_DST, "_dst"), (ngql.K_EDGE_TYPE, "_type"), (ngql.K_EDGE_RANK, "_rank"))]
        r = backend.go(space, g, **go_kw)
        if not r.ok:
            raise FindPathError(r.error)
        for row in r.rows:
            src, dst, typ, rank = (int(c[1]) for c in row)
            names[abs(typ)] = name
            key = (src, typ)
            if key not in frontiers:
                frontiers[key] = []
                order.append(key)
            frontiers[key].append((dst, typ, rank))
    return [(k[0], frontiers[k]) for k in order]


class _MultiMap:
    """std::multimap<VertexID, Path>: entries of one key in insertion order."""

    def __init__(self):
        self.d: Dict[int, List[tuple]] = {}

    def emplace(self, k, v):
        self.d.setdefault(k, []).append(v)

    def range(self, k):
        return self.d.get(k, ())


# ----------------------------------------------------------------------------- the executor
def find_path(backend, space: int, s: ngql.FindPathSentence, from_vids: Sequence[int], to_vids: Sequence[int],
              edge_names: Sequence[str] = (), **go_kw) -> List[str]:
    """The sentence's paths, rendered, in finalPath_ order (by target, then as found)."""
    n_max = s.upto
    steps = n_max // 2 + n_max % 2
    shortest, no_loop, bidirect = s.shortest, s.no_loop, s.direction == ngql.BIDIRECT
    names: Dict[int, str] = {}
    cur_from, cur_to = list(from_vids), list(to_vids)
    visited_to = set(cur_to)
    not_found = set(cur_to)
    path_from, path_to = _MultiMap(), _MultiMap()
    for v in cur_from:
        path_from.emplace(v, ())
    for v in cur_to:
        path_to.emplace(v, ())
    final: Dict[int, List[tuple]] = {}                            # finalPath_: per target, in the order found

    def acceptable(path, nb, by_from) -> bool:                    # isPathAcceptable
        if not path:
            return True
        this_id, this_edge, this_rank = nb
        if bidirect:
            last = path[-1] if by_from else path[0]
            if last[0] == this_id and last[1] == -this_edge and last[2] == this_rank:
                return False
        if no_loop and any(step[0] == this_id for step in path):
            return False
        return True

    def update(src, paths, nb, out, by_from) -> bool:             # updatePath
        updated = False
        for path in paths.range(src):
            if not acceptable(path, nb, by_from):
                continue
            step = (src, nb[1], nb[2])
            out.emplace(nb[0], path + (step,) if by_from else (step,) + path)
            updated = True
        return updated

    def found(path, odd):
        target = path[-1][0]
        if shortest:
            if odd:
                not_found.discard(target)
            have = final.get(target)
            if have and len(have[0]) < len(path):                 # already found a shorter path
                return
            if not odd:
                not_found.discard(target)
        final.setdefault(target, []).append(path)

    step_no = 1
    while cur_from and cur_to:                                    # getNeighborsAndFindPath: a dead end finishes
        f_front = _neighbours(backend, space, s, edge_names, cur_from, False, names, go_kw)
        t_front = _neighbours(backend, space, s, edge_names, cur_to, True, names, go_kw)
        visited_from, path_f = set(), _MultiMap()
        for src, nbs in f_front:
            for nb in nbs:
                dst = nb[0]
                if update(src, path_from, nb, path_f, True):
                    visited_from.add(dst)
                    if dst in visited_to:                         # meetOddPath
                        for pi in path_from.range(src):
                            for pj in path_to.range(dst):
                                if len(pj) + len(pi) > n_max:
                                    continue
                                if not acceptable(pj, (src, -nb[1], nb[2]), False):
                                    continue
                                found(pi + ((src, nb[1], nb[2]), (dst, -nb[1], nb[2])) + pj, True)
        path_from = path_f
        cur_from = sorted(visited_from)
        visited_to, path_t = set(), _MultiMap()
        for src, nbs in t_front:
            for nb in nbs:
                if update(src, path_to, nb, path_t, False):
                    visited_to.add(nb[0])
        path_to = path_t
        cur_to = sorted(visited_to)
        meet = sorted(visited_from & visited_to)
        if meet:
            if shortest and not not_found:
                break
            for v in meet:                                        # meetEvenPath
                for pi in path_from.range(v):
                    for pj in path_to.range(v):
                        if len(pj) + len(pi) > n_max:
                            continue
                        path = pi
                        if pj:
                            st = pj[0]
                            if not acceptable(pi, (st[0], -st[1], st[2]), True):
                                continue
                            path = path + ((v, -st[1], st[2]),)
                        elif pi:
                            st = pi[-1]
                            if not acceptable(pj, (st[0], -st[1], st[2]), False):
                                continue
                            path = path + ((v, st[1], st[2]),)
                        found(path + pj, False)
        if step_no == steps or (shortest and not not_found):
            break
        step_no += 1

    rows = []
    for target in sorted(final):                                  # std::multimap iterates by key
        for path in final[target]:
            text = _render(path, names, no_loop)
            if text is not None:
                rows.append(text)
    return rows


def _render(path, names: Dict[int, str], no_loop: bool) -> Optional[str]:
    """buildPathRow: None when NOLOOP drops the row."""
    turning = len(path) // 2 + len(path) % 2
    seen = set()
    out = []

    def edge(typ, rank):
        return "<%s%s,%d>" % ("" if typ >= 0 else "-", names[abs(typ)], rank)
    i = 0
    while i < len(path):
        vid, typ, rank = path[i]
        if no_loop:
            if vid in seen:
                return None
            seen.add(vid)
        out.append(str(vid))
        i += 1
        if i == turning:
            break
        out.append(edge(typ, rank))
    while i < len(path):
        vid, typ, rank = path[i]
        if no_loop:
            if vid in seen:
                return None
            seen.add(vid)
        out.append(edge(-typ, rank))
        out.append(str(vid))
        i += 1
    return "".join(out)


def run(backend, space: int, s: ngql.FindPathSentence, inp, variables, edge_names: Sequence[str] = (), **go_kw):
    """(column names, schema types, rows) of the sentence on the host; raises FindPathError."""
    from_vids, to_vids = setup_vids(s, inp, variables)
    rows = find_path(backend, space, s, from_vids, to_vids, edge_names, **go_kw)
    return ["_path_"], [T_PATH] if rows else [], [(("path", r),) for r in rows]


# ----------------------------------------------------------------------------- the device call's output
def paths_from_dag(sources: Sequence[int], targets: Sequence[int], src, dst, typ, rank, mask,
                   type_names: Dict[int, str]) -> List[str]:
    """The paths of ngx_find_path's path-DAG edges: edge i leads from src[i] to dst[i] with the signed type
    typ[i] and rank[i], and lies on a shortest path to every target j whose bit is set in mask[i]. For each
    target the paths are every walk over its edges from a source to it: all of one length, so none repeats
    a vertex."""
    rows = []
    source_set = set(int(v) for v in sources)
    mask = np.asarray(mask, dtype=np.uint64)
    for j, target in enumerate(targets):
        adj: Dict[int, List[Tuple[int, int, int]]] = {}
        heads = set()
        for i in np.nonzero(mask & np.uint64(1 << j))[0]:
            adj.setdefault(int(src[i]), []).append((int(dst[i]), int(typ[i]), int(rank[i])))
            heads.add(int(src[i]))
        if not adj:
            continue
        stack = [(v, str(v)) for v in sorted(heads & source_set)]
        while stack:
            v, text = stack.pop()
            if v == target:
                rows.append(text)
                continue
            for d, t, r in adj.get(v, ()):
                stack.append((d, "%s<%s%s,%d>%d" % (text, "" if t >= 0 else "-", type_names[abs(t)], r, d)))
    return rows


def count_walks(sources: Sequence[int], targets: Sequence[int], layer, src, dst) -> int:
    """The ALL walks of a layered edge set (paths_from_layers), without enumerating them: per layer the number of
    walks that end at each vertex, summed over the targets."""
    goal = set(int(v) for v in targets)
    by_layer: Dict[int, List[Tuple[int, int]]] = {}
    for i in range(len(src)):
        by_layer.setdefault(int(layer[i]), []).append((int(src[i]), int(dst[i])))
    ends = {int(v): 1 for v in sources}
    total = 0
    for k in range(max(by_layer) + 1 if by_layer else 0):
        nxt: Dict[int, int] = {}
        for u, v in by_layer.get(k, ()):
            n = ends.get(u)
            if n:
                nxt[v] = nxt.get(v, 0) + n
        total += sum(n for v, n in nxt.items() if v in goal)
        ends = nxt
    return total


def paths_from_layers(sources: Sequence[int], targets: Sequence[int], layer, src, dst, typ, rank, mask,
                      type_names: Dict[int, str], no_loop: bool, max_paths: int) -> List[str]:
    """The paths of ngx_find_path's answer to ALL and NOLOOP: edge i is the layer[i]-th step (from 0) of some walk
    from a source to a target of mask[i], from src[i] to dst[i] with the signed type typ[i] and rank[i]. A walk
    starts at a source in layer 0 and follows only edges of its current layer; each time it stands on a target
    after at least one edge it is a row. Every edge of the set leads on to a target within the layers left, so no
    branch is followed in vain. NOLOOP drops a branch when it comes back to a vertex of its walk. The ALL walks are
    counted first; above max_paths FindPathRefusal is raised and nothing is enumerated."""
    n = count_walks(sources, targets, layer, src, dst)
    if n > max_paths:
        raise FindPathRefusal("find path: more than %d paths" % max_paths)
    goal = set(int(v) for v in targets)
    adj: Dict[Tuple[int, int], List[Tuple[int, int, int]]] = {}
    for i in range(len(src)):
        adj.setdefault((int(layer[i]), int(src[i])), []).append((int(dst[i]), int(typ[i]), int(rank[i])))
    rows = []
    for s in sources:
        stack = [(int(s), 0, str(int(s)), (int(s),))]
        while stack:
            v, k, text, on = stack.pop()
            if k and v in goal:
                rows.append(text)
            for d, t, r in adj.get((k, v), ()):
                if no_loop and d in on:
                    continue
                stack.append((d, k + 1, "%s<%s%s,%d>%d" % (text, "" if t >= 0 else "-", type_names[abs(t)], r, d),
                              on + (d,) if no_loop else on))
    return rows
