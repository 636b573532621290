"""FETCH PROP ON tags / edges: host-side restatement of graphd's FetchVerticesExecutor and FetchEdgesExecutor
(src/graph/FetchVerticesExecutor.cpp, FetchEdgesExecutor.cpp, FetchExecutor.cpp), as they are written.

Vertices (FetchVerticesExecutor):
  - prepareVids (:24-95): literal vid expressions are evaluated (`Vertex ID should be of type integer`) and, under
    YIELD DISTINCT, deduplicated in order; `$-.col` / `$var.col` read the pipe's input or a variable (`Variable `%s'
    not defined`, `Cant not use `*' to reference a vertex id column.`, checkIfDuplicateColumn on the pipe's input,
    getDistinctVIDs' `Interim has no data.` / `Column `%s' not found`); a reference without data is no error;
  - prepareTags (:97-139): `ON *` is every tag of the space, else toTagID per label and `tag(%s) was dup`;
  - prepareYield (:141-257): the leading `VertexID` column (VID); no YIELD: every field of every ON tag is asked
    for and the columns are decided from the response; else aggregates are refused, `$-.*` / `$var.*` expand to
    the input's columns, `$^` / `$$` props are refused, every `tag.prop` needs its tag in ON and the prop in the
    tag's latest schema (`` `%s' is not a prop of `%s' `` with tag and prop in the order the reference prints);
  - execute / onEmptyInputs (:297-320): no vids: the column names and no rows;
  - processResult (:349-589): dataMap holds the vids that have a row of an asked tag; without YIELD the columns
    are `tag.prop` for every tag id seen in the response, in tag id order (std::set), typed by the schema; for a
    reference one output row per input row through applyTo, where "no data for the vid and no `$-` prop in YIELD"
    gives no row and otherwise a missing tag reads RowReader::getDefaultProp values; for literal vids a row per
    vid with data; Collector::getSchema types UNKNOWN columns from the first record.
Edges (FetchEdgesExecutor on FetchExecutor):
  - prepareClauses (:21-77): one edge label, toEdgeType, the edge key reference's `*` and single-source checks,
    the `<edge>._src`, `._dst`, `._rank` columns, FetchExecutor::prepareYield (no YIELD: every field of the edge's
    latest schema; `$^` / `$$` and `$-` / `$var` props are refused), checkEdgeProps;
  - setupEdgeKeys (:161-301): keys from expressions (`ID should be of type integer.`) or from the reference's
    columns through getVIDs, deduplicated by the (src, dst, rank) hash set under YIELD DISTINCT;
  - processResult (:355-431): one row per key whose edge exists: the three key columns, then the yields.
The storage leg is the backend's get_neighbors (Engine and oracle.Oracle both have it; _vertex_props and
_edge_props adapt the two result shapes): TTL and schema versions are the backend's, as in the reference.
Rows come out in the order of the input rows or keys. These functions serve every backend and are the
specification of the device path (ngx_fetch, ngx_go_fetch, include/nebula_gn.h).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import engine as E
from . import ngql

T_UNKNOWN, T_BOOL, T_INT, T_VID, T_FLOAT, T_DOUBLE, T_STRING, T_TIMESTAMP = 0, 1, 2, 3, 4, 5, 6, 21
_TYPE_KIND = {T_BOOL: "bool", T_INT: "int", T_VID: "id", T_FLOAT: "float", T_DOUBLE: "double", T_STRING: "str",
              T_TIMESTAMP: "timestamp"}
_INT_KINDS = ("int", "id", "timestamp")
SOURCE, EDGE = 1, 3                                                # storage::cpp2::PropOwner
_KEY_PROPS = ("_src", "_dst", "_rank", "_type")


class FetchError(Exception):
    """A failed Status of the executor; str() is the outcome's error text."""


@dataclass
class Catalog:
    """What the executors ask meta::SchemaManager: the space's partition count and, per tag / edge name, its id
    and the fields of its latest schema version. Tags keep the order they were added in (getAllTag)."""
    num_parts: int
    tags: Dict[str, Tuple[int, List[Tuple[str, int]]]] = field(default_factory=dict)
    edges: Dict[str, Tuple[int, List[Tuple[str, int]]]] = field(default_factory=dict)

    @staticmethod
    def of(num_parts: int, schemas) -> "Catalog":
        """schemas: objects with is_edge, sid, name, fields and ver (the latest version of a name wins)."""
        c, ver = Catalog(num_parts), {}
        for s in schemas:
            d = c.edges if s.is_edge else c.tags
            key = (bool(s.is_edge), s.name)
            if key not in ver or s.ver >= ver[key]:
                ver[key] = s.ver
                d[s.name] = (s.sid, [(n, t) for n, t in s.fields])
        return c

    def part(self, vid: int) -> int:                             # ID_HASH (src/common/base/Base.h:166-167)
        return (vid % (1 << 64)) % self.num_parts + 1

    def tag_name(self, tag_id: int) -> Optional[str]:
        return next((n for n, (i, _) in self.tags.items() if i == tag_id), None)


def default_of(t: int):
    """RowReader::getDefaultProp."""
    return {T_BOOL: False, T_FLOAT: 0.0, T_DOUBLE: 0.0, T_STRING: ""}.get(t, 0)


def _kind_of_value(v) -> Tuple[str, int]:                        # Collector::getSchema on an UNKNOWN column
    if isinstance(v, bool):
        return "bool", T_BOOL
    if isinstance(v, int):
        return "int", T_INT
    if isinstance(v, float):
        return "double", T_DOUBLE
    return "str", T_STRING


# ----------------------------------------------------------------------------- expressions
def _eval(e: ngql.Expr, prop):
    """Expression::eval; prop(Prop) answers every property reference."""
    if isinstance(e, ngql.Prim):
        return e.value
    if isinstance(e, ngql.Prop):
        return prop(e)
    if isinstance(e, ngql.Unary):
        v = _eval(e.operand, prop)
        if e.op == ngql.UNARY_OPS["!"]:
            return not v
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise FetchError("Wrong type of arithmetic operand")
        return v if e.op == ngql.UNARY_OPS["+"] else (-v if isinstance(v, float) else ngql.to_i64(-v))
    if isinstance(e, ngql.Cast):
        v = _eval(e.operand, prop)
        try:
            return (int, str, float, bool, int)[e.ctype % 5](v)
        except (TypeError, ValueError):
            raise FetchError("Type casting failed")
    if isinstance(e, ngql.Binary):
        a, b = _eval(e.left, prop), _eval(e.right, prop)
        if e.kind == ngql.K_ARITH:
            op = "+-*/%^"[e.op]
            if op == "+" and isinstance(a, str) and isinstance(b, str):
                return a + b
            for v in (a, b):
                if isinstance(v, bool) or not isinstance(v, (int, float)):
                    raise FetchError("Wrong type of arithmetic operand")
            both = isinstance(a, int) and isinstance(b, int)
            if op in "/%" and b == 0:
                raise FetchError("Division by zero")
            if op == "+":
                r = a + b
            elif op == "-":
                r = a - b
            elif op == "*":
                r = a * b
            elif op == "/":
                r = abs(a) // abs(b) * (1 if (a < 0) == (b < 0) else -1) if both else a / b
            elif op == "%":
                r = abs(a) % abs(b) * (1 if a >= 0 else -1) if both else math.fmod(a, b)
            else:
                if not both:
                    raise FetchError("Arithmetic XOR needs integers")
                r = a ^ b
            return ngql.to_i64(r) if both else float(r)
        if e.kind == ngql.K_REL:
            ops = [lambda x, y: x < y, lambda x, y: x <= y, lambda x, y: x > y, lambda x, y: x >= y,
                   lambda x, y: x == y, lambda x, y: x != y, lambda x, y: y in x]
            try:
                return bool(ops[e.op](a, b))
            except TypeError:
                raise FetchError("A relational operand has the wrong type")
        return [bool(a) and bool(b), bool(a) or bool(b), bool(a) != bool(b)][e.op]
    if isinstance(e, ngql.Func):
        args = [_eval(a, prop) for a in e.args]
        try:
            return ngql.eval_const(ngql.Func(e.name, [ngql.Prim(a) for a in args]))
        except ValueError:
            raise FetchError("Function `%s' is not supported in FETCH" % e.name)
    raise FetchError("`%s' cannot be evaluated here" % e.to_string())


def _const(e: ngql.Expr):
    def none(p):
        raise FetchError("`%s' is not a constant" % p.to_string())
    try:
        return _eval(e, none)
    except ValueError as ex:
        raise FetchError(str(ex))


# ----------------------------------------------------------------------------- the pipe's input
def _check_duplicate(inp) -> None:                               # TraverseExecutor::checkIfDuplicateColumn
    if inp is None:
        return
    seen = set()
    for n in inp.names:
        if n in seen:
            raise FetchError("Duplicate column `%s'" % n)
        seen.add(n)


def _vids_of(interim, col: str, distinct: bool) -> List[int]:
    """InterimResult::getVIDs / getDistinctVIDs (InterimResult.cpp:28-72)."""
    if not interim.rows:
        raise FetchError("Interim has no data.")
    if col not in interim.names:
        raise FetchError("Column `%s' not found" % col)
    i = interim.names.index(col)
    out, seen = [], set()
    for row in interim.rows:
        kind, v = row[i]
        if kind not in _INT_KINDS:
            raise FetchError("Column `%s' not found" % col)
        if distinct:
            if v in seen:
                continue
            seen.add(v)
        out.append(int(v))
    return out


def _input_value(interim, row, p: ngql.Prop):
    """Collector::getProp(schema, prop, reader) over an interim row."""
    if p.prop not in interim.names:
        raise FetchError("Unknown type: 0, prop: %s" % p.prop)
    kind, v = row[interim.names.index(p.prop)]
    if kind == "empty":
        return bool(v) if v is not None else 0
    return v


def _column_type(interim, name: str) -> int:                     # InterimResult::getColumnType
    if interim is None or not interim.rows or name not in interim.names:
        return T_UNKNOWN
    i = interim.names.index(name)
    return interim.types[i] if i < len(interim.types) else T_UNKNOWN


def _typed(values: List[object], types: List[int]) -> Tuple[List[int], Tuple]:
    """Collector::getSchema over the first record, then the record's cells."""
    out_t, cells = [], []
    for v, t in zip(values, types):
        if t == T_UNKNOWN:
            k, t = _kind_of_value(v)
        else:
            k = _TYPE_KIND.get(t, "int")
        out_t.append(t)
        cells.append((k, v))
    return out_t, tuple(cells)


def _cells(values: List[object], types: List[int]) -> Tuple:
    return tuple(((_TYPE_KIND.get(t) or _kind_of_value(v)[0]), v) for v, t in zip(values, types))


# ----------------------------------------------------------------------------- the storage leg
def _by_part(cat: Catalog, vids: Sequence[int]):
    parts: Dict[int, List[int]] = {}
    for v in vids:
        parts.setdefault(cat.part(v), []).append(v)
    return sorted(parts.items())


def _is_oracle(backend) -> bool:
    """The CPU restatement's result shape (vertices with tag rows and edge lists) rather than the Engine's arrays."""
    return hasattr(getattr(backend, "L", None), "orc_get_neighbors")


def _plain(cell):
    kind, v = cell
    if kind == "empty":
        return bool(v) if v is not None else None
    return v


def _vertex_props(backend, space: int, cat: Catalog, vids: Sequence[int], cols: Sequence[Tuple[int, str]],
                  now_sec: int = 0) -> Dict[int, Dict[int, Dict[str, object]]]:
    """StorageClient::getVertexProps: vid -> tag id -> prop -> value, for the vids that have a row of an asked tag.
    cols: (tag id, prop). The tag columns are asked for with no edge types."""
    uniq = list(dict.fromkeys(vids))
    parts = _by_part(cat, uniq)
    req = [(SOURCE, t, p) for t, p in cols]
    data: Dict[int, Dict[int, Dict[str, object]]] = {}
    if not uniq or not req:
        return data
    if _is_oracle(backend):
        r = backend.get_neighbors(space, parts, None, req, only_vertex_props=True)
        if r.failed_codes:
            raise FetchError("Get tag props failed")
        for v in r.vertices:
            for td in v["tags"]:
                names = [n for n, _ in r.vertex_schema.get(td["tag_id"], [])]
                if td["values"] is None:
                    continue
                data.setdefault(v["vid"], {})[td["tag_id"]] = dict(zip(names, td["values"]))
        return data
    kw = {"now_sec": now_sec} if now_sec else {}
    r = backend.get_neighbors(space, parts, [], req, **kw)
    if r.failed_codes:
        raise FetchError("Get tag props failed")
    order = [v for _, vs in parts for v in vs]
    nc = len(req)
    for i, vid in enumerate(order):
        for c, (t, p) in enumerate(cols):
            if r.vertex_has_tag[i * nc + c]:
                data.setdefault(vid, {}).setdefault(t, {})[p] = _plain(r.vertex_cells[i][c])
    return data


def _edge_props(backend, space: int, cat: Catalog, etype: int, keys: Sequence[Tuple[int, int, int]],
                props: Sequence[str], now_sec: int = 0) -> Dict[Tuple[int, int, int], Dict[str, object]]:
    """StorageClient::getEdgeProps: (src, dst, rank) -> prop -> value for the keys whose edge exists: the sources'
    edges of the one type are asked for with `_dst`, `_rank` and the props, and the key's edge is picked."""
    srcs = list(dict.fromkeys(k[0] for k in keys))
    want = set(keys)
    out: Dict[Tuple[int, int, int], Dict[str, object]] = {}
    if not srcs:
        return out
    parts = _by_part(cat, srcs)
    names = ["_dst", "_rank"] + [p for p in props if p not in _KEY_PROPS]
    req = [(EDGE, etype, n) for n in names]
    if _is_oracle(backend):
        r = backend.get_neighbors(space, parts, [etype], req)
        if r.failed_codes:
            raise FetchError("Get edge props failed")
        sch = [n for n, _ in r.edge_schema.get(etype, [])]       # the return columns but _dst, in request order
        for v in r.vertices:
            for ed in v["edges"]:
                if ed["type"] != etype:
                    continue
                for x in ed["edges"]:
                    vals = dict(zip(sch, x["values"] or ()))
                    key = (v["vid"], x["dst"], vals.get("_rank", 0))
                    if key in want:
                        out[key] = vals
        return out
    kw = {"now_sec": now_sec} if now_sec else {}
    r = backend.get_neighbors(space, parts, [etype], req, **kw)
    if r.failed_codes:
        raise FetchError("Get edge props failed")
    order = [v for _, vs in parts for v in vs]
    for i in range(r.total_edges):
        if int(r.edge_type[i]) != etype:
            continue
        vals = {n: _plain(r.edge_cells[i][c]) for c, n in enumerate(names)}
        key = (order[int(r.edge_vertex[i])], int(r.edge_dst[i]), int(vals["_rank"]))
        if key in want:
            out[key] = vals
    return out


# ----------------------------------------------------------------------------- FETCH PROP ON tags
@dataclass
class VertexPlan:
    """prepareClauses' outcome for a FETCH on tags."""
    vids: List[int]
    interim: object                                               # inputsPtr_: the referenced rows, or None
    col: str
    tag_ids: List[int]                                            # ON order (`*': every tag)
    tag_names: List[str]
    on_all: bool
    names: List[str]                                              # colNames_ so far: VertexID, then the yields
    types: List[int]
    yields: List[ngql.AggCol]                                     # after `$-.*` expansion
    props: List[Tuple[int, str]]                                  # (tag id, prop) asked of storage
    has_yield: bool
    has_input_prop: bool


def prepare_vertices(cat: Catalog, s: ngql.FetchVerticesSentence, inp, variables) -> VertexPlan:
    distinct = s.distinct
    vids, interim = [], None
    if s.from_type:                                               # prepareVids
        if s.from_type == 1:
            interim = inp
        else:
            if s.from_var not in variables:
                raise FetchError("Variable `%s' not defined" % s.from_var)
            interim = variables[s.from_var]
        if s.from_col == "*":
            raise FetchError("Cant not use `*' to reference a vertex id column.")
        if interim is not None and interim.rows:
            _check_duplicate(inp)
            vids = _vids_of(interim, s.from_col, True)
    else:
        seen = set()
        for e in s.vids:
            v = _const(e)
            if isinstance(v, bool) or not isinstance(v, int):
                raise FetchError("Vertex ID should be of type integer")
            if distinct:
                if v in seen:
                    continue
                seen.add(v)
            vids.append(v)
    tag_ids, tag_names, name_set = [], [], set()                  # prepareTags
    on_all = s.tags == ["*"]
    if on_all:
        for name, (tid, _) in cat.tags.items():
            if name in name_set:
                raise FetchError("tag(%s) was dup" % name)
            name_set.add(name)
    else:
        for name in s.tags:
            if name not in cat.tags:
                raise FetchError("Unknown error(406): ")          # Status::TagNotFound()
            tag_names.append(name)
            tag_ids.append(cat.tags[name][0])
            if name in name_set:
                raise FetchError("tag(%s) was dup" % name)
            name_set.add(name)
    names, types, yields, props = ["VertexID"], [T_VID], [], []   # prepareYield
    has_input = False
    if not s.has_yield:
        for name, tid in (zip(tag_names, tag_ids) if not on_all else [(n, cat.tags[n][0]) for n in cat.tags]):
            for prop, _ in cat.tags[name][1]:
                props.append((tid, prop))
    else:
        alias_props = []
        src_dst = False
        for col in s.yields:
            if col.fun:
                raise FetchError("SyntaxError: Do not support aggregated query with fetch prop on.")
            e = col.expr
            if isinstance(e, ngql.Prop) and e.kind in (ngql.K_INPUT_PROP, ngql.K_VAR_PROP) and e.prop == "*":
                if interim is None:                               # inputsPtr_->getColNames() on a null pointer
                    raise FetchError("Inputs nullptr.")
                for n in interim.names:
                    x = ngql.Prop(e.kind, e.ref, e.alias, n)
                    yields.append(ngql.AggCol(x))
                    names.append(x.to_string())
                    types.append(T_UNKNOWN)
                    has_input = True                              # expCtx_->addInputProp(prop), either kind
                continue
            yields.append(col)
            for k, alias, prop in e.props():
                if k == ngql.K_INPUT_PROP:
                    has_input = True
                elif k in (ngql.K_SRC_PROP, ngql.K_DST_PROP):
                    src_dst = True
                elif k in (ngql.K_ALIAS, ngql.K_EDGE_SRC, ngql.K_EDGE_DST, ngql.K_EDGE_RANK, ngql.K_EDGE_TYPE):
                    if (alias, prop) not in alias_props:
                        alias_props.append((alias, prop))
            names.append(col.alias if col.alias else col.to_string())
            if isinstance(e, ngql.Prop) and e.kind == ngql.K_INPUT_PROP:
                types.append(_column_type(inp, e.prop))
            elif isinstance(e, ngql.Prop) and e.kind == ngql.K_VAR_PROP:
                types.append(_column_type(variables.get(e.alias), e.prop))
            elif isinstance(e, ngql.Binary) and e.kind in (ngql.K_REL, ngql.K_LOGIC):
                types.append(T_BOOL)
            elif isinstance(e, ngql.Cast):
                types.append((T_INT, T_STRING, T_DOUBLE, T_BOOL, T_TIMESTAMP)[e.ctype % 5])
            elif isinstance(e, ngql.Prop) and e.kind == ngql.K_ALIAS and e.alias in cat.edges:
                types.append(dict(cat.edges[e.alias][1]).get(e.prop, T_UNKNOWN))   # calculateExprType asks toEdgeType
            else:
                types.append(T_UNKNOWN)
        if src_dst:
            raise FetchError("SyntaxError: tag.prop and edgetype.prop are supported in fetch sentence.")
        for alias, prop in alias_props:
            if alias not in name_set:
                raise FetchError("SyntaxError: Near [%s.%s], tag should be declared in `ON' clause first." % (alias, prop))
            if alias not in cat.tags:
                raise FetchError("Unknown error(406): ")
            tid, fields = cat.tags[alias]
            if prop not in dict(fields):
                raise FetchError("`%s' is not a prop of `%s'" % (alias, prop))
            props.append((tid, prop))
    return VertexPlan(vids, interim, s.from_col, tag_ids, tag_names, on_all, names, types, yields, props,
                      s.has_yield, has_input)


def fetch_vertices(backend, space: int, cat: Catalog, s: ngql.FetchVerticesSentence, inp, variables, now_sec: int = 0):
    """(column names, schema types, rows) of the sentence on the host; raises FetchError."""
    p = prepare_vertices(cat, s, inp, variables)
    if not p.vids:                                                # onEmptyInputs
        return p.names, [], []
    data = _vertex_props(backend, space, cat, p.vids, p.props, now_sec)
    names, types, yields = list(p.names), list(p.types), list(p.yields)
    if not p.has_yield:                                           # the tags seen in the response, in id order
        for tid in sorted({t for d in data.values() for t in d}):
            name = cat.tag_name(tid)
            if name is None:
                continue
            for prop, t in cat.tags[name][1]:
                e = ngql.Prop(ngql.K_ALIAS, "", name, prop)
                yields.append(ngql.AggCol(e))
                names.append(e.to_string())
                types.append(t)

    def record(vid, ds, interim, row):
        def prop(x: ngql.Prop):
            if x.kind in (ngql.K_INPUT_PROP, ngql.K_VAR_PROP):
                if interim is None:
                    raise FetchError("`%s' has no input" % x.to_string())
                return _input_value(interim, row, x)
            if x.alias not in cat.tags:
                raise FetchError("Unknown error(406): ")
            tid, fields = cat.tags[x.alias]
            if tid in ds:
                if x.prop not in ds[tid]:
                    raise FetchError("Unknown type: 0, prop: %s" % x.prop)
                return ds[tid][x.prop]
            if x.prop not in dict(fields):
                raise FetchError("Unknown type: 0, prop: %s" % x.prop)
            return default_of(dict(fields)[x.prop])
        return [vid] + [_eval(y.expr, prop) for y in yields]

    rows, out_types = [], None
    if s.from_type:
        i = p.interim.names.index(p.col)
        for row in p.interim.rows:                                # InterimResult::applyTo
            kind, vid = row[i]
            if kind not in _INT_KINDS:
                raise FetchError("Column `%s' not found" % p.col)
            if vid not in data and not p.has_input_prop:
                continue
            rec = record(int(vid), data.get(vid, {}), p.interim, row)
            if out_types is None:
                out_types, _ = _typed(rec, types)
            rows.append(_cells(rec, out_types))
    else:
        for vid in p.vids:
            if vid not in data:
                continue
            rec = record(vid, data[vid], None, None)
            if out_types is None:
                out_types, _ = _typed(rec, types)
            rows.append(_cells(rec, out_types))
    return names, out_types or [], rows


# ----------------------------------------------------------------------------- FETCH PROP ON an edge
@dataclass
class EdgePlan:
    etype: int
    label: str
    keys: List[Tuple[int, int, int]]
    names: List[str]                                              # returnColNames_
    types: List[int]                                              # of the yields
    yields: List[ngql.AggCol]
    props: List[str]
    key_cols: Tuple[str, str, Optional[str]] = ("", "", None)     # the reference's column names
    interim: object = None


def prepare_edges(cat: Catalog, s: ngql.FetchEdgesSentence, inp, variables) -> EdgePlan:
    if len(s.edges) != 1:
        raise FetchError("fetch prop on edge support only one edge label now.")
    label = s.edges[0]
    if label not in cat.edges:
        raise FetchError("Unknown error(407): ")                  # Status::EdgeNotFound()
    etype, fields = cat.edges[label]
    var = ""
    if s.from_type:                                               # prepareEdgeKeys
        refs = [s.src_ref, s.dst_ref] + ([s.rank_ref] if s.rank_ref is not None else [])
        if any(r.prop == "*" for r in refs):
            raise FetchError("Can not use `*' to reference a vertex id column.")
        if s.from_type == 2:
            if len({r.alias for r in refs}) != 1:
                raise FetchError("SyntaxError: Near %s, Only support single data source." % s.ref_string())
            var = refs[0].alias
    names = [label + "._src", label + "._dst", label + "._rank"]
    yields = list(s.yields) if s.has_yield else [ngql.AggCol(ngql.Prop(ngql.K_ALIAS, "", label, n)) for n, _ in fields]
    types, alias_props = [], []
    src_dst = in_var = False
    for col in yields:                                            # FetchExecutor::prepareYield
        e = col.expr
        for k, alias, prop in e.props():
            if k in (ngql.K_SRC_PROP, ngql.K_DST_PROP):
                src_dst = True
            elif k in (ngql.K_INPUT_PROP, ngql.K_VAR_PROP):
                in_var = True
            elif (alias, prop) not in alias_props:
                alias_props.append((alias, prop))
        names.append(col.alias if col.alias else col.expr.to_string())
        if isinstance(e, ngql.Prop) and e.kind in (ngql.K_EDGE_SRC, ngql.K_EDGE_DST):
            types.append(T_VID)
        elif isinstance(e, ngql.Prop) and e.kind in (ngql.K_EDGE_RANK, ngql.K_EDGE_TYPE):
            types.append(T_INT)
        elif isinstance(e, ngql.Prop) and e.kind == ngql.K_ALIAS and e.alias in cat.edges:
            types.append(dict(cat.edges[e.alias][1]).get(e.prop, T_UNKNOWN))
        elif isinstance(e, ngql.Binary) and e.kind in (ngql.K_REL, ngql.K_LOGIC):
            types.append(T_BOOL)
        elif isinstance(e, ngql.Cast):
            types.append((T_INT, T_STRING, T_DOUBLE, T_BOOL, T_TIMESTAMP)[e.ctype % 5])
        else:
            types.append(T_UNKNOWN)
    if src_dst:
        raise FetchError("SyntaxError: tag.prop and edgetype.prop are supported in fetch sentence.")
    if in_var:
        raise FetchError("SyntaxError: `$-' and `$variable' not supported in fetch yet.")
    props = []
    for alias, prop in alias_props:                               # checkEdgeProps
        if alias != label:
            raise FetchError("SyntaxError: Near [%s.%s], edge should be declared in `ON' clause first." % (alias, prop))
        if prop in _KEY_PROPS:
            continue
        if prop not in dict(fields):
            raise FetchError("`%s' is not a prop of `%s'" % (prop, alias))
        props.append(prop)
    keys, interim = [], None                                      # setupEdgeKeys
    key_cols = ("", "", None)
    if s.from_type:
        if s.from_type == 1:
            interim = inp
        else:
            if var not in variables:
                raise FetchError("Variable `%s' not defined" % var)
            interim = variables[var]
        if interim is not None and interim.rows:
            _check_duplicate(inp)
            key_cols = (s.src_ref.prop, s.dst_ref.prop, s.rank_ref.prop if s.rank_ref is not None else None)
            srcs = _vids_of(interim, key_cols[0], False)
            dsts = _vids_of(interim, key_cols[1], False)
            ranks = _vids_of(interim, key_cols[2], False) if key_cols[2] is not None else [0] * len(srcs)
            keys = list(zip(srcs, dsts, ranks))
    else:
        for se, de, rank in s.keys:
            a, b = _const(se), _const(de)
            if any(isinstance(v, bool) or not isinstance(v, int) for v in (a, b)):
                raise FetchError("ID should be of type integer.")
            keys.append((a, b, rank))
    if s.distinct:                                                # the EdgeKeyHashSet
        keys = list(dict.fromkeys(keys))
    return EdgePlan(etype, label, keys, names, types, yields, props, key_cols, interim)


def fetch_edges(backend, space: int, cat: Catalog, s: ngql.FetchEdgesSentence, inp, variables, now_sec: int = 0):
    p = prepare_edges(cat, s, inp, variables)
    if not p.keys:                                                # onEmptyInputs
        return p.names, [], []
    found = _edge_props(backend, space, cat, p.etype, p.keys, p.props, now_sec)
    rows, out_types = [], None
    for key in p.keys:
        vals = found.get(key)
        if vals is None:
            continue

        def prop(x: ngql.Prop):
            if x.prop in _KEY_PROPS:
                return {"_src": key[0], "_dst": key[1], "_rank": key[2], "_type": p.etype}[x.prop]
            if x.prop not in vals:
                raise FetchError("Unknown type: 0, prop: %s" % x.prop)
            return vals[x.prop]
        rec = list(key) + [_eval(y.expr, prop) for y in p.yields]
        if out_types is None:
            out_types, _ = _typed(rec, [T_VID, T_VID, T_INT] + p.types)
        rows.append(_cells(rec, out_types))
    return p.names, out_types or [], rows


def run(backend, space: int, cat: Catalog, s, inp, variables, now_sec: int = 0):
    """(column names, schema types, rows) of a parsed FETCH sentence on the host; raises FetchError."""
    if isinstance(s, ngql.FetchVerticesSentence):
        return fetch_vertices(backend, space, cat, s, inp, variables, now_sec)
    return fetch_edges(backend, space, cat, s, inp, variables, now_sec)


# ----------------------------------------------------------------------------- the device call's plan and output
def device_spec(cat, s, inp, variables, placeholder: bool = False):
    """The engine.FetchSpec (ngx_fetch_plan) of a sentence, after the prepare stage above did every check and
    worded every Status. None: empty inputs or a shape only the host restatement serves (it then runs).
    placeholder: `inp' stands for a device-resident result (names only); the keys are its columns."""
    if isinstance(s, ngql.FetchVerticesSentence):
        p = prepare_vertices(cat, s, inp, variables)
        if not p.vids:
            return None
        interim = p.interim
        names = list(p.names)
        types = list(p.types)
        tags = [] if p.on_all else list(p.tag_ids)
        ys, ytag = [], []
        if not p.has_yield:                                   # the response's tags come out in tag id order
            order = sorted(range(len(tags)), key=lambda t: tags[t])
            for t in order:
                tname = p.tag_names[t]
                for prop, ft in cat.tags[tname][1]:
                    ys.append((E.FY_TAG_PROP, tags[t], prop, 0, 0))
                    ytag.append(t)
                    names.append(tname + "." + prop)
                    types.append(ft)
        for y in p.yields:
            e = y.expr
            if isinstance(e, ngql.Prop) and e.kind == ngql.K_ALIAS and e.alias in cat.tags:
                ys.append((E.FY_TAG_PROP, cat.tags[e.alias][0], e.prop, 0, 0))
            elif isinstance(e, ngql.Prop) and e.kind in (ngql.K_INPUT_PROP, ngql.K_VAR_PROP):
                same = s.from_type == (1 if e.kind == ngql.K_INPUT_PROP else 2) and \
                    (e.kind == ngql.K_INPUT_PROP or e.alias == s.from_var)
                if not same or interim is None or e.prop not in interim.names:
                    return None
                col = interim.names.index(e.prop)
                if not placeholder:
                    if e.prop != p.col:                       # host keys: only the key column itself is uploaded
                        return None
                    col = 0
                ys.append((E.FY_INPUT_COL, 0, "", 0, col))
            else:
                ys.append((-1, 0, "", 0, 0))
        keys, key_cols = None, (-1, -1, -1)
        if placeholder:
            key_cols = (interim.names.index(p.col), -1, -1)
        elif s.from_type:
            i = interim.names.index(p.col)
            if any(r[i][0] not in ("int", "id", "timestamp") for r in interim.rows):
                return None
            keys = [np.array([r[i][1] for r in interim.rows], dtype=np.int64)]
        else:
            keys = [np.array(p.vids, dtype=np.int64)]
        return E.FetchSpec(E.FETCH_VERTEX, tags, 0, key_cols, keys, s.distinct, bool(s.from_type and p.has_input_prop), ys,
                         names, types, ytag, not p.has_yield, list(p.names))
    p = prepare_edges(cat, s, inp, variables)
    if not p.keys:
        return None
    ys = []
    for y in p.yields:
        e = y.expr
        if isinstance(e, ngql.Prop) and e.prop in E.EDGE_KEY and e.kind != ngql.K_INPUT_PROP and e.kind != ngql.K_VAR_PROP:
            ys.append((E.FY_EDGE_KEY, 0, "", E.EDGE_KEY[e.prop], 0))
        elif isinstance(e, ngql.Prop) and e.kind == ngql.K_ALIAS:
            ys.append((E.FY_EDGE_PROP, 0, e.prop, 0, 0))
        else:
            ys.append((-1, 0, "", 0, 0))
    keys, key_cols = None, (-1, -1, -1)
    if placeholder:
        n = p.interim.names
        key_cols = (n.index(p.key_cols[0]), n.index(p.key_cols[1]), n.index(p.key_cols[2]) if p.key_cols[2] is not None else -1)
    else:
        keys = [np.array([k[j] for k in p.keys], dtype=np.int64) for j in range(3)]
        key_cols = (0, 1, 2)
    return E.FetchSpec(E.FETCH_EDGE, [], p.etype, key_cols, keys, s.distinct, False, ys, list(p.names),
                     [3, 3, 2] + list(p.types), [], False, list(p.names))

def device_rows(spec, r):
    """(column names, schema types, rows) as the host restatement gives them, from the device's rows."""
    if not r.rows:
        return list(spec.prefix), [], []
    nkey = 1 if spec.kind == E.FETCH_VERTEX else 3
    keep = list(range(nkey + len(spec.yields)))
    if spec.no_yield:                                         # the columns of the tags seen in the response
        keep = list(range(nkey)) + [nkey + y for y, t in enumerate(spec.yield_tag) if r.tags_seen >> t & 1]
    names = [spec.names[c] for c in keep]
    # an input column read in HBM is typed as the result it came from types it
    types = [spec.types[c] or (r.col_types[c] if c >= nkey and spec.yields[c - nkey][0] == E.FY_INPUT_COL else 0) for c in keep]
    values = [[_plain(row[c]) for c in keep] for row in r.rows]
    out_types, _ = _typed(values[0], types)
    return names, out_types, [_cells(v, out_types) for v in values]
