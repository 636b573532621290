"""LOOKUP ON <tag|edge> WHERE ... [YIELD ...]: the reference's one read that finds vertices or edges by what they
hold. This module is its specification in Python, both halves:

  graphd    LookupExecutor (src/graph/LookupExecutor.cpp): prepareFrom, prepareIndexes, prepareWhere, prepareYield,
            checkFilter / traversalExpr, relationalExprCheck / supportedDataTypeForRange, findOptimalIndex with
            findValidIndexWithStr / findValidIndexNoStr / findIndexForEqualScan / findIndexForRangeScan, the result
            column names and types, every Status text as Status::toString prints it.
  storaged  IndexPolicyMaker and IndexExecutor (src/storage/index/): the folded constants, reversalRelationalExprOP,
            buildPolicy / writeScanItem with their quirks, makeScanPair / normalizeScanPair with checkAndCastVariant's
            truncating cast, boundVariant's byte increment, encodeInt64 / encodeDouble.

The outcome is a Plan: per scanned field an unsigned 64-bit [lo, hi) in the encoded-key domain (the field's 8
big-endian key bytes read as a u64; lo == hi is the reference's prefix scan, an equality), for BOOL and STRING
fields an equality constant, and, when requiredFilter_ is set, the residual terms (field, op, constant), evaluated
with RelationalExpression::eval's typing over decodeVariant(encodeVariant(v)).

scan_model applies a Plan to plain Python rows by building the real index keys and scanning them bytewise per part
in key order: the CPU parity leg, and the only place where the reference's row order exists. The Engine holds no
index: ngx_lookup streams the stored columns once (csrc/lookup.hip) and answers in storage order.

max_rows_returned_per_lookup is INT_MAX in the reference and is not restated. No NaN is in the data: encodeDouble
of a NaN is whatever its bits give and is not modelled further.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

from . import engine as E
from . import fetch as fetchmod
from . import ngql

T_UNKNOWN, T_BOOL, T_INT, T_VID, T_FLOAT, T_DOUBLE, T_STRING, T_TIMESTAMP = 0, 1, 2, 3, 4, 5, 6, 21
LT, LE, GT, GE, EQ, NE, CONTAINS = 0, 1, 2, 3, 4, 5, 6               # RelationalExpression::Operator (ngql.REL_OPS)
LK_INT, LK_DOUBLE, LK_BOOL, LK_STRING = 0, 1, 2, 3                  # NGX_LK_*
U64 = (1 << 64) - 1
INT64_MAX = (1 << 63) - 1
INDEX_NOT_FOUND = "Unknown error(411): "                          # Status::IndexNotFound().toString()
INVALID_FILTER = "Lookup vertices failed"                         # completeness 0: what E_INVALID_FILTER comes to


class LookupError(Exception):
    """A failed Status of the executor; str() is the outcome's error text."""


@dataclass
class Index:
    """nebula::cpp2::IndexItem: fields is the ordered list of (name, type)."""
    index_id: int
    name: str
    schema_name: str
    is_edge: bool
    fields: List[Tuple[str, int]]


# ----------------------------------------------------------------------------- NebulaKeyUtils
def encode_int64(v: int) -> bytes:
    """encodeInt64: the sign bit flipped, big-endian."""
    return struct.pack(">Q", (v & U64) ^ (1 << 63))


def encode_double(v: float) -> bytes:
    """encodeDouble: below zero the bits become -(INT64_MAX + bits) (two's complement), then the top bit flips.
    -0.0 is not below zero: its key is all zero, under every other key; the smallest negative subnormal shares
    +0.0's key."""
    bits = struct.unpack("<Q", struct.pack("<d", v))[0]
    if v < 0:
        bits = (-(INT64_MAX + bits)) & U64
    return struct.pack(">Q", bits ^ (1 << 63))


def decode_double(raw: bytes) -> float:
    bits = struct.unpack(">Q", raw)[0] ^ (1 << 63)
    val = struct.unpack("<d", struct.pack("<Q", bits))[0]
    if val < 0:
        bits = (-(INT64_MAX + bits)) & U64
        val = struct.unpack("<d", struct.pack("<Q", bits))[0]
    return val


def decode_int64(raw: bytes) -> int:
    return ngql.to_i64(struct.unpack(">Q", raw)[0] ^ (1 << 63))


def encode_variant(v) -> bytes:
    if isinstance(v, bool):
        return b"\x01" if v else b"\x00"
    if isinstance(v, int):
        return encode_int64(v)
    if isinstance(v, float):
        return encode_double(v)
    return v.encode() if isinstance(v, str) else bytes(v)


def decode_variant(raw: bytes, t: int):
    if t == T_BOOL:
        return raw[0] != 0
    if t in (T_INT, T_TIMESTAMP, T_VID):
        return decode_int64(raw)
    if t in (T_FLOAT, T_DOUBLE):
        return decode_double(raw)
    return raw.decode()


def bound_addition(t: int, v) -> bytes:
    """boundVariant(kAddition): the encoded bytes plus one, all 0xff once it carries out."""
    k = struct.unpack(">Q", encode_int64(v) if t == T_INT else encode_double(v))[0]
    return struct.pack(">Q", U64 if k == U64 else k + 1)


BOUND_MIN, BOUND_MAX = b"\x00" * 8, b"\xff" * 8


def _which(v) -> int:                                             # boost::variant<int64_t, double, bool, std::string>
    return 2 if isinstance(v, bool) else 0 if isinstance(v, int) else 1 if isinstance(v, float) else 3


def _var_lt(a, b) -> bool:                                        # boost::variant operator<: which(), then the value
    return (_which(a), a) < (_which(b), b) if _which(a) != _which(b) else a < b


def _to_double(v) -> float:
    return float(v)


def _to_int(v) -> int:                                            # Expression::toInt: a double truncates
    if isinstance(v, float):
        return ngql.to_i64(int(v))
    return int(v)


def check_and_cast(t: int, v):
    """checkAndCastVariant: the constant cast to the field's type when they differ."""
    wt = (T_INT, T_DOUBLE, T_BOOL, T_STRING)[_which(v)]
    if t == wt:
        return v
    if t in (T_INT, T_TIMESTAMP):
        if isinstance(v, str):
            raise LookupError(INVALID_FILTER)
        return _to_int(v)
    if t == T_BOOL:
        return bool(v) if not isinstance(v, str) else len(v) > 0
    if t in (T_FLOAT, T_DOUBLE):
        if isinstance(v, str):
            raise LookupError(INVALID_FILTER)
        return _to_double(v)
    if t == T_STRING:
        if isinstance(v, bool):
            return "true" if v else "false"
        return str(v)
    raise LookupError(INVALID_FILTER)


# ----------------------------------------------------------------------------- graphd
@dataclass
class Prepared:
    from_: str
    is_edge: bool
    schema_id: int
    schema: List[Tuple[str, int]]
    indexes: List[Index]
    filters: List[Tuple[str, int]]                                # filters_: (prop, op) in traversal order
    return_cols: List[str]
    names: List[str]
    types: List[int]
    index: Optional[Index] = None


def _field_type(schema, name: str) -> int:
    return next((t for n, t in schema if n == name), T_UNKNOWN)


def prepare(cat, indexes: Sequence[Index], s: ngql.LookupSentence) -> Prepared:
    """prepareClauses, then optimize: the sentence checked and the index chosen."""
    # prepareFrom
    if s.from_ in cat.tags:
        is_edge, (sid, schema) = False, cat.tags[s.from_]
    elif s.from_ in cat.edges:
        is_edge, (sid, schema) = True, cat.edges[s.from_]
    else:
        raise LookupError("Tag or Edge was not found : %s" % s.from_)
    # prepareIndexes
    mine = [i for i in indexes if i.is_edge == is_edge and i.schema_name == s.from_]
    if not mine:
        raise LookupError(INDEX_NOT_FOUND)
    # prepareWhere
    if s.where is None:
        raise LookupError("SyntaxError: Where clause is required")
    p = Prepared(s.from_, is_edge, sid, list(schema), mine, [], [], [], [])
    # prepareYield
    for col in s.yields:
        if col.fun:
            raise LookupError("SyntaxError: Not supported yet")
        e = col.expr
        if not (isinstance(e, ngql.Prop) and e.kind == ngql.K_ALIAS):
            raise LookupError("SyntaxError: Expressions other than AliasProp are not supported")
        _check_alias(p, e)
        if _field_type(schema, e.prop) == T_UNKNOWN:
            raise LookupError("Unknown column `%s' in schema" % e.prop)
        p.return_cols.append(e.prop)
    p.names = (["SrcVID", "DstVID", "Ranking"] if is_edge else ["VertexID"]) + \
        [c.alias if c.alias else c.expr.to_string() for c in s.yields]
    p.types = ([T_VID, T_VID, T_INT] if is_edge else [T_VID]) + [_field_type(schema, c) for c in p.return_cols]
    # optimize
    _traversal(p, s.where)
    if not p.filters:
        raise LookupError("SyntaxError: Where clause error . have not index matching")
    p.index = find_optimal_index(p.indexes, p.filters, p.schema)
    return p


def _check_alias(p: Prepared, e: ngql.Prop) -> None:
    if e.alias != p.from_:
        raise LookupError("SyntaxError: Edge or Tag name error : %s " % e.alias)


def _is_alias(e) -> bool:
    return isinstance(e, ngql.Prop) and e.kind == ngql.K_ALIAS


def _traversal(p: Prepared, e: ngql.Expr) -> None:                # traversalExpr
    if isinstance(e, ngql.Binary) and e.kind == ngql.K_LOGIC:
        if e.op in (ngql.LOGIC_OPS["XOR"], ngql.LOGIC_OPS["||"]):
            raise LookupError("SyntaxError: OR and XOR are not supported in lookup where clause ：%s" % e.to_string())
        _traversal(p, e.left)
        _traversal(p, e.right)
        return
    if isinstance(e, ngql.Binary) and e.kind == ngql.K_REL:
        if e.op == CONTAINS:                                      # relationalExprCheck
            raise LookupError("SyntaxError: Unsupported 'CONTAINS' in where clause")
        if _is_alias(e.left) and _is_alias(e.right):
            raise LookupError("SyntaxError: Does not support left and right are both property")
        side = e.left if _is_alias(e.left) else e.right if _is_alias(e.right) else None
        if side is None:
            raise LookupError("SyntaxError: Unsupported expression ：%s" % e.to_string())
        _check_alias(p, side)
        p.filters.append((side.prop, e.op))
        if e.op not in (EQ, NE) and _field_type(p.schema, side.prop) not in (T_INT, T_DOUBLE, T_FLOAT, T_TIMESTAMP):
            raise LookupError("SyntaxError: Data type of field %s not support range scan" % side.prop)
        return
    if isinstance(e, ngql.Func):
        raise LookupError("SyntaxError: Function expressions are not supported yet")
    raise LookupError("SyntaxError: Syntax error ： %s" % e.to_string())


def find_valid_index_with_str(indexes, filters):
    cols = {f for f, _ in filters}                                # std::set: repeated fields once
    return [i for i in indexes if len(i.fields) == len(cols) and all(n in cols for n, _ in i.fields)]


def find_valid_index_no_str(indexes, filters):
    valid = []
    for i in indexes:
        if any(t == T_STRING for _, t in i.fields):
            continue
        names = [n for n, _ in i.fields]
        if all(f in names for f, _ in filters):
            valid.append(i)
    # the index's first field has to meet a condition
    return [i for i in valid if any(f == i.fields[0][0] for f, _ in filters)]


def find_index_for_equal_scan(indexes, filters):
    hints = []
    for i in indexes:
        count = 0
        for n, _ in i.fields:
            op = next((o for f, o in filters if f == n), None)     # find_if: the first filter of the field
            if op != EQ:
                break
            count += 1
        hints.append((count, i))
    hints.sort(key=lambda h: -h[0])                               # the counts descending (ties: as sorted leaves them)
    return [i for c, i in hints if c == hints[0][0]]


def find_index_for_range_scan(indexes, filters):
    by_count: Dict[int, Index] = {}                               # std::map keyed by hint count: the last index per count
    for i in indexes:
        count = 0
        for n, _ in i.fields:
            op = next((o for f, o in filters if f == n), None)
            if op is None:
                break
            if op == EQ:
                continue
            if op in (GE, GT, LE, LT):
                count += 1
            else:
                break
        by_count[count] = i
    return [by_count[max(by_count)]]


def find_optimal_index(indexes, filters, schema) -> Index:
    has_str = any(_field_type(schema, f) == T_STRING for f, _ in filters)
    valid = find_valid_index_with_str(indexes, filters) if has_str else find_valid_index_no_str(indexes, filters)
    if not valid:
        raise LookupError(INDEX_NOT_FOUND)
    eq = find_index_for_equal_scan(valid, filters)
    if len(eq) == 1:
        return eq[0]
    return find_index_for_range_scan(eq, filters)[0]


# ----------------------------------------------------------------------------- storaged
_FUNCS = {
    "abs": lambda a: abs(a[0]),
    "strcasecmp": lambda a: (a[0].lower() > a[1].lower()) - (a[0].lower() < a[1].lower()),
}


def _fold(e: ngql.Expr):
    """The operand's value with getAliasProp failing ("Alias expression cannot be evaluated")."""
    if isinstance(e, ngql.Func) and e.name.lower() in _FUNCS:
        return _FUNCS[e.name.lower()]([_fold(a) for a in e.args])
    if isinstance(e, (ngql.Prim, ngql.Prop)):
        if isinstance(e, ngql.Prop):
            raise LookupError(INVALID_FILTER)
        return e.value
    if isinstance(e, ngql.Func):
        args = [ngql.Prim(_fold(a)) for a in e.args]
        try:
            return fetchmod._eval(ngql.Func(e.name, args), None)
        except fetchmod.FetchError:
            raise LookupError(INVALID_FILTER)

    def prop(_):
        raise LookupError(INVALID_FILTER)
    try:
        return fetchmod._eval(e, prop)
    except fetchmod.FetchError:
        raise LookupError(INVALID_FILTER)


_REVERSE = {LT: GT, LE: GE, GT: LT, GE: LE}                       # reversalRelationalExprOP


def operator_list(e: ngql.Expr, top: bool = True) -> List[Tuple[str, object, int]]:
    """traversalExpression: (prop, folded constant, operator with the prop on the left). An operand that cannot be
    evaluated is E_INVALID_FILTER. The reference returns that code from the top-level expression only and drops
    the term silently under an AND; here it is the error at every depth (deviations)."""
    if isinstance(e, ngql.Binary) and e.kind == ngql.K_LOGIC:
        return operator_list(e.left, False) + operator_list(e.right, False)
    if isinstance(e, ngql.Binary) and e.kind == ngql.K_REL:
        if _is_alias(e.left):
            return [(e.left.prop, _fold(e.right), e.op)]
        return [(e.right.prop, _fold(e.left), _REVERSE.get(e.op, e.op))]
    raise LookupError(INVALID_FILTER)


@dataclass
class Bound:
    rel: Optional[int] = None                                     # GT / GE / LT / LE / EQ; None: kNull
    val: object = 0


def _write_scan_item(items: Dict[str, List[Bound]], prop: str, v, op: int) -> bool:
    if op in (GE, GT):
        if prop not in items:
            items[prop] = [Bound(op, v), Bound()]
        else:
            b = items[prop][0]
            if b.rel is None:
                items[prop][0] = Bound(op, v)
            elif _var_lt(b.val, v):
                b.val = v                                         # the relation stays: `c == 1 and c > 2` scans for 2
            elif b.rel == EQ:
                return False
    elif op in (LE, LT):
        if prop not in items:
            items[prop] = [Bound(), Bound(op, v)]
        else:
            b = items[prop][1]
            if b.rel is None:
                items[prop][1] = Bound(op, v)
            elif _var_lt(v, b.val):
                b.val = v
            elif b.rel == EQ:
                return False
    elif op == EQ:
        if prop in items:
            return False
        items[prop] = [Bound(EQ, v), Bound(EQ, v)]
    return True


@dataclass
class Plan:
    is_edge: bool
    schema_id: int
    index: Index
    scan: List[Tuple[str, int, bytes, bytes]]                     # per scanned field: (name, type, begin bytes, end bytes)
    terms: List[Tuple[str, int, object]]                          # requiredFilter_: (field, op, constant); else []
    required_filter: bool
    return_cols: List[str]
    names: List[str]
    types: List[int]

    def ranges(self):
        """Per scanned numeric field (name, lo, hi) as u64; BOOL / STRING fields (name, constant)."""
        out = []
        for n, t, b, e in self.scan:
            if t in (T_BOOL, T_STRING):
                out.append((n, decode_variant(b, t)))
            else:
                out.append((n, struct.unpack(">Q", b)[0], struct.unpack(">Q", e)[0]))
        return out


def build_plan(p: Prepared, where: ngql.Expr) -> Plan:
    """IndexExecutor::buildExecutionPlan and makeScanPair for the chosen index."""
    ops = operator_list(where)
    all_terms = [(n, o, v) for n, v, o in ops]
    items: Dict[str, List[Bound]] = {}
    required = False
    next_col = True
    for name, _ in p.index.fields:                                # buildPolicy
        k = 0
        while next_col and k < len(ops):
            if ops[k][0] == name:
                if ops[k][2] == NE:
                    required, next_col = True, False
                    break
                if not _write_scan_item(items, name, ops[k][1], ops[k][2]):
                    raise LookupError(INVALID_FILTER)
                del ops[k]
            else:
                k += 1
        if name not in items or items[name][0].rel != EQ:
            break
    if not required and ops:
        required = True
    scan = []
    for name, t in p.index.fields:                                # makeScanPair
        if name not in items:
            break
        b, e = items[name]
        if b.rel is not None:
            b.val = check_and_cast(t, b.val)
        if e.rel is not None:
            e.val = check_and_cast(t, e.val)
        if b.rel == EQ and e.rel == EQ and b.val == e.val and _which(b.val) == _which(e.val):   # normalizeScanPair
            begin = end = encode_variant(b.val)
        else:
            bt = T_INT if t in (T_INT, T_TIMESTAMP) else t
            begin = BOUND_MIN if b.rel is None else bound_addition(bt, b.val) if b.rel == GT else encode_variant(b.val)
            end = BOUND_MAX if e.rel is None else encode_variant(e.val) if e.rel == LT else bound_addition(bt, e.val)
        if t == T_STRING and begin != end:
            raise LookupError(INVALID_FILTER)                     # "String type field does not allow range scan"
        scan.append((name, t, begin, end))
    return Plan(p.is_edge, p.schema_id, p.index, scan, all_terms if required else [], required, p.return_cols,
                p.names, p.types)


def plan_of(cat, indexes: Sequence[Index], s: ngql.LookupSentence) -> Plan:
    p = prepare(cat, indexes, s)
    return build_plan(p, s.where)


# ----------------------------------------------------------------------------- the model
def rel_eval(l, op: int, r) -> bool:
    """RelationalExpression::eval; a failed evaluation (a string against a non-string) drops the row."""
    if _which(l) != _which(r):
        if isinstance(l, str) or isinstance(r, str):
            return False
        if isinstance(l, float) or isinstance(r, float):
            l, r = _to_double(l), _to_double(r)
        else:
            l, r = int(l), int(r)
    if isinstance(l, str):
        l, r = l.encode(), r.encode()
    if op in (EQ, NE) and isinstance(l, float):
        eq = abs(l - r) < 1e-8
        return eq if op == EQ else not eq
    return [l < r, l <= r, l > r, l >= r, l == r, l != r][op]


def _ikey_prefix(part: int, index_id: int) -> bytes:              # indexPrefix: (part << 8) | kIndex, then the id
    return struct.pack("<i", (part << 8) | 0x02) + struct.pack("<i", index_id)


def _index_raw(fields, props) -> bytes:                           # indexRaw: the values, then the string lengths
    raw, lens = b"", b""
    for n, t in fields:
        b = encode_variant(check_and_cast(t, props[n]) if not isinstance(props[n], str) else props[n])
        raw += b
        if t == T_STRING:
            lens += struct.pack("<i", len(b))
    return raw + lens


def scan_model(rows, plan: Plan, num_parts: int = 1):
    """The plan over rows [(vid, {field: value})] or [(src, dst, rank, {...})]: the index keys built as
    NebulaKeyUtils::vertexIndexKey / edgeIndexKey builds them, scanned bytewise per part in key order between
    makeScanPair's strings, conditionsCheck over the values decoded from the key, then the row's YIELD columns.
    Returns the rows [VertexID | SrcVID, DstVID, Ranking, yields ...] in the reference's order."""
    fields = plan.index.fields
    keyed = []
    for row in rows:
        props = row[-1]
        src = row[0]
        part = (src % (1 << 64)) % num_parts + 1
        tail = struct.pack("<q", src) if not plan.is_edge else struct.pack("<qqq", src, row[2], row[1])
        keyed.append((part, _ikey_prefix(part, plan.index.index_id) + _index_raw(fields, props) + tail, row))
    keyed.sort(key=lambda k: (k[0], k[1]))
    colslen = b"".join(struct.pack("<i", len(b)) for _, t, b, _ in plan.scan if t == T_STRING)
    out = []
    for part, key, row in keyed:
        pre = _ikey_prefix(part, plan.index.index_id)
        begin = pre + b"".join(b for _, _, b, _ in plan.scan) + colslen
        end = pre + b"".join(e for _, _, _, e in plan.scan) + colslen
        hit = key.startswith(begin) if begin == end else begin <= key < end
        if not hit:
            continue
        if plan.required_filter:
            props = row[-1]
            ok = True
            for name, op, const in plan.terms:                    # the values as the key gives them back
                t = _field_type(fields, name)
                v = decode_variant(encode_variant(check_and_cast(t, props[name]) if not isinstance(props[name], str)
                                                  else props[name]), t)
                if not rel_eval(v, op, const):
                    ok = False
                    break
            if not ok:
                continue
        head = [row[0]] if not plan.is_edge else [row[0], row[1], row[2]]
        out.append(tuple(head + [row[-1][c] for c in plan.return_cols]))
    return out


def model_cells(plan: Plan, rows) -> List[Tuple]:
    """scan_model's rows as typed cells (setupInterimResult's typing: the schema's field types)."""
    return [fetchmod._cells(list(r), plan.types) for r in rows]


# ----------------------------------------------------------------------------- the device
def _lk_kind(v) -> int:
    return (LK_INT, LK_DOUBLE, LK_BOOL, LK_STRING)[_which(v)]


def _bits(v) -> int:
    if isinstance(v, bool):
        return int(v)
    if isinstance(v, float):
        return struct.unpack("<q", struct.pack("<d", v))[0]
    return int(v) if not isinstance(v, str) else 0


def device_spec(plan: Plan) -> "E.LookupSpec":
    """The Plan as Engine.lookup takes it."""
    fields = []
    for name, t, b, e in plan.scan:
        if t in (T_BOOL, T_STRING):
            v = decode_variant(b, t)
            fields.append((name, _lk_kind(v), 0, 0, 0, _bits(v), v.encode() if isinstance(v, str) else b""))
        else:
            kind = LK_DOUBLE if t in (T_FLOAT, T_DOUBLE) else LK_INT
            fields.append((name, kind, 0, struct.unpack(">Q", b)[0], struct.unpack(">Q", e)[0], 0, b""))
    terms = [(name, _lk_kind(c), op, 0, 0, _bits(c), c.encode() if isinstance(c, str) else b"")
             for name, op, c in plan.terms]
    return E.LookupSpec(plan.is_edge, plan.schema_id, fields, terms, list(plan.return_cols), list(plan.names),
                        list(plan.types))


def device_rows(spec, r):
    """(column names, schema types, rows) from the device's rows, typed as setupInterimResult types them."""
    rows = [fetchmod._cells([fetchmod._plain(c) for c in row], spec.types) for row in r.rows]
    return list(spec.names), list(spec.types) if rows else [], rows
