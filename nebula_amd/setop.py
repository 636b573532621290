"""UNION / INTERSECT / MINUS over two interim results: host-side restatement of graphd's SetExecutor
(src/graph/SetExecutor.cpp).

  - execute (:104-198): a failed side is `left subquery has error: ...` / `right subquery has error: ...` (the left
    first); different column counts are `Field count not match.`; both sides without rows answer with the left
    column names and no rows (onEmptyInputs); the result carries the left side's column names;
  - doUnion (:200-252): an empty left hands the right through under the left's names, an empty right the left;
    else the left rows, then the (cast) right rows; DISTINCT (the default of a bare UNION, parser.yy:1319-1323)
    is std::sort + std::unique over RowValue (doDistinct, :300-304);
  - doIntersect (:306-354): an empty side gives no rows; else each left row, in left order, takes the first equal
    right row and *moves* it out (rows.emplace_back(std::move(rr))): the moved-from row has no columns and
    equals nothing later, so a value occurring cL times left and cR times right comes out min(cL, cR) times.
    SetTest.cpp's own cases hold no equal rows, so they neither confirm nor contradict this; it is what the
    loop does;
  - doMinus (:356-410): an empty left gives no rows, an empty right the left unchanged; else every left row
    equal to any right row is erased, the others (duplicates too) stay in left order;
  - checkSchema / doCasting (:254-297): where the two schemas' column types differ the right rows' cells are
    cast to the left's type with InterimResult::castTo (src/graph/InterimResult.cpp:310-556); a failed cast
    fails the statement with the cast's text.
Row equality is the thrift ColumnValue ==: the same variant type and the same value; doubles with plain ==, so
-0.0 equals 0.0 and a NaN equals nothing.
UNION DISTINCT fixes the set of rows only (std::sort's order over thrift unions is whatever the generated
operator< gives). Here the rows come back sorted under a documented total order, column by column: by variant
type (bool < int < id < double < str < timestamp, the thrift field order), then by value: integers and bools
numerically, doubles by value with every NaN after +inf (by its bits), strings as unsigned bytes with a proper
prefix first. Of equal rows the first in (left, then right) order is kept.
These functions serve every backend and are the specification of the device path (ngx_set_op, ngx_go_set,
include/nebula_gn.h). Cells are (kind, value) pairs as GoResult.rows holds them.
"""
from __future__ import annotations

import math
import re
import struct
from decimal import Decimal
from typing import List, Optional, Sequence, Tuple

T_UNKNOWN, T_BOOL, T_INT, T_VID, T_FLOAT, T_DOUBLE, T_STRING, T_TIMESTAMP = 0, 1, 2, 3, 4, 5, 6, 21
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
_RANK = {"bool": 1, "int": 2, "id": 3, "float": 4, "double": 4, "str": 5, "timestamp": 6, "empty": 0}


class SetError(Exception):
    """A failed Status of the executor; str() is the outcome's error text."""


def _norm(cell):
    """A bool the device typed per row arrives as ("empty", bool): the ColumnValue is a bool_val."""
    kind, v = cell
    if kind == "empty" and v is not None:
        return ("bool", bool(v))
    if kind == "float":
        return ("double", v)
    return cell


def row_key(row) -> Optional[tuple]:
    """A hashable key equal for exactly the rows ColumnValue == calls equal; None: the row holds a NaN (or an
    unset value) and equals no row."""
    out = []
    for cell in row:
        kind, v = _norm(cell)
        if kind == "double":
            if v != v:
                return None
            v = v + 0.0                                           # -0.0 == 0.0
        elif kind == "empty":
            return None
        out.append((kind, v))
    return tuple(out)


def _order_key(row):
    out = []
    for cell in row:
        kind, v = _norm(cell)
        if kind == "double":
            out.append((_RANK[kind], 1, struct.unpack("<q", struct.pack("<d", v))[0]) if v != v else (_RANK[kind], 0, v + 0.0))
        elif kind == "str":
            out.append((_RANK[kind], 0, v.encode("utf-8", "surrogateescape")))
        elif kind == "empty":
            out.append((0, 0, 0))
        else:
            out.append((_RANK[kind], 0, int(v)))
    return tuple(out)


# ----------------------------------------------------------------------------- InterimResult::castTo
def _double_str(d: float) -> str:
    """folly::to<std::string>(double): double-conversion's shortest digits, plain notation for decimal exponents
    -6 .. 20, else d[.ddd]E[-]x; no trailing `.0'."""
    if d != d:
        return "NaN"
    if math.isinf(d):
        return "Infinity" if d > 0 else "-Infinity"
    if d == 0:
        return "-0" if math.copysign(1, d) < 0 else "0"
    sign, digits, exp = Decimal(repr(abs(d))).as_tuple()
    digits = list(digits)
    while len(digits) > 1 and digits[-1] == 0:
        digits.pop()
        exp += 1
    ds = "".join(map(str, digits))
    point = len(ds) + exp                                         # the value is 0.ds x 10^point
    if -6 <= point - 1 < 21:
        if point <= 0:
            s = "0." + "0" * -point + ds
        elif point >= len(ds):
            s = ds + "0" * (point - len(ds))
        else:
            s = ds[:point] + "." + ds[point:]
    else:
        s = ds[0] + ("." + ds[1:] if len(ds) > 1 else "") + "E" + str(point - 1)
    return ("-" if d < 0 else "") + s


def _d2i(d: float) -> int:
    """static_cast<int64_t>(double): truncation; out of range (and NaN) as x86-64's cvttsd2si answers."""
    if d != d or math.isinf(d) or not (-2.0 ** 63 <= d < 2.0 ** 63):
        return I64_MIN
    return int(d)


def _str_to_int(s: str) -> Optional[int]:
    """folly::tryTo<int64_t>: optional spaces, sign, digits, optional spaces; in range."""
    m = re.fullmatch(r"\s*([+-]?\d+)\s*", s)
    if not m:
        return None
    v = int(m.group(1))
    return v if I64_MIN <= v <= I64_MAX else None


def _str_to_double(s: str) -> Optional[float]:
    """folly::tryTo<double>: optional spaces, a decimal number or nan / inf / infinity, optional spaces."""
    t = s.strip(" \t\n\r\f\v")
    if re.fullmatch(r"[+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?", t) or re.fullmatch(r"-?(nan|inf|infinity)", t, re.I):
        return float(t)
    return None


def cast_to(cell, t: int):
    """InterimResult::castTo: the cell as a value of schema type t. Raises SetError with the cast's text."""
    kind, v = _norm(cell)
    if kind == "empty":
        raise SetError("Type not supported yet")
    if t in (T_INT, T_VID, T_TIMESTAMP):
        out = {T_INT: "int", T_VID: "id", T_TIMESTAMP: "timestamp"}[t]
        if kind in ("int", "id", "timestamp"):
            return (out, v)
        if kind == "double":
            return (out, _d2i(v))
        if kind == "bool":
            return (out, int(v))
        r = _str_to_int(v)
        if r is None:
            raise SetError({T_INT: "Casting from string `%s' to int failed.", T_VID: "Casting from string %s to vid failed.",
                            T_TIMESTAMP: "Casting from string %s to timestamp failed."}[t] % v)
        return (out, r)
    if t == T_DOUBLE:
        if kind == "double":
            return (kind, v)
        if kind in ("int", "id", "timestamp", "bool"):
            return ("double", float(int(v)))
        r = _str_to_double(v)
        if r is None:
            raise SetError("Casting from string %s to double failed." % v)
        return ("double", r)
    if t == T_BOOL:
        if kind == "bool":
            return (kind, v)
        if kind == "str":
            return ("bool", v == "")                              # castToBool: col->get_str().empty()
        return ("bool", v != 0)
    if t == T_STRING:
        if kind == "str":
            return (kind, v)
        if kind == "double":
            return ("str", _double_str(v))
        return ("str", str(int(v)))                               # folly::to<std::string>(bool) is "1" / "0"
    raise SetError("Type not supported yet")


# ----------------------------------------------------------------------------- the operators
def apply(op: str, lnames: Sequence[str], ltypes: Sequence[int], lrows: Sequence[tuple],
          rnames: Sequence[str], rtypes: Sequence[int], rrows: Sequence[tuple]) -> Tuple[List[str], List[int], List[tuple]]:
    """`left op right` for op "UNION ALL", "UNION" (DISTINCT), "INTERSECT" or "MINUS" over two interim results
    (column names, schema types, rows): (column names, types, rows). Raises SetError with the reference's text."""
    if op not in ("UNION ALL", "UNION", "INTERSECT", "MINUS"):
        raise SetError("Unknown operator: %s" % op)
    names = list(lnames)
    if len(lnames) != len(rnames):
        raise SetError("Field count not match.")
    if not lrows and not rrows:
        return names, [], []
    if op in ("UNION ALL", "UNION"):
        if not lrows:
            return names, list(rtypes), list(rrows)
        if not rrows:
            return names, list(ltypes), list(lrows)
    elif op == "INTERSECT":
        if not lrows or not rrows:
            return names, [], []
    else:
        if not lrows:
            return names, [], []
        if not rrows:
            return names, list(ltypes), list(lrows)
    casts = [(i, lt) for i, (lt, rt) in enumerate(zip(ltypes, rtypes)) if lt != rt]        # checkSchema
    if casts:
        cast = []
        for row in rrows:                                         # doCasting
            row = list(row)
            for i, t in casts:
                row[i] = cast_to(row[i], t)
            cast.append(tuple(row))
        rrows = cast
    types = list(ltypes)
    if op == "UNION ALL":
        return names, types, list(lrows) + list(rrows)
    if op == "UNION":
        rows = sorted(list(lrows) + list(rrows), key=_order_key)  # stable: the first of equal rows leads
        out, last = [], None
        for row in rows:
            k = row_key(row)
            if k is None or k != last:
                out.append(row)
            last = k
        return names, types, out
    if op == "INTERSECT":
        have = {}                                                 # per value the right rows not moved out yet, in order
        for row in reversed(rrows):
            k = row_key(row)
            if k is not None:
                have.setdefault(k, []).append(row)
        out = []
        for row in lrows:
            k = row_key(row)
            if k is not None and have.get(k):
                out.append(have[k].pop())                         # the right row is what doIntersect emits
        return names, types, out
    there = {k for k in map(row_key, rrows) if k is not None}
    return names, types, [row for row in lrows if row_key(row) not in there]
