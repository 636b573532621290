"""GROUP BY over an interim result: host-side restatement of graphd's GroupByExecutor.

  - GroupByExecutor::prepareYield / prepareGroup / checkAll (src/graph/GroupByExecutor.cpp:44-178):
    the SyntaxError outcomes, with the reference's texts;
  - GroupByExecutor::groupingData (:236-331): one function object per yield column and group
    (src/graph/AggregateFunction.h:130-436), fed every input row's value;
  - generateOutputSchema (:348-385): output types from the first result row.
It is the fallback for every backend and the specification of the device path (ngx_go_group_by,
include/nebula_gn.h). Cells are (kind, value) pairs as GoResult.rows holds them; an input column's
cells take the kind of the interim schema's type, as InterimResult::getRows reads them back.
Output row order is unspecified (the reference iterates an unordered_map); here it is first-seen order.
"""
from __future__ import annotations

import math
from typing import List, Optional, Tuple

from . import ngql

T_UNKNOWN, T_BOOL, T_INT, T_VID, T_FLOAT, T_DOUBLE, T_STRING, T_TIMESTAMP = 0, 1, 2, 3, 4, 5, 6, 21
_TYPE_KIND = {T_BOOL: "bool", T_INT: "int", T_VID: "id", T_FLOAT: "float", T_DOUBLE: "double",
              T_STRING: "str", T_TIMESTAMP: "timestamp"}
_KIND_TYPE = {v: k for k, v in _TYPE_KIND.items()}
_INTS = ("int", "id", "timestamp")
# cpp2::ColumnValue::Type order: the union compares its type before its value
_KIND_RANK = {"empty": 0, "bool": 1, "int": 2, "id": 3, "float": 4, "double": 5, "str": 6, "timestamp": 7}


class GroupByError(Exception):
    """A failed Status of the executor; str() is the outcome's error text."""


def _wrap(v: int) -> int:
    return ngql.to_i64(v)


# ------------------------------------------------------------------------------ expressions
def _num(v):
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise GroupByError("Wrong type of arithmetic operand")
    return v


def _eval(e: ngql.Expr, row, index):
    """Expression::eval over one input row: (python value, kind of the last $-.prop read or None)."""
    if isinstance(e, ngql.Prim):
        return e.value, None
    if isinstance(e, ngql.Prop):
        if e.kind != ngql.K_INPUT_PROP:
            raise GroupByError("`%s' is not an input property" % e.to_string())
        if e.prop not in index:
            raise GroupByError("%s is nonexistent" % e.prop)
        kind, v = row[index[e.prop]]
        return v, kind
    if isinstance(e, ngql.Unary):
        v, k = _eval(e.operand, row, index)
        if e.op == ngql.UNARY_OPS["!"]:
            return (not v), k
        _num(v)
        return (v if e.op == ngql.UNARY_OPS["+"] else (-v if isinstance(v, float) else _wrap(-v))), k
    if isinstance(e, ngql.Binary):
        a, ka = _eval(e.left, row, index)
        b, kb = _eval(e.right, row, index)
        k = kb if kb is not None else ka
        if e.kind == ngql.K_ARITH:
            op = "+-*/%^"[e.op]
            if op == "+" and isinstance(a, str) and isinstance(b, str):
                return a + b, k
            _num(a), _num(b)
            both_int = isinstance(a, int) and isinstance(b, int)
            if op == "+":
                r = a + b
            elif op == "-":
                r = a - b
            elif op == "*":
                r = a * b
            elif op == "/":
                if both_int:
                    if b == 0:
                        raise GroupByError("Division by zero")
                    r = abs(a) // abs(b) * (1 if (a < 0) == (b < 0) else -1)
                else:
                    if b == 0:
                        raise GroupByError("Division by zero")
                    r = a / b
            elif op == "%":
                if b == 0:
                    raise GroupByError("Division by zero")
                r = abs(a) % abs(b) * (1 if a >= 0 else -1) if both_int else math.fmod(a, b)
            else:
                if not both_int:
                    raise GroupByError("Arithmetic XOR needs integers")
                r = a ^ b
            return (_wrap(r) if both_int else float(r)), k
        if e.kind == ngql.K_REL:
            ops = [lambda x, y: x < y, lambda x, y: x <= y, lambda x, y: x > y, lambda x, y: x >= y,
                   lambda x, y: x == y, lambda x, y: x != y, lambda x, y: y in x]
            try:
                return bool(ops[e.op](a, b)), k
            except TypeError:
                raise GroupByError("A relational operand has the wrong type")
        ops = [lambda x, y: bool(x) and bool(y), lambda x, y: bool(x) or bool(y), lambda x, y: bool(x) != bool(y)]
        return ops[e.op](a, b), k
    if isinstance(e, ngql.Func):
        vals, k = [], None
        for a in e.args:
            v, ka = _eval(a, row, index)
            vals.append(v)
            k = ka if ka is not None else k
        return _call(e.name, vals), k
    raise GroupByError("`%s' cannot be evaluated here" % e.to_string())


def _call(name: str, a: list):
    """The FunctionManager entries (src/common/filter/FunctionManager.cpp) a grouping expression can
    reasonably use; the numeric ones return double as there."""
    one = {"abs": abs, "floor": math.floor, "ceil": math.ceil, "round": round, "sqrt": math.sqrt,
           "exp": math.exp, "log": math.log, "log2": math.log2, "log10": math.log10}
    try:
        if name in one and len(a) == 1:
            return float(one[name](float(_num(a[0]))))
        if name == "pow" and len(a) == 2:
            return float(math.pow(_num(a[0]), _num(a[1])))
        if name == "hash" and len(a) == 1:
            return ngql.eval_const(ngql.Func("hash", [ngql.Prim(a[0])]))
        if name in ("lower", "upper") and len(a) == 1 and isinstance(a[0], str):
            return a[0].lower() if name == "lower" else a[0].upper()
        if name == "length" and len(a) == 1 and isinstance(a[0], str):
            return len(a[0].encode())
    except (ValueError, OverflowError) as ex:
        raise GroupByError("%s(): %s" % (name, ex))
    raise GroupByError("Function `%s' with %d arguments is not supported in GROUP BY" % (name, len(a)))


def _to_cell(v, kind: Optional[str]) -> tuple:
    """Executor::toColumnValue (Executor.cpp:300-349): the variant under the type of the input column
    it came from, or under its own type for a constant."""
    own = "bool" if isinstance(v, bool) else "int" if isinstance(v, int) else \
        "double" if isinstance(v, float) else "str"
    if kind is None or kind == "empty":
        return own, v
    want = "int" if kind in _INTS else "double" if kind in ("float", "double") else kind
    if want != own:
        raise GroupByError("Wrong Type: %d" % _KIND_RANK.get(kind, 0))
    return kind, v


# ------------------------------------------------------------------------------ AggregateFunction.h
def _cmp_key(cell):
    return _KIND_RANK.get(cell[0], 0), cell[1]


class _Group:
    def __init__(self):
        self.col = ("empty", None)

    def apply(self, c):
        self.col = c

    def result(self):
        return self.col


class _Count:
    def __init__(self):
        self.n = 0

    def apply(self, c):
        self.n += 1

    def result(self):
        return "int", _wrap(self.n)


class _Sum:
    def __init__(self):
        self.sum = None

    def apply(self, c):
        if c[0] not in ("int", "double", "id", "timestamp"):
            return
        if self.sum is None:
            self.sum = c
        elif self.sum[0] == c[0]:
            self.sum = (c[0], self.sum[1] + c[1] if c[0] == "double" else _wrap(self.sum[1] + c[1]))

    def result(self):
        return self.sum if self.sum is not None else ("int", 0)


class _Avg:
    def __init__(self):
        self.sum, self.n = _Sum(), 0

    def apply(self, c):
        self.sum.apply(c)
        self.n += 1

    def result(self):
        kind, v = self.sum.result()
        if kind == "double":
            return "double", v / self.n
        if kind == "int":
            return "double", float(v) / self.n
        # the reference reads the double member of an id / timestamp sum: the same bits, reinterpreted
        import struct
        return "double", struct.unpack("<d", struct.pack("<q", v))[0] / self.n


class _CountDistinct:
    def __init__(self):
        self.seen = set()

    def apply(self, c):
        self.seen.add(c)

    def result(self):
        return "int", len(self.seen)


class _Max:
    sign = 1

    def __init__(self):
        self.v = None

    def apply(self, c):
        if self.v is None:
            self.v = c
        elif (_cmp_key(c) > _cmp_key(self.v)) if self.sign > 0 else (_cmp_key(c) < _cmp_key(self.v)):
            self.v = c

    def result(self):
        return self.v if self.v is not None else ("empty", None)


class _Min(_Max):
    sign = -1


class _Stdev:
    def __init__(self):
        self.avg, self.elems = _Avg(), []

    def apply(self, c):
        self.avg.apply(c)
        if c[0] == "int":
            self.elems.append(float(c[1]))
        elif c[0] == "double":
            self.elems.append(c[1])

    def result(self):
        if not self.elems:
            return "int", 0
        avg = self.avg.result()[1]
        acc = 0.0
        for x in self.elems:
            acc += (x - avg) * (x - avg)
        return "double", math.sqrt(acc / len(self.elems))


def _bit(op):
    class _Bit:
        def __init__(self):
            self.v = None

        def apply(self, c):
            if c[0] != "int":
                return
            self.v = c[1] if self.v is None else op(self.v, c[1])

        def result(self):
            return "int", (self.v if self.v is not None else 0)
    return _Bit


FUNCS = {"": _Group, "COUNT": _Count, "COUNT_DISTINCT": _CountDistinct, "SUM": _Sum, "AVG": _Avg, "MAX": _Max,
         "MIN": _Min, "STD": _Stdev, "BIT_AND": _bit(lambda a, b: a & b), "BIT_OR": _bit(lambda a, b: a | b),
         "BIT_XOR": _bit(lambda a, b: a ^ b)}


# ------------------------------------------------------------------------------ the executor
def prepare(s: ngql.GroupBySentence) -> dict:
    """prepareYield + prepareGroup: raises GroupByError; returns the alias table (alias -> yield column)
    of the yield columns that are input properties."""
    if not s.yields:
        raise GroupByError("SyntaxError: Yield cols is empty")
    aliases = {}
    for y in s.yields:
        if y.fun not in ("COUNT", "COUNT_DISTINCT") and y.expr.to_string() == "*":
            raise GroupByError("SyntaxError: Syntax error: near `*'")
        if y.alias and isinstance(y.expr, ngql.Prop) and y.expr.kind == ngql.K_INPUT_PROP:
            aliases.setdefault(y.alias, y)
    if not s.groups:
        raise GroupByError("SyntaxError: Group cols is empty")
    for g in s.groups:
        if g.fun:
            raise GroupByError("SyntaxError: Use invalid group function `%s'" % g.fun)
    return aliases


def _is_input(e):
    return isinstance(e, ngql.Prop) and e.kind == ngql.K_INPUT_PROP


def check_all(s: ngql.GroupBySentence, aliases: dict, names: List[str]) -> List[ngql.AggCol]:
    """checkAll: the group columns with alias names replaced by the columns they name."""
    groups, input_groups = [], set()
    for g in s.groups:
        if _is_input(g.expr):
            if g.expr.prop not in names:
                raise GroupByError("SyntaxError: Group `%s' isn't in output fields" % g.expr.prop)
            input_groups.add(g.expr.prop)
        elif isinstance(g.expr, ngql.Func):
            pass
        else:
            name = g.expr.to_string()
            if name not in aliases:
                raise GroupByError("SyntaxError: Group `%s' isn't in output fields" % name)
            g = aliases[name]
            input_groups.add(g.expr.prop)
        groups.append(g)
    for y in s.yields:
        if _is_input(y.expr):
            if y.expr.prop not in names:
                raise GroupByError("SyntaxError: Yield `%s' isn't in output fields" % y.expr.prop)
            if y.expr.prop not in input_groups and not y.fun:
                raise GroupByError("SyntaxError: Yield `%s' isn't in group fields" % y.expr.prop)
        elif isinstance(y.expr, ngql.Prop) and y.expr.kind == ngql.K_VAR_PROP:
            raise GroupByError("SyntaxError: Can't support variableExpression")
    return groups


def typed_rows(names, types, rows) -> List[tuple]:
    """The input rows as InterimResult::getRows returns them: each cell under its column's schema type."""
    out = []
    for r in rows:
        cells = []
        for c, (kind, v) in enumerate(r):
            want = _TYPE_KIND.get(types[c]) if c < len(types) else None
            if want in _INTS and kind in _INTS:
                kind = want
            cells.append((kind, v))
        out.append(tuple(cells))
    return out


def run(s: ngql.GroupBySentence, names: List[str], types: List[int], rows: List[tuple]
        ) -> Tuple[List[str], List[int], List[tuple]]:
    """GroupByExecutor::execute on an interim result: (column names, column types, group rows).
    Raises GroupByError with the reference's Status text."""
    aliases = prepare(s)
    out_names = s.column_names()
    if not rows:                                                  # onEmptyInputs: checkAll is not reached
        return out_names, [], []
    seen = set()
    for n in names:                                               # TraverseExecutor::checkIfDuplicateColumn
        if n in seen:
            raise GroupByError("Duplicate column `%s'" % n)
        seen.add(n)
    groups = check_all(s, aliases, list(names))
    index = {n: i for i, n in enumerate(names)}
    data = {}
    for row in typed_rows(names, types, rows):
        key = tuple(_to_cell(*_eval(g.expr, row, index)) for g in groups)
        funs = data.get(key)
        if funs is None:
            funs = data[key] = [FUNCS[y.fun]() for y in s.yields]
        for f, y in zip(funs, s.yields):
            f.apply(_to_cell(*_eval(y.expr, row, index)))
    out = [tuple(f.result() for f in funs) for funs in data.values()]
    out_types = []
    for kind, _ in out[0]:                                        # generateOutputSchema
        if kind not in _KIND_TYPE or kind == "float":
            raise GroupByError("Unknown VariantType: %d" % _KIND_RANK.get(kind, 0))
        out_types.append(_KIND_TYPE[kind])
    return out_names, out_types, out
