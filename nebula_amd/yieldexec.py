"""`| YIELD <columns> [WHERE <expr>]` over an interim result: host-side restatement of graphd's YieldExecutor.

  - prepareYield / checkAggFun / syntaxCheck (src/graph/YieldExecutor.cpp:33-133): `$-.*` / `$var.*` expand to
    the input's columns, the SyntaxError outcomes with the reference's texts;
  - executeInputs (:171-279): the undefined variable, empty inputs (no rows at all, COUNT(*) included), the
    duplicate-column check, the output schema from the yields evaluated on the FIRST INPUT row
    (getOutputSchema :287-341, Collector::getSchema), then per row in input order WHERE and either one output
    row or every column's value converted (Executor::toColumnValue) and applied to its function
    (src/graph/AggregateFunction.h, restated in groupby.py); inputs with rows of which WHERE keeps none still
    give one aggregate row.
It is the fallback for every backend and the specification of the device path (ngx_go_yield,
include/nebula_gn.h). Cells are (kind, value) pairs as GoResult.rows holds them.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

from . import groupby, ngql

T_UNKNOWN, T_BOOL, T_INT, T_VID, T_FLOAT, T_DOUBLE, T_STRING, T_TIMESTAMP = 0, 1, 2, 3, 4, 5, 6, 21
_TYPE_KIND = groupby._TYPE_KIND
_CAST_TYPE = (T_INT, T_STRING, T_DOUBLE, T_BOOL, T_TIMESTAMP)      # ColumnType -> SupportedType
# SupportedType read as cpp2::ColumnValue::Type (executeInputs casts one to the other): the types toColumnValue knows
_COLUMN_VALUE = {T_BOOL: "bool", T_INT: "int", T_VID: "id", T_DOUBLE: "double", T_STRING: "str"}


class YieldError(Exception):
    """A failed Status of the executor; str() is the outcome's error text."""


def _is_ref(e) -> bool:
    return isinstance(e, ngql.Prop) and e.kind in (ngql.K_INPUT_PROP, ngql.K_VAR_PROP)


def as_bool(v) -> bool:
    """Expression::asBool (Expressions.h:284-298): a string is true when it is empty."""
    if isinstance(v, str):
        return len(v) == 0
    return bool(v)


def _cast(ctype: int, v):
    """TypeCastingExpression::eval."""
    t = ctype % 5
    try:
        if t in (0, 4):
            if isinstance(v, str):
                return ngql.to_i64(int(v.strip().rstrip("\0"), 10))
            return int(v)
        if t == 2:
            return float(v.rstrip("\0")) if isinstance(v, str) else float(v)
        if t == 3:
            return as_bool(v)
    except (ValueError, OverflowError):
        raise YieldError("Cast failed")
    if isinstance(v, bool):
        return "true" if v else "false"
    if isinstance(v, float):
        return repr(v)
    return str(v)


def eval_expr(e: ngql.Expr, row, index):
    """Expression::eval over one input row ($-.x and $var.x both read it). Operators and functions are groupby.py's:
    each node is evaluated there over the values of its operands."""
    try:
        if isinstance(e, ngql.Prim):
            return e.value
        if isinstance(e, ngql.Prop):
            if not _is_ref(e) or e.prop not in index:
                raise YieldError("`%s' cannot be evaluated here" % e.to_string())
            return row[index[e.prop]][1]
        if isinstance(e, ngql.Cast):
            return _cast(e.ctype, eval_expr(e.operand, row, index))
        if isinstance(e, ngql.Unary):
            return groupby._eval(ngql.Unary(e.op, ngql.Prim(eval_expr(e.operand, row, index))), (), {})[0]
        if isinstance(e, ngql.Binary):
            a, b = eval_expr(e.left, row, index), eval_expr(e.right, row, index)
            return groupby._eval(ngql.Binary(e.kind, e.op, ngql.Prim(a), ngql.Prim(b)), (), {})[0]
        if isinstance(e, ngql.Func):
            return groupby._eval(ngql.Func(e.name, [ngql.Prim(eval_expr(a, row, index)) for a in e.args]), (), {})[0]
    except groupby.GroupByError as ex:
        raise YieldError(str(ex))
    raise YieldError("`%s' cannot be evaluated here" % e.to_string())


def expand(s: ngql.YieldSentence, inp, variables) -> List[ngql.AggCol]:
    """YieldClauseWrapper::prepare (TraverseExecutor.cpp:344-420): `$-.*` / `$var.*` -> a column per input column."""
    cols = []
    for y in s.yields:
        e = y.expr
        if isinstance(e, ngql.Prop) and e.kind == ngql.K_INPUT_PROP:
            if inp is None:
                raise YieldError("Inputs nullptr.")
            if e.prop == "*":
                cols += [ngql.AggCol(ngql.Prop(e.kind, e.ref, e.alias, n)) for n in inp.names]
                continue
        elif isinstance(e, ngql.Prop) and e.kind == ngql.K_VAR_PROP and e.prop == "*":
            v = variables.get(e.alias)
            if v is None:
                raise YieldError("Variable `%s' not defined." % e.alias)
            cols += [ngql.AggCol(ngql.Prop(e.kind, e.ref, e.alias, n)) for n in v.names]
            continue
        cols.append(y)
    return cols


def check_agg(yields: List[ngql.AggCol]) -> bool:
    """checkAggFun: whether the sentence aggregates; a bare input column beside a function is refused."""
    if not any(y.fun for y in yields):
        return False
    for y in yields:
        if _is_ref(y.expr) and not y.fun:
            raise YieldError("SyntaxError: Input columns without aggregation are not supported in YIELD statement "
                             "without GROUP BY, near `%s'" % y.expr.to_string())
    return True


def syntax_check(s: ngql.YieldSentence, yields: List[ngql.AggCol]) -> Optional[str]:
    """syntaxCheck: the variable the sentence reads (None: the pipe's input)."""
    props = [p for y in yields for p in y.expr.props()] + (s.where.props() if s.where is not None else [])
    kinds = {k for k, _, _ in props}
    if kinds - {ngql.K_INPUT_PROP, ngql.K_VAR_PROP}:
        raise YieldError("SyntaxError: Only support input and variable in yield sentence.")
    if ngql.K_INPUT_PROP in kinds and ngql.K_VAR_PROP in kinds:
        raise YieldError("Not support both input and variable.")
    names = {a for k, a, _ in props if k == ngql.K_VAR_PROP}
    if len(names) > 1:
        raise YieldError("Only one variable allowed to use.")
    return names.pop() if names else None


def column_type(e: ngql.Expr, names, types, value) -> int:
    """calculateExprType of a yield column, UNKNOWN resolved by the first row's value (Collector::getSchema)."""
    if _is_ref(e):
        t = types[names.index(e.prop)] if e.prop in names and names.index(e.prop) < len(types) else T_UNKNOWN
        if t != T_UNKNOWN:
            return t
    elif isinstance(e, ngql.Cast):
        return _CAST_TYPE[e.ctype % 5]
    elif isinstance(e, ngql.Binary) and e.kind in (ngql.K_REL, ngql.K_LOGIC):
        return T_BOOL
    if isinstance(value, bool):
        return T_BOOL
    if isinstance(value, int):
        return T_INT
    if isinstance(value, float):
        return T_DOUBLE
    return T_STRING


def _column_value(v, t: int) -> tuple:
    """Executor::toColumnValue under the output schema's type (Executor.cpp:300-352)."""
    kind = _COLUMN_VALUE.get(t)
    if kind is None:
        raise YieldError("Wrong Type: %d" % t)
    own = "bool" if isinstance(v, bool) else "int" if isinstance(v, int) else "double" if isinstance(v, float) else "str"
    if own != ("int" if kind == "id" else kind):
        raise YieldError("Wrong Type: %d" % t)
    return kind, v


def run_constant(s: ngql.YieldSentence) -> Tuple[List[str], List[int], List[tuple]]:
    """YieldExecutor::AggregateConstant (:382-417): a sentence without input whose columns carry functions. Every
    column is evaluated once, converted under its own type and applied to its function: one row."""
    check_agg(s.yields)
    syntax_check(s, s.yields)
    cells = []
    for y in s.yields:
        f = groupby.FUNCS[y.fun]()
        v = eval_expr(y.expr, (), {})
        f.apply(("bool" if isinstance(v, bool) else "int" if isinstance(v, int) else "double" if isinstance(v, float)
                 else "str", v))
        cells.append(f.result())
    return s.column_names(), [groupby._KIND_TYPE[k] for k, _ in cells], [tuple(cells)]


def run(s: ngql.YieldSentence, inp, variables) -> Tuple[List[str], List[int], List[tuple]]:
    """YieldExecutor::execute over inputs: (column names, column types, rows). inp is the pipe's Interim or None,
    variables the name -> Interim table. Raises YieldError with the reference's Status text."""
    yields = expand(s, inp, variables)
    aggregate = check_agg(yields)
    out_names = [y.alias if y.alias else y.expr.to_string() for y in yields]
    var = syntax_check(s, yields)
    if var is not None:
        if var not in variables:
            raise YieldError("Variable `%s' not defined." % var)
        inp = variables[var]
    if inp is None or not inp.rows:                               # no rows at all, COUNT(*) included
        return out_names, [], []
    seen = set()
    for n in inp.names:                                           # TraverseExecutor::checkIfDuplicateColumn
        if n in seen:
            raise YieldError("Duplicate column `%s'" % n)
        seen.add(n)
    names, types = list(inp.names), list(inp.types)
    for k, _, prop in [p for y in yields for p in y.expr.props()] + (s.where.props() if s.where is not None else []):
        if prop not in names:
            raise YieldError("column `%s' not exist in %s." % (prop, "variable" if k == ngql.K_VAR_PROP else "input"))
    index = {n: i for i, n in enumerate(names)}
    rows = groupby.typed_rows(names, types, inp.rows)
    first = [eval_expr(y.expr, rows[0], index) for y in yields]   # getOutputSchema: the first input row, kept or not
    out_types = [column_type(y.expr, names, types, v) for y, v in zip(yields, first)]
    funs = [groupby.FUNCS[y.fun]() for y in yields] if aggregate else []
    out = []
    for row in rows:
        if s.where is not None and not as_bool(eval_expr(s.where, row, index)):
            continue
        vals = [eval_expr(y.expr, row, index) for y in yields]
        if not aggregate:
            out.append(tuple((_TYPE_KIND.get(t, "empty"), v) for t, v in zip(out_types, vals)))
            continue
        for f, v, t in zip(funs, vals, out_types):
            f.apply(_column_value(v, t))
    if not aggregate:
        return out_names, out_types, out
    cells = []
    for f, y in zip(funs, yields):
        if y.fun == "AVG" and f.n == 0:                           # 0.0 / 0
            cells.append(("double", float("nan")))
            continue
        c = f.result()
        if c[0] not in groupby._KIND_TYPE:                        # InterimResult::getResultWriter
            raise YieldError("Not Support: %d" % groupby._KIND_RANK.get(c[0], 0))
        cells.append(c)
    return out_names, [groupby._KIND_TYPE[k] for k, _ in cells], [tuple(cells)]
