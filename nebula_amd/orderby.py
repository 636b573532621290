"""ORDER BY and LIMIT over an interim result: host-side restatement of graphd's OrderByExecutor and
LimitExecutor.

  - OrderByExecutor::beforeExecute (src/graph/OrderByExecutor.cpp:122-162): no input at all succeeds with
    nothing; checkIfDuplicateColumn runs first; an input without rows answers with its column names before
    the factors are looked up; a factor that is not an input column is the execution error
    `Field (abc) not exist in input schema.`;
  - its comparator (:88-105) over ColumnValue::operator< / == (:14-68): factors in order; int / vid /
    timestamp as signed 64-bit, bool false < true, double by value (-0.0 == 0.0), strings as unsigned bytes
    with a proper prefix first; DESC is operator>;
  - LimitExecutor::execute (src/graph/LimitExecutor.cpp:33-74): rows [offset, offset + count) of the input
    in input order; a count of 0, an offset at or past the end and an empty input give the column names
    and no rows. The output schema is the input's.
The reference sorts with std::sort, so rows equal on every factor come out in no fixed order; here the
sort is stable (ties keep input order), which is one of the reference's outcomes and makes the host answer
deterministic. These functions serve every backend and are the specification of the device path
(ngx_go_order_by, include/nebula_gn.h). Cells are (kind, value) pairs as GoResult.rows holds them.
"""
from __future__ import annotations

import functools
from typing import List, Tuple

from . import ngql


class OrderByError(Exception):
    """A failed Status of the executor; str() is the outcome's error text."""


def _key(cell):
    """A cell's value as ColumnValue::operator< compares it (both sides have the column's type)."""
    kind, v = cell
    if kind == "str":
        return v.encode("utf-8", "surrogateescape")               # std::string: unsigned bytes, prefix first
    if kind == "empty":
        return 0 if v is None else int(v)                         # operator< of an unset value: never less
    return v


def _compare(a, b) -> int:
    ka, kb = _key(a), _key(b)
    if ka == kb:                                                  # -0.0 == 0.0
        return 0
    return -1 if ka < kb else 1 if kb < ka else 0                 # a NaN is neither: it ties, as in the reference


def order_by(s: ngql.OrderBySentence, names, types, rows) -> Tuple[List[str], List[int], List[tuple]]:
    """OrderByExecutor::execute on an interim result (names None: no input at all): (column names, column
    types, the rows in order). Raises OrderByError with the reference's Status text."""
    if names is None:
        return [], [], []
    seen = set()
    for n in names:                                               # TraverseExecutor::checkIfDuplicateColumn
        if n in seen:
            raise OrderByError("Duplicate column `%s'" % n)
        seen.add(n)
    if not rows:
        return list(names), [], []
    index = {n: i for i, n in enumerate(names)}
    factors = []
    for col, desc in s.factors:
        if col not in index:
            raise OrderByError("Field (%s) not exist in input schema." % col)
        factors.append((index[col], desc))

    def cmp(x, y):
        for i, desc in factors:
            c = _compare(x[i], y[i])
            if c:
                return -c if desc else c
        return 0
    return list(names), list(types), sorted(rows, key=functools.cmp_to_key(cmp))


def limit(s: ngql.LimitSentence, names, types, rows) -> Tuple[List[str], List[int], List[tuple]]:
    """LimitExecutor::execute on an interim result (names None: no input at all)."""
    if names is None:
        return [], [], []
    if s.offset < 0:                                              # LimitExecutor::prepare
        raise OrderByError("SyntaxError: skip `%d' is illegal" % s.offset)
    if s.count < 0:
        raise OrderByError("SyntaxError: count `%d' is illegal" % s.count)
    out = list(rows[s.offset:s.offset + s.count]) if s.count else []
    return list(names), (list(types) if out else []), out
