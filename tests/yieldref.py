"""A plain numpy model of `YIELD <columns> [WHERE ...]` over columns: a boolean mask and wrapping int64 reductions.

Independent of nebula_amd/yieldexec.py (tests/test_yield_host.py pins the two to each other): a column is a numpy
int64 / float64 / bool array or a list of str, an expression a Python function of the columns dict returning an
array, and the functions are numpy reductions over the masked values.
  project(cols, mask, exprs)     -> list of rows (tuples of Python values) in input order
  aggregate(cols, mask, yields)  -> one row; yields are (function name, expr or None for `*`)
"""
from __future__ import annotations

import numpy as np


def _py(v):
    if isinstance(v, (np.bool_, bool)):
        return bool(v)
    if isinstance(v, np.integer):
        return int(v)
    if isinstance(v, np.floating):
        return float(v)
    return v


def project(cols, mask, exprs):
    vals = [e(cols) for e in exprs]
    idx = np.flatnonzero(mask)
    return [tuple(_py(v[i]) for v in vals) for i in idx.tolist()]


def aggregate(cols, mask, yields):
    n = int(np.count_nonzero(mask))
    row = []
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for fn, e in yields:
            v = None if e is None else np.asarray(e(cols))[mask]
            if fn == "COUNT":
                row.append(n)
            elif fn == "SUM" and n == 0:
                row.append(0)                                     # the integer 0 of a sum nothing was added to
            elif fn == "SUM":
                row.append(float(np.add.reduce(v)) if v.dtype == np.float64 else int(np.add.reduce(v, dtype=np.int64)))
            elif fn == "AVG":
                s = float(np.add.reduce(v)) if v.dtype == np.float64 else float(int(np.add.reduce(v, dtype=np.int64)))
                row.append(s / n if n else float("nan"))
            elif fn in ("MAX", "MIN"):
                row.append(_py(v.max() if fn == "MAX" else v.min()))
            elif fn in ("BIT_AND", "BIT_OR", "BIT_XOR"):
                op = {"BIT_AND": np.bitwise_and, "BIT_OR": np.bitwise_or, "BIT_XOR": np.bitwise_xor}[fn]
                row.append(int(op.reduce(v.astype(np.int64))) if n else 0)
            elif fn == "":
                row.append(_py(v[-1]))
            else:
                raise ValueError(fn)
    return tuple(row)
