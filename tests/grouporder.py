"""ngx_go_group_order_by on a synthetic device result (tests/devresult.py), and the check of its answer.

The reference is ref_group's rows ordered in Python by the factors' keys: integers as integers, doubles through
double_key (by value, -0.0 == 0.0), strings as bytes (unsigned, a proper prefix first), DESC reversed. Groups equal
on every factor have no fixed order (include/nebula_gn.h: the group id is the last key, and it depends on which
row won the key table's slot), so a window is compared as tests/test_gpu_orderby.py::same_window compares one:
the factor tuples place by place, a tie wholly inside the window as a set, a tie cut by a window edge as a
sub-multiset of the right size. Where the factors include every key the order is total and the rows compare exactly.
"""
import collections
import ctypes
from typing import List, Sequence, Tuple

import numpy as np

from nebula_amd import engine
from tests import devresult as dr


def group_order_by(e: engine.Engine, res: dr.DevResult, keys: Sequence[int], yields: Sequence[tuple],
                   factors: Sequence[Tuple[int, bool]], offset: int, count: int):
    """yields: (function name, column) as devresult.group_by takes them, or ("", -1, constant) for a constant
    yield column (an int or a float). (0, window rows, number of groups) or (error code, the reason, None)."""
    ks = (ctypes.c_int32 * max(1, len(keys)))(*keys)
    ys = (engine.AggColC * max(1, len(yields)))()
    for i, y in enumerate(yields):
        ys[i].fn, ys[i].col = engine.AGG_FN[y[0]], y[1]
        if y[1] < 0:
            if len(y) > 2 and isinstance(y[2], float):
                ys[i].konst.kind, ys[i].konst.v.d = dr.CELL_DOUBLE, y[2]
            elif len(y) > 2:
                ys[i].konst.kind, ys[i].konst.v.i = dr.CELL_INT, y[2]
            else:
                ys[i].konst.kind = dr.CELL_STR
    gplan = engine.GroupPlanC(len(keys), ks, len(yields), ys)
    fs = (engine.OrderFactorC * max(1, len(factors)))()
    for i, (col, desc) in enumerate(factors):
        fs[i].col, fs[i].desc = col, 1 if desc else 0
    oplan = engine.OrderPlanC(len(factors), fs, offset, count)
    out = ctypes.POINTER(engine.OrderResultC)()
    rc = e.L.ngx_go_group_order_by(e.h, ctypes.byref(res.struct), ctypes.byref(gplan), ctypes.byref(oplan), ctypes.byref(out))
    try:
        if rc:
            return rc, e.L.ngx_last_error(e.h).decode(), None
        o = out.contents
        assert o.ncols == len(yields)
        strings = ctypes.string_at(o.strings, o.strings_len) if o.strings_len else b""
        return 0, dr._decode(o.cells, o.nrows, o.ncols, strings, False), int(o.input_rows)
    finally:
        e.L.ngx_order_result_free(out)


def ref_yields(yields):
    """The yields as ref_group takes them (it knows no constant columns: they are added by with_constants)."""
    return [(y[0], y[1]) for y in yields if not (y[0] == "" and y[1] < 0)]


def with_constants(rows: List[tuple], yields) -> List[tuple]:
    """ref_group's rows with the constant yield columns put in."""
    out = []
    for r in rows:
        it, row = iter(r), []
        for y in yields:
            if y[0] == "" and y[1] < 0:
                row.append((dr.CELL_DOUBLE, y[2] + 0.0) if isinstance(y[2], float) else (dr.CELL_INT, y[2]))
            else:
                row.append(next(it))
        out.append(tuple(row))
    return out


def _ranks(rows: List[tuple], col: int) -> dict:
    """cell value -> its place among the column's distinct values"""
    kind = rows[0][col][0]
    vals = [r[col][1] for r in rows]
    if kind == dr.CELL_DOUBLE:
        keys = dr.double_key(np.array(vals, dtype=np.float64)).tolist()
        return dict(zip(vals, keys))
    return {v: i for i, v in enumerate(sorted(set(vals)))}        # ints as ints, bytes as unsigned bytes


class Ordered:
    """ref rows under one factor list: the full order, computed once."""

    def __init__(self, rows: List[tuple], factors):
        self.rows, self.factors = rows, list(factors)
        self.rank = [_ranks(rows, c) for c, _ in factors] if rows else []
        self.full = sorted(rows, key=self.tup)

    def tup(self, r):
        return tuple((-m[r[c][1]] if desc else m[r[c][1]]) if r[c][1] in m else None
                     for (c, desc), m in zip(self.factors, self.rank))

    def check(self, got: List[tuple], offset: int, count: int, total: bool = False):
        allc, gotc = collections.Counter(self.rows), collections.Counter(got)
        if not self.factors:                                      # LIMIT alone: distinct groups, each a reference row
            assert len(got) == max(0, min(len(self.rows), offset + count) - offset)
            assert not gotc - allc and all(v == 1 for v in gotc.values())
            return
        window = self.full[offset:offset + count]
        if total:
            assert got == window
            return
        assert [self.tup(r) for r in got] == [self.tup(r) for r in window]
        in_all, in_win = collections.Counter(map(self.tup, self.rows)), collections.Counter(map(self.tup, window))
        by_tup, got_by = {}, {}
        for r in self.rows:
            by_tup.setdefault(self.tup(r), collections.Counter())[r] += 1
        for r in got:
            got_by.setdefault(self.tup(r), collections.Counter())[r] += 1
        for t, n in in_win.items():
            if n == in_all[t]:
                assert got_by[t] == by_tup[t], t                  # the whole tie lies inside
            else:
                assert sum(got_by[t].values()) == n and not got_by[t] - by_tup[t], t   # cut by a window edge
