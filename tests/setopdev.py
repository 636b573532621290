"""ngx_set_op over two synthetic device-resident results (tests/devresult.py), and a plain reference.

The reference is collections.Counter arithmetic over canonical row keys: an integer by value (whatever width
stored it), a double by value with -0.0 read as 0.0, a string by its bytes; a row holding a NaN has no key and
equals nothing. It follows SetExecutor's loops (src/graph/SetExecutor.cpp): MINUS drops every left row equal to
a right row, INTERSECT lets each right row match once, UNION DISTINCT keeps one row per key and every NaN row.
"""
from __future__ import annotations

import ctypes
import struct
from collections import Counter
from typing import List, Optional, Tuple

import numpy as np

from nebula_amd import engine
from tests import devresult as dr

UNION, INTERSECT, MINUS, UNION_ALL = 0, 1, 2, 3                    # NGX_SET_*
OPS = (UNION, INTERSECT, MINUS)
E_BAD_ARGUMENT, E_UNSUPPORTED = -1001, -1002


def set_op(e: engine.Engine, left: dr.DevResult, right: dr.DevResult, op: int):
    """(0, output rows as cells, doubles as bits) or (error code, ngx_last_error's text); a completed call must
    raise set_op_device by one, a refused one must leave it."""
    before = e.get_flag("set_op_device")
    plan = engine.SetPlanC(op)
    out = ctypes.POINTER(engine.SetResultC)()
    rc = e.L.ngx_set_op(e.h, ctypes.byref(left.struct), ctypes.byref(right.struct), ctypes.byref(plan), ctypes.byref(out))
    try:
        if rc:
            assert e.get_flag("set_op_device") == before
            return rc, e.L.ngx_last_error(e.h).decode()
        assert e.get_flag("set_op_device") == before + 1
        o = out.contents
        assert o.left_rows == left.n and o.right_rows == right.n and o.ncols == len(left.cols)
        strings = ctypes.string_at(o.strings, o.strings_len) if o.strings_len else b""
        return 0, dr._decode(o.cells, o.nrows, o.ncols, strings, True)
    finally:
        e.L.ngx_set_result_free(out)


def _float(bits: int) -> float:
    return struct.unpack("<d", struct.pack("<q", bits))[0]


def cell_key(row: tuple) -> tuple:
    """The canonical key of an output row of cells; a NaN row keeps its bits (it is compared as itself)."""
    out = []
    for kind, v in row:
        if kind == dr.CELL_DOUBLE:
            f = _float(v)
            out.append(("nan", v) if f != f else f + 0.0)
        else:
            out.append(v)
    return tuple(out)


def row_keys(c: dr.Columns) -> List[Optional[tuple]]:
    """Per row its canonical key, None for a row holding a NaN."""
    cols = []
    for y, (t, w, data) in enumerate(c.cols):
        v = c.values(y)
        if t == dr.T_DOUBLE:
            cols.append([None if x != x else x + 0.0 for x in v.tolist()])
        elif isinstance(v, np.ndarray):
            cols.append(v.tolist())
        else:
            cols.append([bytes(x) for x in v])
    return [None if any(x is None for x in k) else k for k in zip(*cols)] if c.n else []


def reference(left: dr.Columns, right: dr.Columns, op: int) -> Tuple[List[int], List[int]]:
    """(left row indices, right row indices) of the output as the reference's loops pick them, each ascending."""
    kl, kr = row_keys(left), row_keys(right)
    if not kl and not kr:
        return [], []
    if op == UNION:
        if not kl or not kr:                                      # handed through as it is
            return list(range(len(kl))), list(range(len(kr)))
        seen, outl, outr = set(), [], []
        for keys, out in ((kl, outl), (kr, outr)):
            for i, k in enumerate(keys):
                if k is None or k not in seen:
                    out.append(i)
                    if k is not None:
                        seen.add(k)
        return outl, outr
    if op == INTERSECT:
        have = Counter(k for k in kr if k is not None)
        out = []
        for i, k in enumerate(kl):
            if k is not None and have[k] > 0:
                have[k] -= 1
                out.append(i)
        return out, []
    there = set(kr)
    return [i for i, k in enumerate(kl) if k is None or k not in there], []


def check(e: engine.Engine, left: dr.DevResult, right: dr.DevResult, op: int, exact: Optional[bool] = None):
    """Run the operator and compare with the reference: always the multiset of canonical rows; with exact (the
    default for MINUS, whose rows and order the header fixes) the very cells in order."""
    rc, rows = set_op(e, left, right, op)
    assert rc == 0, rows
    il, ir = reference(left, right, op)
    want = left.rows(il) + right.rows(ir)
    assert len(rows) == len(want), f"op {op}: {len(rows)} rows, not {len(want)}"
    assert Counter(cell_key(r) for r in rows) == Counter(cell_key(r) for r in want)
    if exact or (exact is None and op == MINUS):
        if rows != want:
            bad = next(i for i in range(len(rows)) if rows[i] != want[i])
            raise AssertionError(f"op {op}: place {bad} is {rows[bad]}, not {want[bad]}")
    return rows
