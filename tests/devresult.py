"""A synthetic device-resident GO result, and plain references of ORDER BY / GROUP BY over it.

ngx_go_order_by and ngx_go_group_by read only a few fields of ngx_go_result (code, nrows, ncols, col_types,
dev_cols[].x / len / type, dev_col_w, dev_col_const), so a test can put any columns on the GPU, fill the
struct over them and call the kernels directly: any row count, any value, no graph, oracle or JIT.
The columns are placed with hipMalloc / hipMemcpy of the HIP runtime libnebula_gn.so itself links, through
ctypes. Not with torch: the ROCm wheel brings a second copy of the HIP and HSA runtimes, and the one that
initialises second in a process finds no device ("No HIP GPUs are available" once an Engine exists), nor
would either runtime know the other's allocations.
Neither call needs a loaded space: a fresh engine.Engine(0) answers them (the context's stream and scratch
buffers exist from ngx_open on), so nothing from tests/fixtures.py is loaded here.

A column is (type, stored width, data):
  INT / VID / TIMESTAMP / BOOL   width 1 / 2 / 4 / 8 with a numpy integer array (stored as int8 / 16 / 32 / 64),
                                 or width 0 with one int (the column's constant: no array, dev_col_const)
  DOUBLE                         width 8 with a numpy float64 array (stored as its int64 bits; NaN payloads are
                                 kept: build them with .view(np.float64) of the bit patterns)
  STRING                         width 8 with a list of bytes: one uint8 blob, an int64 array of device pointers
                                 into it and a uint32 length array
  UNKNOWN                        width 8 with a list of Python values, typed per row: int (ngx_dev_column::type 1),
                                 float (2), bool (3), bytes (4), None (0: no value)
Cells come back as (kind, value) with kind the NGX_CELL_* number and value an int (doubles of an ORDER BY
result: their bits), bytes for a string (never decoded), and for an EMPTY cell None or, with str_len 1, the
bool it carries. Group results hold their doubles as floats with -0.0 read as 0.0 (MAX / MIN compare by value).

The references: ref_order is a stable sort of the row indices under order-preserving integer keys, the row
index last; ref_group is a Python dict of the key tuples with numpy int64 (wrapping) arithmetic per group.
tests/test_devresult_ref.py pins both to the host restatements (nebula_amd/orderby.py, groupby.py).
"""
from __future__ import annotations

import ctypes
from typing import List, Sequence, Tuple

import numpy as np

from nebula_amd import engine

T_UNKNOWN, T_BOOL, T_INT, T_VID, T_FLOAT, T_DOUBLE, T_STRING, T_TIMESTAMP = 0, 1, 2, 3, 4, 5, 6, 21
CELL_EMPTY, CELL_INT, CELL_DOUBLE, CELL_STR = 0, 2, 5, 6
INT_TYPES = (T_BOOL, T_INT, T_VID, T_TIMESTAMP)
_NP_INT = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}
_CELL_DT = np.dtype([("kind", "<i4"), ("len", "<i4"), ("v", "<i8")])
assert _CELL_DT.itemsize == ctypes.sizeof(engine.Cell)


_hip_rt = None


def hip():
    """The HIP runtime the library runs on: the libamdhip64 mapped into the process by loading libnebula_gn.so."""
    global _hip_rt
    if _hip_rt is None:
        engine.lib()
        with open("/proc/self/maps") as f:
            paths = {line.split()[-1] for line in f if "libamdhip64" in line}
        assert len(paths) == 1, f"one HIP runtime in the process, not {sorted(paths)}"
        H = ctypes.CDLL(paths.pop())
        H.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        H.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        H.hipFree.argtypes = [ctypes.c_void_p]
        _hip_rt = H
    return _hip_rt


class DeviceArray:
    """A numpy array's bytes in device memory (hipMalloc + a blocking hipMemcpy), freed with the object."""

    def __init__(self, a: np.ndarray):
        a = np.ascontiguousarray(a)
        self.ptr = None
        if a.nbytes:
            H = hip()
            p = ctypes.c_void_p()
            rc = H.hipMalloc(ctypes.byref(p), a.nbytes)
            assert rc == 0 and p.value, f"hipMalloc({a.nbytes}): {rc}"
            self.ptr = p.value
            rc = H.hipMemcpy(self.ptr, a.ctypes.data, a.nbytes, 1)        # hipMemcpyHostToDevice
            assert rc == 0, f"hipMemcpy: {rc}"

    def __del__(self):
        if self.ptr:
            hip().hipFree(self.ptr)
            self.ptr = None


def _bits(x: float) -> int:
    return int(np.array([x], dtype=np.float64).view(np.int64)[0])


class Columns:
    """The host side of a synthetic result: the columns as given, checked and normalised."""

    def __init__(self, cols: Sequence[tuple]):
        self.cols = []
        n = None
        for t, w, data in cols:
            if t in INT_TYPES and w == 0:
                data = int(data)
            elif t in INT_TYPES:
                data = np.ascontiguousarray(data, dtype=_NP_INT[w])
            elif t == T_DOUBLE:
                assert w == 8
                data = np.ascontiguousarray(data, dtype=np.float64)
            elif t in (T_STRING, T_UNKNOWN):
                assert w == 8
                data = list(data)
            else:
                raise ValueError(f"column type {t}")
            if not isinstance(data, int):
                assert n is None or n == len(data), "columns of different lengths"
                n = len(data)
            self.cols.append((t, w, data))
        assert n is not None, "at least one column must carry an array (it sets the row count)"
        self.n = n

    def values(self, y):
        """Column y per row: int64 array (integers), float64 array (doubles), else the list."""
        t, w, data = self.cols[y]
        if isinstance(data, int):
            return np.full(self.n, data, dtype=np.int64)
        if t in INT_TYPES:
            return data.astype(np.int64)
        return data

    def cell(self, y, r) -> tuple:
        """The cell an ORDER BY result holds for row r of column y (doubles as bits)."""
        t, w, data = self.cols[y]
        if isinstance(data, int):
            return (t, data)
        v = data[r]
        if t in INT_TYPES:
            return (t, int(v))
        if t == T_DOUBLE:
            return (CELL_DOUBLE, int(data[r:r + 1].view(np.int64)[0]))
        if t == T_STRING:
            return (CELL_STR, bytes(v))
        if isinstance(v, bool):                                   # oCellKind: a bool stays EMPTY, len 1, its value
            return (CELL_EMPTY, v)
        if isinstance(v, int):
            return (CELL_INT, v)
        if isinstance(v, float):
            return (CELL_DOUBLE, _bits(v))
        if isinstance(v, bytes):
            return (CELL_STR, v)
        return (CELL_EMPTY, None)

    def rows(self, idx) -> List[tuple]:
        return [tuple(self.cell(y, int(r)) for y in range(len(self.cols))) for r in idx]


class DevResult(Columns):
    """The columns on the GPU and an engine.GoResultC over them. Every array stays alive with the object."""

    def __init__(self, cols: Sequence[tuple]):
        super().__init__(cols)
        self._keep = []
        nc = len(self.cols)
        dev = (engine.DevColumn * nc)()
        self._types = (ctypes.c_int32 * nc)(*[t for t, _, _ in self.cols])
        self._widths = (ctypes.c_int32 * nc)(*[w for _, w, _ in self.cols])
        self._consts = (ctypes.c_int64 * nc)()

        def put(a: np.ndarray):
            d = DeviceArray(a)
            self._keep.append(d)
            return d.ptr

        def put_strings(vals: List[bytes]):
            """(pointer array, length array) of one blob; a row that is no string points at the blob's start."""
            lens = np.array([len(v) if v is not None else 0 for v in vals], dtype=np.uint32)
            off = np.zeros(len(vals), dtype=np.int64)
            off[1:] = np.cumsum(lens.astype(np.int64))[:-1]
            blob = np.frombuffer(b"".join(v for v in vals if v is not None) + b"\0", dtype=np.uint8)
            base = put(blob)
            return off + base, lens

        for y, (t, w, data) in enumerate(self.cols):
            if isinstance(data, int):
                self._consts[y] = data
            elif t in INT_TYPES:
                dev[y].x = put(data)
            elif t == T_DOUBLE:
                dev[y].x = put(data.view(np.int64))
            elif t == T_STRING:
                ptr, lens = put_strings(data)
                dev[y].x, dev[y].len = put(ptr), put(lens.view(np.int32))
            else:
                x = np.zeros(self.n, dtype=np.int64)
                ty = np.zeros(self.n, dtype=np.uint8)
                strs = [None] * self.n
                for r, v in enumerate(data):
                    if isinstance(v, bool):
                        x[r], ty[r] = int(v), 3
                    elif isinstance(v, int):
                        x[r], ty[r] = v, 1
                    elif isinstance(v, float):
                        x[r], ty[r] = _bits(v), 2
                    elif isinstance(v, bytes):
                        strs[r], ty[r] = v, 4
                ptr, lens = put_strings(strs)
                is_str = ty == 4
                x[is_str] = ptr[is_str]
                dev[y].x, dev[y].len, dev[y].type = put(x), put(lens.view(np.int32)), put(ty)
        self._dev = dev
        r = engine.GoResultC()
        r.code, r.ncols, r.nrows = 0, nc, self.n
        r.col_types = self._types
        r.dev_cols = ctypes.cast(dev, ctypes.c_void_p)
        r.dev_col_w = self._widths
        r.dev_col_const = self._consts
        self.struct = r
        rc = hip().hipDeviceSynchronize()                         # the library runs on a stream of its own
        assert rc == 0, f"hipDeviceSynchronize: {rc}"


# ----------------------------------------------------------------------------- calls
def _decode(cells_ptr, n, ncols, strings: bytes, doubles_as_bits: bool) -> List[tuple]:
    if n == 0 or ncols == 0:
        return []
    raw = ctypes.string_at(ctypes.cast(cells_ptr, ctypes.c_void_p).value, n * ncols * _CELL_DT.itemsize)
    a = np.frombuffer(raw, dtype=_CELL_DT)
    kind, ln, v = a["kind"].tolist(), a["len"].tolist(), a["v"].tolist()
    as_f = a["v"].view(np.float64)
    out = []
    for r in range(n):
        row = []
        for i in range(r * ncols, (r + 1) * ncols):
            k = kind[i]
            if k == CELL_STR:
                row.append((k, strings[v[i]:v[i] + ln[i]]))
            elif k == CELL_EMPTY:
                row.append((k, bool(v[i]) if ln[i] == 1 else None))
            elif k == CELL_DOUBLE and not doubles_as_bits:
                row.append((k, float(as_f[i]) + 0.0))
            else:
                row.append((k, v[i]))
        out.append(tuple(row))
    return out


def order_by(e: engine.Engine, res: DevResult, factors: Sequence[Tuple[int, bool]], offset: int, count: int):
    """ngx_go_order_by on the synthetic result: (0, rows in order) or (error code, ngx_last_error's text)."""
    fs = (engine.OrderFactorC * max(1, len(factors)))()
    for i, (col, desc) in enumerate(factors):
        fs[i].col, fs[i].desc = col, 1 if desc else 0
    plan = engine.OrderPlanC(len(factors), fs, offset, count)
    out = ctypes.POINTER(engine.OrderResultC)()
    rc = e.L.ngx_go_order_by(e.h, ctypes.byref(res.struct), ctypes.byref(plan), ctypes.byref(out))
    try:
        if rc:
            return rc, e.L.ngx_last_error(e.h).decode()
        o = out.contents
        assert o.input_rows == res.n and o.ncols == len(res.cols)
        strings = ctypes.string_at(o.strings, o.strings_len) if o.strings_len else b""
        return 0, _decode(o.cells, o.nrows, o.ncols, strings, True)
    finally:
        e.L.ngx_order_result_free(out)


def group_by(e: engine.Engine, res: DevResult, keys: Sequence[int], yields: Sequence[Tuple[str, int]]):
    """ngx_go_group_by on the synthetic result; yields are (function name, column), "" for a key column and
    column -1 for `*`: (0, group rows in no order) or (error code, ngx_last_error's text)."""
    ks = (ctypes.c_int32 * max(1, len(keys)))(*keys)
    ys = (engine.AggColC * max(1, len(yields)))()
    for i, (fn, col) in enumerate(yields):
        ys[i].fn, ys[i].col = engine.AGG_FN[fn], col
        if col < 0:
            ys[i].konst.kind = CELL_STR
    plan = engine.GroupPlanC(len(keys), ks, len(yields), ys)
    out = ctypes.POINTER(engine.GroupResultC)()
    rc = e.L.ngx_go_group_by(e.h, ctypes.byref(res.struct), ctypes.byref(plan), ctypes.byref(out))
    try:
        if rc:
            return rc, e.L.ngx_last_error(e.h).decode()
        g = out.contents
        assert g.ncols == len(yields)
        strings = ctypes.string_at(g.strings, g.strings_len) if g.strings_len else b""
        return 0, _decode(g.cells, g.ngroups, g.ncols, strings, False)
    finally:
        e.L.ngx_group_result_free(out)


# ----------------------------------------------------------------------------- references
def _dense_rank(sorted_unique: list, vals) -> np.ndarray:
    pos = {v: i for i, v in enumerate(sorted_unique)}
    return np.array([pos[v] for v in vals], dtype=np.int64)


def double_key(x: np.ndarray) -> np.ndarray:
    """An int64 per double that orders as include/nebula_gn.h states: by value with -0.0 == 0.0; negative NaNs
    before -inf and positive NaNs after +inf, each by its bits. Worked out from the values (a rank among the
    distinct ones), not from the device's bit trick."""
    bits = x.view(np.int64)
    nan = np.isnan(x)
    neg_nan = nan & (bits < 0)
    pos_nan = nan & (bits >= 0)
    key = np.zeros(len(x), dtype=np.int64)
    nneg = 0
    if neg_nan.any():                                             # a larger magnitude is further from -inf: first
        mags = sorted(set((bits[neg_nan] & np.int64(0x7FFFFFFFFFFFFFFF)).tolist()), reverse=True)
        key[neg_nan] = _dense_rank(mags, (bits[neg_nan] & np.int64(0x7FFFFFFFFFFFFFFF)).tolist())
        nneg = len(mags)
    uniq = np.unique(x[~nan])                                     # by value: -0.0 and 0.0 are one entry
    key[~nan] = nneg + np.searchsorted(uniq, x[~nan])
    if pos_nan.any():
        pats = sorted(set(bits[pos_nan].tolist()))
        key[pos_nan] = nneg + len(uniq) + _dense_rank(pats, bits[pos_nan].tolist())
    return key


def ref_order(columns: Columns, factors: Sequence[Tuple[int, bool]], offset: int, count: int) -> np.ndarray:
    """The row indices of rows [offset, offset + count) of the result ordered by the factors, each ascending
    or descending, with the row index as the last, ascending key."""
    n = columns.n
    keys = []
    for col, desc in factors:
        t, w, data = columns.cols[col]
        if isinstance(data, int):
            k = np.zeros(n, dtype=np.int64)
        elif t in INT_TYPES:
            k = data.astype(np.int64)
        elif t == T_DOUBLE:
            k = double_key(data)
        elif t == T_STRING:                                       # bytes compare unsigned, a proper prefix first
            k = _dense_rank(sorted(set(data)), data)
        else:
            raise ValueError("an UNKNOWN-typed column is no factor")
        keys.append(~k if desc else k)                            # ~x, not -x: INT64_MIN has no negative
    keys.append(np.arange(n, dtype=np.int64))
    order = np.lexsort(tuple(reversed(keys)))                     # lexsort's last key is the primary one
    return order[offset:offset + count]


def _group_cell(t, v) -> tuple:
    if t == T_DOUBLE:
        return (CELL_DOUBLE, float(v) + 0.0)
    if t == T_STRING:
        return (CELL_STR, bytes(v))
    return (t, int(v))


def ref_group(columns: Columns, keys: Sequence[int], yields: Sequence[Tuple[str, int]]) -> List[tuple]:
    """The group rows (in first-seen order; the device's order is not fixed): COUNT counts rows, int64 sums wrap,
    AVG = float(sum) / count, COUNT_DISTINCT is the size of a set, double MAX / MIN compare by value."""
    n = columns.n
    vals = [columns.values(y) for y in range(len(columns.cols))]

    def hashable(y):
        v = vals[y]
        if isinstance(v, np.ndarray):
            return ((v + 0.0) if v.dtype == np.float64 else v).tolist()     # -0.0 + 0.0 = 0.0: one key, one value
        return v
    groups = {}
    for r, k in enumerate(zip(*[hashable(y) for y in keys])):
        groups.setdefault(k, []).append(r)
    hashed = {}
    out = []
    with np.errstate(over="ignore"):
        for k, members in groups.items():
            idx = np.array(members, dtype=np.int64)
            row = []
            for fn, col in yields:
                t = columns.cols[col][0] if col >= 0 else T_STRING
                v = vals[col][idx] if col >= 0 and isinstance(vals[col], np.ndarray) else None
                if fn == "":
                    row.append(_group_cell(t, vals[col][members[0]]))
                elif fn == "COUNT":
                    row.append((CELL_INT, len(members)))
                elif fn == "COUNT_DISTINCT":
                    if col < 0:
                        row.append((CELL_INT, 1))
                    else:
                        if col not in hashed:
                            hashed[col] = hashable(col)
                        row.append((CELL_INT, len({hashed[col][r] for r in members})))
                elif fn == "SUM":
                    row.append((CELL_DOUBLE, float(np.add.reduce(v)) + 0.0) if t == T_DOUBLE else
                               (t, int(np.add.reduce(v, dtype=np.int64))))
                elif fn == "AVG":
                    s = float(np.add.reduce(v)) if t == T_DOUBLE else float(int(np.add.reduce(v, dtype=np.int64)))
                    row.append((CELL_DOUBLE, s / len(members) + 0.0))
                elif fn in ("MAX", "MIN"):
                    m = v.max() if fn == "MAX" else v.min()
                    row.append(_group_cell(t, m))
                elif fn in ("BIT_AND", "BIT_OR", "BIT_XOR"):
                    op = {"BIT_AND": np.bitwise_and, "BIT_OR": np.bitwise_or, "BIT_XOR": np.bitwise_xor}[fn]
                    row.append((CELL_INT, int(op.reduce(v))))
                else:
                    raise ValueError(fn)
            out.append(tuple(row))
    return out


def exact_sums(x: np.ndarray, largest_group: int) -> bool:
    """Every partial sum of up to `largest_group` of these doubles is exact in any order: integer multiples of
    2^-4, |v| < 2^30 and at most 2^20 rows a group keep |sum| * 16 below 2^54; the tighter |v| <= 2^28 asked
    here keeps it below 2^53, where every integer is a double."""
    return bool(np.all(np.isfinite(x)) and np.all(x * 16 == np.round(x * 16)) and np.all(np.abs(x) < 2.0 ** 30) and
                np.all(np.abs(x) <= 2.0 ** 28) and largest_group <= 2 ** 20)
