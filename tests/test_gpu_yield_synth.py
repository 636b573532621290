"""ngx_go_yield's kernels on synthetic device-resident results (tests/devresult.py), against tests/yieldref.py.

No graph, oracle or JIT: the columns are put on the GPU and the call reads them in place. Every case runs under
yield_grid_max 0 (built-in grids) and 1 (one workgroup sweeps every row) and must raise yield_device by one.
  * row counts around the wave (64) and the workgroup's chunk (256): 0, 1, 63, 64, 65, 255, 256, 257, 1025;
  * keep patterns: all, none, alternate, only the last row, lane 0 of each wave only;
  * columns of stored width 0, 1, 2, 4 and 8, a double column, a bare STRING column carried through a filter;
  * WHERE with &&, arithmetic and a double compare;
  * every supported function over an int and a double column, with an expression argument, COUNT(*), a
    function-less constant; int64 SUM wraparound;
  * the refusals, each with its reason, and the erring row.
Doubles are small integers, so every summation order gives the same bits: results compare exactly. The projection's
rows compare as lists: output order is input order.
"""
import ctypes
import math

import numpy as np
import pytest

from nebula_amd import engine, ngql
from tests import devresult as dr
from tests import yieldref

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1025)
PATTERNS = ("all", "none", "alternate", "last", "lane0")
NAMES = ["a", "b", "c", "d", "k", "x", "s", "p"]
K_CONST = 7


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


def pattern(name, n):
    i = np.arange(n)
    return {"all": np.ones(n, bool), "none": np.zeros(n, bool), "alternate": i % 2 == 1, "last": i == n - 1,
            "lane0": i % 64 == 0}[name]


_results = {}


def result(n, pat):
    """(DevResult, columns dict): widths 1 / 2 / 4 / 8 / 0, a double, a string, the keep column."""
    if (n, pat) not in _results:
        i = np.arange(n, dtype=np.int64)
        cols = {"a": (i * 7 % 251 - 125), "b": (i * 131 % 60001 - 30000), "c": (i * 100003 % (2 ** 31) - 2 ** 30),
                "d": i * 1000003 * 999983 % (2 ** 40) - 2 ** 39, "k": np.full(n, K_CONST, np.int64),
                "x": (i * 13 % 1000 - 500).astype(np.float64), "s": [("s%d" % (j * j)).encode() for j in range(n)],
                "p": pattern(pat, n).astype(np.int64)}
        res = dr.DevResult([(dr.T_INT, 1, cols["a"]), (dr.T_INT, 2, cols["b"]), (dr.T_VID, 4, cols["c"]),
                            (dr.T_INT, 8, cols["d"]), (dr.T_INT, 0, K_CONST) if n else (dr.T_INT, 8, cols["k"]),
                            (dr.T_DOUBLE, 8, cols["x"]), (dr.T_STRING, 8, cols["s"]), (dr.T_INT, 1, cols["p"])])
        _results[(n, pat)] = (res, cols)
    return _results[(n, pat)]


def call(e, res, text, names=NAMES):
    """ngx_go_yield of the sentence `text` on the synthetic result: (code, error or rows, col_types)."""
    s = ngql.parse_yield(text)
    spec = engine.YieldSpec(list(names), s.where.encode() if s.where is not None else None,
                            [(y.fun, y.expr.encode()) for y in s.yields])
    out = engine.GoResult(ok=True, error="", code=0, col_types=[], rows=[])
    e._yield(ctypes.pointer(res.struct), spec, out)
    if not out.ok:
        return out.code, out.error, []
    return 0, [tuple(v for _, v in row) for row in out.rows], list(out.col_types)


def same(got, want):
    if len(got) != len(want):
        return False
    for g, w in zip(got, want):
        for x, y in zip(g, w):
            if isinstance(y, float) and math.isnan(y):
                if not (isinstance(x, float) and math.isnan(x)):
                    return False
            elif x != y or type(x) is not type(y):
                return False
    return True


WHERE = "$-.p == 1 && $-.a + 1 > -1000 && $-.x >= -500.0"
PROJECT = "YIELD $-.a, $-.b, $-.c, $-.d, $-.k, $-.x, $-.s, $-.a * 2 + $-.k AS e, $-.x / 2.0 AS h, $-.a > 0 AS g WHERE " + WHERE
PROJECT_EXPRS = [lambda c: c["a"], lambda c: c["b"], lambda c: c["c"], lambda c: c["d"], lambda c: c["k"],
                 lambda c: c["x"], lambda c: [v.decode() for v in c["s"]], lambda c: c["a"] * 2 + c["k"],
                 lambda c: c["x"] / 2.0, lambda c: c["a"] > 0]
AGG = ("YIELD COUNT(*), COUNT($-.s), SUM($-.a), SUM($-.d), SUM($-.c), SUM($-.x), AVG($-.b), AVG($-.x), BIT_AND($-.d), "
       "BIT_OR($-.a), BIT_XOR($-.b), SUM($-.a * 2), AVG($-.x + 1.0), SUM($-.k) WHERE " + WHERE)
AGG_YIELDS = [("COUNT", None), ("COUNT", None), ("SUM", lambda c: c["a"]), ("SUM", lambda c: c["d"]),
              ("SUM", lambda c: c["c"]), ("SUM", lambda c: c["x"]), ("AVG", lambda c: c["b"]), ("AVG", lambda c: c["x"]),
              ("BIT_AND", lambda c: c["d"]), ("BIT_OR", lambda c: c["a"]), ("BIT_XOR", lambda c: c["b"]),
              ("SUM", lambda c: c["a"] * 2), ("AVG", lambda c: c["x"] + 1.0), ("SUM", lambda c: c["k"])]
# MAX / MIN and a function-less constant need a kept row (the reference fails the sentence without one)
AGG_KEPT = "YIELD MAX($-.a), MIN($-.d), MAX($-.x), MIN($-.x), MAX($-.c), 1 + 1, MIN($-.b - 1) WHERE " + WHERE
AGG_KEPT_YIELDS = [("MAX", lambda c: c["a"]), ("MIN", lambda c: c["d"]), ("MAX", lambda c: c["x"]),
                   ("MIN", lambda c: c["x"]), ("MAX", lambda c: c["c"]), ("", lambda c: np.full(len(c["a"]), 2)),
                   ("MIN", lambda c: c["b"] - 1)]


@pytest.mark.parametrize("grid", (0, 1))
@pytest.mark.parametrize("pat", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_forms(eng, n, pat, grid):
    res, cols = result(n, pat)
    mask = pattern(pat, n)
    eng.set_flag("yield_grid_max", grid)
    try:
        before = eng.get_flag("yield_device")
        rc, rows, types = call(eng, res, PROJECT)
        assert rc == 0, rows
        assert same(rows, yieldref.project(cols, mask, PROJECT_EXPRS))            # as lists: input order
        if rows:
            assert types == [dr.T_INT, dr.T_INT, dr.T_VID, dr.T_INT, dr.T_INT, dr.T_DOUBLE, dr.T_STRING, dr.T_INT,
                             dr.T_DOUBLE, dr.T_BOOL]
        rc, rows, types = call(eng, res, AGG)
        assert rc == 0, rows
        assert same(rows, [yieldref.aggregate(cols, mask, AGG_YIELDS)] if n else [])
        if rows:                          # a VID sum keeps its type; a sum nothing was added to is the integer 0
            assert types[:5] == [dr.T_INT, dr.T_INT, dr.T_INT, dr.T_INT, dr.T_VID if mask.any() else dr.T_INT]
        rc, rows, types = call(eng, res, AGG_KEPT)
        if n and mask.any():
            assert rc == 0, rows
            assert same(rows, [yieldref.aggregate(cols, mask, AGG_KEPT_YIELDS)])
            assert eng.get_flag("yield_device") == before + 3
        elif n:
            assert rc == engine.E_UNSUPPORTED and rows.startswith("yield: no row kept")
        else:
            assert rc == 0 and rows == []
    finally:
        eng.set_flag("yield_grid_max", 0)


@pytest.mark.parametrize("grid", (0, 1))
def test_no_where_keeps_every_row(eng, grid):
    res, cols = result(257, "alternate")
    eng.set_flag("yield_grid_max", grid)
    try:
        rc, rows, _ = call(eng, res, "YIELD $-.s, $-.d AS v")
        assert rc == 0 and same(rows, yieldref.project(cols, np.ones(257, bool), [PROJECT_EXPRS[6], PROJECT_EXPRS[3]]))
        rc, rows, _ = call(eng, res, "YIELD COUNT(*), SUM($-.b)")
        assert rc == 0 and rows == [(257, int(cols["b"].sum()))]
    finally:
        eng.set_flag("yield_grid_max", 0)


def test_sum_wraps(eng):
    d = np.array([2 ** 63 - 1, 2 ** 63 - 1, 5, -2 ** 63], dtype=np.int64)
    res = dr.DevResult([(dr.T_INT, 8, d)])
    rc, rows, _ = call(eng, res, "YIELD SUM($-.d), COUNT(*)", ["d"])
    assert rc == 0 and rows == [(ngql.to_i64(int(d.astype(object).sum())), 4)]


def test_first_row_types_and_rows_none_kept(eng):
    """The types come from the first input row although WHERE drops it; rows in, none kept: still one row."""
    res, cols = result(65, "last")
    rc, rows, types = call(eng, res, "YIELD $-.a + 0.5 AS v WHERE $-.p == 1")
    assert rc == 0 and rows == [(float(cols["a"][64]) + 0.5,)] and types == [dr.T_DOUBLE]
    rc, rows, types = call(eng, res, "YIELD COUNT(*), SUM($-.a), AVG($-.x) WHERE $-.p == 2")
    assert rc == 0 and len(rows) == 1 and rows[0][:2] == (0, 0) and math.isnan(rows[0][2])


def test_erring_row_is_refused(eng):
    a = np.arange(1, 301, dtype=np.int64)
    b = np.ones(300, dtype=np.int64)
    b[200] = 0
    res = dr.DevResult([(dr.T_INT, 8, a), (dr.T_INT, 1, b)])
    before = eng.get_flag("yield_device")
    for text in ("YIELD $-.a / $-.b AS q", "YIELD SUM($-.a / $-.b)", "YIELD $-.a WHERE $-.a / $-.b > 0"):
        rc, err, _ = call(eng, res, text, ["a", "b"])
        assert rc == engine.E_UNSUPPORTED and err == "yield: an expression failed on a row", (text, err)
    assert eng.get_flag("yield_device") == before
    rc, rows, _ = call(eng, res, "YIELD $-.a / $-.b AS q WHERE $-.b != 0", ["a", "b"])     # the row is filtered out first
    assert rc == 0 and len(rows) == 299


@pytest.mark.parametrize("text, reason", [
    ("YIELD $-.u", "yield: UNKNOWN-typed column"),
    ("YIELD COUNT_DISTINCT($-.a)", "yield: COUNT_DISTINCT"),
    ("YIELD STD($-.a)", "yield: STD"),
    ("YIELD (string)$-.a AS t", "yield: an expression whose value is a string"),
    ("YIELD MAX($-.s)", "yield: MAX / MIN of a BOOL or STRING value"),
    ("YIELD $-.nope", "yield: column `nope' is not in the input"),
])
def test_refusals(eng, text, reason):
    res = dr.DevResult([(dr.T_INT, 8, np.arange(10)), (dr.T_UNKNOWN, 8, [1, 2.0] * 5), (dr.T_STRING, 8, [b"x"] * 10)])
    before = eng.get_flag("yield_device")
    rc, err, _ = call(eng, res, text, ["a", "u", "s"])
    assert rc == engine.E_UNSUPPORTED and err.startswith(reason), err
    assert eng.get_flag("yield_device") == before


def test_yield_grid_max_range(eng):
    for bad in (-1, 1025):
        with pytest.raises(engine.EngineError, match="yield_grid_max"):
            eng.set_flag("yield_grid_max", bad)
    assert eng.get_flag("yield_grid_max") == 0


@pytest.mark.parametrize("grid", (0, 1))
def test_double_sum_of_negative_zeros(eng, grid):
    """-0.0 + -0.0 is -0.0: the lanes that add nothing and the untouched state words must not turn it into +0.0."""
    x = np.full(300, -0.0)
    p = (np.arange(300) % 3 == 0).astype(np.int64)
    res = dr.DevResult([(dr.T_DOUBLE, 8, x), (dr.T_INT, 1, p)])
    eng.set_flag("yield_grid_max", grid)
    try:
        rc, rows, _ = call(eng, res, "YIELD SUM($-.x), AVG($-.x), COUNT(*) WHERE $-.p == 1", ["x", "p"])
        assert rc == 0 and rows[0][2] == 100
        assert rows[0][0] == 0.0 and math.copysign(1.0, rows[0][0]) == -1.0
        assert rows[0][1] == 0.0 and math.copysign(1.0, rows[0][1]) == -1.0
    finally:
        eng.set_flag("yield_grid_max", 0)


def test_types_with_no_row_kept(eng):
    """A projection that keeps no row still answers the first input row's types."""
    res, cols = result(65, "none")
    rc, rows, types = call(eng, res, "YIELD $-.c, $-.x / 2.0 AS h, $-.s WHERE $-.p == 1")
    assert rc == 0 and rows == [] and types == [dr.T_VID, dr.T_DOUBLE, dr.T_STRING]
