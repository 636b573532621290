"""ngx_set_op (UNION DISTINCT / INTERSECT / MINUS in HBM) on synthetic device-resident results, against the
Counter reference of tests/setopdev.py: the multiset of output rows always, the very cells in order where
include/nebula_gn.h promises them (MINUS; INTERSECT and UNION DISTINCT over inputs without equal rows).

Shapes are the smallest that reach each path: row counts off the wave and workgroup sizes; one workgroup
sweeping 157 times with its LDS row-id buffer flushed inside the loop (set_grid_max = 1, asserted through
set_loop_flushes), uneven sweeps (3), the same on poisoned scratch; one value in every row (the hot slot: a
wave's equal rows take one atomic); every stored width against every other; +-0.0, NaNs; strings of 0 .. 256
bytes; each refusal; the output cap; and the neighbouring calls' results unchanged by a set call between them.
"""
import numpy as np
import pytest

from nebula_amd import engine
from tests import devresult as dr
from tests import setopdev as sd

pytestmark = pytest.mark.gpu

APPEND_BUF = 2048                                                 # kernels.h kOrderAppendBuf


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


def _pair_cols(rng, n, lo=-40, hi=40):
    """(int8 column with many equal values, int64 column of few values): equal rows within and across sides."""
    return [(dr.T_INT, 1, rng.integers(lo, hi, n).astype(np.int8)),
            (dr.T_VID, 8, rng.integers(0, 3, n).astype(np.int64) * (2 ** 40 + 1) - 2 ** 40)]


@pytest.mark.parametrize("nl,nr", [(1, 1), (63, 257), (64, 64), (65, 1), (257, 63), (1, 65), (5003, 64), (64, 5003)])
def test_row_counts(eng, nl, nr):
    rng = np.random.default_rng(100 * nl + nr)
    left, right = dr.DevResult(_pair_cols(rng, nl)), dr.DevResult(_pair_cols(rng, nr))
    for op in sd.OPS:
        sd.check(eng, left, right, op)


def test_rows_without_equals_come_in_order(eng):
    """No two equal rows on a side: INTERSECT is the left rows found right, in left order; UNION DISTINCT the left
    rows, then the right rows not left, in right order. Cell for cell."""
    rng = np.random.default_rng(5)
    a, b = rng.permutation(3000)[:1500], rng.permutation(3000)[:1100]
    left = dr.DevResult([(dr.T_INT, 2, a.astype(np.int16) - 1500), (dr.T_INT, 0, 7)])
    right = dr.DevResult([(dr.T_INT, 4, b.astype(np.int32) - 1500), (dr.T_INT, 8, np.full(len(b), 7, dtype=np.int64))])
    for op in sd.OPS:
        sd.check(eng, left, right, op, exact=True)


@pytest.fixture(scope="module")
def swept():
    rng = np.random.default_rng(21)
    nl, nr = 40019, 5003
    cols = lambda n: [(dr.T_INT, 4, rng.integers(0, 9000, n).astype(np.int32)), (dr.T_INT, 1, rng.integers(0, 2, n).astype(np.int8))]
    return dr.DevResult(cols(nl)), dr.DevResult(cols(nr))


@pytest.mark.parametrize("grid", [1, 3])
def test_capped_grid(eng, swept, grid):
    left, right = swept
    kept = len(sd.reference(left, right, sd.MINUS)[0])
    assert kept > APPEND_BUF - 256                                # one workgroup cannot hold them: it flushes in its loop
    eng.set_flag("set_grid_max", grid)
    try:
        before = eng.get_flag("set_loop_flushes")
        for op in sd.OPS:
            sd.check(eng, left, right, op)
        if grid == 1:
            assert eng.get_flag("set_loop_flushes") > before
    finally:
        eng.set_flag("set_grid_max", 0)


def test_capped_grid_on_poisoned_scratch(eng, swept):
    left, right = swept
    eng.set_flag("poison_buffers", 1)
    try:
        e2 = engine.Engine(0)
        try:
            e2.set_flag("set_grid_max", 3)
            for op in sd.OPS:
                sd.check(e2, left, right, op)
            e2.set_flag("set_grid_max", 0)
            for op in sd.OPS:
                sd.check(e2, left, right, op)
        finally:
            e2.close()
    finally:
        eng.set_flag("poison_buffers", 0)


@pytest.mark.parametrize("nl,nr", [(70000, 50000), (50000, 70000)])
def test_one_value_everywhere(eng, nl, nr):
    """Every row equal on both sides: one table slot takes every count and every ticket."""
    left = dr.DevResult([(dr.T_INT, 8, np.full(nl, -9, dtype=np.int64)), (dr.T_STRING, 8, [b"same"] * nl)])
    right = dr.DevResult([(dr.T_INT, 1, np.full(nr, -9, dtype=np.int8)), (dr.T_STRING, 8, [b"same"] * nr)])
    assert len(sd.check(eng, left, right, sd.INTERSECT, exact=True)) == min(nl, nr)
    assert len(sd.check(eng, left, right, sd.MINUS)) == 0
    assert len(sd.check(eng, left, right, sd.UNION)) == 1


@pytest.mark.parametrize("cl", [1, 2, 3])
@pytest.mark.parametrize("cr", [1, 2, 3])
def test_intersect_multiplicity(eng, cl, cr):
    left = dr.DevResult([(dr.T_INT, 8, np.array([5] * cl + [6, 6, 7], dtype=np.int64))])
    right = dr.DevResult([(dr.T_INT, 8, np.array([8, 6] + [5] * cr, dtype=np.int64))])
    rows = sd.check(eng, left, right, sd.INTERSECT, exact=True)
    assert rows == [((dr.T_INT, 5),)] * min(cl, cr) + [((dr.T_INT, 6),)]
    assert sd.check(eng, left, right, sd.MINUS) == [((dr.T_INT, 7),)]


WIDTHS = (0, 1, 2, 4, 8)


def _width_col(w, vals):
    return (dr.T_INT, 0, int(vals[0])) if w == 0 else (dr.T_INT, w, vals)


def test_every_stored_width_against_every_other(eng):
    """The same values stored at different widths on the two sides are the same rows (negative ones too: each
    width is sign-extended); a width-0 column is its constant in every row."""
    rng = np.random.default_rng(8)
    n = 300
    for wl in WIDTHS:
        for wr in WIDTHS:
            a = rng.integers(-128, 128, n) if wl else np.full(n, -77)
            b = rng.integers(-128, 128, n - 9) if wr else np.full(n - 9, -77)
            tag_l, tag_r = rng.integers(-3, 0, n), rng.integers(-3, 0, n - 9)
            a[:20], b[:20], tag_l[:20], tag_r[:20] = -77, -77, -1, -1      # rows that do meet, whatever the widths
            left = dr.DevResult([_width_col(wl, a), (dr.T_INT, 8, tag_l.astype(np.int64))])
            right = dr.DevResult([_width_col(wr, b), (dr.T_INT, 1, tag_r.astype(np.int8))])
            for op in sd.OPS:
                rows = sd.check(eng, left, right, op)
                if op == sd.INTERSECT:
                    assert rows, (wl, wr)                         # the widths did meet


def _f64(bits):
    return np.array(bits, dtype=np.uint64).view(np.float64)


QNAN, NEG_QNAN, SNAN = 0x7FF8000000000000, 0xFFF8000000000001, 0x7FF0000000000001
NEG_ZERO = 0x8000000000000000


def test_doubles_by_value(eng):
    left = dr.DevResult([(dr.T_DOUBLE, 8, _f64([NEG_ZERO, 0, QNAN, NEG_QNAN, SNAN, 0x3FF0000000000000, QNAN])),
                         (dr.T_INT, 8, np.array([1, 1, 2, 2, 2, 3, 2], dtype=np.int64))])
    right = dr.DevResult([(dr.T_DOUBLE, 8, _f64([0, QNAN, NEG_QNAN, SNAN, 0x7FF0000000000000])),
                          (dr.T_INT, 8, np.array([1, 2, 2, 2, 3], dtype=np.int64))])
    inter = sd.check(eng, left, right, sd.INTERSECT)
    assert [sd.cell_key(r) for r in inter] == [(0.0, 1)]          # -0.0 met 0.0 (once: one right row); no NaN met a NaN
    minus = sd.check(eng, left, right, sd.MINUS)
    assert minus == left.rows([2, 3, 4, 5, 6])                    # both zeros leave, every NaN row stays
    uni = sd.check(eng, left, right, sd.UNION)
    assert len(uni) == 1 + 4 + 1 + 3 + 1                          # one zero, 4 + 3 NaN rows, 1.0, +inf
    nans = dr.DevResult([(dr.T_DOUBLE, 8, _f64([QNAN] * 70 + [NEG_QNAN] * 70))])
    assert sd.check(eng, nans, nans, sd.MINUS) == nans.rows(range(140))
    assert sd.check(eng, nans, nans, sd.INTERSECT) == []
    assert len(sd.check(eng, nans, nans, sd.UNION)) == 280


def test_strings_by_length_and_bytes(eng):
    rng = np.random.default_rng(3)
    base = [b"R"[:k] + bytes(rng.integers(0, 256, max(k - 1, 0), dtype=np.uint8)) for k in (0, 1, 7, 8, 9, 64, 255, 256)]
    base += [b"s", b"s\0", b"s\0\0", b"\0", b"\xff", b"\xff\xff", b"a\0b", b"a\0c", b"x" * 256, b"x" * 255 + b"y"]
    left_s = base + [b"only-left", b"s"]
    right_s = list(reversed(base[3:])) + [b"only-right", b"s\0", b"s\0"]       # other addresses, other order
    left = dr.DevResult([(dr.T_STRING, 8, left_s), (dr.T_BOOL, 1, np.ones(len(left_s), dtype=np.int8))])
    right = dr.DevResult([(dr.T_STRING, 8, right_s), (dr.T_BOOL, 8, np.ones(len(right_s), dtype=np.int64))])
    minus = sd.check(eng, left, right, sd.MINUS)
    assert [r[0][1] for r in minus] == base[:3] + [b"only-left"]
    inter = sd.check(eng, left, right, sd.INTERSECT)
    assert sorted(r[0][1] for r in inter) == sorted(base[3:])     # `s` twice left, once right: once; `s\0` once left: once
    sd.check(eng, left, right, sd.UNION)


def test_empty_sides(eng):
    some = dr.DevResult([(dr.T_INT, 8, np.array([4, 4, 5], dtype=np.int64)), (dr.T_STRING, 8, [b"a", b"a", b""])])
    none = dr.DevResult([(dr.T_INT, 8, np.zeros(0, dtype=np.int64)), (dr.T_STRING, 8, [])])
    assert sd.check(eng, none, none, sd.UNION) == []
    assert sd.check(eng, some, none, sd.UNION, exact=True) == some.rows(range(3))      # handed through, not made distinct
    assert sd.check(eng, none, some, sd.UNION, exact=True) == some.rows(range(3))
    assert sd.check(eng, some, none, sd.MINUS) == some.rows(range(3))
    for l, r, op in ((none, some, sd.MINUS), (some, none, sd.INTERSECT), (none, some, sd.INTERSECT)):
        assert sd.check(eng, l, r, op) == []


def test_refusals(eng):
    n = 5
    ints = (dr.T_INT, 8, np.arange(n, dtype=np.int64))
    one = dr.DevResult([ints])
    rc, msg = sd.set_op(eng, one, dr.DevResult([ints, ints]), sd.MINUS)
    assert (rc, msg) == (sd.E_BAD_ARGUMENT, "Field count not match.")
    cases = [
        (one, dr.DevResult([(dr.T_VID, 8, np.arange(n, dtype=np.int64))]), sd.MINUS, "set op: column types differ"),
        (one, dr.DevResult([(dr.T_DOUBLE, 8, np.arange(n, dtype=np.float64))]), sd.UNION, "set op: column types differ"),
        (dr.DevResult([(dr.T_UNKNOWN, 8, [1, 2.0, True, b"x", None])]), dr.DevResult([(dr.T_UNKNOWN, 8, [1] * n)]), sd.INTERSECT,
         "set op: UNKNOWN-typed column"),
        (dr.DevResult([ints] * 17), dr.DevResult([ints] * 17), sd.MINUS, "set op: more than 16 columns"),
        (dr.DevResult([(dr.T_STRING, 8, [b"a"] * n)]), dr.DevResult([(dr.T_STRING, 8, [b"a"] * (n - 1) + [b"z" * 257])]), sd.MINUS,
         "set op: a string longer than 256 bytes"),
        (one, one, sd.UNION_ALL, "set op: UNION ALL"),
    ]
    for left, right, op, text in cases:
        rc, msg = sd.set_op(eng, left, right, op)
        assert rc == sd.E_UNSUPPORTED and msg.startswith(text), (rc, msg)
    sixteen = dr.DevResult([ints] * 16)
    assert sd.check(eng, sixteen, sixteen, sd.INTERSECT, exact=True) == sixteen.rows(range(n))


def test_output_cap(eng):
    left = dr.DevResult([(dr.T_INT, 8, np.arange(1000, dtype=np.int64))])
    right = dr.DevResult([(dr.T_INT, 8, np.arange(300, 2000, dtype=np.int64))])
    k = len(sd.reference(left, right, sd.MINUS)[0])
    assert k == 300 and eng.get_flag("set_rows_max") == 1 << 20
    try:
        eng.set_flag("set_rows_max", k)
        assert len(sd.check(eng, left, right, sd.MINUS)) == k
        eng.set_flag("set_rows_max", k - 1)
        rc, msg = sd.set_op(eng, left, right, sd.MINUS)
        assert rc == sd.E_UNSUPPORTED and msg == "set op: output rows above set_rows_max"
        rc, msg = sd.set_op(eng, left, dr.DevResult([(dr.T_INT, 8, np.zeros(0, dtype=np.int64))]), sd.UNION)   # handed through
        assert rc == sd.E_UNSUPPORTED and msg == "set op: output rows above set_rows_max"
    finally:
        eng.set_flag("set_rows_max", 1 << 20)


def test_neighbouring_calls_unchanged(eng):
    rng = np.random.default_rng(17)
    n = 3000
    res = dr.DevResult([(dr.T_INT, 2, rng.integers(-50, 50, n).astype(np.int16)), (dr.T_STRING, 8, [b"k%d" % (i % 11) for i in range(n)]),
                        (dr.T_INT, 8, np.arange(n, dtype=np.int64))])
    other = dr.DevResult([(dr.T_INT, 8, rng.integers(-50, 50, 700).astype(np.int64)), (dr.T_STRING, 8, [b"k%d" % (i % 7) for i in range(700)]),
                          (dr.T_INT, 4, np.arange(700, dtype=np.int32) * 3)])
    order = lambda: dr.order_by(eng, res, [(0, True), (1, False)], 5, 200)
    group = lambda: sorted(dr.group_by(eng, res, [1], [("", 1), ("COUNT", -1), ("SUM", 0)])[1])
    o0, g0 = order(), group()
    assert o0[0] == 0 and o0[1] == res.rows(dr.ref_order(res, [(0, True), (1, False)], 5, 200))
    for op in sd.OPS:
        sd.check(eng, res, other, op)
    assert order() == o0 and group() == g0
