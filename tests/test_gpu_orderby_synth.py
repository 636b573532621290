"""ngx_go_order_by on synthetic device-resident results (tests/devresult.py) against ref_order, row for row.

The header makes the order total (the row index is the last key), so every comparison is exact: the returned
rows are the reference's window, every column of them (each result carries a non-factor int64 arange column,
so a wrong row shows as a wrong row id). Every call must raise order_by_device by one.

What the GO-driven tests (tests/test_gpu_orderby.py) cannot reach and these do:
  * row counts: three sweeps of the grid-stride loops at the built-in grid (n > 2 * 2048 * 256); one workgroup
    doing everything (order_grid_max = 1) so the LDS append buffer flushes inside the sweep loop, in the
    compaction and in the gather; a list -> list compaction, asserted through order_list_compactions; uneven
    sweeps (order_grid_max = 3);
  * values: every row tied (the 24-bit row-index level decides alone), the pivot in digit bucket 0 / 255, waves
    that hold one digit, the extremes of every stored integer width, ±0.0 / ±inf / denormals / NaNs of both
    signs and kinds, strings of 0 .. 256 bytes with NULs and 0xFF bytes, a 257-byte string (refused), an
    UNKNOWN-typed column crossing as cells, and poisoned scratch.
The path assertions are derived from the inputs with numpy inside the tests.
"""
import numpy as np
import pytest

from nebula_amd import engine
from tests import devresult as dr

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
APPEND_BUF, GRID_MAX, COMPACT_DIV = 2048, 2048, 16                # kernels.h kOrderAppendBuf, kOrderGridMax, kOrderCompactDiv


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


class Case:
    """A synthetic result with the full reference order per factor list computed once."""

    def __init__(self, cols):
        self.res = dr.DevResult(cols)
        self._full = {}

    def window(self, factors, offset, count):
        key = tuple(factors)
        if key not in self._full:
            self._full[key] = dr.ref_order(self.res, factors, 0, self.res.n)
        return self._full[key][offset:offset + count]

    def check(self, e, factors, offset, count):
        before = e.get_flag("order_by_device")
        rc, rows = dr.order_by(e, self.res, factors, offset, count)
        assert rc == 0, rows
        assert e.get_flag("order_by_device") == before + 1
        idx = self.window(factors, offset, count)
        assert len(rows) == len(idx)
        want = self.res.rows(idx)
        if rows != want:
            bad = next(i for i in range(len(rows)) if rows[i] != want[i])
            raise AssertionError(f"{factors} window ({offset}, {count}): place {bad} is {rows[bad]}, not {want[bad]}")


def _arange(n):
    return (dr.T_INT, 8, np.arange(n, dtype=np.int64))


# ----------------------------------------------------------------------------- row counts
@pytest.fixture(scope="module")
def three_sweeps():
    n = 2 * GRID_MAX * 256 + 77
    r = np.random.default_rng(11)
    return Case([(dr.T_INT, 1, r.integers(-3, 4, n).astype(np.int8)),
                 (dr.T_INT, 8, r.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)), _arange(n)])


@pytest.mark.parametrize("offset,count", [(0, 1), (0, 1000), (65000, 536)])
def test_three_sweeps_at_the_builtin_grid(eng, three_sweeps, offset, count):
    """4097 blocks of 256 rows over 2048 workgroups: workgroup 0 sweeps three times, most of them twice."""
    assert eng.get_flag("order_grid_max") == 0
    assert (three_sweeps.res.n + 255) // 256 > 2 * GRID_MAX
    three_sweeps.check(eng, [(0, True), (1, False)], offset, count)


ONE_WG_N, ONE_WG_BUCKET = 40019, 2400


@pytest.fixture(scope="module")
def one_wg():
    """First factor: value -5 on 700 rows, -4 on exactly 2400, the rest spread over -3 .. 3; second: random."""
    r = np.random.default_rng(12)
    rest = ONE_WG_N - 700 - ONE_WG_BUCKET
    c0 = np.concatenate([np.full(700, -5), np.full(ONE_WG_BUCKET, -4), r.integers(-3, 4, rest)]).astype(np.int8)
    r.shuffle(c0)
    c1 = r.integers(I64_MIN, I64_MAX, ONE_WG_N, dtype=np.int64, endpoint=True)
    return Case([(dr.T_INT, 1, c0), (dr.T_INT, 8, c1), _arange(ONE_WG_N)])


ONE_WG_FACTORS = [(0, False), (1, False)]


def _one_wg_paths(case, K):
    """From the input: the K-th row's first-factor bucket is the 2400-row one, which the pick lists (<= n / 16,
    within the list's capacity) and one workgroup can only list through an in-loop flush (> 2048 - 256 ids);
    the bucket's rows that share the pivot's top byte of the second factor are 2 .. 2400 / 16, so they are
    listed again, from the list."""
    c0, c1 = case.res.values(0), case.res.values(1)
    n = case.res.n
    below = int(np.sum(c0 < -4))
    bucket = np.flatnonzero(c0 == -4)
    assert len(bucket) == ONE_WG_BUCKET and below <= K - 1 < below + len(bucket)
    assert len(bucket) * COMPACT_DIV <= n and len(bucket) <= n // COMPACT_DIV + 1
    assert len(bucket) > APPEND_BUF - 256
    top = ((c1[bucket].astype(np.uint64) + np.uint64(2 ** 63)) >> np.uint64(56)).astype(np.int64)
    pivot = bucket[np.argsort(c1[bucket], kind="stable")[K - 1 - below]]
    tied = int(np.sum(top == top[np.flatnonzero(bucket == pivot)[0]]))
    assert 2 <= tied and tied * COMPACT_DIV <= len(bucket)


def _path_counters(e):
    return [e.get_flag(f) for f in ("order_compactions", "order_list_compactions", "order_loop_flushes")]


def _one_wg_run(e, case, offset, count):
    _one_wg_paths(case, offset + count)
    e.set_flag("order_grid_max", 1)
    try:
        assert e.get_flag("order_grid_max") == 1
        c0 = _path_counters(e)
        case.check(e, ONE_WG_FACTORS, offset, count)
        return [b - a for a, b in zip(c0, _path_counters(e))]
    finally:
        e.set_flag("order_grid_max", 0)


def test_one_workgroup_compacts_twice_and_flushes_in_its_loop(eng, one_wg):
    compactions, from_list, loop_flushes = _one_wg_run(eng, one_wg, 900, 100)
    assert compactions >= 2 and from_list >= 1
    assert loop_flushes >= 1                                      # the 2400 listed rows pass 1792 in one workgroup


def test_one_workgroup_gather_flushes_in_its_loop(eng, one_wg):
    """K = 3000 winners through one workgroup's 2048-id buffer: the gather flushes inside its loop as well."""
    assert 3000 > APPEND_BUF - 256
    compactions, from_list, loop_flushes = _one_wg_run(eng, one_wg, 2900, 100)
    assert compactions >= 2 and from_list >= 1
    assert loop_flushes >= 2                                      # the compaction's and the gather's


@pytest.mark.parametrize("offset,count", [(900, 100), (2900, 100), (0, 3000)])
def test_three_workgroups_sweep_unevenly(eng, one_wg, offset, count):
    """157 blocks over 3 workgroups: 53, 52 and 52 sweeps."""
    assert ((ONE_WG_N + 255) // 256) % 3 != 0
    _one_wg_paths(one_wg, offset + count)
    eng.set_flag("order_grid_max", 3)
    try:
        c0 = _path_counters(eng)
        one_wg.check(eng, ONE_WG_FACTORS, offset, count)
        assert _path_counters(eng)[0] - c0[0] >= 2
    finally:
        eng.set_flag("order_grid_max", 0)


def test_order_grid_max_range(eng):
    for bad in (-1, GRID_MAX + 1):
        with pytest.raises(engine.EngineError, match="order_grid_max"):
            eng.set_flag("order_grid_max", bad)
    assert eng.get_flag("order_grid_max") == 0


def test_one_workgroup_on_poisoned_scratch(one_wg):
    """A fresh context whose scratch (marks, lists, histogram, state, winners) starts as 0xA5 bytes."""
    e = engine.Engine(0)
    try:
        e.set_flag("poison_buffers", 1)
        compactions, from_list, loop_flushes = _one_wg_run(e, one_wg, 900, 100)
        assert compactions >= 2 and from_list >= 1 and loop_flushes >= 1
    finally:
        try:
            e.set_flag("poison_buffers", 0)
        finally:
            e.close()


# ----------------------------------------------------------------------------- values
def test_every_row_tied(eng):
    """A constant (width 0) factor, an int8 and a string factor, all equal: the row index decides at 24 bits."""
    n = 70000
    assert 2 ** 16 < n - 1 < 2 ** 24
    case = Case([(dr.T_INT, 0, -9), (dr.T_INT, 1, np.full(n, 5, dtype=np.int8)), (dr.T_STRING, 8, [b"same"] * n),
                 _arange(n)])
    factors = [(0, True), (1, False), (2, True)]
    assert case.window(factors, 12345, 100).tolist() == list(range(12345, 12445))
    case.check(eng, factors, 12345, 100)


@pytest.mark.parametrize("K", [1, 1000, 3000])
def test_pivot_in_the_first_and_the_last_digit_bucket(eng, K):
    """The factor's top digit is 0x00 on exactly K rows and 0xFF on the rest (n = K + 1 for K = 3000, so
    K = n - 1). Window (0, K): the pivot is the last row of bucket 0; window (K, 1): the first of bucket 255.
    The mirror (~x under DESC) gives the same digits."""
    n = 3001
    r = np.random.default_rng(K)
    x = np.where(r.permutation(n) < K, I64_MIN + r.integers(0, 2 ** 40, n), I64_MAX - r.integers(0, 2 ** 40, n))
    top = (x.astype(np.uint64) + np.uint64(2 ** 63)) >> np.uint64(56)
    assert int(np.sum(top == 0)) == K and int(np.sum(top == 255)) == n - K
    for cols, desc in (([(dr.T_INT, 8, x), _arange(n)], False), ([(dr.T_INT, 8, ~x), _arange(n)], True)):
        case = Case(cols)
        case.check(eng, [(0, desc)], 0, K)
        case.check(eng, [(0, desc)], max(K - 7, 0), min(7, K))
        if K + 1 < n:
            case.check(eng, [(0, desc)], K, 1)
            case.check(eng, [(0, desc)], 0, n - 1)


@pytest.mark.parametrize("desc", [False, True])
def test_waves_of_one_digit(eng, desc):
    """Stored sorted by the factor: every wave of 64 rows holds one value (one LDS add per wave) and its
    neighbours another; one wave has a single deviating lane; n is off the wave and the block size."""
    n = 64 * 37 + 13
    x = ((np.arange(n) // 64) * 5 - 100).astype(np.int8)
    assert len(set(x[::64].tolist())) == len(x[::64]) and n % 64 and n % 256
    x[64 * 5 + 17] = 99
    case = Case([(dr.T_INT, 1, x), _arange(n)])
    for offset, count in [(0, 1), (0, 100), (1000, 300), (n - 65, 64)]:
        case.check(eng, [(0, desc)], offset, count)


@pytest.mark.parametrize("second", [False, True])
@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("width", [1, 2, 4, 8])
def test_integer_extremes_of_every_stored_width(eng, width, desc, second):
    lo, hi = -(1 << (8 * width - 1)), (1 << (8 * width - 1)) - 1
    r = np.random.default_rng(width)
    n = 5 * 41
    x = np.array([lo, hi, -1, 0, 1] * 41, dtype={1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}[width])
    r.shuffle(x)
    lead = r.integers(0, 3, n).astype(np.int8)
    case = Case([(dr.T_INT, width, x), (dr.T_INT, 1, lead), _arange(n)])
    factors = [(1, not desc), (0, desc)] if second else [(0, desc)]
    for offset, count in [(0, 60), (77, 50), (0, n - 1), (n - 2, 1)]:
        case.check(eng, factors, offset, count)


def _special_doubles():
    bits = [0x0000000000000000, 0x8000000000000000,               # ±0.0
            0x7FF0000000000000, 0xFFF0000000000000,               # ±inf
            0x0000000000000001, 0x8000000000000001,               # ± the smallest denormal
            0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF,               # ±DBL_MAX
            0x3FF8000000000000, 0xBFF8000000000000, 0x4059000000000000, 0x3EB0C6F7A0B5ED8D,   # ±1.5, 100, 1e-6
            0x7FF8000000000000, 0x7FF8000000000123, 0xFFF8000000000000, 0xFFF8000000000456,   # quiet NaNs
            0x7FF0000000000001, 0x7FF4000000000000, 0xFFF0000000000001, 0xFFF4000000000789]   # signalling NaNs
    return np.array(bits, dtype=np.uint64).view(np.float64)


@pytest.mark.parametrize("desc", [False, True])
def test_doubles_as_a_factor_and_as_a_passenger(eng, desc):
    """NaNs are placed as include/nebula_gn.h states (tests/test_devresult_ref.py pins ref_order's rule);
    -0.0 and 0.0 tie and the row index decides. The second double column is no factor: its bits cross unchanged
    (the cells are compared as bits)."""
    sp = _special_doubles()
    r = np.random.default_rng(5)
    x = np.tile(sp, 13)
    r.shuffle(x)
    n = len(x)
    zeros = x == 0.0
    assert np.signbit(x[zeros]).any() and not np.signbit(x[zeros]).all()
    case = Case([(dr.T_DOUBLE, 8, x), (dr.T_DOUBLE, 8, x[::-1].copy()), _arange(n)])
    for offset, count in [(0, 1), (0, 50), (50, 100), (0, n - 1), (n - 30, 29)]:
        case.check(eng, [(0, desc)], offset, count)
    case.check(eng, [(2, not desc)], 3, 40)                       # both double columns as passengers


def _strings():
    base = [b"", b"\0", b"\xff", b"a", b"abcdefg", b"abcdefgh", b"abcdefghi", b"0123456789abcdef",
            b"0123456789abcdefX", b"0123456789abcdefY", b"0123456789abcdef\0", b"s", b"s\0", b"s\0\0",
            b"abcdefgh\0", b"abcdefgh\0\0", b"\0\0", b"\xff\xff", b"\xff\0", b"\0\xff", b"a\xffb", b"a\0b",
            b"x" * 255, b"x" * 256, b"x" * 255 + b"\0", b"x" * 255 + b"\xff", b"\0" * 256, b"\xff" * 256,
            b"y" * 16 + b"\0" * 239, b"y" * 16 + b"\0" * 240]
    assert {len(s) for s in base} >= {0, 1, 7, 8, 9, 16, 255, 256} and max(len(s) for s in base) == 256
    return base


@pytest.mark.parametrize("second", [False, True])
@pytest.mark.parametrize("desc", [False, True])
def test_strings_as_a_factor_and_as_a_passenger(eng, desc, second):
    """s / s + NUL / s + NUL NUL have identical words and differ only at the length level; the second string
    column is no factor: its bytes cross as they are."""
    base = _strings()
    r = np.random.default_rng(6)
    vals = [base[i] for i in r.permutation(np.repeat(np.arange(len(base)), 4))]
    n = len(vals)
    other = [bytes(r.integers(0, 256, int(k)).astype(np.uint8)) for k in r.integers(0, 40, n)]
    lead = r.integers(0, 3, n).astype(np.int8)
    case = Case([(dr.T_STRING, 8, vals), (dr.T_STRING, 8, other), (dr.T_INT, 1, lead), _arange(n)])
    factors = [(2, not desc), (0, desc)] if second else [(0, desc)]
    for offset, count in [(0, 1), (0, 40), (33, 50), (0, n - 1)]:
        case.check(eng, factors, offset, count)


def test_a_257_byte_factor_string_is_refused(eng):
    vals = [b"k" * 256, b"k" * 257, b"", b"z"] * 5
    case = Case([(dr.T_STRING, 8, vals), _arange(len(vals))])
    before = eng.get_flag("order_by_device")
    rc, err = dr.order_by(eng, case.res, [(0, False)], 0, 3)
    assert rc == engine.E_UNSUPPORTED and "longer than 256 bytes" in err
    assert eng.get_flag("order_by_device") == before
    case.check(eng, [(1, True)], 0, 3)                            # as a passenger it crosses; the context answers


def test_unknown_typed_passenger_column(eng):
    """Per-row types 1 - 4 and none: the cells are typed as orderby.hip's oCellKind states (int, double and
    string cells; a bool stays an EMPTY cell with str_len 1 and its value; no type: EMPTY)."""
    vals = [7, -1.5, True, b"str", None, I64_MIN, float("inf"), False, b"", b"\0\xff", I64_MAX, -0.0] * 9
    n = len(vals)
    key = np.random.default_rng(7).permutation(n).astype(np.int32)
    case = Case([(dr.T_UNKNOWN, 8, vals), (dr.T_INT, 4, key), _arange(n)])
    assert case.res.cell(0, 2) == (dr.CELL_EMPTY, True) and case.res.cell(0, 4) == (dr.CELL_EMPTY, None)
    for offset, count in [(0, n - 1), (5, 40)]:
        case.check(eng, [(1, False)], offset, count)
    before = eng.get_flag("order_by_device")
    rc, err = dr.order_by(eng, case.res, [(0, False)], 0, 3)
    assert rc == engine.E_UNSUPPORTED and "UNKNOWN-typed factor" in err
    assert eng.get_flag("order_by_device") == before
