"""ngx_go_group_order_by on synthetic device-resident results (tests/devresult.py) against ref_group's rows
ordered in Python (tests/grouporder.py). Every answered call must raise group_order_device by one and leave
group_by_device and order_by_device alone.

Paths, asserted from the counters where one exists:
  * global-atomic grouping (40,019 groups: no LDS copy) and a select that lists its tied groups
    (order_compactions), with one workgroup sweeping every group (order_loop_flushes) and with three;
  * LDS grouping (group_by_lds) and the same rows without it;
  * COUNT / COUNT_DISTINCT columns at 1 / 2 / 4 bytes: a count of exactly the input's row count at each boundary;
  * every yield kind as first and as second factor, both directions; keys at each stored width; string keys;
    constant yield columns (they tie every group: the group id decides);
  * the window's edges, LIMIT alone (no order_* counter moves), poisoned scratch, refusals and their prefixes.
"""
import numpy as np
import pytest

from nebula_amd import engine
from tests import devresult as dr
from tests import grouporder as go
from tests.devresult import Columns, DevResult, _decode, double_key, exact_sums, ref_group  # noqa: F401

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
DBL_MAX = float(np.finfo(np.float64).max)
COUNTERS = ("group_order_device", "group_by_device", "order_by_device")
PATHS = ("order_compactions", "order_list_compactions", "order_loop_flushes")


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


def flags(e, names):
    return [e.get_flag(f) for f in names]


class Case:
    """A synthetic result; reference group rows per (keys, yields) and their order per factor list, computed once."""

    def __init__(self, cols):
        self.res = DevResult(cols)
        self._groups, self._ordered = {}, {}

    def groups(self, keys, yields):
        k = (tuple(keys), tuple(yields))
        if k not in self._groups:
            self._groups[k] = go.with_constants(ref_group(self.res, keys, go.ref_yields(yields)), yields)
        return self._groups[k]

    def ordered(self, keys, yields, factors):
        k = (tuple(keys), tuple(yields), tuple(factors))
        if k not in self._ordered:
            self._ordered[k] = go.Ordered(self.groups(keys, yields), factors)
        return self._ordered[k]

    def check(self, e, keys, yields, factors, offset, count, total=False):
        before = flags(e, COUNTERS)
        rc, rows, ngroups = go.group_order_by(e, self.res, keys, yields, factors, offset, count)
        assert rc == 0, rows
        after = flags(e, COUNTERS)
        assert [b - a for a, b in zip(before, after)] == [1, 0, 0]
        ref = self.ordered(keys, yields, factors)
        assert ngroups == len(ref.rows)
        ref.check(rows, offset, count, total)
        return rows


# ----------------------------------------------------------------------------- many groups, a select that compacts
BIG_N, BIG_GROUPS = 2 * 262144 + 33, 40019
# (group size, groups of that size): the largest first. The K-th place of K = 1, 1000, 3536 lies in the buckets of
# 2, 900 and 2000 groups, each <= BIG_GROUPS / 16 and > 1, so the pick lists it and the SUM decides inside it.
BIG_SIZES = [(40, 2), (30, 600), (29, 900), (28, 1500), (27, 2000)]
BIG_KEYS, BIG_YIELDS = [0], [("", 0), ("COUNT", -1), ("SUM", 1)]
BIG_FACTORS = [(1, True), (2, False)]


@pytest.fixture(scope="module")
def big():
    r = np.random.default_rng(21)
    sizes = np.concatenate([np.full(m, v) for v, m in BIG_SIZES])
    rest_groups = BIG_GROUPS - len(sizes)
    rest_rows = BIG_N - int(sizes.sum())
    extra = rest_rows - 10 * rest_groups
    assert 0 <= extra <= rest_groups                              # the other groups hold 10 or 11 rows
    sizes = np.concatenate([sizes, np.full(extra, 11), np.full(rest_groups - extra, 10)])
    assert len(sizes) == BIG_GROUPS and int(sizes.sum()) == BIG_N
    keys = np.unique(r.integers(I64_MIN, I64_MAX, 2 * BIG_GROUPS, dtype=np.int64))[:BIG_GROUPS]
    assert len(keys) == BIG_GROUPS
    r.shuffle(keys)
    k = np.repeat(keys, sizes)
    r.shuffle(k)
    v = r.integers(I64_MIN, I64_MAX, BIG_N, dtype=np.int64, endpoint=True)
    return Case([(dr.T_INT, 8, k), (dr.T_INT, 8, v)])


def _big_bucket(K):
    below = 0
    for v, m in BIG_SIZES:
        if K - 1 < below + m:
            return m
        below += m
    raise AssertionError(K)


@pytest.mark.parametrize("offset,count", [(0, 1), (0, 1000), (3000, 536)])
def test_global_atomics_then_a_compacting_select(eng, big, offset, count):
    m = _big_bucket(offset + count)
    assert 1 < m and m * 16 <= BIG_GROUPS
    assert BIG_GROUPS * 2 * 8 > 64 * 1024                         # two state words a group: no LDS copy possible
    lds0, p0 = eng.get_flag("group_by_lds"), flags(eng, PATHS)
    big.check(eng, BIG_KEYS, BIG_YIELDS, BIG_FACTORS, offset, count)
    assert eng.get_flag("group_by_lds") == lds0
    assert flags(eng, PATHS)[0] - p0[0] >= 1


def test_one_workgroup_sweeps_every_group(eng, big):
    """order_grid_max = 1: the 2000 tied groups are listed by one workgroup, past the 1792 ids its buffer takes."""
    eng.set_flag("order_grid_max", 1)
    try:
        p0 = flags(eng, PATHS)
        big.check(eng, BIG_KEYS, BIG_YIELDS, BIG_FACTORS, 3000, 536)
        p1 = flags(eng, PATHS)
        assert p1[0] - p0[0] >= 1 and p1[2] - p0[2] >= 1
    finally:
        eng.set_flag("order_grid_max", 0)


def test_three_workgroups(eng, big):
    eng.set_flag("order_grid_max", 3)
    try:
        p0 = flags(eng, PATHS)
        big.check(eng, BIG_KEYS, BIG_YIELDS, BIG_FACTORS, 0, 1000)
        assert flags(eng, PATHS)[0] - p0[0] >= 1
    finally:
        eng.set_flag("order_grid_max", 0)


def test_compaction_on_poisoned_scratch(big):
    """A fresh context whose scratch (gb*, go*, ob* buffers) starts as 0xA5 bytes."""
    e = engine.Engine(0)
    try:
        e.set_flag("poison_buffers", 1)
        e.set_flag("order_grid_max", 1)
        p0 = flags(e, PATHS)
        big.check(e, BIG_KEYS, BIG_YIELDS, BIG_FACTORS, 3000, 536)
        p1 = flags(e, PATHS)
        assert p1[0] - p0[0] >= 1 and p1[2] - p0[2] >= 1
    finally:
        try:
            e.set_flag("poison_buffers", 0)
        finally:
            e.close()


def test_single_calls_are_left_alone(eng, big):
    """ngx_go_group_by and ngx_go_order_by answer as before, and group_order_device does not move."""
    before = eng.get_flag("group_order_device")
    rc, rows = dr.group_by(eng, big.res, BIG_KEYS, BIG_YIELDS)
    assert rc == 0 and sorted(rows) == sorted(big.groups(BIG_KEYS, BIG_YIELDS))
    rc, rows = dr.order_by(eng, big.res, [(1, True), (0, False)], 5, 40)
    assert rc == 0 and rows == big.res.rows(dr.ref_order(big.res, [(1, True), (0, False)], 5, 40))
    assert eng.get_flag("group_order_device") == before


# ----------------------------------------------------------------------------- few groups: LDS
@pytest.fixture(scope="module")
def five():
    r = np.random.default_rng(22)
    n = 1003
    k = r.integers(0, 5, n).astype(np.int8)
    k[:5] = np.arange(5)
    return Case([(dr.T_INT, 1, k), (dr.T_INT, 4, r.integers(-1000, 1000, n).astype(np.int32))])


@pytest.mark.parametrize("K", [1, 4, 5, 6])
def test_lds_grouping_and_without(eng, five, K):
    keys, yields, factors = [0], [("", 0), ("SUM", 1), ("COUNT", -1)], [(1, True), (0, False)]
    l0 = eng.get_flag("group_by_lds")
    a = five.check(eng, keys, yields, factors, 0, K, total=True)
    l1 = eng.get_flag("group_by_lds")
    eng.set_flag("group_lds_max", 0)
    try:
        b = five.check(eng, keys, yields, factors, 0, K, total=True)
    finally:
        eng.set_flag("group_lds_max", -1)
    assert (l1 - l0, eng.get_flag("group_by_lds") - l1) == (1, 0)
    assert a == b and len(a) == min(K, 5)


# ----------------------------------------------------------------------------- count widths
@pytest.mark.parametrize("n", [127, 128, 32767, 32768])
@pytest.mark.parametrize("fn", ["COUNT", "COUNT_DISTINCT"])
def test_a_count_of_every_row_does_not_wrap(eng, n, fn):
    """n is the largest count the width chosen for n rows must hold (127 | 128: 1 | 2 bytes, 32767 | 32768: 2 | 4).
    One group of all n rows; then n rows of which the last five stand alone, so that the select reads the column."""
    vals = np.arange(n, dtype=np.int64) * 3
    y = [("", 0), (fn, 1 if fn == "COUNT_DISTINCT" else -1)]
    one = Case([(dr.T_INT, 8, np.full(n, 7, dtype=np.int64)), (dr.T_INT, 8, vals)])
    assert one.check(eng, [0], y, [(1, True)], 0, 1, total=True) == [((dr.T_INT, 7), (dr.CELL_INT, n))]
    k = np.full(n, 7, dtype=np.int64)
    k[-5:] = np.arange(100, 105)
    some = Case([(dr.T_INT, 8, k), (dr.T_INT, 8, vals)])
    assert some.check(eng, [0], y, [(1, True)], 0, 1, total=True) == [((dr.T_INT, 7), (dr.CELL_INT, n - 5))]
    rows = some.check(eng, [0], y, [(1, False), (0, True)], 0, 6, total=True)
    assert rows[0] == ((dr.T_INT, 104), (dr.CELL_INT, 1)) and rows[5] == ((dr.T_INT, 7), (dr.CELL_INT, n - 5))


# ----------------------------------------------------------------------------- every yield kind as a factor
KN, KA, KB = 1200, 3, 13                                          # rows, values of the first key, of the second


@pytest.fixture(scope="module")
def kinds():
    """Keys ka (3 values) and kb (13), every (ka, kb) present; value columns of every stored width with their
    extremes, ints that wrap when summed, doubles whose sums are exact, doubles with +-0.0 / +-inf / +-DBL_MAX."""
    r = np.random.default_rng(23)
    ka = r.integers(0, KA, KN).astype(np.int8)
    kb = r.integers(0, KB, KN).astype(np.int16)
    ka[:KA * KB], kb[:KA * KB] = np.repeat(np.arange(KA), KB), np.tile(np.arange(KB), KA)

    def pick(vals, dtype):
        return np.array(vals, dtype=dtype)[r.integers(0, len(vals), KN)]
    i1 = pick([-128, -127, -1, 0, 1, 126, 127], np.int8)
    i2 = pick([-32768, -32767, -129, -1, 0, 128, 32766, 32767], np.int16)
    i4 = pick([-2 ** 31, -2 ** 31 + 1, -32769, 0, 32768, 2 ** 31 - 2, 2 ** 31 - 1], np.int32)
    i8 = pick([I64_MIN, I64_MIN + 1, -2 ** 31 - 1, -1, 0, 2 ** 31, I64_MAX - 1, I64_MAX], np.int64)
    dsum = r.integers(-2 ** 20, 2 ** 20, KN).astype(np.float64) / 16
    assert exact_sums(dsum, KN)
    dext = pick([0.0, -0.0, np.inf, -np.inf, DBL_MAX, -DBL_MAX, 1.5, -2.25, 5e-324], np.float64)
    few = r.integers(0, 4, KN).astype(np.int32)                   # COUNT_DISTINCT: 1 .. 4 values a group
    return Case([(dr.T_INT, 1, ka), (dr.T_INT, 2, kb), (dr.T_INT, 1, i1), (dr.T_INT, 2, i2), (dr.T_INT, 4, i4),
                 (dr.T_INT, 8, i8), (dr.T_DOUBLE, 8, dsum), (dr.T_DOUBLE, 8, dext), (dr.T_INT, 4, few)])


AGGS = [("COUNT", -1), ("COUNT_DISTINCT", 8), ("SUM", 5), ("SUM", 6), ("AVG", 4), ("AVG", 6),
        ("MAX", 2), ("MIN", 2), ("MAX", 3), ("MIN", 3), ("MAX", 4), ("MIN", 4), ("MAX", 5), ("MIN", 5),
        ("MAX", 7), ("MIN", 7), ("BIT_AND", 5), ("BIT_OR", 4), ("BIT_XOR", 5)]


@pytest.mark.parametrize("agg", AGGS, ids=lambda a: "%s_%d" % a)
def test_every_yield_kind_as_first_and_second_factor(eng, kinds, agg):
    """yields ka, kb, agg: the factors hold both keys, so every order is total and the rows compare exactly
    (double SUM / AVG over values for which exact_sums holds)."""
    keys, yields = [0, 1], [("", 0), ("", 1), agg]
    assert len(kinds.groups(keys, yields)) == KA * KB
    for desc in (False, True):
        kinds.check(eng, keys, yields, [(2, desc), (0, False), (1, False)], 0, 10, total=True)
        kinds.check(eng, keys, yields, [(0, not desc), (2, desc), (1, True)], 7, 20, total=True)
        kinds.check(eng, keys, yields, [(2, desc), (1, False), (0, True)], 0, KA * KB, total=True)


@pytest.mark.parametrize("w,vals", [(1, [-128, -1, 0, 1, 127]), (2, [-32768, -129, 0, 128, 32767]),
                                    (4, [-2 ** 31, -32769, 0, 32768, 2 ** 31 - 1]),
                                    (8, [I64_MIN, -2 ** 31 - 1, 0, 2 ** 31, I64_MAX])])
def test_an_int_key_at_each_stored_width(eng, w, vals):
    r = np.random.default_rng(24 + w)
    k = np.array(vals, dtype=dr._NP_INT[w])[np.concatenate([np.arange(5), r.integers(0, 5, 295)])]
    case = Case([(dr.T_INT, w, k), (dr.T_INT, 1, (np.arange(300) % 2).astype(np.int8))])
    yields = [("", 0), ("COUNT_DISTINCT", 1)]                     # 2 in every group of more than a few rows: a tie
    for desc in (False, True):
        for K in (2, 5):
            case.check(eng, [0], yields, [(0, desc)], 0, K, total=True)
            case.check(eng, [0], yields, [(1, False), (0, desc)], 1, K, total=True)


def _string_keys():
    s = b"same-prefix-of-16"
    out = [b"", b"\0", b"\0\0", b"\xff", b"\xff\xff", b"a", b"a\0", s, s + b"\0", s + b"\xff", s + b"\0a"]
    out += [bytes([65 + i % 26]) * i for i in (7, 8, 9, 15, 16, 17, 255, 256)]
    out += [b"x" * 255 + b"\0", b"x" * 255 + b"\xff"]
    assert len(set(out)) == len(out) and max(map(len, out)) == 256
    return out


@pytest.fixture(scope="module")
def strings():
    keys = _string_keys()
    r = np.random.default_rng(25)
    idx = np.concatenate([np.arange(len(keys)), r.integers(0, len(keys), 400)])
    r.shuffle(idx)
    return Case([(dr.T_STRING, 8, [keys[i] for i in idx]), (dr.T_INT, 4, r.integers(-9, 9, len(idx)).astype(np.int32))])


@pytest.mark.parametrize("desc", [False, True])
def test_a_string_key_as_a_factor(eng, strings, desc):
    yields, G = [("", 0), ("COUNT", -1), ("MAX", 1)], len(_string_keys())
    for offset, count in ((0, 1), (0, 7), (5, 9), (0, G), (0, G + 3)):
        strings.check(eng, [0], yields, [(0, desc)], offset, count, total=True)
        strings.check(eng, [0], yields, [(2, True), (0, desc)], offset, count, total=True)


def test_a_constant_yield_column_ties_every_group(eng, kinds):
    """As the only factor the group id decides (any groups, in the right number); before others it changes nothing."""
    for konst in (7, 2.5):
        yields = [("", -1, konst), ("", 0), ("", 1), ("COUNT", -1)]
        p0 = flags(eng, PATHS)
        rows = kinds.check(eng, [0, 1], yields, [(0, False)], 3, 10)
        assert len(rows) == 10 and len(set(rows)) == 10
        assert flags(eng, PATHS) == p0                            # no level: nothing to select
        kinds.check(eng, [0, 1], yields, [(0, True), (3, True), (1, False), (2, False)], 0, 12, total=True)


# ----------------------------------------------------------------------------- edges
def test_window_edges(eng, five):
    keys, yields, factors = [0], [("", 0), ("COUNT", -1)], [(0, True)]
    for offset, count, want in ((0, 0, 0), (5, 3, 0), (4, 3, 1), (0, 5, 5), (2, 3, 3), (7, 1, 0)):
        assert len(five.check(eng, keys, yields, factors, offset, count, total=True)) == want


def test_one_group_and_one_row(eng):
    g1 = Case([(dr.T_INT, 4, np.full(700, -3, dtype=np.int32)), (dr.T_DOUBLE, 8, np.full(700, 0.25))])
    r1 = Case([(dr.T_INT, 4, np.array([9], dtype=np.int32)), (dr.T_DOUBLE, 8, np.array([-0.0]))])
    yields = [("", 0), ("SUM", 1), ("AVG", 1), ("COUNT", -1)]
    for case in (g1, r1):
        for factors in ([(1, True)], [(3, False), (0, False)], []):
            assert len(case.check(eng, [0], yields, factors, 0, 3, total=bool(factors))) == 1
            assert case.check(eng, [0], yields, factors, 1, 3, total=bool(factors)) == []


def test_no_rows(eng):
    case = Case([(dr.T_INT, 8, np.zeros(0, dtype=np.int64)), (dr.T_INT, 8, np.zeros(0, dtype=np.int64))])
    before, p0 = flags(eng, COUNTERS), flags(eng, PATHS)
    rc, rows, ngroups = go.group_order_by(eng, case.res, [0], [("", 0), ("SUM", 1)], [(1, True)], 0, 10)
    assert (rc, rows, ngroups) == (0, [], 0)
    assert [b - a for a, b in zip(before, flags(eng, COUNTERS))] == [1, 0, 0] and flags(eng, PATHS) == p0


@pytest.mark.parametrize("offset,count", [(0, 1), (0, 100), (39000, 2000), (40018, 1)])
def test_limit_alone(eng, big, offset, count):
    """`count` distinct groups, each one of the reference's rows; no select runs."""
    p0 = flags(eng, PATHS)
    rows = big.check(eng, BIG_KEYS, BIG_YIELDS, [], offset, count)
    assert len(rows) == min(count, BIG_GROUPS - offset)
    assert flags(eng, PATHS) == p0


# ----------------------------------------------------------------------------- refusals
def test_refusals_and_their_reasons(eng, kinds):
    long_key = [b"k" * 257, b"a", b"b"] * 20
    long = Case([(dr.T_STRING, 8, long_key), (dr.T_INT, 4, np.arange(60, dtype=np.int32))])
    count = [("", 0), ("COUNT", -1)]
    nine = [(0, False)] * 9
    k_max = eng.get_flag("order_k_max")
    before = flags(eng, COUNTERS)
    for case, keys, yields, factors, offset, cnt, code, reason in [
            (kinds, [0], [("", 0), ("STD", 4)], [(1, True)], 0, 3, engine.E_UNSUPPORTED, "group by: STD"),
            (kinds, [6], [("", 6), ("COUNT", -1)], [(1, True)], 0, 3, engine.E_UNSUPPORTED, "group by: DOUBLE key"),
            (kinds, [0], count, [(1, True)], k_max - 1, 2, engine.E_UNSUPPORTED, "order by: offset + count above order_k_max"),
            (kinds, [0], count, nine, 0, 3, engine.E_UNSUPPORTED, "order by: more than 8 factors"),
            (long, [0], count, [(0, False)], 0, 2, engine.E_UNSUPPORTED, "order by: a factor string longer than 256 bytes"),
            (kinds, [0], count, [(2, False)], 0, 3, engine.E_BAD_ARGUMENT, "order by: no such result column"),
            (kinds, [0], count, [(-1, False)], 0, 3, engine.E_BAD_ARGUMENT, "order by: no such result column")]:
        rc, err, _ = go.group_order_by(eng, case.res, keys, yields, factors, offset, cnt)
        assert rc == code and err.startswith(reason), (rc, err)
    assert flags(eng, COUNTERS) == before
    rows = long.check(eng, [0], count, [(1, True), (0, False)][:1], 0, 3)    # the long key as a passenger crosses
    assert len(rows) == 3 and {r[0][1] for r in rows} == set(long_key)
