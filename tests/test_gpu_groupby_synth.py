"""ngx_go_group_by on synthetic device-resident results (tests/devresult.py) against ref_group.

Group rows have no order: they compare as multisets, every value exactly. Double SUM / AVG are exact too,
because the summed values are integer multiples of 2^-4 small enough that every partial sum is a double
(devresult.exact_sums, asserted per case); double MAX / MIN compare by value (-0.0 == 0.0). Every call must
raise group_by_device by one, and group_by_lds where the LDS path is meant (and only there).

What the GO-driven tests (tests/test_gpu_groupby.py) cannot reach and these do:
  * row counts: n > 2 * 1024 * 256, so the LDS accumulation's grid-stride loop sweeps three times; the same under
    group_lds_max = 0 (global atomics) and under group_grid_max = 1 (one workgroup folds every row);
  * the LDS state at exactly kGroupLdsBytes (2048 groups x 4 words) and one group past it;
  * the assign table at its highest load: n a power of two, capacity 2n, every key distinct; one key; keys that
    differ only above bit 32 or only in the low byte;
  * keys: the extremes of every stored width, a constant (width 0) key, strings with NULs, s / s + NUL, strings
    equal through 16 bytes; -0.0 / 0.0 as one COUNT_DISTINCT value; INT64_MAX / INT64_MIN sums that wrap;
    ±inf and ±0.0 under MAX / MIN; zero rows and one row.
No NaN is grouped or aggregated: the reference leaves its comparisons undefined. A DOUBLE key is refused by the
library (include/nebula_gn.h), so -0.0 == 0.0 is tested where doubles are hashed: under COUNT_DISTINCT.
"""
import collections

import numpy as np
import pytest

from nebula_amd import engine
from tests import devresult as dr

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
LDS_BYTES, LDS_GRID_MAX = 64 * 1024, 1024                         # kernels.h kGroupLdsBytes, kGroupLdsGridMax


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


def check(e, res, keys, yields, lds=None, want=None):
    """One call against the reference; lds: whether group_by_lds must rise (None: not asserted)."""
    before = e.get_flag("group_by_device"), e.get_flag("group_by_lds")
    rc, rows = dr.group_by(e, res, keys, yields)
    assert rc == 0, rows
    assert e.get_flag("group_by_device") == before[0] + 1
    if lds is not None:
        assert e.get_flag("group_by_lds") == before[1] + (1 if lds else 0)
    if want is None:
        want = dr.ref_group(res, keys, yields)
    assert len(rows) == len(want)
    got, ref = collections.Counter(rows), collections.Counter(want)
    if got != ref:
        raise AssertionError(f"{len(got - ref)} group rows differ, e.g. {next(iter(got - ref))} not among "
                             f"{sorted(ref - got, key=repr)[:3]}")
    return rows


class Flags:
    def __init__(self, e, **flags):
        self.e, self.flags = e, flags

    def __enter__(self):
        self.old = {k: self.e.get_flag(k) for k in self.flags}
        for k, v in self.flags.items():
            self.e.set_flag(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.e.set_flag(k, v)


# ----------------------------------------------------------------------------- row counts
SWEEP_YIELDS = [("", 0), ("COUNT", -1), ("SUM", 1), ("AVG", 1), ("MAX", 1), ("MIN", 1), ("BIT_AND", 1), ("BIT_OR", 1),
                ("BIT_XOR", 1), ("COUNT_DISTINCT", 1), ("SUM", 2), ("AVG", 2), ("MAX", 3), ("MIN", 3),
                ("COUNT_DISTINCT", 3)]


@pytest.fixture(scope="module")
def sweeps():
    """5 groups over 2 * 262144 + 33 rows. Column 1: int64 from a pool holding INT64_MAX, INT64_MIN (sums wrap);
    column 2: doubles whose sums are exact; column 3: doubles for MAX / MIN with ±inf and ±0.0 - in group 0 no
    value is above zero and in group 1 none below, so a zero is the maximum / minimum there."""
    n = 2 * LDS_GRID_MAX * 256 + 33
    r = np.random.default_rng(21)
    key = r.integers(0, 5, n).astype(np.int8)
    pool = np.concatenate([np.array([I64_MAX, I64_MIN, -1, 0, 1, I64_MAX - 1, I64_MIN + 1], dtype=np.int64),
                           r.integers(I64_MIN, I64_MAX, 500, dtype=np.int64, endpoint=True)])
    ival = r.choice(pool, n)
    dsum = r.integers(-2 ** 30, 2 ** 30, n).astype(np.float64) / 16
    dmm = r.choice(np.array([0.0, -0.0, np.inf, -np.inf, 1.5, -1.5, 5e-324, -5e-324, 1e300, -1e300]), n)
    dmm = np.where((key == 0) & (dmm > 0) | (key == 1) & (dmm < 0), -dmm, dmm)      # the zeros keep their signs
    res = dr.DevResult([(dr.T_INT, 1, key), (dr.T_INT, 8, ival), (dr.T_DOUBLE, 8, dsum), (dr.T_DOUBLE, 8, dmm)])
    assert dr.exact_sums(dsum, int(np.bincount(key).max()))
    for g, zero_is in ((0, max), (1, min)):
        z = dmm[key == g]
        assert zero_is(z.tolist()) == 0.0 and np.signbit(z[z == 0.0]).any() and not np.signbit(z[z == 0.0]).all()
    want = dr.ref_group(res, [0], SWEEP_YIELDS)
    sums = {row[0][1]: row[2][1] for row in want}                 # the int64 sums did wrap
    assert any(sums[g] != int(ival[key == g].astype(object).sum()) for g in range(5))
    return res, want


@pytest.mark.parametrize("mode,flags,lds", [
    ("lds", {}, True),
    ("global", {"group_lds_max": 0}, False),
    ("lds, one workgroup", {"group_grid_max": 1}, True),
    ("global, 7 workgroups", {"group_lds_max": 0, "group_grid_max": 7}, False),
])
def test_three_sweeps(eng, sweeps, mode, flags, lds):
    res, want = sweeps
    assert (res.n + 255) // 256 > 2 * LDS_GRID_MAX
    with Flags(eng, **flags):
        for k, v in flags.items():
            assert eng.get_flag(k) == v
        check(eng, res, [0], SWEEP_YIELDS, lds=lds, want=want)
    assert eng.get_flag("group_grid_max") == 0 and eng.get_flag("group_lds_max") == -1


def test_group_grid_max_range(eng):
    for bad in (-1, LDS_GRID_MAX + 1):
        with pytest.raises(engine.EngineError, match="group_grid_max"):
            eng.set_flag("group_grid_max", bad)
    assert eng.get_flag("group_grid_max") == 0


@pytest.mark.parametrize("ngroups,lds", [(2048, True), (2049, False)])
def test_lds_state_at_its_limit(eng, ngroups, lds):
    """COUNT (1 word), SUM (1) and AVG (sum + count: 2) are 4 state words a group: 2048 groups are exactly
    kGroupLdsBytes and take the LDS path under a large group_lds_max, 2049 do not. The counter tells."""
    words = 4
    assert 2048 * words * 8 == LDS_BYTES and (ngroups * words * 8 <= LDS_BYTES) == lds
    n = 3 * 2049 + 5
    r = np.random.default_rng(ngroups)
    key = r.permutation(n).astype(np.int32) % ngroups
    assert len(np.unique(key)) == ngroups
    res = dr.DevResult([(dr.T_INT, 4, key), (dr.T_INT, 8, r.integers(-2 ** 40, 2 ** 40, n))])
    with Flags(eng, group_lds_max=1 << 20):
        check(eng, res, [0], [("", 0), ("COUNT", -1), ("SUM", 1), ("AVG", 1)], lds=lds)


# ----------------------------------------------------------------------------- the assign table
def _table_keys(kind, n):
    i = np.arange(n, dtype=np.int64)
    if kind == "distinct":                                        # an odd multiplier permutes the 64-bit integers
        return (np.random.default_rng(3).permutation(n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)).view(np.int64), n
    if kind == "one":
        return np.full(n, I64_MIN, dtype=np.int64), 1
    if kind == "high bits":
        return i << np.int64(32), n
    return np.int64(0x0123456789ABCD00) | (i & np.int64(255)), 256       # "low byte"


@pytest.mark.parametrize("kind", ["distinct", "one", "high bits", "low byte"])
def test_assign_table_at_load_one_half(eng, kind):
    """n = 2^17 rows: the table's capacity is exactly 2n; with every key distinct half its slots fill."""
    n = 1 << 17
    assert n & (n - 1) == 0 and 2 * n >= 1024
    key, ngroups = _table_keys(kind, n)
    assert len(np.unique(key)) == ngroups
    v = np.random.default_rng(4).integers(-2 ** 15, 2 ** 15, n).astype(np.int16)
    res = dr.DevResult([(dr.T_INT, 8, key), (dr.T_INT, 2, v)])
    rows = check(eng, res, [0], [("", 0), ("COUNT", -1), ("SUM", 1)])
    assert len(rows) == ngroups


# ----------------------------------------------------------------------------- keys
def test_four_keys_of_every_stored_width(eng):
    r = np.random.default_rng(31)
    n = 3001
    cols = []
    for w in (1, 2, 4, 8):
        lo, hi = -(1 << (8 * w - 1)), (1 << (8 * w - 1)) - 1
        cols.append((dr.T_INT, w, r.choice(np.array([lo, hi, -1, 0, 1], dtype=np.int64), n)))
    cols.append((dr.T_INT, 8, r.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)))
    res = dr.DevResult(cols)
    rows = check(eng, res, [0, 1, 2, 3], [("", 3), ("", 2), ("", 1), ("", 0), ("COUNT", -1), ("SUM", 4), ("MIN", 4)])
    assert len(rows) > 500
    check(eng, res, [3, 0], [("", 0), ("", 3), ("MAX", 2), ("BIT_XOR", 4)])


def test_constant_key_column(eng):
    r = np.random.default_rng(32)
    n = 777
    res = dr.DevResult([(dr.T_VID, 0, I64_MIN), (dr.T_INT, 1, r.integers(-2, 3, n).astype(np.int8)),
                        (dr.T_INT, 4, r.integers(-2 ** 31, 2 ** 31, n).astype(np.int32))])
    assert len(check(eng, res, [0], [("", 0), ("COUNT", -1), ("SUM", 2)])) == 1
    assert len(check(eng, res, [0, 1], [("", 1), ("", 0), ("COUNT", -1), ("AVG", 2), ("SUM", 0)])) == 5


def test_negative_zero_is_zero_where_doubles_are_hashed(eng):
    """COUNT_DISTINCT keys its table on (keys, value): -0.0 and 0.0 are one value (ColumnValue ==). No NaN among
    them: the reference leaves a NaN's equality undefined. As a key a DOUBLE column is refused."""
    r = np.random.default_rng(33)
    n = 1000
    d = r.choice(np.array([0.0, -0.0, 1.5, -1.5, 5e-324, -5e-324, np.inf]), n)
    key = r.integers(0, 3, n).astype(np.int8)
    only_zeros = key == 2
    d[only_zeros] = np.where(r.random(int(only_zeros.sum())) < 0.5, 0.0, -0.0)
    z = d[only_zeros]
    assert np.signbit(z).any() and not np.signbit(z).all()
    res = dr.DevResult([(dr.T_INT, 1, key), (dr.T_DOUBLE, 8, d)])
    rows = check(eng, res, [0], [("", 0), ("COUNT_DISTINCT", 1), ("COUNT", -1)])
    assert ((dr.T_INT, 2), (dr.CELL_INT, 1), (dr.CELL_INT, int(only_zeros.sum()))) in rows
    before = eng.get_flag("group_by_device")
    rc, err = dr.group_by(eng, res, [1], [("", 1), ("COUNT", -1)])
    assert rc == engine.E_UNSUPPORTED and "DOUBLE key" in err
    assert eng.get_flag("group_by_device") == before


def test_string_keys(eng):
    """b"", embedded NULs, s / s + NUL as different groups, strings equal through 16 bytes, 0xFF bytes."""
    base = [b"", b"\0", b"\0\0", b"s", b"s\0", b"s\0\0", b"a\0b", b"a\0c", b"\xff", b"\xff\xff", b"0123456789abcdef",
            b"0123456789abcdefX", b"0123456789abcdefY", b"0123456789abcdef\0", b"q" * 300, b"q" * 299 + b"r"]
    r = np.random.default_rng(34)
    n = 2000
    keys = [base[i] for i in r.integers(0, len(base), n)]
    k2 = r.integers(0, 2, n).astype(np.int8)
    res = dr.DevResult([(dr.T_STRING, 8, keys), (dr.T_INT, 1, k2), (dr.T_INT, 8, r.integers(-9, 9, n))])
    assert len(check(eng, res, [0], [("", 0), ("COUNT", -1), ("SUM", 2)])) == len(base)
    assert len(check(eng, res, [1, 0], [("", 0), ("", 1), ("COUNT", -1), ("COUNT_DISTINCT", 0)])) == 2 * len(base)
    assert len(check(eng, res, [1], [("", 1), ("COUNT_DISTINCT", 0)])) == 2


def test_unknown_typed_key_is_refused(eng):
    res = dr.DevResult([(dr.T_UNKNOWN, 8, [1, 2.5, True, b"x"] * 8), (dr.T_INT, 8, np.arange(32))])
    before = eng.get_flag("group_by_device")
    rc, err = dr.group_by(eng, res, [0], [("", 0), ("COUNT", -1)])
    assert rc == engine.E_UNSUPPORTED and "UNKNOWN-typed column" in err
    assert eng.get_flag("group_by_device") == before
    check(eng, res, [1], [("", 1), ("COUNT", -1)])                # the context answers the next call


@pytest.mark.parametrize("n", [0, 1])
def test_zero_rows_and_one_row(eng, n):
    res = dr.DevResult([(dr.T_INT, 8, np.array([I64_MAX][:n], dtype=np.int64)),
                        (dr.T_DOUBLE, 8, np.array([-0.0][:n])), (dr.T_STRING, 8, [b"\0"][:n])])
    rows = check(eng, res, [0, 2], [("", 0), ("", 2), ("COUNT", -1), ("SUM", 0), ("AVG", 1), ("MAX", 1), ("MIN", 0),
                                    ("COUNT_DISTINCT", 2)])
    assert len(rows) == n
