"""The references of tests/devresult.py against what the suite already trusts: ref_order against
nebula_amd.orderby.order_by (stable, so ties keep input order: the row index as the last key) and ref_group
against nebula_amd.groupby.run, on random small results with integers of every stored width, doubles (±0.0,
±inf, no NaN: the host comparator ties a NaN with everything) and byte strings with NULs, 0xFF bytes and
prefixes of each other. No GPU: only the host side (devresult.Columns) is built."""
import collections
import random

import numpy as np
import pytest

from nebula_amd import groupby, ngql, orderby
from tests import devresult as dr

KIND = {dr.T_BOOL: "bool", dr.T_INT: "int", dr.T_VID: "id", dr.T_TIMESTAMP: "timestamp", dr.T_DOUBLE: "double",
        dr.T_STRING: "str"}
N = 200


def _columns(seed):
    rng = random.Random(seed)
    r = np.random.default_rng(seed)
    words = [b"", b"\0", b"a", b"a\0", b"a\0\0", b"ab", b"\xff", b"\xff\xff", b"abcdefgh", b"abcdefghi",
             b"abcdefgh\0", b"0123456789abcdefX", b"0123456789abcdefY"]
    dbl = np.array([0.0, -0.0, 1.5, -1.5, np.inf, -np.inf, 5e-324, -5e-324, 1.7976931348623157e308, 2.0 ** -4, 3.0])
    return dr.Columns([
        (dr.T_INT, 1, r.choice(np.array([-128, 127, -1, 0, 1], dtype=np.int8), N)),
        (dr.T_VID, 8, r.choice(np.array([-2 ** 63, 2 ** 63 - 1, -1, 0, 1, 1 << 32, 255], dtype=np.int64), N)),
        (dr.T_DOUBLE, 8, r.choice(dbl, N)),
        (dr.T_STRING, 8, [rng.choice(words) for _ in range(N)]),
        (dr.T_INT, 2, r.integers(-2 ** 15, 2 ** 15, N, dtype=np.int16)),
        (dr.T_INT, 0, 7),
        (dr.T_DOUBLE, 8, r.integers(-2 ** 20, 2 ** 20, N).astype(np.float64) / 16),
        (dr.T_INT, 8, np.arange(N, dtype=np.int64)),
    ])


def _host_rows(cols):
    """The columns as the interim rows the host restatements read: (kind, value), strings as text."""
    out = []
    for r in range(cols.n):
        row = []
        for y, (t, w, data) in enumerate(cols.cols):
            v = cols.values(y)[r]
            if t == dr.T_STRING:
                row.append(("str", v.decode("utf-8", "surrogateescape")))
            elif t == dr.T_DOUBLE:
                row.append(("double", float(v)))
            else:
                row.append((KIND[t], int(v)))
        out.append(tuple(row))
    return out


@pytest.mark.parametrize("seed", range(6))
def test_ref_order_is_the_host_order_by(seed):
    cols = _columns(seed)
    names = [f"c{y}" for y in range(len(cols.cols))]
    types = [t for t, _, _ in cols.cols]
    rows = _host_rows(cols)
    rng = random.Random(100 + seed)
    for _ in range(12):
        factors = [(y, rng.random() < 0.5) for y in rng.sample(range(7), rng.randint(1, 4))]
        s = ngql.OrderBySentence([(names[y], desc) for y, desc in factors])
        _, _, want = orderby.order_by(s, names, types, rows)
        offset, count = rng.choice([(0, N), (0, 1), (17, 50), (N - 1, 5), (N, 3)])
        idx = dr.ref_order(cols, factors, offset, count)
        assert [rows[i] for i in idx] == want[offset:offset + count], factors
        assert [r[7][1] for r in want[offset:offset + count]] == idx.tolist()


def test_double_key_places_nans_as_the_header_states():
    bits = np.array([0x7FF8000000000000, 0x7FF0000000000001, 0xFFF8000000000000, 0xFFF0000000000001,
                     0x7FF0000000000000, 0xFFF0000000000000, 0x8000000000000000, 0, 1, 0x8000000000000001,
                     0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
    k = dr.double_key(bits.view(np.float64)).tolist()
    name = ["+qnan", "+snan", "-qnan", "-snan", "+inf", "-inf", "-0", "+0", "+den", "-den", "+nanmax", "-nanmax"]
    order = [name[i] for i in np.lexsort((np.arange(len(k)), k))]
    assert order == ["-nanmax", "-qnan", "-snan", "-inf", "-den", "-0", "+0", "+den", "+inf", "+snan", "+qnan",
                     "+nanmax"]
    assert k[6] == k[7]                                           # -0.0 == 0.0: a tie, the row index decides


def _normal(rows):
    """Host group rows as devresult's group cells: doubles by value with -0.0 read as 0.0, strings as bytes."""
    num = {"bool": dr.T_BOOL, "int": dr.T_INT, "id": dr.T_VID, "timestamp": dr.T_TIMESTAMP}
    out = []
    for row in rows:
        cells = []
        for kind, v in row:
            if kind == "double":
                cells.append((dr.CELL_DOUBLE, float(v) + 0.0))
            elif kind == "str":
                cells.append((dr.CELL_STR, v.encode("utf-8", "surrogateescape")))
            else:
                cells.append((num[kind], int(v)))
        out.append(tuple(cells))
    return collections.Counter(out)


GROUP_SPECS = [
    ([0], [("", 0), ("COUNT", -1), ("SUM", 1), ("AVG", 4), ("MAX", 1), ("MIN", 1), ("BIT_AND", 4), ("BIT_OR", 4),
           ("BIT_XOR", 4), ("COUNT_DISTINCT", 2), ("COUNT_DISTINCT", 3)]),
    ([3], [("", 3), ("COUNT", -1), ("SUM", 6), ("AVG", 6), ("MAX", 2), ("MIN", 2), ("COUNT_DISTINCT", 1)]),
    ([2], [("", 2), ("COUNT", -1), ("SUM", 4)]),                  # a double key: -0.0 and 0.0 are one group
    ([0, 1, 3, 5], [("", 0), ("", 1), ("", 3), ("", 5), ("COUNT", -1), ("SUM", 0), ("MAX", 6), ("MIN", 6)]),
    ([7], [("", 7), ("COUNT", -1), ("AVG", 4), ("SUM", 1)]),                # every row its own group
]


@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("spec", range(len(GROUP_SPECS)))
def test_ref_group_is_the_host_group_by(seed, spec):
    cols = _columns(seed)
    names = [f"c{y}" for y in range(len(cols.cols))]
    types = [t for t, _, _ in cols.cols]
    keys, yields = GROUP_SPECS[spec]
    assert dr.exact_sums(cols.values(6), N)
    text = "GROUP BY " + ", ".join(f"$-.{names[k]}" for k in keys) + " YIELD " + ", ".join(
        (f"{fn}({'*' if y < 0 else '$-.' + names[y]})" if fn else f"$-.{names[y]}") for fn, y in yields)
    _, _, want = groupby.run(ngql.parse_group_by(text), names, types, _host_rows(cols))
    got = dr.ref_group(cols, keys, yields)
    assert collections.Counter(got) == _normal(want)
    if spec == 2:
        zeros = [r for r in got if r[0] == (dr.CELL_DOUBLE, 0.0)]
        vals = cols.values(2)
        assert len(zeros) == 1 and zeros[0][1] == (dr.CELL_INT, int(np.sum(vals == 0.0)))
        assert np.signbit(vals[vals == 0.0]).any() and not np.signbit(vals[vals == 0.0]).all()
