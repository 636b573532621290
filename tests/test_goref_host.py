"""tests/goref.py against the oracle, on the CPU: the model's authority for tests/test_gpu_go_shapes.py.

For every case and query the device module runs, the model's rows, edges scanned per hop and frontier per hop equal the
oracle's. The row-reservation graphs are checked at 65535, 65536 and 65537 rows and at a reduced size (the generator's
`rows` parameter sets the boundary at every size; the 8 * 65536 + 1 case differs from them in that parameter alone).
The comparator is shown to fail on one dropped row, one duplicated row, one cell off by 1 and one hop count off by 1;
the mirrored kernel constants are read back from the headers they come from.
"""
import os
import re

import numpy as np
import pytest

from nebula_amd import ngql
from oracle import oracle
from tests import goref

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nebula_amd", "csrc")


def test_constants_match_the_headers():
    for name, consts in goref.CONSTANTS.items():
        text = open(os.path.join(CSRC, name)).read()
        for k, v in consts.items():
            m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)" % k, text)
            assert m and int(m.group(1)) == v, (name, k, m and m.group(1), v)
    assert re.search(r"constexpr int kSparseSub = CE / WG;", open(os.path.join(CSRC, "kernels.hip")).read())
    assert re.search(r"constexpr int CE = static_cast<int>\(kChunk\);", open(os.path.join(CSRC, "final_kernels.h")).read())
    assert goref.K_SPARSE_SUB == 8
    # the exchange's named constants are the ones the kernels and the driver use
    hip = open(os.path.join(CSRC, "kernels.hip")).read()
    for use in (r"__launch_bounds__\(kXchgBlock\) void k_pack\(", r"__launch_bounds__\(kXchgBlock\) void k_merge\(",
                r"__launch_bounds__\(kListThreads\) void k_pack_list\(", r"blockIdx\.x\) \* kListTile;",
                r"kListTile == 4 \* kListThreads"):
        assert re.search(use, hip), use
    assert re.search(r"kXchgListFactor \* eMaxShard < minPeer", open(os.path.join(CSRC, "engine.cpp")).read())
    assert (goref.K_XCHG_BLOCK, goref.K_LIST_THREADS, goref.K_LIST_TILE, goref.K_XCHG_LIST_FACTOR, goref.K_MAX_WORLD) == \
        (256, 1024, 4096, 32, 64)


@pytest.mark.parametrize("name", sorted(goref.CASES))
def test_model_equals_oracle(name):
    g, _ = goref.built(name)
    o = oracle.Oracle()
    try:
        space = goref.load_oracle(o, g)
        for q in goref.CASES[name].queries:
            text = goref.case_sentence(name, q)
            ref = o.go(space, ngql.parse_go(text), pushdown=q.pushdown)
            assert ref.ok, (text[:200], ref.error)
            want = goref.case_model(name, q)
            goref.assert_same(ref, want, (name, q.form, q.over, q.direction, q.m, q.n))
            assert ref.col_types == [goref.KIND_TYPE[k] for k in goref.column_kinds(q.form)] or not ref.rows
    finally:
        o.close()


RESV_QUERIES = (      # (sentence, the model's predicate, the closed form's row selection)
    ("GO 2 STEPS FROM %d OVER e YIELD e._dst, e._rank, e.p0, e.p1", None, lambda p0: np.ones(len(p0), bool)),
    ("GO 2 STEPS FROM %d OVER e WHERE e.p0 < 1 YIELD e._dst, e._rank, e.p0, e.p1", lambda row: row.props[0] < 1,
     lambda p0: p0 < 1),
)


@pytest.mark.parametrize("rows", [1000, goref.RESV_ROWS[0], goref.RESV_ROWS[1], goref.RESV_ROWS[2]])
def test_reservation_graph(rows):
    """The numpy-built CSR's closed-form columns equal the model on the same edges, and the model equals the oracle,
    for the two sentences tests/test_gpu_go_shapes.py::test_row_reservation runs."""
    g, seeds = goref.resv_graph(rows)
    cols = goref.resv_arrays(rows)[3]
    yields = [y([1]) for y in goref.FORMS["bench"].yields]        # e._dst, e._rank, e.p0, e.p1
    o = oracle.Oracle()
    try:
        space = goref.load_oracle(o, g)
        for text, where, select in RESV_QUERIES:
            want = goref.go(g, seeds, [1], goref.FORWARD, 2, 2, where, yields, pushed_type=1 if where else None)
            ref = o.go(space, ngql.parse_go(text % seeds[0]))
            goref.assert_same(ref, want, (rows, text))
            sel = select(cols[2])
            mine = sorted(zip(*[c[sel].tolist() for c in cols]))
            assert mine == sorted(tuple(c[1] for c in r) for r in want.rows)
            assert len(mine) == (rows if where is None else (rows + 1) // 2)
    finally:
        o.close()


def _some_model():
    g, seeds = goref.frontier_edges(300)
    return goref.model(g, "keys", seeds, ["e"], n=2)


def _mutate(m, rows=None, hop_edges=None, hop_frontier=None):
    return goref.Model(m.rows if rows is None else rows, m.hop_edges if hop_edges is None else hop_edges,
                       m.hop_frontier if hop_frontier is None else hop_frontier)


def test_comparator_notices():
    m = _some_model()
    assert len(m.rows) == 300 and len(m.hop_edges) == 2
    goref.assert_same(m, m)
    goref.assert_same(_mutate(m, rows=list(reversed(m.rows))), m)          # order is free
    bad = [
        _mutate(m, rows=m.rows[:-1]),                                      # one row dropped
        _mutate(m, rows=m.rows + [m.rows[7]]),                             # one row twice
        _mutate(m, hop_edges=[m.hop_edges[0], m.hop_edges[1] + 1]),        # a hop count off by 1
        _mutate(m, hop_frontier=[m.hop_frontier[0], m.hop_frontier[1] - 1]),
        _mutate(m, hop_edges=m.hop_edges + [0], hop_frontier=m.hop_frontier + [0]),
    ]
    for c in range(len(m.rows[0])):                                        # one cell of any column off by 1
        r = list(m.rows[11])
        r[c] = (r[c][0], r[c][1] + 1)
        bad.append(_mutate(m, rows=m.rows[:11] + [tuple(r)] + m.rows[12:]))
    r = list(m.rows[5])
    r[0] = ("int", r[0][1])                                                # the same value under another type
    bad.append(_mutate(m, rows=m.rows[:5] + [tuple(r)] + m.rows[6:]))
    for b in bad:
        with pytest.raises(AssertionError):
            goref.assert_same(b, m)
