"""FIND SHORTEST PATH on the device (ngx_find_path, nebula_amd/csrc/findpath.hip) on hand-built graphs loaded through
ngx_load_csr, against the host restatement (nebula_amd/findpath.py) over the same Engine (device_find_path=False:
one delivered GO per step, side and edge).

Row r is vid r + 1, one part. Edge `e` is type 1, `f` type 2; every slot is loaded with its exact transpose. Each
shape is the smallest at which one piece of the kernels can go wrong: lengths exactly UPTO and one above it, for odd
and even UPTO; paths from the odd and from the even meet; edges that differ in rank or type only; a row whose edges
pass a wave (65) and a workgroup's lanes (1,100); a sweep whose one row emits 70,000 edges (the LDS buffer flushed
inside the edge loop) and the path_rows_max refusal; 64 targets and 65; a vertex at two distances from two targets
(what the per-target seen mask is for); two sources at different distances; an unreachable target; a vid without a
vertex; a vertex on both sides; poisoned scratch; a GO before and after.
"""
import pytest

from nebula_amd import engine, pipeline
from tests.pathref import load, refused

pytestmark = pytest.mark.gpu

EDGES = ["e", "f"]

@pytest.fixture(scope="module")
def eng():
    with engine.Engine() as e:
        yield e


def device(e, space, q):
    """The sentence on the device path; asserts through the stat that it ran there."""
    before = e.get_flag("find_path_device")
    out = pipeline.run(e, space, q, EDGES, find_path=True)
    assert out.ok, out.error
    assert e.get_flag("find_path_device") == before + 1
    return sorted(r[0][1] for r in out.rows)


def both(e, space, q):
    dev = device(e, space, q)
    host = pipeline.run(e, space, q, EDGES, find_path=True, device_find_path=False)
    assert host.ok, host.error
    assert dev == sorted(r[0][1] for r in host.rows)
    return dev


def chain_text(vids, edge="e", rank=0):
    return ("<%s,%d>" % (edge, rank)).join(str(v) for v in vids)


def test_chain_lengths_at_upto(eng):
    sp = load(eng, 7, [(i, i + 1, 1, 0) for i in range(6)])
    for n in (4, 5, 6):                                           # n edges found, n + 1 not, odd and even n
        to = "%d, %d" % (n + 1, n + 2) if n < 6 else "7"
        got = both(eng, sp, "FIND SHORTEST PATH FROM 1 TO %s OVER e UPTO %d STEPS" % (to, n))
        assert got == [chain_text(range(1, n + 2))]
    assert both(eng, sp, "FIND SHORTEST PATH FROM 1 TO 2, 3, 4, 5, 6, 7 OVER e UPTO 3 STEPS") == \
        [chain_text(range(1, k + 1)) for k in (2, 3, 4)]
    assert both(eng, sp, "FIND SHORTEST PATH FROM 1 TO 2 OVER e UPTO 1 STEPS") == ["1<e,0>2"]
    assert both(eng, sp, "FIND SHORTEST PATH FROM 7 TO 1 OVER e REVERSELY UPTO 6 STEPS") == [chain_text(range(7, 0, -1), "-e")]


def test_diamond_lattice_even_and_odd_meet(eng):
    # 5 diamonds in a row: joint j is row 3 j, its two middles 3 j + 1 and 3 j + 2; one more edge to a tail row
    edges = []
    for j in range(5):
        for mid in (3 * j + 1, 3 * j + 2):
            edges += [(3 * j, mid, 1, 0), (mid, 3 * j + 3, 1, 0)]
    edges.append((15, 16, 1, 0))
    sp = load(eng, 17, edges)
    even = both(eng, sp, "FIND SHORTEST PATH FROM 1 TO 16 OVER e UPTO 10 STEPS")      # 10 edges: the even meet at step 5
    assert len(even) == 32 and len(set(even)) == 32
    odd = both(eng, sp, "FIND SHORTEST PATH FROM 1 TO 17 OVER e UPTO 11 STEPS")       # 11 edges: the odd meet at step 6
    assert len(odd) == 32 and all(p.endswith("<e,0>17") for p in odd)
    assert both(eng, sp, "FIND SHORTEST PATH FROM 1 TO 17 OVER e UPTO 10 STEPS") == []
    assert len(both(eng, sp, "FIND SHORTEST PATH FROM 1 TO 16, 17, 10 OVER e UPTO 12 STEPS")) == 32 + 32 + 8


def test_ranks_and_types_are_distinct_paths(eng):
    edges = [(0, 1, 1, r) for r in (0, 3, 7)] + [(0, 1, 2, 0), (1, 2, 1, 5), (1, 2, 2, 1)]
    sp = load(eng, 3, edges)
    got = both(eng, sp, "FIND SHORTEST PATH FROM 1 TO 3 OVER e, f UPTO 4 STEPS")
    assert got == sorted("1<%s,%d>2<%s,%d>3" % (a, ra, b, rb) for a, ra in (("e", 0), ("e", 3), ("e", 7), ("f", 0))
                         for b, rb in (("e", 5), ("f", 1)))
    assert both(eng, sp, "FIND SHORTEST PATH FROM 1 TO 3 OVER * UPTO 4 STEPS") == got
    assert both(eng, sp, "FIND SHORTEST PATH FROM 1 TO 2 OVER e") == ["1<e,%d>2" % r for r in (0, 3, 7)]
    rev = both(eng, sp, "FIND SHORTEST PATH FROM 3 TO 1 OVER e REVERSELY UPTO 2 STEPS")
    assert rev == ["3<-e,5>2<-e,%d>1" % r for r in (0, 3, 7)]


@pytest.mark.parametrize("deg", [65, 1100])
def test_hub_past_a_wave_and_a_workgroup(eng, deg):
    # source -> hub -> deg middles -> target: the hub's edges pass a wave / a workgroup of lanes striding
    hub, first, target = 1, 2, 2 + deg
    edges = [(0, hub, 1, 0)] + [(hub, first + i, 1, 0) for i in range(deg)] + [(first + i, target, 1, 0) for i in range(deg)]
    sp = load(eng, target + 1, edges)
    got = both(eng, sp, "FIND SHORTEST PATH FROM 1 TO %d OVER e" % (target + 1))
    assert got == sorted("1<e,0>2<e,0>%d<e,0>%d" % (first + i + 1, target + 1) for i in range(deg))
    got = both(eng, sp, "FIND SHORTEST PATH FROM %d TO 1 OVER e REVERSELY UPTO 3 STEPS" % (target + 1))
    assert len(got) == deg


def test_wide_level_flushes_in_the_loop_and_the_cap(eng):
    n = 70000
    edges = [(0, 1 + i, 1, 0) for i in range(n)] + [(1 + i, n + 1, 1, 0) for i in range(n)]
    sp = load(eng, n + 2, edges)
    q = "FIND SHORTEST PATH FROM 1 TO %d OVER e UPTO 2 STEPS" % (n + 2)
    flushes, edges_before = eng.get_flag("find_path_loop_flushes"), eng.get_flag("find_path_edges")
    got = device(eng, sp, q)
    assert got == sorted("1<e,0>%d<e,0>%d" % (2 + i, n + 2) for i in range(n))
    assert eng.get_flag("find_path_edges") == edges_before + 2 * n
    assert eng.get_flag("find_path_loop_flushes") >= flushes + n // 1024       # row 1's 70,000 edges all leave one workgroup
    assert eng.get_flag("path_rows_max") == 1 << 20
    eng.set_flag("path_rows_max", 100000)
    try:
        before = eng.get_flag("find_path_device")
        r = eng.find_path(sp, q)
        assert not r.ok and r.code == engine.E_UNSUPPORTED and r.error == "find path: path edges above path_rows_max"
        assert eng.get_flag("find_path_device") == before
        eng.set_flag("path_rows_max", 2 * n)                      # exactly the edges: answered
        assert len(device(eng, sp, q)) == n
    finally:
        eng.set_flag("path_rows_max", 1 << 20)


def test_target_limit(eng):
    sp = load(eng, 66, [(0, 1 + i, 1, 0) for i in range(65)])
    t64 = ", ".join(str(2 + i) for i in range(64))
    assert both(eng, sp, "FIND SHORTEST PATH FROM 1 TO %s OVER e" % t64) == sorted("1<e,0>%d" % (2 + i) for i in range(64))
    assert len(refused(eng, sp, "FIND SHORTEST PATH FROM 1 TO %s, 66 OVER e" % t64, "more than 64 targets")) == 65


def test_one_vertex_at_two_distances(eng):
    # rows: 0 s, 1 u, 2 v, 3 x, 4 t1, 5 y, 6 t2. x is 1 edge from t1 and 2 from t2: it is in two levels of the to side,
    # and the 5-edge path to t2 meets at the edge v -> x with x in level 2 (an odd meet at step 3)
    sp = load(eng, 7, [(0, 1, 1, 0), (1, 2, 1, 0), (2, 3, 1, 0), (3, 4, 1, 0), (3, 5, 1, 0), (5, 6, 1, 0)])
    got = both(eng, sp, "FIND SHORTEST PATH FROM 1 TO 5, 7 OVER e")
    assert got == sorted([chain_text([1, 2, 3, 4, 5]), chain_text([1, 2, 3, 4, 6, 7])])
    got = both(eng, sp, "FIND SHORTEST PATH FROM 2 TO 5, 7 OVER e UPTO 4 STEPS")     # 3 and 4 edges: x meets at both levels
    assert got == sorted([chain_text([2, 3, 4, 5]), chain_text([2, 3, 4, 6, 7])])


def test_nearer_source_only(eng):
    # s1 -> a -> t and s2 -> b -> a: only s1's path; s3 -> c -> t ties with s1
    sp = load(eng, 7, [(0, 1, 1, 0), (1, 2, 1, 0), (3, 4, 1, 0), (4, 1, 1, 0), (5, 6, 1, 0), (6, 2, 1, 0)])
    assert both(eng, sp, "FIND SHORTEST PATH FROM 1, 4 TO 3 OVER e") == [chain_text([1, 2, 3])]
    assert both(eng, sp, "FIND SHORTEST PATH FROM 1, 4, 6 TO 3 OVER e") == sorted([chain_text([1, 2, 3]), chain_text([6, 7, 3])])
    assert both(eng, sp, "FIND SHORTEST PATH FROM 4 TO 3 OVER e") == [chain_text([4, 5, 2, 3])]


def test_unreachable_missing_and_overlap(eng):
    sp = load(eng, 5, [(0, 1, 1, 0), (1, 2, 1, 0), (3, 4, 1, 0)])
    assert both(eng, sp, "FIND SHORTEST PATH FROM 1 TO 5 OVER e") == []                          # another component
    assert both(eng, sp, "FIND SHORTEST PATH FROM 1 TO 3, 5 OVER e") == [chain_text([1, 2, 3])]
    assert both(eng, sp, "FIND SHORTEST PATH FROM 3 TO 1 OVER e") == []                          # against the edges
    assert both(eng, sp, "FIND SHORTEST PATH FROM 1 TO 999 OVER e") == []                        # no such vertex
    assert both(eng, sp, "FIND SHORTEST PATH FROM 999 TO 3 OVER e") == []
    assert both(eng, sp, "FIND SHORTEST PATH FROM 999, 2 TO 998, 3 OVER e") == ["2<e,0>3"]
    refused(eng, sp, "FIND SHORTEST PATH FROM 1, 2 TO 2, 3 OVER e", "a vertex on both sides")
    refused(eng, sp, "FIND SHORTEST PATH FROM 1, 1 TO 3 OVER e", "a vid listed twice")
    refused(eng, sp, "FIND ALL PATH FROM 1 TO 3 OVER e UPTO 3 STEPS", "ALL and NOLOOP")
    refused(eng, sp, "FIND NOLOOP PATH FROM 1 TO 3 OVER e UPTO 3 STEPS", "ALL and NOLOOP")
    refused(eng, sp, "FIND SHORTEST PATH FROM 1 TO 3 OVER e BIDIRECT", "BIDIRECT")
    piped = "GO FROM 1 OVER e YIELD e._src AS s, e._dst AS d | GO FROM $-.d OVER e YIELD $-.s AS s, e._dst AS d | " \
            "FIND SHORTEST PATH FROM $-.s TO $-.d OVER e"
    assert both(eng, sp, piped) == [chain_text([1, 2, 3])]


def test_poisoned_scratch_and_neighbouring_go():
    """A fresh engine whose every scratch allocation starts as 0xA5 bytes: each sentence twice, with a GO before,
    between and after whose device digest does not move."""
    with engine.Engine() as e:
        e.set_flag("poison_buffers", 1)
        try:
            edges = []
            for j in range(3):
                for mid in (3 * j + 1, 3 * j + 2):
                    edges += [(3 * j, mid, 1, 0), (mid, 3 * j + 3, 1, 0)]
            sp = load(e, 10, edges)
            go = "GO 2 STEPS FROM 1 OVER e YIELD e._dst AS d, e._rank AS r"
            d0 = e.go(sp, go, on_device=True, device_digest=True).device_digest
            assert d0[2] == 2
            for q, n in (("FIND SHORTEST PATH FROM 1 TO 10 OVER e UPTO 6 STEPS", 8), ("FIND SHORTEST PATH FROM 1 TO 7, 9 OVER e", 8),
                         ("FIND SHORTEST PATH FROM 10 TO 1, 4 OVER e REVERSELY UPTO 7 STEPS", 12)):
                for _ in range(2):
                    assert len(both(e, sp, q)) == n
                    assert e.go(sp, go, on_device=True, device_digest=True).device_digest == d0
        finally:
            e.set_flag("poison_buffers", 0)
