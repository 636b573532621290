"""GO's seed lookup, push / sparse / pull hops, next-frontier compaction and final hop on shaped graphs, against the
model of tests/goref.py (shown equal to the oracle on every case and query used here by tests/test_goref_host.py).

Every graph is built so that one boundary of one kernel is met exactly (the constants are mirrored in goref.py from
kargs.h, kernels.h and kernels.hip and checked against those files by the host test). Every case forces the path it is
about with the engine's flags (pull_factor, sparse_factor, dyn_hops, dense_final) and proves by the read-only counters
(pull_hops, sparse_hops, dense_finals; the seed hop by the launch counts of the profiled kernels) that the path ran.
The expected counter values restate the driver's rules (engine.cpp, ngx_go):
    pull    an intermediate hop of E > 0 edges is pulled iff pull_factor > 0, there are at most kPullMaxSlots OVER
            slots with exact mirrors, and E * 100 >= pull_factor * V;
    sparse  with sparse_factor -1 every other intermediate hop of E > 0 edges is a sparse hop;
    dense   see test_dense_final.
Every comparison is exact: typed cells, edges scanned and frontier per hop, counters. Rows are compared as sorted
multisets. An NGX_E_UNSUPPORTED raises out of Engine.go and fails the test.

CSR positions beyond 32 bits (the kernels' non-P32 instantiations) cannot be reached at these sizes and are not covered.
"""
import numpy as np
import pytest

from nebula_amd import engine, ngql
from oracle import oracle
from tests import goref

pytestmark = pytest.mark.gpu

BASE = {"pull_factor": 0, "sparse_factor": 0, "dyn_hops": 0}
COUNTERS = ("pull_hops", "sparse_hops", "dense_finals")


def open_engine(name, flags=None, kv=False):
    g, _ = goref.built(name)
    e = engine.Engine(0)
    try:
        for k, v in dict(BASE, **(flags or {})).items():
            e.set_flag(k, v)
        space = goref.load_engine_kv(e, g) if kv else goref.load_engine_csr(e, g)
    except Exception:
        e.close()
        raise
    return e, space


def run(e, space, name, q, jit=1):
    """One query: the engine's rows and statistics equal the model's. Returns the counters' increase."""
    s = ngql.parse_go(goref.case_sentence(name, q))
    e.set_flag("jit", jit)
    before = [e.get_flag(c) for c in COUNTERS]
    try:
        got = e.go(space, s, pushdown=q.pushdown)
    except engine.EngineError as x:
        if x.code == engine.E_DEVICE:                             # a device error: nothing more is launched
            pytest.exit("device error in %s %s: %s" % (name, q.form, x), returncode=3)
        raise
    delta = dict(zip(COUNTERS, (e.get_flag(c) - b for c, b in zip(COUNTERS, before))))
    if jit:
        assert e.jit_note() == "", (name, q.form, e.jit_note())   # the generated kernels ran, not the interpreter
    goref.assert_same(got, goref.case_model(name, q), (name, q.form, q.over, q.direction, q.m, q.n, "jit", jit))
    return delta


def pulled_hops(name, q, pull_factor):
    """The intermediate hops (1-based) the driver pulls (module docstring)."""
    g, _ = goref.built(name)
    m = goref.case_model(name, q)
    slots = len(q.over) * (2 if q.direction == goref.BIDIRECT else 1)
    if pull_factor <= 0 or slots > goref.K_PULL_MAX_SLOTS:
        return []
    return [h for h, E in enumerate(m.hop_edges, 1) if h < q.n and E > 0 and E * 100 >= pull_factor * len(g.vids)]


def pulls_expected(name, q, pull_factor):
    return len(pulled_hops(name, q, pull_factor))


def pushes_expected(name, q):
    m = goref.case_model(name, q)
    return sum(1 for h, E in enumerate(m.hop_edges, 1) if h < q.n and E > 0)


# ----------------------------------------------------------------------------- seed hop
@pytest.mark.parametrize("name", ["seed1", "seed3", "vids"])
def test_seed_hop(name):
    """Seeds x slots at 1, kSeedFuseMax - 1, kSeedFuseMax and past it (the fused seed kernel up to it, the lookup kernel
    past it: the profiled launch counts say which ran), every vertex as a seed, missing vids beside present ones, a seed
    twice, seeds of degree 0 in some and in all slots; vids of 1, 2, 4 and 8 bytes and negative ones, in all three
    directions. Generated kernels and the interpreter."""
    e, space = open_engine(name)
    try:
        e.set_profiling(True)
        for q in goref.CASES[name].queries:
            g, seeds = goref.built(name)
            seeds = q.seeds if q.seeds is not None else seeds
            n = len(set(seeds)) if goref.FORMS[q.form].distinct else len(seeds)
            slots = len(q.over) * (2 if q.direction == goref.BIDIRECT else 1)
            fused = n <= goref.K_SEED_FUSE_MAX and n * slots <= goref.K_SEED_FUSE_MAX
            for jit in (1, 0):
                k0 = e.kernel_stats()
                d = run(e, space, name, q, jit)
                k1 = e.kernel_stats()
                launched = {k: k1.get(k, (0,))[0] - k0.get(k, (0,))[0] for k in ("seed", "lookup")}
                assert launched == {"seed": 1 if fused else 0, "lookup": 0 if fused else 1}, (name, n, slots, launched)
                assert d["pull_hops"] == 0 and d["sparse_hops"] == 0
    finally:
        e.close()


# ----------------------------------------------------------------------------- chunk map (push hop, generic final hop)
CHUNK_CASES = ["chunk%d" % n for n in goref.CHUNK_SIZES] + ["chunk_supernode", "chunk_sparse_rows", "chunk_slots",
                                                            "chunk_empty_slot"]


@pytest.mark.parametrize("name", CHUNK_CASES)
def test_chunk_map(name):
    """A hop of exactly 1, kChunk - 1, kChunk, kChunk + 1 and 3 * kChunk + 5 edges, as the final hop (GO 2 STEPS) and as
    the pushed intermediate hop (GO 3 STEPS); a row of 5000 edges from mid-chunk over three chunks; more than 256 entries
    in a chunk and a run of empty rows across a chunk boundary; three interleaved slots; a slot empty for every row."""
    e, space = open_engine(name)
    try:
        for q in goref.CASES[name].queries:
            for jit in (1, 0):
                d = run(e, space, name, q, jit)
                assert d == {"pull_hops": 0, "sparse_hops": 0, "dense_finals": 0}, (name, q.form, d)
    finally:
        e.close()


def test_tag_props():
    """`$^.t.x` and `$$.t.x` where a third of the vertices lack the tag (KV-loaded: ngx_load_csr carries no tag rows)."""
    e, space = open_engine("tags", kv=True)
    try:
        for q in goref.CASES["tags"].queries:
            for jit in (1, 0):
                run(e, space, "tags", q, jit)
    finally:
        e.close()


# ----------------------------------------------------------------------------- sparse hop
SPARSE_CASES = ["sparse%d" % n for n in goref.SPARSE_SIZES] + ["sparse_one", "sparse_distinct", "sparse_repeats", "sparse_empty"]


@pytest.mark.parametrize("name", SPARSE_CASES)
def test_sparse_hop(name):
    """sparse_factor -1: every intermediate hop is a sparse hop (sparse_hops counts them). Hops of 255 .. 257 and
    kChunk - 1 .. kChunk + 1 edges; all edges to one destination; one destination in every slice of a chunk and in three
    chunks; an empty next frontier; all destinations distinct."""
    e, space = open_engine(name, {"sparse_factor": -1})
    try:
        for q in goref.CASES[name].queries:
            d = run(e, space, name, q)
            assert d["sparse_hops"] == pushes_expected(name, q) > 0 and d["pull_hops"] == 0, (name, q.form, d)
    finally:
        e.close()


def test_sparse_after_pull():
    """A pulled hop and then sparse hops on the same engine: the frontier bitmap the pull read is clean again."""
    name = "sparse_after_pull"
    e, space = open_engine(name, {"sparse_factor": -1, "pull_factor": 1})
    try:
        for rnd in range(2):
            for q in goref.CASES[name].queries:
                e.set_flag("pull_factor", 1)
                d = run(e, space, name, q)
                assert d["pull_hops"] == pulls_expected(name, q, 1) > 0, d
                e.set_flag("pull_factor", 0)
                d = run(e, space, name, q)
                assert d["pull_hops"] == 0 and d["sparse_hops"] == pushes_expected(name, q) > 0, d
    finally:
        e.close()


# ----------------------------------------------------------------------------- pull hop
PULL_CASES = ["pull_degrees", "pull_degrees_thin"] + ["pull_" + w for w in goref.PULL_WHICH] + \
             ["pull_v%d" % n for n in goref.PULL_V] + ["pull_4types", "pull_5types"]


@pytest.mark.parametrize("dyn", [0, 1])
@pytest.mark.parametrize("name", PULL_CASES)
def test_pull_hop(name, dyn):
    """pull_factor 1: hop 2 of GO 3 STEPS is pulled (pull_hops). In-degrees 0, 1, 15 .. 17, 1023 .. 1025 and 3000; the
    only in-neighbour in the frontier at each end of the head and of a segment; 63 .. 65 and 2047 .. 2049 rows in the
    pull's image; four OVER types are pulled, five (more than kPullMaxSlots) are not: pull_hops stays 0 and the hops
    push. dyn_hops 0 and 1.

    Which driver ran is read from the profiled launch counts. Host-driven (dyn_hops 0), a pulled hop launches `pull`
    alone and a pushed one `expand` alone. Device-driven (dyn_hops 1), every intermediate hop enqueues both and the
    device takes the one its E selects ("dyn: both expansions are enqueued", engine.cpp ngx_go), so `expand` is launched
    once per intermediate hop whatever is pulled; pull_hops then counts by the rule `e >= pullMinE` after the query."""
    e, space = open_engine(name, {"pull_factor": 1, "dyn_hops": dyn})
    try:
        e.set_profiling(True)
        if name[5:] in goref.PULL_WHICH:                          # the premise: one in-neighbour of T in the frontier
            g, seeds, T = goref.CASES[name].build()
            front = {w for _, w, _ in g.rows()[(seeds[0], 1)]}
            srcs = [w for _, w, _ in g.rows()[(T, -1)]]
            assert len(srcs) == 2100 and len([w for w in srcs if w in front]) == 1
        for q in goref.CASES[name].queries:
            k0 = e.kernel_stats()
            d = run(e, space, name, q)
            k1 = e.kernel_stats()
            launched = {k: k1.get(k, (0,))[0] - k0.get(k, (0,))[0] for k in ("pull", "expand")}
            hops = pulled_hops(name, q, 1)
            pullable = len(q.over) <= goref.K_PULL_MAX_SLOTS
            assert d["pull_hops"] == len(hops), (name, q.form, d, hops)
            assert q.n == 3 and pushes_expected(name, q) == 2     # both intermediate hops have edges
            if pullable:
                assert 2 in hops, (name, hops)                    # hop 2, the hop under test, is pulled
            else:
                assert hops == [] and name == "pull_5types"
            if dyn:
                assert launched == {"pull": 2 if pullable else 0, "expand": 2}, (name, launched)
            else:
                assert launched == {"pull": len(hops), "expand": 2 - len(hops)}, (name, launched)
    finally:
        e.close()


# ----------------------------------------------------------------------------- compaction
@pytest.mark.parametrize("kind", goref.COMPACT_REACHED)
@pytest.mark.parametrize("nv", goref.COMPACT_V)
def test_compaction(nv, kind):
    """kCompactTile - 1, kCompactTile, kCompactTile + 1 and 2 * kCompactTile + 1 rows; the compaction after hop 1 lists
    no row, every row, row 0, the last row, rows 1023 / 1024 / 4095 / 4096; at compact_lane_rows 4 / 8 / 16 and
    compact_wg 1024 / 256. The next hop reads the frontier list (pushed: pull_factor 0) and the bitmap (pulled:
    pull_factor 1; every pattern but "none", which leaves no next hop, gives hop 2 enough edges for it)."""
    name = "compact%d_%s" % (nv, kind)
    e, space = open_engine(name)
    try:
        q = goref.CASES[name].queries[0]
        for pf in (0, 1):
            e.set_flag("pull_factor", pf)
            for lane_rows in (4, 8, 16):
                for wg in (1024, 256):
                    e.set_flag("compact_lane_rows", lane_rows)
                    e.set_flag("compact_wg", wg)
                    d = run(e, space, name, q)
                    want = pulls_expected(name, q, pf)
                    assert d["pull_hops"] == want and d["sparse_hops"] == 0, (name, pf, lane_rows, wg, d, want)
        if kind != "none":                                        # hop 2 is pulled at pull_factor 1: it read the bitmap
            assert 2 in pulled_hops(name, q, 1) and pulled_hops(name, q, 0) == []
    finally:
        e.close()


# ----------------------------------------------------------------------------- storage forms in one query
def widened(r, ncol):
    """A fetched compact device result's YIELD columns, widened to int64, as sorted value tuples."""
    return sorted(zip(*[[int(v) for v in r.dev_cols[c][0]] for c in range(ncol)]))


@pytest.mark.parametrize("narrow", [1, 0])
@pytest.mark.parametrize("case", goref.STORAGE, ids=["_".join(c) for c in goref.STORAGE])
def test_storage_forms(case, narrow):
    """Two OVER types stored differently: int8 dst vids against a dst >= 2^31; rank forms constant 0 / 5 / -1, int8,
    int16, int32, int64 paired across the slots; parallel edges that differ in rank; an INT column holding exactly the
    extremes of int8, int8 + 1, int32, int32 + 1 and int64, read in WHERE and in YIELD; narrow_columns 1 and 0; host
    rows and a compact device result widened back, value for value."""
    name = "storage_%s_%s_%s" % case
    e, space = open_engine(name, {"narrow_columns": narrow})
    try:
        for q in goref.CASES[name].queries:
            for jit in ((1, 0) if q.form in ("multi", "bench") else (1,)):
                run(e, space, name, q, jit)
            e.set_flag("jit", 1)
            m = goref.case_model(name, q)
            s = ngql.parse_go(goref.case_sentence(name, q))
            r = e.go(space, s, pushdown=q.pushdown, on_device=True, fetch=True, yield_only=True, compact=True)
            ncol = len(goref.FORMS[q.form].yields)
            assert r.ok and r.nrows == len(m.rows), (name, q.form, r.error)
            assert list(r.hop_edges) == m.hop_edges and list(r.hop_frontier) == m.hop_frontier
            assert list(r.col_types) == [goref.KIND_TYPE[k] for k in goref.column_kinds(q.form)]
            assert widened(r, ncol) == sorted(tuple(c[1] for c in row) for row in m.rows), (name, q.form, r.dev_widths)
    finally:
        e.close()


# ----------------------------------------------------------------------------- dense final hop
@pytest.mark.parametrize("dense", [1, 0])
@pytest.mark.parametrize("case", goref.STORAGE[2:5], ids=["_".join(c) for c in goref.STORAGE[2:5]])
def test_dense_final(case, dense):
    """The mixed-width, non-zero-rank graphs with hop 1 pulled, dense_final 1 and 0. Which final kernel runs
    (engine.cpp, ngx_go, after the compaction of the hop before the last):

        const bool denseNext = (devNext || (c->world > 1 && !dyn && h + 1 == steps && !ownerDst)) && c->denseFinal &&
                               pull && !mask && !capped && !rw && hs.n == 1 && recordFrom == steps &&
                               hs.slotIdx[0] >= 0 && hs.slotIdx[0] < static_cast<int32_t>(d.chunkRow.size());

    so with one OVER type (hs.n == 1) after a pulled hop the dense final hop runs (dense_finals + 1) when the flag is
    set, and with two OVER types, or the flag off, the generic one does (dense_finals unchanged)."""
    name = "storage_%s_%s_%s" % case
    e, space = open_engine(name, {"pull_factor": 1, "dense_final": dense})
    try:
        for q in goref.CASES[name].queries:
            if "e" not in q.over:                                 # the hub's edges are of type e: OVER f has no hop 1
                continue
            d = run(e, space, name, q)
            assert d["pull_hops"] == pulls_expected(name, q, 1) == 1, (name, q.form, d)
            assert d["dense_finals"] == (1 if dense and len(q.over) == 1 else 0), (name, q.form, q.over, d)
    finally:
        e.close()


# ----------------------------------------------------------------------------- row reservation
@pytest.mark.parametrize("rows", goref.RESV_ROWS)
def test_row_reservation(rows):
    """A final hop that returns exactly 2^kResvShift - 1, 2^kResvShift, 2^kResvShift + 1 and kResvGroups * 2^kResvShift + 1
    rows, from four supernodes, with resv_groups 8 and 1; and with a WHERE that keeps every second row, so that every
    block ends partly filled. Delivered on the device, compared by the digest of the expected columns (closed form,
    shown equal to the model and the oracle by the host test)."""
    vpart, vid, slots, cols, nv = goref.resv_arrays(rows)
    seeds = [nv]
    with engine.Engine(0) as e:
        space = goref.load_engine_csr(e, None, arrays=(vpart, vid, slots))
        for groups in (goref.K_RESV_GROUPS, 1):
            e.set_flag("resv_groups", groups)
            for k, where in enumerate(("", "WHERE e.p0 < 1 ")):
                sel = np.ones(rows, bool) if not where else cols[2] < 1
                want = oracle.row_digest([np.zeros(int(sel.sum()), np.int64)] + [c[sel] for c in cols])
                s = ngql.parse_go("GO 2 STEPS FROM %d OVER e %sYIELD e._dst, e._rank, e.p0, e.p1" % (seeds[0], where))
                prep = e.prepare_go(space, s, on_device=True, yield_only=True, compact=bool(k))
                r = e.go(space, prep, rows=False, device_digest=True)
                assert r.ok and e.jit_note() == "", (r.error, e.jit_note())
                assert list(r.hop_edges) == [4, rows] and list(r.hop_frontier) == [1, 4]
                assert r.nrows == int(sel.sum()) == (rows if not where else (rows + 1) // 2)
                assert tuple(r.device_digest) == tuple(want), (rows, groups, where)
