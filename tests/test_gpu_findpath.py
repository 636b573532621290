"""FIND PATH through the Engine: the reference FindPathTest answers (tests/golden/findpath_cases.py) on the NBA
fixture, SHORTEST over FORWARD / REVERSELY on the device path (ngx_find_path; the stat find_path_device proves it
ran), every other sentence through the refusal ("find path: ...") and the host restatement over the Engine; and an
RMAT graph (scale 10) where the device path equals the host restatement over the oracle for 20 seeded draws of 1-4
sources and 1-64 targets, UPTO 4 and UPTO 5, forward and REVERSELY."""
import random

import pytest

from nebula_amd import engine, pipeline
from oracle import oracle
from tests import fixtures
from tests.golden.findpath_cases import CASES
from tests.test_findpath_host import check_golden, golden_text

pytestmark = pytest.mark.gpu

EDGES = ["serve", "like", "teammate"]
DEVICE = [c for c in CASES if c["kind"] == "SHORTEST" and c["direction"] in ("", "REVERSELY") and not c.get("error")]
FALLBACK = [c for c in CASES if c not in DEVICE and not c.get("error")]
ERRORS = [c for c in CASES if c.get("error")]


@pytest.fixture(scope="module")
def nba():
    ds = fixtures.nba()
    with engine.Engine() as e:
        ds.load_engine(e)
        yield ds, e


@pytest.mark.parametrize("case", DEVICE, ids=[f"path{c['line']}" for c in DEVICE])
def test_shortest_on_the_device(nba, case):
    ds, e = nba
    before, levels = e.get_flag("find_path_device"), e.get_flag("find_path_levels")
    p = pipeline.Pipeline(e, ds.space, EDGES, find_path=True)
    check_golden(case, p.run(golden_text(case["query"])))
    assert p.find_path_fallbacks == 0 and e.get_flag("find_path_device") == before + 1
    assert e.get_flag("find_path_levels") >= levels               # one-edge paths meet before any level is expanded
    off = pipeline.run(e, ds.space, golden_text(case["query"]), EDGES, find_path=True, device_find_path=False)
    check_golden(case, off)
    assert e.get_flag("find_path_device") == before + 1


@pytest.mark.parametrize("case", FALLBACK, ids=[f"path{c['line']}" for c in FALLBACK])
def test_the_rest_falls_back(nba, case):
    ds, e = nba
    before = e.get_flag("find_path_device")
    p = pipeline.Pipeline(e, ds.space, EDGES, find_path=True)
    check_golden(case, p.run(golden_text(case["query"])))
    assert p.find_path_fallbacks == 1 and p.find_path_refusal.startswith("find path:")
    assert ("BIDIRECT" in p.find_path_refusal) == (case["kind"] == "SHORTEST")
    assert e.get_flag("find_path_device") == before


@pytest.mark.parametrize("case", ERRORS, ids=[f"path{c['line']}" for c in ERRORS])
def test_reference_errors(nba, case):
    ds, e = nba
    check_golden(case, pipeline.run(e, ds.space, golden_text(case["query"]), EDGES, find_path=True))


def test_levels_stat_moves(nba):
    ds, e = nba
    levels, edges = e.get_flag("find_path_levels"), e.get_flag("find_path_edges")
    q = golden_text("FIND SHORTEST PATH FROM {P:Tiago Splitter} TO {P:LaMarcus Aldridge} OVER like UPTO 5 STEPS")
    r = e.find_path(ds.space, q)
    assert r.ok and r.nrows == 1 and r.go_nrows == 3
    assert e.get_flag("find_path_levels") == levels + 2 and e.get_flag("find_path_edges") == edges + 3


# ----------------------------------------------------------------------------- RMAT
SCALE = 10


@pytest.fixture(scope="module")
def rmat():
    ds = fixtures.RmatDataset(SCALE, ef=4, with_in=True)
    o = oracle.Oracle()
    o.set_flags(threads=8)
    ds.load_oracle(o)
    with engine.Engine() as e:
        ds.load_engine(e)
        yield ds, o, e
    o.close()


@pytest.mark.parametrize("draw", range(20))
def test_rmat_equals_the_host_restatement(rmat, draw):
    ds, o, e = rmat
    rng = random.Random(9000 + draw)
    ns, nt = rng.randint(1, 4), rng.randint(1, 64)
    vids = rng.sample(range(1 << SCALE), ns + nt)
    frm, to = ", ".join(map(str, vids[:ns])), ", ".join(map(str, vids[ns:]))
    for upto in (4, 5):
        for direction in ("", " REVERSELY"):
            q = "FIND SHORTEST PATH FROM %s TO %s OVER e%s UPTO %d STEPS" % (frm, to, direction, upto)
            before = e.get_flag("find_path_device")
            dev = pipeline.run(e, ds.space, q, ["e"], find_path=True)
            assert dev.ok and e.get_flag("find_path_device") == before + 1, dev.error
            ref = pipeline.run(o, ds.space, q, ["e"], find_path=True)
            assert ref.ok, ref.error
            assert sorted(r[0][1] for r in dev.rows) == sorted(r[0][1] for r in ref.rows), q
