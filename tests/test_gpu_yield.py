"""`GO | YIELD ... [WHERE ...]` through Pipeline(engine, yield_sentence=True): the device path (ngx_go_yield) against the
host restatement on the same backend (device_yield=False) and against the oracle backend, on the reference's known
answers (tests/golden/yield_cases.py) and on a small RMAT. Device cases must raise yield_device by one; refused ones
raise yield_fallbacks and still answer correctly."""
import math
import re

import pytest

from nebula_amd import datagen, engine, pipeline
from oracle import oracle
from tests import fixtures
from tests.golden import yield_cases

pytestmark = pytest.mark.gpu

EDGES = ["serve", "like", "teammate"]


@pytest.fixture(scope="module")
def nba():
    ds = fixtures.nba()
    o = oracle.Oracle()
    ds.load_oracle(o)
    e = engine.Engine(0)
    ds.load_engine(e)
    yield ds, o, e
    e.close()
    o.close()


@pytest.fixture(scope="module")
def rmat():
    ds = fixtures.RmatDataset(11, with_in=True, with_tag=True)
    o = oracle.Oracle()
    o.set_flags(threads=8)
    ds.load_oracle(o)
    e = engine.Engine(0)
    ds.load_engine(e)
    seeds = ", ".join(str(int(v)) for v in datagen.sample_vids(91, 1 << ds.scale, 6))
    yield ds, o, e, seeds
    e.close()
    o.close()


def norm(rows):
    out = []
    for r in fixtures.normalize_cells(rows):
        out.append(tuple("nan" if isinstance(v, float) and math.isnan(v) else v for v in r))
    return out


def three_ways(ds, o, e, text, edges=(), ordered=False):
    """(device Outcome, Pipeline) after checking the three answers against each other."""
    p = pipeline.Pipeline(e, ds.space, edges, yield_sentence=True)
    dev = p.run(text)
    host = pipeline.run(e, ds.space, text, edges, yield_sentence=True, device_yield=False)
    ref = pipeline.run(o, ds.space, text, edges, yield_sentence=True)
    assert dev.ok == host.ok == ref.ok, (dev.error, host.error, ref.error)
    if not dev.ok:
        assert dev.error == host.error == ref.error
        return dev, p
    assert dev.names == host.names == ref.names
    a, b, c = norm(dev.rows), norm(host.rows), norm(ref.rows)
    # a GO's rows have no fixed order from run to run: compared sorted (tests/test_gpu_yield_synth.py pins the order)
    assert sorted(a, key=repr) == sorted(b, key=repr) == sorted(c, key=repr)
    assert list(dev.col_types) == list(host.col_types)            # with no row kept too
    return dev, p


@pytest.mark.parametrize("case", yield_cases.CASES, ids=[c["name"] for c in yield_cases.CASES])
def test_golden(nba, case):
    ds, o, e = nba
    before = e.get_flag("yield_device")
    dev, p = three_ways(ds, o, e, fixtures.nba_query(case["query"]), EDGES)
    if "error" in case:
        assert not dev.ok and ("text" not in case or dev.error == case["text"])
        return
    assert "names" not in case or dev.names == case["names"]
    assert sorted(fixtures.normalize_cells(dev.rows)) == sorted(fixtures.nba_expected(case["rows"]))
    # a statement that starts with a GO piped into a YIELD runs that pair in one device call
    head_go = any(re.match(r"\s*(\$\w+\s*=\s*)?GO\b[^|]*\|\s*YIELD\b", st, re.I) for st in case["query"].split(";"))
    assert e.get_flag("yield_device") - before == (1 if head_go else 0)
    assert p.yield_fallbacks == 0


GO = "GO 2 STEPS FROM %s OVER e YIELD e._dst AS d, e.p0 AS w, e.p1 AS v, $$.vt.name AS s"
TAILS = [
    "YIELD COUNT(*)",
    "YIELD COUNT(*), SUM($-.w), MAX($-.v), MIN($-.w), BIT_XOR($-.w), AVG($-.w) WHERE $-.w % 3 == 0",
    "YIELD $-.d, $-.w * 2 + $-.v AS e WHERE $-.w > $-.v && $-.w % 7 != 1",
    "YIELD $-.* WHERE $-.v % 50 == 0",
    "YIELD SUM($-.w * 2), COUNT($-.d), 1 + 1 WHERE $-.w < 0 || $-.w >= 0",
    "YIELD $-.d AS id WHERE $-.w % 64 == 0 | GO FROM $-.id OVER e YIELD e._dst",
]


@pytest.mark.parametrize("tail", TAILS)
def test_rmat(rmat, tail):
    ds, o, e, seeds = rmat
    before = e.get_flag("yield_device")
    dev, p = three_ways(ds, o, e, (GO % seeds) + " | " + tail)
    assert dev.ok and dev.rows
    assert e.get_flag("yield_device") == before + 1 and p.yield_fallbacks == 0


@pytest.mark.parametrize("tail, reason", [
    ("YIELD COUNT_DISTINCT($-.w)", "yield: COUNT_DISTINCT"),
    ("YIELD STD($-.w - $-.w)", "yield: STD"),                    # zeros: exact in any row order
    ("YIELD (string)$-.w AS s WHERE $-.w % 100 == 0", "yield: an expression whose value is a string"),
    ("YIELD 100 / ($-.w % 10) AS q", "yield: an expression failed on a row"),
    ("YIELD MAX($-.w) WHERE $-.w != $-.w", "yield: no row kept"),
])
def test_refused_sentences_answer_from_the_host(rmat, tail, reason):
    ds, o, e, seeds = rmat
    before = e.get_flag("yield_device")
    dev, p = three_ways(ds, o, e, (GO % seeds) + " | " + tail)
    assert p.yield_fallbacks == 1 and p.yield_refusal.startswith(reason), p.yield_refusal
    assert e.get_flag("yield_device") == before


def test_default_arguments_keep_refusing(nba):
    ds, o, e = nba
    q = fixtures.nba_query("GO FROM {P:Tim Duncan} OVER like YIELD like._dst AS id | YIELD COUNT(*)")
    with pytest.raises(pipeline.PipelineError, match="only GO sentences run in this path"):
        pipeline.run(e, ds.space, q, EDGES)
