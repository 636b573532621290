"""The multi-shard (world > 1) frontier exchange on shaped shards, against the GO model of tests/goref.py (shown equal
to the oracle on every case and query used here by tests/test_goshard_host.py).

The kernels under test: k_pack / k_merge (bitmaps), k_pack_list / k_merge_list (vid lists), k_mark_bits /
k_repack_bits (the all-gathered frontier bitmaps of a pulled hop), the dense final hop after a pulled hop, and the `$$`
owner fetch (k_pack_list with includeSelf, allToAllV). goref.SHARD_CASES places each graph so that a shard's row count,
`shardBase[q] & 63` and the marked rows meet one boundary of those kernels exactly; every vertex the hop under test can
reach has one out-edge whose p1 is its global row, so a lost mark costs a row and a spurious one adds a row.

One set of child processes (tests/goshard_worker.py, one per rank, all on device 0, host collective over gloo) per
world in {2, 3, 8} runs every case of that world; the tests are parametrised by case name and only read what the
children wrote. This process never opens the GPU. A child's non-zero exit or a time limit kills the world's other
children, fails every case of that world with the child's log tail and starts no further world; nothing is retried.

Per case: the shards' rows concatenated equal the model's (DISTINCT: their set), the shards' scanned edges sum to the
model's per hop, as do the shards' frontier sizes (a shard reports the frontier rows it expands itself: its own seeds,
then its own marked rows), every shard is ok with jit_failed == 0 and generated kernels, the shard's row count is the
generator's, the counters that prove the path moved by the expected amount on every rank, and hop_xchg equals
    bitmaps  the sum over the peers q of ceil(rows_q / 64) * 8
    lists    (W - 1) * W * 8 + 4 * (rows this rank sent)
    pull     ceil(largest shard's rows / 64) * 8 * (W - 1)
(restated in goref.xchg_*_bytes and checked on hand-computed values by the host test).
"""
import json
import os
import socket
import subprocess
import sys
import time

import pytest

from tests import goref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLDS = (2, 3, 8)
LAUNCH_TIMEOUT = 240
_state = {"dead": None, "out": {}}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _launch(tmp, world, names=None):
    names = goref.shard_cases(world) if names is None else names
    port = _free_port()
    env = dict(os.environ, PYTHONPATH=ROOT)
    logs = [open(os.path.join(tmp, f"w{world}r{r}.log"), "w+b") for r in range(world)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "goshard_worker.py"), str(r), str(world),
                               str(port), os.path.join(tmp, f"w{world}r{r}.json"), ",".join(names)], env=env,
                              stdout=logs[r], stderr=subprocess.STDOUT) for r in range(world)]
    t0 = time.time()
    bad = None
    left = set(range(world))
    while left and bad is None:
        for r in sorted(left):
            rc = procs[r].poll()
            if rc is None:
                continue
            left.discard(r)
            if rc != 0:
                bad = f"rank {r} of world {world} exited with {rc}"
                break
        if bad is None and left:
            if time.time() - t0 > LAUNCH_TIMEOUT:
                bad = f"world {world}: ranks {sorted(left)} still running after {LAUNCH_TIMEOUT} s"
            else:
                try:
                    procs[min(left)].wait(timeout=0.2)
                except subprocess.TimeoutExpired:
                    pass
    if bad is not None:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()
    tails = []
    for r, f in enumerate(logs):
        f.seek(0)
        tails.append(f"--- rank {r}\n" + f.read().decode(errors="replace")[-1500:])
        f.close()
    if bad is not None:
        return None, bad + "\n" + "\n".join(tails)
    print(f"world {world}: {len(names)} cases, shards done in {time.time() - t0:.1f} s\n{tails[0][-600:]}")
    return [json.load(open(os.path.join(tmp, f"w{world}r{r}.json"))) for r in range(world)], ""


@pytest.fixture(scope="module")
def shard_runs(tmp_path_factory):
    """{world: (per-rank output, error)}: the worlds launched one after the other, on first use."""
    tmp = str(tmp_path_factory.mktemp("goshards"))

    def get(world):
        if world not in _state["out"]:
            if _state["dead"] is not None:
                _state["out"][world] = (None, "not started: " + _state["dead"].splitlines()[0])
            else:
                _state["out"][world] = _launch(tmp, world)
                if _state["out"][world][0] is None:
                    _state["dead"] = _state["out"][world][1]
        return _state["out"][world]

    _state["dead"], _state["out"] = None, {}
    return get


def expected(name, k, rank):
    """(hop_xchg by hop index, counters) the driver's rules give query k of a case on `rank`."""
    case = goref.SHARD_CASES[name]
    sq = case.queries[k]
    g, _, sh = goref.shard_built(name)
    m = goref.shard_model(name, k)
    flags = goref.shard_flags(name, k)
    kinds, counters = sq.xchg, sq.counters
    if kinds is None:                                               # a pull case: from the model's edges per hop
        pulls = goref.pulled(m, sq.q, flags["pull_factor"], sh.vglobal)
        assert 2 in pulls, (name, k, pulls)                         # the hop under test
        kinds = {h: "pull" if h in pulls else "bitmap" for h in range(1, sq.q.n)}
        # the dense final hop follows a pulled hop: with its totals on the device its grid is static and every shard
        # with rows launches it; sized on the host, a shard whose final frontier is empty has no final hop at all
        final = [v for v in goref.hop_frontiers(g, goref.shard_seeds(name, sq), sq.q.n)[-1] if sh.where(v)[0] == rank]
        dense = sq.q.n - 1 in pulls and sh.counts[rank] > 0 and (flags["dense_world_dev"] == 1 or len(final) > 0)
        counters = {"pull_hops": len(pulls), "xchg_list_hops": 0, "dense_finals": 1 if dense else 0}
    xchg = {}
    for h, kind in kinds.items():
        if kind == "bitmap":
            xchg[h - 1] = goref.xchg_bitmap_bytes(sh.counts, rank)
        elif kind == "pull":
            xchg[h - 1] = goref.xchg_pull_bytes(sh.counts)
        else:
            xchg[h - 1] = goref.xchg_list_bytes(sh.world, goref.rows_sent(g, sh, goref.shard_seeds(name, sq), h, rank))
    return xchg, counters


def check_case(name, shards):
    """shards: per rank the worker's record of the case."""
    case = goref.SHARD_CASES[name]
    g, _, sh = goref.shard_built(name)
    assert [s["vertices"] for s in shards] == sh.counts, (name, "rows per shard as the engine knows them")
    for k, sq in enumerate(case.queries):
        what = (name, k, sq.q.form, sq.q.n, goref.shard_flags(name, k))
        res = [s["queries"][k] for s in shards]
        want = goref.shard_model(name, k)
        print(what, "rows", [len(r["rows"]) for r in res], "hop_edges", [r["hop_edges"] for r in res], "hop_frontier",
              [r["hop_frontier"] for r in res], "hop_xchg", [r["hop_xchg"] for r in res],
              {c: [r[c] for r in res] for c in goref.SHARD_COUNTERS})
        for rank, r in enumerate(res):
            assert r["ok"], (what, rank, r["error"])
            assert r["jit_failed"] == 0 and r["jit_note"] == "", (what, rank, r["jit_note"])
        goref.assert_merged([r["rows"] for r in res], [r["hop_edges"] for r in res], want,
                            goref.FORMS[sq.q.form].distinct, what)
        hops = len(want.hop_frontier)
        fsum = [sum(r["hop_frontier"][h] if h < len(r["hop_frontier"]) else 0 for r in res) for h in range(hops)]
        assert fsum == list(want.hop_frontier), (what, "hop_frontier", fsum, want.hop_frontier)
        for rank, r in enumerate(res):
            xchg, counters = expected(name, k, rank)
            for c, v in counters.items():
                assert r[c] == v, (what, "rank", rank, c, r[c], v)
            for h, b in xchg.items():
                assert h < len(r["hop_xchg"]) and r["hop_xchg"][h] == b, (what, "rank", rank, "hop_xchg", h, r["hop_xchg"], b)


CASES = [(w, n) for w in WORLDS for n in goref.shard_cases(w)]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world,name", CASES, ids=["w%d-%s" % c for c in CASES])
def test_shard_case(shard_runs, world, name):
    shards, err = shard_runs(world)
    assert shards is not None, err
    check_case(name, [s[name] for s in shards])


def test_every_world_has_its_shapes():
    """No case may be left out: every named shape of the registry is a test id above."""
    assert {n for _, n in CASES} == set(goref.SHARD_CASES) and all(goref.shard_cases(w) for w in WORLDS)
