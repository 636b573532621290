"""Multi-root pipe walks at world > 1 on shaped shards, against the per-root model `goref.pipe` (shown equal to the
oracle on these graphs and inputs by tests/test_pipe_shapes_host.py).

Under test: exchangeRoots and k_merge_roots (every shard sends a peer the root sets of the peer's rows and ORs what it
receives into its own rows), the `E == 0` clearing of the next root sets before the exchange, and runPipe's account of
the exchanged bytes. goref.PIPE_SHARD_CASES places roots, hubs and paths so that the merge's stride differs from the
shard's rows (counts [5, 70]), a shard of no rows takes part ([3, 0, 66]), a row's root sets arrive from its own
shard and a peer, from two peers, and a shard scans edges on hop 1 and none on hop 2 of 3 STEPS.

The child-process scheme is that of tests/test_gpu_go_shards.py (tests/goshard_worker.py, one process per rank on
device 0, host collective over gloo), one set of children per world in {2, 3}; this process never opens the GPU and
nothing is retried. Per case and query (with and without `$-` read, 2 and 3 STEPS): every shard is ok on generated
kernels, the shards' rows concatenated equal the model's, their scanned edges and frontier rows sum to the plan
model's per hop, pipe_walks moved by the plan's walks on every rank, and on every rank and exchanging hop
    hop_xchg = walks x (sum over the peers q of ceil(rows_q / 64) * 8  +  sum over the peers q of rows_q * 8):
the frontier bitmaps (goref.xchg_bitmap_bytes) and a 64-bit root set per peer row (goref.xchg_roots_bytes).
"""
import pytest

from tests import goref
from tests.test_gpu_go_shards import _launch

pytestmark = pytest.mark.gpu

WORLDS = (2, 3)
_state = {"dead": None, "out": {}}


@pytest.fixture(scope="module")
def pipe_shard_runs(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("pipeshards"))

    def get(world):
        if world not in _state["out"]:
            if _state["dead"] is not None:
                _state["out"][world] = (None, "not started: " + _state["dead"].splitlines()[0])
            else:
                _state["out"][world] = _launch(tmp, world, goref.pipe_shard_cases(world))
                if _state["out"][world][0] is None:
                    _state["dead"] = _state["out"][world][1]
        return _state["out"][world]

    _state["dead"], _state["out"] = None, {}
    return get


def check_case(name, shards):
    case = goref.PIPE_SHARD_CASES[name]
    _, _, sh = goref.pipe_shard_built(name)
    assert [s["vertices"] for s in shards] == sh.counts, (name, "rows per shard as the engine knows them")
    for k, q in enumerate(case.queries):
        what = (name, k, q.form, q.n)
        res = [s["queries"][k] for s in shards]
        want, walks = goref.pipe_shard_model(name, k)
        print(what, "rows", [len(r["rows"]) for r in res], "hop_edges", [r["hop_edges"] for r in res], "hop_frontier",
              [r["hop_frontier"] for r in res], "hop_xchg", [r["hop_xchg"] for r in res], "walks", [r["pipe_walks"] for r in res])
        for rank, r in enumerate(res):
            assert r["ok"], (what, rank, r["error"])
            assert r["jit_failed"] == 0 and r["jit_note"] == "", (what, rank, r["jit_note"])
            assert r["pipe_walks"] == walks, (what, rank, "pipe_walks", r["pipe_walks"], walks)
        goref.assert_merged([r["rows"] for r in res], [r["hop_edges"] for r in res], want, False, what)
        hops = len(want.hop_frontier)
        assert hops == q.n                                         # every walk of these cases lives through all hops
        fsum = [sum(r["hop_frontier"][h] if h < len(r["hop_frontier"]) else 0 for r in res) for h in range(hops)]
        assert fsum == list(want.hop_frontier), (what, "hop_frontier", fsum, want.hop_frontier)
        for rank, r in enumerate(res):
            per_hop = walks * (goref.xchg_bitmap_bytes(sh.counts, rank) + goref.xchg_roots_bytes(sh.counts, rank))
            assert r["hop_xchg"][:q.n - 1] == [per_hop] * (q.n - 1), (what, "rank", rank, "hop_xchg", r["hop_xchg"], per_hop)


CASES = [(w, n) for w in WORLDS for n in goref.pipe_shard_cases(w)]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world,name", CASES, ids=["w%d-%s" % c for c in CASES])
def test_pipe_shard_case(pipe_shard_runs, world, name):
    shards, err = pipe_shard_runs(world)
    assert shards is not None, err
    check_case(name, [s[name] for s in shards])


def test_every_world_has_its_shapes():
    assert {n for _, n in CASES} == set(goref.PIPE_SHARD_CASES) and all(goref.pipe_shard_cases(w) for w in WORLDS)
