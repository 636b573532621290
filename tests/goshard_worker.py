"""One shard of a world-N run of the shard cases of tests/goref.py (tests/test_gpu_go_shards.py starts N of these as
child processes, all on device 0, over the host collective `engine.dist_exchange()` on gloo).

A name of goref.PIPE_SHARD_CASES is run by pipe_case below. The rank receives case names, not arrays: it rebuilds each case's graph from goref by name, loads its own rows (through
ngx_load_csr, or as KV rows for the cases with tag rows: ngx_load_kv keeps the rows of its parts) into a fresh space of
one engine, and runs the case's queries with the case's flags. Per query it writes its rows as typed cells, the
per-hop statistics and the increase of the read-only counters; per case the row count the engine reports for the shard.

Usage: python tests/goshard_worker.py RANK WORLD PORT OUT.json CASE[,CASE...]
"""
import datetime
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pipe_case(e, goref, ngql, name, rank, world):
    """A pipe shard case (goref.PIPE_SHARD_CASES): every rank hands the engine the same input; the record adds the
    increase of pipe_walks."""
    case = goref.PIPE_SHARD_CASES[name]
    assert case.world == world, (name, case.world, world)
    g, inputs, sh = goref.pipe_shard_built(name)
    t0 = time.time()
    space = goref.new_space()
    e.add_space(space, sh.num_parts)
    for s in goref.SCHEMA:
        e.add_schema(space, s.is_edge, s.sid, s.name, s.fields)
    e.load_csr(space, *goref.csr_slots(g, rank, world, sh.num_parts))
    e.commit(space)
    for f, v in goref.BITMAP.items():
        e.set_flag(f, v)
    queries = []
    for q in case.queries:
        before = {c: e.get_flag(c) for c in ("pipe_walks", "jit_failed")}
        r = e.go(space, ngql.parse_go(goref.pipe_sentence(q.form, q.over, q.direction, q.m, q.n)), input=inputs[q.inp])
        queries.append({"ok": r.ok, "error": r.error, "rows": [[[c[0], c[1] if c[0] in ("str", "double") else int(c[1])] for c in row] for row in r.rows] if r.ok else [],
                        "hop_edges": [int(x) for x in r.hop_edges], "hop_frontier": [int(x) for x in r.hop_frontier],
                        "hop_xchg": [int(x) for x in r.hop_xchg], "jit_note": e.jit_note(),
                        **{c: e.get_flag(c) - b for c, b in before.items()}})
    print(f"[rank {rank}] {name}: {len(case.queries)} pipe queries in {(time.time() - t0) * 1e3:.0f} ms", file=sys.stderr, flush=True)
    return {"vertices": int(e.info(space).vertices), "queries": queries}


def main():
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    names = sys.argv[5].split(",")
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=120))
    from nebula_amd import engine, ngql
    from tests import goref

    res = {}
    t_all = time.time()
    e = engine.Engine(0, rank, world, exchange=engine.dist_exchange())
    e.set_flag("jit", 1)
    defaults = {k: e.get_flag(k) for k in ("pull_factor", "xchg_lists", "dst_props", "dense_world_dev")}
    for name in names:
        if name in goref.PIPE_SHARD_CASES:
            res[name] = pipe_case(e, goref, ngql, name, rank, world)
            continue
        case = goref.SHARD_CASES[name]
        assert case.world == world, (name, case.world, world)
        g, _, sh = goref.shard_built(name)
        t0 = time.time()
        space = goref.new_space()
        e.add_space(space, sh.num_parts)
        for s in goref.SCHEMA:
            e.add_schema(space, s.is_edge, s.sid, s.name, s.fields)
        if case.kv:
            e.load_kv(space, *goref.kv_batch(g, sh.num_parts).arrays())
        else:
            e.load_csr(space, *goref.csr_slots(g, rank, world, sh.num_parts))
        e.commit(space)
        queries = []
        for k, sq in enumerate(case.queries):
            for f, v in dict(defaults, **goref.shard_flags(name, k)).items():
                e.set_flag(f, v)
            before = {c: e.get_flag(c) for c in goref.SHARD_COUNTERS + ("jit_failed",)}
            r = e.go(space, ngql.parse_go(goref.shard_sentence(name, k)), pushdown=sq.q.pushdown)
            queries.append({"ok": r.ok, "error": r.error, "rows": [[[c[0], int(c[1])] for c in row] for row in r.rows] if r.ok else [],
                            "hop_edges": [int(x) for x in r.hop_edges], "hop_frontier": [int(x) for x in r.hop_frontier],
                            "hop_xchg": [int(x) for x in r.hop_xchg], "jit_note": e.jit_note(),
                            **{c: e.get_flag(c) - b for c, b in before.items()}})
        res[name] = {"vertices": int(e.info(space).vertices), "queries": queries}
        print(f"[rank {rank}] {name}: {len(case.queries)} queries in {(time.time() - t0) * 1e3:.0f} ms", file=sys.stderr, flush=True)
    e.close()
    print(f"[rank {rank}] all cases in {time.time() - t_all:.1f} s", file=sys.stderr, flush=True)
    with open(out, "w") as f:
        json.dump(res, f)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
