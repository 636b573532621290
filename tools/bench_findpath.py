#!/usr/bin/env python3
"""`FIND SHORTEST PATH FROM <1 source> TO <1 | 8 | 64 targets> OVER e UPTO 5 STEPS` on a C2-sized graph (BASELINE.json
configs[1]: RMAT scale 22, edge factor 16), run two ways on the same Engine:

  device  one ngx_find_path: levels, meets and sweeps in HBM, the path DAG's edges across, the paths enumerated from
          them (Engine.find_path; ngx_path_result.device_ms and its split by launch group with --kernels)
  host    what a caller had before the call existed: the FindPathExecutor restatement (nebula_amd/findpath.py) with
          one delivered GO per step, side and edge (pipeline.run(..., device_find_path=False))

The host leg extends every walk by every neighbour, as graphd does; on a C2-sized graph that does not end in
reasonable time, so it runs on a second, smaller graph when --host-scale is below --scale (0: not at all), and the
device leg is measured there too so the two walls compare on one graph. Where both legs run their sorted rows are
compared before anything is printed. One JSON line on stdout, and --out FILE writes it there too.

--kind ALL | NOLOOP measures `FIND ALL PATH` / `FIND NOLOOP PATH` instead (flag find_path_all is set; --upto, at most
8 for them). A sentence the device call refuses (path_rows_max, Engine.path_paths_max) is not an error then: the
target count's entry reports how many sentences were refused and the last refusal's text, and the figures are over
the sentences that were answered."""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TARGETS = (1, 8, 64)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def mean(v):
    return round(sum(v) / len(v), 3) if v else None


def load(eng, space, scale, ef, parts, threads):
    from nebula_amd import datagen
    t0 = time.time()
    csr = datagen.rmat_csr(scale, ef, 42, parts, with_in=True, threads=threads)
    eng.add_space(space, parts)
    for is_edge, sid, name, fields in datagen.rmat_schemas():
        eng.add_schema(space, is_edge, sid, name, fields)
    eng.load_csr(space, csr.vpart, csr.vid, csr.slots)
    eng.commit(space)
    csr.free()
    log(f"RMAT scale {scale} loaded into space {space} in {time.time() - t0:.1f}s")


def sentences(scale, ef, nt, n, threads, kind="SHORTEST", upto=5):
    """n seeded sentences: a source of the bench's seed generator, nt other vids as targets."""
    from nebula_amd import datagen
    out = []
    for i in range(n):
        seeds = [int(v) for v in datagen.rmat_seeds(scale, 4, ef, 42, 1000 + i, threads=threads)]
        rng = random.Random(7000 + 100 * nt + i)
        to = set()
        while len(to) < nt:
            v = rng.randrange(1 << scale)
            if v != seeds[0]:
                to.add(v)
        out.append("FIND %s PATH FROM %d TO %s OVER e UPTO %d STEPS" % (kind, seeds[0], ", ".join(map(str, sorted(to))), upto))
    return out


def measure(eng, space, scale, args, host):
    from nebula_amd import pipeline
    steps, warmup = (args.host_steps, args.host_warmup) if host else (args.steps, args.warmup)
    n = warmup + steps
    res = {}
    for nt in TARGETS:
        qs = sentences(scale, args.ef, nt, n, args.threads, args.kind, args.upto)
        refused, refusal = 0, ""
        dev_ms, dev_wall, host_wall, rows, edges, levels = [], [], [], 0, 0, 0
        kernel_ms = {}
        calls0 = eng.get_flag("find_path_device")
        for i, q in enumerate(qs):
            timed = i >= warmup
            if args.kernels and timed:
                eng.set_profiling(True)
                k0 = eng.kernel_stats()
                eng.find_path(space, q, rows=False)
                for k, v in eng.kernel_stats().items():
                    if k.startswith("path_"):
                        kernel_ms[k] = kernel_ms.get(k, 0.0) + v[1] - k0.get(k, (0, 0.0, 0))[1]
                eng.set_profiling(False)
            t = time.perf_counter()
            r = eng.find_path(space, q)
            dw = (time.perf_counter() - t) * 1e3
            if not r.ok:
                if args.kind == "SHORTEST" or not r.error.startswith("find path:"):
                    raise RuntimeError(r.error)
                refused, refusal = refused + 1, r.error
                continue
            if host:
                t = time.perf_counter()
                h = pipeline.run(eng, space, q, ["e"], find_path=True, device_find_path=False)
                hw = (time.perf_counter() - t) * 1e3
                if not h.ok:
                    raise RuntimeError(h.error)
                if sorted(h.rows) != sorted(r.rows):
                    raise RuntimeError(f"{nt} targets, step {i}: the device rows ({len(r.rows)}) differ from the host's ({len(h.rows)})")
            if not timed:
                continue
            dev_ms.append(r.device_ms)
            dev_wall.append(dw)
            if host:
                host_wall.append(hw)
            rows += r.nrows
            edges += r.go_nrows
            levels += r.hop_frontier[0]
        done = max(len(dev_ms), 1)
        one = {"steps": steps, "warmup": warmup, "device_ms": mean(dev_ms), "device_ms_min": round(min(dev_ms), 3) if dev_ms else None,
               "device_wall_ms": mean(dev_wall), "host_wall_ms": mean(host_wall), "paths_per_step": round(rows / done, 1),
               "dag_edges_per_step": round(edges / done, 1), "levels_per_step": round(levels / done, 1),
               "on_device": eng.get_flag("find_path_device") - calls0 >= n - refused}
        if refused:
            one["refused"], one["refusal"] = refused, refusal
        if host and host_wall:
            one["wall_ratio"] = round(mean(host_wall) / mean(dev_wall), 2)
        if args.kernels:
            one["kernel_ms_per_call"] = {k: round(v / steps, 3) for k, v in kernel_ms.items() if v > 0}
        res[str(nt)] = one
        log(scale, nt, json.dumps(one))
    return res


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--scale", type=int, default=22)
    p.add_argument("--host-scale", type=int, default=10, help="the graph both legs run on; 0: no host leg")
    p.add_argument("--host-steps", type=int, default=3, help="steps / warmup where the host leg runs: a host sentence takes seconds")
    p.add_argument("--host-warmup", type=int, default=1)
    p.add_argument("--ef", type=int, default=16)
    p.add_argument("--parts", type=int, default=100)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--threads", type=int, default=16)
    p.add_argument("--kernels", action="store_true", help="per-launch-group device times (profiling on, a run of its own)")
    p.add_argument("--kind", default="SHORTEST", choices=["SHORTEST", "ALL", "NOLOOP"])
    p.add_argument("--upto", type=int, default=5)
    p.add_argument("--out", default="")
    args = p.parse_args(argv)

    from nebula_amd import datagen, engine

    eng = engine.Engine(0)
    if args.kind != "SHORTEST":
        eng.set_flag("find_path_all", 1)
    out = {"scale": args.scale, "host_scale": args.host_scale, "ef": args.ef, "steps": args.steps, "warmup": args.warmup,
           "kind": args.kind, "upto": args.upto, "counters_collected": False}
    load(eng, datagen.RMAT_SPACE, args.scale, args.ef, args.parts, args.threads)
    if args.host_scale == args.scale:
        out["device_and_host"] = measure(eng, datagen.RMAT_SPACE, args.scale, args, True)
    else:
        out["device"] = measure(eng, datagen.RMAT_SPACE, args.scale, args, False)
        if args.host_scale:
            load(eng, datagen.RMAT_SPACE + 1, args.host_scale, args.ef, args.parts, args.threads)
            out["device_and_host"] = measure(eng, datagen.RMAT_SPACE + 1, args.host_scale, args, True)
    eng.close()
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
