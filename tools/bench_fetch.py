#!/usr/bin/env python3
"""`GO 2 STEPS FROM <seeds> OVER e YIELD e._dst AS id, e._src AS s, e._rank AS r | FETCH PROP ON vt $-.id YIELD vt.v0,
vt.name` and the edge form `... | FETCH PROP ON e $-.s->$-.id@$-.r YIELD e.p0, e.p1` on an RMAT graph with tag rows
(BASELINE.json configs[1] is scale 22, edge factor 16), run two ways on the same Engine:

  device  one ngx_go_fetch: the traversal's rows stay in HBM, the key lookup and the gather run there, the output
          cells cross (Engine.go_fetch; ngx_fetch_result.device_ms and its split by launch group with --kernels)
  host    what a caller had before the call existed: the GO delivered to Python, then the FetchVerticesExecutor /
          FetchEdgesExecutor restatement over Engine.get_neighbors (pipeline.run(..., device_fetch=False))

The host leg builds every row in Python, so it runs on a second, smaller graph when --host-scale is below --scale
(0: not at all), and the device leg is measured there too so the two walls compare on one graph. Where both legs run
their sorted rows are compared before anything is printed. Means of --steps sentences after --warmup. --seeds /
--host-seeds set the start vids per sentence, and with them the keys: the device leg times the call alone
(device_call_wall_ms: the cells arrive in host memory, no Python rows) beside the pipeline's wall, which builds them.
One JSON line on stdout, and --out FILE writes it there too."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GO = "GO 2 STEPS FROM %s OVER e YIELD e._dst AS id, e._src AS s, e._rank AS r"
KINDS = {"vertex": "FETCH PROP ON vt $-.id YIELD vt.v0, vt.name",
         "edge": "FETCH PROP ON e $-.s->$-.id@$-.r YIELD e.p0, e.p1"}


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def mean(v):
    return round(sum(v) / len(v), 3) if v else None


def load(eng, space, scale, ef, parts, threads):
    from nebula_amd import datagen
    t0 = time.time()
    rows = datagen.rmat(scale, ef, 42, parts, with_in=False, with_tag=True, threads=threads)
    eng.add_space(space, parts)
    for is_edge, sid, name, fields in datagen.rmat_schemas(True):
        eng.add_schema(space, is_edge, sid, name, fields)
    eng.load_kv(space, *rows.arrays())
    eng.commit(space)
    log(f"RMAT scale {scale} with tag rows loaded into space {space} in {time.time() - t0:.1f}s")


def catalog(parts):
    from nebula_amd import datagen, fetch
    cat = fetch.Catalog(parts)
    for is_edge, sid, name, fields in datagen.rmat_schemas(True):
        (cat.edges if is_edge else cat.tags)[name] = (sid, list(fields))
    return cat


def measure(eng, space, scale, args, host):
    from nebula_amd import datagen, fetch, ngql, pipeline
    steps, warmup = (args.host_steps, args.host_warmup) if host else (args.steps, args.warmup)
    nseeds = args.host_seeds if host else args.seeds
    n = warmup + steps
    cat = catalog(args.parts)
    res = {}
    for kind, ft in KINDS.items():
        seeds = [", ".join(str(int(v)) for v in datagen.rmat_seeds(scale, nseeds, args.ef, 42, 3000 + i, threads=args.threads))
                 for i in range(n)]
        dev_ms, dev_wall, call_wall, host_wall, rows, keys = [], [], [], [], 0, 0
        kernel_ms = {}
        calls0 = eng.get_flag("fetch_device")
        for i, seed in enumerate(seeds):
            timed = i >= warmup
            go = ngql.parse_go(GO % seed)
            names = go.column_names(["e"])
            probe = pipeline.Interim(names, [], [tuple(("int", 0) for _ in names)])
            spec = fetch.device_spec(cat, ngql.parse_fetch(ft), probe, {}, placeholder=True)
            if args.kernels and timed:
                eng.set_profiling(True)
                k0 = eng.kernel_stats()
                eng.go_fetch(space, go, spec, rows=False)
                for k, v in eng.kernel_stats().items():
                    if k.startswith("fetch_"):
                        kernel_ms[k] = kernel_ms.get(k, 0.0) + v[1] - k0.get(k, (0, 0.0, 0))[1]
                eng.set_profiling(False)
            t = time.perf_counter()
            r = eng.go_fetch(space, go, spec, rows=False)         # the call alone: no Python rows
            cw = (time.perf_counter() - t) * 1e3
            if not r.ok:
                raise RuntimeError(r.error)
            if not host and not args.pipeline_wall:
                if timed:
                    dev_ms.append(r.device_ms)
                    call_wall.append(cw)
                    rows += r.nrows
                    keys += r.go_nrows
                continue
            t = time.perf_counter()
            d = pipeline.run(eng, space, (GO % seed) + " | " + ft, ["e"], fetch=True, catalog=cat)
            dw = (time.perf_counter() - t) * 1e3
            if not d.ok:
                raise RuntimeError(d.error)
            if host:
                t = time.perf_counter()
                h = pipeline.run(eng, space, (GO % seed) + " | " + ft, ["e"], fetch=True, catalog=cat, device_fetch=False)
                hw = (time.perf_counter() - t) * 1e3
                if not h.ok:
                    raise RuntimeError(h.error)
                if sorted(h.rows) != sorted(d.rows):
                    raise RuntimeError(f"{kind}, step {i}: the device rows ({len(d.rows)}) differ from the host's ({len(h.rows)})")
            if not timed:
                continue
            dev_ms.append(r.device_ms)
            dev_wall.append(dw)
            call_wall.append(cw)
            if host:
                host_wall.append(hw)
            rows += r.nrows
            keys += r.go_nrows
        one = {"steps": steps, "warmup": warmup, "fetch_device_ms": mean(dev_ms), "fetch_device_ms_min": round(min(dev_ms), 3),
               "device_call_wall_ms": mean(call_wall), "device_wall_ms": mean(dev_wall), "seeds": nseeds, "host_wall_ms": mean(host_wall), "keys_per_step": round(keys / steps, 1),
               "rows_per_step": round(rows / steps, 1), "on_device": eng.get_flag("fetch_device") - calls0 >= n}
        if host:
            one["wall_ratio"] = round(mean(host_wall) / mean(dev_wall), 2)
        if args.kernels:
            one["kernel_ms_per_call"] = {k: round(v / steps, 4) for k, v in kernel_ms.items() if v > 0}
        res[kind] = one
        log(scale, kind, json.dumps(one))
    return res


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--scale", type=int, default=22)
    p.add_argument("--host-scale", type=int, default=14, help="the graph both legs run on; 0: no host leg")
    p.add_argument("--host-steps", type=int, default=10)
    p.add_argument("--host-warmup", type=int, default=3)
    p.add_argument("--seeds", type=int, default=1000, help="start vids per sentence of the device leg")
    p.add_argument("--host-seeds", type=int, default=300, help="... where the host leg runs")
    p.add_argument("--pipeline-wall", action="store_true", help="the device leg also times pipeline.run (Python rows)")
    p.add_argument("--ef", type=int, default=16)
    p.add_argument("--parts", type=int, default=100)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--threads", type=int, default=16)
    p.add_argument("--kernels", action="store_true", help="per-launch-group device times (profiling on, a call of its own)")
    p.add_argument("--out", default="")
    args = p.parse_args(argv)

    from nebula_amd import datagen, engine

    eng = engine.Engine(0)
    out = {"scale": args.scale, "host_scale": args.host_scale, "ef": args.ef, "steps": args.steps, "warmup": args.warmup,
           "seeds": args.seeds, "host_seeds": args.host_seeds,
           "counters_collected": False}
    load(eng, datagen.RMAT_SPACE, args.scale, args.ef, args.parts, args.threads)
    out["device"] = measure(eng, datagen.RMAT_SPACE, args.scale, args, False)
    if args.host_scale == args.scale:
        out["device_and_host"] = measure(eng, datagen.RMAT_SPACE, args.scale, args, True)
    elif args.host_scale:
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
