#!/usr/bin/env python3
"""GROUP BY ... | ORDER BY ... | LIMIT over the C2 step's result (BASELINE.json configs[1]: RMAT scale 22, edge
factor 16, 1000 seeds, GO 3 STEPS ... WHERE e.p0 < 50 YIELD e._dst AS dst, e._rank AS rank, e.p0 AS p0, e.p1 AS p1),
run two ways through nebula_amd.pipeline with order_limit=True:

  fused     one ngx_go_group_order_by after the step: grouping, the group rows as columns, radix select, emit of
            the window (ngx_order_result.device_ms and its split by launch group with --kernels)
  two_step  device_group_order=False, the path before the call existed: ngx_go_group_by, every group row across
            PCIe and into Python tuples, then ORDER BY / LIMIT on the host (nebula_amd/orderby.py)

for the plans
  dst_count_10  GROUP BY $-.dst YIELD $-.dst AS dst, COUNT(*) AS c | ORDER BY $-.c DESC | LIMIT 10
  p0_sum_5      GROUP BY $-.p0 YIELD $-.p0 AS k, SUM($-.p1) AS s | ORDER BY $-.s | LIMIT 5
  dst_limit_100 GROUP BY $-.dst YIELD $-.dst AS dst, COUNT(*) AS c | LIMIT 100

Both wall times hold the same traversal (go_device_ms) and the same parse of the text. The fused answer's factor
tuples are compared with the two-step answer's place by place (groups equal on every factor are free; LIMIT
alone: the row counts) before anything is printed. One JSON line on stdout. bench.py is the flagship measurement;
this tool only adds the ranked query to its step."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QUERY = "GO 3 STEPS FROM {S} OVER e WHERE e.p0 < 50 YIELD e._dst AS dst, e._rank AS rank, e.p0 AS p0, e.p1 AS p1"
PLANS = {
    "dst_count_10": ("GROUP BY $-.dst YIELD $-.dst AS dst, COUNT(*) AS c", "ORDER BY $-.c DESC", "LIMIT 10"),
    "p0_sum_5": ("GROUP BY $-.p0 YIELD $-.p0 AS k, SUM($-.p1) AS s", "ORDER BY $-.s", "LIMIT 5"),
    "dst_limit_100": ("GROUP BY $-.dst YIELD $-.dst AS dst, COUNT(*) AS c", None, "LIMIT 100"),
}


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def mean(v):
    return round(sum(v) / len(v), 3)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--scale", type=int, default=22)
    p.add_argument("--ef", type=int, default=16)
    p.add_argument("--seeds", type=int, default=1000)
    p.add_argument("--parts", type=int, default=100)
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--threads", type=int, default=16)
    p.add_argument("--kernels", action="store_true", help="per-launch-group device times of the fused call (profiling on)")
    p.add_argument("--no-two-step", action="store_true", help="skip the device_group_order=False leg")
    p.add_argument("--flag", action="append", default=[], metavar="NAME=VALUE")
    args = p.parse_args(argv)

    from nebula_amd import datagen, engine, pipeline

    t0 = time.time()
    csr = datagen.rmat_csr(args.scale, args.ef, 42, args.parts, with_in=True, threads=args.threads)
    eng = engine.Engine(0)
    for f in args.flag:
        name, _, val = f.partition("=")
        eng.set_flag(name, int(val))
    eng.add_space(datagen.RMAT_SPACE, args.parts)
    for is_edge, sid, name, fields in datagen.rmat_schemas():
        eng.add_schema(datagen.RMAT_SPACE, is_edge, sid, name, fields)
    eng.load_csr(datagen.RMAT_SPACE, csr.vpart, csr.vid, csr.slots)
    eng.commit(datagen.RMAT_SPACE)
    csr.free()
    log(f"RMAT scale {args.scale} loaded in {time.time() - t0:.1f}s")

    n = args.warmup + args.steps
    texts = []
    for i in range(n):
        seeds = datagen.rmat_seeds(args.scale, args.seeds, args.ef, 42, 42 + i, threads=args.threads)
        texts.append(QUERY.replace("{S}", ", ".join(str(int(v)) for v in seeds)))
    out = {"scale": args.scale, "seeds": args.seeds, "steps": args.steps, "plans": {}}
    for name, (gb, ob, lim) in PLANS.items():
        tail = " | ".join(t for t in (gb, ob, lim) if t)
        pipe = pipeline.Pipeline(eng, datagen.RMAT_SPACE, order_limit=True)
        dev_ms, sort_ms, go_ms, fused_wall, two_wall, rows, groups = [], [], [], [], [], 0, 0
        calls0 = eng.get_flag("group_order_device")
        kernel_ms = {}
        for i in range(n):
            s, g, gspec, ospec = pipe._group_order_spec(texts[i], gb, ob, lim)
            if args.kernels and i >= args.warmup:                 # around this call alone: the pipes below run unprofiled
                eng.set_profiling(True)
                k0 = eng.kernel_stats()
            r = eng.go(datagen.RMAT_SPACE, s, group_by=gspec, order_by=ospec, yield_only=True, compact=True)
            if not r.ok:
                raise RuntimeError(r.error)
            if args.kernels and i >= args.warmup:
                for k, v in eng.kernel_stats().items():
                    if k.startswith(("group_", "order_")):
                        kernel_ms[k] = kernel_ms.get(k, 0.0) + v[1] - k0.get(k, (0, 0.0, 0))[1]
                eng.set_profiling(False)
            t = time.perf_counter()
            fused = pipeline.run(eng, datagen.RMAT_SPACE, texts[i] + " | " + tail, order_limit=True)
            fw = (time.perf_counter() - t) * 1e3
            if not fused.ok:
                raise RuntimeError(fused.error)
            if not args.no_two_step:
                t = time.perf_counter()
                two = pipeline.run(eng, datagen.RMAT_SPACE, texts[i] + " | " + tail, order_limit=True, device_group_order=False)
                tw = (time.perf_counter() - t) * 1e3
                if not two.ok:
                    raise RuntimeError(two.error)
                fcols = [c for c, _ in ospec.factors]
                if [tuple(row[c] for c in fcols) for row in fused.rows] != [tuple(row[c] for c in fcols) for row in two.rows] \
                        or len(fused.rows) != len(two.rows) or fused.names != two.names:
                    raise RuntimeError(f"plan {name}, step {i}: the fused window differs from the two-step path's")
            if i < args.warmup:
                continue
            dev_ms.append(r.order_device_ms)
            sort_ms.append(r.order_host_sort_ms)
            go_ms.append(r.go_device_ms)
            fused_wall.append(fw)
            rows += r.go_nrows
            groups += r.ngroups
            if not args.no_two_step:
                two_wall.append(tw)
        res = {"fused_device_ms": mean(dev_ms), "fused_device_ms_min": round(min(dev_ms), 3), "host_sort_ms": mean(sort_ms),
               "go_device_ms": mean(go_ms), "rows_per_step": rows // args.steps, "groups_per_step": groups // args.steps,
               "rows_out": len(fused.rows), "fused_wall_ms": mean(fused_wall),
               "on_device": eng.get_flag("group_order_device") - calls0 == 2 * n}
        if two_wall:
            res["two_step_wall_ms"] = mean(two_wall)
            res["wall_speedup"] = round(res["two_step_wall_ms"] / res["fused_wall_ms"], 2)
        if args.kernels:
            res["kernel_ms_per_call"] = {k: round(v / args.steps, 3) for k, v in kernel_ms.items() if v > 0}
        out["plans"][name] = res
        log(name, json.dumps(res))
    out["answers_equal"] = not args.no_two_step
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
