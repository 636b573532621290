#!/usr/bin/env python3
"""GROUP BY over the C2 step's result (BASELINE.json configs[1]: RMAT scale 22, edge factor 16, 1000 seeds,
GO 3 STEPS ... WHERE e.p0 < 50 YIELD e._dst, e._rank, e.p0, e.p1), grouped two ways:

  device  the step device-resident (yield_only + compact), then ngx_go_group_by: ngx_group_result.device_ms,
          and the bytes of the columns the spec reads / that time
  host    what the code before ngx_go_group_by could do: the step delivered as host_columnar arrays, then a
          numpy group-by (sort + reduceat; int64 sums wrap as the device's do)

for the specs
  p0   GROUP BY $-.p0 YIELD $-.p0, COUNT(*), SUM($-.p1)      a few dozen groups (LDS aggregation)
  dst  GROUP BY $-.dst YIELD $-.dst, COUNT(*)                 one group per reached vertex (global atomics)

The two answers are compared group by group before anything is printed. One JSON line on stdout; per-kernel
times (ngx_kernel_stats) with --kernels. bench.py is the flagship measurement; this tool only adds the
grouping to its step."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QUERY = "GO 3 STEPS FROM {S} OVER e WHERE e.p0 < 50 YIELD e._dst, e._rank, e.p0, e.p1"
DST, RANK, P0, P1 = 0, 1, 2, 3                                    # the step's YIELD columns


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def numpy_group_by(np, key, value):
    """(keys, counts, int64 sums or None) of `value` grouped by `key`."""
    order = np.argsort(key, kind="stable")
    k = key[order]
    starts = np.flatnonzero(np.concatenate(([True], k[1:] != k[:-1]))) if len(k) else np.zeros(0, np.int64)
    counts = np.diff(np.concatenate((starts, [len(k)])))
    sums = np.add.reduceat(value[order], starts) if value is not None and len(k) else None
    return k[starts], counts, sums


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--scale", type=int, default=22)
    p.add_argument("--ef", type=int, default=16)
    p.add_argument("--seeds", type=int, default=1000)
    p.add_argument("--parts", type=int, default=100)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--threads", type=int, default=16)
    p.add_argument("--kernels", action="store_true", help="per-kernel device times of the grouping (profiling on)")
    p.add_argument("--no-host", action="store_true", help="skip the host_columnar + numpy leg")
    p.add_argument("--flag", action="append", default=[], metavar="NAME=VALUE")
    args = p.parse_args(argv)

    import numpy as np
    from nebula_amd import datagen, engine, ngql

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
    sentences = []
    for i in range(n):
        seeds = datagen.rmat_seeds(args.scale, args.seeds, args.ef, 42, 42 + i, threads=args.threads)
        sentences.append(ngql.parse_go(QUERY.replace("{S}", ", ".join(str(int(v)) for v in seeds))))
    dev = [eng.prepare_go(datagen.RMAT_SPACE, s, on_device=True, yield_only=True, compact=True) for s in sentences]
    specs = {
        "p0": (engine.GroupBySpec([P0], [("", P0, None), ("COUNT", -1, "*"), ("SUM", P1, None)]), (P0, P1)),
        "dst": (engine.GroupBySpec([DST], [("", DST, None), ("COUNT", -1, "*")]), (DST,)),
    }
    out = {"scale": args.scale, "seeds": args.seeds, "steps": args.steps, "specs": {}}
    answers = {}
    for name, (spec, reads) in specs.items():
        ms, go_ms, wall, rows, groups, nbytes = [], [], [], 0, 0, 0
        lds0 = eng.get_flag("group_by_lds")
        if args.kernels:
            eng.set_profiling(True)
            k0 = eng.kernel_stats()
        for i in range(n):
            t = time.perf_counter()
            r = eng.go(datagen.RMAT_SPACE, dev[i], group_by=spec)
            w = (time.perf_counter() - t) * 1e3
            if not r.ok:
                raise RuntimeError(r.error)
            if i < args.warmup:
                continue
            ms.append(r.group_device_ms)
            go_ms.append(r.go_device_ms)
            wall.append(w)
            rows += r.go_nrows
            groups += r.nrows
            nbytes += r.go_nrows * sum(r.dev_widths[1][c] for c in reads)
            answers[name, i] = r.rows
        res = {"group_device_ms": round(sum(ms) / len(ms), 3), "group_device_ms_min": round(min(ms), 3),
               "go_device_ms": round(sum(go_ms) / len(go_ms), 3), "wall_ms_go_group_and_python_decode": round(sum(wall) / len(wall), 3),
               "rows_per_step": rows // args.steps, "groups_per_step": groups // args.steps,
               "widths_read": [r.dev_widths[1][c] for c in reads],
               "column_bytes_per_step": nbytes // args.steps,
               "column_GBps": round(nbytes / (sum(ms) * 1e-3) / 1e9, 1),
               "rows_per_us": round(rows / (sum(ms) * 1e3), 1),
               "lds_path": eng.get_flag("group_by_lds") - lds0 == n}
        if args.kernels:
            # ms per launch group over warmup + steps (a COUNT_DISTINCT pass would count under group_assign too)
            res["kernel_ms_per_call"] = {k: round((v[1] - k0.get(k, (0, 0.0, 0))[1]) / n, 3)
                                         for k, v in eng.kernel_stats().items() if k.startswith("group_")}
            eng.set_profiling(False)
        out["specs"][name] = res
        log(name, json.dumps(res))

    if not args.no_host:
        col = [eng.prepare_go(datagen.RMAT_SPACE, s, on_device=False, columnar=True) for s in sentences]
        deliver, total = [], {"p0": [], "dst": []}
        for i in range(n):
            t = time.perf_counter()
            r = eng.go(datagen.RMAT_SPACE, col[i], rows=False, arrays=False)
            d = (time.perf_counter() - t) * 1e3
            if not r.ok:
                raise RuntimeError(r.error)
            if i >= args.warmup:
                deliver.append(d - r.device_ms)                   # the delivery leg: the call less the device step
            for name in specs:
                t = time.perf_counter()
                r = eng.go(datagen.RMAT_SPACE, col[i], rows=False)
                cols = [c[0] for c in r.dev_cols]
                if name == "p0":
                    k, cnt, sm = numpy_group_by(np, cols[P0], cols[P1])
                    got = {int(a): (int(b), int(c)) for a, b, c in zip(k, cnt, sm)}
                else:
                    k, cnt, _ = numpy_group_by(np, cols[DST], None)
                    got = {int(a): (int(b),) for a, b in zip(k, cnt)}
                w = (time.perf_counter() - t) * 1e3
                if i < args.warmup:
                    continue
                total[name].append(w - r.device_ms)
                want = {row[0][1]: tuple(c[1] for c in row[1:]) for row in answers[name, i]}
                if got != want:
                    raise RuntimeError(f"spec {name}, step {i}: the device's groups differ from numpy's "
                                       f"({len(want)} against {len(got)} groups)")
        out["host"] = {"delivery_ms": round(sum(deliver) / len(deliver), 3)}
        for name in specs:
            host_ms = sum(total[name]) / len(total[name])
            out["host"][name + "_delivery_plus_numpy_ms"] = round(host_ms, 3)
            out["specs"][name]["speedup_over_host"] = round(host_ms / out["specs"][name]["group_device_ms"], 1)
        out["answers_equal"] = True
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
