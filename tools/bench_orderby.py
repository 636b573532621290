#!/usr/bin/env python3
"""ORDER BY ... LIMIT over the C2 step's result (BASELINE.json configs[1]: RMAT scale 22, edge factor 16, 1000
seeds, GO 3 STEPS ... WHERE e.p0 < 50 YIELD e._dst, e._rank, e.p0, e.p1), cut two ways:

  device  the step device-resident (yield_only + compact), then ngx_go_order_by: ngx_order_result.device_ms
          (selection + emit) and host_sort_ms (the library's sort of the <= K winners)
  host    what a caller could do before ngx_go_order_by: the step delivered as host_columnar arrays (the
          delivery alone), then numpy.argpartition / lexsort over the delivered columns

for the plans
  p1_desc_10   ORDER BY $-.p1 DESC | LIMIT 10
  p0_dst_1000  ORDER BY $-.p0, $-.dst | LIMIT 1000      p0 has 50 values: every level ties heavily
  limit_100    LIMIT 100

The two answers' factor tuples are compared place by place before anything is printed (rows equal on every
factor are free). One JSON line on stdout; per-kernel times (ngx_kernel_stats) with --kernels. bench.py is the
flagship measurement; this tool only adds the cut to its step."""
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


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--scale", type=int, default=22)
    p.add_argument("--ef", type=int, default=16)
    p.add_argument("--seeds", type=int, default=1000)
    p.add_argument("--parts", type=int, default=100)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--threads", type=int, default=16)
    p.add_argument("--kernels", action="store_true", help="per-kernel device times of the cut (profiling on)")
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
    plans = {
        "p1_desc_10": engine.OrderBySpec([(P1, True)], 0, 10),
        "p0_dst_1000": engine.OrderBySpec([(P0, False), (DST, False)], 0, 1000),
        "limit_100": engine.OrderBySpec([], 0, 100),
    }
    out = {"scale": args.scale, "seeds": args.seeds, "steps": args.steps, "plans": {}}
    answers = {}
    for name, spec in plans.items():
        ms, sort_ms, go_ms, wall, rows, nbytes = [], [], [], [], 0, 0
        calls0 = eng.get_flag("order_by_device")
        if args.kernels:
            eng.set_profiling(True)
            k0 = eng.kernel_stats()
        for i in range(n):
            t = time.perf_counter()
            r = eng.go(datagen.RMAT_SPACE, dev[i], order_by=spec)
            w = (time.perf_counter() - t) * 1e3
            if not r.ok:
                raise RuntimeError(r.error)
            if i < args.warmup:
                continue
            ms.append(r.order_device_ms)
            sort_ms.append(r.order_host_sort_ms)
            go_ms.append(r.go_device_ms)
            wall.append(w)
            rows += r.go_nrows
            nbytes += r.go_nrows * sum(r.dev_widths[1][c] for c, _ in spec.factors)
            answers[name, i] = r.rows
        res = {"order_device_ms": round(sum(ms) / len(ms), 3), "order_device_ms_min": round(min(ms), 3),
               "host_sort_ms": round(sum(sort_ms) / len(sort_ms), 3),
               "go_device_ms": round(sum(go_ms) / len(go_ms), 3),
               "wall_ms_go_order_and_python_decode": round(sum(wall) / len(wall), 3),
               "rows_per_step": rows // args.steps, "rows_out": len(r.rows),
               "widths_read": [r.dev_widths[1][c] for c, _ in spec.factors],
               # one read of each factor column: the least any selection reads (the steps read more: DESIGN 7.5)
               "factor_column_bytes_per_step": nbytes // args.steps,
               "factor_column_GBps": round(nbytes / (sum(ms) * 1e-3) / 1e9, 1),
               "rows_per_us": round(rows / (sum(ms) * 1e3), 1),
               "on_device": eng.get_flag("order_by_device") - calls0 == n}
        if args.kernels:
            res["kernel_ms_per_call"] = {k: round((v[1] - k0.get(k, (0, 0.0, 0))[1]) / n, 3)
                                         for k, v in eng.kernel_stats().items() if k.startswith("order_")}
            eng.set_profiling(False)
        out["plans"][name] = res
        log(name, json.dumps(res))

    if not args.no_host:
        col = [eng.prepare_go(datagen.RMAT_SPACE, s, on_device=False, columnar=True) for s in sentences]
        deliver, total = [], {name: [] for name in plans}
        for i in range(n):
            t = time.perf_counter()
            r = eng.go(datagen.RMAT_SPACE, col[i], rows=False, arrays=False)
            d = (time.perf_counter() - t) * 1e3
            if not r.ok:
                raise RuntimeError(r.error)
            if i >= args.warmup:
                deliver.append(d - r.device_ms)                   # the delivery leg: the call less the device step
            for name, spec in plans.items():
                t = time.perf_counter()
                r = eng.go(datagen.RMAT_SPACE, col[i], rows=False)
                cols = [c[0] for c in r.dev_cols]
                k = spec.offset + spec.count
                if name == "p1_desc_10":
                    key = -cols[P1]
                    top = np.argpartition(key, k - 1)[:k] if len(key) > k else np.arange(len(key))
                    got = [(-int(v),) for v in np.sort(key[top])]
                elif name == "p0_dst_1000":
                    order = np.lexsort((cols[DST], cols[P0]))[:k]
                    got = [(int(a), int(b)) for a, b in zip(cols[P0][order], cols[DST][order])]
                else:
                    got = min(k, len(cols[DST]))
                w = (time.perf_counter() - t) * 1e3
                if i < args.warmup:
                    continue
                total[name].append(w - r.device_ms)
                rows_dev = answers[name, i]
                if name == "limit_100":
                    same = len(rows_dev) == got
                else:
                    same = [tuple(row[c][1] for c, _ in spec.factors) for row in rows_dev] == got
                if not same:
                    raise RuntimeError(f"plan {name}, step {i}: the device's window differs from numpy's")
        out["host"] = {"delivery_ms": round(sum(deliver) / len(deliver), 3)}
        for name in plans:
            host_ms = sum(total[name]) / len(total[name])
            out["host"][name + "_delivery_plus_numpy_ms"] = round(host_ms, 3)
            res = out["plans"][name]
            res["speedup_over_delivery"] = round(out["host"]["delivery_ms"] / (res["order_device_ms"] + res["host_sort_ms"]), 1)
            res["speedup_over_host"] = round(host_ms / (res["order_device_ms"] + res["host_sort_ms"]), 1)
        out["answers_equal"] = True
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
