#!/usr/bin/env python3
"""`| YIELD ... [WHERE ...]` over the C2 step's result (BASELINE.json configs[1]: RMAT scale 22, edge factor 16, 1000
seeds, GO 3 STEPS ... WHERE e.p0 < 50 YIELD e._dst AS d, e._rank AS r, e.p0 AS p0, e.p1 AS p1), two ways:

  device  the step device-resident (yield_only + compact), then ngx_go_yield: ngx_yield_result.device_ms
  host    what a caller had to do before ngx_go_yield: the step delivered as host_columnar arrays, then numpy over
          the delivered columns

for the sentences
  count      YIELD COUNT(*)
  sum_avg    YIELD SUM($-.p1), AVG($-.p0)
  keep_1pc   YIELD $-.d, $-.p1 WHERE $-.p1 % 100 == 0     keeps about 1 % of the rows
  keep_50pc  YIELD $-.d, $-.p1 WHERE $-.p1 % 2 == 0       keeps about 50 %

Like against like: either leg is timed until the answer is in hand as numpy arrays (the device's cells copied to the
host; the host's delivered columns reduced or masked), less the traversal's device time, which both run. Medians over
--steps runs (at least 10) after --warmup, each leg in a loop of its own per sentence. The two answers are compared
outside the timed regions.
One JSON line on stdout; per-kernel times (ngx_kernel_stats) with --kernels. bench.py is the flagship measurement;
this tool only adds the sentence to its step."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QUERY = "GO 3 STEPS FROM {S} OVER e WHERE e.p0 < 50 YIELD e._dst AS d, e._rank AS r, e.p0 AS p0, e.p1 AS p1"
NAMES = ["d", "r", "p0", "p1"]
D, R, P0, P1 = 0, 1, 2, 3
SENTENCES = {
    "count": "YIELD COUNT(*)",
    "sum_avg": "YIELD SUM($-.p1), AVG($-.p0)",
    "keep_1pc": "YIELD $-.d, $-.p1 WHERE $-.p1 % 100 == 0",
    "keep_50pc": "YIELD $-.d, $-.p1 WHERE $-.p1 % 2 == 0",
}
READS = {"count": [], "sum_avg": [P1, P0], "keep_1pc": [P1, D], "keep_50pc": [P1, D]}    # the columns a sentence names


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--scale", type=int, default=22)
    p.add_argument("--ef", type=int, default=16)
    p.add_argument("--seeds", type=int, default=1000)
    p.add_argument("--parts", type=int, default=100)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--threads", type=int, default=16)
    p.add_argument("--kernels", action="store_true", help="per-kernel device times of the sentence (profiling on)")
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
    specs = {}
    for name, text in SENTENCES.items():
        y = ngql.parse_yield(text)
        specs[name] = engine.YieldSpec(NAMES, y.where.encode() if y.where is not None else None,
                                       [(c.fun, c.expr.encode()) for c in y.yields])
    out = {"scale": args.scale, "seeds": args.seeds, "steps": args.steps, "sentences": {}}
    col = None if args.no_host else [eng.prepare_go(datagen.RMAT_SPACE, s, on_device=False, columnar=True) for s in sentences]
    for name, spec in specs.items():
        ms, go_ms, path, rows, nbytes, answers = [], [], [], 0, 0, {}
        calls0 = eng.get_flag("yield_device")
        if args.kernels:
            eng.set_profiling(True)
            k0 = eng.kernel_stats()
        for i in range(n):
            t = time.perf_counter()
            r = eng.go(datagen.RMAT_SPACE, dev[i], yield_by=spec, rows=False)     # the cells in hand as one numpy array
            w = (time.perf_counter() - t) * 1e3
            if not r.ok:
                raise RuntimeError(r.error)
            answers[i] = r.yield_cells
            if i < args.warmup:
                continue
            ms.append(r.yield_device_ms)
            go_ms.append(r.go_device_ms)
            path.append(w - r.go_device_ms)                       # the call less the traversal both legs run
            rows += r.go_nrows
            nbytes += r.go_nrows * sum(r.dev_widths[1][c] for c in READS[name]) + r.nrows * 16 * len(spec.yields)
        res = {"yield_device_ms": round(statistics.median(ms), 3), "yield_device_ms_min": round(min(ms), 3),
               "go_device_ms": round(statistics.median(go_ms), 3),
               # kernels, the cells' copy to the host and the numpy view of them: the answer in hand
               "device_path_ms": round(statistics.median(path), 3),
               "rows_per_step": rows // args.steps, "rows_out": r.nrows,
               # one read of each column named and one write of each output cell: the least the sentence moves
               "bytes_per_step": nbytes // args.steps,
               "GBps_of_device_ms": round(nbytes / (sum(ms) * 1e-3) / 1e9, 1) if sum(ms) else 0.0,
               "on_device": eng.get_flag("yield_device") - calls0 == n}
        if args.kernels:
            res["kernel_ms_per_call"] = {k: round((v[1] - k0.get(k, (0, 0.0, 0))[1]) / n, 3)
                                         for k, v in eng.kernel_stats().items() if k.startswith("yield_")}
            eng.set_profiling(False)
        if col is not None:
            # the parent's way to the same answer in hand: the step's columns delivered, then numpy. Its own loop per
            # sentence, its own warm-up (the staging block grows in the first delivery), nothing but the answer timed
            host = []
            for i in range(n):
                t = time.perf_counter()
                r = eng.go(datagen.RMAT_SPACE, col[i], rows=False)
                d, p0, p1 = (r.dev_cols[c][0] for c in (D, P0, P1))
                if name == "count":
                    got = len(d)
                elif name == "sum_avg":
                    got = (int(p1.sum(dtype=np.int64)), float(int(p0.sum(dtype=np.int64))) / max(len(p0), 1))
                else:
                    keep = p1 % (100 if name == "keep_1pc" else 2) == 0
                    got = (d[keep], p1[keep])
                w = (time.perf_counter() - t) * 1e3
                if i >= args.warmup:
                    host.append(w - r.device_ms)
                cells = answers[i]                                # compared outside the timed region
                if name == "count":
                    same = cells.shape == (1, 1) and int(cells["v"][0, 0]) == got
                elif name == "sum_avg":
                    same = len(d) == 0 or (int(cells["v"][0, 0]) == got[0] and
                                           float(cells["v"][0, 1:2].view(np.float64)[0]) == got[1])
                else:                                             # two runs of a GO order their rows freely
                    a = np.lexsort((cells["v"][:, 1], cells["v"][:, 0]))
                    b = np.lexsort((got[1], got[0]))
                    same = len(a) == len(b) and np.array_equal(cells["v"][a, 0], got[0][b]) and \
                        np.array_equal(cells["v"][a, 1], got[1][b])
                if not same:
                    raise RuntimeError(f"sentence {name}, step {i}: the device's answer differs from numpy's")
            res["host_path_ms"] = round(statistics.median(host), 3)
            res["host_over_device"] = round(res["host_path_ms"] / res["device_path_ms"], 2)    # below 1: the device path loses
            out["answers_equal"] = True
        out["sentences"][name] = res
        log(name, json.dumps(res))
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
