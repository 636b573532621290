#!/usr/bin/env python3
"""`LOOKUP ON vt WHERE vt.v0 ...` and `LOOKUP ON e WHERE e.p0 ...` on an RMAT graph with a tag row per vertex
(BASELINE.json configs[1] is scale 22, edge factor 16; v0 = vid % 1000, p0 = hash % 100), a range and an equality,
at selectivities of roughly 0, 1 %, 50 % and 100 %, through Engine.lookup (ngx_lookup): one streaming pass over the
stored columns, a scan of the chunk counts, the emit of the kept rows.

Per sentence, means of --steps calls after --warmup: the call's device ms (HIP events, plan upload to the last
cell), the device ms per launch group (lookup_keep / lookup_scan / lookup_emit: profiling on, in calls of their
own), the bytes the keep pass must read (ngx_lookup_result.keep_bytes: a STRING condition counts its two offsets
only, and a row rejected early reads less), the fraction of the HBM peak (--peak-tbs, 8 TB/s) and of the streaming
copy rate DESIGN 6 records (--copy-tbs, 6.29 TB/s) that the keep pass reaches, and the call's wall time with the
cells in host memory (no Python rows). One JSON line on stdout, and --out FILE writes it there too."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SENTENCES = [
    ("vertex", "range_0", "LOOKUP ON vt WHERE vt.v0 < 0"),
    ("vertex", "range_1pct", "LOOKUP ON vt WHERE vt.v0 < 10"),
    ("vertex", "range_50pct", "LOOKUP ON vt WHERE vt.v0 < 500"),
    ("vertex", "range_100pct", "LOOKUP ON vt WHERE vt.v0 >= 0"),
    ("vertex", "range_50pct_yield", "LOOKUP ON vt WHERE vt.v0 < 500 YIELD vt.v0, vt.name"),
    ("vertex", "equality", "LOOKUP ON vt WHERE vt.v0 == 7"),
    ("edge", "range_0", "LOOKUP ON e WHERE e.p0 < 0"),
    ("edge", "range_1pct", "LOOKUP ON e WHERE e.p0 < 1"),
    ("edge", "range_50pct", "LOOKUP ON e WHERE e.p0 < 50"),
    ("edge", "range_100pct", "LOOKUP ON e WHERE e.p0 >= 0"),
    ("edge", "range_50pct_yield", "LOOKUP ON e WHERE e.p0 < 50 YIELD e.p0, e.p1"),
    ("edge", "equality", "LOOKUP ON e WHERE e.p0 == 7"),
]


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def mean(v):
    return round(sum(v) / len(v), 4) if v else None


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--scale", type=int, default=22)
    p.add_argument("--ef", type=int, default=16)
    p.add_argument("--parts", type=int, default=100)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--threads", type=int, default=16)
    p.add_argument("--peak-tbs", type=float, default=8.0)
    p.add_argument("--copy-tbs", type=float, default=6.29)
    p.add_argument("--rows-max", type=int, default=1 << 28, help="flag lookup_rows_max for the run")
    p.add_argument("--out", default="")
    args = p.parse_args(argv)

    from nebula_amd import datagen, engine, lookup, ngql

    eng = engine.Engine(0)
    space = datagen.RMAT_SPACE
    t0 = time.time()
    rows = datagen.rmat(args.scale, args.ef, 42, args.parts, with_in=False, with_tag=True, threads=args.threads)
    eng.add_space(space, args.parts)
    for is_edge, sid, name, fields in datagen.rmat_schemas(True):
        eng.add_schema(space, is_edge, sid, name, fields)
    eng.load_kv(space, *rows.arrays())
    eng.commit(space)
    del rows
    log(f"RMAT scale {args.scale} with tag rows loaded in {time.time() - t0:.1f}s")
    eng.set_flag("lookup_rows_max", args.rows_max)
    cat = eng.catalog(space)
    indexes = [lookup.Index(1, "vt_v0", datagen.RMAT_TAG_NAME, False, [datagen.RMAT_TAG_FIELDS[0]]),
               lookup.Index(2, "e_p0", datagen.RMAT_EDGE_NAME, True, [datagen.RMAT_EDGE_FIELDS[0]])]
    out = {"scale": args.scale, "ef": args.ef, "steps": args.steps, "warmup": args.warmup, "peak_tbs": args.peak_tbs,
           "copy_tbs": args.copy_tbs, "counters_collected": False, "sentences": []}
    for kind, name, text in SENTENCES:
        spec = lookup.device_spec(lookup.plan_of(cat, indexes, ngql.parse_lookup(text)))
        dev, wall, kernel_ms = [], [], {}
        r = None
        for i in range(args.warmup + args.steps):
            t = time.perf_counter()
            r = eng.lookup(space, spec, rows=False)               # the call alone: the cells in host memory, no Python rows
            w = (time.perf_counter() - t) * 1e3
            if not r.ok:
                raise RuntimeError(r.error)
            if i >= args.warmup:
                dev.append(r.device_ms)
                wall.append(w)
        eng.set_profiling(True)
        for i in range(args.steps):
            k0 = eng.kernel_stats()
            eng.lookup(space, spec, rows=False)
            for k, v in eng.kernel_stats().items():
                if k.startswith("lookup_"):
                    kernel_ms[k] = kernel_ms.get(k, 0.0) + v[1] - k0.get(k, (0, 0.0, 0))[1]
        eng.set_profiling(False)
        keep_ms = kernel_ms.get("lookup_keep", 0.0) / args.steps
        tbs = r.keep_bytes / (keep_ms * 1e-3) / 1e12 if keep_ms > 0 else None
        one = {"kind": kind, "name": name, "sentence": text, "scanned_rows": r.go_nrows, "rows": r.nrows,
               "selectivity": round(r.nrows / r.go_nrows, 4) if r.go_nrows else None, "device_ms": mean(dev),
               "kernel_ms_per_call": {k: round(v / args.steps, 4) for k, v in sorted(kernel_ms.items())},
               "keep_bytes": r.keep_bytes, "keep_tbs": round(tbs, 3) if tbs else None,
               "keep_frac_of_peak": round(tbs / args.peak_tbs, 3) if tbs else None,
               "keep_frac_of_copy": round(tbs / args.copy_tbs, 3) if tbs else None, "call_wall_ms": mean(wall)}
        out["sentences"].append(one)
        log(json.dumps(one))
    eng.close()
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
