#!/usr/bin/env python3
"""INTERSECT / MINUS / UNION DISTINCT of two C2-sized traversals (BASELINE.json configs[1]: RMAT scale 22, edge
factor 16, GO 3 STEPS ... WHERE e.p0 < 50) from two disjoint 1000-seed sets, with YIELD e._dst, run two ways:

  device    one ngx_go_set: both traversals with their results left in HBM, the table build and probe, the emit of
            the output rows (ngx_set_result.device_ms and its split by launch group with --kernels)
  delivery  what a caller had before the call existed: two Engine.go deliveries (host-columnar results) and the set
            operator in numpy over the two dst arrays (np.unique / np.isin; multiplicities as SetExecutor's)

Both wall times hold the same two traversals. The device answer is compared with the numpy answer as sorted
arrays before anything is printed. One JSON line on stdout. bench.py is the flagship measurement; this tool only
adds the set sentence to its step."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QUERY = "GO 3 STEPS FROM {S} OVER e WHERE e.p0 < 50 YIELD e._dst AS dst"
OPS = ("INTERSECT", "MINUS", "UNION")


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def mean(v):
    return round(sum(v) / len(v), 3)


def numpy_set(op, a, b):
    """SetExecutor's answer over one int64 column, as a sorted array."""
    if op == "UNION":
        return np.union1d(a, b)
    if op == "MINUS":
        return np.sort(a[~np.isin(a, b)])
    va, ca = np.unique(a, return_counts=True)                     # INTERSECT: min(cL, cR) of every value
    vb, cb = np.unique(b, return_counts=True)
    common, ia, ib = np.intersect1d(va, vb, assume_unique=True, return_indices=True)
    return np.repeat(common, np.minimum(ca[ia], cb[ib]))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--scale", type=int, default=22)
    p.add_argument("--ef", type=int, default=16)
    p.add_argument("--seeds", type=int, default=1000)
    p.add_argument("--parts", type=int, default=100)
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--threads", type=int, default=16)
    p.add_argument("--kernels", action="store_true", help="per-launch-group device times of the set stage (profiling on)")
    p.add_argument("--flag", action="append", default=[], metavar="NAME=VALUE")
    args = p.parse_args(argv)

    from nebula_amd import datagen, engine

    t0 = time.time()
    csr = datagen.rmat_csr(args.scale, args.ef, 42, args.parts, with_in=True, threads=args.threads)
    eng = engine.Engine(0)
    eng.set_flag("set_rows_max", 1 << 28)                         # UNION DISTINCT of two C2 results is millions of rows
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
    pairs = []
    for i in range(n):
        both = datagen.rmat_seeds(args.scale, 2 * args.seeds, args.ef, 42, 42 + i, threads=args.threads)
        both = np.unique(np.asarray(both, dtype=np.int64))
        half = len(both) // 2
        pairs.append([QUERY.replace("{S}", ", ".join(str(int(v)) for v in part)) for part in (both[:half], both[half:2 * half])])
    out = {"scale": args.scale, "seeds": args.seeds, "steps": args.steps, "ops": {}}
    for op in OPS:
        dev_ms, dev_wall, del_wall, del_go, del_np, rows_in, rows_out = [], [], [], [], [], 0, 0
        kernel_ms = {}
        calls0 = eng.get_flag("set_op_device")
        for i in range(n):
            left, right = pairs[i]
            timed = i >= args.warmup
            if args.kernels and timed:
                eng.set_profiling(True)
                k0 = eng.kernel_stats()
                eng.go_set(datagen.RMAT_SPACE, left, right, op, rows=False)
                for k, v in eng.kernel_stats().items():
                    if k.startswith("set_"):
                        kernel_ms[k] = kernel_ms.get(k, 0.0) + v[1] - k0.get(k, (0, 0.0, 0))[1]
                eng.set_profiling(False)
            t = time.perf_counter()
            r = eng.go_set(datagen.RMAT_SPACE, left, right, op, rows=False)     # the output as an array, as the numpy leg's
            dw = (time.perf_counter() - t) * 1e3
            if not r.ok:
                raise RuntimeError(r.error)
            t = time.perf_counter()
            sides = []
            for text in (left, right):
                g = eng.go(datagen.RMAT_SPACE, text, columnar=True, rows=False, digest_fn=lambda ct, nr, x, ln, ty:
                           np.ctypeslib.as_array(ctypes.cast(x[0], ctypes.POINTER(ctypes.c_int64)), shape=(nr,)).copy()
                           if nr else np.zeros(0, np.int64))
                if not g.ok:
                    raise RuntimeError(g.error)
                sides.append(g.digests)
            tg = (time.perf_counter() - t) * 1e3
            want = numpy_set(op, sides[0], sides[1])
            tw = (time.perf_counter() - t) * 1e3
            got = np.sort(r.digests[:, 0])
            if not np.array_equal(got, want):
                raise RuntimeError(f"{op}, step {i}: the device answer ({len(got)} rows) differs from numpy's ({len(want)})")
            if not timed:
                continue
            dev_ms.append(r.device_ms)
            dev_wall.append(dw)
            del_wall.append(tw)
            del_go.append(tg)
            del_np.append(tw - tg)
            rows_in += r.go_nrows
            rows_out += r.nrows
        res = {"set_device_ms": mean(dev_ms), "set_device_ms_min": round(min(dev_ms), 3), "device_wall_ms": mean(dev_wall),
               "delivery_wall_ms": mean(del_wall), "delivery_go_ms": mean(del_go), "delivery_numpy_ms": mean(del_np),
               "wall_ratio": round(mean(del_wall) / mean(dev_wall), 2), "rows_in_per_step": rows_in // args.steps,
               "rows_out_per_step": rows_out // args.steps, "on_device": eng.get_flag("set_op_device") - calls0 >= n}
        if args.kernels:
            res["kernel_ms_per_call"] = {k: round(v / args.steps, 3) for k, v in kernel_ms.items() if v > 0}
        out["ops"][op] = res
        log(op, json.dumps(res))
    out["answers_equal"] = True
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
