"""bench.py's own contract on a small graph (RMAT scale 12; a child process per run, as the benchmark is
started: its torch initialises the GPU before the engine does): the plain run's result line, --steps,
--dump-outputs (float64 files within the size limit, the same from run to run) and --full (the moved
measurements, and the same outputs from the KV load as from the plain run's bulk load)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--scale", "12", "--seeds", "20", "--parts", "10",
         "--threads", "4"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("roofline", "kernels", "device_ms_per_step", "host_ms_per_step", "get_neighbors", "host_delivery",
             "path_roofline", "cpu_baseline")


def _run(extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + extra, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def _load(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    """One plain run: its result line and the directory of its outputs."""
    d = str(tmp_path_factory.mktemp("bench") / "plain")
    return _run(["--dump-outputs", d]), d


def test_plain_run_line_and_dump(plain, tmp_path):
    out, d1 = plain
    d2 = str(tmp_path / "again")
    for k in HEADLINE:
        assert k in out, k
    assert not [k for k in FULL_ONLY if k in out]
    assert out["steps"] == 3 and out["warmup"] == 1 and out["full"] is False
    assert out["unit"] == "edges/s" and out["higher_is_better"] is True and out["dtype"] == "int64"
    assert out["ms_per_step"] > 0 and out["value"] > 0
    a = _load(d1)
    assert {"step_rows.npy", "step_edges.npy", "last_summary.npy", "last_dst.npy", "last_rank.npy",
            "last_p0.npy"} <= set(a)
    assert "last_p1.npy" in a or {"last_p1_hi.npy", "last_p1_lo.npy"} <= set(a)
    assert all(v.dtype == np.float64 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    # --steps sets the timed steps; the line's per-step figures are those of the dumped steps
    assert a["step_rows.npy"].shape == (3,) and a["step_edges.npy"].shape == (3,)
    assert out["rows_per_step"] == int(a["step_rows.npy"].sum()) // 3
    assert out["edges_per_step"] == int(a["step_edges.npy"].sum()) // 3
    # value = edges / wall time; ms_per_step is that wall time per step, rounded to 1e-3 ms
    tol = 0.0006 / out["ms_per_step"]
    assert abs(out["value"] - a["step_edges.npy"].sum() / (3 * out["ms_per_step"] * 1e-3)) <= tol * out["value"]
    # the last step's columns: every row at this size, sorted, and the query's filter holds
    n = int(a["last_summary.npy"][0])
    assert n == int(a["step_rows.npy"][-1]) and n > 0 and int(a["last_summary.npy"][1]) == n
    assert a["last_dst.npy"].shape == (n,) and (np.diff(a["last_dst.npy"]) >= 0).all()
    assert (a["last_p0.npy"] < 50).all() and (a["last_p0.npy"] >= 0).all()
    assert int(a["last_summary.npy"][2]) == int(a["last_dst.npy"].sum()) & 0xffff
    # the same arguments again: the same inputs, the same outputs
    _run(["--dump-outputs", d2])
    b = _load(d2)
    assert set(a) == set(b) and all(np.array_equal(a[f], b[f]) for f in a)


def test_full_run_keeps_the_other_measurements(plain, tmp_path):
    d1, d2 = plain[1], str(tmp_path / "full")
    out = _run(["--full", "--cpu-budget", "0", "--dump-outputs", d2])
    for k in HEADLINE + FULL_ONLY:
        assert k in out, k
    assert out["full"] is True and out["steps"] == 3
    assert out["roofline"]["kernel"] in out["kernels"] and out["device_ms_per_step"] > 0
    assert out["get_neighbors"]["edges_returned"] > 0 and out["host_delivery"]["columnar_row_bytes"] > 0
    # KV rows through the exporter and the plain run's bulk load build the same shard: the same outputs
    a, b = _load(d1), _load(d2)
    assert set(a) == set(b) and all(np.array_equal(a[f], b[f]) for f in a)
