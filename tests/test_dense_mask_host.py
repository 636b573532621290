"""The frontier bits of the dense final hop (nebula_amd/csrc/dense_mask.h) on the CPU.

finalBodyDense (final_kernels.h) marks, per 2048-edge chunk, the edges whose row is in the frontier by
toggling the two ends of every frontier row's clipped edge range and taking a prefix XOR. The range and
prefix arithmetic is plain C++ shared with the kernel; tools/dense_mask_check.cpp runs it (ASan + UBSan
build, as tools/san does for the host code) against a per-edge loop, and this test checks the words it
prints once more against a loop of its own. The chunks' rows come from chunkRow exactly as the engine
computes it at load (row of every chunk's first edge, the last row for the end).
"""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CE = 2048
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    out = tmp_path_factory.mktemp("dense_mask") / "dense_mask_check"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", *SAN, "-I", os.path.join(ROOT, "nebula_amd", "csrc"),
           "-o", str(out), os.path.join(ROOT, "tools", "dense_mask_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(out)


def chunk_cases(degrees, marks, ep=1):
    """(base, cnt, lo, hi, ep, off[lo..hi+1], mark[lo..hi], want bits) of every chunk of the slot."""
    off = [0]
    for d in degrees:
        off.append(off[-1] + d)
    E, V = off[-1], len(degrees)
    nch = (E + CE - 1) // CE
    cr, r = [], 0
    for ch in range(nch):                       # engine.cpp: the row holding each chunk's first edge
        while r + 1 < len(off) and off[r + 1] <= ch * CE:
            r += 1
        cr.append(r)
    cr.append(V - 1)
    owner = []
    for i, d in enumerate(degrees):
        owner += [i] * d
    cases = []
    for ch in range(nch):
        base, cnt = ch * CE, min(CE, E - ch * CE)
        lo, hi = cr[ch], cr[ch + 1]
        want = [1 if p < cnt and marks[owner[base + p]] == ep else 0 for p in range(CE)]
        cases.append((base, cnt, lo, hi, ep, off[lo:hi + 2], marks[lo:hi + 1], want))
    return cases


def run_cases(checker, tmp_path, cases):
    text = []
    for base, cnt, lo, hi, ep, off, mk, _ in cases:
        text.append(f"{base} {cnt} {lo} {hi} {ep}\n" + " ".join(map(str, off)) + "\n" + " ".join(map(str, mk)) + "\n")
    path = tmp_path / "cases.txt"
    path.write_text("".join(text))
    r = subprocess.run([checker, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.strip().split("\n") if r.stdout.strip() else []
    assert len(lines) == len(cases)
    for line, case in zip(lines, cases):
        words = [int(w, 16) for w in line.split()]
        assert len(words) == CE // 64
        got = [(words[p >> 6] >> (p & 63)) & 1 for p in range(CE)]
        assert got == case[7], case[:5]


def slot(*groups):
    """degrees and marks from (count, degree, mark pattern) groups; the pattern repeats over the group."""
    deg, mk = [], []
    for n, d, pat in groups:
        for i in range(n):
            deg.append(d(i) if callable(d) else d)
            mk.append(pat[i % len(pat)])
    return deg, mk


FIXED = {
    "empty_frontier": slot((300, 9, [0])),
    "every_row_active": slot((300, 9, [1])),
    "alternating": slot((700, 5, [1, 0])),
    "stale_epoch_marks": slot((400, 7, [2, 1, 0, 255])),
    "row_covers_whole_chunk": slot((1, CE, [1]), (1, CE, [0]), (1, CE, [1])),
    "row_spans_three_chunks_in": slot((100, 1, [1, 0]), (1, 5000, [1]), (100, 1, [0, 1])),
    "row_spans_three_chunks_out": slot((100, 1, [1]), (1, 5000, [0]), (100, 1, [1])),
    "row_ends_at_2048": slot((1, 48, [0]), (1, 2000, [1]), (1, 100, [0]), (1, 30, [1])),
    "row_ends_at_2047": slot((1, 47, [0]), (1, 2000, [1]), (1, 100, [0]), (1, 30, [1])),
    "row_ends_at_2047_next_active": slot((1, 47, [1]), (1, 2000, [1]), (1, 1, [1]), (1, 30, [0])),
    "row_starts_at_bit_0": slot((1, 10, [1]), (1, 2038, [0]), (1, 10, [1]), (1, 50, [0])),
    "degree_1_rows_fill_chunk": slot((CE, 1, [1, 0, 0]), (CE, 1, [1]), (CE, 1, [0, 1])),
    "zero_degree_runs_at_ends": slot((700, 0, [1]), (500, 3, [1, 0, 1]), (700, 0, [1, 0]), (300, 4, [0, 1]), (700, 0, [1])),
    "zero_degree_rows_at_chunk_boundary": slot((1, CE, [1]), (300, 0, [1]), (1, CE, [0]), (300, 0, [1]), (1, 5, [1])),
    "adjacent_active_cancel": slot((64, 32, [1]), (64, 32, [0]), (128, 16, [1])),
    "word_boundaries": slot((1, 63, [1]), (1, 1, [0]), (1, 64, [1]), (1, 65, [0]), (1, 63, [1]), (1, 128, [0]), (1, 64, [1])),
}
for _cnt in (1, 63, 64, 65, 2047):
    FIXED[f"cnt_{_cnt}"] = slot((1, _cnt, [1]))
    FIXED[f"cnt_{_cnt}_second_chunk"] = slot((2, 700, [1, 0]), (1, CE - 1400 + _cnt, [1]))
    FIXED[f"cnt_{_cnt}_small_rows"] = slot((_cnt, 1, [1, 0]))


@pytest.mark.parametrize("name", sorted(FIXED))
def test_fixed_rows(checker, tmp_path, name):
    deg, mk = FIXED[name]
    cases = chunk_cases(deg, mk)
    assert cases
    run_cases(checker, tmp_path, cases)


def test_cnt_cases_have_the_counts():
    for cnt in (1, 63, 64, 65, 2047):
        for name in (f"cnt_{cnt}", f"cnt_{cnt}_second_chunk", f"cnt_{cnt}_small_rows"):
            assert chunk_cases(*FIXED[name])[-1][1] == cnt, name


@pytest.mark.parametrize("seed", range(6))
def test_random_rows(checker, tmp_path, seed):
    rnd = random.Random(9100 + seed)
    deg, mk = [], []
    for _ in range(rnd.randrange(200, 1500)):
        kind = rnd.random()
        if kind < 0.25:
            d = 0
        elif kind < 0.9:
            d = rnd.randrange(1, 40)
        elif kind < 0.98:
            d = rnd.randrange(40, 700)
        else:
            d = rnd.randrange(1500, 7000)
        deg.append(d)
        mk.append(rnd.choice([1, 1, 0, 3]))
    if sum(deg) == 0:
        deg[0] = 1
    run_cases(checker, tmp_path, chunk_cases(deg, mk))
