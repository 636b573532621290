"""Multi-root pipe walks (`GO ... | GO FROM $-.id ...`, `$var = ...; GO FROM $var.id ...`) on shaped graphs and inputs,
against the per-root model `goref.pipe` (shown equal to the oracle on every case, input and form used here by
tests/test_pipe_shapes_host.py).

Under test: runPipe's batches of kRootBatch distinct vids, k_scatter_roots / k_expand_roots / k_gather_roots, the host's
way back from root sets to rows (a row repeated per input row of every root in its set; or, where WHERE / YIELD read
`$-.x`, the (frontier row, input row) entries that k_final_in and the generated kernels read through FinalArgs::fin),
the one-walk plan, and the fallback to a walk per vid / per input row under a storage mask. goref.PIPE_CASES names what
each graph pins. The inputs are pipeline.Interim objects handed to Engine.go(..., input=...).

Per case and query, with the generated kernels and with the interpreter: the rows equal the model's as sorted typed
cells (strings exactly, doubles by their bits), the pipe_walks counter moved by the plan's walks, and hop_edges /
hop_frontier equal the plan model's (goref.pipe_plan: the walks' statistics added up).
"""
import pytest

from nebula_amd import engine, kvfmt, ngql, pipeline
from tests import goref

pytestmark = pytest.mark.gpu


def run_case(name):
    case = goref.PIPE_CASES[name]
    g, inputs = goref.pipe_built(name)
    e = engine.Engine(0)
    try:
        if case.cap:
            e.set_flag("max_edge_returned_per_vertex", case.cap)
        space = goref.load_engine_csr(e, g)
        for k, q in enumerate(case.queries):
            want, walks = goref.pipe_case_model(name, k)
            s = ngql.parse_go(goref.pipe_case_sentence(name, k))
            for jit in (1, 0):
                what = (name, k, q.form, q.over, q.direction, q.m, q.n, q.inp, "jit", jit)
                e.set_flag("jit", jit)
                before = e.get_flag("pipe_walks")
                try:
                    got = e.go(space, s, input=inputs[q.inp])
                except engine.EngineError as x:
                    if x.code == engine.E_DEVICE:                 # a device error: nothing more is launched
                        pytest.exit("device error in %s: %s" % (what, x), returncode=3)
                    raise
                delta = e.get_flag("pipe_walks") - before
                print(what, "rows", len(got.rows), "walks", delta, "hop_edges", list(got.hop_edges), "hop_frontier",
                      list(got.hop_frontier))
                if jit:
                    assert e.jit_note() == "", (what, e.jit_note())
                assert delta == walks, (what, "pipe_walks", delta, walks)
                goref.assert_same(got, want, what)
    finally:
        e.close()


@pytest.mark.parametrize("name", sorted(goref.PIPE_CASES))
def test_pipe_case(name):
    run_case(name)


def test_empty_input_keeps_types():
    """An input of no rows: no walk, no row, and the column types of the sentence (`$-.x` is UNKNOWN without data)."""
    g, _ = goref.pipe_built("roots1")
    empty = pipeline.Interim(list(goref.PIPE_COLS))
    with engine.Engine(0) as e:
        space = goref.load_engine_csr(e, g)
        for form, types in (("w", [0, 0, 0, kvfmt.VID, kvfmt.INT]), ("all", [kvfmt.VID, kvfmt.INT]), ("k_d", [0, kvfmt.VID])):
            for jit in (1, 0):
                e.set_flag("jit", jit)
                before = e.get_flag("pipe_walks")
                got = e.go(space, ngql.parse_go(goref.pipe_sentence(form, ["e"], n=2)), input=empty)
                assert got.ok and got.rows == [] and list(got.hop_edges) == [], (form, got.error)
                assert got.col_types == types, (form, got.col_types)
                assert e.get_flag("pipe_walks") == before
