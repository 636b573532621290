"""Known answers transcribed from the reference FindPathTest suite (src/graph/test/FindPathTest.cpp) on the NBA
fixture (tests/golden/nba.json). Data only: queries and expected paths, or an error class.

Placeholders as in gotest_cases.py: {P:<name>} / {T:<name>} is the player's / team's vid, in queries and in paths;
{NOBODY...} a vid nobody has. "line" is the line of the case's query in FindPathTest.cpp. A path is the suite's
rendering (TraverseTestBase.h buildPathString): vid<edge,rank>vid..., a reverse edge as -edge. Rows compare sorted
(verifyPath sorts). "error": "execution" (E_EXECUTION_ERROR). "kind" / "direction" say which sentence it is: the
device path takes SHORTEST over FORWARD or REVERSELY with literal or piped vids.

Left out: UseUUID (FindPathTest.cpp:984-1013; uuid() needs the storage UUID service) and the second EmptyInput case
(:972-981; it pipes through `YIELD ... WHERE`, a YieldExecutor over an input, outside this path).
"""


def _path(*steps):
    """_path("Tim Duncan", "like", "Tony Parker", ...) -> "{P:Tim Duncan}<like,0>{P:Tony Parker}..." (rank 0)."""
    out = []
    for i, s in enumerate(steps):
        out.append(("{T:%s}" if s in ("Spurs",) else "{P:%s}") % s if i % 2 == 0 else "<%s,0>" % s)
    return "".join(out)


def _q(kind, frm, to, over, upto, direction=""):
    vids = lambda names: ",".join(("{T:%s}" if n == "Spurs" else "{P:%s}") % n for n in names)
    return "FIND %s PATH FROM %s TO %s OVER %s%s UPTO %d STEPS" % (kind, vids(frm), vids(to), over,
                                                                  " " + direction if direction else "", upto)


TIM, TONY, MANU, AL, TIAGO = "Tim Duncan", "Tony Parker", "Manu Ginobili", "LaMarcus Aldridge", "Tiago Splitter"
RUDY, YAO, ONEAL = "Rudy Gay", "Yao Ming", "Shaquile O'Neal"
JAYLEN, STEVEN, KYLE, BAM, AG = "Jaylen Adams", "Steven Adams", "Kyle Alexander", "Bam Adebayo", "Grayson Allen"
AJ, JUSTIN, OG = "Jarrett Allen", "Justin Anderson", "OG Anunoby"
_GO_TIM = "GO FROM {P:Tim Duncan} OVER like yield like._src AS src, like._dst AS dst"
_TIM2 = [_path(TIM, "like", MANU), _path(TIM, "like", TONY)]

CASES = [
    # ---- SingleEdgeShortest
    dict(line=30, kind="SHORTEST", direction="", query=_q("SHORTEST", [TIM], [TONY], "like", 5), paths=[_path(TIM, "like", TONY)]),
    dict(line=43, kind="SHORTEST", direction="", query=_q("SHORTEST", [TIM], [TONY, MANU], "like", 5), paths=_TIM2),
    dict(line=58, kind="SHORTEST", direction="", query=_q("SHORTEST", [TIM], [AL], "like", 5),
         paths=[_path(TIM, "like", TONY, "like", AL)]),
    dict(line=71, kind="SHORTEST", direction="", query=_q("SHORTEST", [TIM], [TONY, MANU, AL], "like", 5),
         paths=_TIM2 + [_path(TIM, "like", TONY, "like", AL)]),
    dict(line=88, kind="SHORTEST", direction="", query=_q("SHORTEST", [TIAGO], [AL], "like", 5),
         paths=[_path(TIAGO, "like", TIM, "like", TONY, "like", AL)]),
    dict(line=103, kind="SHORTEST", direction="", query=_q("SHORTEST", [TIM, TIAGO], [TONY, MANU, AL], "like", 5),
         paths=_TIM2 + [_path(TIM, "like", TONY, "like", AL), _path(TIAGO, "like", MANU)]),
    dict(line=123, kind="SHORTEST", direction="", piped=True,
         query=_GO_TIM + " | FIND SHORTEST PATH FROM $-.src TO $-.dst OVER like UPTO 5 STEPS", paths=_TIM2),
    dict(line=137, kind="SHORTEST", direction="", piped=True,
         query="$var = " + _GO_TIM + ";FIND SHORTEST PATH FROM $var.src TO $var.dst OVER like UPTO 5 STEPS", paths=_TIM2),
    dict(line=151, kind="SHORTEST", direction="", piped=True,
         query="$var = GO FROM {P:Tim Duncan} OVER like yield like._src AS src;" + _GO_TIM +
               " | FIND SHORTEST PATH FROM $var.src TO $-.dst OVER like UPTO 5 STEPS", paths=_TIM2),
    # ---- SingleEdgeShortestReversely
    dict(line=169, kind="SHORTEST", direction="REVERSELY", query=_q("SHORTEST", [TONY], [TIM], "like", 5, "REVERSELY"),
         paths=[_path(TONY, "-like", TIM)]),
    dict(line=183, kind="SHORTEST", direction="REVERSELY", query=_q("SHORTEST", [TONY], [RUDY], "like", 5, "REVERSELY"),
         paths=[_path(TONY, "-like", AL, "-like", RUDY)]),
    dict(line=199, kind="SHORTEST", direction="REVERSELY", query=_q("SHORTEST", [TIM], [MANU, YAO], "like", 5, "REVERSELY"),
         paths=[_path(TIM, "-like", MANU), _path(TIM, "-like", ONEAL, "-like", YAO)]),
    # ---- SingleEdgeShortestBidirect
    dict(line=220, kind="SHORTEST", direction="BIDIRECT", query=_q("SHORTEST", [TONY], [TIM], "like", 5, "BIDIRECT"),
         paths=[_path(TONY, "-like", TIM), _path(TONY, "like", TIM)]),
    dict(line=236, kind="SHORTEST", direction="BIDIRECT", query=_q("SHORTEST", [TONY], [RUDY], "like", 5, "BIDIRECT"),
         paths=[_path(TONY, "-like", AL, "-like", RUDY), _path(TONY, "like", AL, "-like", RUDY)]),
    dict(line=254, kind="SHORTEST", direction="BIDIRECT", query=_q("SHORTEST", [TIAGO], [TONY, MANU, AL], "like", 5, "BIDIRECT"),
         paths=[_path(TIAGO, "like", MANU, "-like", TONY), _path(TIAGO, "like", TIM, "-like", TONY),
                _path(TIAGO, "like", TIM, "like", TONY), _path(TIAGO, "like", TIM, "-like", AL), _path(TIAGO, "like", MANU)]),
    # ---- SingleEdgeAll
    dict(line=287, kind="ALL", direction="", query=_q("ALL", [TIM], [TONY], "like", 3),
         paths=[_path(TIM, "like", TONY), _path(TIM, "like", TONY, "like", AL, "like", TONY),
                _path(TIM, "like", TONY, "like", TIM, "like", TONY), _path(TIM, "like", MANU, "like", TIM, "like", TONY)]),
    dict(line=306, kind="ALL", direction="", query=_q("ALL", [TIM], [TONY, MANU], "like", 3),
         paths=[_path(TIM, "like", TONY), _path(TIM, "like", TONY, "like", AL, "like", TONY),
                _path(TIM, "like", TONY, "like", TIM, "like", TONY), _path(TIM, "like", MANU, "like", TIM, "like", TONY),
                _path(TIM, "like", MANU), _path(TIM, "like", TONY, "like", MANU),
                _path(TIM, "like", TONY, "like", TIM, "like", MANU), _path(TIM, "like", MANU, "like", TIM, "like", MANU)]),
    dict(line=332, kind="ALL", direction="", query=_q("ALL", [TIM], [AL], "like", 3), paths=[_path(TIM, "like", TONY, "like", AL)]),
    dict(line=345, kind="ALL", direction="", query=_q("ALL", [TIAGO], [AL], "like", 3),
         paths=[_path(TIAGO, "like", TIM, "like", TONY, "like", AL)]),
    # ---- SingleEdgeAllReversely
    dict(line=362, kind="ALL", direction="REVERSELY", query=_q("ALL", [TONY], [TIM], "like", 3, "REVERSELY"),
         paths=[_path(TONY, "-like", TIM), _path(TONY, "-like", AL, "-like", TONY, "-like", TIM),
                _path(TONY, "-like", TIM, "-like", TONY, "-like", TIM), _path(TONY, "-like", TIM, "-like", MANU, "-like", TIM)]),
    dict(line=384, kind="ALL", direction="REVERSELY", query=_q("ALL", [TONY, MANU], [TIM], "like", 3, "REVERSELY"),
         paths=[_path(TONY, "-like", TIM), _path(MANU, "-like", TIM), _path(MANU, "-like", TONY, "-like", TIM),
                _path(TONY, "-like", AL, "-like", TONY, "-like", TIM), _path(TONY, "-like", TIM, "-like", TONY, "-like", TIM),
                _path(MANU, "-like", TIM, "-like", TONY, "-like", TIM), _path(TONY, "-like", TIM, "-like", MANU, "-like", TIM),
                _path(MANU, "-like", TIM, "-like", MANU, "-like", TIM)]),
    dict(line=414, kind="ALL", direction="REVERSELY", query=_q("ALL", [TIM], [AL], "like", 3, "REVERSELY"),
         paths=[_path(TIM, "-like", AL), _path(TIM, "-like", TONY, "-like", AL),
                _path(TIM, "-like", MANU, "-like", TIM, "-like", AL), _path(TIM, "-like", MANU, "-like", TONY, "-like", AL),
                _path(TIM, "-like", TONY, "-like", TIM, "-like", AL), _path(TIM, "-like", AL, "-like", TONY, "-like", AL)]),
    # ---- SingleEdgeAllBidirect
    dict(line=443, kind="ALL", direction="BIDIRECT", query=_q("ALL", [JAYLEN], [AG], "like", 6, "BIDIRECT"),
         paths=[_path(JAYLEN, "like", STEVEN, "like", KYLE, "like", AG),
                _path(JAYLEN, "like", BAM, "-like", STEVEN, "like", KYLE, "like", AG),
                _path(JAYLEN, "like", STEVEN, "like", BAM, "-like", JAYLEN, "like", STEVEN, "like", KYLE, "like", AG)]),
    dict(line=466, kind="ALL", direction="BIDIRECT", query=_q("ALL", [KYLE], [OG], "like", 6, "BIDIRECT"),
         paths=[_path(KYLE, "like", AG, "like", AJ, "-like", OG), _path(KYLE, "like", AG, "like", AJ, "like", JUSTIN, "like", OG),
                _path(KYLE, "like", AG, "like", AJ, "-like", OG, "-like", JUSTIN, "-like", AJ, "-like", OG)]),
    dict(line=489, kind="ALL", direction="BIDIRECT", query=_q("ALL", [AG], [AJ], "like", 4, "BIDIRECT"),
         paths=[_path(AG, "like", AJ), _path(AG, "like", AJ, "like", JUSTIN, "like", OG, "like", AJ),
                _path(AG, "like", AJ, "-like", OG, "-like", JUSTIN, "-like", AJ)]),
    # ---- SingleEdgeNoLoop
    dict(line=512, kind="NOLOOP", direction="", query=_q("NOLOOP", [TIM], [TONY], "like", 5), paths=[_path(TIM, "like", TONY)]),
    dict(line=526, kind="NOLOOP", direction="", query=_q("NOLOOP", [TIM], [TONY, MANU], "like", 5),
         paths=[_path(TIM, "like", TONY), _path(TIM, "like", MANU), _path(TIM, "like", TONY, "like", MANU)]),
    dict(line=545, kind="NOLOOP", direction="", query=_q("NOLOOP", [AL], [TIM], "like", 5),
         paths=[_path(AL, "like", TIM), _path(AL, "like", TONY, "like", TIM), _path(AL, "like", TONY, "like", MANU, "like", TIM)]),
    # ---- SingleEdgeNoLoopReversely
    dict(line=568, kind="NOLOOP", direction="REVERSELY", query=_q("NOLOOP", [TONY], [TIM], "like", 3, "REVERSELY"),
         paths=[_path(TONY, "-like", TIM)]),
    dict(line=582, kind="NOLOOP", direction="REVERSELY", query=_q("NOLOOP", [TONY, MANU], [TIM], "like", 3, "REVERSELY"),
         paths=[_path(TONY, "-like", TIM), _path(MANU, "-like", TIM), _path(MANU, "-like", TONY, "-like", TIM)]),
    dict(line=601, kind="NOLOOP", direction="REVERSELY", query=_q("NOLOOP", [TIM], [AL], "like", 5, "REVERSELY"),
         paths=[_path(TIM, "-like", AL), _path(TIM, "-like", TONY, "-like", AL),
                _path(TIM, "-like", MANU, "-like", TONY, "-like", AL)]),
    # ---- SingleEdgeNoLoopBidirect
    dict(line=624, kind="NOLOOP", direction="BIDIRECT", query=_q("NOLOOP", [JAYLEN], [AG], "like", 6, "BIDIRECT"),
         paths=[_path(JAYLEN, "like", STEVEN, "like", KYLE, "like", AG),
                _path(JAYLEN, "like", BAM, "-like", STEVEN, "like", KYLE, "like", AG)]),
    dict(line=643, kind="NOLOOP", direction="BIDIRECT", query=_q("NOLOOP", [KYLE], [OG], "like", 6, "BIDIRECT"),
         paths=[_path(KYLE, "like", AG, "like", AJ, "-like", OG), _path(KYLE, "like", AG, "like", AJ, "like", JUSTIN, "like", OG)]),
    dict(line=662, kind="NOLOOP", direction="BIDIRECT", query=_q("NOLOOP", [AG], [AJ], "like", 4, "BIDIRECT"),
         paths=[_path(AG, "like", AJ)]),
    # ---- MultiEdgesShortest
    dict(line=680, kind="SHORTEST", direction="", query=_q("SHORTEST", [TIM], [TONY], "like,serve", 5), paths=[_path(TIM, "like", TONY)]),
    dict(line=693, kind="SHORTEST", direction="", query=_q("SHORTEST", [TIM], [TONY, "Spurs"], "like,serve", 5),
         paths=[_path(TIM, "like", TONY), _path(TIM, "serve", "Spurs")]),
    dict(line=707, kind="SHORTEST", direction="", query=_q("SHORTEST", [TIM], [TONY, MANU, AL, "Spurs"], "like,serve", 5),
         paths=_TIM2 + [_path(TIM, "like", TONY, "like", AL), _path(TIM, "serve", "Spurs")]),
    dict(line=728, kind="SHORTEST", direction="", query=_q("SHORTEST", [TIAGO], [AL, "Spurs"], "like,serve", 5),
         paths=[_path(TIAGO, "like", TIM, "like", TONY, "like", AL), _path(TIAGO, "serve", "Spurs")]),
    dict(line=743, kind="SHORTEST", direction="", query=_q("SHORTEST", [TIM], [TONY], "*", 5),
         paths=[_path(TIM, "like", TONY), _path(TIM, "teammate", TONY)]),
    dict(line=757, kind="SHORTEST", direction="", query=_q("SHORTEST", [TIM], [TONY, "Spurs"], "*", 5),
         paths=[_path(TIM, "like", TONY), _path(TIM, "serve", "Spurs"), _path(TIM, "teammate", TONY)]),
    dict(line=772, kind="SHORTEST", direction="", query=_q("SHORTEST", [TIM], [TONY, MANU, AL, "Spurs"], "*", 5),
         paths=[_path(TIM, "like", TONY), _path(TIM, "like", MANU), _path(TIM, "serve", "Spurs"), _path(TIM, "teammate", AL),
                _path(TIM, "teammate", TONY), _path(TIM, "teammate", MANU)]),
    dict(line=795, kind="SHORTEST", direction="", query=_q("SHORTEST", [TIAGO], [AL, "Spurs"], "*", 5),
         paths=[_path(TIAGO, "like", TIM, "teammate", AL), _path(TIAGO, "serve", "Spurs")]),
    # ---- MultiEdgesAll (the suite runs the same query twice)
    dict(line=816, kind="ALL", direction="", query=_q("ALL", [TIM], [TONY, "Spurs"], "like,serve", 3),
         paths=[_path(TIM, "like", TONY), _path(TIM, "like", TONY, "like", AL, "like", TONY),
                _path(TIM, "like", TONY, "like", TIM, "like", TONY), _path(TIM, "like", MANU, "like", TIM, "like", TONY),
                _path(TIM, "serve", "Spurs"), _path(TIM, "like", TONY, "serve", "Spurs"), _path(TIM, "like", MANU, "serve", "Spurs"),
                _path(TIM, "like", TONY, "like", AL, "serve", "Spurs"), _path(TIM, "like", TONY, "like", MANU, "serve", "Spurs"),
                _path(TIM, "like", TONY, "like", TIM, "serve", "Spurs"), _path(TIM, "like", MANU, "like", TIM, "serve", "Spurs")]),
    # ---- VertexNotExist
    dict(line=879, kind="SHORTEST", direction="", query="FIND SHORTEST PATH FROM {NOBODY1} TO {NOBODY2} OVER like UPTO 5 STEPS", paths=[]),
    dict(line=889, kind="SHORTEST", direction="", query="FIND SHORTEST PATH FROM {P:Tim Duncan} TO {NOBODY} OVER like UPTO 5 STEPS", paths=[]),
    dict(line=899, kind="SHORTEST", direction="", query="FIND SHORTEST PATH FROM {NOBODY} TO {P:Tim Duncan} OVER like UPTO 5 STEPS", paths=[]),
    dict(line=909, kind="ALL", direction="", query="FIND ALL PATH FROM {NOBODY1} TO {NOBODY2} OVER like UPTO 5 STEPS", paths=[]),
    dict(line=919, kind="ALL", direction="", query="FIND ALL PATH FROM {P:Tim Duncan} TO {NOBODY} OVER like UPTO 5 STEPS", paths=[]),
    dict(line=929, kind="ALL", direction="", query="FIND ALL PATH FROM {NOBODY} TO {P:Tim Duncan} OVER like UPTO 5 STEPS", paths=[]),
    # ---- DuplicateColumn, EmptyInput
    dict(line=942, kind="SHORTEST", direction="", error="execution",
         query="GO FROM {P:Tim Duncan} OVER like yield like._src AS src, like._dst AS src| "
               "FIND SHORTEST PATH FROM $-.src TO $-.dst OVER like UPTO 5 STEPS"),
    dict(line=966, kind="SHORTEST", direction="", error="execution",
         query="GO FROM {NONEXIST} OVER like yield like._src AS src, like._dst AS dst| "
               "FIND SHORTEST PATH FROM $-.src TO $-.dst OVER like UPTO 5 STEPS"),
]
