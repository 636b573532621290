"""Known answers transcribed from the reference SetTest suite (src/graph/test/SetTest.cpp) on the NBA fixture
(tests/golden/nba.json). Data only: queries, expected column names and expected rows, or an error class.

Placeholders as in gotest_cases.py: {P:<name>} in a query is the player's vid, {NOBODY} a vid no player has.
"line" is the line of the case's query in SetTest.cpp. The suite builds its expected rows from the fixture's
players (tim.serves(), the serves of everyone tim.likes(), ...); they are written out here. Rows compare sorted
(verifyResult sorts). "empty": the response has the column names and no rows. "names_only": the reference
checks success and the column names and builds expected rows it never verifies. "error": "syntax"
(E_SYNTAX_ERROR) or "execution" (E_EXECUTION_ERROR). "device": the first operator has a kernel and both its operands are
plain GO sentences, eligible for the device path.

Left out, because they need `YIELD $var.*` (YieldExecutor over a variable, outside this path): AssignSet
(SetTest.cpp:490-613), the second EmptyInput case (:649-670) and CatchExceptionInSetOp (:723-772).
"""

_S3 = "GO FROM {P:%s} OVER serve YIELD $^.player.name, serve.start_year, $$.team.name"
_LIKE_SERVE = ("GO FROM {P:%s} OVER like YIELD like._dst as id | "
               "GO FROM $-.id OVER serve YIELD $^.player.name, serve.start_year, $$.team.name")
_NAMES3 = ["$^.player.name", "serve.start_year", "$$.team.name"]
_EMPTY2 = "GO FROM {NOBODY} OVER serve YIELD serve.start_year, $$.team.name"

_TIM = [("Tim Duncan", 1997, "Spurs")]
_TONY = [("Tony Parker", 1999, "Spurs"), ("Tony Parker", 2018, "Hornets")]
_MANU = [("Manu Ginobili", 2002, "Spurs")]
_TIM_LIKES = _TONY + _MANU                                        # the serves of everyone Tim Duncan likes

CASES = [
    # ---- UnionAllTest
    dict(line=32, query=_S3 % "Tim Duncan" + " UNION ALL " + _S3 % "Tony Parker", names=_NAMES3, rows=_TIM + _TONY),
    dict(line=61, query=_S3 % "Tim Duncan" + " UNION ALL " + _S3 % "Tony Parker" + " UNION ALL " + _S3 % "Manu Ginobili",
         names=_NAMES3, rows=_TIM + _TONY + _MANU),
    dict(line=99, query="(" + _LIKE_SERVE % "Tim Duncan" + ")" + " UNION ALL " + _S3 % "Tony Parker", names=_NAMES3,
         rows=_TIM_LIKES + _TONY),
    dict(line=133, query=_LIKE_SERVE % "Tim Duncan" + " UNION ALL " + _S3 % "Tony Parker", names=_NAMES3, rows=_TIM_LIKES + _TONY),
    dict(line=167, query=_S3 % "Tony Parker" + " UNION ALL " + "(" + _LIKE_SERVE % "Tim Duncan" + ")", names=_NAMES3,
         rows=_TIM_LIKES + _TONY),
    dict(line=201, query=_S3 % "Tony Parker" + " UNION ALL " + _LIKE_SERVE % "Tim Duncan", names=_NAMES3, rows=_TIM_LIKES + _TONY),
    dict(line=235, names_only=True,
         query="(GO FROM {P:Tony Parker} OVER like YIELD like._dst as id UNION ALL GO FROM {P:Tim Duncan} OVER like YIELD "
               "like._dst as id) | GO FROM $-.id OVER serve YIELD $^.player.name, serve.start_year, $$.team.name", names=_NAMES3),
    # the column names and types differ: the right side's start_year is cast to the left's string column
    dict(line=272, names_only=True,
         query="GO FROM {P:Tim Duncan} OVER serve YIELD $^.player.name as name, $$.team.name as player UNION ALL "
               "GO FROM {P:Tony Parker} OVER serve YIELD $^.player.name as name, serve.start_year", names=["name", "player"],
         cast_rows=[("Tim Duncan", "Spurs"), ("Tony Parker", "1999"), ("Tony Parker", "2018")]),
    dict(line=302, query="GO FROM {P:Nobody} OVER serve YIELD $^.player.name as player, serve.start_year as start UNION ALL "
                         "GO FROM {P:Tony Parker} OVER serve YIELD $^.player.name, serve.start_year",
         names=["player", "start"], rows=[("Tony Parker", 1999), ("Tony Parker", 2018)]),
    # ---- UnionDistinct
    dict(line=331, query="(" + _LIKE_SERVE % "Tim Duncan" + ")" + " UNION " + _S3 % "Tony Parker" + " UNION " + _S3 % "Manu Ginobili",
         names=_NAMES3, rows=_TIM_LIKES),
    dict(line=363, query="(" + _LIKE_SERVE % "Tim Duncan" + ")" + " UNION DISTINCT " + _S3 % "Tony Parker", names=_NAMES3,
         rows=_TIM_LIKES),
    # ---- Minus, Intersect, Mix
    dict(line=395, query="(" + _LIKE_SERVE % "Tim Duncan" + ")" + " MINUS " + _S3 % "Tony Parker", names=_NAMES3, rows=_MANU),
    dict(line=430, query="(" + _LIKE_SERVE % "Tim Duncan" + ")" + " INTERSECT " + _S3 % "Tony Parker", names=_NAMES3, rows=_TONY),
    dict(line=459, query="(" + _LIKE_SERVE % "Tim Duncan" + ")" + " MINUS " + _S3 % "Tony Parker" + " UNION " + _S3 % "Tim Duncan" +
                         " INTERSECT " + _S3 % "Manu Ginobili", names=_NAMES3, rows=_MANU),
    # ---- EmptyInput
    dict(line=630, device=True, query=_EMPTY2 + " UNION " + _EMPTY2 + " MINUS " + _EMPTY2 + " INTERSECT " + _EMPTY2,
         names=["serve.start_year", "$$.team.name"], empty=True),
    # ---- SyntaxError: a set sentence fed by a pipe
    dict(line=678, query="GO FROM 123 OVER like YIELD like._src as src, like._dst as dst | (GO FROM $-.src OVER serve "
                         "UNION GO FROM $-.dst OVER serve)", error="syntax"),
    # ---- ExecutionError: a prop that does not exist; different column counts (twice in the suite)
    dict(line=690, device=True, query=_S3 % "Tim Duncan" + " UNION " +
         "GO FROM {P:Tony Parker} OVER serve YIELD $^.player.name1, serve.start_year, $$.team.name", error="execution"),
    dict(line=701, query="GO FROM {P:Tim Duncan} OVER serve YIELD $^.player.name, serve.start_year UNION " + _S3 % "Tony Parker",
         error="execution"),
    dict(line=712, query="GO FROM {P:Tim Duncan} OVER serve YIELD $^.player.name, serve.start_year UNION " + _S3 % "Tony Parker",
         error="execution"),
]
