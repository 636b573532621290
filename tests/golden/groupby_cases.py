"""Known answers transcribed from the reference GroupByLimitTest suite
(src/graph/test/GroupByLimitTest.cpp) on the NBA fixture (tests/golden/nba.json). Data only: queries,
expected column names and expected rows, or "syntax error".

Placeholders as in gotest_cases.py: {P:<name>} in a query is the player's vid. Rows are compared sorted
(verifyResult, src/graph/test/TestBase.h:188-233). "error": the reference asserts E_SYNTAX_ERROR.
"empty": the response has column names and no rows. "device": the GO | GROUP BY pair is eligible for the
device path (plain GO on the left; keys and values of static integer / string type; no STD, no
function key).

Left out, because they use ORDER BY or LIMIT (a later step): :30-41 (LIMIT syntax errors), :173-266
(LimitTest), :462-519 (GroupByOrderByLimitTest), :550-569 and :587-603 (EmptyInput with ORDER BY /
LIMIT), and :570-586 (a `| YIELD ... WHERE' segment, YieldExecutor).
"""

_NAME_ID = "GO FROM {P:Marco Belinelli} OVER serve YIELD $$.team.name AS name, serve._dst AS id"

ERROR_CASES = [
    # SyntaxError (GroupByLimitTest.cpp:29-171)
    dict(line=43, query="GO FROM {P:Marco Belinelli} OVER serve YIELD $$.team.name AS name"
                        "| GROUP BY 1+1 YIELD COUNT(1), 1+1", error=True),
    dict(line=56, query="GO FROM {P:Marco Belinelli} OVER serve YIELD $$.team.name AS name, "
                        "serve.end_year AS end_year | GROUP BY $-.start_year YIELD COUNT($var)", error=True),
    dict(line=69, query="GO FROM {P:Marco Belinelli} OVER serve YIELD $$.team.name AS name, "
                        "serve.end_year AS end_year | GROUP BY $-.start_year YIELD COUNT($$.team.name)",
         error=True),
    dict(line=82, query=_NAME_ID + "| GROUP BY $-.start_year YIELD COUNT($-.id)", error=True),
    dict(line=95, query=_NAME_ID + "| GROUP BY team YIELD COUNT($-.id), $-.name AS teamName", error=True),
    dict(line=109, query=_NAME_ID + "| GROUP BY $-.name YIELD COUNT($-.start_year)", error=True),
    dict(line=122, query=_NAME_ID + "| GROUP BY $-.name YIELD SUM(*)", error=True),
    dict(line=135, query=_NAME_ID + "| GROUP BY $-.name YIELD COUNT($-.name, $-.id)", error=True),
    dict(line=148, query=_NAME_ID + "| GROUP BY $-.name, SUM($-.id) YIELD $-.name,  SUM($-.id)", error=True),
    dict(line=161, query="GO FROM {P:Marco Belinelli} OVER serve YIELD $$.team.name AS name, "
                         "COUNT(serve._dst) AS id", error=True),
]

_LIKE_NAME = "GO FROM {P:Carmelo Anthony},{P:Dwyane Wade} OVER like YIELD $$.player.name AS name"

CASES = [
    # GroupByTest (:268-459)
    dict(line=270, device=True,
         query="GO FROM {P:Marco Belinelli} OVER serve YIELD $$.team.name AS name, serve._dst AS id, "
               "serve.start_year AS start_year, serve.end_year AS end_year"
               "| GROUP BY $-.start_year YIELD COUNT($-.id), $-.start_year AS start_year, "
               "AVG($-.end_year) as avg",
         rows=[(2, 2018, 2018.5), (1, 2017, 2018.0), (1, 2016, 2017.0), (1, 2009, 2010.0), (1, 2007, 2009.0),
               (1, 2012, 2013.0), (1, 2015, 2016.0), (1, 2010, 2012.0), (1, 2013, 2015.0)]),
    dict(line=299, device=False,                                   # STD
         query="GO FROM {P:Aron Baynes},{P:Tracy McGrady} OVER serve YIELD $$.team.name AS name, "
               "serve._dst AS id, serve.start_year AS start, serve.end_year AS end"
               "| GROUP BY teamName, start_year YIELD $-.name AS teamName, $-.start AS start_year, "
               "MAX($-.start), MIN($-.end), AVG($-.end) AS avg_end_year, STD($-.end) AS std_end_year, "
               "COUNT($-.id)",
         names=["teamName", "start_year", "MAX($-.start)", "MIN($-.end)", "avg_end_year", "std_end_year",
                "COUNT($-.id)"],
         rows=[("Celtics", 2017, 2017, 2019, 2019.0, 0, 1), ("Magic", 2000, 2000, 2004, 2004.0, 0, 1),
               ("Pistons", 2015, 2015, 2017, 2017.0, 0, 1), ("Raptors", 1997, 1997, 2000, 2000.0, 0, 1),
               ("Rockets", 2004, 2004, 2010, 2010.0, 0, 1), ("Spurs", 2013, 2013, 2013, 2014.0, 1, 2)]),
    dict(line=343, device=True,
         query="GO FROM {P:Carmelo Anthony},{P:Dwyane Wade} OVER like YIELD $$.player.name AS name, "
               "$$.player.age AS dst_age, $$.player.age AS src_age, like.likeness AS likeness"
               "| GROUP BY $-.name YIELD $-.name AS name, SUM($-.dst_age) AS sum_dst_age, "
               "AVG($-.dst_age) AS avg_dst_age, MAX($-.src_age) AS max_src_age, "
               "MIN($-.src_age) AS min_src_age, BIT_AND(1) AS bit_and, BIT_OR(2) AS bit_or, "
               "BIT_XOR(3) AS bit_xor, COUNT($-.likeness), COUNT_DISTINCT($-.likeness)",
         names=["name", "sum_dst_age", "avg_dst_age", "max_src_age", "min_src_age", "bit_and", "bit_or",
                "bit_xor", "COUNT($-.likeness)", "COUNT_DISTINCT($-.likeness)"],
         rows=[("LeBron James", 68, 34.0, 34, 34, 1, 2, 0, 2, 1), ("Chris Paul", 66, 33.0, 33, 33, 1, 2, 0, 2, 1),
               ("Dwyane Wade", 37, 37.0, 37, 37, 1, 2, 3, 1, 1),
               ("Carmelo Anthony", 34, 34.0, 34, 34, 1, 2, 3, 1, 1)]),
    dict(line=401, device=False,                                   # function key abs(5)
         query=_LIKE_NAME + "| GROUP BY $-.name, abs(5) YIELD $-.name AS name, SUM(1.5) AS sum, "
                            "COUNT(*) AS count,1+1 AS cal",
         names=["name", "sum", "count", "cal"],
         rows=[("LeBron James", 3.0, 2, 2), ("Chris Paul", 3.0, 2, 2), ("Dwyane Wade", 1.5, 1, 2),
               ("Carmelo Anthony", 1.5, 1, 2)]),
    dict(line=431, device=True,                                    # the outcome feeds the next GO
         query="GO FROM {P:Paul Gasol} OVER like YIELD $$.player.age AS age, like._dst AS id "
               "| GROUP BY $-.id YIELD $-.id AS id, SUM($-.age) AS age "
               "| GO FROM $-.id OVER serve YIELD $$.team.name AS name, $-.age AS sumAge",
         names=["name", "sumAge"],
         rows=[("Grizzlies", 34), ("Raptors", 34), ("Lakers", 40)]),
    # EmptyInput (:521-549): a vid with no vertex
    dict(line=534, device=False,
         query="GO FROM {P:NON EXIST VERTEX ID} OVER serve YIELD $^.player.name as name, "
               "serve.start_year as start, $$.team.name as name| GROUP BY $-.name YIELD $-.name AS name",
         names=["name"], empty=True),
]
