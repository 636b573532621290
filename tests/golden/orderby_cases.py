"""Known answers transcribed from the reference OrderByTest suite (src/graph/test/OrderByTest.cpp) and the
ORDER BY / LIMIT ranges of GroupByLimitTest (src/graph/test/GroupByLimitTest.cpp) on the NBA fixture
(tests/golden/nba.json). Data only: queries, expected column names and expected rows, or an error class.

Placeholders as in gotest_cases.py: {P:<name>} in a query is the player's vid, {NOBODY} a vid no player has.
"source" names the suite ("order" / "group"), "line" the line of the case. "ordered": the reference compares
the rows in order (verifyResult(resp, expected, false)); otherwise sorted. "empty": the response has the
column names and no rows. "nothing": it has neither. "count": only the number of rows is asserted.
"error": "syntax" (E_SYNTAX_ERROR) or "execution" (E_EXECUTION_ERROR). "device": the pipe holds a plain
`GO | ORDER BY | LIMIT` or `GO | LIMIT` head that is eligible for the device path; "string_factor": its
ORDER BY factor is a string column.

Left out, because their pipe holds a `| YIELD ... WHERE` segment (YieldExecutor, outside this path):
OrderByTest.cpp:86-102, GroupByLimitTest.cpp:570-586 and GroupByLimitTest.cpp:587-603 (`... | YIELD ... WHERE
... | Limit 1` on an input without rows; tests/test_orderby_host.py checks LIMIT on such an input directly).
OrderByTest.cpp:143-164 asserts that a wrong order does NOT verify; it is kept as the same query with its
right order (:121-142).
"""

_SERVE3 = "GO FROM {P:Boris Diaw} OVER serve YIELD $^.player.name as name, serve.start_year as start, $$.team.name as team"
_MULTI = ("GO FROM {P:Boris Diaw},{P:LaMarcus Aldridge} OVER serve WHERE serve.start_year >= 2012 YIELD "
          "$$.team.name as team, $^.player.name as player, $^.player.age as age, serve.start_year as start")
_TEAMS_ASC = [("Boris Diaw", 2003, "Hawks"), ("Boris Diaw", 2008, "Hornets"), ("Boris Diaw", 2016, "Jazz"),
              ("Boris Diaw", 2012, "Spurs"), ("Boris Diaw", 2005, "Suns")]
_GROUPED = ("GO FROM {P:Carmelo Anthony},{P:Dwyane Wade} OVER like YIELD $$.player.name AS name"
            "| GROUP BY $-.name, abs(5) YIELD $-.name AS name, SUM(1.5) AS sum, COUNT(*) AS count ")
_BELINELLI = "GO FROM {P:Marco Belinelli} OVER serve YIELD $$.team.name AS name"
_GREEN = "GO FROM {P:Danny Green} OVER serve YIELD $$.team.name AS name"

CASES = [
    # ---- OrderByTest.cpp
    dict(source="order", line=32, query="ORDER BY ", error="syntax"),
    dict(source="order", line=40,
         query="GO FROM {P:Boris Diaw} OVER serve YIELD $^.player.name as name, serve.start_year as start, $$.team.name"
               "| ORDER BY $-.$$.team.name", error="syntax"),
    dict(source="order", line=64, query="ORDER BY $-.xx", nothing=True),
    dict(source="order", line=72,
         query="GO FROM {NOBODY} OVER serve YIELD $^.player.name as name, serve.start_year as start, $$.team.name as team"
               "| ORDER BY $-.name", names=["name", "start", "team"], empty=True),
    dict(source="order", line=111, query=_SERVE3 + "| ORDER BY $-.abc", error="execution"),
    dict(source="order", line=124, query=_SERVE3 + "| ORDER BY $-.team", names=["name", "start", "team"],
         ordered=True, rows=_TEAMS_ASC),
    dict(source="order", line=168, query=_SERVE3 + "| ORDER BY $-.team ASC", names=["name", "start", "team"],
         ordered=True, rows=_TEAMS_ASC),
    dict(source="order", line=190, query=_SERVE3 + "| ORDER BY $-.team DESC", names=["name", "start", "team"],
         ordered=True, rows=_TEAMS_ASC[::-1]),
    dict(source="order", line=219, query=_MULTI + "| ORDER BY $-.team, $-.age", names=["team", "player", "age", "start"],
         ordered=True, rows=[("Jazz", "Boris Diaw", 36, 2016), ("Spurs", "LaMarcus Aldridge", 33, 2015),
                             ("Spurs", "Boris Diaw", 36, 2012)]),
    dict(source="order", line=240, query=_MULTI + "| ORDER BY $-.team ASC, $-.age ASC",
         ordered=True, rows=[("Jazz", "Boris Diaw", 36, 2016), ("Spurs", "LaMarcus Aldridge", 33, 2015),
                             ("Spurs", "Boris Diaw", 36, 2012)]),
    dict(source="order", line=255, query=_MULTI + "| ORDER BY $-.team ASC, $-.age DESC",
         names=["team", "player", "age", "start"],
         ordered=True, rows=[("Jazz", "Boris Diaw", 36, 2016), ("Spurs", "Boris Diaw", 36, 2012),
                             ("Spurs", "LaMarcus Aldridge", 33, 2015)]),
    dict(source="order", line=276, query=_MULTI + "| ORDER BY $-.team DESC, $-.age ASC",
         names=["team", "player", "age", "start"],
         ordered=True, rows=[("Spurs", "LaMarcus Aldridge", 33, 2015), ("Spurs", "Boris Diaw", 36, 2012),
                             ("Jazz", "Boris Diaw", 36, 2016)]),
    dict(source="order", line=297, query=_MULTI + "| ORDER BY $-.team DESC, $-.age DESC",
         names=["team", "player", "age", "start"],
         ordered=True, rows=[("Spurs", "Boris Diaw", 36, 2012), ("Spurs", "LaMarcus Aldridge", 33, 2015),
                             ("Jazz", "Boris Diaw", 36, 2016)]),
    dict(source="order", line=319, query=_MULTI + "| ORDER BY team DESC, age DESC",      # bare labels
         names=["team", "player", "age", "start"],
         ordered=True, rows=[("Spurs", "Boris Diaw", 36, 2012), ("Spurs", "LaMarcus Aldridge", 33, 2015),
                             ("Jazz", "Boris Diaw", 36, 2016)]),
    dict(source="order", line=343,
         query="GO FROM {P:Boris Diaw} OVER like YIELD like._dst as id | ORDER BY $-.id | GO FROM $-.id over serve",
         names=["serve._dst"], rows=[("T:Spurs",), ("T:Spurs",), ("T:Hornets",)]),
    dict(source="order", line=364,
         query="GO FROM {P:Boris Diaw} OVER serve YIELD $^.player.name as team, serve.start_year as start, "
               "$$.team.name as team| ORDER BY $-.team", error="execution"),
    # ---- GroupByLimitTest.cpp
    dict(source="group", line=32, query="GO FROM 1 OVER server | LIMIT -1, 2", error="syntax"),
    dict(source="group", line=38, query="GO FROM 1 OVER server | LIMIT 1, -2", error="syntax"),
    dict(source="group", line=177, device=True, string_factor=True,
         query=_BELINELLI + " | ORDER BY $-.name | LIMIT 5",
         ordered=True, rows=[("76ers",), ("Bulls",), ("Hawks",), ("Hornets",), ("Hornets",)]),
    dict(source="group", line=195, device=True, string_factor=True,
         query=_BELINELLI + " | ORDER BY $-.name | LIMIT 2,2", ordered=True, rows=[("Hawks",), ("Hornets",)]),
    dict(source="group", line=207, device=True, string_factor=True,
         query=_BELINELLI + " | ORDER BY $-.name | LIMIT 2 OFFSET 2", ordered=True, rows=[("Hawks",), ("Hornets",)]),
    dict(source="group", line=218, device=True, string_factor=True,
         query="GO FROM {P:Marco Belinelli} OVER like YIELD $$.player.name AS name, like._dst AS id "
               "| ORDER BY $-.name | LIMIT 1 "
               "| GO FROM $-.id OVER like YIELD $$.player.name AS name "
               "| ORDER BY $-.name | LIMIT 2",
         ordered=True, rows=[("LeBron James",), ("Marco Belinelli",)]),
    dict(source="group", line=235, device=True, query=_GREEN + " | LIMIT 1 OFFSET 0", names=["name"], empty=True),
    dict(source="group", line=249, device=True, query=_GREEN + " | LIMIT 5", count=3),
    dict(source="group", line=259, device=True, query=_GREEN + " | LIMIT 3, 2", empty=True),
    dict(source="group", line=468, query=_GROUPED + "| ORDER BY $-.sum, $-.name", names=["name", "sum", "count"],
         ordered=True, rows=[("Carmelo Anthony", 1.5, 1), ("Dwyane Wade", 1.5, 1), ("Chris Paul", 3.0, 2),
                             ("LeBron James", 3.0, 2)]),
    dict(source="group", line=497, query=_GROUPED + "| ORDER BY $-.sum, $-.name DESC | LIMIT 2",
         names=["name", "sum", "count"],
         ordered=True, rows=[("Dwyane Wade", 1.5, 1), ("Carmelo Anthony", 1.5, 1)]),
    dict(source="group", line=552,
         query="GO FROM {NOBODY} OVER like YIELD $$.player.name AS name"
               "| GROUP BY $-.name, abs(5) YIELD $-.name AS name, SUM(1.5) AS sum, COUNT(*) AS count "
               "| ORDER BY $-.sum | LIMIT 2", names=["name", "sum", "count"], empty=True),
]
