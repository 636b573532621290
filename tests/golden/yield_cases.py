"""Known answers transcribed from the reference YieldTest suite (src/graph/test/YieldTest.cpp) on the NBA fixture
(tests/golden/nba.json): every case of YieldPipe :219-318, YieldVar :321-420, Error :423-493, AggCall :592-692,
EmptyInput :694-757, DuplicateColumn :760-787 and PipeYieldGo :789-850, in the reference's order, with its players
and its expected values. Data only: queries and expected rows or errors.

Placeholders as in gotest_cases.py: {P:<name>} / {T:<name>} in a query, "P:<name>" / "T:<name>" in a row. Rows are
compared sorted (verifyResult). "names": the reference also verifies the column names. "error": the reference
asserts a failure ("syntax": E_SYNTAX_ERROR, "exec": E_EXECUTION_ERROR, "any": the code is not asserted); "text",
where given, is the Status text YieldExecutor words it with (not part of the reference's assertion).
"""

GO = "GO FROM {P:Boris Diaw} OVER serve YIELD $^.player.name as name, serve.start_year as start, $$.team.name as team"
VAR = " $var = " + GO + ";"
TEAMS = [("Hawks", 2003), ("Suns", 2005), ("Hornets", 2008), ("Spurs", 2012), ("Jazz", 2016)]     # Boris Diaw's serves
AFTER = [(t, y) for t, y in TEAMS if y > 2005]
LIKE = "GO FROM {P:Carmelo Anthony} OVER like YIELD $$.player.age AS age, like.likeness AS like"
NON_EXIST = "GO FROM {P:NON EXIST VERTEX ID} OVER serve YIELD $^.player.name as name, serve.start_year as start, " \
            "$$.team.name as team"
ONLY_INPUT = "SyntaxError: Only support input and variable in yield sentence."

CASES = [
    # YieldPipe
    {"name": "pipe team", "query": GO + "| YIELD $-.team", "rows": [(t,) for t, _ in TEAMS]},
    {"name": "pipe where const", "query": GO + "| YIELD $-.team WHERE 1 == 1", "rows": [(t,) for t, _ in TEAMS]},
    {"name": "pipe where start", "query": GO + "| YIELD $-.team WHERE $-.start > 2005", "rows": [(t,) for t, _ in AFTER]},
    {"name": "pipe star", "query": GO + "| YIELD $-.*", "rows": [("Boris Diaw", y, t) for t, y in TEAMS]},
    {"name": "pipe star where", "query": GO + "| YIELD $-.* WHERE $-.start > 2005",
     "rows": [("Boris Diaw", y, t) for t, y in AFTER]},
    {"name": "pipe star and hash", "query": GO + "| YIELD $-.*,hash(123) as hash WHERE $-.start > 2005",
     "rows": [("Boris Diaw", y, t, 123) for t, y in AFTER]},
    # YieldVar
    {"name": "var team", "query": VAR + "YIELD $var.team", "rows": [(t,) for t, _ in TEAMS]},
    {"name": "var where const", "query": VAR + "YIELD $var.team WHERE 1 == 1", "rows": [(t,) for t, _ in TEAMS]},
    {"name": "var where start", "query": VAR + "YIELD $var.team WHERE $var.start > 2005", "rows": [(t,) for t, _ in AFTER]},
    {"name": "var star", "query": VAR + "YIELD $var.*", "rows": [("Boris Diaw", y, t) for t, y in TEAMS]},
    {"name": "var star where", "query": VAR + "YIELD $var.* WHERE $var.start > 2005",
     "rows": [("Boris Diaw", y, t) for t, y in AFTER]},
    {"name": "var star and hash", "query": VAR + "YIELD $var.*, hash(123) as hash WHERE $var.start > 2005",
     "rows": [("Boris Diaw", y, t, 123) for t, y in AFTER]},
    # Error
    {"name": "input alone", "query": "yield $-", "error": "any"},
    {"name": "both input and variable", "query": VAR + "YIELD $var.team WHERE $-.start > 2005", "error": "exec",
     "text": "Not support both input and variable."},
    {"name": "two variables", "query": VAR + "YIELD $var.team WHERE $var1.start > 2005", "error": "exec",
     "text": "Only one variable allowed to use."},
    {"name": "no such variable column", "query": VAR + "YIELD $var.abc", "error": "exec",
     "text": "column `abc' not exist in variable."},
    {"name": "no such input column", "query": "GO FROM {P:Boris Diaw} OVER like | YIELD $-.abc;", "error": "exec",
     "text": "column `abc' not exist in input."},
    {"name": "dst prop", "query": VAR + "YIELD $$.a.team", "error": "syntax", "text": ONLY_INPUT},
    {"name": "src prop", "query": VAR + "YIELD $^.a.team", "error": "syntax", "text": ONLY_INPUT},
    {"name": "edge prop", "query": VAR + "YIELD a.team", "error": "syntax", "text": ONLY_INPUT},
    # AggCall
    {"name": "count and input without input", "query": "YIELD COUNT(1), $-.name", "error": "exec", "text": "Inputs nullptr."},
    {"name": "constant aggregates", "query": "YIELD COUNT(*), 1+1", "rows": [(1, 2)]},
    {"name": "agg beside input column", "query": LIKE + "| YIELD COUNT(*), $-.age", "error": "syntax",
     "text": "SyntaxError: Input columns without aggregation are not supported in YIELD statement without GROUP BY, "
             "near `$-.age'"},
    {"name": "agg over pipe", "query": LIKE + "| YIELD AVG($-.age), SUM($-.like), COUNT(*), 1+1",
     "rows": [(34.666666666666664, 270, 3, 2)]},
    {"name": "count behind a bare go", "query": "GO FROM {P:Carmelo Anthony} OVER like | YIELD COUNT(*)", "rows": [(3,)]},
    {"name": "constant per row", "query": "GO FROM {P:Carmelo Anthony} OVER like | YIELD 1", "rows": [(1,), (1,), (1,)]},
    {"name": "constant per row of nobody", "query": "GO FROM {P:Nobody} OVER like | YIELD 1", "rows": []},
    {"name": "agg over variable", "query": "$var = " + LIKE + ";YIELD AVG($var.age), SUM($var.like), COUNT(*)",
     "rows": [(34.666666666666664, 270, 3)]},
    # EmptyInput
    {"name": "empty input", "query": NON_EXIST + "| YIELD $-.team", "rows": [], "names": ["$-.team"]},
    {"name": "empty variable", "query": " $var = " + NON_EXIST + ";YIELD $var.team", "rows": [], "names": ["$var.team"]},
    {"name": "where keeps none, then yield",
     "query": "GO FROM {P:Marco Belinelli} OVER serve YIELD $^.player.name as name, serve.start_year as start, "
              "$$.team.name as team | YIELD $-.name as name WHERE $-.start > 20000 | YIELD $-.name AS name",
     "rows": [], "names": ["name"]},
    # DuplicateColumn
    {"name": "duplicate constants", "query": "YIELD 1, 1", "rows": [(1, 1)], "names": ["1", "1"]},
    {"name": "duplicate column", "query": "GO FROM {P:Boris Diaw} OVER serve YIELD $^.player.name as team, "
                                         "serve.start_year as start, $$.team.name as team| YIELD $-.team", "error": "exec",
     "text": "Duplicate column `team'"},
    # PipeYieldGo
    {"name": "yield feeds go", "query": "GO FROM {P:Tim Duncan} OVER serve YIELD serve._src as id |YIELD $-.id as id | "
                                       "GO FROM $-.id OVER serve YIELD $$.team.name as name",
     "rows": [("Spurs",)], "names": ["name"]},
    {"name": "piped yield into a variable", "query": "$var = GO FROM {P:Tim Duncan} OVER serve YIELD serve._src as id |"
                                                    "YIELD $-.id as id; GO FROM $var.id OVER serve YIELD $$.team.name as name",
     "rows": [("Spurs",)], "names": ["name"]},
    {"name": "yield of a variable into a variable",
     "query": "$var = GO FROM {P:Tim Duncan} OVER serve YIELD serve._src as id;$var2 = YIELD $var.id as id; "
              "GO FROM $var2.id OVER serve YIELD $$.team.name as name",
     "rows": [("Spurs",)], "names": ["name"]},
]
