"""Known answers transcribed from the reference FETCH suites (src/graph/test/FetchVerticesTest.cpp,
FetchEdgesTest.cpp) on the NBA fixture (tests/golden/nba.json). Data only: queries, column names, expected rows.

Placeholders as in gotest_cases.py: {P:<name>} / {T:<name>} in a query are replaced by the player / team vid,
"P:<name>" / "T:<name>" in an expected row stand for that vid. Rows are compared sorted, as verifyResult does.
A case is (name, query, column names or None where the reference does not assert them, outcome); the outcome is a
list of rows, "empty" (the response had no rows), "syntax" (E_SYNTAX_ERROR) or "error" (E_EXECUTION_ERROR).

Left out, and why:
  - every uuid("...") case (FetchVerticesTest.cpp:173-187, 225-237; FetchEdgesTest.cpp:225-239, 315-328, 539-554):
    uuid() needs the storage UUID service;
  - FetchVerticesTest FetchAll from :408 on (`FETCH PROP ON bachelor`, and `ON *` over a vertex with two tags): the
    test inserts a bachelor row first, which the fixture does not hold;
  - FetchVerticesTest EmptyInput :566-576 and FetchEdgesTest EmptyInput :476-497: they pipe through
    `| YIELD ... WHERE`, a sentence this path does not run.
"""

BORIS, TIM, TONY = "P:Boris Diaw", "P:Tim Duncan", "P:Tony Parker"
NOBODY = "{P:NON EXIST VERTEX ID}"
BORIS_SERVES = [(BORIS, "T:Hawks", 0, 2003, 2005), (BORIS, "T:Suns", 0, 2005, 2008), (BORIS, "T:Hornets", 0, 2008, 2012),
                (BORIS, "T:Spurs", 0, 2012, 2016), (BORIS, "T:Jazz", 0, 2016, 2017)]
LIKED = [(TONY, "Tony Parker", 36), (TIM, "Tim Duncan", 42)]
PNA = ["VertexID", "player.name", "player.age"]
SSE = ["serve._src", "serve._dst", "serve._rank", "serve.start_year", "serve.end_year"]

VERTEX_CASES = [
    # Base (FetchVerticesTest.cpp:28-171)
    ("v_base", "FETCH PROP ON player {P:Boris Diaw} YIELD player.name, player.age", PNA, [(BORIS, "Boris Diaw", 36)]),
    ("v_base_expr", "FETCH PROP ON player {P:Boris Diaw} YIELD player.name, player.age, player.age > 30",
     PNA + ["(player.age>30)"], [(BORIS, "Boris Diaw", 36, 1)]),
    ("v_pipe", "GO FROM {P:Boris Diaw} over like YIELD like._dst as id"
               "| FETCH PROP ON player $-.id YIELD player.name, player.age", PNA, LIKED),
    ("v_pipe_star", "GO FROM {P:Boris Diaw} over like YIELD like._dst as id"
                    "| FETCH PROP ON player $-.id YIELD player.name, player.age, $-.*", PNA + ["$-.id"], None),
    ("v_pipe_team_star", "GO FROM {P:Boris Diaw} over like YIELD like._dst as id"
                         "| FETCH PROP ON team $-.id YIELD team.name, $-.*", ["VertexID", "team.name", "$-.id"], None),
    ("v_var", "$var = GO FROM {P:Boris Diaw} over like YIELD like._dst as id;"
              "FETCH PROP ON player $var.id YIELD player.name, player.age", PNA, LIKED),
    ("v_var_order", "$var = GO FROM {P:Boris Diaw} over like YIELD like._dst as id;"
                    "FETCH PROP ON player $var.id YIELD player.name as name, player.age | ORDER BY name",
     ["VertexID", "name", "player.age"], [(TIM, "Tim Duncan", 42), (TONY, "Tony Parker", 36)]),
    ("v_hash", 'FETCH PROP ON player hash("Boris Diaw") YIELD player.name, player.age', PNA, [(BORIS, "Boris Diaw", 36)]),
    # NoYield (:189-223)
    ("v_noyield", "FETCH PROP ON player {P:Boris Diaw}", PNA, [(BORIS, "Boris Diaw", 36)]),
    ("v_noyield_hash", 'FETCH PROP ON player hash("Boris Diaw")', PNA, [(BORIS, "Boris Diaw", 36)]),
    # Distinct (:240-281)
    ("v_distinct", "FETCH PROP ON player {P:Boris Diaw}, {P:Boris Diaw} YIELD DISTINCT player.name, player.age", PNA,
     [(BORIS, "Boris Diaw", 36)]),
    ("v_distinct_vids", "FETCH PROP ON player {P:Boris Diaw}, {P:Tony Parker} YIELD DISTINCT player.age",
     ["VertexID", "player.age"], [(BORIS, 36), (TONY, 36)]),
    # SyntaxError (:283-308)
    ("v_syntax_src", "FETCH PROP ON player {P:Boris Diaw} YIELD $^.player.name, player.age", None, "syntax"),
    ("v_syntax_dst", "FETCH PROP ON player {P:Boris Diaw} YIELD $$.player.name, player.age", None, "syntax"),
    ("v_syntax_tag", "FETCH PROP ON player {P:Boris Diaw} YIELD abc.name, player.age", None, "syntax"),
    # NonexistentTag (:310-319)
    ("v_no_tag", "FETCH PROP ON abc {P:Boris Diaw}", None, "error"),
    # NonexistentVertex (:321-357)
    ("v_no_vertex", "FETCH PROP ON player " + NOBODY, None, "empty"),
    ("v_no_vertex_pipe", "GO FROM " + NOBODY + " OVER serve | FETCH PROP ON team $-", None, "empty"),
    ("v_no_vertex_all", "FETCH PROP ON * " + NOBODY, None, "empty"),
    # FetchAll (:359-406)
    ("v_all", "FETCH PROP ON * {P:Boris Diaw} ", PNA, [(BORIS, "Boris Diaw", 36)]),
    ("v_all_pipe", "YIELD {P:Boris Diaw} as id | FETCH PROP ON * $-.id ", PNA, [(BORIS, "Boris Diaw", 36)]),
    ("v_all_twice", "FETCH PROP ON * {P:Boris Diaw}, {P:Boris Diaw} ", PNA, [(BORIS, "Boris Diaw", 36)] * 2),
    # DuplicateColumnName (:503-531)
    ("v_dup_yield", "FETCH PROP ON player {P:Boris Diaw} YIELD player.name, player.name",
     ["VertexID", "player.name", "player.name"], [(BORIS, "Boris Diaw", "Boris Diaw")]),
    ("v_dup_input", "GO FROM {P:Boris Diaw} over like YIELD like._dst as id, like._dst as id"
                    "| FETCH PROP ON player $-.id YIELD player.name, player.age", None, "error"),
    # NonexistentProp (:533-542)
    ("v_no_prop", "FETCH PROP ON player {P:Boris Diaw} YIELD player.name1", None, "error"),
    # EmptyInput (:544-565)
    ("v_empty_input", "GO FROM " + NOBODY + " over like YIELD like._dst as id | FETCH PROP ON player $-.id", None, "empty"),
]

EDGE_CASES = [
    # Base (FetchEdgesTest.cpp:29-223)
    ("e_base", "FETCH PROP ON serve {P:Boris Diaw}->{T:Hawks} YIELD serve.start_year, serve.end_year", SSE, BORIS_SERVES[:1]),
    ("e_base_expr", "FETCH PROP ON serve {P:Boris Diaw}->{T:Hawks} YIELD serve.start_year > 2001, serve.end_year",
     SSE[:3] + ["(serve.start_year>2001)", "serve.end_year"], [(BORIS, "T:Hawks", 0, 1, 2005)]),
    ("e_base_rank", "FETCH PROP ON serve {P:Boris Diaw}->{T:Hawks}@0 YIELD serve.start_year, serve.end_year", SSE,
     BORIS_SERVES[:1]),
    ("e_two_keys", "FETCH PROP ON serve {P:Boris Diaw}->{T:Hawks},{P:Boris Diaw}->{T:Suns}"
                   " YIELD serve.start_year, serve.end_year", SSE, BORIS_SERVES[:2]),
    ("e_pipe", "GO FROM {P:Boris Diaw} OVER serve YIELD serve._src AS src, serve._dst AS dst"
               "| FETCH PROP ON serve $-.src->$-.dst YIELD serve.start_year, serve.end_year", SSE, BORIS_SERVES),
    ("e_var", "$var = GO FROM {P:Boris Diaw} OVER serve YIELD serve._src AS src, serve._dst AS dst;"
              "FETCH PROP ON serve $var.src->$var.dst YIELD serve.start_year, serve.end_year", SSE, BORIS_SERVES),
    ("e_hash", 'FETCH PROP ON serve hash("Boris Diaw")->hash("Hawks") YIELD serve.start_year, serve.end_year', SSE,
     BORIS_SERVES[:1]),
    # NoYield (:241-313)
    ("e_noyield", "FETCH PROP ON serve {P:Boris Diaw}->{T:Hawks}", SSE, BORIS_SERVES[:1]),
    ("e_noyield_rank", "FETCH PROP ON serve {P:Boris Diaw}->{T:Hawks}@0", SSE, BORIS_SERVES[:1]),
    ("e_noyield_hash", 'FETCH PROP ON serve hash("Boris Diaw")->hash("Hawks")', SSE, BORIS_SERVES[:1]),
    # Distinct (:330-443)
    ("e_distinct", "FETCH PROP ON serve {P:Boris Diaw}->{T:Hawks},{P:Boris Diaw}->{T:Hawks}"
                   " YIELD DISTINCT serve.start_year, serve.end_year", SSE, BORIS_SERVES[:1]),
    ("e_distinct_pipe", "GO FROM {P:Boris Diaw},{P:Boris Diaw} OVER serve YIELD serve._src AS src, serve._dst AS dst"
                        "| FETCH PROP ON serve $-.src->$-.dst YIELD DISTINCT serve.start_year, serve.end_year", SSE,
     BORIS_SERVES),
    ("e_distinct_var", "$var = GO FROM {P:Boris Diaw},{P:Boris Diaw} OVER serve YIELD serve._src AS src, serve._dst AS dst;"
                       "FETCH PROP ON serve $var.src->$var.dst YIELD DISTINCT serve.start_year, serve.end_year", SSE,
     BORIS_SERVES),
    ("e_distinct_dst", "GO FROM {P:Tim Duncan},{P:Tony Parker} OVER serve YIELD serve._src AS src, serve._dst AS dst"
                       "| FETCH PROP ON serve $-.src->$-.dst YIELD DISTINCT serve._dst as dst", SSE[:3] + ["dst"],
     [(TIM, "T:Spurs", 0, "T:Spurs"), (TONY, "T:Hornets", 0, "T:Hornets"), (TONY, "T:Spurs", 0, "T:Spurs")]),
    # EmptyInput (:445-474)
    ("e_empty_input", "GO FROM " + NOBODY + " OVER serve YIELD serve._src AS src, serve._dst AS dst"
                      "| FETCH PROP ON serve $-.src->$-.dst YIELD serve.start_year, serve.end_year", SSE, "empty"),
    # SyntaxError (:501-523)
    ("e_syntax_src", 'FETCH PROP ON serve hash("Boris Diaw")->hash("Spurs") YIELD $^.serve.start_year', None, "syntax"),
    ("e_syntax_dst", 'FETCH PROP ON serve hash("Boris Diaw")->hash("Spurs") YIELD $$.serve.start_year', None, "syntax"),
    ("e_syntax_edge", 'FETCH PROP ON serve hash("Boris Diaw")->hash("Spurs") YIELD abc.start_year', None, "syntax"),
    # NonexistentEdge (:525-537)
    ("e_no_edge", 'FETCH PROP ON serve hash("Zion Williamson")->hash("Spurs") YIELD serve.start_year',
     SSE[:3] + ["serve.start_year"], "empty"),
    # DuplicateColumnName (:556-623)
    ("e_dup_yield", "FETCH PROP ON serve {P:Boris Diaw}->{T:Hawks} YIELD serve.start_year, serve.start_year",
     SSE[:3] + ["serve.start_year", "serve.start_year"], [(BORIS, "T:Hawks", 0, 2003, 2003)]),
    ("e_key_props", "FETCH PROP ON serve {P:Boris Diaw}->{T:Hawks} YIELD serve._src, serve._dst, serve._rank",
     SSE[:3] + SSE[:3], [(BORIS, "T:Hawks", 0, BORIS, "T:Hawks", 0)]),
    ("e_dup_input", "GO FROM {P:Boris Diaw} OVER serve YIELD serve._src AS src, serve._dst AS src"
                    "| FETCH PROP ON serve $-.src->$-.dst YIELD serve.start_year, serve.end_year", None, "error"),
    # NonexistentProp (:625-636)
    ("e_no_prop", "FETCH PROP ON serve {P:Boris Diaw}->{T:Hawks} YIELD serve.start_year1", None, "error"),
]

CASES = VERTEX_CASES + EDGE_CASES
