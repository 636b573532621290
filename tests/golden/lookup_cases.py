"""The reference's LookupTest (src/graph/test/LookupTest.cpp with LookupTestBase.h) as data: schemas, indexes,
inserted rows, queries, expected rows, column names and error codes. Types are SupportedType numbers (BOOL 1, INT 2,
DOUBLE 5, STRING 6). The tests of one fixture share a space: rows inserted by an earlier test stay, repeated inserts
overwrite. Expected rows are compared sorted.

Left out:
  - NebulaKeyUtilsTest holds no literal index-key bytes (it checks encodeVariant / decodeVariant round trips only):
    its values are ROUND_TRIP below, and the byte vectors are the ones NebulaKeyUtils.h's comment on encodeInt64
    states (INT_KEYS).
  - LookupTest's DROP TAG INDEX statements after the optimizer tests (no sentence here creates or drops an index).
"""
BOOL, INT, DOUBLE, STRING = 1, 2, 5, 6
PARTS = 3                                                          # CREATE SPACE lookup_space(partition_num=3, ...)

# (is_edge, id, name, fields)
SCHEMAS = [
    (False, 2, "lookup_tag_1", [("col1", INT), ("col2", INT), ("col3", INT)]),
    (False, 3, "lookup_tag_2", [("col1", BOOL), ("col2", INT), ("col3", DOUBLE), ("col4", BOOL)]),
    (True, 4, "lookup_edge_1", [("col1", INT), ("col2", INT), ("col3", INT)]),
    (True, 5, "lookup_edge_2", [("col1", BOOL), ("col2", INT), ("col3", DOUBLE), ("col4", BOOL)]),
    (False, 6, "student", [("number", INT), ("age", INT)]),
    (False, 7, "teacher", [("number", INT), ("age", INT)]),
    (False, 8, "tag_with_str", [("c1", INT), ("c2", STRING), ("c3", STRING)]),
    (False, 9, "identity", [("BIRTHDAY", INT), ("NATION", STRING), ("BIRTHPLACE_CITY", STRING)]),
    (False, 10, "t1", [("c1", INT), ("c2", INT), ("c3", INT), ("c4", INT), ("c5", INT)]),
    (False, 11, "t1_str", [("c1", INT), ("c2", INT), ("c3", STRING), ("c4", STRING)]),
]

# (index id, name, schema name, is_edge, fields) in creation order
INDEXES = [
    (1, "t_index_1", "lookup_tag_1", False, ["col1", "col2", "col3"]),
    (2, "t_index_2", "lookup_tag_2", False, ["col2", "col3", "col4"]),
    (3, "t_index_3", "lookup_tag_1", False, ["col2", "col3"]),
    (4, "t_index_4", "lookup_tag_2", False, ["col3", "col4"]),
    (5, "t_index_5", "lookup_tag_2", False, ["col4"]),
    (6, "e_index_1", "lookup_edge_1", True, ["col1", "col2", "col3"]),
    (7, "e_index_2", "lookup_edge_2", True, ["col2", "col3", "col4"]),
    (8, "e_index_3", "lookup_edge_1", True, ["col2", "col3"]),
    (9, "e_index_4", "lookup_edge_2", True, ["col3", "col4"]),
    (10, "student_index", "student", False, ["number", "age"]),
    (11, "i1_with_str", "tag_with_str", False, ["c1", "c2"]),
    (12, "i2_with_str", "tag_with_str", False, ["c2", "c3"]),
    (13, "i3_with_str", "tag_with_str", False, ["c1", "c2", "c3"]),
    (14, "idx_identity_cname_birth_gender_nation_city", "identity", False, ["BIRTHDAY", "NATION", "BIRTHPLACE_CITY"]),
    (21, "i1", "t1", False, ["c1", "c2"]),
    (22, "i2", "t1", False, ["c2", "c1"]),
    (23, "i3", "t1", False, ["c3"]),
    (24, "i4", "t1", False, ["c1", "c2", "c3", "c4"]),
    (25, "i5", "t1", False, ["c1", "c2", "c3", "c5"]),
    (31, "i1_str", "t1_str", False, ["c1", "c2"]),
    (32, "i2_str", "t1_str", False, ["c4"]),
    (33, "i3_str", "t1_str", False, ["c3", "c1"]),
    (34, "i4_str", "t1_str", False, ["c3", "c4"]),
    (35, "i5_str", "t1_str", False, ["c1", "c2", "c3", "c4"]),
]

# INSERT VERTEX: tag -> [(vid, values in schema order)]
VERTICES = {
    "lookup_tag_1": [(200, [200, 200, 200]), (201, [201, 201, 201]), (202, [202, 202, 202])],
    "lookup_tag_2": [(220, [True, 100, 100.5, True]), (221, [True, 200, 200.5, True]), (222, [True, 300, 300.5, True]),
                     (223, [True, 400, 400.5, True]), (224, [True, 500, 500.5, True]), (225, [True, 600, 600.5, True])],
    "student": [(220, [1, 20]), (221, [2, 22])],
    "teacher": [(220, [1, 30]), (221, [2, 32])],
    "tag_with_str": [(1, [1, "c1_row1", "c2_row1"]), (2, [2, "c1_row2", "c2_row2"]), (3, [3, "abc", "abc"]),
                     (4, [4, "abc", "abc"]), (5, [5, "ab", "cabc"]), (6, [5, "abca", "bc"])],
    "identity": [(1, [19860413, "汉族", "aaa"])],
}
# INSERT EDGE: edge -> [(src, dst, rank, values)]
EDGES = {
    "lookup_edge_1": [(200, 201, 0, [201, 201, 201]), (200, 202, 0, [202, 202, 202])],
    "lookup_edge_2": [(220, 221, 0, [True, 100, 100.5, True]), (220, 222, 0, [True, 200, 200.5, True]),
                      (220, 223, 0, [True, 300, 300.5, True]), (220, 224, 0, [True, 400, 400.5, True]),
                      (220, 225, 0, [True, 500, 500.5, True])],
}

SYNTAX, EXEC = "E_SYNTAX_ERROR", "E_EXECUTION_ERROR"
T2, E2 = "LOOKUP ON lookup_tag_2 WHERE ", "LOOKUP ON lookup_edge_2 WHERE "
ALL6 = [(220,), (221,), (222,), (223,), (224,), (225,)]
E = [(220, 221, 0), (220, 222, 0), (220, 223, 0), (220, 224, 0), (220, 225, 0)]

# (name, query, outcome, names): outcome is a list of rows, or SYNTAX / EXEC; names None: not asserted
CASES = [
    ("sv_bare", "LOOKUP ON lookup_tag_1 WHERE col1 == 200", SYNTAX, None),
    ("sv_none", "LOOKUP ON lookup_tag_1 WHERE lookup_tag_1.col1 == 300", [], None),
    ("sv_one", "LOOKUP ON lookup_tag_1 WHERE lookup_tag_1.col1 == 200", [(200,)], ["VertexID"]),
    ("sv_yield", "LOOKUP ON lookup_tag_1 WHERE lookup_tag_1.col1 == 200 "
     "YIELD lookup_tag_1.col1, lookup_tag_1.col2, lookup_tag_1.col3", [(200, 200, 200, 200)],
     ["VertexID", "lookup_tag_1.col1", "lookup_tag_1.col2", "lookup_tag_1.col3"]),
    ("se_bare", "LOOKUP ON lookup_edge_1 WHERE col1 == 201", SYNTAX, None),
    ("se_none", "LOOKUP ON lookup_edge_1 WHERE lookup_edge_1.col1 == 300", [], None),
    ("se_one", "LOOKUP ON lookup_edge_1 WHERE lookup_edge_1.col1 == 201", [(200, 201, 0)], ["SrcVID", "DstVID", "Ranking"]),
    ("se_yield", "LOOKUP ON lookup_edge_1 WHERE lookup_edge_1.col1 == 201 "
     "YIELD lookup_edge_1.col1, lookup_edge_1.col2, lookup_edge_1.col3", [(200, 201, 0, 201, 201, 201)],
     ["SrcVID", "DstVID", "Ranking", "lookup_edge_1.col1", "lookup_edge_1.col2", "lookup_edge_1.col3"]),
    ("vh_col2", "LOOKUP ON lookup_tag_1 WHERE lookup_tag_1.col2 == 200", [(200,)], None),
    ("vh_no_index", "LOOKUP ON lookup_tag_2 WHERE lookup_tag_2.col1 == true", EXEC, None),
    ("eh_col2", "LOOKUP ON lookup_edge_1 WHERE lookup_edge_1.col2 == 201", [(200, 201, 0)], None),
    ("eh_no_index", "LOOKUP ON lookup_edge_2 WHERE lookup_edge_2.col1 == 200", EXEC, None),
    ("vc_eq", T2 + "lookup_tag_2.col2 == 100", [(220,)], None),
    ("vc_or", T2 + "lookup_tag_2.col2 == 100 OR lookup_tag_2.col2 == 200", SYNTAX, None),
    ("vc_gt", T2 + "lookup_tag_2.col2 > 100", ALL6[1:], None),
    ("vc_ne", T2 + "lookup_tag_2.col2 != 100", ALL6[1:], None),
    ("vc_ge", T2 + "lookup_tag_2.col2 >= 100", ALL6, None),
    ("vc_ge_bool", T2 + "lookup_tag_2.col2 >= 100 AND lookup_tag_2.col4 == true", ALL6, None),
    ("vc_ge_bool_ne", T2 + "lookup_tag_2.col2 >= 100 AND lookup_tag_2.col4 != true", [], None),
    ("vc_between", T2 + "lookup_tag_2.col2 >= 100 AND lookup_tag_2.col2 <= 400", ALL6[:4], None),
    ("vc_dbl_int", T2 + "lookup_tag_2.col3 == 100.5 AND lookup_tag_2.col2 == 100", [(220,)], None),
    ("vc_dbl_int_none", T2 + "lookup_tag_2.col3 == 100.5 AND lookup_tag_2.col2 == 200", [], None),
    ("vc_dbl_gt", T2 + "lookup_tag_2.col3 > 100.5", ALL6[1:], None),
    ("vc_dbl_eq", T2 + "lookup_tag_2.col3 == 100.5", [(220,)], None),
    ("vc_dbl_eq_none", T2 + "lookup_tag_2.col3 == 100.1", [], None),
    ("vc_dbl_between", T2 + "lookup_tag_2.col3 >= 100.5 AND lookup_tag_2.col3 <= 300.5", ALL6[:3], None),
    ("ec_eq", E2 + "lookup_edge_2.col2 == 100", E[:1], None),
    ("ec_or", E2 + "lookup_edge_2.col2 == 100 OR lookup_edge_2.col2 == 200", SYNTAX, None),
    ("ec_gt", E2 + "lookup_edge_2.col2 > 100", E[1:], None),
    ("ec_ne", E2 + "lookup_edge_2.col2 != 100", E[1:], None),
    ("ec_ge", E2 + "lookup_edge_2.col2 >= 100", E, None),
    ("ec_ge_bool", E2 + "lookup_edge_2.col2 >= 100 AND lookup_edge_2.col4 == true", E, None),
    ("ec_ge_bool_ne", E2 + "lookup_edge_2.col2 >= 100 AND lookup_edge_2.col4 != true", [], None),
    ("ec_between", E2 + "lookup_edge_2.col2 >= 100 AND lookup_edge_2.col2 <= 400", E[:4], None),
    ("ec_dbl_int", E2 + "lookup_edge_2.col3 == 100.5 AND lookup_edge_2.col2 == 100", E[:1], None),
    ("ec_dbl_int_none", E2 + "lookup_edge_2.col3 == 100.5 AND lookup_edge_2.col2 == 200", [], None),
    ("ec_dbl_gt", E2 + "lookup_edge_2.col3 > 100.5", E[1:], None),
    ("ec_dbl_eq", E2 + "lookup_edge_2.col3 == 100.5", E[:1], None),
    ("ec_dbl_eq_none", E2 + "lookup_edge_2.col3 == 100.1", [], None),
    ("ec_dbl_between", E2 + "lookup_edge_2.col3 >= 100.5 AND lookup_edge_2.col3 <= 300.5", E[:3], None),
    ("fx_const", T2 + "1 == 1", SYNTAX, None),
    ("fx_const_ne", T2 + "1 != 1", SYNTAX, None),
    ("fx_udf", T2 + "udf_is_in(lookup_tag_2.col2, 100, 200)", SYNTAX, None),
    ("fx_abs_gt", T2 + "lookup_tag_2.col2 > abs(-5)", ALL6, None),
    ("fx_abs_lt", T2 + "lookup_tag_2.col2 < abs(-5)", [], None),
    ("fx_sum_gt", T2 + "lookup_tag_2.col2 > (1 + 2)", ALL6, None),
    ("fx_sum_lt", T2 + "lookup_tag_2.col2 < (1 + 2)", [], None),
    ("fx_bool_ne", T2 + "lookup_tag_2.col4 != (true && true)", [], None),
    ("fx_bool_and", T2 + "lookup_tag_2.col4 == (true && true)", ALL6, None),
    ("fx_bool_or", T2 + "lookup_tag_2.col4 == (true || false)", ALL6, None),
    ("fx_strcasecmp_eq", T2 + 'lookup_tag_2.col4 == strcasecmp("HelLo", "HelLo")', [], None),
    ("fx_strcasecmp_ne", T2 + 'lookup_tag_2.col4 == strcasecmp("HelLo", "hello")', [], None),
    ("fx_both_props", T2 + "lookup_tag_2.col2 != lookup_tag_2.col3", SYNTAX, None),
    ("fx_prop_operand", T2 + "lookup_tag_2.col2 > (lookup_tag_2.col3 - 100)", EXEC, None),
    ("yc_other_tag", "LOOKUP ON student WHERE student.number == 1 YIELD teacher.age", SYNTAX, None),
    ("yc_other_tag_alias", "LOOKUP ON student WHERE student.number == 1 YIELD teacher.age as student_name", SYNTAX, None),
    ("yc_other_tag_where", "LOOKUP ON student WHERE teacher.number == 1 YIELD student.age", SYNTAX, None),
    ("yc_ok", "LOOKUP ON student WHERE student.number == 1 YIELD student.age", [(220, 20)], None),
    ("sf_not_all_fields", "LOOKUP ON tag_with_str WHERE tag_with_str.c1 == 1", EXEC, None),
    ("sf_none", 'LOOKUP ON tag_with_str WHERE tag_with_str.c1 == 1 and tag_with_str.c2 == "ccc"', [], None),
    ("sf_row1", 'LOOKUP ON tag_with_str WHERE tag_with_str.c1 == 1 and tag_with_str.c2 == "c1_row1"', [(1,)], None),
    ("sf_ab", 'LOOKUP ON tag_with_str WHERE tag_with_str.c1 == 5 and tag_with_str.c2 == "ab"', [(5,)], None),
    ("sf_abc", 'LOOKUP ON tag_with_str WHERE tag_with_str.c2 == "abc" and tag_with_str.c3 == "abc"', [(3,), (4,)], None),
    ("sf_three", 'LOOKUP ON tag_with_str WHERE tag_with_str.c1 == 5 and tag_with_str.c2 == "abca" '
     'and tag_with_str.c3 == "bc"', [(6,)], None),
    ("ct_identity", 'lookup on identity where identity.NATION == "汉族" && identity.BIRTHDAY > 19620101 && '
     'identity.BIRTHDAY < 20021231 && identity.BIRTHPLACE_CITY == "bbb"', [], None),
]

LT, LE, GT, GE, EQ, NE = 0, 1, 2, 3, 4, 5
# OptimizerTest / OptimizerWithStringFieldTest: (tag, filters_ as (field, operator), acceptable index names; None:
# findOptimalIndex fails)
OPTIMIZER = [
    ("t1", [("c1", EQ)], ["i1", "i4", "i5"]),
    ("t1", [("c1", EQ), ("c2", GT)], ["i1", "i4", "i5"]),
    ("t1", [("c1", GT), ("c2", EQ)], ["i2"]),
    ("t1", [("c1", GT), ("c2", EQ), ("c3", EQ)], ["i4", "i5"]),
    ("t1", [("c3", GT)], ["i3"]),
    ("t1", [("c3", GT), ("c1", GT)], ["i4", "i5"]),
    ("t1", [("c4", GT)], None),
    ("t1", [("c2", GT), ("c3", GT)], None),
    ("t1", [("c2", GT), ("c1", NE)], ["i2"]),
    ("t1", [("c2", NE)], ["i2"]),
    ("t1_str", [("c1", EQ)], ["i1_str"]),
    ("t1_str", [("c1", EQ), ("c2", GT)], ["i1_str"]),
    ("t1_str", [("c3", EQ)], None),
    ("t1_str", [("c4", EQ)], ["i2_str"]),
    ("t1_str", [("c3", EQ), ("c4", EQ)], ["i4_str"]),
    ("t1_str", [("c3", EQ), ("c1", EQ)], ["i3_str"]),
    ("t1_str", [("c3", EQ), ("c2", EQ), ("c1", EQ)], None),
    # the reference does not clear filters_ before this one: the three above stay in front
    ("t1_str", [("c3", EQ), ("c2", EQ), ("c1", EQ), ("c4", EQ), ("c3", EQ), ("c2", EQ), ("c1", EQ)], ["i5_str"]),
]

# NebulaKeyUtils.h, the comment on encodeInt64
INT_KEYS = [
    (9223372036854775807, b"\xff\xff\xff\xff\xff\xff\xff\xff"),
    (1, b"\x80\x00\x00\x00\x00\x00\x00\x01"),
    (0, b"\x80\x00\x00\x00\x00\x00\x00\x00"),
    (-1, b"\x7f\xff\xff\xff\xff\xff\xff\xff"),
    (-9223372036854775808, b"\x00\x00\x00\x00\x00\x00\x00\x00"),
]
# NebulaKeyUtilsTest encodeVariant / encodeDouble: decodeVariant(encodeVariant(v)) == v
ROUND_TRIP = [1, 0, 9223372036854775807, -9223372036854775808, 1.1, 0.0, 1.7976931348623157e308,
              2.2250738585072014e-308, -1.7976931348623157e308, -(0.000000001 - 2.2250738585072014e-308),
              100.5, 200.5, 300.5, 400.5, 500.5, 600.5]
