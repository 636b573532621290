"""nGQL expression / GO-sentence front end (host side).

The reference parses nGQL with bison (src/parser/parser.yy) and ships WHERE / YIELD expressions
between graphd and storaged in the binary Expression encoding (src/common/filter/Expressions.cpp:
93-116, per-kind encoders :159-199, :450-507, :572-605, :697-711, :779-792, :1002-1021,
:1155-1176, :1249-1268). This module restates the grammar subset the GO path uses
(parser.yy:331-583 expressions, :585-785 GO clauses) and produces that exact encoding, so callers
can hand `Expression.encode()` bytes to the C-ABI (include/nebula_gn.h) the same way graphd hands
`filter` bytes to StorageService.getBound.
"""
from __future__ import annotations

import re
import struct
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

# Expression::Kind (src/common/filter/Expressions.h:386-407)
K_PRIMARY, K_FUNC, K_UNARY, K_CAST, K_ARITH, K_REL, K_LOGIC = 1, 2, 3, 4, 5, 6, 7
K_SRC_PROP, K_EDGE_RANK, K_EDGE_DST, K_EDGE_SRC, K_EDGE_TYPE, K_ALIAS = 8, 9, 10, 11, 12, 13
K_VAR_PROP, K_DST_PROP, K_INPUT_PROP, K_UUID = 14, 15, 16, 17

UNARY_OPS = {"+": 0, "-": 1, "!": 2}                       # UnaryExpression::Operator
ARITH_OPS = {"+": 0, "-": 1, "*": 2, "/": 3, "%": 4, "^": 5}
REL_OPS = {"<": 0, "<=": 1, ">": 2, ">=": 3, "==": 4, "!=": 5, "CONTAINS": 6}
LOGIC_OPS = {"&&": 0, "||": 1, "XOR": 2}
CAST_TYPES = {"int": 0, "string": 1, "double": 2, "bool": 3, "timestamp": 4}   # ColumnType


def _s16(s: str) -> bytes:
    b = s.encode()
    return struct.pack("<H", len(b)) + b


class Expr:
    def encode(self) -> bytes:
        raise NotImplementedError

    def props(self):
        """(kind, alias, prop) of every property reference, in traversal order."""
        return []

    def to_string(self) -> str:
        """Expression::toString (Expressions.cpp): the column name of an un-aliased YIELD column
        (GoExecutor::getResultColumnNames, GoExecutor.cpp:976-987)."""
        raise NotImplementedError


@dataclass
class Prim(Expr):
    value: object
    kind = K_PRIMARY

    def encode(self):
        v = self.value
        if isinstance(v, bool):
            return bytes([K_PRIMARY, 2, 1 if v else 0])
        if isinstance(v, int):
            return bytes([K_PRIMARY, 0]) + struct.pack("<q", v)
        if isinstance(v, float):
            return bytes([K_PRIMARY, 1]) + struct.pack("<d", v)
        return bytes([K_PRIMARY, 3]) + _s16(v)

    def to_string(self):
        v = self.value
        if isinstance(v, bool):
            return "true" if v else "false"
        if isinstance(v, int):
            return str(v)
        if isinstance(v, float):
            return "%.15f" % v
        return v


@dataclass
class Prop(Expr):
    """Alias.prop and relatives: $^.tag.p, $$.tag.p, $-.p, $var.p, e._dst/_src/_rank/_type."""
    kind: int
    ref: str
    alias: str
    prop: str

    def encode(self):
        return bytes([self.kind]) + _s16(self.ref) + _s16(self.alias) + _s16(self.prop)

    def props(self):
        return [(self.kind, self.alias, self.prop)]

    def to_string(self):                                          # Expressions.cpp:118-137
        out = self.ref
        if self.ref not in ("", "$"):
            out += "."
        out += self.alias
        if self.alias:
            out += "."
        return out + self.prop


@dataclass
class Func(Expr):
    name: str
    args: List[Expr]
    kind = K_FUNC

    def encode(self):
        out = bytes([K_FUNC]) + _s16(self.name) + struct.pack("<H", len(self.args))
        return out + b"".join(a.encode() for a in self.args)

    def props(self):
        return [p for a in self.args for p in a.props()]

    def to_string(self):
        return self.name + "(" + ",".join(a.to_string() for a in self.args) + ")"


@dataclass
class Unary(Expr):
    op: int
    operand: Expr
    kind = K_UNARY

    def encode(self):
        return bytes([K_UNARY, self.op]) + self.operand.encode()

    def props(self):
        return self.operand.props()

    def to_string(self):
        return "+-!"[self.op] + "(" + self.operand.to_string() + ")"


@dataclass
class Cast(Expr):
    ctype: int
    operand: Expr
    kind = K_CAST

    def encode(self):
        return bytes([K_CAST, self.ctype]) + self.operand.encode()

    def props(self):
        return self.operand.props()

    def to_string(self):
        return "(" + ("int", "string", "double", "bool", "timestamp")[self.ctype % 5] + ")" + self.operand.to_string()


@dataclass
class Binary(Expr):
    kind: int
    op: int
    left: Expr
    right: Expr

    def encode(self):
        return bytes([self.kind, self.op]) + self.left.encode() + self.right.encode()

    def props(self):
        return self.left.props() + self.right.props()

    def to_string(self):
        names = {K_ARITH: ("+", "-", "*", "/", "%", "^"), K_REL: ("<", "<=", ">", ">=", "==", "!=", " CONTAINS "),
                 K_LOGIC: ("&&", "||", "XOR")}[self.kind]
        o = names[self.op] if self.op < len(names) else "?"
        return "(" + self.left.to_string() + o + self.right.to_string() + ")"


# ------------------------------------------------------------------------------ std::hash
def std_hash_bytes(data: bytes, seed: int = 0xC70F6907) -> int:
    """libstdc++ std::_Hash_bytes (64-bit) — std::hash<std::string> used for NBA vids
    (src/graph/test/TraverseTestBase.h:125) and the hash() function (FunctionManager.cpp:439-465)."""
    mask = (1 << 64) - 1
    mul = (0xC6A4A793 << 32) + 0x5BD1E995

    def shift_mix(v):
        return v ^ (v >> 47)

    n = len(data)
    aligned = n & ~7
    h = (seed ^ (n * mul)) & mask
    for i in range(0, aligned, 8):
        d = int.from_bytes(data[i:i + 8], "little")
        d = (shift_mix((d * mul) & mask) * mul) & mask
        h ^= d
        h = (h * mul) & mask
    if n & 7:
        d = 0
        for b in reversed(data[aligned:]):
            d = (d << 8) + b
        h ^= d
        h = (h * mul) & mask
    h = (shift_mix(h) * mul) & mask
    h = shift_mix(h)
    return h


def to_i64(u: int) -> int:
    u &= (1 << 64) - 1
    return u - (1 << 64) if u >= (1 << 63) else u


def nebula_hash(s: str) -> int:
    return to_i64(std_hash_bytes(s.encode()))


# ------------------------------------------------------------------------------ lexer
_TOKEN = re.compile(r"""
    (?P<ws>\s+)
  | (?P<double>(?:\d+\.\d*|\.\d+)(?:[eE][-+]?\d+)?|\d+[eE][-+]?\d+)
  | (?P<hex>0[xX][0-9a-fA-F]+)
  | (?P<int>\d+)
  | (?P<str>"(?:[^"\\]|\\.)*"|'(?:[^'\\]|\\.)*')
  | (?P<ref>\$\^|\$\$|\$-)
  | (?P<var>\$[A-Za-z_][A-Za-z0-9_]*)
  | (?P<op><=|>=|==|!=|&&|\|\||->|[<>+\-*/%^!(),.@:])
  | (?P<name>[A-Za-z_][A-Za-z0-9_]*)
""", re.X)

KEYWORDS = {"GO", "STEPS", "TO", "FROM", "OVER", "REVERSELY", "BIDIRECT", "WHERE", "YIELD",
            "DISTINCT", "AS", "AND", "OR", "XOR", "NOT", "CONTAINS", "TRUE", "FALSE", "UUID",
            "INT", "DOUBLE", "STRING", "BOOL", "TIMESTAMP"}


@dataclass
class Tok:
    kind: str
    text: str


def tokenize(src: str) -> List[Tok]:
    out, pos = [], 0
    while pos < len(src):
        m = _TOKEN.match(src, pos)
        if not m:
            raise SyntaxError(f"bad token at {src[pos:pos + 20]!r}")
        pos = m.end()
        k = m.lastgroup
        if k == "ws":
            continue
        t = m.group(k)
        if k == "name" and t.upper() in KEYWORDS:
            out.append(Tok("kw", t.upper()))
        else:
            out.append(Tok(k, t))
    out.append(Tok("eof", ""))
    return out


def _unescape(s: str) -> str:
    body = s[1:-1]
    return re.sub(r"\\(.)", lambda m: {"n": "\n", "t": "\t", "r": "\r"}.get(m.group(1), m.group(1)), body)


class Parser:
    def __init__(self, src: str):
        self.toks = tokenize(src)
        self.i = 0

    # helpers
    def peek(self, k=0) -> Tok:
        return self.toks[min(self.i + k, len(self.toks) - 1)]

    def take(self) -> Tok:
        t = self.toks[self.i]
        self.i += 1
        return t

    def accept(self, kind, text=None) -> Optional[Tok]:
        t = self.peek()
        if t.kind == kind and (text is None or t.text == text):
            return self.take()
        return None

    def expect(self, kind, text=None) -> Tok:
        t = self.accept(kind, text)
        if t is None:
            raise SyntaxError(f"expected {text or kind}, got {self.peek().text!r}")
        return t

    def is_op(self, text):
        t = self.peek()
        return t.kind == "op" and t.text == text

    def is_kw(self, text):
        t = self.peek()
        return t.kind == "kw" and t.text == text

    def label(self) -> str:
        t = self.peek()
        if t.kind == "name" or (t.kind == "kw" and t.text not in ("AND", "OR", "XOR", "NOT", "CONTAINS")):
            self.take()
            return t.text if t.kind == "name" else t.text.lower()
        raise SyntaxError(f"expected a name, got {t.text!r}")

    # expression := logic_xor                                   parser.yy:574-583
    def expression(self) -> Expr:
        e = self.logic_or()
        while self.is_kw("XOR"):
            self.take()
            e = Binary(K_LOGIC, LOGIC_OPS["XOR"], e, self.logic_or())
        return e

    def logic_or(self):
        e = self.logic_and()
        while self.is_op("||") or self.is_kw("OR"):
            self.take()
            e = Binary(K_LOGIC, LOGIC_OPS["||"], e, self.logic_and())
        return e

    def logic_and(self):
        e = self.equality()
        while self.is_op("&&") or self.is_kw("AND"):
            self.take()
            e = Binary(K_LOGIC, LOGIC_OPS["&&"], e, self.equality())
        return e

    def equality(self):
        e = self.relational()
        while self.is_op("==") or self.is_op("!="):
            op = self.take().text
            e = Binary(K_REL, REL_OPS[op], e, self.relational())
        return e

    def relational(self):
        e = self.additive()
        while True:
            t = self.peek()
            if t.kind == "op" and t.text in ("<", ">", "<=", ">="):
                self.take()
                e = Binary(K_REL, REL_OPS[t.text], e, self.additive())
            elif t.kind == "kw" and t.text == "CONTAINS":
                self.take()
                e = Binary(K_REL, REL_OPS["CONTAINS"], e, self.additive())
            else:
                return e

    def additive(self):
        e = self.multiplicative()
        while self.is_op("+") or self.is_op("-"):
            op = self.take().text
            e = Binary(K_ARITH, ARITH_OPS[op], e, self.multiplicative())
        return e

    def multiplicative(self):
        e = self.arith_xor()
        while self.is_op("*") or self.is_op("/") or self.is_op("%"):
            op = self.take().text
            e = Binary(K_ARITH, ARITH_OPS[op], e, self.arith_xor())
        return e

    def arith_xor(self):
        e = self.unary()
        while self.is_op("^"):
            self.take()
            e = Binary(K_ARITH, ARITH_OPS["^"], e, self.unary())
        return e

    def unary(self):                                              # parser.yy:471-485
        if self.is_op("+"):
            self.take()
            return Unary(UNARY_OPS["+"], self.unary())
        if self.is_op("!") or self.is_kw("NOT"):
            self.take()
            return Unary(UNARY_OPS["!"], self.unary())
        if self.is_op("(") and self.peek(1).kind == "kw" and self.peek(1).text.lower() in CAST_TYPES \
                and self.peek(2).kind == "op" and self.peek(2).text == ")":
            self.take()
            ct = CAST_TYPES[self.take().text.lower()]
            self.take()
            return Cast(ct, self.unary())
        return self.primary()

    def primary(self):                                            # parser.yy:331-344
        if self.is_op("-"):
            self.take()
            t = self.peek()
            if t.kind in ("int", "hex"):
                self.take()
                return Prim(-int(t.text, 0))
            return Unary(UNARY_OPS["-"], self.base())
        return self.base()

    def base(self):                                               # parser.yy:346-382
        t = self.peek()
        if t.kind in ("int", "hex"):
            self.take()
            v = int(t.text, 0)
            if v > (1 << 63) - 1:
                raise SyntaxError("integer out of range")
            return Prim(v)
        if t.kind == "double":
            self.take()
            return Prim(float(t.text))
        if t.kind == "str":
            self.take()
            return Prim(_unescape(t.text))
        if t.kind == "kw" and t.text in ("TRUE", "FALSE"):
            self.take()
            return Prim(t.text == "TRUE")
        if t.kind == "ref":
            self.take()
            if t.text == "$-":
                if self.accept("op", "."):
                    if self.accept("op", "*"):
                        return Prop(K_INPUT_PROP, "$-", "", "*")
                    return Prop(K_INPUT_PROP, "$-", "", self.label())
                return Prop(K_INPUT_PROP, "$-", "", "id")
            self.expect("op", ".")
            tag = self.label()
            self.expect("op", ".")
            prop = self.label()
            return Prop(K_SRC_PROP if t.text == "$^" else K_DST_PROP, t.text, tag, prop)
        if t.kind == "var":
            self.take()
            name = t.text[1:]
            if self.accept("op", "."):
                if self.accept("op", "*"):
                    return Prop(K_VAR_PROP, "$", name, "*")
                return Prop(K_VAR_PROP, "$", name, self.label())
            return Prop(K_VAR_PROP, "$", name, "id")
        if self.is_op("("):
            self.take()
            e = self.expression()
            self.expect("op", ")")
            return e
        if t.kind == "kw" and t.text == "UUID":
            raise SyntaxError("uuid() needs the storage UUID service and is not supported")
        if t.kind in ("name", "kw"):
            name = self.label()
            if self.is_op("("):                                   # function call
                self.take()
                args = []
                if not self.is_op(")"):
                    args.append(self.expression())
                    while self.accept("op", ","):
                        args.append(self.expression())
                self.expect("op", ")")
                return Func(name, args)
            if self.is_op("."):                                   # alias_ref_expression
                self.take()
                prop = self.label()
                special = {"_type": K_EDGE_TYPE, "_src": K_EDGE_SRC, "_dst": K_EDGE_DST, "_rank": K_EDGE_RANK}
                if prop in special:
                    return Prop(special[prop], "", name, prop)
                return Prop(K_ALIAS, "", name, prop)
            return Prim(name)                                     # bare name_label -> string
        raise SyntaxError(f"unexpected token {t.text!r}")


def parse_expr(src: str) -> Expr:
    p = Parser(src)
    e = p.expression()
    p.expect("eof")
    return e


def eval_const(e: Expr) -> object:
    """Evaluate a constant FROM-list item the way GoExecutor::prepareFrom does (integers, hash())."""
    if isinstance(e, Prim):
        return e.value
    if isinstance(e, Func) and e.name == "hash" and len(e.args) == 1:
        v = eval_const(e.args[0])
        if isinstance(v, str):
            return nebula_hash(v)
        if isinstance(v, bool):
            return int(v)
        if isinstance(v, int):
            return v                       # std::hash<int64_t> is the identity in libstdc++
        raise ValueError("hash() of a double is not supported in FROM")
    if isinstance(e, Unary) and e.op == UNARY_OPS["-"]:
        return -eval_const(e.operand)
    raise ValueError("FROM accepts integer literals and hash(...) only")


# ------------------------------------------------------------------------------ GO sentence
FORWARD, REVERSELY, BIDIRECT = 0, 1, 2


@dataclass
class YieldCol:
    expr: Expr
    alias: str = ""


@dataclass
class GoSentence:
    """Parsed `GO [M TO] N STEPS FROM ... OVER ... [WHERE ...] [YIELD [DISTINCT] ...]`."""
    record_from: int = 1
    record_to: int = 1
    vids: List[int] = field(default_factory=list)
    over: List[Tuple[str, str]] = field(default_factory=list)     # (edge name, alias or "")
    over_all: bool = False
    direction: int = FORWARD
    where: Optional[Expr] = None
    distinct: bool = False
    yields: List[YieldCol] = field(default_factory=list)
    # FROM $-.col / $var.col (GoExecutor fromType_, GoExecutor.cpp:149-180): 0 literal vids, 1 $-, 2 $var
    from_type: int = 0
    from_var: str = ""
    from_col: str = ""

    def column_names(self, edge_names: Sequence[str] = ()) -> List[str]:
        """getResultColumnNames (GoExecutor.cpp:976-987): alias, else the expression text. OVER *
        without YIELD yields `<edge>._dst' per edge of the space (`edge_names', schema order)."""
        if not self.yields and self.over_all:
            return [n + "._dst" for n in edge_names]
        return [y.alias if y.alias else y.expr.to_string() for y in self.yields]


def parse_go(src: str) -> GoSentence:
    p = Parser(src)
    s = GoSentence()
    p.expect("kw", "GO")
    # step_clause (parser.yy:610-625)
    if p.peek().kind == "int":
        a = int(p.take().text)
        if p.accept("kw", "TO"):
            b = int(p.expect("int").text)
            if a > b:
                raise SyntaxError("Invalid step range")
            s.record_from, s.record_to = a, b
        else:
            s.record_from = s.record_to = a
        p.expect("kw", "STEPS")
    # from_clause (:626-656)
    p.expect("kw", "FROM")
    t = p.peek()
    if t.kind == "ref" and t.text == "$-" or t.kind == "var":      # from_clause: input_ref / var_ref
        p.take()
        p.expect("op", ".")
        col = "*" if p.accept("op", "*") else p.label()
        s.from_type, s.from_var, s.from_col = (1, "", col) if t.kind == "ref" else (2, t.text[1:], col)
    while s.from_type == 0:
        if p.peek().kind in ("ref", "var"):
            raise SyntaxError("FROM accepts vids, $-.col or $var.col")
        e = p.primary() if p.is_op("-") or p.is_op("+") else p.base()
        if isinstance(e, Unary) and e.op == UNARY_OPS["+"]:
            e = e.operand
        v = eval_const(e)
        if isinstance(v, bool) or not isinstance(v, int):
            raise SyntaxError("Vertex ID should be of type integer")
        s.vids.append(v)
        if not p.accept("op", ","):
            break
    # over_clause (:681-733)
    p.expect("kw", "OVER")
    if p.accept("op", "*"):
        s.over_all = True
    else:
        while True:
            name = p.label()
            alias = ""
            if p.accept("kw", "AS"):
                alias = p.label()
            s.over.append((name, alias))
            if not p.accept("op", ","):
                break
    if p.accept("kw", "REVERSELY"):
        s.direction = REVERSELY
    elif p.accept("kw", "BIDIRECT"):
        s.direction = BIDIRECT
    if p.accept("kw", "WHERE"):
        s.where = p.expression()
    if p.accept("kw", "YIELD"):
        if p.accept("kw", "DISTINCT"):
            s.distinct = True
        while True:
            e = p.expression()
            alias = ""
            if p.accept("kw", "AS"):
                alias = p.label()
            s.yields.append(YieldCol(e, alias))
            if not p.accept("op", ","):
                break
    else:                                                         # parser.yy:592-604
        for name, _ in s.over:
            s.yields.append(YieldCol(Prop(K_EDGE_DST, "", name, "_dst")))
    p.expect("eof")
    return s


# ------------------------------------------------------------------------------ GROUP BY sentence
# agg_function (parser.yy:318-329); the keywords are case-insensitive in the scanner
AGG_FUNCS = ("COUNT", "COUNT_DISTINCT", "SUM", "AVG", "MAX", "MIN", "STD", "BIT_AND", "BIT_OR", "BIT_XOR")


@dataclass
class AggCol:
    """A yield_column of a GROUP BY sentence (parser.yy:763-792): an expression, an optional aggregate
    function name around it and an optional alias. `*' is PrimaryExpression("*")."""
    expr: Expr
    alias: str = ""
    fun: str = ""

    def to_string(self) -> str:                                   # YieldColumn::toString, Clauses.cpp:194-207
        return self.fun + "(" + self.expr.to_string() + ")" if self.fun else self.expr.to_string()


@dataclass
class GroupBySentence:
    """Parsed `GROUP BY <cols> YIELD <cols>` (group_by_sentence, parser.yy:1013-1020)."""
    groups: List[AggCol] = field(default_factory=list)
    yields: List[AggCol] = field(default_factory=list)

    def column_names(self) -> List[str]:
        """GroupByExecutor::getResultColumnNames (GroupByExecutor.cpp:334-345)."""
        return [y.alias if y.alias else y.to_string() for y in self.yields]


def _agg_columns(p: Parser, stop: str = "") -> List[AggCol]:
    cols = []
    while p.peek().kind != "eof" and not (stop and p.is_kw(stop)):
        t = p.peek()
        fun = ""
        if t.kind == "name" and t.text.upper() in AGG_FUNCS and p.peek(1).kind == "op" and p.peek(1).text == "(":
            fun = p.take().text.upper()
            p.take()
            if p.is_op("*") and p.peek(1).kind == "op" and p.peek(1).text == ")":
                p.take()
                e = Prim("*")
            else:
                e = p.expression()
            p.expect("op", ")")
        else:
            e = p.expression()
        alias = p.label() if p.accept("kw", "AS") else ""
        cols.append(AggCol(e, alias, fun))
        if not p.accept("op", ","):
            break
    return cols


def is_group_by(src: str) -> bool:
    return re.match(r"\s*GROUP\s+BY\b", src, re.I) is not None


def parse_group_by(src: str) -> GroupBySentence:
    p = Parser(src)
    for word in ("GROUP", "BY"):
        t = p.take()
        if t.kind != "name" or t.text.upper() != word:
            raise SyntaxError(f"expected {word}, got {t.text!r}")
    s = GroupBySentence()
    s.groups = _agg_columns(p, "YIELD")
    if p.accept("kw", "YIELD"):
        s.yields = _agg_columns(p)
    p.expect("eof")
    return s


# ------------------------------------------------------------------------------ YIELD sentence
@dataclass
class YieldSentence:
    """Parsed `YIELD <yield_columns> [WHERE <expr>]` (yield_sentence, parser.yy:798-804). The grammar has no
    DISTINCT here: `YIELD DISTINCT ...` is a syntax error."""
    yields: List[AggCol] = field(default_factory=list)
    where: Optional[Expr] = None

    def column_names(self) -> List[str]:
        """YieldExecutor::prepareYield (YieldExecutor.cpp:85-89): the alias, else expr->toString()."""
        return [y.alias if y.alias else y.expr.to_string() for y in self.yields]


def is_yield(src: str) -> bool:
    return re.match(r"\s*YIELD\b", src, re.I) is not None


def parse_yield(src: str) -> YieldSentence:
    p = Parser(src)
    p.expect("kw", "YIELD")
    if p.is_kw("DISTINCT"):
        raise SyntaxError("syntax error near `DISTINCT'")
    s = YieldSentence()
    s.yields = _agg_columns(p, "WHERE")
    if not s.yields:
        raise SyntaxError("syntax error near `YIELD'")
    if p.i and p.toks[p.i - 1].kind == "op" and p.toks[p.i - 1].text == ",":
        raise SyntaxError("syntax error near `,'")
    if p.accept("kw", "WHERE"):
        s.where = p.expression()
    p.expect("eof")
    return s


# ------------------------------------------------------------------------------ ORDER BY / LIMIT sentences
@dataclass
class OrderBySentence:
    """Parsed `ORDER BY <factor>[, <factor>...]` (order_by_sentence, parser.yy:819-859): (input column
    name, descending) per factor. A factor is `$-.col` or a bare label, then ASC (the default) or DESC."""
    factors: List[Tuple[str, bool]] = field(default_factory=list)


@dataclass
class LimitSentence:
    """Parsed `LIMIT n` / `LIMIT off, n` / `LIMIT a OFFSET b` (limit_sentence, parser.yy:996-1011). The
    grammar builds LimitSentence($2, $4) for the OFFSET form too: a is the offset and b the count."""
    offset: int = 0
    count: int = 0


def is_order_by(src: str) -> bool:
    return re.match(r"\s*ORDER\s+BY\b", src, re.I) is not None


def is_limit(src: str) -> bool:
    return re.match(r"\s*LIMIT\b", src, re.I) is not None


def _word(p: Parser, *words: str) -> Optional[str]:
    t = p.peek()
    if t.kind == "name" and t.text.upper() in words:
        p.take()
        return t.text.upper()
    return None


def parse_order_by(src: str) -> OrderBySentence:
    p = Parser(src)
    for word in ("ORDER", "BY"):
        if _word(p, word) is None:
            raise SyntaxError(f"expected {word}, got {p.peek().text!r}")
    s = OrderBySentence()
    while True:
        t = p.peek()
        if t.kind == "ref" and t.text == "$-":                    # input_ref_expression (parser.yy:384-395)
            p.take()
            if p.accept("op", "."):
                col = "*" if p.accept("op", "*") else p.label()
            else:
                col = "id"
        elif t.kind == "name" and t.text.upper() not in ("ASC", "DESC"):
            col = p.take().text                                   # LABEL
        else:
            raise SyntaxError(f"expected an order factor, got {t.text!r}")
        s.factors.append((col, _word(p, "ASC", "DESC") == "DESC"))
        if not p.accept("op", ","):
            break
    p.expect("eof")
    return s


def parse_limit(src: str) -> LimitSentence:
    p = Parser(src)
    if _word(p, "LIMIT") is None:
        raise SyntaxError(f"expected LIMIT, got {p.peek().text!r}")

    def integer() -> int:                                         # INTEGER: no sign in the grammar
        t = p.peek()
        if t.kind not in ("int", "hex"):
            raise SyntaxError(f"expected an integer, got {t.text!r}")
        p.take()
        v = int(t.text, 0)
        if v > (1 << 63) - 1:
            raise SyntaxError("integer out of range")
        return v
    a = integer()
    s = LimitSentence(0, a)
    if p.accept("op", ",") or _word(p, "OFFSET") is not None:
        s = LimitSentence(a, integer())
    p.expect("eof")
    return s


# ----------------------------------------------------------------------------- set sentences
# set_sentence (parser.yy:1316-1331): piped sentences joined by UNION [ALL | DISTINCT], INTERSECT and MINUS, one
# priority, left-associative, looser than `|`; parentheses nest a set sentence as a traverse sentence. A bare UNION
# is DISTINCT (parser.yy:1319-1323 call setDistinct()).
SET_OPS = ("UNION ALL", "UNION", "INTERSECT", "MINUS")


def split_set(src: str) -> Tuple[List[str], List[str]]:
    """(operands, operators) of a set sentence, split at the operator keywords outside quotes and parentheses:
    n + 1 operand texts (piped sentences) and n operators out of SET_OPS, "UNION" meaning UNION DISTINCT. No
    operator: ([src], []). An operand without text is a SyntaxError, as in the grammar."""
    def word_at(i):
        m = re.match(r"[A-Za-z_][A-Za-z_0-9]*", src[i:])
        return m.group(0) if m else ""
    operands, ops, depth, quote, start, i = [], [], 0, None, 0, 0
    while i < len(src):
        ch = src[i]
        if quote:
            if ch == "\\":
                i += 1
            elif ch == quote:
                quote = None
        elif ch in "\"'":
            quote = ch
        elif ch == "(":
            depth += 1
        elif ch == ")":
            depth -= 1
        elif depth == 0 and (ch.isalpha() or ch == "_"):
            w = word_at(i)
            prev = src[i - 1] if i else " "
            if w.upper() in ("UNION", "INTERSECT", "MINUS") and not (prev.isalnum() or prev in "_.$@"):
                op, end = w.upper(), i + len(w)
                if op == "UNION":
                    m = re.match(r"\s+(ALL|DISTINCT)\b", src[end:], re.I)
                    if m:
                        end += m.end()
                        if m.group(1).upper() == "ALL":
                            op = "UNION ALL"
                operands.append(src[start:i])
                ops.append(op)
                start = i = end
                continue
            i += max(len(w), 1)
            continue
        i += 1
    operands.append(src[start:])
    if ops and any(not o.strip() for o in operands):
        raise SyntaxError("syntax error near `%s'" % ops[0])
    return operands, ops


def is_set(src: str) -> bool:
    """The text holds a set operator outside quotes and parentheses."""
    try:
        return bool(split_set(src)[1])
    except SyntaxError:
        return True


# ----------------------------------------------------------------------------- FIND PATH sentence
# find_path_sentence (parser.yy:946-994): FIND SHORTEST | ALL | NOLOOP PATH from_clause to_clause over_clause
# [UPTO n STEPS]. FindPathSentence(isShortest, isNoLoop): SHORTEST is (true, true), ALL (false, false), NOLOOP
# (false, true). FIND, SHORTEST, ALL, NOLOOP, PATH and UPTO are matched as words (_word), not lexed as keywords,
# so GO texts lex as before.
PATH_KINDS = ("SHORTEST", "ALL", "NOLOOP")


@dataclass
class FindPathSentence:
    kind: str = "SHORTEST"
    from_vids: List[int] = field(default_factory=list)
    from_type: int = 0                                            # 0 literal vids, 1 $-.col, 2 $var.col (as GoSentence)
    from_var: str = ""
    from_col: str = ""
    to_vids: List[int] = field(default_factory=list)
    to_type: int = 0
    to_var: str = ""
    to_col: str = ""
    over: List[Tuple[str, str]] = field(default_factory=list)     # (edge name, alias or "")
    over_all: bool = False
    direction: int = FORWARD
    upto: int = 5                                                 # find_path_upto_clause: %empty is StepClause(5)

    @property
    def shortest(self) -> bool:
        return self.kind == "SHORTEST"

    @property
    def no_loop(self) -> bool:
        return self.kind in ("SHORTEST", "NOLOOP")


def is_find_path(src: str) -> bool:
    return re.match(r"\s*FIND\b", src, re.I) is not None


def _vertices(p: Parser):
    """vid_list | vid_ref_expression (from_clause / to_clause): (vids, type, var, col)."""
    t = p.peek()
    if t.kind == "ref" and t.text == "$-" or t.kind == "var":
        p.take()
        p.expect("op", ".")
        col = "*" if p.accept("op", "*") else p.label()
        return ([], 1, "", col) if t.kind == "ref" else ([], 2, t.text[1:], col)
    vids = []
    while True:
        if p.peek().kind in ("ref", "var"):
            raise SyntaxError("FROM / TO accept vids, $-.col or $var.col")
        e = p.primary() if p.is_op("-") or p.is_op("+") else p.base()
        if isinstance(e, Unary) and e.op == UNARY_OPS["+"]:
            e = e.operand
        v = eval_const(e)
        if isinstance(v, bool) or not isinstance(v, int):
            raise SyntaxError("Vertex ID should be of type integer")
        vids.append(v)
        if not p.accept("op", ","):
            return vids, 0, "", ""


def parse_find_path(src: str) -> FindPathSentence:
    p = Parser(src)
    if _word(p, "FIND") is None:
        raise SyntaxError(f"expected FIND, got {p.peek().text!r}")
    kind = _word(p, *PATH_KINDS)
    if kind is None:
        raise SyntaxError(f"expected SHORTEST, ALL or NOLOOP, got {p.peek().text!r}")
    if _word(p, "PATH") is None:
        raise SyntaxError(f"expected PATH, got {p.peek().text!r}")
    s = FindPathSentence(kind=kind)
    p.expect("kw", "FROM")
    s.from_vids, s.from_type, s.from_var, s.from_col = _vertices(p)
    p.expect("kw", "TO")
    s.to_vids, s.to_type, s.to_var, s.to_col = _vertices(p)
    p.expect("kw", "OVER")
    if p.accept("op", "*"):
        s.over_all = True
    else:
        while True:
            name = p.label()
            alias = p.label() if p.accept("kw", "AS") else ""
            s.over.append((name, alias))
            if not p.accept("op", ","):
                break
    if p.accept("kw", "REVERSELY"):
        s.direction = REVERSELY
    elif p.accept("kw", "BIDIRECT"):
        s.direction = BIDIRECT
    if _word(p, "UPTO") is not None:
        t = p.peek()
        if t.kind not in ("int", "hex"):
            raise SyntaxError(f"expected an integer, got {t.text!r}")
        p.take()
        s.upto = int(t.text, 0)
        if s.upto > (1 << 63) - 1:
            raise SyntaxError("integer out of range")
        p.expect("kw", "STEPS")
    p.expect("eof")
    return s


# ----------------------------------------------------------------------------- FETCH sentences
# fetch_vertices_sentence / fetch_edges_sentence (parser.yy:861-944): FETCH PROP ON <labels> | * followed by a vid
# list, `$-.col` / `$var.col`, edge keys `src -> dst[@rank]` or an edge key reference `$-.s -> $-.d[@$-.r]`, then an
# optional yield_clause. FETCH, PROP and ON are matched as words (_word), so GO texts lex as before. Whether the
# labels name tags or one edge type is decided by what follows them: an `->` makes it a FETCH on edges.
@dataclass
class FetchVerticesSentence:
    tags: List[str] = field(default_factory=list)                 # ON order; ["*"]: every tag of the space
    vids: List[Expr] = field(default_factory=list)                # constant vid expressions (from_type 0)
    from_type: int = 0                                            # 0 literal vids, 1 $-.col, 2 $var.col (as GoSentence)
    from_var: str = ""
    from_col: str = ""
    has_yield: bool = False
    distinct: bool = False
    yields: List[AggCol] = field(default_factory=list)


@dataclass
class FetchEdgesSentence:
    edges: List[str] = field(default_factory=list)                # fetch_labels; the executor takes exactly one
    keys: List[Tuple[Expr, Expr, int]] = field(default_factory=list)   # (src expr, dst expr, rank) (from_type 0)
    from_type: int = 0
    src_ref: Optional[Prop] = None                                # edge_key_ref: $-.s -> $-.d [@ $-.r], or $var's
    dst_ref: Optional[Prop] = None
    rank_ref: Optional[Prop] = None
    has_yield: bool = False
    distinct: bool = False
    yields: List[AggCol] = field(default_factory=list)

    def ref_string(self) -> str:                                  # EdgeKeyRef::toString
        out = self.src_ref.to_string() + "->" + self.dst_ref.to_string()
        return out + ("@" + self.rank_ref.to_string() if self.rank_ref is not None else "")


def is_fetch(src: str) -> bool:
    return re.match(r"\s*FETCH\b", src, re.I) is not None


def _fetch_vid(p: Parser) -> Expr:
    """vid (parser.yy:646-656): unary_integer | function_call_expression | uuid_expression."""
    t = p.peek()
    if t.kind in ("ref", "var"):
        raise SyntaxError(f"syntax error near `{t.text}'")
    e = p.primary() if p.is_op("-") or p.is_op("+") else p.base()
    if isinstance(e, Unary) and e.op == UNARY_OPS["+"] and isinstance(e.operand, Prim):
        e = e.operand
    if isinstance(e, Prim) and isinstance(e.value, int) and not isinstance(e.value, bool):
        return e
    if isinstance(e, Func):
        return e
    raise SyntaxError(f"syntax error near `{t.text}'")


def _fetch_ref(p: Parser) -> Prop:
    """input_ref_expression | var_ref_expression"""
    t = p.peek()
    if not (t.kind == "ref" and t.text == "$-" or t.kind == "var"):
        raise SyntaxError(f"syntax error near `{t.text}'")
    return p.base()


def parse_fetch(src: str):
    p = Parser(src)
    for word in ("FETCH", "PROP", "ON"):
        if _word(p, word) is None:
            raise SyntaxError(f"expected {word}, got {p.peek().text!r}")
    labels = []
    if p.accept("op", "*"):
        labels = ["*"]
    else:
        while True:
            labels.append(p.label())
            # `ON a, b 1, 2`: a comma continues the labels only while a label follows it
            if p.is_op(",") and p.peek(1).kind in ("name", "kw") and not (p.peek(2).kind == "op" and p.peek(2).text == "("):
                p.take()
                continue
            break
    t = p.peek()
    s = None
    if t.kind == "ref" and t.text == "$-" or t.kind == "var":
        first = _fetch_ref(p)
        if p.accept("op", "->"):
            if labels == ["*"]:
                raise SyntaxError("syntax error near `->'")
            s = FetchEdgesSentence(edges=labels, from_type=1 if first.kind == K_INPUT_PROP else 2, src_ref=first)
            s.dst_ref = _fetch_ref(p)
            if p.accept("op", "@"):
                s.rank_ref = _fetch_ref(p)
            for r in (s.dst_ref, s.rank_ref):                     # the grammar has no mixed $- / $var key
                if r is not None and r.kind != first.kind:
                    raise SyntaxError("syntax error near `%s'" % r.to_string())
        else:
            s = FetchVerticesSentence(tags=labels, from_type=1 if first.kind == K_INPUT_PROP else 2,
                                      from_var=first.alias if first.kind == K_VAR_PROP else "", from_col=first.prop)
    else:
        first = _fetch_vid(p)
        if p.is_op("->"):
            if labels == ["*"]:
                raise SyntaxError("syntax error near `->'")
            s = FetchEdgesSentence(edges=labels)
            e = first
            while True:
                p.expect("op", "->")
                d = _fetch_vid(p)
                rank = 0
                if p.accept("op", "@"):
                    neg = False
                    if p.accept("op", "-"):
                        neg = True
                    else:
                        p.accept("op", "+")
                    tk = p.peek()
                    if tk.kind not in ("int", "hex"):
                        raise SyntaxError(f"expected an integer, got {tk.text!r}")
                    p.take()
                    rank = -int(tk.text, 0) if neg else int(tk.text, 0)
                s.keys.append((e, d, rank))
                if not p.accept("op", ","):
                    break
                e = _fetch_vid(p)
        else:
            s = FetchVerticesSentence(tags=labels, vids=[first])
            while p.accept("op", ","):
                s.vids.append(_fetch_vid(p))
    if p.accept("kw", "YIELD"):
        s.has_yield = True
        if p.accept("kw", "DISTINCT"):
            s.distinct = True
        s.yields = _agg_columns(p)
        if not s.yields:
            raise SyntaxError("syntax error near `YIELD'")
    p.expect("eof")
    return s


# ----------------------------------------------------------------------------- LOOKUP sentence
# lookup_sentence (parser.yy): LOOKUP ON <name> lookup_where_clause [yield_clause]. LOOKUP is matched as a word
# (_word), so every other text lexes as before. The WHERE of a LOOKUP has no bare column names: `WHERE col1 == 200`
# is the reference's syntax error (a name stands only before `.` or `(`).
@dataclass
class LookupSentence:
    from_: str = ""
    where: Optional[Expr] = None                                  # None: no WHERE ("Where clause is required")
    has_yield: bool = False
    yields: List[AggCol] = field(default_factory=list)


def is_lookup(src: str) -> bool:
    return re.match(r"\s*LOOKUP\b", src, re.I) is not None


def parse_lookup(src: str) -> LookupSentence:
    p = Parser(src)
    for word in ("LOOKUP", "ON"):
        if _word(p, word) is None:
            raise SyntaxError(f"expected {word}, got {p.peek().text!r}")
    s = LookupSentence(from_=p.label())
    if p.accept("kw", "WHERE"):
        start = p.i
        s.where = p.expression()
        for j in range(start, p.i):
            t, nxt, prev = p.toks[j], p.toks[j + 1], p.toks[j - 1]
            if t.kind == "name" and not (nxt.kind == "op" and nxt.text in (".", "(")) \
                    and not (prev.kind == "op" and prev.text == "."):
                raise SyntaxError(f"syntax error near `{t.text}'")
    if p.accept("kw", "YIELD"):
        s.has_yield = True
        s.yields = _agg_columns(p)
        if not s.yields:
            raise SyntaxError("syntax error near `YIELD'")
    p.expect("eof")
    return s
