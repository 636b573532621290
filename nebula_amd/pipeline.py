"""Pipes and variables around GO: `GO ... | GO FROM $-.col ...` and `$v = GO ...; GO FROM $v.col ...`.

Host-side restatement of the graphd pieces that chain GO sentences (the traversal itself runs in the
library, include/nebula_gn.h ngx_go with input_* set):
  - PipeExecutor (src/graph/PipeExecutor.cpp:21-130): the left sentence's InterimResult feeds the
    right one; `A | (B | C)` nests (parser.yy:1298-1314);
  - AssignmentExecutor / VariableHolder: `$v = <sentence>` keeps the result under the name;
    SequentialSentences (parser.yy:2054-2070) run `;`-separated sentences in order, the last one's
    result is the response;
  - GoExecutor::setupInterimResult (GoExecutor.cpp:990-1068): the interim schema takes each
    column's calculateExprType, or for UNKNOWN the variant type of the first record;
  - YieldClauseWrapper::prepare (TraverseExecutor.cpp:344-392): `$-.*` / `$v.*` in YIELD expands to
    every input column.
  - GroupByExecutor (src/graph/GroupByExecutor.cpp): `... | GROUP BY <cols> YIELD <aggregates>` over the
    left side's interim result (nebula_amd/groupby.py).
  - OrderByExecutor / LimitExecutor (src/graph/OrderByExecutor.cpp, LimitExecutor.cpp): `... | ORDER BY
    <factors>` and `... | LIMIT [off,] n` over the left side's interim result (nebula_amd/orderby.py), when
    the caller opts in with order_limit=True.
  - A head `GO | GROUP BY | [ORDER BY |] LIMIT` runs in one device call where the backend has it
    (ngx_go_group_order_by; Pipeline._go_group_order_by), also under order_limit=True.
  - SetExecutor (src/graph/SetExecutor.cpp): `A UNION [ALL | DISTINCT] B`, `A INTERSECT B`, `A MINUS B` over
    piped sentences (nebula_amd/setop.py), when the caller opts in with set_ops=True; two plain GO operands run
    with the operator in one device call where the backend has it (ngx_go_set; Pipeline._go_set).
  - FindPathExecutor (src/graph/FindPathExecutor.cpp): `FIND SHORTEST | ALL | NOLOOP PATH FROM ... TO ... OVER ...
    [UPTO n STEPS]` (nebula_amd/findpath.py), when the caller opts in with find_path=True; FIND SHORTEST PATH runs
    in one device call where the backend has it (ngx_find_path; Pipeline._find_path). It hands no result on: a
    sentence piped behind it runs without input.
  - FetchVerticesExecutor / FetchEdgesExecutor (src/graph/FetchVerticesExecutor.cpp, FetchEdgesExecutor.cpp): `FETCH
    PROP ON <tags> | * <vids> | $-.col | $var.col` and `FETCH PROP ON <edge> <src> -> <dst>[@rank] | $-.s -> $-.d`
    (nebula_amd/fetch.py), when the caller opts in with fetch=True and hands the space's schemas (catalog=). It
    calls onResult_: its rows feed the sentence piped behind it. The key lookup and the property gather run in one
    device call where the backend has it (ngx_fetch; behind a plain head GO, ngx_go_fetch; Pipeline._fetch).
  - LookupExecutor (src/graph/LookupExecutor.cpp): `LOOKUP ON <tag|edge> WHERE ... [YIELD ...]`
    (nebula_amd/lookup.py), when the caller opts in with lookup=True and hands the space's indexes
    (indexes=[lookup.Index, ...]). feedResult keeps its input unused: `GO ... | LOOKUP ...` ignores the input. It
    calls onResult_: its rows (VertexID | SrcVID, DstVID, Ranking, then the yields) feed the sentence piped behind
    it. The scan is the backend's (Engine.lookup, ngx_lookup): no host storage leg stands behind it, so a
    "lookup: ..." refusal is the sentence's error.
  - YieldExecutor (src/graph/YieldExecutor.cpp): `... | YIELD <columns> [WHERE <expr>]` and `YIELD $var.x ...` over an
    interim result (nebula_amd/yieldexec.py), when the caller opts in with yield_sentence=True. It calls onResult_:
    its rows feed the sentence piped behind it. Behind a plain head GO the filter, the projection and the aggregates
    run in the same device call where the backend has it (ngx_go_yield; Pipeline._go_yield).
GO and GROUP BY are the traversal sentences here; ORDER BY and LIMIT run under order_limit=True only, and a YIELD
sentence with an input under yield_sentence=True only (the default keeps refusing them).
`backend` is an Engine (the product) or the oracle's Oracle: both take `go(space, s, input=...)`.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

from . import fetch as fetchmod
from . import findpath, groupby, ngql, orderby, setop, yieldexec
from . import lookup as lookupmod

T_UNKNOWN, T_BOOL, T_INT, T_VID, T_FLOAT, T_DOUBLE, T_STRING, T_TIMESTAMP = 0, 1, 2, 3, 4, 5, 6, 21
_KIND_TYPE = {"bool": T_BOOL, "int": T_INT, "id": T_INT, "timestamp": T_INT, "float": T_DOUBLE,
              "double": T_DOUBLE, "str": T_STRING}


@dataclass
class Interim:
    """InterimResult (src/graph/InterimResult.h): column names, schema types, rows of typed cells
    ((kind, value) pairs as GoResult.rows holds them)."""
    names: List[str]
    types: List[int] = field(default_factory=list)
    rows: List[tuple] = field(default_factory=list)

    @staticmethod
    def from_result(names: Sequence[str], col_types: Sequence[int], rows: Sequence[tuple]) -> "Interim":
        if not rows:
            return Interim(list(names))
        types = []
        for i, t in enumerate(col_types):
            if t == T_UNKNOWN:                                    # GoExecutor.cpp:1008-1026
                kind, v = rows[0][i]
                t = T_BOOL if kind == "empty" and v is not None else _KIND_TYPE.get(kind, T_UNKNOWN)
            types.append(t)
        return Interim(list(names), types, list(rows))


class PipelineError(Exception):
    pass


def _split(text: str, sep: str) -> List[str]:
    """Split at `sep' outside quotes and parentheses; a `|' of `||' is not a pipe."""
    out, depth, quote, cur, i = [], 0, None, [], 0
    while i < len(text):
        ch = text[i]
        if quote:
            cur.append(ch)
            if ch == "\\" and i + 1 < len(text):
                cur.append(text[i + 1])
                i += 1
            elif ch == quote:
                quote = None
        elif ch in "\"'":
            quote = ch
            cur.append(ch)
        elif ch == "(":
            depth += 1
            cur.append(ch)
        elif ch == ")":
            depth -= 1
            cur.append(ch)
        elif ch == sep and depth == 0 and not (sep == "|" and (text[i + 1:i + 2] == "|" or text[i - 1:i] == "|")):
            out.append("".join(cur))
            cur = []
        else:
            cur.append(ch)
        i += 1
    out.append("".join(cur))
    return out


def _unwrap(text: str) -> str:
    """`( piped )' -> `piped' when the parentheses enclose the whole sentence."""
    t = text.strip()
    while t.startswith("(") and t.endswith(")"):
        depth = 0
        for i, ch in enumerate(t):
            depth += ch == "("
            depth -= ch == ")"
            if depth == 0 and i < len(t) - 1:
                return t
        t = t[1:-1].strip()
    return t


def plain_go(s: ngql.GoSentence) -> bool:
    """A GO a device-resident call can take as its head: literal vids, no DISTINCT, a YIELD without aggregates and
    without `$-` / `$var` props."""
    if s.from_type or s.distinct or not s.yields:
        return False
    for y in s.yields:
        if (isinstance(y.expr, ngql.Func) and y.expr.name.upper() in ngql.AGG_FUNCS) or \
                any(k in (ngql.K_INPUT_PROP, ngql.K_VAR_PROP) for k, _, _ in y.expr.props()):
            return False
    return True


def expand_input_star(s: ngql.GoSentence, names: Optional[Sequence[str]], var: str = "") -> None:
    """YieldClauseWrapper::needAllPropsFromInput / needAllPropsFromVar: `$-.*` / `$v.*` -> one
    column per input column."""
    cols = []
    for y in s.yields:
        e = y.expr
        if isinstance(e, ngql.Prop) and e.prop == "*" and e.kind in (ngql.K_INPUT_PROP, ngql.K_VAR_PROP):
            if names is None:
                raise PipelineError("Inputs nullptr." if e.kind == ngql.K_INPUT_PROP else
                                    "Variable `%s' not defined." % e.alias)
            for n in names:
                cols.append(ngql.YieldCol(ngql.Prop(e.kind, e.ref, e.alias, n)))
            continue
        cols.append(y)
    s.yields = cols


@dataclass
class Outcome:
    ok: bool
    error: str = ""
    names: List[str] = field(default_factory=list)
    col_types: List[int] = field(default_factory=list)
    rows: List[tuple] = field(default_factory=list)


class Pipeline:
    """Runs nGQL text made of GO sentences, pipes, parentheses, `$v = ...' and `;'."""

    def __init__(self, backend, space: int, edge_names: Sequence[str] = (), device_group_by: bool = True,
                 order_limit: bool = False, device_order_by: bool = True, device_group_order: bool = True,
                 set_ops: bool = False, device_set_op: bool = True, find_path: bool = False,
                 device_find_path: bool = True, fetch: bool = False, device_fetch: bool = True, catalog=None,
                 lookup: bool = False, indexes=None, yield_sentence: bool = False, device_yield: bool = True, **go_kw):
        """yield_sentence=True: YIELD sentences with a pipe input or a `$var` prop run (off by default, as the other
        opt-ins are; the constant form runs either way); device_yield=False: every one takes the host restatement
        (yieldexec.py) even where the backend could run it over the head GO's rows in HBM. yield_fallbacks counts
        the device calls refused with "yield: ...", yield_refusal keeps the last refusal's text.
        lookup=True: LOOKUP ON sentences run (off by default, as the other opt-ins are); indexes are the space's
        lookup.Index items (what the meta client's index cache holds); the schemas come from catalog, as for fetch.
        The backend has to have `lookup` (an Engine): the oracle has no index scan, and the Pipeline refuses to be
        built over it with lookup=True. lookups counts the sentences scanned, lookup_rows their rows.
        fetch=True: FETCH PROP ON sentences run (off by default, as the other opt-ins are); catalog is the
        space's fetch.Catalog (partition count, tag and edge schemas: what the executors ask the schema manager);
        an Engine backend hands its own (Engine.catalog), the oracle backend needs it passed.
        device_fetch=False: every FETCH takes the host restatement (fetch.py) even where the backend could look the
        keys up in HBM. fetch_fallbacks counts the device calls refused with "fetch: ...", fetch_refusal keeps the
        last refusal's text.
        find_path=True: FIND PATH sentences run (off by default, as order_limit and set_ops are);
        device_find_path=False: every FIND PATH sentence takes the host restatement (findpath.py) even where the
        backend could search in HBM. find_path_fallbacks counts the device calls refused with "find path: ...".
        set_ops=True: UNION / INTERSECT / MINUS sentences run (off by default, as order_limit is: they are
        refused like every sentence outside this path); device_set_op=False: two plain GO operands are delivered
        and combined on the host even where the backend could do it in HBM.
        device_group_by=False: `GO | GROUP BY` groups on the host even where the backend could on the device.
        order_limit=True: ORDER BY and LIMIT sentences run (off by default: they are refused like every
        sentence outside this path); device_order_by=False: `GO | ORDER BY | LIMIT` and `GO | LIMIT` order
        and cut on the host even where the backend could select the rows on the device.
        device_group_order=False: `GO | GROUP BY | [ORDER BY |] LIMIT` groups on the device and orders the group
        rows on the host, even where the backend could do both in one call (it takes all three switches on)."""
        self.device_group_order = device_group_order
        self.yield_sentence = yield_sentence
        self.device_yield = device_yield
        self.yield_fallbacks = 0
        self.yield_refusal = ""
        self.set_ops = set_ops
        self.device_set_op = device_set_op
        self.set_fallbacks = 0                                    # device set calls refused after both traversals ran
        self.find_path = find_path
        self.device_find_path = device_find_path
        self.find_path_fallbacks = 0
        self.find_path_refusal = ""                               # the last refusal's text
        self.fetch = fetch
        self.device_fetch = device_fetch
        self.lookup = lookup
        self.indexes = list(indexes or [])
        self.lookups = 0
        self.lookup_rows = 0
        if lookup and not hasattr(backend, "lookup"):
            raise PipelineError("lookup=True needs a backend with lookup(space, spec): an Engine")
        if catalog is None and (fetch or lookup) and hasattr(backend, "catalog"):
            catalog = backend.catalog(space)                      # an Engine knows the schemas it was given
        if lookup and catalog is None:
            raise PipelineError("lookup=True needs the space's schemas: catalog=fetch.Catalog(...)")
        if fetch and catalog is None:
            raise PipelineError("fetch=True needs the space's schemas: catalog=fetch.Catalog(...)")
        self.catalog = catalog
        self.fetch_fallbacks = 0
        self.fetch_refusal = ""
        self.device_group_by = device_group_by
        self.order_limit = order_limit
        self.device_order_by = device_order_by
        self.backend = backend
        self.space = space
        self.edge_names = list(edge_names)
        self.go_kw = go_kw
        self.variables: Dict[str, Interim] = {}

    def _go(self, text: str, inp: Optional[Interim]) -> Outcome:
        try:
            s = ngql.parse_go(text)
        except (SyntaxError, ValueError) as e:
            return Outcome(False, "SyntaxError: %s" % e)
        for y in s.yields:                                        # GoExecutor::prepareYield, GoExecutor.cpp:343-347
            if isinstance(y.expr, ngql.Func) and y.expr.name.upper() in ngql.AGG_FUNCS:
                return Outcome(False, "SyntaxError: Do not support in aggregated query without group by")
        feed = None
        if s.from_type == 1:
            feed = inp if inp is not None else Interim([])
        elif s.from_type == 2:
            if s.from_var not in self.variables:
                return Outcome(False, "Variable `%s' not defined" % s.from_var)
            feed = self.variables[s.from_var]
        # `$v.*` reads the variable; `$-.*` the pipe input
        star_var = next((e.alias for y in s.yields for e in [y.expr]
                         if isinstance(e, ngql.Prop) and e.kind == ngql.K_VAR_PROP and e.prop == "*"), None)
        try:
            if star_var is not None:
                v = self.variables.get(star_var)
                expand_input_star(s, v.names if v else None, star_var)
            expand_input_star(s, inp.names if inp is not None else None)
        except PipelineError as e:
            return Outcome(False, str(e))
        names = s.column_names(self.edge_names)
        r = self.backend.go(self.space, s, input=feed, **self.go_kw)
        if not r.ok:
            return Outcome(False, r.error, names)
        return Outcome(True, "", names, list(r.col_types), list(r.rows))

    def _yield_constant(self, text: str) -> Outcome:
        """A YIELD sentence with no input (YieldExecutor::executeConstant, YieldExecutor.cpp:343-379):
        one row of its constant expressions (integer literals, hash(...), their negation, and string /
        bool / double literals), typed as Collector::getSchema types the values; it is the left side
        of `YIELD <vid> AS id | GO FROM $-.id ...` (GoTest.cpp:3083-3088)."""
        p = ngql.Parser(text)
        p.expect("kw", "YIELD")
        names, row = [], []
        while True:
            e = p.expression()
            alias = p.label() if p.accept("kw", "AS") else ""
            try:
                v = ngql.eval_const(e)
            except ValueError:
                if not isinstance(e, ngql.Prim):
                    raise PipelineError("only constant YIELD sentences run in this path: " + text[:40])
                v = e.value
            names.append(alias or e.to_string())
            if isinstance(v, bool):
                row.append(("bool", v))
            elif isinstance(v, int):
                row.append(("int", v))
            elif isinstance(v, float):
                row.append(("double", v))
            else:
                row.append(("str", v))
            if not p.accept("op", ","):
                break
        p.expect("eof")
        types = [_KIND_TYPE[k] for k, _ in row]
        return Outcome(True, "", names, types, [tuple(row)])

    def _yield(self, text: str, inp: Optional[Interim]) -> Outcome:
        """A YIELD sentence over the pipe's input or a variable: YieldExecutor restated on the host (yieldexec.run)."""
        try:
            s = ngql.parse_yield(text)
        except (SyntaxError, ValueError) as e:
            return Outcome(False, "SyntaxError: %s" % e)
        try:
            if inp is None and not self._yield_reads(text):       # executeConstant's aggregate form
                names, types, rows = yieldexec.run_constant(s)
            else:
                names, types, rows = yieldexec.run(s, inp, self.variables)
        except yieldexec.YieldError as e:
            return Outcome(False, str(e))
        return Outcome(True, "", names, types, rows)

    def _go_yield(self, go_text: str, yield_text: str) -> Optional[Outcome]:
        """`GO | YIELD ... [WHERE ...]` with the sentence on the device (ngx_go_yield); None when the sentences run
        one by one: a shape only the host words (a `$var`, an unknown column, a SyntaxError), or a "yield: ..."
        refusal, which is counted and costs the traversal once more."""
        from .engine import YieldSpec
        g = self._plain_go(go_text)
        if g is None:
            return None
        names = g.column_names(self.edge_names)
        if len(set(names)) != len(names):
            return None
        try:
            s = ngql.parse_yield(yield_text)
            yields = yieldexec.expand(s, Interim(names), {})
            yieldexec.check_agg(yields)
            if yieldexec.syntax_check(s, yields) is not None:
                return None
        except (SyntaxError, ValueError, yieldexec.YieldError):
            return None
        props = [p for y in yields for p in y.expr.props()] + (s.where.props() if s.where is not None else [])
        if any(prop not in names for _, _, prop in props):
            return None
        spec = YieldSpec(names, s.where.encode() if s.where is not None else None,
                         [(y.fun, y.expr.encode()) for y in yields])
        kw = {k: v for k, v in self.go_kw.items() if k in ("pushdown", "now_sec")}
        try:
            r = self.backend.go_yield(self.space, g, spec, **kw)
        except RuntimeError as e:
            if getattr(e, "code", 0) == -1002:                    # the device-resident GO itself: the plain path decides
                return None
            raise
        if not r.ok:
            if r.code == -1002 and r.error.startswith("yield:"):
                self.yield_fallbacks += 1
                self.yield_refusal = r.error
            return None                                           # the GO's own error: the plain path words it
        out_names = [y.alias if y.alias else y.expr.to_string() for y in yields]
        return Outcome(True, "", out_names, list(r.col_types), list(r.rows))

    @staticmethod
    def _yield_reads(text: str) -> bool:
        """Whether a YIELD sentence without pipe input is YieldExecutor's all the same: it names a prop (`$var.x` runs
        over the variable, `$-.x` is its `Inputs nullptr.`, any other prop its syntaxCheck's error)."""
        try:
            s = ngql.parse_yield(text)
            return bool([p for y in s.yields for p in y.expr.props()] + (s.where.props() if s.where is not None else []))
        except (SyntaxError, ValueError):
            return False

    @staticmethod
    def _yield_aggregates(text: str) -> bool:
        """Whether a YIELD sentence carries a function (its constant form is YieldExecutor::AggregateConstant)."""
        try:
            return any(y.fun for y in ngql.parse_yield(text).yields)
        except (SyntaxError, ValueError):
            return False

    def _device_spec(self, go_text: str, gb_text: str):
        """(GoSentence, GroupBySentence, spec) when `GO | GROUP BY` can group on the device (ngx_go_group_by):
        a plain GO (literal vids, no DISTINCT, no $- / $var), keys that are input columns, yields that are
        input columns or constants, no STD. None: the host path decides (and reports any error)."""
        from .engine import GroupBySpec
        try:
            s, g = ngql.parse_go(go_text), ngql.parse_group_by(gb_text)
            aliases = groupby.prepare(g)
            names = s.column_names(self.edge_names)
            if not plain_go(s) or len(set(names)) != len(names):
                return None
            groups = groupby.check_all(g, aliases, names)
            if len(groups) > 4 or not all(groupby._is_input(c.expr) for c in groups):
                return None
            yields = []
            for y in g.yields:
                if y.fun == "STD":
                    return None
                if groupby._is_input(y.expr):
                    yields.append((y.fun, names.index(y.expr.prop), None))
                    continue
                if y.expr.props():
                    return None
                v, _ = groupby._eval(y.expr, (), {})
                if isinstance(v, bool) or not isinstance(v, (int, float)):
                    if not (isinstance(v, str) and y.fun in ("COUNT", "COUNT_DISTINCT")):
                        return None
                    v = "*"
                yields.append((y.fun, -1, v))
            return s, g, GroupBySpec([names.index(c.expr.prop) for c in groups], yields)
        except (SyntaxError, ValueError, groupby.GroupByError):
            return None

    def _go_group_by(self, go_text: str, gb_text: str) -> Optional[Outcome]:
        """`GO | GROUP BY` with the grouping on the device; None when the host path has to run."""
        plan = self._device_spec(go_text, gb_text)
        if plan is None:
            return None
        s, g, spec = plan
        kw = {k: v for k, v in self.go_kw.items() if k in ("pushdown", "now_sec")}
        try:
            r = self.backend.go(self.space, s, group_by=spec, yield_only=True, compact=True, **kw)
        except RuntimeError as e:
            if getattr(e, "code", 0) == -1002:                    # the device-resident GO itself: the plain path decides
                return None
            raise
        if not r.ok:
            if r.code == -1002:                                   # NGX_E_UNSUPPORTED: group on the host
                return None
            return Outcome(False, r.error, s.column_names(self.edge_names))
        return Outcome(True, "", g.column_names(), list(r.col_types), list(r.rows))

    def _group_by(self, text: str, inp: Optional[Interim]) -> Outcome:
        """A GROUP BY sentence on the pipe's input: GroupByExecutor restated on the host (groupby.run)."""
        try:
            s = ngql.parse_group_by(text)
        except (SyntaxError, ValueError) as e:
            return Outcome(False, "SyntaxError: %s" % e)
        inp = inp if inp is not None else Interim([])
        try:
            names, types, rows = groupby.run(s, inp.names, inp.types, inp.rows)
        except groupby.GroupByError as e:
            return Outcome(False, str(e), s.column_names())
        return Outcome(True, "", names, types, rows)

    def _order_spec(self, go_text: str, ob_text: Optional[str], lim_text: str):
        """(GoSentence, spec) when `GO | ORDER BY | LIMIT` (ob_text None: `GO | LIMIT`) can select its rows on
        the device (ngx_go_order_by): a plain GO as in _device_spec, factors that are its columns. None: the
        host path decides (and reports any error)."""
        from .engine import OrderBySpec
        try:
            s, lim = ngql.parse_go(go_text), ngql.parse_limit(lim_text)
            names = s.column_names(self.edge_names)
            if not plain_go(s) or len(set(names)) != len(names):
                return None
            factors = []
            if ob_text is not None:
                for col, desc in ngql.parse_order_by(ob_text).factors:
                    if col not in names:
                        return None
                    factors.append((names.index(col), desc))
            return s, OrderBySpec(factors, lim.offset, lim.count)
        except (SyntaxError, ValueError):
            return None

    def _go_order_by(self, go_text: str, ob_text: Optional[str], lim_text: str) -> Optional[Outcome]:
        """`GO | [ORDER BY |] LIMIT` with the selection on the device; None when the host path has to run."""
        plan = self._order_spec(go_text, ob_text, lim_text)
        if plan is None:
            return None
        s, spec = plan
        kw = {k: v for k, v in self.go_kw.items() if k in ("pushdown", "now_sec")}
        try:
            r = self.backend.go(self.space, s, order_by=spec, yield_only=True, compact=True, **kw)
        except RuntimeError as e:
            if getattr(e, "code", 0) == -1002:                    # the device-resident GO itself: the plain path decides
                return None
            raise
        names = s.column_names(self.edge_names)
        if not r.ok:
            if r.code == -1002:                                   # NGX_E_UNSUPPORTED: order and cut on the host
                return None
            return Outcome(False, r.error, names)
        # the interim schema the host path would hand on: UNKNOWN columns take the first row's type
        return Outcome(True, "", names, Interim.from_result(names, r.col_types, r.rows).types, list(r.rows))

    def _group_order_spec(self, go_text: str, gb_text: str, ob_text: Optional[str], lim_text: Optional[str]):
        """(GoSentence, GroupBySentence, group spec, order spec) when `GO | GROUP BY | ORDER BY | LIMIT` (ob_text
        None: `GO | GROUP BY | LIMIT`) can run on the device in one call (ngx_go_group_order_by): _device_spec's
        conditions, factors that name columns of the GROUP BY, and those names unique. ORDER BY without LIMIT
        (lim_text None) is not sent: every group row would cross anyway. None: the paths there were decide."""
        from .engine import OrderBySpec
        if lim_text is None:
            return None
        plan = self._device_spec(go_text, gb_text)
        if plan is None:
            return None
        s, g, gspec = plan
        try:
            lim = ngql.parse_limit(lim_text)
            names = g.column_names()
            factors = []
            if ob_text is not None:
                for col, desc in ngql.parse_order_by(ob_text).factors:
                    if col not in names or names.count(col) != 1:
                        return None
                    factors.append((names.index(col), desc))
            return s, g, gspec, OrderBySpec(factors, lim.offset, lim.count)
        except (SyntaxError, ValueError):
            return None

    _HOST = object()                                              # _go_group_order_by: the plain host path has to run

    def _go_group_order_by(self, go_text: str, gb_text: str, ob_text: Optional[str], lim_text: Optional[str]):
        """`GO | GROUP BY | [ORDER BY |] LIMIT` on the device in one call. None: not sent, or refused by the order
        stage ("order by: ..."): the device GROUP BY and the host sentences run as without this path. _HOST:
        refused by the group stage ("group by: ..."), which the device GROUP BY would refuse again: every
        sentence runs on the host. Either way a refusal costs one extra traversal."""
        plan = self._group_order_spec(go_text, gb_text, ob_text, lim_text)
        if plan is None:
            return None
        s, g, gspec, ospec = plan
        kw = {k: v for k, v in self.go_kw.items() if k in ("pushdown", "now_sec")}
        try:
            r = self.backend.go(self.space, s, group_by=gspec, order_by=ospec, yield_only=True, compact=True, **kw)
        except RuntimeError as e:
            if getattr(e, "code", 0) == -1002:                    # the device-resident GO itself: the plain path decides
                return self._HOST
            raise
        if not r.ok:
            if r.code == -1002:                                   # NGX_E_UNSUPPORTED
                return None if r.error.startswith("order by:") else self._HOST
            return Outcome(False, r.error, s.column_names(self.edge_names))
        # the interim schema the host path would hand on
        names = g.column_names()
        return Outcome(True, "", names, Interim.from_result(names, r.col_types, r.rows).types, list(r.rows))

    def _order_by(self, text: str, inp: Optional[Interim]) -> Outcome:
        """An ORDER BY sentence on the pipe's input: OrderByExecutor restated on the host (orderby.order_by)."""
        try:
            s = ngql.parse_order_by(text)
        except (SyntaxError, ValueError) as e:
            return Outcome(False, "SyntaxError: %s" % e)
        try:
            names, types, rows = orderby.order_by(s, *((inp.names, inp.types, inp.rows) if inp is not None else (None, [], [])))
        except orderby.OrderByError as e:
            return Outcome(False, str(e), list(inp.names) if inp is not None else [])
        return Outcome(True, "", names, types, rows)

    def _limit(self, text: str, inp: Optional[Interim]) -> Outcome:
        """A LIMIT sentence on the pipe's input: LimitExecutor restated on the host (orderby.limit)."""
        try:
            s = ngql.parse_limit(text)
        except (SyntaxError, ValueError) as e:
            return Outcome(False, "SyntaxError: %s" % e)
        try:
            names, types, rows = orderby.limit(s, *((inp.names, inp.types, inp.rows) if inp is not None else (None, [], [])))
        except orderby.OrderByError as e:
            return Outcome(False, str(e), list(inp.names) if inp is not None else [])
        return Outcome(True, "", names, types, rows)

    def _set_spec(self, left_text: str, right_text: str, op: str):
        """(left GoSentence, right GoSentence) when `GO <op> GO` can run on the device (ngx_go_set): two plain GOs
        as in _device_spec with as many columns as each other, and an operator with a kernel. None: the host
        path decides (and reports any error)."""
        if op == "UNION ALL":
            return None
        try:
            pair = []
            for text in (left_text, right_text):
                if len(_split(text, "|")) > 1 or not text.strip().upper().startswith("GO"):
                    return None
                s = ngql.parse_go(text)
                if not plain_go(s):
                    return None
                pair.append(s)
            if len(pair[0].yields) != len(pair[1].yields):
                return None
            return pair
        except (SyntaxError, ValueError):
            return None

    def _go_set(self, left_text: str, right_text: str, op: str) -> Optional[Outcome]:
        """`GO <op> GO` with both traversals and the operator on the device; None when the host path has to run
        (after a "set op: ..." refusal that costs the two traversals once more: set_fallbacks counts those)."""
        pair = self._set_spec(left_text, right_text, op)
        if pair is None:
            return None
        kw = {k: v for k, v in self.go_kw.items() if k in ("pushdown", "now_sec")}
        try:
            r = self.backend.go_set(self.space, pair[0], pair[1], op, **kw)
        except RuntimeError as e:
            if getattr(e, "code", 0) == -1002:                    # a device-resident GO itself: the plain path decides
                return None
            raise
        if not r.ok:                                              # a refusal, or a side's own error: the host path words it
            if r.code == -1002 and r.error.startswith("set op:"):
                self.set_fallbacks += 1
            return None
        names = pair[0].column_names(self.edge_names)
        return Outcome(True, "", names, Interim.from_result(names, r.col_types, r.rows).types, list(r.rows))

    def _set(self, text: str, inp: Optional[Interim]) -> Outcome:
        """A set sentence (parser.yy set_sentence): piped sentences folded from the left by SetExecutor."""
        try:
            operands, ops = ngql.split_set(text)
        except SyntaxError as e:
            return Outcome(False, "SyntaxError: %s" % e)
        if not ops:
            return self._piped(text, inp)
        if inp is not None:                                       # SetExecutor::feedResult, SetExecutor.cpp:111-114
            return Outcome(False, "Set operation not support input yet.")
        acc = None
        if self.device_set_op and getattr(self.backend, "device_set_op", False):
            acc = self._go_set(_unwrap(operands[0]), _unwrap(operands[1]), ops[0])
        first = 1 if acc is not None else 0
        if acc is None:
            acc = self._operand(operands[0])
        for op, operand in list(zip(ops, operands[1:]))[first:]:
            right = self._operand(operand)
            if not acc.ok:                                        # both sides ran; the left's error is reported first
                acc = Outcome(False, "left subquery has error: " + acc.error, acc.names)
                continue
            if not right.ok:
                acc = Outcome(False, "right subquery has error: " + right.error, acc.names)
                continue
            li = Interim.from_result(acc.names, acc.col_types, acc.rows)
            ri = Interim.from_result(right.names, right.col_types, right.rows)
            try:
                names, types, rows = setop.apply(op, li.names, li.types, li.rows, ri.names, ri.types, ri.rows)
            except setop.SetError as e:
                return Outcome(False, str(e), list(acc.names))
            acc = Outcome(True, "", names, types, rows)
        return acc

    def _find_path(self, text: str, inp: Optional[Interim]) -> Outcome:
        """A FIND PATH sentence: on the device where the backend has it and takes the sentence, else
        FindPathExecutor restated on the host (findpath.run)."""
        try:
            s = ngql.parse_find_path(text)
        except (SyntaxError, ValueError) as e:
            return Outcome(False, "SyntaxError: %s" % e)
        kw = {k: v for k, v in self.go_kw.items() if k in ("pushdown", "now_sec")}
        try:
            if self.device_find_path and getattr(self.backend, "device_find_path", False):
                from_vids, to_vids = findpath.setup_vids(s, inp, self.variables)
                r = self.backend.find_path(self.space, s, from_vids, to_vids)
                if r.ok:
                    return Outcome(True, "", ["_path_"], [findpath.T_PATH] if r.rows else [], list(r.rows))
                if r.code != -1002 or not r.error.startswith("find path:"):
                    return Outcome(False, r.error, ["_path_"])
                self.find_path_fallbacks += 1
                self.find_path_refusal = r.error
            names, types, rows = findpath.run(self.backend, self.space, s, inp, self.variables, self.edge_names, **kw)
        except findpath.FindPathError as e:
            return Outcome(False, str(e), ["_path_"])
        return Outcome(True, "", names, types, rows)

    def _fetch(self, text: str, inp: Optional[Interim], go_text: Optional[str] = None) -> Optional[Outcome]:
        """A FETCH sentence: on the device where the backend has it and takes the sentence, else the executors
        restated on the host (fetch.run). go_text: the plain head GO in front of it, to run in the same device call
        (ngx_go_fetch); None is returned when that call cannot be made and the two sentences run one by one."""
        try:
            s = ngql.parse_fetch(text)
        except (SyntaxError, ValueError) as e:
            return None if go_text is not None else Outcome(False, "SyntaxError: %s" % e)
        vertices = isinstance(s, ngql.FetchVerticesSentence)
        first = ["VertexID"] if vertices else [s.edges[0] + k for k in ("._src", "._dst", "._rank")] if s.edges else []
        kw = {k: v for k, v in self.go_kw.items() if k in ("pushdown", "now_sec")}
        try:
            if self.device_fetch and getattr(self.backend, "device_fetch", False):
                r = self._device_fetch(s, inp, go_text, kw)
                if r is not None:
                    return r
            if go_text is not None:
                return None
            names, types, rows = fetchmod.run(self.backend, self.space, self.catalog, s, inp, self.variables,
                                              now_sec=kw.get("now_sec", 0))
        except fetchmod.FetchError as e:
            if go_text is not None:
                return None
            return Outcome(False, str(e), first)
        return Outcome(True, "", names, types, rows)

    def _device_fetch(self, s, inp: Optional[Interim], go_text: Optional[str], kw) -> Optional[Outcome]:
        """The sentence through Engine.fetch / Engine.go_fetch; None: the host restatement has to run (a "fetch: ..."
        refusal is counted), or, with go_text, the sentences run one by one. The prepare stage is the host's
        (fetch.prepare_vertices / prepare_edges), so every Status text is the one the host path gives."""
        g = None
        if go_text is not None:
            g = self._plain_go(go_text)
            if g is None or not s.from_type or s.from_type != 1:
                return None
            names = g.column_names(self.edge_names)
            if len(set(names)) != len(names):
                return None
            # the prepare stage wants the input's names and (for `$-.x` in YIELD) types; the rows stay in HBM
            inp = Interim(names, [], [tuple(("int", 0) for _ in names)])
        spec = fetchmod.device_spec(self.catalog, s, inp, self.variables, placeholder=g is not None)
        if spec is None:                                          # empty inputs, or a shape only the host words
            return None
        if g is not None:
            try:
                r = self.backend.go_fetch(self.space, g, spec, **kw)
            except RuntimeError as e:
                if getattr(e, "code", 0) == -1002:                # the device-resident GO itself: the plain path decides
                    return None
                raise
        else:
            r = self.backend.fetch(self.space, spec)
        if not r.ok:
            if r.code == -1002 and r.error.startswith("fetch:"):
                self.fetch_fallbacks += 1
                self.fetch_refusal = r.error
                return None
            if g is not None:                                     # the GO's own error: the plain path words it
                return None
            return Outcome(False, r.error, spec.names)
        names, types, rows = fetchmod.device_rows(spec, r)
        return Outcome(True, "", names, types, rows)

    def _plain_go(self, go_text: str):
        """The GoSentence of a plain GO (plain_go, the condition _device_spec sets too), else None."""
        try:
            s = ngql.parse_go(go_text)
        except (SyntaxError, ValueError):
            return None
        return s if plain_go(s) else None

    def _lookup(self, text: str) -> Outcome:
        """A LOOKUP sentence: graphd's checks and the index choice, storaged's scan policy (lookup.plan_of), then the
        backend's scan. The input of the pipe is not read (LookupExecutor::feedResult keeps it unused)."""
        try:
            s = ngql.parse_lookup(text)
        except (SyntaxError, ValueError) as e:
            return Outcome(False, "SyntaxError: %s" % e)
        try:
            plan = lookupmod.plan_of(self.catalog, self.indexes, s)
        except lookupmod.LookupError as e:
            return Outcome(False, str(e))
        spec = lookupmod.device_spec(plan)
        r = self.backend.lookup(self.space, spec)
        if not r.ok:
            return Outcome(False, r.error, list(plan.names))
        self.lookups += 1
        self.lookup_rows += r.nrows
        names, types, rows = lookupmod.device_rows(spec, r)
        return Outcome(True, "", names, types, rows)

    def _operand(self, text: str) -> Outcome:
        """One operand of a set sentence: a piped sentence, or a parenthesised set sentence."""
        body = _unwrap(text)
        return self._set(body, None) if ngql.is_set(body) else self._piped(text, None)

    def _piped(self, text: str, inp: Optional[Interim]) -> Outcome:
        parts = _split(text, "|")
        if self.set_ops:                                          # PipeExecutor::prepare, PipeExecutor.cpp:101-106
            for part in parts[1:]:
                if ngql.is_set(_unwrap(part)):
                    return Outcome(False, "SyntaxError: Set op not support input.")
        if self.order_limit:                                      # the reference parses the whole text first
            for part in parts:
                body = _unwrap(part)
                if len(_split(body, "|")) > 1:                    # ( piped ): checked when it runs
                    continue
                try:
                    if ngql.is_order_by(body):
                        ngql.parse_order_by(body)
                    elif ngql.is_limit(body):
                        ngql.parse_limit(body)
                except (SyntaxError, ValueError) as e:
                    return Outcome(False, "SyntaxError: %s" % e)
        if self.fetch:
            for part in parts:
                body = _unwrap(part)
                if len(_split(body, "|")) == 1 and ngql.is_fetch(body):
                    try:
                        ngql.parse_fetch(body)
                    except (SyntaxError, ValueError) as e:
                        return Outcome(False, "SyntaxError: %s" % e)
        if self.lookup:
            for part in parts:
                body = _unwrap(part)
                if len(_split(body, "|")) == 1 and ngql.is_lookup(body):
                    try:
                        ngql.parse_lookup(body)
                    except (SyntaxError, ValueError) as e:
                        return Outcome(False, "SyntaxError: %s" % e)
        if self.yield_sentence:
            for part in parts:
                body = _unwrap(part)
                if len(_split(body, "|")) == 1 and ngql.is_yield(body):
                    try:
                        ngql.parse_yield(body)
                    except (SyntaxError, ValueError) as e:
                        return Outcome(False, "SyntaxError: %s" % e)
        cur = inp
        out = None
        skip = 0
        for i, part in enumerate(parts):
            body = _unwrap(part)
            if skip:                                              # ran on the device with the GO before it
                skip -= 1
                if not skip and i + 1 < len(parts):
                    cur = Interim.from_result(out.names, out.col_types, out.rows)
                continue
            host_group = False
            if self.yield_sentence and self.device_yield and getattr(self.backend, "device_yield", False) \
                    and i + 1 < len(parts) and cur is None and body.upper().startswith("GO") \
                    and ngql.is_yield(_unwrap(parts[i + 1])):
                dev = self._go_yield(body, _unwrap(parts[i + 1]))
                if dev is not None:
                    out, skip = dev, 1
                    continue
            if self.fetch and self.device_fetch and getattr(self.backend, "device_fetch", False) and i + 1 < len(parts) \
                    and cur is None and body.upper().startswith("GO") and ngql.is_fetch(_unwrap(parts[i + 1])):
                dev = self._fetch(_unwrap(parts[i + 1]), None, go_text=body)
                if dev is not None:
                    out, skip = dev, 1
                    if not out.ok:
                        return out
                    continue
            if self.order_limit and self.device_order_by and self.device_group_by and self.device_group_order \
                    and getattr(self.backend, "device_group_order", False) and i + 2 < len(parts) \
                    and body.upper().startswith("GO") and ngql.is_group_by(_unwrap(parts[i + 1])):
                nxt = [_unwrap(p) for p in parts[i + 1:i + 4]]
                dev, took = None, 0
                if ngql.is_limit(nxt[1]):
                    dev, took = self._go_group_order_by(body, nxt[0], None, nxt[1]), 2
                elif len(nxt) == 3 and ngql.is_order_by(nxt[1]) and ngql.is_limit(nxt[2]):
                    dev, took = self._go_group_order_by(body, nxt[0], nxt[1], nxt[2]), 3
                if dev is self._HOST:
                    host_group = True
                elif dev is not None:
                    out, skip = dev, took
                    if not out.ok:
                        return out
                    continue
            if self.order_limit and self.device_order_by and getattr(self.backend, "device_order_by", False) \
                    and i + 1 < len(parts) and body.upper().startswith("GO"):
                nxt = [_unwrap(p) for p in parts[i + 1:i + 3]]
                dev, took = None, 0
                if ngql.is_limit(nxt[0]):
                    dev, took = self._go_order_by(body, None, nxt[0]), 1
                elif len(nxt) == 2 and ngql.is_order_by(nxt[0]) and ngql.is_limit(nxt[1]):
                    dev, took = self._go_order_by(body, nxt[0], nxt[1]), 2
                if dev is not None:
                    out, skip = dev, took
                    if not out.ok:
                        return out
                    continue
            if not host_group and self.device_group_by and getattr(self.backend, "device_group_by", False) and i + 1 < len(parts) \
                    and body.upper().startswith("GO") and ngql.is_group_by(_unwrap(parts[i + 1])):
                dev = self._go_group_by(body, _unwrap(parts[i + 1]))
                if dev is not None:
                    out, skip = dev, 1
                    if not out.ok:
                        return out
                    continue
            if self.set_ops and ngql.is_set(body):
                out = self._set(body, cur)                        # ( set_sentence ) as a traverse sentence
            elif len(_split(body, "|")) > 1:
                out = self._piped(body, cur)                      # ( piped ) as a traverse sentence
            elif self.yield_sentence and ngql.is_yield(body) and (cur is not None or self._yield_reads(body)
                                                                  or self._yield_aggregates(body)):
                out = self._yield(body, cur)
            elif body.upper().startswith("YIELD") and cur is None:
                out = self._yield_constant(body)
            elif ngql.is_group_by(body):
                out = self._group_by(body, cur)
            elif self.order_limit and ngql.is_order_by(body):
                out = self._order_by(body, cur)
            elif self.order_limit and ngql.is_limit(body):
                out = self._limit(body, cur)
            elif self.fetch and ngql.is_fetch(body):
                out = self._fetch(body, cur)
            elif self.lookup and ngql.is_lookup(body):
                out = self._lookup(body)
            elif self.find_path and ngql.is_find_path(body):
                out = self._find_path(body, cur)
                if not out.ok:
                    return out
                cur = None                                        # FindPathExecutor never calls onResult_
                continue
            else:
                if not body.upper().startswith("GO"):
                    raise PipelineError("only GO sentences run in this path: " + body[:40])
                out = self._go(body, cur)
            if not out.ok:
                return out
            if i + 1 < len(parts):
                cur = Interim.from_result(out.names, out.col_types, out.rows)
        return out

    def run(self, text: str) -> Outcome:
        out = Outcome(True)
        for stmt in _split(text, ";"):
            stmt = stmt.strip()
            if not stmt:
                continue
            var = None
            if stmt.startswith("$"):
                head, eq, rest = stmt.partition("=")
                if eq and head.strip()[1:].isidentifier():
                    var, stmt = head.strip()[1:], rest.strip()
            out = self._set(stmt, None) if self.set_ops else self._piped(stmt, None)
            if not out.ok:
                return out
            if var is not None:
                self.variables[var] = Interim.from_result(out.names, out.col_types, out.rows)
        return out


def run(backend, space: int, text: str, edge_names: Sequence[str] = (), device_group_by: bool = True,
        order_limit: bool = False, device_order_by: bool = True, device_group_order: bool = True,
        set_ops: bool = False, device_set_op: bool = True, find_path: bool = False, device_find_path: bool = True,
        fetch: bool = False, device_fetch: bool = True, catalog=None, lookup: bool = False, indexes=None,
        yield_sentence: bool = False, device_yield: bool = True, **go_kw) -> Outcome:
    return Pipeline(backend, space, edge_names, device_group_by=device_group_by, order_limit=order_limit,
                    device_order_by=device_order_by, device_group_order=device_group_order, set_ops=set_ops,
                    device_set_op=device_set_op, find_path=find_path, device_find_path=device_find_path, fetch=fetch,
                    device_fetch=device_fetch, catalog=catalog, lookup=lookup, indexes=indexes,
                    yield_sentence=yield_sentence, device_yield=device_yield, **go_kw).run(text)
