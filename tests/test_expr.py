"""The numeric expression engine on the CPU: the parser, the type checker and the compiler of query.py, the Python
run of the compiled ops, and the shared evaluator header csrc/dg_expr.h in a stand-alone program under UBSan,
all held to tests/expr_restate.py (an independent tree-walking restatement of the reference's Expr.eval) bit
for bit, including which rows a long division by zero poisons. The reference's own EvalTest / ParserTest
assertions are the known answers (tests/golden/expr_kats.json)."""
import dataclasses
import importlib
import json
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import expr_restate as ER

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "incubator-druid_amd", "csrc")
with open(os.path.join(HERE, "golden", "expr_kats.json")) as _f:
    KATS = json.load(_f)

LMIN, LMAX = -(1 << 63), (1 << 63) - 1
F32_INEXACT = float(np.float32(0.1))  # a float32 that is no short decimal as a double
COLS = {"a": "LONG", "b": "LONG", "d": "DOUBLE", "e": "DOUBLE", "f": "FLOAT"}
COL_CODE = {"LONG": 1, "FLOAT": 2, "DOUBLE": 3}


def special_rows():
    """Rows over COLS: both long extremes, 0, +-1, +-0.0, +-inf, NaN, float32 values that are not exact doubles."""
    longs = [0, 1, -1, LMIN, LMAX, 7, -7, 3, 2, -5000, 4999, 100]
    dbls = [0.0, -0.0, 1.0, -1.0, math.inf, -math.inf, math.nan, 0.5, -2.5, 1e19, -1e19, 3.0000000001]
    flts = [F32_INEXACT, -0.0, float(np.float32(-3.3)), math.inf, math.nan, 1.0, float(np.float32(1e-30)), 0.0,
            float(np.float32(16777217.0)), -math.inf, 2.0, float(np.float32(-0.7))]
    rows = []
    for i in range(24):
        rows.append({"a": longs[i % 12], "b": longs[(i * 5 + i // 12) % 12], "d": dbls[(i * 7) % 12],
                     "e": dbls[(i + 3 * (i // 12)) % 12], "f": flts[(i * 5) % 12]})
    return rows


def bindings(row):
    return {k: (COLS[k], v) for k, v in row.items()}


def raw_word(col_type, v):
    if col_type == "LONG":
        return int(v) & ER.M64
    if col_type == "DOUBLE":
        return struct.unpack("<Q", struct.pack("<d", v))[0]
    return struct.unpack("<I", struct.pack("<f", v))[0]


def restated(ast, row, out_type=None):
    """(word, poisoned) by the restatement; out_type None: the value's own type."""
    try:
        v = ER.evaluate(ast, bindings(row))
    except ArithmeticError:
        return 0, True
    return (ER.word(v) if out_type is None else ER.as_output(v, out_type)), False


def compiled(Q, prog, row):
    w, p = Q.run_expression(prog.ops, [(COLS[n], row[n]) for n in prog.inputs])
    return (0, True) if p else (w, False)


# ---------------------------------------------------------------------------------------------
# known answers
# ---------------------------------------------------------------------------------------------
def _check_expectation(word, typ, exp, what):
    assert typ == exp["type"], what
    if typ == "long":
        v = word - (1 << 64) if word >> 63 else word
    else:
        v = struct.unpack("<d", struct.pack("<Q", word))[0]
    if "positive" in exp:
        assert (v > 0) == exp["positive"], (what, v)
    elif typ == "long":
        assert v == exp["value"], (what, v)
    else:
        assert abs(v - exp["value"]) <= exp["tol"], (what, v)


@pytest.mark.parametrize("case", KATS["eval"], ids=lambda c: c[0])
def test_eval_kats(Q, case):
    N = importlib.import_module("incubator-druid_amd._native")
    text, binds, exp = case
    if exp.get("supported") is False:
        Q.parse_expression(text, check=False)  # the grammar reads it
        with pytest.raises(N.UnsupportedQuery):
            Q.parse_expression(text)
        return
    ast = Q.parse_expression(text)
    prog = Q.compile_expression(ast, lambda n: binds[n][0] if n in binds else None)
    w, poisoned = Q.run_expression(prog.ops, [tuple(binds[n]) for n in prog.inputs])
    assert not poisoned
    _check_expectation(w, prog.type, exp, text)
    v = ER.evaluate(ast, {k: tuple(x) for k, x in binds.items()})
    _check_expectation(ER.word(v), v[0], exp, text)
    assert ER.word(v) == w  # and the two agree bit for bit


def sexpr(ast):
    """Expr.toString (Expr.java: "(op l r)", "-x", "(name [a, b])")."""
    k = ast[0]
    if k in ("long", "double"):
        return repr(ast[1]) if k == "double" else str(ast[1])
    if k == "id":
        return ast[1]
    if k == "un":
        return ast[1] + sexpr(ast[2])
    if k == "bin":
        return "(%s %s %s)" % (ast[1], sexpr(ast[2]), sexpr(ast[3]))
    return "(%s [%s])" % (ast[1], ", ".join(sexpr(a) for a in ast[2]))


@pytest.mark.parametrize("case", KATS["parse"], ids=lambda c: c[0])
def test_parse_kats(Q, case):
    text, tree, idents = case
    ast = Q.parse_expression(text, check=False)
    assert sexpr(ast) == tree
    assert Q.expression_identifiers(ast) == idents


@pytest.mark.parametrize("case", KATS["flatten"], ids=lambda c: c[0])
def test_flatten_kats(Q, case):
    """Precedence and associativity (the tree), and the constant the reference folds the tree to."""
    text, tree, folded = case
    ast = Q.parse_expression(text, check=False)
    assert sexpr(ast) == tree
    if "^" in text:
        return
    prog = Q.compile_expression(ast, lambda n: None)
    w, poisoned = Q.run_expression(prog.ops, [])
    v = ER.evaluate(ast, {})
    assert not poisoned and ER.word(v) == w
    assert (str(v[1]) if v[0] == "long" else repr(v[1])) == folded


def test_lexer_and_literals(Q):
    assert Q.parse_expression("\"a b\\u0041\" + 1") == ("bin", "+", ("id", "a bA"), ("long", 1))
    assert Q.parse_expression("1. + 2") == ("bin", "+", ("double", 1.0), ("long", 2))
    assert Q.parse_expression("9223372036854775807") == ("long", LMAX)
    with pytest.raises(ValueError, match="overflows"):
        Q.parse_expression("9223372036854775808")
    with pytest.raises(ValueError, match="overflows"):
        Q.parse_expression("-9223372036854775808")  # the literal has no sign of its own (Long.parseLong of the digits)
    assert Q.parse_expression("1" + "0" * 400 + ".0") == ("double", math.inf)  # Double.parseDouble: Infinity
    # && and || share one level, left to right; comparisons too
    assert sexpr(Q.parse_expression("a || b && c")) == "(&& (|| a b) c)"
    assert sexpr(Q.parse_expression("a < b == c")) == "(== (< a b) c)"
    assert sexpr(Q.parse_expression("-a * !b")) == "(* -a !b)"
    for bad in ("1 +", "(1", "1 2", "a ? b", ".5", "f(1,", "1e5", "a = b", "'x"):
        with pytest.raises(ValueError):
            Q.parse_expression(bad)
    with pytest.raises(ValueError, match="unknown function"):
        Q.parse_expression("frobnicate(a)")
    with pytest.raises(ValueError, match="needs 3 arguments"):
        Q.parse_expression("if(a, b)")
    with pytest.raises(ValueError, match="invalid type"):
        Q.parse_expression("cast(a, 'INT')")


# ---------------------------------------------------------------------------------------------
# random trees
# ---------------------------------------------------------------------------------------------
L_CONST = (0, 1, 2, 3, 7, 100, LMAX)
D_CONST = (0.0, 0.5, 1.0, 3.0, 1.25, 1000000.0)
ARITH = ("+", "-", "*", "/", "%")
CMP = ("<", "<=", ">", ">=", "==", "!=")


def gen(rng, depth, want):
    """A random tree of static type `want` ("long" / "double"), depth <= `depth`, over the whole operator and
    function list; integer draws only."""
    def pick(seq):
        return seq[int(rng.integers(0, len(seq)))]

    def anyt(d):
        return gen(rng, d, pick(("long", "double")))

    if depth == 0 or rng.integers(0, 8) == 0:
        if rng.integers(0, 3) == 0:
            return ("long", pick(L_CONST)) if want == "long" else ("double", pick(D_CONST))
        return ("id", pick(("a", "b") if want == "long" else ("d", "e", "f")))
    d = depth - 1
    same = lambda: gen(rng, d, want)  # noqa: E731

    def mixed():  # two operands whose common type is `want`
        if want == "long":
            return gen(rng, d, "long"), gen(rng, d, "long")
        x, y = gen(rng, d, "double"), anyt(d)
        return (x, y) if rng.integers(0, 2) else (y, x)

    kind = int(rng.integers(0, 12))
    if kind == 0:
        return ("un", pick(("-", "!")), same())
    if kind in (1, 2):
        return ("bin", pick(ARITH), *mixed())
    if kind == 3:
        return ("bin", pick(CMP), *mixed())
    if kind == 4:
        return ("bin", pick(("&&", "||")), same(), same())
    if kind == 5:
        return ("fn", "abs", [same()])
    if kind == 6:
        return ("fn", pick(("min", "max")), list(mixed()))
    if kind == 7:
        return ("fn", "cast", [anyt(d), ("str", "LONG" if want == "long" else "DOUBLE")])
    if kind == 8:
        return ("fn", "if", [anyt(d), same(), same()])
    if kind == 9:
        return ("fn", "case_searched", [anyt(d), same(), anyt(d), same(), same()])
    if want == "long":
        return ("fn", "div", [anyt(d), anyt(d)])
    return ("fn", pick(("ceil", "floor")), [anyt(d)])


_TREES = {}


def random_trees(Q):
    """>= 300 accepted trees (a draw the compiler refuses for its size, or for a constant long division by zero,
    is drawn again) with their compiled programs."""
    if "t" in _TREES:
        return _TREES["t"]
    N = importlib.import_module("incubator-druid_amd._native")
    out, k = [], 0
    while len(out) < 320:
        rng = np.random.default_rng([20240519, k])
        k += 1
        tree = gen(rng, int(rng.integers(1, 6)), "long" if k % 2 else "double")
        try:
            ast = Q.parse_expression(ER.render(tree))  # through the text: the parser is under test too
            prog = Q.compile_expression(ast, COLS.get)
        except N.UnsupportedQuery:
            continue
        if len(prog.ops) > Q.EXPR_MAX_OPS - 2:  # (room for the two ops of a FLOAT output's cast)
            continue
        assert ast == _strip(tree), ER.render(tree)
        out.append((tree, ast, prog))
    assert k < 2000
    _TREES["t"] = out
    return out


def _strip(tree):
    """The generator's tree as the parser returns it (a cast's type literal is kept as written)."""
    k = tree[0]
    if k == "un":
        return ("un", tree[1], _strip(tree[2]))
    if k == "bin":
        return ("bin", tree[1], _strip(tree[2]), _strip(tree[3]))
    if k == "fn":
        return ("fn", tree[1], [_strip(a) for a in tree[2]])
    return tree


def test_random_trees_match_restatement(Q):
    trees = random_trees(Q)
    rows = special_rows()
    poisoned = ops_seen = 0
    seen = set()
    for tree, ast, prog in trees:
        seen.update(op for op, _, _ in prog.ops)
        for out_type in (None, "LONG", "DOUBLE", "FLOAT"):
            p = prog if out_type is None else prog.with_output(out_type)
            for row in rows:
                got, exp = compiled(Q, p, row), restated(ast, row, out_type)
                assert got == exp, (ER.render(tree), row, out_type, got, exp)
                poisoned += exp[1]
                ops_seen += 1
    assert seen >= set(range(Q.EX_D2F)) | set(range(Q.EX_ADD, Q.EX_IDIV + 1))  # every op class was drawn
    assert poisoned > 100 and ops_seen - poisoned > 10000


# ---------------------------------------------------------------------------------------------
# the expressions of the GPU tests (tests/test_expr_gpu.py evaluates them on the device)
# ---------------------------------------------------------------------------------------------
# over the querygen fixture's columns: v, l LONG; d, x DOUBLE; f FLOAT; __time
FIXTURE_COLS = {"v": "LONG", "l": "LONG", "d": "DOUBLE", "x": "DOUBLE", "f": "FLOAT", "d_abs": "DOUBLE", "f_abs": "FLOAT"}
VALUE_EXPRS = [
    ("x * l + 0.5", "DOUBLE"),                                   # the exact-sum expression
    ("d * f / 3.0 - x", "DOUBLE"),                               # a rounding chain, all three floating inputs
    ("if(l % 7 != 0, l / (l % 7), 0)", "LONG"),                  # guarded zero divisors: no poison
    ("v / (0 - 1)", "LONG"),                                     # MIN / -1
    ("v % (0 - 1) + abs(v)", "LONG"),                            # MIN % -1, abs(MIN)
    ("__time / 3600000 % 24", "LONG"),
    ("1 + 2 * 3", "LONG"),                                       # constant only
    ("case_searched(l > 1000 && l < 4000, l * 2, x < 0.0 || !d, 0 - l, 7)", "LONG"),
    ("cast(d, 'LONG') + cast(min(f, x), 'LONG') - div(l, 4.5)", "LONG"),
    ("max(ceil(d / 7.0), floor(f)) * (l >= v) - (d == x)", "DOUBLE"),
    ("d * 1000000000000000.0 * 100000.0", "LONG"),               # D2L saturates
    ("f * x", "FLOAT"),                                          # D2F
    ("l", "FLOAT"),                                              # L2D, D2F
]


def fixture_bindings(c, r):
    out = {k: (t, (c[k][r].item() if hasattr(c[k][r], "item") else c[k][r])) for k, t in FIXTURE_COLS.items()}
    out["__time"] = ("LONG", int(c["t"][r]))
    return out


def fixture_values(Q, text, out_type, c):
    """The restated words of `text` cast to out_type over every row of a querygen.columns() dict."""
    ast = Q.parse_expression(text)
    n = len(c["t"])
    names = Q.expression_identifiers(ast)  # (only the columns it reads, as plain Python values)
    cols = [("LONG", c["t"].tolist()) if k == "__time" else (FIXTURE_COLS[k], np.asarray(c[k]).tolist()) for k in names]
    words = np.zeros(n, dtype=np.uint64)
    for r in range(n):
        words[r] = ER.as_output(ER.evaluate(ast, {k: (t, v[r]) for k, (t, v) in zip(names, cols)}), out_type)
    return words


def test_exact_sum_expression_is_exact():
    """x * l + 0.5 over the fixture: every value a multiple of 2^-3 below 2^20 in magnitude, so any summation
    order of up to 2^30 of them gives the same double (each partial sum is a multiple of 2^-3 below 2^53 * 2^-3)."""
    import querygen
    Q = importlib.import_module("incubator-druid_amd.query")
    ast = Q.parse_expression("x * l + 0.5")
    for i in range(2):
        c = querygen.columns(i)
        for r in range(0, len(c["t"]), 1):
            v = ER.evaluate(ast, fixture_bindings(c, r))[1]
            assert abs(v) < 2.0 ** 20 and v * 8.0 == int(v * 8.0)


def test_gpu_expressions_compile_and_agree(Q):
    """Every expression of the GPU tests: compiled program == restatement over a sample of the fixture's rows
    (both long extremes of v among them)."""
    import querygen
    c = querygen.columns(1)
    rows = sorted(set(range(0, 9001, 97)) | {int(r) for r in np.nonzero(np.abs(c["v"]) > 1000)[0]})
    types = dict(FIXTURE_COLS)
    for text, out_type in VALUE_EXPRS:
        ast = Q.parse_expression(text)
        prog = Q.compile_expression(ast, types.get).with_output(out_type)
        for r in rows:
            b = fixture_bindings(c, r)
            got = Q.run_expression(prog.ops, [b[n] for n in prog.inputs])
            assert got == (ER.as_output(ER.evaluate(ast, b), out_type), False), (text, r)


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
REFUSED = [
    ("'abc'", "string literal"), ("a + 'x'", "string literal"), ("concat(a, b)", "string function concat"),
    ("strlen(a)", "string function strlen"), ("null", "null"), ("a ^ 2", "operator \\^"), ("pow(a, 2)", "function pow"),
    ("sqrt(a)", "function sqrt"), ("sin(d)", "function sin"), ("log(d)", "function log"), ("round(d)", "function round"),
    ("timestamp('2010-04-12')", "time function timestamp"), ("timestamp_floor(a, 'PT1H')", "time function timestamp_floor"),
    ("like(a, 'x')", "string function like"), ("nvl(a, 1)", "function nvl"), ("isnull(a)", "function isnull"),
    ("notnull(a)", "function notnull"), ("case_simple(a, 1, 2, 3)", "function case_simple"),
    ("case_searched(a, 1, b, 2)", "without an ELSE"), ("cast(a, 'STRING')", "cast to STRING"),
    ("cast(a, b)", "not a literal"),
]
REFUSED_TYPED = [
    ("if(a, 1, 2.0)", "branches of if differ in type"), ("case_searched(a, d, b)", "branches of case differ in type"),
    ("a && d", "operands of && differ in type"), ("d || 1", "operands of \\|\\| differ in type"),
    ("1 / 0", "constant subexpression divides a long by zero"), ("a + 7 % (2 - 2)", "divides a long by zero"),
    ("div(3, 0)", "divides a long by zero"), ("nope + 1", "no column nope"), ("s + 1", "column s is not numeric"),
    (" + ".join("c%d" % i for i in range(9)), "more than 8 input columns"),
    (" + ".join(["a"] * 34), "more than 64 ops"),
    ("a" + "".join(" + (a" for _ in range(17)) + ")" * 17, "more than 16 operands"),
]


@pytest.mark.parametrize("text,msg", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_at_parse(Q, text, msg):
    N = importlib.import_module("incubator-druid_amd._native")
    with pytest.raises(N.UnsupportedQuery, match=msg):
        Q.parse_expression(text)
    with pytest.raises(N.UnsupportedQuery, match=msg):  # wherever an expression may appear
        Q.AggregatorFactory.from_json({"type": "doubleSum", "name": "s", "expression": text})
    with pytest.raises(N.UnsupportedQuery, match=msg):
        Q.DimFilter.from_json({"type": "expression", "expression": text})
    with pytest.raises(N.UnsupportedQuery, match=msg):
        Q.ExpressionVirtualColumn("v", text)


@pytest.mark.parametrize("text,msg", REFUSED_TYPED, ids=[r[1] for r in REFUSED_TYPED])
def test_refused_at_compile(Q, text, msg):
    N = importlib.import_module("incubator-druid_amd._native")
    types = dict(COLS, s="STRING", **{"c%d" % i: "LONG" for i in range(9)})
    with pytest.raises(N.UnsupportedQuery, match=msg):
        Q.compile_expression(Q.parse_expression(text), types.get)


def test_function_names_are_case_insensitive(Q):
    """Parser.getFunction looks a name up lower-cased (Parser.java:55,67)."""
    N = importlib.import_module("incubator-druid_amd._native")
    assert Q.parse_expression("IF(a, ABS(b), Cast(d, 'LONG'))") == Q.parse_expression("if(a, abs(b), cast(d, 'LONG'))")
    assert Q.parse_expression("CASE_SEARCHED(a, 1, 2)")[1] == "case_searched"
    p = Q.compile_expression(Q.parse_expression("MAX(Ceil(d), FLOOR(a))"), COLS.get)
    assert p.ops == Q.compile_expression(Q.parse_expression("max(ceil(d), floor(a))"), COLS.get).ops
    with pytest.raises(N.UnsupportedQuery, match="function getexponent"):
        Q.parse_expression("getExponent(d)")
    with pytest.raises(N.UnsupportedQuery, match="function sqrt"):
        Q.parse_expression("SQRT(d)")
    with pytest.raises(ValueError, match="unknown function"):
        Q.parse_expression("Frobnicate(a)")


class _FakeSegment:
    """What virtual.lower_query asks of a segment, without a device."""
    num_rows = 10
    TYPES = {"a": 1, "b": 1, "f": 2, "d": 3, "lo": 4}

    def __init__(self):
        self.derived, self.timeouts = {}, []

    def column_type(self, name):
        return self.TYPES.get(name, 0)

    def derive(self, name, ops, inputs, out_type, in_use=(), cancel=None, timeout_ms=0):
        self.timeouts.append(timeout_ms)
        built = name not in self.derived
        self.derived[name] = out_type
        return {"built": int(built), "build_ms": 0.5 if built else 0.0}


def test_lowering_refuses_expressions_over_virtual_columns(Q):
    """An aggregator expression or an expression filter that names a virtual column of the query is refused by
    name: the reference binds virtual columns first, the engine derives from stored columns only. A stored
    column of the same name must not be read in its place."""
    N = importlib.import_module("incubator-druid_amd._native")
    V = importlib.import_module("incubator-druid_amd.virtual")
    segs = [_FakeSegment()]
    for name in ("v", "a"):  # "a" is also a stored column
        vcs = [{"type": "expression", "name": name, "expression": "b * 2", "outputType": "LONG"}]
        q = Q.TimeseriesQuery(intervals=IV, virtualColumns=vcs,
                              aggregations=[{"type": "longSum", "name": "s", "expression": name + " + 1"}])
        with pytest.raises(N.UnsupportedQuery, match="expression of aggregator s references virtual column " + name):
            V.lower_query(q, segs)
        q = Q.TimeseriesQuery(intervals=IV, virtualColumns=vcs, aggregations=[Q.count("n")],
                              filter={"type": "expression", "expression": name + " > 1"})
        with pytest.raises(N.UnsupportedQuery, match="expression filter references virtual column " + name):
            V.lower_query(q, segs)
        q = Q.TimeseriesQuery(intervals=IV, virtualColumns=vcs, aggregations=[
            {"type": "filtered", "filter": {"type": "expression", "expression": "b + " + name},
             "aggregator": {"type": "count", "name": "n"}}])
        with pytest.raises(N.UnsupportedQuery, match="expression filter references virtual column " + name):
            V.lower_query(q, segs)
    assert segs[0].derived == {}
    # fieldName naming the virtual column is the supported form
    q = Q.TimeseriesQuery(intervals=IV, aggregations=[Q.long_sum("s", "a")],
                          virtualColumns=[{"type": "expression", "name": "a", "expression": "b * 2", "outputType": "LONG"}])
    low = V.lower_query(q, segs)
    assert low.aggregations[0].fieldName.startswith("\x01expr:") and low.virtualColumns == []
    assert V.lower_query(low, segs) is low


def test_lowering_spends_one_timeout_budget(Q):
    """The context's timeout is one budget: every build gets what is left of it and so does the lowered query."""
    V = importlib.import_module("incubator-druid_amd.virtual")
    segs = [_FakeSegment(), _FakeSegment()]
    q = Q.TimeseriesQuery(intervals=IV, context={"timeout": 60_000}, aggregations=[
        {"type": "longSum", "name": "s%d" % k, "expression": "a + %d" % k} for k in range(3)])
    low = V.lower_query(q, segs)
    seen = segs[0].timeouts + segs[1].timeouts
    assert len(seen) == 6 and all(0 < t <= 60_000 for t in seen) and seen == sorted(seen, reverse=True)
    assert 0 < low.context["timeout"] <= seen[-1] and q.context["timeout"] == 60_000
    N = importlib.import_module("incubator-druid_amd._native")

    class Slow(_FakeSegment):
        def derive(self, *a, **kw):
            import time
            time.sleep(0.003)
            return super().derive(*a, **kw)
    with pytest.raises(N.DruidGpuError, match="DG_ERR_TIMEOUT"):
        V.lower_query(dataclasses.replace(q, context={"timeout": 1}), [Slow()])
    plain = Q.TimeseriesQuery(intervals=IV, aggregations=[{"type": "longSum", "name": "s", "expression": "a + 1"}])
    assert "timeout" not in V.lower_query(plain, segs).context and segs[0].timeouts[-1] == 0


def test_cross_process_merges_refuse_virtual_column_dimensions(Q):
    """A dimension over a virtual column is a derived LONG column per segment: no cluster-wide dictionary."""
    N = importlib.import_module("incubator-druid_amd._native")
    D = importlib.import_module("incubator-druid_amd.distributed")
    V = importlib.import_module("incubator-druid_amd.virtual")
    segs = [_FakeSegment()]
    for out_type in ("STRING", "LONG"):
        vcs = [{"type": "expression", "name": "bucket", "expression": "a / 100", "outputType": "LONG"}]
        tn = Q.TopNQuery(intervals=IV, dimension={"type": "default", "dimension": "bucket", "outputType": out_type},
                         metric="n", threshold=3, aggregations=[Q.count("n")], virtualColumns=vcs)
        gb = Q.GroupByQuery(intervals=IV, dimensions=["lo", {"type": "default", "dimension": "bucket", "outputType": out_type}],
                            aggregations=[Q.count("n")], virtualColumns=vcs)
        for lowered in (False, True):
            t, g = (V.lower_query(tn, segs), V.lower_query(gb, segs)) if lowered else (tn, gb)
            with pytest.raises(N.UnsupportedQuery, match="topN gather over the virtual column bucket"):
                D.gather_topn(None, t, None, None, [], segs)
            with pytest.raises(N.UnsupportedQuery, match="groupBy merge over the virtual column bucket"):
                D.GroupByExchange(None, g, segs)


def test_output_casts(Q):
    p = Q.compile_expression(Q.parse_expression("a + 1"), COLS.get)
    assert p.type == "long" and p.natural().out_type == "LONG" and p.natural().ops == p.ops
    assert p.with_output("DOUBLE").ops[-1][0] == Q.EX_L2D
    assert [o[0] for o in p.with_output("FLOAT").ops[-2:]] == [Q.EX_L2D, Q.EX_D2F]
    q = Q.compile_expression(Q.parse_expression("d + 1"), COLS.get)
    assert q.type == "double" and q.with_output("LONG").ops[-1][0] == Q.EX_D2L
    assert q.natural().digest() != q.with_output("FLOAT").digest() != p.natural().digest()
    assert q.natural().digest() == Q.compile_expression(Q.parse_expression("d+1"), COLS.get).natural().digest()
    assert q.natural().digest().startswith("\x01")  # no Druid column has a control character in its name


# ---------------------------------------------------------------------------------------------
# the query model
# ---------------------------------------------------------------------------------------------
IV = ["2018-03-10/2018-03-14"]


def test_aggregator_expression_json(Q):
    a = Q.AggregatorFactory.from_json({"type": "doubleSum", "name": "rev", "expression": "price * qty"})
    assert a.fieldName is None and a.expression == "price * qty"
    assert a.to_json() == {"type": "doubleSum", "name": "rev", "expression": "price * qty"}
    assert Q.AggregatorFactory.from_json(a.to_json()) == a
    f = Q.AggregatorFactory.from_json({"type": "filtered", "filter": {"type": "expression", "expression": "a > b"},
                                       "aggregator": a.to_json()})
    assert f.expression == a.expression and isinstance(f.filter, Q.ExpressionDimFilter)
    assert Q.AggregatorFactory.from_json(f.to_json()) == f
    for t in ("longSum", "doubleSum", "floatSum", "longMin", "longMax", "doubleMin", "doubleMax", "floatMin", "floatMax"):
        assert Q.AggregatorFactory(t, "n", expression="a + 1").expression == "a + 1"
    with pytest.raises(ValueError, match="exactly one"):  # SimpleDoubleAggregatorFactory.java:59
        Q.AggregatorFactory.from_json({"type": "doubleSum", "name": "r", "fieldName": "a", "expression": "a"})
    with pytest.raises(ValueError, match="fieldName or expression"):
        Q.AggregatorFactory.from_json({"type": "doubleSum", "name": "r"})
    for t in ("count", "longFirst", "doubleLast"):  # no such field in the reference
        with pytest.raises(ValueError, match="no expression field"):
            Q.AggregatorFactory(t, "n", expression="a")
    with pytest.raises(ValueError):
        Q.AggregatorFactory("longSum", "n", expression="a +")


def test_virtual_columns_json(Q):
    vc = {"type": "expression", "name": "vc", "expression": "a * 2", "outputType": "LONG"}
    base = {"dataSource": "ds", "intervals": IV, "granularity": "all",
            "aggregations": [{"type": "longSum", "name": "s", "fieldName": "vc"}]}
    for extra in ({"queryType": "timeseries"}, {"queryType": "topN", "dimension": "lo", "metric": "s", "threshold": 3},
                  {"queryType": "groupBy", "dimensions": ["lo"]}):
        js = dict(base, **extra)
        plain = Q.query_from_json(js)
        assert plain.virtualColumns == [] and "virtualColumns" not in plain.to_json()  # as it always serialized
        q = Q.query_from_json(dict(js, virtualColumns=[vc]))
        assert q.virtualColumns == [Q.ExpressionVirtualColumn("vc", "a * 2", "LONG")]
        assert q.to_json()["virtualColumns"] == [vc]
        assert Q.query_from_json(q.to_json()) == q
        assert Q.query_uses_expressions(q) and not Q.query_uses_expressions(plain)
    assert Q.ExpressionVirtualColumn("v", "a").outputType == "FLOAT"  # ExpressionVirtualColumn.java:59
    assert Q.ExpressionVirtualColumn.from_json({"type": "expression", "name": "v", "expression": "a"}).outputType == "FLOAT"
    ts = dict(base, queryType="timeseries")
    with pytest.raises(ValueError, match="duplicate virtual column"):
        Q.query_from_json(dict(ts, virtualColumns=[vc, vc]))
    with pytest.raises(ValueError, match="__time"):
        Q.query_from_json(dict(ts, virtualColumns=[dict(vc, name="__time")]))
    with pytest.raises(ValueError, match="unsupported virtual column type"):
        Q.query_from_json(dict(ts, virtualColumns=[dict(vc, type="other")]))
    N = importlib.import_module("incubator-druid_amd._native")
    with pytest.raises(N.UnsupportedQuery, match="references virtual column vc"):
        Q.query_from_json(dict(ts, virtualColumns=[vc, dict(vc, name="w", expression="vc + 1")]))
    with pytest.raises(N.UnsupportedQuery):  # the scan query keeps its refusal
        Q.query_from_json({"queryType": "scan", "intervals": IV, "virtualColumns": [vc]})
    with pytest.raises(N.UnsupportedQuery, match="virtual columns on a search query"):
        Q.query_from_json({"queryType": "search", "intervals": IV, "virtualColumns": [vc], "query":
                           {"type": "contains", "value": "a"}})


def test_expression_filter_json(Q):
    f = Q.DimFilter.from_json({"type": "and", "fields": [{"type": "expression", "expression": "a + b > 3"},
                                                          {"type": "not", "field": {"type": "expression", "expression": "d"}}]})
    assert isinstance(f.fields[0], Q.ExpressionDimFilter) and isinstance(f.fields[1].field, Q.ExpressionDimFilter)
    assert Q.DimFilter.from_json(f.to_json()) == f
    assert f.optimize() == f
    q = Q.TimeseriesQuery(intervals=IV, filter=f.to_json(), aggregations=[Q.count("n")])
    assert Q.query_uses_expressions(q) and Q.query_from_json(q.to_json()) == q
    with pytest.raises(ValueError):
        Q.DimFilter.from_json({"type": "expression", "expression": "a +"})
    # a call that was not lowered must refuse, not read 0
    N = importlib.import_module("incubator-druid_amd._native")
    with pytest.raises(N.UnsupportedQuery):
        N.make_scan(q, Q)
    with pytest.raises(N.UnsupportedQuery, match="expression filter"):
        N.FilterProgram(f, Q)


# ---------------------------------------------------------------------------------------------
# the shared evaluator header, stand-alone under UBSan
# ---------------------------------------------------------------------------------------------
def _cxx():
    for c in ("g++", "c++", "clang++"):
        if shutil.which(c):
            return c
    return None


def _line(out_code, in_types, words, ops):
    out = [str(out_code), str(len(in_types)), str(len(ops))]
    for t, w in zip(in_types, words):
        out += [str(t), "%x" % w]
    for op, arg, imm in ops:
        out += [str(op), str(arg), "%x" % imm]
    return " ".join(out)


def test_evaluator_header_under_ubsan(Q, tmp_path):
    cxx = _cxx()
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "expr_eval")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                    os.path.join(HERE, "expr_eval_main.cpp"), "-o", exe], check=True)
    lines, want = [], []

    def add(prog_ops, inputs, row, out_type, expect):
        lines.append(_line(COL_CODE[out_type], [COL_CODE[COLS[n]] for n in inputs],
                           [raw_word(COLS[n], row[n]) for n in inputs], prog_ops))
        want.append(expect)

    def add_text(text, row, out_type=None):
        ast = Q.parse_expression(text)
        p = Q.compile_expression(ast, COLS.get)
        p = p.natural() if out_type is None else p.with_output(out_type)
        w, poisoned = restated(ast, row, p.out_type)
        add(p.ops, p.inputs, row, p.out_type, (0, w, int(poisoned)))
        return w

    rows = special_rows()
    # what a plain C++ operator is undefined for
    mn = {"a": LMIN, "b": -1, "d": 0.0, "e": 0.0, "f": 0.0}
    assert add_text("a / b", mn) == LMIN & ER.M64
    assert add_text("a % b", mn) == 0
    assert add_text("abs(a)", mn) == LMIN & ER.M64
    assert add_text("-a", mn) == LMIN & ER.M64
    assert add_text("a * b - 1", mn) == LMAX  # MIN * -1 wraps to MIN, MIN - 1 to MAX
    assert add_text("div(a, b)", mn) == LMIN & ER.M64
    for dv, exp in ((math.nan, 0), (math.inf, LMAX), (-math.inf, LMIN), (1e19, LMAX), (-1e19, LMIN), (2.0 ** 63, LMAX),
                    (-(2.0 ** 63), LMIN), (2.0 ** 63 - 1024.0, 2 ** 63 - 1024), (-1.9, -1)):
        assert add_text("cast(d, 'LONG')", dict(mn, d=dv)) == exp & ER.M64
        add_text("div(d, 1.0)", dict(mn, d=dv))
        add_text("d", dict(mn, d=dv), "FLOAT")
    add_text("a / (b + 1)", mn)  # poisoned
    assert want[-1] == (0, 0, 1)
    assert add_text("if(b + 1 != 0, a / (b + 1), 5)", mn) == 5  # the guard: not poisoned
    assert add_text("b + 1 && a / (b + 1)", mn) == 0 and want[-1][2] == 0  # && is a select too
    add_text("b || a % (b + 1)", mn)
    assert want[-1][2] == 1  # b = -1 is false: the right side is the value
    # d * e + c with a product whose low bits a fused multiply-add would keep: the value is the separately rounded
    # one. (On a host without FMA instructions this holds with or without the header's contraction pragma, and on
    # the device every op round-trips through the LDS stack, so this pins the expected value, not the pragma.)
    x = 1.0 + 2.0 ** -30
    assert add_text("d * e + (0.0 - 1.0 - 0.000000001862645149230957)", dict(mn, d=x, e=x)) == ER.word(("double", 0.0))
    # every random tree over every special row, natural and FLOAT outputs
    for tree, ast, prog in random_trees(Q):
        for out_type in (None, "FLOAT"):
            p = prog.natural() if out_type is None else prog.with_output(out_type)
            for row in rows:
                w, poisoned = restated(ast, row, p.out_type)
                add(p.ops, p.inputs, row, p.out_type, (0, w, int(poisoned)))
    # what the checker refuses, each with its own code (the driver does not run those)
    I, CL, CD = (Q.EX_INPUT, 0, 0), (Q.EX_CONST_L, 0, 1), (Q.EX_CONST_D, 0, 0)
    r0 = rows[0]
    for ops, inputs, out_type, rc in (
            ([(Q.EX_ADD, 0, 0)], [], "LONG", -4), ([CL] * 17 + [(Q.EX_ADD, 0, 0)] * 16, [], "LONG", -5),
            ([CL, CL], [], "LONG", -7), ([(Q.EX_INPUT, 1, 0)], ["a"], "LONG", -3), ([(28, 0, 0)], [], "LONG", -2),
            ([CL, CD, (Q.EX_ADD, 0, 0)], [], "DOUBLE", -6), ([CL, (Q.EX_CEIL, 0, 0)], [], "DOUBLE", -6),
            ([CL, CL, CD, (Q.EX_SELECT, 0, 0)], [], "LONG", -6), ([CL], [], "DOUBLE", -8), ([CD], [], "FLOAT", -8),
            ([CD, (Q.EX_D2F, 0, 0)], [], "DOUBLE", -9), ([CD, (Q.EX_D2F, 0, 0), (Q.EX_NEG, 0, 0)], [], "FLOAT", -9),
            ([CL] + [CL, (Q.EX_ADD, 0, 0)] * 32, [], "LONG", -1), ([I], ["a"] * 9, "LONG", -10)):
        add(ops, inputs, r0, out_type, (rc, 0, 0))
    lines.append("9 0 1 1 0 1")  # output type
    want.append((-11, 0, 0))
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    got = [tuple(int(x, 16) if i == 1 else int(x) for i, x in enumerate(ln.split())) for ln in run.stdout.splitlines()]
    assert len(got) == len(want) > 15000
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, lines[i], g, w)


def test_kernel_has_no_scratch(tmp_path):
    """k_expr_eval keeps its operand stack in LDS: the compiler must report 0 bytes of scratch per lane."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    run = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-I", os.path.join(CSRC, "..", "..", "include"),
                          "-c", "-x", "hip", os.path.join(CSRC, "dg_expr.hip"), "-o", str(tmp_path / "dg_expr.o"),
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    report = run.stderr.splitlines()
    kernels = [i for i, ln in enumerate(report) if "Function Name:" in ln and "k_expr_eval" in ln]
    assert len(kernels) == 2, run.stderr  # the 8-byte and the FLOAT output
    for i in kernels:
        scratch = [ln for ln in report[i:i + 12] if "ScratchSize [bytes/lane]" in ln]
        assert scratch and scratch[0].split(":")[-1].split("[")[0].strip() == "0", report[i:i + 12]
        lds = [ln for ln in report[i:i + 12] if "LDS Size [bytes/block]" in ln]
        assert lds and int(lds[0].split("]:")[-1].split("[")[0]) >= 16 * 256 * 8, lds
