"""Writes expr_kats.json: known answers for the numeric expression engine, transcribed by hand as data from the
assertions of the reference's EvalTest (testDoubleEval, testLongEval, testBooleanReturn) and ParserTest
(common/src/test/java/org/apache/druid/math/expr/).

eval: [expression, bindings {name: [type, value]}, expectation]. An expectation is what the reference's test
asserts and no more: {"type", "value"} (a long exactly, a double within "tol") or {"type", "positive"} for its
assertTrue / assertFalse(value > 0). "supported": false marks a case over a construct the engine refuses (^,
sqrt): the parser still has to read it, the compiler has to refuse it.
parse: [expression, Expr.toString() of the unflattened tree, the identifiers in first-use order].
flatten: [expression, Expr.toString() of the unflattened tree, the constant Parser.flatten folds it to].

Run: python tests/golden/make_expr_kats.py"""
import json
import os

LMAX = 9223372036854775807


def d(value, tol=0.0001):
    return {"type": "double", "value": value, "tol": tol}


def l(value):
    return {"type": "long", "value": value}


def pos(t, positive):
    return {"type": t, "positive": positive}


X2 = {"x": ["DOUBLE", 2.0]}
XL = {"x": ["LONG", LMAX]}
XYZW = {"x": ["LONG", 100], "y": ["LONG", 100], "z": ["DOUBLE", 100.0], "w": ["DOUBLE", 100.0]}

EVAL = [
    # testDoubleEval
    ["x", X2, d(2.0)], ["\"x\"", X2, d(2.0)], ["300 + \"x\" * 2", X2, d(304.0)],
    ["1.0 && 0.0", X2, pos("double", False)], ["1.0 && 2.0", X2, pos("double", True)],
    ["1.0 || 0.0", X2, pos("double", True)], ["0.0 || 0.0", X2, pos("double", False)],
    ["2.0 > 1.0", X2, pos("double", True)], ["2.0 >= 2.0", X2, pos("double", True)],
    ["1.0 < 2.0", X2, pos("double", True)], ["2.0 <= 2.0", X2, pos("double", True)],
    ["2.0 == 2.0", X2, pos("double", True)], ["2.0 != 1.0", X2, pos("double", True)],
    ["2.0 + 1.5", X2, d(3.5)], ["2.0 - 1.5", X2, d(0.5)], ["2.0 * 1.5", X2, d(3.0)], ["2.0 / 0.5", X2, d(4.0)],
    ["2.0 % 0.3", X2, d(0.2)], ["2.0 ^ 3.0", X2, dict(d(8.0), supported=False)], ["-1.5", X2, d(-1.5)],
    ["!-1.0", X2, pos("double", True)], ["!0.0", X2, pos("double", True)], ["!2.0", X2, pos("double", False)],
    ["sqrt(4.0)", X2, dict(d(2.0), supported=False)], ["if(1.0, 2.0, 3.0)", X2, d(2.0)], ["if(0.0, 2.0, 3.0)", X2, d(3.0)],
    # testLongEval
    ["x", XL, l(LMAX)], ["\"x\"", XL, l(LMAX)], ["\"x\" / 100 + 1", XL, l(92233720368547759)],
    ["9223372036854775807 && 0", XL, pos("long", False)],
    ["9223372036854775807 && 9223372036854775806", XL, pos("long", True)],
    ["9223372036854775807 || 0", XL, pos("long", True)],
    ["-9223372036854775807 || -9223372036854775807", XL, pos("long", False)],
    ["-9223372036854775807 || 9223372036854775807", XL, pos("long", True)], ["0 || 0", XL, pos("long", False)],
    ["9223372036854775807 > 9223372036854775806", XL, pos("long", True)],
    ["9223372036854775807 >= 9223372036854775807", XL, pos("long", True)],
    ["9223372036854775806 < 9223372036854775807", XL, pos("long", True)],
    ["9223372036854775807 <= 9223372036854775807", XL, pos("long", True)],
    ["9223372036854775807 == 9223372036854775807", XL, pos("long", True)],
    ["9223372036854775807 != 9223372036854775806", XL, pos("long", True)],
    ["9223372036854775806 + 1", XL, l(LMAX)], ["9223372036854775807 - 1", XL, l(LMAX - 1)],
    ["4611686018427387903 * 2", XL, l(LMAX - 1)], ["9223372036854775806 / 2", XL, l(4611686018427387903)],
    ["9223372036854775807 % 9223372036854775800", XL, l(7)],
    ["3037000499 ^ 2", XL, dict(l(9223372030926249001), supported=False)],
    ["-9223372036854775807", XL, l(-LMAX)],
    ["!-9223372036854775807", XL, pos("long", True)], ["!0", XL, pos("long", True)],
    ["!9223372036854775807", XL, pos("long", False)],
    ["cast(sqrt(9223372036854775807), 'long')", XL, dict(l(3037000499), supported=False)],
    ["if(x == 9223372036854775807, 1, 0)", XL, l(1)], ["if(x - 1 == 9223372036854775807, 1, 0)", XL, l(0)],
    # testBooleanReturn
    ["x==y", XYZW, pos("long", True)], ["x!=y", XYZW, pos("long", False)], ["x==z", XYZW, pos("double", True)],
    ["x!=z", XYZW, pos("double", False)], ["z==w", XYZW, pos("double", True)], ["z!=w", XYZW, pos("double", False)],
]

PARSE = [
    ["-x", "-x", ["x"]], ["!x", "!x", ["x"]],
    ["x>y", "(> x y)", ["x", "y"]], ["x<y", "(< x y)", ["x", "y"]], ["x<=y", "(<= x y)", ["x", "y"]],
    ["x>=y", "(>= x y)", ["x", "y"]], ["x==y", "(== x y)", ["x", "y"]], ["x!=y", "(!= x y)", ["x", "y"]],
    ["x && y", "(&& x y)", ["x", "y"]], ["x || y", "(|| x y)", ["x", "y"]],
    ["x+y", "(+ x y)", ["x", "y"]], ["x-y", "(- x y)", ["x", "y"]],
    ["x+y+z", "(+ (+ x y) z)", ["x", "y", "z"]], ["x+y-z", "(- (+ x y) z)", ["x", "y", "z"]],
    ["x-y+z", "(+ (- x y) z)", ["x", "y", "z"]], ["x-y-z", "(- (- x y) z)", ["x", "y", "z"]],
    ["x-y-x", "(- (- x y) x)", ["x", "y"]],
    ["x*y", "(* x y)", ["x", "y"]], ["x/y", "(/ x y)", ["x", "y"]], ["x%y", "(% x y)", ["x", "y"]],
    ["foo", "foo", ["foo"]], ["\"foo\"", "foo", ["foo"]], ["\"foo bar\"", "foo bar", ["foo bar"]],
    ["\"foo\\\"bar\"", "foo\"bar", ["foo\"bar"]],
    ["sqrt(x)", "(sqrt [x])", ["x"]], ["if(cond,then,else)", "(if [cond, then, else])", ["cond", "then", "else"]],
]

FLATTEN = [
    ["1", "1", "1"], ["-1", "-1", "-1"], ["--1", "--1", "1"], ["-1+2", "(+ -1 2)", "1"], ["-1*2", "(* -1 2)", "-2"],
    ["-1^2", "(^ -1 2)", "1"],
    ["1*2*3", "(* (* 1 2) 3)", "6"], ["1*2/3", "(/ (* 1 2) 3)", "0"], ["1/2*3", "(* (/ 1 2) 3)", "0"],
    ["1/2/3", "(/ (/ 1 2) 3)", "0"],
    ["1.0*2*3", "(* (* 1.0 2) 3)", "6.0"], ["1.0*2/3", "(/ (* 1.0 2) 3)", "0.6666666666666666"],
    ["1.0/2*3", "(* (/ 1.0 2) 3)", "1.5"], ["1.0/2/3", "(/ (/ 1.0 2) 3)", "0.16666666666666666"],
    ["1^2", "(^ 1 2)", "1"], ["1^2^3", "(^ 1 (^ 2 3))", "1"],
    ["1+2*3", "(+ 1 (* 2 3))", "7"], ["1+(2*3)", "(+ 1 (* 2 3))", "7"], ["(1+2)*3", "(* (+ 1 2) 3)", "9"],
    ["1*2+3", "(+ (* 1 2) 3)", "5"], ["(1*2)+3", "(+ (* 1 2) 3)", "5"], ["1*(2+3)", "(* 1 (+ 2 3))", "5"],
    ["1+2^3", "(+ 1 (^ 2 3))", "9"], ["1+(2^3)", "(+ 1 (^ 2 3))", "9"], ["(1+2)^3", "(^ (+ 1 2) 3)", "27"],
    ["1^2+3", "(+ (^ 1 2) 3)", "4"], ["(1^2)+3", "(+ (^ 1 2) 3)", "4"], ["1^(2+3)", "(^ 1 (+ 2 3))", "1"],
    ["1^2*3+4", "(+ (* (^ 1 2) 3) 4)", "7"], ["-1^2*-3+-4", "(+ (* (^ -1 2) -3) -4)", "-7"],
    ["max(3, 4)", "(max [3, 4])", "4"], ["min(1, max(3, 4))", "(min [1, (max [3, 4])])", "1"],
]

if __name__ == "__main__":
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "expr_kats.json")
    with open(out, "w") as f:
        json.dump({"eval": EVAL, "parse": PARSE, "flatten": FLATTEN}, f, indent=1)
        f.write("\n")
    print(out)
