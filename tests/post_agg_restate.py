"""The tests' own restatement of the post-aggregator ops, comparators and order keys, written from the reference
(processing/src/main/java/org/apache/druid/query/aggregation/post/): ArithmeticPostAggregator.java:107-124,206-242,
277-299, DoubleGreatestPostAggregator.java:77-92 and its three siblings, ConstantPostAggregator.java. It imports
nothing of the product: values are raw 64-bit words, a double being its bit pattern with every NaN the canonical
one (Double.doubleToLongBits), so results compare bit for bit."""
import math
import struct

AGG, CONST_D, CONST_L, L2D, D2L, ADD, SUB, MUL, DIV, QUOT, DMAX, DMIN, LMAX, LMIN = range(14)
ORDER_NONE, ORDER_DOUBLE, ORDER_LONG, ORDER_NUMERIC_FIRST = range(4)
SLOT_LONG, SLOT_DOUBLE, SLOT_FLOAT = range(3)
M64 = (1 << 64) - 1
SIGN = 1 << 63
NAN_BITS = 0x7FF8000000000000
LONG_MIN, LONG_MAX = -(1 << 63), (1 << 63) - 1


def bits(d):
    return NAN_BITS if d != d else struct.unpack("<Q", struct.pack("<d", d))[0]


def dbl(w):
    return struct.unpack("<d", struct.pack("<Q", w & M64))[0]


def to_signed(w):
    return w - (1 << 64) if w & SIGN else w


def d2l(d):
    """(long) double of the Java language (JLS 5.1.3)."""
    if d != d:
        return 0
    if d >= 2.0 ** 63:
        return LONG_MAX
    if d <= -(2.0 ** 63):
        return LONG_MIN
    return int(d)


def ieee_div(a, b):
    if b != b or b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def double_compare(a, b):
    """Double.compare."""
    if a < b:
        return -1
    if a > b:
        return 1
    x, y = to_signed(bits(a)), to_signed(bits(b))
    return (x > y) - (x < y)


def numeric_first_compare(a, b):
    """ArithmeticPostAggregator.Ordering.numericFirst.compare (:283-297)."""
    fa, fb = math.isfinite(a), math.isfinite(b)
    if fa and not fb:
        return 1
    if not fa and fb:
        return -1
    return double_compare(a, b)


def interpret(ops, slot_words, slot_classes):
    """The value of a compiled program [(op, arg, imm)] over one cell's ABI slots."""
    st = []
    for op, arg, imm in ops:
        if op == AGG:
            w = int(slot_words[arg]) & M64
            c = slot_classes[arg]
            if c == SLOT_LONG:
                st.append(w)
            elif c == SLOT_DOUBLE:
                st.append(bits(dbl(w)))
            else:
                st.append(bits(struct.unpack("<f", struct.pack("<I", w & 0xFFFFFFFF))[0]))
        elif op == CONST_D:
            st.append(bits(dbl(imm)))
        elif op == CONST_L:
            st.append(imm & M64)
        elif op == L2D:
            st.append(bits(float(to_signed(st.pop()))))
        elif op == D2L:
            st.append(d2l(dbl(st.pop())) & M64)
        elif op in (LMAX, LMIN):
            b, a = to_signed(st.pop()), to_signed(st.pop())
            st.append(((b if b > a else a) if op == LMAX else (b if b < a else a)) & M64)
        elif op in (DMAX, DMIN):
            b, a = st.pop(), st.pop()
            c = double_compare(dbl(b), dbl(a))
            st.append(b if (c > 0 if op == DMAX else c < 0) else a)
        else:
            rhs, lhs = dbl(st.pop()), dbl(st.pop())
            if op == ADD:
                r = lhs + rhs
            elif op == SUB:
                r = lhs - rhs
            elif op == MUL:
                r = lhs * rhs
            elif op == DIV:
                r = 0.0 if rhs == 0.0 else lhs / rhs
            else:
                assert op == QUOT
                r = ieee_div(lhs, rhs)
            st.append(bits(r))
    assert len(st) == 1
    return st[0]


def order_key(order, w):
    """Comparator order as unsigned key order (the header's description of the keys)."""
    if order == ORDER_NONE:
        return 0
    if order == ORDER_LONG:
        return w ^ SIGN
    d = dbl(w)
    if d != d:
        return 2 if order == ORDER_NUMERIC_FIRST else M64
    if order == ORDER_NUMERIC_FIRST and math.isinf(d):
        return 0 if d < 0 else 1
    return (~w & M64) if w & SIGN else (w | SIGN)


def compare_words(order, a, b):
    """The comparator itself over two values of a program."""
    if order == ORDER_NONE:
        return 0
    if order == ORDER_LONG:
        x, y = to_signed(a), to_signed(b)
        return (x > y) - (x < y)
    if order == ORDER_NUMERIC_FIRST:
        return numeric_first_compare(dbl(a), dbl(b))
    return double_compare(dbl(a), dbl(b))


def slot_class(out_type):
    return {"long": SLOT_LONG, "double": SLOT_DOUBLE, "float": SLOT_FLOAT}[out_type]


def value_word(v, out_type):
    """A row's aggregator value as its ABI slot."""
    if out_type == "long":
        return int(v) & M64
    if out_type == "double":
        return struct.unpack("<Q", struct.pack("<d", float(v)))[0]
    return struct.unpack("<I", struct.pack("<f", float(v)))[0]
