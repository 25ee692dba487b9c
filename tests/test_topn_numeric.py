"""CPU suite of the numeric topN dimensions: the C-ABI additions (dg_topn_opts, dg_topn_run_opts,
dg_topn_merge_opts, dg_segment_numeric_dim_values / _info), the TopNQuery outputType round trip, the
order-preserving key of a float's canonical bits, the TopNBinaryFn fold over signed 64-bit keys (global
mode: no device) and the cross-process path's refusal."""
import ctypes
import importlib
import struct

import numpy as np
import pytest

IV = [(0, 1 << 40)]


@pytest.fixture(scope="module")
def N():
    return importlib.import_module("incubator-druid_amd._native")


@pytest.fixture(scope="module")
def R():
    return importlib.import_module("incubator-druid_amd.runners")


def test_abi(N):
    assert ctypes.sizeof(N.dg_topn_opts) == 16
    assert (N.dg_topn_opts.output_type.offset, N.dg_topn_opts.reserved.offset, N.dg_topn_opts.out_cut_ties.offset) == (0, 4, 8)
    assert N.lib().dg_abi_version() == 16
    assert ctypes.sizeof(N.dg_topn) == 56 and ctypes.sizeof(N.dg_topn_lists) == 40 and ctypes.sizeof(N.dg_metrics) == 192
    for name in ("dg_topn_run_opts", "dg_topn_merge_opts", "dg_segment_numeric_dim_values", "dg_segment_numeric_dim_info"):
        assert name in N.EXPORTS and hasattr(N.lib(), name)
    # argument checks that need no device
    assert N.lib().dg_segment_numeric_dim_info(None, b"v", None, None, None, None) == N.ERR_ARG
    assert N.lib().dg_segment_numeric_dim_values(None, b"v", None, 0, None) == N.ERR_ARG
    assert N.lib().dg_topn_merge_opts(None, None, None, None, None, None, None, None, None) == N.ERR_ARG


def test_float_and_double_kernels_are_in_the_gfx950_code_object(N):
    data = open(N.LIB_PATH, "rb").read()
    # the three forms of each templated kernel (Itanium mangling: ILi<ViewKind>E)
    for k in (b"k_nd_minmax", b"k_nd_words", b"k_nd_encode"):
        for kind in (1, 2, 3):
            assert k + b"ILi%dE" % kind in data, (k, kind)


def test_query_json_round_trip(Q):
    aggs = [Q.count("rows")]
    plain = Q.TopNQuery(intervals=IV, dimension="v", metric="rows", threshold=3, aggregations=aggs)
    assert plain.dimension == "v" and plain.dimension_type == "STRING" and plain.to_json()["dimension"] == "v"
    for t in ("LONG", "FLOAT", "DOUBLE"):
        q = Q.TopNQuery(intervals=IV, dimension={"type": "default", "dimension": "v", "outputType": t.lower()},
                        metric="rows", threshold=3, aggregations=aggs)
        assert q.dimension == "v" and q.dimension_type == t
        js = q.to_json()
        assert js["dimension"] == {"type": "default", "dimension": "v", "outputName": "v", "outputType": t}
        back = Q.query_from_json(js)
        assert back.dimension == "v" and back.dimension_type == t and back.to_json() == js
    as_string = Q.TopNQuery(intervals=IV, dimension={"type": "default", "dimension": "v", "outputType": "STRING"},
                            metric="rows", threshold=3, aggregations=aggs)
    assert as_string.to_json() == plain.to_json() and Q.query_from_json(plain.to_json()).dimension_type == "STRING"
    with pytest.raises(ValueError):
        Q.TopNQuery(intervals=IV, dimension={"dimension": "v", "outputType": "COMPLEX"}, metric="rows", aggregations=aggs)


def _f32(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def _f64(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def test_key_transform_and_inverse(R):
    # ascending Double.compare order: -inf, negatives, -0.0, 0.0, subnormal, positives, inf, NaN
    doubles = [float("-inf"), -1.5e300, -2.0, _f64(0x8000000000000001), -0.0, 0.0, _f64(1), 2.2250738585072014e-308, 1.0,
               1.5e300, float("inf"), _f64(0x7ff8000000000000)]
    keys = [R.numeric_key(v) for v in doubles]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert all(-(1 << 63) <= k < (1 << 63) for k in keys)
    for v, k in zip(doubles, keys):
        assert struct.pack("<d", R.numeric_key_value(k)) == struct.pack("<d", v)
    # every NaN is one key (doubleToLongBits), and it comes back canonical
    for bits in (0x7ff8000000000123, 0xfff8000000000000, 0x7ff0000000000001):
        assert R.numeric_key(_f64(bits)) == keys[-1] == 0x7ff8000000000000
    floats = [float("-inf"), -3.0e38, -2.0, _f32(0x80000001), -0.0, 0.0, _f32(1), 1.17549435e-38, 1.0, 3.0e38, float("inf"),
              _f32(0x7fc00000)]
    fkeys = [R.numeric_key(v, single=True) for v in floats]
    assert fkeys == sorted(fkeys) and len(set(fkeys)) == len(fkeys) and all(-(1 << 31) <= k < (1 << 31) for k in fkeys)
    for v, k in zip(floats, fkeys):
        want = struct.pack("<f", v)
        assert struct.pack("<f", R.numeric_key_value(k, single=True)) == want
    for bits in (0x7fc00123, 0xffc00000, 0x7f800001):
        # (a signalling NaN's payload does not survive a Python float; its key is the canonical one all the same)
        assert R.numeric_key(_f32(bits), single=True) == 0x7fc00000
    assert R.numeric_key(-0.0) == -1 and R.numeric_key(0.0) == 0 and R.numeric_key(-0.0, single=True) == -1


def test_merge_opts_global_mode_with_negative_keys(Q, R):
    """TopNBinaryFn fold keyed by the long itself: shared keys combine, metric ties break by Long.compare."""
    q = Q.TopNQuery(intervals=IV, dimension={"type": "default", "dimension": "v", "outputType": "LONG"}, metric="m",
                    threshold=4, aggregations=[Q.long_sum("m", "m"), Q.count("rows")])
    K = 4
    keys = np.array([[-5, 7, -(1 << 63), 3], [7, -9, -5, (1 << 63) - 1]], dtype=np.int64)
    vals = np.array([[[10, 1], [10, 1], [4, 1], [1, 1]], [[5, 1], [20, 2], [5, 1], [15, 1]]], dtype=np.int64)
    cnt = np.array([4, 4], dtype=np.int32)
    ts = np.array([100, 200], dtype=np.int64)
    res = R.topn_merge_raw(q, cnt, keys.ravel(), vals.view(np.uint64).ravel(), K, ts, handles=None)
    t0, lists, out_keys, slots = res
    # sums: -9 -> 20, -5 -> 15, 7 -> 15, MAX -> 15, MIN -> 4, 3 -> 1; the three 15s in signed order
    assert t0 == 100 and out_keys.tolist() == [-9, -5, 7, (1 << 63) - 1]
    assert slots.view(np.int64).tolist() == [[20, 2], [15, 2], [15, 2], [15, 1]]
    # the plain call is the same fold
    plain = Q.TopNQuery(intervals=IV, dimension="v", metric="m", threshold=4, aggregations=q.aggregations)
    again = R.topn_merge_raw(plain, cnt, keys.ravel(), vals.view(np.uint64).ravel(), K, ts, handles=None)
    assert again[2].tolist() == out_keys.tolist()


def test_python_fold_breaks_ties_by_value_type(Q, R):
    aggs = [Q.count("rows")]
    for out, vals, want in (("LONG", [10, -5, 9], [-5, 9, 10]), ("STRING", ["10", "-5", "9"], ["-5", "10", "9"]),
                            ("DOUBLE", [0.0, float("nan"), -0.0, float("-inf")], None)):
        q = Q.TopNQuery(intervals=IV, dimension={"type": "default", "dimension": "v", "outputType": out}, metric="rows",
                        threshold=10, aggregations=aggs)
        r1 = Q.Result(0, [{"v": v, "rows": 1} for v in vals[:2]])
        r2 = Q.Result(0, [{"v": v, "rows": 1} for v in vals[2:]])
        got = [e["v"] for e in R.topn_binary_fn(q, r1, r2).value]
        if want is None:
            assert [struct.pack("<d", v) for v in got[:3]] == [struct.pack("<d", v) for v in (float("-inf"), -0.0, 0.0)]
            assert got[3] != got[3]
        else:
            assert got == want
    dq = Q.TopNQuery(intervals=IV, dimension={"type": "default", "dimension": "v", "outputType": "LONG"},
                     metric={"type": "dimension", "ordering": "lexicographic"}, threshold=3, aggregations=aggs)
    r = R.topn_binary_fn(dq, Q.Result(0, [{"v": 9, "rows": 1}, {"v": -5, "rows": 1}]), Q.Result(0, [{"v": 10, "rows": 2}]))
    assert [e["v"] for e in r.value] == [-5, 10, 9]


def test_distributed_refuses_numeric_dimensions(Q, N):
    D = importlib.import_module("incubator-druid_amd.distributed")
    q = Q.TopNQuery(intervals=IV, dimension={"type": "default", "dimension": "v", "outputType": "LONG"}, metric="rows",
                    threshold=3, aggregations=[Q.count("rows")])

    class Raw:
        segments = []

    with pytest.raises(N.UnsupportedQuery, match="v"):
        D.gather_topn(None, q, Raw(), None, [])

    class LongColumn:
        def column_type(self, name):
            return N.COL_LONG

    plain = Q.TopNQuery(intervals=IV, dimension="v", metric="rows", threshold=3, aggregations=[Q.count("rows")])
    with pytest.raises(N.UnsupportedQuery, match="v"):
        D.gather_topn(None, plain, Raw(), None, [], segments=[LongColumn()])
