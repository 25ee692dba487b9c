"""The opt-in hash grouper's host side (CPU): the C-ABI additions (dg_groupby_run_opts,
dg_result_grouper_info, dg_groupby_opts / dg_grouper_info under ABI 16), its kernels in the gfx950 code
object, and the mapping of the query context's forceHashAggregation / bufferGrouperMaxSize
(GroupByQueryConfig.java:35-40,179-200) to the call's options. The GPU behaviour is in
test_hash_grouper_gpu.py."""
import ctypes
import importlib

import pytest


@pytest.fixture(scope="module")
def N():
    return importlib.import_module("incubator-druid_amd._native")


@pytest.fixture(scope="module")
def R():
    return importlib.import_module("incubator-druid_amd.runners")


def test_library_exports_grouper_symbols(N):
    lib = ctypes.CDLL(N.LIB_PATH)
    for name in ("dg_groupby_run_opts", "dg_result_grouper_info", "dg_groupby_run", "dg_context_set_limit"):
        assert hasattr(lib, name), name
        assert name in N.EXPORTS
    assert N.lib().dg_abi_version() == 16


def test_struct_sizes_and_constants(N):
    assert ctypes.sizeof(N.dg_groupby_opts) == 16
    assert ctypes.sizeof(N.dg_grouper_info) == 40
    assert (N.GROUPER_SORT, N.GROUPER_HASH) == (0, 1)
    assert (N.LIMIT_GROUPER, N.LIMIT_GROUPER_MAX_GROUPS) == (2, 3)
    assert N.ERRORS[N.ERR_TABLE_FULL] == "DG_ERR_TABLE_FULL"
    assert issubclass(N.TableFull, N.DruidGpuError)


def test_hash_kernels_in_gfx950_code_object(N):
    with open(N.LIB_PATH, "rb") as f:
        blob = f.read()
    assert b"gfx950" in blob
    for k in (b"k_gb_hash_insert", b"k_gb_hash_collect", b"k_gb_hash_emit", b"k_gb_hash_fill"):
        assert k in blob, k


def test_argument_errors_need_no_device(N):
    L = N.lib()
    info = N.dg_grouper_info()
    assert L.dg_result_grouper_info(None, ctypes.byref(info)) == 6  # DG_ERR_ARG
    assert L.dg_context_set_limit(None, N.LIMIT_GROUPER, 1) == 6
    with pytest.raises(N.TableFull) as e:
        N.check(5)
    assert e.value.code == 5


def test_context_keys_round_trip_and_map_to_options(N, R, Q):
    js = {"queryType": "groupBy", "dataSource": "ds", "intervals": ["1970-01-01/1971-01-01"], "granularity": "all",
          "dimensions": ["a"], "aggregations": [{"type": "count", "name": "rows"}],
          "context": {"forceHashAggregation": True, "bufferGrouperMaxSize": 1000}}
    q = Q.query_from_json(js)
    assert q.force_hash_aggregation() and q.buffer_grouper_max_size() == 1000
    assert q.to_json()["context"] == js["context"]
    assert Q.query_from_json(q.to_json()).context == js["context"]
    assert R.grouper_options(q) == (N.GROUPER_HASH, 1000)

    def mk(ctx):
        return Q.GroupByQuery(intervals=js["intervals"], dimensions=["a"], aggregations=[Q.count("rows")], context=ctx)

    assert R.grouper_options(mk({})) is None  # neither key: the plain dg_groupby_run call
    assert R.grouper_options(mk({"timeout": 5})) is None
    assert R.grouper_options(mk({"forceHashAggregation": "true"})) == (N.GROUPER_HASH, 0)  # QueryContexts.parseBoolean
    assert R.grouper_options(mk({"forceHashAggregation": False})) == (N.GROUPER_SORT, 0)
    assert R.grouper_options(mk({"bufferGrouperMaxSize": 77})) == (-1, 77)  # the grouper stays the context's
    assert R.grouper_options(mk({"bufferGrouperMaxSize": "12"})) == (-1, 12)
    assert R.grouper_options(mk({"bufferGrouperMaxSize": -3})) == (-1, 0)
