"""CPU: fq_group_aggregate_columns without a GPU.  Every shape of
tests/test_groupby_columns_gpu.py is generated and compiled for gfx950 by a
zero-length call; a one-column call generates fq_group_aggregate's source byte
for byte; every argument error has its exact text; and a numpy restatement of
the launch (groupby_columns_cases.launch_rows) shows that each of five
mistakes a kernel could make changes the expected table of a generated case."""
import ctypes as C
import os

import numpy as np
import pytest

import groupby_columns_cases as G
from fq_amd import abi, ops
from fq_amd._lib import FQError, lib
from fq_amd.expr import Col, chain, chain_columns, load, pred_tree, predicate, predicate_columns
from fuzz_groupby import apply_knobs, same, small_knobs, DEFAULTS

U64, I64, F64 = abi.DT_UINT64, abi.DT_INT64, abi.DT_FLOAT64
CUS = 256  # the restated launches: an MI355X's compute units
SPECS = {s.name: s for s in G.make_specs() + [G.zero_spec(True), G.zero_spec(False)]}
CHUNK0 = ("k2_expr", "k3_q1", "k4")  # the shapes the GPU file also runs with GROUP_CHUNKED = 0


@pytest.fixture(autouse=True)
def _knobs():
    yield
    ops.tune_reset()


def compile_spec(spec):
    key, vals, pred = spec.device()
    ops.group_compile_check_columns(spec.cdt, spec.table_aggs(), key=key, values=vals, pred=pred,
                                    key_dtype=abi.DT_BY_NAME[spec.key_t])


KNOB_SETS = [("default", name, dict(DEFAULTS)) for name in SPECS] + \
            [("small", name, small_knobs()) for name in SPECS] + \
            [("small_strided", name, small_knobs(GROUP_CHUNKED=0)) for name in CHUNK0]


@pytest.mark.parametrize("knobs,name", [(k, n) for k, n, _ in KNOB_SETS])
def test_every_gpu_shape_compiles_for_gfx950(knobs, name):
    apply_knobs(ops, next(v for k, n, v in KNOB_SETS if (k, n) == (knobs, name)))
    before = ops.jit_stats()["kernels_compiled"]
    compile_spec(SPECS[name])
    assert ops.jit_stats()["kernels_compiled"] == before + 1


# ---------------------------------------------------------------------------
# n_cols == 1 IS fq_group_aggregate
# ---------------------------------------------------------------------------
def _bitmap():
    p = abi.fq_pred()
    p.kind = abi.PRED_BITMAP
    return p


CNT, SUM3 = [(abi.AGG_COUNT, U64)], [(abi.AGG_COUNT, U64), (abi.AGG_SUM, U64), (abi.AGG_MAX, U64)]
ONE_COLUMN = {
    # name: (column dtype, aggs, key steps, [value steps], predicate, key dtype)
    "dense": (U64, SUM3, [("%", 1000)], [None, [], [("+", 1)]], None, U64),
    "hashed": (U64, SUM3, [("/", 3)], [None, [], []], None, U64),
    "column_key": (I64, [(abi.AGG_MIN, I64)], None, [[]], None, I64),
    "expr_pred": (U64, CNT, [("%", 7)], [None], lambda: predicate(U64, [("%", 8)], "<", 3), U64),
    "column_pred": (U64, CNT, [("%", 7)], [None], lambda: predicate(U64, [("%", 8)], "<", abi_col()), U64),
    "tree_pred": (U64, SUM3, [("%", 64)], [None, [], []],
                  lambda: pred_tree(U64, [([("%", 8)], "<", 3), ([], ">", 100)], [0, 1, "or"]), U64),
    "bitmap": (U64, SUM3, [("*", 3), ("%", 16)], [None, [], []], _bitmap, U64),
    "float_states": (U64, [(abi.AGG_SUM, F64), (abi.AGG_MAX, F64)], [("%", 100)], [[("*", 0.5)], [("*", 0.5)]],
                     None, U64),
    "int64_key": (U64, CNT, [("-", (5, "Int64"))], [None], None, I64),
}


def abi_col():
    from fq_amd.expr import COL
    return COL


def newest_dump(d):
    files = sorted((f for f in os.listdir(d) if f.endswith(".hip")), key=lambda f: int(f[7:-4]))
    return open(os.path.join(d, files[-1]), "rb").read(), len(files)


@pytest.mark.parametrize("name", list(ONE_COLUMN))
def test_one_column_call_generates_the_single_column_source(name, tmp_path):
    dt, aggs, key_steps, val_steps, pred, kdt = ONE_COLUMN[name]
    key = chain(dt, key_steps)[0] if key_steps is not None else None
    vals = [None if s is None or not s else chain(dt, s)[0] for s in val_steps]
    p = pred() if pred else None
    assert lib.fq_tune_jit_dump_dir(str(tmp_path).encode()) == 0
    try:
        ops.group_compile_check(dt, aggs, key=key, values=vals, pred=p, key_dtype=kdt)
        one, n1 = newest_dump(str(tmp_path))
        ops.group_compile_check_columns([dt], aggs, key=key, values=vals, pred=p, key_dtype=kdt)
        cols, n2 = newest_dump(str(tmp_path))
    finally:
        lib.fq_tune_jit_dump_dir(None)
    assert (n1, n2) == (1, 2)
    assert b"fq_jit_groupby(" in one and b"fq_jit_groupby_cols" not in one
    assert cols == one
    # and a load(0) in front of the key changes nothing either
    if key_steps:
        k0 = chain_columns([dt], [load(0)] + key_steps)[0]
        lib.fq_tune_jit_dump_dir(str(tmp_path).encode())
        try:
            ops.group_compile_check_columns([dt], aggs, key=k0, values=vals, pred=p, key_dtype=kdt)
            again, _ = newest_dump(str(tmp_path))
        finally:
            lib.fq_tune_jit_dump_dir(None)
        assert again == one


def test_dense_keys_columns_host():
    key, _ = chain(U64, [("%", 1000)])
    assert ops.group_dense_keys_columns([U64], key, 3) == ops.group_dense_keys(U64, key, 3) == 1000
    assert ops.group_dense_keys_columns([U64], None, 3) == 0
    k2, _ = chain_columns([F64, U64], [load(1), ("%", 1000)])
    assert ops.group_dense_keys_columns([F64, U64], k2, 3) == 1000
    k3, _ = chain_columns([U64, U64], [("+", Col(1)), ("%", 100000)])
    assert ops.group_dense_keys_columns([U64, U64], k3, 3) == 0       # more keys than LDS slots
    assert ops.group_dense_keys_columns([U64, U64], k2, 3) == 1000
    k4, _ = chain_columns([U64, U64], [load(1)])
    assert ops.group_dense_keys_columns([U64, U64], k4, 3) == 0
    assert ops.group_dense_keys_columns([U64] * 5, key, 3) == 0


def test_multi_column_module_holds_one_kernel(tmp_path):
    spec = SPECS["k3_q1"]
    lib.fq_tune_jit_dump_dir(str(tmp_path).encode())
    try:
        compile_spec(spec)
        src, _ = newest_dump(str(tmp_path))
    finally:
        lib.fq_tune_jit_dump_dir(None)
    assert src.count(b"__global__") == 1 and b"fq_jit_groupby_cols(const TIn0" in src
    assert b"#define GROWS 2\n" in src and b"fq_jit_groupby_bins(" not in src
    for j, t in enumerate((b"unsigned long long", b"unsigned long long", b"double")):
        assert b"typedef " + t + b" TIn%d;" % j in src


# ---------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------
W = "fq_group_aggregate_columns: "


def refused(status, text, dtypes, aggs=CNT, **kw):
    with pytest.raises(FQError) as e:
        ops.group_compile_check_columns(dtypes, aggs, **kw)
    assert (e.value.status, str(e.value)) == (status, text)


def test_argument_errors_have_their_exact_text():
    refused(abi.FQ_E_INVALID, W + "n_cols must be 1..4, got 5", [U64] * 5)
    refused(abi.FQ_E_INVALID, W + "column 1 has 5 rows, column 0 has 0", [U64, U64], lengths=[0, 5])
    refused(abi.FQ_E_UNSUPPORTED, W + "UInt32 column (scans over several columns need UInt64, Int64 or Float64 "
            "columns)", [U64, abi.DT_UINT32])
    refused(abi.FQ_E_INVALID, W + "column not aligned to its element size", [U64, U64], ptrs=[0x1000, 0x1004])
    refused(abi.FQ_E_INVALID, W + "NULL column data", [U64, U64], lengths=[5, 5])
    # a Float64 key: column 0 itself, and by an expression
    refused(abi.FQ_E_INVALID, W + "key expression is Float64, table key is UInt64", [F64, U64])
    refused(abi.FQ_E_INVALID, W + "key expression is Float64, table key is UInt64", [U64, F64],
            key=chain_columns([U64, F64], [("+", Col(1))])[0])
    refused(abi.FQ_E_INVALID, W + "key expression is Float64, table key is UInt64", [F64])
    # an argument whose type is not the state's
    refused(abi.FQ_E_INVALID, W + "argument dtype does not match the table state", [U64, F64],
            aggs=[(abi.AGG_SUM, U64)], values=[chain_columns([U64, F64], [load(1)])[0]])
    refused(abi.FQ_E_INVALID, W + "argument dtype does not match the table state", [U64],
            aggs=[(abi.AGG_SUM, F64)])
    # a column reference >= n_cols: in the key, an argument and the predicate, with two columns and with one
    for dts in ([U64, U64], [U64]):
        bad = chain_columns([U64] * 3, [load(2), ("%", 10)])[0]
        refused(abi.FQ_E_INVALID, "fq_step: column index out of range", dts, key=bad)
        refused(abi.FQ_E_INVALID, "fq_step: column index out of range", dts, aggs=[(abi.AGG_SUM, U64)],
                values=[chain_columns([U64] * 3, [("+", Col(2))])[0]])
        with pytest.raises(FQError) as e:
            ops.group_compile_check_columns(dts, CNT, pred=predicate_columns([U64] * 3, [], "<", Col(2)))
        assert e.value.status == abi.FQ_E_INVALID and "column index out of range" in str(e.value)
    # the Float64 column that fq_group_aggregate can never take is fine behind an integer key
    ops.group_compile_check_columns([F64, U64], [(abi.AGG_SUM, F64)], key=chain_columns([F64, U64], [load(1)])[0])


# ---------------------------------------------------------------------------
# the launch, restated
# ---------------------------------------------------------------------------
def restated_cases():
    """(spec, n, knobs): two rounds of a small grid plus half a tile and 3 rows, chunked and strided"""
    out = []
    for name in ("k2_expr", "k3_q1", "k4"):
        spec = SPECS[name]
        for chunked in (1, 0):
            knobs = small_knobs(GROUP_CHUNKED=chunked)
            n = G.sizes(spec.K, knobs["GROUP_THREADS"], 8)[-1]
            out.append((spec, n, knobs))
    return out


@pytest.mark.parametrize("n_cols", [2, 3, 4])
@pytest.mark.parametrize("chunked", [1, 0])
def test_restated_launch_reads_every_row_once(n_cols, chunked):
    for knobs in (small_knobs(GROUP_CHUNKED=chunked), dict(DEFAULTS, GROUP_CHUNKED=chunked)):
        T = knobs["GROUP_THREADS"]
        assert G.tile_rows(n_cols, T) == (4 if n_cols == 2 else 2) * T
        for cus in (8, CUS):
            for n in G.sizes(n_cols, T, cus) + [5 * G.tile_rows(n_cols, T) + 7]:
                if n > 1 << 21:
                    continue
                cols = G.launch_rows(n, n_cols, knobs, cus)
                assert all(c is cols[0] for c in cols)
                assert np.array_equal(np.sort(cols[0]), np.arange(n)), (n_cols, chunked, cus, n)
                grid = G.launch_grid(n, n_cols, knobs, cus)
                assert 1 <= grid <= cus and grid == max(1, min(-(-n // G.tile_rows(n_cols, T)), cus))
                tiles = G.workgroup_tiles(n, n_cols, knobs, cus)
                assert sorted(t for w in tiles for t in w) == list(range(n // G.tile_rows(n_cols, T)))
    # the two-round size gives every workgroup a second tile
    knobs = small_knobs(GROUP_CHUNKED=chunked)
    n = G.sizes(n_cols, 256, 8)[-1]
    assert min(len(w) for w in G.workgroup_tiles(n, n_cols, knobs, 8)) == 2 and n % G.tile_rows(n_cols, 256)


def test_restated_launch_gives_the_reference_table():
    for spec, n, knobs in restated_cases():
        host, keep = G.data(spec, n)
        st, exp = G.reference(spec, host, keep)
        st2, got = G.launch_expected(spec, host, keep, knobs, 8)
        assert st == st2 == "ok"
        assert same((got.keys, got.states), exp) is None


@pytest.mark.parametrize("mistake", G.MISTAKES)
def test_each_mistake_changes_a_generated_table(mistake):
    changed = []
    for spec, n, knobs in restated_cases():
        if mistake in ("key_col0", "pred_wrong_col") and spec.name != "k2_expr":
            continue  # (the shape whose key and predicate name columns 0 and 1 of one type)
        host, keep = G.data(spec, n)
        exp = G.reference(spec, host, keep)[1]
        got = G.launch_expected(spec, host, keep, knobs, 8, mistake)[1]
        if same((got.keys, got.states), exp) is not None:
            changed.append((spec.name, knobs["GROUP_CHUNKED"]))
    assert changed, mistake
    # the tile map's mistakes show under both maps
    if mistake in ("tail_dropped", "second_tile_skipped", "col1_row_off"):
        assert {c for _, c in changed} == {0, 1}


def test_zero_divisor_reference_only_counts_kept_rows():
    for kept in (True, False):
        spec = G.zero_spec(kept)
        host, keep = G.data(spec, 1027)
        assert G.reference(spec, host, keep)[0] == ("err" if kept else "ok")
