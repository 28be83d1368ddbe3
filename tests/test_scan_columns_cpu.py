"""fq_aggregate_columns on CPU: every shape class of a scan over several
columns of one block is generated and cross-compiled for gfx950 through
fq_jit_prepare_columns (no GPU needed -- the code object is built but not
loaded), in flat and in block mode, and the argument checks answer without a
device.  GPU parity against the oracle is in tests/test_scan_columns_gpu.py."""
import pytest

from fq_amd import abi, ops
from fq_amd._lib import FQError
from fq_amd.expr import STACK, Col, chain, chain_columns, load, pred_tree_columns, predicate, predicate_columns, push

ALL = abi.AGG_SUM | abi.AGG_MAX | abi.AGG_MIN | abi.AGG_COUNT
U64, I64, F64, I32 = abi.DT_UINT64, abi.DT_INT64, abi.DT_FLOAT64, abi.DT_INT32


@pytest.fixture(autouse=True, scope="module")
def _rtc_available():
    ops.jit_config(abi.JIT_AUTO, 1 << 22)
    if not ops.jit_prepare(U64, value=chain(U64, [("+", 1)])[0]):
        pytest.skip("hipRTC not loadable here")
    if ops.jit_stats()["available"] != 1:
        pytest.skip("hipRTC not loadable here")


def both_modes(dts, pred, value):
    """flat (no sum, or one reference block) and block mode (a filtered sum
    over more than one reference block)"""
    assert ops.jit_prepare_columns(dts, pred=pred, value=value, mask=abi.AGG_MAX | abi.AGG_MIN | abi.AGG_COUNT,
                                   block_rows=10000)
    assert ops.jit_prepare_columns(dts, pred=pred, value=value, mask=ALL, block_rows=0, length=30017)
    if pred is not None:
        assert ops.jit_prepare_columns(dts, pred=pred, value=value, mask=ALL, block_rows=10000)
        assert ops.jit_prepare_columns(dts, pred=pred, value=value, mask=ALL, block_rows=8191)


# (column dtypes, argument steps): a*b, a+b*c (PUSH), (a-b)/c, a%b, mixed dtypes
VALUES = [
    ("a*b", [U64, U64], [("*", Col(1))]),
    ("a+b*c", [U64, U64, U64], [push(1), ("*", Col(2)), ("+", STACK, True)]),
    ("(a-b)/c", [U64, U64, U64], [("-", Col(1)), ("/", Col(2))]),
    ("a%b", [U64, U64], [("%", Col(1))]),
    ("u64*i64", [U64, I64], [("*", Col(1))]),
    ("u64*f64", [U64, F64], [("*", Col(1))]),
    ("i64*f64", [I64, F64], [("*", Col(1))]),
    ("b/a from load", [U64, I64], [load(1), ("/", Col(0))]),
    ("f64-u64 reversed", [U64, F64], [("-", Col(1), True)]),
    ("(a+1)*(b-2)+c+d", [U64, I64, F64, U64],
     [("+", 1), push(1), ("-", 2), ("*", STACK, True), ("+", Col(2)), ("+", Col(3))]),
]


@pytest.mark.parametrize("name,dts,steps", VALUES, ids=[v[0] for v in VALUES])
def test_value_shapes_compile_flat_and_block(name, dts, steps):
    value, _ = chain_columns(dts, steps)
    last = len(dts) - 1
    both_modes(dts, None, value)
    both_modes(dts, predicate_columns(dts, [load(last)], "<", 5), value)


# (column dtypes, lhs steps, cmp, rhs): c<k, a<b, (a+1)>=b
PREDS = [
    ("c<k", [U64, U64, U64], [load(2)], "<", 7),
    ("a<b", [U64, U64], [], "<", Col(1)),
    ("(a+1)>=b", [U64, U64], [("+", 1)], ">=", Col(1)),
    ("u64<i64", [U64, I64], [], "<", Col(1)),
    ("i64=f64", [I64, F64], [], "=", Col(1)),
    ("a%b<c over 4", [U64, U64, U64, U64], [("%", Col(1))], "<", Col(2)),
]


@pytest.mark.parametrize("name,dts,lhs,cmp,rhs", PREDS, ids=[p[0] for p in PREDS])
def test_predicate_shapes_compile_flat_and_block(name, dts, lhs, cmp, rhs):
    pred = predicate_columns(dts, lhs, cmp, rhs)
    value, _ = chain_columns(dts, [("*", Col(len(dts) - 1))])
    both_modes(dts, pred, value)
    both_modes(dts, pred, None)


@pytest.mark.parametrize("k", [2, 3, 4])
def test_and_or_tree_with_leaves_on_different_columns(k):
    dts = [U64, I64, F64, U64][:k]
    leaves = [([], "<", Col(1)), ([load(k - 1)], "=", 7), ([("+", Col(k - 1))], ">=", 3.5)]
    pred = pred_tree_columns(dts, leaves, [0, 1, "or", 2, "and"])
    value, _ = chain_columns(dts, [push(1), ("*", Col(k - 1)), ("+", STACK, True)])
    both_modes(dts, pred, value)


@pytest.mark.parametrize("k", [2, 3, 4])
def test_bitmap_predicate_compiles(k):
    dts = [U64] * k
    pred = abi.fq_pred()
    pred.kind = abi.PRED_BITMAP
    value, _ = chain_columns(dts, [("*", Col(k - 1))])
    both_modes(dts, pred, value)


def test_column_scans_specialise_below_min_rows_and_need_the_jit():
    dts = [U64, U64]
    value, _ = chain_columns(dts, [("*", Col(1))])
    ops.jit_config(abi.JIT_AUTO, 1 << 40)
    try:
        assert ops.jit_prepare_columns(dts, value=value, mask=ALL, length=10)
        ops.jit_config(abi.JIT_OFF, 0)
        with pytest.raises(FQError) as e:
            ops.jit_prepare_columns(dts, value=value, mask=ALL)
        assert e.value.status == abi.FQ_E_UNSUPPORTED and "hipRTC" in str(e.value)
    finally:
        ops.jit_config(abi.JIT_AUTO, 1 << 22)


def invalid(dts, status, text, **kw):
    with pytest.raises(FQError) as e:
        ops.jit_prepare_columns(dts, **kw)
    assert e.value.status == status, str(e.value)
    assert text in str(e.value), str(e.value)


def test_validation_errors():
    v2, _ = chain_columns([U64, U64], [("*", Col(1))])
    invalid([], abi.FQ_E_INVALID, "n_cols")
    invalid([U64] * 5, abi.FQ_E_INVALID, "n_cols")
    invalid([U64, U64], abi.FQ_E_INVALID, "rows", value=v2, lengths=[100, 101])
    # an index >= n_cols: an operand, a PUSH, a LOAD, a predicate's right-hand column, a tree leaf's
    for steps in ([("*", Col(2))], [push(2), ("*", Col(1)), ("+", STACK, True)], [load(2), ("*", Col(1))]):
        bad, _ = chain_columns([U64, U64, U64], steps)
        invalid([U64, U64], abi.FQ_E_INVALID, "column index", value=bad)
    invalid([U64, U64], abi.FQ_E_INVALID, "column index", pred=predicate_columns([U64] * 3, [], "<", Col(2)))
    invalid([U64, U64], abi.FQ_E_INVALID, "column index",
            pred=pred_tree_columns([U64] * 3, [([], "<", Col(1)), ([], "<", Col(2))], [0, 1, "and"]))
    one, _ = chain_columns([U64, U64], [("*", Col(1))])
    invalid([U64], abi.FQ_E_INVALID, "column index", value=one)
    # LOAD anywhere but first
    late, _ = chain_columns([U64, U64], [("+", 1)])
    late.steps[1].op, late.steps[1].dtype, late.steps[1].bits = abi.OP_LOAD, U64, 1
    late.n_steps = 2
    invalid([U64, U64], abi.FQ_E_INVALID, "FQ_OP_LOAD", value=late)
    # a narrow column
    invalid([U64, I32], abi.FQ_E_UNSUPPORTED, "Int32", value=v2)
    invalid([I32], abi.FQ_E_UNSUPPORTED, "Int32")


ONE_COLUMN = [
    (U64, None, None), (U64, [("+", 1)], None), (U64, [("+", 1)], ([("%", 8)], "<", 3)),
    (I64, [("/", (-3, "Int64"))], None), (F64, [("*", 2.0)], ([], ">=", 1.5)),
]


@pytest.mark.parametrize("dt,steps,pr", ONE_COLUMN, ids=[str(c[1:]) for c in ONE_COLUMN])
@pytest.mark.parametrize("mode", [abi.JIT_OFF, abi.JIT_AUTO, abi.JIT_ALWAYS])
def test_one_column_program_reports_what_fq_jit_prepare_reports(dt, steps, pr, mode):
    value = chain(dt, steps)[0] if steps is not None else None
    pred = predicate(dt, *pr) if pr is not None else None
    ops.jit_config(mode, 1 << 22)
    try:
        want = ops.jit_prepare(dt, pred=pred, value=value, mask=ALL, block_rows=10000)
        got = ops.jit_prepare_columns([dt], pred=pred, value=value, mask=ALL, block_rows=10000)
    finally:
        ops.jit_config(abi.JIT_AUTO, 1 << 22)
    assert got == want
