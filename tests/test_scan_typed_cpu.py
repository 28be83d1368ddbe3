"""fq_aggregate_typed on CPU: the shape classes of a scan over narrow and
mixed-width columns are generated and cross-compiled for gfx950 through
fq_jit_prepare_typed (no GPU needed -- the code object is built but not
loaded): a column of every narrow type, every arithmetic operator and
comparison in Int32, UInt8 and Float32, all 45 casts of numerical_coercion,
the Q6 shape flat and in block mode.  All-64-bit shapes report what
fq_jit_prepare_columns reports from byte-identical sources, and the argument
checks answer without a device.  GPU parity against the oracle is in
tests/test_scan_typed_gpu.py."""
import glob
import os

import pytest

from fq_amd import abi, ops
from fq_amd._lib import FQError, lib
from fq_amd.expr import STACK, Col, chain, chain_columns, load, pred_tree_columns, predicate, predicate_columns, push

ALL = abi.AGG_SUM | abi.AGG_MAX | abi.AGG_MIN | abi.AGG_COUNT
I8, I16, I32, I64 = abi.DT_INT8, abi.DT_INT16, abi.DT_INT32, abi.DT_INT64
U8, U16, U32, U64 = abi.DT_UINT8, abi.DT_UINT16, abi.DT_UINT32, abi.DT_UINT64
F32, F64 = abi.DT_FLOAT32, abi.DT_FLOAT64
NAME = abi.DT_NAMES
NARROW = [I8, I16, I32, U8, U16, U32, F32]
# numerical_coercion's order: a type casts to every type before it
ORDER = [F64, F32, I64, I32, I16, I8, U64, U32, U16, U8]


@pytest.fixture(autouse=True, scope="module")
def _rtc_available():
    ops.jit_config(abi.JIT_AUTO, 1 << 22)
    if not ops.jit_prepare(U64, value=chain(U64, [("+", 1)])[0]):
        pytest.skip("hipRTC not loadable here")
    if ops.jit_stats()["available"] != 1:
        pytest.skip("hipRTC not loadable here")


def q6():
    dts = [F64, F32, I32, U8]
    pred = pred_tree_columns(dts, [([load(2)], "<", (9950, "Int32")), ([load(3)], "<", (26, "UInt8"))], [0, 1, "and"])
    value, vdt = chain_columns(dts, [("*", Col(1))])
    assert vdt == F64
    return dts, pred, value


@pytest.mark.parametrize("dt", NARROW, ids=[NAME[d] for d in NARROW])
def test_one_narrow_column_compiles(dt):
    one = (1, NAME[dt])
    value, vdt = chain_columns([dt], [("+", one)])
    assert vdt == dt
    pred = predicate_columns([dt], [], "<", (100, NAME[dt]))
    assert pred.cmp_dtype == dt
    assert ops.jit_prepare_typed([dt], pred=pred, value=value, mask=ALL, block_rows=0, length=30017)
    assert ops.jit_prepare_typed([dt], pred=pred, value=value, mask=ALL, block_rows=10000)
    assert ops.jit_prepare_typed([dt], value=None, pred=None, mask=ALL)  # the identity of a narrow column


@pytest.mark.parametrize("dt", [I32, U8, F32], ids=["Int32", "UInt8", "Float32"])
def test_every_operator_and_comparison_compiles(dt):
    dts = [dt, dt]
    k = (3, NAME[dt])
    # + - * / % against the other column, then against a constant, then reversed
    for steps in ([(op, Col(1)) for op in "+-*/%"], [(op, k) for op in "+-*/%"], [(op, k, True) for op in "-/%"]):
        value, vdt = chain_columns(dts, steps)
        assert vdt == dt and all(value.steps[i].dtype == dt for i in range(len(steps)))
        assert ops.jit_prepare_typed(dts, value=value, mask=ALL)
    value, _ = chain_columns(dts, [("+", Col(1))])
    cmps = ["=", "<", "<=", ">", ">="]
    pred = pred_tree_columns(dts, [([], c, Col(1)) for c in cmps[:4]], [0, 1, "or", 2, "or", 3, "or"])
    assert all(pred._tree.leaves[i].cmp_dtype == dt for i in range(4))
    assert ops.jit_prepare_typed(dts, pred=pred, value=value, mask=ALL, block_rows=10000)
    assert ops.jit_prepare_typed(dts, pred=predicate_columns(dts, [], cmps[4], k), value=value, mask=ALL)
    # an expression tree: (a + k) * (b - k)
    tree, vdt = chain_columns(dts, [("+", k), push(1), ("-", k), ("*", STACK, True)])
    assert vdt == dt
    assert ops.jit_prepare_typed(dts, value=tree, mask=ALL, block_rows=10000, pred=predicate_columns(dts, [], "<", k))


CAST_KERNELS = []
for _ti, _t in enumerate(ORDER[:-1]):
    for _k in range(0, len(ORDER) - _ti - 1, 3):
        CAST_KERNELS.append((_t, tuple(ORDER[_ti + 1:][_k:_k + 3])))
assert sum(len(s) for _, s in CAST_KERNELS) == 45


@pytest.mark.parametrize("T,srcs", CAST_KERNELS, ids=["%s<-%s" % (NAME[t], "+".join(NAME[s] for s in ss)) for t, ss in CAST_KERNELS])
def test_all_45_casts_compile(T, srcs):
    # x0 (type T) + x1 + x2 + x3: every step in T, each source cast to it; the last source also compared as T
    dts = [T] + list(srcs)
    value, vdt = chain_columns(dts, [("+", Col(j)) for j in range(1, len(dts))])
    assert vdt == T and all(value.steps[i].dtype == T for i in range(len(srcs)))
    pred = predicate_columns(dts, [], "<", Col(len(dts) - 1))
    assert pred.cmp_dtype == T
    assert ops.jit_prepare_typed(dts, pred=pred, value=value, mask=ALL, block_rows=1000 if len(srcs) == 3 else 0, length=5003)


def test_q6_shape_compiles_flat_and_in_block_mode():
    dts, pred, value = q6()
    assert ops.jit_prepare_typed(dts, pred=pred, value=value, mask=ALL, block_rows=0, length=1 << 27)
    assert ops.jit_prepare_typed(dts, pred=pred, value=value, mask=ALL, block_rows=10000)
    assert ops.jit_prepare_typed(dts, pred=pred, value=value, mask=ALL, block_rows=8191)
    bitmap = abi.fq_pred()
    bitmap.kind = abi.PRED_BITMAP
    assert ops.jit_prepare_typed(dts, pred=bitmap, value=value, mask=ALL, block_rows=10000)
    # below min_rows too: typed scans have no other kernel
    ops.jit_config(abi.JIT_AUTO, 1 << 40)
    try:
        assert ops.jit_prepare_typed(dts, pred=pred, value=value, mask=ALL, length=10)
    finally:
        ops.jit_config(abi.JIT_AUTO, 1 << 22)


# ---------------------------------------------------------------------------
# all-64-bit shapes: the call is fq_aggregate_columns
# ---------------------------------------------------------------------------
ONE_COLUMN = [  # tests/test_scan_columns_cpu.py ONE_COLUMN
    (U64, None, None), (U64, [("+", 1)], None), (U64, [("+", 1)], ([("%", 8)], "<", 3)),
    (I64, [("/", (-3, "Int64"))], None), (F64, [("*", 2.0)], ([], ">=", 1.5)),
]


def wide_shapes():
    out = []
    for dt, steps, pr in ONE_COLUMN:
        out.append(([dt], predicate(dt, *pr) if pr is not None else None, chain(dt, steps)[0] if steps is not None else None))
    two = [U64, I64]
    out.append((two, predicate_columns(two, [load(1)], "<", (5, "Int64")), chain_columns(two, [("*", Col(1))])[0]))
    three = [U64, I64, F64]
    out.append((three, predicate_columns(three, [], "<", Col(1)),
                chain_columns(three, [push(1), ("*", Col(2)), ("+", STACK, True)])[0]))
    return out


WIDE = wide_shapes()


@pytest.mark.parametrize("i", range(len(WIDE)))
@pytest.mark.parametrize("mode", [abi.JIT_OFF, abi.JIT_AUTO, abi.JIT_ALWAYS])
def test_all_64_bit_shapes_report_what_jit_prepare_columns_reports(i, mode):
    dts, pred, value = WIDE[i]

    def report(fn):
        try:
            return fn(dts, pred=pred, value=value, mask=ALL, block_rows=10000)
        except FQError as e:
            return (e.status, str(e))

    ops.jit_config(mode, 1 << 22)
    try:
        want = report(ops.jit_prepare_columns)
        got = report(ops.jit_prepare_typed)
    finally:
        ops.jit_config(abi.JIT_AUTO, 1 << 22)
    assert got == want


@pytest.mark.parametrize("i", range(len(WIDE)))
def test_all_64_bit_shapes_generate_byte_identical_sources(i, tmp_path):
    """Without a device nothing is cached: both entry points compile, and their dumped sources are compared.
    With a device a shape is compiled once per shape key (everything its source depends on): the typed entry
    point must then find the kernels fq_jit_prepare_columns left in the cache and compile nothing."""
    import torch
    dts, pred, value = WIDE[i]
    texts, compiled, reports = [], [], []
    for name, fn in (("columns", ops.jit_prepare_columns), ("typed", ops.jit_prepare_typed)):
        d = tmp_path / name
        d.mkdir()
        c0 = ops.jit_stats()["kernels_compiled"]
        lib.fq_tune_jit_dump_dir(str(d).encode())
        try:
            reports.append([fn(dts, pred=pred, value=value, mask=ALL, block_rows=br, length=30017) for br in (0, 10000)])
        finally:
            lib.fq_tune_jit_dump_dir(None)
        compiled.append(ops.jit_stats()["kernels_compiled"] - c0)
        files = sorted(glob.glob(os.path.join(str(d), "*.hip")), key=os.path.getmtime)
        texts.append([open(f, "rb").read() for f in files])
    assert reports[0] == reports[1]
    assert len(texts[0]) == compiled[0] and len(texts[1]) == compiled[1]
    if torch.cuda.is_available():
        assert compiled[1] == 0 and texts[1] == []  # the same shape keys: the same cached kernels
    else:
        assert texts[0] == texts[1] and compiled[0] == sum(reports[0])  # an identity scan is precompiled: no dump


def test_one_64_bit_column_accepts_a_load_of_its_one_column():
    """include/fq_gpu.h: FQ_OP_LOAD is a step of the *_columns calls, and with n_cols == 1 such a call is the
    single-column entry point.  load(0) over one column was refused there as "fq_step: bad op" (found by
    tests/test_fuzz_typed_cpu.py); a column that is not there still is a bad index."""
    for dt, k in ((I64, (3, "Int64")), (U64, 3), (F64, 2.0)):
        pred = predicate_columns([dt], [load(0), ("+", k)], "<", Col(0))
        for steps in ([load(0), ("%", k)], [load(0)]):
            value = chain_columns([dt], steps)[0]
            for fn in (ops.jit_prepare_columns, ops.jit_prepare_typed):
                for br in (0, 10000):
                    assert fn([dt], pred=pred, value=value, mask=ALL, block_rows=br)
        with pytest.raises(FQError) as e:
            ops.jit_prepare_typed([dt], value=chain_columns([dt, dt], [load(1), ("+", k)])[0], mask=ALL)
        assert e.value.status == abi.FQ_E_INVALID and "column index" in str(e.value)


# ---------------------------------------------------------------------------
# validation
# ---------------------------------------------------------------------------
def invalid(dts, status, text, **kw):
    with pytest.raises(FQError) as e:
        ops.jit_prepare_typed(dts, **kw)
    assert e.value.status == status, str(e.value)
    assert text in str(e.value), str(e.value)


def test_validation_errors():
    dts, pred, value = q6()
    invalid([], abi.FQ_E_INVALID, "n_cols")
    invalid([U8] * 5, abi.FQ_E_INVALID, "n_cols")
    invalid(dts, abi.FQ_E_INVALID, "rows", pred=pred, value=value, lengths=[100, 100, 101, 100])
    # a column index out of range: an operand, a PUSH, a LOAD, a predicate's right-hand column, a tree leaf's
    for steps in ([("*", Col(2))], [push(2), ("*", Col(1)), ("+", STACK, True)], [load(2), ("*", Col(1))]):
        bad, _ = chain_columns([I32, U8, U8], steps)
        invalid([I32, U8], abi.FQ_E_INVALID, "column index", value=bad)
    invalid([I32, U8], abi.FQ_E_INVALID, "column index", pred=predicate_columns([I32, U8, U8], [], "<", Col(2)))
    invalid(dts[:3], abi.FQ_E_INVALID, "column index", pred=pred, value=value)
    invalid([abi.DT_UTF8], abi.FQ_E_INTERNAL, "Utf8")


def test_step_types_must_be_what_numerical_coercion_yields():
    # a Float32 column operand in an Int32 step
    dts = [I32, F32]
    bad, _ = chain_columns([I32, I32], [("+", Col(1))])
    assert bad.steps[0].dtype == I32
    invalid(dts, abi.FQ_E_INVALID, "numerical_coercion", value=bad)
    # an Int32 column under a UInt8 step with a constant: the order never goes that way
    narrow, _ = chain_columns([U8], [("+", (1, "UInt8"))])
    invalid([I32], abi.FQ_E_INVALID, "numerical_coercion", value=narrow)
    # out_dtype that is not the last step's type
    good, _ = chain_columns(dts, [("+", Col(1))])
    good.out_dtype = I32
    invalid(dts, abi.FQ_E_INVALID, "out_dtype", value=good)
    # a comparison type that equal_coercion does not yield: Int32 against a Float32 column as Int32
    pred = predicate_columns([I32, I32], [], "<", Col(1))
    invalid(dts, abi.FQ_E_INVALID, "equal_coercion", pred=pred)
    # a stack operand of another type than the step's coercion
    tree, _ = chain_columns([I32, I32], [push(1), ("*", Col(1)), ("+", STACK, True)])
    invalid([I32, F32], abi.FQ_E_INVALID, "numerical_coercion", value=tree)
    # a non-numeric step type
    boolean, _ = chain_columns([U8], [("+", (1, "UInt8"))])
    boolean.steps[0].dtype = abi.DT_BOOLEAN
    invalid([U8], abi.FQ_E_UNSUPPORTED, "numeric", value=boolean)


def test_typed_scans_need_the_jit():
    dts, pred, value = q6()
    ops.jit_config(abi.JIT_OFF, 0)
    try:
        invalid(dts, abi.FQ_E_UNSUPPORTED, "hipRTC", pred=pred, value=value, mask=ALL)
        invalid([I32], abi.FQ_E_UNSUPPORTED, "hipRTC", mask=ALL)
    finally:
        ops.jit_config(abi.JIT_AUTO, 1 << 22)


def test_the_existing_entry_points_still_refuse_narrow_columns():
    value, _ = chain_columns([U64, I32], [("*", Col(1))])
    with pytest.raises(FQError) as e:
        ops.jit_prepare_columns([U64, I32], value=value)
    assert e.value.status == abi.FQ_E_UNSUPPORTED and "Int32" in str(e.value)
    assert not ops.jit_prepare(I32, mask=ALL)
    assert ops.jit_prepare_typed([U64, I32], value=value)  # the shape they refuse
