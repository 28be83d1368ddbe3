"""Filter -> Projection over narrow and mixed-width columns on CPU: the shape
classes of fq_filter_project_typed / fq_filter_project_blocks_typed /
fq_predicate_bitmap_typed are generated and cross-compiled for gfx950 through
fq_jit_prepare_project_typed (no GPU needed -- the code object is built but not
loaded), all-64-bit shapes generate the *_columns entry points' source text
byte for byte, and the argument checks answer without a device.  GPU parity
against the oracle is in tests/test_project_typed_gpu.py."""
import glob
import os

import pytest

from fq_amd import abi, ops
from fq_amd._lib import FQError, lib
from fq_amd.expr import STACK, Col, chain, chain_columns, load, pred_tree_columns, predicate, predicate_columns, push

I8, I16, I32, I64 = abi.DT_INT8, abi.DT_INT16, abi.DT_INT32, abi.DT_INT64
U8, U16, U32, U64 = abi.DT_UINT8, abi.DT_UINT16, abi.DT_UINT32, abi.DT_UINT64
F32, F64 = abi.DT_FLOAT32, abi.DT_FLOAT64


@pytest.fixture(autouse=True, scope="module")
def _rtc_available():
    ops.jit_config(abi.JIT_AUTO, 1 << 22)
    if not ops.jit_prepare(U64, value=chain(U64, [("+", 1)])[0]):
        pytest.skip("hipRTC not loadable here")
    if ops.jit_stats()["available"] != 1:
        pytest.skip("hipRTC not loadable here")


def bitmap_pred():
    p = abi.fq_pred()
    p.kind = abi.PRED_BITMAP
    return p


def dumped_sources(tmp, fn):
    before = set(glob.glob(os.path.join(tmp, "*.hip")))
    lib.fq_tune_jit_dump_dir(tmp.encode())
    try:
        fn()
    finally:
        lib.fq_tune_jit_dump_dir(None)
    new = sorted(set(glob.glob(os.path.join(tmp, "*.hip"))) - before)
    return [open(p).read() for p in new]


# ---------------------------------------------------------------------------
# all-64-bit shapes: the call is its *_columns twin
# ---------------------------------------------------------------------------
def wide_shapes():
    """(column dtypes, predicate, outputs): one and several columns; predicate none, expr and tree; 1 and 8 outputs"""
    out = []
    one = [U64]
    v1 = chain(U64, [("+", 1), ("*", 3)])[0]
    out.append((one, None, [v1]))
    out.append((one, predicate(U64, [("%", 8)], "<", 3), [v1, None]))
    out.append(([F64], predicate(F64, [("*", 2.0)], ">=", 1.5), [chain(F64, [("+", 0.5)])[0]]))
    two = [U64, I64]
    out.append((two, None, [chain_columns(two, [("*", Col(1))])[0]]))
    out.append((two, predicate_columns(two, [load(1)], "<", (5, "Int64")), [chain_columns(two, [("*", Col(1))])[0], None]))
    three = [U64, I64, F64]
    tree = pred_tree_columns(three, [([], "<", Col(1)), ([load(2)], ">=", 3.5)], [0, 1, "or"])
    out.append((three, tree, [chain_columns(three, [push(1), ("*", Col(2)), ("+", STACK, True)])[0],
                              chain_columns(three, [load(2)])[0]]))
    four = [U64] * 4
    eight = [chain_columns(four, [load(j % 4), ("+", j)])[0] for j in range(abi.MAX_PROJECT)]
    out.append((four, predicate_columns(four, [load(3)], "<", 5), eight))
    out.append((four, pred_tree_columns(four, [([], "<", Col(1)), ([load(2)], "=", 7)], [0, 1, "and"]), eight))
    return out


WIDE = wide_shapes()


@pytest.mark.parametrize("i", range(len(WIDE)))
def test_all_64_bit_shapes_generate_the_columns_source(i, tmp_path):
    assert {len(w[0]) for w in WIDE} >= {1, 2, 4} and {len(w[2]) for w in WIDE} >= {1, 8}
    assert {None if w[1] is None else w[1].kind for w in WIDE} == {None, abi.PRED_EXPR, abi.PRED_TREE}
    dts, pred, values = WIDE[i]
    for br in (0, 10000):
        old = dumped_sources(str(tmp_path), lambda: ops.jit_prepare_project_columns(dts, pred=pred, values=values,
                                                                                   block_rows=br))
        new = dumped_sources(str(tmp_path), lambda: ops.jit_prepare_project_typed(dts, pred=pred, values=values,
                                                                                 block_rows=br))
        assert len(old) == 1 and len(new) == 1
        assert new[0] == old[0]
        assert "fq_cast<" not in new[0]  # the 64-bit text, not the typed one


def test_one_64_bit_column_accepts_a_load_of_its_one_column():
    # FQ_OP_LOAD over one 64-bit column: the single-column module, whose lowering refused the step as "bad op"
    for dt, k in ((I64, (3, "Int64")), (U64, 3), (F64, 2.0)):
        pred = predicate_columns([dt], [load(0), ("+", k)], "<", Col(0))
        values = [chain_columns([dt], [load(0), ("%", k)])[0], chain_columns([dt], [load(0)])[0], None]
        for fn in (ops.jit_prepare_project_columns, ops.jit_prepare_project_typed):
            for br in (0, 10000):
                assert fn([dt], pred=pred, values=values, block_rows=br)


# ---------------------------------------------------------------------------
# narrow and mixed-width shapes compile
# ---------------------------------------------------------------------------
def q6():
    dts = [F64, F32, I32, U8]
    pred = pred_tree_columns(dts, [([load(2)], "<", (9950, "Int32")), ([load(3)], "<", (26, "UInt8"))], [0, 1, "and"])
    values = [chain_columns(dts, [("*", Col(1))])[0], chain_columns(dts, [load(3)])[0],
              chain_columns(dts, [load(1), ("*", Col(1))])[0]]
    assert [v.out_dtype for v in values] == [F64, U8, F32]
    return dts, pred, values


def every_geometry(dts, pred, values):
    for br in (0, 8192, 10000):
        assert ops.jit_prepare_project_typed(dts, pred=pred, values=values, block_rows=br)


def test_q6_shape_compiles(tmp_path):
    dts, pred, values = q6()
    every_geometry(dts, pred, values)
    src = dumped_sources(str(tmp_path), lambda: ops.jit_prepare_project_typed(dts, pred=pred, values=values))
    assert len(src) == 1  # one module per shape
    for kernel in ("fq_jit_pbits", "fq_jit_pselect", "fq_jit_pmap", "fq_jit_pblocks"):
        assert src[0].count("\n" + kernel + "(") == 1, kernel  # holding all its kernels
    # 16 rows per thread (16 * 17 B <= 384 B), groups of 4 rows (4 * 17 B <= 128 B), outputs at their own widths
    assert "#define PS_ROWS 16\n" in src[0] and "#define PB_ROWS 16\n" in src[0] and "#define PB_G 4\n" in src[0]
    assert "typedef f64 V0;" in src[0] and "typedef u8 V1;" in src[0] and "typedef f32 V2;" in src[0]


def test_u8_u16_shape_with_a_u16_output_compiles():
    dts = [U8, U16]
    value, vdt = chain_columns(dts, [("+", Col(1))])
    assert vdt == U16
    every_geometry(dts, predicate_columns(dts, [], "<", (100, "UInt8")), [value, None])


def test_int32_single_column_compiles():
    dts = [I32]
    value, vdt = chain_columns(dts, [("+", Col(0))])
    assert vdt == I32
    every_geometry(dts, predicate_columns(dts, [("%", 8)], "<", 3), [value])


def test_eight_outputs_of_mixed_widths_over_four_columns_compile():
    dts = [F64, F32, I32, U8]
    values = [chain_columns(dts, [("*", Col(1))])[0], chain_columns(dts, [load(3)])[0],
              chain_columns(dts, [load(1), ("*", Col(1))])[0], chain_columns(dts, [load(2), ("+", Col(3))])[0],
              chain_columns(dts, [load(3), ("*", Col(3))])[0], chain_columns(dts, [load(2), ("*", Col(1))])[0],
              chain_columns(dts, [load(2)])[0], None]
    assert [v.out_dtype for v in values[:-1]] == [F64, U8, F32, I32, U8, F32, I32]
    every_geometry(dts, q6()[1], values)


def test_bitmap_predicate_and_no_predicate_shapes_compile():
    dts, _, values = q6()
    assert ops.jit_prepare_project_typed(dts, pred=bitmap_pred(), values=values, block_rows=10000)
    assert ops.jit_prepare_project_typed(dts, pred=None, values=values)  # the map kernel
    assert ops.jit_prepare_project_typed([U8], pred=None, values=[None])  # a narrow pass-through column alone


def test_a_narrow_comparison_over_64_bit_columns_takes_the_typed_checks():
    # 64-bit columns alone do not make the call its twin: a UInt8 comparison of a UInt64 column is no coercion
    pred = predicate_columns([U8, U64], [], "<", (100, "UInt8"))
    with pytest.raises(FQError) as e:
        ops.jit_prepare_project_typed([U64, U64], pred=pred, values=[None])
    assert e.value.status == abi.FQ_E_INVALID and "numerical_coercion" in str(e.value)
    # a narrow step over them is a typed shape
    value, vdt = chain_columns([I64, I64], [("+", Col(1)), ("*", (1.5, "Float32"))])
    assert vdt == F32
    assert ops.jit_prepare_project_typed([I64, I64], values=[value], block_rows=10000)


def test_needs_the_jit():
    dts, pred, values = q6()
    ops.jit_config(abi.JIT_OFF, 0)
    try:
        assert not ops.jit_prepare_project_typed(dts, pred=pred, values=values)  # specialised == 0
    finally:
        ops.jit_config(abi.JIT_AUTO, 1 << 22)
    assert ops.jit_prepare_project_typed(dts, pred=pred, values=values, length=10)  # whatever min_rows says


# ---------------------------------------------------------------------------
# validation
# ---------------------------------------------------------------------------
def invalid(dts, status, text, **kw):
    with pytest.raises(FQError) as e:
        ops.jit_prepare_project_typed(dts, **kw)
    assert e.value.status == status, str(e.value)
    assert text in str(e.value), str(e.value)


def test_validation_errors():
    dts = [U8, U16]
    v = chain_columns(dts, [("+", Col(1))])[0]
    # a step type that numerical_coercion does not give: UInt8 + UInt16 typed UInt8, and typed UInt64
    for wrong in (U8, U64):
        bad = chain_columns(dts, [("+", Col(1))])[0]
        bad.steps[0].dtype = wrong
        bad.out_dtype = wrong
        invalid(dts, abi.FQ_E_INVALID, "numerical_coercion", values=[bad])
    badp = predicate_columns(dts, [], "<", Col(1))
    badp.cmp_dtype = U8
    invalid(dts, abi.FQ_E_INVALID, "equal_coercion", values=[v], pred=badp)
    invalid([], abi.FQ_E_INVALID, "n_cols")
    invalid([U8] * 5, abi.FQ_E_INVALID, "n_cols")
    invalid(dts, abi.FQ_E_INVALID, "rows", values=[v], lengths=[100, 101])
    # a column number >= n_cols: an operand, a PUSH, a LOAD, a predicate's right-hand column
    three = [U8, U16, U16]
    for steps in ([("+", Col(2))], [push(2), ("+", Col(1)), ("+", STACK, True)], [load(2), ("+", Col(1))]):
        invalid(dts, abi.FQ_E_INVALID, "column index", values=[v, chain_columns(three, steps)[0]])
    invalid(dts, abi.FQ_E_INVALID, "column index", values=[v], pred=predicate_columns(three, [load(1)], "<", Col(2)))
    invalid(dts, abi.FQ_E_INVALID, "n_out", values=[])
    invalid(dts, abi.FQ_E_INVALID, "n_out", values=[v] * 9)
    invalid(dts, abi.FQ_E_INVALID, "FQ_PROJECT_MIN_BLOCK_ROWS", values=[v], block_rows=8191)


def test_a_chain_whose_casts_exceed_the_program_is_too_long():
    # eight steps, each over a column of an earlier type of the coercion order: a cast before every step but the first
    dts = [U8, U16, U32, U64]
    steps = [("+", Col(1)), ("+", Col(2)), ("+", Col(3))]
    assert ops.jit_prepare_project_typed(dts, values=[chain_columns(dts, steps)[0]])  # three casts fit
    up = [U8, I8, I16, I32]
    climb = [("+", Col(1)), ("+", Col(2)), ("+", Col(3)), ("+", (1, "Int64")), ("+", (1.0, "Float32")), ("+", 1.0),
             ("+", 1.0), ("+", 1.0)]
    long_chain, vdt = chain_columns(up, climb)
    assert vdt == F64 and long_chain.n_steps == abi.MAX_STEPS
    with pytest.raises(FQError) as e:
        ops.jit_prepare_project_typed(up, values=[long_chain])
    assert e.value.status == abi.FQ_E_UNSUPPORTED and "too long" in str(e.value)


def test_the_columns_entry_points_still_refuse_narrow_columns():
    with pytest.raises(FQError) as e:
        ops.jit_prepare_project_columns([I32])
    assert e.value.status == abi.FQ_E_UNSUPPORTED and "Int32" in str(e.value)
    with pytest.raises(FQError) as e:
        ops.jit_prepare_project_columns([U64, I32], values=[chain_columns([U64, U64], [("*", Col(1))])[0]])
    assert e.value.status == abi.FQ_E_UNSUPPORTED and "Int32" in str(e.value)


def test_workspace_holds_one_status_word_per_typed_tile():
    n = 1 << 24

    def ws(dts):
        arr = (abi.fq_col * len(dts))(*[abi.fq_col(None, n, dt, 0) for dt in dts])
        return lib.fq_filter_project_typed_workspace_bytes(n, arr, len(dts))

    # tiles of 256 * 16 rows at the most (an 8-byte output may be among them): one status word each
    assert ws([U8]) == ws([U8, U16]) == (2 + 16 + n // 4096) * 8
    assert ws([F64, F32, I32, U8]) >= ws([U8])
    # never below the 64-bit twin's
    for k in (1, 2, 3, 4):
        assert ws([U64] * k) >= lib.fq_filter_project_columns_workspace_bytes(n, k)
