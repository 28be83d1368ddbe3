"""GPU: the Filter -> Projection block stream over nullable columns
(fq_filter_project_blocks_nullable, fq_predicate_bitmap_nullable) against
oracle/fq_ref.py; cases, oracle and comparison rules are
tests/project_nullable_cases.py's (values bit for bit where the expected
validity bit is 1, any NaN equal to any NaN; the output bitmap as whole words,
zeros outside the kept ranges; per-block counts; no tolerance).

Every check also asserts what must not be touched: the sentinel word after
each output bitmap's ceil(len / 64) words and after each input bitmap, and the
fill under the rows past a block's count.

Shapes: the Q6 layout Float64, Float32, Int32, UInt8; UInt8, UInt16 (a + b in
UInt16) with one comparison and with an `or` tree; one UInt64 column cast to
Int64.  Layouts: all columns aligned; all offset by one row and one column
offset (every group then lies off the row group's grid, or the columns share
no phase: the element path, one bit per row); all offset by G - 1 rows with
blocks of 10,001 rows (odd blocks are on the grid with their groups crossing
bitmap words: the two-word path).  A bitmap's bit 0 is row 0 of its column's
view in every layout.  Sizes: PC.SIZES."""
import numpy as np
import pytest

import fq_ref as R
import project_nullable_cases as PC
from fq_amd import abi
from fq_amd._lib import FQError
from fq_amd.expr import Col, chain_columns, load, predicate_columns

pytestmark = pytest.mark.gpu

I8, I16, U8, U16, U64, F64 = PC.I8, PC.I16, PC.U8, PC.U16, PC.U64, PC.F64
FILL = PC.FILL
SENTINEL = int(np.full(8, FILL, np.uint8).view(np.uint64)[0])
IN_SENTINEL = 0x5A5A5A5A5A5A5A5A
LAYOUTS = ("aligned", "all_offset", "one_offset")
ops = None


def setup_module():
    global ops
    from fq_amd import ops as _ops
    _ops.require_gpu()
    ops = _ops


def offsets(layout, K, G=4):
    if layout == "aligned":
        return [0] * K
    if layout == "all_offset":
        return [1] * K
    if layout == "one_offset":
        return [1] if K == 1 else [0, 1] + [0] * (K - 2)
    assert layout == "cross"
    return [G - 1] * K


def numpy_dev(arr, dt, off):
    """the rows of arr starting `off` elements into a 256-byte aligned buffer"""
    pad = np.zeros(off + len(arr), dtype=arr.dtype)
    pad[off:] = arr
    c = ops.from_numpy(pad, dt)
    assert c.ptr % 256 == 0
    return ops.DeviceColumn(c.buf, len(arr), dt, offset=arr.dtype.itemsize * off)


def bitmap_dev(valid):
    """an Arrow validity bitmap on the device: bit i = valid[i], the bits past the last row set, then a sentinel word"""
    if valid is None:
        return None
    words = np.append(PC.pack_bits(valid, pad=True), np.uint64(IN_SENTINEL))
    return ops.from_numpy(words, U64)


def device(case, layout="aligned"):
    out_dts = [case.dts[0] if v is None else v.out_dtype for v in case.values]
    offs = offsets(layout, len(case.dts), PC.geometry(case.dts, out_dts)[1])
    return [numpy_dev(h, dt, o) for h, dt, o in zip(case.host, case.dts, offs)], [bitmap_dev(v) for v in case.valid]


def words_of(col):
    return col.buf[col.offset:col.offset + 8 * col.len].cpu().numpy().view(np.uint64)


def check_blocks(case, block_rows, layout="aligned", out_offset=0, fill=FILL, out_validity=None):
    want = case.oracle(block_rows)
    cols, vbs = device(case, layout)
    outs, outv, cnt, kept = ops.filter_project_blocks_nullable(cols, vbs, block_rows, case.pred, case.values,
                                                               out_offset=out_offset, fill=fill, out_validity=out_validity)
    what = (case.name, case.n, block_rows, layout, out_offset)
    assert list(cnt) == want["counts"], what
    assert kept == sum(want["counts"]), what
    nw = (case.n + 63) // 64
    fillword = int(np.full(8, fill, np.uint8).view(np.uint64)[0])
    for j, (o, ov) in enumerate(zip(outs, outv)):
        dt = want["dts"][j]
        assert o.dtype == dt, what
        got = o.to_numpy()
        words = words_of(ov)
        assert int(words[nw]) == fillword, what + (j, "the word after the bitmap")
        if out_validity is not None and out_validity[j] is None:
            assert np.all(words[:nw] == np.uint64(fillword)), what + (j, "a bitmap that was not passed")
            assert want["bits"][j][want["kept"]].all(), what
        else:
            assert np.array_equal(words[:nw], PC.pack_bits(want["bits"][j])), what + (j, "validity")
        assert PC.same(got, want["rows"][j], dt, want["bits"][j]), what + (j, "values under 1 bits")
        fillrows = np.full(case.n * got.dtype.itemsize, fill & 0xFF, np.uint8).view(got.dtype)
        assert PC.same(got, fillrows, dt, ~want["kept"]), what + (j, "rows past a count")
    for v, vb in zip(case.valid, vbs):
        if vb is not None:
            w = words_of(vb)
            assert int(w[-1]) == IN_SENTINEL and np.array_equal(w[:-1], PC.pack_bits(v, pad=True)), what
    return outs, outv, cnt


def check_bitmap(case, layout="aligned"):
    cols, vbs = device(case, layout)
    bm = ops.predicate_bitmap_nullable(cols, vbs, case.pred)
    want = case.oracle_bitmap()
    assert np.array_equal(bm.to_numpy(), want), (case.name, case.n, layout)
    words = bm.buf[bm.offset:bm.offset + bm.nbytes()].cpu().numpy().view(np.uint64)
    if case.n % 64:
        assert int(words[-1]) >> (case.n % 64) == 0, (case.name, case.n, layout)  # bits past n are cleared


# ---------------------------------------------------------------------------
# shapes x layouts x sizes x null patterns
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", list(PC.SHAPES))
def test_sizes_and_layouts(shape, layout):
    for n, br in PC.SIZES:
        check_blocks(PC.get_case(shape, n, "random"), br, layout)


@pytest.mark.parametrize("shape", list(PC.SHAPES))
def test_groups_that_cross_bitmap_words(shape):
    # blocks of 10,001 rows behind G - 1 rows of offset: block 1 starts on the grid, one row into a group of bits
    case = PC.get_case(shape, 25003, "random")
    check_blocks(case, 10001, "cross")
    check_blocks(PC.get_case(shape, 25003, "ones"), 10001, "cross")


@pytest.mark.parametrize("pattern", [p for p in PC.PATTERNS if p != "random"])
@pytest.mark.parametrize("shape", list(PC.SHAPES))
def test_null_patterns(shape, pattern):
    n, br = PC.SIZES[0]
    case = PC.get_case(shape, n, pattern)
    want = case.oracle(br)
    if pattern == "pred_null" and shape != "u8u16":
        assert sum(want["counts"]) == 0  # the predicate's column all null: nothing is kept
    if pattern == "first_null":
        assert not want["bits"][0].any()  # every value of output 0 is null
    for layout in LAYOUTS:
        check_blocks(case, br, layout)


@pytest.mark.parametrize("shape", list(PC.SHAPES))
def test_output_offset_by_one_element(shape):
    # the values' ragged head before the first 16-byte store; the bitmap's bit 0 stays the output's row 0
    check_blocks(PC.get_case(shape, 25003, "random"), 10000, "aligned", out_offset=1)


@pytest.mark.parametrize("shape", ["q6", "u8u16", "u8u16_or", "u64cast"])
def test_all_ones_bitmaps_equal_the_typed_call_byte_for_byte(shape):
    n, br = PC.SIZES[0]
    case = PC.get_case(shape, n, "ones")
    if shape == "u64cast":  # the typed call refuses a cast that leaves its range: none here
        case = case.replace(host=[case.host[0] >> np.uint64(2)])
    outs, outv, cnt = check_blocks(case, br)
    cols, _ = device(case)
    touts, tcnt, tkept = ops.filter_project_blocks_typed(cols, br, case.pred, case.values, fill=FILL)
    assert list(cnt) == list(tcnt)
    for o, t in zip(outs, touts):
        assert np.array_equal(o.to_numpy().view(np.uint8), t.to_numpy().view(np.uint8))
    want = case.oracle(br)
    for ov in outv:  # all ones on the kept ranges, zero elsewhere
        assert np.array_equal(words_of(ov)[:-1], PC.pack_bits(want["kept"]))


def test_stale_output_bitmaps_are_zeroed():
    for shape in PC.SHAPES:
        check_blocks(PC.get_case(shape, 25003, "random"), 10000, fill=0xFF)  # bitmaps pre-filled with ones


def test_no_predicate_runs_through_the_block_kernel():
    for shape in ("q6", "u64cast"):
        base = PC.get_case(shape, 25003, "random")
        case = PC.Case(base.name, base.names, base.dts, base.host, base.valid, None, base.values, None, None, base.exprs,
                       None, None)
        assert case.oracle(10000)["counts"] == [10000, 10000, 5003]
        for layout in LAYOUTS:
            check_blocks(case, 10000, layout)


def test_an_always_valid_output_takes_a_null_bitmap():
    case = PC.get_case("u64cast", 25003, "none")  # x + 1 as Int64 can be null, x itself cannot
    check_blocks(case, 10000, out_validity=[True, None])
    cols, vbs = device(case)
    with pytest.raises(FQError) as e:
        ops.filter_project_blocks_nullable(cols, vbs, 10000, case.pred, case.values, out_validity=[None, True])
    assert e.value.status == abi.FQ_E_INVALID and "output 0, which can hold nulls" in str(e.value)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", list(PC.SHAPES))
def test_predicate_bitmap(shape, layout):
    for n in (25003, 8192, 1, 63, 64, 65):
        check_bitmap(PC.get_case(shape, n, "random"), layout)
    check_bitmap(PC.get_case(shape, 25003, "pred_null"), layout)


def test_needs_the_jit():
    case = PC.get_case("q6", 8192, "random")
    cols, vbs = device(case)
    ops.jit_config(abi.JIT_OFF, 0)
    try:
        for run in (lambda: ops.filter_project_blocks_nullable(cols, vbs, 10000, case.pred, case.values),
                    lambda: ops.predicate_bitmap_nullable(cols, vbs, case.pred)):
            with pytest.raises(FQError) as e:
                run()
            assert e.value.status == abi.FQ_E_UNSUPPORTED and "no unfused path over nulls" in str(e.value)
    finally:
        ops.jit_config(abi.JIT_AUTO, 1 << 22)


# ---------------------------------------------------------------------------
# casts: out of range is a null, never an error
# ---------------------------------------------------------------------------
def test_uint64_beyond_int64_is_a_null_at_the_first_row_inside_a_tile_and_at_the_last_row():
    n, br = PC.SIZES[0]
    for pattern in ("none", "random"):
        base = PC.get_case("u64cast", n, pattern)
        x = base.host[0].copy()
        rows = [0, 5000, n - 1]
        x[rows] = np.uint64(1 << 63)  # 2^63 % 8 = 0: kept
        valid = base.valid
        if valid[0] is not None:
            v = valid[0].copy()
            v[rows] = True
            valid = [v]
        case = base.replace(host=[x], valid=valid)
        want = case.oracle(br)
        pos = [0, int(np.count_nonzero(case.oracle_bitmap()[:5000])), 20000 + want["counts"][2] - 1]
        assert all(want["kept"][p] and not want["bits"][0][p] and want["bits"][1][p] for p in pos)
        for layout in LAYOUTS:
            check_blocks(case, br, layout)


def case_i8_over_u64(n):
    """a / b as Int8 over Int8, UInt64, no predicate: a divisor of 256 does not fit Int8 -- a null, and no zero"""
    rng = np.random.default_rng(5000003 + n)
    dts = [I8, U64]
    b = rng.integers(1, 100, n).astype(np.uint64)
    b[rng.random(n) < 0.1] = 256
    b[[0, n - 1]] = 256
    value, vdt = chain_columns(dts, [("/", Col(1))])
    assert vdt == I8
    return PC.Case("i8_over_u64", ["a", "b"], dts, [rng.integers(-128, 128, n).astype(np.int8), b], [None, None], None,
                   [value], None, None, [R.Arith("/", PC.fld("a"), PC.fld("b"))], None, None)


def test_a_divisor_that_does_not_fit_its_cast_is_a_null_not_a_zero():
    n, br = PC.SIZES[0]
    case = case_i8_over_u64(n)
    want = case.oracle(br)
    assert not want["bits"][0][0] and not want["bits"][0][n - 1] and want["bits"][0].sum() > n // 2
    for layout in LAYOUTS:
        check_blocks(case, br, layout)
    # with the divisor's bitmap (10 % nulls, zero divisors under them) the same
    rng = np.random.default_rng(11)
    vb = rng.random(n) >= 0.1
    b = case.host[1].copy()
    b[~vb] = 0
    check_blocks(case.replace(host=[case.host[0], b], valid=[None, vb]), br)


# ---------------------------------------------------------------------------
# zero divisors: a predicate's on any row first, then a value's on a kept row
# ---------------------------------------------------------------------------
def case_div(n, seed=0):
    """a / c WHERE a % b < 5 over three Int16 columns, every one with a bitmap; zero divisors only under 0 bits"""
    rng = np.random.default_rng(6000003 + n + seed)
    dts = [I16, I16, I16]
    host = [rng.integers(0, 30000, n).astype(np.int16)] + [rng.integers(1, 50, n).astype(np.int16) for _ in range(2)]
    valid = [rng.random(n) >= 0.1 for _ in range(3)]
    host[1][~valid[1]] = 0
    host[2][~valid[2]] = 0
    pred = predicate_columns(dts, [("%", Col(1))], "<", (5, "Int16"))
    value, vdt = chain_columns(dts, [("/", Col(2))])
    assert vdt == I16 and pred.cmp_dtype == I16
    where = R.Compare("<", R.Arith("%", PC.fld("a"), PC.fld("b")), PC.const(5, "Int16"))
    return PC.Case("div", ["a", "b", "c"], dts, host, valid, pred, [value], where, None,
                   [R.Arith("/", PC.fld("a"), PC.fld("c"))], None, None)


def expect_div_zero(case, br):
    with pytest.raises(R.RefError) as r:
        case.oracle(br)
    assert "Divide by zero" in str(r.value)
    for layout in ("aligned", "one_offset"):
        cols, vbs = device(case, layout)
        with pytest.raises(FQError) as e:
            ops.filter_project_blocks_nullable(cols, vbs, br, case.pred, case.values)
        assert e.value.status == abi.FQ_E_DIVIDE_BY_ZERO and str(e.value) == PC.DIV_ZERO, str(e.value)


def test_zero_divisors():
    n, br = PC.SIZES[0]
    base = case_div(n)
    for layout in LAYOUTS:
        check_blocks(base, br, layout)  # zero divisors under 0 bits only: no error, no flag
    keep = base.oracle_bitmap()
    dropped = [int(r) for r in np.flatnonzero(~keep & base.valid[0] & base.valid[1] & base.valid[2])]
    kept = [int(r) for r in np.flatnonzero(keep & base.valid[2])]
    spots = lambda rows: [rows[0], rows[len(rows) // 2], rows[-1]]  # near the first row, inside a tile, near the last
    for r in spots(dropped):
        # a valid zero divisor in the predicate, on a row that would be dropped anyway: the call fails
        b = base.host[1].copy()
        b[r] = 0
        expect_div_zero(base.replace(host=[base.host[0], b, base.host[2]]), br)
        # one in a value on a dropped row: no error
        c = base.host[2].copy()
        c[r] = 0
        check_blocks(base.replace(host=[base.host[0], base.host[1], c]), br)
    for r in spots(kept):
        c = base.host[2].copy()
        c[r] = 0
        expect_div_zero(base.replace(host=[base.host[0], base.host[1], c]), br)
    # a zero divisor whose other operand is null raises nothing either
    r = int(np.flatnonzero(~base.valid[0] & base.valid[1])[0])
    b = base.host[1].copy()
    b[r] = 0
    check_blocks(base.replace(host=[base.host[0], b, base.host[2]]), br)


# ---------------------------------------------------------------------------
# the ticket loop: workgroups draw a second block
# ---------------------------------------------------------------------------
def test_workgroups_that_draw_a_second_block():
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = (cus + 3) * 10000 - 7
    case = PC.get_case("q6", n, "random")
    assert len(case.oracle(10000)["counts"]) == cus + 3
    default = check_blocks(case, 10000)
    ops.tune_set("SELECT_BLOCKS_WG_PER_CU", 1)  # one workgroup per CU: at least three of them take a second block
    try:
        one = check_blocks(case, 10000)
    finally:
        ops.tune_reset()
    for a, b in zip(default[0] + default[1], one[0] + one[1]):
        assert np.array_equal(a.buf.cpu().numpy(), b.buf.cpu().numpy())
    assert list(default[2]) == list(one[2])
