"""GPU: Filter -> Projection over columns, steps, comparisons and outputs of any
numeric type (fq_filter_project_typed, fq_filter_project_blocks_typed,
fq_predicate_bitmap_typed) against oracle/fq_ref.py, per reference block:
R.Block -> R.filter_block -> Fn.eval.  Integer outputs are compared bit for
bit, float outputs bit for bit with NaN equal to NaN; inputs hold no NaN except
in the dedicated case.

Sizes are the smallest at which the kernels can go wrong: 1, 3, one tile of
256 * R rows of each shape (fq_scan.h typed_project_geometry) with its
neighbours, 3 * 2^20 + 5 rows (the look-back crosses workgroups, the block
kernel draws many blocks), and the block stream at 30017 rows in blocks on the
row group's grid (10000) and at the smallest block (8192).  Every size runs
with all columns aligned, all offset by one element (every group off the grid:
the element loads) and one column offset (no shared phase), with the outputs
aligned and offset by one element (a ragged head before the first 16-byte
store), and with every row kept, no row kept and about 3/8 kept."""
import threading

import numpy as np
import pytest

import fq_ref as R
from fq_amd import abi
from fq_amd._lib import FQError
from fq_amd.expr import Col, chain_columns, load, pred_tree_columns, predicate_columns

pytestmark = pytest.mark.gpu

I8, I16, I32, I64 = abi.DT_INT8, abi.DT_INT16, abi.DT_INT32, abi.DT_INT64
U8, U16, U32, U64 = abi.DT_UINT8, abi.DT_UINT16, abi.DT_UINT32, abi.DT_UINT64
F32, F64 = abi.DT_FLOAT32, abi.DT_FLOAT64
REF = {I8: "Int8", I16: "Int16", I32: "Int32", I64: "Int64", U8: "UInt8", U16: "UInt16", U32: "UInt32",
       U64: "UInt64", F32: "Float32", F64: "Float64"}
DT_OF_REF = {v: k for k, v in REF.items()}
NP = {I8: np.int8, I16: np.int16, I32: np.int32, I64: np.int64, U8: np.uint8, U16: np.uint16, U32: np.uint32,
      U64: np.uint64, F32: np.float32, F64: np.float64}
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
BIG = 3 * (1 << 20) + 5
FILL = 0xA5
DIV_ZERO = "Internal Error: Divide by zero error"
CAST_NULL = "cast produced nulls (nulls are not supported on the device path)"
LAYOUTS = {"aligned": (0, 0, 0, 0), "all_offset": (1, 1, 1, 1), "one_offset": (0, 1, 0, 0)}
ops = None


def setup_module():
    global ops
    from fq_amd import ops as _ops
    _ops.require_gpu()
    ops = _ops


def numpy_dev(arr, dt, off):
    """the rows of arr starting `off` elements into a 256-byte aligned buffer"""
    pad = np.zeros(off + len(arr), dtype=arr.dtype)
    pad[off:] = arr
    c = ops.from_numpy(pad, dt)
    assert c.ptr % 256 == 0
    return ops.DeviceColumn(c.buf, len(arr), dt, offset=arr.dtype.itemsize * off)


def fld(n):
    return R.Field(n)


def const(v, t):
    return R.Const(R.Value(t, v))


def tile_rows(dts, out_dts):
    """256 * R of fq_scan.h typed_project_geometry"""
    width = sum(np.dtype(NP[d]).itemsize for d in dts)
    wout = max(np.dtype(NP[d]).itemsize for d in out_dts)
    r = 32
    while r > 1 and (r * width > 384 or r * wout > 128):
        r //= 2
    return 256 * r


class Case:
    """one statement: the kernel's column list (names, dtypes, host rows), its fq_pred and fq_exprs, and the same
    filter and expressions as oracle functions"""

    def __init__(self, names, dts, host, pred, values, where, exprs):
        self.names, self.dts, self.host = names, dts, [np.ascontiguousarray(h) for h in host]
        self.pred, self.values, self.where, self.exprs = pred, values, where, exprs
        self.n = len(host[0])
        self._oracle = {}

    def dev(self, layout="aligned"):
        offs = LAYOUTS[layout]
        if len(self.dts) == 1 and layout == "one_offset":
            offs = (1,)
        return [numpy_dev(h, dt, off) for h, dt, off in zip(self.host, self.dts, offs)]

    def with_pred(self, pred, where):
        return Case(self.names, self.dts, self.host, pred, self.values, where, self.exprs)

    def oracle(self, block_rows=0):
        """([output j's kept rows, one array per reference block], [rows kept per block], [output dtypes]); raises
        R.RefError for a zero divisor and CastNull for a cast that arrow turns into null, as the device path does"""
        if block_rows not in self._oracle:
            br = block_rows if block_rows > 0 else max(self.n, 1)
            outs, counts, dts = [[] for _ in self.exprs], [], [None] * len(self.exprs)
            for s in range(0, self.n, br):
                blk = R.Block([(nm, R.Arr(REF[dt], h[s:s + br])) for nm, dt, h in zip(self.names, self.dts, self.host)])
                fb = blk
                if self.where is not None:
                    res = self.where.eval(blk)
                    if res.valid is not None and not np.all(res.valid):
                        raise CastNull("predicate")
                    fb = R.filter_block(self.where, blk)
                counts.append(fb.num_rows())
                for j, e in enumerate(self.exprs):
                    v = e.eval(fb)
                    if v.valid is not None and not np.all(v.valid):
                        raise CastNull("value")
                    dts[j] = DT_OF_REF[v.type]
                    outs[j].append(np.ascontiguousarray(v.values, dtype=NP[dts[j]]))
            self._oracle[block_rows] = (outs, counts, dts)
        return self._oracle[block_rows]


class CastNull(Exception):
    pass


def same(got, want, dt):
    """bit for bit; float NaNs equal each other"""
    w = np.dtype(NP[dt]).itemsize
    g, x = np.ascontiguousarray(got).view(UINT[w]), np.ascontiguousarray(want).view(UINT[w])
    if g.shape != x.shape:
        return False
    if dt in (F32, F64):
        gn, xn = np.isnan(np.asarray(got)), np.isnan(np.asarray(want))
        return bool(np.array_equal(gn, xn) and np.array_equal(g[~gn], x[~xn]))
    return bool(np.array_equal(g, x))


def check_contiguous(case, layout="aligned", out_offset=0, stream=None, cols=None):
    want, counts, dts = case.oracle(0)
    outs = ops.filter_project_typed(cols or case.dev(layout), case.pred, case.values, stream=stream, out_offset=out_offset)
    assert len(outs) == len(want)
    for j, o in enumerate(outs):
        what = (case.n, layout, out_offset, j)
        assert o.len == sum(counts), what + (o.len, sum(counts))
        assert o.dtype == dts[j], what
        assert same(o.to_numpy(), np.concatenate(want[j]), dts[j]), what


def check_blocks(case, block_rows, layout="aligned", out_offset=0):
    want, counts, dts = case.oracle(block_rows if block_rows < case.n else 0)
    outs, cnt, kept = ops.filter_project_blocks_typed(case.dev(layout), block_rows, case.pred, case.values,
                                                      out_offset=out_offset, fill=FILL)
    what = (case.n, block_rows, layout, out_offset)
    assert list(cnt) == counts, what  # d_counts = the oracle's per-block counts
    assert kept == sum(counts), what
    br = min(block_rows, case.n)
    for j, o in enumerate(outs):
        assert o.dtype == dts[j], what
        exp = np.full(case.n * np.dtype(NP[dts[j]]).itemsize, FILL, np.uint8).view(NP[dts[j]])  # rows past a count stay
        for b, rows in enumerate(want[j]):
            exp[b * br:b * br + len(rows)] = rows
        assert same(o.to_numpy(), exp, dts[j]), what + (j,)


def check_bitmap(case, layout="aligned"):
    blk = R.Block([(nm, R.Arr(REF[dt], h)) for nm, dt, h in zip(case.names, case.dts, case.host)])
    want = np.asarray(case.where.eval(blk).values, dtype=bool)
    bm = ops.predicate_bitmap_typed(case.dev(layout), case.pred)
    assert np.array_equal(bm.to_numpy(), want), (case.n, layout)
    words = bm.buf[bm.offset:bm.offset + bm.nbytes()].cpu().numpy().view(np.uint64)
    if case.n % 64:
        assert int(words[-1]) >> (case.n % 64) == 0, (case.n, layout)  # bits past n are cleared


# ---------------------------------------------------------------------------
# the three shapes; keep: "some" (about 3/8 of the rows), "all", "none"
# ---------------------------------------------------------------------------
def case_q6(n, keep="some"):
    """price * discount (Float64), quantity (UInt8), discount * discount (Float32) WHERE shipdate < k and quantity < q"""
    rng = np.random.default_rng(1000003 + n)
    dts = [F64, F32, I32, U8]
    ship = rng.integers(8000, 10600, n).astype(np.int32)
    qty = rng.integers(1, 51, n).astype(np.uint8)
    if keep == "all":
        ship[:], qty[:] = 8000, 1 + qty % 25
    elif keep == "none":
        ship[:] = 10000
    host = [rng.uniform(1.0, 1000.0, n), (rng.integers(0, 11, n) / 100.0).astype(np.float32), ship, qty]
    pred = pred_tree_columns(dts, [([load(2)], "<", (9950, "Int32")), ([load(3)], "<", (26, "UInt8"))], [0, 1, "and"])
    values = [chain_columns(dts, [("*", Col(1))])[0], chain_columns(dts, [load(3)])[0],
              chain_columns(dts, [load(1), ("*", Col(1))])[0]]
    assert [v.out_dtype for v in values] == [F64, U8, F32]
    where = R.Logic("and", R.Compare("<", fld("shipdate"), const(9950, "Int32")),
                    R.Compare("<", fld("quantity"), const(26, "UInt8")))
    exprs = [R.Arith("*", fld("price"), fld("discount")), fld("quantity"), R.Arith("*", fld("discount"), fld("discount"))]
    return Case(["price", "discount", "shipdate", "quantity"], dts, host, pred, values, where, exprs)


def case_u8u16(n, keep="some"):
    """a + b (UInt16: wraps at 16 bits), a (UInt8) WHERE a < 100"""
    rng = np.random.default_rng(2000003 + n)
    dts = [U8, U16]
    a = rng.integers(0, 256, n).astype(np.uint8)
    if keep == "all":
        a %= 100
    elif keep == "none":
        a = (100 + a % 156).astype(np.uint8)
    host = [a, rng.integers(0, 65536, n).astype(np.uint16)]
    values = [chain_columns(dts, [("+", Col(1))])[0], None]
    assert values[0].out_dtype == U16
    return Case(["a", "b"], dts, host, predicate_columns(dts, [], "<", (100, "UInt8")), values,
                R.Compare("<", fld("a"), const(100, "UInt8")), [R.Arith("+", fld("a"), fld("b")), fld("a")])


def case_i32(n, keep="some"):
    """x + x (Int32, wrapping) WHERE x % 8 < 3; every 16th row negative (a truncated remainder <= 0 is kept)"""
    rng = np.random.default_rng(3000003 + n)
    dts = [I32]
    x = rng.integers(0, 1 << 31, n).astype(np.int32)
    x[::16] = -x[::16]
    if keep == "all":
        x &= ~np.int32(7)
    elif keep == "none":
        x = ((x & np.int32(0x7FFFFFF8)) | np.int32(5)).astype(np.int32)
    pred = predicate_columns(dts, [("%", 8)], "<", 3)
    assert pred.cmp_dtype == I32
    values = [chain_columns(dts, [("+", Col(0))])[0]]
    assert values[0].out_dtype == I32
    where = R.Compare("<", R.Arith("%", fld("x"), const(8, "UInt64")), const(3, "UInt64"))
    return Case(["x"], dts, [x], pred, values, where, [R.Arith("+", fld("x"), fld("x"))])


CASES = {"q6": case_q6, "u8u16": case_u8u16, "i32": case_i32}
TILE = {"q6": tile_rows([F64, F32, I32, U8], [F64, U8, F32]), "u8u16": tile_rows([U8, U16], [U16, U8]),
        "i32": tile_rows([I32], [I32])}
_CASES = {}


def get_case(name, n, keep="some"):
    if (name, n, keep) not in _CASES:
        _CASES[(name, n, keep)] = CASES[name](n, keep)
    return _CASES[(name, n, keep)]


def test_tiles_of_the_three_shapes():
    assert TILE == {"q6": 4096, "u8u16": 8192, "i32": 8192}


def every_entry_point(case, layout, block_rows=10000):
    for out_offset in (0, 1):
        check_contiguous(case, layout, out_offset)
        check_blocks(case, block_rows, layout, out_offset)
    check_bitmap(case, layout)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("name", list(CASES))
def test_flat_sizes(name, layout):
    t = TILE[name]
    for n in (1, 3, t - 1, t, t + 1):
        for keep in ("some", "all", "none"):
            every_entry_point(get_case(name, n, keep), layout)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("name", list(CASES))
def test_many_tiles_and_blocks(name, layout):
    every_entry_point(get_case(name, BIG), layout)


@pytest.mark.parametrize("keep", ["all", "none"])
@pytest.mark.parametrize("name", list(CASES))
def test_many_tiles_every_row_and_no_row_kept(name, keep):
    every_entry_point(get_case(name, BIG, keep), "aligned")


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("name", list(CASES))
def test_block_stream_geometry(name, layout):
    for br in (10000, 8192):
        for keep in ("some", "all", "none"):
            every_entry_point(get_case(name, 30017, keep), layout, br)


def test_block_that_keeps_no_row_beside_one_that_keeps_every_row():
    base = get_case("u8u16", 30017)
    a = base.host[0].copy()
    a[0:10000] = 7       # block 0 keeps every row: whole tiles of kept rows
    a[10000:20000] = 200  # block 1 keeps none
    case = Case(base.names, base.dts, [a, base.host[1]], base.pred, base.values, base.where, base.exprs)
    assert case.oracle(10000)[1][:2] == [10000, 0]
    for layout in LAYOUTS:
        every_entry_point(case, layout)


def test_bitmap_predicate_and_no_predicate():
    """the map kernel (with a narrow pass-through column) and a precomputed Boolean column as the filter"""
    for name in CASES:
        for n in (TILE[name] + 1, 30017):
            base = get_case(name, n)
            nopred = base.with_pred(None, None)
            for layout in LAYOUTS:
                for out_offset in (0, 1):
                    check_contiguous(nopred, layout, out_offset)
                check_blocks(nopred, 10000, layout)
            bm = ops.predicate_bitmap_typed(base.dev(), base.pred)
            bp = abi.fq_pred()
            bp.kind = abi.PRED_BITMAP
            bp.bitmap = bm.ptr
            with_bitmap = base.with_pred(bp, base.where)
            for layout in LAYOUTS:
                for out_offset in (0, 1):
                    check_contiguous(with_bitmap, layout, out_offset)
                    check_blocks(with_bitmap, 10000, layout, out_offset)


# ---------------------------------------------------------------------------
# errors: a predicate error on any row first, then a value error on a kept row only
# ---------------------------------------------------------------------------
N_ERR = 30017
ROWS_ERR = [0, 5000, 30010, N_ERR - 1]  # the first row, inside a tile, in the ragged tail, the last row


def expect_error(case, status, text):
    for layout in ("aligned", "one_offset"):
        for run in (lambda: ops.filter_project_typed(case.dev(layout), case.pred, case.values),
                    lambda: ops.filter_project_blocks_typed(case.dev(layout), 10000, case.pred, case.values)):
            with pytest.raises(FQError) as e:
                run()
            assert e.value.status == status and str(e.value) == text, (layout, str(e.value))


def expect_answer(case):
    for layout in ("aligned", "one_offset"):
        check_contiguous(case, layout)
        check_blocks(case, 10000, layout)


def keep_column(rng, row, kept):
    """c UInt8, WHERE c < 100; row `row` kept or dropped"""
    c = rng.integers(0, 256, N_ERR).astype(np.uint8)
    if row is not None:
        c[row] = 5 if kept else 200
    return c


def cast_case(row, kept):
    """a + b (UInt32 + Int32 coerces to Int32) WHERE c < 100: a >= 2^31 at `row` does not fit"""
    rng = np.random.default_rng(41)
    dts = [U8, U32, I32]
    a = rng.integers(0, 1 << 31, N_ERR).astype(np.uint32)
    a[row] = (1 << 31) + 11
    b = rng.integers(-(1 << 20), 1 << 20, N_ERR).astype(np.int32)
    values = [chain_columns(dts, [load(1), ("+", Col(2))])[0]]
    assert values[0].out_dtype == I32
    return Case(["c", "a", "b"], dts, [keep_column(rng, row, kept), a, b], predicate_columns(dts, [], "<", (100, "UInt8")),
                values, R.Compare("<", fld("c"), const(100, "UInt8")), [R.Arith("+", fld("a"), fld("b"))])


@pytest.mark.parametrize("row", ROWS_ERR)
def test_narrowing_cast_out_of_range(row):
    expect_error(cast_case(row, True), abi.FQ_E_UNSUPPORTED, CAST_NULL)
    with pytest.raises(CastNull):
        cast_case(row, True).oracle(0)
    expect_answer(cast_case(row, False))  # a dropped row does not reach the value's cast
    # under the predicate (a < b compares as Int32): any row
    rng = np.random.default_rng(42)
    dts = [U32, I32]
    a = rng.integers(0, 1 << 31, N_ERR).astype(np.uint32)
    a[row] = (1 << 31) + 11
    b = rng.integers(0, 1 << 31, N_ERR).astype(np.int32)
    case = Case(["a", "b"], dts, [a, b], predicate_columns(dts, [], "<", Col(1)), [chain_columns(dts, [load(1)])[0]],
                R.Compare("<", fld("a"), fld("b")), [fld("b")])
    with pytest.raises(CastNull):
        case.oracle(0)
    expect_error(case, abi.FQ_E_UNSUPPORTED, CAST_NULL)


def divide_case(dt, row, kept):
    """a / b in Int32 or Float32 WHERE c < 100 with b = 0 at `row` (None: nowhere)"""
    rng = np.random.default_rng(43)
    dts = [U8, dt, dt]
    if dt == I32:
        a = rng.integers(-(1 << 31), 1 << 31, N_ERR).astype(np.int32)
        b = (rng.integers(1, 1 << 20, N_ERR) * rng.choice([-1, 1], N_ERR)).astype(np.int32)
    else:
        a = rng.uniform(-1000.0, 1000.0, N_ERR).astype(np.float32)
        b = rng.uniform(1.0, 9.0, N_ERR).astype(np.float32)
    if row is not None:
        b[row] = 0
    values = [chain_columns(dts, [load(1), ("/", Col(2))])[0], chain_columns(dts, [load(1)])[0]]
    assert values[0].out_dtype == dt
    return Case(["c", "a", "b"], dts, [keep_column(rng, row, kept), a, b], predicate_columns(dts, [], "<", (100, "UInt8")),
                values, R.Compare("<", fld("c"), const(100, "UInt8")), [R.Arith("/", fld("a"), fld("b")), fld("a")])


@pytest.mark.parametrize("row", ROWS_ERR)
@pytest.mark.parametrize("dt", [I32, F32], ids=["Int32", "Float32"])
def test_zero_divisor_at_a_kept_row_a_dropped_row_and_no_row(dt, row):
    expect_error(divide_case(dt, row, True), abi.FQ_E_DIVIDE_BY_ZERO, DIV_ZERO)
    with pytest.raises(R.RefError):
        divide_case(dt, row, True).oracle(0)
    expect_answer(divide_case(dt, row, False))
    if row == ROWS_ERR[0]:
        expect_answer(divide_case(dt, None, False))


def pred_divide_case(row, cast_row):
    """a + d (UInt32 + Int32) WHERE a / b < k in UInt32, b = 0 at `row`; a >= 2^31 at cast_row, a kept row"""
    rng = np.random.default_rng(44)
    dts = [U32, U32, I32]
    a = rng.integers(0, 1 << 31, N_ERR).astype(np.uint32)
    b = rng.integers(1, 16, N_ERR).astype(np.uint32)
    d = rng.integers(-(1 << 20), 1 << 20, N_ERR).astype(np.int32)
    if row is not None:
        b[row] = 0
    if cast_row is not None:
        a[cast_row] = (1 << 31) + 5
        b[cast_row] = 1 << 31  # a / b = 1: kept
    k = 1 << 27
    pred = predicate_columns(dts, [("/", Col(1))], "<", (k, "UInt32"))
    assert pred.cmp_dtype == U32
    return Case(["a", "b", "d"], dts, [a, b, d], pred, [chain_columns(dts, [("+", Col(2))])[0]],
                R.Compare("<", R.Arith("/", fld("a"), fld("b")), const(k, "UInt32")), [R.Arith("+", fld("a"), fld("d"))])


@pytest.mark.parametrize("row", ROWS_ERR)
def test_predicate_error_on_any_row_wins_over_a_value_error(row):
    other = 5007 if row != 5000 else N_ERR - 2
    expect_answer(pred_divide_case(None, None))
    expect_error(pred_divide_case(None, other), abi.FQ_E_UNSUPPORTED, CAST_NULL)  # the value's own error
    expect_error(pred_divide_case(row, None), abi.FQ_E_DIVIDE_BY_ZERO, DIV_ZERO)
    expect_error(pred_divide_case(row, other), abi.FQ_E_DIVIDE_BY_ZERO, DIV_ZERO)


# ---------------------------------------------------------------------------
# Float32
# ---------------------------------------------------------------------------
def test_f32_special_values():
    """max-magnitude, +-0.0, +-inf and NaN through discount * discount and through a pass-through column"""
    n = 8193
    fmax = np.finfo(np.float32).max
    special = np.array([fmax, -fmax, 0.0, -0.0, np.inf, -np.inf, np.nan, 1.5, -2.25], np.float32)
    d = np.resize(special, n)
    d.view(np.uint32)[6::90] = 0x7FC0BEEF  # a NaN payload
    rng = np.random.default_rng(45)
    dts = [F32, U8]
    case = Case(["discount", "c"], dts, [d, rng.integers(0, 256, n).astype(np.uint8)],
                predicate_columns(dts, [load(1)], "<", (100, "UInt8")), [chain_columns(dts, [("*", Col(0))])[0], None],
                R.Compare("<", fld("c"), const(100, "UInt8")), [R.Arith("*", fld("discount"), fld("discount")), fld("discount")])
    with np.errstate(all="ignore"):
        expect_answer(case)
        expect_answer(case.with_pred(None, None))
    # the pass-through column bit for bit, NaN payloads included
    keep = case.host[1] < 100
    got = ops.filter_project_typed(case.dev(), case.pred, case.values)[1].to_numpy()
    assert np.array_equal(got.view(np.uint32), d[keep].view(np.uint32))
    outs, cnt, kept = ops.filter_project_blocks_typed(case.dev(), 8192, case.pred, case.values)
    assert kept == int(keep.sum())
    assert np.array_equal(outs[1].to_numpy().view(np.uint32)[:cnt[0]], d[:8192][keep[:8192]].view(np.uint32))


# ---------------------------------------------------------------------------
# the look-back kernel beside itself; the 64-bit twin
# ---------------------------------------------------------------------------
def test_two_lookback_launches_side_by_side():
    """tests/test_project_gpu.py::test_two_lookback_launches_side_by_side at typed tiles: two host threads, each on
    its own stream, run the look-back kernel of the q6 shape over 1,281 tiles of 4,096 rows each -- more than stay
    resident (at most 4 workgroups of its 104 VGPRs per CU) -- at the same time; both finish and agree with the
    oracle."""
    import torch
    n = 5 * (1 << 20) + 5
    cases = [case_q6(n), case_q6(n + 64)]
    for c in cases:
        c.oracle(0)
    torch.cuda.synchronize()
    start = threading.Barrier(2)
    errors = []

    def run(case):
        try:
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                cols = case.dev()
                stream.synchronize()
                start.wait()
                check_contiguous(case, stream=stream, cols=cols)
        except Exception as e:  # the poll bound reports "did not complete"
            errors.append(repr(e))

    threads = [threading.Thread(target=run, args=(c,)) for c in cases]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=100)
    assert not any(t.is_alive() for t in threads)
    assert not errors, errors


def test_all_64_bit_call_is_the_columns_call():
    n = 30017
    rng = np.random.default_rng(46)
    dts = [U64, U64, I64]
    host = [rng.integers(0, 1 << 62, n).astype(np.uint64), rng.integers(0, 1 << 62, n).astype(np.uint64),
            rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64)]
    cols = [numpy_dev(h, dt, 0) for h, dt in zip(host, dts)]
    pred = predicate_columns(dts, [], "<", Col(1))
    values = [chain_columns(dts, [("*", Col(1))])[0], chain_columns(dts, [load(2), ("+", 7)])[0], None]
    want = ops.filter_project_columns(cols, pred, values)
    got = ops.filter_project_typed(cols, pred, values)
    assert [o.len for o in got] == [o.len for o in want]
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g.to_numpy(), w.to_numpy())
    wouts, wcnt, wkept = ops.filter_project_blocks_columns(cols, 10000, pred, values, fill=0xA5A5A5A5A5A5A5A5)
    gouts, gcnt, gkept = ops.filter_project_blocks_typed(cols, 10000, pred, values, fill=FILL)
    assert list(gcnt) == list(wcnt) and gkept == wkept
    for g, w in zip(gouts, wouts):
        assert np.array_equal(g.to_numpy(), w.to_numpy())
    assert np.array_equal(ops.predicate_bitmap_typed(cols, pred).to_numpy(),
                          ops.predicate_bitmap_columns(cols, pred).to_numpy())


def test_one_64_bit_column_with_a_load_of_its_one_column():
    # load(0) over one 64-bit column (the single-column module): the outputs of the program without it
    n = 30017
    x = np.random.default_rng(47).integers(-(1 << 40), 1 << 40, n).astype(np.int64)
    dts = [I64]
    case = Case(["x"], dts, [x], predicate_columns(dts, [load(0), ("%", (8, "Int64"))], "<", (3, "Int64")),
                [chain_columns(dts, [load(0), ("+", Col(0))])[0], chain_columns(dts, [load(0)])[0], None],
                R.Compare("<", R.Arith("%", fld("x"), const(8, "Int64")), const(3, "Int64")),
                [R.Arith("+", fld("x"), fld("x")), fld("x"), fld("x")])
    for layout in ("aligned", "all_offset"):
        every_entry_point(case, layout)
