"""GPU: Filter -> Projection over expressions of several 64-bit columns
(fq_filter_project_columns, fq_filter_project_blocks_columns,
fq_predicate_bitmap_columns) against oracle/fq_ref.py, per reference block:
R.Block -> R.filter_block -> Fn.eval, every output compared by bits.

Sizes are the smallest at which the kernels can go wrong: 1, 3, one tile of the
four-column kernels (2048 rows), of the two- and three-column ones (4096) and
of the single-column one (8192) with their neighbours, several tiles with a ragged end (30017), and once 3 * 2^20 + 5
rows (the look-back crosses workgroups; the block kernel draws many blocks).
Every size runs with all columns 16-byte aligned, all offset by one element
and only one offset (no common 16-byte phase: the 8-byte loads)."""
import threading

import numpy as np
import pytest

import fq_ref as R
from fq_amd import abi
from fq_amd._lib import FQError
from fq_amd.expr import STACK, Col, chain, chain_columns, load, pred_tree_columns, predicate, predicate_columns, push

pytestmark = pytest.mark.gpu

U64, I64, F64 = abi.DT_UINT64, abi.DT_INT64, abi.DT_FLOAT64
REF = {U64: "UInt64", I64: "Int64", F64: "Float64"}
DT_OF_REF = {v: k for k, v in REF.items()}
K38 = 3 << 61  # keeps 0.379 of uniformly random u64 rows: no block is empty by accident
BIG = 3 * (1 << 20) + 5
SENTINEL = 0xA5A5A5A5DEADBEEF
DIV_ZERO = "Internal Error: Divide by zero error"
CAST_NULL = "cast produced nulls (nulls are not supported on the device path)"
ops = None


def setup_module():
    global ops
    from fq_amd import ops as _ops
    _ops.require_gpu()
    ops = _ops


LAYOUTS = {"aligned": (0, 0, 0, 0), "all_offset": (1, 1, 1, 1), "one_offset": (0, 1, 0, 0)}
_HOST = {}


def splitmix_host(seed, n):
    if (seed, n) not in _HOST:
        _HOST[(seed, n)] = ops.splitmix_column(seed, 1000, n).to_numpy()
    return _HOST[(seed, n)]


def numpy_dev(arr, dt, off):
    pad = np.zeros(off + len(arr), dtype=arr.dtype)
    pad[off:] = arr
    c = ops.from_numpy(pad, dt)
    assert c.ptr % 16 == 0
    return ops.DeviceColumn(c.buf, len(arr), dt, offset=8 * off)


def as_f64(u):  # [-1000, 1000)
    return (u >> np.uint64(11)).astype(np.float64) * (2000.0 / (1 << 53)) - 1000.0


def fld(n):
    return R.Field(n)


def const(v, t="UInt64"):
    return R.Const(R.Value(t, v))


class Case:
    """one statement: the kernel's column list (names, dtypes, host rows), its fq_pred and fq_exprs, and the same
    filter and expressions as oracle functions"""

    def __init__(self, names, dts, host, pred, values, where, exprs):
        self.names, self.dts, self.host = names, dts, host
        self.pred, self.values, self.where, self.exprs = pred, values, where, exprs
        self.n = len(host[0])
        self._oracle = {}

    def dev(self, layout="aligned"):
        return [numpy_dev(h, dt, off) for h, dt, off in zip(self.host, self.dts, LAYOUTS[layout])]

    def oracle(self, block_rows=0):
        """([uint64 bits of output j's kept rows, one array per reference block], [rows kept per block],
        [output dtypes]); raises R.RefError as the reference would"""
        if block_rows not in self._oracle:
            br = block_rows if block_rows > 0 else max(self.n, 1)
            outs, counts, dts = [[] for _ in self.exprs], [], [None] * len(self.exprs)
            for s in range(0, self.n, br):
                blk = R.Block([(nm, R.Arr(REF[dt], h[s:s + br])) for nm, dt, h in zip(self.names, self.dts, self.host)])
                fb = R.filter_block(self.where, blk) if self.where is not None else blk
                counts.append(fb.num_rows())
                for j, e in enumerate(self.exprs):
                    v = e.eval(fb)
                    assert v.valid is None or np.all(v.valid)
                    dts[j] = DT_OF_REF[v.type]
                    outs[j].append(np.ascontiguousarray(v.values).view(np.uint64))
            self._oracle[block_rows] = (outs, counts, dts)
        return self._oracle[block_rows]


def bits(col):
    return col.to_numpy().view(np.uint64)


def check_contiguous(case, layout="aligned", stream=None, cols=None):
    want, counts, dts = case.oracle(0)
    outs = ops.filter_project_columns(cols or case.dev(layout), case.pred, case.values, stream=stream)
    assert len(outs) == len(want)
    for j, o in enumerate(outs):
        assert o.len == sum(counts), (case.n, layout, j, o.len, sum(counts))
        assert o.dtype == dts[j]
        assert np.array_equal(bits(o), np.concatenate(want[j])), (case.n, layout, j)


def check_blocks(case, block_rows, layout="aligned", out_offset=0):
    want, counts, dts = case.oracle(block_rows if block_rows < case.n else 0)
    outs, cnt, kept = ops.filter_project_blocks_columns(case.dev(layout), block_rows, case.pred, case.values,
                                                        out_offset=out_offset, fill=SENTINEL)
    what = (case.n, block_rows, layout, out_offset)
    assert list(cnt) == counts, what
    assert kept == sum(counts), what
    br = min(block_rows, case.n)
    for j, o in enumerate(outs):
        assert o.dtype == dts[j]
        got = bits(o)
        exp = np.full(case.n, SENTINEL, np.uint64)  # rows of a block past its count are left as they were
        for b, rows in enumerate(want[j]):
            exp[b * br:b * br + len(rows)] = rows
        assert np.array_equal(got, exp), what + (j,)


# ---------------------------------------------------------------------------
# the statements
# ---------------------------------------------------------------------------
def case_q6(n):
    """a * b, a + c WHERE c < k; the kernel's columns are c, a, b (the filter's first)"""
    dts = [U64, U64, U64]
    host = [splitmix_host(s, n) for s in (11, 12, 13)]
    values = [chain_columns(dts, [load(1), ("*", Col(2))])[0], chain_columns(dts, [load(1), ("+", Col(0))])[0]]
    return Case(["c", "a", "b"], dts, host, predicate_columns(dts, [], "<", K38), values,
                R.Compare("<", fld("c"), const(K38)),
                [R.Arith("*", fld("a"), fld("b")), R.Arith("+", fld("a"), fld("c"))])


def case_tree(n):
    """a + b * c, c WHERE a < b or c = 7 (c = 7 on every 5th row)"""
    dts = [U64, U64, U64]
    c = splitmix_host(23, n).copy()
    c[::5] = 7
    host = [splitmix_host(21, n), splitmix_host(22, n), c]
    values = [chain_columns(dts, [push(1), ("*", Col(2)), ("+", STACK, True)])[0], chain_columns(dts, [load(2)])[0]]
    return Case(["a", "b", "c"], dts, host, pred_tree_columns(dts, [([], "<", Col(1)), ([load(2)], "=", 7)], [0, 1, "or"]),
                values, R.Logic("or", R.Compare("<", fld("a"), fld("b")), R.Compare("=", fld("c"), const(7))),
                [R.Arith("+", fld("a"), R.Arith("*", fld("b"), fld("c"))), fld("c")])


def case_mixed(n):
    """a * b (Int64), a + c (Float64), b WHERE (b + 1) >= c over u64 < 2^24, i64, f64"""
    dts = [U64, I64, F64]
    a = splitmix_host(31, n) >> np.uint64(40)
    b = splitmix_host(32, n).view(np.int64) >> np.int64(41)
    c = as_f64(splitmix_host(33, n))
    values = [chain_columns(dts, [("*", Col(1))])[0], chain_columns(dts, [("+", Col(2))])[0],
              chain_columns(dts, [load(1)])[0]]
    return Case(["a", "b", "c"], dts, [a, b, c], predicate_columns(dts, [load(1), ("+", 1)], ">=", Col(2)), values,
                R.Compare(">=", R.Arith("+", fld("b"), const(1)), fld("c")),
                [R.Arith("*", fld("a"), fld("b")), R.Arith("+", fld("a"), fld("c")), fld("b")])


def case_four(n):
    """FQ_MAX_PROJECT outputs over four columns WHERE d < k"""
    dts = [U64] * 4
    names = ["d", "a", "b", "c"]
    host = [splitmix_host(s, n) for s in (41, 42, 43, 44)]
    values, exprs = [], []
    for j in range(abi.MAX_PROJECT):
        p, q = j % 4, (j + 1 + j // 4) % 4
        values.append(chain_columns(dts, [load(p), ("*" if j & 1 else "+", Col(q)), ("+", j)])[0])
        exprs.append(R.Arith("+", R.Arith("*" if j & 1 else "+", fld(names[p]), fld(names[q])), const(j)))
    return Case(names, dts, host, predicate_columns(dts, [], "<", K38), values, R.Compare("<", fld("d"), const(K38)),
                exprs)


CASES = {"q6": case_q6, "tree": case_tree, "mixed": case_mixed, "four": case_four}
SIZES = [1, 3, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 30017]
GEOMETRY = [(1, 8192), (8192, 8192), (8193, 8192), (24576, 8192), (30017, 8192), (30017, 10000)]
_CASES = {}


def get_case(name, n):
    if (name, n) not in _CASES:
        _CASES[(name, n)] = CASES[name](n)
    return _CASES[(name, n)]


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("name", list(CASES))
def test_contiguous_kernel(name, layout):
    for n in SIZES:
        check_contiguous(get_case(name, n), layout)


@pytest.mark.parametrize("name", ["q6", "tree"])
def test_contiguous_kernel_many_tiles(name):
    check_contiguous(get_case(name, BIG))


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("name", list(CASES))
def test_block_stream_kernel(name, layout):
    for n, br in GEOMETRY:
        for out_offset in (0, 1):
            check_blocks(get_case(name, n), br, layout, out_offset)


def test_block_stream_kernel_many_blocks():
    check_blocks(get_case("q6", BIG), 10000)


def test_block_that_keeps_no_row_and_block_that_keeps_every_row():
    n = 30017
    base = case_q6(n)
    c = base.host[0].copy()
    c[0:10000] = 0         # block 0 keeps every row: whole tiles of kept rows
    c[10000:20000] = K38   # block 1 keeps none
    case = Case(base.names, base.dts, [c] + base.host[1:], base.pred, base.values, base.where, base.exprs)
    assert case.oracle(10000)[1][:2] == [10000, 0]
    for layout in LAYOUTS:
        for out_offset in (0, 1):
            check_blocks(case, 10000, layout, out_offset)
        check_contiguous(case, layout)


def test_no_predicate_map_kernel_and_bitmap_predicate():
    n = 30017
    base = case_q6(n)
    nopred = Case(base.names, base.dts, base.host, None, base.values, None, base.exprs)
    for layout in LAYOUTS:
        check_contiguous(nopred, layout)
    check_blocks(nopred, 10000)
    # the same filter as a precomputed Boolean column
    cols = base.dev()
    bm = ops.predicate_bitmap_columns(cols, base.pred)
    bp = abi.fq_pred()
    bp.kind = abi.PRED_BITMAP
    bp.bitmap = bm.ptr
    with_bitmap = Case(base.names, base.dts, base.host, bp, base.values, base.where, base.exprs)
    for layout in LAYOUTS:
        check_contiguous(with_bitmap, layout)
        check_blocks(with_bitmap, 10000, layout)


@pytest.mark.parametrize("name", ["q6", "tree", "a<b"])
def test_predicate_bitmap_columns(name):
    for n in (1, 63, 64, 65, 30017):
        if name == "a<b":
            dts = [U64, U64]
            host = [splitmix_host(51, n), splitmix_host(52, n)]
            case = Case(["a", "b"], dts, host, predicate_columns(dts, [], "<", Col(1)), [], R.Compare("<", fld("a"), fld("b")), [])
        else:
            case = get_case(name, n)
        blk = R.Block([(nm, R.Arr(REF[dt], h)) for nm, dt, h in zip(case.names, case.dts, case.host)])
        want = np.asarray(case.where.eval(blk).values, dtype=bool)
        for layout in LAYOUTS:
            bm = ops.predicate_bitmap_columns(case.dev(layout)[:len(case.dts)], case.pred)
            assert np.array_equal(bm.to_numpy(), want), (name, n, layout)
            words = bm.buf[bm.offset:bm.offset + bm.nbytes()].cpu().numpy().view(np.uint64)
            if n % 64:
                assert int(words[-1]) >> (n % 64) == 0, (name, n, layout)  # bits past n are cleared


# ---------------------------------------------------------------------------
# errors: a predicate error on any row first, then an expression error on a kept row only
# ---------------------------------------------------------------------------
N_ERR = 30017
ROWS_ERR = [5000, N_ERR - 1]  # inside a tile; the last ragged row


def both_kernels(case, layout):
    """the statement through both kernels: [callable]"""
    return [lambda: ops.filter_project_columns(case.dev(layout), case.pred, case.values),
            lambda: ops.filter_project_blocks_columns(case.dev(layout), 10000, case.pred, case.values)]


def expect_error(case, status, text):
    for layout in ("aligned", "one_offset"):
        for run in both_kernels(case, layout):
            with pytest.raises(FQError) as e:
                run()
            assert e.value.status == status and str(e.value) == text, (layout, str(e.value))


def expect_answer(case):
    for layout in ("aligned", "one_offset"):
        check_contiguous(case, layout)
        check_blocks(case, 10000, layout)


def divide_case(row, kept):
    """a / b, a WHERE c < k with b = 0 at `row`"""
    dts = [U64, U64, U64]
    c = splitmix_host(61, N_ERR).copy()
    b = splitmix_host(63, N_ERR) | np.uint64(1)
    b[row] = 0
    c[row] = 0 if kept else K38
    values = [chain_columns(dts, [load(1), ("/", Col(2))])[0], chain_columns(dts, [load(1)])[0]]
    return Case(["c", "a", "b"], dts, [c, splitmix_host(62, N_ERR), b], predicate_columns(dts, [], "<", K38), values,
                R.Compare("<", fld("c"), const(K38)), [R.Arith("/", fld("a"), fld("b")), fld("a")])


@pytest.mark.parametrize("row", ROWS_ERR)
def test_zero_divisor_raises_at_a_kept_row_only(row):
    expect_error(divide_case(row, True), abi.FQ_E_DIVIDE_BY_ZERO, DIV_ZERO)
    with pytest.raises(R.RefError):
        divide_case(row, True).oracle(0)
    expect_answer(divide_case(row, False))


def pred_divide_case(row, cast_row=None):
    """a + d WHERE a / b < k with b = 0 at `row` (d Int64: a >= 2^63 at cast_row is a cast null in the value)"""
    dts = [U64, U64, I64]
    a = splitmix_host(71, N_ERR) >> np.uint64(1)
    b = (splitmix_host(72, N_ERR) >> np.uint64(60)) + np.uint64(1)
    d = splitmix_host(73, N_ERR).view(np.int64) >> np.int64(2)
    if row is not None:
        b[row] = 0
    if cast_row is not None:
        a[cast_row] = (1 << 63) + 5
        b[cast_row] = 1 << 63  # a / b = 1: kept
    k = 1 << 61
    return Case(["a", "b", "d"], dts, [a, b, d], predicate_columns(dts, [("/", Col(1))], "<", k),
                [chain_columns(dts, [("+", Col(2))])[0]],
                R.Compare("<", R.Arith("/", fld("a"), fld("b")), const(k)), [R.Arith("+", fld("a"), fld("d"))])


@pytest.mark.parametrize("row", ROWS_ERR)
def test_zero_divisor_under_the_predicate_raises_on_any_row(row):
    expect_error(pred_divide_case(row), abi.FQ_E_DIVIDE_BY_ZERO, DIV_ZERO)
    expect_answer(pred_divide_case(None))


@pytest.mark.parametrize("row", ROWS_ERR)
def test_predicate_error_wins_over_an_expression_error(row):
    other = ROWS_ERR[0] + 7 if row == ROWS_ERR[1] else ROWS_ERR[1]
    expect_error(pred_divide_case(None, cast_row=other), abi.FQ_E_UNSUPPORTED, CAST_NULL)  # the value's own error
    expect_error(pred_divide_case(row, cast_row=other), abi.FQ_E_DIVIDE_BY_ZERO, DIV_ZERO)


def cast_case(row, kept):
    """a + b WHERE c < k over u64, i64: a >= 2^63 at `row` does not fit the coerced Int64"""
    dts = [U64, U64, I64]
    c = splitmix_host(81, N_ERR).copy()
    a = splitmix_host(82, N_ERR) >> np.uint64(1)  # below 2^63 everywhere else
    a[row] = (1 << 63) + 11
    c[row] = 0 if kept else K38
    b = splitmix_host(83, N_ERR).view(np.int64) >> np.int64(2)
    return Case(["c", "a", "b"], dts, [c, a, b], predicate_columns(dts, [], "<", K38),
                [chain_columns(dts, [load(1), ("+", Col(2))])[0]], R.Compare("<", fld("c"), const(K38)),
                [R.Arith("+", fld("a"), fld("b"))])


@pytest.mark.parametrize("row", ROWS_ERR)
def test_u64_above_i64_meeting_an_int64_column(row):
    expect_error(cast_case(row, True), abi.FQ_E_UNSUPPORTED, CAST_NULL)
    expect_answer(cast_case(row, False))
    # under the predicate (a < b coerces to Int64): any row
    dts = [U64, I64]
    a = splitmix_host(84, N_ERR) >> np.uint64(1)
    a[row] = (1 << 63) + 11
    b = splitmix_host(85, N_ERR).view(np.int64) >> np.int64(1)
    case = Case(["a", "b"], dts, [a, b], predicate_columns(dts, [], "<", Col(1)), [chain_columns(dts, [load(1)])[0]],
                R.Compare("<", fld("a"), fld("b")), [fld("b")])
    expect_error(case, abi.FQ_E_UNSUPPORTED, CAST_NULL)


# ---------------------------------------------------------------------------
# Float64
# ---------------------------------------------------------------------------
def test_f64_chain_rounds_twice_like_fq_arith():
    n = 30017
    dts = [F64, F64, F64]
    host = [as_f64(splitmix_host(s, n)) for s in (91, 92, 93)]
    case = Case(["a", "b", "c"], dts, host, predicate_columns(dts, [], "<", Col(1)),
                [chain_columns(dts, [("*", Col(1)), ("-", Col(2))])[0]], R.Compare("<", fld("a"), fld("b")),
                [R.Arith("-", R.Arith("*", fld("a"), fld("b")), fld("c"))])
    expect_answer(case)
    a, b, c = case.dev()
    twice = ops.arith("-", ops.arith("*", a, b), c).to_numpy()
    fused = ops.filter_project_columns([a, b, c], case.pred, case.values)[0]
    assert np.array_equal(bits(fused), twice[host[0] < host[1]].view(np.uint64))
    nopred = Case(case.names, dts, host, None, case.values, None, case.exprs)
    check_contiguous(nopred)
    assert np.array_equal(bits(ops.filter_project_columns([a, b, c], None, case.values)[0]), twice.view(np.uint64))


def test_f64_special_values_pass_through_unchanged():
    n = 8193
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 5e-324, -1.5], np.float64)
    a = np.resize(special, n)
    b = np.resize(special[::-1], n)
    a.view(np.uint64)[7::97] = 0x7FF8DEADBEEF0001  # a NaN payload
    c = splitmix_host(95, n)
    dts = [F64, F64, U64]
    case = Case(["a", "b", "c"], dts, [a, b, c], predicate_columns(dts, [load(2)], "<", K38),
                [None, chain_columns(dts, [load(1)])[0]], R.Compare("<", fld("c"), const(K38)), [fld("a"), fld("b")])
    expect_answer(case)


# ---------------------------------------------------------------------------
# one column: the call IS the single-column entry point
# ---------------------------------------------------------------------------
ONE = [
    ("p1", U64, ([("%", 8)], "<", 3), [[("+", 1)], None]),
    ("i64", I64, ([], "<", 0), [[("/", (-3, "Int64"))]]),
    ("f64", F64, ([("*", 2.0)], ">=", 1.5), [[("+", 0.5)], None]),
]


@pytest.mark.parametrize("name,dt,pr,steps", ONE, ids=[o[0] for o in ONE])
def test_one_column_is_the_single_column_entry_point(name, dt, pr, steps):
    n = 30017
    u = splitmix_host(97, n)
    host = u if dt == U64 else (u.view(np.int64) if dt == I64 else as_f64(u))
    col = numpy_dev(np.ascontiguousarray(host), dt, 0)
    pred = predicate(dt, *pr)
    values = [chain(dt, s)[0] if s is not None else None for s in steps]
    want = ops.filter_project(col, pred, values)
    got = ops.filter_project_columns([col], pred, values)
    assert [o.len for o in got] == [o.len for o in want]
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(bits(g), bits(w))
    wouts, wcnt = ops.filter_project_blocks(col, 10000, pred, values)
    gouts, gcnt, kept = ops.filter_project_blocks_columns([col], 10000, pred, values)
    assert list(gcnt) == list(wcnt) and kept == int(wcnt.sum()) == want[0].len
    for g, w in zip(gouts, wouts):
        for b, k in enumerate(wcnt):
            assert np.array_equal(bits(g)[b * 10000:b * 10000 + k], bits(w)[b * 10000:b * 10000 + k])
    assert np.array_equal(ops.predicate_bitmap_columns([col], pred).to_numpy(), ops.predicate_bitmap(col, pred).to_numpy())


def test_two_contiguous_launches_side_by_side():
    """The multi-column twin of test_project_gpu.test_two_lookback_launches_side_by_side: two host threads, each
    on its own stream, run the look-back kernel over three columns (1,537 tiles each) at the same time; both
    finish and agree with the oracle."""
    import torch
    cases = [get_case("q6", BIG), get_case("tree", BIG)]
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

