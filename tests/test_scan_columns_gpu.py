"""GPU: fq_aggregate_columns (fused aggregate scans whose predicate and
argument read several 64-bit columns of one block) against oracle/fq_ref.py:
a Block of the same columns, FilterTransform (filter_block) and the Agg
argument evaluated per reference block, data_array_aggregate_op per block,
the per-block results merged the way fq_agg_state states them.

Sizes are the smallest at which the kernel can go wrong: 1, 3, one flat
single-column tile of 2048 rows and its neighbours, more than one grid sweep
(3 * 2^20 + 5 rows: the prefetch loop iterates), block mode with an even
(10000: 16-byte loads) and an odd (8191: 8-byte loads) block size.  Every size
runs with all columns 16-byte aligned, all offset by one element (one shared
head row) and only one offset (no shared 16-byte phase: the 8-byte path).
Integer results are bit-exact; f64 sums within 1e-12 * sum(|x|)
(tests/test_kernels_gpu.py test_f64_sum_tolerance_minmax_exact)."""
import numpy as np
import pytest

import fq_ref as R
from fq_amd import abi
from fq_amd.expr import STACK, Col, chain, chain_columns, load, pred_tree_columns, predicate, predicate_columns, push, to_bits

pytestmark = pytest.mark.gpu

ALL = abi.AGG_SUM | abi.AGG_MAX | abi.AGG_MIN | abi.AGG_COUNT
U64, I64, F64 = abi.DT_UINT64, abi.DT_INT64, abi.DT_FLOAT64
REF = {U64: "UInt64", I64: "Int64", F64: "Float64"}
DT_OF_REF = {v: k for k, v in REF.items()}
ERR = abi.STATE_DIV_ZERO | abi.STATE_CAST_NULL
M64 = (1 << 64) - 1
ops = None


def setup_module():
    global ops
    from fq_amd import ops as _ops
    _ops.require_gpu()
    ops = _ops


# ---------------------------------------------------------------------------
# columns: the same rows in every layout
# ---------------------------------------------------------------------------
LAYOUTS = {"aligned": (0, 0, 0, 0), "all_offset": (1, 1, 1, 1), "one_offset": (0, 1, 0, 0)}
_HOST = {}


def splitmix_host(seed, n):
    key = (seed, n)
    if key not in _HOST:
        _HOST[key] = ops.splitmix_column(seed, 1000, n).to_numpy()
    return _HOST[key]


def splitmix_dev(seed, n, off):
    """rows splitmix64(seed, 1000 ..) starting `off` elements into an aligned buffer"""
    c = ops.splitmix_column(seed, 1000 - off, n + off)
    assert c.ptr % 16 == 0
    return ops.DeviceColumn(c.buf, n, U64, offset=8 * off)


def numpy_dev(arr, dt, off):
    pad = np.zeros(off + len(arr), dtype=arr.dtype)
    pad[off:] = arr
    c = ops.from_numpy(pad, dt)
    assert c.ptr % 16 == 0
    return ops.DeviceColumn(c.buf, len(arr), dt, offset=8 * off)


def as_i64(u):  # signed values over the whole range
    return u.view(np.int64)


def as_f64(u):  # [-1000, 1000)
    return (u >> np.uint64(11)).astype(np.float64) * (2000.0 / (1 << 53)) - 1000.0


# ---------------------------------------------------------------------------
# the oracle: fq_ref per reference block -> what fq_agg_state states
# ---------------------------------------------------------------------------
def ref_scan(names, dts, host, where, arg, block_rows):
    """dict(sum, max, min as fq_ref Values or None; count; flags; abs = sum |x| of a Float64 argument)"""
    n = len(host[0])
    br = block_rows if block_rows > 0 else max(n, 1)
    out = {"sum": None, "max": None, "min": None, "count": 0, "flags": 0, "abs": 0.0, "dtype": None}
    for s in range(0, n, br):
        blk = R.Block([(nm, R.Arr(REF[dt], h[s:s + br])) for nm, dt, h in zip(names, dts, host)])
        try:
            fb = blk
            if where is not None:
                res = where.eval(blk)
                if res.valid is not None and not np.all(res.valid):
                    out["flags"] |= abi.STATE_CAST_NULL  # the device path has no nulls: a cast null is an error
                fb = R.filter_block(where, blk)
            val = arg.eval(fb)
        except R.RefError as e:
            assert "Divide by zero" in str(e), str(e)
            out["flags"] |= abi.STATE_DIV_ZERO
            continue
        if val.valid is not None and not np.all(val.valid):
            out["flags"] |= abi.STATE_CAST_NULL
            continue
        out["dtype"] = DT_OF_REF[val.type]
        kept = len(val)
        out["count"] += kept
        if kept == 0:
            if where is not None:  # arrow sum of a block without rows is None
                out["flags"] |= abi.STATE_ANY_EMPTY
            continue
        if val.type == "Float64":
            with np.errstate(all="ignore"):
                out["abs"] += float(np.abs(val.values[np.isfinite(val.values)]).sum())
        for op in ("sum", "max", "min"):
            with np.errstate(all="ignore"):  # a Float64 sum may overflow to inf or meet inf - inf
                d = R.data_array_aggregate_op(op, val)
            if out[op] is None:
                out[op] = d
            elif op == "sum" and val.type == "Float64":
                out[op] = R.Value(val.type, out[op].value + d.value)
            elif op == "sum":
                out[op] = R.Value(val.type, (out[op].value + d.value) & M64)
            else:
                out[op] = R.data_value_aggregate_op(op, out[op], d)
    return out


def f64_of(bits):
    return np.array([bits], np.uint64).view(np.float64)[0]


def check(st, exp, mask=ALL, what=""):
    """the device state against ref_scan's"""
    assert st.flags & ERR == exp["flags"] & ERR, (what, st.flags, exp["flags"])
    if exp["flags"] & ERR:
        return
    assert st.count == exp["count"], (what, st.count, exp["count"])
    if mask & abi.AGG_SUM:
        assert bool(st.flags & abi.STATE_ANY_EMPTY) == bool(exp["flags"] & abi.STATE_ANY_EMPTY), (what, st.flags)
    if exp["count"] == 0:
        return
    dt = exp["dtype"]
    assert st.dtype == dt, (what, st.dtype, dt)
    if dt == F64:
        if mask & abi.AGG_SUM:
            got, want = f64_of(st.sum), exp["sum"].value
            print("%s f64 sum: got %r want %r bound %r" % (what, got, want, 1e-12 * exp["abs"]))
            if np.isfinite(want):
                assert abs(got - want) <= 1e-12 * exp["abs"], (what, got, want, exp["abs"])
            else:
                assert (np.isnan(got) and np.isnan(want)) or got == want, (what, got, want)
        for op, bits in (("max", st.max), ("min", st.min)):
            if mask & (abi.AGG_MAX if op == "max" else abi.AGG_MIN):
                got, want = f64_of(bits), exp[op].value
                assert (np.isnan(got) and np.isnan(want)) or got == want, (what, op, got, want)
        return
    if mask & abi.AGG_SUM:
        assert st.sum == to_bits(exp["sum"].value, dt), (what, st.sum, exp["sum"])
    if mask & abi.AGG_MAX:
        assert st.max == to_bits(exp["max"].value, dt), (what, st.max, exp["max"])
    if mask & abi.AGG_MIN:
        assert st.min == to_bits(exp["min"].value, dt), (what, st.min, exp["min"])


def fld(n):
    return R.Field(n)


def const(v, t):
    return R.Const(R.Value(t, v))


# ---------------------------------------------------------------------------
# the programs: (column dtypes, host columns of n rows, device builders, fq_pred, fq_expr, oracle filter, oracle argument)
# ---------------------------------------------------------------------------
K38 = 3 << 61  # keeps ~3/8 of uniformly random u64 rows


def case_q6(n):
    """[sum, max, min, count](a * b) WHERE c < k over three u64 columns; the scan's columns are c, a, b"""
    dts = [U64, U64, U64]
    host = [splitmix_host(s, n) for s in (11, 12, 13)]
    dev = [lambda off, s=s: splitmix_dev(s, n, off) for s in (11, 12, 13)]
    pred = predicate_columns(dts, [], "<", K38)
    value, _ = chain_columns(dts, [load(1), ("*", Col(2))])
    where = R.Compare("<", fld("c"), const(K38, "UInt64"))
    arg = R.Arith("*", fld("a"), fld("b"))
    return ["c", "a", "b"], dts, host, dev, pred, value, where, arg


def case_tree(n):
    """(a + b * c) WHERE a < b or c = 7 (u64, u64, u64; c = 7 on every 5th row)"""
    dts = [U64, U64, U64]
    c = splitmix_host(23, n).copy()
    c[::5] = 7
    host = [splitmix_host(21, n), splitmix_host(22, n), c]
    dev = [lambda off: splitmix_dev(21, n, off), lambda off: splitmix_dev(22, n, off), lambda off: numpy_dev(c, U64, off)]
    pred = pred_tree_columns(dts, [([], "<", Col(1)), ([load(2)], "=", 7)], [0, 1, "or"])
    value, _ = chain_columns(dts, [push(1), ("*", Col(2)), ("+", STACK, True)])
    where = R.Logic("or", R.Compare("<", fld("a"), fld("b")), R.Compare("=", fld("c"), const(7, "UInt64")))
    arg = R.Arith("+", fld("a"), R.Arith("*", fld("b"), fld("c")))
    return ["a", "b", "c"], dts, host, dev, pred, value, where, arg


def case_mixed(n):
    """(a * b + c) / d WHERE (b + 1) >= c: u64 < 2^63, i64, f64, u64 (four columns, Float64 result)"""
    dts = [U64, I64, F64, U64]
    a = splitmix_host(31, n) >> np.uint64(40)
    b = as_i64(splitmix_host(32, n)) >> np.int64(41)
    c = as_f64(splitmix_host(33, n))
    d = (splitmix_host(34, n) >> np.uint64(50)) + np.uint64(1)
    host = [a, b, c, d]
    dev = [lambda off, h=h, dt=dt: numpy_dev(h, dt, off) for h, dt in zip(host, dts)]
    pred = predicate_columns(dts, [load(1), ("+", 1)], ">=", Col(2))
    value, _ = chain_columns(dts, [("*", Col(1)), ("+", Col(2)), ("/", Col(3))])
    where = R.Compare(">=", R.Arith("+", fld("b"), const(1, "UInt64")), fld("c"))
    arg = R.Arith("/", R.Arith("+", R.Arith("*", fld("a"), fld("b")), fld("c")), fld("d"))
    return ["a", "b", "c", "d"], dts, host, dev, pred, value, where, arg


def case_two(n):
    """(a - b) % 1000 WHERE a >= b over two columns: u64 and a bitmap-free comparison of columns"""
    dts = [U64, U64]
    host = [splitmix_host(41, n), splitmix_host(42, n)]
    dev = [lambda off, s=s: splitmix_dev(s, n, off) for s in (41, 42)]
    pred = predicate_columns(dts, [], ">=", Col(1))
    value, _ = chain_columns(dts, [("-", Col(1)), ("%", 1000)])
    where = R.Compare(">=", fld("a"), fld("b"))
    arg = R.Arith("%", R.Arith("-", fld("a"), fld("b")), const(1000, "UInt64"))
    return ["a", "b"], dts, host, dev, pred, value, where, arg


CASES = {"q6": case_q6, "tree": case_tree, "mixed": case_mixed, "two": case_two}
# (rows, block_rows): flat sizes as one reference block, then block mode
SIZES = [(1, 0), (3, 0), (2047, 0), (2048, 0), (2049, 0), (3 * (1 << 20) + 5, 0), (30017, 10000), (30017, 8191)]
_REF = {}


def reference(case, n, br):
    key = (case, n, br)
    if key not in _REF:
        names, dts, host, _, _, _, where, arg = CASES[case](n)
        _REF[key] = ref_scan(names, dts, host, where, arg, br)
    return _REF[key]


# the large size runs the three-column and the four-column program
RUNS = [(c, n, br) for c in CASES for n, br in SIZES if n < (1 << 21) or c in ("q6", "mixed")]


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("case,n,br", RUNS, ids=["%s-%d/%d" % r for r in RUNS])
def test_against_oracle(case, n, br, layout):
    names, dts, host, dev, pred, value, where, arg = CASES[case](n)
    cols = [d(off) for d, off in zip(dev, LAYOUTS[layout])]
    if n <= 2049:  # every layout holds the same rows
        for c, h in zip(cols, host):
            assert np.array_equal(c.to_numpy(), h)
    exp = reference(case, n, br)
    st = ops.aggregate_columns(cols, br, pred, value, ALL)
    check(st, exp, ALL, "%s n=%d br=%d %s" % (case, n, br, layout))
    if case == "mixed":
        again = ops.aggregate_columns(cols, br, pred, value, ALL)
        assert bytes(again) == bytes(st)  # float sums too: the partials fold in a fixed order


def test_flat_scan_without_predicate_and_identity_value():
    # no WHERE: max/min/count(a * b); and the identity of column 0 under a predicate on column 1
    n = 4099
    dts = [U64, U64]
    host = [splitmix_host(51, n), splitmix_host(52, n)]
    for layout in ((0, 0), (1, 0)):
        cols = [splitmix_dev(51, n, layout[0]), splitmix_dev(52, n, layout[1])]
        value, _ = chain_columns(dts, [("*", Col(1))])
        exp = ref_scan(["a", "b"], dts, host, None, R.Arith("*", fld("a"), fld("b")), 0)
        check(ops.aggregate_columns(cols, 0, None, value, ALL), exp, ALL, "no predicate")
        pred = predicate_columns(dts, [load(1)], "<", K38)
        exp = ref_scan(["a", "b"], dts, host, R.Compare("<", fld("b"), const(K38, "UInt64")), fld("a"), 1000)
        check(ops.aggregate_columns(cols, 1000, pred, None, ALL), exp, ALL, "identity")


def test_bitmap_predicate_over_columns():
    n, br = 30017, 10000
    dts = [U64, U64]
    host = [splitmix_host(61, n), splitmix_host(62, n)]
    keep = host[0] % np.uint64(3) == 0
    words = np.zeros((n + 63) // 64, np.uint64)
    idx = np.flatnonzero(keep)
    np.bitwise_or.at(words, idx // 64, np.uint64(1) << (idx % 64).astype(np.uint64))
    bm = ops.from_numpy(words, U64)
    pred = abi.fq_pred()
    pred.kind = abi.PRED_BITMAP
    pred.bitmap = bm.ptr
    value, _ = chain_columns(dts, [("+", Col(1))])
    where = R.Compare("=", R.Arith("%", fld("a"), const(3, "UInt64")), const(0, "UInt64"))
    exp = ref_scan(["a", "b"], dts, host, where, R.Arith("+", fld("a"), fld("b")), br)
    for layout in ((0, 0), (1, 1), (0, 1)):
        cols = [splitmix_dev(61, n, layout[0]), splitmix_dev(62, n, layout[1])]
        check(ops.aggregate_columns(cols, br, pred, value, ALL), exp, ALL, "bitmap %r" % (layout,))


# ---------------------------------------------------------------------------
# errors: a predicate error on any row, a value error on a kept row only
# ---------------------------------------------------------------------------
NE = 5003
MODES = [(0, (0, 0, 0)), (0, (0, 1, 0)), (1000, (0, 0, 0)), (1001, (0, 0, 0)), (1000, (1, 0, 0))]


def edge_columns(seed):
    """small u64 a, b in [1, 2^20) and a selector c: rows with c < 10 are kept (every 3rd row)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(1, 1 << 20, NE, dtype=np.uint64)
    b = rng.integers(1, 1 << 20, NE, dtype=np.uint64)
    c = np.full(NE, 100, np.uint64)
    c[::3] = 5
    return a, b, c


def run_edge(dts, host, pred, value, where, arg, br, offs, mask=ALL):
    cols = [numpy_dev(h, dt, off) for h, dt, off in zip(host, dts, offs)]
    st = ops.aggregate_columns(cols, br, pred, value, mask)
    exp = ref_scan(["a", "b", "c"][:len(dts)], dts, host, where, arg, br)
    return st, exp


@pytest.mark.parametrize("br,offs", MODES, ids=[str(m) for m in MODES])
@pytest.mark.parametrize("row", [3003, 3004], ids=["kept", "filtered_out"])
def test_u64_above_i64_max_meets_an_i64_column_in_the_argument(row, br, offs):
    a, b, c = edge_columns(1)
    a[row] = (1 << 63) + 5  # row 3003 is kept (c = 5), row 3004 is not
    dts = [U64, I64, U64]
    host = [a, b.astype(np.int64), c]
    pred = predicate_columns(dts, [load(2)], "<", 10)
    value, _ = chain_columns(dts, [("*", Col(1))])
    where = R.Compare("<", fld("c"), const(10, "UInt64"))
    st, exp = run_edge(dts, host, pred, value, where, R.Arith("*", fld("a"), fld("b")), br, offs)
    assert bool(exp["flags"] & abi.STATE_CAST_NULL) == (row == 3003)
    check(st, exp, ALL, "cast in the argument")
    # the u64 column as the OPERAND of an i64 step (b * a): the same rule
    value, _ = chain_columns(dts, [load(1), ("*", Col(0))])
    st, exp = run_edge(dts, host, pred, value, where, R.Arith("*", fld("b"), fld("a")), br, offs)
    assert bool(exp["flags"] & abi.STATE_CAST_NULL) == (row == 3003)
    check(st, exp, ALL, "cast of the operand column")


@pytest.mark.parametrize("br,offs", MODES, ids=[str(m) for m in MODES])
@pytest.mark.parametrize("row", [3003, 3004], ids=["kept", "filtered_out"])
def test_u64_above_i64_max_meets_an_i64_column_in_the_predicate(row, br, offs):
    # WHERE a < b and c < 10: arrow evaluates a < b on every row, so the cast null raises on either row
    a, b, c = edge_columns(2)
    a[row] = (1 << 63) + 5
    dts = [U64, I64, U64]
    host = [a, b.astype(np.int64), c]
    pred = pred_tree_columns(dts, [([], "<", Col(1)), ([load(2)], "<", 10)], [0, 1, "and"])
    value, _ = chain_columns(dts, [load(2), ("+", 1)])
    where = R.Logic("and", R.Compare("<", fld("a"), fld("b")), R.Compare("<", fld("c"), const(10, "UInt64")))
    # the oracle's cast of that row is null in the leaf (arrow's and() then drops the validity: the
    # reference would quietly lose the row, the device path has no nulls and raises)
    leaf = R.Compare("<", fld("a"), fld("b")).eval(R.Block([("a", R.Arr("UInt64", a)), ("b", R.Arr("Int64", host[1]))]))
    assert leaf.valid is not None and not leaf.valid[row] and leaf.valid.sum() == NE - 1
    cols = [numpy_dev(h, dt, off) for h, dt, off in zip(host, dts, offs)]
    st = ops.aggregate_columns(cols, br, pred, value, ALL)
    assert st.flags & ERR == abi.STATE_CAST_NULL
    # the comparison alone as the predicate: through ref_scan
    pred = predicate_columns(dts, [], "<", Col(1))
    st, exp = run_edge(dts, host, pred, value, R.Compare("<", fld("a"), fld("b")),
                       R.Arith("+", fld("c"), const(1, "UInt64")), br, offs)
    assert exp["flags"] & abi.STATE_CAST_NULL
    check(st, exp, ALL, "cast in the predicate")


@pytest.mark.parametrize("br,offs", MODES, ids=[str(m) for m in MODES])
@pytest.mark.parametrize("row", [3003, 3004, None], ids=["kept", "filtered_out", "none"])
@pytest.mark.parametrize("op", ["/", "%"])
def test_zero_in_a_divisor_column(op, row, br, offs):
    a, b, c = edge_columns(3)
    if row is not None:
        b[row] = 0
    dts = [U64, U64, U64]
    pred = predicate_columns(dts, [load(2)], "<", 10)
    value, _ = chain_columns(dts, [(op, Col(1))])
    where = R.Compare("<", fld("c"), const(10, "UInt64"))
    st, exp = run_edge(dts, [a, b, c], pred, value, where, R.Arith(op, fld("a"), fld("b")), br, offs)
    assert bool(exp["flags"] & abi.STATE_DIV_ZERO) == (row == 3003)
    check(st, exp, ALL, "zero divisor")
    assert bool(st.flags & abi.STATE_DIV_ZERO) == (row == 3003)


@pytest.mark.parametrize("row", [3003, 3004], ids=["kept", "filtered_out"])
def test_zero_divisor_in_the_predicate_raises_on_any_row(row):
    # WHERE a / b < c: the division runs on every row of the block
    a, b, c = edge_columns(4)
    b[row] = 0
    c[:] = 5
    c[row] = 0  # 0 < 0: the row itself would not pass
    dts = [U64, U64, U64]
    pred = predicate_columns(dts, [("/", Col(1))], "<", Col(2))
    value, _ = chain_columns(dts, [("+", Col(1))])
    where = R.Compare("<", R.Arith("/", fld("a"), fld("b")), fld("c"))
    for br, offs in MODES:
        st, exp = run_edge(dts, [a, b, c], pred, value, where, R.Arith("+", fld("a"), fld("b")), br, offs)
        assert exp["flags"] & abi.STATE_DIV_ZERO and st.flags & abi.STATE_DIV_ZERO


@pytest.mark.parametrize("br,offs", MODES, ids=[str(m) for m in MODES])
def test_i64_min_over_minus_one_in_a_column(br, offs):
    # the oracle's pinned choice: i64::MIN / -1 wraps to i64::MIN, x % -1 = 0
    a, b, c = edge_columns(5)
    ai, bi = a.astype(np.int64) - (1 << 19), b.astype(np.int64)
    ai[[0, 3003, 3006]] = np.iinfo(np.int64).min
    bi[[0, 3003, 9]] = -1
    dts = [I64, I64, U64]
    pred = predicate_columns(dts, [load(2)], "<", 10)
    where = R.Compare("<", fld("c"), const(10, "UInt64"))
    for op in ("/", "%"):
        value, _ = chain_columns(dts, [(op, Col(1))])
        st, exp = run_edge(dts, [ai, bi, c], pred, value, where, R.Arith(op, fld("a"), fld("b")), br, offs)
        assert not exp["flags"] & ERR
        check(st, exp, ALL, "i64::MIN %s -1" % op)
    if br == 0:  # the row alone: the wrapped value itself
        value, _ = chain_columns(dts, [("/", Col(1))])
        cols = [numpy_dev(h[:1], dt, 0) for h, dt in zip([ai, bi, c], dts)]
        st = ops.aggregate_columns(cols, 0, pred, value, ALL)
        assert st.count == 1 and st.sum == st.max == st.min == 1 << 63


@pytest.mark.parametrize("br,offs", MODES, ids=[str(m) for m in MODES])
def test_f64_specials_under_max_min(br, offs):
    # NaN, +-inf and +-0.0 in an f64 column; a NaN is never the first kept row of a reference block
    # (arrow 2.0's fold from the first row would make that block NaN, tests/test_edge_values_gpu.py)
    _, _, c = edge_columns(6)
    rng = np.random.default_rng(6)
    x = rng.standard_normal(NE) * 10.0
    specials = [np.nan, np.inf, -np.inf, 0.0, -0.0, np.nan, 1e308, -1e308, 5e-324]
    for i, v in enumerate(specials):
        x[300 * (i + 1) + 3] = v       # 303, 603, ...: kept rows (multiples of 3)
        x[300 * (i + 1) + 4] = v       # and their filtered-out neighbours
    one = np.ones(NE)
    dts = [F64, F64, U64]
    pred = predicate_columns(dts, [load(2)], "<", 10)
    where = R.Compare("<", fld("c"), const(10, "UInt64"))
    mask = abi.AGG_MAX | abi.AGG_MIN | abi.AGG_COUNT
    value, _ = chain_columns(dts, [("*", Col(1))])
    st, exp = run_edge(dts, [x, one, c], pred, value, where, R.Arith("*", fld("a"), fld("b")), br, offs, mask)
    assert exp["max"].value == np.inf and exp["min"].value == -np.inf
    check(st, exp, mask, "specials")
    # without the infinities: the extremes are +-1e308; the zeros and NaNs stay
    y = np.where(np.isinf(x), 1.0, x)
    st, exp = run_edge(dts, [y, one, c], pred, value, where, R.Arith("*", fld("a"), fld("b")), br, offs, mask)
    assert exp["max"].value == 1e308 and exp["min"].value == -1e308
    check(st, exp, mask, "specials without inf")
    # every kept row NaN: NaN, with the count
    z = np.where(c < 10, np.nan, x)
    cols = [numpy_dev(h, dt, off) for h, dt, off in zip([z, one, c], dts, offs)]
    st = ops.aggregate_columns(cols, br, pred, value, mask)
    assert np.isnan(f64_of(st.max)) and np.isnan(f64_of(st.min)) and st.count == int((c < 10).sum())
    # only zeros kept, of both signs: an extreme that is a zero
    w = np.where(np.arange(NE) % 2 == 0, 0.0, -0.0)
    cols = [numpy_dev(h, dt, off) for h, dt, off in zip([w, one, c], dts, offs)]
    st = ops.aggregate_columns(cols, br, pred, value, mask)
    assert f64_of(st.max) == 0.0 and f64_of(st.min) == 0.0


@pytest.mark.parametrize("offs", [(0, 0, 0), (1, 1, 1), (0, 1, 0)], ids=["aligned", "all_offset", "one_offset"])
@pytest.mark.parametrize("br", [1000, 1001])
def test_a_block_without_a_kept_row_sets_any_empty(br, offs):
    a, b, c = edge_columns(7)
    dts = [U64, U64, U64]
    pred = predicate_columns(dts, [load(2)], "<", 10)
    value, _ = chain_columns(dts, [("*", Col(1))])
    where = R.Compare("<", fld("c"), const(10, "UInt64"))
    arg = R.Arith("*", fld("a"), fld("b"))
    st, exp = run_edge(dts, [a, b, c], pred, value, where, arg, br, offs, abi.AGG_SUM | abi.AGG_COUNT)
    assert not exp["flags"] & abi.STATE_ANY_EMPTY and not st.flags & abi.STATE_ANY_EMPTY
    c[2 * br:3 * br] = 100  # the third reference block keeps nothing
    st, exp = run_edge(dts, [a, b, c], pred, value, where, arg, br, offs, abi.AGG_SUM | abi.AGG_COUNT)
    assert exp["flags"] & abi.STATE_ANY_EMPTY and st.flags & abi.STATE_ANY_EMPTY
    check(st, exp, abi.AGG_SUM | abi.AGG_COUNT, "empty block")
    # one reference block that keeps nothing
    c[:] = 100
    st, exp = run_edge(dts, [a, b, c], pred, value, where, arg, 0, offs, abi.AGG_SUM | abi.AGG_COUNT)
    assert st.count == 0 and st.flags & abi.STATE_ANY_EMPTY


ONE_COLUMN = [
    (U64, None, None), (U64, [("+", 1)], ([("%", 8)], "<", 3)), (U64, [("*", "col"), ("-", 1, True)], None),
    (I64, [("/", (-3, "Int64"))], ([], "<", (5, "Int64"))), (F64, [("*", 2.0)], ([], ">=", 0.25)),
]


@pytest.mark.parametrize("dt,steps,pr", ONE_COLUMN, ids=[str(c[1:]) for c in ONE_COLUMN])
@pytest.mark.parametrize("mode", ["interpreted", "specialised"])
def test_one_column_equals_fq_aggregate_byte_for_byte(dt, steps, pr, mode):
    n = 50021
    u = splitmix_host(71, n)
    host = u if dt == U64 else (as_i64(u) if dt == I64 else as_f64(u))
    value = chain(dt, steps)[0] if steps is not None else None
    pred = predicate(dt, *pr) if pr is not None else None
    ops.jit_config(abi.JIT_ALWAYS if mode == "specialised" else abi.JIT_AUTO, 1 << 22)
    try:
        for off in (0, 1):
            col = numpy_dev(host, dt, off)
            for br in (0, 10000):
                want = ops.aggregate(col, br, pred, value, ALL)
                got = ops.aggregate_columns([col], br, pred, value, ALL)
                assert bytes(got) == bytes(want)
    finally:
        ops.jit_config(abi.JIT_AUTO, 1 << 22)


def test_arguments_are_checked():
    from fq_amd._lib import FQError
    a = splitmix_dev(81, 100, 0)
    b = splitmix_dev(82, 101, 0)
    value, _ = chain_columns([U64, U64], [("*", Col(1))])
    with pytest.raises(FQError) as e:
        ops.aggregate_columns([a, b], 0, None, value, ALL)
    assert e.value.status == abi.FQ_E_INVALID and "rows" in str(e.value)
    with pytest.raises(FQError) as e:
        ops.aggregate_columns([a], 0, None, value, ALL)
    assert e.value.status == abi.FQ_E_INVALID and "column index" in str(e.value)
    narrow = ops.from_numpy(np.arange(100, dtype=np.int32), abi.DT_INT32)
    with pytest.raises(FQError) as e:
        ops.aggregate_columns([a, narrow], 0, None, value, ALL)
    assert e.value.status == abi.FQ_E_UNSUPPORTED and "Int32" in str(e.value)
    ops.jit_config(abi.JIT_OFF, 0)
    try:
        with pytest.raises(FQError) as e:
            ops.aggregate_columns([a, splitmix_dev(82, 100, 0)], 0, None, value, ALL)
        assert e.value.status == abi.FQ_E_UNSUPPORTED and "hipRTC" in str(e.value)
    finally:
        ops.jit_config(abi.JIT_AUTO, 1 << 22)
