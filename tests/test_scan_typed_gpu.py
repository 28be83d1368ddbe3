"""GPU: fq_aggregate_typed (fused aggregate scans over columns, steps and
comparisons of any numeric type) against oracle/fq_ref.py: a Block of the same
columns, FilterTransform (filter_block) and the Agg argument evaluated per
reference block, data_array_aggregate_op per block, the per-block results
merged with data_value_arithmetic_op / data_value_aggregate_op, so narrow sums
wrap and Float32 merges round as the reference's do.

Sizes are the smallest at which the kernel can go wrong: 1, 3, one tile of
256 * G rows and its neighbours for the shape's row group G (and for G = 2, the
first rule's group of the Q6 shape), more than one grid sweep (3 * 2^20 + 5
rows: the tile loop iterates), block mode with a block size on the group's
grid (10000) and off it (8191: the element path).  Every size runs with all
columns aligned, all offset by one row (one shared non-zero phase) and only
one column offset (no shared phase: the element path).

Integer results are bit-exact.  Float64 sums are within 1e-12 * sum(|x|)
(tests/test_kernels_gpu.py).  Float32 max/min are exact; Float32 sums of small
integers (n * max|v| < 2^24: every partial sum is exact in any order) are
bit-equal; one general Float32 sum of n = 20,009 values is within
2 (n - 1) 2^-24 sum(|x|), the any-order recursive-summation bound of both sides."""
import numpy as np
import pytest

import fq_ref as R
from fq_amd import abi
from fq_amd.expr import Col, chain_columns, load, pred_tree_columns, predicate_columns, to_bits

pytestmark = pytest.mark.gpu

ALL = abi.AGG_SUM | abi.AGG_MAX | abi.AGG_MIN | abi.AGG_COUNT
NOSUM = abi.AGG_MAX | abi.AGG_MIN | abi.AGG_COUNT
I8, I16, I32, I64 = abi.DT_INT8, abi.DT_INT16, abi.DT_INT32, abi.DT_INT64
U8, U16, U32, U64 = abi.DT_UINT8, abi.DT_UINT16, abi.DT_UINT32, abi.DT_UINT64
F32, F64 = abi.DT_FLOAT32, abi.DT_FLOAT64
REF = {I8: "Int8", I16: "Int16", I32: "Int32", I64: "Int64", U8: "UInt8", U16: "UInt16", U32: "UInt32",
       U64: "UInt64", F32: "Float32", F64: "Float64"}
DT_OF_REF = {v: k for k, v in REF.items()}
# numerical_coercion's order: a type casts to every type before it (45 casts)
ORDER = [F64, F32, I64, I32, I16, I8, U64, U32, U16, U8]
ERR = abi.STATE_DIV_ZERO | abi.STATE_CAST_NULL
NP = {I8: np.int8, I16: np.int16, I32: np.int32, I64: np.int64, U8: np.uint8, U16: np.uint16, U32: np.uint32,
      U64: np.uint64, F32: np.float32, F64: np.float64}
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


# ---------------------------------------------------------------------------
# the oracle: fq_ref per reference block -> what fq_agg_state states
# ---------------------------------------------------------------------------
def ref_scan(names, dts, host, where, arg, block_rows):
    """dict(sum, max, min as fq_ref Values or None; count; flags; abs = sum |x| of a float argument)"""
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
        if val.type.startswith("Float"):
            with np.errstate(all="ignore"):
                v64 = val.values.astype(np.float64)
                out["abs"] += float(np.abs(v64[np.isfinite(v64)]).sum())
        for op in ("sum", "max", "min"):
            with np.errstate(all="ignore"):
                d = R.data_array_aggregate_op(op, val)
                if out[op] is None:
                    out[op] = d
                elif op == "sum":
                    out[op] = R.data_value_arithmetic_op("+", out[op], d)
                else:
                    out[op] = R.data_value_aggregate_op(op, out[op], d)
    return out


def f64_of(bits):
    return np.array([bits], np.uint64).view(np.float64)[0]


def check(st, exp, mask=ALL, what="", f32_sum="exact", n=0):
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
    if dt in (F32, F64):
        if mask & abi.AGG_SUM:
            got, want = f64_of(st.sum), exp["sum"].value
            if dt == F64:
                bound = 1e-12 * exp["abs"]
            elif f32_sum == "exact":
                bound = 0.0
            else:
                bound = 2.0 * (n - 1) * 2.0 ** -24 * exp["abs"]
            print("%s %s sum: got %r want %r error %r bound %r" % (what, REF[dt], got, want, abs(got - want), bound))
            if dt == F32:
                assert float(np.float32(got)) == got, (what, got)  # a binary32 value, stored widened
            if np.isfinite(want):
                assert abs(got - want) <= bound, (what, got, want, bound)
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
# the three shapes: (names, dtypes, host columns, fq_pred, fq_expr, oracle filter, oracle argument, mask)
# ---------------------------------------------------------------------------
_HOST = {}


def host_cols(kind, n):
    key = (kind, n)
    if key not in _HOST:
        rng = np.random.default_rng(len(kind) * 1000003 + n)
        if kind == "q6":
            _HOST[key] = [rng.uniform(1.0, 1000.0, n), (rng.integers(0, 11, n) / 100.0).astype(np.float32),
                          rng.integers(8000, 10600, n).astype(np.int32), rng.integers(1, 51, n).astype(np.uint8)]
        elif kind == "u8u16":
            _HOST[key] = [rng.integers(0, 256, n).astype(np.uint8), rng.integers(0, 65536, n).astype(np.uint16)]
        else:
            _HOST[key] = [rng.integers(-(1 << 31), 1 << 31, n).astype(np.int32)]
    return _HOST[key]


def case_q6(n):
    """[sum, max, min, count](price * discount) WHERE shipdate < k and quantity < q: about 3/8 of the rows"""
    dts = [F64, F32, I32, U8]
    pred = pred_tree_columns(dts, [([load(2)], "<", (9950, "Int32")), ([load(3)], "<", (26, "UInt8"))], [0, 1, "and"])
    value, vdt = chain_columns(dts, [("*", Col(1))])
    assert vdt == F64
    where = R.Logic("and", R.Compare("<", fld("shipdate"), const(9950, "Int32")),
                    R.Compare("<", fld("quantity"), const(26, "UInt8")))
    arg = R.Arith("*", fld("price"), fld("discount"))
    return ["price", "discount", "shipdate", "quantity"], dts, host_cols("q6", n), pred, value, where, arg, ALL


def case_u8u16(n):
    """[sum, max, min, count](a + b) WHERE a < 100: UInt8 + UInt16 wraps at 16 bits"""
    dts = [U8, U16]
    pred = predicate_columns(dts, [], "<", (100, "UInt8"))
    value, vdt = chain_columns(dts, [("+", Col(1))])
    assert vdt == U16
    where = R.Compare("<", fld("a"), const(100, "UInt8"))
    return ["a", "b"], dts, host_cols("u8u16", n), pred, value, where, R.Arith("+", fld("a"), fld("b")), ALL


def case_i32(n):
    """max(x + x) WHERE x % 8 < 3 over one Int32 column (the planner's UInt64 literals coerce to Int32)"""
    dts = [I32]
    pred = predicate_columns(dts, [("%", 8)], "<", 3)
    assert pred.cmp_dtype == I32 and pred.lhs.steps[0].dtype == I32
    value, vdt = chain_columns(dts, [("+", Col(0))])
    assert vdt == I32
    where = R.Compare("<", R.Arith("%", fld("x"), const(8, "UInt64")), const(3, "UInt64"))
    return ["x"], dts, host_cols("i32", n), pred, value, where, R.Arith("+", fld("x"), fld("x")), abi.AGG_MAX | abi.AGG_COUNT


CASES = {"q6": case_q6, "u8u16": case_u8u16, "i32": case_i32}
# the row group of each shape (fq_scan.h typed_group); q6 also at the first rule's G = 2
GROUPS = {"q6": (2, 4), "u8u16": (16,), "i32": (16,)}
LAYOUTS = {"aligned": (0, 0, 0, 0), "all_offset": (1, 1, 1, 1), "one_offset": (0, 1, 0, 0)}
BIG = 3 * (1 << 20) + 5


def sizes(case):
    flat = [1, 3] + [256 * g + d for g in GROUPS[case] for d in (-1, 0, 1)] + [BIG]
    return [(n, 0) for n in flat] + [(30017, 10000), (30017, 8191)]


RUNS = [(c, n, br) for c in CASES for n, br in sizes(c)]
_REF = {}


def reference(case, n, br):
    key = (case, n, br)
    if key not in _REF:
        names, dts, host, _, _, where, arg, _ = CASES[case](n)
        _REF[key] = ref_scan(names, dts, host, where, arg, br)
    return _REF[key]


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("case,n,br", RUNS, ids=["%s-%d/%d" % r for r in RUNS])
def test_against_oracle(case, n, br, layout):
    names, dts, host, pred, value, where, arg, mask = CASES[case](n)
    offs = LAYOUTS[layout]
    if len(dts) == 1 and layout == "one_offset":
        offs = (1,)  # one column: its own phase, still the grouped path with a head
    cols = [numpy_dev(h, dt, off) for h, dt, off in zip(host, dts, offs)]
    if n <= 4097:  # every layout holds the same rows
        for c, h in zip(cols, host):
            assert np.array_equal(c.to_numpy(), h)
    exp = reference(case, n, br)
    st = ops.aggregate_typed(cols, br, pred, value, mask)
    check(st, exp, mask, "%s n=%d br=%d %s" % (case, n, br, layout))
    if case == "q6":
        again = ops.aggregate_typed(cols, br, pred, value, mask)
        assert bytes(again) == bytes(st)  # float sums too: the partials fold in a fixed order


def test_bitmap_predicate_and_no_predicate():
    n, br = 30017, 10000
    dts = [U8, U16]
    host = host_cols("u8u16", n)
    keep = host[0] % 3 == 0
    words = np.zeros((n + 63) // 64, np.uint64)
    idx = np.flatnonzero(keep)
    np.bitwise_or.at(words, idx // 64, np.uint64(1) << (idx % 64).astype(np.uint64))
    bm = ops.from_numpy(words, U64)
    pred = abi.fq_pred()
    pred.kind = abi.PRED_BITMAP
    pred.bitmap = bm.ptr
    value, _ = chain_columns(dts, [("+", Col(1))])
    arg = R.Arith("+", fld("a"), fld("b"))
    where = R.Compare("=", R.Arith("%", fld("a"), const(3, "UInt8")), const(0, "UInt8"))
    exp = ref_scan(["a", "b"], dts, host, where, arg, br)
    none = ref_scan(["a", "b"], dts, host, None, arg, 0)
    for layout in ((0, 0), (1, 1), (0, 1)):
        cols = [numpy_dev(h, dt, off) for h, dt, off in zip(host, dts, layout)]
        check(ops.aggregate_typed(cols, br, pred, value, ALL), exp, ALL, "bitmap %r" % (layout,))
        check(ops.aggregate_typed(cols, 0, None, value, ALL), none, ALL, "no predicate %r" % (layout,))


# ---------------------------------------------------------------------------
# the 45 casts: target T = column 0 (also the selector: rows with x0 < 10 are
# kept), up to three sources per kernel as operands of T-typed additions
# ---------------------------------------------------------------------------
NE = 5003
CAST_KERNELS = []
for ti, T in enumerate(ORDER[:-1]):
    later = ORDER[ti + 1:]
    for k in range(0, len(later), 3):
        CAST_KERNELS.append((T, tuple(later[k:k + 3])))
assert sum(len(s) for _, s in CAST_KERNELS) == 45 and len(CAST_KERNELS) <= 20


def is_int(dt):
    return dt not in (F32, F64)


def signed(dt):
    return dt in (I8, I16, I32, I64)


def int_max(dt):
    return int(np.iinfo(NP[dt]).max)


def cast_program(T, srcs):
    dts = [T] + list(srcs)
    names = ["x%d" % j for j in range(len(dts))]
    pred = predicate_columns(dts, [], "<", (10, REF[T]))
    steps = [("+", Col(j)) for j in range(1, len(dts))]
    value, vdt = chain_columns(dts, steps)
    assert vdt == T and all(value.steps[i].dtype == T for i in range(len(steps)))
    where = R.Compare("<", fld("x0"), const(10, REF[T]))
    arg = fld("x0")
    for nm in names[1:]:
        arg = R.Arith("+", arg, fld(nm))
    return names, dts, pred, value, where, arg


def cast_columns(T, srcs, seed):
    """small values every type holds: selector x0 in {5 (kept, every 3rd row), 100}; sources in [0, 20]
    (signed ones in [-20, 20]).  Float targets: n * max|v| = 5003 * 160 < 2^24, every partial sum exact."""
    rng = np.random.default_rng(seed)
    x0 = np.full(NE, 100, NP[T])
    x0[::3] = 5
    cols = [x0]
    for s in srcs:
        lo = -20 if signed(s) else 0
        cols.append(rng.integers(lo, 21, NE).astype(NP[s]))
    assert NE * (100 + 20 * len(srcs)) < (1 << 24)
    return cols


# (block_rows, element offsets): flat and block mode are two kernels of a shape, the grouped and the element
# path two branches of one kernel.  The file keeps to about 60 compiled shapes: the cast kernels alternate
# between the two modes, the edge-value programs run in block mode.
FLAT_MODES = [(0, (0, 0, 0, 0)), (0, (0, 1, 0, 0))]
BLOCK_MODES = [(1000, (0, 0, 0, 0)), (1001, (1, 1, 1, 1))]
CAST_MODES = FLAT_MODES + BLOCK_MODES


def cast_modes(T, srcs):
    return FLAT_MODES if CAST_KERNELS.index((T, srcs)) % 2 == 0 else BLOCK_MODES


@pytest.mark.parametrize("T,srcs", CAST_KERNELS, ids=["%s<-%s" % (REF[t], "+".join(REF[s] for s in ss)) for t, ss in CAST_KERNELS])
def test_casts_in_range_are_bit_exact(T, srcs):
    names, dts, pred, value, where, arg = cast_program(T, srcs)
    host = cast_columns(T, srcs, 7)
    for br, offs in cast_modes(T, srcs):
        cols = [numpy_dev(h, dt, off) for h, dt, off in zip(host, dts, offs)]
        exp = ref_scan(names, dts, host, where, arg, br)
        assert not exp["flags"] & ERR and exp["count"] == (NE + 2) // 3
        check(ops.aggregate_typed(cols, br, pred, value, ALL), exp, ALL, "casts to %s br=%d %r" % (REF[T], br, offs))


# integer-narrowing casts: an unsigned source at least as wide as its signed target
NARROWING = [(T, srcs, j) for T, srcs in CAST_KERNELS for j, s in enumerate(srcs)
             if is_int(T) and signed(T) and not signed(s) and NP[s]().itemsize >= NP[T]().itemsize]
assert len(NARROWING) == 10


@pytest.mark.parametrize("row", [3003, 3004], ids=["kept", "filtered_out"])
@pytest.mark.parametrize("T,srcs,j", NARROWING, ids=["%s<-%s" % (REF[t], REF[ss[j]]) for t, ss, j in NARROWING])
def test_narrowing_cast_out_of_range_raises_on_a_kept_row_only(T, srcs, j, row):
    names, dts, pred, value, where, arg = cast_program(T, srcs)
    host = cast_columns(T, srcs, 8)
    host[1 + j][row] = int_max(T) + 1  # row 3003 is kept (x0 = 5), row 3004 is not
    for br, offs in cast_modes(T, srcs):
        cols = [numpy_dev(h, dt, off) for h, dt, off in zip(host, dts, offs)]
        exp = ref_scan(names, dts, host, where, arg, br)
        assert bool(exp["flags"] & abi.STATE_CAST_NULL) == (row == 3003)
        st = ops.aggregate_typed(cols, br, pred, value, ALL)
        assert bool(st.flags & abi.STATE_CAST_NULL) == (row == 3003)
        check(st, exp, ALL, "%s <- %s br=%d %r" % (REF[T], REF[srcs[j]], br, offs))


def test_narrowing_cast_in_the_predicate_raises_on_any_row():
    # WHERE a < b with a UInt32, b Int16: compared as Int16, a's cast runs on every row
    dts = [U32, I16, U8]
    rng = np.random.default_rng(9)
    a = rng.integers(0, 100, NE).astype(np.uint32)
    b = rng.integers(-100, 100, NE).astype(np.int16)
    c = rng.integers(0, 50, NE).astype(np.uint8)
    pred = predicate_columns(dts, [], "<", Col(1))
    assert pred.cmp_dtype == I16
    value, _ = chain_columns(dts, [load(2), ("+", (1, "UInt8"))])
    where = R.Compare("<", fld("a"), fld("b"))
    arg = R.Arith("+", fld("c"), const(1, "UInt8"))
    for bad in (None, 3003):
        if bad is not None:
            a[bad], b[bad] = 40000, -5  # the row would not pass either way
        for br, offs in BLOCK_MODES:
            cols = [numpy_dev(h, dt, off) for h, dt, off in zip([a, b, c], dts, offs)]
            exp = ref_scan(["a", "b", "c"], dts, [a, b, c], where, arg, br)
            assert bool(exp["flags"] & abi.STATE_CAST_NULL) == (bad is not None)
            check(ops.aggregate_typed(cols, br, pred, value, ALL), exp, ALL, "predicate cast")


def test_integer_to_float_casts_round_to_nearest():
    # UInt64, Int64 and UInt32 values that binary32 cannot hold: max/min of x0 + a + b + c in Float32
    dts = [F32, U64, I64, U32]
    n = 4099
    rng = np.random.default_rng(10)
    x0 = np.zeros(n, np.float32)
    a = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    b = rng.integers(-(1 << 62), 1 << 62, n, dtype=np.int64)
    c = rng.integers(1 << 24, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    for j, (src, h) in enumerate(((1, a), (2, b), (3, c))):
        value, vdt = chain_columns(dts, [("+", Col(src))])
        assert vdt == F32
        exp = ref_scan(["x0", "a", "b", "c"], dts, [x0, a, b, c], None, R.Arith("+", fld("x0"), fld("abc"[j])), 0)
        cols = [numpy_dev(hh, dt, 0) for hh, dt in zip([x0, a, b, c], dts)]
        check(ops.aggregate_typed(cols, 0, None, value, NOSUM), exp, NOSUM, "to Float32 from %s" % REF[dts[src]])
        assert exp["max"].value == float(h.astype(np.float32).max())
    # Float32 -> Float64 is exact, UInt64 -> Float64 rounds to nearest
    dts = [F64, F32, U64]
    f = rng.standard_normal(n).astype(np.float32)
    z = np.zeros(n)
    for src, nm in ((1, "f"), (2, "a")):
        value, _ = chain_columns(dts, [("+", Col(src))])
        exp = ref_scan(["z", "f", "a"], dts, [z, f, a], None, R.Arith("+", fld("z"), fld(nm)), 0)
        cols = [numpy_dev(hh, dt, 0) for hh, dt in zip([z, f, a], dts)]
        check(ops.aggregate_typed(cols, 0, None, value, NOSUM), exp, NOSUM, "to Float64 from %s" % nm)


# ---------------------------------------------------------------------------
# wrap and divide at each signed width
# ---------------------------------------------------------------------------
def edge_ints(T, seed):
    """a, b of type T with the extremes on kept and dropped rows, and the UInt8 selector (c < 10: every 3rd row)"""
    info = np.iinfo(NP[T])
    rng = np.random.default_rng(seed)
    a = rng.integers(info.min, int(info.max) + 1, NE).astype(NP[T])
    b = rng.integers(info.min, int(info.max) + 1, NE).astype(NP[T])
    b[b == 0] = 1
    ext = [info.min, info.max, -1, 1]
    for i, (x, y) in enumerate((x, y) for x in ext for y in ext):
        a[30 * i + 3], b[30 * i + 3] = x, y  # kept rows (multiples of 3)
        a[30 * i + 4], b[30 * i + 4] = x, y  # dropped neighbours
    c = np.full(NE, 100, np.uint8)
    c[::3] = 5
    return a, b, c


@pytest.mark.parametrize("op", ["+", "-", "*", "/", "%"])
@pytest.mark.parametrize("T", [I8, I16, I32], ids=["Int8", "Int16", "Int32"])
def test_integer_steps_wrap_and_truncate_at_their_width(T, op):
    a, b, c = edge_ints(T, 11)
    dts = [T, T, U8]
    pred = predicate_columns(dts, [load(2)], "<", (10, "UInt8"))
    value, vdt = chain_columns(dts, [(op, Col(1))])
    assert vdt == T
    where = R.Compare("<", fld("c"), const(10, "UInt8"))
    arg = R.Arith(op, fld("a"), fld("b"))
    for br, offs in BLOCK_MODES:
        cols = [numpy_dev(h, dt, off) for h, dt, off in zip([a, b, c], dts, offs)]
        exp = ref_scan(["a", "b", "c"], dts, [a, b, c], where, arg, br)
        assert not exp["flags"] & ERR
        check(ops.aggregate_typed(cols, br, pred, value, ALL), exp, ALL, "%s %s br=%d" % (REF[T], op, br))
    if op in "/%":  # the row alone, twice as two one-row blocks: MIN / -1 wraps to MIN, MIN % -1 is 0 (_int_div)
        lo = int(np.iinfo(NP[T]).min)
        two = [np.array([lo, lo], NP[T]), np.array([-1, -1], NP[T]), np.array([5, 5], np.uint8)]
        st = ops.aggregate_typed([numpy_dev(h, dt, 0) for h, dt in zip(two, dts)], 1, pred, value, ALL)
        want = to_bits(lo if op == "/" else 0, T)
        assert st.count == 2 and st.max == st.min == want and not st.flags & ERR
        assert st.sum == to_bits(0, T)  # MIN + MIN wraps to 0


@pytest.mark.parametrize("row", [3003, 3004, None], ids=["kept", "filtered_out", "none"])
@pytest.mark.parametrize("op", ["/", "%"])
@pytest.mark.parametrize("T", [I32, F32], ids=["Int32", "Float32"])
def test_zero_divisor_in_the_value_raises_on_a_kept_row_only(T, op, row):
    a, b, c = edge_ints(I32, 12)
    a, b = a.astype(NP[T]), b.astype(NP[T])
    if row is not None:
        b[row] = 0
    dts = [T, T, U8]
    pred = predicate_columns(dts, [load(2)], "<", (10, "UInt8"))
    value, _ = chain_columns(dts, [(op, Col(1))])
    where = R.Compare("<", fld("c"), const(10, "UInt8"))
    for br, offs in CAST_MODES:
        cols = [numpy_dev(h, dt, off) for h, dt, off in zip([a, b, c], dts, offs)]
        exp = ref_scan(["a", "b", "c"], dts, [a, b, c], where, R.Arith(op, fld("a"), fld("b")), br)
        st = ops.aggregate_typed(cols, br, pred, value, NOSUM)
        assert bool(exp["flags"] & abi.STATE_DIV_ZERO) == (row == 3003)
        assert bool(st.flags & abi.STATE_DIV_ZERO) == (row == 3003)
        check(st, exp, NOSUM, "zero divisor %s %s" % (REF[T], op))


def test_zero_divisor_in_the_predicate_raises_on_a_dropped_row():
    # WHERE a / b < c over Int32: the division runs on every row of the block
    a, b, c = edge_ints(I32, 13)
    a, b = np.abs(a // 2), np.abs(b // 2) + 1
    k = np.full(NE, 5, np.int32)
    b[3004], k[3004] = 0, 0  # 0 < 0: the row itself would not pass
    dts = [I32, I32, I32]
    pred = predicate_columns(dts, [("/", Col(1))], "<", Col(2))
    value, _ = chain_columns(dts, [("+", Col(1))])
    where = R.Compare("<", R.Arith("/", fld("a"), fld("b")), fld("c"))
    for br, offs in BLOCK_MODES:
        cols = [numpy_dev(h, dt, off) for h, dt, off in zip([a, b, k], dts, offs)]
        exp = ref_scan(["a", "b", "c"], dts, [a, b, k], where, R.Arith("+", fld("a"), fld("b")), br)
        st = ops.aggregate_typed(cols, br, pred, value, ALL)
        assert exp["flags"] & abi.STATE_DIV_ZERO and st.flags & abi.STATE_DIV_ZERO


# ---------------------------------------------------------------------------
# Float32
# ---------------------------------------------------------------------------
def f32_program():
    dts = [F32, F32, U8]
    pred = predicate_columns(dts, [load(2)], "<", (10, "UInt8"))
    value, vdt = chain_columns(dts, [("*", Col(1))])
    assert vdt == F32
    where = R.Compare("<", fld("c"), const(10, "UInt8"))
    return dts, pred, value, where, R.Arith("*", fld("a"), fld("b"))


def test_f32_sums_of_small_integers_are_bit_equal():
    n = 20009
    rng = np.random.default_rng(14)
    a = rng.integers(-20, 21, n).astype(np.float32)
    b = rng.integers(-20, 21, n).astype(np.float32)
    assert n * 400 < (1 << 24)  # every partial sum is an integer below 2^24: exact in any order
    c = np.full(n, 100, np.uint8)
    c[::3] = 5
    dts, pred, value, where, arg = f32_program()
    for br, offs in CAST_MODES + [(10000, (0, 0, 0, 0))]:
        cols = [numpy_dev(h, dt, off) for h, dt, off in zip([a, b, c], dts, offs)]
        exp = ref_scan(["a", "b", "c"], dts, [a, b, c], where, arg, br)
        check(ops.aggregate_typed(cols, br, pred, value, ALL), exp, ALL, "f32 exact br=%d" % br, f32_sum="exact")


def test_f32_general_sum_within_the_recursive_summation_bound():
    n = 20009
    rng = np.random.default_rng(15)
    a = (rng.standard_normal(n) * 100.0).astype(np.float32)
    b = rng.uniform(0.5, 2.0, n).astype(np.float32)
    c = np.full(n, 5, np.uint8)  # every row kept: n values summed
    dts, pred, value, where, arg = f32_program()
    for br in (0, 10000):
        cols = [numpy_dev(h, dt, 0) for h, dt in zip([a, b, c], dts)]
        exp = ref_scan(["a", "b", "c"], dts, [a, b, c], where, arg, br)
        assert exp["count"] == n
        check(ops.aggregate_typed(cols, br, pred, value, ALL), exp, ALL, "f32 general br=%d" % br, f32_sum="bound", n=n)


@pytest.mark.parametrize("br,offs", CAST_MODES, ids=[str(m) for m in CAST_MODES])
def test_f32_max_min_with_nan(br, offs):
    # a NaN is never the first kept row of a reference block (arrow 2.0 folds from the first row)
    rng = np.random.default_rng(16)
    x = (rng.standard_normal(NE) * 10.0).astype(np.float32)
    for i, v in enumerate([np.nan, np.inf, -np.inf, 0.0, -0.0, np.nan, 3e38, -3e38, 1e-45]):
        x[300 * (i + 1) + 3] = v  # kept rows (multiples of 3)
        x[300 * (i + 1) + 4] = v  # and their dropped neighbours
    one = np.ones(NE, np.float32)
    c = np.full(NE, 100, np.uint8)
    c[::3] = 5
    dts, pred, value, where, arg = f32_program()

    def run(col):
        cols = [numpy_dev(h, dt, off) for h, dt, off in zip([col, one, c], dts, offs)]
        return ops.aggregate_typed(cols, br, pred, value, NOSUM)

    exp = ref_scan(["a", "b", "c"], dts, [x, one, c], where, arg, br)
    assert exp["max"].value == np.inf and exp["min"].value == -np.inf
    check(run(x), exp, NOSUM, "partly NaN")
    y = np.where(np.isinf(x), np.float32(1.0), x)
    exp = ref_scan(["a", "b", "c"], dts, [y, one, c], where, arg, br)
    assert exp["max"].value == float(np.float32(3e38)) and exp["min"].value == float(np.float32(-3e38))
    check(run(y), exp, NOSUM, "partly NaN without inf")
    z = np.where(c < 10, np.float32(np.nan), x)  # every kept row NaN: NaN, with the count
    st = run(z)
    assert np.isnan(f64_of(st.max)) and np.isnan(f64_of(st.min)) and st.count == int((c < 10).sum())


# ---------------------------------------------------------------------------
# all-64-bit shapes are fq_aggregate_columns; the arguments are checked
# ---------------------------------------------------------------------------
def test_all_64_bit_columns_return_the_bytes_of_aggregate_columns():
    n = 50021
    rng = np.random.default_rng(17)
    a = rng.integers(0, 1 << 40, n, dtype=np.uint64)
    b = rng.integers(-(1 << 20), 1 << 20, n, dtype=np.int64)
    f = rng.standard_normal(n)
    dts = [U64, I64, F64]
    pred = predicate_columns(dts, [load(1)], "<", (5, "Int64"))
    value, _ = chain_columns(dts, [("*", Col(1)), ("+", Col(2))])
    for offs in ((0, 0, 0), (1, 1, 1), (0, 1, 0)):
        cols = [numpy_dev(h, dt, off) for h, dt, off in zip([a, b, f], dts, offs)]
        for br in (0, 10000):
            assert bytes(ops.aggregate_typed(cols, br, pred, value, ALL)) == \
                bytes(ops.aggregate_columns(cols, br, pred, value, ALL))
    one = [numpy_dev(a, U64, 0)]
    v1, _ = chain_columns([U64], [("+", 1)])
    assert bytes(ops.aggregate_typed(one, 10000, None, v1, ALL)) == bytes(ops.aggregate_columns(one, 10000, None, v1, ALL))


def test_one_64_bit_column_with_a_load_of_its_one_column():
    """load(0) over one 64-bit column is the program without it (tests/test_fuzz_typed_gpu.py agg seed 17: the
    single-column entry point such a call becomes refused FQ_OP_LOAD as "fq_step: bad op")"""
    n = 30017
    a = np.random.default_rng(18).integers(-(1 << 40), 1 << 40, n).astype(np.int64)
    steps = [("%", (3, "Int64")), ("/", (2147483647, "Int32"))]
    value, vdt = chain_columns([I64], [load(0)] + steps)
    plain, _ = chain_columns([I64], steps)
    assert vdt == I64
    pred = predicate_columns([I64], [load(0)], ">=", (-5, "Int64"))
    where = R.Compare(">=", fld("a"), const(-5, "Int64"))
    arg = R.Arith("/", R.Arith("%", fld("a"), const(3, "Int64")), const(2147483647, "Int32"))
    for br, off in ((0, 0), (0, 1), (10000, 0)):
        cols = [numpy_dev(a, I64, off)]
        st = ops.aggregate_typed(cols, br, pred, value, ALL)
        check(st, ref_scan(["a"], [I64], [a], where, arg, br), ALL, "load(0) br=%d" % br)
        assert bytes(st) == bytes(ops.aggregate_typed(cols, br, predicate_columns([I64], [], ">=", (-5, "Int64")), plain, ALL))
        lone = ops.aggregate_typed(cols, br, None, chain_columns([I64], [load(0)])[0], ALL)
        assert bytes(lone) == bytes(ops.aggregate_typed(cols, br, None, None, ALL))


def test_arguments_are_checked():
    from fq_amd._lib import FQError
    a = numpy_dev(np.arange(100, dtype=np.int32), I32, 0)
    b = numpy_dev(np.arange(101, dtype=np.uint8), U8, 0)
    value, _ = chain_columns([I32, U8], [("*", Col(1))])
    with pytest.raises(FQError) as e:
        ops.aggregate_typed([a, b], 0, None, value, ALL)
    assert e.value.status == abi.FQ_E_INVALID and "rows" in str(e.value)
    with pytest.raises(FQError) as e:
        ops.aggregate_typed([a], 0, None, value, ALL)
    assert e.value.status == abi.FQ_E_INVALID and "column index" in str(e.value)
    ops.jit_config(abi.JIT_OFF, 0)
    try:
        with pytest.raises(FQError) as e:
            ops.aggregate_typed([a, numpy_dev(np.arange(100, dtype=np.uint8), U8, 0)], 0, None, value, ALL)
        assert e.value.status == abi.FQ_E_UNSUPPORTED and "hipRTC" in str(e.value)
    finally:
        ops.jit_config(abi.JIT_AUTO, 1 << 22)
