"""GPU: fq_aggregate_nullable (fused aggregate scans over nullable columns:
Arrow validity bitmaps) against oracle/fq_ref.py.  The reference is fq_ref per
reference block, as tests/test_scan_typed_gpu.py has it, over R.Arr(type,
values, valid) columns: FilterTransform (filter_block: a null predicate drops
the row), the Agg argument, data_array_aggregate_op per block (sum / max / min
over the valid values, None when there are none), the blocks merged with
data_value_arithmetic_op / data_value_aggregate_op.  An out-of-range cast is a
null, not an error.  count is compared with the kept rows (nulls included),
valid with the valid kept values, FQ_STATE_ANY_EMPTY with "some block's sum is
None".

One rule is the test's own: fq_ref's data_array_logic_op returns the and / or
of the underlying values without a validity, where arrow 2.0 combines the null
bitmaps (null if either side is null).  For a predicate tree the mask the
oracle keeps is AND-ed here with the validity of every leaf's comparison; where
all leaves are valid the oracle's values are right, so this is exact.

Every value under a 0 bit is garbage chosen to hurt: zero divisors, NaN and
+-inf, the integer extremes (beyond every valid value, outside the range of the
shape's casts, passing the shape's predicates).  The grid has no valid zero
divisor: the expected and the device's error flags are asserted to be 0 there.

Sizes per shape's row group G: 0, 1, 3, 63, 64, 65, 256 G - 1, 256 G,
256 G + 1, 2 * 256 G + G + 3; once 3 * 2^20 + 5 (the tile loop iterates);
block mode 25,003 rows in blocks of 10,000 (on the group's grid) and 8,191 (off
it: the element path).  Every size in three layouts: all columns aligned, all
offset by one row (groups cross bitmap words: a bitmap starts at bit 0 of its
column's view), one column offset (the element path).

Integers are bit-exact, Float64 sums within 1e-12 * sum(|x|) over the valid
kept values, Float32 sums of small integers bit-equal, max / min exact."""
import numpy as np
import pytest

import fq_ref as R
from fq_amd import abi
from fq_amd.expr import Col, chain_columns, load, pred_tree_columns, predicate_columns, to_bits

pytestmark = pytest.mark.gpu

ALL = abi.AGG_SUM | abi.AGG_MAX | abi.AGG_MIN | abi.AGG_COUNT
I8, I16, I32, I64 = abi.DT_INT8, abi.DT_INT16, abi.DT_INT32, abi.DT_INT64
U8, U16, U32, U64 = abi.DT_UINT8, abi.DT_UINT16, abi.DT_UINT32, abi.DT_UINT64
F32, F64 = abi.DT_FLOAT32, abi.DT_FLOAT64
REF = {I8: "Int8", I16: "Int16", I32: "Int32", I64: "Int64", U8: "UInt8", U16: "UInt16", U32: "UInt32",
       U64: "UInt64", F32: "Float32", F64: "Float64"}
DT_OF_REF = {v: k for k, v in REF.items()}
NP = {I8: np.int8, I16: np.int16, I32: np.int32, I64: np.int64, U8: np.uint8, U16: np.uint16, U32: np.uint32,
      U64: np.uint64, F32: np.float32, F64: np.float64}
ERR = abi.STATE_DIV_ZERO | abi.STATE_CAST_NULL
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


def bitmap_dev(valid):
    """an Arrow validity bitmap on the device: bit i = valid[i]; the bits past the last row are set"""
    if valid is None:
        return None
    n = len(valid)
    bits = np.ones(((n + 63) // 64) * 64, bool)
    bits[:n] = valid
    words = np.packbits(bits, bitorder="little").view(np.uint64) if n else np.zeros(0, np.uint64)
    return ops.from_numpy(words, U64)


def group(dts):
    """fq_scan.h typed_group"""
    w = [NP[d]().itemsize for d in dts]

    def fit(nbytes):
        g = 16
        while g > 1 and g * sum(w) > nbytes:
            g >>= 1
        return g
    g0, g1 = fit(64), fit(128)
    return g1 if g0 * min(w) < 4 and g1 * min(w) >= 4 else g0


# ---------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------
def ref_scan(names, dts, host, valid, where, leaves, arg, block_rows):
    """dict(sum, max, min: fq_ref Values or None; count; valid; flags; abs = sum |x| of the valid kept values)"""
    n = len(host[0])
    br = block_rows if block_rows > 0 else max(n, 1)
    out = {"sum": None, "max": None, "min": None, "count": 0, "valid": 0, "flags": 0, "abs": 0.0, "dtype": None}
    for s in range(0, n, br):
        blk = R.Block([(nm, R.Arr(REF[dt], h[s:s + br], None if v is None else v[s:s + br]))
                       for nm, dt, h, v in zip(names, dts, host, valid)])
        try:
            fb = blk
            if where is not None and leaves is None:
                fb = R.filter_block(where, blk)
            elif where is not None:  # a tree: null if any leaf is null (the module's docstring)
                keep = np.array(where.eval(blk).values, bool)
                for lf in leaves:
                    lv = lf.eval(blk).valid
                    if lv is not None:
                        keep &= np.asarray(lv, bool)
                fb = blk.take(keep)
            val = arg.eval(fb)
        except R.RefError as e:
            assert "Divide by zero" in str(e), str(e)
            out["flags"] |= abi.STATE_DIV_ZERO
            continue
        out["dtype"] = DT_OF_REF[val.type]
        out["count"] += len(val)
        ok = np.ones(len(val), bool) if val.valid is None else np.asarray(val.valid, bool)
        out["valid"] += int(ok.sum())
        with np.errstate(all="ignore"):
            d = {op: R.data_array_aggregate_op(op, val) for op in ("sum", "max", "min")}
        if d["sum"].value is None:
            assert not ok.any() and d["max"].value is None and d["min"].value is None
            out["flags"] |= abi.STATE_ANY_EMPTY
            continue
        if val.type.startswith("Float"):
            with np.errstate(all="ignore"):
                v64 = val.values[ok].astype(np.float64)
                out["abs"] += float(np.abs(v64[np.isfinite(v64)]).sum())
        for op in ("sum", "max", "min"):
            with np.errstate(all="ignore"):
                if out[op] is None:
                    out[op] = d[op]
                elif op == "sum":
                    out[op] = R.data_value_arithmetic_op("+", out[op], d[op])
                else:
                    out[op] = R.data_value_aggregate_op(op, out[op], d[op])
    return out


def f64_of(bits):
    return np.array([bits], np.uint64).view(np.float64)[0]


def check(st, exp, mask, what, flags=0):
    """the device's fq_agg_state_n against ref_scan's"""
    s = st.s
    assert exp["flags"] & ERR == flags and s.flags & ERR == flags, (what, s.flags, exp["flags"])
    assert not s.flags & abi.STATE_CAST_NULL, what
    if flags:
        return
    assert s.count == exp["count"], (what, s.count, exp["count"])
    assert st.valid == exp["valid"], (what, st.valid, exp["valid"])
    if mask & abi.AGG_SUM:
        assert bool(s.flags & abi.STATE_ANY_EMPTY) == bool(exp["flags"] & abi.STATE_ANY_EMPTY), (what, s.flags)
    if exp["valid"] == 0:
        return
    dt = exp["dtype"]
    assert s.dtype == dt, (what, s.dtype, dt)
    if dt in (F32, F64):
        if mask & abi.AGG_SUM:
            got, want = f64_of(s.sum), exp["sum"].value
            bound = 1e-12 * exp["abs"] if dt == F64 else 0.0
            if dt == F32:
                assert float(np.float32(got)) == got, (what, got)
            if np.isfinite(want):
                assert abs(got - want) <= bound, (what, got, want, abs(got - want), bound)
            else:
                assert (np.isnan(got) and np.isnan(want)) or got == want, (what, got, want)
        for op, bits in (("max", s.max), ("min", s.min)):
            if mask & (abi.AGG_MAX if op == "max" else abi.AGG_MIN):
                got, want = f64_of(bits), exp[op].value
                assert (np.isnan(got) and np.isnan(want)) or got == want, (what, op, got, want)
        return
    for op, bit, got in (("sum", abi.AGG_SUM, s.sum), ("max", abi.AGG_MAX, s.max), ("min", abi.AGG_MIN, s.min)):
        if mask & bit:
            assert got == to_bits(exp[op].value, dt), (what, op, got, exp[op])


def fld(n):
    return R.Field(n)


def const(v, t):
    return R.Const(R.Value(t, v))


# ---------------------------------------------------------------------------
# shapes: names, dtypes, which columns carry a bitmap, fq_pred, fq_expr, the oracle's filter (with its leaves
# when it is a tree) and argument, mask, base(rng, n) -> the valid values, garbage per column
# ---------------------------------------------------------------------------
class Shape:
    def __init__(self, names, dts, nullable, pred, value, where, leaves, arg, mask, base, garbage):
        self.names, self.dts, self.nullable, self.pred, self.value = names, dts, nullable, pred, value
        self.where, self.leaves, self.arg, self.mask, self.base, self.garbage = where, leaves, arg, mask, base, garbage
        self.G = group(dts)


def shape_q6():
    """[sum, max, min, count](price * discount) WHERE shipdate < k and quantity < q, every column nullable"""
    dts = [F64, F32, I32, U8]
    pred = pred_tree_columns(dts, [([load(2)], "<", (9950, "Int32")), ([load(3)], "<", (26, "UInt8"))], [0, 1, "and"])
    value, vdt = chain_columns(dts, [("*", Col(1))])
    assert vdt == F64
    leaves = [R.Compare("<", fld("shipdate"), const(9950, "Int32")), R.Compare("<", fld("quantity"), const(26, "UInt8"))]
    base = lambda rng, n: [rng.uniform(1.0, 1000.0, n), (rng.integers(0, 11, n) / 100.0).astype(np.float32),
                           rng.integers(8000, 10600, n).astype(np.int32), rng.integers(1, 51, n).astype(np.uint8)]
    garbage = [[np.nan, np.inf, -np.inf, 1e308, -1e308], [np.nan, np.inf, -np.inf, 3e38],
               [-(1 << 31), (1 << 31) - 1, 0], [0, 255]]  # the integer ones pass the predicate
    return Shape(["price", "discount", "shipdate", "quantity"], dts, [1, 1, 1, 1], pred, value,
                 R.Logic("and", leaves[0], leaves[1]), leaves, R.Arith("*", fld("price"), fld("discount")), ALL, base, garbage)


def shape_lone(dt, lo, hi, garbage):
    """[sum, max, min, count](x) over one nullable column"""
    if dt == F64:
        base = lambda rng, n: [rng.uniform(lo, hi, n)]
    else:
        base = lambda rng, n: [rng.integers(lo, hi, n).astype(NP[dt])]
    return Shape(["x"], [dt], [1], None, None, None, None, fld("x"), ALL, base, [garbage])


def shape_div():
    """max(a / b) over Int16, Int16: zero divisors (and MIN / -1) only under null bits"""
    dts = [I16, I16]
    value, vdt = chain_columns(dts, [("/", Col(1))])
    assert vdt == I16

    def base(rng, n):
        b = rng.integers(-50, 50, n).astype(np.int16)
        b[b == 0] = 7
        return [rng.integers(-30000, 30000, n).astype(np.int16), b]
    return Shape(["a", "b"], dts, [1, 1], None, value, None, None, R.Arith("/", fld("a"), fld("b")),
                 abi.AGG_MAX | abi.AGG_COUNT, base, [[-32768, 32767], [0, 0, -1]])


def shape_castnull():
    """sum(a + b) over UInt64, Int8 without any bitmap: computed in Int8, a above 127 (2^63 too) is a null"""
    dts = [U64, I8]
    value, vdt = chain_columns(dts, [("+", Col(1))])
    assert vdt == I8

    def base(rng, n):
        a = rng.integers(0, 100, n).astype(np.uint64)
        bad = rng.random(n) < 0.2
        a[bad] = rng.choice(np.array([1 << 63, (1 << 64) - 1, 128, 200, 1 << 32], np.uint64), int(bad.sum()))
        return [a, rng.integers(-100, 100, n).astype(np.int8)]
    return Shape(["a", "b"], dts, [0, 0], None, value, None, None, R.Arith("+", fld("a"), fld("b")), ALL, base, [[], []])


def shape_cmp():
    """[sum, max, min, count](b + 1) WHERE a < b over UInt32, Int16: compared as Int16, nulls on either side"""
    dts = [U32, I16]
    pred = predicate_columns(dts, [], "<", Col(1))
    assert pred.cmp_dtype == I16
    value, vdt = chain_columns(dts, [load(1), ("+", (1, "Int16"))])
    assert vdt == I16
    base = lambda rng, n: [rng.integers(0, 100, n).astype(np.uint32), rng.integers(-50, 100, n).astype(np.int16)]
    return Shape(["a", "b"], dts, [1, 1], pred, value, R.Compare("<", fld("a"), fld("b")), None,
                 R.Arith("+", fld("b"), const(1, "Int16")), ALL, base, [[(1 << 32) - 1, 40000, 0], [32767, -32768]])


def shape_or():
    """[sum, max, min, count](a + b) WHERE a < 10 or b < 10 over Int32, Int32: null if either leaf is null"""
    dts = [I32, I32]
    pred = pred_tree_columns(dts, [([], "<", (10, "Int32")), ([load(1)], "<", (10, "Int32"))], [0, 1, "or"])
    value, vdt = chain_columns(dts, [("+", Col(1))])
    assert vdt == I32
    leaves = [R.Compare("<", fld("a"), const(10, "Int32")), R.Compare("<", fld("b"), const(10, "Int32"))]
    base = lambda rng, n: [rng.integers(0, 30, n).astype(np.int32), rng.integers(0, 30, n).astype(np.int32)]
    return Shape(["a", "b"], dts, [1, 1], pred, value, R.Logic("or", leaves[0], leaves[1]), leaves,
                 R.Arith("+", fld("a"), fld("b")), ALL, base, [[-(1 << 31), (1 << 31) - 1], [-(1 << 31), (1 << 31) - 1]])


SHAPES = {
    "q6": shape_q6,
    "i32": lambda: shape_lone(I32, -1000000, 1000000, [-(1 << 31), (1 << 31) - 1]),
    "u8": lambda: shape_lone(U8, 1, 200, [0, 255]),
    "f64": lambda: shape_lone(F64, -1000.0, 1000.0, [np.nan, np.inf, -np.inf, 1e308, -1e308]),
    "div": shape_div,
    "castnull": shape_castnull,
    "cmp": shape_cmp,
    "or": shape_or,
}
_SHAPE = {}


def shape(name):
    if name not in _SHAPE:
        _SHAPE[name] = SHAPES[name]()
    return _SHAPE[name]


def test_row_groups():
    assert {k: shape(k).G for k in SHAPES} == {"q6": 4, "i32": 16, "u8": 16, "f64": 8, "div": 16, "castnull": 4,
                                               "cmp": 8, "or": 8}


# ---------------------------------------------------------------------------
# validity patterns
# ---------------------------------------------------------------------------
PATTERNS = ["none", "ones", "zeros", "z_first", "z_63", "z_64", "z_last", "z_tile2_first", "z_tile2_last", "random"]


def pattern(kind, n, G, seed, br=0):
    """the validity of one column (None: no bitmap)"""
    if kind == "none":
        return None
    v = np.ones(n, bool)
    if kind == "zeros":
        v[:] = False
    elif kind == "random":
        v = np.random.default_rng(seed).random(n) >= 0.3
    elif kind == "block_null":  # one reference block entirely null, its neighbours not
        v[br:2 * br] = False
    elif kind != "ones":
        row = {"z_first": 0, "z_63": 63, "z_64": 64, "z_last": n - 1, "z_tile2_first": 256 * G,
               "z_tile2_last": 2 * 256 * G - 1}[kind]
        if 0 <= row < n:
            v[row] = False
    return v


def columns(sh, n, kinds, seed, br=0):
    """host columns (garbage under every 0 bit) and their validity"""
    rng = np.random.default_rng(seed)
    host = sh.base(rng, n)
    valid = []
    for j, (h, kind) in enumerate(zip(host, kinds)):
        v = pattern(kind if sh.nullable[j] else "none", n, sh.G, seed * 7 + j, br)
        valid.append(v)
        if v is not None and not v.all():
            bad = np.flatnonzero(~v)
            g = np.array(sh.garbage[j], dtype=h.dtype)
            h[bad] = g[np.arange(len(bad)) % len(g)]
    return host, valid


def combos(sh, extra=()):
    """pattern per column: combo k gives column j pattern (k + 3 j) mod 10, so every column meets every pattern
    and the columns differ; plus all-random"""
    P = PATTERNS
    out = [tuple(P[(k + 3 * j) % len(P)] for j in range(len(sh.dts))) for k in range(len(P))]
    return out + [("random",) * len(sh.dts)] + [tuple(e for _ in sh.dts) for e in extra]


LAYOUTS = {"aligned": (0, 0, 0, 0), "all_offset": (1, 1, 1, 1), "one_offset": (0, 1, 0, 0)}
_REF = {}


def run_case(name, n, br, kinds, layout, seed):
    sh = shape(name)
    key = (name, n, br, kinds, seed)
    host, valid = columns(sh, n, kinds, seed, br)
    if key not in _REF:
        _REF[key] = ref_scan(sh.names, sh.dts, host, valid, sh.where, sh.leaves, sh.arg, br)
    exp = _REF[key]
    offs = LAYOUTS[layout][:len(sh.dts)]
    if len(sh.dts) == 1 and layout == "one_offset":
        offs = (1,)
    cols = [numpy_dev(h, dt, off) for h, dt, off in zip(host, sh.dts, offs)]
    bms = [bitmap_dev(v) for v in valid]
    st = ops.aggregate_nullable(cols, bms, br, sh.pred, sh.value, sh.mask)
    check(st, exp, sh.mask, "%s n=%d br=%d %s %r" % (name, n, br, layout, kinds))
    return st, exp


def flat_sizes(G):
    return [0, 1, 3, 63, 64, 65, 256 * G - 1, 256 * G, 256 * G + 1, 2 * 256 * G + G + 3]


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("name", list(SHAPES))
def test_flat_against_oracle(name, layout):
    sh = shape(name)
    for n in flat_sizes(sh.G):
        for k, kinds in enumerate(combos(sh)):
            if not any(sh.nullable) and k > 0:
                break  # a shape without bitmaps has one pattern
            run_case(name, n, 0, kinds, layout, 100 + k)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("br", [10000, 8191])
@pytest.mark.parametrize("name", list(SHAPES))
def test_block_mode_against_oracle(name, br, layout):
    sh = shape(name)
    n = 25003
    seen_empty = False
    for k, kinds in enumerate([("random",) * len(sh.dts), ("block_null",) * len(sh.dts),
                               tuple(("block_null", "ones", "none", "random")[j] for j in range(len(sh.dts)))]):
        st, exp = run_case(name, n, br, kinds, layout, 200 + k)
        seen_empty = seen_empty or bool(exp["flags"] & abi.STATE_ANY_EMPTY)
        assert st.s.blocks == (n + br - 1) // br
    if any(sh.nullable):
        assert seen_empty  # the block that is entirely null is a None sum


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_the_tile_loop_iterates(layout):
    n = 3 * (1 << 20) + 5
    st, exp = run_case("q6", n, 0, ("random",) * 4, layout, 300)
    assert 0 < exp["valid"] < exp["count"] < n
    if layout == "aligned":
        sh = shape("q6")
        host, valid = columns(sh, n, ("random",) * 4, 300)
        cols = [numpy_dev(h, dt, 0) for h, dt in zip(host, sh.dts)]
        bms = [bitmap_dev(v) for v in valid]
        again = ops.aggregate_nullable(cols, bms, 0, sh.pred, sh.value, sh.mask)
        assert bytes(again) == bytes(st)  # float sums too: the partials fold in a fixed order


# ---------------------------------------------------------------------------
# named cases
# ---------------------------------------------------------------------------
NE = 5003


def test_all_valid_bitmaps_give_the_typed_scan_and_valid_equals_count():
    sh = shape("q6")
    host, valid = columns(sh, 30017, ("ones",) * 4, 1)
    cols = [numpy_dev(h, dt, 0) for h, dt in zip(host, sh.dts)]
    for br in (0, 10000):
        st = ops.aggregate_nullable(cols, [bitmap_dev(v) for v in valid], br, sh.pred, sh.value, sh.mask)
        typed = ops.aggregate_typed(cols, br, sh.pred, sh.value, sh.mask)
        assert bytes(st.s) == bytes(typed) and st.valid == typed.count and st.reserved == 0
        none = ops.aggregate_nullable(cols, [None] * 4, br, sh.pred, sh.value, sh.mask)
        assert bytes(none) == bytes(st)


@pytest.mark.parametrize("br,offs", [(0, (0, 0, 0)), (0, (1, 1, 1)), (0, (0, 1, 0)), (1000, (0, 0, 0)), (1001, (1, 1, 1))])
def test_zero_divisors(br, offs):
    """value a / b WHERE c < 10 over Int32, Int32, UInt8: a valid zero divisor raises on a kept row only; not
    under a null bit of either operand, and not on a row that is dropped because its predicate is null"""
    dts = [I32, I32, U8]
    rng = np.random.default_rng(21)
    a = rng.integers(-1000, 1000, NE).astype(np.int32)
    b = rng.integers(1, 50, NE).astype(np.int32)
    c = np.full(NE, 100, np.uint8)
    c[::3] = 5  # kept rows: the multiples of 3
    pred = predicate_columns(dts, [load(2)], "<", (10, "UInt8"))
    value, _ = chain_columns(dts, [("/", Col(1))])
    where = R.Compare("<", fld("c"), const(10, "UInt8"))
    arg = R.Arith("/", fld("a"), fld("b"))
    mask = abi.AGG_MAX | abi.AGG_MIN | abi.AGG_COUNT
    row = 3003
    # (what is null at the row, expected flag)
    for null_at, flag in ((None, abi.STATE_DIV_ZERO), ("b", 0), ("a", 0), ("c", 0)):
        bb = b.copy()
        bb[row] = 0
        valid = [np.ones(NE, bool) for _ in dts]
        if null_at is not None:
            valid["abc".index(null_at)][row] = False
        exp = ref_scan(["a", "b", "c"], dts, [a, bb, c], valid, where, None, arg, br)
        cols = [numpy_dev(h, dt, off) for h, dt, off in zip([a, bb, c], dts, offs)]
        st = ops.aggregate_nullable(cols, [bitmap_dev(v) for v in valid], br, pred, value, mask)
        check(st, exp, mask, "zero divisor, null at %s" % null_at, flags=flag)
    # a valid zero divisor on a row the (valid, false) predicate drops: no flag either
    bb = b.copy()
    bb[row + 1] = 0
    valid = [np.ones(NE, bool) for _ in dts]
    exp = ref_scan(["a", "b", "c"], dts, [a, bb, c], valid, where, None, arg, br)
    cols = [numpy_dev(h, dt, off) for h, dt, off in zip([a, bb, c], dts, offs)]
    check(ops.aggregate_nullable(cols, [bitmap_dev(v) for v in valid], br, pred, value, mask), exp, mask, "dropped row")


def test_zero_divisor_in_the_predicate_raises_on_any_row_with_valid_operands():
    # WHERE a / b < c over Int32: the division runs on every row of the block
    dts = [I32, I32, I32]
    rng = np.random.default_rng(22)
    a = rng.integers(0, 1000, NE).astype(np.int32)
    b = rng.integers(1, 50, NE).astype(np.int32)
    k = np.full(NE, 5, np.int32)
    b[3004], k[3004] = 0, 0  # 0 < 0: the row itself would not pass
    pred = predicate_columns(dts, [("/", Col(1))], "<", Col(2))
    value, _ = chain_columns(dts, [("+", Col(1))])
    where = R.Compare("<", R.Arith("/", fld("a"), fld("b")), fld("c"))
    arg = R.Arith("+", fld("a"), fld("b"))
    for null_at, flag in ((None, abi.STATE_DIV_ZERO), (1, 0), (0, 0)):
        valid = [np.ones(NE, bool) for _ in dts]
        if null_at is not None:
            valid[null_at][3004] = False
        for br in (0, 1000):
            exp = ref_scan(["a", "b", "c"], dts, [a, b, k], valid, where, None, arg, br)
            cols = [numpy_dev(h, dt, 0) for h, dt in zip([a, b, k], dts)]
            st = ops.aggregate_nullable(cols, [bitmap_dev(v) for v in valid], br, pred, value, ALL)
            check(st, exp, ALL, "predicate divisor, null at %r" % null_at, flags=flag)


@pytest.mark.parametrize("name", [k for k in SHAPES if k != "castnull"])  # the shapes with a bitmap
def test_every_row_null(name):
    sh = shape(name)
    n = 5003
    host, valid = columns(sh, n, ("zeros",) * len(sh.dts), 5)
    cols = [numpy_dev(h, dt, 0) for h, dt in zip(host, sh.dts)]
    for br in (0, 1000):
        st = ops.aggregate_nullable(cols, [bitmap_dev(v) for v in valid], br, sh.pred, sh.value, sh.mask)
        assert st.valid == 0 and not st.s.flags & ERR
        assert st.s.count == (n if sh.pred is None else 0)  # a null predicate drops the row
        if sh.mask & abi.AGG_SUM:
            assert st.s.flags & abi.STATE_ANY_EMPTY
        assert ops.state_values(st)["sum"] is None


def test_or_of_a_null_leaf_and_a_true_leaf_drops_the_row():
    sh = shape("or")
    a = np.array([5, 50, 5, 50, 5], np.int32)
    b = np.array([50, 5, 5, 50, 5], np.int32)
    va = np.array([1, 0, 1, 1, 0], bool)  # row 1: a null, b < 10 true -> null -> dropped; row 4: both
    vb = np.array([1, 1, 0, 1, 1], bool)  # row 2: a < 10 true, b null -> dropped
    a[~va], b[~vb] = -(1 << 31), -(1 << 31)
    exp = ref_scan(sh.names, sh.dts, [a, b], [va, vb], sh.where, sh.leaves, sh.arg, 0)
    assert exp["count"] == 1 and exp["sum"].value == 55
    st = ops.aggregate_nullable([numpy_dev(a, I32, 0), numpy_dev(b, I32, 0)], [bitmap_dev(va), bitmap_dev(vb)], 0,
                                sh.pred, sh.value, sh.mask)
    check(st, exp, sh.mask, "true or null")
    assert st.s.count == 1 and st.valid == 1 and st.s.sum == 55


@pytest.mark.parametrize("br,off", [(0, 0), (0, 1), (1000, 0), (1001, 1)])
def test_f64_max_with_a_valid_nan_in_the_middle_of_a_block(br, off):
    # a NaN is never the first valid kept row of a reference block (arrow 2.0 folds from the first row)
    sh = shape("f64")
    rng = np.random.default_rng(23)
    x = rng.uniform(-1000.0, 1000.0, NE)
    v = rng.random(NE) >= 0.3
    step = br if br else NE
    for s in range(0, NE, step):
        first = s + int(np.flatnonzero(v[s:s + step])[0])
        if first + 1 < min(s + step, NE):
            x[first + 1], v[first + 1] = np.nan, True  # a valid NaN right after the block's first valid row
    x[~v] = np.where(np.arange(int((~v).sum())) % 2 == 0, np.nan, np.inf)
    exp = ref_scan(["x"], [F64], [x], [v], None, None, fld("x"), br)
    assert np.isfinite(exp["max"].value) and np.isfinite(exp["min"].value)
    mask = abi.AGG_MAX | abi.AGG_MIN | abi.AGG_COUNT
    st = ops.aggregate_nullable([numpy_dev(x, F64, off)], [bitmap_dev(v)], br, None, None, mask)
    check(st, exp, mask, "valid NaN")
    assert st.s.count == NE and st.valid == int(v.sum())


def test_f32_sums_of_small_integers_are_bit_equal():
    n = 20009
    rng = np.random.default_rng(24)
    a = rng.integers(-20, 21, n).astype(np.float32)
    b = rng.integers(-20, 21, n).astype(np.float32)
    assert n * 400 < (1 << 24)  # every partial sum is an integer below 2^24: exact in any order
    va, vb = rng.random(n) >= 0.3, rng.random(n) >= 0.3
    a[~va], b[~vb] = np.nan, np.inf
    dts = [F32, F32]
    value, vdt = chain_columns(dts, [("*", Col(1))])
    assert vdt == F32
    for br, offs in ((0, (0, 0)), (0, (1, 1)), (0, (0, 1)), (10000, (0, 0)), (1001, (1, 1))):
        exp = ref_scan(["a", "b"], dts, [a, b], [va, vb], None, None, R.Arith("*", fld("a"), fld("b")), br)
        cols = [numpy_dev(h, dt, off) for h, dt, off in zip([a, b], dts, offs)]
        st = ops.aggregate_nullable(cols, [bitmap_dev(va), bitmap_dev(vb)], br, None, value, ALL)
        check(st, exp, ALL, "f32 exact br=%d" % br)


def test_count_alone_reads_nothing_and_bitmap_predicates_have_no_validity():
    sh = shape("u8")
    n = 30017
    host, valid = columns(sh, n, ("random",), 6)
    col = numpy_dev(host[0], U8, 0)
    launches = ops.jit_stats()["jit_launches"]
    st = ops.aggregate_nullable([col], [bitmap_dev(valid[0])], 10000, None, None, abi.AGG_COUNT)
    assert st.s.count == n and st.valid == 0 and st.s.blocks == 4
    assert ops.jit_stats()["jit_launches"] == launches  # no scan
    keep = host[0] % 3 == 0
    pred = abi.fq_pred()
    pred.kind = abi.PRED_BITMAP
    kb = bitmap_dev(keep)
    pred.bitmap = kb.ptr
    st = ops.aggregate_nullable([col], [bitmap_dev(valid[0])], 10000, pred, None, ALL)
    assert st.s.count == int(keep.sum()) and st.valid == int((keep & valid[0]).sum())
    assert st.s.sum == int(host[0][keep & valid[0]].sum(dtype=np.uint8))


def test_arguments_are_checked():
    from fq_amd._lib import FQError
    a = numpy_dev(np.arange(100, dtype=np.int32), I32, 0)
    b = numpy_dev(np.arange(101, dtype=np.uint8), U8, 0)
    bm = bitmap_dev(np.ones(128, bool))
    value, _ = chain_columns([I32, U8], [("*", Col(1))])
    with pytest.raises(FQError) as e:
        ops.aggregate_nullable([a, b], [None, None], 0, None, value, ALL)
    assert e.value.status == abi.FQ_E_INVALID and "rows" in str(e.value)
    with pytest.raises(FQError) as e:
        ops.aggregate_nullable([a], None, 0, None, None, ALL)
    assert e.value.status == abi.FQ_E_INVALID and "NULL" in str(e.value)
    with pytest.raises(FQError) as e:
        ops.aggregate_nullable([a], [bm.ptr + 4], 0, None, None, ALL)
    assert e.value.status == abi.FQ_E_INVALID and "aligned" in str(e.value)
    ops.jit_config(abi.JIT_OFF, 0)
    try:
        with pytest.raises(FQError) as e:
            ops.aggregate_nullable([a], [bm], 0, None, None, ALL)
        assert e.value.status == abi.FQ_E_UNSUPPORTED and "hipRTC" in str(e.value)
    finally:
        ops.jit_config(abi.JIT_AUTO, 1 << 22)
