"""Inputs and expectations of the unfused element-wise kernels (fq_arith,
fq_compare, fq_logic, fq_filter_compact), drawn in one place so that
tests/test_elementwise_cpu.py (no GPU) vouches for what
tests/test_elementwise_gpu.py runs.

Reference: oracle/fq_ref.py data_array_arithmetic_op / data_array_comparison_op
(pinned by the reference's own tables); numpy Boolean masks for logic and
compaction (x[keep] is the definition).  An expectation is an Outcome:

  values       the result column (its dtype is the coercion type) or the rows of a Boolean result
  cast-null    a column row's cast is arrow's null: the device path has no nulls -> FQ_E_UNSUPPORTED, CAST_NULL text
  scalar-null  the scalar's own cast is null: the host-side check answers first -> FQ_E_UNSUPPORTED, SCALAR_NULL text
  div-zero     the reference's RefError -> FQ_E_DIVIDE_BY_ZERO with its text
  error        any other RefError (a None scalar) -> its text

The reference refuses scalar o scalar comparisons (ComparisonFunction's caller
checks that, engine/functions.cpp); fq_compare itself answers the one-row
comparison, so that form is expected as a one-row column against the scalar.

Data classes per column type (column_pair): fit, edge, edge-clipped, zero,
null-then-zero; see each function.  Sides of a case: ("col", type, values at
element offset `off` of a 256-byte aligned buffer) or ("scalar", type, value).
"""
from collections import namedtuple

import numpy as np

import fq_ref as R
import launch_shapes as LS

TYPES = list(R.NUMERIC)
PAIRS = [(l, r) for l in TYPES for r in TYPES]
ARITH_OPS = ["+", "-", "*", "/", "%"]
CMP_OPS = ["=", "<", "<=", ">", ">="]
SMALL = [0, 1, 63, 64, 65, 255, 256, 257, 4099]
LENGTHS = [257, 4099]
DIV_ZERO = "Internal Error: Divide by zero error"
CAST_NULL = "cast produced nulls (nulls are not supported on the device path)"
SCALAR_NULL = "scalar cast produced a null (nulls are not supported on the device path)"
NONE_SCALAR = "Internal Error: DataValue to array cannot be NONE NULL"

Side = namedtuple("Side", "kind type data off")        # kind "col": data = numpy values; "scalar": a Python value / None
Outcome = namedtuple("Outcome", "kind data")            # data: numpy result, or the error text
Case = namedtuple("Case", "fn op form cls n left right exp")


def width(t):
    return np.dtype(R.NP[t]).itemsize


def is_float(t):
    return t.startswith("Float")


def coercion(lt, rt):
    return R.numerical_coercion("+", lt, rt)


# a signed type against an unsigned type at least as wide, in either order: the unsigned side's large values are
# arrow's nulls in the (signed) coercion type
NULL_PAIRS = [(l, r) for l, r in PAIRS if R.is_int(l) and R.is_int(r) and R.is_signed(l) != R.is_signed(r)
              and width(r if R.is_signed(l) else l) >= width(l if R.is_signed(l) else r)]
assert len(NULL_PAIRS) == 20


# ---------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------
def specials(t):
    """the edge values of a type, as a numpy array of it"""
    dt = R.NP[t]
    if is_float(t):
        fi = np.finfo(dt)
        v = [np.nan, np.inf, -np.inf, 0.0, -0.0, float(fi.smallest_subnormal), float(fi.tiny), -float(fi.tiny),
             2.0 ** 24 + 1, 2.0 ** 53 + 1 if t == "Float64" else 2.0 ** 24 - 1, float(fi.max), -float(fi.max), 1.0, -1.0]
        with np.errstate(all="ignore"):
            return np.array(v, dtype=dt)
    lo, hi = R.int_range(t)
    v = [lo, hi, hi - 1, lo + 1]
    v += [x for x in (0, 1, -1) if lo <= x and x not in v]
    # values a float coercion type has to round (Int64 / UInt64: lo and hi are i64::MIN and u64::MAX)
    v += [x for x in (2 ** 24 + 1, 2 ** 53 + 1, 2 ** 31 - 63, 2 ** 63 - 513) if lo <= x <= hi and x not in v]
    return np.array(v, dtype=dt)


def random_full(t, n, rng):
    dt = R.NP[t]
    if is_float(t):
        bits = rng.integers(0, 2 ** (8 * width(t)), n, dtype=np.uint64).astype(np.uint32 if t == "Float32" else np.uint64)
        return bits.view(dt)  # every bit pattern: NaNs, subnormals, both zeros and infinities among them
    lo, hi = R.int_range(t)
    return rng.integers(lo, hi, n, dtype=dt, endpoint=True)


def fit(t, n, rng):
    """values every cast holds"""
    return rng.integers(1, 100, n).astype(R.NP[t])


def nonzero(v):
    out = v.copy()
    out[out == 0] = 1  # also -0.0
    return out


def clip_to(v, t, ct):
    """the values of an integer column of type t clipped to the range of the integer coercion type ct"""
    lo, hi = R.int_range(ct)
    tlo, thi = R.int_range(t)
    return np.clip(v, max(lo, tlo), min(hi, thi)).astype(v.dtype)


def column_pair(cls, lt, rt, n, op, seed):
    """(a, b): n rows of types lt and rt of data class cls
    fit           values 1..99
    edge          every special of lt against every special of rt (rows i < |Sl| * |Sr|), then random over the full
                  range; divisors made non-zero for '/' and '%'
    edge-clipped  edge, with integer values clipped to the coercion type's range (no cast is null)"""
    rng = np.random.default_rng(seed)
    if cls == "fit":
        return fit(lt, n, rng), fit(rt, n, rng)
    assert cls in ("edge", "edge-clipped"), cls
    sl, sr = specials(lt), specials(rt)
    i = np.arange(n)
    a, b = random_full(lt, n, rng), random_full(rt, n, rng)
    k = min(n, len(sl) * len(sr))
    a[:k] = sl[i[:k] % len(sl)]
    b[:k] = sr[(i[:k] // len(sl)) % len(sr)]
    if cls == "edge-clipped":
        ct = coercion(lt, rt)
        assert R.is_int(ct)
        a, b = clip_to(a, lt, ct), clip_to(b, rt, ct)
    if op in ("/", "%"):
        b = nonzero(b)
    return a, b


def scalar_of(cls, t, k, ct=None, divisor=False):
    """the k-th scalar of a class: a special (edge), a small value (fit)"""
    if cls == "fit":
        v = np.array([1 + (7 * k + 3) % 99], dtype=R.NP[t])
    else:
        s = specials(t)
        v = s[k % len(s): k % len(s) + 1].copy()
        if cls == "edge-clipped":
            v = clip_to(v, t, ct)
    if divisor:
        v = nonzero(v)
    return v[0].item()


# ---------------------------------------------------------------------------
# expectations
# ---------------------------------------------------------------------------
def ref_side(side):
    if side.kind == "col":
        return R.Arr(side.type, side.data)
    return R.Value(side.type, side.data)


def scalar_cast_is_null(side, ct):
    if side.kind != "scalar" or side.data is None:
        return False
    return R.cast(R.to_array(R.Value(side.type, side.data), 1), ct).valid is not None


def expect(fn, op, left, right):
    """the Outcome of fq_arith / fq_compare on two Sides"""
    ct = coercion(left.type, right.type)
    try:
        with np.errstate(all="ignore"):
            if fn == "arith":
                res = R.data_array_arithmetic_op(op, ref_side(left), ref_side(right))
            elif left.kind == "scalar" and right.kind == "scalar":
                if left.data is None or right.data is None:
                    raise R.internal("DataValue to array cannot be NONE NULL")
                one = R.to_array(R.Value(left.type, left.data), 1)
                res = R.data_array_comparison_op(op, one, ref_side(right))
            else:
                res = R.data_array_comparison_op(op, ref_side(left), ref_side(right))
    except R.RefError as e:
        return Outcome("div-zero" if str(e) == DIV_ZERO else "error", str(e))
    if res.valid is not None and not np.all(res.valid):
        if scalar_cast_is_null(left, ct) or scalar_cast_is_null(right, ct):
            return Outcome("scalar-null", SCALAR_NULL)
        return Outcome("cast-null", CAST_NULL)
    if fn == "arith":
        assert res.type == ct
        return Outcome("values", res.values)
    return Outcome("values", np.asarray(res.values, dtype=bool))


def col(t, data, off=0):
    return Side("col", t, np.ascontiguousarray(data, dtype=R.NP[t]), off)


def scalar(t, v):
    return Side("scalar", t, v, 0)


def make(fn, op, form, cls, left, right):
    n = len(left.data) if left.kind == "col" else (len(right.data) if right.kind == "col" else 1)
    return Case(fn, op, form, cls, n, left, right, expect(fn, op, left, right))


def classes_of(lt, rt):
    return ["fit", "edge"] + (["edge-clipped"] if (lt, rt) in NULL_PAIRS else [])


def pair_seed(lt, rt, *more):
    s = TYPES.index(lt) * 10 + TYPES.index(rt)
    for m in more:
        s = s * 131 + m
    return s


def pair_cases(fn, lt, rt, lengths=LENGTHS):
    """every operator x form x class of one type pair: column o column, column o scalar and scalar o column at
    `lengths` (columns at element offsets 0 and 1), scalar o scalar once, and for '+' / '=' column o column at
    every SMALL length"""
    ops = ARITH_OPS if fn == "arith" else CMP_OPS
    ct = coercion(lt, rt)
    out = []
    for oi, op in enumerate(ops):
        div = op in ("/", "%")
        for cls in classes_of(lt, rt):
            for li, n in enumerate(lengths):
                a, b = column_pair(cls, lt, rt, n, op, pair_seed(lt, rt, oi, li))
                out.append(make(fn, op, "cc", cls, col(lt, a, li & 1), col(rt, b, 1 - (li & 1))))
                # 20 scalars per pair, class and form (three at the first length, one at the others): every
                # special of either type
                for k in ([4 * oi, 4 * oi + 1, 4 * oi + 2] if li == 0 else [4 * oi + 3]):
                    out.append(make(fn, op, "cs", cls, col(lt, a, 1), scalar(rt, scalar_of(cls, rt, k, ct, div))))
                    out.append(make(fn, op, "sc", cls, scalar(lt, scalar_of(cls, lt, k, ct)), col(rt, b, li & 1)))
    for n in SMALL:
        a, b = column_pair("fit", lt, rt, n, ops[0], pair_seed(lt, rt, 77, n))
        out.append(make(fn, ops[0], "cc", "fit", col(lt, a, n & 1), col(rt, b, 1 - (n & 1))))
    # scalar o scalar, once per pair (n = 1), the operator rotating over the pairs
    op = ops[pair_seed(lt, rt) % len(ops)]
    out.append(make(fn, op, "ss", "fit", scalar(lt, scalar_of("fit", lt, 3)), scalar(rt, scalar_of("fit", rt, 4))))
    return out


def assert_edge_split():
    """the oracle alone: column o column `edge` returns values for 80 of the 100 pairs (400 of 500 pair x
    operator cases) and meets a cast null for exactly the 20 NULL_PAIRS; -> {(pair, op): kind}"""
    kinds = {}
    for lt, rt in PAIRS:
        for oi, op in enumerate(ARITH_OPS):
            a, b = column_pair("edge", lt, rt, 257, op, pair_seed(lt, rt, oi, 0))
            kinds[(lt, rt), op] = expect("arith", op, col(lt, a), col(rt, b)).kind
    bad = sorted({p for (p, _), k in kinds.items() if k != "values"})
    assert bad == sorted(NULL_PAIRS), bad
    assert all(k == "cast-null" for (p, _), k in kinds.items() if p in NULL_PAIRS)
    assert sum(k == "values" for k in kinds.values()) == 400 and len(kinds) == 500
    return kinds


# ---------------------------------------------------------------------------
# error classes
# ---------------------------------------------------------------------------
def zero_pair(ct):
    """a pair of types that lands on the coercion type ct (the same pairs carry the stride cases)"""
    return STRIDE_PAIRS[ct]


def zero_cases(ct, n=4099, rows=None):
    """`fit` with one zero divisor (0, and -0.0 for floats) at row 0, in the middle or at the last row: '/' and
    '%' as column o column, and as column o scalar with the zero as the scalar"""
    lt, rt = zero_pair(ct)
    out = []
    zeros = [0.0, -0.0] if is_float(rt) else [0]
    for oi, op in enumerate(("/", "%")):
        for ri, row in enumerate(rows if rows is not None else (0, n // 2, n - 1)):
            a, b = column_pair("fit", lt, rt, n, op, pair_seed(lt, rt, 5, oi))
            b[row] = zeros[(oi + ri) % len(zeros)]
            out.append(make("arith", op, "cc", "zero", col(lt, a, 1), col(rt, b, 0)))
        out.append(make("arith", op, "cs", "zero", col(lt, a, 0), scalar(rt, zeros[-1])))
    assert all(c.exp.kind == "div-zero" for c in out)
    return out


# an unsigned divisor wider than the signed coercion type: 2^w truncates to 0 in it
NULL_THEN_ZERO_PAIRS = [("Int8", "UInt16"), ("Int8", "UInt32"), ("Int8", "UInt64"), ("Int16", "UInt32"),
                        ("Int16", "UInt64"), ("Int32", "UInt64")]


def null_then_zero_columns(lt, rt, n, with_zero):
    """(a, b): `fit`, one divisor 2^w of the coercion type's width w (out of range: a null whose truncation is
    0) and, with_zero, a genuine zero divisor in another, valid row"""
    rng = np.random.default_rng(pair_seed(lt, rt, 9))
    a, b = fit(lt, n, rng), fit(rt, n, rng)
    b[n // 3] = 1 << (8 * width(lt))
    if with_zero:
        b[(2 * n) // 3] = 0
    return a, b


def null_then_zero_cases(n=257):
    """(a) cast-null, never div-zero; (b) div-zero as in the reference; column o column and scalar o column"""
    out = []
    for lt, rt in NULL_THEN_ZERO_PAIRS:
        for op in ("/", "%"):
            for with_zero in (False, True):
                cls = "null-then-zero-b" if with_zero else "null-then-zero-a"
                a, b = null_then_zero_columns(lt, rt, n, with_zero)
                out.append(make("arith", op, "cc", cls, col(lt, a, 1), col(rt, b, 0)))
                out.append(make("arith", op, "sc", cls, scalar(lt, 7), col(rt, b, 1)))
                assert out[-1].exp.kind == out[-2].exp.kind == ("div-zero" if with_zero else "cast-null")
    return out


def none_scalar_cases():
    rng = np.random.default_rng(3)
    a = fit("Int16", 65, rng)
    return [make("arith", "+", "cs", "none", col("Int16", a), scalar("UInt8", None)),
            make("arith", "/", "sc", "none", scalar("Float32", None), col("Int16", a)),
            make("compare", "<", "cs", "none", col("Int16", a), scalar("Int64", None)),
            make("compare", "=", "sc", "none", scalar("UInt8", None), col("Int16", a))]


# ---------------------------------------------------------------------------
# stride cases: the grid-stride loop's third, ragged round
# ---------------------------------------------------------------------------
# one pair per coercion type, mixed wherever another type casts to it without nulls
STRIDE_PAIRS = {"Float64": ("UInt64", "Float64"), "Float32": ("Float32", "Int64"), "Int64": ("Int64", "UInt32"),
                "Int32": ("UInt16", "Int32"), "Int16": ("Int16", "UInt8"), "Int8": ("Int8", "Int8"),
                "UInt64": ("UInt8", "UInt64"), "UInt32": ("UInt32", "UInt16"), "UInt16": ("UInt8", "UInt16"),
                "UInt8": ("UInt8", "UInt8")}
assert all(coercion(*p) == ct for ct, p in STRIDE_PAIRS.items()) and sorted(STRIDE_PAIRS) == sorted(TYPES)
# the coercion type per width whose `zero` row lies in the second stride round
SECOND_ROUND_ZERO = ["Int8", "UInt16", "Float32", "Int64"]


def stride_rows(cus, fn="arith"):
    m = LS.ew_arith_generic(cus) if fn == "arith" else LS.ew_compare_generic(cus)
    return m.cases()["ragged"][0]


def logic_stride_bits(cus):
    return LS.ew_logic(cus).cases()["ragged"][0]


def stride_columns(ct, n):
    """edge rows first, then random over the full range with non-zero divisors; no cast is null for these pairs"""
    lt, rt = STRIDE_PAIRS[ct]
    a, b = column_pair("edge", lt, rt, n, "/", pair_seed(lt, rt, 11))
    return a, b


def stride_cases(cus, ct):
    """arith ('*' and '%') and compare ('<' and its complement '>=': one of them is set in every row without a NaN) of the coercion type's pair at the stride length: column o
    column, and column o scalar for one operator each"""
    lt, rt = STRIDE_PAIRS[ct]
    n = stride_rows(cus)
    assert n == stride_rows(cus, "compare")
    a, b = stride_columns(ct, n)
    L, Rr = col(lt, a, 1), col(rt, b, 0)
    k = scalar(rt, scalar_of("fit", rt, 5))
    out = [make("arith", "*", "cc", "stride", L, Rr), make("arith", "%", "cc", "stride", L, Rr),
           make("arith", "-", "cs", "stride", L, k),
           make("compare", "<", "cc", "stride", L, Rr), make("compare", ">=", "cc", "stride", L, Rr),
           make("compare", "<=", "sc", "stride", scalar(lt, scalar_of("fit", lt, 6)), Rr)]
    assert all(c.exp.kind == "values" for c in out), (ct, [c.exp.kind for c in out])
    return out


def stride_same_type_cases(cus):
    """8-byte same-type columns at element offset 1 (8 mod 16): the generic kernels over the whole length"""
    n = stride_rows(cus)
    out = []
    for t in ("UInt64", "Float64"):
        a, b = column_pair("edge", t, t, n, "/", pair_seed(t, t, 12))
        out += [make("arith", "/", "cc", "stride", col(t, a, 1), col(t, b, 1)),
                make("compare", "<=", "cc", "stride", col(t, a, 1), col(t, b, 1))]
    return out


def second_round_zero_cases(cus, ct):
    """a `zero` row in the second round of the grid-stride loop (past cap * 256 rows)"""
    n = stride_rows(cus)
    first_round = LS.ew_arith_generic(cus).cap * LS.THREADS
    assert first_round + 1000 < n
    return zero_cases(ct, n, rows=(first_round + 777,))[:1]


# ---------------------------------------------------------------------------
# comparing results
# ---------------------------------------------------------------------------
def same_bits(got, want):
    """bit for bit (the sign of zero included), except that any NaN equals any NaN"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype.kind == "f":
        u = np.uint32 if got.dtype.itemsize == 4 else np.uint64
        nan = np.isnan(got) & np.isnan(want)
        return bool(np.all(nan | (got.view(u) == want.view(u))))
    return bool(np.array_equal(got, want))


def pack(bits, dirty=False, n_words=None):
    """LSB-first uint64 bitmap words of a Boolean array; dirty: every bit past its length set"""
    n = len(bits)
    nw = (n + 63) // 64 if n_words is None else n_words
    full = np.full(nw * 64, dirty, dtype=bool)
    full[:n] = bits
    return np.packbits(full, bitorder="little").view(np.uint64) if nw else np.zeros(0, np.uint64)


def unpack(words, n):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:n].astype(bool)


# ---------------------------------------------------------------------------
# fq_logic and fq_filter_compact inputs
# ---------------------------------------------------------------------------
LOGIC_LENGTHS = SMALL + [1000]
# (lhs, rhs, out) offsets in words from a 16-byte boundary: aligned, and each pointer in turn at 8 mod 16
LOGIC_PLACEMENTS = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)]


def logic_bits(n, seed):
    rng = np.random.default_rng(seed)
    return rng.random(n) < 0.5, rng.random(n) < 0.5


COMPACT_TYPES = ["UInt8", "Int16", "Float32", "UInt32", "UInt64", "Float64"]
COMPACT_LENGTHS = [n for n in SMALL if n] + [16383, 16384, 16385, 16384 * 16 - 1, 16384 * 16 + 1, 16384 * 17 + 5]
SELECTIVITIES = ["none", "all", "3%", "97%", "ends"]


def compact_keep(n, sel, seed):
    """the rows to keep; the last row always is (but for `none`)"""
    rng = np.random.default_rng(seed)
    if sel == "none":
        return np.zeros(n, bool)
    if sel == "all":
        return np.ones(n, bool)
    if sel == "ends":
        keep = np.zeros(n, bool)
        keep[0] = True
    else:
        keep = rng.random(n) < (0.03 if sel == "3%" else 0.97)
    keep[-1] = True
    return keep


def compact_column(t, n, seed):
    return random_full(t, n, np.random.default_rng(seed))


def compact_runs(t):
    """(n, selectivity, dirty tail, bitmap word offset, input element offset, output element offset) of one type:
    every length x selectivity, the placements and tails rotating so that each occurs at every length"""
    out = []
    for li, n in enumerate(COMPACT_LENGTHS):
        for si, sel in enumerate(SELECTIVITIES):
            k = li + si + COMPACT_TYPES.index(t)
            out.append((n, sel, bool(k & 1), (k >> 1) & 1, (k >> 2) & 1, ((k >> 1) ^ k) & 1))
    return out


# ---------------------------------------------------------------------------
# a numpy model of the element-wise path, with switchable mistakes
# ---------------------------------------------------------------------------
MISTAKES = {
    "cast-unchecked": "a cast without the range check",
    "sign-extend": "a sign-extending load of an unsigned narrow type",
    "floor-div": "floor instead of truncating division",
    "min-over-minus-one": "T::MIN / -1 not wrapped",
    "no-flip": "the scalar o column comparison not flipped",
    "div-zero-on-null": "div-zero raised on a null row",
    "one-round": "the second stride round dropped",
    "dirty-tail": "the bitmap tail left dirty",
    "word-boundary": "a compaction position off by one at a 64-row word boundary",
    "wrong-width": "a narrow column compacted at the wrong element size",
}


def model_cast(v, t, ct, mistake=None):
    """(values in ct, ok) of arrow's cast of a column of type t"""
    if mistake == "sign-extend" and R.is_int(t) and not R.is_signed(t) and width(t) < 8:
        v = v.view(np.dtype("i%d" % width(t)))
        t = "Int%d" % (8 * width(t))
    dt = R.NP[ct]
    ok = np.ones(len(v), bool)
    if is_float(ct) or is_float(t):
        assert is_float(ct)
        with np.errstate(all="ignore"):
            return v.astype(dt), ok
    lo, hi = R.int_range(ct)
    if R.is_signed(t):
        s = v.astype(np.int64)
        ok = (s >= lo) & ((s < 0) | (s.astype(np.uint64) <= np.uint64(hi)))
        out = s.astype(dt)
    else:
        u = v.astype(np.uint64)
        ok = u <= np.uint64(hi)
        out = u.astype(dt)
    if mistake == "cast-unchecked":
        ok = np.ones(len(v), bool)
    return out, ok


def model_int_divmod(a, b, ct, mod, mistake=None):
    """truncating '/' and '%' of two columns of the integer type ct, b != 0; wrapping"""
    dt = R.NP[ct]
    if not R.is_signed(ct):
        return (a % b) if mod else (a // b)
    lo, hi = R.int_range(ct)
    x, y = a.astype(np.int64), b.astype(np.int64)
    m1 = y == -1
    ys = np.where(m1, 1, y)
    q = x // ys
    r = x - q * ys
    if mistake != "floor-div":
        fix = (r != 0) & ((x < 0) != (ys < 0))
        q = q + fix
        r = x - q * ys
    neg = (np.uint64(0) - x.view(np.uint64)).view(np.int64)  # -x, wrapping
    if mistake == "min-over-minus-one":
        neg = np.where(x == lo, hi, neg)
    q = np.where(m1, neg, q)
    r = np.where(m1, 0, r)
    return (r if mod else q).astype(dt)


def model_op(op, a, b, ct, mistake=None):
    with np.errstate(all="ignore"):
        if op == "+":
            return a + b
        if op == "-":
            return a - b
        if op == "*":
            return a * b
        if is_float(ct):
            return a / b if op == "/" else np.fmod(a, b)
        bb = np.where(b == 0, np.ones(1, b.dtype), b)
        return np.where(b == 0, np.zeros(1, b.dtype), model_int_divmod(a, bb, ct, op == "%", mistake))


def model_operand(side, ct, n, mistake):
    """(values in ct, ok, scalar cast null)"""
    if side.kind == "col":
        v, ok = model_cast(side.data, side.type, ct, mistake)
        return v, ok, False
    if side.data is None:
        return None, None, None
    v, ok = model_cast(np.array([side.data], dtype=R.NP[side.type]), side.type, ct, mistake)
    return np.repeat(v, n), np.ones(n, bool), not ok[0]


def model(case, mistake=None, round_rows=None):
    """the Outcome of the device path as the kernels compute it: cast, operate, flag, pack.  round_rows: rows the
    grid takes per round of its stride loop (`one-round` computes no row past them)"""
    fn, op, left, right, n = case.fn, case.op, case.left, case.right, case.n
    ct = coercion(left.type, right.type)
    a, oka, na = model_operand(left, ct, n, mistake)
    b, okb, nb = model_operand(right, ct, n, mistake)
    if a is None or b is None:
        return Outcome("error", NONE_SCALAR)
    if na or nb:
        return Outcome("scalar-null", SCALAR_NULL)
    ok = oka & okb
    live = np.ones(n, bool)
    if mistake == "one-round" and round_rows is not None:
        live = np.arange(n) < round_rows
    if fn == "arith":
        zero = (b == 0) & live if op in ("/", "%") else np.zeros(n, bool)
        if np.any(zero if mistake == "div-zero-on-null" else zero & ok):
            return Outcome("div-zero", DIV_ZERO)
        if np.any(~ok & live):
            return Outcome("cast-null", CAST_NULL)
        out = model_op(op, a, b, ct, mistake).astype(R.NP[ct])
        return Outcome("values", np.where(live, out, np.zeros(1, out.dtype)))
    if np.any(~ok & live):
        return Outcome("cast-null", CAST_NULL)
    if left.kind == "scalar" and right.kind == "col" and mistake != "no-flip":
        op, a, b = R.FLIP[op], b, a  # the reference's flipped operator on (column, scalar)
    elif left.kind == "scalar" and right.kind == "col":
        a, b = b, a
    with np.errstate(all="ignore"):
        bits = {"=": a == b, "<": a < b, "<=": a <= b, ">": a > b, ">=": a >= b}[op] & live
    return Outcome("values", model_words(bits, mistake))


def model_words(bits, mistake=None):
    """the bitmap words of a Boolean result (tail clear)"""
    return pack(bits, dirty=mistake == "dirty-tail")


def model_logic(op, lw, rw, n, mistake=None):
    out = (lw & rw) if op == "and" else (lw | rw)
    if n & 63 and mistake != "dirty-tail":
        out = out.copy()
        out[-1] &= np.uint64((1 << (n & 63)) - 1)
    return out


def model_compact(x, words, n, mistake=None):
    """(rows written from position 0, out_len): word w's rows go to the exclusive prefix of the earlier words'
    popcounts (bits past n masked) plus the popcount of the word's lower bits"""
    keep = unpack(words, n)
    esz = x.dtype.itemsize
    src = x
    if mistake == "wrong-width":
        wrong = 2 * esz if esz < 8 else 4
        raw = np.zeros(n * max(wrong, esz) + 8, np.uint8)
        raw[:n * esz] = x.view(np.uint8)
        src = raw[:n * wrong].view(np.dtype("u%d" % wrong))
    pos = np.cumsum(keep) - keep
    if mistake == "word-boundary":
        pos = pos + (np.arange(n) >= 64)
    total = int(keep.sum())
    out = np.zeros(total + 1, src.dtype)
    out[pos[keep]] = src[keep]
    out = out[:total]
    if mistake == "wrong-width":
        b = out.view(np.uint8)
        b = np.concatenate([b, np.zeros(total * esz, np.uint8)])[:total * esz]
        out = b.view(x.dtype)
    return out, total
