"""No GPU: what vouches for tests/test_elementwise_gpu.py.

(1) oracle/fq_ref.py against exact arithmetic on the edge rows of every type
    pair x operator x class: Python integers wrapped modulo 2^w with
    truncating division; for a float coercion type the operands converted
    exactly (fractions.Fraction), one operation, one rounding to the format
    (round-half-even written out here, so nothing goes through numpy's casts).
(2) the invariants of tests/elementwise_cases.py: every pair x operator cell
    in every form, the 80 / 20 split of `edge`, a stride case per coercion
    type whose rows reach a third, ragged round at 64, 256 and 304 CUs.
(3) a numpy model of the element-wise path (elementwise_cases.model) agrees
    with the oracle on every generated case, and each of its ten switchable
    mistakes changes the result of at least one of them."""
import math
from fractions import Fraction

import numpy as np
import pytest

import elementwise_cases as E
import fq_ref as R
import launch_shapes as LS

CU_COUNTS = [64, 256, 304]
CUS = 256
FMT = {"Float32": (24, -126, 127), "Float64": (53, -1022, 1023)}  # precision, emin, emax


# ---------------------------------------------------------------------------
# (1) exact arithmetic
# ---------------------------------------------------------------------------
def round_to(fr, t):
    """a Fraction rounded once (half to even) to the float format of t -> Python float (inf on overflow); the
    sign of a zero result is the caller's"""
    if fr == 0:
        return 0.0
    p, emin, emax = FMT[t]
    neg, fr = fr < 0, abs(fr)
    e = fr.numerator.bit_length() - fr.denominator.bit_length()
    if Fraction(2) ** e > fr:
        e -= 1
    assert Fraction(2) ** e <= fr < Fraction(2) ** (e + 1)
    e = max(e, emin)
    ulp = Fraction(2) ** (e - p + 1)
    q, rem = divmod(fr, ulp)
    q = int(q)
    if rem * 2 > ulp or (rem * 2 == ulp and q & 1):
        q += 1
    v = q * ulp
    if v >= Fraction(2) ** (emax + 1):
        return -math.inf if neg else math.inf
    f = float(v)  # exact: v has at most 53 significant bits and lies in binary64's range
    assert Fraction(f) == v
    return -f if neg else f


def neg_sign(x):
    return math.copysign(1.0, x) < 0


def float_op(op, a, b, t):
    """one IEEE operation on two Python floats that hold values of format t, rounded once to t"""
    if not (math.isfinite(a) and math.isfinite(b)):
        if op == "%":
            try:
                return math.fmod(a, b)
            except ValueError:
                return math.nan
        if op == "/":
            return a / b  # b is infinite or NaN, or a is: no division by zero here
        return {"+": a + b, "-": a - b, "*": a * b}[op]  # non-finite in, non-finite or exact out
    fa, fb = Fraction(a), Fraction(b)
    if op in "+-":
        if op == "-":
            fb, b = -fb, -b
        s = fa + fb
        if s == 0:
            return -0.0 if (neg_sign(a) and neg_sign(b)) else 0.0
        return round_to(s, t)
    sign = neg_sign(a) != neg_sign(b)
    if op == "*":
        r = round_to(abs(fa * fb), t)
    elif op == "/":
        r = round_to(abs(fa / fb), t)
    else:
        m = abs(fa) - (abs(fa) // abs(fb)) * abs(fb)
        r, sign = round_to(m, t), neg_sign(a)
    return -r if sign else r


def exact_float(v, t_src, ct):
    """a column value converted to the float coercion type, exactly then rounded once"""
    if E.is_float(t_src):
        return float(v)  # binary32 -> binary64 is exact, and the coercion type is at least as wide
    f = round_to(Fraction(int(v)), ct)
    return f


def exact_row(op, fn, x, lt, y, rt):
    """("null",) | ("value", Python value) of one row in exact arithmetic"""
    ct = E.coercion(lt, rt)
    if E.is_float(ct):
        a, b = exact_float(x, lt, ct), exact_float(y, rt, ct)
        if fn == "compare":
            return ("value", {"=": a == b, "<": a < b, "<=": a <= b, ">": a > b, ">=": a >= b}[op])
        return ("value", float_op(op, a, b, ct))
    lo, hi = R.int_range(ct)
    a, b = int(x), int(y)
    if not (lo <= a <= hi and lo <= b <= hi):
        return ("null",)
    if fn == "compare":
        return ("value", {"=": a == b, "<": a < b, "<=": a <= b, ">": a > b, ">=": a >= b}[op])
    if op in "/%":
        q = abs(a) // abs(b) * (-1 if (a < 0) != (b < 0) else 1)
        r = q if op == "/" else a - q * b
    else:
        r = {"+": a + b, "-": a - b, "*": a * b}[op]
    w = 8 * E.width(ct)
    r &= (1 << w) - 1
    if lo < 0 and r >> (w - 1):
        r -= 1 << w
    return ("value", r)


def check_rows(fn, op, lt, rt, a, b, rows):
    ct = E.coercion(lt, rt)
    with np.errstate(all="ignore"):
        la, ra = R.Arr(lt, a[:rows]), R.Arr(rt, b[:rows])
        res = R.data_array_arithmetic_op(op, la, ra) if fn == "arith" else R.data_array_comparison_op(op, la, ra)
    for i in range(rows):
        want = exact_row(op, fn, a[i], lt, b[i], rt)
        if want[0] == "null":
            assert not res.is_valid(i), (fn, op, lt, rt, i, a[i], b[i])
            continue
        assert res.is_valid(i), (fn, op, lt, rt, i, a[i], b[i])
        got = res.values[i]
        if fn == "arith" and E.is_float(ct):
            w = np.array([want[1]], dtype=R.NP[ct])
            assert float(w[0]) == want[1] or math.isnan(want[1])  # already a value of the format
            assert E.same_bits(np.array([got]), w), (op, lt, rt, i, a[i], b[i], got, want[1])
        else:
            assert got == want[1], (fn, op, lt, rt, i, a[i], b[i], got, want[1])


@pytest.mark.parametrize("lt", E.TYPES)
def test_oracle_matches_exact_arithmetic_on_the_edge_rows(lt):
    for rt in E.TYPES:
        rows = len(E.specials(lt)) * len(E.specials(rt))
        assert rows <= 257
        for fn, ops in (("arith", E.ARITH_OPS), ("compare", E.CMP_OPS)):
            for oi, op in enumerate(ops):
                for cls in E.classes_of(lt, rt):
                    a, b = E.column_pair(cls, lt, rt, 257, op, E.pair_seed(lt, rt, oi, 0))
                    check_rows(fn, op, lt, rt, a, b, rows + 8)  # and a few random rows


def test_round_to_rounds_half_to_even_once():
    assert round_to(Fraction(2 ** 24 + 1), "Float32") == 2.0 ** 24
    assert round_to(Fraction(2 ** 24 + 3), "Float32") == 2.0 ** 24 + 4
    assert round_to(Fraction(2 ** 53 + 1), "Float64") == 2.0 ** 53
    # through binary64 first this would round twice: 2^24 + 1 + 2^-30 lies above the half-way point
    assert round_to(Fraction(2 ** 24 + 1) + Fraction(1, 2 ** 30), "Float32") == 2.0 ** 24 + 2
    assert round_to(Fraction(2 ** 64 - 1), "Float32") == 2.0 ** 64
    assert round_to(Fraction(1, 2 ** 150), "Float32") == 0.0 and round_to(Fraction(3, 2 ** 151), "Float32") == 2.0 ** -149
    assert round_to(Fraction(2 ** 128), "Float32") == math.inf


# ---------------------------------------------------------------------------
# (2) the generator
# ---------------------------------------------------------------------------
_CASES = {}


def pair_cases(fn, lt, rt):
    if (fn, lt, rt) not in _CASES:
        _CASES[fn, lt, rt] = E.pair_cases(fn, lt, rt)
    return _CASES[fn, lt, rt]


def test_the_edge_class_errors_for_the_twenty_listed_pairs_only():
    kinds = E.assert_edge_split()
    assert len({p for (p, _), k in kinds.items() if k == "values"}) == 80


@pytest.mark.parametrize("fn", ["arith", "compare"])
def test_every_cell_occurs_in_every_form_and_class(fn):
    ops = E.ARITH_OPS if fn == "arith" else E.CMP_OPS
    seen_ss = 0
    for lt, rt in E.PAIRS:
        cases = pair_cases(fn, lt, rt)
        for op in ops:
            for form in ("cc", "cs", "sc"):
                for cls in E.classes_of(lt, rt):
                    got = [c for c in cases if (c.op, c.form, c.cls) == (op, form, cls)]
                    assert sorted({c.n for c in got} & set(E.LENGTHS)) == E.LENGTHS, (lt, rt, op, form, cls)
                    for c in got:
                        if cls in ("fit", "edge-clipped"):
                            assert c.exp.kind == "values", (lt, rt, op, form, cls, c.exp)
                        elif (lt, rt) not in E.NULL_PAIRS:
                            assert c.exp.kind == "values", (lt, rt, op, form, cls, c.exp)
                        else:  # edge on one of the 20 pairs: values or a cast null, nothing else
                            assert c.exp.kind in ("values", "cast-null", "scalar-null"), (lt, rt, op, form, c.exp)
        small = [c for c in cases if c.form == "cc" and c.op == ops[0] and c.cls == "fit" and c.left.off == (c.n & 1)
                 and c.right.off == 1 - (c.n & 1)]
        assert sorted({c.n for c in small}) == sorted(E.SMALL), (lt, rt)
        ss = [c for c in cases if c.form == "ss"]
        assert len(ss) == 1 and ss[0].n == 1 and ss[0].exp.kind == "values"
        seen_ss += 1
        # offsets 0 and 1 both occur on either side
        assert {c.left.off for c in cases if c.left.kind == "col"} == {0, 1}
        assert {c.right.off for c in cases if c.right.kind == "col"} == {0, 1}
    assert seen_ss == 100
    # the scalars of `edge` reach every special of either type
    for lt, rt in (("Int8", "Float32"), ("UInt64", "Int64"), ("Float64", "UInt16")):
        cases = pair_cases(fn, lt, rt)
        for form, side, t in (("cs", "right", rt), ("sc", "left", lt)):
            used = [getattr(c, side).data for c in cases if c.form == form and c.cls == "edge"]
            want = E.specials(t)
            if fn == "arith" and form == "cs":
                continue  # divisors are made non-zero there
            assert all(any(E.same_bits(np.array([u], want.dtype), want[i:i + 1]) for u in used)
                       for i in range(len(want))), (lt, rt, form)


def test_scalar_forms_of_compare_expect_the_flipped_operator():
    a = np.array([1, 5, 9], np.int16)
    c = E.make("compare", "<", "sc", "fit", E.scalar("Int16", 5), E.col("Int16", a))
    assert list(c.exp.data) == [False, False, True]  # 5 < x
    c = E.make("compare", "<", "cs", "fit", E.col("Int16", a), E.scalar("Int16", 5))
    assert list(c.exp.data) == [True, False, False]


def test_error_classes_expect_what_the_reference_answers():
    for ct in E.TYPES:
        z = E.zero_cases(ct)
        assert len(z) == 8 and {c.exp.data for c in z} == {E.DIV_ZERO}
        assert E.coercion(*E.zero_pair(ct)) == ct
    ntz = E.null_then_zero_cases()
    assert len(ntz) == 6 * 2 * 2 * 2
    assert {c.cls: c.exp.kind for c in ntz} == {"null-then-zero-a": "cast-null", "null-then-zero-b": "div-zero"}
    for c in ntz:  # the divisor's truncation to the coercion type is 0
        ct = E.coercion(c.left.type, c.right.type)
        big = int(c.right.data.max())
        assert big == 1 << (8 * E.width(ct)) and big & ((1 << (8 * E.width(ct))) - 1) == 0
    # the issue's own example
    c = E.make("arith", "/", "cc", "x", E.col("Int8", [10, 20]), E.col("UInt64", [256, 3]))
    assert c.exp == E.Outcome("cast-null", E.CAST_NULL)
    assert {c.exp for c in E.none_scalar_cases()} == {E.Outcome("error", E.NONE_SCALAR)}
    c = E.make("arith", "+", "cs", "x", E.col("Int8", [1, 2]), E.scalar("UInt8", 200))
    assert c.exp == E.Outcome("scalar-null", E.SCALAR_NULL)


@pytest.mark.parametrize("cus", CU_COUNTS)
def test_stride_lengths_reach_a_third_ragged_round(cus):
    for m in (LS.ew_arith_generic(cus), LS.ew_compare_generic(cus), LS.ew_logic(cus)):
        n = m.cases()["ragged"][0]
        assert n % 2 == 1 and n % m.unit_rows > 3, m.family          # a partial unit and odd rows
        per = m.per_worker(n, m.cap)
        assert len(per) == m.cap and min(per) >= 2 and max(per) == min(per) + 1 == 3, m.family
        assert m.units(n) % m.cap, m.family
    assert E.stride_rows(cus) == E.stride_rows(cus, "compare") == LS.ew_arith_generic(cus).cases()["ragged"][0]
    # fq_logic's own grid: whole word pairs, 256 per workgroup
    bits = E.logic_stride_bits(cus)
    nwords = (bits + 63) // 64
    grid = max(1, min((nwords // 2 + 255) // 256, cus * 2))
    assert grid == LS.ew_logic(cus).cap and nwords // 2 > 2 * grid * 256 and (nwords // 2) % (grid * 256)
    assert bits & 63  # a partial last word
    first_round = LS.ew_arith_generic(cus).cap * 256
    for ct in E.SECOND_ROUND_ZERO:
        (c,) = E.second_round_zero_cases(cus, ct)
        zero_row = int(np.flatnonzero(c.right.data == 0)[0])
        assert first_round <= zero_row < 2 * first_round and c.exp.kind == "div-zero"
    assert sorted(E.width(t) for t in E.SECOND_ROUND_ZERO) == [1, 2, 4, 8]


def test_geometry_restated_from_the_launch_code():
    for cus in CU_COUNTS:
        assert LS.ew_arith_generic(cus) == LS.Model("ew_arith_generic", 256, 8 * cus, True, True)
        assert LS.ew_compare_generic(cus) == LS.Model("ew_compare_generic", 256, 8 * cus, True, True)
        assert LS.ew_logic(cus) == LS.Model("ew_logic", 32768, 2 * cus, True, False)
    assert 1_200_000 < E.stride_rows(256) < 1_250_000 and 39_000_000 < E.logic_stride_bits(256) < 39_500_000


def test_every_coercion_type_has_a_stride_case():
    assert sorted(E.STRIDE_PAIRS) == sorted(E.TYPES)
    for ct, (lt, rt) in E.STRIDE_PAIRS.items():
        assert E.coercion(lt, rt) == ct and (lt, rt) not in E.NULL_PAIRS
        assert lt != rt or ct in ("Int8", "UInt8")  # mixed wherever another type casts to it without nulls


# ---------------------------------------------------------------------------
# (3) the model and its mistakes
# ---------------------------------------------------------------------------
def same_outcome(fn, got, want):
    if got.kind != want.kind:
        return False
    if got.kind != "values":
        return got.data == want.data
    if fn == "compare":  # the model gives words, the expectation rows
        return np.array_equal(got.data, E.pack(want.data))
    return E.same_bits(got.data, want.data)


def all_small_cases():
    for fn in ("arith", "compare"):
        for lt, rt in E.PAIRS:
            yield from pair_cases(fn, lt, rt)
    for ct in E.TYPES:
        yield from E.zero_cases(ct)
    yield from E.null_then_zero_cases()
    yield from E.none_scalar_cases()


def test_model_agrees_with_the_oracle_on_every_generated_case():
    n = 0
    for c in all_small_cases():
        assert same_outcome(c.fn, E.model(c), c.exp), (c.fn, c.op, c.form, c.cls, c.left.type, c.right.type, c.n)
        n += 1
    assert n > 100 * 2 * (5 * 3 * 2 * 2 + 9 + 1)


def caught_by(mistake, cases, **kw):
    return [c for c in cases if not same_outcome(c.fn, E.model(c, mistake, **kw), c.exp)]


@pytest.mark.parametrize("mistake", ["cast-unchecked", "sign-extend", "floor-div", "min-over-minus-one", "no-flip",
                                     "div-zero-on-null"])
def test_value_mistakes_change_a_generated_case(mistake):
    caught = caught_by(mistake, all_small_cases())
    assert caught, mistake
    cls = {c.cls for c in caught}
    if mistake == "div-zero-on-null":  # exactly what null-then-zero (a) is there for
        assert "null-then-zero-a" in cls and cls <= {"null-then-zero-a", "edge"}
    if mistake == "cast-unchecked":
        assert "edge" in cls and "null-then-zero-a" in cls and not cls & {"fit", "edge-clipped"}
    if mistake == "no-flip":
        assert {c.form for c in caught} == {"sc"} and {c.fn for c in caught} == {"compare"}
    if mistake in ("floor-div", "min-over-minus-one"):
        assert {c.op for c in caught} <= {"/", "%"}
        assert {E.coercion(c.left.type, c.right.type) for c in caught} >= {"Int8", "Int16", "Int32", "Int64"}


def test_a_dropped_second_round_changes_every_stride_case():
    round_rows = LS.ew_arith_generic(CUS).cap * 256
    for ct in ("Int8", "Float32", "UInt64"):  # one per kernel width class; the GPU file runs all ten
        cases = E.stride_cases(CUS, ct)
        for c in cases:
            assert same_outcome(c.fn, E.model(c), c.exp), (ct, c.fn, c.op)
            dropped = not same_outcome(c.fn, E.model(c, "one-round", round_rows=round_rows), c.exp)
            # a comparison that holds nowhere past the first round cannot show it; its complement does
            assert dropped == bool(np.any(c.exp.data[round_rows:] != 0)), (ct, c.fn, c.op)
        assert sum(not same_outcome(c.fn, E.model(c, "one-round", round_rows=round_rows), c.exp) for c in cases) >= 5
    for c in pair_cases("arith", "Int8", "UInt8"):  # nothing to see at one round
        assert same_outcome(c.fn, E.model(c, "one-round", round_rows=round_rows), c.exp)
    (c,) = E.second_round_zero_cases(CUS, "UInt16")
    assert E.model(c).kind == "div-zero" and E.model(c, "one-round", round_rows=round_rows).kind == "values"


def test_a_dirty_bitmap_tail_shows_at_every_length_that_has_one():
    for n in E.SMALL + [1000]:
        l, r = E.logic_bits(n, n)
        for op in ("and", "or"):
            want = E.pack((l & r) if op == "and" else (l | r))
            for dirty in (False, True):
                lw, rw = E.pack(l, dirty), E.pack(r, dirty)
                assert np.array_equal(E.model_logic(op, lw, rw, n), want)
                bad = E.model_logic(op, lw, rw, n, "dirty-tail")
                assert (not np.array_equal(bad, want)) == (dirty and n % 64 != 0), (n, op, dirty)
    c = pair_cases("compare", "Int16", "UInt8")[0]
    assert c.n % 64 and not same_outcome("compare", E.model(c, "dirty-tail"), c.exp)


@pytest.mark.parametrize("mistake", ["word-boundary", "wrong-width"])
def test_compaction_mistakes_change_a_generated_case(mistake):
    hit = set()
    for t in E.COMPACT_TYPES:
        for n, sel, dirty, _, _, _ in E.compact_runs(t):
            if n > 20000:
                continue
            x = E.compact_column(t, n, n)
            keep = E.compact_keep(n, sel, n + 1)
            words = E.pack(keep, dirty)
            good, total = E.model_compact(x, words, n)
            assert total == int(keep.sum()) and E.same_bits(good, x[keep]), (t, n, sel, dirty)
            bad, _ = E.model_compact(x, words, n, mistake)
            if not E.same_bits(bad, x[keep]):
                hit.add((t, n > 64, sel))
    if mistake == "word-boundary":  # only past the first word, at every type
        assert hit and all(big for _, big, _ in hit) and {t for t, _, _ in hit} == set(E.COMPACT_TYPES)
    else:
        assert {t for t, _, _ in hit} == set(E.COMPACT_TYPES)


def test_compaction_runs_cover_every_placement_at_every_length():
    for t in E.COMPACT_TYPES:
        runs = E.compact_runs(t)
        assert len(runs) == len(E.COMPACT_LENGTHS) * len(E.SELECTIVITIES)
        for n in E.COMPACT_LENGTHS:
            mine = [r for r in runs if r[0] == n]
            assert {r[1] for r in mine} == set(E.SELECTIVITIES)
            for k in (2, 3, 4, 5):
                assert {r[k] for r in mine} == {0, 1}, (t, n, k)
    assert 16384 * 16 - 1 in E.COMPACT_LENGTHS and 16384 * 16 + 1 in E.COMPACT_LENGTHS
    assert E.compact_keep(100, "ends", 1).sum() == 2 and E.compact_keep(100, "3%", 1)[-1]


def test_the_ten_mistakes_are_the_listed_ones():
    assert len(E.MISTAKES) == 10
