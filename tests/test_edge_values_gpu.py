"""Int64 / Float64 / UInt64 edge values in every fused kernel.

The workload columns are small consecutive UInt64 numbers; here the columns
hold the values where signed and IEEE code goes wrong -- i64::MIN/MAX, the
sign boundary, 2^31/2^32/2^53 neighbours, NaN, +-inf, +-0.0, DBL_MAX, the
smallest subnormal, u64 >= 2^63 -- at index 0, inside a scan tile, in the
vector remainder and in the last row.  References: the C oracle
(oracle_c.column_partial) for aggregate states, numpy for rows; integers and
Float64 max/min by bits, Float64 sums by the project's bound
1e-12 * sum(|kept finite x|) or by class (NaN / +inf / -inf).

Float64 max/min contract of the device: the fold of Rust's
f64::max / f64::min over the kept rows -- a NaN is ignored unless every kept
row is NaN.  arrow 2.0's min_max_helper folds from the block's first row
instead, so a reference block whose first kept row is NaN followed by other
rows yields NaN; that one deviation (and the sign of a zero extreme) is pinned
by test_f64_minmax_deviation_from_arrow_fold_is_pinned.

The column builders below need no GPU; tests/test_edge_values_cpu.py imports
them and checks their preconditions against the oracle."""
import numpy as np
import pytest

from fq_amd import abi
from fq_amd.expr import COL, PUSH, STACK, chain, predicate, pred_tree

import oracle_c
from replay import as_tuple, replay

pytestmark = pytest.mark.gpu

ops = None
U64, I64, F64 = abi.DT_UINT64, abi.DT_INT64, abi.DT_FLOAT64
ALL = abi.AGG_SUM | abi.AGG_MAX | abi.AGG_MIN | abi.AGG_COUNT
EXT = abi.AGG_MAX | abi.AGG_MIN | abi.AGG_COUNT
AGGS = [abi.AGG_SUM, abi.AGG_MAX, abi.AGG_MIN, abi.AGG_COUNT]

# the flat scan's workgroup tile is 4 vectors x 256 lanes x 2 rows = 2048 rows:
# N0 runs the tile loop, the vector remainder (36 rows) and the scalar tail (1)
N0 = 3 * 2048 + 37
NB = 25_003        # three 10,000-row reference blocks (the last short), 391 of 64 rows
NBIG = 1_050_001   # every one of the flat grid's 512 workgroups holds a tile
I64_MIN, I64_MAX = -2**63, 2**63 - 1
DBL_MAX = np.finfo(np.float64).max
SUBNORMAL = 5e-324
INF, NAN = float("inf"), float("nan")
DIV_ZERO = "Internal Error: Divide by zero error"

PLACES = ("first", "tile", "vec_rem", "last")
I64_SPECIALS = [I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX, 2**31, -2**31, 2**32, -2**32,
                2**53 + 1, 2**53 - 1, -(2**53 + 1), -(2**53 - 1)]
I64_K = [-1, 1, -2, 2, -3, 3, 7, -7, 10000, -10000, 2**31, -2**31, 2**32 + 1, I64_MIN, I64_MAX]
I64_CMP_K = [I64_MIN, -1, 0, 1, I64_MAX]
F64_CMP_K = [NAN, INF, -INF, 0.0, -0.0, 1.5]
CMPS = ["=", "<", "<=", ">", ">="]
NP_CMP = {"=": np.equal, "<": np.less, "<=": np.less_equal, ">": np.greater, ">=": np.greater_equal}


# ---------------------------------------------------------------------------
# shared inputs (no GPU needed)
# ---------------------------------------------------------------------------
def place_index(n, place, run=1):
    """First row of a run of `run` specials at one of the four places: row 0,
    inside the first 2048-row tile, the vector remainder after the last whole
    tile, and the column's last rows (the run ends on row n - 1)."""
    assert n % 2048 >= 2 * run + 2, "no room for the remainder and tail runs"
    return {"first": 0, "tile": 1000, "vec_rem": (n // 2048) * 2048 + 2, "last": n - run}[place]


def _put(x, specials, places):
    """The specials as a run at every place, rotated so that a different one
    sits on row 0 and on the last row."""
    for g, place in enumerate(PLACES):
        if place not in places:
            continue
        r = specials[2 * g:] + specials[:2 * g]
        if place == "last":
            r = specials[::-1]  # specials[0] on the last row
        i = place_index(len(x), place, len(r))
        x[i:i + len(r)] = r


def i64_column(n=N0, places=PLACES, zero_free=False, seed=1):
    """Random full-range int64 with I64_SPECIALS at `places`; zero_free: no
    zero anywhere (for `k / x`)."""
    rng = np.random.default_rng(seed)
    x = rng.integers(I64_MIN, I64_MAX, size=n, dtype=np.int64, endpoint=True)
    _put(x, [v for v in I64_SPECIALS if not (zero_free and v == 0)], places)
    if zero_free:
        x[x == 0] = 1
    return x


def block_starts(n, block_rows):
    return range(0, n, block_rows if block_rows > 0 else max(n, 1))


def first_kept_rows(keep, block_rows):
    """Index of every reference block's first kept row (blocks keeping none skipped)."""
    n, out = len(keep), []
    for s in block_starts(n, block_rows):
        k = np.flatnonzero(keep[s:s + (block_rows if block_rows > 0 else n)])
        if len(k):
            out.append(s + int(k[0]))
    return out


def keep_mask(n, block_sizes, seed=3):
    """A bitmap predicate's rows: ~60% at random, the special runs' rows and
    every block's first row kept (no reference block ends up empty)."""
    rng = np.random.default_rng(seed)
    keep = rng.random(n) < 0.6
    for place in PLACES:
        i = place_index(n, place, 8)
        keep[i:i + 8] = True
    for br in block_sizes:
        keep[list(block_starts(n, br))] = True
    return keep


def f64_column(variant, n=N0, block_sizes=(10000,), keep=None, infs="both", extremes=False, places=PLACES,
               seed=2):
    """Finite fill of magnitude <= 1e6 with the Float64 specials at `places`.

    variant: nan_safe   NaNs at the places and sprinkled, but never a reference
                        block's first kept row (asserted for every block size)
             all_nan    every kept row NaN (dropped rows stay finite)
             nan_first_mixed   the first kept row of the first block is NaN and
                        that block holds the column's extremes
             no_nan     the specials without NaN
             zeros_max / zeros_min   +-0.0 are the maximum / minimum
    infs: which infinities are among the specials; extremes: DBL_MAX, -DBL_MAX
    and the smallest subnormal too (such columns are scanned without SUM)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1e6, 1e6, size=n)
    kept = keep if keep is not None else np.ones(n, bool)
    sp = [0.0, -0.0] + {"both": [INF, -INF], "pos": [INF], "neg": [-INF], "none": []}[infs]
    if extremes:
        sp += [DBL_MAX, -DBL_MAX, SUBNORMAL]
    if variant == "nan_safe":
        x[rng.random(n) < 0.02] = NAN
        _put(x, sp[:2] + [NAN] + sp[2:], places)
        for br in block_sizes:
            for i in first_kept_rows(kept, br):
                if np.isnan(x[i]):
                    x[i] = 0.5
        for br in block_sizes:
            assert not np.isnan(x[first_kept_rows(kept, br)]).any()
        assert np.isnan(x[kept]).sum() >= 4
    elif variant == "all_nan":
        x[kept] = NAN
    elif variant == "nan_first_mixed":
        br = block_sizes[0]
        first = first_kept_rows(kept, br)[0]
        x[br:] *= 1e-3  # the later blocks' extremes lie inside the first block's
        x[first] = NAN
        rest = np.flatnonzero(kept[:br if br > 0 else n])
        x[rest[1]], x[rest[2]] = 1e6, -1e6
    elif variant == "no_nan":
        _put(x, sp, places)
    elif variant in ("zeros_max", "zeros_min"):
        x = -np.abs(x) - 1.0 if variant == "zeros_max" else np.abs(x) + 1.0
        _put(x, [0.0, -0.0, -0.0, 0.0], places)
    else:
        raise ValueError(variant)
    return x


def u64_full_range(n=N0, seed=0x5EED):
    """splitmix64 values: half of them >= 2^63, most > 2^53."""
    L = oracle_c.lib()
    x = np.array([L.fqo_splitmix64(seed, i) for i in range(n)], dtype=np.uint64)
    assert (x >> np.uint64(63)).sum() > n // 3 and (x > np.uint64(2**53)).sum() > n * 9 // 10
    return x


def u64_cast_null_column(place, n=N0):
    """arange with a single 2^63 (the smallest value the Int64 cast nulls)."""
    x = np.arange(n, dtype=np.uint64)
    x[place_index(n, place)] = np.uint64(2**63)
    return x


def contract_minmax(x):
    """(max, min) of the device contract: f64::max / f64::min folds."""
    return np.fmax.reduce(x), np.fmin.reduce(x)


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def f64_of(b):
    return float(np.array([b], dtype=np.uint64).view(np.float64)[0])


def trunc_div_i64(a, b):
    """Rust's wrapping_div / wrapping_rem on int64 arrays (the reference's
    arithmetic), b != 0: truncating, i64::MIN / -1 = i64::MIN, x % -1 = 0.
    (tests/test_kernels_gpu.py's _trunc_divmod takes abs(), which i64::MIN has
    not; here numpy's floor division is corrected towards zero.)"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    m1 = b == -1
    bb = np.where(m1, np.int64(1), b)
    q = a // bb
    r = a - q * bb
    fix = (r != 0) & ((a < 0) != (bb < 0))  # floor went below the truncated quotient
    q = q + fix
    r = r - np.where(fix, bb, np.int64(0))
    with np.errstate(over="ignore"):
        neg = np.where(a == I64_MIN, np.int64(I64_MIN), -a)  # i64::MIN / -1 wraps to i64::MIN
    return np.where(m1, neg, q), np.where(m1, np.int64(0), r)  # x % -1 = 0


# value / predicate shapes shared with the compile checks of the CPU file
def k64(k):
    return (k, "Int64")


I64_VALUE_SHAPES = {
    "x_div_mod_k": [[("/", k64(-3))], [("%", k64(-3))]],
    "k_div_mod_x": [[("/", k64(-3), True)], [("%", k64(-3), True)]],
    "wraps": [[("+", k64(I64_MAX))], [("-", k64(I64_MIN))], [("*", k64(3))]],
}
F64_CONST_OPS = [[(s, 2.5)] for s in "+-*/%"]
F64_SELF_OPS = [[("/", COL)], [("%", COL)], [("-", COL)], [("*", 0.0)]]
# a product feeding a sum: two roundings, never one fused multiply-add
F64_TWO_ROUNDINGS = [[("*", 10.0), ("-", COL)], [("*", 0.1), ("+", 1.0)], [("*", COL), ("+", COL)]]
CAST_VALUE = [("-", k64(5))]
CAST_TREE = [("-", k64(5)), PUSH, ("*", 3), ("+", STACK, True)]
# GROUP BY argument: x * 1.0 where `sel` is odd, else NaN (0 * inf -> NaN, 1 / NaN -> NaN; 1 / inf -> 0)
def nan_unless_odd(sel_steps):
    return [("*", 1.0), PUSH] + sel_steps + [("%", 2), ("*", INF), ("/", 1.0, True), ("+", STACK, True)]


# ---------------------------------------------------------------------------
# GPU helpers
# ---------------------------------------------------------------------------
def setup_module():
    global ops
    from fq_amd import ops as _ops
    _ops.require_gpu()
    _ops.jit_config(abi.JIT_AUTO, 1 << 22)
    ops = _ops


@pytest.fixture(params=["interp", "jit"])
def jit_mode(request):
    """Scans run twice: on the precompiled program-interpreting kernel and on
    the hipRTC-specialised one (row kernels are specialised only)."""
    ops.jit_config(abi.JIT_ALWAYS if request.param == "jit" else abi.JIT_OFF, 0)
    yield request.param
    ops.jit_config(abi.JIT_AUTO, 1 << 22)


def layouts(host, dtype):
    """The column 16-byte aligned, and as an 8-byte-offset view (one head row)."""
    aligned = ops.from_numpy(host, dtype)
    base = ops.from_numpy(np.concatenate([np.zeros(1, host.dtype), host]), dtype)
    return [("aligned", aligned), ("offset8", ops.DeviceColumn(base.buf, host.shape[0], dtype, offset=8))]


def bitmap_pred(keep):
    bm = ops.compare("=", ops.from_numpy(keep.astype(np.uint64)), 1)
    p = abi.fq_pred()
    p.kind = abi.PRED_BITMAP
    p.bitmap = bm.ptr
    p._bm = bm  # keep the device bitmap alive with the predicate
    return p


def oracle_states(host, dtype, block_rows, value, pred, keep, ops_):
    """The oracle's partial states [(kind, dtype, bits)] or its error.  A
    bitmap predicate (which the oracle's C ABI does not take) is the oracle's
    own per-block aggregate over each block's kept rows, merged by its
    AggregatorFunction::merge_state restatement."""
    aggs = [(op, value) for op in ops_]
    try:
        if keep is None:
            return [as_tuple(s) for s in oracle_c.column_partial(host, dtype, block_rows, aggs, pred)], None
        per = []
        for s in block_starts(len(host), block_rows):
            k = keep[s:s + (block_rows if block_rows > 0 else len(host))]
            assert k.any(), "keep_mask leaves no block empty"
            per.append(oracle_c.column_partial(np.ascontiguousarray(host[s:s + len(k)][k]), dtype, 0, aggs))
        return [tuple(oracle_c.merge_states(op, [p[a] for p in per])) for a, op in enumerate(ops_)], None
    except oracle_c.OracleError as e:
        return None, e


def check_against_oracle(host, dtype, block_rows, pred=None, value=None, gpu_col=None, mask=ALL, keep=None):
    """tests/test_kernels_gpu.py's check with the Float64 rules of this file:
    integers and Float64 max/min by bits, Float64 sums by class or bound."""
    col = gpu_col if gpu_col is not None else ops.from_numpy(host, dtype)
    ops_ = [op for op in AGGS if mask & op]
    exp, exp_err = oracle_states(host, dtype, block_rows, value, pred, keep, ops_)
    st = ops.aggregate(col, block_rows, bitmap_pred(keep) if keep is not None else pred, value, mask)
    if exp_err is not None:
        with pytest.raises(oracle_c.OracleError) as ei:
            for op in ops_:
                replay(op, st)
        assert str(ei.value) == str(exp_err)
        return st
    got = [replay(op, st) for op in ops_]
    print("device", got, "oracle", exp)
    for op, g, e in zip(ops_, got, exp):
        if op == abi.AGG_SUM and st.dtype == F64 and e[0] == oracle_c.FQO_SOME:
            assert g[:2] == e[:2]
            gv, ev = f64_of(g[2]), f64_of(e[2])
            if np.isnan(ev):
                assert np.isnan(gv), (gv, ev)
            elif np.isinf(ev):
                assert gv == ev, (gv, ev)
            else:
                assert value is None, "bound below is over the column's own values"
                kept = host if keep is None else host[keep]
                bound = 1e-12 * float(np.abs(kept[np.isfinite(kept)]).sum())
                print("f64 sum error", abs(gv - ev), "bound", bound)
                assert abs(gv - ev) <= bound, (gv, ev, bound)
        else:
            assert g == e, (op, g, e, ops.state_values(st))
    return st


def rows_of(host, dtype, pred, values, block_rows=8192):
    """fq_filter_project and fq_filter_project_blocks over `host`: per output
    the kept rows in order (both kernels must agree on them), and the count."""
    col = ops.from_numpy(host, dtype)
    outs = ops.filter_project(col, pred, values)
    flat = [o.to_numpy() for o in outs]
    bouts, counts = ops.filter_project_blocks(col, block_rows, pred, values)
    for o, f in zip(bouts, flat):
        h = o.to_numpy()
        blk = np.concatenate([h[b * block_rows: b * block_rows + int(c)] for b, c in enumerate(counts)])
        assert blk.view(np.uint64).tolist() == f.view(np.uint64).tolist(), "row kernels disagree"
    return flat


def assert_rows(got, exp):
    """Bits equal; where the reference is NaN any NaN is accepted."""
    exp = np.asarray(exp)
    assert got.shape == exp.shape, (got.shape, exp.shape)
    if exp.dtype == np.float64:
        nan = np.isnan(exp)
        assert np.isnan(got[nan]).all()
        bad = np.flatnonzero(bits(got)[~nan] != bits(exp)[~nan])
        assert len(bad) == 0, (got[~nan][bad[:5]], exp[~nan][bad[:5]])
    else:
        assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:5]


def pred_entry_points(host, dtype, pred, keep):
    """One predicate through fq_predicate_bitmap, fq_aggregate (interpreted and
    specialised: the count and the kept rows' max/min) and both row kernels,
    against numpy's mask.  (A kept Float64 row is never NaN; max/min compare
    as values, so a +-0.0 tie may take either sign.)"""
    col = ops.from_numpy(host, dtype)
    assert np.array_equal(ops.predicate_bitmap(col, pred).to_numpy(), keep)
    try:
        for mode in (abi.JIT_OFF, abi.JIT_ALWAYS):
            ops.jit_config(mode, 0)
            v = ops.state_values(ops.aggregate(col, 0, pred, None, EXT))
            assert v["count"] == int(keep.sum())
            if keep.any():
                k = host[keep]
                assert [v["max"], v["min"]] == [k.max().item(), k.min().item()]
    finally:
        ops.jit_config(abi.JIT_AUTO, 1 << 22)
    got, = rows_of(host, dtype, pred, [None])
    assert got.view(np.uint64).tolist() == host[keep].view(np.uint64).tolist()


# ---------------------------------------------------------------------------
# 1. aggregate against the oracle
# ---------------------------------------------------------------------------
I64_PRED = ([], ">", k64(-1))  # across the sign boundary


@pytest.mark.parametrize("mode", ["identity", "pred", "block"])
@pytest.mark.parametrize("case", list(PLACES) + ["all", "zero_free"])
def test_i64_aggregate_matches_oracle(case, mode, jit_mode):
    n = NB if mode == "block" else N0
    host = i64_column(n, places=PLACES if case in ("all", "zero_free") else (case,), zero_free=case == "zero_free")
    pred = None if mode == "identity" else predicate(I64, *I64_PRED)
    for _, col in layouts(host, I64):
        for br in ((10000, 64) if mode == "block" else (10000,)):
            st = check_against_oracle(host, I64, br, pred=pred, gpu_col=col)
            assert st.flags == 0
    if mode == "identity" and case != "zero_free":
        assert ops.state_values(st)["max"] == I64_MAX and ops.state_values(st)["min"] == I64_MIN


F64_AGG_CASES = [  # variant, infs, extremes
    ("nan_safe", "both", False), ("nan_safe", "pos", False), ("nan_safe", "none", False), ("nan_safe", "none", True),
    ("no_nan", "both", False), ("no_nan", "neg", False), ("no_nan", "none", False), ("no_nan", "none", True),
    ("all_nan", "none", False),
]


# block mode is the filtered-SUM path; the DBL_MAX columns are scanned without SUM
F64_AGG_PARAMS = [c + (m,) for c in F64_AGG_CASES for m in ("identity", "pred", "block") if not (c[2] and m == "block")]


@pytest.mark.parametrize("variant,infs,extremes,mode", F64_AGG_PARAMS, ids=["-".join(map(str, c)) for c in F64_AGG_PARAMS])
def test_f64_aggregate_matches_oracle(variant, infs, extremes, mode, jit_mode):
    """Float64 max/min by bits, sums by class or bound.  `pred` is a bitmap
    (a comparison on the column itself never keeps a NaN row).  all_nan fails
    before the NaN-aware accumulators: the device returned -inf / +inf."""
    n = NB if mode == "block" else N0
    sizes = (10000, 64) if mode == "block" else (10000,)
    keep = None if mode == "identity" else keep_mask(n, sizes)
    host = f64_column(variant, n, sizes, keep, infs, extremes)
    for _, col in layouts(host, F64):
        for br in sizes:
            st = check_against_oracle(host, F64, br, gpu_col=col, mask=EXT if extremes else ALL, keep=keep)
            assert st.flags == 0 and st.count == (n if keep is None else int(keep.sum()))
            if variant == "all_nan":
                assert np.isnan(f64_of(st.max)) and np.isnan(f64_of(st.min))


@pytest.mark.parametrize("dtype", ["i64", "f64"])
def test_aggregate_every_workgroup_holds_a_tile(dtype, jit_mode):
    if dtype == "i64":
        host = i64_column(NBIG)
        check_against_oracle(host, I64, 10000)
        check_against_oracle(host, I64, 10000, pred=predicate(I64, *I64_PRED), mask=EXT)
    else:
        keep = keep_mask(NBIG, (10000,))
        host = f64_column("nan_safe", NBIG, (10000,), keep, "none")
        check_against_oracle(host, F64, 10000, keep=keep)
        check_against_oracle(f64_column("nan_safe", NBIG, (10000,), None, "none"), F64, 10000)


# ---------------------------------------------------------------------------
# 2. the deviation from arrow's fold, pinned
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("blocks", ["one_block", "three_blocks"])
def test_f64_minmax_deviation_from_arrow_fold_is_pinned(blocks, jit_mode):
    """A reference block whose first kept row is NaN, followed by other rows:
    arrow 2.0's min_max_helper yields NaN for that block (and so loses its
    rows); the device ignores the NaN."""
    n = N0 if blocks == "one_block" else NB
    host = f64_column("nan_first_mixed", n, (10000,))
    mx, mn = [f64_of(s.bits) for s in oracle_c.column_partial(host, F64, 10000, [(abi.AGG_MAX, None),
                                                                                  (abi.AGG_MIN, None)])]
    if blocks == "one_block":
        assert np.isnan(mx) and np.isnan(mn)
    else:  # the first block's state is NaN, which the merge ignores
        assert (mx, mn) == (host[10000:].max(), host[10000:].min())
    fmx, fmn = contract_minmax(host)
    assert (fmx, fmn) == (1e6, -1e6)
    for _, col in layouts(host, F64):
        for value in (None, chain(F64, [("*", 1.0)])[0]):  # the chain makes it a specialised / interpreted scan
            st = ops.aggregate(col, 10000, None, value, EXT)
            assert [st.max, st.min, st.count] == bits([fmx, fmn]).tolist() + [n]


@pytest.mark.parametrize("variant", ["zeros_max", "zeros_min"])
def test_f64_zero_extreme_either_sign(variant, jit_mode):
    host = f64_column(variant)
    for _, col in layouts(host, F64):
        for value in (None, chain(F64, [("*", 1.0)])[0]):
            v = ops.state_values(ops.aggregate(col, 10000, None, value, EXT))
            assert v["max" if variant == "zeros_max" else "min"] == 0.0  # +0.0 or -0.0


# ---------------------------------------------------------------------------
# 3. i64 value expressions
# ---------------------------------------------------------------------------
def _i64_ref(steps, x):
    sym, (k, _) = steps[0][0], steps[0][1]
    rev = len(steps[0]) > 2
    kk = np.full(len(x), k, dtype=np.int64)
    a, b = (kk, x) if rev else (x, kk)
    if sym in "/%":
        q, r = trunc_div_i64(a, b)
        return q if sym == "/" else r
    with np.errstate(over="ignore"):  # int64 arithmetic wraps
        return a + b if sym == "+" else a - b if sym == "-" else a * b


@pytest.mark.parametrize("group", ["x_div_mod_k", "k_div_mod_x", "wraps"])
def test_i64_value_expressions(group, jit_mode):
    """x / k, x % k, k / x, k % x at the signed edges, and the wrapping + - *:
    fq_aggregate against the oracle (interpreted and specialised), rows of
    both row kernels against truncating numpy."""
    x = i64_column(N0, zero_free=group == "k_div_mod_x")
    xr = i64_column(NB, zero_free=group == "k_div_mod_x")
    if group == "wraps":
        cases = [I64_VALUE_SHAPES[group]]
    else:
        tail = (True,) if group == "k_div_mod_x" else ()
        cases = [[[("/", k64(k)) + tail], [("%", k64(k)) + tail]] for k in I64_K]
    for steps_list in cases:
        for steps in steps_list:
            st = check_against_oracle(x, I64, 10000, value=chain(I64, steps)[0])
            assert st.flags == 0 and st.dtype == I64
        if jit_mode == "jit":  # the row kernels are specialised only: once
            outs = rows_of(xr, I64, None, [chain(I64, s)[0] for s in steps_list])
            for got, steps in zip(outs, steps_list):
                assert_rows(got.view(np.int64), _i64_ref(steps, xr))


def test_i64_division_by_a_zero_row_is_an_error(jit_mode):
    x = i64_column(N0)
    assert (x == 0).sum() == 4
    v = chain(I64, [("/", k64(7), True)])[0]
    st = check_against_oracle(x, I64, 10000, value=v)
    assert st.flags & abi.STATE_DIV_ZERO
    if jit_mode == "jit":
        col = ops.from_numpy(x, I64)
        for call in (lambda: ops.filter_project(col, None, [v]), lambda: ops.filter_project_blocks(col, 8192, None, [v])):
            with pytest.raises(ops.FQError) as ei:
                call()
            assert str(ei.value) == DIV_ZERO and ei.value.status == abi.FQ_E_DIVIDE_BY_ZERO


# ---------------------------------------------------------------------------
# 4. i64 predicates
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cmp", CMPS)
@pytest.mark.parametrize("form", ["const", "flipped", "column_rhs"])
def test_i64_predicates_across_the_sign_boundary(form, cmp):
    """All five comparisons as signed: against i64::MIN, -1, 0, 1, i64::MAX in
    both orientations, and with the column on the right (x + (-1) cmp x,
    which wraps at i64::MIN)."""
    x = i64_column(N0)
    if form == "column_rhs":
        with np.errstate(over="ignore"):
            keep = NP_CMP[cmp](x + np.int64(-1), x)
        pred_entry_points(x, I64, predicate(I64, [("+", k64(-1))], cmp, COL), keep)
        return
    for k in I64_CMP_K:
        kv = np.int64(k)
        keep = NP_CMP[cmp](kv, x) if form == "flipped" else NP_CMP[cmp](x, kv)
        pred_entry_points(x, I64, predicate(I64, [], cmp, k64(k), flipped=form == "flipped"), keep)


# ---------------------------------------------------------------------------
# 5. f64 predicates with non-finite rows
# ---------------------------------------------------------------------------
def _f64_pred_column():
    x = f64_column("nan_safe", N0, infs="both", extremes=True)
    x[place_index(N0, "tile") + 20] = 1.5
    x[0] = NAN  # a NaN on row 0 too: no oracle fold is involved here
    return x


@pytest.mark.parametrize("cmp", CMPS)
def test_f64_predicates_with_non_finite_rows(cmp):
    x = _f64_pred_column()
    with np.errstate(invalid="ignore"):
        for k in F64_CMP_K:
            pred_entry_points(x, F64, predicate(F64, [], cmp, float(k)), NP_CMP[cmp](x, k))


@pytest.mark.parametrize("cmp", ["=", "<"])
def test_f64_predicate_column_on_the_right(cmp):
    """x = x keeps every row but the NaNs; x < x keeps none."""
    x = _f64_pred_column()
    with np.errstate(invalid="ignore"):
        keep = NP_CMP[cmp](x, x)
    assert keep.sum() == (0 if cmp == "<" else (~np.isnan(x)).sum())
    pred_entry_points(x, F64, predicate(F64, [], cmp, COL), keep)


def test_f64_predicate_tree_keeps_no_nan_row():
    x = _f64_pred_column()
    leaves = [([], "<", -0.0), ([], ">=", 1.5), ([], "<=", INF)]
    with np.errstate(invalid="ignore"):
        keep = ((x < -0.0) | (x >= 1.5)) & (x <= INF)
    assert not keep[np.isnan(x)].any() and keep.sum() > 0
    pred_entry_points(x, F64, pred_tree(F64, leaves, [0, 1, "or", 2, "and"]), keep)
    # a NaN row is kept by no leaf, yet a scan without a predicate counts it
    for mode in (abi.JIT_OFF, abi.JIT_ALWAYS):
        ops.jit_config(mode, 0)
        st = ops.aggregate(ops.from_numpy(x), 10000, None, chain(F64, [("+", 0.0)])[0], EXT)
        assert st.count == N0
    ops.jit_config(abi.JIT_AUTO, 1 << 22)


# ---------------------------------------------------------------------------
# 6. f64 value expressions per row
# ---------------------------------------------------------------------------
NP_F64 = {"+": np.add, "-": np.subtract, "*": np.multiply, "/": np.divide, "%": np.fmod}


def _f64_value_column(zero_free=False):
    x = f64_column("nan_safe", N0, infs="both", extremes=True)
    if zero_free:
        x[x == 0.0] = 3.25
    return x


@pytest.mark.parametrize("c", [2.5, INF, -INF, NAN], ids=["2.5", "inf", "-inf", "nan"])
def test_f64_arithmetic_with_non_finite_operands(c):
    """+ - * / % with a finite constant, +-inf and NaN over NaN / inf / +-0 /
    DBL_MAX / subnormal rows; a NaN divisor never raises."""
    x = _f64_value_column()
    outs = rows_of(x, F64, None, [chain(F64, [(s, float(c))])[0] for s in "+-*/%"])
    with np.errstate(all="ignore"):
        for got, s in zip(outs, "+-*/%"):
            assert_rows(got, NP_F64[s](x, np.float64(c)))


def test_f64_column_operand_expressions():
    x = _f64_value_column(zero_free=True)
    outs = rows_of(x, F64, None, [chain(F64, s)[0] for s in F64_SELF_OPS])
    with np.errstate(all="ignore"):
        for got, exp in zip(outs, [x / x, np.fmod(x, x), x - x, x * 0.0]):
            assert_rows(got, exp)


def test_f64_product_then_sum_rounds_twice():
    """x * 10.0 - x and its kin, per row: each step rounds as the reference's
    separate arrow kernels do.  (Generated code compiled with floating-point
    contraction fused them into one fma: 1e308 * 10.0 - inf gave -inf where
    inf - inf is NaN, and finite rows differed in the last bit.)"""
    x = _f64_value_column()
    outs = rows_of(x, F64, None, [chain(F64, s)[0] for s in F64_TWO_ROUNDINGS])
    with np.errstate(all="ignore"):
        exp = [x * 10.0 - x, x * 0.1 + 1.0, x * x + x]
        fused = np.abs((x * 10.0 - x) - 9.0 * x) > 0  # rows where one rounding and two differ
    assert fused[np.isfinite(x)].sum() > 100  # the column tells the two apart
    for got, e in zip(outs, exp):
        assert_rows(got, e)


def _raises_div_zero(call):
    with pytest.raises(ops.FQError) as ei:
        call()
    assert str(ei.value) == DIV_ZERO and ei.value.status == abi.FQ_E_DIVIDE_BY_ZERO


INV = [("/", 1.0, True)]  # 1.0 / x


@pytest.mark.parametrize("sym", ["/", "%"])
def test_f64_zero_constant_divisor_raises_for_kept_rows_only(sym):
    """A divisor of 0.0 or -0.0 raises "Divide by zero error" (the check is
    == 0.0) when a kept row reaches it, and not when no row is kept."""
    x = _f64_value_column()
    col = ops.from_numpy(x)
    nothing = predicate(F64, [], ">", INF)
    for z in (0.0, -0.0):
        v = chain(F64, [(sym, z)])[0]
        _raises_div_zero(lambda: ops.filter_project(col, None, [v]))
        _raises_div_zero(lambda: ops.filter_project_blocks(col, 8192, None, [v]))
        got, = rows_of(x, F64, nothing, [v])
        assert len(got) == 0


def test_f64_zero_column_divisor_in_a_value():
    """1.0 / x: kept +0.0 or -0.0 rows raise; dropped ones and NaN rows do not."""
    x = _f64_value_column()
    assert (bits(x) == bits(-0.0)).any() and (bits(x) == bits(0.0)).any()
    inv = chain(F64, INV)[0]
    _raises_div_zero(lambda: ops.filter_project(ops.from_numpy(x), None, [inv]))
    xm = x.copy()
    xm[bits(xm) == bits(0.0)] = 1.0  # -0.0 the only zero divisor left
    _raises_div_zero(lambda: ops.filter_project(ops.from_numpy(xm), None, [inv]))
    _raises_div_zero(lambda: ops.filter_project_blocks(ops.from_numpy(xm), 8192, None, [inv]))
    xz = _f64_value_column(zero_free=True)
    assert np.isnan(xz).any()
    with np.errstate(all="ignore"):
        got, = rows_of(xz, F64, None, [inv])
        assert_rows(got, 1.0 / xz)


def test_f64_zero_column_divisor_dropped_by_the_predicate():
    x = _f64_value_column()
    with np.errstate(all="ignore"):
        got, = rows_of(x, F64, predicate(F64, [], ">", 0.0), [chain(F64, INV)[0]])
        assert_rows(got, 1.0 / x[x > 0.0])


def test_f64_zero_divisor_inside_a_predicate_reaches_every_row():
    x = _f64_value_column()
    col = ops.from_numpy(x)
    pdiv = predicate(F64, INV, ">", 0.5)
    _raises_div_zero(lambda: ops.filter_project(col, pdiv, [None]))
    _raises_div_zero(lambda: ops.filter_project_blocks(col, 8192, pdiv, [None]))
    _raises_div_zero(lambda: ops.predicate_bitmap(col, pdiv))
    xz = _f64_value_column(zero_free=True)  # NaN divisors, none that is zero: no error
    with np.errstate(all="ignore"):
        assert np.array_equal(ops.predicate_bitmap(ops.from_numpy(xz), pdiv).to_numpy(), 1.0 / xz > 0.5)


# ---------------------------------------------------------------------------
# 7. u64 -> f64 and the u64 -> i64 cast
# ---------------------------------------------------------------------------
def test_u64_to_f64_rounds_like_numpy_per_row():
    x = u64_full_range()
    outs = rows_of(x, U64, None, [chain(U64, [("*", 1.0)])[0], chain(U64, [("/", 2.0)])[0]])
    assert_rows(outs[0], x.astype(np.float64) * 1.0)
    assert_rows(outs[1], x.astype(np.float64) / 2.0)


def _raises_cast_null(call):
    with pytest.raises(ops.FQError) as ei:
        call()
    assert ei.value.status == abi.FQ_E_UNSUPPORTED and str(ei.value).startswith("cast produced nulls"), str(ei.value)


@pytest.mark.parametrize("place", PLACES)
def test_u64_to_i64_cast_null_scan(place, jit_mode):
    """A single 2^63 coerced to Int64 (value chain, value tree, predicate):
    the oracle's "cast produced nulls" through the state's flag."""
    x = u64_cast_null_column(place)
    shapes = [(None, CAST_VALUE), (predicate(U64, CAST_VALUE, "<", 0), None)]
    if jit_mode == "jit":
        shapes.append((None, CAST_TREE))  # trees run on the specialised kernels only
    drop = predicate(U64, [], "<", 2**63)
    for _, col in layouts(x, U64):
        for pred, steps in shapes:
            st = check_against_oracle(x, U64, 10000, pred=pred, value=chain(U64, steps)[0] if steps else None,
                                      gpu_col=col)
            assert st.flags & abi.STATE_CAST_NULL
        # the row dropped by a predicate that casts nothing: the value's cast never sees it
        st = check_against_oracle(x, U64, 10000, pred=drop, value=chain(U64, CAST_VALUE)[0], gpu_col=col)
        assert st.flags == 0 and st.count == N0 - 1


def _cast_shapes():
    value, tree = chain(U64, CAST_VALUE)[0], chain(U64, CAST_TREE)[0]
    cast_pred = predicate(U64, CAST_VALUE, "<", 0)
    return {"value": (None, [value]), "tree": (None, [tree]), "pred": (cast_pred, [None]),
            "pred_and_value": (cast_pred, [value]), "dropped": (predicate(U64, [], "<", 2**63), [value])}


@pytest.mark.parametrize("shape", ["value", "tree", "pred", "pred_and_value", "dropped"])
def test_u64_to_i64_cast_null_row_kernels(shape):
    """The 2^63 at each of the four places: FQ_E_UNSUPPORTED "cast produced
    nulls" from both row kernels and fq_predicate_bitmap; no error when a
    predicate that casts nothing drops the row and only the value casts."""
    pred, values = _cast_shapes()[shape]
    for place in PLACES:
        x = u64_cast_null_column(place)
        col = ops.from_numpy(x)
        if shape == "dropped":
            got, = rows_of(x, U64, pred, values)
            assert_rows(got.view(np.int64), x[x < np.uint64(2**63)].astype(np.int64) - 5)
            continue
        _raises_cast_null(lambda: ops.filter_project(col, pred, values))
        _raises_cast_null(lambda: ops.filter_project_blocks(col, 8192, pred, values))
        if pred is not None:
            _raises_cast_null(lambda: ops.predicate_bitmap(col, pred))


@pytest.mark.parametrize("shape", ["value", "pred_and_value", "dropped"])
def test_u64_to_i64_cast_null_group_table(shape):
    pred, values = _cast_shapes()[shape]
    key = chain(U64, [("%", 100)])[0]
    for place in PLACES:
        t = ops.GroupTable(1 << 10, [(abi.AGG_COUNT, U64), (abi.AGG_MAX, I64)])
        t.aggregate(ops.from_numpy(u64_cast_null_column(place)), pred, key, [None, values[0]])
        if shape == "dropped":
            assert t.count() == 100
        else:
            _raises_cast_null(t.count)


# ---------------------------------------------------------------------------
# 8. interpreter against the specialised scan on the edge shapes
# ---------------------------------------------------------------------------
def _parity_shape(name):
    """-> host, dtype, block_rows, bitmap rows, predicate, value steps, mask"""
    if name == "item1_f64_nan_safe_block_sum":
        keep = keep_mask(NB, (64,))
        return f64_column("nan_safe", NB, (64,), keep, "none"), F64, 64, keep, None, None, ALL
    if name == "item1_f64_all_nan_bitmap":
        keep = keep_mask(N0, (10000,))
        return f64_column("all_nan", N0, (10000,), keep), F64, 10000, keep, None, None, ALL
    return {
        "item3_i64_div_minus_1": (i64_column(), I64, 10000, None, None, [("/", k64(-1))], ALL),
        "item3_i64_k_mod_x": (i64_column(zero_free=True), I64, 10000, None, None, [("%", k64(I64_MIN), True)], ALL),
        "item5_f64_pred_ge_minus_zero": (_f64_pred_column(), F64, 10000, None, ([], ">=", -0.0), None, EXT),
        "item6_f64_mod_inf": (_f64_value_column(), F64, 10000, None, None, [("%", INF)], EXT),
        "item6_f64_x_minus_x": (_f64_value_column(), F64, 10000, None, ([], "=", COL), [("-", COL)], ALL),
        "item6_f64_product_then_sum": (f64_column("no_nan", infs="none"), F64, 10000, None, None,
                                       [("*", 10.0), ("-", COL)], ALL),
    }[name]


@pytest.mark.parametrize("shape", ["item1_f64_nan_safe_block_sum", "item1_f64_all_nan_bitmap", "item3_i64_div_minus_1",
                                   "item3_i64_k_mod_x", "item5_f64_pred_ge_minus_zero", "item6_f64_mod_inf",
                                   "item6_f64_x_minus_x", "item6_f64_product_then_sum"])
def test_edge_shapes_bit_identical_interpreter_and_specialised(shape):
    """Same grid, same per-lane order: the fq_agg_state bytes must match (the
    per-row checks above run the specialised kernels only)."""
    host, dt, br, keep, pred, steps, mask = _parity_shape(shape)
    col = ops.from_numpy(host, dt)
    p = bitmap_pred(keep) if keep is not None else (predicate(dt, *pred) if pred else None)
    v = chain(dt, steps)[0] if steps else None
    try:
        ops.jit_config(abi.JIT_ALWAYS, 0)
        before = ops.jit_stats()["jit_launches"]
        got = bytes(ops.aggregate(col, br, p, v, mask))
        assert ops.jit_stats()["jit_launches"] == before + 1
        ops.jit_config(abi.JIT_OFF)
        exp = bytes(ops.aggregate(col, br, p, v, mask))
    finally:
        ops.jit_config(abi.JIT_AUTO, 1 << 22)
    assert got == exp


# ---------------------------------------------------------------------------
# 9. GROUP BY f64 MAX / MIN under the contract
# ---------------------------------------------------------------------------
NG = 200_003
G_AGGS = [(abi.AGG_COUNT, U64), (abi.AGG_MAX, F64), (abi.AGG_MIN, F64)]


def group_nan_column(kind, n=NG, seed=9):
    """A UInt64 column whose key and Float64 argument are both expressions of
    it: -> (x, key steps, argument steps, keys, values).  The argument is
    x * 1.0 where a selector derived from x is odd, else NaN.  Key 7's rows are
    all NaN, keys 8..40 have some NaN rows, the rest none."""
    rng = np.random.default_rng(seed)
    if kind == "mod1000":  # x = 1000 * q + key, selector q
        key = rng.integers(0, 1000, size=n).astype(np.uint64)
        odd = np.ones(n, bool)
        odd[key == 7] = False
        some = (key >= 8) & (key <= 40)
        odd[some] = rng.random(int(some.sum())) < 0.5
        q = rng.integers(0, 2**40, size=n).astype(np.uint64) * np.uint64(2) + odd.astype(np.uint64)
        x = q * np.uint64(1000) + key
        ksteps, sel, base = [("%", 1000)], [("/", 1000)], 0
    else:  # "div3": x = 3 * key + r, selector r in {0, 1, 2}
        key = rng.integers(0, 3000, size=n).astype(np.uint64) + np.uint64(10**9)
        k0 = key - np.uint64(10**9)
        odd = np.ones(n, bool)
        odd[k0 == 7] = False
        some = (k0 >= 8) & (k0 <= 40)
        odd[some] = rng.random(int(some.sum())) < 0.5
        r = np.where(odd, 1, rng.integers(0, 2, size=n) * 2).astype(np.uint64)
        x = key * np.uint64(3) + r
        ksteps, sel, base = [("/", 3)], [("%", 3)], 10**9
    v = np.where(odd, x.astype(np.float64), NAN)
    assert np.isnan(v[key == base + 7]).all() and (key == base + 7).any() and not np.isnan(v[key == base + 100]).any()
    return x, ksteps, nan_unless_odd(sel), key, v


def group_reference(key, v):
    """{key: (count, max bits, min bits)} with np.fmax / np.fmin (the existing
    helper's np.maximum propagates NaN)."""
    order = np.argsort(key, kind="stable")
    k, vs = key[order], v[order]
    uniq, start = np.unique(k, return_index=True)
    cnt = np.diff(np.append(start, len(k)))
    mx, mn = np.fmax.reduceat(vs, start), np.fmin.reduceat(vs, start)
    return {int(a): (int(c), int(b1), int(b2)) for a, c, b1, b2 in zip(uniq, cnt, bits(mx), bits(mn))}


def group_result(keys, states):
    return {int(k): (int(states[0][i]), int(states[1][i]), int(states[2][i])) for i, k in enumerate(keys)}


def _group_check(got, exp):
    assert set(got) == set(exp)
    nan_groups = 0
    for k, e in exp.items():
        g = got[k]
        if np.isnan(f64_of(e[1])):
            nan_groups += 1
            assert g[0] == e[0] and np.isnan(f64_of(g[1])) and np.isnan(f64_of(g[2])), (k, g, e)
        else:
            assert g == e, (k, g, e)
    assert nan_groups == 1


@pytest.mark.parametrize("path", ["dense_lds", "hashed_lds", "partitioned"])
def test_group_by_f64_minmax_ignores_nan_unless_all_nan(path):
    x, ksteps, vsteps, key, v = group_nan_column("div3" if path == "hashed_lds" else "mod1000")
    col = ops.from_numpy(x)
    val = chain(U64, vsteps)[0]
    t = ops.GroupTable(1 << 13, G_AGGS)
    t.aggregate(col, None, chain(U64, ksteps)[0], [None, val, val], log2_parts=3 if path == "partitioned" else 0)
    _group_check(group_result(*t.extract()), group_reference(key, v))


def test_group_table_merge_f64_minmax_with_nan_states():
    x, ksteps, vsteps, key, v = group_nan_column("mod1000")
    val, kexp = chain(U64, vsteps)[0], chain(U64, ksteps)[0]
    half = NG // 2
    tabs = []
    for lo, hi in ((0, half), (half, NG)):
        t = ops.GroupTable(1 << 13, G_AGGS)
        t.aggregate(ops.from_numpy(x[lo:hi]), None, kexp, [None, val, val])
        tabs.append(t)
    k1, s1 = tabs[1].extract()
    assert np.isnan(s1[1].view(np.float64)).any()  # key 7's state in the merged-in table is NaN
    tabs[0].merge(k1, s1)
    _group_check(group_result(*tabs[0].extract()), group_reference(key, v))
    # NaN state on either side, and on both
    t = ops.GroupTable(64, G_AGGS)
    five, nan = bits(5.0)[()], bits(NAN)[()]
    ks = np.array([1, 2, 3], np.uint64)
    ones = np.ones(3, np.uint64)
    t.merge(ks, [ones, np.array([nan, five, nan], np.uint64), np.array([nan, five, nan], np.uint64)])
    t.merge(ks, [ones, np.array([five, nan, nan], np.uint64), np.array([five, nan, nan], np.uint64)])
    got = group_result(*t.extract())
    assert got[1] == (2, int(five), int(five)) and got[2] == (2, int(five), int(five))
    assert got[3][0] == 2 and np.isnan(f64_of(got[3][1])) and np.isnan(f64_of(got[3][2]))


def test_group_by_i64_specials_and_key_minus_one():
    """MIN / MAX / SUM of an Int64 argument holding i64::MIN and i64::MAX; the
    key -1 is, as bits, the table's empty marker and has its own slot."""
    x = i64_column(NG)
    key = np.fmod(x, np.int64(7))  # truncating: the dividend's sign
    assert (key == -1).any() and key[x == I64_MIN][0] == -1
    aggs = [(abi.AGG_COUNT, U64), (abi.AGG_MIN, I64), (abi.AGG_MAX, I64), (abi.AGG_SUM, I64)]
    t = ops.GroupTable(64, aggs, key_dtype=I64)
    t.aggregate(ops.from_numpy(x, I64), None, chain(I64, [("%", k64(7))])[0], [None, None, None, None])
    keys, st = t.extract()
    got = {int(k): (int(st[0][i]), int(st[1].view(np.int64)[i]), int(st[2].view(np.int64)[i]),
                    int(st[3].view(np.int64)[i])) for i, k in enumerate(keys.view(np.int64))}
    exp = {}
    for k in np.unique(key):
        g = x[key == k]
        with np.errstate(over="ignore"):
            exp[int(k)] = (len(g), int(g.min()), int(g.max()), int(g.sum(dtype=np.int64)))
    assert got == exp
    assert got[-1][1] == I64_MIN


# ---------------------------------------------------------------------------
# 10. engine, through SQL
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [30000, 5])
def test_sql_max_min_of_all_nan_rows(n):
    """x = number * 1e308 * 10.0 - number * 1e308 * 10.0 is inf - inf = NaN on
    every row but number = 0, which the WHERE drops.  (Row number = 1 reaches
    inf only at the `* 10.0`: a multiply fused into the subtraction gives -inf
    there.)"""
    import fq_ref as R
    from fq_amd.engine import Engine
    x = "(number*1e308*10.0) - (number*1e308*10.0)"
    E = Engine()
    try:
        r = E.execute("select max(%s), min(%s), count(%s) from system.numbers_mt(%d) where number > 0" % (x, x, x, n))
    finally:
        E.close()
    N, c = R.E_field("number"), R.E_const
    half = R.E_bin("*", R.E_bin("*", N, c(1e308)), c(10.0))
    xe = R.E_bin("-", half, half)
    exp = R.aggregate_query(n, [R.E_fn("max", xe), R.E_fn("min", xe), R.E_fn("count", xe)],
                            where=R.E_bin(">", N, c(0)))
    ev = [v.value for v in exp]
    assert np.isnan(ev[0]) and np.isnan(ev[1]) and ev[2] == n - 1
    (mx, mn, cnt), = r.rows
    assert np.isnan(mx) and np.isnan(mn) and cnt == n - 1
    assert r.text_rows == [("NaN", "NaN", str(n - 1))]
