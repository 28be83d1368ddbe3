"""CPU side of tests/test_edge_values_gpu.py: the shared column builders'
preconditions, the oracle's stated Float64 max/min choice where it differs
from the device contract, fq_state_merge under that contract, and a gfx950
compile of every generated-kernel shape the GPU file uses (so the GPU run is
not the first time that source meets the compiler)."""
import struct

import numpy as np
import pytest

from fq_amd import abi, ops
from fq_amd.expr import COL, chain, predicate, pred_tree

import oracle_c
import test_edge_values_gpu as G

U64, I64, F64 = abi.DT_UINT64, abi.DT_INT64, abi.DT_FLOAT64
MAXMIN = [(abi.AGG_MAX, None), (abi.AGG_MIN, None)]
INF, NAN = G.INF, G.NAN


def f64_bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def oracle_maxmin(x, block_rows):
    return [s.bits for s in oracle_c.column_partial(np.ascontiguousarray(x, dtype=np.float64), F64, block_rows, MAXMIN)]


# ---------------------------------------------------------------------------
# 1. builder self-checks
# ---------------------------------------------------------------------------
def test_special_values_sit_at_the_four_places():
    for n in (G.N0, G.NB, G.NBIG):
        x = G.i64_column(n)
        assert x[0] == G.I64_MIN and x[n - 1] == G.I64_MIN
        tiles = (n // 2048) * 2048
        for place, lo, hi in (("first", 0, 14), ("tile", 14, 2048), ("vec_rem", tiles, n - 14), ("last", n - 14, n)):
            i = G.place_index(n, place, 14)
            assert lo <= i and i + 14 <= hi
            assert sorted(x[i:i + 14].tolist()) == sorted(G.I64_SPECIALS)
        assert n - tiles > 14 + 16 and (n - tiles) % 2 == 1  # a vector remainder and one scalar tail row
    z = G.i64_column(zero_free=True)
    assert not (z == 0).any() and (z == -1).sum() >= 4
    f = G.f64_column("nan_safe", extremes=True)
    for v in (INF, -INF, G.DBL_MAX, -G.DBL_MAX, G.SUBNORMAL):
        assert (f == v).sum() == 4
    assert (G.bits(f) == G.bits(-0.0)).sum() == 4 and np.isnan(f).sum() > 4
    assert np.abs(f[np.isfinite(f) & (np.abs(f) < 1e300)]).max() <= 1e6
    assert not np.isfinite(G.f64_column("no_nan", infs="both")).all() and not np.isnan(G.f64_column("no_nan")).any()


def test_nan_safe_never_starts_a_block_with_nan():
    for n, sizes in ((G.N0, (10000,)), (G.NB, (10000, 64)), (G.NBIG, (10000,))):
        for keep in (None, G.keep_mask(n, sizes)):
            x = G.f64_column("nan_safe", n, sizes, keep, "none")
            kept = keep if keep is not None else np.ones(n, bool)
            for br in sizes:
                first = G.first_kept_rows(kept, br)
                assert len(first) == -(-n // br) and not np.isnan(x[first]).any()
            assert np.isnan(x[kept]).sum() > n // 100


@pytest.mark.parametrize("variant,infs,extremes", G.F64_AGG_CASES, ids=["-".join(map(str, c)) for c in G.F64_AGG_CASES])
def test_contract_equals_the_oracle_where_the_issue_says_so(variant, infs, extremes):
    """np.fmax / np.fmin (the device contract) == the oracle, bit for bit, on
    every variant but nan_first_mixed and the zero extremes."""
    for n, sizes in ((G.N0, (10000,)), (G.NB, (10000, 64))):
        for keep in (None, G.keep_mask(n, sizes)):
            x = G.f64_column(variant, n, sizes, keep, infs, extremes)
            for br in sizes:
                if keep is None:
                    got = oracle_maxmin(x, br)
                    k = x
                else:
                    exp, err = G.oracle_states(x, F64, br, None, None, keep, [abi.AGG_MAX, abi.AGG_MIN])
                    assert err is None
                    got = [e[2] for e in exp]
                    k = x[keep]
                mx, mn = G.contract_minmax(k)
                if variant == "all_nan":
                    assert np.isnan(mx) and np.isnan(mn) and all(np.isnan(G.f64_of(b)) for b in got)
                else:
                    assert got == G.bits([mx, mn]).tolist()


def test_oracle_fold_from_the_first_row_is_pinned():
    """arrow 2.0's min_max_helper folds from m[0] (DESIGN.md 5 only names this
    choice): a block that starts with NaN yields NaN and loses its other rows,
    and the sign of a zero extreme depends on the order."""
    assert all(np.isnan(G.f64_of(b)) for b in oracle_maxmin([NAN, 1.0, 2.0], 10000))
    assert oracle_maxmin([NAN, 100.0, 1.0], 2) == [f64_bits(1.0), f64_bits(1.0)]  # blocks [NaN, 100] | [1]
    assert oracle_maxmin([1.0, NAN, 2.0], 10000) == [f64_bits(2.0), f64_bits(1.0)]  # a later NaN is ignored
    assert oracle_maxmin([0.0, -0.0], 10000) == [f64_bits(0.0), f64_bits(0.0)]
    assert oracle_maxmin([-0.0, 0.0], 10000) == [f64_bits(-0.0), f64_bits(-0.0)]
    # the GPU file's deviation columns: the oracle's answers there
    x = G.f64_column("nan_first_mixed", G.N0, (10000,))
    assert all(np.isnan(G.f64_of(b)) for b in oracle_maxmin(x, 10000))
    assert G.contract_minmax(x) == (1e6, -1e6)
    x = G.f64_column("nan_first_mixed", G.NB, (10000,))
    assert oracle_maxmin(x, 10000) == G.bits([x[10000:].max(), x[10000:].min()]).tolist()
    assert G.contract_minmax(x) == (1e6, -1e6) and x[10000:].max() < 1e4
    for variant, i in (("zeros_max", 0), ("zeros_min", 1)):
        x = G.f64_column(variant)
        assert G.f64_of(oracle_maxmin(x, 10000)[i]) == 0.0 and G.contract_minmax(x)[i] == 0.0


def test_truncating_division_reference():
    """The numpy reference of the per-row checks against Python integers."""
    def py(a, b):
        q = abs(a) // abs(b)
        q = q if (a < 0) == (b < 0) else -q
        r = a - q * b
        return ((q + 2**63) % 2**64) - 2**63, r
    xs = np.array(G.I64_SPECIALS + [7, -7, 9999, -10001], dtype=np.int64)
    for k in G.I64_K:
        q, r = G.trunc_div_i64(xs, np.full(len(xs), k, dtype=np.int64))
        assert [(int(a), int(b)) for a, b in zip(q, r)] == [py(int(a), k) for a in xs]
        nz = xs[xs != 0]
        q, r = G.trunc_div_i64(np.full(len(nz), k, dtype=np.int64), nz)
        assert [(int(a), int(b)) for a, b in zip(q, r)] == [py(k, int(a)) for a in nz]
    q, r = G.trunc_div_i64([G.I64_MIN, 5], [-1, -1])
    assert q.tolist() == [G.I64_MIN, -5] and r.tolist() == [0, 0]
    q, r = G.trunc_div_i64([7, -7], [-3, -3])
    assert q.tolist() == [-2, 2] and r.tolist() == [1, -1]  # the dividend's sign


def test_oracle_signed_division_edges():
    """What the issue states of the oracle: i64::MIN / -1 wraps, x % -1 = 0,
    % -3 takes the dividend's sign; -0.0 divides by zero, NaN does not."""
    x = np.array([G.I64_MIN, 7, -7], dtype=np.int64)

    def per_row(steps):
        return [np.uint64(oracle_c.column_partial(x[i:i + 1], I64, 10000, [(abi.AGG_MAX, chain(I64, steps)[0])])[0].bits)
                .astype(np.int64).item() for i in range(len(x))]
    assert per_row([("/", G.k64(-1))]) == [G.I64_MIN, -7, 7]
    assert per_row([("%", G.k64(-1))]) == [0, 0, 0]
    assert per_row([("%", G.k64(-3))]) == [-2, 1, -1]
    f = np.array([1.0, NAN, INF])
    for z in (0.0, -0.0):
        with pytest.raises(oracle_c.OracleError, match="Divide by zero"):
            oracle_c.column_partial(f, F64, 10000, [(abi.AGG_MAX, chain(F64, [("/", z)])[0])])
    s = oracle_c.column_partial(f, F64, 10000, [(abi.AGG_COUNT, chain(F64, [("/", NAN)])[0])])
    assert s[0].bits == 3
    with pytest.raises(oracle_c.OracleError, match="cast produced nulls"):
        oracle_c.column_partial(G.u64_cast_null_column("tile"), U64, 10000, [(abi.AGG_MAX, chain(U64, G.CAST_VALUE)[0])])


# ---------------------------------------------------------------------------
# 2. fq_state_merge under the contract
# ---------------------------------------------------------------------------
def state(dt, sum_, mx, mn, count, blocks=1):
    s = abi.fq_agg_state()
    enc = f64_bits if dt == F64 else (lambda v: int(v) & 0xFFFFFFFFFFFFFFFF)
    s.sum, s.max, s.min, s.count, s.blocks, s.flags, s.dtype = enc(sum_), enc(mx), enc(mn), count, blocks, 0, dt
    return s


def fvals(s):
    v = ops.state_values(s)
    return v["max"], v["min"], v["count"]


def test_state_merge_f64_ignores_a_nan_state_on_either_side():
    """Fails before the fix on the leading NaN state: `mx_b > mx_a ? mx_b :
    mx_a` kept a NaN that arrived first."""
    nan_state, five = state(F64, NAN, NAN, NAN, 3), state(F64, 10.0, 5.0, 5.0, 2)
    assert fvals(ops.state_merge([nan_state, five])) == (5.0, 5.0, 5)
    assert fvals(ops.state_merge([five, nan_state])) == (5.0, 5.0, 5)
    assert fvals(ops.state_merge([nan_state, five, state(F64, 0.0, 7.0, -7.0, 1), nan_state])) == (7.0, -7.0, 9)
    mx, mn, cnt = fvals(ops.state_merge([nan_state, nan_state]))
    assert np.isnan(mx) and np.isnan(mn) and cnt == 6  # a value, not "none"


def test_state_merge_count_zero_states_hold_no_value():
    empty = state(F64, 0.0, NAN, NAN, 0)
    five, nan_state = state(F64, 10.0, 5.0, 5.0, 2), state(F64, NAN, NAN, NAN, 3)
    for order in ([empty, five], [five, empty], [empty, five, empty]):
        assert fvals(ops.state_merge(order)) == (5.0, 5.0, 2)
    for order in ([empty, nan_state], [nan_state, empty]):
        mx, mn, cnt = fvals(ops.state_merge(order))
        assert np.isnan(mx) and np.isnan(mn) and cnt == 3
    assert ops.state_merge([empty, empty]).count == 0
    # whatever an empty state's max/min fields hold is not a value
    junk = state(F64, 0.0, INF, -INF, 0)
    assert fvals(ops.state_merge([junk, five])) == (5.0, 5.0, 2)
    assert fvals(ops.state_merge([five, junk])) == (5.0, 5.0, 2)


def test_state_merge_i64_at_the_limits():
    lo = state(I64, G.I64_MIN, G.I64_MIN, G.I64_MIN, 1)
    hi = state(I64, G.I64_MAX, G.I64_MAX, G.I64_MAX, 1)
    mid = state(I64, -1, 0, -1, 2)
    for order in ([lo, hi, mid], [mid, hi, lo], [hi, mid, lo]):
        v = ops.state_values(ops.state_merge(order))
        assert (v["max"], v["min"], v["count"], v["sum"]) == (G.I64_MAX, G.I64_MIN, 4, -2)
    v = ops.state_values(ops.state_merge([lo, lo]))
    assert (v["max"], v["min"], v["sum"]) == (G.I64_MIN, G.I64_MIN, 0)  # the sum wraps
    v = ops.state_values(ops.state_merge([state(I64, 0, 0, 0, 0), hi]))
    assert (v["max"], v["min"], v["count"]) == (G.I64_MAX, G.I64_MAX, 1)


def test_engine_data_value_merge_has_the_same_tables():
    """The engine's merge (fq_data_value_aggregate_op) on the same cases."""
    from fq_amd.functions import DataValue, data_value_aggregate_op as agg
    nan, five, none = DataValue("Float64", NAN), DataValue("Float64", 5.0), DataValue("Float64", None)
    for op in ("max", "min"):
        assert agg(op, nan, five) == five and agg(op, five, nan) == five
        r = agg(op, nan, nan)
        assert r.type == "Float64" and np.isnan(r.value)
        assert agg(op, none, five) == five and agg(op, five, none) == five
        r = agg(op, none, nan)
        assert np.isnan(r.value)
        assert agg(op, none, none) == none
    lo, hi = DataValue("Int64", G.I64_MIN), DataValue("Int64", G.I64_MAX)
    assert agg("max", lo, hi) == hi and agg("max", hi, lo) == hi
    assert agg("min", lo, hi) == lo and agg("min", hi, lo) == lo
    assert agg("sum", lo, lo) == DataValue("Int64", 0)


# ---------------------------------------------------------------------------
# 3. compile checks of the generated kernels the GPU file runs
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rtc():
    ops.jit_config(abi.JIT_AUTO, 1 << 22)
    if not ops.jit_prepare(U64, value=chain(U64, [("+", 1)])[0]) or ops.jit_stats()["available"] != 1:
        pytest.skip("hipRTC not loadable here")


def _bitmap():
    p = abi.fq_pred()
    p.kind = abi.PRED_BITMAP
    return p


def _scan_shapes():
    i64p = predicate(I64, *G.I64_PRED)
    out = [("i64_pred_flat", I64, i64p, None, G.EXT, 10000), ("i64_pred_block", I64, i64p, None, G.ALL, 64),
           ("f64_bitmap_flat", F64, _bitmap(), None, G.ALL, 0), ("f64_bitmap_block", F64, _bitmap(), None, G.ALL, 64),
           ("f64_times_one", F64, None, [("*", 1.0)], G.EXT, 10000),
           ("f64_plus_zero", F64, None, [("+", 0.0)], G.EXT, 10000),
           ("f64_mod_inf", F64, None, [("%", INF)], G.EXT, 10000),
           ("f64_x_minus_x", F64, predicate(F64, [], "=", COL), [("-", COL)], G.ALL, 10000),
           ("f64_product_then_sum", F64, None, G.F64_TWO_ROUNDINGS[0], G.ALL, 10000),
           ("i64_column_rhs", I64, predicate(I64, [("+", G.k64(-1))], "<=", COL), None, G.EXT, 0),
           ("f64_const_rhs", F64, predicate(F64, [], ">=", -0.0), None, G.EXT, 0),
           ("f64_tree", F64, pred_tree(F64, [([], "<", -0.0), ([], ">=", 1.5), ([], "<=", INF)], [0, 1, "or", 2, "and"]),
            None, G.EXT, 0),
           ("cast_value", U64, None, G.CAST_VALUE, G.ALL, 10000), ("cast_tree", U64, None, G.CAST_TREE, G.ALL, 10000),
           ("cast_pred", U64, predicate(U64, G.CAST_VALUE, "<", 0), None, G.ALL, 10000),
           ("cast_dropped", U64, predicate(U64, [], "<", 2**63), G.CAST_VALUE, G.ALL, 10000)]
    for name, lists in G.I64_VALUE_SHAPES.items():
        out += [("%s_%d" % (name, j), I64, None, steps, G.ALL, 10000) for j, steps in enumerate(lists)]
    return out


@pytest.mark.parametrize("shape", _scan_shapes(), ids=[s[0] for s in _scan_shapes()])
def test_edge_scan_shapes_compile(shape, rtc):
    _, dt, pred, steps, mask, br = shape
    assert ops.jit_prepare(dt, pred=pred, value=chain(dt, steps)[0] if steps else None, mask=mask, block_rows=br,
                           length=G.NB)


def _project_shapes():
    cast = G._cast_shapes()
    out = [("i64_" + name, I64, None, lists) for name, lists in G.I64_VALUE_SHAPES.items()]
    out += [("i64_cmp_const", I64, predicate(I64, [], "<", G.k64(-1)), [None]),
            ("i64_cmp_column_rhs", I64, predicate(I64, [("+", G.k64(-1))], ">=", COL), [None]),
            ("f64_cmp_const", F64, predicate(F64, [], "=", NAN), [None]),
            ("f64_cmp_column_rhs", F64, predicate(F64, [], "=", COL), [None]),
            ("f64_tree", F64, pred_tree(F64, [([], "<", -0.0), ([], ">=", 1.5), ([], "<=", INF)], [0, 1, "or", 2, "and"]),
             [None]),
            ("f64_const_ops", F64, None, G.F64_CONST_OPS), ("f64_self_ops", F64, None, G.F64_SELF_OPS),
            ("f64_two_roundings", F64, None, G.F64_TWO_ROUNDINGS),
            ("f64_div_const", F64, predicate(F64, [], ">", INF), [[("/", -0.0)]]),
            ("f64_inv", F64, None, [G.INV]), ("f64_inv_positive", F64, predicate(F64, [], ">", 0.0), [G.INV]),
            ("f64_inv_in_pred", F64, predicate(F64, G.INV, ">", 0.5), [None]),
            ("u64_to_f64", U64, None, [[("*", 1.0)], [("/", 2.0)]])]
    out += [("cast_" + k, U64, p, v) for k, (p, v) in cast.items()]
    return out


@pytest.mark.parametrize("shape", _project_shapes(), ids=[s[0] for s in _project_shapes()])
def test_edge_row_kernel_shapes_compile(shape, rtc):
    _, dt, pred, values = shape
    values = [v if v is None or isinstance(v, abi.fq_expr) else chain(dt, v)[0] for v in values]
    # FQ_E_HIP: compiled, then no device to launch on
    assert ops.project_compile_check(dt, pred, values) in (abi.FQ_OK, abi.FQ_E_HIP), ops.last_error()


GROUP_SHAPES = ["nan_mod1000", "nan_div3", "nan_mod1000_partitioned", "i64_key_minus_one", "cast_value",
                "cast_pred_and_value", "cast_dropped"]


@pytest.mark.parametrize("shape", GROUP_SHAPES)
def test_edge_group_by_shapes_compile(shape, rtc):
    if shape.startswith("nan_"):
        _, ksteps, vsteps, _, _ = G.group_nan_column(shape.split("_")[1])
        val = chain(U64, vsteps)[0]
        ops.group_compile_check(U64, G.G_AGGS, key=chain(U64, ksteps)[0], values=[None, val, val],
                                log2_parts=3 if shape.endswith("partitioned") else 0)
    elif shape == "i64_key_minus_one":
        aggs = [(abi.AGG_COUNT, U64), (abi.AGG_MIN, I64), (abi.AGG_MAX, I64), (abi.AGG_SUM, I64)]
        ops.group_compile_check(I64, aggs, key=chain(I64, [("%", G.k64(7))])[0], values=[None] * 4, key_dtype=I64)
    else:
        pred, values = G._cast_shapes()[shape[5:]]
        ops.group_compile_check(U64, [(abi.AGG_COUNT, U64), (abi.AGG_MAX, I64)], key=chain(U64, [("%", 100)])[0],
                                values=[None, values[0]], pred=pred)
