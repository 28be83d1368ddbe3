"""Directed tests of the GROUP BY kernels' branch boundaries at the small launch
shape: FQ_TUNE_GROUP_THREADS = 256 and FQ_TUNE_GROUP_LDS_KB = 8, where a tile is
2,048 rows and an LDS table has S = 512 / 256 / 64 slots for 1 / 3 / 8
aggregates, so every boundary lies within a few thousand rows (at the defaults
tests/test_groupby_gpu.py needs millions).  Each case runs the direct launch
and at least one radix-partitioned plan; every plan's table must equal the
reference of tests/fuzz_groupby.py (fq_ref's arithmetic for the chains, numpy's
stable sort and reduceat for the groups) and the other plans', bit for bit.

The knobs are set per test and reset after each; the last test checks that."""
import numpy as np
import pytest

import fuzz_groupby as G
from fq_amd import abi

pytestmark = pytest.mark.gpu

U, I, F = G.U, G.I, G.F
CNT, SUM, MAX, MIN = abi.AGG_COUNT, abi.AGG_SUM, abi.AGG_MAX, abi.AGG_MIN
TILE = 2048
ops = None
CUS = 0


def setup_module():
    global ops, CUS
    import torch
    from fq_amd import ops as _ops
    _ops.require_gpu()
    ops = _ops
    CUS = torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(autouse=True, scope="module")
def _knobs_never_leak():
    yield
    ops.tune_reset()


def S_of(n_aggs):
    return G.lds_slots(n_aggs, 8)


def direct(cap):
    return G.Plan("direct", [("direct",)], capacity=cap)


def part(cap, lp, narrow=False):
    return G.Plan("part", [("part", lp, narrow)], capacity=cap)


def check(q, plans, **knobs):
    """every plan under the small knobs (and `knobs`) -> the first plan's table; all equal the reference"""
    status, exp = G.reference(q)
    assert status == "ok"
    G.apply_knobs(ops, G.small_knobs(**knobs))
    try:
        tables = [G.execute(ops, q, p) for p in plans]
    finally:
        ops.tune_reset()
    for p, t in zip(plans, tables):
        diff = G.same(t, exp)
        assert diff is None, (q.describe(), p, diff)
    for p, t in zip(plans[1:], tables[1:]):
        diff = G.tables_equal(tables[0], t, exp)
        assert diff is None, (q.describe(), plans[0], p, diff)
    return tables[0], exp


def int_aggs(n_aggs, with_count):
    """n_aggs integer states over the column itself, the first a COUNT or not"""
    kinds = ([CNT] if with_count else []) + [SUM, MAX, MIN, SUM, MAX, MIN, SUM, MAX]
    return [(k, U, []) for k in kinds[:n_aggs]]


def mod_key(d):
    return [("%", d, U, False)]


@pytest.mark.parametrize("with_count", [True, False], ids=["count", "nocount"])
@pytest.mark.parametrize("n_aggs", [1, 3, 8])
def test_dense_boundary(n_aggs, with_count):
    # `% d` keys index the LDS table directly when d <= S; with a COUNT state the flush rebuilds the key from the
    # slot (DENSE_CNT), without one the key is stored.  d = S is the `& (S - 1)` form
    S = S_of(n_aggs)
    x = np.random.default_rng(n_aggs).integers(0, 1 << 64, 3 * TILE + 37, dtype=np.uint64)
    for d in (S - 1, S, S + 1):
        q = G.Query(U, x, mod_key(d), int_aggs(n_aggs, with_count))
        G.apply_knobs(ops, G.small_knobs())
        try:
            assert ops.group_dense_keys(abi.DT_UINT64, q.device()[0], n_aggs) == (d if d <= S else 0)
        finally:
            ops.tune_reset()
        (keys, _), _ = check(q, [direct(4 * d), part(4 * d, 2)])
        assert len(keys) == d


@pytest.mark.parametrize("distinct", ["3S/4-1", "3S/4", "3S/4+1", "S", "2S"])
def test_saturation_of_one_workgroup(distinct):
    # one workgroup (n = one tile) whose LDS table stops claiming slots at 3S/4: shuffled, so resident and
    # non-resident keys keep arriving after the bypass flag is set (probe limit 4, the rest to HBM directly)
    S = S_of(3)
    k = {"3S/4-1": 3 * S // 4 - 1, "3S/4": 3 * S // 4, "3S/4+1": 3 * S // 4 + 1, "S": S, "2S": 2 * S}[distinct]
    rng = np.random.default_rng(k)
    pool = rng.integers(0, 1 << 64, k, dtype=np.uint64)
    x = np.concatenate([pool, pool[rng.integers(0, k, TILE - k)]])
    rng.shuffle(x)
    q = G.Query(U, x, [], [(CNT, U, []), (SUM, U, []), (MIN, U, [("/", 3, U, False)])])
    (keys, _), _ = check(q, [direct(4 * k), part(4 * k, 1)])
    assert len(keys) == len(np.unique(pool))


@pytest.mark.parametrize("chain_len", [3, 16, 17, 40])
def test_probe_limit(chain_len):
    # keys congruent modulo S whose LDS probes start at one slot (fuzz_groupby.lds_home restates the kernel's
    # slot hash): up to 16 probes find a slot in LDS, the keys past them live in the HBM table; count, sum, max
    # and min of every group are exact either way.  Interleaved with 100 other keys
    S = S_of(4)
    rng = np.random.default_rng(chain_len)
    keys = G.colliding_keys(rng, S, chain_len)
    assert len(set(G.lds_home(keys, S).tolist())) == 1 and len(set((keys % np.uint64(S)).tolist())) == 1
    pool = np.concatenate([keys, rng.integers(0, 1 << 40, 100, dtype=np.uint64)])
    x = pool[rng.integers(0, len(pool), TILE + 300)]
    x[:chain_len] = keys  # every key of the chain occurs
    q = G.Query(U, x, [], [(CNT, U, []), (SUM, U, []), (MAX, U, []), (MIN, I, [("%", 1000, U, False), ("-", 500, I, False)])])
    check(q, [direct(1024), part(1024, 3)])


@pytest.mark.parametrize("rows2", [6 * TILE, 8 * TILE + 5])
def test_key_partitions_after_a_saturated_launch(rows2):
    # launch 1: one workgroup saturates its LDS table (hdr[5]) and leaves more than 3S/4 groups in the table;
    # launches 2 and 3, several workgroups over old and new keys, then split the keys into P partitions when
    # the grid is a multiple of P (6 tiles -> 6 workgroups: P = 2; 8 tiles + 5 rows -> 9 workgroups: P = 1)
    S = S_of(1)
    rng = np.random.default_rng(rows2)
    pool = rng.integers(0, 1 << 64, 3 * S // 4 + 40, dtype=np.uint64)  # P = 2: S/2 < groups <= S
    more = rng.integers(0, 1 << 64, 60, dtype=np.uint64)
    first = np.concatenate([pool, pool[rng.integers(0, len(pool), TILE - len(pool))]])
    both = np.concatenate([pool, more])
    x = np.concatenate([first, both[rng.integers(0, len(both), 2 * rows2)]])
    q = G.Query(U, x, [], [(CNT, U, [])])
    cap = 4096
    blocks = G.Plan("blocks", [("direct",)] * 3, [TILE, TILE + rows2], cap)
    assert G.direct_geometry(rows2, 0, G.small_knobs(), CUS)[0] == -(-rows2 // TILE)
    check(q, [blocks, direct(cap), part(cap, 2), G.Plan("blocks", [("direct",), ("part", 2, False), ("direct",)],
                                                        [TILE, TILE + rows2], cap)])


@pytest.mark.parametrize("n_aggs,pool_keys,P", [(3, 450, 4), (8, 250, 8), (8, 400, 16)])
def test_key_partitions_with_value_states(n_aggs, pool_keys, P):
    # the same with count, sum, max and min states and more partitions: S = 256 / 64, so the groups the first
    # launch leaves make P = 4, 8 or 16 (the smallest P with P S/2 >= groups); 16 tiles -> a grid of 16, which
    # every P divides; the third launch (5 tiles + 3 rows, 6 workgroups) falls back to P = 1 unless P = 2
    S = S_of(n_aggs)
    rng = np.random.default_rng(pool_keys)
    pool = rng.integers(0, 1 << 64, pool_keys, dtype=np.uint64)
    assert pool_keys > 3 * S // 4 and (P // 2) * (S // 2) < pool_keys <= P * (S // 2)
    more = rng.integers(0, 1 << 64, 30, dtype=np.uint64)
    both = np.concatenate([pool, more])
    x = np.concatenate([pool, pool[rng.integers(0, pool_keys, TILE - pool_keys)],
                        both[rng.integers(0, len(both), 21 * TILE + 3)]])
    q = G.Query(U, x, [], int_aggs(n_aggs, True))
    cap = 4096
    cuts = [TILE, 17 * TILE]
    assert G.direct_geometry(16 * TILE, 0, G.small_knobs(), CUS)[0] == 16
    check(q, [G.Plan("blocks", [("direct",)] * 3, cuts, cap), direct(cap), part(cap, 3)])


def test_narrow_mod_key_over_values_that_wrap_below_a_small_first_row():
    # col[0] = 5: the narrow range col[0] - 2^31 .. col[0] + 2^31 - 1 reaches below zero, modulo 2^64.  A one-step
    # `% d` key over narrow rows with range bins is computed from the row's 32-bit offset (GP_MOD32): (2^64 - 1)
    # % 1000 is 615, not (2^32 - 1) % 1000 = 295.  The other way round: col[0] = 2^64 - 7, rows past zero
    aggs = int_aggs(3, True)
    for first, others in [(5, [2**64 - 1, 2**64 - 2**31 + 5, 2**64 - 1000, 0, 4, 2**31 + 4]),
                          (2**64 - 7, [0, 1, 999, 2**31 - 8, 2**64 - 7 - 2**31, 2**64 - 1])]:
        rng = np.random.default_rng(first % 1000)
        lo = (first - 2**31) % 2**64
        x = ((np.uint64(lo) + rng.integers(0, 1 << 32, TILE + 77, dtype=np.uint64)) & np.uint64(G.E1))
        x[0] = first
        x[1:1 + len(others)] = np.array(others, dtype=np.uint64)
        x[-1] = others[0]
        q = G.Query(U, x, mod_key(1000), aggs)
        check(q, [part(4096, 3, True), direct(4096), part(4096, 3, False)])


@pytest.mark.parametrize("run", [3, 4, 5, TILE + 1])
def test_clustered_mode_from_the_second_tile_on(run):
    # two tiles per workgroup and 37 rows: the first tile is processed lane-consecutive and votes, the rest go
    # through the LDS transpose (eight rows per lane, fq_runs / fq_wave_runs) when GROUP_CLUSTER > 0.  The
    # predicate removes rows inside runs; GROUP_CLUSTER 0 and 160 must give the same table
    n = 2 * TILE * CUS + TILE + 37
    x = np.arange(7, 7 + n, dtype=np.uint64)
    key = [("/", run, U, False), ("%", 1000, U, False)]
    aggs = [(CNT, U, []), (SUM, U, []), (MAX, F, [("*", 0.5, F, False)]), (MIN, I, [("-", 1 << 20, I, False)])]
    leaf = G.Leaf([("%", 7, U, False)], "<", 5, U)
    q = G.Query(U, x, key, aggs, "expr", [leaf], offset=1)
    a, exp = check(q, [direct(4096)], GROUP_CLUSTER=0)
    b, _ = check(q, [direct(4096), part(4096, 2)], GROUP_CLUSTER=160)
    assert G.tables_equal(a, b, exp) is None


@pytest.mark.parametrize("log2p", [1, 4, 8])
def test_range_and_hash_bins(log2p):
    # `% d` keys take range bins when 2^sh <= S for the smallest sh with 2^(log2p + sh) >= d: d = 2^log2p S does,
    # d + 1 takes hash bins.  Rows 0..2 tiles hold every key, the rest only keys of the first bin's range (the
    # other bins receive nothing from there on); one more query sends every row to one bin
    S = S_of(3)
    rng = np.random.default_rng(log2p)
    aggs = int_aggs(3, True)
    for d in ((S << log2p), (S << log2p) + 1):
        x = np.concatenate([rng.integers(0, 1 << 63, 2 * TILE, dtype=np.uint64) // np.uint64(d) * np.uint64(d)
                            + rng.integers(0, d, 2 * TILE, dtype=np.uint64),
                            np.uint64(d) * rng.integers(0, 1 << 40, TILE + 11, dtype=np.uint64)
                            + rng.integers(0, S, TILE + 11, dtype=np.uint64)])
        q = G.Query(U, x, mod_key(d), aggs)
        check(q, [part(4 * d, log2p), direct(4 * d)])
        check(q, [part(4 * d, log2p)], GROUP_RANGE_BINS=0)
    one = G.Query(U, np.uint64(S << log2p) * rng.integers(0, 1 << 30, 2 * TILE + 3, dtype=np.uint64) + np.uint64(5),
                  mod_key(S << log2p), aggs)
    check(one, [part(64, log2p), direct(64)])


def test_narrow_rows_accept_exactly_the_documented_range():
    # FQ_GROUP_NARROW_ROWS (include/fq_gpu.h): 4-byte offsets from col[0] - 2^31, so the values accepted are
    # col[0] - 2^31 .. col[0] + 2^31 - 1, both ends included; one past either end is reported
    first = 1 << 40
    n = TILE + 100
    aggs = int_aggs(3, True)
    for lo, hi, ok in [(first - 2**31, first + 2**31 - 1, True), (first - 2**31 - 1, first, False),
                       (first, first + 2**31, False)]:
        x = np.arange(first, first + n, dtype=np.uint64)
        x[n // 2], x[n - 1] = lo, hi
        q = G.Query(U, x, mod_key(1000), aggs)
        if ok:
            check(q, [part(4096, 3, True), part(4096, 3, False), direct(4096)])
            continue
        G.apply_knobs(ops, G.small_knobs())
        try:
            with pytest.raises(ops.FQError, match="narrow rows"):
                G.execute(ops, q, part(4096, 3, True))
        finally:
            ops.tune_reset()


@pytest.mark.parametrize("key", ["direct", "staged", "hash"])
def test_narrow_rows_over_an_int64_column_crossing_zero(key):
    # Int64 values -1,500 .. : the offset base col[0] - 2^31 wraps below zero.  `(x + 2000) / 3 % d` stores each
    # row straight from its registers, `* 17` stages the tile in LDS (group_stage_narrow); no `%`: hash bins
    n = 3 * TILE + 37
    x = np.arange(-1500, -1500 + n, dtype=np.int64)
    S = S_of(3)
    aggs = [(CNT, U, []), (SUM, I, []), (MIN, I, [])]
    if key == "hash":
        q = G.Query(I, x, [], aggs, offset=1)
    else:
        # range bins need a UInt64 key, so an unsigned column: from 2^64 - 1,500 on, wrapping through zero
        x = np.uint64(2**64 - 1500) + np.arange(n, dtype=np.uint64)
        first = [("/", 3, U, False)] if key == "direct" else [("*", 17, U, False)]
        assert G.stages_narrow(first + mod_key(4 * S)) == (key == "staged")
        q = G.Query(U, x, first + mod_key(4 * S), int_aggs(3, True), offset=1)
    check(q, [part(16384, 2, True), part(16384, 2, False), direct(16384)])
    check(q, [part(16384, 2, True)], GROUP_NARROW=0)


@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_tiny_lengths_through_every_plan_kind(n):
    x = np.array([5, 2**64 - 1, 5][:n], dtype=np.uint64)  # (2^64 - 1 lies 6 below 5, modulo 2^64: narrow rows hold it)
    q = G.Query(U, x, [], [(CNT, U, []), (MAX, F, [("*", 0.5, F, False)])], offset=n % 2)
    plans = [direct(64), part(64, 1), part(64, 8, True), G.Plan("blocks", [("direct",), ("part", 3, False)], [n // 2], 64),
             G.Plan("blocks", [("part", 2, False), ("direct",), ("direct",)], [0, n], 64),
             G.Plan("merge", [("direct",), ("part", 1, False)], [n // 2], 64),
             G.Plan("merge", [("part", 1, False), ("direct",)], [n], 64)]
    (keys, _), _ = check(q, plans)
    assert len(keys) == len(set(x.tolist()))


def test_group_knobs_are_back_at_their_defaults():
    assert {k: ops.tune_get(k) for k in G.DEFAULTS} == G.DEFAULTS
