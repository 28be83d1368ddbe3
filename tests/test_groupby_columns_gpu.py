"""GPU: fq_group_aggregate_columns (GROUP BY over 2..4 64-bit columns of one
block) against the reference of tests/groupby_columns_cases.py: an fq_ref Block
of the columns, the predicate, the key and every argument evaluated as fq_ref
function trees, grouped on the host.

The launch shape is shrunk to GROUP_THREADS = 256 and GROUP_LDS_KB = 8, so a
tile is 1,024 rows over two columns and 512 over three and four, and an LDS
table has 512 / 256 / 64 slots for 1 / 3 / 8 aggregates.  Sizes: 0, 1, 3, one
tile and its neighbours, and two rounds of the grid (from the device's CU
count) plus half a tile and 3 rows, where every workgroup's loop takes a second
tile with the prefetch live and the tail is ragged.  Every size runs with all
columns 16-byte aligned, all offset by one element, and one column only offset.
One shape per column count repeats the sizes with GROUP_CHUNKED = 0 (the tile
map does not depend on the per-row functions) and at the default knobs.

Integer states and Float64 sums are compared bit for bit (the Float64 values are
exactly summable, which the reference asserts); Float64 max / min by DESIGN.md
section 4 (NaN = NaN, a zero of unspecified sign by value)."""
import numpy as np
import pytest

import groupby_columns_cases as G
from fq_amd import abi
from fq_amd._lib import FQError
from fq_amd.expr import chain, chain_columns, predicate, predicate_columns
from fuzz_groupby import DEFAULTS, apply_knobs, keep_words, same, small_knobs, tables_equal

pytestmark = pytest.mark.gpu

SPECS = {s.name: s for s in G.make_specs()}
ONE_PER_K = ("k2_expr", "k3_q1", "k4")
MODES = {"small": small_knobs(), "small_strided": small_knobs(GROUP_CHUNKED=0), "default": dict(DEFAULTS)}
RUNS = [("small", name) for name in SPECS] + [(m, name) for m in ("small_strided", "default") for name in ONE_PER_K]
ops = None
_REF = {}


def setup_module():
    global ops
    from fq_amd import ops as _ops
    _ops.require_gpu()
    ops = _ops


def teardown_module():
    ops.tune_reset()


@pytest.fixture(autouse=True)
def _restore_knobs():
    yield
    ops.tune_reset()


def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def expected(spec, n):
    k = (spec.name, n)
    if k not in _REF:
        _REF[k] = G.reference(spec, *G.data(spec, n))
    return _REF[k]


def device_cols(spec, host, offsets, lo=0, hi=None):
    """rows [lo, hi) of the host columns on the device, column j starting offsets[j] elements into its buffer"""
    out = []
    for h, dt, off in zip(host, spec.cdt, offsets):
        h = h[lo:hi]
        pad = np.zeros(off + len(h) + 2, h.dtype)
        pad[off:off + len(h)] = h
        c = ops.from_numpy(pad, dt)
        assert c.ptr % 16 == 0
        out.append(ops.DeviceColumn(c.buf, len(h), dt, offset=8 * off))
    return out


def launch(table, spec, host, keep, offsets, lo=0, hi=None):
    """one fq_group_aggregate_columns launch of rows [lo, hi) into `table`; what must stay alive until extract"""
    key, vals, pred = spec.device()
    cols = device_cols(spec, host, offsets, lo, hi)
    alive = [cols]
    if spec.pred_kind() == "bitmap":
        bm = ops.from_numpy(keep_words(keep[lo:hi]), abi.DT_UINT64)
        pred.bitmap = bm.ptr
        alive.append(bm)
    table.aggregate_columns(cols, pred, key, vals)
    return alive


def run(spec, n, offsets, capacity=None):
    host, keep = G.data(spec, n)
    status, exp = expected(spec, n)
    groups = len(exp.keys) if status == "ok" else 256
    t = ops.GroupTable(capacity or max(64, 2 * groups), spec.table_aggs(), abi.DT_BY_NAME[spec.key_t])
    alive = launch(t, spec, host, keep, offsets)
    out = t.extract()
    del alive
    return out


@pytest.mark.parametrize("layout", list(G.LAYOUTS))
@pytest.mark.parametrize("mode,name", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_against_reference(mode, name, layout):
    spec, knobs = SPECS[name], MODES[mode]
    apply_knobs(ops, knobs)
    offsets = G.LAYOUTS[layout]
    for n in G.sizes(spec.K, knobs["GROUP_THREADS"], cus() * knobs["GROUP_WG_PER_CU"]):
        status, exp = expected(spec, n)
        assert status == "ok"
        if n and n <= 3 * knobs["GROUP_THREADS"]:  # every layout holds the same rows
            for c, h in zip(device_cols(spec, G.data(spec, n)[0], offsets), G.data(spec, n)[0]):
                assert np.array_equal(c.to_numpy().view(np.uint64), h.view(np.uint64))
        diff = same(run(spec, n, offsets), exp)
        assert diff is None, "%s %s %s n=%d: %s" % (mode, name, layout, n, diff)


def test_shapes_reach_what_they_are_for():
    """the key sets really are dense at d = S, hashed at S + 1, past 3/4 S where the bypass is meant, and hold the
    empty marker; the two-round size gives every workgroup a second tile"""
    knobs = small_knobs()
    kb = knobs["GROUP_LDS_KB"]
    apply_knobs(ops, knobs)
    for name, want in (("k2_dense", True), ("k2_dense1", False), ("k2_dense_nocount", True), ("k3_q1", True),
                       ("k2_expr", False), ("k2_marker", False), ("k4", False), ("k2_key1", False)):
        spec = SPECS[name]
        key = spec.device()[0]
        d = ops.group_dense_keys_columns(spec.cdt, key, spec.n_aggs) if key is not None else 0
        assert (d > 0) == want and (not want or d == spec.slots(kb)), (name, d)
    n2 = G.sizes(2, 256, cus())[-1]
    for name in ("k2_dense1", "k2_expr"):
        assert len(expected(SPECS[name], n2)[1].keys) > 3 * SPECS[name].slots(kb) // 4
    n4 = G.sizes(4, 256, cus())[-1]
    assert len(expected(SPECS["k4"], n4)[1].keys) > 3 * SPECS["k4"].slots(kb) // 4
    assert int(expected(SPECS["k2_marker"], n2)[1].keys[-1]) == G.E1
    assert len(expected(SPECS["k2_dense"], n2)[1].keys) == SPECS["k2_dense"].slots(kb)
    for K in (2, 3, 4):
        n = G.sizes(K, 256, cus())[-1]
        for chunked in (0, 1):
            tiles = G.workgroup_tiles(n, K, small_knobs(GROUP_CHUNKED=chunked), cus())
            assert min(len(w) for w in tiles) >= 2 and n % G.tile_rows(K, 256)


@pytest.mark.parametrize("kept", [False, True])
def test_zero_divisor_counts_on_kept_rows_only(kept):
    apply_knobs(ops, small_knobs())
    spec = G.zero_spec(kept)
    n = 3 * G.tile_rows(2, 256) + 5
    status, exp = expected(spec, n)
    assert status == ("err" if kept else "ok")
    if kept:
        with pytest.raises(FQError) as e:
            run(spec, n, (0, 1))
        assert e.value.status == abi.FQ_E_DIVIDE_BY_ZERO and str(e.value) == G.DIV_ZERO
    else:
        assert same(run(spec, n, (0, 1)), exp) is None


@pytest.mark.parametrize("name", ["k2_dense1", "k2_dense", "k4", "k3_q1"])
def test_blocks_and_merge_give_the_one_launch_table(name):
    """the two-round size cut into three blocks accumulated into one table (the later launches of a hashed shape
    that saturated split the keys into partitions), and two tables of its halves merged"""
    spec = SPECS[name]
    apply_knobs(ops, small_knobs())
    n = G.sizes(spec.K, 256, cus())[-1]
    host, keep = G.data(spec, n)
    status, exp = expected(spec, n)
    assert status == "ok"
    cap = max(64, 2 * len(exp.keys))
    kdt = abi.DT_BY_NAME[spec.key_t]
    one = run(spec, n, (0, 0, 0, 0), cap)
    assert same(one, exp) is None
    # three blocks: one tile (it saturates the workgroup's table when the keys outgrow it), 16 tiles, the rest
    tile = G.tile_rows(spec.K, 256)
    cuts = [0, tile + 1, 17 * tile + 1, n]
    t = ops.GroupTable(cap, spec.table_aggs(), kdt)
    alive = [launch(t, spec, host, keep, (0, 1, 0, 1), lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
    blocks = t.extract()
    assert same(blocks, exp) is None and tables_equal(blocks, one, exp) is None
    # two tables from the halves, merged
    a, b = ops.GroupTable(cap, spec.table_aggs(), kdt), ops.GroupTable(cap, spec.table_aggs(), kdt)
    alive += [launch(a, spec, host, keep, (1, 0, 0, 0), 0, n // 2), launch(b, spec, host, keep, (0, 0, 1, 0), n // 2, n)]
    k, s = b.extract()
    a.merge(k, s)
    merged = a.extract()
    del alive
    assert same(merged, exp) is None and tables_equal(merged, one, exp) is None


def test_mixed_entry_points_fill_one_table():
    """a statement that reads only column 0: fq_group_aggregate_columns over two columns gives the table
    fq_group_aggregate gives over that column alone, and launches of both calls accumulate into one table"""
    apply_knobs(ops, small_knobs())
    U = abi.DT_UINT64
    n = G.sizes(2, 256, cus())[-1]
    rng = np.random.default_rng(77)
    a = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    b = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    aggs = [(abi.AGG_COUNT, U), (abi.AGG_SUM, U), (abi.AGG_MAX, U)]
    steps, psteps = [("%", 1000)], [("%", 8)]
    k1, p1 = chain(U, steps)[0], predicate(U, psteps, "<", 3)
    k2, p2 = chain_columns([U, U], steps)[0], predicate_columns([U, U], psteps, "<", 3)
    da, db = ops.from_numpy(a, U), ops.from_numpy(b, U)
    t1 = ops.GroupTable(2048, aggs, U)
    t1.aggregate(da, p1, k1, [None, None, None])
    t2 = ops.GroupTable(2048, aggs, U)
    t2.aggregate_columns([da, db], p2, k2, [None, None, None])
    one, two = t1.extract(), t2.extract()
    o1, o2 = np.argsort(one[0]), np.argsort(two[0])
    want = np.unique((a % np.uint64(1000))[a % np.uint64(8) < 3])  # (8 divides 1000: 375 of the 1,000 keys)
    assert np.array_equal(one[0][o1], want) and np.array_equal(two[0][o2], want)
    for s1, s2 in zip(one[1], two[1]):
        assert np.array_equal(s1[o1], s2[o2])
    # half through each call into one table
    h = n // 2 + 1
    t3 = ops.GroupTable(2048, aggs, U)
    t3.aggregate(ops.DeviceColumn(da.buf, h, U), p1, k1, [None, None, None])
    t3.aggregate_columns([ops.DeviceColumn(da.buf, n - h, U, offset=8 * h), ops.DeviceColumn(db.buf, n - h, U, offset=8 * h)],
                         p2, k2, [None, None, None])
    three = t3.extract()
    o3 = np.argsort(three[0])
    assert np.array_equal(one[0][o1], three[0][o3])
    for s1, s3 in zip(one[1], three[1]):
        assert np.array_equal(s1[o1], s3[o3])


def test_one_column_call_runs_the_single_column_kernel():
    apply_knobs(ops, small_knobs())
    U = abi.DT_UINT64
    n = 5000
    a = np.random.default_rng(5).integers(0, 1 << 64, n, dtype=np.uint64)
    da = ops.from_numpy(a, U)
    aggs = [(abi.AGG_COUNT, U), (abi.AGG_SUM, U)]
    key = chain(U, [("%", 100)])[0]
    t1, t2 = ops.GroupTable(256, aggs, U), ops.GroupTable(256, aggs, U)
    t1.aggregate(da, None, key, [None, None])
    compiled = ops.jit_stats()["kernels_compiled"]
    t2.aggregate_columns([da], None, key, [None, None])
    assert ops.jit_stats()["kernels_compiled"] == compiled  # the cached single-column module
    one, two = t1.extract(), t2.extract()
    assert np.array_equal(np.sort(one[0]), np.arange(100, dtype=np.uint64))
    o1, o2 = np.argsort(one[0]), np.argsort(two[0])
    for s1, s2 in zip(one[1], two[1]):
        assert np.array_equal(s1[o1], s2[o2])
