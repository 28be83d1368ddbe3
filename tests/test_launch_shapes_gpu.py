"""GPU: every streaming kernel at the sizes where a workgroup (or a wave) takes
more than one unit of work -- the second and third iterations of the persistent
loops, which the tile- and vector-edge sizes of the other test files do not
reach because the grids are capped at CUs x knob (tests/launch_shapes.py has the
launch model and the named cases: one_round_minus, exact_2, ragged,
ragged_head).  The knobs that shrink a grid are set to their lowest value, so
most cases need 0.6-5 M rows; the CU count is read from the device.

Oracles are the existing ones, imported: oracle_c.column_partial and
tests/replay.py for fq_aggregate / fq_aggregate_for32, fq_ref through the
per-block oracles of tests/test_scan_typed_gpu.py (ref_scan, check),
tests/test_scan_nullable_gpu.py and tests/test_project_typed_gpu.py (Case.oracle,
same).  Integer results are bit-exact; Float64 results are sums of integer-valued
data below 2^53 (Float32 steps below 2^24), so they are exact in any order and
the grid cannot change a byte: a result must equal the oracle AND the same
call's result under the other knob values.

What runs (FLAT_RUNS, SELECT_RUNS ... below are the exact lists):
  for32         four cases x SCAN_WG_PER_CU 1, 2 x random-base-per-frame and
                span_max data x every mask of tests/test_for32_gpu.py.  The delta
                buffer must be 16-byte aligned (the ABI refuses another), so
                ragged_head offsets the plain column the encoder and fq_aggregate
                read.
  flat scans    fq_aggregate (UInt64, Float64; hipRTC kernel and interpreter, and
                the interpreter's prefetching variant under sum + count),
                fq_aggregate_columns (2 and 4 columns), fq_aggregate_typed
                (Float64 + Float32 + Int32 + UInt8: 1,024-row tiles; UInt8 + Int8:
                4,096-row tiles), fq_aggregate_nullable.  Sized for SCAN_WG_PER_CU
                1 and 2: the four cases (knob 1: with and without predicate x with
                and without value chain; knob 2: neither and both).  Sized for 16
                (a 4,096-workgroup grid, 10-40 M rows): the four cases for
                fq_aggregate over UInt64; `ragged` for Float64, two and four
                columns and the four-width typed layout (predicate and chain).
                Every input runs under SCAN_WG_PER_CU 1, 2 and 16.  Left out for
                the time fq_ref takes: at 16, the other three cases of those entry
                points (4-10 M rows each), and every case of UInt8 + Int8
                (39,147,523 rows for `ragged`, 10 s) and of fq_aggregate_nullable
                (9,786,883 rows, 8 s).
  block mode    144-row reference blocks, 2 1/3 blocks per wave of the capped grid
                (CUs x 8 x 4 waves; 2.7 M rows at 256 CUs).  Blocks without a kept
                row lie only where a wave has a later block to go: on waves' first
                blocks, or on their second blocks.  BLOCK_U 4, 8, 16, all four
                entry points; fq_aggregate also with no empty block.
  look-back     fq_filter_project, _columns (2, 3, 4 columns), _typed (the Q6
                layout, UInt8 + UInt16) at SELECT_WG_PER_CU 1: `ragged` at keep
                rates 1/1000, 1/8, 999/1000 and every row, the other cases at 1/8;
                each by comparison and by bitmap predicate.  `ragged` for
                SELECT_WG_PER_CU 16 runs for fq_filter_project_columns over four
                columns, whose 2,048-row tile is the smallest (19.6 M rows at 256
                CUs, 1/8 kept by a hashed column); the other entry points need 39 M
                (two and three columns, the Q6 layout) or 78 M rows (one column,
                UInt8 + UInt16), 13-20 s through fq_ref each, and are left out.  That
                one run is by comparison predicate only (no bitmap predicate at 16),
                and what it tests in effect is the occupancy cap: the launch takes
                CUs x min(16, occupancy) workgroups (1,280 = 256 x 5 in
                profiles/r15_launch_shapes.json), so its 9,558 tiles give every
                workgroup seven or eight tickets, not two or three.  The other
                three cases run at 1/8 only.
  block stream  fq_filter_project_blocks at SELECT_BLOCKS_WG_PER_CU 1 over
                SELECT_BLOCKS_ROWS {8, 16, 32} x SELECT_BLOCKS_STAGE {0, 1, 2, 4},
                10,000- and 8,192-row blocks, 2 1/3 blocks per workgroup and a
                short last block, outputs aligned and one element off (al == 0);
                _columns and _typed (whose tiles do not follow those two knobs)
                once per geometry.
  bitmap, map   fq_predicate_bitmap, _columns, _typed and the no-predicate path of
                fq_filter_project, _columns, _typed at 1 1/3 rounds of the
                CUs x 8 grid, pointers aligned and one element off.
  element-wise  fq_arith and fq_compare at EW_WG_PER_CU 0, 1 and 16, `ragged` for
                each grid, column-column and column-scalar, against numpy (the
                reference of tests/test_kernels_gpu.py for these two).

fq_filter_compact has no capped grid: compact_count_kernel runs one workgroup
per group of 16 tiles (262,144 rows) and the scatter kernels one per tile, so a
"second tile of a group" is any length above 16,384 rows and "many groups" any
above 262,144 -- tests/test_kernels_gpu.py runs 3 x 16,384 + 77, 1,000,003 and
16,384 x 9,001 + 77 rows (test_filter_compaction_large_ragged, _vector_path_edges,
_many_tiles).  The only loop left is compact_scan_kernel's second round of 1,024
x 16 group totals, reached above 16,384 groups = 4,294,967,296 rows (32 GiB of
u64): left out.  Likewise for32_encode_kernel's frame stride needs more than
CUs x 8 frames, 134 M rows (1 GiB) at 256 CUs: left out.

With FQ_LAUNCH_SHAPES_LOG=<file> every call's kernel, rows, model units and
model grid are appended to that file (profiles/r15_launch_shapes.json holds
them beside the grids a kernel trace saw)."""
import functools
import json
import os

import numpy as np
import pytest

import fq_ref as R
import launch_shapes as LS
import oracle_c
import test_for32_gpu as TF
import test_project_typed_gpu as TP
import test_scan_nullable_gpu as TN
import test_scan_typed_gpu as TA
from fq_amd import abi
from fq_amd.expr import Col, chain, chain_columns, load, predicate, predicate_columns
from replay import as_tuple, replay

pytestmark = pytest.mark.gpu

ALL = abi.AGG_SUM | abi.AGG_MAX | abi.AGG_MIN | abi.AGG_COUNT
AGGS = [abi.AGG_SUM, abi.AGG_MAX, abi.AGG_MIN, abi.AGG_COUNT]
I8, I32, I64 = abi.DT_INT8, abi.DT_INT32, abi.DT_INT64
U8, U16, U64 = abi.DT_UINT8, abi.DT_UINT16, abi.DT_UINT64
F32, F64 = abi.DT_FLOAT32, abi.DT_FLOAT64
NP = TA.NP
WIDTH = {dt: np.dtype(t).itemsize for dt, t in NP.items()}
K38 = 3 << 61  # keeps 3/8 of uniformly random u64 rows
ops = None
CUS = 0
_LOG = os.environ.get("FQ_LAUNCH_SHAPES_LOG")


def setup_module():
    global ops, CUS
    import torch
    for m in (TF, TA, TN, TP):
        m.setup_module()
    ops = TA.ops
    CUS = torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(autouse=True)
def _knobs_and_jit_policy_restored():
    st = ops.jit_stats()
    saved = {k: ops.tune_get(k) for k in LS.DEFAULT_KNOBS}
    try:
        yield
    finally:
        ops.tune_reset()
        for k, v in saved.items():
            if ops.tune_get(k) != v:
                ops.tune_set(k, v)
        ops.jit_config(st["mode"], st["min_rows"])


def note(kernel, model, n, knob=None):
    """one line per distinct call for the kernel-trace evidence"""
    if _LOG:
        per_wg = LS.WAVES if model.family == "block" else 1  # block mode: a unit per wave, four waves a workgroup
        rec = {"kernel": kernel, "family": model.family, "rows": int(n), "unit_rows": model.unit_rows,
               "units": int(model.units(n)), "units_per_round": int(model.workers(n)),
               "model_grid": -(-int(model.workers(n)) // per_wg), "grid_is_exact": model.exact_grid,
               "knob": knob, "cus": CUS}
        with open(_LOG, "a") as f:
            f.write(json.dumps(rec) + "\n")


def fld(n):
    return R.Field(n)


def const(v, t="UInt64"):
    return R.Const(R.Value(t, v))


def dev(arr, dt, off=0):
    """the rows of arr starting `off` elements into a 256-byte aligned buffer"""
    return TA.numpy_dev(np.ascontiguousarray(arr), dt, off)


def bitmap_pred(keep):
    """(fq_pred of kind BITMAP over the LSB-first words of `keep`, the device words that back it)"""
    bits = np.zeros(((len(keep) + 63) // 64) * 64, bool)
    bits[:len(keep)] = keep
    words = ops.from_numpy(np.packbits(bits, bitorder="little").view(np.uint64), U64)
    p = abi.fq_pred()
    p.kind = abi.PRED_BITMAP
    p.bitmap = words.ptr
    return p, words


# ---------------------------------------------------------------------------
# for32
# ---------------------------------------------------------------------------
FOR32_DATA = ["random", "span_max"]  # tests/test_for32_gpu.py host_values: a random base per frame; a frame spanning 2^32 - 1


def for32_input(cus, wg, case, data):
    m = LS.for32(cus, wg)
    n, head = m.cases()[case]
    return m, n, head, TF.host_values(n, data)


@pytest.mark.parametrize("data", FOR32_DATA)
@pytest.mark.parametrize("case", LS.CASES)
@pytest.mark.parametrize("wg", [1, 2])
def test_for32_scan_strides_over_tiles_of_other_frames(wg, case, data):
    m, n, head, host = for32_input(CUS, wg, case, data)
    assert TF.encodable(host)
    # a workgroup's next tile is `grid` tiles on: another frame as soon as the grid holds a frame's 16 tiles
    assert m.cap >= LS.FOR32_TILES_PER_FRAME
    col = dev(host, U64, head)
    assert col.ptr % 16 == 8 * head
    ops.tune_set("SCAN_WG_PER_CU", wg)
    enc, ok = ops.for32_encode(col)
    assert ok
    note("agg_flat_kernel_for32", m, n, wg)
    s, c, mx, mn = [x.bits for x in oracle_c.column_partial(host, U64, n, TF.AGGS)]
    for mask in TF.MASKS:
        got = ops.aggregate_for32(enc, mask)
        plain = ops.aggregate(col, 0, None, None, mask)
        assert TF.fields(got) == TF.fields(plain), (mask, TF.fields(got), TF.fields(plain))
        assert got.dtype == U64 and got.flags == 0 and got.count == c == n
        if mask & abi.AGG_SUM:
            assert got.sum == s, mask
        if mask & abi.AGG_MAX:
            assert got.max == mx, mask
        if mask & abi.AGG_MIN:
            assert got.min == mn, mask


# ---------------------------------------------------------------------------
# flat scans.  A combo: its launch model, host columns, and per shape (predicate?, chain?) the C-ABI structs and
# the oracle's functions
# ---------------------------------------------------------------------------
class Combo:
    def __init__(self, entry, names, dts, model, data, pred, value, where, arg, nullable=None):
        self.entry, self.names, self.dts, self.model, self.data = entry, names, dts, model, data
        self.pred, self.value, self.where, self.arg, self.nullable = pred, value, where, arg, nullable

    def shape(self, p, c):
        """(fq_pred, fq_expr, oracle filter, oracle argument) with / without the predicate and the value chain"""
        return (self.pred if p else None, self.value if c else None, self.where if p else None,
                self.arg if c else fld(self.names[0]))


def _u64(rng, n):
    return rng.integers(0, 1 << 64, n, dtype=np.uint64)


def combo_agg_u64():
    return Combo("aggregate", ["x"], [U64], lambda cus, wg: LS.flat_scan(cus, 8, wg), lambda rng, n: [_u64(rng, n)],
                 predicate(U64, [("%", 8)], "<", 3), chain(U64, [("+", 1)])[0], None, None)


def combo_agg_f64():
    # integers below 2^20 as Float64: any order of n < 2^32 of them sums exactly
    return Combo("aggregate", ["x"], [F64], lambda cus, wg: LS.flat_scan(cus, 8, wg),
                 lambda rng, n: [rng.integers(0, 1 << 20, n).astype(np.float64)],
                 predicate(F64, [], "<", float(1 << 19)), chain(F64, [("+", 1.0)])[0], None, None)


def combo_cols2():
    dts = [U64, U64]
    return Combo("columns", ["a", "b"], dts, lambda cus, wg: LS.flat_scan_columns(cus, 2, wg),
                 lambda rng, n: [_u64(rng, n), _u64(rng, n)],
                 predicate_columns(dts, [], "<", K38), chain_columns(dts, [("+", Col(1))])[0],
                 R.Compare("<", fld("a"), const(K38)), R.Arith("+", fld("a"), fld("b")))


def combo_cols4():
    # a % 8 < 3; c + d + b in Float64: integers below 2^13, exact
    dts = [U64, I64, F64, U64]
    return Combo("columns", ["a", "b", "c", "d"], dts, lambda cus, wg: LS.flat_scan_columns(cus, 4, wg),
                 lambda rng, n: [_u64(rng, n), rng.integers(-1000, 1001, n).astype(np.int64),
                                 rng.integers(0, 4096, n).astype(np.float64), rng.integers(0, 1000, n).astype(np.uint64)],
                 predicate_columns(dts, [("%", 8)], "<", 3),
                 chain_columns(dts, [load(2), ("+", Col(3)), ("+", Col(1))])[0],
                 R.Compare("<", R.Arith("%", fld("a"), const(8)), const(3)),
                 R.Arith("+", R.Arith("+", fld("c"), fld("d")), fld("b")))


WIDE = [F64, F32, I32, U8]
WIDE_NAMES = ["price", "discount", "shipdate", "quantity"]


def wide_data(rng, n):
    return [rng.integers(0, 1000, n).astype(np.float64), rng.integers(0, 16, n).astype(np.float32),
            rng.integers(8000, 10600, n).astype(np.int32), rng.integers(1, 51, n).astype(np.uint8)]


def wide_value():
    # discount * discount in Float32 (below 2^24), + price + shipdate in Float64 (below 2^14 each)
    return (chain_columns(WIDE, [load(1), ("*", Col(1)), ("+", Col(0)), ("+", Col(2))])[0],
            R.Arith("+", R.Arith("+", R.Arith("*", fld("discount"), fld("discount")), fld("price")), fld("shipdate")))


def combo_typed_wide():
    value, arg = wide_value()
    return Combo("typed", WIDE_NAMES, WIDE, lambda cus, wg: LS.flat_scan_typed(cus, [8, 4, 4, 1], wg), wide_data,
                 predicate_columns(WIDE, [load(3)], "<", (26, "UInt8")), value,
                 R.Compare("<", fld("quantity"), const(26, "UInt8")), arg)


def combo_typed_8bit():
    dts = [U8, I8]
    return Combo("typed", ["a", "b"], dts, lambda cus, wg: LS.flat_scan_typed(cus, [1, 1], wg),
                 lambda rng, n: [rng.integers(0, 256, n).astype(np.uint8), rng.integers(-128, 128, n).astype(np.int8)],
                 predicate_columns(dts, [], "<", (100, "UInt8")), chain_columns(dts, [("+", Col(1))])[0],
                 R.Compare("<", fld("a"), const(100, "UInt8")), R.Arith("+", fld("a"), fld("b")))


def combo_nullable():
    # validity bitmaps on price and shipdate (7/8 of the rows valid); the predicate reads a nullable column
    value, arg = wide_value()
    return Combo("nullable", WIDE_NAMES, WIDE, lambda cus, wg: LS.flat_scan_typed(cus, [8, 4, 4, 1], wg), wide_data,
                 predicate_columns(WIDE, [load(2)], "<", (9950, "Int32")), value,
                 R.Compare("<", fld("shipdate"), const(9950, "Int32")), arg, nullable=[1, 0, 1, 0])


COMBOS = {"agg_u64": combo_agg_u64, "agg_f64": combo_agg_f64, "cols2": combo_cols2, "cols4": combo_cols4,
          "typed_wide": combo_typed_wide, "typed_8bit": combo_typed_8bit, "nullable": combo_nullable}
SCAN_KNOBS = [1, 2, 16]
# (combo, the SCAN_WG_PER_CU the input is sized for, case)
FLAT_RUNS = [(c, k, case) for c in COMBOS for k in (1, 2) for case in LS.CASES] + \
            [("agg_u64", 16, case) for case in LS.CASES] + \
            [(c, 16, "ragged") for c in ("agg_f64", "cols2", "cols4", "typed_wide")]


@functools.lru_cache(maxsize=None)
def combo(name):
    return COMBOS[name]()


def flat_input(cus, name, sized_for, case):
    """(combo, model, rows, head, host columns, validity per column or None)"""
    C = combo(name)
    m = C.model(cus, sized_for)
    n, head = m.cases()[case]
    rng = np.random.default_rng([sorted(COMBOS).index(name), n])
    host = C.data(rng, n)
    valid = None
    if C.nullable:
        valid = [rng.integers(0, 8, n) != 0 if nl else None for nl in C.nullable]
    return C, m, n, head, host, valid


def flat_shapes(name, sized_for):
    """(predicate?, value chain?) per input size: all four at the smallest; at 16 the fq_ref-checked entry points
    run the one with both"""
    if sized_for == 1:
        return [(0, 0), (1, 0), (0, 1), (1, 1)]
    return [(0, 0), (1, 1)] if sized_for == 2 or combo(name).entry == "aggregate" else [(1, 1)]


def flat_reference(C, host, valid, p, c, block_rows=0):
    """the oracle's answer for shape (p, c): fq_aggregate -> the replayed states of oracle_c.column_partial, the
    others -> the dict of their file's ref_scan"""
    pred, value, where, arg = C.shape(p, c)
    if C.entry == "aggregate":
        n = len(host[0])
        return [as_tuple(s) for s in oracle_c.column_partial(host[0], C.dts[0], block_rows or n,
                                                             [(op, value) for op in AGGS], pred)]
    if C.entry == "nullable":
        return TN.ref_scan(C.names, C.dts, host, valid, where, None, arg, block_rows)
    return TA.ref_scan(C.names, C.dts, host, where, arg, block_rows)


def exact_sum(st, exp):
    """Float64 sums of this file are exact: not within a bound, equal"""
    if exp["dtype"] == F64 and exp["sum"] is not None:
        assert TA.f64_of(st.sum) == exp["sum"].value, (TA.f64_of(st.sum), exp["sum"].value)


def flat_run(C, cols, vdev, p, c, block_rows, mask=ALL):
    pred, value, _, _ = C.shape(p, c)
    if C.entry == "aggregate":
        return ops.aggregate(cols[0], block_rows, pred, value, mask)
    if C.entry == "columns":
        return ops.aggregate_columns(cols, block_rows, pred, value, mask)
    if C.entry == "typed":
        return ops.aggregate_typed(cols, block_rows, pred, value, mask)
    return ops.aggregate_nullable(cols, vdev, block_rows, pred, value, mask)


def flat_check(C, st, exp, what):
    if C.entry == "aggregate":
        got = [replay(op, st) for op in AGGS]
        assert got == exp, (what, got, exp)
    elif C.entry == "nullable":
        TN.check(st, exp, ALL, what)
        exact_sum(st.s, exp)
    else:
        TA.check(st, exp, ALL, what)
        exact_sum(st, exp)


def modes_of(C):
    # only fq_aggregate has an interpreting kernel; the other entry points run hipRTC kernels whatever the policy
    return [abi.JIT_ALWAYS, abi.JIT_OFF] if C.entry == "aggregate" else [abi.JIT_ALWAYS]


@pytest.mark.parametrize("name,sized_for,case", FLAT_RUNS, ids=["%s-wg%d-%s" % r for r in FLAT_RUNS])
def test_flat_scan_equals_oracle_under_every_grid(name, sized_for, case):
    C, m, n, head, host, valid = flat_input(CUS, name, sized_for, case)
    per = m.per_worker(n)
    if case == "one_round_minus":
        assert max(per) <= 1
    else:
        assert min(per) >= 2
    cols = [dev(h, dt, head) for h, dt in zip(host, C.dts)]
    vdev = [TN.bitmap_dev(v) for v in valid] if valid else None
    block_rows = n if C.entry == "aggregate" else 0  # one reference block: the flat kernels
    kernel = "fq_jit_scan" if C.entry != "aggregate" else "agg_flat_kernel+fq_jit_scan"
    for p, c in flat_shapes(name, sized_for):
        exp = flat_reference(C, host, valid, p, c)
        seen = set()
        for wg in SCAN_KNOBS:
            ops.tune_set("SCAN_WG_PER_CU", wg)
            for mode in modes_of(C):
                ops.jit_config(mode, 0)
                st = flat_run(C, cols, vdev, p, c, block_rows)
                flat_check(C, st, exp, "%s n=%d wg=%d mode=%d shape=%d%d" % (name, n, wg, mode, p, c))
                seen.add(bytes(st))
            note(kernel, C.model(CUS, wg), n, wg)
        assert len(seen) == 1, (name, n, p, c)  # every grid, both kernels: the same bytes
    if C.entry == "aggregate":
        # sum + count without predicate or chain: the interpreter's prefetching variant (agg_flat_kernel<.., PF>)
        mask = abi.AGG_SUM | abi.AGG_COUNT
        exp = flat_reference(C, host, valid, 0, 0)
        seen = set()
        for wg in SCAN_KNOBS:
            ops.tune_set("SCAN_WG_PER_CU", wg)
            ops.jit_config(abi.JIT_OFF, 0)
            st = flat_run(C, cols, vdev, 0, 0, block_rows, mask)
            assert (replay(abi.AGG_SUM, st), replay(abi.AGG_COUNT, st)) == (exp[0], exp[3]), (name, n, wg)
            seen.add((st.sum, st.count, st.flags, st.blocks))
        assert len(seen) == 1


# ---------------------------------------------------------------------------
# block mode: one wave per reference block, W = grid x 4 waves, block b on wave b % W
# ---------------------------------------------------------------------------
BLOCK_ROWS = 144  # even and a multiple of every row group used here (4): 16-byte loads; 72 vectors: a second, partial step
BLOCK_ENTRIES = ["aggregate", "columns", "typed", "nullable"]
BLOCK_PATTERNS = ["second", "first"]
BLOCK_TYPED = [I32, U8, F64]


def block_geometry(cus, case="ragged"):
    m = LS.block_scan(cus, BLOCK_ROWS)
    n = m.cases()[case][0]
    return m, n, m.units(n), m.cap


def emptied_blocks(pattern, nb, W):
    """blocks that keep no row: every third block among the waves' first blocks, or among those second blocks
    whose wave has a third -- a wave that meets one always has a later, kept block to go.  (With one block per
    wave at the most, the launch model's one_round_minus, both are every third block.)"""
    if pattern == "none":
        return np.zeros(0, np.int64)
    if nb <= W:
        lo, hi = 0, nb
    else:
        assert nb > 2 * W
        lo, hi = (0, W) if pattern == "first" else (W, nb - W)
    b = np.arange(lo, hi)
    return b[b % 3 == 0]


def block_input(cus, entry, pattern, case="ragged"):
    """column 0 holds (7 row) % 1000 where the predicate `x < 2000` keeps a row and 5000 + row % 1000 in the
    emptied blocks; -> (combo, model, rows, blocks, host, validity)"""
    m, n, nb, W = block_geometry(cus, case)
    row = np.arange(n, dtype=np.uint64)
    x = (row * np.uint64(7)) % np.uint64(1000)
    gone = np.zeros(nb, bool)
    gone[emptied_blocks(pattern, nb, W)] = True
    x = np.where(np.repeat(gone, BLOCK_ROWS)[:n], np.uint64(5000) + row % np.uint64(1000), x)
    rng = np.random.default_rng([BLOCK_ENTRIES.index(entry), len(pattern)])
    valid = None
    if entry == "aggregate":
        C = Combo("aggregate", ["x"], [U64], None, None, predicate(U64, [], "<", 2000), chain(U64, [("+", 1)])[0],
                  R.Compare("<", fld("x"), const(2000)), R.Arith("+", fld("x"), const(1)))
        host = [x]
    elif entry == "columns":
        dts = [U64, U64]
        C = Combo("columns", ["a", "b"], dts, None, None, predicate_columns(dts, [], "<", 2000),
                  chain_columns(dts, [("+", Col(1))])[0], R.Compare("<", fld("a"), const(2000)),
                  R.Arith("+", fld("a"), fld("b")))
        host = [x, _u64(rng, n)]
    else:
        dts = BLOCK_TYPED
        C = Combo(entry, ["x", "q", "f"], dts, None, None, predicate_columns(dts, [], "<", (2000, "Int32")),
                  chain_columns(dts, [("+", Col(2)), ("+", Col(1))])[0], R.Compare("<", fld("x"), const(2000, "Int32")),
                  R.Arith("+", R.Arith("+", fld("x"), fld("f")), fld("q")),
                  nullable=[0, 0, 1] if entry == "nullable" else None)
        host = [x.astype(np.int32), rng.integers(0, 256, n).astype(np.uint8), rng.integers(0, 4096, n).astype(np.float64)]
        if entry == "nullable":
            valid = [None, None, rng.integers(0, 8, n) != 0]
    return C, m, n, nb, host, valid


def block_reference(C, host, valid):
    """the per-block oracle of the entry point's own test file (fq_aggregate: the typed one over its one column)"""
    _, _, where, arg = C.shape(1, 1)
    if C.entry == "nullable":
        return TN.ref_scan(C.names, C.dts, host, valid, where, None, arg, BLOCK_ROWS)
    return TA.ref_scan(C.names, C.dts, host, where, arg, BLOCK_ROWS)


@pytest.mark.parametrize("pattern", BLOCK_PATTERNS)
@pytest.mark.parametrize("entry", BLOCK_ENTRIES)
def test_block_mode_carries_any_empty_and_the_sums_across_a_waves_blocks(entry, pattern):
    C, m, n, nb, host, valid = block_input(CUS, entry, pattern)
    per = m.per_worker(n)
    assert min(per) >= 2 and max(per) == min(per) + 1 and len(per) == m.cap
    assert LS.typed_group([WIDTH[d] for d in BLOCK_TYPED])[0] == 4 and BLOCK_ROWS % 4 == 0
    exp = block_reference(C, host, valid)
    assert exp["flags"] & abi.STATE_ANY_EMPTY and exp["count"] > 0
    cols = [dev(h, dt) for h, dt in zip(host, C.dts)]
    vdev = [TN.bitmap_dev(v) for v in valid] if valid else None
    note("agg_block_kernel+fq_jit_scan" if entry == "aggregate" else "fq_jit_scan", m, n)
    seen = set()
    for u in (4, 8, 16):
        ops.tune_set("BLOCK_U", u)
        for mode in modes_of(C):
            ops.jit_config(mode, 0)
            st = flat_run(C, cols, vdev, 1, 1, BLOCK_ROWS)
            what = "%s %s BLOCK_U=%d mode=%d" % (entry, pattern, u, mode)
            s = st.s if entry == "nullable" else st
            assert s.blocks == nb, (what, s.blocks, nb)
            if entry == "nullable":
                TN.check(st, exp, ALL, what)
            else:
                TA.check(st, exp, ALL, what)
            exact_sum(s, exp)
            seen.add(bytes(st))
    assert len(seen) == 1


def test_block_mode_without_an_empty_block_raises_no_flag():
    # the same geometry, every block keeps rows: oracle_c's per-block loop and the reference's state machine
    C, m, n, nb, host, _ = block_input(CUS, "aggregate", "none")
    pred, value, _, _ = C.shape(1, 1)
    exp = [as_tuple(s) for s in oracle_c.column_partial(host[0], U64, BLOCK_ROWS, [(op, value) for op in AGGS], pred)]
    col = dev(host[0], U64)
    for u in (4, 8, 16):
        ops.tune_set("BLOCK_U", u)
        for mode in (abi.JIT_ALWAYS, abi.JIT_OFF):
            ops.jit_config(mode, 0)
            st = ops.aggregate(col, BLOCK_ROWS, pred, value, ALL)
            assert st.blocks == nb and not st.flags & abi.STATE_ANY_EMPTY, (u, mode, st.flags)
            assert [replay(op, st) for op in AGGS] == exp, (u, mode)


# ---------------------------------------------------------------------------
# Filter -> Projection: columns derived from an iota, so a row written to the wrong place or taken from the
# wrong LDS slot changes an output.  Keep rates by `key % 1000 < k`: 1,000 divides no tile, so neighbouring
# tiles' ballots differ
# ---------------------------------------------------------------------------
PROJ_ENTRIES = ["one", "cols2", "cols3", "cols4", "typed_q6", "typed_narrow"]
HASHED = "hashed"  # four columns only: keep by the hashed column instead of a remainder (cheap for the oracle at 20 M rows)
RATES = {"1/1000": 1, "1/8": 125, "999/1000": 999, "every": 1000, "1/8 hashed": HASHED}
Q6_OUT = [F64, U8, F32]
NARROW = [U8, U16]
NARROW_OUT = [U16, U8]
MULT = np.uint64(0x9E3779B97F4A7C15)


def proj_typed(entry):
    """(column widths, output widths) of a typed entry's geometry, else None"""
    if entry == "typed_q6":
        return [WIDTH[d] for d in WIDE], [WIDTH[d] for d in Q6_OUT]
    if entry == "typed_narrow":
        return [WIDTH[d] for d in NARROW], [WIDTH[d] for d in NARROW_OUT]
    return None


def proj_n_cols(entry):
    return int(entry[4]) if entry.startswith("cols") else 1


def proj_case(entry, n, k, first=7):
    """tests/test_project_typed_gpu.py Case over rows first .. first + n of the iota; the predicate keeps
    key % 1000 < k (k = None: no predicate)"""
    i = np.arange(first, first + n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        if entry == "one":
            names, dts, host = ["x"], [U64], [i]
            pred = predicate(U64, [("%", 1000)], "<", k) if k is not None else None
            values = [chain(U64, [("+", 1)])[0], None]
            exprs = [R.Arith("+", fld("x"), const(1)), fld("x")]
            key = fld("x")
        elif entry.startswith("cols"):
            K = proj_n_cols(entry)
            names, dts = ["a", "b", "c", "d"][:K], [U64, I64, F64, U64][:K]
            host = [i, i.astype(np.int64) - np.int64(1000), i.astype(np.float64), i * MULT][:K]
            pred = predicate_columns(dts, [("%", 1000)], "<", k) if k not in (None, HASHED) else None
            values = [chain_columns(dts, [("+", Col(K - 1))])[0], chain_columns(dts, [load(1)])[0]]
            exprs = [R.Arith("+", fld("a"), fld(names[K - 1])), fld("b")]
            if K == 4:
                values.append(chain_columns(dts, [load(2)])[0])
                exprs.append(fld("c"))
            key = fld("a")
            if k == HASHED:  # d = row x an odd constant, modulo 2^64: below 2^61 on an eighth of the rows
                assert K == 4
                return TP.Case(names, dts, host, predicate_columns(dts, [load(3)], "<", 1 << 61), values,
                               R.Compare("<", fld("d"), const(1 << 61)), exprs)
        elif entry == "typed_q6":
            names, dts = WIDE_NAMES, WIDE
            host = [i.astype(np.float64), (i % np.uint64(16)).astype(np.float32), (i % np.uint64(1000)).astype(np.int32),
                    (i % np.uint64(251)).astype(np.uint8)]
            pred = predicate_columns(dts, [load(2)], "<", (k, "Int32")) if k is not None else None
            values = [chain_columns(dts, [("*", Col(1))])[0], chain_columns(dts, [load(3)])[0],
                      chain_columns(dts, [load(1), ("*", Col(1))])[0]]
            assert [v.out_dtype for v in values] == Q6_OUT
            exprs = [R.Arith("*", fld("price"), fld("discount")), fld("quantity"),
                     R.Arith("*", fld("discount"), fld("discount"))]
            where = R.Compare("<", fld("shipdate"), const(k, "Int32")) if k is not None else None
            return TP.Case(names, dts, host, pred, values, where, exprs)
        else:
            names, dts = ["a", "b"], NARROW
            host = [(i % np.uint64(251)).astype(np.uint8), (i % np.uint64(65521)).astype(np.uint16)]
            pred = predicate_columns(dts, [load(1), ("%", 1000)], "<", k) if k is not None else None
            values = [chain_columns(dts, [("+", Col(1))])[0], None]
            assert values[0].out_dtype == U16
            exprs = [R.Arith("+", fld("a"), fld("b")), fld("a")]
            key = fld("b")
    where = R.Compare("<", R.Arith("%", key, const(1000)), const(k)) if k is not None else None
    return TP.Case(names, dts, host, pred, values, where, exprs)


def proj_keep(case):
    """the predicate's Boolean column from the oracle"""
    blk = R.Block([(nm, R.Arr(TP.REF[dt], h)) for nm, dt, h in zip(case.names, case.dts, case.host)])
    return np.asarray(case.where.eval(blk).values, dtype=bool)


def proj_dev(case, off=0):
    return [dev(h, dt, off) for h, dt in zip(case.host, case.dts)]


def run_select(entry, cols, pred, values, out_offset=0):
    if entry == "one":
        assert out_offset == 0
        return ops.filter_project(cols[0], pred, values)
    if entry.startswith("cols"):
        assert out_offset == 0
        return ops.filter_project_columns(cols, pred, values)
    return ops.filter_project_typed(cols, pred, values, out_offset=out_offset)


def check_contiguous(entry, case, cols, pred, what, out_offset=0):
    """every output and its length against the oracle; a look-back that gave up raises FQError here"""
    want, counts, dts = case.oracle(0)
    outs = run_select(entry, cols, pred, case.values, out_offset)
    assert len(outs) == len(want)
    for j, o in enumerate(outs):
        assert o.len == sum(counts), (what, j, o.len, sum(counts))
        assert o.dtype == dts[j], (what, j)
        assert TP.same(o.to_numpy(), np.concatenate(want[j]), dts[j]), (what, j)


def select_model(cus, entry, wg):
    return LS.select(cus, wg, proj_n_cols(entry), proj_typed(entry))


# (entry, SELECT_WG_PER_CU the input is sized for and runs at, case, keep rates)
SELECT_RUNS = [(e, 1, case, list(RATES)[:4] if case == "ragged" else ["1/8"]) for e in PROJ_ENTRIES for case in LS.CASES] + \
              [("cols4", 16, "ragged", ["1/8 hashed"])]


@pytest.mark.parametrize("entry,wg,case,rates", SELECT_RUNS, ids=["%s-wg%d-%s" % r[:3] for r in SELECT_RUNS])
def test_lookback_select_when_a_workgroup_draws_a_second_ticket(entry, wg, case, rates):
    m = select_model(CUS, entry, wg)
    n, head = m.cases()[case]
    if case == "exact_2":
        assert m.units(n) == 2 * m.cap
    elif case != "one_round_minus":
        assert m.units(n) > 2 * m.cap and m.units(n) % m.cap  # whatever the occupancy leaves of the cap
    ops.tune_set("SELECT_WG_PER_CU", wg)
    note("fq_jit_pselect", m, n, wg)
    cols = None
    for rate in rates:
        case_ = proj_case(entry, n, RATES[rate])
        cols = cols or proj_dev(case_, head)  # the same rows at every rate
        what = "%s n=%d wg=%d %s" % (entry, n, wg, rate)
        check_contiguous(entry, case_, cols, case_.pred, what + " comparison")
        if wg == 1:  # (the 20 M-row case: by comparison only, the oracle's second pass costs another second)
            bm, words = bitmap_pred(proj_keep(case_))
            check_contiguous(entry, case_, cols, bm, what + " bitmap")
            del words


# ---- block stream ----
STREAM_BLOCKS = [10000, LS.PROJECT_MIN_BLOCK_ROWS]
STREAM_K = 375  # keeps 3/8 of the rows


def stream_rows(cus, block_rows, case="ragged"):
    m = LS.block_stream(cus, block_rows, 1)
    n = m.cases()[case][0]
    if case == "ragged":
        assert n % block_rows and m.units(n) > 2 * m.cap  # a short last block, in some workgroup's third run
    return m, n


def run_blocks(entry, cols, block_rows, pred, values, out_offset):
    """-> (outputs, per-block counts, the byte left in rows that no block wrote or None)"""
    if entry == "one":
        outs, cnt = ops.filter_project_blocks(cols[0], block_rows, pred, values, out_offset=out_offset)
        return outs, cnt, None
    if entry.startswith("cols"):
        outs, cnt, kept = ops.filter_project_blocks_columns(cols, block_rows, pred, values, out_offset=out_offset,
                                                            fill=0xA5A5A5A5A5A5A5A5)
    else:
        outs, cnt, kept = ops.filter_project_blocks_typed(cols, block_rows, pred, values, out_offset=out_offset, fill=0xA5)
    assert kept == int(cnt.sum())
    return outs, cnt, 0xA5


def check_blocks(entry, case, cols, block_rows, out_offset, what):
    """per-block counts and every block's kept rows at [b B, b B + count) against the oracle; rows past a count
    keep the fill where the wrapper can set one"""
    want, counts, dts = case.oracle(block_rows)
    outs, cnt, fill = run_blocks(entry, cols, block_rows, case.pred, case.values, out_offset)
    assert list(cnt) == counts, what
    pos = np.concatenate([b * block_rows + np.arange(c) for b, c in enumerate(counts)])
    for j, o in enumerate(outs):
        assert o.dtype == dts[j], (what, j)
        got = o.to_numpy()
        assert TP.same(got[pos], np.concatenate(want[j]), dts[j]), (what, j)
        if fill is not None:
            rest = np.ones(case.n, bool)
            rest[pos] = False
            assert np.all(got[rest].view(np.uint8) == fill), (what, j)


@functools.lru_cache(maxsize=4)
def stream_case(entry, n):
    return proj_case(entry, n, STREAM_K)


@pytest.mark.parametrize("stage", [0, 1, 2, 4])
@pytest.mark.parametrize("rows", [8, 16, 32])
def test_block_stream_single_column_over_rows_and_stage(rows, stage):
    ops.tune_set("SELECT_BLOCKS_WG_PER_CU", 1)
    ops.tune_set("SELECT_BLOCKS_ROWS", rows)
    ops.tune_set("SELECT_BLOCKS_STAGE", stage)
    for B in STREAM_BLOCKS:
        m, n = stream_rows(CUS, B)
        case = stream_case("one", n)
        cols = proj_dev(case)
        note("fq_jit_pblocks", m, n, 1)
        for out_offset in (0, 1):  # 1: outputs 8 bytes off the 16-byte boundary, the kernel's al == 0 stores
            check_blocks("one", case, cols, B, out_offset, "rows=%d stage=%d B=%d off=%d" % (rows, stage, B, out_offset))


@pytest.mark.parametrize("entry", ["cols2", "cols3", "cols4", "typed_q6", "typed_narrow"])
def test_block_stream_columns_and_typed(entry):
    ops.tune_set("SELECT_BLOCKS_WG_PER_CU", 1)
    for B in STREAM_BLOCKS:
        m, n = stream_rows(CUS, B)
        case = proj_case(entry, n, STREAM_K)
        cols = proj_dev(case)
        note("fq_jit_pblocks", m, n, 1)
        for out_offset in (0, 1):
            check_blocks(entry, case, cols, B, out_offset, "%s B=%d off=%d" % (entry, B, out_offset))


# ---- predicate -> bitmap, and the no-predicate map ----
def run_bitmap(entry, cols, pred):
    if entry == "one":
        return ops.predicate_bitmap(cols[0], pred)
    if entry.startswith("cols"):
        return ops.predicate_bitmap_columns(cols, pred)
    return ops.predicate_bitmap_typed(cols, pred)


@pytest.mark.parametrize("entry", ["one", "cols2", "cols4", "typed_narrow"])
def test_predicate_bitmap_past_the_grid_cap(entry):
    # typed_narrow: UInt8 + UInt16, 3 bytes per row, the narrowest layout with two widths
    m = LS.bitmap(CUS, len(proj_typed(entry)[0]) if proj_typed(entry) else proj_n_cols(entry))
    n = m.just_above()
    per = m.per_worker(n)
    assert len(per) == m.cap and max(per) == 2 and min(per) == 1
    case = proj_case(entry, n, RATES["1/8"])
    want = proj_keep(case)
    note("fq_jit_pbits", m, n)
    for off in (0, 1):
        bm = run_bitmap(entry, proj_dev(case, off), case.pred)
        assert np.array_equal(bm.to_numpy(), want), (entry, n, off)
        words = bm.buf[bm.offset:bm.offset + bm.nbytes()].cpu().numpy().view(np.uint64)
        assert int(words[-1]) >> (n % 64) == 0, (entry, n, off)  # bits past n are cleared


@pytest.mark.parametrize("entry", ["one", "cols2", "typed_narrow"])
def test_map_path_past_the_grid_cap(entry):
    m = LS.project_map(CUS, proj_typed(entry))
    n = m.just_above()
    per = m.per_worker(n)
    assert len(per) == m.cap and max(per) == 2 and min(per) == 1
    case = proj_case(entry, n, None)
    note("fq_jit_pmap", m, n)
    for off in (0, 1):  # 1: off the 16-byte boundary (typed: off the row group's grid), the element path
        check_contiguous(entry, case, proj_dev(case, off), None, "%s map n=%d off=%d" % (entry, n, off))
    if entry == "typed_narrow":
        check_contiguous(entry, case, proj_dev(case), None, "typed map, outputs one element off", out_offset=1)


# ---------------------------------------------------------------------------
# element-wise fast paths
# ---------------------------------------------------------------------------
def ew_host(n):
    rng = np.random.default_rng(n)
    return _u64(rng, n), rng.integers(1, 1 << 40, n).astype(np.uint64)


@pytest.fixture(scope="module")
def ew_columns():
    """the two host columns at the longest length of the six runs (0.6 GB at 256 CUs), drawn once, sliced by each
    run and released when this module's tests are over"""
    big = max(ew_rows(CUS, k, g)[1] for k in ("arith", "compare") for g in (0, 1, 16))
    return ew_host(big)


def ew_rows(cus, kind, knob):
    m = (LS.ew_arith if kind == "arith" else LS.ew_compare)(cus, knob)
    return m, m.cases()["ragged"][0]


@pytest.mark.parametrize("knob", [0, 1, 16])
@pytest.mark.parametrize("kind", ["arith", "compare"])
def test_elementwise_fast_paths_iterate(kind, knob, ew_columns):
    m, n = ew_rows(CUS, kind, knob)
    per = m.per_worker(n)
    assert len(per) == m.cap and min(per) >= 2 and max(per) == min(per) + 1
    a, b = (h[:n] for h in ew_columns)
    A, B = ops.from_numpy(a), ops.from_numpy(b)
    ops.tune_set("EW_WG_PER_CU", knob)
    note("arith_vec_kernel" if kind == "arith" else "compare_vec_kernel", m, n, knob)
    # numpy is the reference, as in tests/test_kernels_gpu.py test_elementwise_vector_fast_paths: wrapping
    # UInt64 arithmetic, truncating division (b >= 1)
    k = np.uint64(12345)
    if kind == "arith":
        with np.errstate(over="ignore"):
            runs = [("+", B, a + b), ("*", (int(k), "UInt64"), a * k), ("/", B, a // b)]
        for sym, rhs, want in runs:
            assert np.array_equal(ops.arith(sym, A, rhs).to_numpy(), want), (sym, knob)
    else:
        half = 1 << 63
        a2 = np.roll(a, 1)  # a row against its predecessor: true on about half the rows
        for sym, rhs, want in (("<", ops.from_numpy(a2), a < a2), (">=", (half, "UInt64"), a >= np.uint64(half))):
            assert np.array_equal(ops.compare(sym, A, rhs).to_numpy(), want), (sym, knob)


def test_knobs_and_jit_policy_are_back_at_their_defaults():
    assert {k: ops.tune_get(k) for k in LS.DEFAULT_KNOBS} == LS.DEFAULT_KNOBS
    st = ops.jit_stats()
    assert (st["mode"], st["min_rows"]) == (abi.JIT_AUTO, 1 << 22)
