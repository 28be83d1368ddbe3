"""The cases of fq_group_aggregate_columns and their reference (no test of its
own; imported by tests/test_groupby_columns_cpu.py and
tests/test_groupby_columns_gpu.py).

A Spec is one logical GROUP BY over the K columns c0 .. c{K-1} of one block.
Every chain is stated twice: as the step list fq_amd.expr.chain_columns /
predicate_columns / pred_tree_columns lower to the C ABI, and as the matching
oracle/fq_ref.py function tree; Spec asserts that both state the same types.
reference() builds an fq_ref Block of the columns, evaluates the predicate on
it, the key and every argument on the kept rows (so a zero divisor on a dropped
row is no error), and groups on the host with a stable sort and reduceat, as
tests/fuzz_groupby.py fold_rows does.  Its Result is fuzz_groupby's, so `same`
and `tables_equal` compare device tables with it.

Float64 values are drawn as multiples of one power of two, few enough per
group that every partial sum is exact: the device's sums, in whatever order its
atomics run, equal the reference's bit for bit (exactly_summable is asserted
on the reference side).

launch_rows() restates the launch of fq_jit_groupby_cols in numpy -- the rows
per lane, the tile, the grid, the chunked or strided map of tiles to
workgroups, the one-row tail -- and can make five mistakes on purpose
(MISTAKES); tests/test_groupby_columns_cpu.py shows that each of them changes
the expected table of a generated case."""
import numpy as np

import fq_ref as R
from fq_amd import abi
from fq_amd.expr import STACK, Col, chain_columns, load, pred_tree_columns, predicate_columns, push
from fuzz_groupby import DIV_ZERO, Result, exactly_summable, keep_words, lds_slots, small_knobs  # noqa: F401

U, I, F = "UInt64", "Int64", "Float64"
DT = abi.DT_BY_NAME
NPT = {U: np.uint64, I: np.int64, F: np.float64}
E1 = 0xFFFFFFFFFFFFFFFF
COUNT, SUM, MAX, MIN = abi.AGG_COUNT, abi.AGG_SUM, abi.AGG_MAX, abi.AGG_MIN
SMALL_THREADS, SMALL_LDS_KB = 256, 8
LAYOUTS = {"aligned": (0, 0, 0, 0), "all_offset": (1, 1, 1, 1), "one_offset": (0, 1, 0, 0)}


def rows_per_lane(n_cols):
    """fq_scan.h group_cols_rows"""
    return 4 if n_cols <= 2 else 2


def tile_rows(n_cols, threads):
    return rows_per_lane(n_cols) * threads


def fld(j):
    return R.Field("c%d" % j)


def const(v, t=U):
    return R.Const(R.Value(t, v))


class Spec:
    """dts: the columns' type names; draw(rng, n) -> [host arrays]; key: (steps or None, fq_ref tree);
    aggs: [(kind, state type name, steps or None, fq_ref tree or None)]; pred: None | ("expr", (lhs steps, cmp,
    rhs), tree) | ("tree", (leaves, prog), tree) | ("bitmap", rate); key_t: the table's key type"""

    def __init__(self, name, dts, draw, key, aggs, pred=None):
        self.name, self.dts, self.draw, self.key, self.aggs, self.pred = name, dts, draw, key, aggs, pred
        self.K = len(dts)
        self.cdt = [DT[t] for t in dts]
        self.schema = {"c%d" % j: t for j, t in enumerate(dts)}
        self.key_t = key[1].return_type(self.schema)
        assert self.key_t in (U, I), self.key_t
        if key[0] is not None:
            assert abi.DT_NAMES[chain_columns(self.cdt, key[0])[1]] == self.key_t, name
        else:
            assert dts[0] == self.key_t
        for kind, t, steps, tree in aggs:
            if kind == COUNT:
                assert t == U
                continue
            assert tree.return_type(self.schema) == t, (name, t)
            assert (abi.DT_NAMES[chain_columns(self.cdt, steps)[1]] if steps is not None else dts[0]) == t, (name, t)

    @property
    def n_aggs(self):
        return len(self.aggs)

    def table_aggs(self):
        return [(k, DT[t]) for k, t, _, _ in self.aggs]

    def pred_kind(self):
        return self.pred[0] if self.pred else "none"

    def device(self):
        """(key fq_expr or None, [value fq_expr or None], fq_pred or None); a bitmap's pointer is set per launch"""
        key = None if self.key[0] is None else chain_columns(self.cdt, self.key[0])[0]
        vals = [None if k == COUNT or s is None else chain_columns(self.cdt, s)[0] for k, _, s, _ in self.aggs]
        pred = None
        if self.pred_kind() == "expr":
            lhs, sym, rhs = self.pred[1]
            pred = predicate_columns(self.cdt, lhs, sym, rhs)
        elif self.pred_kind() == "tree":
            pred = pred_tree_columns(self.cdt, *self.pred[1])
        elif self.pred_kind() == "bitmap":
            pred = abi.fq_pred()
            pred.kind = abi.PRED_BITMAP
        return key, vals, pred

    def slots(self, lds_kb):
        return lds_slots(self.n_aggs, lds_kb)


# ---------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------
def keep_mask(spec, host, keep=None, pred_swap=None):
    """the rows the predicate keeps; pred_swap = (i, j): the predicate reads column j where it names column i"""
    n = len(host[0])
    if spec.pred_kind() == "none":
        return np.ones(n, bool)
    if spec.pred_kind() == "bitmap":
        return np.asarray(keep, bool).copy()
    if n == 0:
        return np.zeros(0, bool)
    cols = list(host)
    if pred_swap is not None:
        i, j = pred_swap
        assert spec.dts[i] == spec.dts[j]
        cols[i] = host[j]
    blk = R.Block([("c%d" % j, R.Arr(t, h)) for j, (t, h) in enumerate(zip(spec.dts, cols))])
    with np.errstate(all="ignore"):
        res = spec.pred[2].eval(blk)
    assert res.valid is None or np.all(res.valid), "a cast gave nulls"
    return np.asarray(res.values, bool)


def fold(spec, cols, key_col=None):
    """Result of the rows of `cols` (all of them kept); key_col = (i, j): the key reads column j for column i"""
    n = len(cols[0])
    if n == 0:
        return Result(np.zeros(0, np.uint64), [np.zeros(0, np.uint64) for _ in spec.aggs], [None] * spec.n_aggs)
    blk = R.Block([("c%d" % j, R.Arr(t, h)) for j, (t, h) in enumerate(zip(spec.dts, cols))])
    kblk = blk
    if key_col is not None:
        i, j = key_col
        assert spec.dts[i] == spec.dts[j]
        kc = list(cols)
        kc[i] = cols[j]
        kblk = R.Block([("c%d" % c, R.Arr(t, h)) for c, (t, h) in enumerate(zip(spec.dts, kc))])

    def ev(tree, b):
        with np.errstate(all="ignore"):
            a = tree.eval(b)
        assert a.valid is None or np.all(a.valid), "a cast gave nulls"
        return np.ascontiguousarray(a.values)
    kb = ev(spec.key[1], kblk).view(np.uint64)
    vals = [None if k == COUNT else ev(tree, blk) for k, _, _, tree in spec.aggs]
    order = np.argsort(kb, kind="stable")
    k = kb[order]
    uniq, start = np.unique(k, return_index=True)
    states, amb = [], []
    for (kind, t, _, _), v in zip(spec.aggs, vals):
        a = None
        if kind == COUNT:
            s = np.diff(np.append(start, len(k))).astype(np.uint64)
        else:
            v = v[order]
            if kind == SUM:
                if t == F:  # exact in any order, or the comparison below would be of roundings
                    for lo, hi in zip(start, np.append(start[1:], len(k))):
                        assert exactly_summable(v[lo:hi]), (spec.name, "a Float64 sum is not exact")
                with np.errstate(all="ignore"):
                    # (a Float64 sum starts from +0.0, as the table's states do)
                    s = np.add.reduceat(v, start) + 0.0 if t == F else np.add.reduceat(v.view(np.uint64), start)
            elif t == F:
                # a NaN is ignored unless every kept row of the group is NaN; the sign of a
                # zero extreme is unspecified when both zeros occur
                s = (np.fmax if kind == MAX else np.fmin).reduceat(v, start)
                neg = np.logical_or.reduceat((v == 0) & np.signbit(v), start)
                pos = np.logical_or.reduceat((v == 0) & ~np.signbit(v), start)
                a = (s == 0) & neg & pos
            else:
                s = (np.maximum if kind == MAX else np.minimum).reduceat(v, start)
            s = np.ascontiguousarray(s).view(np.uint64)
        states.append(s)
        amb.append(a)
    return Result(uniq, states, amb)


def reference(spec, host, keep=None, rows=None, cols_rows=None, key_col=None, pred_swap=None):
    """("ok", Result) | ("err", DIV_ZERO).  rows: the row numbers that are folded (default: all; a kept row twice
    counts twice); cols_rows: per column the row numbers read for them (default: `rows`); key_col / pred_swap: see
    fold / keep_mask"""
    n = len(host[0])
    mask = keep_mask(spec, host, keep, pred_swap)
    if cols_rows is None:
        cols_rows = [np.arange(n) if rows is None else rows] * spec.K
    # (the predicate's verdict goes by the row of column 0)
    sel = mask[cols_rows[0]]
    idx = [c[sel] for c in cols_rows]
    try:
        return "ok", fold(spec, [h[i] for h, i in zip(host, idx)], key_col)
    except R.RefError as e:
        assert "Divide by zero" in str(e), str(e)
        return "err", DIV_ZERO


# ---------------------------------------------------------------------------
# numpy restatement of the launch (fq_jit.hip jit_groupby_columns, gen_groupby_cols_kernel)
# ---------------------------------------------------------------------------
MISTAKES = ["col1_row_off", "tail_dropped", "key_col0", "pred_wrong_col", "second_tile_skipped"]


def launch_grid(n, n_cols, knobs, cus):
    tile = tile_rows(n_cols, knobs["GROUP_THREADS"])
    return max(1, min(-(-n // tile), cus * knobs["GROUP_WG_PER_CU"]))


def workgroup_tiles(n, n_cols, knobs, cus):
    """[[tile numbers] per workgroup] (no key partitions)"""
    tile = tile_rows(n_cols, knobs["GROUP_THREADS"])
    grid, ntiles = launch_grid(n, n_cols, knobs, cus), n // tile
    if knobs["GROUP_CHUNKED"]:
        per = -(-ntiles // grid)
        return [list(range(min(w * per, ntiles), min(w * per + per, ntiles))) for w in range(grid)]
    return [list(range(w, ntiles, grid)) for w in range(grid)]


def launch_rows(n, n_cols, knobs, cus, mistake=None):
    """per column the row numbers the launch reads, in one common order (row i of column 0 meets the i-th entry
    of every other column)"""
    T = knobs["GROUP_THREADS"]
    tile = tile_rows(n_cols, T)
    grid, ntiles = launch_grid(n, n_cols, knobs, cus), n // tile
    out = []
    for w, tiles in enumerate(workgroup_tiles(n, n_cols, knobs, cus)):
        for i, t in enumerate(tiles):
            if mistake == "second_tile_skipped" and i == 1:
                continue
            # lane tid holds rows k * T + tid of the tile, k < rows per lane
            k, tid = np.meshgrid(np.arange(rows_per_lane(n_cols)), np.arange(T), indexing="ij")
            out.append((t * tile + k * T + tid).ravel())
        if mistake != "tail_dropped":
            # rows past the last whole tile: lane tid takes rows first + tid + j * grid * T
            first = ntiles * tile + w * T
            i = np.arange(first, n)
            out.append(i[(i - first) % (grid * T) < T])
    rows = np.concatenate(out).astype(np.int64) if out else np.zeros(0, np.int64)
    cols = [rows] * n_cols
    if mistake == "col1_row_off":
        cols = [rows, np.minimum(rows + 1, n - 1)] + [rows] * (n_cols - 2)
    return cols


def launch_expected(spec, host, keep, knobs, cus, mistake=None):
    """the table the restated launch gives"""
    n = len(host[0])
    cols = launch_rows(n, spec.K, knobs, cus, mistake)
    return reference(spec, host, keep, cols_rows=cols, key_col=(1, 0) if mistake == "key_col0" else None,
                     pred_swap=(0, 1) if mistake == "pred_wrong_col" else None)


# ---------------------------------------------------------------------------
# the specs
# ---------------------------------------------------------------------------
def u_full(rng, n):
    return rng.integers(0, 1 << 64, n, dtype=np.uint64)


def u_small(rng, n, top=1 << 40):
    return rng.integers(0, top, n, dtype=np.uint64)


def f_exact(rng, n, nan_rate=0.0):
    """multiples of 1/8 in [-4096, 4096): 2^16 values; a group's sum stays far below 2^53 / 8"""
    v = rng.integers(-(1 << 15), 1 << 15, n).astype(np.float64) / 8.0
    if nan_rate and n:
        v[rng.random(n) < nan_rate] = np.nan
    return v


def pool_keys(rng, n, count, with_e1):
    pool = rng.integers(0, 1 << 64, count, dtype=np.uint64)
    if with_e1:
        pool[0] = np.uint64(E1)
    x = pool[rng.integers(0, count, n)]
    if with_e1 and n:
        x[0] = x[n - 1] = np.uint64(E1)
    return x


def make_specs(lds_kb=SMALL_LDS_KB):
    """the shapes of the GPU tests; S of the small knob set sizes the keys"""
    S1, S3, S8 = lds_slots(1, lds_kb), lds_slots(3, lds_kb), lds_slots(8, lds_kb)
    specs = []
    # K = 2: a dense key of column 0 with d = S; count, sum(b), max(b)
    specs.append(Spec(
        "k2_dense", [U, U], lambda rng, n: [u_full(rng, n), u_small(rng, n)],
        ([("%", S3)], R.Arith("%", fld(0), const(S3))),
        [(COUNT, U, None, None), (SUM, U, [load(1)], fld(1)), (MAX, U, [load(1)], fld(1))]))
    # d = S + 1: hashed, and more groups than 3/4 S -- the bypass to the HBM table; one aggregate, no count
    specs.append(Spec(
        "k2_dense1", [U, U], lambda rng, n: [u_full(rng, n), u_small(rng, n)],
        ([("%", S1 + 1)], R.Arith("%", fld(0), const(S1 + 1))),
        [(SUM, U, [load(1)], fld(1))]))
    # dense without a count state (the key is stored), d = S, one aggregate, a bitmap
    specs.append(Spec(
        "k2_dense_nocount", [U, I], lambda rng, n: [u_full(rng, n), u_full(rng, n).view(np.int64)],
        ([("%", S1)], R.Arith("%", fld(0), const(S1))),
        [(MIN, I, [load(1)], fld(1))], ("bitmap", 0.5)))
    # the key is column 1 (Int64) by load(1); arguments without steps take column 0
    specs.append(Spec(
        "k2_key1", [U, I], lambda rng, n: [u_small(rng, n), rng.integers(-40, 40, n).astype(np.int64)],
        ([load(1)], fld(1)),
        [(COUNT, U, None, None), (SUM, U, None, fld(0)), (MIN, U, None, fld(0))]))
    # a key over two columns, (a + b) % 1000: hashed, 1000 groups > 3/4 S; WHERE a < b
    specs.append(Spec(
        "k2_expr", [U, U], lambda rng, n: [u_full(rng, n), u_full(rng, n)],
        ([("+", Col(1)), ("%", 1000)], R.Arith("%", R.Arith("+", fld(0), fld(1)), const(1000))),
        [(COUNT, U, None, None), (SUM, U, [load(1)], fld(1)), (MAX, U, None, fld(0))],
        ("expr", ([], "<", Col(1)), R.Compare("<", fld(0), fld(1)))))
    # column 0 itself as a hashed key, the empty marker 2^64 - 1 among them and kept; a bitmap
    specs.append(Spec(
        "k2_marker", [U, U], lambda rng, n: [pool_keys(rng, n, 100, True), u_small(rng, n)],
        (None, fld(0)),
        [(SUM, U, [load(1)], fld(1))], ("bitmap", 0.7)))
    # K = 3, the Q1 shape: eight aggregates with UInt64, Int64 and Float64 states, b * c with stack steps, an
    # and/or tree whose leaves read different columns; dense key d = S
    bc = [load(1), push(2), ("*", STACK, True)]
    specs.append(Spec(
        "k3_q1", [U, U, F], lambda rng, n: [u_full(rng, n), u_small(rng, n, 1 << 10), f_exact(rng, n)],
        ([("%", S8)], R.Arith("%", fld(0), const(S8))),
        [(COUNT, U, None, None), (SUM, U, [load(1)], fld(1)), (SUM, F, bc, R.Arith("*", fld(1), fld(2))),
         (SUM, F, [load(2)], fld(2)), (MAX, F, [load(2)], fld(2)), (MIN, F, [load(2)], fld(2)),
         (MAX, I, [load(1), ("-", (500, I))], R.Arith("-", fld(1), const(500, I))),
         (MIN, I, [load(1), ("-", (500, I))], R.Arith("-", fld(1), const(500, I)))],
        ("tree", ([([load(2)], "<", 1024.0), ([("%", 8)], "<", 5), ([load(1)], ">", 100)], [0, 1, 2, "or", "and"]),
         R.Logic("and", R.Compare("<", fld(2), const(1024.0, F)),
                 R.Logic("or", R.Compare("<", R.Arith("%", fld(0), const(8)), const(5)),
                         R.Compare(">", fld(1), const(100)))))))
    # K = 4: a hashed key from column 3 with more groups than 3/4 S (the bypass, and key partitions in later
    # launches); Int64 and Float64 states with NaNs; WHERE b < c compares an Int64 with a Float64 column
    specs.append(Spec(
        "k4", [U, I, F, U],
        lambda rng, n: [u_small(rng, n), rng.integers(-5000, 5000, n).astype(np.int64), f_exact(rng, n, 0.3),
                        pool_keys(rng, n, 3 * S3, False)],
        ([load(3)], fld(3)),
        [(COUNT, U, None, None), (SUM, I, [load(1)], fld(1)), (MAX, F, [load(2)], fld(2))],
        ("expr", ([load(1)], "<", Col(2)), R.Compare("<", fld(1), fld(2)))))
    return specs


def zero_spec(kept):
    """sum(1000 / (b - 7)) WHERE a % 8 < 3 over two columns; b is 7 on one row, which the predicate keeps
    (the error at count()) or drops (no error)"""
    def draw(rng, n):
        a = u_full(rng, n)
        b = np.arange(100, 100 + n, dtype=np.uint64)
        if n:
            r = n // 2
            b[r] = 7
            a[r] = (a[r] & ~np.uint64(7)) | np.uint64(1 if kept else 6)
        return [a, b]
    return Spec(
        "zero_kept" if kept else "zero_dropped", [U, U], draw,
        ([("%", 100)], R.Arith("%", fld(0), const(100))),
        [(COUNT, U, None, None),
         (SUM, U, [load(1), ("-", 7), ("/", 1000, True)], R.Arith("/", const(1000), R.Arith("-", fld(1), const(7))))],
        ("expr", ([("%", 8)], "<", 3), R.Compare("<", R.Arith("%", fld(0), const(8)), const(3))))


_DATA = {}


def data(spec, n, seed=0):
    """(host columns, bitmap keep bits or None) of the spec at n rows; the same arrays every time"""
    k = (spec.name, n, seed)
    if k not in _DATA:
        rng = np.random.default_rng([0x6763, seed, n, sum(map(ord, spec.name))])
        host = [np.ascontiguousarray(h, NPT[t]) for h, t in zip(spec.draw(rng, n), spec.dts)]
        keep = rng.random(n) < spec.pred[1] if spec.pred_kind() == "bitmap" else None
        _DATA[k] = (host, keep)
    return _DATA[k]


def sizes(n_cols, threads, grid_cap):
    """0, 1, 3, around one tile, and two rounds of the capped grid plus half a tile and 3 rows"""
    t = tile_rows(n_cols, threads)
    return [0, 1, 3, t - 1, t, t + 1, 2 * grid_cap * t + t // 2 + 3]
