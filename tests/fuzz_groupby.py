"""Generator of random GROUP BY cases and their reference (no test of its own;
imported by tests/test_fuzz_groupby_cpu.py, tests/test_fuzz_groupby_gpu.py and
tests/test_groupby_small_gpu.py the way tests/fuzz_typed.py is).

generate(seed, cus) deterministically draws one Case: a launch-shape knob set
(the defaults, or "small": 256 threads and an 8 KB LDS table, so a tile is
2,048 rows and an LDS table has 512 / 256 / 128 / 64 slots for 1 / 3 / 7 / 8
aggregates), one 64-bit column (type, length tier, 16- or 8-byte alignment,
data class), a key chain, a predicate (none, one comparison, an and/or tree, a
bitmap), one to eight aggregates and a list of plans: executions of the same
logical query that must all end with the same table (one direct launch, the
radix-partitioned entry, narrow rows, the column split into blocks accumulated
into one table, two tables merged).  Every chain is one abstract step list
lowered twice: dev_chain() builds the fq_expr through fq_amd.expr, ref_chain()
the oracle/fq_ref.py function tree; the types both state are asserted equal.
reference() evaluates the chains with fq_ref and groups on the host with a
stable sort and reduceat.

Seed s aims at TARGETS[s % 16], one branch boundary of the kernels each (what
tests/test_fuzz_groupby_cpu.py counts), and draws everything else freely.

What the generator cannot reach: a Float64 column.  The key of a table is
UInt64 or Int64, numerical_coercion makes every step over a Float64 column
Float64 and fq_expr has no cast step, so fq_group_aggregate refuses every such
shape ("key expression is Float64"); a seed that draws one is redrawn from a
sub-seed (Case.refused counts it).  Float64 states, with +-inf, +-0.0 and NaN,
come from value chains over the integer columns.  The length tier of two
tiles per workgroup is drawn at the small knob set only (at the defaults it is
4.2 million rows; tests/test_groupby_gpu.py runs those sizes)."""
import numpy as np

import fq_ref as R
from fq_amd import abi
from fq_amd._lib import FQError
from fq_amd.expr import chain, pred_tree, predicate

U, I, F = "UInt64", "Int64", "Float64"
DT = abi.DT_BY_NAME
NPT = {U: np.uint64, I: np.int64, F: np.float64}
E1 = 0xFFFFFFFFFFFFFFFF
DIV_ZERO = "Internal Error: Divide by zero error"
DEFAULTS = {"GROUP_THREADS": 1024, "GROUP_LDS_KB": 128, "GROUP_WG_PER_CU": 1, "GROUP_CLUSTER": 160,
            "GROUP_CHUNKED": 1, "GROUP_RANGE_BINS": 1, "GROUP_NARROW": 1}
SMALL = {"GROUP_THREADS": 256, "GROUP_LDS_KB": 8}
TARGETS = ["dense_S", "dense_S1", "saturate", "chain", "clustered2", "range_bins", "hash_bins", "narrow_direct",
           "narrow_staged", "second_launch", "merge", "empty_marker", "cap22", "short_chunk", "zero_dropped",
           "zero_kept"]
# the targets that need kept rows to mean anything
BOUNDARY_TARGETS = ("dense_S", "dense_S1", "range_bins", "hash_bins", "narrow_direct", "narrow_staged", "clustered2",
                    "short_chunk", "cap22")
SMALL_LENGTHS = {"merge": 0, "empty_marker": 1, "dense_S1": 2, "cap22": 3}
KINDS = [abi.AGG_COUNT, abi.AGG_SUM, abi.AGG_MAX, abi.AGG_MIN]
MAX_GROUPS = 1 << 18


def small_knobs(**more):
    k = dict(DEFAULTS)
    k.update(SMALL)
    k.update(more)
    return k


def apply_knobs(ops, knobs):
    ops.tune_reset()
    for name, v in knobs.items():
        ops.tune_set(name, v)


def lds_slots(n_aggs, lds_kb):
    """fq_jit.hip lds_slots: the largest power of two S <= 16,384 whose keys and states fit the budget"""
    s = 16384
    while s > 64 and s * 8 * (1 + n_aggs) > lds_kb * 1024:
        s >>= 1
    return s


def lds_home(keys, S):
    """fq_jit.hip lds_hash & (S - 1): the LDS slot a key's probe starts at (hashed shapes)"""
    k = np.asarray(keys, np.uint64)
    f = (k & np.uint64(0xFFFFFFFF)).astype(np.uint32) ^ (k >> np.uint64(32)).astype(np.uint32)
    log2s = int(S).bit_length() - 1
    g = ((f >> np.uint32(log2s)).astype(np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    return ((f.astype(np.uint64) + (g >> np.uint64(32 - log2s))) & np.uint64(S - 1)).astype(np.int64)


# ---------------------------------------------------------------------------
# chains: [(sym, value, type name, reversed)], lowered twice
# ---------------------------------------------------------------------------
def dev_chain(col_t, steps):
    """(fq_expr or None, type name)"""
    if not steps:
        return None, col_t
    e, out = chain(DT[col_t], [(s, (v, t), True) if rev else (s, (v, t)) for s, v, t, rev in steps])
    return e, abi.DT_NAMES[out]


def ref_chain(steps, plain=R.Arith):
    acc = R.Field("c0")
    for s, v, t, rev in steps:
        k = R.Const(R.Value(t, v))
        acc = plain(s, k, acc) if rev else plain(s, acc, k)
    return acc


def chain_type(col_t, steps):
    e, t = dev_chain(col_t, steps)
    assert t == ref_chain(steps).return_type({"c0": col_t}), (col_t, steps)
    return t


def eval_chain(col_t, steps, x):
    """the chain over the rows x with the reference's arithmetic (raises R.RefError on a zero divisor)"""
    if not steps or len(x) == 0:
        t = chain_type(col_t, steps)
        return (x if not steps else np.zeros(0, NPT[t])), t
    with np.errstate(all="ignore"):
        a = ref_chain(steps).eval(R.Block([("c0", R.Arr(col_t, x))]))
    assert a.valid is None or np.all(a.valid), ("a cast gave nulls", col_t, steps)
    return a.values, a.type


class Leaf:
    def __init__(self, steps, sym, value, t):
        self.steps, self.sym, self.value, self.t = steps, sym, value, t

    def __repr__(self):
        return "%r %s %r:%s" % (self.steps, self.sym, self.value, self.t)


class Query:
    """One logical GROUP BY over one host column: what the plans execute and reference() evaluates.
    x: the column's rows; offset: 0 (16-byte aligned) or 1 (the device column starts 8 bytes into its buffer);
    pred_kind "none" | "expr" | "tree" | "bitmap"; keep: a bitmap predicate's bits; aggs: [(kind, state type
    name, steps)]"""

    def __init__(self, col_t, x, key_steps, aggs, pred_kind="none", leaves=(), prog=(), keep=None, offset=0):
        self.col_t, self.x, self.key_steps, self.aggs = col_t, np.ascontiguousarray(x, NPT[col_t]), key_steps, aggs
        self.pred_kind, self.leaves, self.prog, self.keep, self.offset = pred_kind, list(leaves), list(prog), keep, offset
        self.key_t = chain_type(col_t, key_steps)
        assert self.key_t in (U, I), self.key_t
        for kind, t, steps in aggs:
            assert kind == abi.AGG_COUNT and t == U or chain_type(col_t, steps) == t, (kind, t, steps)

    @property
    def n(self):
        return len(self.x)

    @property
    def n_aggs(self):
        return len(self.aggs)

    def table_aggs(self):
        return [(k, DT[t]) for k, t, _ in self.aggs]

    def device(self):
        """(key fq_expr or None, [value fq_expr or None], fq_pred or None); a bitmap's pointer is set per launch"""
        key = dev_chain(self.col_t, self.key_steps)[0]
        vals = [None if k == abi.AGG_COUNT else dev_chain(self.col_t, s)[0] for k, _, s in self.aggs]
        cdt = DT[self.col_t]

        def lower(lf):
            return [(s, (v, t), True) if rev else (s, (v, t)) for s, v, t, rev in lf.steps]
        pred = None
        if self.pred_kind == "expr":
            lf = self.leaves[0]
            pred = predicate(cdt, lower(lf), lf.sym, (lf.value, lf.t))
            assert abi.DT_NAMES[pred.cmp_dtype] == R.equal_coercion(lf.sym, chain_type(self.col_t, lf.steps), lf.t)
        elif self.pred_kind == "tree":
            pred = pred_tree(cdt, [(lower(lf), lf.sym, (lf.value, lf.t)) for lf in self.leaves], self.prog)
        elif self.pred_kind == "bitmap":
            pred = abi.fq_pred()
            pred.kind = abi.PRED_BITMAP
        return key, vals, pred

    def keep_mask(self, mut=None):
        n = self.n
        if self.pred_kind == "none":
            keep = np.ones(n, bool)
        elif self.pred_kind == "bitmap":
            keep = self.keep.copy()
            if mut == "e" and n % 64:  # the last partial word read as all ones
                keep[n - n % 64:] = True
        else:
            blk = R.Block([("c0", R.Arr(self.col_t, self.x))])
            bits = []
            for lf in self.leaves:
                if n == 0:
                    bits.append(np.zeros(0, bool))
                    continue
                with np.errstate(all="ignore"):
                    a = R.Compare(lf.sym, ref_chain(lf.steps), R.Const(R.Value(lf.t, lf.value))).eval(blk)
                assert a.valid is None or np.all(a.valid)
                bits.append(np.asarray(a.values, bool))
            if self.pred_kind == "expr":
                keep = bits[0]
            else:
                st = []
                for tok in self.prog:
                    if isinstance(tok, str):
                        b, a = st.pop(), st.pop()
                        st.append((a & b) if tok == "and" else (a | b))
                    else:
                        st.append(bits[tok])
                keep = st[0]
        keep = keep.copy()
        if mut == "a" and n:
            keep[n - 1] = False
        if mut == "b" and n and self.offset:
            keep[0] = False
        return keep

    def describe(self):
        return "col=%s n=%d offset=%d key=%r aggs=%r pred(%s)=%r prog=%r" % (
            self.col_t, self.n, self.offset, self.key_steps, self.aggs, self.pred_kind, self.leaves, self.prog)


# ---------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------
class Result:
    """keys: uint64 bits ascending; states: [uint64 bits]; amb: per aggregate None or a mask of the groups
    whose Float64 extreme is a zero with both signs among the kept rows (unspecified sign)"""

    def __init__(self, keys, states, amb):
        self.keys, self.states, self.amb = keys, states, amb

    def canon(self):
        out = [self.keys.tobytes()]
        for s, a in zip(self.states, self.amb):
            s = s.copy()
            if a is not None:  # a Float64 extreme: an unpinned zero is one value, a NaN is a NaN
                s[a] = 0
                s[np.isnan(s.view(np.float64))] = 0x7FF8000000000000
            out.append(s.tobytes())
        return tuple(out)


def fold_rows(q, rows, mut=None):
    """Result of the rows selected by the boolean mask `rows` (kept rows of the query or of one block of it)"""
    x = q.x[rows]
    kv, _ = eval_chain(q.col_t, q.key_steps, x)
    kb = np.ascontiguousarray(kv).view(np.uint64)
    vals = [None if k == abi.AGG_COUNT else eval_chain(q.col_t, s, x)[0] for k, _, s in q.aggs]
    if mut == "c":
        live = kb != np.uint64(E1)
        kb, vals = kb[live], [None if v is None else v[live] for v in vals]
    order = np.argsort(kb, kind="stable")
    k = kb[order]
    if len(k) == 0:
        return Result(np.zeros(0, np.uint64), [np.zeros(0, np.uint64) for _ in q.aggs], [None] * q.n_aggs)
    uniq, start = np.unique(k, return_index=True)
    states, amb = [], []
    for (kind, t, _), v in zip(q.aggs, vals):
        a = None
        if kind == abi.AGG_COUNT:
            s = np.diff(np.append(start, len(k))).astype(np.uint64)
        else:
            v = np.ascontiguousarray(v)[order]
            if kind == abi.AGG_SUM:
                with np.errstate(all="ignore"):
                    # (a Float64 sum starts from +0.0, as the table's states do: a group of -0.0 alone sums to +0.0)
                    s = np.add.reduceat(v, start) + 0.0 if t == F else np.add.reduceat(v.view(np.uint64), start)
            elif t == F:
                # f64::max / f64::min: a NaN is ignored unless every kept row of the group is NaN
                s = (np.fmax if kind == abi.AGG_MAX else np.fmin).reduceat(v, start)
                neg = np.logical_or.reduceat((v == 0) & np.signbit(v), start)
                pos = np.logical_or.reduceat((v == 0) & ~np.signbit(v), start)
                a = (s == 0) & neg & pos
            else:
                if mut == "d" and t == I:
                    v = v.view(np.uint64)  # folded unsigned
                s = (np.maximum if kind == abi.AGG_MAX else np.minimum).reduceat(v, start)
            s = np.ascontiguousarray(s).view(np.uint64)
        states.append(s)
        amb.append(a)
    return Result(uniq, states, amb)


def merge_results(q, a, b, add_extremes=False):
    """b folded into a as fq_group_table_merge does (add_extremes: mutation (f))"""
    keys = np.union1d(a.keys, b.keys)
    ia, ib = np.searchsorted(keys, a.keys), np.searchsorted(keys, b.keys)
    states, amb = [], []
    for j, (kind, t, _) in enumerate(q.aggs):
        view = np.uint64 if (kind in (abi.AGG_COUNT, abi.AGG_SUM) and t != F) or t == U else NPT[t]
        adds = kind in (abi.AGG_COUNT, abi.AGG_SUM) or add_extremes
        if adds:
            ident = 0
        elif t == F:
            ident = np.nan
        else:
            info = np.iinfo(view)
            ident = info.min if kind == abi.AGG_MAX else info.max
        sa, sb = np.full(len(keys), ident, view), np.full(len(keys), ident, view)
        sa[ia], sb[ib] = a.states[j].view(view), b.states[j].view(view)
        with np.errstate(all="ignore"):
            if adds:
                s = sa + sb
            elif t == F:
                s = (np.fmax if kind == abi.AGG_MAX else np.fmin)(sa, sb)
            else:
                s = (np.maximum if kind == abi.AGG_MAX else np.minimum)(sa, sb)
        m = None
        if a.amb[j] is not None or b.amb[j] is not None:
            m = np.zeros(len(keys), bool)
            za, zb = np.zeros(len(keys), bool), np.zeros(len(keys), bool)
            za[ia], zb[ib] = a.states[j].view(np.float64) == 0, b.states[j].view(np.float64) == 0
            m |= za & zb & (sa.view(np.uint64) != sb.view(np.uint64))
            for r, ir in ((a, ia), (b, ib)):
                if r.amb[j] is not None:
                    m[ir] |= r.amb[j]
            m &= s == 0
        states.append(np.ascontiguousarray(s).view(np.uint64))
        amb.append(m)
    return Result(keys, states, amb)


def reference(q, mut=None, merge_cut=None):
    """("ok", Result) | ("err", DIV_ZERO).  mut: a mistake made on the reference's side -- "a" the last row lost,
    "b" row 0 of a misaligned column lost, "c" the key 2^64-1 treated as absent, "d" an Int64 max/min folded
    unsigned, "e" a bitmap's last partial word read as all ones, "f" (with merge_cut) the merge adds extremes,
    "g" a zero divisor on a dropped row raises"""
    keep = q.keep_mask(mut)
    try:
        if mut == "g":
            every = np.ones(q.n, bool)
            for steps in [q.key_steps] + [s for k, _, s in q.aggs if k != abi.AGG_COUNT]:
                eval_chain(q.col_t, steps, q.x[every])
        if merge_cut is not None:
            first = np.arange(q.n) < merge_cut
            return "ok", merge_results(q, fold_rows(q, keep & first, mut), fold_rows(q, keep & ~first, mut),
                                       add_extremes=mut == "f")
        return "ok", fold_rows(q, keep, mut)
    except R.RefError as e:
        assert "Divide by zero" in str(e), str(e)
        return "err", DIV_ZERO


def same(got, exp):
    """None, or what differs between a device table (keys, states as extract() gives them) and a Result"""
    keys, states = got
    o = np.argsort(keys, kind="stable")
    keys, states = keys[o], [s[o] for s in states]
    if not np.array_equal(keys, exp.keys):
        extra, missing = np.setdiff1d(keys, exp.keys)[:4], np.setdiff1d(exp.keys, keys)[:4]
        return "keys: %d groups, expected %d; unexpected %r, missing %r" % (len(keys), len(exp.keys), extra, missing)
    for j, (g, e, a) in enumerate(zip(states, exp.states, exp.amb)):
        ok = g == e
        gf, ef = g.view(np.float64), e.view(np.float64)
        if a is not None:  # a Float64 max / min: NaN equals NaN, an unpinned zero by value
            ok |= np.isnan(gf) & np.isnan(ef)
            ok |= a & (gf == 0)
        if not ok.all():
            i = int(np.flatnonzero(~ok)[0])
            return "aggregate %d, key %#x: got %#x expected %#x (%d groups differ)" % (
                j, int(keys[i]), int(g[i]), int(e[i]), int((~ok).sum()))
    return None


def tables_equal(a, b, exp):
    """two device tables key for key and bit for bit (but the zeros whose sign is unspecified, and NaN = NaN)"""
    return same(a, Result(np.sort(b[0]), [s[np.argsort(b[0], kind="stable")] for s in b[1]], exp.amb))


# ---------------------------------------------------------------------------
# plans and their execution (GPU)
# ---------------------------------------------------------------------------
class Plan:
    """kind "direct" | "part" | "blocks" | "merge"; paths: per block ("direct",) | ("part", log2p, narrow);
    cuts: the blocks' first rows after row 0; capacity: slots of the table(s)"""

    def __init__(self, kind, paths, cuts=(), capacity=64):
        self.kind, self.paths, self.cuts, self.capacity = kind, list(paths), list(cuts), capacity

    def __repr__(self):
        return "%s%r cuts=%r cap=%d" % (self.kind, self.paths, self.cuts, self.capacity)

    def bounds(self, n):
        edges = [0] + list(self.cuts) + [n]
        return list(zip(edges[:-1], edges[1:]))


def keep_words(keep):
    bits = np.zeros(((len(keep) + 63) // 64) * 64 + 64, bool)
    bits[:len(keep)] = keep
    return np.packbits(bits, bitorder="little").view(np.uint64)


def execute(ops, q, plan):
    """the plan on the GPU -> (keys, states) of its table; FQError from count() propagates"""
    key, vals, pred = q.device()
    cdt = DT[q.col_t]
    base = ops.from_numpy(np.concatenate([np.zeros(q.offset, q.x.dtype), q.x, np.zeros(2, q.x.dtype)]), cdt)
    kdt = DT[q.key_t]
    tables = [ops.GroupTable(plan.capacity, q.table_aggs(), kdt)]
    if plan.kind == "merge":
        tables.append(ops.GroupTable(plan.capacity, q.table_aggs(), kdt))
    alive = []
    for b, ((lo, hi), path) in enumerate(zip(plan.bounds(q.n), plan.paths)):
        col = ops.DeviceColumn(base.buf, hi - lo, cdt, 8 * (q.offset + lo))
        p = pred
        if q.pred_kind == "bitmap":
            p = abi.fq_pred()
            p.kind = abi.PRED_BITMAP
            bm = ops.from_numpy(keep_words(q.keep[lo:hi]), abi.DT_UINT64)
            p.bitmap = bm.ptr
            alive.append(bm)
        t = tables[b] if plan.kind == "merge" else tables[0]
        if path[0] == "direct":
            t.aggregate(col, p, key, vals)
        else:
            t.aggregate(col, p, key, vals, log2_parts=path[1], narrow=path[2])
        alive.append(getattr(t, "_ws", None))
    if plan.kind == "merge":
        k, s = tables[1].extract()
        tables[0].merge(k, s)
    out = tables[0].extract()
    del alive
    return out


# ---------------------------------------------------------------------------
# host restatement of the launch geometry (for the coverage accounting)
# ---------------------------------------------------------------------------
def direct_geometry(n, head, knobs, cus):
    """(grid, ntiles, tile rows) of fq_group_aggregate's launch over n rows (no key partitions)"""
    T = knobs["GROUP_THREADS"]
    nvec = (n - head) // 2
    grid = min(max(1, -(-nvec // (4 * T))), cus * knobs["GROUP_WG_PER_CU"])
    return grid, nvec // (4 * T), 8 * T


def workgroup_tiles(n, head, knobs, cus):
    """[[tile numbers] per workgroup] of the direct launch"""
    grid, ntiles, _ = direct_geometry(n, head, knobs, cus)
    if knobs["GROUP_CHUNKED"]:
        per = -(-ntiles // grid)
        return [list(range(min(w * per, ntiles), min(w * per + per, ntiles))) for w in range(grid)]
    return [list(range(w, ntiles, grid)) for w in range(grid)]


def workgroup_load(key_bits, keep, n, head, knobs, cus, S):
    """(the most distinct kept keys any workgroup's tiles hold, the most of them that start their LDS probe at
    one slot, the most tiles a workgroup has); the rows past the last whole tile are left out"""
    _, ntiles, tile = direct_geometry(n, head, knobs, cus)
    distinct = chain_len = most = 0
    for tiles in workgroup_tiles(n, head, knobs, cus):
        most = max(most, len(tiles))
        if not tiles:
            continue
        rows = np.concatenate([np.arange(head + t * tile, head + (t + 1) * tile) for t in tiles])
        keys = np.unique(key_bits[rows[keep[rows]]])
        distinct = max(distinct, len(keys))
        if len(keys):
            chain_len = max(chain_len, int(np.bincount(lds_home(keys, S), minlength=S).max()))
    return distinct, chain_len, most


def stages_narrow(key_steps):
    """fq_jit.hip group_stage_narrow for a range-binned key: the steps before the last"""
    for s, v, t, rev in key_steps[:-1]:
        if rev or t == F or not (s in "+-/" or (s == "*" and 0 <= v <= 16)):
            return True
    return False


def key_range(q):
    """d of a UInt64 key ending in `% d` (fq_jit.hip group_key_range), else 0"""
    if q.key_t != U or not q.key_steps:
        return 0
    s, v, t, rev = q.key_steps[-1]
    return int(v) if s == "%" and not rev and t == U and v >= 1 else 0


# ---------------------------------------------------------------------------
# drawing a case
# ---------------------------------------------------------------------------
class Case:
    def __init__(self, seed, target, knobs, q, plans, S, tile, data_class, tier, log2p, zero, refused):
        self.seed, self.target, self.knobs, self.q, self.plans = seed, target, knobs, q, plans
        self.S, self.tile, self.data_class, self.tier, self.log2p, self.zero, self.refused = \
            S, tile, data_class, tier, log2p, zero, refused
        self._ref = {}

    def expected(self, mut=None, merge_cut=None):
        k = (mut, merge_cut)
        if k not in self._ref:
            self._ref[k] = reference(self.q, mut, merge_cut)
        return self._ref[k]

    def describe(self):
        return "seed %d (%s) knobs=%r S=%d class=%s tier=%s | %s | plans=%r" % (
            self.seed, self.target, {k: v for k, v in self.knobs.items() if DEFAULTS[k] != v}, self.S,
            self.data_class, self.tier, self.q.describe(), self.plans)

    def fingerprint(self):
        q = self.q
        key, vals, pred = q.device()
        d = b"".join(b"-" if e is None else bytes(e) for e in [key] + vals)
        if pred is not None and q.pred_kind in ("expr", "tree"):
            d += bytes(pred.lhs) + (bytes(pred._tree) if q.pred_kind == "tree" else b"") + \
                repr((pred.cmp, pred.cmp_dtype, pred.rhs_bits)).encode()
        return (self.describe(), d, q.x.tobytes(), b"" if q.keep is None else np.packbits(q.keep).tobytes())


def colliding_keys(rng, S, count):
    """`count` keys congruent modulo S whose LDS probes start at one slot"""
    k0 = int(rng.integers(0, S))
    cand = np.uint64(k0) + np.uint64(S) * np.arange(1, 80 * S, dtype=np.uint64)
    home = lds_home(cand, S)
    slot = np.bincount(home, minlength=S).argmax()
    out = cand[home == slot][:count]
    assert len(out) == count
    return out


def draw_data(rng, col_t, n, cls, tile, S, positive):
    """the column's rows as uint64 bits"""
    top = 63 if positive else 64
    if n == 0:
        return np.zeros(0, np.uint64)
    if cls == "scattered":
        x = rng.integers(0, 1 << top, n, dtype=np.uint64)
    elif cls == "sorted":
        pool = rng.integers(0, 1 << top, n // 4 + 1, dtype=np.uint64)
        x = pool[rng.integers(0, len(pool), n)]
        x = np.sort(x.view(NPT[col_t])).view(np.uint64)
    elif cls == "clustered":
        lens = []
        while sum(lens) < n:
            m = rng.integers(1, 301, 256)
            m[rng.random(256) < 0.01] = int(rng.integers(tile + 1, 2 * tile))
            lens.extend(m.tolist())
        x = np.repeat(rng.integers(0, 1 << top, len(lens), dtype=np.uint64), lens)[:n]
    elif cls == "consecutive":
        firsts = [0, 5, 2**31 - 10, 2**40 - 1000]
        if col_t == I:
            firsts += [-(n // 2), -(2**40)]
        elif not positive:
            firsts += [2**64 - 2**31 + 77, 2**64 - 1500]
        first = int(firsts[int(rng.integers(len(firsts)))])
        x = (np.uint64(first & E1) + np.arange(n, dtype=np.uint64))
        if first == 2**64 - 1500:  # through zero, and begun in the middle: col[0] is small, rows lie below it modulo 2^64
            x = np.roll(x, -min(n // 2, 2000))
    elif cls == "pool":  # (the second_launch target) 2S .. 8S keys, the first rows all distinct: one tile saturates
        pool = rng.integers(0, 1 << top, int(rng.integers(2 * S, 8 * S + 1)), dtype=np.uint64)
        x = np.concatenate([pool[:n], pool[rng.integers(0, len(pool), max(0, n - len(pool)))]])
    else:  # "collisions": 40 keys on one LDS slot among 50 others
        pool = np.concatenate([colliding_keys(rng, S, 40), rng.integers(0, 1 << 32, 50, dtype=np.uint64)])
        x = pool[rng.integers(0, len(pool), n)]
    return np.ascontiguousarray(x, np.uint64)


def plant_specials(rng, x, tile, positive, force_e1):
    n = len(x)
    sp = [2**63 - 1, 0, 1] if positive else [E1, 2**63, 2**63 - 1, 2**63 + 5, E1 - 1, 0]
    rows = sorted({0, min(n - 1, tile // 2), min(n - 1, (n // tile) * tile + 1), max(0, n - 2), n - 1})
    for r in rows:
        x[r] = np.uint64(sp[int(rng.integers(len(sp)))])
    if force_e1:
        x[0] = x[n - 1] = np.uint64(E1)


def draw_key(rng, col_t, S, log2p, target, force_mod):
    steps = []
    ct = col_t
    pre = int(rng.integers(0, 3)) if rng.random() < 0.9 else 7
    if target in ("chain", "empty_marker", "merge", "saturate", "second_launch", "clustered2"):
        pre = 0
    if target == "narrow_direct":
        steps, pre = ([("/", 3, U, False)] if rng.random() < 0.5 else []), 0
    if target == "narrow_staged":
        steps, pre = [("*", 17, U, False)], 0
    for _ in range(pre):
        r = rng.random()
        if r < 0.3:
            steps.append(("/", [3, 1000, 7][int(rng.integers(3))], ct, False))
        elif r < 0.6:
            steps.append(("*", [3, 16, 17, 7919][int(rng.integers(4))], ct, False))
        elif target in ("dense_S", "dense_S1", "range_bins", "hash_bins"):
            steps.append(("+", int(rng.integers(1, 100)), ct, False))
        else:
            sym, v = "+-"[int(rng.integers(2))], int(rng.integers(-1000, 1000))
            # an Int64 step casts what the UInt64 steps before it gave, and after `*` or `+` that may be past 2^63
            # (a cast null): there the Int64 step goes first, and every later step is Int64 arithmetic
            grown = ct == U and any(s in "*+" for s, _, _, _ in steps)
            steps.insert(0 if grown else len(steps), (sym, v, I, False))
            ct = I
    ds = {"dense_S": S, "dense_S1": S + 1, "range_bins": (S << log2p), "hash_bins": (S << log2p) + 1,
          "narrow_direct": S << log2p, "narrow_staged": S << log2p}
    if target in ds:
        steps.append(("%", ds[target], U, False))
    elif force_mod or (pre < 7 and rng.random() < 0.5 and target not in ("chain", "empty_marker", "merge",
                                                                         "saturate", "second_launch")):
        d = [S - 1, S, S + 1, S << log2p, (S << log2p) + 1, 1000, 7][int(rng.integers(7))]
        steps.append(("%", d, U, False))
    return steps[:abi.MAX_STEPS]


F_EXACT = [("%", 1024, U, False), ("*", 0.25, F, False)]
F_CHAINS = [[("*", 0.5, F, False)], F_EXACT, [("*", 1e308, F, False), ("*", 1e308, F, False)],
            [("*", 1e308, F, False), ("*", 1e308, F, False), ("*", 0.0, F, False)], [("*", -0.0, F, False)],
            [("%", 7, U, False), ("*", -0.0, F, False)]]


def draw_aggs(rng, col_t, n_aggs, with_count, full_range):
    aggs = []
    for a in range(n_aggs):
        kind = KINDS[int(rng.integers(4))]
        if kind == abi.AGG_COUNT and not with_count:
            kind = abi.AGG_SUM
        if kind == abi.AGG_COUNT:
            aggs.append((kind, U, []))
            continue
        r = rng.random()
        if r < 0.4:
            steps = [] if rng.random() < 0.6 else [("+", 1, col_t, False)]
        elif r < 0.47 and not full_range:
            # (2^62: about half of a full-range column's values go negative)
            steps = [("-", [1 << 62, int(rng.integers(0, 1 << 40)), 7][int(rng.integers(3))], I, False)]
        elif r < 0.55:  # values on both sides of zero whatever the column holds
            steps = [("%", 1000, col_t, False), ("-", 500, I, False)]
        elif r < 0.65:
            steps = [("/", 3, col_t, False)]
        else:
            steps = list(F_CHAINS[int(rng.integers(len(F_CHAINS)))])
        aggs.append((kind, chain_type(col_t, steps), steps))
    if with_count and not any(k == abi.AGG_COUNT for k, _, _ in aggs):
        aggs[int(rng.integers(n_aggs))] = (abi.AGG_COUNT, U, [])
    return aggs


def casts_column(steps):
    """an Int64 step of a chain over a UInt64 column meets a value that `% d` has not bounded"""
    for s, v, t, rev in steps:
        if s == "%" and t == U and not rev:
            return False
        if t == I:
            return True
    return False


def exactly_summable(v):
    """every value a multiple of one power of two q with sum(|v|) < 2^53 q: the sum is exact in any order"""
    if len(v) == 0:
        return True
    if not np.all(np.isfinite(v)):
        return False
    nz = v[v != 0]
    if len(nz) == 0:
        return True
    m, e = np.frexp(np.abs(nz))
    mant = (m * 2.0 ** 53).astype(np.uint64)
    low = mant & (~mant + np.uint64(1))
    q = 2.0 ** float((e - 53 + np.log2(low.astype(np.float64)).astype(np.int64)).min())
    return float(np.abs(nz).sum()) < 2.0 ** 52 * q  # (a factor of two for the rounding of this very sum)


def draw_pred(rng, col_t, x, kind, rate):
    n = len(x)
    if kind == "bitmap":
        return [], [], rng.random(n) < rate
    leaves = []
    k = 1 if kind == "expr" else int(rng.integers(2, abi.MAX_PRED_LEAVES + 1))
    for i in range(k):
        m = [100, 997, 64, 13][int(rng.integers(4))]
        steps = ([("/", 3, col_t, False)] if rng.random() < 0.3 else []) + [("%", m, col_t, False)]
        v, t = eval_chain(col_t, steps, x)
        if n == 0:
            c = 1
        elif rate == 0.0 and kind == "expr":
            c = int(v.min())
        else:
            c = int(np.sort(v)[min(n - 1, int(rate * n))])
        leaves.append(Leaf(steps, "<" if rate == 0.0 else "<=", c, t))
    prog = []
    if kind == "tree":
        prog = [0]
        for i in range(1, k):
            prog += [i, "and" if rng.random() < 0.5 else "or"]
    return leaves, prog, None


def plant_zero(rng, q, kept, consecutive):
    """a zero divisor on a kept row (kept=True) or on dropped rows only: a chain 1000 / (x - x[r]) as the key or
    as one aggregate's argument.  -> the place, or None when no row serves"""
    keep = q.keep_mask()
    rows = np.flatnonzero(keep if kept else ~keep)
    if len(rows) == 0:
        return None
    for _ in range(50):
        r = int(rows[int(rng.integers(len(rows)))])
        hit = q.x == q.x[r]
        if kept or not keep[hit].any():
            break
    else:
        return None
    v0 = int(q.x[r])
    steps = [("-", v0, q.col_t, False), ("/", 1000, q.col_t, True)]
    places = ["key"] + [a for a, (k, _, _) in enumerate(q.aggs) if k != abi.AGG_COUNT]
    where = places[int(rng.integers(len(places)))]
    if where == "key":
        q.key_steps = steps
        q.key_t = chain_type(q.col_t, steps)
    else:
        q.aggs[where] = (q.aggs[where][0], q.col_t, steps)
    return where, v0


def pow2_at_least(v):
    c = 64
    while c < v:
        c *= 2
    return c


def draw_case(rng, seed, cus):
    target = TARGETS[seed % len(TARGETS)]
    two_tiles = target in ("clustered2", "short_chunk")
    small = two_tiles or rng.random() < 0.7
    knobs = small_knobs() if small else dict(DEFAULTS)
    knobs["GROUP_CLUSTER"] = [0, 160, 512][int(rng.integers(3))]
    for name in ("GROUP_CHUNKED", "GROUP_RANGE_BINS", "GROUP_NARROW"):
        knobs[name] = int(rng.integers(2))
    if target == "clustered2":
        knobs["GROUP_CLUSTER"] = [160, 512][int(rng.integers(2))]
    if target == "short_chunk":
        knobs["GROUP_CHUNKED"] = 1
    if target in ("range_bins", "hash_bins", "narrow_direct", "narrow_staged"):
        knobs["GROUP_RANGE_BINS"] = 1
    if target in ("narrow_direct", "narrow_staged"):
        knobs["GROUP_NARROW"] = 1
    col_t = [U, I, F][int(rng.choice(3, p=[0.5, 0.4, 0.1]))]
    if target in ("dense_S", "dense_S1", "range_bins", "hash_bins", "narrow_direct", "narrow_staged", "chain"):
        col_t = U
    n_aggs = [1, 3, 7, 8][seed // len(TARGETS) % 4 if rng.random() < 0.5 else int(rng.integers(4))] \
        if rng.random() < 0.8 else int(rng.integers(1, 9))
    S = lds_slots(n_aggs, knobs["GROUP_LDS_KB"])
    tile = 8 * knobs["GROUP_THREADS"]
    log2p = int(rng.integers(1, 9))
    if S << log2p > MAX_GROUPS // 2:
        log2p = max(1, (MAX_GROUPS // 2 // S).bit_length() - 1)
    # the length tier
    if two_tiles:
        tier, n = "two_tiles", 2 * tile * cus * knobs["GROUP_WG_PER_CU"] + tile + 37
    elif target in ("saturate", "chain", "second_launch", "zero_dropped", "zero_kept") or rng.random() < 0.55:
        tier, n = "several", 20 * tile + int(rng.integers(0, tile))
    else:
        tier = "tiny"
        sizes = [0, 1, 2, 3, tile - 1, tile, tile + 1, 3 * tile + 37]
        n = sizes[int(rng.integers(4 if target in BOUNDARY_TARGETS + ("empty_marker", "merge") else 0, len(sizes)))]
    # columns of 0 .. 3 rows: every other seed of four targets
    if seed // len(TARGETS) % 2 == 1 and target in SMALL_LENGTHS:
        tier, n = "tiny", (SMALL_LENGTHS[target] + seed // (2 * len(TARGETS))) % 4 or (0 if target == "merge" else 1)
    offset = int(rng.integers(2))
    # the data class
    classes = ["scattered", "clustered", "sorted", "consecutive", "collisions"]
    cls = classes[int(rng.integers(5))]
    cls = {"saturate": "scattered", "second_launch": "pool", "chain": "collisions", "clustered2": "clustered",
           "narrow_direct": "consecutive", "narrow_staged": "consecutive", "empty_marker": "scattered",
           "merge": "scattered"}.get(target, cls)
    if col_t == F:
        x = rng.uniform(-1e6, 1e6, n)
        key_steps = draw_key(rng, col_t, S, log2p, target, False)
        return ("refused", col_t, x, key_steps, n_aggs)
    with_count = seed % 2 == 0
    key_steps = draw_key(rng, col_t, S, log2p, target, tier == "two_tiles" and cls in ("scattered", "sorted"))
    aggs = draw_aggs(rng, col_t, n_aggs, with_count, col_t == U and target in ("empty_marker", "merge"))
    if target in ("dense_S1", "range_bins", "hash_bins") and (n_aggs > 1 or not with_count):
        # an Int64 max / min over values on both sides of zero, in groups of several rows (`% d` keys)
        a = n_aggs - 1 if aggs[n_aggs - 1][0] != abi.AGG_COUNT or sum(k == abi.AGG_COUNT for k, _, _ in aggs) > 1 else 0
        aggs[a] = (abi.AGG_MAX if seed % 2 else abi.AGG_MIN, I, [("%", 1000, col_t, False), ("-", 500, I, False)])
    # a UInt64 column whose chains mix in Int64 constants is cast to Int64: values below 2^63 only
    every = [key_steps] + [s for _, _, s in aggs]
    positive = col_t == U and any(casts_column(steps) for steps in every)
    bits = draw_data(rng, col_t, n, cls, tile, S, positive)
    specials = n > 0 and cls not in ("consecutive", "collisions") and \
        (target in ("empty_marker", "merge") or rng.random() < 0.4)
    if specials:
        plant_specials(rng, bits, tile, positive, target in ("empty_marker", "merge") and not key_steps)
    x = bits.view(NPT[col_t])
    # exactly summable Float64 sums only
    for a, (kind, t, steps) in enumerate(aggs):
        if kind == abi.AGG_SUM and t == F and not exactly_summable(eval_chain(col_t, steps, x)[0]):
            aggs[a] = (abi.AGG_MAX, t, steps)
    # the predicate
    kind = ["none", "expr", "tree", "bitmap"][int(rng.choice(4, p=[0.3, 0.3, 0.15, 0.25]))]
    rate = [0.01, 0.5, 0.99, 0.0][int(rng.choice(4, p=[0.25, 0.4, 0.25, 0.1]))]
    if rate == 0.0 and target in BOUNDARY_TARGETS:
        rate = 0.5
    if target in ("empty_marker", "merge", "saturate", "second_launch", "chain"):
        kind = "none"
    if target in ("zero_dropped", "zero_kept"):
        kind, rate = ["expr", "bitmap"][int(rng.integers(2))], 0.5
    if target in ("narrow_direct", "short_chunk"):  # bitmaps whose last word is partial and holds dropped rows
        kind, rate = "bitmap", (0.5 if rate == 0.99 else rate)
    leaves, prog, keep = ([], [], None) if kind == "none" else draw_pred(rng, col_t, x, kind, rate)
    q = Query(col_t, x, key_steps, aggs, kind, leaves, prog, keep, offset)
    zero = None
    if target in ("zero_dropped", "zero_kept"):
        planted = plant_zero(rng, q, target == "zero_kept", cls == "consecutive")
        if planted is None:
            return None
        zero = "kept" if target == "zero_kept" else "dropped"
    # the groups, on the host: the tables are sized from them (an error seed: the rows that divide by zero go on
    # with one more key at the most, and a full table would be reported before the zero divisor)
    status, res = reference(q)
    if status == "ok":
        groups = len(res.keys)
    else:
        groups = len(fold_rows(q, q.keep_mask() & (q.x != q.x.dtype.type(planted[1]))).keys) + 2
    if groups > MAX_GROUPS or (groups == 0 and target in BOUNDARY_TARGETS):
        return None
    cap = pow2_at_least(2 * groups)
    if target == "cap22":
        cap = 1 << 22
    # the plans
    narrow_ok = cls == "consecutive" and n > 0
    def path():
        r = rng.random()
        if r < 0.4:
            return ("direct",)
        # (the seed's own log2p or one other: every distinct value is one more module to compile)
        return ("part", log2p if rng.random() < 0.5 else log2p % 8 + 1, bool(narrow_ok and rng.random() < 0.5))
    plans = [Plan("direct", [("direct",)], capacity=cap), Plan("part", [("part", log2p, False)], capacity=cap)]
    if narrow_ok:
        plans.append(Plan("part", [("part", log2p, True)], capacity=cap))
    nb = 3 if target == "second_launch" else int(rng.integers(2, 4))
    if target == "second_launch":
        # one saturated workgroup, then 16 workgroups (a grid every P <= 16 divides), then the rest
        cuts = [tile + offset, tile + offset + 16 * tile]
        plans.append(Plan("blocks", [("direct",)] * 3, cuts, cap))
    else:
        cuts = sorted(int(c) for c in rng.integers(0, n + 1, nb - 1))
        plans.append(Plan("blocks", [path() for _ in range(nb)], cuts, cap))
    plans.append(Plan("merge", [path(), path()], [int(rng.integers(0, n + 1))], cap))
    return Case(seed, target, knobs, q, plans, S, tile, cls, tier, log2p, zero, 0)


_CACHE = {}


def refused_by_lowering(col_t, key_steps, n_aggs):
    """what fq_group_aggregate says to a key that is no integer (a zero-length call: no GPU needed)"""
    from fq_amd import ops
    e, t = dev_chain(col_t, key_steps)
    try:
        ops.group_compile_check(DT[col_t], [(abi.AGG_COUNT, abi.DT_UINT64)] * n_aggs, key=e)
    except FQError as err:
        return err.status == abi.FQ_E_INVALID and "key expression is Float64" in str(err)
    return False


def generate(seed, cus, cache=True):
    """the Case of a seed for a device of `cus` compute units; the same object every time unless cache=False"""
    if cache and (seed, cus) in _CACHE:
        return _CACHE[(seed, cus)]
    refused = 0
    for attempt in range(64):
        rng = np.random.default_rng([0x6B67, seed, attempt])
        c = draw_case(rng, seed, cus)
        if c is None:
            continue
        if isinstance(c, tuple):
            assert refused_by_lowering(c[1], c[3], c[4]), "a Float64 column's key was not refused: %r" % (c[3],)
            refused += 1
            continue
        c.refused = refused
        if cache:
            _CACHE[(seed, cus)] = c
        return c
    raise AssertionError("seed %d: no case in 64 draws" % seed)


# ---------------------------------------------------------------------------
# which branches a case reaches, from the host values alone
# ---------------------------------------------------------------------------
FEATURES = ["dense d == S", "d == S + 1", "workgroup with more than 3S/4 distinct keys", "collision chain > 16",
            "clustered, two tiles per workgroup, GROUP_CLUSTER > 0", "range bins at d == 2^log2p S",
            "hash bins at d == 2^log2p S + 1", "narrow rows stored directly", "narrow rows staged",
            "key partitions (P > 1) in a later launch", "merge", "empty-marker key", "capacity >= 2^22",
            "short or empty last GCHUNK run", "zero divisor on dropped rows only", "zero divisor on a kept row"]


def features(c, cus):
    q, k, S = c.q, c.knobs, c.S
    out = set()
    status, res = c.expected()
    if c.zero:
        out.add("zero divisor on a kept row" if c.zero == "kept" else "zero divisor on dropped rows only")
        assert (status == "err") == (c.zero == "kept"), c.describe()
    if status != "ok":
        return out
    keep = q.keep_mask()
    d = key_range(q)
    dense = 0 < d <= S
    if len(res.keys) and d == S:
        out.add("dense d == S")
    if len(res.keys) and d == S + 1:
        out.add("d == S + 1")
    if len(res.keys) and int(res.keys[-1]) == E1:
        out.add("empty-marker key")
    if any(p.capacity >= 1 << 22 for p in c.plans):
        out.add("capacity >= 2^22")
    key_bits = np.zeros(q.n, np.uint64)
    key_bits[keep] = np.ascontiguousarray(eval_chain(q.col_t, q.key_steps, q.x[keep])[0]).view(np.uint64)
    head = 1 if q.offset and q.n else 0
    if q.n and keep.any():
        distinct, chain_len, most = workgroup_load(key_bits, keep, q.n, head, k, cus, S)
        if not dense and distinct > 3 * S // 4:
            out.add("workgroup with more than 3S/4 distinct keys")
        if not dense and chain_len > 16:
            out.add("collision chain > 16")
        if c.data_class == "clustered" and most >= 2 and k["GROUP_CLUSTER"] > 0:
            out.add("clustered, two tiles per workgroup, GROUP_CLUSTER > 0")
        tiles = workgroup_tiles(q.n, head, k, cus)
        if k["GROUP_CHUNKED"] and sum(len(t) for t in tiles) and len(tiles[-1]) < len(tiles[0]):
            out.add("short or empty last GCHUNK run")
    for p in c.plans:
        seen, saturated = np.zeros(0, np.uint64), False
        for (lo, hi), path in zip(p.bounds(q.n), p.paths):
            kept = keep[lo:hi]
            if not kept.any():
                continue
            keys = np.unique(key_bits[lo:hi][kept])
            if path[0] == "part":
                lp = path[1]
                sh = 0
                while (1 << lp << sh) < d:
                    sh += 1
                ranged = d > 0 and k["GROUP_RANGE_BINS"] and (1 << sh) <= S
                if ranged and d == S << lp:
                    out.add("range bins at d == 2^log2p S")
                if k["GROUP_RANGE_BINS"] and d == (S << lp) + 1:
                    assert not ranged
                    out.add("hash bins at d == 2^log2p S + 1")
                if path[2] and k["GROUP_NARROW"]:
                    out.add("narrow rows stored directly" if ranged and not stages_narrow(q.key_steps)
                            else "narrow rows staged")
            elif p.kind == "blocks" and not dense:
                h = 1 if (q.offset + lo) % 2 else 0
                if saturated and len(seen) > 3 * S // 4:  # fq_jit_groupby: P from the groups claimed so far
                    P = 1
                    while P <= 16 and P * (S // 2) < len(seen):
                        P *= 2
                    if P <= 16 and P > 1 and direct_geometry(hi - lo, h, k, cus)[0] % P == 0:
                        out.add("key partitions (P > 1) in a later launch")
                if workgroup_load(key_bits[lo:hi], kept, hi - lo, h, k, cus, S)[0] >= 3 * S // 4:
                    saturated = True
            if p.kind == "blocks":
                seen = np.union1d(seen, keys)
        if p.kind == "merge":
            cut = p.cuts[0]
            if keep[:cut].any() and keep[cut:].any():
                out.add("merge")
    return out
