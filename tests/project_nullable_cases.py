"""Cases, oracle and kernel model of the Filter -> Projection block stream over
nullable columns (fq_filter_project_blocks_nullable, fq_predicate_bitmap_nullable),
shared by tests/test_project_nullable_cpu.py and tests/test_project_nullable_gpu.py.
Needs no GPU.

A case is one statement over columns that each carry a validity array (or
None): the kernel's fq_pred / fq_exprs, the same filter and expressions as
oracle/fq_ref.py functions, and -- for the model -- as numpy over (values,
validity).

The oracle loops per reference block over R.Block of R.Arr(type, values,
valid): R.filter_block gives the kept rows (a null predicate drops the row);
for a predicate tree the kept mask is the tree's values AND-ed with every leaf
comparison's validity (fq_ref's data_array_logic_op returns no validity where
arrow 2.0 combines the null bitmaps: the rule tests/test_scan_nullable_gpu.py
states); each expression's .values / .valid on the filtered block.  An
out-of-range cast is a null.  Expectations per output: the rows, the output
bitmap as whole words (zeros outside the kept ranges), per-block counts.
Values are compared bit for bit, only where the expected bit is 1, any NaN
equal to any NaN; no tolerance anywhere: one IEEE operation per step.

Every value under a 0 bit is garbage chosen to hurt: zero divisors, NaN and
+-inf, integer extremes outside the shape's casts, values passing the
predicate.

model(): the kernel restated in numpy -- load -> validity -> predicate -> in-tile
rank -> the kept rows' bits staged from bit (first output row) mod 64 -> the
staged words OR-ed into a zeroed bitmap, tile by tile, block by block.  Its
`mistake` argument plants one of MISTAKES, each a way the kernel could be wrong."""
import numpy as np

import fq_ref as R
from fq_amd import abi
from fq_amd.expr import Col, chain_columns, load, pred_tree_columns, predicate_columns

I8, I16, I32, I64 = abi.DT_INT8, abi.DT_INT16, abi.DT_INT32, abi.DT_INT64
U8, U16, U32, U64 = abi.DT_UINT8, abi.DT_UINT16, abi.DT_UINT32, abi.DT_UINT64
F32, F64 = abi.DT_FLOAT32, abi.DT_FLOAT64
REF = {I8: "Int8", I16: "Int16", I32: "Int32", I64: "Int64", U8: "UInt8", U16: "UInt16", U32: "UInt32",
       U64: "UInt64", F32: "Float32", F64: "Float64"}
DT_OF_REF = {v: k for k, v in REF.items()}
NP = {I8: np.int8, I16: np.int16, I32: np.int32, I64: np.int64, U8: np.uint8, U16: np.uint16, U32: np.uint32,
      U64: np.uint64, F32: np.float32, F64: np.float64}
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
DT_OF_NP = {np.dtype(v): k for k, v in NP.items()}
FILL = 0xA5
DIV_ZERO = "Internal Error: Divide by zero error"
MISTAKES = ("bitmap_shifted_one_row", "garbage_read_as_valid", "validity_at_input_position", "block_bits_from_word_start",
            "kleene_or", "bits_past_count_left_set", "plain_store_over_shared_word")


def fld(n):
    return R.Field(n)


def const(v, t):
    return R.Const(R.Value(t, v))


def geometry(dts, out_dts):
    """(rows per thread R, row group G) of fq_scan.h typed_project_geometry; a tile is 256 * R rows"""
    width = sum(np.dtype(NP[d]).itemsize for d in dts)
    wout = max(np.dtype(NP[d]).itemsize for d in out_dts)
    r = 32
    while r > 1 and (r * width > 384 or r * wout > 128):
        r //= 2
    g = 16
    while g > 1 and (g > r or g * width > 128):
        g //= 2
    return r, g


def same(got, want, dt, where=None):
    """bit for bit where `where` (default: everywhere); any NaN equals any NaN"""
    w = np.dtype(NP[dt]).itemsize
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape:
        return False
    sel = np.ones(len(got), bool) if where is None else np.asarray(where, bool)
    g, x = got.view(UINT[w])[sel], want.view(UINT[w])[sel]
    if dt in (F32, F64):
        gn, xn = np.isnan(got[sel]), np.isnan(want[sel])
        return bool(np.array_equal(gn, xn) and np.array_equal(g[~gn], x[~xn]))
    return bool(np.array_equal(g, x))


def pack_bits(bits, pad=False):
    """bool rows -> LSB-first u64 words; pad: the bits past the last row set (an input bitmap's may hold anything)"""
    n = len(bits)
    full = np.full(((n + 63) // 64) * 64, bool(pad))
    full[:n] = bits
    return np.packbits(full, bitorder="little").view(np.uint64) if n else np.zeros(0, np.uint64)


class Case:
    """names, dts, host: the kernel's columns (garbage under nulls included); valid: per column a bool array or
    None (no bitmap); pred / values: the fq_pred and fq_exprs; where (leaves: its comparisons when it is a tree)
    and exprs: the oracle's functions; np_pred(cols, vs, kleene) -> kept rows and np_vals(cols, vs) -> [(values,
    validity)]: the same statement in numpy for model()"""

    def __init__(self, name, names, dts, host, valid, pred, values, where, leaves, exprs, np_pred, np_vals):
        self.name, self.names, self.dts = name, names, dts
        self.host = [np.ascontiguousarray(h) for h in host]
        self.valid = [None if v is None else np.ascontiguousarray(v, dtype=bool) for v in valid]
        self.pred, self.values, self.where, self.leaves, self.exprs = pred, values, where, leaves, exprs
        self.np_pred, self.np_vals = np_pred, np_vals
        self.n = len(self.host[0])
        self._oracle = {}

    def replace(self, host=None, valid=None):
        return Case(self.name, self.names, self.dts, host or self.host, valid if valid is not None else self.valid,
                    self.pred, self.values, self.where, self.leaves, self.exprs, self.np_pred, self.np_vals)

    def block(self, s, e):
        return R.Block([(nm, R.Arr(REF[dt], h[s:e], None if v is None else v[s:e]))
                        for nm, dt, h, v in zip(self.names, self.dts, self.host, self.valid)])

    def keep(self, blk):
        """the oracle's kept rows of a block as a mask (None: every row)"""
        if self.where is None:
            return None
        res = self.where.eval(blk)
        keep = np.array(res.values, bool)
        if res.valid is not None:
            keep &= np.asarray(res.valid, bool)
        for lf in self.leaves or []:  # a tree is null if any leaf is
            lv = lf.eval(blk).valid
            if lv is not None:
                keep &= np.asarray(lv, bool)
        return keep

    def oracle(self, block_rows):
        """{"dts", "counts", "rows": per output the expected rows (FILL elsewhere), "bits": per output the expected
        validity of every output row (False outside the kept ranges), "kept": the rows inside the kept ranges};
        raises R.RefError for a zero divisor with both operands valid"""
        if block_rows in self._oracle:
            return self._oracle[block_rows]
        n = self.n
        br = min(block_rows, n) if n else block_rows
        counts, dts, rows = [], [None] * len(self.exprs), [None] * len(self.exprs)
        kept = np.zeros(n, bool)
        bits = [np.zeros(n, bool) for _ in self.exprs]
        for b, s in enumerate(range(0, n, br)):
            blk = self.block(s, min(s + br, n))
            if self.where is not None and self.leaves is None:
                fb = R.filter_block(self.where, blk)
            else:
                keep = self.keep(blk)
                fb = blk if keep is None else blk.take(keep)
            cnt = fb.num_rows()
            counts.append(cnt)
            kept[s:s + cnt] = True
            for j, e in enumerate(self.exprs):
                v = e.eval(fb)
                dts[j] = DT_OF_REF[v.type]
                if rows[j] is None:
                    rows[j] = np.full(n * np.dtype(NP[dts[j]]).itemsize, FILL, np.uint8).view(NP[dts[j]])
                rows[j][s:s + cnt] = np.ascontiguousarray(v.values, dtype=NP[dts[j]])
                bits[j][s:s + cnt] = True if v.valid is None else np.asarray(v.valid, bool)
        self._oracle[block_rows] = {"dts": dts, "counts": counts, "rows": rows, "bits": bits, "kept": kept}
        return self._oracle[block_rows]

    def oracle_bitmap(self):
        """fq_predicate_bitmap_nullable's rows: the oracle's mask AND the leaf validities, over the whole column"""
        return self.keep(self.block(0, self.n))


# ---------------------------------------------------------------------------
# the kernel, restated
# ---------------------------------------------------------------------------
def model(case, block_rows, mistake=None):
    """{"counts", "rows", "bits"} as Case.oracle gives them, computed the way fq_jit_pblocks does"""
    assert mistake is None or mistake in MISTAKES
    n = case.n
    B = min(block_rows, n) if n else block_rows
    vs = []
    for v in case.valid:  # load -> validity
        if v is None or mistake == "garbage_read_as_valid":
            vs.append(np.ones(n, bool))
        elif mistake == "bitmap_shifted_one_row":
            vs.append(np.append(v[1:], True))  # bit i + 1 for row i; the bits past the last row are set
        else:
            vs.append(v)
    keep = case.np_pred(case.host, vs, mistake == "kleene_or")
    keep = np.ones(n, bool) if keep is None else keep
    vals = case.np_vals(case.host, vs)
    out_dts = [DT_OF_NP[np.dtype(v.dtype)] for v, _ in vals]
    tile = 256 * geometry(case.dts, out_dts)[0]
    nw = (n + 63) // 64
    words = [np.full(nw, ~np.uint64(0) if mistake == "bits_past_count_left_set" else np.uint64(0)) for _ in vals]
    rows = [np.full(n * v.dtype.itemsize, FILL, np.uint8).view(v.dtype) for v, _ in vals]
    counts = []
    for s in range(0, n, B):
        e, carry = min(s + B, n), 0
        for r0 in range(s, e, tile):
            r1 = min(r0 + tile, e)
            k = keep[r0:r1]
            tot = int(k.sum())
            rank = np.cumsum(k) - k  # the in-tile rank of a kept row
            base = s + carry         # the tile's first output row
            first_bit = base if mistake != "block_bits_from_word_start" else ((s >> 6) << 6) + carry
            vsh = first_bit & 63
            for j, (v, ok) in enumerate(vals):
                rows[j][base:base + tot] = v[r0:r1][k]
                stage = np.zeros(tile + 64, bool)  # the zeroed LDS bit stage
                if mistake == "validity_at_input_position":
                    stage[vsh:vsh + tot] = ok[r0:r0 + tot]
                else:
                    stage[vsh + rank[k]] = ok[r0:r1][k]
                sw = pack_bits(stage)[:(vsh + tot + 63) // 64 if tot else 0]
                w0 = first_bit >> 6
                sw = sw[:max(0, min(len(sw), nw - w0))]
                if mistake == "plain_store_over_shared_word":
                    words[j][w0:w0 + len(sw)] = sw
                else:
                    words[j][w0:w0 + len(sw)] |= sw
            carry += tot
        counts.append(carry)
    bits = [np.unpackbits(w.view(np.uint8), bitorder="little")[:n].astype(bool) for w in words]
    return {"counts": counts, "rows": rows, "bits": bits, "words": words}


def model_agrees(case, block_rows, mistake=None):
    """the model's counts, whole bitmap words and the values under 1 bits equal the oracle's"""
    want, got = case.oracle(block_rows), model(case, block_rows, mistake)
    if got["counts"] != want["counts"]:
        return False
    for j, dt in enumerate(want["dts"]):
        if not np.array_equal(got["words"][j], pack_bits(want["bits"][j])):
            return False
        if not same(got["rows"][j], want["rows"][j], dt, want["bits"][j]):
            return False
    return True


# ---------------------------------------------------------------------------
# null patterns and garbage
# ---------------------------------------------------------------------------
def with_nulls(case, pattern, garbage, seed):
    """the case with validity arrays by `pattern` and `garbage` (per column: values to cycle through) under the 0
    bits.  ones: every column an all-ones bitmap; none: no bitmaps; random: 10 % seeded nulls per column; last: the
    last column's bitmap alone (10 %); first_null: the first column all null; pred_null: the last column all null"""
    rng = np.random.default_rng(seed)
    n, K = case.n, len(case.dts)
    if pattern == "none":
        return case.replace(valid=[None] * K)
    valid = []
    for j in range(K):
        if pattern == "ones":
            valid.append(np.ones(n, bool))
        elif pattern == "random":
            valid.append(rng.random(n) >= 0.1)
        elif pattern == "last":
            valid.append(rng.random(n) >= 0.1 if j == K - 1 else None)
        elif pattern == "first_null":
            valid.append(np.zeros(n, bool) if j == 0 else rng.random(n) >= 0.1)
        elif pattern == "pred_null":
            valid.append(np.zeros(n, bool) if j == K - 1 else rng.random(n) >= 0.1)
        else:
            raise ValueError(pattern)
    host = []
    for j, (h, v) in enumerate(zip(case.host, valid)):
        h = h.copy()
        if v is not None and len(garbage[j]) and not v.all():
            bad = np.flatnonzero(~v)
            with np.errstate(all="ignore"):
                h[bad] = np.array(garbage[j], dtype=h.dtype)[np.arange(len(bad)) % len(garbage[j])]
        host.append(h)
    return case.replace(host=host, valid=valid)


# ---------------------------------------------------------------------------
# the shapes
# ---------------------------------------------------------------------------
def shape_q6(n, seed=0):
    """price * discount (Float64), quantity (UInt8), discount * discount (Float32)
    WHERE shipdate < 9950 and quantity < 26: about 3/8 of the rows pass"""
    rng = np.random.default_rng(1000003 + n + seed)
    dts = [F64, F32, I32, U8]
    host = [rng.uniform(1.0, 1000.0, n), (rng.integers(0, 11, n) / 100.0).astype(np.float32),
            rng.integers(8000, 10600, n).astype(np.int32), rng.integers(1, 51, n).astype(np.uint8)]
    pred = pred_tree_columns(dts, [([load(2)], "<", (9950, "Int32")), ([load(3)], "<", (26, "UInt8"))], [0, 1, "and"])
    values = [chain_columns(dts, [("*", Col(1))])[0], chain_columns(dts, [load(3)])[0],
              chain_columns(dts, [load(1), ("*", Col(1))])[0]]
    assert [v.out_dtype for v in values] == [F64, U8, F32]
    leaves = [R.Compare("<", fld("shipdate"), const(9950, "Int32")), R.Compare("<", fld("quantity"), const(26, "UInt8"))]
    exprs = [R.Arith("*", fld("price"), fld("discount")), fld("quantity"), R.Arith("*", fld("discount"), fld("discount"))]

    def np_pred(c, v, kleene):
        return (c[2] < 9950) & (c[3] < 26) & v[2] & v[3]  # `false and null` drops the row under either rule

    def np_vals(c, v):
        with np.errstate(all="ignore"):
            return [(c[0] * c[1].astype(np.float64), v[0] & v[1]), (c[3], v[3]), (c[1] * c[1], v[1])]
    garbage = [[np.nan, np.inf, -np.inf, 1e308, -1e308], [np.nan, np.inf, -np.inf, 3e38],
               [-(1 << 31), (1 << 31) - 1, 0], [0, 255, 1]]  # the integer ones pass the predicate
    case = Case("q6", ["price", "discount", "shipdate", "quantity"], dts, host, [None] * 4, pred, values,
                R.Logic("and", leaves[0], leaves[1]), leaves, exprs, np_pred, np_vals)
    return case, garbage


def shape_u8u16(n, seed=0):
    """a + b (UInt16: wraps at 16 bits), a (UInt8) WHERE a < 100"""
    rng = np.random.default_rng(2000003 + n + seed)
    dts = [U8, U16]
    host = [rng.integers(0, 256, n).astype(np.uint8), rng.integers(0, 65536, n).astype(np.uint16)]
    values = [chain_columns(dts, [("+", Col(1))])[0], None]
    assert values[0].out_dtype == U16

    def np_pred(c, v, kleene):
        return (c[0] < 100) & v[0]

    def np_vals(c, v):
        return [((c[0].astype(np.uint16) + c[1]).astype(np.uint16), v[0] & v[1]), (c[0], v[0])]
    case = Case("u8u16", ["a", "b"], dts, host, [None] * 2, predicate_columns(dts, [], "<", (100, "UInt8")), values,
                R.Compare("<", fld("a"), const(100, "UInt8")), None, [R.Arith("+", fld("a"), fld("b")), fld("a")],
                np_pred, np_vals)
    return case, [[0, 99, 255], [0, 65535]]


def shape_u8u16_or(n, seed=0):
    """a + b, b WHERE a < 100 or b < 20000: a tree whose one leaf is null on rows where the other is true"""
    rng = np.random.default_rng(2500003 + n + seed)
    dts = [U8, U16]
    host = [rng.integers(0, 256, n).astype(np.uint8), rng.integers(0, 65536, n).astype(np.uint16)]
    pred = pred_tree_columns(dts, [([], "<", (100, "UInt8")), ([load(1)], "<", (20000, "UInt16"))], [0, 1, "or"])
    values = [chain_columns(dts, [("+", Col(1))])[0], chain_columns(dts, [load(1)])[0]]
    leaves = [R.Compare("<", fld("a"), const(100, "UInt8")), R.Compare("<", fld("b"), const(20000, "UInt16"))]

    def np_pred(c, v, kleene):
        if kleene:  # true or null = true
            return ((c[0] < 100) & v[0]) | ((c[1] < 20000) & v[1])
        return ((c[0] < 100) | (c[1] < 20000)) & v[0] & v[1]

    def np_vals(c, v):
        return [((c[0].astype(np.uint16) + c[1]).astype(np.uint16), v[0] & v[1]), (c[1], v[1])]
    case = Case("u8u16_or", ["a", "b"], dts, host, [None] * 2, pred, values, R.Logic("or", leaves[0], leaves[1]), leaves,
                [R.Arith("+", fld("a"), fld("b")), fld("b")], np_pred, np_vals)
    return case, [[0, 99, 255], [0, 65535]]


def shape_u64cast(n, seed=0):
    """x + 1 (Int64: x is cast, 2^63 and above are nulls), x (UInt64) WHERE x % 8 < 3"""
    rng = np.random.default_rng(3000003 + n + seed)
    dts = [U64]
    x = rng.integers(0, 1 << 62, n).astype(np.uint64)
    big = rng.random(n) < 0.05  # valid rows whose cast leaves Int64; some pass the predicate
    x[big] = np.array([1 << 63, (1 << 64) - 8, (1 << 63) + 2], np.uint64)[np.arange(int(big.sum())) % 3]
    pred = predicate_columns(dts, [("%", 8)], "<", 3)
    assert pred.cmp_dtype == U64
    values = [chain_columns(dts, [("+", (1, "Int64"))])[0], None]
    assert values[0].out_dtype == I64

    def np_pred(c, v, kleene):
        return (c[0] % np.uint64(8) < 3) & v[0]

    def np_vals(c, v):
        return [((c[0] + np.uint64(1)).astype(np.int64), v[0] & (c[0] < np.uint64(1 << 63))), (c[0], v[0])]
    case = Case("u64cast", ["x"], dts, [x], [None], pred, values,
                R.Compare("<", R.Arith("%", fld("x"), const(8, "UInt64")), const(3, "UInt64")), None,
                [R.Arith("+", fld("x"), const(1, "Int64")), fld("x")], np_pred, np_vals)
    return case, [[1 << 63, (1 << 64) - 1, 0, 1]]


SHAPES = {"q6": shape_q6, "u8u16": shape_u8u16, "u64cast": shape_u64cast, "u8u16_or": shape_u8u16_or}
# (n, block_rows): block boundaries mid-word with a short last block; boundaries on words with a one-row last
# block; one whole block; one short block around a bitmap word
SIZES = [(25003, 10000), (16385, 8192), (8192, 8192), (1, 10000), (63, 10000), (64, 10000), (65, 10000)]
PATTERNS = ["ones", "none", "random", "last", "first_null", "pred_null"]
_CASES = {}


def get_case(shape, n, pattern, seed=0):
    key = (shape, n, pattern, seed)
    if key not in _CASES:
        base, garbage = SHAPES[shape](n, seed)
        _CASES[key] = with_nulls(base, pattern, garbage, 7000003 + n + seed)
    return _CASES[key]


def grid(ticket_blocks=259):
    """every (case, block_rows) the GPU file runs: the three shapes and the or-tree at every size with 10 % nulls,
    every null pattern at the first size, and the ticket-loop case (CUs + 3 blocks of 10,000 rows; 256 CUs here)"""
    out = []
    for shape in SHAPES:
        for n, br in SIZES:
            out.append((get_case(shape, n, "random"), br))
        for pattern in PATTERNS:
            if pattern != "random":
                out.append((get_case(shape, SIZES[0][0], pattern), SIZES[0][1]))
    out.append((get_case("q6", ticket_blocks * 10000 - 7, "random"), 10000))
    return out
