"""Generator of random programs and inputs for the typed and nullable fused
kernels (no test of its own; imported by tests/test_fuzz_typed_cpu.py and
tests/test_fuzz_typed_gpu.py the way tests/replay.py is).

generate(family, seed) deterministically draws one abstract program (columns of
any of the ten numeric types, value chains with load / push / stack / reversed
steps, a predicate: none, one comparison, an and/or tree or a precomputed
bitmap; an aggregate mask or a list of projection outputs; which columns carry
a validity bitmap) and three runs of it (two flat sizes and one block-mode
size, with column offsets and inputs).  The one program object is lowered twice:
device() builds the fq_expr / fq_pred descriptors through fq_amd.expr, ref()
builds the oracle/fq_ref.py function tree; where both sides state a type
(chain_columns' out_dtype, a predicate's cmp_dtype) the lowering asserts that
they agree.  expected() evaluates a run with the per-block oracles of the three
shape tests (tests/test_scan_typed_gpu.py, tests/test_scan_nullable_gpu.py,
tests/test_project_typed_gpu.py).

Families: "agg" ops.aggregate_typed, "null" ops.aggregate_nullable, "proj"
ops.filter_project_typed / filter_project_blocks_typed / predicate_bitmap_typed.

What the generator avoids, because the device contract differs from the
reference's fold there:
  * NaN among the valid values of an aggregate argument (max / min of NaN);
  * agg / proj: a cast null in a program that also divides -- the reference
    raises the first error it meets and evaluates nothing after it, the device
    ORs the flags of every live row and goes on with the wrapped value;
  * agg / proj: a cast null in a leaf of an and/or tree (fq_ref's logic op
    drops the leaves' validity, tests/test_scan_nullable_gpu.py's docstring);
  * a float sum whose sum of magnitudes comes within a factor of four of the
    format's maximum (whether a partial sum overflows depends on the order),
    or whose argument holds both infinities (the sum is NaN, which the shape
    tests' check of a Float32 sum does not take): such a seed's mask drops
    AGG_SUM.
A program that jit_prepare_* refuses as "too long" (its casts do not fit the
lowered program) is redrawn from a sub-seed; any other refusal propagates."""
import numpy as np

import fq_ref as R
from fq_amd import abi, ops
from fq_amd._lib import FQError
from fq_amd.expr import STACK, Col, chain_columns, load, pred_tree_columns, predicate_columns, push

import test_project_typed_gpu as TP
import test_scan_nullable_gpu as TN
import test_scan_typed_gpu as TA

FAMILIES = ("agg", "null", "proj")
TYPES = list(R.NUMERIC)
DT = abi.DT_BY_NAME
NAME = abi.DT_NAMES
OPS = ["+", "-", "*", "/", "%"]
CMPS = ["=", "<", "<=", ">", ">="]
ERR = abi.STATE_DIV_ZERO | abi.STATE_CAST_NULL
NAMES = ["c0", "c1", "c2", "c3"]
# the share of '/' and '%' steps whose divisor is an intermediate (not a column, not a constant) that are kept: what
# brings the seeds whose reference result is an error between 1/16 and 1/4 of each family (a projection has up to
# eight chains that can divide by an intermediate zero)
KEEP_INTERMEDIATE_DIVISOR = {"agg": 0.3, "null": 0.3, "proj": 0.03}
# how often a bitmap has no, ~1 %, ~50 %, ~99 %, only null bits
NULL_SHARES, NULL_SHARE_P = [0.0, 0.01, 0.5, 0.99, 1.0], [0.25, 0.2, 0.3, 0.15, 0.1]


def is_float(t):
    return t.startswith("Float")


def width(t):
    return np.dtype(R.NP[t]).itemsize


def wide_of(t):
    return "Int64" if R.is_signed(t) else "UInt64"


# ---------------------------------------------------------------------------
# the abstract program
# ---------------------------------------------------------------------------
class K:
    """a typed constant; its value is drawn once the shape's integer range is known"""

    def __init__(self, t, divisor=False):
        self.t, self.v, self.divisor = t, None, divisor

    def __repr__(self):
        return "%r:%s" % (self.v, self.t)


class Chain:
    """steps: ("load", j) | ("push", j) | (op, operand, reversed); operand: ("col", j) | ("stack",) | K"""

    def __init__(self, steps):
        self.steps = steps

    def __repr__(self):
        out = []
        for s in self.steps:
            if s[0] in ("load", "push"):
                out.append("%s(%d)" % s)
            else:
                o = s[1]
                x = "c%d" % o[1] if isinstance(o, tuple) and o[0] == "col" else ("STACK" if isinstance(o, tuple) else repr(o))
                out.append("(%s %s%s)" % (s[0], x, " rev" if s[2] else ""))
        return "[" + " ".join(out) + "]"


def walk(chain, dts):
    """per arithmetic step: dict(i, op, rev, acc, opd, t, acc_col, opd_col, opd_kind); and the chain's type"""
    acc, acc_col, stack, info = dts[0], 0, [], []
    for i, s in enumerate(chain.steps):
        if s[0] == "load":
            acc, acc_col = dts[s[1]], s[1]
        elif s[0] == "push":
            stack.append((acc, acc_col))
            acc, acc_col = dts[s[1]], s[1]
        else:
            op, o, rev = s
            if isinstance(o, K):
                ot, oc, kind = o.t, None, "const"
            elif o[0] == "col":
                ot, oc, kind = dts[o[1]], o[1], "col"
            else:
                (ot, oc), kind = stack.pop(), "stack"
            t = R.numerical_coercion(op, ot, acc) if rev else R.numerical_coercion(op, acc, ot)
            info.append(dict(i=i, op=op, rev=rev, acc=acc, opd=ot, t=t, acc_col=acc_col, opd_col=oc, opd_kind=kind))
            acc, acc_col = t, None
    assert not stack
    return info, acc


class Leaf:
    def __init__(self, chain, sym, rhs, flipped=False):
        self.chain, self.sym, self.rhs, self.flipped = chain, sym, rhs, flipped  # rhs: ("col", j) | K

    def __repr__(self):
        r = "c%d" % self.rhs[1] if isinstance(self.rhs, tuple) else repr(self.rhs)
        return "%s %s %s%s" % (self.chain, self.sym, r, " flipped" if self.flipped else "")


class Program:
    """family, seed, dts (reference type names), value (agg / null: Chain or None), outputs (proj: [Chain or
    None]), kind ("none" | "expr" | "tree" | "bitmap"), leaves, prog (postfix of a tree), mask, nullable"""

    def __init__(self, family, seed):
        self.family, self.seed = family, seed
        self.dts, self.value, self.outputs, self.kind, self.leaves, self.prog = [], None, [], "none", [], []
        self.mask, self.nullable, self.small, self.too_long, self.ambiguous = 0, [], False, 0, 0
        self.force_cast = self.plant_zero = False

    @property
    def adts(self):
        return [DT[t] for t in self.dts]

    @property
    def names(self):
        return NAMES[:len(self.dts)]

    def chains(self):
        """(id, chain) of every chain: v<j> the values, p<i> the predicate's leaves"""
        out = [("v%d" % j, c) for j, c in enumerate(self.outputs if self.family == "proj" else [self.value]) if c is not None]
        return out + [("p%d" % i, lf.chain) for i, lf in enumerate(self.leaves)]

    def consts(self):
        ks = [s[1] for _, c in self.chains() for s in c.steps if s[0] not in ("load", "push") and isinstance(s[1], K)]
        return ks + [lf.rhs for lf in self.leaves if isinstance(lf.rhs, K)]

    def has_division(self):
        return any(s[0] in "/%" for _, c in self.chains() for s in c.steps if s[0] not in ("load", "push"))

    def out_types(self):
        return [self.dts[0] if c is None else walk(c, self.dts)[1] for c in self.outputs]

    def describe(self):
        what = "outputs=%r" % (self.outputs,) if self.family == "proj" else "value=%r mask=%d" % (self.value, self.mask)
        pred = {"none": "none", "bitmap": "bitmap of " + repr(self.leaves[0]) if self.leaves else "bitmap"}.get(
            self.kind, "%r prog=%r" % (self.leaves, self.prog))
        return "%s seed %d: dtypes=%r %s pred(%s)=%s nullable=%r" % (self.family, self.seed, self.dts, what, self.kind,
                                                                    pred, self.nullable)

    # ---- lowering 1: the device descriptors ----
    def device(self):
        """(fq_pred or None, fq_expr or None | [fq_expr or None]); a bitmap predicate's pointer is set per run"""
        adts = self.adts

        def chain(c):
            steps = []
            for s in c.steps:
                if s[0] == "load":
                    steps.append(load(s[1]))
                elif s[0] == "push":
                    steps.append(push(s[1]))
                else:
                    o = s[1]
                    x = (o.v, o.t) if isinstance(o, K) else (Col(o[1]) if o[0] == "col" else STACK)
                    steps.append((s[0], x, True) if s[2] else (s[0], x))
            e, out = chain_columns(adts, steps)
            assert NAME[out] == walk(c, self.dts)[1] == NAME[e.out_dtype], (self.describe(), c)
            return e, steps

        def rhs(lf):
            return (lf.rhs.v, lf.rhs.t) if isinstance(lf.rhs, K) else Col(lf.rhs[1])

        pred = None
        if self.kind == "expr":
            lf = self.leaves[0]
            pred = predicate_columns(adts, chain(lf.chain)[1], lf.sym, rhs(lf), flipped=lf.flipped)
            assert NAME[pred.cmp_dtype] == self.cmp_type(lf), self.describe()
        elif self.kind == "tree":
            pred = pred_tree_columns(adts, [(chain(lf.chain)[1], lf.sym, rhs(lf)) for lf in self.leaves], self.prog)
            for i, lf in enumerate(self.leaves):
                assert NAME[pred._tree.leaves[i].cmp_dtype] == self.cmp_type(lf), self.describe()
        elif self.kind == "bitmap":
            pred = abi.fq_pred()
            pred.kind = abi.PRED_BITMAP
        if self.family == "proj":
            return pred, [None if c is None else chain(c)[0] for c in self.outputs]
        return pred, (None if self.value is None else chain(self.value)[0])

    def cmp_type(self, lf):
        """the type the reference compares a leaf in"""
        schema = dict(zip(self.names, self.dts))
        lt = self.ref_chain(lf.chain, "").return_type(schema)
        return R.equal_coercion(lf.sym, lt, lf.rhs.t if isinstance(lf.rhs, K) else self.dts[lf.rhs[1]])

    def descriptor_bytes(self):
        pred, val = self.device()
        out = b"" if pred is None else b"".join(bytes(x) for x in (
            [pred.lhs] + ([pred._tree] if self.kind == "tree" else [])))
        if pred is not None:
            out += repr((pred.kind, pred.cmp, pred.cmp_dtype, pred.rhs_operand, pred.rhs_bits)).encode()
        vals = val if isinstance(val, list) else [val]
        return out + b"".join(b"-" if v is None else bytes(v) for v in vals)

    # ---- lowering 2: the oracle's function tree ----
    def ref_chain(self, c, cid, mut=None, tolerant=False):
        """mut: (kind, (chain id, step)): "a" drops `reversed`, "f" swaps the stack operands, "b" evaluates the
        step at 64 bits (truncated at the chain's end).  tolerant: a zero divisor does not raise"""
        names = self.names
        plain = TolerantArith if tolerant else R.Arith
        acc, stack, widened = R.Field(names[0]), [], False
        for i, s in enumerate(c.steps):
            if s[0] == "load":
                acc = R.Field(names[s[1]])
            elif s[0] == "push":
                stack.append(acc)
                acc = R.Field(names[s[1]])
            else:
                op, o, rev = s
                x = R.Const(R.Value(o.t, o.v)) if isinstance(o, K) else (R.Field(names[o[1]]) if o[0] == "col" else stack.pop())
                cls = plain
                if mut is not None and mut[1] == (cid, i):
                    if mut[0] == "a":
                        rev = False
                    elif mut[0] == "f":
                        rev = not rev
                    elif mut[0] == "b":
                        cls, widened = WideArith, True
                acc = cls(op, x, acc) if rev else cls(op, acc, x)
        return Truncate(acc, walk(c, self.dts)[1]) if widened else acc

    def ref_leaf(self, i, mut=None, tolerant=False):
        lf = self.leaves[i]
        lhs = self.ref_chain(lf.chain, "p%d" % i, mut, tolerant)
        rhs = R.Const(R.Value(lf.rhs.t, lf.rhs.v)) if isinstance(lf.rhs, K) else R.Field(self.names[lf.rhs[1]])
        cls = UnsignedCompare if mut is not None and mut == ("c", ("p%d" % i, -1)) else R.Compare
        return cls(lf.sym, rhs, lhs) if lf.flipped else cls(lf.sym, lhs, rhs)

    def ref(self, mut=None, tolerant=False):
        """(where or None, the leaves' comparisons when the predicate is a tree else None, [value functions])"""
        leaves = [self.ref_leaf(i, mut, tolerant) for i in range(len(self.leaves))]
        where, tree = None, None
        if self.kind in ("expr", "bitmap"):
            where = leaves[0]
        elif self.kind == "tree":
            st = []
            for tok in self.prog:
                if isinstance(tok, str):
                    b, a = st.pop(), st.pop()
                    st.append(R.Logic(tok, a, b))
                else:
                    st.append(leaves[tok])
            where, tree = st[0], leaves
        chains = self.outputs if self.family == "proj" else [self.value]
        vals = [R.Field(self.names[0]) if c is None else self.ref_chain(c, "v%d" % j, mut, tolerant)
                for j, c in enumerate(chains)]
        return where, tree, vals

    # ---- where a reference-side mutation applies ----
    def sites(self, kind):
        out = []
        for cid, c in self.chains():
            info, _ = walk(c, self.dts)
            for k, st in enumerate(info):
                if kind == "a" and st["rev"] and st["op"] in "-/%":
                    out.append((cid, st["i"]))
                if kind == "f" and st["opd_kind"] == "stack" and st["op"] in "-/%":
                    out.append((cid, st["i"]))
                # a narrow integer step whose result meets something that is no ring operation of its own width
                if kind == "b" and not is_float(st["t"]) and width(st["t"]) < 8:
                    nxt = info[k + 1] if k + 1 < len(info) else None
                    if nxt is not None and (nxt["op"] in "/%" or nxt["t"] != st["t"]):
                        out.append((cid, st["i"]))
        if kind == "c":
            for i, lf in enumerate(self.leaves):
                if self.kind == "bitmap":
                    break
                ct = self.cmp_type(lf)
                lt = walk(lf.chain, self.dts)[1]
                rt = lf.rhs.t if isinstance(lf.rhs, K) else self.dts[lf.rhs[1]]
                if not is_float(ct) and R.is_signed(ct) and (not R.is_signed(lt) or not R.is_signed(rt)):
                    out.append(("p%d" % i, -1))
        return out


def _arrays(l, r):
    if isinstance(l, R.Arr) and isinstance(r, R.Arr):
        return l, r
    if isinstance(l, R.Arr):
        return l, R.to_array(r, len(l))
    if isinstance(r, R.Arr):
        return R.to_array(l, len(r)), r
    return R.to_array(l, 1), R.to_array(r, 1)


class TolerantArith(R.Arith):
    """the reference's arithmetic with every zero divisor read as 1: for looking at a program's nulls and NaNs"""

    def eval(self, b):
        la, ra = _arrays(self.left.eval(b), self.right.eval(b))
        ct = R.numerical_coercion(self.op, la.type, ra.type)
        lc, rc = R.cast(la, ct), R.cast(ra, ct)
        if self.op in "/%":
            rc = R.Arr(ct, np.where(rc.values == 0, np.ones(1, rc.values.dtype), rc.values), rc.valid)
        return R.arith_arrays(self.op, lc, rc)


class WideArith(R.Arith):
    """mutation (b): the step at 64 bits"""

    def eval(self, b):
        la, ra = _arrays(self.left.eval(b), self.right.eval(b))
        ct = wide_of(R.numerical_coercion(self.op, la.type, ra.type))
        with np.errstate(all="ignore"):
            return R.arith_arrays(self.op, R.Arr(ct, la.values.astype(R.NP[ct]), la.valid),
                                  R.Arr(ct, ra.values.astype(R.NP[ct]), ra.valid))


class Truncate(R.Fn):
    def __init__(self, inner, t):
        self.inner, self.t = inner, t

    def return_type(self, s):
        return self.t

    def eval(self, b):
        a = self.inner.eval(b)
        if a.type == self.t:
            return a
        with np.errstate(all="ignore"):
            return R.Arr(self.t, a.values.astype(R.NP[self.t]), a.valid)


class UnsignedCompare(R.Compare):
    """mutation (c): a comparison the coercion makes signed, done on the same bits as unsigned"""

    def eval(self, b):
        la, ra = _arrays(self.left.eval(b), self.right.eval(b))
        ct = R.equal_coercion(self.op, la.type, ra.type)
        lc, rc = R.cast(la, ct), R.cast(ra, ct)
        u = TP.UINT[width(ct)]
        return R.Arr("Boolean", list(R._cmp(self.op, lc.values.view(u), rc.values.view(u))), R._both_valid(lc, rc))


# ---------------------------------------------------------------------------
# drawing a program
# ---------------------------------------------------------------------------
def draw_chain(rng, dts, max_steps, p, no_div=False, first=None):
    """0..max_steps arithmetic steps; about one chain in four a tree, one step in four reversed.  first: a step
    the chain begins with (then it has no load)"""
    ncols = len(dts)
    n = int(rng.integers(0, max_steps + 1))
    tree = n >= 2 and rng.random() < 0.3
    steps = []
    if first is not None:
        steps.append(first)
    elif rng.random() < (0.6 if n == 0 else 0.3):
        steps.append(("load", int(rng.integers(ncols))))
    depth, acc_plain = 0, first is None  # acc_plain: acc is a column as loaded
    for k in range(n):
        left = n - k
        if tree and depth < abi.MAX_STACK and left > depth + 1 and len(steps) + 1 + left <= abi.MAX_STEPS \
                and rng.random() < 0.5:
            steps.append(("push", int(rng.integers(ncols))))
            depth += 1
            acc_plain = True
        if depth > 0 and (left <= depth or rng.random() < 0.4):
            o, o_plain = ("stack",), False
            depth -= 1
        elif rng.random() < 0.6:
            o, o_plain = ("col", int(rng.integers(ncols))), True
        else:
            t = dts[int(rng.integers(ncols))] if rng.random() < 0.5 else TYPES[int(rng.integers(len(TYPES)))]
            o, o_plain = K(t), True
        rev = rng.random() < 0.25
        for _ in range(8):
            op = "+-*"[int(rng.integers(3))] if no_div else OPS[int(rng.integers(5))]
            divisor_plain = acc_plain if rev else o_plain
            if op not in "/%" or divisor_plain or rng.random() < p:
                break
        if op in "/%" and isinstance(o, K) and not rev:
            o.divisor = True
        steps.append((op, o, bool(rev)))
        acc_plain = False
    assert depth == 0
    return Chain(steps)


def draw_leaf(rng, dts, flippable, p):
    rhs = ("col", int(rng.integers(len(dts)))) if rng.random() < 0.35 else K(TYPES[int(rng.integers(len(TYPES)))])
    if isinstance(rhs, K) and rng.random() < 0.5:
        rhs = K(dts[int(rng.integers(len(dts)))])
    return Leaf(draw_chain(rng, dts, 3, p), CMPS[int(rng.integers(5))], rhs,
                bool(flippable and rng.random() < 0.25))


def draw_program(rng, family, seed):
    P = Program(family, seed)
    P.small = seed % 2 == 0
    # a cast that can be null, planted: one row (agg / proj, one seed in 16), many rows (null, one seed in 4)
    P.force_cast = seed % 4 == 1 if family == "null" else seed % 16 == 5
    P.plant_zero = seed % 8 == 3
    ncols = int(rng.integers(1, 5))
    P.dts = [TYPES[int(rng.integers(10))] for _ in range(ncols)]
    if P.force_cast:  # column 0 unsigned, column 1 signed and no wider: c0 op c1 is computed in c1's type
        ncols = max(ncols, 2)
        P.dts = (P.dts + ["Int8"])[:ncols]
        u = ["UInt8", "UInt16", "UInt32", "UInt64"][int(rng.integers(4))]
        s = [t for t in ("Int8", "Int16", "Int32", "Int64") if width(t) <= width(u)]
        P.dts[0], P.dts[1] = u, s[int(rng.integers(len(s)))]
    no_div = P.force_cast and family != "null"

    def value():
        first = ("+-*"[int(rng.integers(3))], ("col", 1), False) if P.force_cast else None
        return draw_chain(rng, P.dts, 5, KEEP_INTERMEDIATE_DIVISOR[family], no_div, first)

    if family == "proj":
        for j in range(int(rng.integers(1, abi.MAX_PROJECT + 1))):
            P.outputs.append(None if rng.random() < 0.2 else value())
        if P.force_cast and P.outputs[0] is None:
            P.outputs[0] = value()
    else:
        c = value()
        P.value = c if c.steps else None
        P.mask = int(rng.integers(1, 16))
    u = rng.random()
    if family != "proj" and rng.random() < 0.125:
        P.kind = "bitmap"  # the bits of one comparison of a column with a constant of its own type: no cast, no error
        j = int(rng.integers(ncols))
        P.leaves = [Leaf(Chain([("load", j)]), CMPS[int(rng.integers(5))], K(P.dts[j]))]
    elif u < 0.25:
        P.kind = "none"
    elif u < 0.6:
        P.kind, P.leaves = "expr", [draw_leaf(rng, P.dts, True, KEEP_INTERMEDIATE_DIVISOR[family])]
    else:
        P.kind = "tree"
        k = int(rng.integers(2, abi.MAX_PRED_LEAVES + 1))
        P.leaves = [draw_leaf(rng, P.dts, False, KEEP_INTERMEDIATE_DIVISOR[family]) for _ in range(k)]
        nxt, sp = 0, 0
        while nxt < k or sp > 1:
            if sp >= 2 and (nxt == k or rng.random() < 0.5):
                P.prog.append("and" if rng.random() < 0.5 else "or")
                sp -= 1
            else:
                P.prog.append(nxt)
                nxt, sp = nxt + 1, sp + 1
    if family == "null":
        how = int(rng.integers(3))  # none, some, all of the columns carry a bitmap
        P.nullable = [bool(how == 2 or (how == 1 and rng.random() < 0.5)) for _ in range(ncols)]
    return P


def int_range(P):
    """{signedness: (lo, hi)}: what the integer columns and constants of the shape draw from, so that no cast is
    null by accident.  numerical_coercion casts an unsigned value to every signed type of the shape and a signed
    one only to wider signed types: unsigned values lie in the intersection of the ranges of every integer type
    of the shape, columns and constants together, signed values in the intersection of its signed types' ranges
    (so they are negative too, and a comparison coerced to the signed side meets them)"""
    ts = [t for t in P.dts + [k.t for k in P.consts()] if not is_float(t)]
    signed = [R.int_range(t) for t in ts if R.is_signed(t)]
    slo, shi = max([r[0] for r in signed] + [-(1 << 63)]), min([r[1] for r in signed] + [(1 << 63) - 1])
    uhi = min([R.int_range(t)[1] for t in ts if not R.is_signed(t)] + [(1 << 64) - 1] + ([shi] if signed else []))
    return {True: (slo, shi), False: (0, uhi)}


def range_of(rg, t):
    return rg[R.is_signed(t)]


def draw_consts(rng, P, rg):
    """the chains' constants (a predicate's right-hand constant comes from the data: set_pred_consts)"""
    pred = [lf.rhs for lf in P.leaves if isinstance(lf.rhs, K)]
    for k in P.consts():
        if any(k is q for q in pred):
            continue
        lo, hi = (0, 0) if is_float(k.t) else range_of(rg, k.t)
        while True:
            if is_float(k.t):
                k.v = float(rng.integers(-40, 41)) / 4.0
            elif P.small or rng.random() < 0.5:
                k.v = int(rng.integers(max(lo, -11), min(hi, 11) + 1))
            else:
                k.v = [lo, hi, lo + 1, hi - 1][int(rng.integers(4))]
            if k.v != 0 or not k.divisor:
                break


# ---------------------------------------------------------------------------
# runs: geometry and inputs
# ---------------------------------------------------------------------------
class Run:
    def __init__(self, n, br, offsets, out_offset):
        self.n, self.br, self.offsets, self.out_offset = n, br, offsets, out_offset
        self.host, self.valid, self.keep = [], [], None  # keep: the bits of a bitmap predicate
        self._exp = {}

    def describe(self):
        return "n=%d block_rows=%d offsets=%r out_offset=%d" % (self.n, self.br, self.offsets, self.out_offset)

    def input_bytes(self):
        out = b"".join(h.tobytes() for h in self.host)
        out += b"".join(b"-" if v is None else np.packbits(v).tobytes() for v in self.valid)
        return out + (b"" if self.keep is None else np.packbits(self.keep).tobytes())


def draw_geometry(rng, P):
    k = len(P.dts)
    if P.family == "proj":
        T = TP.tile_rows(P.adts, [DT[t] for t in P.out_types()])
        flat = [1, 3, T - 1, T, T + 1, 2 * T + 5]
        br = [8192, 10000][int(rng.integers(2))]
        block = (2 * br + 37, br)
    else:
        G = TN.group(P.adts)
        flat = [1, 3, 63, 64, 65, 256 * G - 1, 256 * G, 256 * G + 1, 2 * 256 * G + G + 3]
        br = [1000, 1001, 4096][int(rng.integers(3))]
        block = (3 * br + 7, br)
    sizes = [(int(flat[i]), 0) for i in sorted(rng.choice(len(flat), 2, replace=False))] + [block]
    how = P.seed % 3
    runs = []
    for n, b in sizes:
        if how == 0:
            offs = [0] * k
        elif how == 1:
            offs = [[1, 3, 7][int(rng.integers(3))]] * k
        else:
            offs = [[0, 1, 3, 7][int(rng.integers(4))] for _ in range(k)]
        runs.append(Run(n, b, offs, int(rng.integers(2)) if P.family == "proj" else 0))
    return runs


def draw_column(rng, P, t, n, rg):
    if is_float(t):
        if P.small:
            return (rng.integers(-40, 41, n) / 4.0).astype(R.NP[t])
        v = rng.uniform(-1000.0, 1000.0, n).astype(R.NP[t])
        special = [0.0, -0.0, np.inf, -np.inf] + ([np.nan, float(np.finfo(R.NP[t]).max)] if P.family == "proj" else [])
        rows = np.unique(np.concatenate([[0, n // 2, n - 1], rng.integers(0, n, max(1, n // 50))]))
        v[rows] = np.array(special, R.NP[t])[rng.integers(0, len(special), len(rows))]
        return v
    lo, hi = range_of(rg, t)
    l, h = (max(lo, -11), min(hi, 11)) if P.small else (lo, hi)
    if h > (1 << 63) - 1:
        v = rng.integers(l, h, n, dtype=np.uint64, endpoint=True)
    else:
        v = rng.integers(l, h, n, dtype=np.int64, endpoint=True)
    if not P.small:  # the extremes, their neighbours, 0 and +-1 at the first row, mid-tile, the last row and a few more
        special = [l, h, l + 1, h - 1, 0, 1] + ([-1] if l < 0 else [])
        rows = np.unique(np.concatenate([[0, n // 2, n - 1], rng.integers(0, n, max(1, n // 50))]))
        v[rows] = np.array(special, v.dtype)[rng.integers(0, len(special), len(rows))]
    return v.astype(R.NP[t])


def garbage(t):
    """what lies under a 0 bit: zero divisors, NaN, +-inf, the column's own extremes (outside the casts' ranges)"""
    if is_float(t):
        return [np.nan, np.inf, -np.inf, 0.0, float(np.finfo(R.NP[t]).max)]
    lo, hi = R.int_range(t)
    return [0, lo, hi, 1]


def direct_divisors(P):
    """the columns used directly as a divisor"""
    out = set()
    for _, c in P.chains():
        for st in walk(c, P.dts)[0]:
            if st["op"] in "/%":
                j = st["acc_col"] if st["rev"] else st["opd_col"]
                if j is not None:
                    out.add(j)
    return sorted(out)


def block_of(P, run, valid=None, rows=slice(None)):
    valid = run.valid if valid is None else valid
    return R.Block([(nm, R.Arr(t, h[rows], None if v is None else v[rows]))
                    for nm, t, h, v in zip(P.names, P.dts, run.host, valid)])


def draw_inputs(rng, P, run, rg):
    n, k = run.n, len(P.dts)
    run.host = [draw_column(rng, P, t, n, rg) for t in P.dts]
    div = direct_divisors(P)
    for j in div:
        run.host[j][run.host[j] == 0] = 1
    run.valid = [None] * k
    if P.plant_zero and div:
        run.host[div[int(rng.integers(len(div)))]][int(rng.integers(n))] = 0
    if P.force_cast:  # values of column 0 above column 1's maximum
        top, own = R.int_range(P.dts[1])[1], R.int_range(P.dts[0])[1]
        bad = [top + 1, own, min(own, 2 * top + 1)]
        rows = np.flatnonzero(rng.random(n) < 0.2) if P.family == "null" else rng.integers(0, n, 1)
        run.host[0][rows] = np.array(bad, dtype=np.uint64)[rng.integers(0, 3, len(rows))].astype(R.NP[P.dts[0]])
    if P.family == "proj":
        return
    # no NaN among an aggregate argument's values: the rows that give one get plain floats
    arg = P.ref(tolerant=True)[2][0]
    for _ in range(2):
        with np.errstate(all="ignore"):
            val = arg.eval(block_of(P, run))
        if not is_float(val.type) or not np.isnan(val.values).any():
            break
        rows = np.isnan(val.values)
        for j, t in enumerate(P.dts):
            if is_float(t):
                run.host[j][rows] = 1.5
    if P.family == "null":
        for j, t in enumerate(P.dts):
            if not P.nullable[j]:
                continue
            share = NULL_SHARES[int(rng.choice(5, p=NULL_SHARE_P))]
            v = rng.random(n) >= share
            g = np.array(garbage(t), dtype=R.NP[t])
            bad = np.flatnonzero(~v)
            run.host[j][bad] = g[rng.integers(0, len(g), len(bad))]
            run.valid[j] = v


def set_pred_consts(rng, P, run, rg):
    """each right-hand constant a quantile of its left side's values in `run`, in the constant's type"""
    for i, lf in enumerate(P.leaves):
        if not isinstance(lf.rhs, K):
            continue
        with np.errstate(all="ignore"):
            a = P.ref_chain(lf.chain, "", tolerant=True).eval(block_of(P, run))
        vals = a.values if a.valid is None else a.values[np.asarray(a.valid, bool)]
        vals = vals[np.isfinite(vals)] if is_float(a.type) else vals
        q = [0.0, 0.03, 0.5, 1.0][int(rng.choice(4, p=[0.04, 0.26, 0.5, 0.2]))]
        x = np.sort(vals)[min(len(vals) - 1, int(q * len(vals)))] if len(vals) else 0
        if is_float(lf.rhs.t):
            lf.rhs.v = float(R.NP[lf.rhs.t](x))
        else:
            l, h = range_of(rg, lf.rhs.t)
            lf.rhs.v = int(min(max(int(np.floor(float(x))) if is_float(a.type) else int(x), l), h))


def keep_mask(P, run, tolerant=False):
    """the rows the reference's filter keeps (a null predicate drops the row; a tree is null where a leaf is)"""
    where, tree, _ = P.ref(tolerant=tolerant)
    if where is None:
        return np.ones(run.n, bool)
    blk = block_of(P, run)
    with np.errstate(all="ignore"):
        res = where.eval(blk)
        keep = np.array(res.values, bool)
        for a in [res] + ([lf.eval(blk) for lf in tree] if tree else []):
            if a.valid is not None:
                keep &= np.asarray(a.valid, bool)
    return keep


COMPLEMENT = {"<": ">=", ">=": "<", ">": "<=", "<=": ">", "=": "<="}


def steer(rng, P, run):
    """most of the predicates that keep no row of `run` at all (a left side that is one value, c0 > c0) are turned
    round, so that the seeds do not crowd at the early return: a tree's `and`s become `or`s, then the first
    comparison its complement"""
    if P.kind not in ("expr", "tree") or rng.random() < 0.3 or keep_mask(P, run, True).any():
        return
    P.prog = ["or" if tok == "and" else tok for tok in P.prog]
    if not keep_mask(P, run, True).any():
        P.leaves[0].sym = COMPLEMENT[P.leaves[0].sym]


def both_infinities(P, run):
    """+inf and -inf among the aggregate argument's valid values, kept or not: their sum is NaN"""
    with np.errstate(all="ignore"):
        val = P.ref(tolerant=True)[2][0].eval(block_of(P, run))
    v = val.values if val.valid is None else val.values[np.asarray(val.valid, bool)]
    return bool(is_float(val.type) and np.isposinf(v).any() and np.isneginf(v).any())


def ambiguous(P, run):
    """what the generator avoids (the module's docstring)"""
    where, tree, vals = P.ref(tolerant=True)
    blk = block_of(P, run)
    with np.errstate(all="ignore"):
        leaves = [P.ref_leaf(i, tolerant=True).eval(blk) for i in range(len(P.leaves))]
        values = [v.eval(blk) for v in vals]
    if P.family != "proj":
        val = values[0]
        ok = np.ones(len(val), bool) if val.valid is None else np.asarray(val.valid, bool)
        if is_float(val.type) and np.isnan(val.values[ok]).any():
            return True
    if P.family == "null":
        return False
    leaf_null = any(a.valid is not None and not np.all(a.valid) for a in leaves)
    val_null = any(a.valid is not None and not np.all(a.valid) for a in values)
    return (P.has_division() and (leaf_null or val_null)) or (P.kind == "tree" and leaf_null)


# ---------------------------------------------------------------------------
# the oracle's answer for a run
# ---------------------------------------------------------------------------
def make_case(P, run, mut=None):
    where, _, vals = P.ref(mut)
    return TP.Case(P.names, P.adts, run.host, None, None, where, vals)


def expected(P, run, mut=None):
    """agg / null: the dict of the shape test's ref_scan; proj: ("ok", outs, counts, dtypes) of Case.oracle or
    ("err", abi.FQ_E_DIVIDE_BY_ZERO | abi.FQ_E_UNSUPPORTED).  mut: a reference-side mutation -- ("a" | "b" | "c" |
    "f", site), ("d",) garbage read as valid, ("e", j) column j's bitmap shifted by one row"""
    key = repr(mut)
    if key in run._exp:
        return run._exp[key]
    fmut = mut if mut is not None and mut[0] in "abcf" else None
    where, tree, vals = P.ref(fmut)
    with np.errstate(all="ignore"):
        if P.family == "agg":
            out = TA.ref_scan(P.names, P.adts, run.host, where, vals[0], run.br)
        elif P.family == "null":
            valid = list(run.valid)
            if mut is not None and mut[0] == "d":
                valid = [None] * len(valid)
            elif mut is not None and mut[0] == "e":
                valid[mut[1]] = np.roll(valid[mut[1]], 1)
            out = TN.ref_scan(P.names, P.adts, run.host, valid, where, tree, vals[0], run.br)
        else:
            try:
                out = ("ok",) + make_case(P, run, fmut).oracle(run.br if run.br < run.n else 0)
            except R.RefError as e:
                assert "Divide by zero" in str(e), str(e)
                out = ("err", abi.FQ_E_DIVIDE_BY_ZERO)
            except TP.CastNull:
                out = ("err", abi.FQ_E_UNSUPPORTED)
    run._exp[key] = out
    return out


def is_error(P, exp):
    return exp[0] == "err" if P.family == "proj" else bool(exp["flags"] & ERR)


def kept_rows(P, exp):
    if is_error(P, exp):
        return 0
    return sum(exp[2]) if P.family == "proj" else exp["count"]


def canon(P, exp):
    """an expected result as a comparable value (what the device is held to under the program's mask)"""
    if P.family == "proj":
        if exp[0] == "err":
            return exp
        return (tuple(exp[2]), tuple(exp[3]), tuple(b"".join(np.ascontiguousarray(x).tobytes() for x in o) for o in exp[1]))
    if exp["flags"] & ERR:
        return ("err", exp["flags"] & ERR)
    out = [exp["count"], exp.get("valid"), bool(exp["flags"] & abi.STATE_ANY_EMPTY) if P.mask & abi.AGG_SUM else None]
    if exp.get("valid", exp["count"]):
        out.append(exp["dtype"])
        for op, bit in (("sum", abi.AGG_SUM), ("max", abi.AGG_MAX), ("min", abi.AGG_MIN)):
            out.append(repr(exp[op].value) if P.mask & bit else None)
    return tuple(out)


def argument_values(P, run):
    """the valid kept values of the aggregate argument over the whole run (None when the reference raises)"""
    try:
        with np.errstate(all="ignore"):
            val = P.ref()[2][0].eval(block_of(P, run).take(keep_mask(P, run)))
    except R.RefError:
        return None
    return val.values if val.valid is None else val.values[np.asarray(val.valid, bool)]


# ---------------------------------------------------------------------------
# generate
# ---------------------------------------------------------------------------
def prepare(P, block_rows):
    """compile the program's module for gfx950 (no GPU needed); raises FQError when the library refuses it"""
    pred, val = P.device()
    if P.family == "agg":
        return ops.jit_prepare_typed(P.adts, pred=pred, value=val, mask=P.mask, block_rows=block_rows)
    if P.family == "null":
        return ops.jit_prepare_nullable(P.adts, P.nullable, pred=pred, value=val, mask=P.mask, block_rows=block_rows)
    return ops.jit_prepare_project_typed(P.adts, pred=pred, values=val, block_rows=block_rows)


_CACHE = {}


def generate(family, seed, cache=True):
    """(Program, [Run, Run, Run]) of a seed; the same objects every time unless cache=False"""
    if cache and (family, seed) in _CACHE:
        return _CACHE[(family, seed)]
    too_long = amb = 0
    for attempt in range(64):
        rng = np.random.default_rng([FAMILIES.index(family), seed, attempt])
        P = draw_program(rng, family, seed)
        rg = int_range(P)
        draw_consts(rng, P, rg)
        runs = draw_geometry(rng, P)
        for run in runs:
            draw_inputs(rng, P, run, rg)
        set_pred_consts(rng, P, runs[2], rg)
        steer(rng, P, runs[2])
        if any(ambiguous(P, run) for run in runs):
            amb += 1
            continue
        if P.kind == "bitmap":
            for run in runs:
                res = P.ref()[0].eval(block_of(P, run))
                run.keep = np.array(res.values, bool) & (np.ones(run.n, bool) if res.valid is None else np.asarray(res.valid, bool))
        if P.family != "proj" and P.mask & abi.AGG_SUM:
            exps = [expected(P, run) for run in runs]
            t = [NAME[e["dtype"]] for e in exps if e["dtype"] is not None]
            if t and is_float(t[0]) and (max(e["abs"] for e in exps) >= float(np.finfo(R.NP[t[0]]).max) / 4
                                         or any(both_infinities(P, run) for run in runs)):
                P.mask = (P.mask & ~abi.AGG_SUM) or abi.AGG_COUNT
        try:
            prepare(P, 0)
        except FQError as e:
            if e.status == abi.FQ_E_UNSUPPORTED and "too long" in str(e):
                too_long += 1
                continue
            raise AssertionError("%s: refused: %s" % (P.describe(), e))
        P.too_long, P.ambiguous = too_long, amb
        if cache:
            _CACHE[(family, seed)] = (P, runs)
        return P, runs
    raise AssertionError("%s seed %d: no program in 64 draws" % (family, seed))
