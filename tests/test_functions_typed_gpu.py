"""GPU: aggregate scans over narrow and mixed-width columns through the Function
handles (fq_functions_accumulate over an fq_block whose fields are Float64,
Float32, Int32, UInt8, UInt32, Int16 and a pending filter): the boundary a
fuse-query host that keeps its own tables uses, with dates as Int32, quantities
as UInt8 and discounts as Float32.  Each distinct aggregate argument must run as
ONE fused scan per block that reads every column once at its own width
(fq_aggregate_typed), equal oracle/fq_ref.py, and equal the same handles on the
unfused branch (JIT off: one kernel per expression node, a compaction, an
identity scan).  A fifth column takes the unfused branch."""
import numpy as np
import pytest

import fq_ref as R
from fq_amd import abi

pytestmark = pytest.mark.gpu

ROWS = 20_009
ops = F = ENGINE = None
HOST = {}
TYPES = {"price": "Float64", "discount": "Float32", "shipdate": "Int32", "quantity": "UInt8",
         "a": "UInt32", "b": "Int16", "n1": "UInt8", "n2": "UInt8", "n3": "UInt16", "n4": "UInt8", "n5": "UInt16", "w": "UInt32", "f": "Float32"}


def setup_module():
    global ops, F, ENGINE
    from fq_amd import functions as _F
    from fq_amd import ops as _ops
    _ops.require_gpu()
    ops, F = _ops, _F
    ENGINE = _F.Engine(device=0)
    rng = np.random.default_rng(2024)
    HOST["price"] = rng.uniform(1.0, 1000.0, ROWS)
    HOST["discount"] = (rng.integers(0, 11, ROWS) / 100.0).astype(np.float32)
    HOST["shipdate"] = rng.integers(8000, 10600, ROWS).astype(np.int32)
    HOST["quantity"] = rng.integers(1, 51, ROWS).astype(np.uint8)
    HOST["a"] = rng.integers(0, 100, ROWS).astype(np.uint32)   # every value casts to Int16
    HOST["b"] = rng.integers(-100, 100, ROWS).astype(np.int16)
    HOST["n1"] = rng.integers(0, 256, ROWS).astype(np.uint8)   # unsigned throughout: every cast widens
    HOST["n2"] = rng.integers(0, 256, ROWS).astype(np.uint8)
    HOST["n3"] = rng.integers(0, 65536, ROWS).astype(np.uint16)
    HOST["n4"] = rng.integers(0, 128, ROWS).astype(np.uint8)
    HOST["n5"] = rng.integers(0, 65536, ROWS).astype(np.uint16)
    HOST["w"] = rng.integers(0, 1 << 20, ROWS).astype(np.uint32)
    HOST["f"] = rng.integers(-1000, 1000, ROWS).astype(np.float32)


def teardown_module():
    if ENGINE is not None:
        ENGINE.close()


class Both:
    """builds a Function tree twice: product handle and oracle object"""

    def __init__(self, product, oracle):
        self.p, self.o = product, oracle


def field(n):
    return Both(F.FieldFunction.try_create(n), R.Field(n))


def const(v, t):
    return Both(F.ConstantFunction.try_create(F.DataValue(t, v)), R.Const(R.Value(t, v)))


def binop(op, l, r):
    kind = R.Arith if op in "+-*/%" else (R.Logic if op in ("and", "or") else R.Compare)
    return Both(F.ScalarFunctionFactory.get(op, [l.p, r.p]), kind(op, l.o, r.o))


def agg(name, arg):
    return Both(F.AggregatorFunction.try_create(name, [arg.p]), R.Agg(name, arg.o))


def q6():
    """[sum, max, count](price * discount) WHERE shipdate < k and quantity < q: one argument, one scan of 17 B rows"""
    def arg():
        return binop("*", field("price"), field("discount"))
    where = binop("and", binop("<", field("shipdate"), const(9950, "Int32")),
                  binop("<", field("quantity"), const(26, "UInt8")))
    return ["price", "discount", "shipdate", "quantity"], [agg("sum", arg()), agg("max", arg()), agg("count", arg())], where


def ab():
    """sum(a * b), max(a + b) WHERE a < b over UInt32 a, Int16 b: every step and the comparison in Int16;
    two arguments, one scan of 6 B rows each"""
    funcs = [agg("sum", binop("*", field("a"), field("b"))), agg("max", binop("+", field("a"), field("b")))]
    return ["a", "b"], funcs, binop("<", field("a"), field("b"))


def five():
    arg = binop("+", binop("+", binop("+", binop("+", field("n1"), field("n2")), field("n3")), field("n4")), field("n5"))
    return ["n1", "n2", "n3", "n4", "n5"], [agg("sum", arg), agg("max", arg)], binop("<", field("n4"), const(48, "UInt8"))


def long_chain():
    """n1 + n3 + w + 1:UInt64 + (-1):Int64 + f + 1.5:Float64 + 1.0:Float64 over UInt8, UInt16, UInt32, Float32:
    seven steps (within FQ_MAX_STEPS) whose type changes six times -- thirteen lowered steps, one more than the
    lowered program holds, so the block takes the unfused branch.  Every value is a multiple of 0.5 below 2^22:
    the Float64 sum is exact in any order."""
    def arg():
        e = binop("+", binop("+", field("n1"), field("n3")), field("w"))
        e = binop("+", binop("+", e, const(1, "UInt64")), const(-1, "Int64"))
        return binop("+", binop("+", binop("+", e, field("f")), const(1.5, "Float64")), const(1.0, "Float64"))
    return ["n1", "n3", "w", "f"], [agg("sum", arg()), agg("max", arg())], binop("<", field("n1"), const(100, "UInt8"))


def device_block(names, block_rows, where):
    cols = [ops.from_numpy(HOST[n], abi.DT_BY_NAME[TYPES[n]]) for n in names]
    return F.DataBlock(list(names), cols, block_rows=block_rows, filter=where.p)


def oracle_results(names, funcs, where, block_rows):
    br = block_rows or ROWS
    for s in range(0, ROWS, br):
        blk = R.Block([(n, R.Arr(TYPES[n], HOST[n][s:s + br])) for n in names])
        fb = R.filter_block(where.o, blk)
        for f in funcs:
            f.o.accumulate(fb)
    return [(f.o.merge_result().type, f.o.merge_result().value) for f in funcs]


def product_results(funcs, blk):
    F.Function.accumulate_all(ENGINE, [f.p for f in funcs], blk)
    return [(f.p.merge_result().type, f.p.merge_result().value) for f in funcs]


def kept_abs_sum():
    """sum |price * discount| over the kept rows: the scale of the Float64 sum's bound"""
    keep = (HOST["shipdate"] < 9950) & (HOST["quantity"] < 26)
    return float(np.abs(HOST["price"][keep] * HOST["discount"][keep].astype(np.float64)).sum())


def same(got, want, what):
    """integer results, max/min and counts exactly; a Float64 sum within 1e-12 * sum(|x|)
    (tests/test_kernels_gpu.py): the scans add in another order than the oracle"""
    assert len(got) == len(want)
    for i, ((gt, gv), (wt, wv)) in enumerate(zip(got, want)):
        assert gt == wt, (what, i, gt, wt)
        if gt == "Float64" and i == 0:
            bound = 1e-12 * kept_abs_sum()
            print("%s Float64 sum: got %r want %r error %r bound %r" % (what, gv, wv, abs(gv - wv), bound))
            assert abs(gv - wv) <= bound, (what, gv, wv, bound)
        else:
            assert gv == wv, (what, i, gv, wv)


@pytest.mark.parametrize("block_rows", [0, 10000])
@pytest.mark.parametrize("plan,row_bytes,scans", [(q6, 17, 1), (ab, 6, 2)], ids=["q6", "u32_i16"])
def test_typed_fused_scan_equals_the_oracle_and_the_unfused_branch(plan, row_bytes, scans, block_rows):
    names, funcs, where = plan()
    want = oracle_results(names, funcs, where, block_rows)
    blk = device_block(names, block_rows, where)
    j0 = ops.jit_stats()["jit_launches"]
    s0 = ENGINE.stats()
    got = product_results(funcs, blk)
    s1 = ENGINE.stats()
    same(got, want, "fused")
    # one scan launch per distinct argument, each reading every column once at its own width
    assert s1["scan_launches"] - s0["scan_launches"] == scans
    assert s1["scan_bytes"] - s0["scan_bytes"] == scans * row_bytes * ROWS
    assert s1["scan_rows"] - s0["scan_rows"] == scans * ROWS
    assert ops.jit_stats()["jit_launches"] - j0 == scans
    # the same handles on the unfused branch
    _, unfused, uwhere = plan()
    ops.jit_config(abi.JIT_OFF, 0)
    try:
        ublk = device_block(names, block_rows, uwhere)
        u0 = ENGINE.stats()["scan_launches"]
        ugot = product_results(unfused, ublk)
        u1 = ENGINE.stats()["scan_launches"]
    finally:
        ops.jit_config(abi.JIT_AUTO, 1 << 22)
    same(ugot, want, "unfused")
    assert u1 - u0 > scans  # one scan per aggregator plus the predicate's probe
    same([(g[0], g[1]) for g in got], ugot, "fused against unfused")


@pytest.mark.parametrize("block_rows", [0, 10000])
def test_each_argument_alone_is_one_launch(block_rows):
    names, funcs, where = ab()
    want = oracle_results(names, funcs, where, block_rows)
    for i, f in enumerate(funcs):
        blk = device_block(names, block_rows, where)
        s0 = ENGINE.stats()
        got = product_results([f], blk)
        s1 = ENGINE.stats()
        assert got == [want[i]]
        assert s1["scan_launches"] - s0["scan_launches"] == 1
        assert s1["scan_bytes"] - s0["scan_bytes"] == 6 * ROWS


@pytest.mark.parametrize("block_rows", [0, 10000])
def test_a_fifth_column_takes_the_unfused_branch(block_rows):
    names, funcs, where = five()
    want = oracle_results(names, funcs, where, block_rows)
    blk = device_block(names, block_rows, where)
    s0 = ENGINE.stats()["scan_launches"]
    assert product_results(funcs, blk) == want
    assert ENGINE.stats()["scan_launches"] - s0 > 1


@pytest.mark.parametrize("block_rows", [0, 10000])
def test_a_chain_whose_casts_do_not_fit_takes_the_unfused_branch(block_rows):
    names, funcs, where = long_chain()
    want = oracle_results(names, funcs, where, block_rows)
    assert want[0][0] == "Float64" and ROWS * float(1 << 22) < 2.0 ** 52
    blk = device_block(names, block_rows, where)
    s0 = ENGINE.stats()["scan_launches"]
    assert product_results(funcs, blk) == want
    assert ENGINE.stats()["scan_launches"] - s0 > 1  # not the one fused scan
    # the lowering itself refuses the shape: what the engine asked before it chose the branch
    from fq_amd._lib import FQError
    from fq_amd.expr import Col, chain_columns
    dts = [abi.DT_UINT8, abi.DT_UINT16, abi.DT_UINT32, abi.DT_FLOAT32]
    value, vdt = chain_columns(dts, [("+", Col(1)), ("+", Col(2)), ("+", 1), ("+", -1), ("+", Col(3)), ("+", 1.5), ("+", 1.0)])
    assert vdt == abi.DT_FLOAT64
    with pytest.raises(FQError) as e:
        ops.jit_prepare_typed(dts, value=value)
    assert e.value.status == abi.FQ_E_UNSUPPORTED and "too long" in str(e.value)
    # the same handles with the JIT off: the same branch, the same bytes
    _, unfused, uwhere = long_chain()
    ops.jit_config(abi.JIT_OFF, 0)
    try:
        ugot = product_results(unfused, device_block(names, block_rows, uwhere))
    finally:
        ops.jit_config(abi.JIT_AUTO, 1 << 22)
    assert ugot == want


@pytest.mark.parametrize("block_rows", [0, 10000])
def test_a_wide_integer_constant_in_a_float32_step_rounds_once(block_rows):
    # 2^60 + 2^36 + 1 lies just above a binary32 tie; through binary64 it would land on the tie and round down
    k = (1 << 60) + (1 << 36) + 1
    assert float(np.float32(np.uint64(k))) == float((1 << 60) + (1 << 37)) != float(np.float32(np.float64(k)))

    def plan():
        return [agg("max", binop("+", field("f"), const(k, "UInt64")))], binop("<", field("quantity"), const(26, "UInt8"))
    funcs, where = plan()
    names = ["quantity", "f"]
    want = oracle_results(names, funcs, where, block_rows)
    assert want == [("Float32", float((1 << 60) + (1 << 37)))]
    s0 = ENGINE.stats()["scan_launches"]
    assert product_results(funcs, device_block(names, block_rows, where)) == want
    assert ENGINE.stats()["scan_launches"] - s0 == 1
    unfused, uwhere = plan()
    ops.jit_config(abi.JIT_OFF, 0)
    try:
        assert product_results(unfused, device_block(names, block_rows, uwhere)) == want
    finally:
        ops.jit_config(abi.JIT_AUTO, 1 << 22)


def test_a_lone_narrow_column_keeps_the_precompiled_identity_scan():
    # sum(quantity) without WHERE: one launch of 1 B rows, not a hipRTC kernel
    f = agg("sum", field("quantity"))
    for s in range(0, ROWS, 10000):
        f.o.accumulate(R.Block([("quantity", R.Arr("UInt8", HOST["quantity"][s:s + 10000]))]))
    cols = [ops.from_numpy(HOST["quantity"], abi.DT_UINT8)]
    blk = F.DataBlock(["quantity"], cols, block_rows=10000)
    j0 = ops.jit_stats()["jit_launches"]
    s0 = ENGINE.stats()
    F.Function.accumulate_all(ENGINE, [f.p], blk)
    s1 = ENGINE.stats()
    assert s1["scan_launches"] - s0["scan_launches"] == 1 and s1["scan_bytes"] - s0["scan_bytes"] == ROWS
    assert ops.jit_stats()["jit_launches"] == j0
    assert (f.p.merge_result().type, f.p.merge_result().value) == (f.o.merge_result().type, f.o.merge_result().value)
