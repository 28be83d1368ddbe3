"""GPU: aggregate scans over expressions of several columns through the
Function handles (fq_functions_accumulate over an fq_block with three and more
columns and a pending filter), the boundary a fuse-query host that keeps its own
tables uses.  `[sum(a * b), max(a * b), count(a * b)] WHERE c < k` and
`sum(a + b * c) WHERE a < b or c = 7` must run as ONE fused scan per block that
reads every column once, equal oracle/fq_ref.py, and equal the same handles on
the unfused branch (JIT off: one kernel per expression node, a compaction, an
identity scan)."""
import pytest

import fq_ref as R
from fq_amd import abi

pytestmark = pytest.mark.gpu

ROWS = 20_009
K38 = 3 << 61  # keeps ~3/8 of uniformly random u64 rows
ops = F = ENGINE = None
HOST = {}


def setup_module():
    global ops, F, ENGINE
    from fq_amd import functions as _F
    from fq_amd import ops as _ops
    _ops.require_gpu()
    ops, F = _ops, _F
    ENGINE = _F.Engine(device=0)
    for i, name in enumerate("abcde"):
        HOST[name] = ops.splitmix_column(90 + i, 0, ROWS).to_numpy()
    HOST["c"][::5] = 7


def teardown_module():
    if ENGINE is not None:
        ENGINE.close()


# ---- the same trees on the product's handles (F) and on the oracle (R) ----
class Both:
    """builds a Function tree twice: product handle and oracle object"""

    def __init__(self, product, oracle):
        self.p, self.o = product, oracle


def field(n):
    return Both(F.FieldFunction.try_create(n), R.Field(n))


def const(v):
    return Both(F.ConstantFunction.try_create(F.DataValue("UInt64", v)), R.Const(R.Value("UInt64", v)))


def binop(op, l, r):
    kind = R.Arith if op in "+-*/%" else (R.Logic if op in ("and", "or") else R.Compare)
    return Both(F.ScalarFunctionFactory.get(op, [l.p, r.p]), kind(op, l.o, r.o))


def agg(name, arg):
    return Both(F.AggregatorFunction.try_create(name, [arg.p]), R.Agg(name, arg.o))


def a_times_b():
    return binop("*", field("a"), field("b"))


def q6():
    return [agg("sum", a_times_b()), agg("max", a_times_b()), agg("count", a_times_b())], \
        binop("<", field("c"), const(K38))


def tree():
    arg = binop("+", field("a"), binop("*", field("b"), field("c")))
    where = binop("or", binop("<", field("a"), field("b")), binop("=", field("c"), const(7)))
    return [agg("sum", arg)], where


def five():
    arg = binop("+", binop("+", binop("+", binop("+", field("a"), field("b")), field("c")), field("d")), field("e"))
    return [agg("sum", arg), agg("max", arg)], binop("<", field("c"), const(K38))


def device_block(names, block_rows, where, host=None):
    host = host or HOST
    cols = [ops.from_numpy(host[n], abi.DT_UINT64) for n in names]
    return F.DataBlock(list(names), cols, block_rows=block_rows, filter=where.p)


def oracle_results(names, funcs, where, block_rows, host=None):
    host = host or HOST
    br = block_rows or ROWS
    for s in range(0, ROWS, br):
        blk = R.Block([(n, R.Arr("UInt64", host[n][s:s + br])) for n in names])
        fb = R.filter_block(where.o, blk)
        for f in funcs:
            f.o.accumulate(fb)
    return [(f.o.merge_result().type, f.o.merge_result().value) for f in funcs]


def product_results(funcs, blk):
    F.Function.accumulate_all(ENGINE, [f.p for f in funcs], blk)
    return [(f.p.merge_result().type, f.p.merge_result().value) for f in funcs]


@pytest.mark.parametrize("block_rows", [0, 10000])
@pytest.mark.parametrize("plan", [q6, tree], ids=["q6", "tree"])
def test_one_fused_scan_equals_the_oracle_and_the_unfused_branch(plan, block_rows):
    names = "abc"
    funcs, where = plan()
    want = oracle_results(names, funcs, where, block_rows)
    blk = device_block(names, block_rows, where)
    s0 = ENGINE.stats()
    got = product_results(funcs, blk)
    s1 = ENGINE.stats()
    assert got == want
    assert s1["scan_launches"] - s0["scan_launches"] == 1
    assert s1["scan_bytes"] - s0["scan_bytes"] == 24 * ROWS
    assert s1["scan_rows"] - s0["scan_rows"] == ROWS
    # the same handles on the unfused branch
    unfused, uwhere = plan()
    ops.jit_config(abi.JIT_OFF, 0)
    try:
        ublk = device_block(names, block_rows, uwhere)
        u0 = ENGINE.stats()["scan_launches"]
        ugot = product_results(unfused, ublk)
        u1 = ENGINE.stats()["scan_launches"]
    finally:
        ops.jit_config(abi.JIT_AUTO, 1 << 22)
    assert ugot == want
    assert u1 - u0 > 1  # one scan per aggregator plus the predicate's probe
    assert [f.p.accumulate_result() for f in funcs] == [f.p.accumulate_result() for f in unfused]


@pytest.mark.parametrize("block_rows", [0, 10000])
def test_two_blocks_accumulate_one_launch_each(block_rows):
    funcs, where = q6()
    blk = device_block("abc", block_rows, where)
    s0 = ENGINE.stats()["scan_launches"]
    F.Function.accumulate_all(ENGINE, [f.p for f in funcs], blk)
    F.Function.accumulate_all(ENGINE, [f.p for f in funcs], blk)
    assert ENGINE.stats()["scan_launches"] - s0 == 2
    ref, rwhere = q6()
    oracle_results("abc", ref, rwhere, block_rows)
    want = oracle_results("abc", ref, rwhere, block_rows)  # the oracle's objects keep their state: the second pass
    assert [(f.p.merge_result().type, f.p.merge_result().value) for f in funcs] == want


@pytest.mark.parametrize("block_rows", [0, 10000])
def test_five_column_expression_falls_back_and_answers(block_rows):
    funcs, where = five()
    want = oracle_results("abcde", funcs, where, block_rows)
    blk = device_block("abcde", block_rows, where)
    s0 = ENGINE.stats()["scan_launches"]
    assert product_results(funcs, blk) == want
    assert ENGINE.stats()["scan_launches"] - s0 > 1


def test_filtered_sum_over_an_empty_reference_block_fails_as_the_reference():
    # the second 10,000-row reference block keeps no row: the reference's Sum meets a None block sum
    # (DataValue::to_array) -- through the fused scan over three columns and through the unfused branch
    host = dict(HOST)
    host["c"] = HOST["c"].copy()
    host["c"][10000:20000] = K38
    funcs, where = q6()
    with pytest.raises(R.RefError) as oracle_err:
        oracle_results("abc", funcs[:1], where, 10000, host)
    assert str(oracle_err.value) == "Internal Error: DataValue to array cannot be NONE NULL"
    for mode in (abi.JIT_AUTO, abi.JIT_OFF):
        fs, w = q6()
        ops.jit_config(mode, 1 << 22)
        try:
            blk = device_block("abc", 10000, w, host)
            s0 = ENGINE.stats()["scan_launches"]
            with pytest.raises(F.FQError) as e:
                F.Function.accumulate_all(ENGINE, [f.p for f in fs], blk)
            launches = ENGINE.stats()["scan_launches"] - s0
        finally:
            ops.jit_config(abi.JIT_AUTO, 1 << 22)
        assert str(e.value) == str(oracle_err.value)
        assert (launches == 1) == (mode == abi.JIT_AUTO)
    # max and count skip the empty block
    fs, w = q6()
    want = oracle_results("abc", fs[1:], w, 10000, host)
    assert product_results(fs[1:], device_block("abc", 10000, w, host)) == want
