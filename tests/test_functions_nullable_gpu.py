"""GPU: aggregate scans over nullable columns through the Function handles
(fq_functions_accumulate_nullable over an fq_block and its Arrow validity
bitmaps) and the state protocol, against oracle/fq_ref.py's Agg functions over
the same blocks as R.Arr(type, values, valid).  Each distinct argument is ONE
fq_aggregate_nullable scan; Count adds the kept rows (nulls included), Min /
Max / Sum see None for a block without a valid kept value (a Sum over >= 2
blocks then fails as the reference does); an overflowing cast is a null, where
fq_functions_accumulate still refuses it; a statement that does not fuse fails
with FQ_E_UNSUPPORTED.  The values under 0 bits are garbage.

For an and / or filter the oracle's kept rows are AND-ed with the validity of
every leaf's comparison (tests/test_scan_nullable_gpu.py says why)."""
import numpy as np
import pytest

import fq_ref as R
from fq_amd import abi

pytestmark = pytest.mark.gpu

ROWS = 25_003
ops = F = ENGINE = None
HOST, VALID = {}, {}
TYPES = {"x": "Int32", "price": "Float64", "discount": "Float32", "shipdate": "Int32", "quantity": "UInt8",
         "a": "UInt64", "b": "Int8", "n1": "UInt8", "n2": "UInt8", "n3": "UInt16", "n4": "UInt8", "n5": "UInt16"}


def setup_module():
    global ops, F, ENGINE
    from fq_amd import functions as _F
    from fq_amd import ops as _ops
    _ops.require_gpu()
    ops, F = _ops, _F
    ENGINE = _F.Engine(device=0)
    rng = np.random.default_rng(2025)
    HOST["x"] = rng.integers(-1000000, 1000000, ROWS).astype(np.int32)
    HOST["price"] = rng.uniform(1.0, 1000.0, ROWS)
    HOST["discount"] = (rng.integers(0, 11, ROWS) / 100.0).astype(np.float32)
    HOST["shipdate"] = rng.integers(8000, 10600, ROWS).astype(np.int32)
    HOST["quantity"] = rng.integers(1, 51, ROWS).astype(np.uint8)
    HOST["a"] = rng.integers(0, 100, ROWS).astype(np.uint64)
    HOST["a"][::7] = 1 << 63  # Int8 + UInt64 is computed in Int8: these rows (and 200) are nulls
    HOST["a"][3::11] = 200
    HOST["b"] = rng.integers(-100, 100, ROWS).astype(np.int8)
    for n in ("n1", "n2", "n4"):
        HOST[n] = rng.integers(0, 100, ROWS).astype(np.uint8)
    for n in ("n3", "n5"):
        HOST[n] = rng.integers(0, 1000, ROWS).astype(np.uint16)
    garbage = {"x": [-(1 << 31), (1 << 31) - 1], "price": [np.nan, np.inf, -np.inf, 1e308], "discount": [np.nan, np.inf],
               "shipdate": [-(1 << 31), 0], "quantity": [0, 255]}
    for j, n in enumerate(("x", "price", "discount", "shipdate", "quantity")):
        v = np.random.default_rng(77 + j).random(ROWS) >= 0.3
        bad = np.flatnonzero(~v)
        g = np.array(garbage[n], dtype=HOST[n].dtype)
        HOST[n][bad] = g[np.arange(len(bad)) % len(g)]
        VALID[n] = v


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


def bitmap_dev(valid):
    if valid is None:
        return None
    n = len(valid)
    bits = np.ones(((n + 63) // 64) * 64, bool)
    bits[:n] = valid
    return ops.from_numpy(np.packbits(bits, bitorder="little").view(np.uint64), abi.DT_UINT64)


def device_block(names, block_rows, where, host=HOST):
    cols = [ops.from_numpy(host[n], abi.DT_BY_NAME[TYPES[n]]) for n in names]
    return F.DataBlock(list(names), cols, block_rows=block_rows, filter=where.p if where is not None else None)


def oracle_results(names, funcs, where, leaves, block_rows, valid, host=HOST):
    rows = len(host[names[0]])
    br = block_rows or rows
    for s in range(0, rows, br):
        blk = R.Block([(n, R.Arr(TYPES[n], host[n][s:s + br], None if valid.get(n) is None else valid[n][s:s + br]))
                       for n in names])
        fb = blk
        if where is not None and leaves is None:
            fb = R.filter_block(where.o, blk)
        elif where is not None:
            keep = np.array(where.o.eval(blk).values, bool)
            for lf in leaves:
                lv = lf.o.eval(blk).valid
                if lv is not None:
                    keep &= np.asarray(lv, bool)
            fb = blk.take(keep)
        for f in funcs:
            f.o.accumulate(fb)
    return [(f.o.merge_result().type, f.o.merge_result().value) for f in funcs]


def product_results(funcs, blk, bitmaps):
    F.Function.accumulate_all_nullable(ENGINE, [f.p for f in funcs], blk, bitmaps)
    return [(f.p.merge_result().type, f.p.merge_result().value) for f in funcs]


def c3():
    def x():
        return field("x")
    return [binop("/", agg("sum", x()), agg("count", x())), agg("max", x()), agg("min", x())]


@pytest.mark.parametrize("block_rows", [10000, 0])
def test_sum_count_max_min_of_a_nullable_column_is_one_fused_scan(block_rows):
    funcs = c3()
    want = oracle_results(["x"], funcs, None, None, block_rows, VALID)
    blk = device_block(["x"], block_rows, None)
    s0 = ENGINE.stats()
    got = product_results(funcs, blk, [bitmap_dev(VALID["x"])])
    s1 = ENGINE.stats()
    assert got == want
    assert s1["scan_launches"] - s0["scan_launches"] == 1
    assert s1["scan_rows"] - s0["scan_rows"] == ROWS
    assert s1["scan_bytes"] - s0["scan_bytes"] == 4 * ROWS + (ROWS + 7) // 8  # the column and a bit per row
    # count includes the null rows
    cnt = [agg("count", field("x"))]
    assert product_results(cnt, device_block(["x"], block_rows, None), [bitmap_dev(VALID["x"])]) == [("UInt64", ROWS)]


def test_one_whole_block_null():
    from fq_amd._lib import FQError
    valid = {"x": VALID["x"].copy()}
    valid["x"][10000:20000] = False
    host = {"x": HOST["x"].copy()}
    host["x"][10000:20000] = -(1 << 31)
    bm = bitmap_dev(valid["x"])
    funcs = c3()
    with pytest.raises(R.RefError) as oe:
        oracle_results(["x"], funcs, None, None, 10000, valid, host)
    assert "DataValue to array cannot be NONE NULL" in str(oe.value)
    with pytest.raises(FQError) as e:
        product_results(c3(), device_block(["x"], 10000, None, host), [bm])
    assert "DataValue to array cannot be NONE NULL" in str(e.value)
    rest = [agg("max", field("x")), agg("min", field("x")), agg("count", field("x"))]
    want = oracle_results(["x"], rest, None, None, 10000, valid, host)
    assert want[2] == ("UInt64", ROWS)
    s0 = ENGINE.stats()["scan_launches"]
    assert product_results(rest, device_block(["x"], 10000, None, host), [bm]) == want
    assert ENGINE.stats()["scan_launches"] - s0 == 1


def test_a_single_all_null_block():
    n = 1000
    host = {"x": np.full(n, -(1 << 31), np.int32)}
    valid = {"x": np.zeros(n, bool)}
    funcs = [agg("sum", field("x")), agg("max", field("x")), agg("min", field("x")), agg("count", field("x"))]
    want = oracle_results(["x"], funcs, None, None, 0, valid, host)
    assert want == [("Int32", None), ("Int32", None), ("Int32", None), ("UInt64", n)]
    assert product_results(funcs, device_block(["x"], 0, None, host), [bitmap_dev(valid["x"])]) == want


@pytest.mark.parametrize("block_rows", [0, 10000])
def test_q6_with_four_bitmaps(block_rows):
    names = ["price", "discount", "shipdate", "quantity"]

    def arg():
        return binop("*", field("price"), field("discount"))
    leaves = [binop("<", field("shipdate"), const(9950, "Int32")), binop("<", field("quantity"), const(26, "UInt8"))]
    where = binop("and", leaves[0], leaves[1])
    funcs = [agg("sum", arg()), agg("max", arg()), agg("min", arg()), agg("count", arg())]
    want = oracle_results(names, funcs, where, leaves, block_rows, VALID)
    keep = (HOST["shipdate"] < 9950) & (HOST["quantity"] < 26) & VALID["shipdate"] & VALID["quantity"]
    ok = keep & VALID["price"] & VALID["discount"]
    assert want[3] == ("UInt64", int(keep.sum())) and 0 < ok.sum() < keep.sum()
    s0 = ENGINE.stats()
    got = product_results(funcs, device_block(names, block_rows, where), [bitmap_dev(VALID[n]) for n in names])
    s1 = ENGINE.stats()
    assert s1["scan_launches"] - s0["scan_launches"] == 1
    assert s1["scan_bytes"] - s0["scan_bytes"] == 17 * ROWS + 4 * ((ROWS + 7) // 8)
    bound = 1e-12 * float(np.abs(HOST["price"][ok] * HOST["discount"][ok].astype(np.float64)).sum())
    assert got[0][0] == want[0][0] == "Float64" and abs(got[0][1] - want[0][1]) <= bound, (got[0], want[0], bound)
    assert got[1:] == want[1:]


@pytest.mark.parametrize("block_rows", [0, 10000])
def test_an_overflowing_cast_is_a_null_here_and_still_refused_by_the_plain_call(block_rows):
    from fq_amd._lib import FQError
    names = ["a", "b"]

    def funcs():
        def arg():
            return binop("+", field("a"), field("b"))
        return [agg("sum", arg()), agg("max", arg()), agg("count", arg())]
    fs = funcs()
    want = oracle_results(names, fs, None, None, block_rows, {})
    assert want[0][0] == "Int8" and want[2] == ("UInt64", ROWS)
    s0 = ENGINE.stats()["scan_launches"]
    assert product_results(fs, device_block(names, block_rows, None), [None, None]) == want
    assert ENGINE.stats()["scan_launches"] - s0 == 1
    with pytest.raises(FQError) as e:
        F.Function.accumulate_all(ENGINE, [f.p for f in funcs()], device_block(names, block_rows, None))
    assert e.value.status == abi.FQ_E_UNSUPPORTED and "cast produced nulls" in str(e.value)


def test_statements_that_do_not_fuse_are_unsupported():
    from fq_amd._lib import FQError
    names = ["n1", "n2", "n3", "n4", "n5"]
    arg = binop("+", binop("+", binop("+", binop("+", field("n1"), field("n2")), field("n3")), field("n4")), field("n5"))
    where = binop("<", field("n4"), const(48, "UInt8"))
    with pytest.raises(FQError) as e:
        product_results([agg("sum", arg)], device_block(names, 0, where), [None] * 5)
    assert e.value.status == abi.FQ_E_UNSUPPORTED and "does not fuse" in str(e.value)
    ops.jit_config(abi.JIT_OFF, 0)
    try:
        with pytest.raises(FQError) as e:
            product_results([agg("sum", field("x"))], device_block(["x"], 0, None), [bitmap_dev(VALID["x"])])
        assert e.value.status == abi.FQ_E_UNSUPPORTED and "hipRTC" in str(e.value)
    finally:
        ops.jit_config(abi.JIT_AUTO, 1 << 22)
    with pytest.raises(FQError) as e:  # a misaligned bitmap
        product_results([agg("sum", field("x"))], device_block(["x"], 0, None), [bitmap_dev(VALID["x"]).ptr + 4])
    assert e.value.status == abi.FQ_E_INVALID and "aligned" in str(e.value)
