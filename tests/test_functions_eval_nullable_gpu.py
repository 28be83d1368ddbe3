"""GPU: ProjectionTransform's loop body over a block of nullable columns through
the Function handles (fq_functions_eval_nullable over an fq_block, its pending
filter and its Arrow validity bitmaps), against the oracle of
tests/project_nullable_cases.py over the same Q6 block: per reference block
R.filter_block / the leaf validities, each expression's values and validity on
the filtered block.  Values are compared bit for bit where the expected bit is
1, the bitmaps as whole words, the counts per block.  The contiguous form is
refused, a statement that does not fuse is refused with its reason, and with no
bitmap at all an overflowing cast is a null bit where fq_functions_eval fails
with "cast produced nulls"."""
import numpy as np
import pytest

import project_nullable_cases as PC
from fq_amd import abi
from fq_amd._lib import FQError

pytestmark = pytest.mark.gpu

N, BR = 25003, 10000
FILL = PC.FILL
ops = F = ENGINE = None


def setup_module():
    global ops, F, ENGINE
    from fq_amd import functions as _F
    from fq_amd import ops as _ops
    _ops.require_gpu()
    ops, F = _ops, _F
    ENGINE = _F.Engine(device=0)


def teardown_module():
    if ENGINE is not None:
        ENGINE.close()


def field(n):
    return F.FieldFunction.try_create(n)


def const(v, t):
    return F.ConstantFunction.try_create(F.DataValue(t, v))


def fn(op, l, r):
    return F.ScalarFunctionFactory.get(op, [l, r])


def bitmap_dev(valid):
    return None if valid is None else ops.from_numpy(PC.pack_bits(valid, pad=True), abi.DT_UINT64)


def block_of(case, where):
    cols = [ops.from_numpy(h, dt) for h, dt in zip(case.host, case.dts)]
    return F.DataBlock(list(case.names), cols, block_rows=BR, filter=where)


def q6_functions():
    where = fn("and", fn("<", field("shipdate"), const(9950, "Int32")), fn("<", field("quantity"), const(26, "UInt8")))
    funcs = [fn("*", field("price"), field("discount")), field("quantity"), fn("*", field("discount"), field("discount"))]
    return where, funcs


def check(case, cols, bitmaps, counts, out_validity=None):
    want = case.oracle(BR)
    assert list(counts) == want["counts"]
    nw = (case.n + 63) // 64
    sentinel = int(np.full(8, FILL, np.uint8).view(np.uint64)[0])
    for j, (c, bm) in enumerate(zip(cols, bitmaps)):
        dt = want["dts"][j]
        assert c.dtype == dt, j
        words = bm.to_numpy()
        assert int(words[nw]) == sentinel, j
        if out_validity is None or out_validity[j] is not None:
            assert np.array_equal(words[:nw], PC.pack_bits(want["bits"][j])), j
        got = c.to_numpy()
        assert PC.same(got, want["rows"][j], dt, want["bits"][j]), j
        fill = np.full(case.n * got.dtype.itemsize, FILL, np.uint8).view(got.dtype)
        assert PC.same(got, fill, dt, ~want["kept"]), j  # rows past a count keep the fill


@pytest.mark.parametrize("pattern", ["random", "last", "ones"])
def test_q6_block_through_function_handles(pattern):
    case = PC.get_case("q6", N, pattern)
    where, funcs = q6_functions()
    blk = block_of(case, where)
    # the block's columns are price, discount, shipdate, quantity; the kernel numbers the filter's first
    cols, bitmaps, counts = F.Function.eval_all_nullable(ENGINE, funcs, blk, [bitmap_dev(v) for v in case.valid], fill=FILL)
    check(case, cols, bitmaps, counts)


def test_the_contiguous_form_is_refused():
    case = PC.get_case("q6", N, "random")
    where, funcs = q6_functions()
    with pytest.raises(FQError) as e:
        F.Function.eval_all_nullable(ENGINE, funcs, block_of(case, where), [bitmap_dev(v) for v in case.valid], blocks=False)
    assert e.value.status == abi.FQ_E_UNSUPPORTED and "contiguous nullable projection is not built" in str(e.value)


def test_a_fifth_column_is_refused_by_name():
    rng = np.random.default_rng(5)
    names = ["c0", "c1", "c2", "c3", "c4"]
    cols = [ops.from_numpy(rng.integers(0, 100, N).astype(np.uint8), abi.DT_UINT8) for _ in names]
    blk = F.DataBlock(names, cols, block_rows=BR, filter=fn("<", field("c0"), const(50, "UInt8")))
    total = field("c1")
    for n in names[2:]:
        total = fn("+", total, field(n))
    with pytest.raises(FQError) as e:
        F.Function.eval_all_nullable(ENGINE, [total], blk, [None] * 5)
    msg = str(e.value)
    assert e.value.status == abi.FQ_E_UNSUPPORTED and "fq_functions_eval_nullable" in msg
    assert "more than 4 columns" in msg and "no unfused path" in msg, msg
    # four columns of the same statement fuse
    four = fn("+", fn("+", field("c1"), field("c2")), field("c3"))
    cols4, bitmaps, counts = F.Function.eval_all_nullable(ENGINE, [four], blk, [None] * 5)
    assert int(counts.sum()) > 0


def test_the_jit_off_is_refused():
    case = PC.get_case("q6", N, "random")
    where, funcs = q6_functions()
    ops.jit_config(abi.JIT_OFF, 0)
    try:
        with pytest.raises(FQError) as e:
            F.Function.eval_all_nullable(ENGINE, funcs, block_of(case, where), [bitmap_dev(v) for v in case.valid])
        assert e.value.status == abi.FQ_E_UNSUPPORTED and "hipRTC kernels are off" in str(e.value)
    finally:
        ops.jit_config(abi.JIT_AUTO, 1 << 22)


def test_without_bitmaps_an_overflowing_cast_is_a_null_not_an_error():
    case = PC.get_case("u64cast", N, "none")  # x + 1 as Int64, x WHERE x % 8 < 3; some kept x are 2^63 and above
    where = fn("<", fn("%", field("x"), const(8, "UInt64")), const(3, "UInt64"))
    funcs = [fn("+", field("x"), const(1, "Int64")), field("x")]
    want = case.oracle(BR)
    assert (want["kept"] & ~want["bits"][0]).sum() > 50
    blk = block_of(case, where)
    cols, bitmaps, counts = F.Function.eval_all_nullable(ENGINE, funcs, blk, [None], fill=FILL)
    check(case, cols, bitmaps, counts)
    # x itself cannot be null: its bitmap may be left out
    cols, bitmaps, counts = F.Function.eval_all_nullable(ENGINE, funcs, blk, [None], fill=FILL, out_validity=[True, None])
    check(case, cols, bitmaps, counts, out_validity=[True, None])
    with pytest.raises(FQError) as e:
        F.Function.eval_all(ENGINE, funcs, blk, blocks=True)
    assert "cast produced nulls" in str(e.value)
