"""GPU: ProjectionTransform's loop for one block through the Function handles
(fq_functions_eval over an fq_block with several columns and a pending
filter), the boundary a fuse-query host that keeps its own tables uses.
`[a * b, a + c, c] WHERE c < k` and `[a + b * c] WHERE a < b or c = 7` must run
as ONE fused kernel (fused == 1), equal oracle/fq_ref.py per reference block
(R.Block -> R.filter_block -> Fn.eval), equal the same handles on the unfused
branch (JIT off) bit for bit, and equal n separate Function.eval calls."""
import numpy as np
import pytest

import fq_ref as R
from fq_amd import abi

pytestmark = pytest.mark.gpu

ROWS = 20_009
K38 = 3 << 61  # keeps ~3/8 of uniformly random u64 rows
NP = {"UInt64": np.uint64, "Int64": np.int64, "Float64": np.float64}
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
        HOST[name] = ops.splitmix_column(190 + i, 0, ROWS).to_numpy()
    HOST["c"][::5] = 7


def teardown_module():
    if ENGINE is not None:
        ENGINE.close()


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


def q6():
    return [binop("*", field("a"), field("b")), binop("+", field("a"), field("c")), field("c")], \
        binop("<", field("c"), const(K38))


def tree():
    return [binop("+", field("a"), binop("*", field("b"), field("c")))], \
        binop("or", binop("<", field("a"), field("b")), binop("=", field("c"), const(7)))


def five():
    e = binop("+", binop("+", binop("+", binop("+", field("a"), field("b")), field("c")), field("d")), field("e"))
    return [e, binop("*", field("a"), field("b"))], binop("<", field("c"), const(K38))


def device_block(names, block_rows, where, host=None):
    host = host or HOST
    cols = [ops.from_numpy(host[n], abi.DT_UINT64) for n in names]
    return F.DataBlock(list(names), cols, block_rows=block_rows, filter=where.p if where is not None else None)


def oracle(names, funcs, where, block_rows, host=None):
    """per reference block: ([(type, values) per function], rows kept)"""
    host = host or HOST
    br = block_rows or ROWS
    blocks = []
    for s in range(0, ROWS, br):
        blk = R.Block([(n, R.Arr("UInt64", host[n][s:s + br])) for n in names])
        fb = R.filter_block(where.o, blk) if where is not None else blk
        outs = []
        for f in funcs:
            v = f.o.eval(fb)
            if not isinstance(v, R.Arr):
                v = R.to_array(v, fb.num_rows())
            outs.append((v.type, np.asarray(v.values)))
        blocks.append((outs, fb.num_rows()))
    return blocks


def concat(blocks, j):
    return np.concatenate([b[0][j][1] for b in blocks])


def host_of(col):
    return col.to_numpy()


def same(col, typ, values):
    got = host_of(col)
    if typ == "Boolean":
        return col.dtype == abi.DT_BOOLEAN and np.array_equal(got, values.astype(bool))
    return col.dtype == abi.DT_BY_NAME[typ] and np.array_equal(got.view(np.uint64), values.astype(NP[typ]).view(np.uint64))


@pytest.mark.parametrize("block_rows", [0, 10000])
@pytest.mark.parametrize("plan", [q6, tree], ids=["q6", "tree"])
def test_one_fused_kernel_equals_the_oracle_the_unfused_branch_and_separate_evals(plan, block_rows):
    funcs, where = plan()
    want = oracle("abc", funcs, where, block_rows)
    kept = sum(b[1] for b in want)
    blk = device_block("abc", block_rows, where)
    cols, fused = F.Function.eval_all(ENGINE, [f.p for f in funcs], blk)
    assert fused
    for j, c in enumerate(cols):
        assert c.len == kept and same(c, want[0][0][j][0], concat(want, j)), j
    # the same handles on the unfused branch
    ops.jit_config(abi.JIT_OFF, 0)
    try:
        ucols, ufused = F.Function.eval_all(ENGINE, [f.p for f in funcs], blk)
    finally:
        ops.jit_config(abi.JIT_AUTO, 1 << 22)
    assert not ufused
    for c, u in zip(cols, ucols):
        assert c.dtype == u.dtype and c.len == u.len
        assert np.array_equal(host_of(c).view(np.uint64), host_of(u).view(np.uint64))
    # n separate Function.eval calls
    for c, f in zip(cols, funcs):
        one = f.p.eval(ENGINE, blk)
        assert one.dtype == c.dtype and one.len == c.len
        assert np.array_equal(host_of(c).view(np.uint64), host_of(one).view(np.uint64))


def test_block_geometry_counts_rows_and_stats():
    funcs, where = q6()
    want = oracle("abc", funcs, where, 10000)
    blk = device_block("abc", 10000, where)
    s0 = ENGINE.stats()
    cols, counts, fused = F.Function.eval_all(ENGINE, [f.p for f in funcs], blk, blocks=True)
    s1 = ENGINE.stats()
    assert fused
    assert list(counts) == [b[1] for b in want]
    for j, c in enumerate(cols):
        got = host_of(c).view(np.uint64)
        assert c.len == ROWS
        for b, (outs, rows) in enumerate(want):
            assert np.array_equal(got[b * 10000:b * 10000 + rows], outs[j][1].astype(np.uint64)), (j, b)
    kept = int(counts.sum())
    assert s1["project_launches"] - s0["project_launches"] == 1
    assert s1["project_bytes"] - s0["project_bytes"] == 8 * 3 * ROWS + 8 * len(funcs) * kept
    # the same geometry from the unfused branch
    ops.jit_config(abi.JIT_OFF, 0)
    try:
        ucols, ucounts, ufused = F.Function.eval_all(ENGINE, [f.p for f in funcs], blk, blocks=True)
    finally:
        ops.jit_config(abi.JIT_AUTO, 1 << 22)
    assert not ufused and list(ucounts) == list(counts)
    for c, u in zip(cols, ucols):
        cg, ug = host_of(c).view(np.uint64), host_of(u).view(np.uint64)
        for b, rows in enumerate(counts):
            assert np.array_equal(cg[b * 10000:b * 10000 + rows], ug[b * 10000:b * 10000 + rows])


def test_block_geometry_needs_the_minimum_block():
    funcs, where = q6()
    blk = device_block("abc", 1000, where)
    with pytest.raises(F.FQError) as e:
        F.Function.eval_all(ENGINE, [f.p for f in funcs], blk, blocks=True)
    assert e.value.status == abi.FQ_E_INVALID and "FQ_PROJECT_MIN_BLOCK_ROWS" in str(e.value)


@pytest.mark.parametrize("block_rows", [0, 10000])
def test_five_columns_fall_back_and_answer(block_rows):
    funcs, where = five()
    want = oracle("abcde", funcs, where, block_rows)
    blk = device_block("abcde", block_rows, where)
    cols, fused = F.Function.eval_all(ENGINE, [f.p for f in funcs], blk)
    assert not fused
    for j, c in enumerate(cols):
        assert same(c, want[0][0][j][0], concat(want, j)), j


def test_a_filter_that_does_not_fit_beside_the_functions_is_not_reported_as_one_kernel():
    # a * b WHERE c + d + e < k: five columns in all -- the filter's Boolean column is evaluated first, node by
    # node, and the fused kernel reads it: the answer is the oracle's, but fused stays 0
    where = binop("<", binop("+", binop("+", field("c"), field("d")), field("e")), const(K38))
    funcs = [binop("*", field("a"), field("b"))]
    for block_rows, blocks in ((0, False), (10000, True)):
        want = oracle("abcde", funcs, where, block_rows)
        res = F.Function.eval_all(ENGINE, [f.p for f in funcs], device_block("abcde", block_rows, where), blocks=blocks)
        assert not res[-1]
        got = host_of(res[0][0]).view(np.uint64)
        if not blocks:
            assert np.array_equal(got, concat(want, 0).astype(np.uint64))
        else:
            assert list(res[1]) == [b[1] for b in want]
            for b, (outs, rows) in enumerate(want):
                assert np.array_equal(got[b * 10000:b * 10000 + rows], outs[0][1].astype(np.uint64))


def test_unfusable_functions_take_the_unfused_branch_and_answer():
    where = binop("<", field("c"), const(K38))
    for funcs in ([binop("*", field("a"), field("b")), const(42)],          # a Constant: to_array of the kept rows
                  [binop("<", field("a"), field("b")), field("a")]):        # a Boolean output
        want = oracle("abc", funcs, where, 0)
        cols, fused = F.Function.eval_all(ENGINE, [f.p for f in funcs], device_block("abc", 0, where))
        assert not fused
        for j, c in enumerate(cols):
            assert c.len == want[0][1] and same(c, want[0][0][j][0], concat(want, j)), j


def test_short_buffers_report_the_bytes_needed():
    funcs, where = q6()
    kept = sum(b[1] for b in oracle("abc", funcs, where, 0))
    blk = device_block("abc", 0, where)
    for mode in (abi.JIT_AUTO, abi.JIT_OFF):  # the fused kernel (through temporaries) and the unfused branch
        ops.jit_config(mode, 1 << 22)
        try:
            with pytest.raises(F.FQError) as e:
                F.Function.eval_all(ENGINE, [f.p for f in funcs], blk, cap=8 * kept - 8)
            assert e.value.status == abi.FQ_E_INVALID and e.value.needed == 8 * kept
            cols, fused = F.Function.eval_all(ENGINE, [f.p for f in funcs], blk, cap=8 * kept)
            assert fused == (mode == abi.JIT_AUTO) and cols[0].len == kept
            assert np.array_equal(host_of(cols[0]), concat(oracle("abc", funcs, where, 0), 0))
        finally:
            ops.jit_config(abi.JIT_AUTO, 1 << 22)
    with pytest.raises(F.FQError) as e:
        F.Function.eval_all(ENGINE, [f.p for f in funcs], device_block("abc", 10000, where), blocks=True, cap=8 * ROWS - 8)
    assert e.value.status == abi.FQ_E_INVALID and e.value.needed == 8 * ROWS


def test_an_error_in_the_second_function_is_returned_with_the_reference_text():
    host = dict(HOST)
    host["b"] = HOST["b"].copy()
    host["b"][12345] = 0
    host["c"] = HOST["c"].copy()
    host["c"][12345] = 0  # kept
    where = binop("<", field("c"), const(K38))
    funcs = [binop("+", field("a"), field("c")), binop("/", field("a"), field("b"))]
    with pytest.raises(R.RefError) as oracle_err:
        oracle("abc", funcs, where, 0, host)
    assert str(oracle_err.value) == "Internal Error: Divide by zero error"
    for mode in (abi.JIT_AUTO, abi.JIT_OFF):
        ops.jit_config(mode, 1 << 22)
        try:
            for blocks in (False, True):
                with pytest.raises(F.FQError) as e:
                    F.Function.eval_all(ENGINE, [f.p for f in funcs], device_block("abc", 10000, where, host), blocks=blocks)
                assert str(e.value) == str(oracle_err.value)
        finally:
            ops.jit_config(abi.JIT_AUTO, 1 << 22)
    # filtered out: it answers
    host["c"][12345] = K38
    want = oracle("abc", funcs, where, 0, host)
    cols, fused = F.Function.eval_all(ENGINE, [f.p for f in funcs], device_block("abc", 0, where, host))
    assert fused and same(cols[1], "UInt64", concat(want, 1))
