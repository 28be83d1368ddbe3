"""GPU: ProjectionTransform's loop for one block through the Function handles
(fq_functions_eval) over an fq_block whose fields are Float64, Float32, Int32,
UInt8 and UInt16 with a pending filter: the boundary a fuse-query host that
keeps its own tables uses.  `[price * discount, quantity] WHERE shipdate < k
and quantity < q` and `[a + b, a] WHERE a < 100` must run as ONE fused kernel
(fused == 1) that writes every output at its own width, equal oracle/fq_ref.py
per reference block (R.Block -> R.filter_block -> Fn.eval), equal the same
handles on the unfused branch (JIT off) bit for bit, and equal n separate
Function.eval calls -- contiguous and in block geometry.  A fifth column, a
Boolean output, a Constant and a chain whose casts do not fit take the unfused
branch; an all-UInt64 block is served as before."""
import numpy as np
import pytest

import fq_ref as R
from fq_amd import abi

pytestmark = pytest.mark.gpu

ROWS = 20_009
ops = F = ENGINE = None
HOST = {}
TYPES = {"price": "Float64", "discount": "Float32", "shipdate": "Int32", "quantity": "UInt8", "a": "UInt8",
         "b": "UInt16", "n1": "UInt8", "n2": "UInt8", "n3": "UInt16", "n4": "UInt8", "n5": "UInt16", "w": "UInt32",
         "f": "Float32", "u": "UInt64", "v": "UInt64"}
NP = {"Float64": np.float64, "Float32": np.float32, "Int32": np.int32, "UInt8": np.uint8, "UInt16": np.uint16,
      "UInt32": np.uint32, "UInt64": np.uint64, "Int64": np.int64}
WIDTH = {t: np.dtype(d).itemsize for t, d in NP.items()}
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def setup_module():
    global ops, F, ENGINE
    from fq_amd import functions as _F
    from fq_amd import ops as _ops
    _ops.require_gpu()
    ops, F = _ops, _F
    ENGINE = _F.Engine(device=0)
    rng = np.random.default_rng(2025)
    HOST["price"] = rng.uniform(1.0, 1000.0, ROWS)
    HOST["discount"] = (rng.integers(0, 11, ROWS) / 100.0).astype(np.float32)
    HOST["shipdate"] = rng.integers(8000, 10600, ROWS).astype(np.int32)
    HOST["quantity"] = rng.integers(1, 51, ROWS).astype(np.uint8)
    HOST["a"] = rng.integers(0, 256, ROWS).astype(np.uint8)
    HOST["b"] = rng.integers(0, 65536, ROWS).astype(np.uint16)
    for n in ("n1", "n2", "n4"):
        HOST[n] = rng.integers(0, 128, ROWS).astype(np.uint8)
    for n in ("n3", "n5"):
        HOST[n] = rng.integers(0, 65536, ROWS).astype(np.uint16)
    HOST["w"] = rng.integers(0, 1 << 20, ROWS).astype(np.uint32)
    HOST["f"] = rng.integers(-1000, 1000, ROWS).astype(np.float32)
    HOST["u"] = rng.integers(0, 1 << 62, ROWS).astype(np.uint64)
    HOST["v"] = rng.integers(0, 1 << 62, ROWS).astype(np.uint64)


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


def q6():
    """price * discount (Float64), quantity (UInt8) WHERE shipdate < k and quantity < q: 17 B read, 9 B per kept row"""
    where = binop("and", binop("<", field("shipdate"), const(9950, "Int32")),
                  binop("<", field("quantity"), const(26, "UInt8")))
    return ["price", "discount", "shipdate", "quantity"], [binop("*", field("price"), field("discount")), field("quantity")], \
        where, ["Float64", "UInt8"]


def u8u16():
    """a + b (UInt16), a (UInt8) WHERE a < 100"""
    return ["a", "b"], [binop("+", field("a"), field("b")), field("a")], binop("<", field("a"), const(100, "UInt8")), \
        ["UInt16", "UInt8"]


def device_block(names, block_rows, where):
    cols = [ops.from_numpy(HOST[n], abi.DT_BY_NAME[TYPES[n]]) for n in names]
    return F.DataBlock(list(names), cols, block_rows=block_rows, filter=where.p if where is not None else None)


def oracle(names, funcs, where, block_rows):
    """per reference block: ([(type, values) per function], rows kept)"""
    br = block_rows or ROWS
    blocks = []
    for s in range(0, ROWS, br):
        blk = R.Block([(n, R.Arr(TYPES[n], HOST[n][s:s + br])) for n in names])
        fb = R.filter_block(where.o, blk) if where is not None else blk
        outs = []
        for f in funcs:
            v = f.o.eval(fb)
            if not isinstance(v, R.Arr):
                v = R.to_array(v, fb.num_rows())
            assert v.valid is None or np.all(v.valid)
            outs.append((v.type, np.asarray(v.values)))
        blocks.append((outs, fb.num_rows()))
    return blocks


def concat(blocks, j):
    return np.concatenate([b[0][j][1] for b in blocks])


def raw(values, typ):
    """the values as unsigned words of the type's width"""
    return np.ascontiguousarray(np.asarray(values).astype(NP[typ], copy=False)).view(UINT[WIDTH[typ]])


def same(col, typ, values):
    got = col.to_numpy()
    if typ == "Boolean":
        return col.dtype == abi.DT_BOOLEAN and np.array_equal(got, np.asarray(values).astype(bool))
    return col.dtype == abi.DT_BY_NAME[typ] and np.array_equal(raw(got, typ), raw(values, typ))


@pytest.mark.parametrize("block_rows", [0, 10000])
@pytest.mark.parametrize("plan", [q6, u8u16], ids=["q6", "u8u16"])
def test_one_fused_kernel_equals_the_oracle_the_unfused_branch_and_separate_evals(plan, block_rows):
    names, funcs, where, types = plan()
    want = oracle(names, funcs, where, block_rows)
    kept = sum(b[1] for b in want)
    blk = device_block(names, block_rows, where)
    cols, fused = F.Function.eval_all(ENGINE, [f.p for f in funcs], blk)
    assert fused
    for j, c in enumerate(cols):
        assert want[0][0][j][0] == types[j]
        assert c.len == kept and c.dtype == abi.DT_BY_NAME[types[j]]  # the narrow dtype, its own length
        assert same(c, types[j], concat(want, j)), j
    # the same handles on the unfused branch
    ops.jit_config(abi.JIT_OFF, 0)
    try:
        ucols, ufused = F.Function.eval_all(ENGINE, [f.p for f in funcs], blk)
    finally:
        ops.jit_config(abi.JIT_AUTO, 1 << 22)
    assert not ufused
    for c, u, t in zip(cols, ucols, types):
        assert c.dtype == u.dtype and c.len == u.len
        assert np.array_equal(raw(c.to_numpy(), t), raw(u.to_numpy(), t))
    # n separate Function.eval calls
    for c, f, t in zip(cols, funcs, types):
        one = f.p.eval(ENGINE, blk)
        assert one.dtype == c.dtype and one.len == c.len
        assert np.array_equal(raw(c.to_numpy(), t), raw(one.to_numpy(), t))


@pytest.mark.parametrize("plan", [q6, u8u16], ids=["q6", "u8u16"])
def test_block_geometry_counts_rows_and_stats(plan):
    names, funcs, where, types = plan()
    want = oracle(names, funcs, where, 10000)
    blk = device_block(names, 10000, where)
    s0 = ENGINE.stats()
    cols, counts, fused = F.Function.eval_all(ENGINE, [f.p for f in funcs], blk, blocks=True)
    s1 = ENGINE.stats()
    assert fused
    assert list(counts) == [b[1] for b in want]
    for j, c in enumerate(cols):
        assert c.len == ROWS and c.dtype == abi.DT_BY_NAME[types[j]]
        got = raw(c.to_numpy(), types[j])
        for b, (outs, rows) in enumerate(want):
            assert np.array_equal(got[b * 10000:b * 10000 + rows], raw(outs[j][1], types[j])), (j, b)
    kept = int(counts.sum())
    assert s1["project_launches"] - s0["project_launches"] == 1
    # every column read once at its own width, every kept row's outputs written at theirs
    read = sum(WIDTH[TYPES[n]] for n in names)
    written = sum(WIDTH[t] for t in types)
    assert s1["project_bytes"] - s0["project_bytes"] == read * ROWS + written * kept
    # the same geometry from the unfused branch
    ops.jit_config(abi.JIT_OFF, 0)
    try:
        ucols, ucounts, ufused = F.Function.eval_all(ENGINE, [f.p for f in funcs], blk, blocks=True)
    finally:
        ops.jit_config(abi.JIT_AUTO, 1 << 22)
    assert not ufused and list(ucounts) == list(counts)
    for c, u, t in zip(cols, ucols, types):
        assert c.dtype == u.dtype
        cg, ug = raw(c.to_numpy(), t), raw(u.to_numpy(), t)
        for b, rows in enumerate(counts):
            assert np.array_equal(cg[b * 10000:b * 10000 + rows], ug[b * 10000:b * 10000 + rows])


def test_short_buffers_report_the_bytes_needed():
    """Every output buffer has `cap` bytes and holds its output at its own width, so a buffer needs the widest
    output's kept rows: 8 bytes per kept row for [Float64, UInt8], 2 for [UInt16, UInt8]."""
    for plan in (q6, u8u16):
        names, funcs, where, types = plan()
        kept = sum(b[1] for b in oracle(names, funcs, where, 0))
        need = max(WIDTH[t] for t in types) * kept
        blk = device_block(names, 0, where)
        for mode in (abi.JIT_AUTO, abi.JIT_OFF):  # the fused kernel (through temporaries) and the unfused branch
            ops.jit_config(mode, 1 << 22)
            try:
                with pytest.raises(F.FQError) as e:
                    F.Function.eval_all(ENGINE, [f.p for f in funcs], blk, cap=need - 1)
                assert e.value.status == abi.FQ_E_INVALID and e.value.needed == need
                cols, fused = F.Function.eval_all(ENGINE, [f.p for f in funcs], blk, cap=need)
                assert fused == (mode == abi.JIT_AUTO) and cols[0].len == kept
                for j, c in enumerate(cols):
                    assert same(c, types[j], concat(oracle(names, funcs, where, 0), j))
            finally:
                ops.jit_config(abi.JIT_AUTO, 1 << 22)


def five():
    e = binop("+", binop("+", binop("+", binop("+", field("n1"), field("n2")), field("n3")), field("n4")), field("n5"))
    return ["n1", "n2", "n3", "n4", "n5"], [e, binop("*", field("n1"), field("n2"))], \
        binop("<", field("n4"), const(48, "UInt8"))


def long_chain():
    """n1 + n3 + w + 1:UInt64 + (-1):Int64 + f + 1.5:Float64 + 1.0:Float64 over UInt8, UInt16, UInt32, Float32:
    seven steps whose type changes six times -- one lowered step more than the program holds"""
    e = binop("+", binop("+", field("n1"), field("n3")), field("w"))
    e = binop("+", binop("+", e, const(1, "UInt64")), const(-1, "Int64"))
    e = binop("+", binop("+", binop("+", e, field("f")), const(1.5, "Float64")), const(1.0, "Float64"))
    return ["n1", "n3", "w", "f"], [e], binop("<", field("n1"), const(100, "UInt8"))


def boolean_output():
    return ["a", "b"], [binop("<", field("a"), field("b")), field("a")], binop("<", field("a"), const(100, "UInt8"))


def constant_output():
    return ["a", "b"], [binop("+", field("a"), field("b")), const(42, "UInt8")], binop("<", field("a"), const(100, "UInt8"))


@pytest.mark.parametrize("plan", [five, long_chain, boolean_output, constant_output],
                         ids=["a fifth column", "casts that do not fit", "a Boolean output", "a Constant"])
def test_unfusable_shapes_take_the_unfused_branch_and_answer(plan):
    names, funcs, where = plan()
    want = oracle(names, funcs, where, 0)
    cols, fused = F.Function.eval_all(ENGINE, [f.p for f in funcs], device_block(names, 0, where))
    assert not fused
    for j, c in enumerate(cols):
        assert c.len == want[0][1] and same(c, want[0][0][j][0], concat(want, j)), j


def test_an_all_uint64_block_is_served_as_before():
    """the 64-bit entry points, the same launches and statistics"""
    names = ["u", "v"]
    funcs = [binop("*", field("u"), field("v")), field("v")]
    where = binop("<", field("u"), const(3 << 59, "UInt64"))
    want = oracle(names, funcs, where, 10000)
    kept = sum(b[1] for b in want)
    blk = device_block(names, 10000, where)
    F.Function.eval_all(ENGINE, [f.p for f in funcs], blk)  # compiled
    F.Function.eval_all(ENGINE, [f.p for f in funcs], blk, blocks=True)
    j0, s0 = ops.jit_stats(), ENGINE.stats()
    cols, fused = F.Function.eval_all(ENGINE, [f.p for f in funcs], blk)
    j1 = ops.jit_stats()
    assert fused and j1["jit_launches"] - j0["jit_launches"] == 1 and j1["kernels_compiled"] == j0["kernels_compiled"]
    for j, c in enumerate(cols):
        assert c.len == kept and same(c, "UInt64", concat(want, j))
    bcols, counts, fused = F.Function.eval_all(ENGINE, [f.p for f in funcs], blk, blocks=True)
    j2, s1 = ops.jit_stats(), ENGINE.stats()
    assert fused and j2["jit_launches"] - j1["jit_launches"] == 1 and j2["kernels_compiled"] == j0["kernels_compiled"]
    assert list(counts) == [b[1] for b in want]
    assert s1["project_launches"] - s0["project_launches"] == 1
    assert s1["project_bytes"] - s0["project_bytes"] == 8 * 2 * ROWS + 8 * 2 * kept
