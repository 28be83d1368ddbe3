"""fq_aggregate_for32_expr at the C ABI: fq_aggregate over base[i / F] + delta[i]
read as 4-byte deltas.  Every result is compared field by field (sum, max, min,
count, blocks, flags, dtype) with fq_aggregate (JIT ALWAYS) over the plain
column, and with the oracle tests/test_kernels_gpu.py uses for the same shape on
the decoded host values: oracle_c.column_partial replayed through
AggregatorFunction's state machine (tests/replay.py) for expression predicates
and value chains, numpy for predicate trees and bitmap predicates.

Lengths: around the 4-row vector, the 4,096-row tile and the 65,536-row frame,
and more than one workgroup.  Data (tests/for32_expr_shapes.py): an iota from
1,250,000,000; seeded random deltas over a seeded random base per frame, so a
stale or neighbouring base changes the result; a frame with span 2^32 - 1; and
columns just below 2^63 with a single row above it, for the cast flag."""
import ctypes as C
import functools

import numpy as np
import pytest

from fq_amd import abi
from fq_amd._lib import FQError, last_error, lib
from fq_amd.expr import chain, predicate

import oracle_c
from replay import as_tuple, replay

import for32_expr_shapes as S

pytestmark = pytest.mark.gpu

U64 = abi.DT_UINT64
AGGS = [abi.AGG_SUM, abi.AGG_MAX, abi.AGG_MIN, abi.AGG_COUNT]
MASK = {"c4": abi.AGG_MAX | abi.AGG_COUNT, "c4s": abi.AGG_SUM | abi.AGG_COUNT, "max1": abi.AGG_MAX}

ops = None


def setup_module():
    global ops
    from fq_amd import ops as _ops
    _ops.require_gpu()
    _ops.jit_config(abi.JIT_ALWAYS, 0)
    ops = _ops


def teardown_module():
    if ops is not None:
        ops.jit_config(abi.JIT_AUTO, 1 << 22)


def fields(st):
    return (st.sum, st.max, st.min, st.count, st.blocks, st.flags, st.dtype)


def encode(host):
    col = ops.from_numpy(host)
    enc, ok = ops.for32_encode(col)
    assert ok and np.array_equal(enc.decode(), host)
    return col, enc


@functools.lru_cache(maxsize=None)
def encoded(n, data):
    host = S.host_values(n, data)
    return (host,) + encode(host)


def check(host, col, enc, block_rows, pred, value, mask, numpy_ref=None):
    """The delta scan against the plain scan (every field) and against the oracle; returns the state."""
    before = ops.jit_stats()["jit_launches"]
    got = ops.aggregate_for32_expr(enc, block_rows, pred, value, mask)
    assert ops.jit_stats()["jit_launches"] == before + 1  # the hipRTC kernel, whatever min_rows says
    plain = ops.aggregate(col, block_rows, pred, value, mask)
    assert fields(got) == fields(plain), (fields(got), fields(plain))
    if numpy_ref is not None:
        s, mx, mn, c = S.reference(host, *numpy_ref)
        assert got.count == c and got.flags & ~abi.STATE_ANY_EMPTY == 0
        if mask & abi.AGG_SUM:
            assert got.sum == s
        if c and mask & abi.AGG_MAX:
            assert got.max == mx
        if c and mask & abi.AGG_MIN:
            assert got.min == mn
        return got
    want = [op for op in AGGS if mask & op]
    try:
        exp = [as_tuple(s) for s in oracle_c.column_partial(host, U64, block_rows or max(len(host), 1),
                                                            [(op, value) for op in want], pred)]
    except oracle_c.OracleError as e:
        with pytest.raises(oracle_c.OracleError) as ei:
            for op in want:
                replay(op, got)
        assert str(ei.value) == str(e)
        return got
    assert [replay(op, got) for op in want] == exp, (ops.state_values(got), exp)
    return got


@pytest.mark.parametrize("name", ["c4", "c4s", "max1", "push", "libdivide"])
@pytest.mark.parametrize("data", S.DATA)
@pytest.mark.parametrize("n", S.LENGTHS)
def test_flat_scan_equals_plain_scan_and_oracle(n, data, name):
    host, col, enc = encoded(n, data)
    pred, value, _, _ = S.shape(name)
    st = check(host, col, enc, 0, pred, value, MASK.get(name, S.ALL))
    # (one block that keeps no row is the empty state: FQ_STATE_ANY_EMPTY, as in fq_aggregate)
    assert st.flags == (abi.STATE_ANY_EMPTY if pred is not None and st.count == 0 else 0)
    assert st.dtype == U64 and st.blocks == 1


@pytest.mark.parametrize("data", S.DATA)
@pytest.mark.parametrize("n", S.LENGTHS)
def test_predicate_tree_equals_plain_scan_and_numpy(n, data):
    host, col, enc = encoded(n, data)
    pred, value, keep, val = S.shape("tree")
    check(host, col, enc, 0, pred, value, S.ALL, numpy_ref=(keep, val))


@pytest.mark.parametrize("n", S.LENGTHS)
def test_bitmap_predicate_sees_the_true_row_index(n):
    """The kept rows depend on the row's position only (a hash of the index), the values on the frame."""
    host, col, enc = encoded(n, "random")
    key = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(2**32)
    bm = ops.compare("<", ops.from_numpy(key), 2**31)
    pred = abi.fq_pred()
    pred.kind = abi.PRED_BITMAP
    pred.bitmap = bm.ptr
    value, _ = chain(U64, [("+", 1)])
    kept = key < np.uint64(2**31)
    ref = (lambda x: kept, lambda x: x + np.uint64(1))
    check(host, col, enc, 0, pred, value, S.ALL, numpy_ref=ref)
    if n > 20000:  # block mode: the bitmap under one ballot per block
        check(host, col, enc, 10000, pred, value, S.ALL, numpy_ref=ref)


@pytest.mark.parametrize("n", S.LENGTHS)
def test_float64_value_with_an_exact_sum_is_bit_for_bit(n):
    """(x % 1000003) * 1.0: integers below 2^31 as Float64, so every partial sum is below 2^53 and exact in any
    order -- the delta scan gives a lane other rows than the plain scan."""
    host, col, enc = encoded(n, "iota")
    value, dt = chain(U64, [("%", 1000003), ("*", 1.0)])
    assert dt == abi.DT_FLOAT64
    st = check(host, col, enc, 0, predicate(U64, [("%", 8)], "<", 3), value, S.ALL)
    assert st.dtype == abi.DT_FLOAT64 and st.flags == (0 if st.count else abi.STATE_ANY_EMPTY)
    check(host, col, enc, 0, None, value, S.ALL)


def test_zero_divisor_only_counts_on_kept_rows():
    n = 2 * 65536 + 4099  # the last row is one of 3 after the last whole vector
    host, col, enc = encoded(n, "iota")
    div0, _ = chain(U64, [("/", 0)])
    none = check(host, col, enc, 0, predicate(U64, [], "<", 0), div0, S.ALL)  # keeps no row: no error flag
    assert none.flags == abi.STATE_ANY_EMPTY and none.count == 0  # (the one block is empty, nothing else)
    last = check(host, col, enc, 0, predicate(U64, [], "=", int(host[-1])), div0, S.ALL)
    assert last.flags & abi.STATE_DIV_ZERO and last.count == 1
    first_of_tail = check(host, col, enc, 0, predicate(U64, [], "=", int(host[n - 3])), div0, S.ALL)
    assert first_of_tail.flags & abi.STATE_DIV_ZERO


N_CAST = 2 * 65536 + 4096 + 2048 + 3  # two frames, a whole tile, half a tile of remainder vectors, 3 tail rows
CAST_ROWS = {"first": 0, "in_tile": 70_005, "in_remainder": 2 * 65536 + 4096 + 1001, "last": N_CAST - 1}


@pytest.mark.parametrize("where", list(CAST_ROWS))
def test_cast_null_of_a_single_row_above_2_63(where):
    """UInt64 - Int64 casts the column to Int64: null for the one row >= 2^63, wherever the loop meets it."""
    row = CAST_ROWS[where]
    host = np.uint64(2**63 - 1) - (np.arange(N_CAST, dtype=np.uint64) % np.uint64(1000))
    value, dt = chain(U64, [("-", (5, "Int64"))])
    assert dt == abi.DT_INT64
    col, enc = encode(host)
    clean = check(host, col, enc, 0, None, value, S.ALL)
    assert clean.flags == 0 and clean.dtype == abi.DT_INT64
    host = host.copy()
    host[row] = np.uint64(2**63 + 7)
    col, enc = encode(host)
    st = check(host, col, enc, 0, None, value, S.ALL)
    assert st.flags == abi.STATE_CAST_NULL
    # ... and dropped by the predicate it raises nothing
    dropped = check(host, col, enc, 0, predicate(U64, [], "<", 2**63), value, S.ALL)
    assert dropped.flags == 0 and dropped.count == N_CAST - 1


def test_iota_ending_above_2_63_raises_the_cast_flag():
    host, col, enc = encoded(100_003, "iota_hi")
    value, _ = chain(U64, [("-", (5, "Int64"))])
    assert check(host, col, enc, 0, None, value, S.ALL).flags == abi.STATE_CAST_NULL


# block mode: sum under a predicate over more than one reference block
BLOCKS = [(10000, 70_001),     # block 6 (rows 60,000 .. 69,999) crosses the frame edge
          (10002, 70_001),     # % 4 != 0: the element path
          (65536, 200_003),    # blocks equal frames
          (100000, 200_003)]   # two frame edges inside one block, and a ragged last block


@pytest.mark.parametrize("data", ["random", "iota"])
@pytest.mark.parametrize("block_rows,n", BLOCKS)
def test_block_mode_equals_plain_scan_and_oracle(block_rows, n, data):
    host, col, enc = encoded(n, data)
    pred, value, keep, _ = S.shape("c4s")
    kept = keep(host)
    empty = any(not kept[s:s + block_rows].any() for s in range(0, n, block_rows))  # (a ragged last block of one row)
    for mask in (abi.AGG_SUM | abi.AGG_COUNT, S.ALL):
        st = check(host, col, enc, block_rows, pred, value, mask)
        assert st.blocks == -(-n // block_rows) and st.count == int(kept.sum())
        assert st.flags == (abi.STATE_ANY_EMPTY if empty else 0)
    tree, value, keep, val = S.shape("tree")
    check(host, col, enc, block_rows, tree, value, S.ALL, numpy_ref=(keep, val))


@pytest.mark.parametrize("block_rows,n", [(10000, 70_001), (10002, 70_015)])
def test_a_predicate_that_empties_exactly_one_block(block_rows, n):
    """An iota from 125,000 blocks in: (x / B + k) % 8 > 0 drops exactly the rows of block 3."""
    host = np.arange(n, dtype=np.uint64) + np.uint64(125_000 * block_rows)
    col, enc = encode(host)
    first = int(host[0]) // block_rows
    k = (8 - (first + 3) % 8) % 8
    pred = predicate(U64, [("/", block_rows), ("+", k), ("%", 8)], ">", 0)
    kept = (host // np.uint64(block_rows) + np.uint64(k)) % np.uint64(8) > 0
    per_block = [int(kept[s:s + block_rows].sum()) for s in range(0, n, block_rows)]
    assert [i for i, c in enumerate(per_block) if c == 0] == [3]
    value, _ = chain(U64, [("+", 1)])
    st = check(host, col, enc, block_rows, pred, value, abi.AGG_SUM | abi.AGG_COUNT)
    assert st.blocks == len(per_block) == 8 and st.count == sum(per_block)
    assert st.flags == abi.STATE_ANY_EMPTY
    c4s, _, keep, _ = S.shape("c4s")  # every whole block keeps rows; the ragged last one may not
    k4 = keep(host)
    every = check(host, col, enc, block_rows, c4s, value, abi.AGG_SUM | abi.AGG_COUNT)
    assert every.flags == (0 if all(k4[s:s + block_rows].any() for s in range(0, n, block_rows)) else abi.STATE_ANY_EMPTY)


def test_without_predicate_and_expression_it_is_fq_aggregate_for32():
    host, col, enc = encoded(1_000_003, "random")
    before = ops.jit_stats()["jit_launches"]
    for mask in (abi.AGG_SUM, abi.AGG_COUNT, S.ALL):
        got = ops.aggregate_for32_expr(enc, 0, None, None, mask)
        assert fields(got) == fields(ops.aggregate_for32(enc, mask)) == fields(ops.aggregate(col, 0, None, None, mask))
        blocks = ops.aggregate_for32_expr(enc, 10000, None, None, mask)
        assert fields(blocks) == fields(ops.aggregate(col, 10000, None, None, mask)) and blocks.blocks == 101
    assert ops.jit_stats()["jit_launches"] == before  # precompiled kernels only


def raw(delta, base, n, mask, pred, value, out, ws, ws_bytes=None):
    return lib.fq_aggregate_for32_expr(C.c_void_p(delta), C.c_void_p(base), n, 0,
                                       C.byref(pred) if pred is not None else None,
                                       C.byref(value) if value is not None else None, mask,
                                       C.c_void_p(out), ws.ptr, ws.nbytes if ws_bytes is None else ws_bytes, None)


def test_count_alone_without_predicate_and_expression_reads_nothing():
    import torch
    ws = ops.Workspace(lib.fq_aggregate_workspace_bytes(1000))
    out = torch.zeros(48, dtype=torch.uint8, device="cuda")
    assert raw(None, None, 12345, abi.AGG_COUNT, None, None, out.data_ptr(), ws) == abi.FQ_OK
    st = ops.state_from_device(out)
    assert st.count == 12345 and st.blocks == 1 and st.flags == 0


def test_argument_errors_and_jit_off():
    import torch
    host, col, enc = encoded(65537, "random")
    pred, value, _, _ = S.shape("c4")
    ws = ops.Workspace(lib.fq_aggregate_workspace_bytes(enc.len))
    out = torch.zeros(48, dtype=torch.uint8, device="cuda")
    d, b, o = enc.delta.ptr, enc.base.ptr, out.data_ptr()
    assert raw(d, b, enc.len, S.ALL, pred, value, o, ws) == abi.FQ_OK
    for args, text in (((d + 4, b, enc.len, S.ALL), "delta not aligned to 16 bytes"),
                       ((d + 8, b, enc.len, S.ALL), "delta not aligned to 16 bytes"),
                       ((d, b + 4, enc.len, S.ALL), "base not aligned to 8 bytes"),
                       ((d, b, enc.len, 16), "unknown bits in agg_mask"),
                       ((d, b, -1, S.ALL), "negative length"),
                       ((None, b, enc.len, S.ALL), "NULL argument"),
                       ((d, None, enc.len, S.ALL), "NULL argument")):
        assert raw(*args, pred, value, o, ws) == abi.FQ_E_INVALID, text
        assert text in last_error()
    assert raw(d, b, enc.len, S.ALL, pred, value, None, ws) == abi.FQ_E_INVALID and "NULL argument" in last_error()
    assert raw(d, b, enc.len, S.ALL, pred, value, o, ws, ws_bytes=4096 * 48 - 1) == abi.FQ_E_INVALID
    assert "workspace too small" in last_error()
    ops.jit_config(abi.JIT_OFF)
    try:
        with pytest.raises(FQError) as ei:
            ops.aggregate_for32_expr(enc, 0, pred, value, S.ALL)
        assert ei.value.status == abi.FQ_E_UNSUPPORTED and "hipRTC kernel only" in str(ei.value)
        # the call without predicate and expression needs no JIT
        assert fields(ops.aggregate_for32_expr(enc, 0, None, None, S.ALL)) == fields(ops.aggregate_for32(enc, S.ALL))
    finally:
        ops.jit_config(abi.JIT_ALWAYS, 0)
