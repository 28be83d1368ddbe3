"""fq_filter_project_blocks_for32 on the GPU: the Filter -> Projection block
stream over a window [first, first + len) of a UInt64 column stored as per-frame
32-bit deltas equals fq_filter_project_blocks over the decoded window -- counts,
out_len and the whole output buffers byte for byte, rows past a block's count
and guard rows around the outputs left as they were -- and equals numpy and
oracle/fq_ref.py over the decoded rows.  Windows start and end anywhere in a
frame (tests/for32_project_cases.py: every length x block size x first, on a
column that ends inside its last frame and on one that ends at a frame edge),
the frames' bases are 64-bit random, so a stale or wrong base changes every row
it touches.  Every test runs under test_project_blocks_gpu.py's `stage` fixture
(kept rows stored from registers, staged, staged through a quarter tile)."""
import ctypes as C

import numpy as np
import pytest
import torch

from fq_amd import abi
from fq_amd._lib import lib, last_error

import for32_project_cases as S
import launch_shapes
import test_project_blocks_gpu as PB
from test_project_blocks_gpu import stage  # noqa: F401  (autouse: every test at SELECT_BLOCKS_STAGE 0, 1, 4)

pytestmark = pytest.mark.gpu

U64 = abi.DT_UINT64
SENT = 0xA5A5A5A5_5A5A5A5A  # fills the output buffers before a call
GUARD = 16                  # sentinel rows before and after every output
ops = None
_cols = {}


def setup_module():
    global ops
    PB.setup_module()  # the stage fixture reads that module's ops
    ops = PB.ops


def encoded(kind, enc_len):
    """(host rows, For32Column on the device), encoded by fq_for32_encode, cached for the module."""
    key = (kind, enc_len)
    if key not in _cols:
        host = S.host_column(S.ENC_LEN, kind)[:enc_len]
        enc, ok = ops.for32_encode(ops.from_numpy(host))
        assert ok and enc.base.len == -(-enc_len // S.F)
        delta, base = S.encode_host(host)
        assert np.array_equal(enc.delta.to_numpy(), delta) and np.array_equal(enc.base.to_numpy(), base)
        _cols[key] = (host, enc)
    return _cols[key]


class Run:
    """One call into sentinel-filled buffers: .rc, .kept, .counts (numpy), .bufs (uint64 tensors, guards included)"""


def run(fn, lead, n, block_rows, pred, values, out_offset=0):
    """fn(*lead, block_rows, pred, exprs, n_out, ptrs, counts, &kept, ws, ws_bytes, stream) with every output of n
    rows inside a buffer of GUARD + out_offset rows before and GUARD after, all filled with SENT."""
    n_out = len(values)
    exprs = ops._project_exprs(values, U64)
    r = Run()
    r.bufs = [torch.full((n + 2 * GUARD + out_offset,), SENT - 2**64, dtype=torch.int64, device="cuda")
              for _ in range(n_out)]
    ptrs = (C.c_void_p * n_out)(*[b.data_ptr() + 8 * (GUARD + out_offset) for b in r.bufs])
    nb = (1 if block_rows >= n else -(-n // block_rows)) if n > 0 else 0
    counts = torch.full((nb + 2,), -7, dtype=torch.int64, device="cuda")
    ws = ops.Workspace(lib.fq_filter_project_blocks_workspace_bytes())
    kept = C.c_int64(-1)
    r.rc = fn(*lead, block_rows, C.byref(pred) if pred is not None else None, exprs, n_out, ptrs,
              C.c_void_p(counts.data_ptr() + 8), C.byref(kept), ws.ptr, ws.nbytes, ops._stream())
    r.error = last_error() if r.rc else ""
    r.kept = kept.value
    c = counts.cpu().numpy()
    assert c[0] == -7 and c[-1] == -7  # nothing written around the counts
    r.counts = c[1:-1]
    return r


def run_for32(enc, first, n, block_rows, pred, values, out_offset=0):
    return run(lib.fq_filter_project_blocks_for32, (C.c_void_p(enc.delta.ptr), C.c_void_p(enc.base.ptr), first, n), n,
               block_rows, pred, values, out_offset)


def run_plain(col, block_rows, pred, values, out_offset=0):
    c = col.col()
    return run(lib.fq_filter_project_blocks, (C.byref(c),), col.len, block_rows, pred, values, out_offset)


def same(a, b):
    assert (a.rc, a.error, a.kept) == (b.rc, b.error, b.kept)
    assert np.array_equal(a.counts, b.counts)
    for x, y in zip(a.bufs, b.bufs):
        assert torch.equal(x, y)  # kept ranges, untouched rows and guards alike


def check_numpy(r, host, keep, fns, block_rows, out_offset=0):
    """counts and every block's kept rows against numpy; rows past a count and the guards hold the sentinel"""
    n = len(host)
    B = max(min(block_rows, n), 1)
    want = [int(keep[b0:b0 + B].sum()) for b0 in range(0, n, B)]
    assert r.rc == 0 and r.counts.tolist() == want and r.kept == sum(want)
    exp = S.expect_blocks(host, keep, fns, B)
    for buf, per in zip(r.bufs, exp):
        h = buf.cpu().numpy().view(np.uint64)
        lo = GUARD + out_offset
        assert (h[:lo] == SENT).all() and (h[lo + n:] == SENT).all()
        for b, e in enumerate(per):
            got = h[lo + b * B: lo + min((b + 1) * B, n)]
            assert np.array_equal(got[:len(e)], np.asarray(e).view(np.uint64)), b
            assert (got[len(e):] == SENT).all(), b


@pytest.mark.parametrize("first", S.FIRSTS)
@pytest.mark.parametrize("block_rows", S.BLOCK_ROWS)
def test_every_window_equals_the_plain_call_and_numpy(first, block_rows):
    pred, values, keep, fns = S.shape("p1")
    for kind in ("random", "iota"):
        for enc_len, f, n in S.windows():
            if f != first:
                continue
            host, enc = encoded(kind, enc_len)
            win = host[first:first + n]
            a = run_for32(enc, first, n, block_rows, pred, values)
            check_numpy(a, win, keep(win), fns, block_rows)
            same(a, run_plain(ops.from_numpy(win), block_rows, pred, values))


@pytest.mark.parametrize("sel", ["none", "all", "p1", "runs"])
def test_selectivities(sel):
    pred, values, keep, fns = S.shape(sel)
    for kind, first, n, block_rows in (("random", 4097, 200_003, 10_000), ("iota", 65_535, 65_537, 10_001)):
        host, enc = encoded(kind, S.ENC_LEN)
        win = host[first:first + n]
        a = run_for32(enc, first, n, block_rows, pred, values)
        check_numpy(a, win, keep(win), fns, block_rows)
        same(a, run_plain(ops.from_numpy(win), block_rows, pred, values))


@pytest.mark.parametrize("name", ["tree", "eight"])
def test_tree_predicate_float_output_and_eight_outputs(name):
    pred, values, keep, fns = S.shape(name)
    host, enc = encoded("iota", S.ENC_LEN)  # (random 64-bit rows are no exact Float64)
    first, n = 65_535, 200_003
    win = host[first:first + n]
    a = run_for32(enc, first, n, 10_000, pred, values)
    check_numpy(a, win, keep(win), fns, 10_000)
    same(a, run_plain(ops.from_numpy(win), 10_000, pred, values))
    if name == "tree":
        assert values[0].out_dtype == abi.DT_FLOAT64 and values[1].out_dtype == abi.DT_INT64


def test_bitmap_predicate_rows_are_relative_to_the_window():
    _, values, keep, fns = S.shape("p1")
    host, enc = encoded("random", S.ENC_LEN)
    first, n = 131_071, 200_003
    win = host[first:first + n]
    col = ops.from_numpy(win)
    bm = ops.predicate_bitmap(col, S.shape("p1")[0])
    p = abi.fq_pred()
    p.kind = abi.PRED_BITMAP
    p.bitmap = bm.ptr
    for block_rows in (8192, 10_001):
        a = run_for32(enc, first, n, block_rows, p, values)
        check_numpy(a, win, keep(win), fns, block_rows)
        same(a, run_plain(col, block_rows, p, values))


@pytest.mark.parametrize("block_rows", [8192, 10_001])
def test_outputs_offset_by_one_element(block_rows):
    pred, values, keep, fns = S.shape("p1")
    host, enc = encoded("random", S.ENC_LEN)
    first, n = 1, 65_537
    win = host[first:first + n]
    a = run_for32(enc, first, n, block_rows, pred, values, out_offset=1)
    check_numpy(a, win, keep(win), fns, block_rows, out_offset=1)
    same(a, run_plain(ops.from_numpy(win), block_rows, pred, values, out_offset=1))
    # the public wrapper: what filter_project_blocks returns
    outs, cnt = ops.filter_project_blocks_for32(enc, block_rows, pred, values, first=first, length=n, out_offset=1)
    ref, rcnt = ops.filter_project_blocks(ops.from_numpy(win), block_rows, pred, values, out_offset=1)
    assert np.array_equal(cnt, rcnt) and np.array_equal(cnt, a.counts)
    for g, e in zip(PB._blocks_of(outs, cnt, block_rows), PB._blocks_of(ref, rcnt, block_rows)):
        assert all(np.array_equal(x, y) for x, y in zip(g, e))
    outs, cnt = ops.filter_project_blocks_for32(enc, block_rows, pred, values, first=S.ENC_LEN - 9000)  # to the end
    assert outs[0].len == 9000 and int(cnt.sum()) == int(keep(host[-9000:]).sum())


def test_the_reference_blocks_over_a_window():
    """oracle/fq_ref.py's filter_block + Arith eval on each 10,000-row block of the decoded window."""
    import fq_ref as R
    num, c = R.E_field("number"), R.E_const
    pred_fn = R.to_function(R.E_bin("<", R.E_bin("%", num, c(8)), c(3)))
    funcs = [R.to_function(R.E_bin("+", num, c(1))), R.to_function(R.E_bin("/", num, c(2)))]
    pred, values, _, _ = S.shape("p1")
    host, enc = encoded("random", S.ENC_LEN)
    first, n = 65_535, 65_537
    a = run_for32(enc, first, n, 10_000, pred, values)
    assert a.rc == 0
    bufs = [b.cpu().numpy().view(np.uint64)[GUARD:] for b in a.bufs]
    for b, b0 in enumerate(range(0, n, 10_000)):
        blk = R.Block({"number": R.Arr("UInt64", host[first + b0:first + min(b0 + 10_000, n)])})
        kept = R.filter_block(pred_fn, blk)
        assert a.counts[b] == kept.num_rows()
        for j, f in enumerate(funcs):
            v = f.eval(kept)
            assert v.type == "UInt64"
            assert bufs[j][b0:b0 + kept.num_rows()].tolist() == [int(x) for x in v.values]


def test_errors_have_the_plain_calls_status_and_text():
    from fq_amd.expr import chain, predicate
    host, enc = encoded("iota", S.ENC_LEN)
    first, n = 4097, 65_537
    col = ops.from_numpy(host[first:first + n])
    val = chain(U64, [("%", 8), ("/", 100, True)])[0]  # 100 / (number % 8)
    keep_zero = predicate(U64, [("%", 8)], "<", 3)    # keeps rows with number % 8 == 0
    drop_zero = predicate(U64, [("%", 8)], ">=", 1)
    in_pred = predicate(U64, [("%", 8), ("/", 100, True)], ">", 0)  # the predicate itself divides by zero
    for pred, values in ((keep_zero, [val]), (in_pred, [None])):
        a = run_for32(enc, first, n, 10_000, pred, values)
        b = run_plain(col, 10_000, pred, values)
        assert a.rc == b.rc == abi.FQ_E_DIVIDE_BY_ZERO and a.kept == b.kept == 0
        assert a.error == b.error == "Internal Error: Divide by zero error"
    a = run_for32(enc, first, n, 10_000, drop_zero, [val])  # the row that would divide by zero is dropped
    win = host[first:first + n]
    check_numpy(a, win, win % np.uint64(8) >= np.uint64(1), [lambda k: np.uint64(100) // (k % np.uint64(8))], 10_000)
    same(a, run_plain(col, 10_000, drop_zero, [val]))


def test_refusals_and_empty_windows():
    pred, values, _, _ = S.shape("p1")
    _, enc = encoded("iota", S.ENC_LEN)
    none = abi.fq_pred()
    none.kind = abi.PRED_NONE
    for p in (None, none):
        a = run_for32(enc, 0, 10_000, 10_000, p, values)
        assert a.rc == abi.FQ_E_UNSUPPORTED and "no predicate" in a.error
    assert run_for32(enc, -1, 100, 10_000, pred, values).rc == abi.FQ_E_INVALID
    assert run_for32(enc, 0, 100, 8191, pred, values).rc == abi.FQ_E_INVALID
    with pytest.raises(ops.FQError) as ei:
        ops.filter_project_blocks_for32(enc, 10_000, pred, values, first=5, length=-1)
    assert ei.value.status == abi.FQ_E_INVALID
    ops.jit_config(abi.JIT_OFF)
    try:
        a = run_for32(enc, 0, 10_000, 10_000, pred, values)
        assert a.rc == abi.FQ_E_UNSUPPORTED and "JIT is off" in a.error
    finally:
        ops.jit_config(abi.JIT_AUTO, 1 << 22)
    a = run_for32(enc, 77, 0, 10_000, pred, values)  # an empty window: nothing launched, nothing written
    assert a.rc == 0 and a.kept == 0 and len(a.counts) == 0
    # a block longer than the window: one block
    a = run_for32(enc, 3, 70_000, 2**63 - 1, pred, values)
    assert a.rc == 0 and len(a.counts) == 1 and a.counts[0] == a.kept


def test_two_and_a_third_rounds_of_ticket_draws():
    """Sized from the CU count: every workgroup draws two blocks, a third of them a third, at the smallest
    block (one tile) and an odd first; the whole output buffer equals the plain kernel's."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    m = launch_shapes.block_stream(cus, 8192, ops.tune_get("SELECT_BLOCKS_WG_PER_CU"))
    n, _ = m.cases()["ragged"]
    assert min(m.per_worker(n)) == 2 and max(m.per_worker(n)) == 3
    first = 65_535
    col = ops.numbers_column(7 << 40, first + n)
    enc, ok = ops.for32_encode(col)
    assert ok
    pred, values, _, _ = S.shape("p1")
    a = run_for32(enc, first, n, 8192, pred, values[:1])
    b = run_plain(ops.DeviceColumn(col.buf, n, U64, offset=8 * first), 8192, pred, values[:1])
    same(a, b)
    assert a.rc == 0 and a.kept == int(a.counts.sum()) and len(a.counts) == -(-n // 8192)
    x0 = (7 << 40) + first  # numbers: the kept count in closed form
    assert a.kept == sum((n - ((r - x0) % 8) + 7) // 8 for r in range(3))
