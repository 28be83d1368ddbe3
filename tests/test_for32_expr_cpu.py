"""fq_aggregate_for32_expr / fq_jit_prepare_for32 without a GPU: the generated
fq_jit_scan_for32 source of every shape the GPU tests run compiles for gfx950
(flat and block mode), the call without predicate and expression is the
precompiled kernel, a delta shape has a kernel and a cache key of its own, the
argument checks answer before any device call, the ABI mirror and option 9 --
and a numpy model of the kernel's walk (tile -> frame -> base, the prefetch,
the remainder vectors, the tail rows, the blocks) that equals the decoded column
on the GPU tests' inputs and is changed by each of three mistakes.  GPU parity:
tests/test_for32_expr_gpu.py, tests/test_for32_expr_launch_gpu.py and
tests/test_engine_for32_expr_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fq_amd import abi, ops
from fq_amd._lib import GPU_SYMBOLS, _protos, last_error, lib
from fq_amd.expr import chain, predicate

import for32_expr_shapes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = abi.DT_UINT64
WS = 4096 * 48  # fq_aggregate_workspace_bytes
SHAPES = ["c4", "c4s", "max1", "push", "tree", "libdivide"]
MASK = {"c4": abi.AGG_MAX | abi.AGG_COUNT, "c4s": abi.AGG_SUM | abi.AGG_COUNT, "max1": abi.AGG_MAX}


@pytest.fixture(autouse=True)
def jit_auto():
    ops.jit_config(abi.JIT_AUTO, 1 << 22)
    yield
    ops.jit_config(abi.JIT_AUTO, 1 << 22)


def test_the_new_calls_and_the_option_are_declared_exported_and_mirrored():
    for name in ("fq_aggregate_for32_expr", "fq_jit_prepare_for32"):
        assert name in GPU_SYMBOLS and hasattr(lib, name)
    assert len(_protos["fq_aggregate_for32_expr"][1]) == 11
    assert len(_protos["fq_jit_prepare_for32"][1]) == 6
    eng = open(os.path.join(ROOT, "include", "fq_engine.h")).read()
    from fq_amd import engine
    opt = int(re.search(r"#define FQ_OPT_RESIDENT_FOR32_FUSED (\d+)", eng).group(1))
    assert opt == engine.OPT_RESIDENT_FOR32_FUSED == 9 != engine.OPT_RESIDENT_FOR32


@pytest.mark.parametrize("block_rows,n", [(0, 1_000_003), (10000, 70_001), (10002, 70_001), (65536, 200_003),
                                          (100000, 200_003)])
@pytest.mark.parametrize("name", SHAPES)
def test_every_shape_compiles_flat_and_in_block_mode(name, block_rows, n):
    pred, value, _, _ = S.shape(name)
    # with a predicate, sum and more than one reference block the scan is in block mode
    for mask in (MASK.get(name, S.ALL), S.ALL):
        assert ops.jit_prepare_for32(pred, value, mask, block_rows, n) is True


def test_more_shapes_compile():
    bm = abi.fq_pred()
    bm.kind = abi.PRED_BITMAP  # the pointer is not read by prepare
    value, _ = chain(U64, [("+", 1)])
    for br in (0, 10000):
        assert ops.jit_prepare_for32(bm, value, S.ALL, br, 200_003)
    f64, dt = chain(U64, [("*", 0.5)])
    assert dt == abi.DT_FLOAT64 and ops.jit_prepare_for32(None, f64, S.ALL, 0, 200_003)
    i64, dt = chain(U64, [("-", (5, "Int64"))])  # the u64 -> i64 cast of the column
    assert dt == abi.DT_INT64 and ops.jit_prepare_for32(None, i64, S.ALL, 0, 200_003)
    div0, _ = chain(U64, [("/", 0)])
    assert ops.jit_prepare_for32(predicate(U64, [], ">", 10**19), div0, S.ALL, 0, 200_003)


def test_without_predicate_and_expression_it_is_the_precompiled_kernel():
    assert ops.jit_prepare_for32(None, None, S.ALL, 0, 1_000_003) is False
    assert ops.jit_prepare_for32(None, None, S.ALL, 10000, 1_000_003) is False
    ident = abi.fq_expr()
    ident.n_steps = 0
    ident.out_dtype = U64
    none = abi.fq_pred()
    none.kind = abi.PRED_NONE
    assert ops.jit_prepare_for32(none, ident, S.ALL, 10000, 1_000_003) is False


def test_jit_off_is_unsupported():
    pred, value, _, _ = S.shape("c4")
    ops.jit_config(abi.JIT_OFF)
    out = C.c_int32(7)
    rc = lib.fq_jit_prepare_for32(1000, 0, C.byref(pred), C.byref(value), abi.AGG_MAX, C.byref(out))
    assert rc == abi.FQ_E_UNSUPPORTED and out.value == 0 and "hipRTC kernel only" in last_error()


def test_a_delta_shape_has_a_source_and_a_key_of_its_own(tmp_path):
    """The same call shape prepared plain and over deltas: two sources (a shared key would have compiled
    one), the delta one with the (delta, fbase) parameters and the frame shift, the plain one without."""
    pred, value, _, _ = S.shape("c4")
    lib.fq_tune_jit_dump_dir(str(tmp_path).encode())
    try:
        assert ops.jit_prepare(U64, pred, value, abi.AGG_MAX | abi.AGG_COUNT, 0, 1_000_003)
        assert ops.jit_prepare_for32(pred, value, abi.AGG_MAX | abi.AGG_COUNT, 0, 1_000_003)
    finally:
        lib.fq_tune_jit_dump_dir(None)
    srcs = sorted(p for p in os.listdir(tmp_path) if p.endswith(".hip"))
    assert len(srcs) == 2
    plain, delta = (open(os.path.join(tmp_path, p)).read() for p in srcs)
    assert "fq_jit_scan(const TIn *__restrict__ col" in plain
    assert "delta" not in plain and "fbase" not in plain and "for32" not in plain
    assert "fq_jit_scan_for32(const u32 *__restrict__ delta, const u64 *__restrict__ fbase" in delta
    assert ">> 16]" in delta and "/ 65536" not in delta  # the frame is a shift, never a 64-bit division
    assert "asm" not in delta
    # the per-row functions are the plain shape's text
    cut = lambda s: s[s.index("struct Step"):s.index('extern "C"')]
    assert cut(plain) == cut(delta)
    # one store: the workgroup's partial
    body = delta[delta.index('extern "C"'):]
    assert body.count("parts[blockIdx.x] = p;") == 1 and "atomic" not in body


def agg(delta, base, n, mask, pred, value, block_rows=0, out=1 << 20, ws=1 << 21, ws_bytes=WS):
    return lib.fq_aggregate_for32_expr(C.c_void_p(delta), C.c_void_p(base), n, block_rows,
                                       C.byref(pred) if pred is not None else None,
                                       C.byref(value) if value is not None else None, mask, C.c_void_p(out),
                                       C.c_void_p(ws), ws_bytes, None)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "identity"])
def test_argument_errors_are_those_of_fq_aggregate_for32(fused):
    # the pointers are never read: every refusal comes before any device call
    pred, value, _, _ = S.shape("c4") if fused else (None, None, None, None)
    for off in (4, 8, 12):
        assert agg((1 << 22) + off, 1 << 23, 100, S.ALL, pred, value) == abi.FQ_E_INVALID
        assert "delta not aligned to 16 bytes" in last_error()
    assert agg(1 << 22, (1 << 23) + 4, 100, S.ALL, pred, value) == abi.FQ_E_INVALID
    assert "base not aligned to 8 bytes" in last_error()
    for mask in (16, 0x1F, 0x80000000):
        assert agg(1 << 22, 1 << 23, 100, mask, pred, value) == abi.FQ_E_INVALID
        assert "unknown bits in agg_mask" in last_error()
    assert agg(1 << 22, 1 << 23, -1, S.ALL, pred, value) == abi.FQ_E_INVALID and "negative length" in last_error()
    assert agg(1 << 22, 1 << 23, 100, S.ALL, pred, value, ws_bytes=WS - 1) == abi.FQ_E_INVALID
    assert "workspace too small" in last_error()
    assert agg(1 << 22, 1 << 23, 100, S.ALL, pred, value, out=None) == abi.FQ_E_INVALID
    assert "NULL argument" in last_error()
    assert agg(1 << 22, 1 << 23, 100, S.ALL, pred, value, ws=None) == abi.FQ_E_INVALID
    assert agg(None, 1 << 23, 100, S.ALL, pred, value) == abi.FQ_E_INVALID and "NULL argument" in last_error()
    assert agg(1 << 22, None, 100, S.ALL, pred, value) == abi.FQ_E_INVALID and "NULL argument" in last_error()


# ---------------------------------------------------------------------------
# the numpy model of the walk
# ---------------------------------------------------------------------------
GRIDS = [3, 16, 512]  # workgroups: several rounds at 1,000,003 rows; a frame per round; MI355X's 256 CUs x 2


@pytest.mark.parametrize("data", S.DATA + ["iota_hi"])
@pytest.mark.parametrize("n", S.LENGTHS)
def test_flat_model_equals_the_decoded_column(n, data):
    host = S.host_values(n, data)
    delta, base = S.encode_host(host)
    for cap in GRIDS:
        x, visits = S.flat_model(delta, base, S.flat_grid(n, cap))
        assert np.array_equal(visits, np.ones(n, np.int32))  # every row once
        assert np.array_equal(x, host)
    for name in ("c4", "c4s", "max1"):
        _, _, keep, val = S.shape(name)
        assert S.reference(x, keep, val) == S.reference(host, keep, val)


@pytest.mark.parametrize("block_rows,n", [(10000, 70_001), (10002, 70_001), (65536, 200_003), (100000, 200_003)])
def test_block_model_equals_the_decoded_column(block_rows, n):
    host = S.host_values(n, "random")
    delta, base = S.encode_host(host)
    x, visits = S.block_model(delta, base, block_rows)
    assert np.array_equal(visits, np.ones(n, np.int32)) and np.array_equal(x, host)


@pytest.fixture(scope="module")
def two_rounds():
    """Exactly two rounds of a 32-workgroup grid (two frames per round) and a ragged end, random bases."""
    grid = 32
    n = 2 * grid * S.TILE + S.TILE // 2 + 3
    host = S.host_values(n, "random")
    return grid, host, S.encode_host(host)


@pytest.mark.parametrize("mistake", ["prefetched_base", "base0_remainder"])
def test_a_wrong_base_in_the_flat_loop_changes_the_result(two_rounds, mistake):
    grid, host, (delta, base) = two_rounds
    assert S.flat_grid(len(host), grid) == grid
    x, _ = S.flat_model(delta, base, grid, mistake)
    assert not np.array_equal(x, host)
    for name in ("c4", "c4s"):
        _, _, keep, val = S.shape(name)
        got, exp = S.reference(x, keep, val), S.reference(host, keep, val)
        assert got != exp and got[0] != exp[0]  # the sum moves with the changed rows


def test_a_blocks_first_frames_base_for_the_whole_block_changes_the_result(two_rounds):
    _, host, (delta, base) = two_rounds
    x, _ = S.block_model(delta, base, 10000, "first_frame_base")  # block 6 = rows 60,000 .. 69,999 crosses 65,536
    assert np.array_equal(x[:65536], host[:65536]) and not np.array_equal(x[65536:70000], host[65536:70000])
    _, _, keep, val = S.shape("c4s")
    assert S.reference(x, keep, val)[0] != S.reference(host, keep, val)[0]
