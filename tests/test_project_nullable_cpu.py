"""The Filter -> Projection block stream over nullable columns without a GPU:
the entry points exist (the ABI version stays 3), the shapes' modules are
generated and cross-compiled for gfx950 through fq_jit_prepare_project_nullable
(one module per set of columns that carry a bitmap), the typed projection's
generated sources hold no text of the nullable variant, the numpy model of the
kernel (tests/project_nullable_cases.py model()) equals the oracle on every case
tests/test_project_nullable_gpu.py runs, every planted mistake is caught by at
least one of those cases, and the argument checks answer before any device call.

Without a device nothing is cached (tests/test_scan_typed_cpu.py): every
prepare compiles, so "the same set compiles once" is asserted where a device is
present and, here, as "the same set generates the same source"."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import project_nullable_cases as PC
from fq_amd import abi, ops
from fq_amd._lib import FQError, check, lib

F64, F32, I32, I64, U8, U16, U64 = PC.F64, PC.F32, PC.I32, PC.I64, PC.U8, PC.U16, PC.U64
NULLABLE_TEXT = ("OutsV", "vst[", "pb_bits", "pb_ones", "fq_vbits", "nv[k]", "u32 n0", "u32 &ok", "vb0")


@pytest.fixture(scope="module")
def rtc():
    ops.jit_config(abi.JIT_AUTO, 1 << 22)
    from fq_amd.expr import chain
    if not ops.jit_prepare(U64, value=chain(U64, [("+", 1)])[0]) or ops.jit_stats()["available"] != 1:
        pytest.skip("hipRTC not loadable here")


def has_device():
    import torch
    return torch.cuda.is_available()


def shapes():
    """(dtypes, pred, values) of the three shapes: the Q6 layout, UInt8 + UInt16, one UInt64 column cast to Int64"""
    out = []
    for name in ("q6", "u8u16", "u64cast"):
        case = PC.SHAPES[name](8)[0]
        out.append((name, case.dts, case.pred, case.values))
    return out


def dumped(tmp, fn):
    before = set(glob.glob(os.path.join(tmp, "*.hip")))
    c0 = ops.jit_stats()["kernels_compiled"]
    lib.fq_tune_jit_dump_dir(tmp.encode())
    try:
        assert fn()
    finally:
        lib.fq_tune_jit_dump_dir(None)
    new = sorted(set(glob.glob(os.path.join(tmp, "*.hip"))) - before, key=os.path.getmtime)
    return [open(p).read() for p in new], ops.jit_stats()["kernels_compiled"] - c0


def test_symbols_exist_and_the_abi_version_stays_3():
    for name in ("fq_filter_project_blocks_nullable", "fq_predicate_bitmap_nullable", "fq_jit_prepare_project_nullable",
                 "fq_functions_eval_nullable"):
        assert hasattr(lib, name), name
    assert lib.fq_abi_version() == 3 == abi.FQ_ABI_VERSION


@pytest.mark.parametrize("shape", [0, 1, 2])
def test_shapes_compile_per_set_of_bitmaps(shape, tmp_path, rtc):
    name, dts, pred, values = shapes()[shape]
    K = len(dts)
    sets = [[0] * K, [0] * (K - 1) + [1], [1] * K]
    if K == 1:
        sets = [[0], [1]]
    texts = []
    for hv in sets:
        src, compiled = dumped(str(tmp_path), lambda: ops.jit_prepare_project_nullable(dts, hv, pred=pred, values=values))
        if has_device():  # compiled at most once per set (0: an earlier test of this process left it in the cache)
            assert compiled <= 1 and len(src) == compiled, (name, hv, compiled)
        else:
            assert compiled == 1 and len(src) == 1, (name, hv, compiled)
        if src:
            text = src[0]
            # block mode only: the block kernel and the predicate bitmap's, no look-back and no map kernel
            assert text.count("\nfq_jit_pblocks(") == 1 and text.count("\nfq_jit_pbits(") == 1, (name, hv)
            assert "fq_jit_pselect" not in text and "fq_jit_pmap" not in text, (name, hv)
            # a column without a bitmap generates neither a parameter nor a load
            for j in range(K):
                assert ("vb%d" % j in text) == bool(hv[j]), (name, hv, j)
            texts.append(text)
        # the same set again: the same module
        again, compiled2 = dumped(str(tmp_path), lambda: ops.jit_prepare_project_nullable(dts, hv, pred=pred, values=values))
        if has_device():
            assert compiled2 == 0 and again == [], (name, hv)
        else:
            assert again == src, (name, hv)
    if not has_device():
        assert len(set(texts)) == len(sets), name  # different sets are different modules


def test_an_absent_has_validity_array_means_no_bitmaps(tmp_path, rtc):
    name, dts, pred, values = shapes()[0]
    src, _ = dumped(str(tmp_path), lambda: ops.jit_prepare_project_nullable(dts, None, pred=pred, values=values))
    for text in src:
        assert "vb0" not in text and "vb3" not in text


@pytest.mark.parametrize("shape", [0, 1, 2])
def test_typed_projection_sources_hold_no_nullable_text(shape, tmp_path, rtc):
    name, dts, pred, values = shapes()[shape]
    for br in (0, 10000):
        src, _ = dumped(str(tmp_path), lambda: ops.jit_prepare_project_typed(dts, pred=pred, values=values, block_rows=br))
        for text in src:
            for word in NULLABLE_TEXT:
                assert word not in text, (name, br, word)
    if not has_device():
        assert src  # something was looked at


def test_needs_the_jit_and_block_geometry(rtc):
    name, dts, pred, values = shapes()[0]
    ops.jit_config(abi.JIT_OFF, 0)
    try:
        with pytest.raises(FQError) as e:
            ops.jit_prepare_project_nullable(dts, [1] * 4, pred=pred, values=values)
        assert e.value.status == abi.FQ_E_UNSUPPORTED and "no unfused path over nulls" in str(e.value)
    finally:
        ops.jit_config(abi.JIT_AUTO, 1 << 22)
    for br in (0, 8191):
        with pytest.raises(FQError) as e:
            ops.jit_prepare_project_nullable(dts, [1] * 4, pred=pred, values=values, block_rows=br)
        assert e.value.status == abi.FQ_E_INVALID and "FQ_PROJECT_MIN_BLOCK_ROWS" in str(e.value)
    assert ops.jit_prepare_project_nullable(dts, [1] * 4, pred=pred, values=values, block_rows=8192)
    assert ops.jit_prepare_project_nullable(dts, [1] * 4, pred=None, values=values)  # FQ_PRED_NONE: the block kernel


# ---------------------------------------------------------------------------
# the model of the kernel against the oracle
# ---------------------------------------------------------------------------
GRID = PC.grid()


def test_the_grid_covers_what_the_issue_lists():
    names = {c.name for c, _ in GRID}
    assert names == {"q6", "u8u16", "u64cast", "u8u16_or"}
    assert {(c.n, br) for c, br in GRID} >= set(PC.SIZES)
    assert max(c.n for c, _ in GRID) > 2_500_000  # the ticket-loop case
    c = PC.get_case("u8u16_or", 25003, "random")
    null_b_true_a = (~c.valid[1]) & c.valid[0] & (c.host[0] < 100)
    assert null_b_true_a.sum() > 100  # a null leaf on rows where the other leaf is true
    c = PC.get_case("u64cast", 25003, "none")
    assert ((c.host[0] >= np.uint64(1 << 63)) & (c.host[0] % np.uint64(8) < 3)).sum() > 50  # kept rows whose cast is a null


def test_model_equals_the_oracle_on_every_case():
    for case, br in GRID:
        assert PC.model_agrees(case, br), (case.name, case.n, br)


@pytest.mark.parametrize("mistake", PC.MISTAKES)
def test_each_mistake_changes_the_model_on_some_case(mistake):
    small = [(c, br) for c, br in GRID if c.n <= 30000]
    caught = [(c.name, c.n, br) for c, br in small if not PC.model_agrees(c, br, mistake)]
    assert caught, mistake


# ---------------------------------------------------------------------------
# argument checks that answer before any device call
# ---------------------------------------------------------------------------
def call(dts, pred, values, validity="ones", out_validity="all", block_rows=10000, vptr=0x2000):
    """fq_filter_project_blocks_nullable over fake, aligned device pointers (never dereferenced by a failing check)"""
    n, K, n_out = 25003, len(dts), len(values)
    arr = (abi.fq_col * K)(*[abi.fq_col(C.c_void_p(0x100000 * (j + 1)), n, dt, 0) for j, dt in enumerate(dts)])
    exprs = ops._project_exprs(values, dts[0])
    outs = (C.c_void_p * n_out)(*[0x1000000 * (j + 1) for j in range(n_out)])
    vb = None if validity is None else (C.c_void_p * K)(*[vptr] * K)
    ov = None
    if out_validity is not None:
        ov = (C.c_void_p * n_out)(*[None if out_validity == "null" else 0x2000000 * (j + 1) for j in range(n_out)])
    kept = C.c_int64(-1)
    st = lib.fq_filter_project_blocks_nullable(arr, vb, K, block_rows, C.byref(pred) if pred is not None else None, exprs,
                                               n_out, outs, ov, C.c_void_p(0x3000000), C.byref(kept), C.c_void_p(0x4000000),
                                               64, None)
    return st, kept.value


def refused(text, **kw):
    name, dts, pred, values = shapes()[0]
    with pytest.raises(FQError) as e:
        st, kept = call(dts, pred, values, **kw)
        assert kept == 0
        check(st)
    assert e.value.status == abi.FQ_E_INVALID and text in str(e.value), str(e.value)


def test_argument_checks_before_any_device_call():
    refused("not aligned to 8 bytes", vptr=0x2004)
    refused("NULL validity array", validity=None)
    refused("NULL output validity array", out_validity=None)
    refused("which can hold nulls", out_validity="null")
    refused("FQ_PROJECT_MIN_BLOCK_ROWS", block_rows=8191)


def test_a_null_output_bitmap_is_refused_exactly_where_the_output_can_be_null():
    name, dts, pred, values = shapes()[2]  # x + 1 as Int64 (the cast can leave its range), x itself
    n = 25003
    arr = (abi.fq_col * 1)(abi.fq_col(C.c_void_p(0x100000), n, U64, 0))
    exprs = ops._project_exprs(values, U64)
    outs = (C.c_void_p * 2)(0x1000000, 0x2000000)
    kept = C.c_int64(0)
    for vb, ov, bad in (((C.c_void_p * 1)(None), (C.c_void_p * 2)(None, 0x5000000), "output 0"),
                        ((C.c_void_p * 1)(0x2000), (C.c_void_p * 2)(0x5000000, None), "output 1")):
        st = lib.fq_filter_project_blocks_nullable(arr, vb, 1, 10000, C.byref(pred), exprs, 2, outs, ov, C.c_void_p(0x3000000),
                                                   C.byref(kept), C.c_void_p(0x4000000), 64, None)
        with pytest.raises(FQError) as e:
            check(st)
        assert e.value.status == abi.FQ_E_INVALID and bad in str(e.value) and "which can hold nulls" in str(e.value)
