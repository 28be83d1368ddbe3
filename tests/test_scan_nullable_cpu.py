"""fq_aggregate_nullable on CPU: the shapes of a fused aggregate scan over
nullable columns (Arrow validity bitmaps) are generated and cross-compiled for
gfx950 through fq_jit_prepare_nullable (no GPU needed -- the code object is
built but not loaded): the Q6 shape with all four bitmaps flat and in block
mode and with one bitmap, a lone UInt8 (G = 16), a lone UInt64, a cast that can
null without any bitmap, a three-leaf tree.  The nullable source is a source of
its own (the typed one of the same types is what fq_jit_prepare_typed alone
produces), a column without a bitmap generates no bitmap parameter, the
argument checks answer without a device.  GPU parity against the oracle is in
tests/test_scan_nullable_gpu.py."""
import ctypes as C
import glob
import os
import re

import pytest

from fq_amd import abi, ops
from fq_amd._lib import FQError, lib
from fq_amd.expr import Col, chain, chain_columns, load, pred_tree_columns, predicate_columns

ALL = abi.AGG_SUM | abi.AGG_MAX | abi.AGG_MIN | abi.AGG_COUNT
I8, I16, I32, I64 = abi.DT_INT8, abi.DT_INT16, abi.DT_INT32, abi.DT_INT64
U8, U16, U32, U64 = abi.DT_UINT8, abi.DT_UINT16, abi.DT_UINT32, abi.DT_UINT64
F32, F64 = abi.DT_FLOAT32, abi.DT_FLOAT64


@pytest.fixture(autouse=True, scope="module")
def _rtc_available():
    ops.jit_config(abi.JIT_AUTO, 1 << 22)
    if not ops.jit_prepare(U64, value=chain(U64, [("+", 1)])[0]):
        pytest.skip("hipRTC not loadable here")
    if ops.jit_stats()["available"] != 1:
        pytest.skip("hipRTC not loadable here")


def q6():
    dts = [F64, F32, I32, U8]
    pred = pred_tree_columns(dts, [([load(2)], "<", (9950, "Int32")), ([load(3)], "<", (26, "UInt8"))], [0, 1, "and"])
    value, vdt = chain_columns(dts, [("*", Col(1))])
    assert vdt == F64
    return dts, pred, value


def test_state_sizes():
    assert C.sizeof(abi.fq_agg_state_n) == 64
    assert C.sizeof(abi.fq_agg_state) == 48
    assert abi.fq_agg_state_n.valid.offset == 48
    assert lib.fq_aggregate_nullable_workspace_bytes(1 << 20) >= 64 * 4096 > lib.fq_aggregate_workspace_bytes(1 << 20)
    assert lib.fq_abi_version() == abi.FQ_ABI_VERSION == 3


def test_q6_shape_compiles_with_four_bitmaps_and_with_one():
    dts, pred, value = q6()
    four = [1, 1, 1, 1]
    assert ops.jit_prepare_nullable(dts, four, pred=pred, value=value, mask=ALL, block_rows=0, length=1 << 27)
    assert ops.jit_prepare_nullable(dts, four, pred=pred, value=value, mask=ALL, block_rows=10000)
    assert ops.jit_prepare_nullable(dts, four, pred=pred, value=value, mask=ALL, block_rows=8191)
    assert ops.jit_prepare_nullable(dts, [0, 0, 0, 1], pred=pred, value=value, mask=ALL, block_rows=0, length=1 << 27)
    assert ops.jit_prepare_nullable(dts, [0, 0, 0, 1], pred=pred, value=value, mask=ALL, block_rows=10000)
    # block mode without a predicate: an unfiltered block whose values are all null is a None sum too
    assert ops.jit_prepare_nullable(dts, four, pred=None, value=value, mask=ALL, block_rows=10000)


def test_lone_columns_compile():
    assert ops.jit_prepare_nullable([U8], [1], mask=ALL, length=30017)  # G = 16
    assert ops.jit_prepare_nullable([U8], [1], mask=ALL, block_rows=10000)
    assert ops.jit_prepare_nullable([I32], [1], mask=ALL, block_rows=10000)
    assert ops.jit_prepare_nullable([F64], [1], mask=ALL, block_rows=10000)
    pred = predicate_columns([U64], [("%", 8)], "<", 3)
    value, _ = chain_columns([U64], [("+", 1)])
    # a 64-bit shape: this entry point runs the typed generator all the same
    assert ops.jit_prepare_nullable([U64], [1], pred=pred, value=value, mask=ALL, length=30017)
    assert ops.jit_prepare_nullable([U64], [1], pred=pred, value=value, mask=ALL, block_rows=10000)


def test_a_cast_that_can_null_compiles_without_any_bitmap():
    dts = [U64, I8]
    value, vdt = chain_columns(dts, [("+", Col(1))])
    assert vdt == I8  # numerical_coercion's order puts Int8 before UInt64: a above 127 is a null
    assert ops.jit_prepare_nullable(dts, None, value=value, mask=ALL, length=30017)
    assert ops.jit_prepare_nullable(dts, [0, 0], value=value, mask=ALL, block_rows=10000)


def test_a_three_leaf_tree_and_a_division_compile():
    dts = [U32, I16, I16]
    pred = pred_tree_columns(dts, [([], "<", Col(1)), ([load(2)], ">", (5, "Int16")), ([load(1)], "=", (7, "Int16"))],
                             [0, 1, "and", 2, "or"])
    value, vdt = chain_columns(dts, [load(1), ("/", Col(2))])
    assert vdt == I16
    for hv in ([1, 1, 1], [0, 1, 0]):
        assert ops.jit_prepare_nullable(dts, hv, pred=pred, value=value, mask=ALL, length=30017)
        assert ops.jit_prepare_nullable(dts, hv, pred=pred, value=value, mask=ALL, block_rows=10000)


def dump(tmp_path, name, fn):
    d = tmp_path / name
    d.mkdir()
    lib.fq_tune_jit_dump_dir(str(d).encode())
    try:
        assert fn()
    finally:
        lib.fq_tune_jit_dump_dir(None)
    return [open(f, "rb").read() for f in sorted(glob.glob(os.path.join(str(d), "*.hip")), key=os.path.getmtime)]


def test_nullable_sources_are_their_own_and_typed_sources_are_unchanged(tmp_path):
    """Only a compile dumps a source.  Without a device nothing is cached and every call compiles; with one, the
    shapes of this test (no other test asks for sum and min alone) compile once each, so the typed shape asked
    for again after the nullable ones finds its own kernel in the cache."""
    import torch
    dts, pred, value = q6()
    kw = dict(pred=pred, value=value, mask=abi.AGG_SUM | abi.AGG_MIN, block_rows=0, length=1 << 27)
    typed = dump(tmp_path, "typed", lambda: ops.jit_prepare_typed(dts, **kw))
    nullable = dump(tmp_path, "nullable", lambda: ops.jit_prepare_nullable(dts, [1, 1, 1, 1], **kw))
    typed_again = dump(tmp_path, "typed_again", lambda: ops.jit_prepare_typed(dts, **kw))
    one = dump(tmp_path, "one", lambda: ops.jit_prepare_nullable(dts, [0, 0, 0, 1], **kw))
    none = dump(tmp_path, "none", lambda: ops.jit_prepare_nullable(dts, None, **kw))
    assert len(typed) == len(nullable) == len(one) == len(none) == 1
    assert typed_again == ([] if torch.cuda.is_available() else typed)
    assert typed[0] != nullable[0]
    assert b"PartialN" in nullable[0] and b"PartialN" not in typed[0] and b"vb0" not in typed[0]

    def bitmap_params(src):
        sig = re.search(rb"fq_jit_scan\((.*?)\)\s*\{", src, re.S).group(1)
        return re.findall(rb"const u64 \*__restrict__ (vb\d)", sig)

    assert bitmap_params(nullable[0]) == [b"vb0", b"vb1", b"vb2", b"vb3"]
    assert bitmap_params(one[0]) == [b"vb3"] and b"vb0" not in one[0]
    assert bitmap_params(none[0]) == [] and re.search(rb"vb\d", none[0]) is None
    assert len({nullable[0], one[0], none[0]}) == 3


def invalid(status, text, fn):
    with pytest.raises(FQError) as e:
        fn()
    assert e.value.status == status, str(e.value)
    assert text in str(e.value), str(e.value)


def test_argument_errors():
    dts, pred, value = q6()
    invalid(abi.FQ_E_INVALID, "n_cols", lambda: ops.jit_prepare_nullable([], None))
    invalid(abi.FQ_E_INVALID, "n_cols", lambda: ops.jit_prepare_nullable([U8] * 5, [1] * 5))
    invalid(abi.FQ_E_INVALID, "rows", lambda: ops.jit_prepare_nullable(dts, [1] * 4, pred=pred, value=value,
                                                                        lengths=[100, 100, 101, 100]))
    invalid(abi.FQ_E_INTERNAL, "Utf8", lambda: ops.jit_prepare_nullable([abi.DT_UTF8], [1]))
    bad, _ = chain_columns([I32, I32], [("+", Col(1))])
    invalid(abi.FQ_E_INVALID, "numerical_coercion", lambda: ops.jit_prepare_nullable([I32, F32], [1, 1], value=bad))
    ops.jit_config(abi.JIT_OFF, 0)
    try:
        invalid(abi.FQ_E_UNSUPPORTED, "hipRTC", lambda: ops.jit_prepare_nullable(dts, [1] * 4, pred=pred, value=value))
        invalid(abi.FQ_E_UNSUPPORTED, "hipRTC", lambda: ops.jit_prepare_nullable([U64], [1], mask=ALL))
    finally:
        ops.jit_config(abi.JIT_AUTO, 1 << 22)


def launch(cols, validity, n_cols=None, ws_bytes=1 << 20):
    """fq_aggregate_nullable straight through ctypes: the argument checks come before any device work"""
    arr = (abi.fq_col * max(len(cols), 1))(*cols)
    vb = (C.c_void_p * max(len(cols), 1))(*validity) if validity is not None else None
    out = (C.c_uint8 * 64)()
    ws = (C.c_uint8 * 64)()
    return lib.fq_aggregate_nullable(arr, vb, len(cols) if n_cols is None else n_cols, 0, None, None, ALL,
                                     C.addressof(out), C.addressof(ws), ws_bytes, None)


def test_launch_argument_errors_answer_before_any_device_work():
    from fq_amd._lib import last_error
    data = (C.c_uint64 * 64)()
    p = C.addressof(data)
    col = abi.fq_col(p, 100, I32, 0)
    assert launch([col], None) == abi.FQ_E_INVALID and "NULL" in last_error()
    assert launch([col], [p + 4]) == abi.FQ_E_INVALID and "aligned to 8" in last_error()
    assert launch([col], [p], n_cols=0) == abi.FQ_E_INVALID and "n_cols" in last_error()
    assert launch([col] * 5, [p] * 5) == abi.FQ_E_INVALID and "n_cols" in last_error()
    assert launch([col, abi.fq_col(p, 101, U8, 0)], [p, None]) == abi.FQ_E_INVALID and "rows" in last_error()
    assert launch([col], [p], ws_bytes=48 * 4096) == abi.FQ_E_INVALID and "workspace" in last_error()


def test_the_launch_fails_loudly_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("needs a machine without a GPU")
    data = (C.c_uint64 * 64)()
    p = C.addressof(data)
    st = launch([abi.fq_col(p, 100, I32, 0)], [p])
    assert st != abi.FQ_OK
    with pytest.raises(FQError):
        ops.aggregate_nullable([], [])
