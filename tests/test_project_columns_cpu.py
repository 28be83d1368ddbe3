"""Filter -> Projection over several columns on CPU: every shape class of
fq_filter_project_columns / fq_filter_project_blocks_columns /
fq_predicate_bitmap_columns is generated and cross-compiled for gfx950 through
fq_jit_prepare_project_columns (no GPU needed -- the code object is built but
not loaded), the argument checks answer without a device, and a one-column
shape generates the single-column entry point's source text.  GPU parity
against the oracle is in tests/test_project_columns_gpu.py."""
import glob
import itertools
import os

import pytest

from fq_amd import abi, ops
from fq_amd._lib import FQError, lib
from fq_amd.expr import STACK, Col, chain, chain_columns, load, pred_tree_columns, predicate, predicate_columns, push
from test_scan_columns_cpu import VALUES

U64, I64, F64, I32 = abi.DT_UINT64, abi.DT_INT64, abi.DT_FLOAT64, abi.DT_INT32


@pytest.fixture(autouse=True, scope="module")
def _rtc_available():
    ops.jit_config(abi.JIT_AUTO, 1 << 22)
    if not ops.jit_prepare(U64, value=chain(U64, [("+", 1)])[0]):
        pytest.skip("hipRTC not loadable here")
    if ops.jit_stats()["available"] != 1:
        pytest.skip("hipRTC not loadable here")


def bitmap_pred():
    p = abi.fq_pred()
    p.kind = abi.PRED_BITMAP
    return p


def every_geometry(dts, pred, values):
    """contiguous (block_rows 0), the minimum block, the reference's block; and the same shape behind a bitmap"""
    for br in (0, 8192, 10000):
        assert ops.jit_prepare_project_columns(dts, pred=pred, values=values, block_rows=br)
    assert ops.jit_prepare_project_columns(dts, pred=bitmap_pred(), values=values, block_rows=10000)


def value_sets():
    """The value shapes of test_scan_columns_cpu.VALUES taken two and three at a time as the outputs of one call:
    (names, column dtypes, [steps per output]).  The shapes keep their own column numbers, so a combination is
    taken only when its members fit ONE column list: each one's dtypes are a prefix of the widest one's (a*b with
    a+b*c; u64*i64 with the four-column mixed tree; ...).  Combinations over conflicting lists (u64*i64 with
    u64*f64: column 1 cannot be both) are left out; a shape that fits no combination (i64*f64: nothing else
    starts from an Int64 column) is paired with a plain reference to its last column."""
    out = []
    for r in (2, 3):
        for combo in itertools.combinations(VALUES, r):
            widest = max((c[1] for c in combo), key=len)
            if all(list(c[1]) == list(widest[:len(c[1])]) for c in combo):
                out.append((tuple(c[0] for c in combo), list(widest), [c[2] for c in combo]))
    used = {n for s in out for n in s[0]}
    for name, dts, steps in VALUES:
        if name not in used:
            out.append(((name, "last column"), list(dts), [steps, [load(len(dts) - 1)]]))
    return out


SETS = value_sets()


@pytest.mark.parametrize("names,dts,steps", SETS, ids=[" , ".join(s[0]) for s in SETS])
def test_value_shapes_as_outputs_over_one_column_list(names, dts, steps):
    assert {len(s[2]) for s in SETS} == {2, 3}
    assert {v[0] for v in VALUES} <= {n for s in SETS for n in s[0]}  # every value shape is an output somewhere
    values = [chain_columns(dts, st)[0] for st in steps]
    last = len(dts) - 1
    every_geometry(dts, predicate_columns(dts, [load(last)], "<", 5), values)  # (every module holds the map kernel)


PREDS = [
    ("c<k", [U64, U64, U64], [load(2)], "<", 7),
    ("a<b", [U64, U64], [], "<", Col(1)),
    ("(a+1)>=b", [U64, U64], [("+", 1)], ">=", Col(1)),
]


@pytest.mark.parametrize("name,dts,lhs,cmp,rhs", PREDS, ids=[p[0] for p in PREDS])
def test_predicate_shapes(name, dts, lhs, cmp, rhs):
    last = len(dts) - 1
    values = [chain_columns(dts, [("*", Col(last))])[0], chain_columns(dts, [load(last), ("+", Col(0))])[0]]
    every_geometry(dts, predicate_columns(dts, lhs, cmp, rhs), values)


@pytest.mark.parametrize("k", [2, 3, 4])
def test_and_or_tree_with_leaves_on_different_columns_mixed_dtypes(k):
    dts = [U64, I64, F64, U64][:k]
    leaves = [([], "<", Col(1)), ([load(k - 1)], "=", 7), ([("+", Col(k - 1))], ">=", 3.5)]
    pred = pred_tree_columns(dts, leaves, [0, 1, "or", 2, "and"])
    values = [chain_columns(dts, [push(1), ("*", Col(k - 1)), ("+", STACK, True)])[0],
              chain_columns(dts, [load(k - 1)])[0], None]
    every_geometry(dts, pred, values)


@pytest.mark.parametrize("k", [2, 3, 4])
def test_max_project_outputs_over_k_columns(k):
    dts = [U64] * k
    values = [chain_columns(dts, [load(j % k), ("+", j)])[0] for j in range(abi.MAX_PROJECT)]
    assert ops.jit_prepare_project_columns(dts, pred=predicate_columns(dts, [load(k - 1)], "<", 5), values=values,
                                           block_rows=10000)
    assert ops.jit_prepare_project_columns(dts, pred=None, values=values)  # the map kernel


def test_needs_the_jit():
    dts = [U64, U64]
    values = [chain_columns(dts, [("*", Col(1))])[0]]
    ops.jit_config(abi.JIT_OFF, 0)
    try:
        assert not ops.jit_prepare_project_columns(dts, values=values)
    finally:
        ops.jit_config(abi.JIT_AUTO, 1 << 22)
    assert ops.jit_prepare_project_columns(dts, values=values, length=10)


def invalid(dts, status, text, **kw):
    with pytest.raises(FQError) as e:
        ops.jit_prepare_project_columns(dts, **kw)
    assert e.value.status == status, str(e.value)
    assert text in str(e.value), str(e.value)


def test_validation_errors():
    v2 = chain_columns([U64, U64], [("*", Col(1))])[0]
    invalid([], abi.FQ_E_INVALID, "n_cols")
    invalid([U64] * 5, abi.FQ_E_INVALID, "n_cols")
    invalid([U64, I32], abi.FQ_E_UNSUPPORTED, "Int32", values=[v2])
    invalid([I32], abi.FQ_E_UNSUPPORTED, "Int32")
    invalid([U64, U64], abi.FQ_E_INVALID, "rows", values=[v2], lengths=[100, 101])
    # a column number >= n_cols: an operand, a PUSH, a LOAD, a predicate's right-hand column, a tree leaf's
    for steps in ([("*", Col(2))], [push(2), ("*", Col(1)), ("+", STACK, True)], [load(2), ("*", Col(1))]):
        bad = chain_columns([U64, U64, U64], steps)[0]
        invalid([U64, U64], abi.FQ_E_INVALID, "column index", values=[v2, bad])
    invalid([U64, U64], abi.FQ_E_INVALID, "column index", values=[v2],
            pred=predicate_columns([U64] * 3, [], "<", Col(2)))
    invalid([U64, U64], abi.FQ_E_INVALID, "column index", values=[v2],
            pred=pred_tree_columns([U64] * 3, [([], "<", Col(1)), ([], "<", Col(2))], [0, 1, "and"]))
    invalid([U64], abi.FQ_E_INVALID, "column index", values=[v2])
    invalid([U64, U64], abi.FQ_E_INVALID, "n_out", values=[])
    invalid([U64, U64], abi.FQ_E_INVALID, "n_out", values=[v2] * 9)
    invalid([U64, U64], abi.FQ_E_INVALID, "FQ_PROJECT_MIN_BLOCK_ROWS", values=[v2], block_rows=8191)


def test_workspace_depends_on_the_column_count():
    n = 1 << 20
    one = lib.fq_filter_project_workspace_bytes(n)
    assert lib.fq_filter_project_columns_workspace_bytes(n, 1) == one
    sizes = [lib.fq_filter_project_columns_workspace_bytes(n, k) for k in (2, 3, 4)]
    assert one < sizes[0] == sizes[1] < sizes[2]  # tiles of 8192, 4096, 4096, 2048 rows: one status word each


def dumped_sources(tmp, fn):
    before = set(glob.glob(os.path.join(tmp, "*.hip")))
    lib.fq_tune_jit_dump_dir(tmp.encode())
    try:
        fn()
    finally:
        lib.fq_tune_jit_dump_dir(None)
    new = sorted(set(glob.glob(os.path.join(tmp, "*.hip"))) - before)
    return [open(p).read() for p in new]


def test_one_column_shape_generates_the_single_column_source(tmp_path):
    value = chain(U64, [("+", 1), ("*", 3)])[0]
    pred = predicate(U64, [("%", 8)], "<", 3)
    old = dumped_sources(str(tmp_path), lambda: ops.project_compile_check(U64, pred, [value, None]))
    new = dumped_sources(str(tmp_path), lambda: ops.jit_prepare_project_columns([U64], pred=pred, values=[value, None],
                                                                               block_rows=10000))
    assert len(old) == 1 and len(new) == 1
    assert new[0] == old[0]
    assert "TIn0" not in new[0] and "fq_pred(TIn x," in new[0]
