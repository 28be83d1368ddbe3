"""fq_filter_project_blocks_for32 / fq_jit_prepare_project_for32 without a GPU:
the calls are declared, exported and mirrored; the generated
fq_jit_pblocks_for32 source of every shape the GPU tests run compiles for gfx950
at every block size; the module holds that kernel alone under a key of its own
and shares the per-row functions and the walk with fq_jit_pblocks; the argument
checks answer before any device call; and a numpy model of the load phase (tile
-> fb_lo / fb_hi -> per-row choice, aligned pair loads against element loads)
equals the decoded window on the GPU tests' cases and is changed by each of four
mistakes.  GPU parity: tests/test_for32_project_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fq_amd import abi, ops
from fq_amd._lib import GPU_SYMBOLS, _protos, last_error, lib

import for32_project_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = abi.DT_UINT64


@pytest.fixture(autouse=True)
def jit_auto():
    ops.jit_config(abi.JIT_AUTO, 1 << 22)
    yield
    ops.jit_config(abi.JIT_AUTO, 1 << 22)


def test_the_new_calls_are_declared_exported_and_mirrored():
    gpu_h = open(os.path.join(ROOT, "include", "fq_gpu.h")).read()
    for name, nargs in (("fq_filter_project_blocks_for32", 14), ("fq_jit_prepare_project_for32", 5)):
        assert name in GPU_SYMBOLS and hasattr(lib, name)
        assert len(_protos[name][1]) == nargs
        decl = re.search(r"fq_status %s\(([^;]*)\);" % name, gpu_h).group(1)
        assert decl.count(",") + 1 == nargs
    assert int(re.search(r"#define FQ_ABI_VERSION (\d+)", gpu_h).group(1)) == 3 == lib.fq_abi_version()
    import inspect
    sig = inspect.signature(ops.filter_project_blocks_for32)
    assert list(sig.parameters) == ["enc", "block_rows", "pred", "values", "first", "length", "stream", "out_offset"]


@pytest.mark.parametrize("block_rows", [8192, 10_000, 10_001, 65_536])
@pytest.mark.parametrize("name", ["p1", "tree", "eight", "runs", "all", "none"])
def test_every_shape_compiles(name, block_rows):
    pred, values, _, _ = S.shape(name)
    assert ops.jit_prepare_project_for32(pred, values, block_rows) is True


def test_a_bitmap_predicate_and_a_float_output_compile():
    bm = abi.fq_pred()
    bm.kind = abi.PRED_BITMAP  # the pointer is not read by prepare
    _, values, _, _ = S.shape("tree")
    assert values[0].out_dtype == abi.DT_FLOAT64
    for br in (8192, 10_000, 10_001, 65_536):
        assert ops.jit_prepare_project_for32(bm, values, br) is True


def prep(block_rows, pred, values, n_out=None):
    exprs = ops._project_exprs(values, U64)
    out = C.c_int32(7)
    rc = lib.fq_jit_prepare_project_for32(block_rows, C.byref(pred) if pred is not None else None, exprs,
                                          len(values) if n_out is None else n_out, C.byref(out))
    return rc, out.value


def test_prepare_refusals():
    pred, values, _, _ = S.shape("p1")
    assert prep(8191, pred, values) == (abi.FQ_E_INVALID, 0) and "FQ_PROJECT_MIN_BLOCK_ROWS" in last_error()
    assert prep(0, pred, values)[0] == abi.FQ_E_INVALID  # (0 means "no block stream" to the plain prepare only)
    assert prep(10_000, pred, values, 0)[0] == abi.FQ_E_INVALID
    assert prep(10_000, pred, values, 9)[0] == abi.FQ_E_INVALID
    none = abi.fq_pred()
    none.kind = abi.PRED_NONE
    for p in (None, none):  # the map kernel is another launch
        assert prep(10_000, p, values) == (abi.FQ_E_UNSUPPORTED, 0) and "no predicate" in last_error()
    ops.jit_config(abi.JIT_OFF)
    assert prep(10_000, pred, values) == (abi.FQ_OK, 0)  # the caller's plain path answers


def test_the_module_holds_the_for32_kernel_alone_under_a_key_of_its_own(tmp_path):
    """The same call shape prepared plain and over deltas: two sources (a shared key would have compiled one)."""
    pred, values, _, _ = S.shape("p1")
    lib.fq_tune_jit_dump_dir(str(tmp_path).encode())
    try:
        assert ops.jit_prepare_project_columns([U64], pred, values, 10_000)
        assert ops.jit_prepare_project_for32(pred, values, 10_000)
    finally:
        lib.fq_tune_jit_dump_dir(None)
    srcs = sorted(p for p in os.listdir(tmp_path) if p.endswith(".hip"))
    assert len(srcs) == 2
    plain, delta = sorted((open(os.path.join(tmp_path, p)).read() for p in srcs), key=lambda t: "_for32(" in t)
    assert "fq_jit_pblocks(const TIn *__restrict__ col" in plain
    assert "delta" not in plain and "fbase" not in plain and "for32" not in plain
    assert "fq_jit_pblocks_for32(const u32 *__restrict__ delta, const u64 *__restrict__ fbase, long long first" in delta
    assert re.findall(r"\nfq_jit_\w+", delta) == ["\nfq_jit_pblocks_for32"]  # no bits / select / map kernel
    assert ">> 16" in delta and "/ 65536" not in delta and "asm" not in delta
    # the second base's index is clamped to the window's last row
    assert "fbase[f_hi < f_last ? f_hi : f_last]" in delta and "(first + end - 1) >> 16" in delta
    # the per-row functions are the plain shape's text
    cut = lambda s: s[s.index("struct Step"):s.index("__device__ __forceinline__ u32 wave_or")]
    assert cut(plain) == cut(delta)
    # so is everything of the walk but the load phase: from the ballots to the kernel's end, and the PB_* head
    tail = lambda s: s[s.rindex("#pragma unroll\n        for (int k = 0; k < PB_NP; ++k) {\n"
                                "            const long long row = r0 + 2 * (long long)(tid + k * PB_THREADS);\n"
                                "            const u32 live0"):]
    assert tail(plain) == tail(delta)
    head = lambda s: s[s.index("#define PB_ROWS"):s.rindex('extern "C"')]
    assert head(plain) == head(delta)


def call(delta=1 << 22, base=1 << 23, first=0, n=100, block_rows=10_000, pred="p1", out=1 << 24, counts=1 << 25,
         ws=1 << 26, ws_bytes=24, out_len=True):
    p, values, _, _ = S.shape("p1")
    p = p if pred == "p1" else pred
    exprs = ops._project_exprs(values, U64)
    ptrs = (C.c_void_p * 2)(out, out)
    kept = C.c_int64(-1)
    rc = lib.fq_filter_project_blocks_for32(C.c_void_p(delta), C.c_void_p(base), first, n, block_rows,
                                            C.byref(p) if p is not None else None, exprs, 2, ptrs, C.c_void_p(counts),
                                            C.byref(kept) if out_len else None, C.c_void_p(ws), ws_bytes, None)
    return rc


def test_the_argument_checks_answer_without_a_device():
    # the pointers are never read: every refusal comes before any device call
    I = abi.FQ_E_INVALID
    assert call(first=-1) == I and "negative first" in last_error()
    assert call(n=-1) == I and "negative length" in last_error()
    assert call(delta=None) == I and "NULL" in last_error()
    assert call(base=None) == I and "NULL" in last_error()
    assert call(counts=None) == I and "NULL" in last_error()
    assert call(out=None) == I and "NULL" in last_error()
    assert call(block_rows=8191) == I and "FQ_PROJECT_MIN_BLOCK_ROWS" in last_error()
    assert call(block_rows=0) == I
    assert call(out_len=False) == I and "out_len" in last_error()
    assert call(delta=(1 << 22) + 2) == I and call(base=(1 << 23) + 4) == I
    none = abi.fq_pred()
    none.kind = abi.PRED_NONE
    for p in (None, none):
        assert call(pred=p) == abi.FQ_E_UNSUPPORTED and "no predicate" in last_error()
    ops.jit_config(abi.JIT_OFF)
    assert call() == abi.FQ_E_UNSUPPORTED and "JIT is off" in last_error()


# ---------------------------------------------------------------------------
# the numpy model of the load phase
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def encoded():
    """kind -> {encoded length: (host, delta, base)}; the short column is the long one's first three frames"""
    res = {}
    for kind in ("random", "iota"):
        host = S.host_column(S.ENC_LEN, kind)
        delta, base = S.encode_host(host)
        assert np.array_equal(delta.astype(np.uint64) + np.repeat(base, S.F)[:len(host)], host)
        res[kind] = {S.ENC_LEN: (host, delta, base),
                     S.ENC_SHORT: (host[:S.ENC_SHORT], delta[:S.ENC_SHORT], base[:S.ENC_SHORT // S.F])}
    return res


def test_the_cases_end_inside_the_last_frame_and_at_the_encoded_end():
    for enc_len in (S.ENC_LEN, S.ENC_SHORT):
        frames = -(-enc_len // S.F)
        ends = {first + n for e, first, n in S.windows() if e == enc_len}
        assert max(ends) == enc_len
        assert any((e - 1) >> 16 == frames - 1 and e < enc_len for e in ends) or enc_len == S.ENC_LEN
    # without the clamp a last tile's second base would be read past the short column's bases
    frames = S.ENC_SHORT // S.F
    over = [(first, n, br) for e, first, n in S.windows() if e == S.ENC_SHORT for br in S.BLOCK_ROWS
            for b0 in range(0, n, br) for r0 in range(b0, min(b0 + br, n), S.TILE)
            if (first + r0 + S.TILE - 1) >> 16 >= frames]
    assert over and all(first + n > S.ENC_SHORT - S.TILE for first, n, _ in over)


@pytest.mark.parametrize("kind", ["random", "iota"])
@pytest.mark.parametrize("block_rows", S.BLOCK_ROWS)
def test_the_model_equals_the_decoded_window(encoded, kind, block_rows):
    for enc_len, first, n in S.windows():
        host, delta, base = encoded[kind][enc_len]
        for addr in (0, 4):  # the deltas' start 8-byte aligned or not
            x, visits = S.walk(delta, base, first, n, block_rows, delta_addr=addr)  # (asserts every base index)
            assert np.array_equal(visits, np.ones(n, np.int32))  # every row once
            assert np.array_equal(x, host[first:first + n]), (first, n, addr)


@pytest.mark.parametrize("mistake", S.MISTAKES)
def test_each_mistake_changes_a_case(encoded, mistake):
    host, delta, base = encoded["random"][S.ENC_LEN]
    changed = []
    for block_rows in S.BLOCK_ROWS:
        for _, first, n in S.windows():
            x, _ = S.walk(delta, base, first, n, block_rows, mistake)
            if not np.array_equal(x, host[first:first + n]):
                changed.append((first, n, block_rows))
    assert changed, mistake
    if mistake == "pair_base":  # only a pair that straddles a frame edge: an odd first, or an odd block size
        assert all(first % 2 == 1 or br % 2 == 1 for first, _, br in changed)
    if mistake in ("no_first_in_frame", "no_first_in_alignment"):
        assert all(first != 0 for first, _, _ in changed)
    # and a changed row changes the p1 outputs of its block
    first, n, br = changed[0]
    x, _ = S.walk(delta, base, first, n, br, mistake)
    _, _, keep, fns = S.shape("all")
    want = S.expect_blocks(host[first:first + n], keep(host[first:first + n]), fns, br)
    got = S.expect_blocks(x, keep(x), fns, br)
    assert any(not np.array_equal(g, w) for g, w in zip(got[0], want[0]))
