"""Frame-of-reference storage (fq_for32_encode / fq_aggregate_for32) on CPU:
the frame arithmetic the host code exposes (frames for a length, the sizes of
the two buffers), the argument checks that answer without a device (alignment,
masks, lengths, the workspace), and the ABI mirror of the new calls and of
FQ_OPT_RESIDENT_FOR32.  GPU parity is in tests/test_for32_gpu.py and
tests/test_engine_for32_gpu.py."""
import ctypes as C
import os
import re

import pytest

from fq_amd import abi
from fq_amd._lib import GPU_SYMBOLS, _protos, last_error, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = abi.FOR32_FRAME_ROWS
ALL = abi.AGG_SUM | abi.AGG_MAX | abi.AGG_MIN | abi.AGG_COUNT
WS = 4096 * 48  # fq_aggregate_workspace_bytes


def test_frame_constant_mirrors_the_header_and_holds_whole_tiles():
    hdr = open(os.path.join(ROOT, "include", "fq_gpu.h")).read()
    assert int(re.search(r"#define FQ_FOR32_FRAME_ROWS (\d+)", hdr).group(1)) == F == 65536
    assert F % 4096 == 0  # the scan's tile: 4 vectors x 256 lanes x 4 u32
    eng = open(os.path.join(ROOT, "include", "fq_engine.h")).read()
    from fq_amd import engine
    assert int(re.search(r"#define FQ_OPT_RESIDENT_FOR32 (\d+)", eng).group(1)) == engine.OPT_RESIDENT_FOR32 == 8


@pytest.mark.parametrize("n,frames", [(-5, 0), (0, 0), (1, 1), (F - 1, 1), (F, 1), (F + 1, 2), (2 * F + 4099, 3),
                                      (1_250_000_000, 19074), (10_000_000_000, 152588)])
def test_frames_and_buffer_sizes(n, frames):
    assert lib.fq_for32_frames(n) == frames
    assert lib.fq_for32_base_bytes(n) == 8 * frames
    db = lib.fq_for32_delta_bytes(n)
    assert db % 256 == 0 and db >= 4 * max(n, 0) and db < 4 * max(n, 0) + 256
    assert (db == 0) == (n <= 0)


def test_the_new_calls_are_declared_exported_and_mirrored():
    for name in ("fq_for32_frames", "fq_for32_delta_bytes", "fq_for32_base_bytes", "fq_for32_encode",
                 "fq_aggregate_for32"):
        assert name in GPU_SYMBOLS and hasattr(lib, name)
    assert len(_protos["fq_for32_encode"][1]) == 5
    assert len(_protos["fq_aggregate_for32"][1]) == 8
    assert lib.fq_aggregate_workspace_bytes(1 << 20) == WS


def agg(delta, base, n, mask, out=1 << 20, ws=1 << 21, ws_bytes=WS):
    return lib.fq_aggregate_for32(C.c_void_p(delta), C.c_void_p(base), n, mask, C.c_void_p(out), C.c_void_p(ws),
                                  ws_bytes, None)


def test_aggregate_refuses_a_delta_pointer_off_16_bytes():
    # the pointers are never read: every refusal comes before any device call
    for off in (4, 8, 12):
        assert agg((1 << 22) + off, 1 << 23, 100, ALL) == abi.FQ_E_INVALID
        assert "delta not aligned to 16 bytes" in last_error()
    assert agg(1 << 22, (1 << 23) + 4, 100, ALL) == abi.FQ_E_INVALID
    assert "base not aligned to 8 bytes" in last_error()


def test_aggregate_refuses_bad_masks_lengths_and_workspaces():
    for mask in (16, 0x1F, 0x80000000):
        assert agg(1 << 22, 1 << 23, 100, mask) == abi.FQ_E_INVALID
        assert "unknown bits in agg_mask" in last_error()
    assert agg(1 << 22, 1 << 23, -1, ALL) == abi.FQ_E_INVALID and "negative length" in last_error()
    assert agg(1 << 22, 1 << 23, 100, ALL, ws_bytes=WS - 1) == abi.FQ_E_INVALID
    assert "workspace too small" in last_error()
    assert agg(1 << 22, 1 << 23, 100, ALL, out=None) == abi.FQ_E_INVALID and "NULL argument" in last_error()
    assert agg(1 << 22, 1 << 23, 100, ALL, ws=None) == abi.FQ_E_INVALID
    assert agg(None, 1 << 23, 100, ALL) == abi.FQ_E_INVALID and "NULL argument" in last_error()


def enc(col, base=1 << 23, delta=1 << 24, flag=1 << 25):
    return lib.fq_for32_encode(C.byref(col) if col is not None else None, C.c_void_p(base), C.c_void_p(delta),
                               C.c_void_p(flag), None)


def test_encode_argument_checks():
    u64 = abi.fq_col(C.c_void_p(1 << 22), 100, abi.DT_UINT64, 0)
    assert enc(None) == abi.FQ_E_INVALID
    assert enc(u64, flag=None) == abi.FQ_E_INVALID and "NULL argument" in last_error()
    assert enc(u64, delta=(1 << 24) + 8) == abi.FQ_E_INVALID and "delta not aligned to 16 bytes" in last_error()
    assert enc(u64, base=(1 << 23) + 4) == abi.FQ_E_INVALID
    assert enc(u64, base=None) == abi.FQ_E_INVALID
    assert enc(abi.fq_col(C.c_void_p(1 << 22), -1, abi.DT_UINT64, 0)) == abi.FQ_E_INVALID
    for dt in (abi.DT_INT64, abi.DT_UINT32, abi.DT_FLOAT64):
        assert enc(abi.fq_col(C.c_void_p(1 << 22), 100, dt, 0)) == abi.FQ_E_UNSUPPORTED
        assert "defined for UInt64" in last_error()
