"""Tensor-level wrappers over the C ABI of include/fq_gpu.h.

PyTorch only provides device memory and the current HIP stream here; every
computation is one of the library's gfx950 kernels.  All functions raise
FQError (status + the reference's error text) on failure, and raise
immediately when no GPU is present -- there is no CPU fallback.
"""
import ctypes as C

import numpy as np
import torch

from . import abi
from ._lib import FQError, check, last_error, lib  # noqa: F401
from .expr import from_bits, to_bits

NP_DTYPES = {
    abi.DT_INT8: np.int8, abi.DT_INT16: np.int16, abi.DT_INT32: np.int32,
    abi.DT_INT64: np.int64, abi.DT_UINT8: np.uint8, abi.DT_UINT16: np.uint16,
    abi.DT_UINT32: np.uint32, abi.DT_UINT64: np.uint64, abi.DT_FLOAT32: np.float32,
    abi.DT_FLOAT64: np.float64,
}
DT_OF_NP = {np.dtype(v): k for k, v in NP_DTYPES.items()}
ELEM_SIZE = {k: np.dtype(v).itemsize for k, v in NP_DTYPES.items()}


def require_gpu():
    if not torch.cuda.is_available():
        raise FQError(abi.FQ_E_HIP, "fq_amd: no GPU visible (the device path has no CPU fallback)")


def _stream(stream=None):
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


class DeviceColumn:
    """An Arrow-layout column in HBM (values buffer, no nulls).  Boolean
    columns are LSB-first bitmaps in uint64 words."""

    def __init__(self, buf, length, dtype, offset=0):
        self.buf = buf  # torch uint8 tensor owning the bytes
        self.len = int(length)
        self.dtype = dtype
        self.offset = offset

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.offset

    def col(self):
        return abi.fq_col(C.c_void_p(self.ptr), self.len, self.dtype, 0)

    def nbytes(self):
        if self.dtype == abi.DT_BOOLEAN:
            return ((self.len + 63) // 64) * 8
        return self.len * ELEM_SIZE[self.dtype]

    def to_numpy(self):
        nb = self.nbytes()
        host = self.buf[self.offset:self.offset + nb].cpu().numpy()
        if self.dtype == abi.DT_BOOLEAN:
            words = host.view(np.uint64)
            bits = np.unpackbits(words.view(np.uint8), bitorder="little")
            return bits[: self.len].astype(bool)
        return host.view(NP_DTYPES[self.dtype]).copy()


def empty_column(n, dtype, device=None):
    require_gpu()
    nb = ((n + 63) // 64) * 8 if dtype == abi.DT_BOOLEAN else n * ELEM_SIZE[dtype]
    buf = torch.empty(max(nb, 16), dtype=torch.uint8, device=device or "cuda")
    return DeviceColumn(buf, n, dtype)


class _RawDevice:
    """A device allocation presented to torch through __cuda_array_interface__."""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


_hip = None


def contiguous_column(n, dtype):
    """A column in physically contiguous HBM (hipExtMallocWithFlags with
    hipDeviceMallocContiguous), freed with its tensor.  Output buffers of the
    block-stream Filter -> Projection run faster more often in such memory
    (profiles/r03_s3_output_placement.txt); the kernels accept any device memory."""
    global _hip
    require_gpu()
    import weakref
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so.7")  # torch's HIP runtime, already loaded (see _lib._load)
        _hip.hipExtMallocWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
        _hip.hipFree.argtypes = [C.c_void_p]
    nb = max(((n + 63) // 64) * 8 if dtype == abi.DT_BOOLEAN else n * ELEM_SIZE[dtype], 16)
    p = C.c_void_p()
    rc = _hip.hipExtMallocWithFlags(C.byref(p), nb, 0x4)  # hipDeviceMallocContiguous
    if rc != 0:
        raise FQError(abi.FQ_E_HIP, "hipExtMallocWithFlags(hipDeviceMallocContiguous, %d bytes) failed: %d" % (nb, rc))
    buf = torch.as_tensor(_RawDevice(p.value, nb), device="cuda")
    fin = weakref.finalize(buf, _hip.hipFree, C.c_void_p(p.value))
    fin.atexit = False  # never call into HIP during interpreter shutdown; process exit releases it
    return DeviceColumn(buf, n, dtype)


def device_view(ptr, nbytes):
    """A torch uint8 tensor over device memory the library owns (no copy, not
    freed by torch): e.g. a block of fq_engine_execute_blocks."""
    require_gpu()
    return torch.as_tensor(_RawDevice(int(ptr), max(int(nbytes), 1)), device="cuda")


def device_block_to_numpy(b):
    """An fq_device_block's columns as numpy, one list of per-block arrays per
    column (block-stream layout) or one array per column (plain)."""
    cols = [b.columns[j] for j in range(b.n_columns)]
    if b.block_rows > 0:
        counts = device_view(b.d_counts, 8 * b.n_blocks).cpu().numpy().view(np.int64).copy() if b.n_blocks else \
            np.zeros(0, np.int64)
    out = []
    for c in cols:
        h = device_view(c.data, c.len * ELEM_SIZE[c.dtype]).cpu().numpy().view(NP_DTYPES[c.dtype]).copy() \
            if c.len else np.zeros(0, NP_DTYPES[c.dtype])
        if b.block_rows > 0:
            out.append([h[k * b.block_rows: k * b.block_rows + int(n)] for k, n in enumerate(counts)])
        else:
            out.append(h[:b.rows])
    return out


def from_numpy(arr, dtype=None):
    require_gpu()
    arr = np.ascontiguousarray(arr)
    dt = dtype if dtype is not None else DT_OF_NP[arr.dtype]
    raw = arr.view(np.uint8).reshape(-1) if arr.size else np.zeros(16, np.uint8)
    buf = torch.from_numpy(raw.copy()).to("cuda")
    return DeviceColumn(buf, arr.shape[0], dt)


def numbers_column(begin, count, stream=None):
    """SourceTransform of one numbers_mt range: [begin, begin+count)."""
    c = empty_column(count, abi.DT_UINT64)
    check(lib.fq_fill_numbers_u64(C.c_void_p(c.ptr), begin, count, _stream(stream)))
    return c


def splitmix_column(seed, first_index, count, stream=None):
    c = empty_column(count, abi.DT_UINT64)
    check(lib.fq_fill_splitmix64(C.c_void_p(c.ptr), seed, first_index, count, _stream(stream)))
    return c


class Workspace:
    def __init__(self, nbytes):
        require_gpu()
        self.buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device="cuda")
        self.nbytes = self.buf.numel()

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr())


def aggregate_async(col, block_rows=0, pred=None, value=None, mask=0xF, ws=None, out=None,
                    stream=None):
    """Launch fq_aggregate; returns the device tensor holding the fq_agg_state."""
    require_gpu()
    ws = ws or Workspace(lib.fq_aggregate_workspace_bytes(col.len))
    if out is None:
        out = torch.empty(48, dtype=torch.uint8, device="cuda")
    c = col.col()
    check(lib.fq_aggregate(C.byref(c), block_rows, C.byref(pred) if pred is not None else None,
                           C.byref(value) if value is not None else None, mask,
                           C.c_void_p(out.data_ptr()), ws.ptr, ws.nbytes, _stream(stream)))
    return out


def state_from_device(t):
    raw = t.cpu().numpy().tobytes()
    return abi.fq_agg_state.from_buffer_copy(raw)


def aggregate(col, block_rows=0, pred=None, value=None, mask=0xF, ws=None, stream=None):
    """Fused AggregatePartial over one device block -> host fq_agg_state."""
    t = aggregate_async(col, block_rows, pred, value, mask, ws, None, stream)
    return state_from_device(t)


def aggregate_columns_async(cols, block_rows=0, pred=None, value=None, mask=0xF, ws=None, out=None, stream=None):
    """Launch fq_aggregate_columns over a list of DeviceColumns of one block
    (expr.chain_columns / predicate_columns number them by position); returns
    the device tensor holding the fq_agg_state."""
    require_gpu()
    ws = ws or Workspace(lib.fq_aggregate_workspace_bytes(cols[0].len if cols else 0))
    if out is None:
        out = torch.empty(48, dtype=torch.uint8, device="cuda")
    arr = (abi.fq_col * max(len(cols), 1))(*[c.col() for c in cols])
    check(lib.fq_aggregate_columns(arr, len(cols), block_rows, C.byref(pred) if pred is not None else None,
                                   C.byref(value) if value is not None else None, mask,
                                   C.c_void_p(out.data_ptr()), ws.ptr, ws.nbytes, _stream(stream)))
    return out


def aggregate_columns(cols, block_rows=0, pred=None, value=None, mask=0xF, ws=None, stream=None):
    """Fused AggregatePartial over up to abi.MAX_SCAN_COLS columns of one
    device block -> host fq_agg_state."""
    return state_from_device(aggregate_columns_async(cols, block_rows, pred, value, mask, ws, None, stream))


def aggregate_typed_async(cols, block_rows=0, pred=None, value=None, mask=0xF, ws=None, out=None, stream=None):
    """Launch fq_aggregate_typed over a list of DeviceColumns of one block, each
    of any numeric dtype (expr.chain_columns / predicate_columns type the steps);
    returns the device tensor holding the fq_agg_state."""
    require_gpu()
    ws = ws or Workspace(lib.fq_aggregate_workspace_bytes(cols[0].len if cols else 0))
    if out is None:
        out = torch.empty(48, dtype=torch.uint8, device="cuda")
    arr = (abi.fq_col * max(len(cols), 1))(*[c.col() for c in cols])
    check(lib.fq_aggregate_typed(arr, len(cols), block_rows, C.byref(pred) if pred is not None else None,
                                 C.byref(value) if value is not None else None, mask,
                                 C.c_void_p(out.data_ptr()), ws.ptr, ws.nbytes, _stream(stream)))
    return out


def aggregate_typed(cols, block_rows=0, pred=None, value=None, mask=0xF, ws=None, stream=None):
    """Fused AggregatePartial over up to abi.MAX_SCAN_COLS columns of any
    numeric dtypes of one device block -> host fq_agg_state."""
    return state_from_device(aggregate_typed_async(cols, block_rows, pred, value, mask, ws, None, stream))


def aggregate_nullable_async(cols, validity, block_rows=0, pred=None, value=None, mask=0xF, ws=None, out=None,
                             stream=None):
    """Launch fq_aggregate_nullable: aggregate_typed_async over nullable columns.
    validity: per column None or a UInt64 DeviceColumn of ceil(len / 64) Arrow
    validity-bitmap words (bit i = row i of the column is valid); returns the
    device tensor holding the fq_agg_state_n."""
    require_gpu()
    ws = ws or Workspace(lib.fq_aggregate_nullable_workspace_bytes(cols[0].len if cols else 0))
    if out is None:
        out = torch.empty(64, dtype=torch.uint8, device="cuda")
    arr = (abi.fq_col * max(len(cols), 1))(*[c.col() for c in cols])
    vb = None
    if validity is not None:
        vb = (C.c_void_p * max(len(cols), 1))(*[getattr(v, "ptr", v) for v in validity])
    check(lib.fq_aggregate_nullable(arr, vb, len(cols), block_rows, C.byref(pred) if pred is not None else None,
                                    C.byref(value) if value is not None else None, mask,
                                    C.c_void_p(out.data_ptr()), ws.ptr, ws.nbytes, _stream(stream)))
    return out


def aggregate_nullable(cols, validity, block_rows=0, pred=None, value=None, mask=0xF, ws=None, stream=None):
    """Fused AggregatePartial over up to abi.MAX_SCAN_COLS nullable columns of
    one device block -> host fq_agg_state_n."""
    t = aggregate_nullable_async(cols, validity, block_rows, pred, value, mask, ws, None, stream)
    return abi.fq_agg_state_n.from_buffer_copy(t.cpu().numpy().tobytes())


class For32Column:
    """A UInt64 column as fq_for32_encode stores it: `delta` (UInt32, one per
    row) and `base` (UInt64, one per frame of abi.FOR32_FRAME_ROWS rows)."""

    def __init__(self, delta, base, length):
        self.delta = delta
        self.base = base
        self.len = int(length)

    def decode(self):
        """base[i / F] + delta[i] on the host (numpy uint64, wrapping)."""
        d = self.delta.to_numpy().astype(np.uint64)
        b = self.base.to_numpy()
        return d + np.repeat(b, abi.FOR32_FRAME_ROWS)[: self.len]


def for32_encode(col, stream=None):
    """fq_for32_encode of a UInt64 DeviceColumn -> (For32Column, encodable)."""
    require_gpu()
    n = col.len
    delta = DeviceColumn(torch.empty(max(lib.fq_for32_delta_bytes(n), 256), dtype=torch.uint8, device="cuda"), n,
                         abi.DT_UINT32)
    base = DeviceColumn(torch.empty(max(lib.fq_for32_base_bytes(n), 256), dtype=torch.uint8, device="cuda"),
                        lib.fq_for32_frames(n), abi.DT_UINT64)
    flag = torch.empty(1, dtype=torch.int32, device="cuda")
    c = col.col()
    check(lib.fq_for32_encode(C.byref(c), C.c_void_p(base.ptr), C.c_void_p(delta.ptr), C.c_void_p(flag.data_ptr()),
                              _stream(stream)))
    return For32Column(delta, base, n), int(flag.cpu().item()) == 0


def aggregate_for32(enc, mask=0xF, ws=None, stream=None):
    """fq_aggregate_for32 over a For32Column -> host fq_agg_state."""
    require_gpu()
    ws = ws or Workspace(lib.fq_aggregate_workspace_bytes(enc.len))
    out = torch.empty(48, dtype=torch.uint8, device="cuda")
    check(lib.fq_aggregate_for32(C.c_void_p(enc.delta.ptr), C.c_void_p(enc.base.ptr), enc.len, mask,
                                 C.c_void_p(out.data_ptr()), ws.ptr, ws.nbytes, _stream(stream)))
    return state_from_device(out)


def aggregate_for32_expr(enc, block_rows=0, pred=None, value=None, mask=0xF, ws=None, stream=None):
    """fq_aggregate_for32_expr over a For32Column: fq_aggregate over the column it
    stands for, read as 4-byte deltas -> host fq_agg_state."""
    require_gpu()
    ws = ws or Workspace(lib.fq_aggregate_workspace_bytes(enc.len))
    out = torch.empty(48, dtype=torch.uint8, device="cuda")
    check(lib.fq_aggregate_for32_expr(C.c_void_p(enc.delta.ptr), C.c_void_p(enc.base.ptr), enc.len, int(block_rows),
                                      C.byref(pred) if pred is not None else None,
                                      C.byref(value) if value is not None else None, mask,
                                      C.c_void_p(out.data_ptr()), ws.ptr, ws.nbytes, _stream(stream)))
    return state_from_device(out)


def state_values(st):
    """fq_agg_state -> dict(sum, max, min, count, blocks, flags) of Python values;
    fq_agg_state_n: also `valid`, and sum / max / min are None when valid == 0."""
    if isinstance(st, abi.fq_agg_state_n):
        d = state_values(st.s)
        d["valid"] = st.valid
        if st.valid == 0:
            d["sum"] = d["max"] = d["min"] = None
        return d
    dt = st.dtype
    return {
        "sum": from_bits(st.sum, dt), "max": from_bits(st.max, dt),
        "min": from_bits(st.min, dt), "count": st.count, "blocks": st.blocks,
        "flags": st.flags, "dtype": dt,
    }


def _side(x):
    """DeviceColumn -> (fq_col, None); python scalar / (value, dtype) -> (None, fq_value)."""
    if isinstance(x, DeviceColumn):
        return x.col(), None
    if isinstance(x, abi.fq_value):
        return None, x
    from .expr import literal
    val, dt = literal(x)
    if val is None:
        return None, abi.fq_value(dt, 0, 0)
    return None, abi.fq_value(dt, 1, to_bits(val, dt))


def arith(op_sym, lhs, rhs, stream=None):
    """ArithmeticFunction::eval on device columns / scalars -> DeviceColumn."""
    require_gpu()
    lc, ls = _side(lhs)
    rc, rs = _side(rhs)
    ldt = lc.dtype if lc is not None else ls.dtype
    rdt = rc.dtype if rc is not None else rs.dtype
    out_dt = C.c_int32(0)
    check(lib.fq_arith_result_type(abi.OP_BY_SYM[op_sym], ldt, rdt, C.byref(out_dt)))
    n = lc.len if lc is not None else (rc.len if rc is not None else 1)
    out = empty_column(n, out_dt.value)
    oc = out.col()
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    check(lib.fq_arith(abi.OP_BY_SYM[op_sym], C.byref(lc) if lc is not None else None,
                       C.byref(ls) if ls is not None else None, C.byref(rc) if rc is not None else None,
                       C.byref(rs) if rs is not None else None, C.byref(oc),
                       C.c_void_p(flag.data_ptr()), _stream(stream)))
    return out


def compare(cmp_sym, lhs, rhs, stream=None):
    """ComparisonFunction::eval -> Boolean DeviceColumn (LSB-first bitmap)."""
    require_gpu()
    lc, ls = _side(lhs)
    rc, rs = _side(rhs)
    n = lc.len if lc is not None else (rc.len if rc is not None else 1)
    out = empty_column(n, abi.DT_BOOLEAN)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    check(lib.fq_compare(abi.CMP_BY_SYM[cmp_sym], C.byref(lc) if lc is not None else None,
                         C.byref(ls) if ls is not None else None,
                         C.byref(rc) if rc is not None else None,
                         C.byref(rs) if rs is not None else None, C.c_void_p(out.ptr), n,
                         C.c_void_p(flag.data_ptr()), _stream(stream)))
    return out


def logic(op, lhs, rhs, stream=None):
    """LogicFunction::eval: 'and' / 'or' of two Boolean DeviceColumns."""
    require_gpu()
    out = empty_column(lhs.len, abi.DT_BOOLEAN)
    check(lib.fq_logic(0 if op == "and" else 1, C.c_void_p(lhs.ptr), C.c_void_p(rhs.ptr), C.c_void_p(out.ptr),
                       lhs.len, _stream(stream)))
    return out


def filter_compact(col, bitmap, stream=None):
    """FilterTransform: keep rows whose bit is set, in order -> DeviceColumn."""
    require_gpu()
    out = empty_column(col.len, col.dtype)
    ws = Workspace(lib.fq_filter_workspace_bytes(col.len))
    n = C.c_int64(0)
    c = col.col()
    check(lib.fq_filter_compact(C.byref(c), C.c_void_p(bitmap.ptr), C.c_void_p(out.ptr), C.byref(n),
                                ws.ptr, ws.nbytes, _stream(stream)))
    out.len = n.value
    return out


def filter_project(col, pred, values, stream=None):
    """FilterTransform -> ProjectionTransform fused (fq_filter_project): the
    kept rows of `col` (pred None = all) through each fq_expr of `values`
    (None = the column itself) -> [DeviceColumn] in row order."""
    require_gpu()
    n_out = len(values)
    exprs = (abi.fq_expr * n_out)()
    outs = []
    for j, v in enumerate(values):
        if v is None:
            v = abi.fq_expr()
            v.n_steps = 0
            v.out_dtype = col.dtype
        exprs[j] = v
        outs.append(empty_column(col.len, v.out_dtype))
    ptrs = (C.c_void_p * max(n_out, 1))(*[o.ptr for o in outs])
    ws = Workspace(lib.fq_filter_project_workspace_bytes(col.len))
    n = C.c_int64(0)
    c = col.col()
    check(lib.fq_filter_project(C.byref(c), C.byref(pred) if pred is not None else None, exprs, n_out, ptrs,
                                C.byref(n), ws.ptr, ws.nbytes, _stream(stream)))
    for o in outs:
        o.len = n.value
    return outs


def filter_project_blocks(col, block_rows, pred, values, stream=None, out_offset=0):
    """FilterTransform -> ProjectionTransform over a stream of DataBlocks of
    block_rows rows (fq_filter_project_blocks): -> ([DeviceColumn of col.len
    rows per output], per-block kept counts as an int64 numpy array).  Block
    b's kept rows are rows [b * block_rows, + counts[b]) of each output.
    out_offset: each output a view that many 8-byte rows into its buffer
    (tests: outputs not 16-byte aligned)."""
    require_gpu()
    n_out = len(values)
    exprs = (abi.fq_expr * n_out)()
    outs = []
    for j, v in enumerate(values):
        if v is None:
            v = abi.fq_expr()
            v.n_steps = 0
            v.out_dtype = col.dtype
        exprs[j] = v
        if out_offset:
            full = empty_column(col.len + out_offset, v.out_dtype)
            outs.append(DeviceColumn(full.buf, col.len, v.out_dtype, offset=8 * out_offset))
        else:
            outs.append(empty_column(col.len, v.out_dtype))
    ptrs = (C.c_void_p * max(n_out, 1))(*[o.ptr for o in outs])
    nb =(1 if block_rows >= col.len else -(-col.len // block_rows)) if block_rows > 0 and col.len > 0 else 0
    counts = Workspace(max(8 * nb, 8))
    ws = Workspace(lib.fq_filter_project_blocks_workspace_bytes())
    n = C.c_int64(0)
    c = col.col()
    check(lib.fq_filter_project_blocks(C.byref(c), block_rows, C.byref(pred) if pred is not None else None, exprs,
                                       n_out, ptrs, counts.ptr, C.byref(n), ws.ptr, ws.nbytes, _stream(stream)))
    cnt = counts.buf[:8 * nb].view(torch.int64).cpu().numpy() if nb else np.zeros(0, np.int64)
    assert int(cnt.sum()) == n.value
    return outs, cnt


def filter_project_blocks_for32(enc, block_rows, pred, values, first=0, length=None, stream=None, out_offset=0):
    """fq_filter_project_blocks_for32: filter_project_blocks over rows [first,
    first + length) of the UInt64 column a For32Column stands for (length None:
    up to its end), read as 4-byte deltas -> what filter_project_blocks returns
    for the decoded window.  A bitmap predicate's rows are relative to the
    window."""
    require_gpu()
    n = enc.len - int(first) if length is None else int(length)
    n_out = len(values)
    exprs = _project_exprs(values, abi.DT_UINT64)
    outs = []
    for j in range(n_out):
        dt = exprs[j].out_dtype
        if out_offset:
            full = empty_column(max(n, 0) + out_offset, dt)
            outs.append(DeviceColumn(full.buf, max(n, 0), dt, offset=8 * out_offset))
        else:
            outs.append(empty_column(max(n, 0), dt))
    ptrs = (C.c_void_p * max(n_out, 1))(*[o.ptr for o in outs])
    nb = (1 if block_rows >= n else -(-n // block_rows)) if block_rows > 0 and n > 0 else 0
    counts = Workspace(max(8 * nb, 8))
    ws = Workspace(lib.fq_filter_project_blocks_workspace_bytes())
    kept = C.c_int64(0)
    check(lib.fq_filter_project_blocks_for32(C.c_void_p(enc.delta.ptr), C.c_void_p(enc.base.ptr), int(first), n,
                                             int(block_rows), C.byref(pred) if pred is not None else None, exprs, n_out,
                                             ptrs, counts.ptr, C.byref(kept), ws.ptr, ws.nbytes, _stream(stream)))
    cnt = counts.buf[:8 * nb].view(torch.int64).cpu().numpy() if nb else np.zeros(0, np.int64)
    assert int(cnt.sum()) == kept.value
    return outs, cnt


def jit_prepare_project_for32(pred=None, values=(None,), block_rows=10000):
    """Compile fq_filter_project_blocks_for32's kernel for this shape ahead of
    time (works without a GPU: the source is then only compiled for gfx950);
    returns True if the shape has a module."""
    exprs = _project_exprs(values, abi.DT_UINT64)
    out = C.c_int32(0)
    check(lib.fq_jit_prepare_project_for32(int(block_rows), C.byref(pred) if pred is not None else None, exprs,
                                           len(values), C.byref(out)))
    return bool(out.value)


def predicate_bitmap(col, pred, stream=None):
    """FilterTransform's predicate as a Boolean column (fq_predicate_bitmap)."""
    require_gpu()
    out = empty_column(col.len, abi.DT_BOOLEAN)
    flag = Workspace(4)
    c = col.col()
    check(lib.fq_predicate_bitmap(C.byref(c), C.byref(pred), C.c_void_p(out.ptr), flag.ptr, _stream(stream)))
    return out


def _project_exprs(values, dtype0):
    """[fq_expr or None] -> the fq_expr array (None: column 0 itself)."""
    exprs = (abi.fq_expr * max(len(values), 1))()
    for j, v in enumerate(values):
        if v is None:
            v = abi.fq_expr()
            v.n_steps = 0
            v.out_dtype = dtype0
        exprs[j] = v
    return exprs


def filter_project_columns(cols, pred, values, stream=None):
    """fq_filter_project_columns over a list of DeviceColumns of one block
    (expr.chain_columns / predicate_columns number them by position): the kept
    rows (pred None = all) through each fq_expr of `values` (None = column 0
    itself) -> [DeviceColumn] in row order."""
    require_gpu()
    n_out, n = len(values), cols[0].len
    exprs = _project_exprs(values, cols[0].dtype)
    outs = [empty_column(n, exprs[j].out_dtype) for j in range(n_out)]
    ptrs = (C.c_void_p * max(n_out, 1))(*[o.ptr for o in outs])
    ws = Workspace(lib.fq_filter_project_columns_workspace_bytes(n, len(cols)))
    kept = C.c_int64(0)
    arr = (abi.fq_col * max(len(cols), 1))(*[c.col() for c in cols])
    check(lib.fq_filter_project_columns(arr, len(cols), C.byref(pred) if pred is not None else None, exprs, n_out,
                                        ptrs, C.byref(kept), ws.ptr, ws.nbytes, _stream(stream)))
    for o in outs:
        o.len = kept.value
    return outs


def filter_project_blocks_columns(cols, block_rows, pred, values, stream=None, out_offset=0, fill=None):
    """fq_filter_project_blocks_columns: filter_project_blocks over a list of
    DeviceColumns of one block -> ([DeviceColumn of len rows per output],
    per-block kept counts).  out_offset as filter_project_blocks; fill: a
    uint64 the output buffers are set to first (tests: rows past a block's
    count must be left as they were)."""
    require_gpu()
    n_out, n = len(values), cols[0].len
    exprs = _project_exprs(values, cols[0].dtype)
    outs = []
    for j in range(n_out):
        full = empty_column(n + out_offset, exprs[j].out_dtype)
        if fill is not None:
            full.buf.view(torch.int64).fill_(int(np.uint64(fill).astype(np.int64)))
        outs.append(DeviceColumn(full.buf, n, exprs[j].out_dtype, offset=8 * out_offset) if out_offset else full)
    ptrs = (C.c_void_p * max(n_out, 1))(*[o.ptr for o in outs])
    nb = (1 if block_rows >= n else -(-n // block_rows)) if block_rows > 0 and n > 0 else 0
    counts = Workspace(max(8 * nb, 8))
    ws = Workspace(lib.fq_filter_project_blocks_workspace_bytes())
    kept = C.c_int64(0)
    arr = (abi.fq_col * max(len(cols), 1))(*[c.col() for c in cols])
    check(lib.fq_filter_project_blocks_columns(arr, len(cols), block_rows, C.byref(pred) if pred is not None else None,
                                               exprs, n_out, ptrs, counts.ptr, C.byref(kept), ws.ptr, ws.nbytes,
                                               _stream(stream)))
    cnt = counts.buf[:8 * nb].view(torch.int64).cpu().numpy() if nb else np.zeros(0, np.int64)
    return outs, cnt, kept.value


def predicate_bitmap_columns(cols, pred, stream=None):
    """fq_predicate_bitmap_columns: the predicate over a list of DeviceColumns
    as a Boolean column."""
    require_gpu()
    out = empty_column(cols[0].len, abi.DT_BOOLEAN)
    flag = Workspace(4)
    arr = (abi.fq_col * max(len(cols), 1))(*[c.col() for c in cols])
    check(lib.fq_predicate_bitmap_columns(arr, len(cols), C.byref(pred), C.c_void_p(out.ptr), flag.ptr,
                                          _stream(stream)))
    return out


def jit_prepare_project_columns(dtypes, pred=None, values=(None,), block_rows=0, length=1 << 30, lengths=None):
    """Compile the fused projection module of fq_filter_project_columns /
    _blocks_columns / fq_predicate_bitmap_columns for this shape ahead of time
    (works without a GPU: the source is then only compiled for gfx950).  One
    dtype per column; returns True if the shape has a module."""
    lens = list(lengths) if lengths is not None else [int(length)] * len(dtypes)
    arr = (abi.fq_col * max(len(dtypes), 1))(*[abi.fq_col(None, int(n), dt, 0) for dt, n in zip(dtypes, lens)])
    exprs = _project_exprs(values, dtypes[0] if dtypes else 0)
    out = C.c_int32(0)
    check(lib.fq_jit_prepare_project_columns(arr, len(dtypes), int(block_rows),
                                             C.byref(pred) if pred is not None else None, exprs, len(values),
                                             C.byref(out)))
    return bool(out.value)


# ---- the same over columns, steps, comparisons and outputs of any numeric type ----
def filter_project_typed(cols, pred, values, stream=None, out_offset=0):
    """fq_filter_project_typed over a list of DeviceColumns of any numeric
    dtype each: the kept rows (pred None = all) through each fq_expr of
    `values` (None = column 0 itself) -> [DeviceColumn], each of its
    expression's out_dtype at that type's own width.  out_offset: each output a
    view that many of its elements into its buffer."""
    require_gpu()
    n_out, n = len(values), cols[0].len
    exprs = _project_exprs(values, cols[0].dtype)
    outs = []
    for j in range(n_out):
        dt = exprs[j].out_dtype
        full = empty_column(n + out_offset, dt)
        outs.append(DeviceColumn(full.buf, n, dt, offset=ELEM_SIZE[dt] * out_offset) if out_offset else full)
    ptrs = (C.c_void_p * max(n_out, 1))(*[o.ptr for o in outs])
    arr = (abi.fq_col * max(len(cols), 1))(*[c.col() for c in cols])
    ws = Workspace(lib.fq_filter_project_typed_workspace_bytes(n, arr, len(cols)))
    kept = C.c_int64(0)
    check(lib.fq_filter_project_typed(arr, len(cols), C.byref(pred) if pred is not None else None, exprs, n_out,
                                      ptrs, C.byref(kept), ws.ptr, ws.nbytes, _stream(stream)))
    for o in outs:
        o.len = kept.value
    return outs


def filter_project_blocks_typed(cols, block_rows, pred, values, stream=None, out_offset=0, fill=None):
    """fq_filter_project_blocks_typed: filter_project_blocks_columns over
    DeviceColumns of any numeric dtype -> ([DeviceColumn of len rows per
    output, in its out_dtype], per-block kept counts, rows kept).  out_offset:
    each output a view that many of its elements into its buffer; fill: a byte
    value the output buffers are set to first (rows past a block's count must
    be left as they were)."""
    require_gpu()
    n_out, n = len(values), cols[0].len
    exprs = _project_exprs(values, cols[0].dtype)
    outs = []
    for j in range(n_out):
        dt = exprs[j].out_dtype
        full = empty_column(n + out_offset, dt)
        if fill is not None:
            full.buf.fill_(int(fill) & 0xFF)
        outs.append(DeviceColumn(full.buf, n, dt, offset=ELEM_SIZE[dt] * out_offset) if out_offset else full)
    ptrs = (C.c_void_p * max(n_out, 1))(*[o.ptr for o in outs])
    nb = (1 if block_rows >= n else -(-n // block_rows)) if block_rows > 0 and n > 0 else 0
    counts = Workspace(max(8 * nb, 8))
    ws = Workspace(lib.fq_filter_project_blocks_workspace_bytes())
    kept = C.c_int64(0)
    arr = (abi.fq_col * max(len(cols), 1))(*[c.col() for c in cols])
    check(lib.fq_filter_project_blocks_typed(arr, len(cols), block_rows, C.byref(pred) if pred is not None else None,
                                             exprs, n_out, ptrs, counts.ptr, C.byref(kept), ws.ptr, ws.nbytes,
                                             _stream(stream)))
    cnt = counts.buf[:8 * nb].view(torch.int64).cpu().numpy() if nb else np.zeros(0, np.int64)
    return outs, cnt, kept.value


def predicate_bitmap_typed(cols, pred, stream=None):
    """fq_predicate_bitmap_typed: the predicate over DeviceColumns of any
    numeric dtype as a Boolean column."""
    require_gpu()
    out = empty_column(cols[0].len, abi.DT_BOOLEAN)
    flag = Workspace(4)
    arr = (abi.fq_col * max(len(cols), 1))(*[c.col() for c in cols])
    check(lib.fq_predicate_bitmap_typed(arr, len(cols), C.byref(pred), C.c_void_p(out.ptr), flag.ptr, _stream(stream)))
    return out


def jit_prepare_project_typed(dtypes, pred=None, values=(None,), block_rows=0, length=1 << 30, lengths=None):
    """jit_prepare_project_columns for the *_typed entry points: one dtype (any
    numeric) per column; works without a GPU."""
    lens = list(lengths) if lengths is not None else [int(length)] * len(dtypes)
    arr = (abi.fq_col * max(len(dtypes), 1))(*[abi.fq_col(None, int(n), dt, 0) for dt, n in zip(dtypes, lens)])
    exprs = _project_exprs(values, dtypes[0] if dtypes else 0)
    out = C.c_int32(0)
    check(lib.fq_jit_prepare_project_typed(arr, len(dtypes), int(block_rows),
                                           C.byref(pred) if pred is not None else None, exprs, len(values),
                                           C.byref(out)))
    return bool(out.value)


# ---- the block stream over nullable columns (Arrow validity bitmaps) ----
def _validity_array(validity, n_cols):
    """[None | DeviceColumn | pointer] per column -> the `validity` argument (None: a NULL array)."""
    if validity is None:
        return None
    return (C.c_void_p * max(n_cols, 1))(*[getattr(v, "ptr", v) for v in validity])


def filter_project_blocks_nullable(cols, validity, block_rows, pred, values, out_offset=0, fill=None, stream=None,
                                   out_validity=None):
    """fq_filter_project_blocks_nullable: filter_project_blocks_typed over
    nullable columns.  validity: per column None or a UInt64 DeviceColumn of
    ceil(len / 64) Arrow validity-bitmap words (bit i = row i of the column is
    valid).  Returns ([DeviceColumn of len rows per output], [UInt64
    DeviceColumn of ceil(len / 64) + 1 words per output: bit p = row p of the
    output, then one sentinel word], per-block kept counts, rows kept).
    out_offset: each output a view that many of its elements into its buffer
    (its bitmap's bit 0 stays its row 0).  fill: a byte value the output buffers AND
    their bitmaps are set to first (rows past a count keep it; the bitmap's words
    are zeroed by the call, the sentinel word after them keeps it).
    out_validity: per output None to pass a NULL bitmap (allowed only for an
    output that cannot hold a null)."""
    require_gpu()
    n_out, n = len(values), cols[0].len
    exprs = _project_exprs(values, cols[0].dtype)
    outs, outv = [], []
    for j in range(n_out):
        dt = exprs[j].out_dtype
        full = empty_column(n + out_offset, dt)
        fullv = empty_column((n + 63) // 64 + 1, abi.DT_UINT64)
        if fill is not None:
            full.buf.fill_(int(fill) & 0xFF)
            fullv.buf.fill_(int(fill) & 0xFF)
        outs.append(DeviceColumn(full.buf, n, dt, offset=ELEM_SIZE[dt] * out_offset) if out_offset else full)
        outv.append(fullv)
    ptrs = (C.c_void_p * max(n_out, 1))(*[o.ptr for o in outs])
    vptrs = (C.c_void_p * max(n_out, 1))(*[None if out_validity is not None and out_validity[j] is None else outv[j].ptr
                                           for j in range(n_out)])
    nb = (1 if block_rows >= n else -(-n // block_rows)) if block_rows > 0 and n > 0 else 0
    counts = Workspace(max(8 * nb, 8))
    ws = Workspace(lib.fq_filter_project_blocks_workspace_bytes())
    kept = C.c_int64(0)
    arr = (abi.fq_col * max(len(cols), 1))(*[c.col() for c in cols])
    check(lib.fq_filter_project_blocks_nullable(arr, _validity_array(validity, len(cols)), len(cols), block_rows,
                                                C.byref(pred) if pred is not None else None, exprs, n_out, ptrs, vptrs,
                                                counts.ptr, C.byref(kept), ws.ptr, ws.nbytes, _stream(stream)))
    cnt = counts.buf[:8 * nb].view(torch.int64).cpu().numpy() if nb else np.zeros(0, np.int64)
    return outs, outv, cnt, kept.value


def predicate_bitmap_nullable(cols, validity, pred, stream=None):
    """fq_predicate_bitmap_nullable: bit i = the predicate over row i of the
    nullable columns is valid and true, as a Boolean column."""
    require_gpu()
    out = empty_column(cols[0].len, abi.DT_BOOLEAN)
    flag = Workspace(4)
    arr = (abi.fq_col * max(len(cols), 1))(*[c.col() for c in cols])
    check(lib.fq_predicate_bitmap_nullable(arr, _validity_array(validity, len(cols)), len(cols), C.byref(pred),
                                           C.c_void_p(out.ptr), flag.ptr, _stream(stream)))
    return out


def jit_prepare_project_nullable(dtypes, has_validity=None, pred=None, values=(None,), block_rows=10000,
                                 length=1 << 30, lengths=None):
    """jit_prepare_project_typed for the *_nullable entry points (block-stream
    geometry only): one dtype per column, and whether it will carry a validity
    bitmap (default: none does); works without a GPU."""
    lens = list(lengths) if lengths is not None else [int(length)] * len(dtypes)
    arr = (abi.fq_col * max(len(dtypes), 1))(*[abi.fq_col(None, int(n), dt, 0) for dt, n in zip(dtypes, lens)])
    hv = None
    if has_validity is not None:
        hv = (C.c_uint8 * max(len(dtypes), 1))(*[1 if h else 0 for h in has_validity])
    exprs = _project_exprs(values, dtypes[0] if dtypes else 0)
    out = C.c_int32(0)
    check(lib.fq_jit_prepare_project_nullable(arr, hv, len(dtypes), int(block_rows),
                                              C.byref(pred) if pred is not None else None, exprs, len(values),
                                              C.byref(out)))
    return bool(out.value)


def project_compile_check(col_dtype, pred=None, values=(None,)):
    """Generate + compile the fused projection module for this shape without
    running it (no GPU needed: gfx950 code object only).  Returns the
    fq_status of fq_filter_project on a fake column (FQ_E_HIP when there is no
    device after a successful compile)."""
    exprs = (abi.fq_expr * len(values))()
    for j, v in enumerate(values):
        if v is None:
            v = abi.fq_expr()
            v.out_dtype = col_dtype
        exprs[j] = v
    fake = (C.c_void_p * len(values))(*([C.c_void_p(256)] * len(values)))
    c = abi.fq_col(C.c_void_p(256), 1 << 20, col_dtype, 0)
    n = C.c_int64(0)
    return lib.fq_filter_project(C.byref(c), C.byref(pred) if pred is not None else None, exprs, len(values), fake,
                                 C.byref(n), C.c_void_p(256), lib.fq_filter_project_workspace_bytes(1 << 20), None)


def state_merge(states):
    arr = (abi.fq_agg_state * len(states))(*states)
    out = abi.fq_agg_state()
    check(lib.fq_state_merge(arr, len(states), C.byref(out)))
    return out


# ---- expression specialisation (include/fq_gpu.h fq_jit_*) ----
def jit_config(mode, min_rows=1 << 22):
    """Process-wide JIT policy: abi.JIT_OFF / JIT_AUTO / JIT_ALWAYS."""
    check(lib.fq_jit_config(mode, int(min_rows)))


def jit_stats():
    st = abi.fq_jit_stats()
    check(lib.fq_jit_get_stats(C.byref(st)))
    return {f: getattr(st, f) for f, _ in abi.fq_jit_stats._fields_}


def jit_prepare(dtype, pred=None, value=None, mask=abi.AGG_SUM, block_rows=0, length=1 << 30):
    """Compile the specialised scan for this shape ahead of time (works
    without a GPU: the source is then only compiled for gfx950).  Returns
    True if the shape has a specialised kernel."""
    c = abi.fq_col(None, int(length), dtype, 0)
    out = C.c_int32(0)
    check(lib.fq_jit_prepare(C.byref(c), int(block_rows), C.byref(pred) if pred is not None else None,
                             C.byref(value) if value is not None else None, mask, C.byref(out)))
    return bool(out.value)


def jit_prepare_for32(pred=None, value=None, mask=abi.AGG_SUM, block_rows=0, length=1 << 30):
    """jit_prepare for fq_aggregate_for32_expr (a UInt64 column as 32-bit deltas).
    False for the call without predicate and expression: its kernel is precompiled."""
    out = C.c_int32(0)
    check(lib.fq_jit_prepare_for32(int(length), int(block_rows), C.byref(pred) if pred is not None else None,
                                   C.byref(value) if value is not None else None, mask, C.byref(out)))
    return bool(out.value)


def jit_prepare_columns(dtypes, pred=None, value=None, mask=abi.AGG_SUM, block_rows=0, length=1 << 30, lengths=None):
    """jit_prepare for fq_aggregate_columns: one dtype per column (`lengths`:
    one length per column, default `length` for all)."""
    lens = list(lengths) if lengths is not None else [int(length)] * len(dtypes)
    arr = (abi.fq_col * max(len(dtypes), 1))(*[abi.fq_col(None, int(n), dt, 0) for dt, n in zip(dtypes, lens)])
    out = C.c_int32(0)
    check(lib.fq_jit_prepare_columns(arr, len(dtypes), int(block_rows), C.byref(pred) if pred is not None else None,
                                     C.byref(value) if value is not None else None, mask, C.byref(out)))
    return bool(out.value)


def jit_prepare_typed(dtypes, pred=None, value=None, mask=abi.AGG_SUM, block_rows=0, length=1 << 30, lengths=None):
    """jit_prepare for fq_aggregate_typed: one dtype (any numeric) per column."""
    lens = list(lengths) if lengths is not None else [int(length)] * len(dtypes)
    arr = (abi.fq_col * max(len(dtypes), 1))(*[abi.fq_col(None, int(n), dt, 0) for dt, n in zip(dtypes, lens)])
    out = C.c_int32(0)
    check(lib.fq_jit_prepare_typed(arr, len(dtypes), int(block_rows), C.byref(pred) if pred is not None else None,
                                   C.byref(value) if value is not None else None, mask, C.byref(out)))
    return bool(out.value)


def jit_prepare_nullable(dtypes, has_validity=None, pred=None, value=None, mask=abi.AGG_SUM, block_rows=0,
                         length=1 << 30, lengths=None):
    """jit_prepare for fq_aggregate_nullable: one dtype per column, and whether it
    will carry a validity bitmap (default: none does)."""
    lens = list(lengths) if lengths is not None else [int(length)] * len(dtypes)
    arr = (abi.fq_col * max(len(dtypes), 1))(*[abi.fq_col(None, int(n), dt, 0) for dt, n in zip(dtypes, lens)])
    hv = None
    if has_validity is not None:
        hv = (C.c_uint8 * max(len(dtypes), 1))(*[1 if h else 0 for h in has_validity])
    out = C.c_int32(0)
    check(lib.fq_jit_prepare_nullable(arr, hv, len(dtypes), int(block_rows),
                                      C.byref(pred) if pred is not None else None,
                                      C.byref(value) if value is not None else None, mask, C.byref(out)))
    return bool(out.value)


# ---- GROUP BY hash aggregation (include/fq_gpu.h fq_group_*) ----
class GroupTable:
    """A device hash table of groups: key -> one 64-bit state per aggregate.
    aggs: [(abi.AGG_*, state dtype)]; Count's state dtype is UInt64."""

    def __init__(self, capacity, aggs, key_dtype=abi.DT_UINT64, stream=None):
        require_gpu()
        cap = 64
        while cap < capacity:
            cap *= 2
        self.desc = abi.fq_group_table()
        self.desc.capacity = cap
        self.desc.key_dtype = key_dtype
        self.desc.n_aggs = len(aggs)
        for i, (k, dt) in enumerate(aggs):
            self.desc.kinds[i] = k
            self.desc.dtypes[i] = dt
        self.buf = torch.empty(lib.fq_group_table_bytes(cap, len(aggs)), dtype=torch.uint8, device="cuda")
        self.desc.d_mem = self.buf.data_ptr()
        self.aggs = list(aggs)
        check(lib.fq_group_table_init(C.byref(self.desc), _stream(stream)))

    def aggregate(self, col, pred=None, key=None, values=None, stream=None, log2_parts=0, narrow=False):
        """fq_group_aggregate, or with log2_parts > 0 the radix-partitioned
        fq_group_aggregate_partitioned (2^log2_parts bins; narrow: the caller
        vouches every value v has col[0] - 2^31 <= v <= col[0] + 2^31 - 1, FQ_GROUP_NARROW_ROWS)."""
        c = col.col()
        vals = (abi.fq_expr * abi.MAX_GROUP_AGGS)()
        for i, v in enumerate(values or []):
            if v is not None:
                vals[i] = v
        p = C.byref(pred) if pred is not None else None
        k = C.byref(key) if key is not None else None
        if not log2_parts:
            check(lib.fq_group_aggregate(C.byref(self.desc), C.byref(c), p, k, vals, _stream(stream)))
            return
        ws = Workspace(lib.fq_group_partition_workspace_bytes(col.len, log2_parts))
        lp = log2_parts | (abi.GROUP_NARROW_ROWS if narrow else 0)
        check(lib.fq_group_aggregate_partitioned(C.byref(self.desc), C.byref(c), p, k, vals, lp, ws.ptr,
                                                 ws.nbytes, _stream(stream)))
        self._ws = ws  # alive until the next call (the launch is asynchronous)

    def aggregate_columns(self, cols, pred=None, key=None, values=None, stream=None):
        """fq_group_aggregate_columns over a list of DeviceColumns of one block
        (expr.chain_columns / predicate_columns / pred_tree_columns number them
        by position; key None = column 0, values[i] None = column 0)."""
        arr = (abi.fq_col * max(len(cols), 1))(*[c.col() for c in cols])
        vals = (abi.fq_expr * abi.MAX_GROUP_AGGS)()
        for i, v in enumerate(values or []):
            if v is not None:
                vals[i] = v
        p = C.byref(pred) if pred is not None else None
        k = C.byref(key) if key is not None else None
        check(lib.fq_group_aggregate_columns(C.byref(self.desc), arr, len(cols), p, k, vals, _stream(stream)))

    def merge(self, keys, states, stream=None):
        """fq_group_table_merge: host uint64 keys[n] and per-aggregate uint64
        states[n] (state bits) folded into this table."""
        n = len(keys)
        dk = torch.from_numpy(np.ascontiguousarray(keys, dtype=np.uint64).view(np.int64)).cuda()
        ds = [torch.from_numpy(np.ascontiguousarray(s, dtype=np.uint64).view(np.int64)).cuda() for s in states]
        ptrs = (C.c_void_p * max(len(ds), 1))(*[t.data_ptr() for t in ds])
        check(lib.fq_group_table_merge(C.byref(self.desc), C.c_void_p(dk.data_ptr()), ptrs, n, _stream(stream)))
        torch.cuda.synchronize()

    def count(self, stream=None):
        n = C.c_int64(0)
        check(lib.fq_group_table_count(C.byref(self.desc), C.byref(n), _stream(stream)))
        return n.value

    def extract(self, stream=None):
        """-> (keys uint64[g], [states uint64[g] per aggregate]) in slot order."""
        g = self.count(stream)
        n = max(g, 1)
        keys = torch.empty(n, dtype=torch.int64, device="cuda")
        sts = [torch.empty(n, dtype=torch.int64, device="cuda") for _ in self.aggs]
        ptrs = (C.c_void_p * len(sts))(*[t.data_ptr() for t in sts])
        out = C.c_int64(0)
        check(lib.fq_group_table_extract(C.byref(self.desc), C.c_void_p(keys.data_ptr()), ptrs, n, C.byref(out),
                                         _stream(stream)))
        k = keys[: out.value].cpu().numpy().view(np.uint64)
        return k, [t[: out.value].cpu().numpy().view(np.uint64) for t in sts]


def group_compile_check(col_dtype, aggs, key=None, values=None, pred=None, key_dtype=abi.DT_UINT64, log2_parts=0):
    """Generate + compile the group-by kernel for a shape (no GPU needed: a
    zero-length call compiles the source for gfx950 without loading it);
    log2_parts > 0 through fq_group_aggregate_partitioned (range bins for a
    `% d` key, else hash bins)."""
    d = abi.fq_group_table()
    d.d_mem = 0x1000  # never dereferenced for a zero-length column
    d.capacity = 64
    d.key_dtype = key_dtype
    d.n_aggs = len(aggs)
    for i, (k, dt) in enumerate(aggs):
        d.kinds[i] = k
        d.dtypes[i] = dt
    c = abi.fq_col(None, 0, col_dtype, 0)
    vals = (abi.fq_expr * abi.MAX_GROUP_AGGS)()
    for i, v in enumerate(values or []):
        if v is not None:
            vals[i] = v
    p = C.byref(pred) if pred is not None else None
    k = C.byref(key) if key is not None else None
    if log2_parts:
        check(lib.fq_group_aggregate_partitioned(C.byref(d), C.byref(c), p, k, vals, log2_parts, None, 0, None))
    else:
        check(lib.fq_group_aggregate(C.byref(d), C.byref(c), p, k, vals, None))


def group_dense_keys(col_dtype, key, n_aggs):
    """fq_group_dense_keys: d when the key over a column of col_dtype ends in `% d` and d fits the GROUP BY
    kernel's LDS table for n_aggs states (the table is then indexed by the key itself), else 0."""
    return int(lib.fq_group_dense_keys(col_dtype, C.byref(key) if key is not None else None, n_aggs))


def group_compile_check_columns(col_dtypes, aggs, key=None, values=None, pred=None, key_dtype=abi.DT_UINT64,
                                lengths=None, ptrs=None):
    """group_compile_check for fq_group_aggregate_columns: a zero-length call
    over columns of col_dtypes generates and compiles the shape's kernel for
    gfx950 (no GPU needed).  lengths / ptrs: per-column len and data address,
    for the argument checks (nothing is read)."""
    d = abi.fq_group_table()
    d.d_mem = 0x1000  # never dereferenced for a zero-length column
    d.capacity = 64
    d.key_dtype = key_dtype
    d.n_aggs = len(aggs)
    for i, (k, dt) in enumerate(aggs):
        d.kinds[i] = k
        d.dtypes[i] = dt
    lens = list(lengths) if lengths is not None else [0] * len(col_dtypes)
    addr = list(ptrs) if ptrs is not None else [None] * len(col_dtypes)
    arr = (abi.fq_col * max(len(col_dtypes), 1))(*[abi.fq_col(a, int(n), dt, 0)
                                                   for a, n, dt in zip(addr, lens, col_dtypes)])
    vals = (abi.fq_expr * abi.MAX_GROUP_AGGS)()
    for i, v in enumerate(values or []):
        if v is not None:
            vals[i] = v
    p = C.byref(pred) if pred is not None else None
    k = C.byref(key) if key is not None else None
    check(lib.fq_group_aggregate_columns(C.byref(d), arr, len(col_dtypes), p, k, vals, None))


def group_dense_keys_columns(col_dtypes, key, n_aggs):
    """fq_group_dense_keys_columns: group_dense_keys for a key over columns of col_dtypes."""
    arr = (C.c_int32 * max(len(col_dtypes), 1))(*col_dtypes)
    return int(lib.fq_group_dense_keys_columns(arr, len(col_dtypes), C.byref(key) if key is not None else None,
                                               n_aggs))


def tune_set(name, value):
    """fq_tune_set by knob name (abi.TUNE); tuning tools only."""
    check(lib.fq_tune_set(abi.TUNE[name], int(value)))


def tune_get(name):
    return int(lib.fq_tune_get(abi.TUNE[name]))


def tune_reset():
    check(lib.fq_tune_reset())


