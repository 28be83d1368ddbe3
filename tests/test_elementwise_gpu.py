"""GPU: the unfused element-wise path -- fq_arith, fq_compare, fq_logic and
fq_filter_compact -- against oracle/fq_ref.py and numpy masks, on the inputs
of tests/elementwise_cases.py (tests/test_elementwise_cpu.py checks those
inputs and the oracle without a GPU).

fq_arith / fq_compare: all 10 x 10 type pairs, every operator, column o column,
column o scalar, scalar o column (the reference's flipped comparison) and
scalar o scalar, on values every cast holds (`fit`), on each type's limits
(`edge`, and `edge-clipped` where `edge` meets arrow's nulls), at 257 and 4,099
rows and at every SMALL length; columns at element offsets 0 and 1 of a
256-byte aligned buffer (8 mod 16 for 64-bit types: the generic kernels).
Stride cases put rows in the grid-stride loop's third, ragged round
(launch_shapes.ew_arith_generic / ew_compare_generic, sized from the device's
CU count).  Results are bit for bit: integers exact, floats by bit pattern with
any NaN equal to any NaN and the sign of zero kept; every result is one IEEE
operation or an exact fmod, so there is no tolerance.  A Boolean result is
read as bitmap words: bits past len are 0.

Errors: exact texts and statuses of the `zero` and `null-then-zero` classes
(a row whose cast is null raises no Divide by zero, as arrow's divide checks
valid rows only).  Not run here: the same class through fq_aggregate_typed and
fq_filter_project_typed, whose generated kernels still raise Divide by zero for
(a) -- Int8 / UInt64 columns, one '/' step: flags DIV_ZERO | CAST_NULL where the
oracle has CAST_NULL (profiles/r17_elementwise.json).

fq_logic and fq_filter_compact take bitmaps built on the host: clean and dirty
tails (every bit past len set), pointers at 0 and 8 mod 16, every element
width, and nothing written outside [0, out_len)."""
import ctypes as C

import numpy as np
import pytest

import elementwise_cases as E
import fq_ref as R
from fq_amd import abi
from fq_amd._lib import FQError

pytestmark = pytest.mark.gpu

DT = abi.DT_BY_NAME
FILL = 0xA5
ops = None
torch = None


def setup_module():
    global ops, torch
    from fq_amd import ops as _ops
    _ops.require_gpu()
    import torch as _torch
    ops, torch = _ops, _torch
    E.assert_edge_split()


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---------------------------------------------------------------------------
# running a case
# ---------------------------------------------------------------------------
def numpy_dev(arr, dt, off):
    """the rows of arr starting `off` elements into a 256-byte aligned buffer"""
    pad = np.zeros(off + len(arr), dtype=arr.dtype)
    pad[off:] = arr
    c = ops.from_numpy(pad, dt)
    assert c.ptr % 256 == 0
    return ops.DeviceColumn(c.buf, len(arr), dt, offset=arr.dtype.itemsize * off)


def arg(side):
    if side.kind == "col":
        return numpy_dev(side.data, DT[side.type], side.off)
    if side.data is None:
        return abi.fq_value(DT[side.type], 0, 0)
    return (side.data, side.type)


def words_of(col):
    """the bitmap words of a Boolean DeviceColumn as the kernel wrote them"""
    nw = (col.len + 63) // 64
    return col.buf[:8 * nw].cpu().numpy().view(np.uint64).copy() if nw else np.zeros(0, np.uint64)


def run(c):
    """("values", result) or ("error", status, text)"""
    try:
        if c.fn == "arith":
            out = ops.arith(c.op, arg(c.left), arg(c.right))
            return ("values", out.dtype, out.to_numpy())
        return ("values", abi.DT_BOOLEAN, words_of(ops.compare(c.op, arg(c.left), arg(c.right))))
    except FQError as e:
        return ("error", e.status, str(e))


STATUS = {"cast-null": abi.FQ_E_UNSUPPORTED, "scalar-null": abi.FQ_E_UNSUPPORTED, "div-zero": abi.FQ_E_DIVIDE_BY_ZERO,
          "error": abi.FQ_E_INTERNAL}


def check(c):
    what = (c.fn, c.left.type, c.op, c.right.type, c.form, c.cls, c.n)
    got = run(c)
    if c.exp.kind != "values":
        assert got == ("error", STATUS[c.exp.kind], c.exp.data), what + (got[:3],)
        return
    assert got[0] == "values", what + got
    if c.fn == "arith":
        ct = DT[E.coercion(c.left.type, c.right.type)]
        rt = C.c_int32(0)
        ops.check(ops.lib.fq_arith_result_type(abi.OP_BY_SYM[c.op], DT[c.left.type], DT[c.right.type], C.byref(rt)))
        assert got[1] == ct == rt.value, what
        if not E.same_bits(got[2], c.exp.data):
            bad = np.flatnonzero(~((got[2] == c.exp.data) | ((got[2] != got[2]) & (c.exp.data != c.exp.data))))[:5]
            raise AssertionError(what + (bad, got[2][bad], c.exp.data[bad]))
        return
    want = E.pack(c.exp.data)  # bits past len are 0
    if not np.array_equal(got[2], want):
        bad = np.flatnonzero(got[2] != want)[:5]
        raise AssertionError(what + (bad, got[2][bad], want[bad]))
    if c.n & 63:
        assert int(got[2][-1]) >> (c.n & 63) == 0, what


PAIR_IDS = ["%s-%s" % p for p in E.PAIRS]


@pytest.mark.parametrize("lt,rt", E.PAIRS, ids=PAIR_IDS)
def test_arith_every_operator_form_and_class(lt, rt):
    cases = E.pair_cases("arith", lt, rt)
    for c in cases:
        if c.cls in ("fit", "edge-clipped") or (lt, rt) not in E.NULL_PAIRS:
            assert c.exp.kind == "values", (lt, rt, c.op, c.form, c.cls)
        check(c)


@pytest.mark.parametrize("lt,rt", E.PAIRS, ids=PAIR_IDS)
def test_compare_every_operator_form_and_class(lt, rt):
    cases = E.pair_cases("compare", lt, rt)
    for c in cases:
        if c.cls in ("fit", "edge-clipped") or (lt, rt) not in E.NULL_PAIRS:
            assert c.exp.kind == "values", (lt, rt, c.op, c.form, c.cls)
        check(c)


# ---------------------------------------------------------------------------
# the grid-stride loop's later rounds
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ct", E.TYPES)
def test_stride_rounds_of_every_coercion_type(ct):
    for c in E.stride_cases(cus(), ct):
        check(c)


def test_stride_rounds_of_64_bit_same_type_columns_off_the_16_byte_boundary():
    for c in E.stride_same_type_cases(cus()):
        assert c.exp.kind == "values"
        check(c)


# ---------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ct", E.TYPES)
def test_zero_divisor_at_the_first_a_middle_and_the_last_row(ct):
    for c in E.zero_cases(ct):
        check(c)


@pytest.mark.parametrize("ct", E.SECOND_ROUND_ZERO)
def test_zero_divisor_in_the_second_stride_round(ct):
    for c in E.second_round_zero_cases(cus(), ct):
        check(c)


@pytest.mark.parametrize("lt,rt", E.NULL_THEN_ZERO_PAIRS, ids=["%s-%s" % p for p in E.NULL_THEN_ZERO_PAIRS])
def test_a_null_row_raises_no_divide_by_zero(lt, rt):
    """(a) the out-of-range divisor truncates to 0 in the coercion type: a cast null, never Divide by zero;
    (b) with a genuine zero divisor in a valid row: Divide by zero, as in the reference"""
    cases = [c for c in E.null_then_zero_cases() if (c.left.type, c.right.type) == (lt, rt)]
    assert len(cases) == 8
    for c in cases:
        check(c)


def test_none_scalars_answer_the_reference_text():
    for c in E.none_scalar_cases():
        check(c)


# ---------------------------------------------------------------------------
# fq_logic
# ---------------------------------------------------------------------------
def dev_words(words, off, extra=2, fill=None):
    """(tensor, pointer): the words `off` words past a 256-byte boundary, `extra` words of room after them"""
    host = np.full(off + len(words) + extra, 0 if fill is None else fill, dtype=np.uint64)
    host[off:off + len(words)] = words
    t = torch.from_numpy(host.view(np.int64).copy()).to("cuda")
    assert t.data_ptr() % 256 == 0
    return t, t.data_ptr() + 8 * off


def run_logic(n, placement, dirty, seed):
    lo, ro, oo = placement
    l, r = E.logic_bits(n, seed)
    nw = (n + 63) // 64
    lt_, lp = dev_words(E.pack(l, dirty), lo)
    rt_, rp = dev_words(E.pack(r, dirty), ro)
    sentinel = np.uint64(0xA5A5A5A5A5A5A5A5)
    for op, want in (("and", l & r), ("or", l | r)):
        ot, op_ptr = dev_words(np.full(nw, sentinel, np.uint64), oo, fill=sentinel)
        ops.check(ops.lib.fq_logic(0 if op == "and" else 1, C.c_void_p(lp), C.c_void_p(rp), C.c_void_p(op_ptr), n, None))
        torch.cuda.synchronize()
        got = ot.cpu().numpy().view(np.uint64)
        assert np.array_equal(got[oo:oo + nw], E.pack(want)), (n, placement, dirty, op)  # the tail is clear
        assert np.all(got[:oo] == sentinel) and np.all(got[oo + nw:] == sentinel), (n, placement, dirty, op)
        assert np.array_equal(got[oo:oo + nw], E.model_logic(op, E.pack(l, dirty), E.pack(r, dirty), n))


@pytest.mark.parametrize("dirty", [False, True], ids=["clean", "dirty"])
@pytest.mark.parametrize("placement", E.LOGIC_PLACEMENTS, ids=["aligned", "lhs8", "rhs8", "out8"])
def test_logic_tail_is_clear_at_every_placement(placement, dirty):
    for n in E.LOGIC_LENGTHS + [128 * 3 + 5, 128 * 3 + 64 + 5]:  # even and odd word counts with a partial last word
        run_logic(n, placement, dirty, n)


@pytest.mark.parametrize("placement", [E.LOGIC_PLACEMENTS[0], E.LOGIC_PLACEMENTS[3]], ids=["aligned", "out8"])
def test_logic_past_its_grid_cap(placement):
    run_logic(E.logic_stride_bits(cus()), placement, True, 5)


# ---------------------------------------------------------------------------
# fq_filter_compact
# ---------------------------------------------------------------------------
_COLS = {}


def compact_input(t, n):
    if (t, n) not in _COLS:
        _COLS[t, n] = E.compact_column(t, n, n)
    return _COLS[t, n]


@pytest.mark.parametrize("t", E.COMPACT_TYPES)
def test_compact_every_width_placement_and_tail(t):
    esz = E.width(t)
    for n, sel, dirty, bm_off, in_off, out_off in E.compact_runs(t):
        what = (t, n, sel, dirty, bm_off, in_off, out_off)
        x = compact_input(t, n)
        keep = E.compact_keep(n, sel, n + len(sel))
        want = x[keep]
        X = numpy_dev(x, DT[t], in_off)
        bt, bp = dev_words(E.pack(keep, dirty), bm_off)
        room = 256 + esz * (out_off + n + 1)
        out = torch.full((room + 64,), FILL, dtype=torch.uint8, device="cuda")
        assert out.data_ptr() % 256 == 0
        first = 256 + esz * out_off
        ws = ops.Workspace(ops.lib.fq_filter_workspace_bytes(n))
        kept = C.c_int64(-1)
        c = X.col()
        ops.check(ops.lib.fq_filter_compact(C.byref(c), C.c_void_p(bp), C.c_void_p(out.data_ptr() + first),
                                            C.byref(kept), ws.ptr, ws.nbytes, None))
        assert kept.value == int(keep.sum()), what + (kept.value,)
        raw = out.cpu().numpy()
        got = raw[first:first + esz * kept.value].view(R.NP[t])
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), what  # the rows' bytes, NaN payloads included
        # nothing outside [0, out_len) is written
        assert np.all(raw[:first] == FILL) and np.all(raw[first + esz * kept.value:] == FILL), what
