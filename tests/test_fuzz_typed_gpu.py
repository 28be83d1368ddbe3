"""GPU: random programs over typed and nullable columns (tests/fuzz_typed.py)
through ops.aggregate_typed, ops.aggregate_nullable and ops.filter_project_typed
/ filter_project_blocks_typed / predicate_bitmap_typed, against the per-block
oracles of the three shape tests: ref_scan / check of
tests/test_scan_typed_gpu.py and tests/test_scan_nullable_gpu.py, Case.oracle /
same of tests/test_project_typed_gpu.py.  One test per family and seed; each
runs the seed's one program at two flat sizes and one block-mode size
(tests/test_fuzz_typed_cpu.py shows, without a GPU, that the seeds cover the
generator's types, operators and shapes and would catch six kinds of mistake).
FQ_FUZZ_SCALE=k runs k times the seeds, as in tests/test_fuzz_gpu.py.

Integers, counts, dtypes, FQ_STATE_ANY_EMPTY and the error flags are compared
exactly; when the reference expects an error the device must report the same
one and nothing else is compared.  Float max / min by value; Float64 sums
within 1e-12 * sum(|x|) over the valid kept finite values; Float32 sums bit-equal
when every value of the reference's argument is an integer and n * max|v| <
2^24 (every partial sum exact in any order), else within 2 (n - 1) 2^-24
sum(|x|) (tests/test_scan_typed_gpu.py).  Projection outputs bit for bit with
NaN equal to NaN, with the per-block counts, the fill bytes past each count and
the bitmap's cleared tail bits.  An agg state is read twice, byte-identical."""
import os

import numpy as np
import pytest

import fq_ref as R
import fuzz_typed as F
from fq_amd import abi
from fq_amd._lib import FQError

pytestmark = pytest.mark.gpu

SCALE = max(1, int(os.environ.get("FQ_FUZZ_SCALE", "1")))
SEEDS = range(48 * SCALE)
TA, TN, TP = F.TA, F.TN, F.TP
F32 = abi.DT_FLOAT32
ops = None


def setup_module():
    global ops
    for m in (TA, TN, TP):
        m.setup_module()
    ops = TA.ops


def dev_cols(P, run):
    return [TA.numpy_dev(h, dt, off) for h, dt, off in zip(run.host, P.adts, run.offsets)]


def keep_dev(keep):
    """a predicate bitmap: bit i = keep[i]"""
    bits = np.zeros(((len(keep) + 63) // 64) * 64, bool)
    bits[:len(keep)] = keep
    return ops.from_numpy(np.packbits(bits, bitorder="little").view(np.uint64), abi.DT_UINT64)


def with_bitmap(P, run, pred):
    """the device predicate of a run; the second value keeps a bitmap's buffer alive"""
    if P.kind != "bitmap":
        return pred, None
    kb = keep_dev(run.keep)
    pred.bitmap = kb.ptr
    return pred, kb


def f32_sum_rule(P, run, exp):
    """("exact" | "bound", n) for a Float32 sum, from the reference's argument values"""
    vals = F.argument_values(P, run)
    if vals is None or len(vals) == 0:
        return "exact", 0
    v = vals.astype(np.float64)
    exact = bool(np.all(np.isfinite(v)) and np.all(v == np.floor(v)) and len(v) * float(np.abs(v).max()) < 2.0 ** 24)
    return ("exact" if exact else "bound"), len(v)


@pytest.mark.parametrize("seed", SEEDS)
def test_agg(seed):
    P, runs = F.generate("agg", seed)
    pred, value = P.device()
    for run in runs:
        what = "%s | %s" % (P.describe(), run.describe())
        exp = F.expected(P, run)
        pr, _alive = with_bitmap(P, run, pred)
        cols = dev_cols(P, run)
        st = ops.aggregate_typed(cols, run.br, pr, value, P.mask)
        again = ops.aggregate_typed(cols, run.br, pr, value, P.mask)
        assert bytes(again) == bytes(st), what
        rule, n = ("exact", 0)
        if exp["dtype"] == F32 and P.mask & abi.AGG_SUM and not exp["flags"] & F.ERR:
            rule, n = f32_sum_rule(P, run, exp)
        TA.check(st, exp, P.mask, what, f32_sum=rule, n=n)


@pytest.mark.parametrize("seed", SEEDS)
def test_null(seed):
    P, runs = F.generate("null", seed)
    pred, value = P.device()
    for run in runs:
        what = "%s | %s" % (P.describe(), run.describe())
        exp = F.expected(P, run)
        pr, _alive = with_bitmap(P, run, pred)
        bms = [TN.bitmap_dev(v) for v in run.valid]
        st = ops.aggregate_nullable(dev_cols(P, run), bms, run.br, pr, value, P.mask)
        flags = exp["flags"] & F.ERR
        mask = P.mask
        if exp["dtype"] == F32 and mask & abi.AGG_SUM and not flags and exp["valid"]:
            rule, n = f32_sum_rule(P, run, exp)
            if rule == "bound":  # the shape test's check knows the exact rule only: the sum here, the rest there
                mask &= ~abi.AGG_SUM
                assert bool(st.s.flags & abi.STATE_ANY_EMPTY) == bool(exp["flags"] & abi.STATE_ANY_EMPTY), (what, st.s.flags)
                got, want = TN.f64_of(st.s.sum), exp["sum"].value
                bound = 2.0 * (n - 1) * 2.0 ** -24 * exp["abs"]
                assert float(np.float32(got)) == got, (what, got)
                if np.isfinite(want):
                    assert abs(got - want) <= bound, (what, "sum", got, want, bound)
                else:
                    assert (np.isnan(got) and np.isnan(want)) or got == want, (what, "sum", got, want)
        TN.check(st, exp, mask, what, flags=flags)


def first_difference(got, want, dt):
    w = np.dtype(TP.NP[dt]).itemsize
    g, x = np.ascontiguousarray(got).view(TP.UINT[w]), np.ascontiguousarray(want).view(TP.UINT[w])
    if g.shape != x.shape:
        return "lengths %d and %d" % (len(g), len(x))
    bad = np.flatnonzero(g != x)
    if dt in (abi.DT_FLOAT32, abi.DT_FLOAT64):
        bad = np.array([i for i in bad if not (np.isnan(got[i]) and np.isnan(want[i]))])
    return "row %d: got %r want %r" % (bad[0], got[bad[0]], want[bad[0]]) if len(bad) else "none"


ERR_TEXT = {abi.FQ_E_DIVIDE_BY_ZERO: TP.DIV_ZERO, abi.FQ_E_UNSUPPORTED: TP.CAST_NULL}


def predicate_outcome(P, run):
    """("ok", bits) | ("err", status) of the predicate alone over the whole run"""
    where = P.ref()[0]
    try:
        with np.errstate(all="ignore"):
            res = where.eval(F.block_of(P, run))
    except R.RefError:
        return "err", abi.FQ_E_DIVIDE_BY_ZERO
    if res.valid is not None and not np.all(res.valid):
        return "err", abi.FQ_E_UNSUPPORTED
    return "ok", np.asarray(res.values, dtype=bool)


@pytest.mark.parametrize("seed", SEEDS)
def test_proj(seed):
    P, runs = F.generate("proj", seed)
    pred, values = P.device()
    for run in runs:
        what = "%s | %s" % (P.describe(), run.describe())
        exp = F.expected(P, run)
        cols = dev_cols(P, run)
        if run.br == 0:
            call = lambda: ops.filter_project_typed(cols, pred, values, out_offset=run.out_offset)  # noqa: E731
        else:
            call = lambda: ops.filter_project_blocks_typed(cols, run.br, pred, values, out_offset=run.out_offset,  # noqa: E731
                                                           fill=TP.FILL)
        if exp[0] == "err":
            with pytest.raises(FQError) as e:
                call()
            assert e.value.status == exp[1] and str(e.value) == ERR_TEXT[exp[1]], (what, str(e.value))
        elif run.br == 0:
            _, want, counts, dts = exp
            outs = call()
            assert len(outs) == len(want), what
            for j, o in enumerate(outs):
                assert o.len == sum(counts) and o.dtype == dts[j], (what, j, o.len, sum(counts), o.dtype, dts[j])
                got, x = o.to_numpy(), np.concatenate(want[j])
                assert TP.same(got, x, dts[j]), (what, "output %d" % j, first_difference(got, x, dts[j]))
        else:
            _, want, counts, dts = exp
            outs, cnt, kept = call()
            assert list(cnt) == counts and kept == sum(counts), (what, list(cnt), counts, kept)
            for j, o in enumerate(outs):
                assert o.dtype == dts[j], (what, j)
                x = np.full(run.n * np.dtype(TP.NP[dts[j]]).itemsize, TP.FILL, np.uint8).view(TP.NP[dts[j]])
                for b, rows in enumerate(want[j]):  # rows past a block's count stay as they were
                    x[b * run.br:b * run.br + len(rows)] = rows
                got = o.to_numpy()
                assert TP.same(got, x, dts[j]), (what, "output %d" % j, first_difference(got, x, dts[j]))
        if run.br and P.kind in ("expr", "tree"):  # the bitmap kernel once
            kind, bits = predicate_outcome(P, run)
            if kind == "err":
                with pytest.raises(FQError) as e:
                    ops.predicate_bitmap_typed(cols, pred)
                assert e.value.status == bits and str(e.value) == ERR_TEXT[bits], (what, str(e.value))
            else:
                bm = ops.predicate_bitmap_typed(cols, pred)
                got = bm.to_numpy()
                assert np.array_equal(got, bits), (what, "bitmap row %d" % np.flatnonzero(got != bits)[0])
                words = bm.buf[bm.offset:bm.offset + bm.nbytes()].cpu().numpy().view(np.uint64)
                if run.n % 64:
                    assert int(words[-1]) >> (run.n % 64) == 0, (what, "bits past n")
