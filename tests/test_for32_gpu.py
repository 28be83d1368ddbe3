"""fq_for32_encode / fq_aggregate_for32 at the C ABI, bit for bit against the
oracle (oracle_c.column_partial, wrapping u64) on the decoded values and against
fq_aggregate on the plain column.

Lengths: around the 4-row vector, the 4,096-row tile and the 65,536-row frame,
more than one workgroup, and 0.  Data: (a) an iota from 1,250,000,000; (b) an
iota from 2^64 - 70,000 (the sum wraps; past row 70,000 the values wrap too, and
the frame that holds 2^64 - 1 and 0 then spans more than 32 bits, so by the
encoding's definition -- base = the frame's minimum, encodable iff max - min <=
2^32 - 1 in every frame -- those lengths must raise the encoder's flag);
(c) seeded random deltas below 2^32 over a seeded random base per frame; (d) a
frame with max - min == 2^32 - 1; (e) a frame with max - min == 2^32, which the
encoder must refuse.  Whether a column is encodable is worked out here from the
host values, never taken from the encoder."""
import functools

import numpy as np
import pytest

from fq_amd import abi

import oracle_c

pytestmark = pytest.mark.gpu

F = abi.FOR32_FRAME_ROWS
U64 = abi.DT_UINT64
LENGTHS = [1, 3, 4, 5, 4095, 4096, 4097, 65535, 65536, 65537, 2 * 65536 + 4099, 1_000_003]
DATA = ["iota", "iota_wrap", "random", "span_max", "span_over"]
MASKS = [abi.AGG_SUM, abi.AGG_MAX, abi.AGG_MIN, abi.AGG_COUNT, abi.AGG_SUM | abi.AGG_COUNT,
         abi.AGG_SUM | abi.AGG_MAX | abi.AGG_MIN | abi.AGG_COUNT]
AGGS = [(abi.AGG_SUM, None), (abi.AGG_COUNT, None), (abi.AGG_MAX, None), (abi.AGG_MIN, None)]

ops = None


def setup_module():
    global ops
    from fq_amd import ops as _ops
    _ops.require_gpu()
    ops = _ops


def host_values(n, data):
    if data == "iota":
        return np.arange(n, dtype=np.uint64) + np.uint64(1_250_000_000)
    if data == "iota_wrap":
        with np.errstate(over="ignore"):
            return np.arange(n, dtype=np.uint64) + np.uint64(2**64 - 70_000)
    rng = np.random.default_rng(1000 * n + DATA.index(data))
    frames = (n + F - 1) // F
    if data == "random":
        base = rng.integers(0, 2**64 - 2**32, size=frames, dtype=np.uint64)
        return np.repeat(base, F)[:n] + rng.integers(0, 2**32, size=n, dtype=np.uint64)
    # span_max / span_over: small values around one base, and in the last frame
    # of at least two rows a pair whose difference is 2^32 - 1 / 2^32
    v = np.uint64(3 << 40) + rng.integers(1000, 2000, size=n, dtype=np.uint64)
    f = frames - 1 if n - (frames - 1) * F >= 2 else frames - 2
    lo, hi = f * F, min((f + 1) * F, n) - 1
    v[lo] = np.uint64(3 << 40)
    v[hi] = np.uint64((3 << 40) + (2**32 - 1 if data == "span_max" else 2**32))
    return v


def encodable(host):
    for s in range(0, len(host), F):
        fr = host[s:s + F]
        if int(fr.max()) - int(fr.min()) > 2**32 - 1:
            return False
    return True


def cases():
    for n in LENGTHS:
        for d in DATA:
            if d.startswith("span") and n < 2:
                continue  # one row has no span
            yield n, d


@functools.lru_cache(maxsize=None)
def encoded(n, data):
    """(host values, plain column, For32Column, encoder's verdict, the oracle's [sum, count, max, min])."""
    host = host_values(n, data)
    col = ops.from_numpy(host)
    enc, ok = ops.for32_encode(col)
    exp = [s.bits for s in oracle_c.column_partial(host, U64, n, AGGS)]
    return host, col, enc, ok, exp


@pytest.mark.parametrize("n,data", list(cases()))
def test_encoder_flags_exactly_the_unencodable_columns_and_decodes_exactly(n, data):
    host, _, enc, ok, _ = encoded(n, data)
    assert ok == encodable(host)
    if data == "span_over":
        assert not ok
    if data in ("iota", "random", "span_max"):
        assert ok
    if not ok:
        return
    base = enc.base.to_numpy()
    assert len(base) == (n + F - 1) // F
    assert np.array_equal(base, np.array([host[s:s + F].min() for s in range(0, n, F)], dtype=np.uint64))
    assert np.array_equal(enc.decode(), host)
    if data == "span_max":
        assert int(enc.delta.to_numpy().max()) == 2**32 - 1


def fields(st):
    return (st.sum, st.max, st.min, st.count, st.blocks, st.flags, st.dtype)


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("n,data", [c for c in cases() if c[1] != "span_over"])
def test_scan_equals_oracle_and_plain_scan(n, data, mask):
    host, col, enc, ok, (s, c, mx, mn) = encoded(n, data)
    if not ok:
        assert not encodable(host)  # (b) past the wrap: checked by the encoder test
        return
    got = ops.aggregate_for32(enc, mask)
    plain = ops.aggregate(col, 0, None, None, mask)
    assert fields(got) == fields(plain)
    assert got.dtype == U64 and got.flags == 0 and got.count == c == n
    if mask & abi.AGG_SUM:
        assert got.sum == s
    if mask & abi.AGG_MAX:
        assert got.max == mx
    if mask & abi.AGG_MIN:
        assert got.min == mn


@pytest.mark.parametrize("mask", MASKS)
def test_length_zero_is_the_empty_state_of_the_plain_scan(mask):
    col = ops.from_numpy(np.zeros(0, np.uint64))
    enc, ok = ops.for32_encode(col)
    assert ok and enc.len == 0
    assert fields(ops.aggregate_for32(enc, mask)) == fields(ops.aggregate(col, 0, None, None, mask))
