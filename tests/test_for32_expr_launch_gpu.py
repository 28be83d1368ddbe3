"""fq_jit_scan_for32's persistent loop past its first iteration.  The flat grid is
CUs x SCAN_WG_PER_CU workgroups over tiles of 4,096 rows, so only inputs sized
from the device's CU count make a workgroup take a second tile -- where the
prefetched tile lies in another frame than the one being decoded (16 tiles to a
frame: any grid of 16 or more workgroups).  For the knob at 1 and at 2: one round
less a tile, exactly two rounds, and two and a third rounds with a partial tile
and 3 odd rows (tests/for32_expr_shapes.py launch_rows), random frame bases, the
c4 and c4s shapes -- each against the plain scan and numpy, and every input
under both grids byte for byte (the states are integers)."""
import functools

import numpy as np
import pytest

from fq_amd import abi

import for32_expr_shapes as S

pytestmark = pytest.mark.gpu

ops = None
CUS = None
KNOBS = (1, 2)
CASES = ("one_round_minus", "exact_2", "ragged")
MASK = {"c4": abi.AGG_MAX | abi.AGG_COUNT, "c4s": abi.AGG_SUM | abi.AGG_COUNT}


def setup_module():
    global ops, CUS
    import torch
    from fq_amd import ops as _ops
    _ops.require_gpu()
    _ops.jit_config(abi.JIT_ALWAYS, 0)
    ops = _ops
    CUS = torch.cuda.get_device_properties(0).multi_processor_count


def teardown_module():
    if ops is not None:
        ops.tune_reset()
        ops.jit_config(abi.JIT_AUTO, 1 << 22)


@functools.lru_cache(maxsize=None)
def encoded(n):
    host = S.host_values(n, "random")
    col = ops.from_numpy(host)
    enc, ok = ops.for32_encode(col)
    assert ok
    return host, col, enc


def test_the_sizes_pass_the_first_iteration():
    for k in KNOBS:
        rows = S.launch_rows(CUS, k)
        cap = CUS * k
        tiles = {c: (rows[c] // 4) // 1024 for c in CASES}
        assert tiles["one_round_minus"] == cap - 1 and tiles["exact_2"] == 2 * cap
        assert tiles["ragged"] > 2 * cap and rows["ragged"] % 4 == 3 and (rows["ragged"] // 4) % 1024 == 512
        assert S.flat_grid(rows["exact_2"], cap) == cap >= S.TILES_PER_FRAME  # the next tile is in another frame


@pytest.mark.parametrize("name", ["c4", "c4s"])
@pytest.mark.parametrize("sized_for", KNOBS)
@pytest.mark.parametrize("case", CASES)
def test_every_input_under_both_grids(case, sized_for, name):
    n = S.launch_rows(CUS, sized_for)[case]
    host, col, enc = encoded(n)
    pred, value, keep, val = S.shape(name)
    s, mx, mn, c = S.reference(host, keep, val)
    states = []
    try:
        for knob in KNOBS:
            ops.tune_set("SCAN_WG_PER_CU", knob)
            got = ops.aggregate_for32_expr(enc, 0, pred, value, MASK[name])
            plain = ops.aggregate(col, 0, pred, value, MASK[name])
            assert bytes(got) == bytes(plain), (case, sized_for, knob)
            assert got.count == c and got.flags == 0 and got.blocks == 1
            assert got.sum == s if name == "c4s" else got.max == mx
            states.append(bytes(got))
    finally:
        ops.tune_reset()
    assert states[0] == states[1]
