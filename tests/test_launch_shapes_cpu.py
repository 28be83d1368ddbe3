"""No GPU: (1) the row counts of tests/launch_shapes.py satisfy their own
definitions for 64, 256 and 304 CUs, for every family and knob value that
tests/test_launch_shapes_gpu.py uses; (2) the inputs of that file would show
the mistakes the new sizes are there for.

For (2) each persistent loop has a small numpy model here: tiles dealt
round-robin to `grid` workers (a ticket deals them the same way when every tile
takes as long), per-frame bases, one ballot per block and wave, two LDS slots
by the parity of a worker's draws.  A model runs the GPU file's own input once
as written and once with one mistake; MUTATIONS lists (a)-(g) with the cases
that must change the result.  No mistake may change it on one_round_minus:
there no worker takes a second unit, which is all the older sizes gave."""
import numpy as np
import pytest

import launch_shapes as LS
import test_launch_shapes_gpu as G

CU_COUNTS = [64, 256, 304]
CUS = 256  # the models run the inputs the GPU file builds on a 256-CU device
LATER = ["exact_2", "ragged", "ragged_head"]   # some worker takes a second unit
RAGGED = ["ragged", "ragged_head"]             # ... and only some a third

MUTATIONS = {
    "a": ("units of round >= 2 dropped", {"for32": LATER, "flat": LATER, "block": ["ragged"], "select": LATER,
                                          "stream": ["ragged"]}),
    "b": ("the for32 base taken from the frame of the worker's first tile", {"for32": LATER}),
    "c": ("the prefetch hands the last, ragged round the previous tile's data", {"flat": RAGGED}),
    "d": ("ANY_EMPTY decided from a wave's last block only", {"block": ["ragged"]}),
    "e": ("LDS slot 1 of the select reads slot 0's ballots", {"select": LATER}),
    "f": ("the select's base for a worker's second tile taken without its predecessors", {"select": LATER}),
    "g": ("the short last block of a workgroup's later run given the full length", {"stream": ["ragged"]}),
}


# ---------------------------------------------------------------------------
# (1) the cases meet their definitions
# ---------------------------------------------------------------------------
def models(cus):
    """(label, model, uses the four cases?, uses just_above?) for every launch the GPU file sizes an input for"""
    out = []
    for wg in (1, 2):
        out.append(("for32 wg=%d" % wg, LS.for32(cus, wg), True, False))
    for name in G.COMBOS:
        for wg in G.SCAN_KNOBS:
            out.append(("flat %s wg=%d" % (name, wg), G.combo(name).model(cus, wg), True, False))
    out.append(("block", LS.block_scan(cus, G.BLOCK_ROWS), True, False))
    for e in G.PROJ_ENTRIES:
        out.append(("select %s" % e, G.select_model(cus, e, 1), True, False))
    out.append(("select cols4 wg=16", G.select_model(cus, "cols4", 16), True, False))
    for B in G.STREAM_BLOCKS:
        out.append(("stream B=%d" % B, LS.block_stream(cus, B, 1), True, False))
    for K in (1, 2, 4):
        out.append(("bitmap K=%d" % K, LS.bitmap(cus, K), False, True))
    out.append(("map", LS.project_map(cus), False, True))
    out.append(("map typed", LS.project_map(cus, G.proj_typed("typed_narrow")), False, True))
    for knob in (0, 1, 16):
        out.append(("arith knob=%d" % knob, LS.ew_arith(cus, knob), True, False))
        out.append(("compare knob=%d" % knob, LS.ew_compare(cus, knob), True, False))
    return out


@pytest.mark.parametrize("cus", CU_COUNTS)
def test_cases_meet_their_definitions(cus):
    for label, m, four, above in models(cus):
        if four:
            c = m.cases()
            assert set(c) == set(LS.CASES)
            per = m.per_worker(c["one_round_minus"][0])
            assert max(per) <= 1 and len(per) == m.cap - 1, label   # no worker takes a second unit
            per = m.per_worker(c["exact_2"][0])
            assert set(per) == {2} and len(per) == m.cap, label
            assert c["ragged"][0] == c["ragged_head"][0] and (c["ragged"][1], c["ragged_head"][1]) == (0, 1), label
            n = c["ragged"][0]
            assert n % 2 == 1 and n % m.unit_rows > 3, label            # a partial unit and odd rows
            # the grid the launch takes (the cap), and for the select kernels every smaller one an occupancy
            # below the knob would leave: every worker two units at least; at the cap some take one more
            grids = [m.cap] if m.exact_grid else [cus * o for o in range(1, m.cap // cus + 1)]
            for g in grids:
                per = m.per_worker(n, g)
                assert min(per) >= 2, (label, g)
            per = m.per_worker(n, m.cap)
            assert max(per) == min(per) + 1 == 3, label
            assert m.units(n) % m.cap, label                            # the trace's "not a multiple of the grid"
        if above:
            per = m.per_worker(m.just_above())
            assert len(per) == m.cap and min(per) == 1 and max(per) == 2, label


@pytest.mark.parametrize("cus", CU_COUNTS)
def test_geometry_restated_from_the_launch_code(cus):
    assert LS.flat_scan(cus, 8, 2) == LS.Model("flat", 2048, 2 * cus, False, True)
    assert [LS.flat_scan(cus, w, 1).unit_rows for w in (4, 2, 1)] == [4096, 4096, 4096]
    assert [LS.flat_scan_columns(cus, k, 1).unit_rows for k in (2, 3, 4)] == [1024, 512, 512]
    assert LS.typed_group([8, 4, 4, 1]) == (4, False) and LS.typed_group([1, 1]) == (16, True)
    assert LS.typed_group([4, 1, 8]) == (4, True)
    assert LS.for32(cus, 2).unit_rows == 4096 and LS.FOR32_TILES_PER_FRAME == 16
    assert LS.block_scan(cus, 144).cap == min(cus * 8, 4096) * 4
    assert [G.select_model(cus, e, 1).unit_rows for e in G.PROJ_ENTRIES] == [8192, 4096, 4096, 2048, 4096, 8192]
    assert [LS.bitmap(cus, k).unit_rows for k in (1, 2, 4)] == [2048, 1024, 512]
    assert LS.project_map(cus).unit_rows == 2048 and LS.project_map(cus, ([1, 2], [2, 1])).unit_rows == 8192
    assert LS.ew_arith(cus, 0).cap == 8 * cus and LS.ew_compare(cus, 0).cap == 2 * cus and LS.ew_arith(cus, 1).cap == cus
    assert LS.COMPACT_SECOND_ROUND_ROWS == (1 << 32) + 1


def test_for32_second_tile_lies_in_another_frame():
    for cus in CU_COUNTS:
        for wg in (1, 2):
            grid = LS.for32(cus, wg).cap
            t = np.arange(grid)
            assert np.all((t + grid) // LS.FOR32_TILES_PER_FRAME != t // LS.FOR32_TILES_PER_FRAME)


# ---------------------------------------------------------------------------
# (2) the loop models
# ---------------------------------------------------------------------------
def fold(v):
    """(wrapping sum, count, max, min) of uint64 values"""
    if len(v) == 0:
        return (0, 0, None, None)
    return (int(v.sum(dtype=np.uint64)), len(v), int(v.max()), int(v.min()))


def dealt(units, grid):
    """(worker, draw number) of each unit dealt round-robin"""
    t = np.arange(units)
    return t % grid, t // grid


def flat_model(x, tile, grid, mistake=None, base=None):
    """agg_flat_kernel / agg_flat_kernel_for32 over uint64 x: whole tiles by the grid, the rest by the tail
    loops.  base: per-frame bases of a for32 column (x then holds the deltas)"""
    n = len(x)
    ntiles = n // tile
    worker, draw = dealt(ntiles, grid)
    src = np.arange(ntiles)          # the tile whose data each iteration reduces
    frame = src // LS.FOR32_TILES_PER_FRAME
    live = np.ones(ntiles, bool)
    if mistake == "a":
        live = draw < 1
    if mistake == "b":
        frame = worker // LS.FOR32_TILES_PER_FRAME   # worker w's first tile is tile w
    if mistake == "c" and ntiles % grid and ntiles > grid:
        last = draw == draw.max()                    # the ragged round: tn < ntiles held for some workgroups only
        src = np.where(last, src - grid, src)
    body = x[:ntiles * tile].reshape(ntiles, tile)[src]
    if base is not None:
        body = body + base[frame][:, None]
    tail = x[ntiles * tile:]
    if base is not None:
        tail = tail + base[(np.arange(ntiles * tile, n)) // LS.FRAME_ROWS]
    return fold(np.concatenate([body[live].reshape(-1), tail]))


def for32_columns(host):
    F = LS.FRAME_ROWS
    base = np.array([host[s:s + F].min() for s in range(0, len(host), F)], dtype=np.uint64)
    return host - np.repeat(base, F)[:len(host)], base


@pytest.mark.parametrize("data", G.FOR32_DATA)
@pytest.mark.parametrize("wg", [1, 2])
def test_for32_inputs_show_a_dropped_round_and_a_stale_base(wg, data):
    for case in LS.CASES:
        m, n, _, host = G.for32_input(CUS, wg, case, data)
        delta, base = for32_columns(host)
        good = flat_model(delta, m.unit_rows, m.workers(n), base=base)
        assert good == fold(host)
        for mistake in "ab":
            bad = flat_model(delta, m.unit_rows, m.workers(n), mistake, base)
            assert (bad != good) == (case in MUTATIONS[mistake][1]["for32"]), (mistake, case)


def as_u64(col):
    return col.view(np.uint64) if col.dtype.itemsize == 8 else col.astype(np.int64).view(np.uint64)


@pytest.mark.parametrize("name,sized_for,case", G.FLAT_RUNS, ids=["%s-wg%d-%s" % r for r in G.FLAT_RUNS])
def test_flat_inputs_show_a_dropped_round_and_a_stale_prefetch(name, sized_for, case):
    _, m, n, _, host, _ = G.flat_input(CUS, name, sized_for, case)
    x = as_u64(host[0])
    good = flat_model(x, m.unit_rows, m.workers(n))
    assert good == fold(x)
    for mistake in "ac":
        bad = flat_model(x, m.unit_rows, m.workers(n), mistake)
        assert (bad != good) == (case in MUTATIONS[mistake][1]["flat"]), (mistake, name, case)


def block_model(keep, R, W, mistake=None):
    """agg_block_kernel: block b on wave b % W; -> (kept rows, ANY_EMPTY)"""
    n = len(keep)
    nb = -(-n // R)
    pad = np.zeros(nb * R, bool)
    pad[:n] = keep
    kept = pad.reshape(nb, R).sum(axis=1)
    wave, draw = dealt(nb, W)
    live = np.ones(nb, bool)
    if mistake == "a":
        live = draw < 1
    counts = np.bincount(wave, minlength=W)
    empty = (kept == 0) & live
    if mistake == "d":
        empty &= draw == counts[wave] - 1   # the flag overwritten per block instead of OR-ed
    return int(kept[live].sum()), bool(empty.any())


@pytest.mark.parametrize("pattern", G.BLOCK_PATTERNS)
def test_block_inputs_show_a_flag_that_is_not_carried(pattern):
    for case in ("one_round_minus", "ragged"):
        _, m, n, nb, host, _ = G.block_input(CUS, "aggregate", pattern, case)
        keep = host[0] < 2000
        good = block_model(keep, G.BLOCK_ROWS, m.workers(n))
        assert good == (int(keep.sum()), True)
        for mistake in "ad":
            bad = block_model(keep, G.BLOCK_ROWS, m.workers(n), mistake)
            assert (bad != good) == (case in MUTATIONS[mistake][1]["block"]), (mistake, pattern, case)


def select_model(keep, value, tile, grid, mistake=None):
    """fq_jit_pselect: tile t drawn by worker t % grid into LDS slot (draw & 1); -> the output column"""
    n = len(keep)
    ntiles = -(-n // tile)
    pad = np.zeros(ntiles * tile, bool)
    pad[:n] = keep
    masks = pad.reshape(ntiles, tile)
    worker, draw = dealt(ntiles, grid)
    counts = masks.sum(axis=1)
    base = np.concatenate([[0], np.cumsum(counts)[:-1]])
    out = np.zeros(int(counts.sum()) + tile, dtype=value.dtype)  # room for a misplaced tile
    vals = np.zeros(ntiles * tile, dtype=value.dtype)
    vals[:n] = value
    vals = vals.reshape(ntiles, tile)
    for t in range(ntiles):
        if mistake == "a" and draw[t] >= 1:
            continue
        mask = masks[t - grid] if mistake == "e" and draw[t] & 1 else masks[t]
        b = 0 if mistake == "f" and draw[t] >= 1 else base[t]
        rows = vals[t][mask]
        out[b:b + len(rows)] = rows[:len(out) - b]
    return out


@pytest.mark.parametrize("entry", ["one", "cols4"])
def test_select_inputs_show_a_wrong_slot_and_a_wrong_base(entry):
    m = G.select_model(CUS, entry, 1)
    for case in LS.CASES:
        n = m.cases()[case][0]
        rates = list(G.RATES)[:4] if case == "ragged" else ["1/8"]
        for rate in rates:
            c = G.proj_case(entry, n, G.RATES[rate])
            keep = G.proj_keep(c)
            good = select_model(keep, c.host[0], m.unit_rows, m.workers(n))
            assert np.array_equal(good[:int(keep.sum())], c.host[0][keep])
            for mistake in "aef":
                bad = select_model(keep, c.host[0], m.unit_rows, m.workers(n), mistake)
                # every row kept: both slots hold the same ballots, so (e) cannot show there
                caught = case in MUTATIONS[mistake][1]["select"] and not (mistake == "e" and rate == "every")
                assert (not np.array_equal(bad, good)) == caught, (mistake, entry, case, rate)


def stream_model(keep_ext, n, B, grid, mistake=None):
    """fq_jit_pblocks: block b drawn by worker b % grid; keep_ext continues the predicate past row n, which is
    what a block end computed without `< n` would read; -> per-block counts"""
    nb = -(-n // B)
    _, draw = dealt(nb, grid)
    counts = []
    for b in range(nb):
        end = min((b + 1) * B, n)
        if mistake == "g" and b == nb - 1 and draw[b] >= 1:
            end = (b + 1) * B
        if mistake == "a" and draw[b] >= 1:
            end = b * B
        counts.append(int(keep_ext[b * B:end].sum()))
    return counts


@pytest.mark.parametrize("B", G.STREAM_BLOCKS)
def test_stream_inputs_show_a_last_block_taken_whole(B):
    for case in ("one_round_minus", "ragged"):
        m, n = G.stream_rows(CUS, B, case)
        nb = m.units(n)
        assert n % B  # the last block is short in both cases
        ext = G.proj_case("one", nb * B, G.STREAM_K)  # the same iota, continued to the end of the last block
        assert np.array_equal(ext.host[0][:n], G.proj_case("one", n, G.STREAM_K).host[0])
        keep = G.proj_keep(ext)
        good = stream_model(keep, n, B, m.workers(n))
        assert sum(good) == int(keep[:n].sum())
        for mistake in "ag":
            bad = stream_model(keep, n, B, m.workers(n), mistake)
            assert (bad != good) == (case in MUTATIONS[mistake][1]["stream"]), (mistake, B, case)


def test_mutation_table_lists_every_mistake_with_the_cases_that_catch_it():
    assert sorted(MUTATIONS) == list("abcdefg")
    for key, (what, caught) in MUTATIONS.items():
        assert what and caught, key
        for family, cases in caught.items():
            assert cases and "one_round_minus" not in cases, (key, family)
            assert set(cases) <= set(LS.CASES)
    print("\n".join("(%s) %s: %s" % (k, w, "; ".join("%s at %s" % (f, ", ".join(c)) for f, c in fam.items()))
                    for k, (w, fam) in MUTATIONS.items()))
