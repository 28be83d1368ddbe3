"""Resident numbers_mt partitions stored once more as per-frame 32-bit deltas
(FQ_OPT_RESIDENT_FOR32): the unfiltered sum / max / min / count scans read the
delta copy and return the rows of the plain scan, of the closed forms and of
oracle/fq_ref.py -- with the option on and off over the same resident data, over
the whole table and over one rank's shard; the statistics account the bytes
each path really reads; every other reader (filtered or expression scans, the
Filter -> Projection block stream, GROUP BY) still reads the plain column; and
releasing the table frees the copies with it."""
import functools

import numpy as np
import pytest

from fq_amd import abi
from fq_amd.numbers import generate_parts, shard, stream_rows

import fq_ref as R

pytestmark = pytest.mark.gpu

F = abi.FOR32_FRAME_ROWS
# 80: 10-row partitions; 100001: the 20,009-row quirk; 800000: whole 10,000-row blocks;
# 8 * 65536 * 3 + 80000: partitions of three whole frames and a part; 20,000,000: several workgroups' tiles
SIZES = [80, 100001, 800000, 8 * 65536 * 3 + 80000, 20_000_000]
SHARDS = [(0, 1), (0, 2), (1, 2), (7, 8)]
QUERIES = {
    "c2": "SELECT sum(number) FROM system.numbers_mt(%d)",
    "c3": "SELECT sum(number)/count(number), max(number), min(number) FROM system.numbers_mt(%d)",
    "max": "SELECT max(number) FROM system.numbers_mt(%d)",
    "avg": "SELECT sum(number) / count(number) FROM system.numbers_mt(%d)",
    "count": "SELECT count(number) FROM system.numbers_mt(%d)",
}

E = None
OPT = None


def setup_module():
    global E, OPT
    from fq_amd import ops
    ops.require_gpu()
    from fq_amd import engine
    OPT = engine.OPT_RESIDENT_FOR32
    E = engine.Engine()


def teardown_module():
    if E is not None:
        E.close()


def runs(n, rank, world):
    """[(first value, rows)] of the partitions rank owns."""
    return [(b, stream_rows(b, e)) for _, b, e in shard(generate_parts(n), rank, world)]


def rows_of(s, c, mx, mn):
    return {"c2": [(s,)], "c3": [(s // c, mx, mn)], "max": [(mx,)], "avg": [(s // c,)], "count": [(c,)]}


def closed_forms(n, rank, world):
    rs = runs(n, rank, world)
    s = sum((2 * b + r - 1) * r // 2 for b, r in rs) % 2**64
    return rows_of(s, sum(r for _, r in rs), max(b + r - 1 for b, r in rs), min(b for b, _ in rs))


@functools.lru_cache(maxsize=None)
def reference_partition(n, b, e):
    """oracle/fq_ref.py's Source -> AggregatePartial -> AggregateFinal over one partition: (sum, count, max, min).
    One pass per partition for every statement and shard of this module (20,000,000 rows take it ~6 s in all)."""
    num = R.E_field("number")
    return tuple(v.value for v in R.aggregate_query(
        n, [R.E_fn("sum", num), R.E_fn("count", num), R.E_fn("max", num), R.E_fn("min", num)], parts=[(b, e)]))


def reference(n, rank, world):
    """The rank's partitions merged as AggregateFinal merges them (wrapping sum, summed count, max, min)."""
    ps = [reference_partition(n, b, e) for _, b, e in shard(generate_parts(n), rank, world)]
    return rows_of(sum(p[0] for p in ps) % 2**64, sum(p[1] for p in ps), max(p[2] for p in ps), min(p[3] for p in ps))


def execute(sql, rank, world):
    if world == 1:
        return E.execute(sql).rows
    return E.execute_final(sql, [E.execute_partial(sql, rank, world)]).rows


@pytest.mark.parametrize("rank,world", SHARDS)
@pytest.mark.parametrize("n", SIZES)
def test_same_rows_and_true_bytes_with_the_option_on_and_off(n, rank, world):
    rs = runs(n, rank, world)
    rows = sum(r for _, r in rs)
    frames = sum((r + F - 1) // F for _, r in rs)
    exp, ref = closed_forms(n, rank, world), reference(n, rank, world)
    assert exp == ref
    E.set_option(OPT, 1)
    E.materialize_numbers(n, rank, world)
    try:
        for on in (1, 0, 1):
            E.set_option(OPT, on)
            for name, sql in QUERIES.items():
                E.reset_stats()
                assert execute(sql % n, rank, world) == exp[name], (name, on)
                st = E.stats()
                assert st["scan_launches"] == len(rs) and st["scan_rows"] == rows, (name, on, st)
                assert st["scan_bytes"] == (4 * rows + 8 * frames if on else 8 * rows), (name, on, st)
    finally:
        E.set_option(OPT, 1)
        E.release_numbers()


def test_option_off_at_materialise_time_builds_no_copy():
    n = 800000
    E.set_option(OPT, 0)
    E.materialize_numbers(n)
    try:
        E.set_option(OPT, 1)  # nothing to read: the scans stay plain
        E.reset_stats()
        assert E.execute(QUERIES["c3"] % n).rows == closed_forms(n, 0, 1)["c3"]
        assert E.stats()["scan_bytes"] == 8 * n
    finally:
        E.release_numbers()
    from fq_amd.engine import FQError
    with pytest.raises(FQError):
        E.set_option(OPT, 2)


def test_the_library_default_is_off_and_the_python_engine_opts_in():
    from fq_amd.engine import Engine
    n = 800000
    for kwargs, per_row, frames in (({"resident_for32": None}, 8, 0), ({}, 4, 8 * ((n // 8 + F - 1) // F)),
                                    ({"resident_for32": False}, 8, 0)):
        with Engine(**kwargs) as e:
            e.materialize_numbers(n)
            try:
                assert e.execute(QUERIES["c3"] % n).rows == closed_forms(n, 0, 1)["c3"]
                assert e.stats()["scan_bytes"] == per_row * n + 8 * frames, kwargs
            finally:
                e.release_numbers()


def flat(c):
    """One column of fq_amd.ops.device_block_to_numpy: per-block arrays, or one array."""
    if isinstance(c, list):
        return np.concatenate(c) if c else np.zeros(0, np.uint64)
    return np.asarray(c)


def block_stream(sql):
    """Every projected column of the stream, its kept rows sorted (the pipes interleave)."""
    from fq_amd import ops
    cols = None
    with E.execute_blocks(sql) as st:
        for b in st:
            got = [flat(c) for c in ops.device_block_to_numpy(b)]
            cols = got if cols is None else [np.concatenate([a, g]) for a, g in zip(cols, got)]
    return [np.sort(c) for c in cols]


def test_other_readers_still_read_the_plain_column():
    n = 800000
    c4 = "SELECT max(number+1) FROM system.numbers_mt(%d) WHERE (number%%8)<3" % n
    max1 = "SELECT max(number+1) FROM system.numbers_mt(%d)" % n
    g1 = ("SELECT number%%1000, count(number), sum(number), max(number) FROM system.numbers_mt(%d) "
          "GROUP BY number%%1000" % n)
    p1 = "SELECT number+1, number/2 FROM system.numbers_mt(%d) WHERE (number%%8)<3" % n
    E.set_option(OPT, 1)
    E.materialize_numbers(n)
    try:
        seen = {}
        for on in (1, 0):
            E.set_option(OPT, on)
            for name, sql in (("c4", c4), ("max1", max1), ("g1", g1)):
                E.reset_stats()
                got = sorted(E.execute(sql).rows)
                st = E.stats()
                assert st["scan_rows"] == n and st["scan_bytes"] == 8 * n, (name, on, st)
                assert seen.setdefault(name, got) == got, (name, on)
            E.reset_stats()
            cols = block_stream(p1)
            st = E.stats()
            kept = len(cols[0])
            assert st["project_rows"] == n and st["project_kept"] == kept == 3 * n // 8
            assert st["project_bytes"] == 8 * n + 16 * kept, (on, st)
            prev = seen.setdefault("p1", cols)
            assert all(np.array_equal(a, b) for a, b in zip(prev, cols))
        assert seen["c4"] == [(n - 5,)] and seen["max1"] == [(n,)]  # 799,994 % 8 == 2 is the last kept row
        assert len(seen["g1"]) == 1000 and seen["g1"][7] == (7, 800, 7 * 800 + 1000 * (799 * 800 // 2), 799007)
        k = np.arange(n, dtype=np.uint64)
        k = k[k % 8 < 3]
        assert np.array_equal(seen["p1"][0], k + 1) and np.array_equal(seen["p1"][1], np.sort(k // 2))
    finally:
        E.set_option(OPT, 1)
        E.release_numbers()


def test_release_frees_the_copies_with_the_columns():
    import torch

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    n = 20_000_000
    E.set_option(OPT, 1)
    E.trim_memory()
    before = free()
    E.materialize_numbers(n)
    try:
        E.reset_stats()
        assert E.execute(QUERIES["c2"] % n).rows == closed_forms(n, 0, 1)["c2"]
        assert E.stats()["scan_bytes"] == 4 * n + 8 * 8 * ((n // 8 + F - 1) // F)
        held = before - free()
        assert held >= 12 * n  # the plain columns and their copies
    finally:
        E.release_numbers()
    E.trim_memory()
    assert before - free() <= 64 << 20
