"""FQ_OPT_RESIDENT_FOR32_FUSED (option 9, Engine(for32_fused=True)): with the
delta copies on (option 8), a fused aggregate scan of a resident numbers_mt
partition WITH a fused WHERE and/or an argument expression reads the 32-bit
delta copy too, wherever the JIT specialises the scan.  The rows are those of
the plain path, of numpy over the partitions' runs and of oracle/fq_ref.py, over
the whole table and over one rank's shard; scan_bytes accounts 4 B per row and
8 B per frame when the copy is read and 8 B per row when it is not; scans the
JIT would not specialise, GROUP BY and the Filter -> Projection block stream
stay plain; an error query returns the same text on both paths."""
import functools

import numpy as np
import pytest

from fq_amd import abi
from fq_amd.numbers import generate_parts, shard, stream_rows

import fq_ref as R

pytestmark = pytest.mark.gpu

F = abi.FOR32_FRAME_ROWS
SIZES = [80, 100001, 800000, 8 * 65536 * 3 + 80000, 20_000_000]
SHARDS = [(0, 1), (1, 2), (7, 8)]
WHERE_C4 = "(number%8)<3"
WHERE_TREE = "((number%8)<3 AND number>1000) OR (number%7)=0"
QUERIES = {
    "c4": "SELECT max(number+1) FROM system.numbers_mt(%%d) WHERE %s" % WHERE_C4.replace("%", "%%"),
    "c4s": "SELECT sum(number+1) FROM system.numbers_mt(%%d) WHERE %s" % WHERE_C4.replace("%", "%%"),
    "max1": "SELECT max(number+1) FROM system.numbers_mt(%d)",
    "tree": "SELECT max(number+1) FROM system.numbers_mt(%%d) WHERE %s" % WHERE_TREE.replace("%", "%%"),
}

E = None
ops = None
OPT8 = OPT9 = None


def setup_module():
    global E, ops, OPT8, OPT9
    from fq_amd import ops as _ops
    _ops.require_gpu()
    ops = _ops
    from fq_amd import engine
    OPT8, OPT9 = engine.OPT_RESIDENT_FOR32, engine.OPT_RESIDENT_FOR32_FUSED
    ops.jit_config(abi.JIT_ALWAYS, 0)
    E = engine.Engine(for32_fused=True)


def teardown_module():
    if E is not None:
        E.close()
    if ops is not None:
        ops.jit_config(abi.JIT_AUTO, 1 << 22)


def runs(n, rank, world):
    """[(first value, rows)] of the partitions rank owns."""
    return [(b, stream_rows(b, e)) for _, b, e in shard(generate_parts(n), rank, world)]


@functools.lru_cache(maxsize=None)
def expected(n, rank, world):
    """The four queries' rows from numpy over the rank's runs (u64 arithmetic wraps as the engine's does)."""
    s = mx4 = mx1 = mxt = 0
    for b, r in runs(n, rank, world):
        x = np.arange(b, b + r, dtype=np.uint64)
        k = x[x % np.uint64(8) < np.uint64(3)]
        t = x[((x % np.uint64(8) < np.uint64(3)) & (x > np.uint64(1000))) | (x % np.uint64(7) == np.uint64(0))]
        s = (s + int((k + np.uint64(1)).sum(dtype=np.uint64))) % 2**64
        mx4 = max(mx4, int(k.max()) + 1) if len(k) else mx4
        mx1 = max(mx1, int(x.max()) + 1)
        mxt = max(mxt, int(t.max()) + 1) if len(t) else mxt
    return {"c4": [(mx4,)], "c4s": [(s,)], "max1": [(mx1,)], "tree": [(mxt,)]}


def reference(n):
    """oracle/fq_ref.py's pipeline for the four queries over the whole table (small tables only: it is slow)."""
    num, c = R.E_field("number"), R.E_const
    plus1 = R.E_bin("+", num, c(1))
    w4 = R.E_bin("<", R.E_bin("%", num, c(8)), c(3))
    wt = R.E_bin("or", R.E_bin("and", w4, R.E_bin(">", num, c(1000))), R.E_bin("=", R.E_bin("%", num, c(7)), c(0)))
    row = lambda exprs, where: [tuple(v.value for v in R.aggregate_query(n, exprs, where=where))]
    return {"c4": row([R.E_fn("max", plus1)], w4), "c4s": row([R.E_fn("sum", plus1)], w4),
            "max1": row([R.E_fn("max", plus1)], None),
            "tree": row([R.E_fn("max", plus1)], wt)}


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
    exp = expected(n, rank, world)
    if n <= 100001 and world == 1:
        assert reference(n) == exp
    E.set_option(OPT8, 1)
    E.materialize_numbers(n, rank, world)
    try:
        for on in (1, 0, 1):
            E.set_option(OPT9, on)
            for name, sql in QUERIES.items():
                E.reset_stats()
                assert execute(sql % n, rank, world) == exp[name], (name, on)
                st = E.stats()
                assert st["scan_launches"] == len(rs) and st["scan_rows"] == rows, (name, on, st)
                assert st["scan_bytes"] == (4 * rows + 8 * frames if on else 8 * rows), (name, on, st)
    finally:
        E.set_option(OPT9, 1)
        E.release_numbers()


def scan_bytes(sql):
    E.reset_stats()
    rows = E.execute(sql).rows
    return rows, E.stats()["scan_bytes"]


def test_jit_auto_keeps_scans_below_min_rows_plain():
    """The interpreting kernels know no deltas: under FQ_JIT_AUTO only partitions of at least min_rows rows take
    the copy.  20,000,000 rows are 8 partitions of 2,500,000, below the default 2^22 and above 2^20."""
    n = 20_000_000
    frames = 8 * ((n // 8 + F - 1) // F)
    exp = expected(n, 0, 1)
    E.set_option(OPT8, 1)
    E.set_option(OPT9, 1)
    E.materialize_numbers(n)
    try:
        for min_rows, want in ((1 << 22, 8 * n), (1 << 20, 4 * n + 8 * frames), (2_500_001, 8 * n),
                               (2_500_000, 4 * n + 8 * frames)):
            ops.jit_config(abi.JIT_AUTO, min_rows)
            for name in ("c4", "c4s", "max1"):
                assert scan_bytes(QUERIES[name] % n) == (exp[name], want), (name, min_rows)
        ops.jit_config(abi.JIT_OFF)
        assert scan_bytes(QUERIES["c4"] % n) == (exp["c4"], 8 * n)
    finally:
        ops.jit_config(abi.JIT_ALWAYS, 0)
        E.release_numbers()


def flat(c):
    if isinstance(c, list):
        return np.concatenate(c) if c else np.zeros(0, np.uint64)
    return np.asarray(c)


def test_option_8_off_and_the_other_readers_stay_plain():
    n = 800000
    frames = 8 * ((n // 8 + F - 1) // F)
    exp = expected(n, 0, 1)
    g1 = ("SELECT number%%1000, count(number), sum(number), max(number) FROM system.numbers_mt(%d) "
          "GROUP BY number%%1000" % n)
    p1 = "SELECT number+1, number/2 FROM system.numbers_mt(%d) WHERE (number%%8)<3" % n
    E.set_option(OPT8, 1)
    E.set_option(OPT9, 1)
    E.materialize_numbers(n)
    try:
        assert scan_bytes(QUERIES["c4"] % n) == (exp["c4"], 4 * n + 8 * frames)
        # the identity scans are option 8's, with or without option 9
        c3 = "SELECT sum(number)/count(number), max(number), min(number) FROM system.numbers_mt(%d)" % n
        for on in (1, 0):
            E.set_option(OPT9, on)
            assert scan_bytes(c3) == ([((n - 1) // 2, n - 1, 0)], 4 * n + 8 * frames)
        E.set_option(OPT9, 1)
        # GROUP BY and the block stream read the plain column with both options on
        E.reset_stats()
        got = sorted(E.execute(g1).rows)
        st = E.stats()
        assert st["scan_rows"] == n and st["scan_bytes"] == 8 * n
        assert len(got) == 1000 and got[7] == (7, 800, 7 * 800 + 1000 * (799 * 800 // 2), 799007)
        E.reset_stats()
        kept = 0
        with E.execute_blocks(p1) as stream:
            for b in stream:
                kept += len(flat(ops.device_block_to_numpy(b)[0]))
        st = E.stats()
        assert st["project_rows"] == n and st["project_kept"] == kept == 3 * n // 8
        assert st["project_bytes"] == 8 * n + 16 * kept
        # option 8 off: option 9 alone reads nothing but the plain column
        E.set_option(OPT8, 0)
        for name in ("c4", "c4s", "max1", "tree"):
            assert scan_bytes(QUERIES[name] % n) == (exp[name], 8 * n), name
    finally:
        E.set_option(OPT8, 1)
        E.release_numbers()


def test_an_error_query_returns_the_same_text_on_both_paths():
    """10 / number divides by zero in row 0, which (0 % 8) < 3 keeps."""
    from fq_amd.engine import FQError
    n = 800000
    sql = "SELECT max(10/number) FROM system.numbers_mt(%d) WHERE (number%%8)<3" % n
    ok = "SELECT max(10/number) FROM system.numbers_mt(%d) WHERE (number%%8)>3" % n  # drops row 0
    E.set_option(OPT8, 1)
    E.materialize_numbers(n)
    try:
        text, fine = {}, {}
        for on in (1, 0):
            E.set_option(OPT9, on)
            with pytest.raises(FQError) as ei:
                E.execute(sql)
            text[on] = (ei.value.status, str(ei.value))
            fine[on] = scan_bytes(ok)
        assert text[1] == text[0] and "ivide by zero" in text[1][1]
        assert fine[1][0] == fine[0][0] == [(2,)] and fine[0][1] == 8 * n and fine[1][1] < fine[0][1]  # 10 / 4
    finally:
        E.set_option(OPT9, 1)
        E.release_numbers()


def test_the_default_is_off_and_the_variable_turns_it_on(monkeypatch):
    from fq_amd.engine import Engine, FQError
    n = 800000
    frames = 8 * ((n // 8 + F - 1) // F)
    exp = expected(n, 0, 1)["c4"]
    monkeypatch.delenv("FQ_RESIDENT_FOR32_FUSED", raising=False)
    cases = [({}, 8 * n), ({"for32_fused": False}, 8 * n), ({"for32_fused": True}, 4 * n + 8 * frames),
             ({"for32_fused": True, "resident_for32": None}, 8 * n)]  # (the library's option 8 is off)
    for env, want in ((None, None), ("1", 4 * n + 8 * frames), ("0", 8 * n)):
        if env is not None:
            monkeypatch.setenv("FQ_RESIDENT_FOR32_FUSED", env)
            cases = [({}, want), ({"for32_fused": False}, 8 * n)]
        for kwargs, nbytes in cases:
            with Engine(**kwargs) as e:
                e.materialize_numbers(n)
                try:
                    e.reset_stats()
                    assert e.execute(QUERIES["c4"] % n).rows == exp
                    assert e.stats()["scan_bytes"] == nbytes, (env, kwargs)
                finally:
                    e.release_numbers()
    with pytest.raises(FQError):
        E.set_option(OPT9, 2)
    with pytest.raises(FQError):
        E.set_option(OPT9, -1)
