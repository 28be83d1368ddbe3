"""Randomised GROUP BY at scale: seeded key shapes over `number` -- scattered
(`% m`), clustered (`/ d`, runs of d rows) and both (`(number / d) % m`) --
with random predicates and integer aggregates, through the engine on the GPU
(sampled LDS-table launches, dense keys, the clustered row layout, radix-
partitioned launches by key range or hash) against the C GROUP BY
restatement (oracle/fq_oracle.c fqo_numbers_group) over the same numbers_mt
blocks.  GROUP BY has no reference transform (plan_parser.rs:284-308 plans it,
pipeline_builder.rs:50-66 ignores it): the semantics are the ungrouped path's
per group, pinned for small sizes against fq_ref in test_fuzz_gpu.py.

Below the engine-level seeds, the kernel-level fuzz: the cases of
tests/fuzz_groupby.py through ops.GroupTable on every path -- one direct
launch, the radix-partitioned entry, narrow rows, the column split into blocks
accumulated into one table, two tables merged -- under the seed's launch-shape
knobs (the defaults, or 256 threads and an 8 KB LDS table, where every branch
boundary of the kernels lies within a few thousand rows;
tests/test_fuzz_groupby_cpu.py counts, without a GPU, which boundaries the
seeds reach and which mistakes they would catch).  Each plan's table must equal
the reference (fq_ref's arithmetic for the key, argument and predicate chains,
a stable sort and reduceat on the host) and every other plan's, key for key and
bit for bit: integer states exactly, Float64 sums exactly (the generator keeps
a Float64 sum only where it is exact in any order), Float64 max / min by bits
with NaN equal to NaN and a zero whose sign DESIGN.md section 4 leaves open by
value.  A seed whose kept rows divide by zero must raise "Divide by zero error"
from count() on every plan; no plan may report a full table (the capacities
come from the host's group count).  FQ_FUZZ_SCALE=k runs k times the seeds, as
tests/test_fuzz_typed_gpu.py does."""
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E = None
U = None


def setup_module():
    global E, U
    from fq_amd import abi, ops
    ops.require_gpu()
    from fq_amd.engine import Engine
    U = abi.DT_UINT64
    E = Engine()


def teardown_module():
    if E is not None:
        E.close()


def chain_sql(steps):
    s = "number"
    for op, v in steps:
        s = "(%s %s %d)" % (s, op, v)
    return s


def gen_key(rng):
    d = rng.choice([3, 8, 64, 100, 1000, 4096, 70000])
    m = rng.choice([7, 1000, 5000, 65536, 100003, 200000])
    a = rng.choice([3, 7])
    c = rng.choice([1, 12345])
    shape = rng.choice(["mod", "div", "divmod", "muldivmod", "adddivmod", "modmul"])
    return {"mod": [("%", m)], "div": [("/", max(d, 64))], "divmod": [("/", d), ("%", m)],
            "muldivmod": [("*", a), ("/", d), ("%", m)], "adddivmod": [("+", c), ("/", d), ("%", m)],
            "modmul": [("%", min(m, 5000)), ("*", a)]}[shape]


@pytest.mark.parametrize("seed", range(16))
def test_random_group_by_at_scale_matches_c_oracle(seed):
    import oracle_c
    from fq_amd import abi
    from fq_amd.expr import chain, predicate
    rng = random.Random(0x6B00 + seed)
    n = rng.choice([4_000_000, 12_000_000, 40_000_000])
    key_steps = gen_key(rng)
    aggs_sql, aggs = [], []
    for _ in range(rng.randint(1, 4)):
        kind = rng.choice(["count", "sum", "max", "min"])
        vsteps = rng.choice([[], [("+", 1)], [("*", 3)], [("%", 1000)]])
        aggs_sql.append("%s(%s)" % (kind, chain_sql(vsteps)))
        op = {"count": abi.AGG_COUNT, "sum": abi.AGG_SUM, "max": abi.AGG_MAX, "min": abi.AGG_MIN}[kind]
        aggs.append((op, U, chain(U, vsteps)[0] if vsteps else None))
    pred, where = None, ""
    if rng.random() < 0.5:
        p, q = rng.choice([(5, 3), (8, 3), (97, 50)])
        pred = predicate(U, [("%", p)], "<", q)
        where = " WHERE number %% %d < %d" % (p, q)
    k = chain_sql(key_steps)
    sql = "SELECT %s, %s FROM system.numbers_mt(%d)%s GROUP BY %s" % (k, ", ".join(aggs_sql), n, where, k)
    got = [tuple(r) for r in E.execute(sql).rows]
    keys, st = oracle_c.numbers_group(n, chain(U, key_steps)[0], aggs, pred=pred, threads=8, cap_groups=1 << 21)
    o = np.argsort(keys)
    exp = [(int(kk),) + tuple(int(x) for x in s) for kk, s in zip(keys[o], st[o])]
    assert len(got) == len(exp), (sql, len(got), len(exp))
    assert got == exp, (sql, [g for g, e in zip(got, exp) if g != e][:3])


# ---- the kernels on every path, under small and default launch-shape knobs (tests/fuzz_groupby.py) ----
import fuzz_groupby as G  # noqa: E402
from fq_amd._lib import FQError  # noqa: E402

SCALE = max(1, int(os.environ.get("FQ_FUZZ_SCALE", "1")))
SEEDS = range(32 * SCALE)


@pytest.fixture(autouse=True, scope="module")
def _knobs_never_leak():
    from fq_amd import ops
    yield
    ops.tune_reset()


@pytest.fixture(scope="module")
def dev():
    """(ops, the device's compute units)"""
    import torch
    from fq_amd import ops
    return ops, torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("seed", SEEDS)
def test_every_plan_equals_the_reference_and_the_other_plans(dev, seed):
    ops, cus = dev
    c = G.generate(seed, cus)
    outcome = c.expected()
    tables = []
    G.apply_knobs(ops, c.knobs)  # the seed's knobs, for this test only
    try:
        for plan in c.plans:
            what = "%s | %r" % (c.describe(), plan)
            if outcome[0] == "err":
                with pytest.raises(FQError) as e:
                    G.execute(ops, c.q, plan)
                assert str(e.value) == G.DIV_ZERO, (what, str(e.value))
                continue
            try:
                got = G.execute(ops, c.q, plan)
            except FQError as e:  # FQ_E_TABLE_FULL among them: the capacity holds twice the groups
                pytest.fail("%s: %s" % (what, e))
            diff = G.same(got, outcome[1])
            assert diff is None, (what, diff)
            tables.append((plan, got))
    finally:
        ops.tune_reset()
    for plan, got in tables[1:]:
        diff = G.tables_equal(tables[0][1], got, outcome[1])
        assert diff is None, (c.describe(), tables[0][0], plan, diff)


def test_group_knobs_are_back_at_their_defaults(dev):
    ops, _ = dev
    assert {k: ops.tune_get(k) for k in G.DEFAULTS} == G.DEFAULTS
