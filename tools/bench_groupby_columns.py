"""Times fq_group_aggregate_columns against fq_group_aggregate on the same
build (profiles/r20_groupby_columns.json).

One process, 2^27 rows, per leg 3 warm-up launches and then 20 event-timed
ones; the table is re-initialised before every launch, outside the timed
region.  Legs:
  1  fq_group_aggregate, one UInt64 column a: key a % 1000; count, sum(a), max(a)
     (bench.py's g1 shape, the yardstick)
  2  _columns over a, b: key a % 1000; count, sum(b), max(b)
  3  _columns over a, b, c (c Float64): key a % 1000; count, sum(b * c), max(b)
     WHERE c < k keeping 3/8 of the rows
  4  _columns over a, b with a holding 4 distinct values in random order:
     key a; count, sum(b)  (the Q1 key shape: 64 lanes meet 4 LDS slots)
Reported per leg: median [min .. max] ms, TB/s and its share of 8 TB/s on 8 K
bytes per row, and for legs 2-4 the time per byte over leg 1's.  The VGPRs,
SGPRs, LDS and scratch bytes of the three _columns kernels come from the
metadata of the code objects hipRTC produced (llvm-readelf --notes).

python tools/bench_groupby_columns.py [--rows N] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fuse-query_amd")]
PEAK_TBPS = 8.0


def kernel_resources(co_path):
    """{vgprs, sgprs, lds_bytes, scratch_bytes, *_spills} of fq_jit_groupby_cols in a code object"""
    readelf = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")
    notes = subprocess.run([readelf, "--notes", co_path], check=True, capture_output=True, text=True).stdout
    out = {}
    for block in notes.split("- .agpr_count")[1:]:
        if ".name:           fq_jit_groupby_cols" not in block:
            continue
        for field, name in ((".vgpr_count", "vgprs"), (".sgpr_count", "sgprs"), (".group_segment_fixed_size", "lds_bytes"),
                            (".private_segment_fixed_size", "scratch_bytes"), (".vgpr_spill_count", "vgpr_spills"),
                            (".sgpr_spill_count", "sgpr_spills")):
            m = re.search(re.escape(field) + r":\s+(\d+)", block)
            out[name] = int(m.group(1)) if m else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 27)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch

    from fq_amd import abi, ops
    from fq_amd._lib import check, lib
    from fq_amd.expr import STACK, chain, chain_columns, load, predicate_columns, push

    ops.require_gpu()
    n = a.rows
    U, F = abi.DT_UINT64, abi.DT_FLOAT64
    rng = np.random.default_rng(20)
    da = ops.from_numpy(rng.integers(0, 1 << 64, n, dtype=np.uint64), U)
    db = ops.from_numpy(rng.integers(0, 1 << 40, n, dtype=np.uint64), U)
    dc = ops.from_numpy(rng.integers(0, 8, n).astype(np.float64), F)       # c < 3 keeps 3/8 of the rows
    d4 = ops.from_numpy(rng.integers(0, 4, n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15), U)
    stream = ops._stream()
    dump = tempfile.mkdtemp(prefix="fq_groupby_columns_")

    def leg(name, n_cols, aggs, launch):
        t = ops.GroupTable(2048, aggs, U)
        before = set(os.listdir(dump))
        lib.fq_tune_jit_dump_dir(dump.encode())
        try:
            launch(t)  # compiles the shape
        finally:
            lib.fq_tune_jit_dump_dir(None)
        new = sorted(f for f in set(os.listdir(dump)) - before if f.endswith(".co"))
        for _ in range(3):
            check(lib.fq_group_table_init(C.byref(t.desc), stream))
            launch(t)
        ms = []
        for _ in range(a.reps):
            check(lib.fq_group_table_init(C.byref(t.desc), stream))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch(t)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        groups = t.count()
        med, nbytes = float(np.median(ms)), 8 * n_cols * n
        out = {"leg": name, "columns": n_cols, "groups": groups, "ms_median": med, "ms_min": min(ms), "ms_max": max(ms),
               "bytes": nbytes, "TBps": nbytes / med / 1e9, "share_of_8TBps": nbytes / med / 1e9 / PEAK_TBPS}
        if n_cols > 1 and new:
            out["kernel"] = kernel_resources(os.path.join(dump, new[-1]))
        return out

    agg3 = [(abi.AGG_COUNT, U), (abi.AGG_SUM, U), (abi.AGG_MAX, U)]
    k1 = chain(U, [("%", 1000)])[0]
    k2 = chain_columns([U, U], [("%", 1000)])[0]
    b2 = chain_columns([U, U], [load(1)])[0]
    dts3 = [U, U, F]
    k3 = chain_columns(dts3, [("%", 1000)])[0]
    b3 = chain_columns(dts3, [load(1)])[0]
    bc = chain_columns(dts3, [load(1), push(2), ("*", STACK, True)])[0]
    p3 = predicate_columns(dts3, [load(2)], "<", 3.0)
    legs = [
        ("1 fq_group_aggregate: a % 1000; count, sum(a), max(a)", 1, agg3,
         lambda t: t.aggregate(da, None, k1, [None, None, None])),
        ("2 _columns K=2: a % 1000; count, sum(b), max(b)", 2, agg3,
         lambda t: t.aggregate_columns([da, db], None, k2, [None, b2, b2])),
        ("3 _columns K=3: a % 1000; count, sum(b*c), max(b) WHERE c < k (3/8 kept)", 3,
         [(abi.AGG_COUNT, U), (abi.AGG_SUM, F), (abi.AGG_MAX, U)],
         lambda t: t.aggregate_columns([da, db, dc], p3, k3, [None, bc, b3])),
        ("4 _columns K=2: 4 distinct keys in random order; count, sum(b)", 2, [(abi.AGG_COUNT, U), (abi.AGG_SUM, U)],
         lambda t: t.aggregate_columns([d4, db], None, None, [None, b2])),
    ]
    result = {"rows": n, "reps": a.reps, "device": torch.cuda.get_device_name(0), "legs": []}
    base = None
    for name, n_cols, aggs, launch in legs:
        r = leg(name, n_cols, aggs, launch)
        if base is None:
            base = r
        else:
            r["ms_per_byte_over_leg1"] = (r["ms_median"] / r["bytes"]) / (base["ms_median"] / base["bytes"])
        result["legs"].append(r)
        print(json.dumps(r), flush=True)
    # by bytes alone leg 2 costs 2 x leg 1: is its median within leg 1's own spread of that?
    l1, l2 = result["legs"][0], result["legs"][1]
    result["leg2_within_twice_leg1_spread"] = bool(2 * l1["ms_min"] <= l2["ms_median"] <= 2 * l1["ms_max"])
    result["leg1_spread_over_median"] = (l1["ms_max"] - l1["ms_min"]) / l1["ms_median"]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
