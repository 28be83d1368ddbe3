"""Times the Filter -> Projection block stream over nullable columns against
its typed twin on the same build (profiles/r19_project_nullable.json).

Statement: SELECT price * discount, quantity WHERE shipdate < k and quantity < q
over the Q6 layout (price Float64, discount Float32, shipdate Int32, quantity
UInt8), 2^27 rows in blocks of 10,000, 3/8 of the rows kept.  Legs, each 20
event-timed calls in this one process after 3 warm-up calls:
  1  fq_filter_project_blocks_typed
  2  fq_filter_project_blocks_nullable, four all-ones bitmaps
  3  the same with 10 % nulls per column
  4  quantity's bitmap alone (10 % nulls)
A call is timed from before its memsets to after its result copy (the calls
synchronise the stream themselves).  Reported per leg: median [min .. max] ms,
the time over leg 1's median, and the same ratio of bytes moved (17 B per row
and 1 bit per row and bitmap read; 9 B and 2 bits per kept row written; the
bitmaps' zeroing).

python tools/bench_project_nullable.py [--rows N] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fuse-query_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 27)
    ap.add_argument("--block-rows", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch

    from fq_amd import abi, ops
    from fq_amd._lib import check, lib
    from fq_amd.expr import Col, chain_columns, load, pred_tree_columns

    ops.require_gpu()
    n, B = a.rows, a.block_rows
    F64, F32, I32, U8 = abi.DT_FLOAT64, abi.DT_FLOAT32, abi.DT_INT32, abi.DT_UINT8
    dts = [F64, F32, I32, U8]
    rng = np.random.default_rng(19)
    host = [rng.uniform(1.0, 1000.0, n), (rng.integers(0, 11, n) / 100.0).astype(np.float32),
            rng.integers(8000, 10600, n).astype(np.int32), rng.integers(1, 51, n).astype(np.uint8)]
    cols = [ops.from_numpy(h, dt) for h, dt in zip(host, dts)]
    pred = pred_tree_columns(dts, [([load(2)], "<", (9950, "Int32")), ([load(3)], "<", (26, "UInt8"))], [0, 1, "and"])
    values = [chain_columns(dts, [("*", Col(1))])[0], chain_columns(dts, [load(3)])[0]]
    exprs = ops._project_exprs(values, dts[0])
    nw = (n + 63) // 64

    def bitmap(p_null, seed):
        if p_null == 0:
            return ops.from_numpy(np.full(nw, ~np.uint64(0)), abi.DT_UINT64)
        bits = np.ones(nw * 64, bool)
        bits[:n] = np.random.default_rng(seed).random(n) >= p_null
        return ops.from_numpy(np.packbits(bits, bitorder="little").view(np.uint64), abi.DT_UINT64)

    outs = [ops.empty_column(n, F64), ops.empty_column(n, U8)]
    outv = [ops.empty_column(nw, abi.DT_UINT64) for _ in outs]
    ptrs = (C.c_void_p * 2)(*[o.ptr for o in outs])
    vptrs = (C.c_void_p * 2)(*[o.ptr for o in outv])
    nb = -(-n // B)
    counts = ops.Workspace(8 * nb)
    ws = ops.Workspace(lib.fq_filter_project_blocks_workspace_bytes())
    arr = (abi.fq_col * 4)(*[c.col() for c in cols])
    stream = ops._stream()
    kept = C.c_int64(0)

    def typed():
        check(lib.fq_filter_project_blocks_typed(arr, 4, B, C.byref(pred), exprs, 2, ptrs, counts.ptr, C.byref(kept), ws.ptr,
                                                 ws.nbytes, stream))

    def nullable(vbs):
        vb = (C.c_void_p * 4)(*[None if v is None else v.ptr for v in vbs])

        def run():
            check(lib.fq_filter_project_blocks_nullable(arr, vb, 4, B, C.byref(pred), exprs, 2, ptrs, vptrs, counts.ptr,
                                                        C.byref(kept), ws.ptr, ws.nbytes, stream))
        return run

    ones = [bitmap(0, 0) for _ in range(4)]
    tenth = [bitmap(0.1, 100 + j) for j in range(4)]
    legs = [("1 typed", typed, 0), ("2 nullable, four all-ones bitmaps", nullable(ones), 4),
            ("3 nullable, 10 % nulls per column", nullable(tenth), 4),
            ("4 nullable, quantity's bitmap alone (10 % nulls)", nullable([None, None, None, tenth[3]]), 1)]
    result = {"rows": n, "block_rows": B, "reps": a.reps, "device": torch.cuda.get_device_name(0), "legs": []}
    base_ms = base_bytes = None
    for name, fn, nbm in legs:
        for _ in range(3):
            fn()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        k = kept.value
        nbytes = 17 * n + 9 * k + (n // 8) * nbm + (2 * (k // 8) + 2 * (n // 8) if nbm or "nullable" in name else 0)
        med = float(np.median(ms))
        if base_ms is None:
            base_ms, base_bytes = med, nbytes
        leg = {"leg": name, "kept": k, "ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "bytes": nbytes,
               "time_over_leg1": med / base_ms, "bytes_over_leg1": nbytes / base_bytes,
               "GBps": nbytes / med / 1e6}
        result["legs"].append(leg)
        print(json.dumps(leg), flush=True)
    lo, hi = result["legs"][0]["ms_min"], result["legs"][0]["ms_max"]
    result["leg1_spread_over_median"] = (hi - lo) / base_ms
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
