"""fq_filter_project_blocks_for32 against fq_filter_project_blocks, called directly (no engine): the p1 shape
(`number+1, number/2 WHERE (number%8)<3`, 10,000-row blocks) over one numbers_mt device block of 3.125e8 rows and
over a window of it that starts inside a frame.  The two calls alternate in one process, each timed with a HIP event
pair around the whole call (its host sync for the kept-row count included, on both sides alike); every call is
checked against the closed-form kept count, and the two calls' outputs are compared once.  Prints one JSON line.

usage: python tools/bench_for32_project.py [--rows N] [--rounds R] [--warmup W]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fuse-query_amd"))

import torch  # noqa: E402

from fq_amd import abi, ops  # noqa: E402
from fq_amd._lib import check, lib  # noqa: E402
from fq_amd.expr import chain, predicate  # noqa: E402

HBM_PEAK = 8e12
F = abi.FOR32_FRAME_ROWS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=3.125e8)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    n_enc, B, begin = int(a.rows), 10_000, 1_250_000_000
    ops.require_gpu()
    U64 = abi.DT_UINT64
    pred, values = predicate(U64, [("%", 8)], "<", 3), [chain(U64, [("+", 1)])[0], chain(U64, [("/", 2)])[0]]
    exprs = ops._project_exprs(values, abi.DT_UINT64)
    col = ops.numbers_column(begin, n_enc)
    enc, ok = ops.for32_encode(col)
    assert ok
    outs = [[torch.zeros(n_enc, dtype=torch.int64, device="cuda") for _ in range(2)] for _ in range(2)]
    counts = torch.empty(-(-n_enc // B), dtype=torch.int64, device="cuda")
    ws = ops.Workspace(lib.fq_filter_project_blocks_workspace_bytes())
    st = ops._stream()

    def call(path, first, n):
        ptrs = (C.c_void_p * 2)(*[o.data_ptr() for o in outs[path]])
        kept = C.c_int64(0)
        if path:
            check(lib.fq_filter_project_blocks_for32(C.c_void_p(enc.delta.ptr), C.c_void_p(enc.base.ptr), first, n, B,
                                                     C.byref(pred), exprs, 2, ptrs, C.c_void_p(counts.data_ptr()),
                                                     C.byref(kept), ws.ptr, ws.nbytes, st))
        else:
            c = abi.fq_col(C.c_void_p(col.ptr + 8 * first), n, abi.DT_UINT64, 0)
            check(lib.fq_filter_project_blocks(C.byref(c), B, C.byref(pred), exprs, 2, ptrs,
                                               C.c_void_p(counts.data_ptr()), C.byref(kept), ws.ptr, ws.nbytes, st))
        return kept.value

    res = {"what": "fq_filter_project_blocks (plain, 8 B per row read) against fq_filter_project_blocks_for32 (4 B per "
                   "row read), direct calls alternating in one process, p1 shape, 10,000-row blocks; ms per call from "
                   "a HIP event pair around the call, host sync included", "rounds": a.rounds, "windows": []}
    for first in (0, 70_000):
        n = n_enc - first
        x0 = begin + first
        want = sum((n - ((r - x0) % 8) + 7) // 8 for r in range(3))
        ms = [[], []]
        for r in range(a.warmup + a.rounds):
            for path in (0, 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                kept = call(path, first, n)
                e1.record()
                e1.synchronize()
                assert kept == want, (path, kept, want)
                if r >= a.warmup:
                    ms[path].append(e0.elapsed_time(e1))
        assert all(torch.equal(x[:n], y[:n]) for x, y in zip(outs[0], outs[1]))  # same blocks, rows past counts too
        frames = ((first + n - 1) >> 16) - (first >> 16) + 1
        nbytes = [8 * n + 16 * want, 4 * n + 8 * frames + 16 * want]
        w = {"first": first, "rows": n, "kept": want}
        for path, name in ((0, "plain"), (1, "for32")):
            v = sorted(ms[path])
            med = v[len(v) // 2]
            w[name] = {"ms_median": round(med, 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4),
                       "algorithmic_bytes": nbytes[path],
                       "hbm_share_of_8TBps_at_median": round(nbytes[path] / (med * 1e-3) / HBM_PEAK, 4)}
        w["plain_over_for32"] = round(w["plain"]["ms_median"] / w["for32"]["ms_median"], 3)
        res["windows"].append(w)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
