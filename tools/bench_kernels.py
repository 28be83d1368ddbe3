#!/usr/bin/env python3
"""Per-kernel HBM roofline of every C-ABI kernel on one MI355X, at the size of
one numbers_mt partition (1.25e9 u64 rows = 10 GB at N = 1e10).

Each entry point is called raw through include/fq_gpu.h (no flag buffer, so
no host sync), timed with HIP events on the stream it is launched on, median
of R repetitions; achieved GB/s = algorithmic bytes / time.  Results are
checked against numpy on a prefix.  Prints one JSON document.

usage: python tools/bench_kernels.py [--rows 1.25e9] [--reps 10] > gpurun_out/kernels.json
       python tools/bench_kernels.py --only q6 [--q6-rows 134217728] [--reps 20]   (the q6 lines alone)
       python tools/bench_kernels.py --only pcols [--q6-rows 134217728] [--reps 20]   (Filter -> Projection over 3 columns)
       python tools/bench_kernels.py --only typed [--q6-rows 134217728] [--reps 20]   (the Q6 shape over narrow columns)
       python tools/bench_kernels.py --only ptyped [--q6-rows 134217728] [--reps 20]   (Filter -> Projection over them)
       python tools/bench_kernels.py --only nullable [--q6-rows 134217728] [--reps 20]   (the Q6 shape with validity bitmaps)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fuse-query_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fq_amd import abi, ops  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knobs  # noqa: E402
knobs.apply_env()
from fq_amd._lib import check, lib  # noqa: E402
from fq_amd.expr import chain, predicate  # noqa: E402

PEAK = 8000.0  # GB/s, MI355X HBM3E spec


def timed(fn, reps):
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()  # warm (and JIT compile)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0.record(s)
        fn()
        e1.record(s)
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def timed_all(fn, reps, warm=3):
    """every sample (ms) of `reps` event-timed calls after `warm` untimed ones"""
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0.record(s)
        fn()
        e1.record(s)
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def q6_lines(n, reps, st, res):
    """q6 sum(a*b) where c<k, 3 u64 columns: ONE fq_aggregate_columns scan (24 B/row), beside the
    single-column scans timed in the same process and the unfused path for the same statement (what
    engine/functions.cpp AggregatorFunction::summarize runs when the shape does not fuse: fq_compare,
    a bitmap probe scan, fq_filter_compact of every column, fq_arith on the kept rows, an identity
    scan), every launch event-timed."""
    from fq_amd.expr import Col, chain_columns, load, predicate_columns
    U = abi.DT_UINT64
    k38 = (3 * 2**64) // 8  # keeps ~3/8 of the rows
    c, a, b = (ops.splitmix_column(seed, 0, n) for seed in (101, 102, 103))
    dts = [U, U, U]
    pred = predicate_columns(dts, [], "<", k38)
    value, _ = chain_columns(dts, [load(1), ("*", Col(2))])
    cols = (abi.fq_col * 3)(c.col(), a.col(), b.col())
    aws = ops.Workspace(lib.fq_aggregate_workspace_bytes(n))
    dst = torch.empty(48, dtype=torch.uint8, device="cuda")
    SC = abi.AGG_SUM | abi.AGG_COUNT

    def rec(name, ts, nbytes, note=""):
        ms = statistics.median(ts)
        gbps = nbytes / (ms * 1e-3) / 1e9
        res.append({"kernel": name, "ms": ms, "ms_min": min(ts), "ms_max": max(ts), "reps": len(ts),
                    "algorithmic_bytes": nbytes, "achieved_gbps": gbps, "frac_of_peak": gbps / PEAK, "note": note})
        print("%-58s %8.3f ms [%.3f .. %.3f]  %7.0f GB/s  %4.1f %%" % (name, ms, min(ts), max(ts), gbps,
                                                                     100 * gbps / PEAK), file=sys.stderr)
        return ms

    def fused(br, mask):
        check(lib.fq_aggregate_columns(cols, 3, br, C.byref(pred), C.byref(value), mask,
                                       C.c_void_p(dst.data_ptr()), aws.ptr, aws.nbytes, st))

    def single(col, p, v, mask, br):
        cc = col.col()
        check(lib.fq_aggregate(C.byref(cc), br, C.byref(p), C.byref(v), mask, C.c_void_p(dst.data_ptr()), aws.ptr,
                               aws.nbytes, st))

    f_flat = rec("q6 sum(a*b) where c<k, 3 u64 columns", timed_all(lambda: fused(0, SC), reps), 24 * n,
                 "one DataBlock (block_rows 0): flat scan")
    got = ops.state_from_device(dst)
    hc, ha, hb = (x.to_numpy() for x in (c, a, b))
    keep = hc < np.uint64(k38)
    with np.errstate(over="ignore"):
        want = int((ha[keep] * hb[keep]).sum(dtype=np.uint64))
    assert got.count == int(keep.sum()) and got.sum == want and got.flags == 0, (got.count, got.sum, want)
    rec("q6 max(a*b) where c<k, 3 u64 columns", timed_all(lambda: fused(10000, abi.AGG_MAX | abi.AGG_COUNT), reps),
        24 * n, "flat scan, as the single-column C4 line")
    f_blk = rec("q6 sum(a*b) where c<k, 3 u64 columns, 10,000-row blocks",
                timed_all(lambda: fused(10000, SC), reps), 24 * n, "block mode: one wave per reference block")
    got = ops.state_from_device(dst)
    assert got.count == int(keep.sum()) and got.sum == want and got.flags == 0
    v1, _ = chain(U, [("+", 1)])
    p1 = predicate(U, [("%", 8)], "<", 3)
    rec("single column: max(x+1) where x%8<3", timed_all(lambda: single(a, p1, v1, abi.AGG_MAX | abi.AGG_COUNT, 10000),
                                                         reps), 8 * n, "C4 shape, flat scan, same process")
    rec("single column: sum(x+1) where x%8<3, 10,000-row blocks",
        timed_all(lambda: single(a, p1, v1, SC, 10000), reps), 8 * n, "block mode, same process")

    # the unfused path for the same statement (this tree, what runs with the JIT off)
    bm = ops.empty_column(n, abi.DT_BOOLEAN)
    kc, ka, kb, prod = (ops.empty_column(n, U) for _ in range(4))
    fws = ops.Workspace(lib.fq_filter_workspace_bytes(n))
    bound = abi.fq_value(U, 1, k38)
    kept = C.c_int64(0)
    pb = abi.fq_pred()
    pb.kind = abi.PRED_BITMAP
    pb.bitmap = bm.ptr
    cc = c.col()

    def unfused():
        check(lib.fq_compare(abi.CMP_BY_SYM["<"], C.byref(cc), None, None, C.byref(bound), C.c_void_p(bm.ptr), n,
                             None, st))
        check(lib.fq_aggregate(C.byref(cc), 0, C.byref(pb), None, SC, C.c_void_p(dst.data_ptr()), aws.ptr,
                               aws.nbytes, st))
        for src, out in ((c, kc), (a, ka), (b, kb)):
            sc = src.col()
            check(lib.fq_filter_compact(C.byref(sc), C.c_void_p(bm.ptr), C.c_void_p(out.ptr), C.byref(kept), fws.ptr,
                                        fws.nbytes, st))
        m = kept.value
        lc = abi.fq_col(C.c_void_p(ka.ptr), m, U, 0)
        rc = abi.fq_col(C.c_void_p(kb.ptr), m, U, 0)
        oc = abi.fq_col(C.c_void_p(prod.ptr), m, U, 0)
        check(lib.fq_arith(abi.OP_BY_SYM["*"], C.byref(lc), None, C.byref(rc), None, C.byref(oc), None, st))
        check(lib.fq_aggregate(C.byref(oc), 0, None, None, SC, C.c_void_p(dst.data_ptr()), aws.ptr, aws.nbytes, st))

    ts = timed_all(unfused, reps)
    m = kept.value
    got = ops.state_from_device(dst)
    assert got.count == int(keep.sum()) == m and got.sum == want
    moved = (8 * n + n // 8) * 2 + 3 * (8 * n + n // 8 + 8 * m) + 24 * m + 8 * m
    u = rec("q6 unfused: compare, probe, 3 compactions, arith, scan", ts, moved,
            "this tree with the JIT off; includes fq_filter_compact's host syncs; bytes = what the path moves")
    res.append({"q6_fused_over_unfused": {"flat": u / f_flat, "block_mode": u / f_blk,
                                          "bytes_ratio": moved / (24 * n)}})


def pcols_lines(n, reps, st, res):
    """SELECT a*b, a+c WHERE c < 3<<61 over 3 u64 splitmix columns: ONE fq_filter_project_blocks_columns /
    fq_filter_project_columns launch (24 B read + 16 B written per kept row), beside -- in the same process -- the
    unfused path for the same statement (what ProjectionTransform runs when the shape does not fuse:
    fq_compare, fq_filter_compact of every column, fq_arith per expression node on the kept rows) and the
    single-column p1 shape through fq_filter_project_blocks.  Every launch event-timed; the entry points
    synchronise their stream for the kept-row count, so each sample holds that host sync too."""
    from fq_amd.expr import Col, chain_columns, load, predicate_columns
    U = abi.DT_UINT64
    k38 = 3 << 61
    c, a, b = (ops.splitmix_column(seed, 0, n) for seed in (101, 102, 103))
    dts = [U, U, U]
    pred = predicate_columns(dts, [], "<", k38)
    vals = (abi.fq_expr * 2)(chain_columns(dts, [load(1), ("*", Col(2))])[0], chain_columns(dts, [load(1), ("+", Col(0))])[0])
    cols = (abi.fq_col * 3)(c.col(), a.col(), b.col())
    o0, o1 = ops.empty_column(n, U), ops.empty_column(n, U)
    outs = (C.c_void_p * 2)(o0.ptr, o1.ptr)
    B = 10000
    nb = -(-n // B)
    counts = ops.Workspace(8 * nb)
    bws = ops.Workspace(lib.fq_filter_project_blocks_workspace_bytes())
    cws = ops.Workspace(lib.fq_filter_project_columns_workspace_bytes(n, 3))
    kept = C.c_int64(0)

    def rec(name, ts, nbytes, note=""):
        ms = statistics.median(ts)
        gbps = nbytes / (ms * 1e-3) / 1e9
        res.append({"kernel": name, "ms": ms, "ms_min": min(ts), "ms_max": max(ts), "reps": len(ts),
                    "algorithmic_bytes": nbytes, "achieved_gbps": gbps, "frac_of_peak": gbps / PEAK,
                    "frac_of_peak_min_max": [nbytes / (max(ts) * 1e-3) / 1e9 / PEAK, nbytes / (min(ts) * 1e-3) / 1e9 / PEAK],
                    "note": note})
        print("%-58s %8.3f ms [%.3f .. %.3f]  %7.0f GB/s  %4.1f %%" % (name, ms, min(ts), max(ts), gbps,
                                                                     100 * gbps / PEAK), file=sys.stderr)
        return ms

    def blocks():
        check(lib.fq_filter_project_blocks_columns(cols, 3, B, C.byref(pred), vals, 2, outs, counts.ptr, C.byref(kept),
                                                   bws.ptr, bws.nbytes, st))

    def contiguous():
        check(lib.fq_filter_project_columns(cols, 3, C.byref(pred), vals, 2, outs, C.byref(kept), cws.ptr, cws.nbytes, st))

    hc, ha, hb = (x.to_numpy() for x in (c, a, b))
    keep = hc < np.uint64(k38)
    m = int(keep.sum())
    with np.errstate(over="ignore"):
        w0, w1 = ha[keep] * hb[keep], ha[keep] + hc[keep]
    ts = timed_all(blocks, reps)
    assert kept.value == m
    cnt = counts.buf[:8 * nb].view(torch.int64).cpu().numpy()
    k0 = int(cnt[0])
    assert k0 == int(keep[:B].sum()) and np.array_equal(o0.to_numpy()[:k0], w0[:k0]) and np.array_equal(o1.to_numpy()[:k0], w1[:k0])
    f_blk = rec("pcols a*b, a+c where c<k, 3 u64 columns, 10,000-row blocks", ts, 24 * n + 16 * m,
                "fq_filter_project_blocks_columns")
    ts = timed_all(contiguous, reps)
    assert kept.value == m and np.array_equal(o0.to_numpy()[:m], w0) and np.array_equal(o1.to_numpy()[:m], w1)
    f_con = rec("pcols a*b, a+c where c<k, 3 u64 columns, contiguous", ts, 24 * n + 16 * m, "fq_filter_project_columns")

    # the unfused path for the same statement (this tree with the JIT off, the parent commit's only path)
    bm = ops.empty_column(n, abi.DT_BOOLEAN)
    kc, ka, kb = (ops.empty_column(n, U) for _ in range(3))
    fws = ops.Workspace(lib.fq_filter_workspace_bytes(n))
    bound = abi.fq_value(U, 1, k38)
    cc = c.col()

    def unfused():
        check(lib.fq_compare(abi.CMP_BY_SYM["<"], C.byref(cc), None, None, C.byref(bound), C.c_void_p(bm.ptr), n, None, st))
        for src, out in ((c, kc), (a, ka), (b, kb)):
            sc = src.col()
            check(lib.fq_filter_compact(C.byref(sc), C.c_void_p(bm.ptr), C.c_void_p(out.ptr), C.byref(kept), fws.ptr,
                                        fws.nbytes, st))
        k = kept.value
        for op, l, r, o in (("*", ka, kb, o0), ("+", ka, kc, o1)):
            lc, rc, oc = (abi.fq_col(C.c_void_p(x.ptr), k, U, 0) for x in (l, r, o))
            check(lib.fq_arith(abi.OP_BY_SYM[op], C.byref(lc), None, C.byref(rc), None, C.byref(oc), None, st))

    ts = timed_all(unfused, reps)
    assert kept.value == m and np.array_equal(o0.to_numpy()[:m], w0) and np.array_equal(o1.to_numpy()[:m], w1)
    moved = (8 * n + n // 8) + 3 * (8 * n + n // 8 + 8 * m) + 2 * 24 * m
    u = rec("pcols unfused: compare, 3 compactions, 2 arith", ts, moved,
            "six launches; includes fq_filter_compact's host syncs; bytes = what the path moves")

    # the single-column p1 shape: number+1, number/2 where number%8<3 (bench.py --query p1)
    p1 = predicate(U, [("%", 8)], "<", 3)
    v1 = (abi.fq_expr * 2)(chain(U, [("+", 1)])[0], chain(U, [("/", 2)])[0])
    ac = a.col()

    def single():
        check(lib.fq_filter_project_blocks(C.byref(ac), B, C.byref(p1), v1, 2, outs, counts.ptr, C.byref(kept), bws.ptr,
                                           bws.nbytes, st))

    ts = timed_all(single, reps)
    m1 = kept.value
    assert m1 == int((ha % np.uint64(8) < np.uint64(3)).sum())
    rec("single column p1: x+1, x/2 where x%8<3, 10,000-row blocks", ts, 8 * n + 16 * m1, "fq_filter_project_blocks, same process")
    res.append({"pcols_unfused_over_fused": {"block_stream": u / f_blk, "contiguous": u / f_con,
                                             "bytes_ratio": moved / (24 * n + 16 * m)},
                "gate_fused_below_unfused": bool(f_blk < u and f_con < u)})


def typed_lines(n, reps, st, res):
    """sum(price * discount) WHERE shipdate < k and quantity < q over price Float64, discount Float32,
    shipdate Int32, quantity UInt8 (17 B/row, about 3/8 of the rows kept): ONE fq_aggregate_typed scan,
    beside -- in the same process -- the same statement over the four columns widened to 64 bits through
    fq_aggregate_columns (32 B/row) and the unfused path (what engine/functions.cpp
    AggregatorFunction::summarize runs with the JIT off, the only path for this block before the typed scan:
    two fq_compare, fq_logic, a bitmap probe scan, fq_filter_compact of every column, fq_arith on the kept
    rows, an identity scan).  Every launch event-timed."""
    from fq_amd.expr import Col, chain_columns, load, pred_tree_columns
    F64, F32, I32, U8, I64, U64 = (abi.DT_FLOAT64, abi.DT_FLOAT32, abi.DT_INT32, abi.DT_UINT8, abi.DT_INT64,
                                   abi.DT_UINT64)
    K, Q = 9950, 26  # shipdate in [8000, 10600): 3/4 below K; quantity in [1, 50]: 1/2 below Q
    g = torch.Generator(device="cuda")
    g.manual_seed(9)
    t_price = torch.rand(n, dtype=torch.float64, device="cuda", generator=g) * 999.0 + 1.0
    t_disc = torch.randint(0, 11, (n,), device="cuda", generator=g).to(torch.float32) / 100.0
    t_ship = torch.randint(8000, 10600, (n,), dtype=torch.int32, device="cuda", generator=g)
    t_qty = torch.randint(1, 51, (n,), dtype=torch.uint8, device="cuda", generator=g)

    def column(t, dt):
        return ops.DeviceColumn(t.view(torch.uint8), n, dt)

    narrow = [column(t_price, F64), column(t_disc, F32), column(t_ship, I32), column(t_qty, U8)]
    ndts = [F64, F32, I32, U8]
    wide_t = [t_price, t_disc.to(torch.float64), t_ship.to(torch.int64), t_qty.to(torch.int64)]
    wdts = [F64, F64, I64, U64]
    wide = [column(t, dt) for t, dt in zip(wide_t, wdts)]

    def program(dts, kt, qt):
        pred = pred_tree_columns(dts, [([load(2)], "<", (K, kt)), ([load(3)], "<", (Q, qt))], [0, 1, "and"])
        value, vdt = chain_columns(dts, [("*", Col(1))])
        assert vdt == F64
        return pred, value

    npred, nvalue = program(ndts, "Int32", "UInt8")
    wpred, wvalue = program(wdts, "Int64", "UInt64")
    ncols = (abi.fq_col * 4)(*[c.col() for c in narrow])
    wcols = (abi.fq_col * 4)(*[c.col() for c in wide])
    aws = ops.Workspace(lib.fq_aggregate_workspace_bytes(n))
    dst = torch.empty(48, dtype=torch.uint8, device="cuda")
    SC = abi.AGG_SUM | abi.AGG_COUNT

    def rec(name, ts, nbytes, note=""):
        ms = statistics.median(ts)
        gbps = nbytes / (ms * 1e-3) / 1e9
        res.append({"kernel": name, "ms": ms, "ms_min": min(ts), "ms_max": max(ts), "reps": len(ts),
                    "algorithmic_bytes": nbytes, "achieved_gbps": gbps, "frac_of_peak": gbps / PEAK, "note": note})
        print("%-58s %8.3f ms [%.3f .. %.3f]  %7.0f GB/s  %4.1f %%" % (name, ms, min(ts), max(ts), gbps,
                                                                     100 * gbps / PEAK), file=sys.stderr)
        return ts

    keep = (t_ship < K) & (t_qty < Q)
    kept_rows = int(keep.sum())
    prod = t_price[keep] * t_disc[keep].to(torch.float64)
    want, scale = float(prod.sum()), float(prod.abs().sum())
    del prod

    def verify(what):
        got = ops.state_from_device(dst)
        s = ops.state_values(got)["sum"]
        assert got.count == kept_rows and got.flags == 0 and abs(s - want) <= 1e-12 * scale, (what, got.count, kept_rows, s, want)

    def typed(br):
        check(lib.fq_aggregate_typed(ncols, 4, br, C.byref(npred), C.byref(nvalue), SC, C.c_void_p(dst.data_ptr()),
                                     aws.ptr, aws.nbytes, st))

    def widened(br):
        check(lib.fq_aggregate_columns(wcols, 4, br, C.byref(wpred), C.byref(wvalue), SC, C.c_void_p(dst.data_ptr()),
                                       aws.ptr, aws.nbytes, st))

    t_flat = rec("typed q6 sum(price*discount), f64 f32 i32 u8 columns", timed_all(lambda: typed(0), reps), 17 * n,
                 "fq_aggregate_typed, one DataBlock (block_rows 0): flat scan, 17 B/row")
    verify("typed flat")
    t_blk = rec("typed q6, 10,000-row blocks", timed_all(lambda: typed(10000), reps), 17 * n,
                "fq_aggregate_typed, block mode: one wave per reference block")
    verify("typed blocks")
    w_flat = rec("widened q6, 4 64-bit columns", timed_all(lambda: widened(0), reps), 32 * n,
                 "fq_aggregate_columns over the columns widened to 64 bits, flat scan, 32 B/row")
    verify("widened flat")
    w_blk = rec("widened q6, 4 64-bit columns, 10,000-row blocks", timed_all(lambda: widened(10000), reps), 32 * n,
                "fq_aggregate_columns, block mode")
    verify("widened blocks")

    # the unfused path for the same statement over the narrow columns
    bm1, bm2, bm = (ops.empty_column(n, abi.DT_BOOLEAN) for _ in range(3))
    kept_cols = [ops.empty_column(n, dt) for dt in ndts]
    prod_col = ops.empty_column(n, F64)
    fws = ops.Workspace(lib.fq_filter_workspace_bytes(n))
    kv, qv = abi.fq_value(I32, 1, K), abi.fq_value(U8, 1, Q)
    kept = C.c_int64(0)
    pb = abi.fq_pred()
    pb.kind = abi.PRED_BITMAP
    pb.bitmap = bm.ptr
    sc, qc = narrow[2].col(), narrow[3].col()

    def unfused():
        lt = abi.CMP_BY_SYM["<"]
        check(lib.fq_compare(lt, C.byref(sc), None, None, C.byref(kv), C.c_void_p(bm1.ptr), n, None, st))
        check(lib.fq_compare(lt, C.byref(qc), None, None, C.byref(qv), C.c_void_p(bm2.ptr), n, None, st))
        check(lib.fq_logic(0, C.c_void_p(bm1.ptr), C.c_void_p(bm2.ptr), C.c_void_p(bm.ptr), n, st))
        check(lib.fq_aggregate(C.byref(sc), 0, C.byref(pb), None, SC, C.c_void_p(dst.data_ptr()), aws.ptr, aws.nbytes, st))
        for src, out in zip(narrow, kept_cols):
            c = src.col()
            check(lib.fq_filter_compact(C.byref(c), C.c_void_p(bm.ptr), C.c_void_p(out.ptr), C.byref(kept), fws.ptr,
                                        fws.nbytes, st))
        m = kept.value
        lc = abi.fq_col(C.c_void_p(kept_cols[0].ptr), m, F64, 0)
        rc = abi.fq_col(C.c_void_p(kept_cols[1].ptr), m, F32, 0)
        oc = abi.fq_col(C.c_void_p(prod_col.ptr), m, F64, 0)
        check(lib.fq_arith(abi.OP_BY_SYM["*"], C.byref(lc), None, C.byref(rc), None, C.byref(oc), None, st))
        check(lib.fq_aggregate(C.byref(oc), 0, None, None, SC, C.c_void_p(dst.data_ptr()), aws.ptr, aws.nbytes, st))

    ops.jit_config(abi.JIT_OFF, 0)
    try:
        ts = timed_all(unfused, reps)
    finally:
        ops.jit_config(abi.JIT_AUTO, 1 << 22)
    m = kept.value
    assert m == kept_rows
    verify("unfused")
    bits = n // 8
    moved = (4 * n + bits) + (n + bits) + 3 * bits + (4 * n + bits) + (17 * n + 4 * bits + 17 * m) + 20 * m + 8 * m
    u = rec("typed q6 unfused: 2 compare, and, probe, 4 compactions, arith, scan", ts, moved,
            "this block with the JIT off (the parent's only path); includes fq_filter_compact's host syncs; "
            "bytes = what the path moves")
    med = statistics.median
    res.append({"typed_q6": {
        "rows": n, "kept_rows": kept_rows, "bytes_per_row": {"typed": 17, "widened": 32},
        "typed_tb_per_s": {"flat": 17 * n / (med(t_flat) * 1e-3) / 1e12, "block_mode": 17 * n / (med(t_blk) * 1e-3) / 1e12},
        "unfused_over_typed": {"flat": med(u) / med(t_flat), "block_mode": med(u) / med(t_blk)},
        "widened_over_typed": {"flat": med(w_flat) / med(t_flat), "block_mode": med(w_blk) / med(t_blk)},
        "gate_typed_below_unfused_non_overlapping": bool(max(t_flat) < min(u) and max(t_blk) < min(u)),
        "typed_below_widened": {"flat": bool(med(t_flat) < med(w_flat)), "block_mode": bool(med(t_blk) < med(w_blk))}}})


def ptyped_lines(n, reps, st, res):
    """SELECT price * discount, quantity WHERE shipdate < k and quantity < q over price Float64, discount Float32,
    shipdate Int32, quantity UInt8 (17 B read + 9 B written per kept row, about 3/8 of the rows kept): ONE
    fq_filter_project_blocks_typed / fq_filter_project_typed launch, beside -- in the same process -- the same
    statement over the four columns widened to 64 bits through the *_columns entry points (32 B + 16 B per kept
    row) and the unfused path for the narrow block (what ProjectionTransform runs when the shape does not fuse,
    the parent commit's only path for it: two fq_compare, fq_logic, fq_filter_compact of the projected columns,
    fq_arith on the kept rows).  Every launch event-timed; the entry points synchronise their stream for the
    kept-row count, so each sample holds that host sync too."""
    from fq_amd.expr import Col, chain_columns, load, pred_tree_columns
    F64, F32, I32, U8, I64, U64 = (abi.DT_FLOAT64, abi.DT_FLOAT32, abi.DT_INT32, abi.DT_UINT8, abi.DT_INT64,
                                   abi.DT_UINT64)
    K, Q = 9950, 26  # shipdate in [8000, 10600): 3/4 below K; quantity in [1, 50]: 1/2 below Q
    g = torch.Generator(device="cuda")
    g.manual_seed(9)  # typed_lines' generator
    t_price = torch.rand(n, dtype=torch.float64, device="cuda", generator=g) * 999.0 + 1.0
    t_disc = torch.randint(0, 11, (n,), device="cuda", generator=g).to(torch.float32) / 100.0
    t_ship = torch.randint(8000, 10600, (n,), dtype=torch.int32, device="cuda", generator=g)
    t_qty = torch.randint(1, 51, (n,), dtype=torch.uint8, device="cuda", generator=g)

    def column(t, dt):
        return ops.DeviceColumn(t.view(torch.uint8), n, dt)

    narrow = [column(t_price, F64), column(t_disc, F32), column(t_ship, I32), column(t_qty, U8)]
    ndts = [F64, F32, I32, U8]
    wide_t = [t_price, t_disc.to(torch.float64), t_ship.to(torch.int64), t_qty.to(torch.int64)]
    wdts = [F64, F64, I64, U64]
    wide = [column(t, dt) for t, dt in zip(wide_t, wdts)]

    def program(dts, kt, qt):
        pred = pred_tree_columns(dts, [([load(2)], "<", (K, kt)), ([load(3)], "<", (Q, qt))], [0, 1, "and"])
        vals = (abi.fq_expr * 2)(chain_columns(dts, [("*", Col(1))])[0], chain_columns(dts, [load(3)])[0])
        assert vals[0].out_dtype == F64 and vals[1].out_dtype == dts[3]
        return pred, vals

    npred, nvals = program(ndts, "Int32", "UInt8")
    wpred, wvals = program(wdts, "Int64", "UInt64")
    ncols = (abi.fq_col * 4)(*[c.col() for c in narrow])
    wcols = (abi.fq_col * 4)(*[c.col() for c in wide])
    o_prod, o_qty, o_wqty = ops.empty_column(n, F64), ops.empty_column(n, U8), ops.empty_column(n, U64)
    nouts = (C.c_void_p * 2)(o_prod.ptr, o_qty.ptr)
    wouts = (C.c_void_p * 2)(o_prod.ptr, o_wqty.ptr)
    B = 10000
    nb = -(-n // B)
    counts = ops.Workspace(8 * nb)
    bws = ops.Workspace(lib.fq_filter_project_blocks_workspace_bytes())
    tws = ops.Workspace(lib.fq_filter_project_typed_workspace_bytes(n, ncols, 4))
    cws = ops.Workspace(lib.fq_filter_project_columns_workspace_bytes(n, 4))
    kept = C.c_int64(0)

    def rec(name, ts, nbytes, note=""):
        ms = statistics.median(ts)
        gbps = nbytes / (ms * 1e-3) / 1e9
        res.append({"kernel": name, "ms": ms, "ms_min": min(ts), "ms_max": max(ts), "reps": len(ts),
                    "algorithmic_bytes": nbytes, "achieved_gbps": gbps, "frac_of_peak": gbps / PEAK, "note": note})
        print("%-58s %8.3f ms [%.3f .. %.3f]  %7.0f GB/s  %4.1f %%" % (name, ms, min(ts), max(ts), gbps,
                                                                     100 * gbps / PEAK), file=sys.stderr)
        return ts

    keep = (t_ship < K) & (t_qty < Q)
    m = int(keep.sum())
    want_prod = (t_price[keep] * t_disc[keep].to(torch.float64)).view(torch.int64)
    want_qty = t_qty[keep]
    k0 = int(keep[:B].sum())

    def out_t(col, dtype, rows):
        return col.buf[col.offset:col.offset + rows * torch.empty(0, dtype=dtype).element_size()].view(dtype)

    def verify(what, qty_col, qty_dtype, rows):
        """the first `rows` output rows against torch (block geometry: block 0's kept rows)"""
        assert kept.value == m, (what, kept.value, m)
        assert torch.equal(out_t(o_prod, torch.int64, rows), want_prod[:rows]), what
        assert torch.equal(out_t(qty_col, qty_dtype, rows).to(torch.uint8), want_qty[:rows]), what

    def typed_blocks():
        check(lib.fq_filter_project_blocks_typed(ncols, 4, B, C.byref(npred), nvals, 2, nouts, counts.ptr, C.byref(kept),
                                                 bws.ptr, bws.nbytes, st))

    def typed_contiguous():
        check(lib.fq_filter_project_typed(ncols, 4, C.byref(npred), nvals, 2, nouts, C.byref(kept), tws.ptr, tws.nbytes, st))

    def wide_blocks():
        check(lib.fq_filter_project_blocks_columns(wcols, 4, B, C.byref(wpred), wvals, 2, wouts, counts.ptr, C.byref(kept),
                                                   bws.ptr, bws.nbytes, st))

    def wide_contiguous():
        check(lib.fq_filter_project_columns(wcols, 4, C.byref(wpred), wvals, 2, wouts, C.byref(kept), cws.ptr, cws.nbytes, st))

    t_blk = rec("ptyped price*discount, quantity, 10,000-row blocks", timed_all(typed_blocks, reps), 17 * n + 9 * m,
                "fq_filter_project_blocks_typed over f64 f32 i32 u8 columns: 17 B read + 9 B per kept row")
    verify("typed blocks", o_qty, torch.uint8, k0)
    assert int(counts.buf[:8].view(torch.int64)[0]) == k0
    t_con = rec("ptyped price*discount, quantity, contiguous", timed_all(typed_contiguous, reps), 17 * n + 9 * m,
                "fq_filter_project_typed (look-back kernel)")
    verify("typed contiguous", o_qty, torch.uint8, m)
    w_blk = rec("widened to 4 64-bit columns, 10,000-row blocks", timed_all(wide_blocks, reps), 32 * n + 16 * m,
                "fq_filter_project_blocks_columns: 32 B read + 16 B per kept row")
    verify("widened blocks", o_wqty, torch.int64, k0)
    w_con = rec("widened to 4 64-bit columns, contiguous", timed_all(wide_contiguous, reps), 32 * n + 16 * m,
                "fq_filter_project_columns")
    verify("widened contiguous", o_wqty, torch.int64, m)

    # the unfused path for the narrow block
    bm1, bm2, bm = (ops.empty_column(n, abi.DT_BOOLEAN) for _ in range(3))
    k_price, k_disc = ops.empty_column(n, F64), ops.empty_column(n, F32)
    fws = ops.Workspace(lib.fq_filter_workspace_bytes(n))
    kv, qv = abi.fq_value(I32, 1, K), abi.fq_value(U8, 1, Q)
    sc, qc = narrow[2].col(), narrow[3].col()

    def unfused():
        lt = abi.CMP_BY_SYM["<"]
        check(lib.fq_compare(lt, C.byref(sc), None, None, C.byref(kv), C.c_void_p(bm1.ptr), n, None, st))
        check(lib.fq_compare(lt, C.byref(qc), None, None, C.byref(qv), C.c_void_p(bm2.ptr), n, None, st))
        check(lib.fq_logic(0, C.c_void_p(bm1.ptr), C.c_void_p(bm2.ptr), C.c_void_p(bm.ptr), n, st))
        for src, out in ((narrow[0], k_price), (narrow[1], k_disc), (narrow[3], o_qty)):
            c = src.col()
            check(lib.fq_filter_compact(C.byref(c), C.c_void_p(bm.ptr), C.c_void_p(out.ptr), C.byref(kept), fws.ptr,
                                        fws.nbytes, st))
        k = kept.value
        lc = abi.fq_col(C.c_void_p(k_price.ptr), k, F64, 0)
        rc = abi.fq_col(C.c_void_p(k_disc.ptr), k, F32, 0)
        oc = abi.fq_col(C.c_void_p(o_prod.ptr), k, F64, 0)
        check(lib.fq_arith(abi.OP_BY_SYM["*"], C.byref(lc), None, C.byref(rc), None, C.byref(oc), None, st))

    ts = timed_all(unfused, reps)
    verify("unfused", o_qty, torch.uint8, m)
    bits = n // 8
    moved = (4 * n + bits) + (n + bits) + 3 * bits + (13 * n + 3 * bits + 13 * m) + 20 * m
    u = rec("ptyped unfused: 2 compare, and, 3 compactions, arith", ts, moved,
            "seven launches; includes fq_filter_compact's host syncs; bytes = what the path moves")
    med = statistics.median
    res.append({"project_typed_q6": {
        "rows": n, "kept_rows": m, "bytes": {"typed": 17 * n + 9 * m, "widened": 32 * n + 16 * m},
        "typed_tb_per_s": {"block_stream": (17 * n + 9 * m) / (med(t_blk) * 1e-3) / 1e12,
                           "contiguous": (17 * n + 9 * m) / (med(t_con) * 1e-3) / 1e12},
        "unfused_over_typed": {"block_stream": med(u) / med(t_blk), "contiguous": med(u) / med(t_con)},
        "widened_over_typed": {"block_stream": med(w_blk) / med(t_blk), "contiguous": med(w_con) / med(t_con),
                               "bytes_ratio": (32 * n + 16 * m) / (17 * n + 9 * m)},
        "typed_below_unfused_non_overlapping": bool(max(t_blk) < min(u) and max(t_con) < min(u)),
        "typed_below_widened": {"block_stream": bool(med(t_blk) < med(w_blk)), "contiguous": bool(med(t_con) < med(w_con))}}})


def nullable_lines(n, reps, st, res):
    """The Q6 statement of typed_lines (17 B/row, about 3/8 of the rows kept) with Arrow validity bitmaps,
    flat and in block mode, in ONE process: (1) fq_aggregate_typed without bitmaps, the yardstick; then
    fq_aggregate_nullable with (2) four bitmaps of all ones, (3) four bitmaps with 10 % seeded random nulls
    each, (4) a bitmap on quantity alone (all ones).  Algorithmic bytes: 17 B + 1/8 B per bitmap per row.
    Every launch event-timed; each leg's ratio is its median over leg 1's median."""
    from fq_amd.expr import Col, chain_columns, load, pred_tree_columns
    F64, F32, I32, U8, U64 = abi.DT_FLOAT64, abi.DT_FLOAT32, abi.DT_INT32, abi.DT_UINT8, abi.DT_UINT64
    K, Q = 9950, 26
    g = torch.Generator(device="cuda")
    g.manual_seed(9)  # typed_lines' generator
    t_price = torch.rand(n, dtype=torch.float64, device="cuda", generator=g) * 999.0 + 1.0
    t_disc = torch.randint(0, 11, (n,), device="cuda", generator=g).to(torch.float32) / 100.0
    t_ship = torch.randint(8000, 10600, (n,), dtype=torch.int32, device="cuda", generator=g)
    t_qty = torch.randint(1, 51, (n,), dtype=torch.uint8, device="cuda", generator=g)
    cols = [ops.DeviceColumn(t.view(torch.uint8), n, dt) for t, dt in zip((t_price, t_disc, t_ship, t_qty), (F64, F32, I32, U8))]
    dts = [F64, F32, I32, U8]
    pred = pred_tree_columns(dts, [([load(2)], "<", (K, "Int32")), ([load(3)], "<", (Q, "UInt8"))], [0, 1, "and"])
    value, vdt = chain_columns(dts, [("*", Col(1))])
    assert vdt == F64
    words = (n + 63) // 64
    ones = torch.full((words,), -1, dtype=torch.int64, device="cuda")
    valid, bitmaps = [], []
    for j in range(4):  # 10 % nulls per column, seeded; packed LSB-first into u64 words
        v = torch.rand(words * 64, device="cuda", generator=g) >= 0.1
        w = (v.view(words, 64).to(torch.int64) << torch.arange(64, device="cuda", dtype=torch.int64)).sum(dim=1)
        valid.append(v[:n])
        bitmaps.append(w)
    ccols = (abi.fq_col * 4)(*[c.col() for c in cols])
    aws = ops.Workspace(lib.fq_aggregate_workspace_bytes(n))
    nws = ops.Workspace(lib.fq_aggregate_nullable_workspace_bytes(n))
    dst = torch.empty(64, dtype=torch.uint8, device="cuda")
    SC = abi.AGG_SUM | abi.AGG_COUNT

    def vb(ptrs):
        return (C.c_void_p * 4)(*ptrs)

    legs = [("2 four bitmaps, all ones", vb([ones.data_ptr()] * 4), 4, None),
            ("3 four bitmaps, 10 % nulls each", vb([b.data_ptr() for b in bitmaps]), 4, valid),
            ("4 quantity's bitmap alone, all ones", vb([None, None, None, ones.data_ptr()]), 1, None)]

    def expected(v):
        keep = (t_ship < K) & (t_qty < Q)
        ok = keep
        if v is not None:
            keep = keep & v[2] & v[3]
            ok = keep & v[0] & v[1]
        prod = t_price[ok] * t_disc[ok].to(torch.float64)
        return int(keep.sum()), int(ok.sum()), float(prod.sum()), float(prod.abs().sum())

    def typed(br):
        check(lib.fq_aggregate_typed(ccols, 4, br, C.byref(pred), C.byref(value), SC, C.c_void_p(dst.data_ptr()),
                                     aws.ptr, aws.nbytes, st))

    def nullable(ptrs, br):
        check(lib.fq_aggregate_nullable(ccols, ptrs, 4, br, C.byref(pred), C.byref(value), SC,
                                        C.c_void_p(dst.data_ptr()), nws.ptr, nws.nbytes, st))

    def rec(name, ts, nbytes, note=""):
        ms = statistics.median(ts)
        gbps = nbytes / (ms * 1e-3) / 1e9
        res.append({"kernel": name, "ms": ms, "ms_min": min(ts), "ms_max": max(ts), "reps": len(ts),
                    "algorithmic_bytes": nbytes, "achieved_gbps": gbps, "frac_of_peak": gbps / PEAK, "note": note})
        print("%-58s %8.3f ms [%.3f .. %.3f]  %7.0f GB/s  %4.1f %%" % (name, ms, min(ts), max(ts), gbps,
                                                                     100 * gbps / PEAK), file=sys.stderr)
        return ts

    summary = {}
    for mode, br in (("flat", 0), ("block_mode", 10000)):
        t1 = rec("nullable q6 %s: 1 fq_aggregate_typed, no bitmaps" % mode, timed_all(lambda: typed(br), reps), 17 * n,
                 "the typed scan of the same statement: the yardstick of the legs below")
        kept, _, want, scale = expected(None)
        got = ops.state_from_device(dst[:48])
        assert got.count == kept and abs(ops.state_values(got)["sum"] - want) <= 1e-12 * scale
        out = {"typed_ms": statistics.median(t1), "typed_ms_min": min(t1), "typed_ms_max": max(t1)}
        for name, ptrs, nb, v in legs:
            nbytes = 17 * n + nb * ((n + 7) // 8)
            ts = rec("nullable q6 %s: %s" % (mode, name), timed_all(lambda: nullable(ptrs, br), reps), nbytes,
                     "fq_aggregate_nullable, %.3f B/row" % (nbytes / n))
            sn = abi.fq_agg_state_n.from_buffer_copy(dst.cpu().numpy().tobytes())
            kept, ok, want, scale = expected(v)
            assert sn.s.count == kept and sn.valid == ok and not sn.s.flags & 6, (name, sn.s.count, kept, sn.valid, ok)
            assert abs(ops.state_values(sn)["sum"] - want) <= 1e-12 * scale, (name, ops.state_values(sn)["sum"], want)
            out["leg" + name[0]] = {"ms": statistics.median(ts), "over_typed": statistics.median(ts) / statistics.median(t1),
                                    "bytes_over_typed": nbytes / (17 * n), "tb_per_s": nbytes / (statistics.median(ts) * 1e-3) / 1e12,
                                    "share_of_8_tb_per_s": nbytes / (statistics.median(ts) * 1e-3) / 1e9 / PEAK,
                                    "above_bytes_by_more_than_typed_spread": bool(
                                        statistics.median(ts) - statistics.median(t1) * nbytes / (17 * n) > max(t1) - min(t1))}
        summary[mode] = out
    res.append({"nullable_q6": {"rows": n, **summary}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1.25e9)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", choices=["q6", "pcols", "typed", "ptyped", "nullable"], default=None, help="run only the named group of lines")
    ap.add_argument("--q6-rows", type=float, default=float(1 << 27))
    args = ap.parse_args()
    n = int(args.rows)
    st = ops._stream()
    res = []
    if args.only in ("q6", "pcols", "typed", "ptyped", "nullable"):
        {"q6": q6_lines, "pcols": pcols_lines, "typed": typed_lines, "ptyped": ptyped_lines,
         "nullable": nullable_lines}[args.only](
            int(args.q6_rows), args.reps, st, res)
        print(json.dumps({"rows": int(args.q6_rows), "peak_gbps": PEAK, "device": torch.cuda.get_device_name(0),
                          "kernels": res}, indent=1))
        return

    def rec(name, ref, ms, nbytes, note=""):
        gbps = nbytes / (ms * 1e-3) / 1e9
        res.append({"kernel": name, "replaces": ref, "ms": ms, "algorithmic_bytes": nbytes,
                    "achieved_gbps": gbps, "frac_of_peak": gbps / PEAK, "note": note})
        print("%-34s %8.3f ms  %7.0f GB/s  %4.1f %%" % (name, ms, gbps, 100 * gbps / PEAK), file=sys.stderr)

    a = ops.empty_column(n, abi.DT_UINT64)
    b = ops.splitmix_column(7, 0, n)
    out = ops.empty_column(n, abi.DT_UINT64)
    bm = ops.empty_column(n, abi.DT_BOOLEAN)

    # source: NumbersStream::poll_next
    ms = timed(lambda: check(lib.fq_fill_numbers_u64(C.c_void_p(a.ptr), 0, n, st)), args.reps)
    rec("fill_numbers_u64", "numbers_stream.rs:65-83", ms, 8 * n)

    ac, bc, oc = a.col(), b.col(), out.col()
    one = abi.fq_value(abi.DT_UINT64, 1, 1)
    seven = abi.fq_value(abi.DT_UINT64, 1, 7)

    def arith(op, rhs_col=None, rhs_s=None):
        check(lib.fq_arith(op, C.byref(ac), None, C.byref(rhs_col) if rhs_col is not None else None,
                           C.byref(rhs_s) if rhs_s is not None else None, C.byref(oc), None, st))

    ms = timed(lambda: arith(abi.OP_BY_SYM["+"], rhs_s=one), args.reps)
    rec("arith u64 + const", "data_array_arithmetic.rs:14-55", ms, 16 * n)
    k = 1 << 20
    assert np.array_equal(out.to_numpy()[:k], np.arange(1, k + 1, dtype=np.uint64))
    ms = timed(lambda: arith(abi.OP_BY_SYM["*"], rhs_col=bc), args.reps)
    rec("arith u64 * col", "data_array_arithmetic.rs:14-55", ms, 24 * n)
    ms = timed(lambda: arith(abi.OP_BY_SYM["/"], rhs_s=seven), args.reps)
    rec("arith u64 / const 7", "data_array_arithmetic.rs:14-55", ms, 16 * n)
    assert np.array_equal(out.to_numpy()[:k], np.arange(0, k, dtype=np.uint64) // np.uint64(7))

    bound = abi.fq_value(abi.DT_UINT64, 1, (3 * 2**64) // 8)

    def compare():
        check(lib.fq_compare(abi.CMP_BY_SYM["<"], C.byref(bc), None, None, C.byref(bound),
                             C.c_void_p(bm.ptr), n, None, st))

    ms = timed(compare, args.reps)
    rec("compare u64 < const -> bitmap", "data_array_comparison.rs:14-94", ms, 8 * n + n // 8)
    hb = b.to_numpy()[:k]
    assert np.array_equal(bm.to_numpy()[:k], hb < np.uint64((3 * 2**64) // 8))

    ws = ops.Workspace(lib.fq_filter_workspace_bytes(n))
    kept = C.c_int64(0)

    def compact():
        check(lib.fq_filter_compact(C.byref(bc), C.c_void_p(bm.ptr), C.c_void_p(out.ptr), C.byref(kept),
                                    ws.ptr, ws.nbytes, st))

    ms = timed(compact, args.reps)
    rec("filter_compact (3/8 kept)", "transform_filter.rs:51 (arrow filter)", ms,
        8 * n + n // 8 + 8 * kept.value, "includes the host sync for out_len")

    aws = ops.Workspace(lib.fq_aggregate_workspace_bytes(n))
    dst = torch.empty(48, dtype=torch.uint8, device="cuda")
    ALL = abi.AGG_SUM | abi.AGG_MAX | abi.AGG_MIN | abi.AGG_COUNT

    def agg(col, pred=None, value=None, mask=ALL, br=10000):
        c = col.col()
        check(lib.fq_aggregate(C.byref(c), br, C.byref(pred) if pred is not None else None,
                               C.byref(value) if value is not None else None, mask,
                               C.c_void_p(dst.data_ptr()), aws.ptr, aws.nbytes, st))

    pb = abi.fq_pred()
    pb.kind = abi.PRED_BITMAP
    pb.bitmap = bm.ptr
    ms = timed(lambda: agg(b, pred=pb, mask=abi.AGG_MAX | abi.AGG_COUNT), args.reps)
    rec("aggregate, bitmap predicate", "function_aggregator.rs:57-100 + filter", ms, 8 * n + n // 8)
    ms = timed(lambda: agg(a), args.reps)
    rec("aggregate identity (C3 shape)", "function_aggregator.rs:57-100", ms, 8 * n)
    v, _ = chain(abi.DT_UINT64, [("+", 1)])
    p = predicate(abi.DT_UINT64, [("%", 8)], "<", 3)
    ms = timed(lambda: agg(a, pred=p, value=v, mask=abi.AGG_MAX | abi.AGG_COUNT), args.reps)
    rec("aggregate C4 shape (specialised)", "C4: max(number+1) WHERE (number%8)<3", ms, 8 * n)
    ms = timed(lambda: agg(a, pred=p, value=v, mask=abi.AGG_SUM), args.reps)
    rec("aggregate filtered sum (block mode)", "sum(number+1) WHERE (number%8)<3", ms, 8 * n)
    from fq_amd.expr import pred_tree
    tp = pred_tree(abi.DT_UINT64, [([("%", 8)], "<", 3), ([], ">", 1000)], [0, 1, "and"])
    ms = timed(lambda: agg(a, pred=tp, value=v, mask=abi.AGG_MAX | abi.AGG_COUNT), args.reps)
    rec("aggregate AND-tree predicate", "max(number+1) WHERE number%8<3 AND number>1000", ms, 8 * n)
    vf, _ = chain(abi.DT_UINT64, [("*", 1.5), ("+", 0.25)])
    ms = timed(lambda: agg(a, value=vf), args.reps)
    rec("aggregate f64 chain", "sum/max/min(number*1.5+0.25)", ms, 8 * n)
    vd, _ = chain(abi.DT_UINT64, [("%", 1000003)])
    ms = timed(lambda: agg(b, value=vd), args.reps)
    rec("aggregate u64 % 1000003 (magic)", "sum/max/min(x % 1000003)", ms, 8 * n)
    vm, _ = chain(abi.DT_UINT64, [("%", 1000)])
    ms = timed(lambda: agg(b, value=vm), args.reps)
    rec("aggregate u64 % 1000 (32-bit halves)", "sum/max/min(x % 1000)", ms, 8 * n)
    vq, _ = chain(abi.DT_UINT64, [("/", 1000)])
    ms = timed(lambda: agg(b, value=vq), args.reps)
    rec("aggregate u64 / 1000 (32-bit long division)", "sum/max/min(x / 1000)", ms, 8 * n)
    ops.jit_config(abi.JIT_OFF)
    ms = timed(lambda: agg(a, pred=p, value=v, mask=abi.AGG_MAX | abi.AGG_COUNT), args.reps)
    rec("aggregate C4 shape (interpreted)", "C4 with FQ_JIT_OFF", ms, 8 * n)
    ops.jit_config(abi.JIT_AUTO, 1 << 22)

    # expression trees (FQ_OP_PUSH / FQ_OPERAND_STACK) in the fused scan
    from fq_amd.expr import PUSH, STACK
    vt, _ = chain(abi.DT_UINT64, [("+", 1), PUSH, ("%", 1000), ("*", STACK, True)])
    ms = timed(lambda: agg(a, value=vt), args.reps)
    rec("aggregate tree (number+1)*(number%1000)", "sum/max/min of an ArithmeticFunction tree", ms, 8 * n)

    # FilterTransform -> ProjectionTransform fused (fq_filter_project)
    flag = ops.Workspace(8)
    readme_pred = predicate(abi.DT_UINT64, [("+", 1), PUSH, ("/", 2), ("+", STACK, True), ("+", 1)], "<", 100)
    ac2 = a.col()
    ms = timed(lambda: check(lib.fq_predicate_bitmap(C.byref(ac2), C.byref(readme_pred), C.c_void_p(bm.ptr),
                                                     flag.ptr, st)), args.reps)
    rec("predicate_bitmap (number+1)+(number/2)+1<100", "README WHERE, one kernel", ms, 8 * n + n // 8,
        "includes the host sync for the error flag")
    pws = ops.Workspace(lib.fq_filter_project_workspace_bytes(n))
    out2 = ops.empty_column(n, abi.DT_UINT64)
    p38 = predicate(abi.DT_UINT64, [], "<", (3 * 2**64) // 8)
    vals = (abi.fq_expr * 2)(chain(abi.DT_UINT64, [("+", 1)])[0], chain(abi.DT_UINT64, [("/", 2)])[0])
    outs = (C.c_void_p * 2)(out.ptr, out2.ptr)
    bc2 = b.col()

    def project():
        check(lib.fq_filter_project(C.byref(bc2), C.byref(p38), vals, 2, outs, C.byref(kept), pws.ptr, pws.nbytes, st))

    ms = timed(project, args.reps)
    rec("filter_project 3/8 kept -> x+1, x/2", "Filter + Projection fused", ms, 8 * n + 2 * 8 * kept.value,
        "two passes over the column (bits, scatter) + host sync for out_len")
    hb = b.to_numpy()[:k]
    kk = hb[hb < np.uint64((3 * 2**64) // 8)]
    assert np.array_equal(out.to_numpy()[:len(kk)], kk + np.uint64(1))
    vals1 = (abi.fq_expr * 1)(chain(abi.DT_UINT64, [("*", 3), ("+", 1)])[0])
    outs1 = (C.c_void_p * 1)(out.ptr)
    ms = timed(lambda: check(lib.fq_filter_project(C.byref(ac2), None, vals1, 1, outs1, C.byref(kept), pws.ptr,
                                                   pws.nbytes, st)), args.reps)
    rec("filter_project map x*3+1 (no predicate)", "Projection fused", ms, 16 * n, "host sync for out_len")

    # GROUP BY (fq_group_aggregate): LDS pre-aggregation, low and high cardinality
    key, _ = chain(abi.DT_UINT64, [("%", 1000)])
    aggs3 = [(abi.AGG_COUNT, abi.DT_UINT64), (abi.AGG_SUM, abi.DT_UINT64), (abi.AGG_MAX, abi.DT_UINT64)]
    gt = ops.GroupTable(1 << 12, aggs3)

    def group_low():
        check(lib.fq_group_table_init(C.byref(gt.desc), st))
        gt.aggregate(a, key=key)

    ms = timed(group_low, args.reps)
    rec("group by number%1000: count,sum,max", "no reference (plan_parser.rs:284-308)", ms, 8 * n,
        "includes the table init")
    assert gt.count() == 1000
    key8, _ = chain(abi.DT_UINT64, [("%", 8)])
    pred = predicate(abi.DT_UINT64, [("%", 8)], "<", 3)
    v1, _ = chain(abi.DT_UINT64, [("+", 1)])
    gt8 = ops.GroupTable(64, [(abi.AGG_MAX, abi.DT_UINT64), (abi.AGG_COUNT, abi.DT_UINT64)])

    def group_c4():
        check(lib.fq_group_table_init(C.byref(gt8.desc), st))
        gt8.aggregate(a, pred=pred, key=key8, values=[v1, None])

    ms = timed(group_c4, args.reps)
    rec("group by number%8 WHERE %8<3: max(+1),count", "C4 shape grouped", ms, 8 * n, "includes the table init")
    hn = min(n, 1 << 27)
    hc = ops.DeviceColumn(b.buf, hn, abi.DT_UINT64)
    gth = ops.GroupTable(1 << 28, [(abi.AGG_COUNT, abi.DT_UINT64)])

    def group_high():
        check(lib.fq_group_table_init(C.byref(gth.desc), st))
        gth.aggregate(hc)

    ms = timed(group_high, max(3, args.reps // 3))
    rec("group by x (distinct, %d rows): count" % hn, "high cardinality: HBM table, 2^28 slots", ms, 8 * hn,
        "includes the table init (4 GB)")

    q6_lines(int(args.q6_rows), args.reps, st, res)
    typed_lines(int(args.q6_rows), args.reps, st, res)
    ptyped_lines(int(args.q6_rows), args.reps, st, res)

    print(json.dumps({"rows": n, "peak_gbps": PEAK, "device": torch.cuda.get_device_name(0),
                      "kernels": res}, indent=1))


if __name__ == "__main__":
    main()
