"""Shared by tests/test_for32_expr_{cpu,gpu}.py and tests/test_for32_expr_launch_gpu.py:
the inputs, the fused shapes with their numpy references, and a numpy model of
how fq_jit_scan_for32 walks a column stored as per-frame 32-bit deltas.

Nothing here needs a GPU.  The model restates the kernel's loops (fq_jit.hip,
gen_for32_loop): which frame base each row is decoded with.  It returns the
column as the kernel sees it, so `model == decoded column` is the statement that
every row meets its own frame's base, and a wrong base shows as a changed value.
"""
import numpy as np

from fq_amd import abi
from fq_amd.expr import PUSH, STACK, chain, pred_tree, predicate

F = abi.FOR32_FRAME_ROWS      # rows per frame
TILE = 4 * 256 * 4            # rows per tile: 4 vectors x 256 lanes x 4 deltas (fq_scan.h kFor32TileRows)
TILES_PER_FRAME = F // TILE   # 16 whole tiles make a frame
U64, I64, F64 = abi.DT_UINT64, abi.DT_INT64, abi.DT_FLOAT64
ALL = abi.AGG_SUM | abi.AGG_MAX | abi.AGG_MIN | abi.AGG_COUNT
LENGTHS = [1, 3, 4, 5, 4095, 4096, 4097, 65535, 65536, 65537, 2 * 65536 + 4099, 1_000_003]
DATA = ["iota", "random", "span_max"]


def host_values(n, data):
    """iota: from 1,250,000,000; random: seeded deltas below 2^32 over a seeded random base per frame (a stale
    or neighbouring base changes every value); span_max: a frame with max - min == 2^32 - 1; iota_hi: an iota
    ending above 2^63 (its last row is 2^63 + 5)."""
    if data == "iota":
        return np.arange(n, dtype=np.uint64) + np.uint64(1_250_000_000)
    if data == "iota_hi":
        return np.arange(n, dtype=np.uint64) + np.uint64(2**63 + 5 - (n - 1))
    rng = np.random.default_rng(1000 * n + 17 * DATA.index(data))
    frames = (n + F - 1) // F
    if data == "random":
        base = rng.integers(0, 2**63 - 2**32, size=frames, dtype=np.uint64)
        return np.repeat(base, F)[:n] + rng.integers(0, 2**32, size=n, dtype=np.uint64)
    v = np.uint64(3 << 40) + rng.integers(1000, 2000, size=n, dtype=np.uint64)
    if n >= 2:
        f = frames - 1 if n - (frames - 1) * F >= 2 else frames - 2
        lo, hi = f * F, min((f + 1) * F, n) - 1
        v[lo] = np.uint64(3 << 40)
        v[hi] = np.uint64((3 << 40) + 2**32 - 1)
    return v


def encode_host(host):
    """fq_for32_encode on the host: (delta uint32, base uint64), base = each frame's minimum."""
    n = len(host)
    base = np.array([host[s:s + F].min() for s in range(0, n, F)], dtype=np.uint64)
    delta = host - np.repeat(base, F)[:n]
    assert n == 0 or int(delta.max()) <= 2**32 - 1
    return delta.astype(np.uint32), base


# ---------------------------------------------------------------------------
# the fused shapes: name -> (pred or None, value or None, keep(x) -> bool mask, val(x) -> values)
# ---------------------------------------------------------------------------
def _u(k):
    return np.uint64(k)


def shape(name):
    with np.errstate(over="ignore"):
        if name in ("c4", "c4s"):  # max / sum (x+1) WHERE x%8<3
            return (predicate(U64, [("%", 8)], "<", 3), chain(U64, [("+", 1)])[0],
                    lambda x: x % _u(8) < _u(3), lambda x: x + _u(1))
        if name == "max1":  # max(x+1)
            return None, chain(U64, [("+", 1)])[0], lambda x: np.ones(len(x), bool), lambda x: x + _u(1)
        if name == "push":  # (x+1)*(x%1000): PUSH and a stack operand
            return (None, chain(U64, [("+", 1), PUSH, ("%", 1000), ("*", STACK, True)])[0],
                    lambda x: np.ones(len(x), bool), lambda x: (x + _u(1)) * (x % _u(1000)))
        if name == "tree":  # (x%8<3 AND x>1000) OR x%97=0
            return (pred_tree(U64, [([("%", 8)], "<", 3), ([], ">", 1000), ([("%", 97)], "=", 0)],
                              [0, 1, "and", 2, "or"]), chain(U64, [("+", 1)])[0],
                    lambda x: ((x % _u(8) < _u(3)) & (x > _u(1000))) | (x % _u(97) == _u(0)), lambda x: x + _u(1))
        if name == "libdivide":  # x / 7: the multiply-high form with its "add" marker; % 1000003: without it
            return (predicate(U64, [("%", 1000003)], "<", 400000), chain(U64, [("/", 7)])[0],
                    lambda x: x % _u(1000003) < _u(400000), lambda x: x // _u(7))
    raise KeyError(name)


def reference(x, keep, val):
    """(sum, max, min, count) of val(x) over the kept rows, as wrapping u64 (max / min 0 when no row is kept:
    compare them only when count > 0)."""
    with np.errstate(over="ignore"):
        y = val(x)[keep(x)]
        if len(y) == 0:
            return 0, 0, 0, 0
        return int(y.sum(dtype=np.uint64)), int(y.max()), int(y.min()), len(y)


# ---------------------------------------------------------------------------
# the kernel's walk
# ---------------------------------------------------------------------------
def flat_grid(n, cap):
    """for32_flat_grid (fq_scan.h): min(ceil((n / 4) / 1024), cap), at least 1"""
    return max(1, min(-(-(n // 4) // (TILE // 4)), cap))


def flat_model(delta, base, grid, mistake=None):
    """The flat loop: workgroup b takes tiles b, b + grid, ...; the next tile's loads are in flight while the
    current one is decoded with ITS frame's base (one load per tile); then whole 4-row vectors past the last
    whole tile, and up to 3 rows, with the base looked up from the row index.  Returns (x as decoded, visits).
    mistake: 'prefetched_base' (the tile in flight's base for the current tile), 'base0_remainder' (base[0]
    for the remainder vectors)."""
    n = len(delta)
    d = delta.astype(np.uint64)
    x = np.zeros(n, np.uint64)
    visits = np.zeros(n, np.int32)
    nvec = n // 4
    ntiles = nvec // (TILE // 4)
    for b in range(grid):
        for t in range(b, ntiles, grid):
            tn = t + grid  # the prefetched tile
            tb = tn if (mistake == "prefetched_base" and tn < ntiles) else t
            rows = slice(t * TILE, (t + 1) * TILE)
            x[rows] = base[tb // TILES_PER_FRAME] + d[rows]
            visits[rows] += 1
    r0, r1 = ntiles * TILE, nvec * 4  # remainder vectors: row >> 16 per vector (never straddles a frame)
    if r1 > r0:
        idx = np.arange(r0, r1, 4)
        fb = base[0] if mistake == "base0_remainder" else np.repeat(base[idx >> 16], 4)
        x[r0:r1] = fb + d[r0:r1]
        visits[r0:r1] += 1
    if n > r1:  # the up to 3 tail rows
        idx = np.arange(r1, n)
        x[r1:] = base[idx >> 16] + d[r1:]
        visits[r1:] += 1
    return x, visits


def block_model(delta, base, block_rows, mistake=None):
    """Block mode: one wave per reference block.  block_rows % 4 == 0: 4-row vectors from the block's start
    (a multiple of 4, so no vector straddles a frame) with the base per vector, then the last block's up to 3
    rows; otherwise 4-byte elements with the base per row.  mistake: 'first_frame_base' (the block's first
    frame's base for the whole block)."""
    n = len(delta)
    d = delta.astype(np.uint64)
    x = np.zeros(n, np.uint64)
    visits = np.zeros(n, np.int32)
    for s in range(0, n, block_rows):
        e = min(s + block_rows, n)
        if mistake == "first_frame_base":
            x[s:e] = base[s >> 16] + d[s:e]
        elif block_rows % 4 == 0:
            nv = (e - s) // 4
            vrow = s + 4 * np.arange(nv)
            x[s:s + 4 * nv] = np.repeat(base[vrow >> 16], 4) + d[s:s + 4 * nv]
            idx = np.arange(s + 4 * nv, e)
            x[s + 4 * nv:e] = base[idx >> 16] + d[s + 4 * nv:e]
        else:
            idx = np.arange(s, e)
            x[s:e] = base[idx >> 16] + d[s:e]
        visits[s:e] += 1
    return x, visits


def launch_rows(cus, wg_per_cu):
    """Rows at which fq_jit_scan_for32's persistent loop passes its first iteration: 4,096 rows per tile, grid =
    CUs x SCAN_WG_PER_CU.  {name: rows}: one round less a tile; exactly two rounds; two and a third rounds with
    a partial tile (half a tile of remainder vectors) and 3 odd rows."""
    cap = cus * wg_per_cu
    return {"one_round_minus": (cap - 1) * TILE, "exact_2": 2 * cap * TILE,
            "ragged": (2 * cap + max(1, cap // 3)) * TILE + TILE // 2 + 3}
