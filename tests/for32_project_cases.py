"""Inputs, shapes and a numpy model for fq_filter_project_blocks_for32 (the
Filter -> Projection block stream over a window of a frame-of-reference copy),
shared by tests/test_for32_project_cpu.py and tests/test_for32_project_gpu.py.

Columns: `random` gives every 65,536-row frame a 64-bit base of its own (every
third one >= 2^63) and deltas over the whole 32-bit range, 0 and 2^32 - 1
included, so a row decoded with a neighbouring frame's base is wrong in its high
bits; `iota` is numbers_mt's shape (the same deltas in every frame).

walk() restates the kernel's load phase row for row: one block per ticket, tiles
of 8,192 rows from the block's first row, per tile the two frame bases fb_lo /
fb_hi (the second index clamped to the window's last row), the base chosen per
row, and 8-byte delta-pair loads where the tile is whole and its first delta
8-byte aligned, element loads with row guards elsewhere.  The model gives a pair
load the meaning the source's `const u64 *` cast promises -- the aligned 8-byte
word; gfx950's global loads tolerate a misaligned address, so on the device the
`no_first_in_alignment` mistake would be undefined behaviour that happens to
read the right rows, not a wrong result: the model pins the test the source must
make, tests/test_for32_project_gpu.py pins the rows the kernel produces.  Nothing
here needs a GPU."""
import numpy as np

from fq_amd import abi
from fq_amd.expr import chain, pred_tree, predicate

F = abi.FOR32_FRAME_ROWS
TILE = 8192  # FQ_PROJECT_MIN_BLOCK_ROWS: the kernel's tile at the default SELECT_BLOCKS_ROWS
U64 = abi.DT_UINT64

LENGTHS = [1, 8191, 8192, 8193, 65536, 65537, 200_003]
BLOCK_ROWS = [8192, 10_000, 10_001, 65_536]
FIRSTS = [0, 1, 2, 4097, 65_535, 65_536, 131_071]
# Two encoded columns over the same rows.  The long one ends where the longest window from the largest first does
# (131,071 + 200,003 rows: 5 frames and 3,394 rows).  The short one is its first three frames exactly (131,071 +
# 65,537 rows), and every window that fits runs on it: windows end inside its last frame and exactly at its end,
# where the nominal last row of the last tile lies in a frame the bases do not hold (the fb_hi clamp).
ENC_LEN = FIRSTS[-1] + LENGTHS[-1]
ENC_SHORT = 3 * F
assert ENC_SHORT == FIRSTS[-1] + 65_537


def windows():
    """(encoded length, first, len) of every case"""
    for first in FIRSTS:
        for n in LENGTHS:
            yield (ENC_SHORT if first + n <= ENC_SHORT else ENC_LEN), first, n


def host_column(n, kind, seed=0xF032):
    rng = np.random.default_rng(seed)
    if kind == "iota":
        return np.arange(n, dtype=np.uint64) + np.uint64(3 << 40)
    assert kind == "random"
    frames = -(-n // F)
    base = rng.integers(0, 2**62, size=frames, dtype=np.uint64) * np.uint64(2)
    base[::3] += np.uint64(1 << 63)  # below 2^64 - 2^32: base + delta never wraps
    delta = rng.integers(0, 2**32, size=n, dtype=np.uint64)
    delta[::F] = 0  # each frame's minimum is its base
    delta[1::F] = 2**32 - 1
    return np.repeat(base, F)[:n] + delta


def encode_host(host):
    """fq_for32_encode on the host: (delta uint32, base uint64), base = the frame's minimum."""
    n = len(host)
    frames = -(-n // F)
    base = np.array([host[f * F:(f + 1) * F].min() for f in range(frames)], dtype=np.uint64)
    delta = host - np.repeat(base, F)[:n]
    assert int(delta.max(initial=0)) < 2**32
    return delta.astype(np.uint32), base


MISTAKES = ("tile_base", "pair_base", "no_first_in_frame", "no_first_in_alignment")


def walk(delta, base, first, n, block_rows, mistake=None, delta_addr=0):
    """The window [first, first + n) as the kernel's load phase decodes it -> (uint64 rows, visits per row).
    delta_addr: the byte address of delta[0] modulo 8 (fq_for32_encode's buffers are 16-byte aligned)."""
    out = np.zeros(n, np.uint64)
    visits = np.zeros(n, np.int32)
    B = min(block_rows, n) if n else block_rows
    # the deltas as the aligned 8-byte words a pair load returns
    pad = np.zeros(len(delta) + 4, np.uint32)
    pad[:len(delta)] = delta
    for b0 in range(0, n, B):
        end = min(b0 + B, n)
        for r0 in range(b0, end, TILE):
            g0 = first + r0
            fg0 = r0 if mistake == "no_first_in_frame" else g0
            fe = ((fg0 >> 16) + 1) << 16
            f_hi = min((fg0 + TILE - 1) >> 16, ((fg0 - r0) + end - 1) >> 16)
            assert 0 <= (fg0 >> 16) < len(base) and f_hi < len(base)  # the clamp keeps the second index inside
            fb_lo, fb_hi = int(base[fg0 >> 16]), int(base[f_hi])
            rows = np.arange(r0, min(r0 + TILE, end))
            g = rows + first
            addr = delta_addr + 4 * (r0 if mistake == "no_first_in_alignment" else g0)
            if r0 + TILE <= end and addr % 8 == 0:
                start = g0 - ((delta_addr // 4 + g0) & 1)  # the aligned words the pair loads return begin here
                d = pad[start + np.arange(TILE)].astype(np.uint64)
            else:
                d = delta[g].astype(np.uint64)
            fg = rows + (fg0 - r0)
            if mistake == "tile_base":
                lo = np.ones(len(rows), bool)
            elif mistake == "pair_base":
                lo = (fg - ((rows - r0) & 1)) < fe  # the pair's first row decides for both
            else:
                lo = fg < fe
            out[rows] = np.where(lo, np.uint64(fb_lo), np.uint64(fb_hi)) + d
            visits[rows] += 1
    return out, visits


# ---------------------------------------------------------------------------
# call shapes: name -> (fq_pred, [fq_expr], keep(x) -> bool rows, [value(kept rows) -> numpy])
# ---------------------------------------------------------------------------
def shape(name):
    u = np.uint64
    if name == "p1":  # SELECT number+1, number/2 WHERE (number%8)<3
        return (predicate(U64, [("%", 8)], "<", 3), [chain(U64, [("+", 1)])[0], chain(U64, [("/", 2)])[0]],
                lambda x: x % u(8) < u(3), [lambda k: k + u(1), lambda k: k // u(2)])
    if name == "none":
        return predicate(U64, [("%", 8)], ">", 8), [None], lambda x: np.zeros(len(x), bool), [lambda k: k]
    if name == "all":
        return predicate(U64, [], ">=", 0), [None, chain(U64, [("+", 1)])[0]], lambda x: np.ones(len(x), bool), \
            [lambda k: k, lambda k: k + u(1)]
    if name == "runs":  # kept / dropped runs of thousands of rows (the deltas' low bits are the row's for iota)
        return (predicate(U64, [("%", 30_000)], "<", 11_000), [chain(U64, [("*", 3), ("-", 5)])[0]],
                lambda x: x % u(30_000) < u(11_000), [lambda k: k * u(3) - u(5)])
    if name == "tree":  # ((x%8)<3 AND x>1000) OR (x%97)=0 with a Float64 and an Int64 output
        return (pred_tree(U64, [([("%", 8)], "<", 3), ([], ">", 1000), ([("%", 97)], "=", 0)], [0, 1, "and", 2, "or"]),
                [chain(U64, [("/", 2.0)])[0], chain(U64, [("-", (5000, "Int64"))])[0]],
                lambda x: ((x % u(8) < u(3)) & (x > u(1000))) | (x % u(97) == u(0)),
                [lambda k: k.astype(np.float64) / 2.0, lambda k: k.astype(np.int64) - np.int64(5000)])
    if name == "eight":
        return (predicate(U64, [("%", 3)], "=", 1), [chain(U64, [("+", j)])[0] for j in range(8)],
                lambda x: x % u(3) == u(1), [(lambda j: (lambda k: k + u(j)))(j) for j in range(8)])
    raise KeyError(name)


def expect_blocks(host, keep, fns, block_rows):
    """tests/test_project_blocks_gpu.py's _expect_blocks: [output][block] -> the block's kept rows through fn."""
    from test_project_blocks_gpu import _expect_blocks
    return _expect_blocks(host, keep, fns, block_rows)
