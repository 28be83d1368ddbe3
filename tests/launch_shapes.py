"""A model of how every streaming kernel is launched: rows per unit of work
(a tile, a reference block, a group of bitmap words), and how many units the
capped grid takes per round of its persistent loop.  From a CU count and a
knob setting it gives the row counts at which a workgroup (or a wave) takes
more than one unit -- the sizes tests/test_launch_shapes_gpu.py runs and
tests/test_launch_shapes_cpu.py checks against their definitions.

Every formula restates one line of the launch code; the comment beside it
names that line and its function (the numbers are those of the commit that
added this file; the function finds the line after they move).  Nothing here
needs a GPU; the GPU tests pass the CU count they read from the device
(torch's multi_processor_count).

Named cases of a Model (cases()):
  one_round_minus  cap - 1 units less one row: no worker takes a second unit;
  exact_2          two full rounds;
  ragged           two rounds, about a third of a round, half a unit and 3 rows:
                   every worker takes two units, some a third, and the vector
                   and scalar tails are not empty;
  ragged_head      `ragged` read from a pointer one element off the 16-byte
                   boundary (8 bytes for a 64-bit column), so head != 0.

The two select kernels (look-back and block stream) size their grid by
CUs x min(knob, occupancy).  The occupancy of a compiled kernel is not known
here, so the knob is treated as an upper bound of the grid: `ragged` is sized
for the knob's cap and therefore holds for any occupancy >= 1 (a smaller grid
only gives every workgroup more tiles).  At knob 1 the grid is exactly the CU
count.

Not modelled: fq_aggregate's flat grid is capped by CUs x SCAN_WG_PER_CU only;
the workspace holds kMaxPartials = 4,096 partials, which that cap reaches
exactly at 256 CUs x 16 (the knob's maximum; a tuning value, the default is 2).
"""
from collections import namedtuple

THREADS = 256           # fq_scan.h:13 kThreads, workgroup size of every kernel here
WAVES = THREADS // 64   # waves per workgroup
MAX_PARTIALS = 4096     # fq_scan.h:14 kMaxPartials
FRAME_ROWS = 65536      # include/fq_gpu.h FQ_FOR32_FRAME_ROWS (fq_aggregate.hip:302 kFrame)
PROJECT_MIN_BLOCK_ROWS = 8192  # fq_scan.h:305 kProjectBlockTile == FQ_PROJECT_MIN_BLOCK_ROWS (fq_filter.hip:755)

DEFAULT_KNOBS = {"SCAN_WG_PER_CU": 2, "EW_WG_PER_CU": 0, "BLOCK_U": 8, "SELECT_WG_PER_CU": 8,
                 "SELECT_BLOCKS_WG_PER_CU": 8, "SELECT_BLOCKS_ROWS": 32, "SELECT_BLOCKS_STAGE": 2}  # fq_knobs.cpp:21-29

CASES = ("one_round_minus", "exact_2", "ragged", "ragged_head")


class Model(namedtuple("Model", "family unit_rows cap ceil exact_grid")):
    """unit_rows: rows of one unit of work; cap: units the capped grid takes per round (workgroups x units per
    workgroup and round); ceil: a partial last unit is a unit of its own (else it goes to the kernel's tail
    loops); exact_grid: the launch's grid IS min(units, cap) workgroups (False: the cap is an upper bound)"""

    def units(self, n):
        return -(-n // self.unit_rows) if self.ceil else n // self.unit_rows

    def workers(self, n):
        """workers that take units when the grid is at its cap for n rows (never more than the cap)"""
        return max(1, min(-(-n // self.unit_rows), self.cap))

    def per_worker(self, n, workers=None):
        """units each worker takes, dealt round-robin (unit u -> worker u % workers)"""
        w = workers or self.workers(n)
        u = self.units(n)
        return [u // w + (1 if i < u % w else 0) for i in range(w)]

    def cases(self):
        """{name: (rows, leading elements off the 16-byte boundary)}"""
        u, c = self.unit_rows, self.cap
        ragged = (2 * c + max(1, c // 3)) * u + u // 2 + 3
        return {"one_round_minus": ((c - 1) * u - 1, 0), "exact_2": (2 * c * u, 0), "ragged": (ragged, 0),
                "ragged_head": (ragged, 1)}

    def just_above(self):
        """one round, about a third of a round, half a unit and 3 rows: some workers take a second unit"""
        return (self.cap + max(1, self.cap // 3)) * self.unit_rows + self.unit_rows // 2 + 3


# ---------------------------------------------------------------------------
# flat scans
# ---------------------------------------------------------------------------
def flat_scan(cus, width_bytes, wg_per_cu):
    """fq_aggregate over one column (agg_flat_kernel, its PF variant, the single-column fq_jit_scan)"""
    # fq_aggregate.hip:1109 (plan_scan)  tile = kThreads * (esize >= 4 ? 4 : (esize == 2 ? 2 : 1)) 16-byte vectors
    vectors = THREADS * (4 if width_bytes >= 4 else (2 if width_bytes == 2 else 1))
    rows = vectors * (16 // width_bytes)  # fq_aggregate.hip:1103 (plan_scan) vec_elems = 16 / esize
    # fq_aggregate.hip:1113-1114 (plan_scan)  grid = min(tiles, cus * scan_wg_per_cu())
    return Model("flat", rows, cus * wg_per_cu, False, True)


def scan_cols_vectors(n_cols):
    return 2 if n_cols <= 2 else 1  # fq_scan.h:119 (FQ_SCAN_COLS_VECTORS_3 = 1)


def flat_scan_columns(cus, n_cols, wg_per_cu):
    """fq_aggregate_columns over n_cols >= 2 64-bit columns (fq_jit_scan, gen_cols_loop)"""
    # fq_aggregate.hip:1169 (plan_scan_cols)  tile_rows = kThreads * scan_cols_vectors(n_cols) * 2
    # fq_aggregate.hip:1172-1173 (plan_scan_cols)  grid = min(tiles, cus * scan_wg_per_cu())
    return Model("flat_columns", THREADS * scan_cols_vectors(n_cols) * 2, cus * wg_per_cu, False, True)


def typed_group(widths):
    """fq_scan.h:64-83 typed_group -> (rows per lane G, prefetch)"""
    total, wmin = sum(widths), min(widths)

    def fit(nbytes):
        g = 16
        while g > 1 and g * total > nbytes:
            g >>= 1
        return g
    g0, g1 = fit(64), fit(128)
    if g0 * wmin < 4 and g1 * wmin >= 4:
        return g1, False
    return g0, True


def flat_scan_typed(cus, widths, wg_per_cu):
    """fq_aggregate_typed / fq_aggregate_nullable (the typed fq_jit_scan)"""
    # fq_aggregate.hip:1385 (plan_scan_typed)  tile_rows = kThreads * G;  :1388-1389  grid = min(tiles, cus * scan_wg_per_cu())
    return Model("flat_typed", THREADS * typed_group(widths)[0], cus * wg_per_cu, False, True)


FOR32_TILE = 4 * THREADS * 4  # fq_aggregate.hip:303 kFor32Tile
FOR32_TILES_PER_FRAME = FRAME_ROWS // FOR32_TILE  # fq_aggregate.hip:360 kTilesPerFrame


def for32(cus, wg_per_cu):
    """fq_aggregate_for32 (agg_flat_kernel_for32)"""
    # fq_aggregate.hip:1622-1625 (fq_aggregate_for32)  grid = min(ceil((len / 4) / (kFor32Tile / 4)), cus * scan_wg_per_cu())
    return Model("for32", FOR32_TILE, cus * wg_per_cu, False, True)


# ---------------------------------------------------------------------------
# block-mode scans: a wave owns whole reference blocks
# ---------------------------------------------------------------------------
def block_scan(cus, block_rows):
    """agg_block_kernel and the block-mode fq_jit_scan of every entry point: unit = one reference block, a
    round = one block per wave"""
    # fq_aggregate.hip:1096 / 1157 / 1374 (plan_scan, plan_scan_cols, plan_scan_typed)  max_grid = min(cus * 8, kMaxPartials)
    # fq_aggregate.hip:1099-1100 / 1159-1160 / 1376-1377  grid = min(ceil(blocks / 4), max_grid)
    # fq_aggregate.hip:431-433 (agg_block_kernel)  W = gridDim.x * kThreads / kWave waves; block b -> wave b % W
    return Model("block", block_rows, min(cus * 8, MAX_PARTIALS) * WAVES, True, True)


# ---------------------------------------------------------------------------
# Filter -> Projection
# ---------------------------------------------------------------------------
def project_cols_rows(n_cols):
    return 32 if n_cols <= 1 else (16 if n_cols <= 3 else 8)  # fq_scan.h:277


def typed_project_geometry(widths, out_widths):
    """fq_scan.h:260-269 -> (rows per thread R, row group G)"""
    total, wout = sum(widths), max(out_widths)
    r = 32
    while r > 1 and (r * total > 384 or r * wout > 128):
        r >>= 1
    g = 16
    while g > 1 and (g > r or g * total > 128):
        g >>= 1
    return r, g


def select_tile_rows(n_cols=1, typed=None):
    """fq_scan.h:293-297 project_tile_rows: 256 x project_cols_rows(K), a typed call's 256 x rows"""
    if typed is not None:
        return THREADS * typed_project_geometry(*typed)[0]
    return THREADS * project_cols_rows(n_cols)


def select(cus, wg_per_cu, n_cols=1, typed=None):
    """fq_jit_pselect: tiles drawn from one ticket; the knob bounds the grid from above (see the module docstring)"""
    # fq_jit.hip:4825 (jit_project_select)  ntiles = ceil(n / project_tile_rows(P))
    # fq_jit.hip:4851 (jit_project_select)  grid = max(1, min(ntiles, cus * min(wg_per_cu, occ)))
    return Model("select", select_tile_rows(n_cols, typed), cus * wg_per_cu, True, wg_per_cu == 1)


def block_stream(cus, block_rows, wg_per_cu):
    """fq_jit_pblocks: whole blocks drawn from one ticket, one block per draw"""
    # fq_jit.hip:4871-4872 (jit_project_blocks)  B = min(block_rows, n); nb = ceil(n / B)
    # fq_jit.hip:4900 (jit_project_blocks)  grid = max(1, min(nb, cus * min(wg_per_cu, occ)))
    assert block_rows >= PROJECT_MIN_BLOCK_ROWS  # fq_jit.hip:4863 (jit_project_blocks)
    return Model("block_stream", block_rows, cus * wg_per_cu, True, wg_per_cu == 1)


def proj_grid_cap(cus):
    return cus * 8  # fq_jit.hip:4782 proj_grid: cap = cus * 8


def bitmap(cus, n_cols=1):
    """fq_jit_pbits: a wave takes 8 / K bitmap words per step, a workgroup four times that"""
    # fq_jit.hip:4806 (jit_project_bits)  wave_words = n_cols > 1 ? max(1, 8 / n_cols) : 8
    wave_words = max(1, 8 // n_cols) if n_cols > 1 else 8
    # fq_jit.hip:4807 (jit_project_bits)  proj_grid(nwords, 4 * wave_words)
    return Model("bitmap", WAVES * wave_words * 64, proj_grid_cap(cus), True, True)


def project_map(cus, typed=None):
    """fq_jit_pmap (no predicate)"""
    if typed is None:
        # fq_jit.hip:4924-4925 (jit_project_map)  units = n / 2 row pairs, per_wg = kThreads * 4;  :4943 proj_grid(units, per_wg)
        return Model("map", 2 * THREADS * 4, proj_grid_cap(cus), True, True)
    widths, out_widths = typed
    group = typed_project_geometry(widths, out_widths)[1]
    # fq_jit.hip:4938-4939 (jit_project_map)  units = n / group, per_wg = kThreads * max(1, 128 / (group * sum))
    return Model("map_typed", group * THREADS * max(1, 128 // (group * sum(widths))), proj_grid_cap(cus), True, True)


# ---------------------------------------------------------------------------
# element-wise fast paths (64-bit operands of one type, 16-byte aligned)
# ---------------------------------------------------------------------------
def ew_arith(cus, ew_wg_per_cu):
    """arith_vec_kernel: one tile of kEwU * 256 16-byte vectors per workgroup iteration"""
    # fq_elementwise.hip:433 (launch_fast)  rows_per_unit = kEwU * 256 * 2 (kEwU = 8, :201)
    # fq_elementwise.hip:440-443 (launch_fast)  cap = cus * (override ? override : 8); grid = min(units, cap)
    return Model("ew_arith", 8 * 256 * 2, cus * (ew_wg_per_cu or 8), False, True)


def ew_compare(cus, ew_wg_per_cu):
    """compare_vec_kernel: one 1,024-row group per wave, four per workgroup"""
    # fq_elementwise.hip:433 (launch_fast)  rows_per_unit = 1024;  :440  cap = cus * (override ? override : 2)
    # fq_elementwise.hip:442-443 (launch_fast)  want = (units + 3) / 4; grid = min(want, cap)
    return Model("ew_compare", 1024 * WAVES, cus * (ew_wg_per_cu or 2), False, True)


# ---------------------------------------------------------------------------
# the generic element-wise kernels (any type pair, any alignment) and fq_logic
# (line numbers of the commit that added these three models)
# ---------------------------------------------------------------------------
def ew_arith_generic(cus):
    """arith_kernel<TC>: one row per thread and round of the grid-stride loop"""
    # fq_elementwise.hip:420-423 (prepare)  max_grid = cus * 8; grid = max(1, min(ceil(n / 256), max_grid))
    # fq_elementwise.hip:150, :153 (arith_kernel)  T = gridDim.x * 256 rows per round; row i -> thread i % T
    return Model("ew_arith_generic", THREADS, cus * 8, True, True)


def ew_compare_generic(cus):
    """compare_kernel<TC>: one 64-row bitmap word per wave and round, four per workgroup"""
    # fq_elementwise.hip:542-545 (fq_compare)  nwords = ceil(len / 64); grid = min(ceil(nwords / 4), cus * 8)
    # fq_elementwise.hip:174, :177 (compare_kernel)  W = gridDim.x * 256 / 64 words per round; word w -> wave w % W
    return Model("ew_compare_generic", WAVES * 64, cus * 8, True, True)


def ew_logic(cus):
    """logic_kernel: one pair of bitmap words (16 bytes) per thread and round; an odd last word to the scalar loop"""
    # fq_elementwise.hip:605-609 (fq_logic)  nwords = ceil(len / 64); grid = max(1, min(ceil((nwords / 2) / 256), cus * 2))
    # fq_elementwise.hip:567-568, :576 (logic_kernel)  T = gridDim.x * 256 pairs per round; pair p -> thread p % T
    # (the grid counts whole pairs, so the cap is its upper bound: one word past k * 512 still gives k workgroups)
    return Model("ew_logic", THREADS * 2 * 64, cus * 2, True, False)


# ---------------------------------------------------------------------------
# fq_filter_compact: no capped grid (fq_filter.hip:1128-1132, fq_filter_compact: one workgroup per group of kGroupTiles = 16 tiles
# of kTileWords = 256 bitmap words, one scatter workgroup per tile), so only these sizes matter
# ---------------------------------------------------------------------------
COMPACT_TILE_ROWS = 256 * 64                    # fq_filter.hip:25 kTileWords words of 64 rows
COMPACT_GROUP_ROWS = 16 * COMPACT_TILE_ROWS     # fq_filter.hip:39 kGroupTiles
COMPACT_SCAN_ROUND_GROUPS = 1024 * 16           # fq_filter.hip:89-90, :99 kScanThreads * kScanPer groups per round
COMPACT_SECOND_ROUND_ROWS = COMPACT_SCAN_ROUND_GROUPS * COMPACT_GROUP_ROWS + 1  # 4,294,967,297 rows (32 GiB of u64)
