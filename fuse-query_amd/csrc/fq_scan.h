// One fused-scan launch as prepared by fq_aggregate (fq_aggregate.hip) and
// consumed by either the precompiled program-interpreting kernels or a
// hipRTC-specialised kernel (fq_jit.hip).  Internal; not part of the ABI.
#pragma once

#include <stdlib.h>

#include "fq_common.h"
#include "fq_device.h"

namespace fqk {

constexpr int kThreads = 256;       // 4 waves per workgroup
constexpr int kMaxPartials = 4096;  // workgroups per launch upper bound
// the workspace: kMaxPartials Partials, folded by agg_finalize_kernel
constexpr size_t kPartialsBytes = (size_t)kMaxPartials * sizeof(Partial);

struct Launch {
    const void *col;
    int64_t n;
    int64_t head;  // flat mode: scalar elements before the first 16-byte boundary
    int64_t block_rows;
    bool block_mode;
    KPred pred;
    KProg val;
    uint32_t mask;
    int32_t vdtype;
    Partial *parts;
    int grid;
    hipStream_t stream;
    // fq_aggregate_columns with more than one column (else n_cols == 0): the
    // columns, their dtypes, and whether they share the 16-byte phase that the
    // vector loads need (flat mode: one `head`; block mode: all aligned) --
    // when they do not, the whole scan reads 8 bytes at a time
    int n_cols;
    const void *cols[FQ_MAX_SCAN_COLS];
    int32_t cdt[FQ_MAX_SCAN_COLS];
    bool vec;
    // fq_aggregate_typed with a narrow column, step or comparison (n_cols >= 1):
    // a lane owns `group` consecutive rows of a tile of 256 * group rows and
    // loads its group * width bytes of every column in one piece; `prefetch`:
    // the next tile's pieces in flight.  vec: the columns share one phase
    // (ptr / width) mod group (flat mode: `head` rows lead up to it; block mode:
    // phase 0 and block_rows a multiple of group), else one row per lane.
    bool typed;
    int group;
    bool prefetch;
    // fq_aggregate_nullable (a typed launch): has_bm[j], column j carries an Arrow
    // validity bitmap validity[j] (bit i = row i of cols[j]); the partials behind
    // `parts` are PartialN
    bool nullable;
    bool has_bm[FQ_MAX_SCAN_COLS];
    const uint64_t *validity[FQ_MAX_SCAN_COLS];
    // fq_aggregate_for32_expr: one UInt64 column given as its 32-bit deltas
    // (`col`, 16-byte aligned) and frame bases; a kernel and a shape key of its
    // own (fq_jit_scan_for32), grid as fq_aggregate_for32 in flat mode
    bool for32;
    const uint64_t *for32_base;
};

// Geometry of the scans over a frame-of-reference copy (fq_aggregate_for32,
// fq_jit_scan_for32): a tile is 4 16-byte vectors of 4 deltas per lane, and 16
// whole tiles make a frame, so a tile never straddles one.
constexpr int kFor32FrameShift = 16;  // log2(FQ_FOR32_FRAME_ROWS)
constexpr int64_t kFor32TileRows = 4 * kThreads * 4;
static_assert(((int64_t)1 << kFor32FrameShift) == FQ_FOR32_FRAME_ROWS, "row >> kFor32FrameShift is the frame");
static_assert(FQ_FOR32_FRAME_ROWS % kFor32TileRows == 0, "a tile never straddles a frame");
// workgroups of a flat scan over `len` deltas (flat_max = CUs x FQ_TUNE_SCAN_WG_PER_CU)
inline int for32_flat_grid(int64_t len, int64_t flat_max) {
    int64_t grid = (len / 4 + kFor32TileRows / 4 - 1) / (kFor32TileRows / 4);
    if (grid < 1) grid = 1;
    return (int)(grid < flat_max ? grid : flat_max);
}

// Row group of a typed scan over columns of the given widths: the largest
// power of two G <= 16 with G * sum(w) <= 64 bytes per lane, so that a tile and
// its prefetch stay within the single-column kernel's 128 bytes in flight.  A
// column whose piece G * w would fall below a dword gives up the prefetch for
// twice the bytes per tile instead (scalar narrow loads cost 2-2.5x a dword's),
// when that lifts every piece to a dword (the first rule alone, and the
// doubled group with its prefetch, measured slower and no faster: DESIGN.md
// section 3, profiles/r09_typed_group_ab.json).
inline void typed_group(const int32_t *cdt, int n_cols, int *group, bool *prefetch) {
    int sum = 0, wmin = 8;
    for (int j = 0; j < n_cols; ++j) {
        const int w = fqc::dtype_size(cdt[j]);
        sum += w;
        wmin = w < wmin ? w : wmin;
    }
    auto fit = [sum](int bytes) {
        int g = 16;
        while (g > 1 && g * sum > bytes) g >>= 1;
        return g;
    };
    const int g0 = fit(64), g1 = fit(128);
    *group = g0;
    *prefetch = true;
    if (g0 * wmin < 4 && g1 * wmin >= 4) {
        *group = g1;
        *prefetch = false;
    }
}

// Host lowering (fq_aggregate.hip): fq_expr -> KProg (res_dtype = result
// type) and fq_pred -> KPred.
fq_status lower_expr(const fq_expr &e, int32_t col_dtype, KProg &out, int32_t &res_dtype);
fq_status lower_pred(const fq_pred *pred, int32_t col_dtype, int64_t len, bool need_data, KPred &out);
// The same over the n_cols columns of fq_aggregate_columns (dtypes cdt): the
// column indices in the steps' `bits` / the predicates' `rhs_bits` are read and
// checked, FQ_OP_LOAD is accepted.
fq_status lower_expr_cols(const fq_expr &e, const int32_t *cdt, int n_cols, KProg &out, int32_t &res_dtype);
fq_status lower_pred_cols(const fq_pred *pred, const int32_t *cdt, int n_cols, int64_t len, bool need_data,
                          KPred &out);
// Typed mode (fq_aggregate_typed): columns, steps and comparisons of any numeric
// type; every step type is checked against numerical_coercion of its operands
// and every cast is an explicit K_CAST.
fq_status lower_expr_typed(const fq_expr &e, const int32_t *cdt, int n_cols, KProg &out, int32_t &res_dtype);
fq_status lower_pred_typed(const fq_pred *pred, const int32_t *cdt, int n_cols, int64_t len, bool need_data,
                           KPred &out);
// Argument checks of the *_columns entry points: 1..FQ_MAX_SCAN_COLS columns of
// equal len, each UINT64 / INT64 / FLOAT64 (`who` names the caller in the messages).
fq_status check_cols(const fq_col *cols, int32_t n_cols, bool need_data, const char *who = "fq_aggregate_columns");
// The same for the *_typed entry points (any numeric dtype each), and whether
// every column, step and comparison type of a call is 64-bit (the call then IS
// its *_columns twin).
fq_status check_cols_typed(const fq_col *cols, int32_t n_cols, bool need_data, const char *who);
bool call_is_64(const fq_col *cols, int32_t n_cols, const fq_pred *pred, const fq_expr *value);

// Flat scan over K >= 2 columns: 16-byte vectors per lane per column in a
// tile, the next tile's as many in flight.  One column holds 2 x 4; K columns
// share that budget (2 x K x U <= 8 up to K = 4) so that the registers a lane
// ties up in loads, and with them the waves per SIMD, stay where the
// single-column kernel has them.
// (FQ_SCAN_COLS_VECTORS_3: the A/B of three and four columns, 1 against 2.)
#ifndef FQ_SCAN_COLS_VECTORS_3
#define FQ_SCAN_COLS_VECTORS_3 1
#endif
inline int scan_cols_vectors(int n_cols) { return n_cols <= 2 ? 2 : FQ_SCAN_COLS_VECTORS_3; }

// Launches the scan of `L` from a specialised kernel when the JIT policy
// (fq_jit_config) selects it -- or, with `force` (expression trees, which the
// interpreter does not run), whenever the JIT is not off; *used tells the
// caller whether it did.
fq_status jit_scan(int32_t col_dtype, bool chain, const Launch &L, bool *used, bool force = false);

// expression trees (FQ_OP_PUSH / FQ_OPERAND_STACK) in a lowered program
inline bool prog_has_tree(const KProg &p) {
    for (int i = 0; i < p.n; ++i)
        if (p.s[i].code == K_PUSH) return true;
    return false;
}
inline bool pred_has_tree(const KPred &p) {
    if (p.kind == FQ_PRED_EXPR) return prog_has_tree(p.lhs);
    if (p.kind == FQ_PRED_TREE)
        for (int l = 0; l < p.n_leaves; ++l)
            if (prog_has_tree(p.leaves[l].lhs)) return true;
    return false;
}

// Compiles (and caches) the specialised kernel for L's shape ahead of the
// first scan; *ready = the shape is specialisable.  Without a device the
// source is compiled for gfx950 only to validate it.
fq_status jit_prepare(int32_t col_dtype, bool chain, const Launch &L, bool *ready);

// State replicas of a group table of `cap` slots: workgroup b updates replica
// b % R, so the 256 flushing workgroups (one per CU) contend at most 16-fold
// for one group's state words (the extract folds the replicas).
// R * cap <= 2^22 words per aggregate (32 MB), at most 16 replicas; tables
// of 2^22 slots and more get one.
inline int group_replicas(int64_t cap) {
    int r = 1;
    while (r < 16 && cap * (int64_t)r * 2 <= ((int64_t)1 << 22)) r *= 2;
    return r;
}

// One fq_group_aggregate launch (fq_groupby.hip -> fq_jit.hip).
struct GroupLaunch {
    const void *col;
    int64_t n;
    int64_t head;
    KPred pred;
    KProg key;  // key expression (lowered); n == 0 = the column itself
    int32_t key_dtype;
    int32_t n_aggs;
    int32_t kinds[FQ_MAX_GROUP_AGGS];
    int32_t dtypes[FQ_MAX_GROUP_AGGS];
    bool chain[FQ_MAX_GROUP_AGGS];
    KProg vals[FQ_MAX_GROUP_AGGS];
    uint64_t *keys;  // capacity + 1 slots
    uint64_t *states[FQ_MAX_GROUP_AGGS];
    uint32_t *hdr;
    int64_t capacity;
    int lds_bytes;  // LDS hash table budget per workgroup (sets S and the occupancy)
    int threads;    // workgroup size
    int rowmap;     // 1: lane-consecutive rows (8-byte loads), 0: row pairs per lane (16-byte loads)
    int narrow;     // partitioned path: 4-byte rows (offsets from col[0] - 2^31, FQ_GROUP_NARROW_ROWS)
    int range_bins; // partitioned path: bin = key >> log2(S) and LDS slot = key & (S - 1) (a UInt64
                    // key below d <= P * S: `% d`), else bins by the key's hash
    int grid;
    hipStream_t stream;
    // fq_group_aggregate_columns with more than one column (else n_cols == 0):
    // the columns and their dtypes; key, predicate and arguments name them by
    // number.  `rows`: rows per lane per tile of rows * threads rows (see
    // group_cols_rows); the launch takes its grid from them.
    int n_cols;
    const void *cols[FQ_MAX_SCAN_COLS];
    int32_t cdt[FQ_MAX_SCAN_COLS];
    int rows;
};

// Rows per lane per tile of the GROUP BY kernel over K >= 2 columns: a tile and
// the next tile's loads are 2 x K x rows x 8 <= 128 bytes per lane, the budget
// of the one-column kernel's nxt[8] + raw[8]
constexpr int group_cols_rows(int n_cols) { return n_cols <= 2 ? 4 : 2; }

// Keys of a dense GROUP BY key (a UInt64 key ending in `% d`, d <= the LDS
// slots for n_aggs states in lds_bytes): d, else 0 (fq_jit.hip)
int64_t group_dense_bound(const KProg &key, int32_t key_dtype, int n_aggs, int lds_bytes);
// d for a UInt64 key ending in `% d` / `& (d - 1)` (keys in [0, d)), else 0;
// and the LDS table slots S for n_aggs states in lds_bytes
int64_t group_key_range(const KProg &key, int32_t key_dtype);
int group_lds_slots(int n_aggs, int lds_bytes);

// Launches the hipRTC-specialised group-by kernel for G.
fq_status jit_groupby(int32_t col_dtype, const GroupLaunch &G);
// The same over G.n_cols >= 2 columns (fq_jit_groupby_cols): a module and a
// cache entry of its own, the grid from the rows per lane the shape compiled
// with.  Nothing is launched for n == 0 or without a device (the shape is then
// compiled for gfx950 only).
fq_status jit_groupby_columns(const GroupLaunch &G);

// The partitioned (high-cardinality) path of fq_group_aggregate_partitioned:
// partition into block chains -> blocks grouped by bin -> per-bin
// aggregation, in the caller's workspace (fq_groupby.hip lays it out).
constexpr int kMaxPartGrid = 1024;    // workgroups of the partition kernel
constexpr int kPartBlockRows = 256;   // rows per partition block (2 KB of u64; narrow blocks hold 2x the rows)
struct GroupPartition {
    int log2p;            // bits 0..7: 1..8, P = 2^log2p bins; bits 8..15: the key shift of range bins
    int grid;             // workgroups of fq_jit_gpart
    int bins_grid;        // workgroups of fq_jit_groupby_bins
    uint32_t max_blocks;  // blocks the workspace holds
    uint32_t q;           // blocks per workgroup region: workgroup w of fq_jit_gpart owns [w q, (w + 1) q)
    uint32_t *head;       // [kMaxPartGrid] blocks used per region + [256] blocks per bin: zeroed per launch
    size_t head_bytes;
    uint32_t *used;       // [grid] (head)
    uint32_t *bin_blocks; // [P] blocks per bin (head + kMaxPartGrid)
    uint32_t *bstart;     // [P + 1] each bin's first entry in order
    uint32_t *cursor;     // [P] scatter cursors
    uint32_t *blk_bin;    // [max_blocks] each block's bin
    uint32_t *blk_fill;   // [max_blocks] its rows
    uint64_t *order;      // [max_blocks] block | rows << 32, grouped by bin
    void *vals;           // max_blocks x kPartBlockRows rows (8-byte values, or 4-byte offsets when narrow)
};
fq_status jit_groupby_partitioned(int32_t col_dtype, const GroupLaunch &G, const GroupPartition &X);
// the blocks of fq_jit_gpart grouped by bin: a scan of X.bin_blocks into
// X.bstart, then a scatter of the block numbers into X.order (fq_groupby.hip)
fq_status launch_group_part_blocks(const GroupPartition &X, hipStream_t stream);

// One fq_filter_project / fq_predicate_bitmap call (fq_filter.hip ->
// fq_jit.hip): FilterTransform's predicate and ProjectionTransform's
// expressions over one 64-bit column, hipRTC-specialised per shape.
struct ProjLaunch {
    const void *col;
    int64_t n;
    KPred pred;  // FQ_PRED_NONE / EXPR / TREE (a BITMAP predicate skips the bits kernel)
    int32_t n_out;
    KProg vals[FQ_MAX_PROJECT];
    bool chain[FQ_MAX_PROJECT];
    int32_t dtypes[FQ_MAX_PROJECT];
    void *out[FQ_MAX_PROJECT];
    hipStream_t stream;
    // the *_columns entry points with more than one column (else n_cols == 0):
    // the columns and their dtypes, as in Launch
    int n_cols;
    const void *cols[FQ_MAX_SCAN_COLS];
    int32_t cdt[FQ_MAX_SCAN_COLS];
    // the *_typed entry points with a narrow column, step, comparison or output
    // (n_cols >= 1): `rows` per thread per tile of 256 * rows rows; in the
    // block-stream and map kernels a lane owns `group` consecutive rows and
    // loads its group * width bytes of every column in one piece
    // (typed_project_geometry)
    bool typed;
    int rows;
    int group;
    // fq_filter_project_blocks_for32 (jit_project_blocks only): col holds the
    // per-frame 32-bit deltas of an encoded UInt64 column, for32_base its frame
    // bases, and the n rows are [for32_first, for32_first + n) of it
    bool for32;
    const uint64_t *for32_base;
    int64_t for32_first;
    // fq_filter_project_blocks_nullable / fq_predicate_bitmap_nullable (a typed
    // launch; jit_project_blocks and jit_project_bits only): has_bm[j], column j
    // carries an Arrow validity bitmap validity[j] (bit i = row i of cols[j]);
    // out_validity[j]: output j's bitmap (bit p = row p of out[j]; zeroed by the
    // caller on the stream), null only where project_output_nullable is false
    bool nullable;
    bool has_bm[FQ_MAX_SCAN_COLS];
    const uint64_t *validity[FQ_MAX_SCAN_COLS];
    uint64_t *out_validity[FQ_MAX_PROJECT];
};
// output j of a nullable launch can hold a null: the lowering gives its value a
// validity expression (a column with a bitmap, or a cast that can leave its range)
bool project_output_nullable(const ProjLaunch &P, int j);

// Load geometry of a typed projection over columns of widths cdt whose widest
// output has wout bytes.  Rows per thread per tile R: the largest power of two
// <= 32 with R * sum(w) <= 384 bytes of row data per lane (the measured K = 3
// point of project_cols_rows: 16 rows of three 8-byte columns) and R * wout <=
// 128, so that the LDS stage of one output of one tile stays within the 32 KB
// the 64-bit kernels use; the tile of 256 * R rows never exceeds
// FQ_PROJECT_MIN_BLOCK_ROWS.  Row group G: the largest power of two <= 16 and
// <= R with G * sum(w) <= 128 bytes (typed_group's bound without a prefetch:
// the tile's other groups are the loads in flight); G >= 4, so every piece is a
// 4- or 8-byte word or whole 16-byte vectors.
inline void typed_project_geometry(const int32_t *cdt, int n_cols, int wout, int *rows, int *group) {
    int sum = 0;
    for (int j = 0; j < n_cols; ++j) sum += fqc::dtype_size(cdt[j]);
    int r = 32;
    while (r > 1 && (r * sum > 384 || r * wout > 128)) r >>= 1;
    int g = 16;
    while (g > 1 && (g > r || g * sum > 128)) g >>= 1;
    *rows = r;
    *group = g;
}

// Rows per thread per tile of the look-back and block-stream kernels over K
// columns: 16, 16, 8 for K = 2, 3, 4 (64, 96, 64 VGPRs of row data; one column
// holds 32 rows, 64 VGPRs).  Dividing 32 by K and rounding down (8 at K = 3)
// kept the registers where the single-column kernels have them but measured
// 9-17 % slower than 16: half the barriers and status words per row win
// (profiles/r08_project_columns_rows_ab.json).
constexpr int project_cols_rows(int n_cols) { return n_cols <= 1 ? 32 : (n_cols <= 3 ? 16 : 8); }

// predicate -> LSB-first bitmap words; predicate errors OR-ed into *d_flag
fq_status jit_project_bits(int32_t col_dtype, const ProjLaunch &P, uint64_t *d_bitmap, uint32_t *d_flag);
// one pass: predicate (or P.pred.bitmap), decoupled look-back over tiles of
// select_tile_rows() rows for the output offsets, the n_out outputs of the kept
// rows.  status: one zeroed word per tile; ticket: one zeroed word;
// d_flags[0] predicate errors, d_flags[1] expression errors (bit 31: the
// look-back gave up); *d_total = rows kept.
// tile = select_threads() x select_rows_per_thread() rows, s_sleep
// select_sleep() between look-back polls of a predecessor that has not
// published (round-2 sweeps, tools/select_sweep.sh; their knobs were removed
// in round 6)
constexpr int select_threads() { return 256; }
constexpr int select_rows_per_thread() { return 32; }
constexpr int select_sleep() { return 2; }
constexpr int64_t select_tile_rows(int n_cols = 1) { return (int64_t)select_threads() * project_cols_rows(n_cols); }
// the look-back tile of P: a typed call's 256 * rows
inline int64_t project_tile_rows(const ProjLaunch &P) {
    return P.typed ? (int64_t)select_threads() * P.rows : select_tile_rows(P.n_cols);
}
fq_status jit_project_select(int32_t col_dtype, const ProjLaunch &P, const uint64_t *d_bitmap, uint64_t *status,
                             uint32_t *ticket, uint32_t *d_flags, uint64_t *d_total);
// stream of DataBlocks of block_rows rows (fq_filter_project_blocks): block b's
// kept rows -> output rows [b * block_rows, + d_counts[b]); tiles of
// kProjectBlockTile rows (kProjectBlockThreads threads), block_rows >= the tile;
// d_flags / *d_total / *d_ticket as jit_project_select (zeroed by the caller)
constexpr int kProjectBlockThreads = 256;
constexpr int64_t kProjectBlockTile = 256 * 32;
fq_status jit_project_blocks(int32_t col_dtype, const ProjLaunch &P, int64_t block_rows, const uint64_t *d_bitmap,
                             int64_t *d_counts, uint32_t *d_flags, uint64_t *d_total, uint32_t *d_ticket);
// filter_project_blocks_enqueue / _result: fq_common.h (the engine calls them)
// no predicate: every row -> the n_out outputs
fq_status jit_project_map(int32_t col_dtype, const ProjLaunch &P, uint32_t *d_flag);
// hipRTC loadable and the policy not FQ_JIT_OFF
bool jit_project_available();
// compiles (and caches) P's module; without a device the source is compiled
// for gfx950 only to validate it
fq_status jit_project_prepare(int32_t col_dtype, const ProjLaunch &P);

// Counts a fused (non-identity) scan that ran on the interpreting kernel.
void jit_count_interp();

}  // namespace fqk
