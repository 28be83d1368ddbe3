/*
 * fq_gpu.h -- C ABI of the MI355X (gfx950) kernels behind fuse-query's
 * DataBlock expression + aggregation hot path.
 *
 * Every entry point replaces one call site of the reference's CPU path
 * (dantengsky/fuse-query @ /root/reference, Rust + arrow 2.0 compute):
 *
 *   fq_fill_numbers_u64   NumbersStream::poll_next        src/datasources/system/numbers_stream.rs:65-83
 *   fq_fill_value         DataValue::to_array             src/datavalues/data_value.rs:77-111
 *   fq_aggregate          AggregatorFunction::accumulate  src/functions/function_aggregator.rs:57-100
 *                         (-> data_array_aggregate_op     src/datavalues/data_array_aggregate.rs:14-163,
 *                             arrow::compute::sum/min/max src/datavalues/macros.rs:143-157)
 *                         fused with the argument eval    src/functions/function_arithmetic.rs:64-72
 *                         and the WHERE predicate         src/transforms/transform_filter.rs:38-55
 *   fq_arith              data_array_arithmetic_op        src/datavalues/data_array_arithmetic.rs:14-55
 *   fq_compare            data_array_comparison_op        src/datavalues/data_array_comparison.rs:14-94
 *   fq_filter_compact     arrow filter_record_batch       src/transforms/transform_filter.rs:51
 *   fq_logic              data_array_logic_op             src/datavalues/data_array_logic.rs:10-31
 *   fq_state_merge        AggregatorFunction::merge_state src/functions/function_aggregator.rs:106-139
 *
 * Conventions:
 *   - plain pointers and sizes only; device buffers are owned by the caller and
 *     are never freed by the library;
 *   - column values use the Arrow layout: a contiguous values buffer (16-byte
 *     aligned for the vector path), no null bitmap; Boolean columns are
 *     LSB-first bit-packed into little-endian uint64 words;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); every
 *     call is asynchronous on that stream unless documented otherwise;
 *   - errors are returned as fq_status and the message (the reference's
 *     FuseQueryError display text where one exists, e.g.
 *     "Internal Error: Divide by zero error") is kept in a thread-local buffer
 *     readable with fq_last_error().
 */
#ifndef FQ_GPU_H
#define FQ_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FQ_ABI_VERSION 3

/* ---- status (src/error.rs:10-22 FuseQueryError{SQLParse,Plan,Internal}) ---- */
typedef int32_t fq_status;
#define FQ_OK 0
#define FQ_E_INTERNAL 1       /* FuseQueryError::Internal                       */
#define FQ_E_PLAN 2           /* FuseQueryError::Plan                           */
#define FQ_E_DIVIDE_BY_ZERO 3 /* ArrowError::DivideByZero -> Internal (error.rs:24-28) */
#define FQ_E_UNSUPPORTED 4    /* not supported on the device path (message says what) */
#define FQ_E_HIP 5            /* HIP runtime error / no GPU                     */
#define FQ_E_RCCL 6           /* RCCL error                                     */
#define FQ_E_INVALID 7        /* bad argument (null pointer, misaligned buffer, ...) */

/* ---- DataType (arrow::datatypes::DataType as used by src/datavalues/data_type.rs) ---- */
#define FQ_DT_NULL 0
#define FQ_DT_BOOLEAN 1
#define FQ_DT_INT8 2
#define FQ_DT_INT16 3
#define FQ_DT_INT32 4
#define FQ_DT_INT64 5
#define FQ_DT_UINT8 6
#define FQ_DT_UINT16 7
#define FQ_DT_UINT32 8
#define FQ_DT_UINT64 9
#define FQ_DT_FLOAT32 10
#define FQ_DT_FLOAT64 11
#define FQ_DT_UTF8 12

/* ---- operators (src/datavalues/data_value_operator.rs:5-81) ---- */
#define FQ_OP_ADD 0
#define FQ_OP_SUB 1
#define FQ_OP_MUL 2
#define FQ_OP_DIV 3
#define FQ_OP_MOD 4 /* EXTENSION: '%' has no arm in function_factory.rs:17-39 */
#define FQ_OP_PUSH 5 /* fq_step only: push acc, acc = the column (see FQ_OPERAND_STACK) */
#define FQ_OP_LOAD 6 /* fq_step only, fq_aggregate_columns: acc = column[bits] (no push) */

#define FQ_CMP_EQ 0
#define FQ_CMP_LT 1
#define FQ_CMP_LTEQ 2
#define FQ_CMP_GT 3
#define FQ_CMP_GTEQ 4

/* aggregate op bit mask (DataValueAggregateOperator) */
#define FQ_AGG_MIN 1u
#define FQ_AGG_MAX 2u
#define FQ_AGG_SUM 4u
#define FQ_AGG_COUNT 8u

/*
 * A scalar DataValue (src/datavalues/data_value.rs:20-35), numeric/boolean
 * subset.  dtype FQ_DT_NULL is DataValue::Null; is_some=0 is `X(None)`.
 * bits: integers hold the value sign/zero-extended to 64 bits, floats hold
 * the IEEE binary64 bits (Float32 values are widened exactly), booleans 0/1.
 */
typedef struct fq_value {
    int32_t dtype;
    int32_t is_some;
    uint64_t bits;
} fq_value;

/* A device column: Arrow PrimitiveArray values buffer (or Boolean bitmap). */
typedef struct fq_col {
    void *data; /* device pointer */
    int64_t len;
    int32_t dtype;
    int32_t reserved;
} fq_col;

/*
 * Fusable expression: a chain of binary operators applied to one column x,
 *   acc = x;  for each step: acc = acc OP operand   (or operand OP acc if reversed)
 * where operand is a constant or x itself.  This is the shape that
 * Function::eval produces for ArithmeticFunction trees whose every right (or
 * left) child is a Constant/Field leaf (function_arithmetic.rs:64-72).
 * Each step carries the coerced type of that step
 * (numerical_coercion, data_type.rs:27-90); the library inserts the casts.
 */
#define FQ_MAX_STEPS 8
#define FQ_OPERAND_CONST 0
#define FQ_OPERAND_COLUMN 1
/* Expression TREES over the one column (e.g. (x + 1) + (x / 2)) use a
 * two-deep value stack: FQ_OP_PUSH pushes acc and restarts acc = x; a later
 * step with operand FQ_OPERAND_STACK pops that value as its operand
 * (reversed = 1: popped OP acc, the left subtree first, as the reference
 * evaluates ArithmeticFunction's children, function_arithmetic.rs:64-72).
 * The popped value is cast to the step's dtype like acc.  Trees run on the
 * hipRTC-specialised kernels only (FQ_E_UNSUPPORTED with FQ_JIT_OFF).     */
#define FQ_OPERAND_STACK 2
#define FQ_MAX_STACK 2
typedef struct fq_step {
    int32_t op;       /* FQ_OP_*                                  */
    int32_t operand;  /* FQ_OPERAND_CONST / FQ_OPERAND_COLUMN     */
    int32_t reversed; /* 1: operand OP acc (scalar-array form)    */
    int32_t dtype;    /* UINT64 / INT64 / FLOAT64 (fq_aggregate_typed: any numeric type) */
    uint64_t bits;    /* constant in `dtype` (fq_value encoding)  */
} fq_step;

typedef struct fq_expr {
    int32_t n_steps; /* 0 = identity (the column itself)            */
    int32_t out_dtype; /* type of the result; == column type if n_steps==0 */
    fq_step steps[FQ_MAX_STEPS];
} fq_expr;

/* WHERE predicate, fused into the aggregate scan (transform_filter.rs:38-55). */
#define FQ_PRED_NONE 0
#define FQ_PRED_EXPR 1   /* cmp(lhs(x), rhs) with rhs a constant or x            */
#define FQ_PRED_BITMAP 2 /* precomputed Boolean column (from fq_compare)          */
#define FQ_PRED_TREE 3   /* and/or of up to FQ_MAX_PRED_LEAVES comparisons        */

/* One comparison leaf of an and/or predicate tree: cmp(lhs(x), rhs). */
typedef struct fq_pred_leaf {
    int32_t cmp, cmp_dtype, rhs_operand, reserved;
    uint64_t rhs_bits;
    fq_expr lhs;
} fq_pred_leaf;

/* LogicFunction trees (function_logic.rs) over comparisons of one column, as
 * a postfix program: prog[i] < FQ_MAX_PRED_LEAVES pushes leaf prog[i],
 * FQ_PRED_AND / FQ_PRED_OR pop two and push their and/or.  Both sides are
 * always evaluated (arrow and/or work on whole arrays), so an error in
 * either raises.                                                          */
#define FQ_MAX_PRED_LEAVES 4
#define FQ_PRED_AND 100
#define FQ_PRED_OR 101
typedef struct fq_pred_tree {
    int32_t n_leaves;
    int32_t n_prog;
    int32_t prog[2 * FQ_MAX_PRED_LEAVES];
    fq_pred_leaf leaves[FQ_MAX_PRED_LEAVES];
} fq_pred_tree;

typedef struct fq_pred {
    int32_t kind;
    int32_t cmp;         /* FQ_CMP_*  (already flipped for scalar-array forms)   */
    int32_t cmp_dtype;   /* equal_coercion type: UINT64 / INT64 / FLOAT64 (fq_aggregate_typed: any numeric) */
    int32_t rhs_operand; /* FQ_OPERAND_CONST / FQ_OPERAND_COLUMN                  */
    uint64_t rhs_bits;   /* constant in cmp_dtype                                */
    fq_expr lhs;         /* lhs.out_dtype must equal cmp_dtype                   */
    const uint64_t *bitmap; /* device, kind == FQ_PRED_BITMAP                    */
    const fq_pred_tree *tree; /* host, kind == FQ_PRED_TREE (read during the call) */
} fq_pred;

/*
 * Partial aggregate over one device block = a run of `blocks` reference
 * blocks of `block_rows` rows (numbers_stream.rs:29 block_size = 10000; the
 * last one may be shorter).  Values are in `dtype` (fq_value bit encoding).
 * flags lets the host replay the reference's per-block state machine exactly:
 *   FQ_STATE_ANY_EMPTY   some reference block had no row left after the
 *                        predicate (arrow sum -> None -> the Sum state errors,
 *                        data_value_arithmetic.rs:10-27)
 *   FQ_STATE_DIV_ZERO    a row reaching an integer/float '/' or '%' had a zero
 *                        divisor (ArrowError::DivideByZero)
 *   FQ_STATE_CAST_NULL   a coercion cast overflowed (arrow cast -> null; nulls
 *                        are not representable on the device path)
 */
#define FQ_STATE_ANY_EMPTY 1u
#define FQ_STATE_DIV_ZERO 2u
#define FQ_STATE_CAST_NULL 4u
typedef struct fq_agg_state {
    uint64_t sum;   /* wrapping sum (integers) / binary64 sum bits (floats)      */
    uint64_t max;    /* float dtypes: f64::max / f64::min folds -- a NaN row is ignored */
    uint64_t min;    /* unless every kept row is NaN (then NaN, with count > 0)      */
    uint64_t count;  /* rows that passed the predicate                           */
    uint64_t blocks; /* reference blocks covered                                 */
    uint32_t flags;
    int32_t dtype; /* value dtype                                               */
} fq_agg_state;

/* ---- library ---- */
int32_t fq_abi_version(void);
const char *fq_last_error(void);
fq_status fq_device_count(int32_t *out);

/* ---- SourceTransform: system.numbers_mt (numbers_stream.rs:65-83) ----
 * Writes d_out[i] = begin + i for i in [0, count).  One partition of
 * numbers_mt is one contiguous range (see SURVEY.md finding 8).            */
fq_status fq_fill_numbers_u64(uint64_t *d_out, uint64_t begin, uint64_t count, void *stream);
/* Anti-closed-form control column: d_out[i] = splitmix64(seed, first_index + i). */
fq_status fq_fill_splitmix64(uint64_t *d_out, uint64_t seed, uint64_t first_index,
                             uint64_t count, void *stream);

/* DataValue::to_array(size) (data_value.rs:77-111): broadcast one scalar.
 * dtype is a numeric type (bits in fq_value encoding) or FQ_DT_BOOLEAN
 * (writes ceil(n/64) bitmap words, bits past n cleared).                   */
fq_status fq_fill_value(void *d_out, int64_t n, int32_t dtype, uint64_t bits, void *stream);

/* ---- AggregatePartial: fused predicate + argument expression + sum/max/min/count ----
 * One pass over `col`; writes one fq_agg_state to device memory d_out.
 * block_rows: reference block size of this device block (10000 for
 * numbers_mt, or col->len for a single DataBlock).  Workspace is device
 * memory of at least fq_aggregate_workspace_bytes(col->len) bytes.
 * value may be NULL (identity).  pred may be NULL (no WHERE).
 *
 * The scan writes one partial per workgroup into the workspace; a second,
 * one-workgroup launch folds them into *d_out in a fixed order (the same
 * bytes run to run, float sums too).  Calls sharing a workspace must be
 * ordered (one stream).                                                     */
size_t fq_aggregate_workspace_bytes(int64_t len);
fq_status fq_aggregate(const fq_col *col, int64_t block_rows, const fq_pred *pred,
                       const fq_expr *value, uint32_t agg_mask, fq_agg_state *d_out,
                       void *d_ws, size_t ws_bytes, void *stream);

/* ---- The same scan over up to FQ_MAX_SCAN_COLS 64-bit columns of one block ----
 * (`sum(a * b) WHERE c < k`: Function trees range over every field of a
 * DataBlock, function_field.rs:33-40).  cols[0..n_cols) have equal len and a
 * dtype each among UINT64 / INT64 / FLOAT64 (FQ_E_UNSUPPORTED for a narrow
 * one).  Column references use fields that the single-column entry points
 * ignore:
 *   - a step with operand FQ_OPERAND_COLUMN reads column `bits`;
 *   - FQ_OP_PUSH restarts acc from column `bits`;
 *   - an expression starts as column 0 unless its first step is FQ_OP_LOAD,
 *     which starts it as column `bits`;
 *   - a predicate (or tree leaf) with rhs_operand FQ_OPERAND_COLUMN compares
 *     against column `rhs_bits`.
 * Each step's dtype is the coerced type; the casts of acc and of the operand
 * column (from that column's own dtype) are inserted by the library with the
 * rules of fq_aggregate.  Errors keep the reference's order: a predicate
 * error on any row, then a value error on a kept row only.  Workspace,
 * block_rows, predicate kinds, flags and the fixed-order fold are
 * fq_aggregate's; with n_cols == 1 the call IS fq_aggregate.  Scans over more
 * than one column run on hipRTC-specialised kernels only, whatever min_rows
 * says (FQ_E_UNSUPPORTED with FQ_JIT_OFF or without hipRTC).                */
#define FQ_MAX_SCAN_COLS 4
fq_status fq_aggregate_columns(const fq_col *cols, int32_t n_cols, int64_t block_rows,
                               const fq_pred *pred, const fq_expr *value, uint32_t agg_mask,
                               fq_agg_state *d_out, void *d_ws, size_t ws_bytes, void *stream);

/* ---- The same scan over columns, steps and comparisons of any numeric type ----
 * (numerical_coercion ranges over all ten numeric types, data_type.rs:27-87: a
 * host brings dates as Int32, quantities as UInt8, discounts as Float32).
 * cols[0..n_cols) have equal len and any numeric dtype each; the column
 * references, workspace, block_rows, predicate kinds, flags, the fixed-order
 * fold and the error order are fq_aggregate_columns'.  Every fq_step.dtype,
 * cmp_dtype and out_dtype may be any numeric type, and must be the type that
 * numerical_coercion / equal_coercion yields for its operands (FQ_E_INVALID
 * otherwise; for a constant operand: a type at or before acc's in the
 * coercion order).  A step or comparison in type T sees acc, a column operand
 * and a popped stack value cast to T as arrow 2.0 casts: an integer outside
 * T's range is arrow's null, FQ_STATE_CAST_NULL on a live row; integer ->
 * float rounds to nearest; Float32 -> Float64 is exact.  A constant arrives
 * already in the step's type (fq_value encoding).  Integer steps of width w
 * wrap modulo 2^w, '/' and '%' truncate (T::MIN / -1 wraps to T::MIN,
 * T::MIN % -1 = 0), Float32 steps round to binary32 one step at a time ('%'
 * is fmodf); a zero divisor on a live row sets FQ_STATE_DIV_ZERO.  The state
 * is in the value's type V with the encoding of a scan over a single narrow
 * column: integer sums wrap at V's width and are stored sign- or
 * zero-extended, Float32 accumulates in binary32 and is stored widened.
 *
 * When every column, step and comparison type is 64-bit the call IS
 * fq_aggregate_columns.  Any other shape runs on hipRTC-specialised kernels
 * only, whatever min_rows says (FQ_E_UNSUPPORTED with FQ_JIT_OFF or without
 * hipRTC).  fq_jit_prepare_typed compiles (and caches) the kernel of a call
 * shape ahead of the first scan (the columns' data may be NULL: they then
 * count as aligned); without a GPU the generated source is compiled for
 * gfx950 only to validate it.                                               */
fq_status fq_aggregate_typed(const fq_col *cols, int32_t n_cols, int64_t block_rows,
                             const fq_pred *pred, const fq_expr *value, uint32_t agg_mask,
                             fq_agg_state *d_out, void *d_ws, size_t ws_bytes, void *stream);
fq_status fq_jit_prepare_typed(const fq_col *cols, int32_t n_cols, int64_t block_rows,
                               const fq_pred *pred, const fq_expr *value, uint32_t agg_mask,
                               int32_t *specialised);

/* ---- The same scan over nullable columns (Arrow validity bitmaps) ----
 * validity[j] belongs to cols[j]: NULL (every row valid) or a device pointer,
 * 8-byte aligned (FQ_E_INVALID otherwise), to ceil(len / 64) u64 words whose
 * bit i (LSB first, as Boolean columns are laid out) is 1 when row i of
 * cols[j].data is valid.  Bit 0 is row 0 of cols[j].data: a sliced array whose
 * bitmap has a bit offset is the host's to re-base.  Bits at and past len are
 * ignored and no word past ceil(len / 64) is read.  `validity` itself must be
 * non-NULL.  A value under a 0 bit never influences a result, a flag or an
 * error.  The rules are arrow 2.0's as the reference uses them:
 *   - a constant is valid; a step is valid iff both operands are; a cast is
 *     valid iff its input is and the value is in range -- an out-of-range cast
 *     is a null here, FQ_STATE_CAST_NULL is never set;
 *   - FQ_STATE_DIV_ZERO: a zero divisor on a live row whose operands are both
 *     valid (predicate: any row; value: kept rows);
 *   - a comparison is null if either side is; an and / or node is null if
 *     either side is (arrow 2.0 combines the null bitmaps: `true or null` is
 *     null); a row is kept iff the predicate is valid and true.  An
 *     FQ_PRED_BITMAP predicate has no validity of its own;
 *   - count = kept rows, nulls included; valid = kept rows whose value is
 *     valid; sum / max / min fold those and hold a value iff valid > 0 (no scan
 *     runs for a request of count alone without predicate and expression:
 *     valid is then 0);
 *   - FQ_STATE_ANY_EMPTY: some reference block had no valid kept value, with
 *     or without a predicate (reported, as by the other entry points, when
 *     agg_mask has FQ_AGG_SUM or the scan covers a single reference block).
 * Arguments, coercion checks, block_rows, predicate kinds and the fixed-order
 * fold are fq_aggregate_typed's.  This entry point always runs the typed
 * hipRTC kernels, 64-bit shapes included (FQ_E_UNSUPPORTED with FQ_JIT_OFF or
 * without hipRTC); a column without a bitmap costs no bitmap load.  The
 * workspace holds 64-byte partials: fq_aggregate_nullable_workspace_bytes.
 * fq_jit_prepare_nullable: has_validity[j] != 0 where the call will pass a
 * bitmap (NULL: none).                                                       */
typedef struct fq_agg_state_n {   /* 64 bytes */
    fq_agg_state s;               /* count = rows kept by the predicate (nulls included) */
    uint64_t valid;               /* kept rows whose value is valid: sum/max/min hold a value iff valid > 0 */
    uint64_t reserved;
} fq_agg_state_n;
size_t fq_aggregate_nullable_workspace_bytes(int64_t len);
fq_status fq_aggregate_nullable(const fq_col *cols, const uint64_t *const *validity, int32_t n_cols,
                                int64_t block_rows, const fq_pred *pred, const fq_expr *value,
                                uint32_t agg_mask, fq_agg_state_n *d_out, void *d_ws, size_t ws_bytes,
                                void *stream);
fq_status fq_jit_prepare_nullable(const fq_col *cols, const uint8_t *has_validity, int32_t n_cols,
                                  int64_t block_rows, const fq_pred *pred, const fq_expr *value,
                                  uint32_t agg_mask, int32_t *specialised);

/* ---- Frame-of-reference storage of a resident UInt64 column (no reference
 * counterpart: the reference regenerates numbers_mt for every query) ----
 * A frame is FQ_FOR32_FRAME_ROWS consecutive rows.  An encoded column is
 *   base[fq_for32_frames(len)]  each frame's minimum, and
 *   delta[len]                  delta[i] = value[i] - base[i / FQ_FOR32_FRAME_ROWS]
 * in 32 bits: half the bytes of the plain column wherever the values of a
 * frame span less than 2^32.  Lossless: base[i / F] + delta[i] is value[i].
 * fq_for32_delta_bytes / fq_for32_base_bytes size the two buffers (delta
 * rounded up to 256 bytes); delta must be 16-byte aligned.
 *
 * fq_for32_encode computes every frame's minimum and maximum from the data,
 * writes bases and deltas, and leaves *d_flag (4 bytes of device memory, zeroed
 * by the call) 0, or 1 when some frame has max - min > 0xFFFFFFFF: the column
 * is then not encodable and the buffers' contents are to be discarded.
 * Asynchronous on `stream`; the caller reads the flag after waiting for it.
 *
 * fq_aggregate_for32 is fq_aggregate over the encoded column with block_rows
 * = 0, no predicate and no expression: the same fq_agg_state, bit for bit
 * (wrapping sum, max, min, count, flags 0, dtype UInt64), from 4 bytes per row
 * read.  Workspace and the fixed-order fold are fq_aggregate's; a request for
 * count alone reads nothing.  FQ_E_INVALID for a delta pointer that is not
 * 16-byte aligned or unknown bits in agg_mask.
 *
 * fq_aggregate_for32_expr is fq_aggregate over the UInt64 column
 * base[i / FQ_FOR32_FRAME_ROWS] + delta[i] with the same block_rows, pred,
 * value and agg_mask: the same fq_agg_state (integer sum, max, min and count,
 * blocks, flags and dtype bit for bit; a Float64 max/min bit for bit up to the
 * sign of a zero extreme; a Float64 sum bit for bit wherever it is exactly
 * summable -- a lane owns other rows here than in the plain scan), and the same
 * error order.  Without predicate and expression the call is
 * fq_aggregate_for32 (over block_rows' blocks).  Any other shape runs on a
 * hipRTC-specialised kernel of its own (fq_jit_scan_for32) whatever min_rows
 * says: FQ_E_UNSUPPORTED with FQ_JIT_OFF or without hipRTC.  Argument errors
 * are fq_aggregate_for32's.  fq_jit_prepare_for32 compiles that kernel ahead
 * of the first scan (*specialised = 0 for the call without predicate and
 * expression, whose kernel is precompiled); without a GPU the source is
 * compiled for gfx950 only to validate it.                                  */
#define FQ_FOR32_FRAME_ROWS 65536
int64_t fq_for32_frames(int64_t len);
size_t fq_for32_delta_bytes(int64_t len);
size_t fq_for32_base_bytes(int64_t len);
fq_status fq_for32_encode(const fq_col *col, uint64_t *d_base, uint32_t *d_delta, uint32_t *d_flag, void *stream);
fq_status fq_aggregate_for32(const uint32_t *d_delta, const uint64_t *d_base, int64_t len, uint32_t agg_mask,
                             fq_agg_state *d_out, void *d_ws, size_t ws_bytes, void *stream);
fq_status fq_aggregate_for32_expr(const uint32_t *d_delta, const uint64_t *d_base, int64_t len, int64_t block_rows,
                                  const fq_pred *pred, const fq_expr *value, uint32_t agg_mask, fq_agg_state *d_out,
                                  void *d_ws, size_t ws_bytes, void *stream);
fq_status fq_jit_prepare_for32(int64_t len, int64_t block_rows, const fq_pred *pred, const fq_expr *value,
                               uint32_t agg_mask, int32_t *specialised);

/* ---- ArithmeticFunction::eval (data_array_arithmetic.rs:14-55) ----
 * Exactly one of {lhs, lhs_scalar} and one of {rhs, rhs_scalar} is non-NULL.
 * out->data must hold out->len elements of the coercion type returned by
 * fq_arith_result_type.  d_flag: 4 bytes of device scratch; when non-NULL the
 * call synchronises `stream` and reports FQ_E_DIVIDE_BY_ZERO / cast nulls.   */
fq_status fq_arith_result_type(int32_t op, int32_t lhs_dtype, int32_t rhs_dtype, int32_t *out);
fq_status fq_arith(int32_t op, const fq_col *lhs, const fq_value *lhs_scalar, const fq_col *rhs,
                   const fq_value *rhs_scalar, fq_col *out, uint32_t *d_flag, void *stream);

/* ---- ComparisonFunction::eval (data_array_comparison.rs:14-94) ----
 * Writes an LSB-first bitmap of ceil(len/64) uint64 words (bits past len are 0).
 * Scalar-array forms flip the operator as the reference does (:76-84).       */
fq_status fq_compare(int32_t cmp, const fq_col *lhs, const fq_value *lhs_scalar,
                     const fq_col *rhs, const fq_value *rhs_scalar, uint64_t *d_bitmap,
                     int64_t len, uint32_t *d_flag, void *stream);

/* ---- LogicFunction::eval (function_logic.rs:47-53 -> data_array_logic.rs:10-31) ----
 * out = lhs AND/OR rhs over two Boolean bitmaps of `len` rows (ceil(len/64)
 * words each; bits past len are cleared in the output).  Both sides must be
 * Boolean ARRAYS: the reference errors on a scalar side ("Cannot do
 * data_array and, left:..., right:...") and on a non-Boolean array
 * ("Cannot downcast_array from datatype:<T> item to:BooleanArray"); those
 * checks are the caller's (engine/functions.cpp LogicFunction).          */
#define FQ_LOGIC_AND 0
#define FQ_LOGIC_OR 1
fq_status fq_logic(int32_t op, const uint64_t *d_lhs, const uint64_t *d_rhs, uint64_t *d_out, int64_t len,
                   void *stream);

/* ---- FilterTransform: order-preserving compaction (arrow filter_record_batch) ----
 * Synchronises `stream`; *out_len receives the number of rows kept.          */
size_t fq_filter_workspace_bytes(int64_t len);
fq_status fq_filter_compact(const fq_col *in, const uint64_t *d_bitmap, void *d_out,
                            int64_t *out_len, void *d_ws, size_t ws_bytes, void *stream);

/* ---- FilterTransform -> ProjectionTransform fused over one column ----
 * (transform_filter.rs:38-55 then transform_projection.rs:45-56 /
 * stream_expression.rs:37-50, for a predicate and expressions over the same
 * 64-bit column).  Keeps the rows of `col` where `pred` holds (NULL or
 * FQ_PRED_NONE: every row; FQ_PRED_BITMAP: the given bitmap) in order and
 * writes d_out[j][r] = values[j](kept row r) for j < n_out
 * (values[j].n_steps == 0: the column itself; the element type is
 * values[j].out_dtype, 8 bytes).  Errors follow the reference's order: a
 * predicate error on any row first ("Internal Error: Divide by zero error",
 * cast nulls), then an expression error on a kept row.  hipRTC-specialised
 * per expression shape (FQ_E_UNSUPPORTED when hipRTC is unavailable or the
 * JIT is off: the caller then runs fq_compare / fq_filter_compact /
 * fq_arith).  Synchronises `stream`; *out_len = rows kept.                  */
#define FQ_MAX_PROJECT 8
size_t fq_filter_project_workspace_bytes(int64_t len);
fq_status fq_filter_project(const fq_col *col, const fq_pred *pred, const fq_expr *values, int32_t n_out,
                            void *const *d_out, int64_t *out_len, void *d_ws, size_t ws_bytes, void *stream);
/* ---- FilterTransform -> ProjectionTransform over a stream of DataBlocks ----
 * The reference runs both transforms block by block: ExpressionStream applies
 * FilterTransform::expression_executor (transform_filter.rs:38-55) to every
 * block the numbers stream yields (numbers_stream.rs:29-48, 10,000 rows), then
 * ProjectionTransform (transform_projection.rs:45-56) to each filtered block.
 * This is that loop over a batch of blocks in one call: `col` holds
 * ceil(len / block_rows) blocks of block_rows consecutive rows (the last may
 * be short); block b's kept rows are written in order to
 * d_out[j][b * block_rows + r] for r < d_counts[b] (device int64, one per
 * block): each output block starts where its input block does, so no block
 * waits on another's count.  d_out[j] must hold len rows; rows of a block past
 * its count are left as they were.  block_rows >= FQ_PROJECT_MIN_BLOCK_ROWS
 * (the kernel's tile); blocks are independent, so a call runs on up to
 * ceil(len / block_rows) workgroups.  *out_len = rows kept over all blocks.
 * Predicate kinds, expressions and the error order are fq_filter_project's.
 * Synchronises `stream`.                                                    */
#define FQ_PROJECT_MIN_BLOCK_ROWS 8192
size_t fq_filter_project_blocks_workspace_bytes(void);
fq_status fq_filter_project_blocks(const fq_col *col, int64_t block_rows, const fq_pred *pred,
                                   const fq_expr *values, int32_t n_out, void *const *d_out, int64_t *d_counts,
                                   int64_t *out_len, void *d_ws, size_t ws_bytes, void *stream);
/* A block stream's valid rows as one array: for each of n_cols 64-bit columns
 * of the geometry above (len rows, ceil(len / block_rows) blocks, block b's
 * valid rows the first d_counts[b] of its range), d_out[j] receives block 0's
 * rows, then block 1's, ... (what arrow's concat of the reference's filtered
 * blocks would hold).  *out_len (optional: the call then synchronises
 * `stream`) = the rows written.  Workspace: fq_blocks_compact_workspace_bytes.
 */
size_t fq_blocks_compact_workspace_bytes(int64_t n_blocks);
fq_status fq_blocks_compact(int32_t n_cols, const void *const *d_in, int64_t len, int64_t block_rows,
                            const int64_t *d_counts, void *const *d_out, int64_t *out_len, void *d_ws, size_t ws_bytes,
                            void *stream);
/* FilterTransform's predicate alone as a Boolean column: LSB-first bitmap of
 * ceil(len/64) words, bits past len cleared (one kernel instead of one
 * fq_arith per expression node plus fq_compare).  d_flag: 4 bytes of device
 * scratch; the call synchronises `stream` and reports predicate errors.    */
fq_status fq_predicate_bitmap(const fq_col *col, const fq_pred *pred, uint64_t *d_bitmap, uint32_t *d_flag,
                              void *stream);

/* ---- Filter -> Projection over up to FQ_MAX_SCAN_COLS 64-bit columns of one block ----
 * (`SELECT a * b, a + c WHERE c < k`: FilterTransform's and
 * ProjectionTransform's expression_executor range over every field of a
 * DataBlock, function_field.rs:33-40, transform_filter.rs:38-55,
 * transform_projection.rs:45-56).  The columns and every column reference
 * follow fq_aggregate_columns (the encoding documented there): equal len,
 * UINT64 / INT64 / FLOAT64 each (FQ_E_UNSUPPORTED for a narrow one,
 * FQ_E_INVALID for unequal lengths or n_cols outside 1..FQ_MAX_SCAN_COLS); the
 * predicate and each values[j] may start from, and read, different columns
 * (values[j].n_steps == 0: column 0 itself).  Outputs, predicate kinds, the
 * error order, statuses and texts are the single-column entry points'; with
 * n_cols == 1 each call IS its single-column entry point.  More than one
 * column runs on hipRTC-specialised kernels only (FQ_E_UNSUPPORTED with
 * FQ_JIT_OFF or without hipRTC).
 *
 * fq_filter_project_columns: the contiguous (look-back) kernel; its tile, and
 * so the workspace's status words, depend on n_cols.
 * fq_filter_project_blocks_columns: the block-stream kernel, with
 * fq_filter_project_blocks' geometry, block_rows >= FQ_PROJECT_MIN_BLOCK_ROWS
 * rule and workspace (fq_filter_project_blocks_workspace_bytes).
 * fq_predicate_bitmap_columns: the predicate alone as a Boolean column.      */
size_t fq_filter_project_columns_workspace_bytes(int64_t len, int32_t n_cols);
fq_status fq_filter_project_columns(const fq_col *cols, int32_t n_cols, const fq_pred *pred, const fq_expr *values,
                                    int32_t n_out, void *const *d_out, int64_t *out_len, void *d_ws, size_t ws_bytes,
                                    void *stream);
fq_status fq_filter_project_blocks_columns(const fq_col *cols, int32_t n_cols, int64_t block_rows, const fq_pred *pred,
                                           const fq_expr *values, int32_t n_out, void *const *d_out,
                                           int64_t *d_counts, int64_t *out_len, void *d_ws, size_t ws_bytes,
                                           void *stream);
fq_status fq_predicate_bitmap_columns(const fq_col *cols, int32_t n_cols, const fq_pred *pred, uint64_t *d_bitmap,
                                      uint32_t *d_flag, void *stream);
/* Compiles (and caches) the module those three calls use for this shape (one
 * module holds all their kernels; block_rows is 0 or a block-stream block size,
 * checked only).  The columns' data may be NULL.  *specialised = 1 when the
 * shape has a module (0 with FQ_JIT_OFF or without hipRTC: the caller's unfused
 * path answers).  Without a GPU the generated source is compiled for gfx950
 * only to validate it.                                                        */
fq_status fq_jit_prepare_project_columns(const fq_col *cols, int32_t n_cols, int64_t block_rows, const fq_pred *pred,
                                         const fq_expr *values, int32_t n_out, int32_t *specialised);

/* ---- Filter -> Projection block stream over a frame-of-reference copy ----
 * fq_filter_project_blocks over rows [first, first + len) of the UInt64 column
 * that fq_for32_encode stored as d_base / d_delta (both the encoded column's
 * own starts; the window may begin and end anywhere in a frame, and must lie
 * inside the encoded column): row r of the window is
 * d_base[(first + r) / FQ_FOR32_FRAME_ROWS] + d_delta[first + r], read as 4
 * bytes.  Geometry (blocks count from the window's first row), workspace
 * (fq_filter_project_blocks_workspace_bytes), outputs, d_counts, *out_len,
 * synchronisation, the error order and the error texts are
 * fq_filter_project_blocks' over the decoded window, byte for byte; the rows of
 * a FQ_PRED_BITMAP predicate are relative to the window.  Runs on a
 * hipRTC-specialised kernel of its own (fq_jit_pblocks_for32): FQ_E_UNSUPPORTED
 * with FQ_JIT_OFF or without hipRTC, and for FQ_PRED_NONE / a NULL predicate
 * (no row dropped: nothing for this kernel to do).  FQ_E_INVALID, before any
 * device call, for a NULL d_delta / d_base / d_out[j] / d_counts with len > 0,
 * first < 0, len < 0, first + len past INT64_MAX, block_rows <
 * FQ_PROJECT_MIN_BLOCK_ROWS, or a d_delta / d_base not aligned to its element
 * (4 / 8 bytes; the plain call checks d_counts only after compiling the shape).
 * fq_jit_prepare_project_for32 compiles that kernel ahead of the first call
 * (*specialised = 0 with FQ_JIT_OFF or without hipRTC); without a GPU the
 * source is compiled for gfx950 only to validate it.                         */
fq_status fq_filter_project_blocks_for32(const uint32_t *d_delta, const uint64_t *d_base, int64_t first, int64_t len,
                                         int64_t block_rows, const fq_pred *pred, const fq_expr *values, int32_t n_out,
                                         void *const *d_out, int64_t *d_counts, int64_t *out_len, void *d_ws,
                                         size_t ws_bytes, void *stream);
fq_status fq_jit_prepare_project_for32(int64_t block_rows, const fq_pred *pred, const fq_expr *values, int32_t n_out,
                                       int32_t *specialised);

/* ---- Filter -> Projection over columns, steps, comparisons and outputs of any numeric type ----
 * (`SELECT price * discount, quantity WHERE shipdate < k and quantity < q` over
 * price Float64, discount Float32, shipdate Int32, quantity UInt8).  The twins
 * of the four *_columns entry points above: cols[0..n_cols) have equal len and
 * any numeric dtype each, 1..FQ_MAX_SCAN_COLS of them, with the column
 * references of fq_aggregate_columns.  Every fq_step.dtype, cmp_dtype and
 * out_dtype may be any numeric type and is checked against numerical_coercion
 * / equal_coercion of its operands exactly as fq_aggregate_typed checks them
 * (FQ_E_INVALID; "expression too long" when the inserted casts exceed the
 * program); casts, wrapping + - *, truncating / %, Float32 steps and zero
 * divisors follow the rules documented at fq_aggregate_typed.
 *
 * d_out[j] holds elements of values[j].out_dtype at that type's own width (1,
 * 2, 4 or 8 bytes) and is aligned to it; values[j].n_steps == 0 writes column
 * 0 as it is (a lone FQ_OP_LOAD step: that column).  The block-stream form
 * keeps fq_filter_project_blocks' geometry in rows: block b's kept rows at rows
 * [b * block_rows, b * block_rows + d_counts[b]) of each output, rows past the
 * count untouched, block_rows >= FQ_PROJECT_MIN_BLOCK_ROWS.  The error order,
 * predicate kinds, *out_len and the synchronisation are the *_columns entry
 * points'; a cast that arrow turns into null on a row that reaches it (any row
 * for the predicate, a kept row for a value) is FQ_E_UNSUPPORTED "cast produced
 * nulls".
 *
 * When every column, step, comparison and output type is 64-bit each call IS
 * its *_columns twin (same source, same shape key).  Any other shape runs on
 * hipRTC-specialised kernels only (FQ_E_UNSUPPORTED with FQ_JIT_OFF or without
 * hipRTC); fq_jit_prepare_project_typed compiles the shape's one module (all
 * its kernels) ahead of time and, without a GPU, validates the generated
 * source by compiling it for gfx950.  The workspace of fq_filter_project_typed
 * holds one look-back status word per tile of the typed kernel, whose rows
 * depend on the columns' widths: fq_filter_project_typed_workspace_bytes.    */
size_t fq_filter_project_typed_workspace_bytes(int64_t len, const fq_col *cols, int32_t n_cols);
fq_status fq_filter_project_typed(const fq_col *cols, int32_t n_cols, const fq_pred *pred, const fq_expr *values,
                                  int32_t n_out, void *const *d_out, int64_t *out_len, void *d_ws, size_t ws_bytes,
                                  void *stream);
fq_status fq_filter_project_blocks_typed(const fq_col *cols, int32_t n_cols, int64_t block_rows, const fq_pred *pred,
                                         const fq_expr *values, int32_t n_out, void *const *d_out, int64_t *d_counts,
                                         int64_t *out_len, void *d_ws, size_t ws_bytes, void *stream);
fq_status fq_predicate_bitmap_typed(const fq_col *cols, int32_t n_cols, const fq_pred *pred, uint64_t *d_bitmap,
                                    uint32_t *d_flag, void *stream);
fq_status fq_jit_prepare_project_typed(const fq_col *cols, int32_t n_cols, int64_t block_rows, const fq_pred *pred,
                                       const fq_expr *values, int32_t n_out, int32_t *specialised);

/* ---- The Filter -> Projection block stream over nullable columns (Arrow validity bitmaps) ----
 * fq_filter_project_blocks_typed over columns that carry validity bitmaps, the
 * form ProjectionTransform takes over an Arrow host's blocks.  `validity` is
 * fq_aggregate_nullable's argument: the array itself non-NULL, validity[j] NULL
 * (every row of cols[j] valid) or a device pointer, 8-byte aligned, to
 * ceil(len / 64) u64 words whose bit i (LSB first) is 1 when row i of
 * cols[j].data is valid (FQ_E_INVALID otherwise).  Bit 0 is row 0 of
 * cols[j].data; bits at and past len are ignored and no word at or past
 * ceil(len / 64) is read.  A value under a 0 bit never influences a result, a
 * flag or an error.  The rules are arrow 2.0's, the ones fq_aggregate_nullable
 * documents:
 *   - a constant is valid; a step is valid iff both operands are; a cast is
 *     valid iff its input is and the value is in range -- an out-of-range cast
 *     is a null here, never an error: FQ_STATE_CAST_NULL is never set and
 *     "cast produced nulls" is never returned;
 *   - "Divide by zero": a zero divisor on a live row whose operands are both
 *     valid, cast validity included (predicate: any row; value: a kept row);
 *   - a comparison is null if either side is; an and / or node is null if
 *     either side is (`true or null` is null: not Kleene logic); a row is kept
 *     iff the predicate is valid and true.  An FQ_PRED_BITMAP predicate has no
 *     validity of its own; FQ_PRED_NONE / a NULL predicate keeps every row.
 * Columns, coercion checks, d_out, d_counts, block_rows >=
 * FQ_PROJECT_MIN_BLOCK_ROWS, the workspace
 * (fq_filter_project_blocks_workspace_bytes), *out_len and the synchronisation
 * are fq_filter_project_blocks_typed's: block b's kept rows go, in order, to
 * rows [b * block_rows, b * block_rows + d_counts[b]) of every output, rows past
 * the count are untouched.
 *
 * d_out_validity[j] is output j's bitmap: ceil(len / 64) words, 8-byte aligned,
 * bit p describing row p of d_out[j] -- Arrow's one offset for values and
 * validity, so a host slices block b at b * block_rows in both.  The call
 * zeroes these words itself, on `stream`.  Afterwards bit b * block_rows + r,
 * r < d_counts[b], is the validity of that kept row; every other bit of the
 * ceil(len / 64) words is 0 and no word past them is written.  The value stored
 * under a 0 output bit is unspecified.  An entry may be NULL only when the
 * lowering proves the output always valid -- no column with a bitmap and no
 * integer cast reaches it (FQ_E_INVALID otherwise).  Block starts are in
 * general no multiples of 64, so neighbouring blocks, and consecutive tiles of
 * one block, share bitmap words: the kernel combines them with device-scope
 * atomic ORs.
 *
 * Errors: a predicate "Divide by zero" on any row first, then a value's on a
 * kept row.  FQ_E_INVALID, before any device call: a NULL `validity` or
 * d_out_validity array, a bitmap that is not 8-byte aligned, a NULL bitmap of an
 * output that can hold nulls, block_rows below the minimum.  These entry points
 * always run hipRTC-specialised typed kernels, 64-bit shapes included, one
 * module per shape and set of columns that carry a bitmap (a column without one
 * costs no load): FQ_E_UNSUPPORTED with FQ_JIT_OFF or without hipRTC -- there
 * is no unfused path over nulls.
 *
 * fq_predicate_bitmap_nullable: the predicate alone, bit i = valid and true,
 * bits past len cleared; otherwise fq_predicate_bitmap_typed.
 * fq_jit_prepare_project_nullable compiles the shape's module (both kernels)
 * ahead of the first call: has_validity[j] != 0 where the call will pass a
 * bitmap (NULL: none); without a GPU the source is compiled for gfx950 only to
 * validate it.
 *
 * Not built over nulls: the contiguous form (fq_filter_project), the
 * unfiltered map kernel (FQ_PRED_NONE runs through the block kernel), the
 * frame-of-reference window (fq_filter_project_blocks_for32), GROUP BY, and SQL
 * (the planner has no nullable table to query).                              */
fq_status fq_filter_project_blocks_nullable(const fq_col *cols, const uint64_t *const *validity, int32_t n_cols,
                                            int64_t block_rows, const fq_pred *pred, const fq_expr *values,
                                            int32_t n_out, void *const *d_out, uint64_t *const *d_out_validity,
                                            int64_t *d_counts, int64_t *out_len, void *d_ws, size_t ws_bytes,
                                            void *stream);
fq_status fq_predicate_bitmap_nullable(const fq_col *cols, const uint64_t *const *validity, int32_t n_cols,
                                       const fq_pred *pred, uint64_t *d_bitmap, uint32_t *d_flag, void *stream);
fq_status fq_jit_prepare_project_nullable(const fq_col *cols, const uint8_t *has_validity, int32_t n_cols,
                                          int64_t block_rows, const fq_pred *pred, const fq_expr *values, int32_t n_out,
                                          int32_t *specialised);

/* ---- AggregateFinal state merge (host, function_aggregator.rs:106-139) ----
 * Merges `n` partial states in the given order into *out (wrapping sum,
 * summed counts/blocks, max, min, OR-ed flags).  All dtypes must match.      */
fq_status fq_state_merge(const fq_agg_state *states, int32_t n, fq_agg_state *out);

/* ---- Expression specialisation for fq_aggregate (no reference counterpart:
 * the reference evaluates each Function node per block, function.rs:17-132).
 * A fused predicate/argument expression is compiled once per expression
 * SHAPE (ops, operand kinds, dtypes; constants stay kernel arguments) with
 * hipRTC into a straight-line gfx950 scan kernel and cached for the process.
 * Shapes below `min_rows` rows, or with the JIT off, run the precompiled
 * program-interpreting kernel (same results, bit for bit).
 *   mode FQ_JIT_OFF    always interpret
 *   mode FQ_JIT_AUTO   specialise when col->len >= min_rows (default 2^22;
 *                      silently interprets if hipRTC cannot be loaded)
 *   mode FQ_JIT_ALWAYS specialise every fused expression; fails with
 *                      FQ_E_UNSUPPORTED if hipRTC cannot be loaded
 * Initial values come from $FQ_JIT (0/1/2) and $FQ_JIT_MIN_ROWS.           */
#define FQ_JIT_OFF 0
#define FQ_JIT_AUTO 1
#define FQ_JIT_ALWAYS 2
typedef struct fq_jit_stats {
    int64_t kernels_compiled; /* distinct shapes compiled in this process        */
    int64_t jit_launches;     /* fq_aggregate scans run by a specialised kernel  */
    int64_t interp_launches;  /* fused scans run by the interpreting kernel      */
    double compile_ms;        /* total hipRTC compile + module load time         */
    int32_t available;        /* 1 if hipRTC loaded, 0 if not, -1 not tried yet  */
    int32_t mode;
    int64_t min_rows;
} fq_jit_stats;
fq_status fq_jit_config(int32_t mode, int64_t min_rows);
fq_status fq_jit_get_stats(fq_jit_stats *out);
/* Compiles (and caches) the specialised kernel fq_aggregate would use for
 * this call shape, so the first scan does not pay the compile; col->data may
 * be NULL.  *specialised = 1 if the shape has a specialised kernel (mode not
 * OFF, a fused 64-bit expression).  Without a GPU the generated source is
 * compiled for gfx950 only to validate it.                                  */
fq_status fq_jit_prepare(const fq_col *col, int64_t block_rows, const fq_pred *pred,
                         const fq_expr *value, uint32_t agg_mask, int32_t *specialised);
/* The same for fq_aggregate_columns (the columns' data may be NULL: they then
 * count as 16-byte aligned). */
fq_status fq_jit_prepare_columns(const fq_col *cols, int32_t n_cols, int64_t block_rows,
                                 const fq_pred *pred, const fq_expr *value, uint32_t agg_mask,
                                 int32_t *specialised);

/* ---- Launch-shape knobs (tuning tools only; no reference counterpart) ----
 * Every knob has a compiled-in default, the measured best on MI355X
 * (DESIGN.md "Launch-shape knobs" names the sweep each came from).  The
 * library reads no environment variable for them and never prints: the sweep
 * tools (bench.py --tune, tools/) set them here.  Knobs read by a hipRTC
 * kernel are part of its shape key, so a change applies from the next launch. */
#define FQ_TUNE_SCAN_WG_PER_CU 0      /* fused aggregate scan: workgroups per CU, 2 (1..16)           */
#define FQ_TUNE_EW_WG_PER_CU 1        /* arith/compare kernels: 0 = per-op defaults (8/2), 1..16      */
#define FQ_TUNE_BLOCK_U 2             /* block-mode scan: 16-B vectors per lane in flight, 8 (4/8/16) */
#define FQ_TUNE_SELECT_WG_PER_CU 3    /* filter+projection (look-back kernel): workgroups per CU, 8 (1..16) */
#define FQ_TUNE_SELECT_BLOCKS_WG_PER_CU 4 /* block-stream filter+projection: workgroups per CU, 8 (1..16) */
#define FQ_TUNE_SELECT_BLOCKS_ROWS 5  /* block-stream filter+projection: rows per thread per tile, 32 (8/16/32) */
#define FQ_TUNE_SELECT_BLOCKS_STAGE 6 /* block-stream filter+projection: kept rows staged in LDS and written by
                                         consecutive threads, the stage 1/S of a tile: S = 2 (0 = off, 1/2/4) */
#define FQ_TUNE_BLOCK_CACHE 7         /* engine's stream-ordered device block cache, 1 (0/1)          */
#define FQ_TUNE_POOL_SPIN_US 8        /* engine pipe threads poll for the next task before sleeping, 0 us (0..100000) */
#define FQ_TUNE_GROUP_THREADS 9       /* GROUP BY kernels: threads per workgroup, 1024 (256..1024 step 256) */
#define FQ_TUNE_GROUP_LDS_KB 10       /* GROUP BY LDS table budget, 128 (8..160)                      */
#define FQ_TUNE_GROUP_WG_PER_CU 11    /* GROUP BY LDS kernel workgroups per CU: 1 (1..8)              */
#define FQ_TUNE_GROUP_CLUSTER 12      /* clustered row layout threshold (key changes/wave): 160 (0..512) */
#define FQ_TUNE_GROUP_CHUNKED 13      /* contiguous tile runs per workgroup: 1 (0/1)                  */
#define FQ_TUNE_GROUP_RANGE_BINS 14   /* partitioned GROUP BY: range bins for `% d` keys, 1 (0/1)     */
#define FQ_TUNE_GROUP_NARROW 15       /* partitioned GROUP BY: honour FQ_GROUP_NARROW_ROWS, 1 (0/1)   */
#define FQ_TUNE_GPART_WG_PER_CU 16    /* GROUP BY partition kernel: workgroups per CU, 2 (1..4)       */
#define FQ_TUNE_GBINS_WG_PER_CU 17    /* GROUP BY bins pass, fitted table: workgroups per CU, 2 (1..4) */
#define FQ_TUNE_COUNT 18
/* FQ_E_INVALID for an unknown knob or a value outside the knob's set */
fq_status fq_tune_set(int32_t knob, int64_t value);
/* the knob's current value; -1 for an unknown knob */
int64_t fq_tune_get(int32_t knob);
/* every knob back to its default */
fq_status fq_tune_reset(void);
/* dir != NULL: every hipRTC source compiled from now on is written to dir
 * (with its code object) for ISA inspection; NULL turns it off.            */
fq_status fq_tune_jit_dump_dir(const char *dir);

/* ---- GROUP BY hash aggregation (NO reference counterpart:
 * plan_parser.rs:284-308 plans group_expr but pipeline_builder.rs:50-66 builds
 * AggregatePartial/Final from aggr_expr only, so the reference has no grouped
 * semantics to match.  Here a group is a distinct value of an integer key
 * expression over the column; each aggregate is count/sum/min/max of an
 * argument expression over the rows of the group that pass the predicate,
 * with the same value semantics as fq_aggregate (wrapping integer sums, f64
 * IEEE sums in unspecified order).
 *
 * The table is caller-owned device memory of fq_group_table_bytes(capacity,
 * n_aggs) bytes described by an fq_group_table; capacity is a power of two.
 * One extra slot holds the key 0xFFFFFFFFFFFFFFFF (the empty marker).
 * fq_group_aggregate streams a column once: every workgroup pre-aggregates
 * in an LDS hash table and flushes its groups into the HBM table with
 * atomics; keys that do not fit in LDS go to HBM directly.  The kernel is
 * specialised per expression shape with hipRTC (see fq_jit_config); there is
 * no interpreting fallback, so it fails with FQ_E_UNSUPPORTED if hipRTC
 * cannot be loaded.  A table that runs out of slots is reported by
 * fq_group_table_count (FQ_E_TABLE_FULL): re-run into a larger table.       */
#define FQ_MAX_GROUP_AGGS 8
#define FQ_E_TABLE_FULL 8
typedef struct fq_group_table {
    void *d_mem;       /* fq_group_table_bytes(capacity, n_aggs) bytes, device */
    int64_t capacity;  /* slots, a power of two >= 64                          */
    int32_t key_dtype; /* FQ_DT_UINT64 or FQ_DT_INT64                          */
    int32_t n_aggs;    /* 1..FQ_MAX_GROUP_AGGS                                 */
    int32_t kinds[FQ_MAX_GROUP_AGGS];  /* FQ_AGG_COUNT / SUM / MIN / MAX        */
    int32_t dtypes[FQ_MAX_GROUP_AGGS]; /* state dtype: COUNT UInt64, else the
                                          argument's dtype (64-bit types)      */
} fq_group_table;
size_t fq_group_table_bytes(int64_t capacity, int32_t n_aggs);
/* Empties the table (async on stream). */
fq_status fq_group_table_init(const fq_group_table *t, void *stream);
/* Accumulates one device block: key = key_expr(x) (fq_expr over col, integer
 * result of dtype t->key_dtype), aggregate i over values[i](x), rows kept by
 * pred (may be NULL).  Asynchronous. */
fq_status fq_group_aggregate(const fq_group_table *t, const fq_col *col, const fq_pred *pred,
                             const fq_expr *key_expr, const fq_expr *values, void *stream);
/* High-cardinality variant: the rows kept by pred are radix-partitioned by
 * key (range for a `% d` key, else hash) into 2^log2_parts bins (1..8) -- one
 * read + write pass over col into 2 KB block chains in d_ws, the blocks then
 * grouped by bin -- and then aggregated bin by bin, so each workgroup's LDS
 * table only meets the groups of one bin (about groups / 2^log2_parts of
 * them).  Same table, results and errors as fq_group_aggregate; 24 B of HBM
 * traffic per kept row instead of 8 B plus random HBM atomics once the groups
 * outgrow LDS.  d_ws: 256-B aligned, at least
 * fq_group_partition_workspace_bytes(col->len, log2_parts) bytes (about 8 B
 * per row plus ~2 KB per (workgroup, bin) chain).  Asynchronous. */
/* FQ_GROUP_NARROW_ROWS or-ed into log2_parts: the caller guarantees that every
 * value v of the (8-byte integer) column satisfies col[0] - 2^31 <= v <=
 * col[0] + 2^31 - 1, modulo 2^64 (e.g. a numbers_mt block: consecutive
 * integers; col[0] + 2^31 itself is outside).  The partition pass then writes
 * each kept row as a 4-byte offset from col[0] - 2^31 instead of the 8-byte
 * value: 16 B of HBM traffic per kept row instead of 24.  A value outside
 * the range is reported at count/extract (FQ_E_INVALID); Float64 columns
 * ignore the flag.                                                          */
#define FQ_GROUP_NARROW_ROWS 0x10000
size_t fq_group_partition_workspace_bytes(int64_t len, int32_t log2_parts);
fq_status fq_group_aggregate_partitioned(const fq_group_table *t, const fq_col *col, const fq_pred *pred,
                                         const fq_expr *key_expr, const fq_expr *values, int32_t log2_parts,
                                         void *d_ws, size_t ws_bytes, void *stream);
/* Dense keys: when key_expr over a column of col_dtype is a UInt64 key
 * ending in `% d` by a constant and d fits the kernel's LDS table for n_aggs
 * states, the kernel indexes that table by the key itself (no hashing, never
 * saturated) and the query has at most d groups: returns d, else 0. */
int64_t fq_group_dense_keys(int32_t col_dtype, const fq_expr *key_expr, int32_t n_aggs);
/* fq_group_aggregate over the same rows of 1..FQ_MAX_SCAN_COLS columns of one
 * block (`sum(b) ... GROUP BY a`): cols[j] are UInt64 / Int64 / Float64 columns
 * of equal len, 8-byte aligned; they need share no 16-byte phase.  The key,
 * the predicate and every argument name the columns as fq_aggregate_columns
 * documents: a step's `bits` with FQ_OPERAND_COLUMN, FQ_OP_LOAD as the first
 * step, FQ_OP_PUSH with a column number, `rhs_bits` of a comparison against a
 * column.  key_expr NULL or without steps is column 0, and so is an argument
 * without steps; any other column is a one-step FQ_OP_LOAD.  The key's result
 * type must be t->key_dtype (so a Float64 column 0 needs a key expression over
 * an integer column) and argument a's type t->dtypes[a].  FQ_PRED_BITMAP is
 * indexed by row.  The table, its results and its errors (at count / extract,
 * for kept rows only) are fq_group_aggregate's, and launches of either call,
 * of the partitioned variant and fq_group_table_merge may fill one table in
 * any order.  There is no partitioned variant over several columns: keys that
 * outgrow the LDS table go to the HBM table.  n_cols == 1 is
 * fq_group_aggregate itself (same kernels).  Asynchronous. */
fq_status fq_group_aggregate_columns(const fq_group_table *t, const fq_col *cols, int32_t n_cols,
                                     const fq_pred *pred, const fq_expr *key_expr, const fq_expr *values,
                                     void *stream);
/* fq_group_dense_keys for a key expression over n_cols columns of col_dtypes
 * (one dtype: fq_group_dense_keys of it). */
int64_t fq_group_dense_keys_columns(const int32_t *col_dtypes, int32_t n_cols, const fq_expr *key_expr,
                                    int32_t n_aggs);
/* Number of groups (synchronises stream); FQ_E_TABLE_FULL if any insert
 * found no free slot, FQ_E_DIVIDE_BY_ZERO / FQ_E_UNSUPPORTED for the flags
 * fq_aggregate reports. */
fq_status fq_group_table_count(const fq_group_table *t, int64_t *groups, void *stream);
/* Compacts the occupied slots into d_keys[0..groups) and, per aggregate i,
 * d_states[i][0..groups) (64-bit state bits; slot order, unsorted);
 * *groups = the number written (synchronises stream).  cap = room in the
 * output arrays. */
fq_status fq_group_table_extract(const fq_group_table *t, uint64_t *d_keys, uint64_t *const *d_states,
                                 int64_t cap, int64_t *groups, void *stream);
/* Merge n (key, state) rows -- d_keys[n] and d_states[a][n] as the table's
 * state bits, e.g. other GPUs' extracted tables -- into t: a new key claims a
 * slot, an existing one folds with the table's kinds (Count / Sum add, Max /
 * Min keep the extreme), atomically.  The cross-GPU AggregateFinal of a GROUP
 * BY (no reference counterpart: the reference has no GROUP BY execution).
 * A table too small for the keys reports FQ_E_TABLE_FULL on count/extract.  */
fq_status fq_group_table_merge(const fq_group_table *t, const uint64_t *d_keys, const uint64_t *const *d_states,
                               int64_t n, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FQ_GPU_H */
