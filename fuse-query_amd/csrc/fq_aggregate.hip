// Fused AggregatePartial scan for gfx950.
//
// Replaces, per device block (one numbers_mt partition or one DataBlock):
//   FilterTransform::expression_executor  (transform_filter.rs:38-55)   -> predicate
//   AggregatorFunction::accumulate        (function_aggregator.rs:57-100)
//     arg.eval  -> ArithmeticFunction chain (function_arithmetic.rs:64-72)
//     data_array_aggregate_op sum/min/max (data_array_aggregate.rs:14-163)
// with ONE read of the column from HBM: coalesced 16-byte loads (4 in flight
// per lane), per-lane accumulators in registers, a wave64 butterfly reduce,
// an LDS combine across the 4 waves of a workgroup, one Partial per
// workgroup, and a single-workgroup finalize in a fixed order (so float sums
// are reproducible run to run).  No MFMA: nothing here is a contraction.
//
// Block mode: when a predicate is fused with sum(), the reference's per-block
// state machine errors if ANY 10,000-row block is empty after filtering
// (arrow sum -> None, data_value_arithmetic.rs:10-27).  Block mode assigns
// whole reference blocks to waves and reduces "any row passed" with one
// ballot per block, so that flag is exact.
#include <hip/hip_runtime.h>

#include <string>

#include "fq_common.h"
#include "fq_device.h"
#include "fq_scan.h"

namespace fqk {

template <typename V>
struct Acc {
    V sum, mx, mn;
    uint64_t cnt;
    uint32_t flags;
    __device__ void init() {
        sum = V(0);
        mx = MinMaxId<V>::max_id();
        mn = MinMaxId<V>::min_id();
        cnt = 0;
        flags = 0;
    }
};

// Evaluate predicate and value expression for M elements, accumulate.
// Returns the pass mask (bit j = element j passed and is live).
template <typename TIn, typename V, int PRED, bool CHAIN, int M>
__device__ __forceinline__ uint32_t process(const TIn (&x)[M], const int64_t (&idx)[M],
                                            uint32_t live, const KPred &pred, const KProg &val,
                                            uint32_t mask, Acc<V> &acc) {
    uint32_t pass = live;
    if constexpr (PRED == FQ_PRED_EXPR) {
        uint64_t l[M], r[M];
#pragma unroll
        for (int j = 0; j < M; ++j) l[j] = to_bits<TIn>(x[j]);
        run_prog<M, TIn>(pred.lhs, x, l, live, acc.flags);
        if (pred.rhs_operand == FQ_OPERAND_COLUMN) {
#pragma unroll
            for (int j = 0; j < M; ++j)
                r[j] = col_as<TIn>(pred.cmp_dtype, x[j], (live >> j) & 1u, acc.flags);
        } else {
#pragma unroll
            for (int j = 0; j < M; ++j) r[j] = pred.rhs;
        }
        pass &= cmp_mask<M>(pred.cmp, pred.cmp_dtype, l, r);
    } else if constexpr (PRED == FQ_PRED_BITMAP) {
#pragma unroll
        for (int j = 0; j < M; ++j) {
            if ((live >> j) & 1u) {
                const uint64_t w = pred.bitmap[idx[j] >> 6];
                if (!((w >> (idx[j] & 63)) & 1ull)) pass &= ~(1u << j);
            }
        }
    } else if constexpr (PRED == FQ_PRED_TREE) {
        // every leaf over every live row (arrow and/or evaluate both sides),
        // then the tree through its truth table
        uint32_t m[FQ_MAX_PRED_LEAVES] = {};
#pragma unroll
        for (int li = 0; li < FQ_MAX_PRED_LEAVES; ++li) {
            if (li >= pred.n_leaves) break;
            const KLeaf &lf = pred.leaves[li];
            uint64_t l[M], r[M];
#pragma unroll
            for (int j = 0; j < M; ++j) l[j] = to_bits<TIn>(x[j]);
            run_prog<M, TIn>(lf.lhs, x, l, live, acc.flags);
            if (lf.rhs_operand == FQ_OPERAND_COLUMN) {
#pragma unroll
                for (int j = 0; j < M; ++j) r[j] = col_as<TIn>(lf.cmp_dtype, x[j], (live >> j) & 1u, acc.flags);
            } else {
#pragma unroll
                for (int j = 0; j < M; ++j) r[j] = lf.rhs;
            }
            m[li] = cmp_mask<M>(lf.cmp, lf.cmp_dtype, l, r);
        }
        uint32_t t = 0;
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const uint32_t idxbits = ((m[0] >> j) & 1u) | (((m[1] >> j) & 1u) << 1) | (((m[2] >> j) & 1u) << 2) |
                                     (((m[3] >> j) & 1u) << 3);
            t |= ((pred.truth >> idxbits) & 1u) << j;
        }
        pass &= t;
    }
    V v[M];
    if constexpr (CHAIN) {
        uint64_t a[M];
#pragma unroll
        for (int j = 0; j < M; ++j) a[j] = to_bits<TIn>(x[j]);
        run_prog<M, TIn>(val, x, a, pass, acc.flags);
#pragma unroll
        for (int j = 0; j < M; ++j) v[j] = from_bits<V>(a[j]);
    } else {
#pragma unroll
        for (int j = 0; j < M; ++j) v[j] = (V)x[j];
    }
    if (mask & FQ_AGG_SUM) {
#pragma unroll
        for (int j = 0; j < M; ++j) acc.sum = acc.sum + (((pass >> j) & 1u) ? v[j] : V(0));
    }
    if (mask & FQ_AGG_MAX) {
#pragma unroll
        for (int j = 0; j < M; ++j) acc.mx = ((pass >> j) & 1u) ? vmax(acc.mx, v[j]) : acc.mx;
    }
    if (mask & FQ_AGG_MIN) {
#pragma unroll
        for (int j = 0; j < M; ++j) acc.mn = ((pass >> j) & 1u) ? vmin(acc.mn, v[j]) : acc.mn;
    }
    acc.cnt += __builtin_popcount(pass);
    return pass;
}

// wave butterfly + LDS combine; thread 0 of the workgroup stores the result
template <typename V>
__device__ __forceinline__ void reduce_and_store(Acc<V> &acc, Partial *out, int32_t dtype) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        acc.sum = acc.sum + shfl_xor64(acc.sum, off);
        acc.mx = vmax(acc.mx, shfl_xor64(acc.mx, off));
        acc.mn = vmin(acc.mn, shfl_xor64(acc.mn, off));
        acc.cnt += shfl_xor64(acc.cnt, off);
        acc.flags |= (uint32_t)__shfl_xor((int)acc.flags, off, kWave);
    }
    __shared__ V s_sum[kThreads / kWave], s_mx[kThreads / kWave], s_mn[kThreads / kWave];
    __shared__ uint64_t s_cnt[kThreads / kWave];
    __shared__ uint32_t s_flags[kThreads / kWave];
    const int wave = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) {
        s_sum[wave] = acc.sum;
        s_mx[wave] = acc.mx;
        s_mn[wave] = acc.mn;
        s_cnt[wave] = acc.cnt;
        s_flags[wave] = acc.flags;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        V sum = s_sum[0], mx = s_mx[0], mn = s_mn[0];
        uint64_t cnt = s_cnt[0];
        uint32_t flags = s_flags[0];
#pragma unroll
        for (int w = 1; w < kThreads / kWave; ++w) {
            sum = sum + s_sum[w];
            mx = vmax(mx, s_mx[w]);
            mn = vmin(mn, s_mn[w]);
            cnt += s_cnt[w];
            flags |= s_flags[w];
        }
        Partial p;
        p.sum = to_bits<V>(sum);
        p.max = to_bits<V>(mx);
        p.min = to_bits<V>(mn);
        p.count = cnt;
        p.blocks = 0;
        p.flags = flags;
        p.dtype = dtype;
        *out = p;
    }
}

// The launch's partials folded in a fixed order by ONE workgroup: thread t
// folds partials t, t+256, ... then the wave butterfly and the LDS combine,
// so a grid gives the same bytes run to run (float sums too).  An in-launch
// fold by the scan's last workgroup (agent-scope release / ticket / acquire)
// measured slower than this separate 4.4 us launch: 8 scans 11.07 against
// 11.02 ms (profiles/r05_b_scan_fin_ab.json), and was removed in round 6.
template <typename V>
__device__ __forceinline__ void fold_partials(Partial *parts, int nparts, uint64_t blocks, uint64_t rows,
                                              int32_t vdtype, int empty_if_zero, fq_agg_state *out) {
    Acc<V> acc;
    acc.init();
    if (threadIdx.x == 0) acc.cnt = rows;  // count-only scans: no column read (nparts == 0)
    for (int i = threadIdx.x; i < nparts; i += kThreads) {
        const Partial p = parts[i];
        acc.sum = acc.sum + from_bits<V>(p.sum);
        acc.mx = vmax(acc.mx, from_bits<V>(p.max));
        acc.mn = vmin(acc.mn, from_bits<V>(p.min));
        acc.cnt += p.count;
        acc.flags |= p.flags;
    }
    __shared__ Partial s_out;
    reduce_and_store<V>(acc, &s_out, vdtype);
    __syncthreads();
    if (threadIdx.x == 0) {
        fq_agg_state r;
        r.sum = s_out.sum;
        r.max = s_out.max;
        r.min = s_out.min;
        r.count = s_out.count;
        r.blocks = blocks;
        r.flags = s_out.flags;
        if (empty_if_zero && r.count == 0) r.flags |= FQ_STATE_ANY_EMPTY;
        r.dtype = vdtype;
        *out = r;
    }
}

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// Flat streaming mode: grid-stride over 16-byte vectors, U vectors in flight
// per lane.  `head` scalar elements precede the first 16-byte boundary.
template <typename TIn, typename V, int PRED, bool CHAIN, int U, bool PF = false>
__global__ void __launch_bounds__(kThreads)
    agg_flat_kernel(const TIn *__restrict__ col, int64_t n, int64_t head, KPred pred, KProg val,
                    uint32_t mask, int32_t vdtype, Partial *parts) {
    constexpr int VE = 16 / sizeof(TIn);
    constexpr int E = VE * U;
    static_assert(E <= 32, "pass mask is 32 bits");
    Acc<V> acc;
    acc.init();
    const int64_t T = (int64_t)gridDim.x * kThreads;
    const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t nvec = (n - head) / VE;
    const u32x4 *__restrict__ vp = reinterpret_cast<const u32x4 *>(col + head);
    constexpr uint32_t kFull = (E == 32) ? 0xffffffffu : ((1u << E) - 1u);

    // Tile-contiguous streaming: a workgroup reads one contiguous tile of
    // U * 256 vectors (16 KB for u64 at U=4) per iteration, non-temporal,
    // and strides over tiles by the grid.  Measured on MI355X against the
    // vector-granular grid stride: 7.2 vs 6.2 TB/s (tools/tune_scan.py,
    // profiles/r01_tune_*.json); few workgroups per CU (see launch) helps too.
    constexpr int64_t TV = (int64_t)U * kThreads;
    const int64_t ntiles = nvec / TV;
    u32x4 nxt[U];  // PF: the next tile's vectors in flight while this tile is reduced (launch_scan)
    if constexpr (PF) {
        if ((int64_t)blockIdx.x < ntiles) {
#pragma unroll
            for (int k = 0; k < U; ++k)
                nxt[k] = __builtin_nontemporal_load(vp + (int64_t)blockIdx.x * TV + threadIdx.x + (int64_t)k * kThreads);
        }
    }
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t base = t * TV + threadIdx.x;
        u32x4 raw[U];
        if constexpr (PF) {
#pragma unroll
            for (int k = 0; k < U; ++k) raw[k] = nxt[k];
            const int64_t tn = t + gridDim.x;
            if (tn < ntiles) {
#pragma unroll
                for (int k = 0; k < U; ++k)
                    nxt[k] = __builtin_nontemporal_load(vp + tn * TV + threadIdx.x + (int64_t)k * kThreads);
            }
        } else {
#pragma unroll
            for (int k = 0; k < U; ++k) raw[k] = __builtin_nontemporal_load(vp + base + (int64_t)k * kThreads);
        }
        TIn x[E];
        int64_t idx[E];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            __builtin_memcpy(&x[k * VE], &raw[k], 16);
#pragma unroll
            for (int e = 0; e < VE; ++e) idx[k * VE + e] = head + (base + (int64_t)k * kThreads) * VE + e;
        }
        process<TIn, V, PRED, CHAIN, E>(x, idx, kFull, pred, val, mask, acc);
    }
    for (int64_t v = ntiles * TV + g; v < nvec; v += T) {
        const u32x4 raw = __builtin_nontemporal_load(vp + v);
        TIn x[VE];
        int64_t idx[VE];
        __builtin_memcpy(&x[0], &raw, 16);
#pragma unroll
        for (int e = 0; e < VE; ++e) idx[e] = head + v * VE + e;
        process<TIn, V, PRED, CHAIN, VE>(x, idx, (1u << VE) - 1u, pred, val, mask, acc);
    }
    // scalar edges: [0, head) and [head + nvec*VE, n)
    const int64_t tail0 = head + nvec * VE;
    const int64_t nedge = head + (n - tail0);
    for (int64_t t = g; t < nedge; t += T) {
        const int64_t i = t < head ? t : tail0 + (t - head);
        TIn x[1] = {col[i]};
        int64_t idx[1] = {i};
        process<TIn, V, PRED, CHAIN, 1>(x, idx, 1u, pred, val, mask, acc);
    }
    reduce_and_store<V>(acc, parts + blockIdx.x, vdtype);
}

// ---------------------------------------------------------------------------
// Frame-of-reference storage of a resident UInt64 column (fq_for32_encode /
// fq_aggregate_for32): frame f = rows [f F, (f + 1) F), F = FQ_FOR32_FRAME_ROWS,
// is base[f] = its minimum and delta[i] = value[i] - base[i / F] in 32 bits.
// The scan reads 4 bytes per row instead of 8; sum (wrapping), max, min and
// count over base + delta are the plain column's, bit for bit.
// ---------------------------------------------------------------------------
constexpr int64_t kFrame = FQ_FOR32_FRAME_ROWS;
constexpr int64_t kFor32Tile = 4 * kThreads * 4;  // rows of a tile: 4 vectors x 256 lanes x 4 u32 (16 KB)
static_assert(kFrame % kFor32Tile == 0, "a tile never straddles a frame");

// One workgroup per frame (a grid stride over frames): the frame's minimum and
// maximum from the data, then its deltas (the second read of the 512 KB frame
// comes from L2).  *flag = 1 when a frame spans more than 32 bits.
__global__ void __launch_bounds__(kThreads)
    for32_encode_kernel(const uint64_t *__restrict__ col, int64_t n, uint64_t *__restrict__ base,
                        uint32_t *__restrict__ delta, uint32_t *flag) {
    __shared__ uint64_t s_mn[kThreads / kWave], s_mx[kThreads / kWave];
    const int64_t frames = (n + kFrame - 1) / kFrame;
    for (int64_t f = blockIdx.x; f < frames; f += gridDim.x) {
        const int64_t s = f * kFrame;
        const int64_t e = s + kFrame < n ? s + kFrame : n;
        uint64_t mn = ~0ull, mx = 0;
        for (int64_t i = s + threadIdx.x; i < e; i += kThreads) {
            const uint64_t v = col[i];
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
        }
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) {
            mn = vmin(mn, shfl_xor64(mn, off));
            mx = vmax(mx, shfl_xor64(mx, off));
        }
        __syncthreads();  // the previous frame's s_mn / s_mx have been read
        if ((threadIdx.x & (kWave - 1)) == 0) {
            s_mn[threadIdx.x / kWave] = mn;
            s_mx[threadIdx.x / kWave] = mx;
        }
        __syncthreads();
        mn = s_mn[0];
        mx = s_mx[0];
#pragma unroll
        for (int w = 1; w < kThreads / kWave; ++w) {
            mn = vmin(mn, s_mn[w]);
            mx = vmax(mx, s_mx[w]);
        }
        if (threadIdx.x == 0) {
            base[f] = mn;
            if (mx - mn > 0xFFFFFFFFull) *flag = 1u;
        }
        for (int64_t i = s + threadIdx.x; i < e; i += kThreads) delta[i] = (uint32_t)(col[i] - mn);
    }
}

// agg_flat_kernel's streaming loop over the 32-bit deltas: a workgroup reads
// one contiguous 16 KB tile (4 non-temporal 16-byte loads per lane) per
// iteration and strides over tiles by the grid.  Per row the work is 32-bit; a
// lane folds its 16 deltas of a tile into its 64-bit accumulators once, with
// the tile's frame base (workgroup-uniform).  Vectors past the last whole tile
// and the up to 3 rows after them look their base up from the row index.
__global__ void __launch_bounds__(kThreads)
    agg_flat_kernel_for32(const uint32_t *__restrict__ delta, const uint64_t *__restrict__ base, int64_t n,
                          uint32_t mask, Partial *parts) {
    constexpr int U = 4, VE = 4, E = U * VE;
    constexpr int64_t TV = (int64_t)U * kThreads;   // vectors per tile
    constexpr int64_t kTilesPerFrame = kFrame / kFor32Tile;
    Acc<uint64_t> acc;
    acc.init();
    const int64_t T = (int64_t)gridDim.x * kThreads;
    const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t nvec = n / VE;
    const int64_t ntiles = nvec / TV;
    const u32x4 *__restrict__ vp = reinterpret_cast<const u32x4 *>(delta);
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t v0 = t * TV + threadIdx.x;
        u32x4 raw[U];
#pragma unroll
        for (int k = 0; k < U; ++k) raw[k] = __builtin_nontemporal_load(vp + v0 + (int64_t)k * kThreads);
        const uint64_t b = base[t / kTilesPerFrame];
        uint32_t x[E];
#pragma unroll
        for (int k = 0; k < U; ++k) __builtin_memcpy(&x[k * VE], &raw[k], 16);
        if (mask & FQ_AGG_SUM) {
            uint64_t dsum = 0;
#pragma unroll
            for (int j = 0; j < E; ++j) dsum += x[j];
            acc.sum += dsum + (uint64_t)E * b;
        }
        if (mask & FQ_AGG_MAX) {
            uint32_t dmax = 0;
#pragma unroll
            for (int j = 0; j < E; ++j) dmax = x[j] > dmax ? x[j] : dmax;
            acc.mx = vmax(acc.mx, b + dmax);
        }
        if (mask & FQ_AGG_MIN) {
            uint32_t dmin = 0xFFFFFFFFu;
#pragma unroll
            for (int j = 0; j < E; ++j) dmin = x[j] < dmin ? x[j] : dmin;
            acc.mn = vmin(acc.mn, b + dmin);
        }
        acc.cnt += E;
    }
    for (int64_t v = ntiles * TV + g; v < nvec; v += T) {
        const u32x4 raw = __builtin_nontemporal_load(vp + v);
        const uint64_t b = base[(v * VE) / kFrame];  // a 4-row vector never straddles a frame
        uint32_t x[VE];
        __builtin_memcpy(&x[0], &raw, 16);
#pragma unroll
        for (int j = 0; j < VE; ++j) {
            const uint64_t val = b + x[j];
            if (mask & FQ_AGG_SUM) acc.sum += val;
            if (mask & FQ_AGG_MAX) acc.mx = vmax(acc.mx, val);
            if (mask & FQ_AGG_MIN) acc.mn = vmin(acc.mn, val);
        }
        acc.cnt += VE;
    }
    for (int64_t i = nvec * VE + g; i < n; i += T) {
        const uint64_t val = base[i / kFrame] + delta[i];
        if (mask & FQ_AGG_SUM) acc.sum += val;
        if (mask & FQ_AGG_MAX) acc.mx = vmax(acc.mx, val);
        if (mask & FQ_AGG_MIN) acc.mn = vmin(acc.mn, val);
        acc.cnt += 1;
    }
    reduce_and_store<uint64_t>(acc, parts + blockIdx.x, FQ_DT_UINT64);
}

// Block mode: one wave owns whole reference blocks of R rows; one ballot per
// block tells whether any of its rows survived the predicate.
template <typename TIn, typename V, int PRED, bool CHAIN, int U>
__global__ void __launch_bounds__(kThreads)
    agg_block_kernel(const TIn *__restrict__ col, int64_t n, int64_t R, KPred pred, KProg val,
                     uint32_t mask, int32_t vdtype, Partial *parts) {
    Acc<V> acc;
    acc.init();
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t w = ((int64_t)blockIdx.x * kThreads + threadIdx.x) / kWave;
    const int64_t W = ((int64_t)gridDim.x * kThreads) / kWave;
    const int64_t nb = (n + R - 1) / R;
    for (int64_t b = w; b < nb; b += W) {
        const int64_t s = b * R;
        const int64_t e = (s + R < n) ? s + R : n;
        uint32_t any = 0;
        for (int64_t i = s + lane; i < e; i += (int64_t)kWave * U) {
            TIn x[U];
            int64_t idx[U];
            uint32_t live = 0;
#pragma unroll
            for (int k = 0; k < U; ++k) {
                idx[k] = i + (int64_t)k * kWave;
                if (idx[k] < e) {
                    x[k] = __builtin_nontemporal_load(col + idx[k]);
                    live |= 1u << k;
                } else {
                    x[k] = TIn(0);
                }
            }
            any |= process<TIn, V, PRED, CHAIN, U>(x, idx, live, pred, val, mask, acc);
        }
        if (__ballot(any != 0) == 0ull) acc.flags |= FQ_STATE_ANY_EMPTY;
    }
    reduce_and_store<V>(acc, parts + blockIdx.x, vdtype);
}

// Single workgroup, fixed order (fold_partials): the result is deterministic
// for a given grid.
template <typename V>
__global__ void __launch_bounds__(kThreads)
    agg_finalize_kernel(Partial *parts, int nparts, uint64_t blocks, uint64_t rows, int32_t vdtype,
                        int empty_if_zero, fq_agg_state *out) {
    fold_partials<V>(parts, nparts, blocks, rows, vdtype, empty_if_zero, out);
}

// fq_aggregate_nullable: the same fold over the scan's PartialN, and their
// valid counts (integers: any order).  A single reference block is empty when
// it has no valid kept value; nparts == 0 is the count-only call, which reads
// no value.
template <typename V>
__global__ void __launch_bounds__(kThreads)
    agg_finalize_nullable_kernel(const PartialN *parts, int nparts, uint64_t blocks, uint64_t rows, int32_t vdtype,
                                 int empty_if_zero, fq_agg_state_n *out) {
    Acc<V> acc;
    acc.init();
    if (threadIdx.x == 0) acc.cnt = rows;
    unsigned long long valid = 0;
    for (int i = threadIdx.x; i < nparts; i += kThreads) {
        const PartialN q = parts[i];
        acc.sum = acc.sum + from_bits<V>(q.p.sum);
        acc.mx = vmax(acc.mx, from_bits<V>(q.p.max));
        acc.mn = vmin(acc.mn, from_bits<V>(q.p.min));
        acc.cnt += q.p.count;
        acc.flags |= q.p.flags;
        valid += q.valid;
    }
    __shared__ Partial s_out;
    __shared__ unsigned long long s_valid;
    if (threadIdx.x == 0) s_valid = 0;
    __syncthreads();
    atomicAdd(&s_valid, valid);
    reduce_and_store<V>(acc, &s_out, vdtype);
    __syncthreads();
    if (threadIdx.x == 0) {
        fq_agg_state_n r;
        r.s.sum = s_out.sum;
        r.s.max = s_out.max;
        r.s.min = s_out.min;
        r.s.count = s_out.count;
        r.s.blocks = blocks;
        r.s.flags = s_out.flags;
        if (empty_if_zero && nparts > 0 && s_valid == 0) r.s.flags |= FQ_STATE_ANY_EMPTY;
        r.s.dtype = vdtype;
        r.valid = s_valid;
        r.reserved = 0;
        *out = r;
    }
}

// ---------------------------------------------------------------------------
// host-side lowering and dispatch
// ---------------------------------------------------------------------------

static bool is_pow2(uint64_t v) { return v && !(v & (v - 1)); }

// Workgroups per CU for the flat scan (FQ_TUNE_SCAN_WG_PER_CU, default 2).
static int scan_wg_per_cu() { return (int)fqc::knob(FQ_TUNE_SCAN_WG_PER_CU); }

// libdivide's u64 round-up magic (branchful form)
static void u64_magic(uint64_t d, uint64_t &magic, uint32_t &shift, uint32_t &add) {
    const uint32_t l = 63 - __builtin_clzll(d);
    const unsigned __int128 num = (unsigned __int128)1 << (64 + l);
    uint64_t proposed = (uint64_t)(num / d);
    const uint64_t rem = (uint64_t)(num % d);
    const uint64_t e = d - rem;
    if (e < (1ull << l)) {
        add = 0;
    } else {
        proposed += proposed;
        const uint64_t twice_rem = rem + rem;
        if (twice_rem >= d || twice_rem < rem) proposed += 1;
        add = 1;
    }
    shift = l;
    magic = proposed + 1;
}

// libdivide's u32 round-up magic (branchful form), for K_MODM32_U
static void u32_magic(uint32_t d, uint32_t &magic, uint32_t &shift, uint32_t &add) {
    const uint32_t l = 31 - __builtin_clz(d);
    const uint64_t num = (uint64_t)1 << (32 + l);
    uint32_t proposed = (uint32_t)(num / d);
    const uint32_t rem = (uint32_t)(num % d);
    const uint32_t e = d - rem;
    if (e < (1u << l)) {
        add = 0;
    } else {
        proposed += proposed;
        const uint32_t twice_rem = rem + rem;
        if (twice_rem >= d || twice_rem < rem) proposed += 1;
        add = 1;
    }
    shift = l;
    magic = proposed + 1;
}

static bool is_chain_dtype(int32_t dt) {
    return dt == FQ_DT_UINT64 || dt == FQ_DT_INT64 || dt == FQ_DT_FLOAT64;
}

// position in numerical_coercion's order (fq_common.cpp order[]): the coerced
// type of two is the one that comes first; -1 for a non-numeric type
static int coercion_rank(int32_t dt) {
    static const int32_t order[] = {FQ_DT_FLOAT64, FQ_DT_FLOAT32, FQ_DT_INT64,  FQ_DT_INT32, FQ_DT_INT16,
                                    FQ_DT_INT8,    FQ_DT_UINT64,  FQ_DT_UINT32, FQ_DT_UINT16, FQ_DT_UINT8};
    for (int i = 0; i < 10; ++i)
        if (order[i] == dt) return i;
    return -1;
}
static int32_t coerced(int32_t l, int32_t r) { return coercion_rank(l) <= coercion_rank(r) ? l : r; }

static fq_status push_cast(int32_t from, int32_t to, KProg &out, bool typed = false) {
    if (from == to) return FQ_OK;
    if (out.n >= (int)(sizeof(out.s) / sizeof(out.s[0])))
        return fqc::fail(FQ_E_UNSUPPORTED, "expression too long for the fused device path");
    if (typed) {  // one of the 45 casts towards an earlier type of the order
        if (coercion_rank(to) < 0 || coercion_rank(from) < coercion_rank(to))
            return fqc::fail(FQ_E_INVALID, std::string("fq_step: numerical_coercion never casts ") +
                                               fqc::dtype_name(from) + " to " + fqc::dtype_name(to));
        KStep &s = out.s[out.n++];
        s = KStep{};
        s.code = K_CAST;
        s.sdtype = from;
        s.dtype = to;
        return FQ_OK;
    }
    KStep &s = out.s[out.n++];
    s = KStep{};
    s.dtype = to;
    if (from == FQ_DT_UINT64 && to == FQ_DT_INT64) s.code = K_CAST_U2I;
    else if (from == FQ_DT_UINT64 && to == FQ_DT_FLOAT64) s.code = K_CAST_U2F;
    else if (from == FQ_DT_INT64 && to == FQ_DT_FLOAT64) s.code = K_CAST_I2F;
    else
        return fqc::fail(FQ_E_UNSUPPORTED, std::string("fused cast ") + fqc::dtype_name(from) + " -> " +
                                               fqc::dtype_name(to) + " is not supported on the device path");
    return FQ_OK;
}

// fq_expr (semantic) -> KProg (lowered).  Returns the resulting dtype.
// n_cols == 0: the single-column entry points, which ignore the column indices
// (every reference is the one column, of dtype cdt[0]).
// typed: fq_aggregate_typed -- any numeric column and step type; every step's
// type must be what numerical_coercion yields for acc and the operand.
static fq_status lower_expr_impl(const fq_expr &e, const int32_t *cdt, int n_cols, KProg &out, int32_t &res_dtype,
                                 bool typed = false) {
    out.n = 0;
    const int32_t col_dtype = cdt[0];
    // the column a step's `bits` names (-1: out of range)
    auto col_of = [n_cols](uint64_t bits) -> int { return n_cols == 0 ? 0 : (bits < (uint64_t)n_cols ? (int)bits : -1); };
    int32_t acc = col_dtype;
    if (e.n_steps < 0 || e.n_steps > FQ_MAX_STEPS)
        return fqc::fail(FQ_E_INVALID, "fq_expr: n_steps out of range");
    if (e.n_steps > 0 && !typed && !is_chain_dtype(col_dtype))
        return fqc::fail(FQ_E_UNSUPPORTED, std::string("fused expressions over ") + fqc::dtype_name(col_dtype) +
                                               " columns are not supported on the device path");
    int32_t stack[FQ_MAX_STACK];
    int depth = 0;
    for (int i = 0; i < e.n_steps; ++i) {
        const fq_step &st = e.steps[i];
        if (st.op == FQ_OP_LOAD && n_cols > 0) {  // the expression starts as another column than 0
            if (i != 0) return fqc::fail(FQ_E_INVALID, "fq_step: FQ_OP_LOAD is the first step only");
            const int c = col_of(st.bits);
            if (c < 0) return fqc::fail(FQ_E_INVALID, "fq_step: column index out of range");
            KStep &k = out.s[out.n++];
            k = KStep{};
            k.code = K_LOAD;
            k.dtype = cdt[c];
            k.col = c;
            acc = cdt[c];
            continue;
        }
        // a one-column *_columns / *_typed call is the single-column entry point: its FQ_OP_LOAD names the
        // one column (the caller checked the index), which acc already is
        if (st.op == FQ_OP_LOAD && i == 0) continue;
        if (st.op == FQ_OP_PUSH) {  // expression tree: acc onto the stack, restart from the column
            if (depth >= FQ_MAX_STACK) return fqc::fail(FQ_E_UNSUPPORTED, "expression tree too deep for the fused device path");
            if (!typed && !is_chain_dtype(col_dtype))
                return fqc::fail(FQ_E_UNSUPPORTED, "fused expression trees need a 64-bit column");
            if (out.n >= (int)(sizeof(out.s) / sizeof(out.s[0])))
                return fqc::fail(FQ_E_UNSUPPORTED, "expression too long for the fused device path");
            const int c = col_of(st.bits);
            if (c < 0) return fqc::fail(FQ_E_INVALID, "fq_step: column index out of range");
            KStep &k = out.s[out.n++];
            k = KStep{};
            k.code = K_PUSH;
            k.dtype = cdt[c];
            k.col = c;
            stack[depth++] = acc;
            acc = cdt[c];
            continue;
        }
        if (typed ? !fqc::dtype_is_numeric(st.dtype) : !is_chain_dtype(st.dtype))
            return fqc::fail(FQ_E_UNSUPPORTED, typed ? "fused step dtype must be numeric"
                                                     : "fused step dtype must be UInt64, Int64 or Float64");
        // typed: the step's type against numerical_coercion(acc, operand)
        auto coercion_ok = [&](int32_t odt, const char *what) -> fq_status {
            if (coerced(acc, odt) == st.dtype) return FQ_OK;
            return fqc::fail(FQ_E_INVALID, std::string("fq_step: ") + fqc::dtype_name(odt) + " " + what + " in a " +
                                               fqc::dtype_name(st.dtype) + " step over " + fqc::dtype_name(acc) +
                                               " (numerical_coercion gives " + fqc::dtype_name(coerced(acc, odt)) + ")");
        };
        int32_t sdt = 0;
        if (st.operand == FQ_OPERAND_STACK) {
            if (depth == 0) return fqc::fail(FQ_E_INVALID, "fq_step: stack operand without a pushed value");
            sdt = stack[--depth];
            if (typed) {
                fq_status cs = coercion_ok(sdt, "stack operand");
                if (cs != FQ_OK) return cs;
            } else if (sdt != st.dtype && !(sdt == FQ_DT_UINT64 && st.dtype != FQ_DT_UINT64) &&
                !(sdt == FQ_DT_INT64 && st.dtype == FQ_DT_FLOAT64))
                return fqc::fail(FQ_E_UNSUPPORTED, std::string("fused cast ") + fqc::dtype_name(sdt) + " -> " +
                                                       fqc::dtype_name(st.dtype) + " is not supported on the device path");
        } else if (st.operand != FQ_OPERAND_CONST && st.operand != FQ_OPERAND_COLUMN) {
            return fqc::fail(FQ_E_INVALID, "fq_step: bad operand kind");
        }
        int ocol = 0;
        if (typed) {
            if (st.operand == FQ_OPERAND_COLUMN) {
                ocol = col_of(st.bits);
                if (ocol < 0) return fqc::fail(FQ_E_INVALID, "fq_step: column index out of range");
                fq_status cs = coercion_ok(cdt[ocol], "column operand");
                if (cs != FQ_OK) return cs;
            } else if (st.operand == FQ_OPERAND_CONST && coercion_rank(st.dtype) > coercion_rank(acc)) {
                return fqc::fail(FQ_E_INVALID, std::string("fq_step: a ") + fqc::dtype_name(st.dtype) +
                                                   " step over " + fqc::dtype_name(acc) +
                                                   " (numerical_coercion never yields it)");
            }
        }
        fq_status s = push_cast(acc, st.dtype, out, typed);
        if (s != FQ_OK) return s;
        if (!typed && st.operand == FQ_OPERAND_COLUMN) {
            ocol = col_of(st.bits);
            if (ocol < 0) return fqc::fail(FQ_E_INVALID, "fq_step: column index out of range");
            if (cdt[ocol] == FQ_DT_FLOAT64 && st.dtype != FQ_DT_FLOAT64)
                return fqc::fail(FQ_E_INVALID, "fq_step: Float64 column operand in an integer step");
            if (n_cols > 0 && cdt[ocol] == FQ_DT_INT64 && st.dtype == FQ_DT_UINT64)
                return fqc::fail(FQ_E_INVALID, "fq_step: Int64 column operand in a UInt64 step");
        }
        if (out.n >= (int)(sizeof(out.s) / sizeof(out.s[0])))
            return fqc::fail(FQ_E_UNSUPPORTED, "expression too long for the fused device path");
        KStep &k = out.s[out.n++];
        k = KStep{};
        k.operand = st.operand;
        k.reversed = st.reversed;
        k.dtype = st.dtype;
        k.sdtype = sdt;
        k.col = ocol;
        k.c = st.bits;
        // typed scans keep the constant a kernel argument of a plain '/' or '%'
        const bool konst = st.operand == FQ_OPERAND_CONST && !st.reversed && !typed;
        if (fqc::dtype_is_float(st.dtype)) {
            switch (st.op) {
                case FQ_OP_ADD: k.code = K_ADD_F; break;
                case FQ_OP_SUB: k.code = K_SUB_F; break;
                case FQ_OP_MUL: k.code = K_MUL_F; break;
                case FQ_OP_DIV: k.code = K_DIV_F; break;
                case FQ_OP_MOD: k.code = K_MOD_F; break;
                default: return fqc::fail(FQ_E_INVALID, "fq_step: bad op");
            }
        } else {
            const bool u = fqc::dtype_is_unsigned_int(st.dtype);
            switch (st.op) {
                case FQ_OP_ADD: k.code = K_ADD_I; break;
                case FQ_OP_SUB: k.code = K_SUB_I; break;
                case FQ_OP_MUL: k.code = K_MUL_I; break;
                case FQ_OP_DIV:
                    if (u && konst && st.bits != 0) {
                        if (is_pow2(st.bits)) {
                            k.code = K_SHR_U;
                            k.shift = (uint32_t)__builtin_ctzll(st.bits);
                        } else if (st.bits <= 65535) {
                            k.code = K_DIVM32_U;  // 32/16/16-bit long division
                            uint32_t m32 = 0;
                            u32_magic((uint32_t)st.bits, m32, k.shift, k.add);
                            k.magic = m32;
                        } else {
                            k.code = K_DIVM_U;
                            u64_magic(st.bits, k.magic, k.shift, k.add);
                        }
                    } else {
                        k.code = u ? K_DIV_U : K_DIV_S;
                    }
                    break;
                case FQ_OP_MOD:
                    if (u && konst && st.bits != 0) {
                        if (is_pow2(st.bits)) {
                            k.code = K_AND_U;
                            k.magic = st.bits - 1;
                        } else if (st.bits <= 65535) {
                            // 32-bit halves: (x>>32)%d * (2^32 % d) + (u32)x % d < 2^32
                            k.code = K_MODM32_U;
                            uint32_t m32 = 0;
                            u32_magic((uint32_t)st.bits, m32, k.shift, k.add);
                            k.magic = (uint64_t)m32 | ((((uint64_t)1 << 32) % st.bits) << 32);
                        } else {
                            k.code = K_MODM_U;
                            u64_magic(st.bits, k.magic, k.shift, k.add);
                        }
                    } else {
                        k.code = u ? K_MOD_U : K_MOD_S;
                    }
                    break;
                default: return fqc::fail(FQ_E_INVALID, "fq_step: bad op");
            }
        }
        acc = st.dtype;
    }
    if (depth != 0) return fqc::fail(FQ_E_INVALID, "fq_expr: pushed values left on the stack");
    if (e.n_steps > 0 && e.out_dtype != acc)
        return fqc::fail(FQ_E_INVALID, "fq_expr: out_dtype does not match the last step");
    res_dtype = acc;
    out.out_dtype = acc;
    return FQ_OK;
}

fq_status lower_expr(const fq_expr &e, int32_t col_dtype, KProg &out, int32_t &res_dtype) {
    return lower_expr_impl(e, &col_dtype, 0, out, res_dtype);
}

fq_status lower_expr_cols(const fq_expr &e, const int32_t *cdt, int n_cols, KProg &out, int32_t &res_dtype) {
    return lower_expr_impl(e, cdt, n_cols, out, res_dtype);
}

fq_status lower_expr_typed(const fq_expr &e, const int32_t *cdt, int n_cols, KProg &out, int32_t &res_dtype) {
    return lower_expr_impl(e, cdt, n_cols, out, res_dtype, true);
}

// fq_pred (semantic) -> KPred (lowered): predicate program cast to the
// comparison type.
static fq_status lower_pred_impl(const fq_pred *pred, const int32_t *cdt, int n_cols, int64_t len, bool need_data,
                                 KPred &out, bool typed = false) {
    out = KPred{};
    out.kind = pred ? pred->kind : FQ_PRED_NONE;
    const int32_t col_dtype = cdt[0];
    // the right-hand column of a comparison in cmp_dtype: its index in *rc
    // (typed: cmp_dtype against equal_coercion of the left side's type ldt and the right side)
    auto rhs_col = [cdt, n_cols, typed](int32_t rhs_operand, uint64_t bits, int32_t cmp_dtype, int32_t *rc,
                                        int32_t ldt) -> fq_status {
        *rc = 0;
        if (typed && rhs_operand != FQ_OPERAND_COLUMN && rhs_operand != FQ_OPERAND_CONST)
            return fqc::fail(FQ_E_INVALID, "fq_pred: bad rhs_operand");
        if (rhs_operand != FQ_OPERAND_COLUMN) return FQ_OK;
        if (n_cols > 0) {
            if (bits >= (uint64_t)n_cols) return fqc::fail(FQ_E_INVALID, "fq_pred: column index out of range");
            *rc = (int32_t)bits;
        }
        if (typed) {
            if (coerced(ldt, cdt[*rc]) == cmp_dtype) return FQ_OK;
            return fqc::fail(FQ_E_INVALID, std::string("fq_pred: ") + fqc::dtype_name(ldt) + " compared with a " +
                                               fqc::dtype_name(cdt[*rc]) + " column as " + fqc::dtype_name(cmp_dtype) +
                                               " (equal_coercion gives " + fqc::dtype_name(coerced(ldt, cdt[*rc])) + ")");
        }
        if (cdt[*rc] == FQ_DT_FLOAT64 && cmp_dtype != FQ_DT_FLOAT64)
            return fqc::fail(FQ_E_INVALID, "fq_pred: Float64 column compared as integer");
        if (n_cols > 0 && cdt[*rc] == FQ_DT_INT64 && cmp_dtype == FQ_DT_UINT64)
            return fqc::fail(FQ_E_INVALID, "fq_pred: Int64 column compared as UInt64");
        return FQ_OK;
    };
    if (out.kind == FQ_PRED_EXPR) {
        int32_t ldt = col_dtype;
        fq_status s = lower_expr_impl(pred->lhs, cdt, n_cols, out.lhs, ldt, typed);
        if (s != FQ_OK) return s;
        if (typed ? !fqc::dtype_is_numeric(pred->cmp_dtype) : !is_chain_dtype(pred->cmp_dtype))
            return fqc::fail(FQ_E_UNSUPPORTED, typed ? "fused comparison type must be numeric"
                                                     : "fused comparison type must be UInt64, Int64 or Float64");
        if (typed && (pred->cmp < FQ_CMP_EQ || pred->cmp > FQ_CMP_GTEQ)) return fqc::fail(FQ_E_INVALID, "fq_pred: bad cmp");
        // (typed: the right side first -- its message names the types that do not coerce)
        if (typed) s = rhs_col(pred->rhs_operand, pred->rhs_bits, pred->cmp_dtype, &out.rhs_col, ldt);
        if (s != FQ_OK) return s;
        s = push_cast(ldt, pred->cmp_dtype, out.lhs, typed);
        if (s != FQ_OK) return s;
        if (!typed) s = rhs_col(pred->rhs_operand, pred->rhs_bits, pred->cmp_dtype, &out.rhs_col, ldt);
        if (s != FQ_OK) return s;
        out.cmp = pred->cmp;
        out.cmp_dtype = pred->cmp_dtype;
        out.rhs_operand = pred->rhs_operand;
        out.rhs = pred->rhs_bits;
    } else if (out.kind == FQ_PRED_BITMAP) {
        if (need_data && !pred->bitmap && len > 0) return fqc::fail(FQ_E_INVALID, "fq_pred: NULL bitmap");
        out.bitmap = pred->bitmap;
    } else if (out.kind == FQ_PRED_TREE) {
        const fq_pred_tree *t = pred->tree;
        if (!t) return fqc::fail(FQ_E_INVALID, "fq_pred: NULL tree");
        if (t->n_leaves < 1 || t->n_leaves > FQ_MAX_PRED_LEAVES || t->n_prog < 1 ||
            t->n_prog > 2 * FQ_MAX_PRED_LEAVES)
            return fqc::fail(FQ_E_INVALID, "fq_pred_tree: leaf / program count out of range");
        if (!typed && fqc::dtype_size(col_dtype) != 8)
            return fqc::fail(FQ_E_UNSUPPORTED, "fused predicates need a 64-bit column");
        out.n_leaves = t->n_leaves;
        out.n_prog = t->n_prog;
        for (int i = 0; i < t->n_leaves; ++i) {
            const fq_pred_leaf &lf = t->leaves[i];
            KLeaf &k = out.leaves[i];
            int32_t ldt = col_dtype;
            fq_status s = lower_expr_impl(lf.lhs, cdt, n_cols, k.lhs, ldt, typed);
            if (s != FQ_OK) return s;
            if (typed ? !fqc::dtype_is_numeric(lf.cmp_dtype) : !is_chain_dtype(lf.cmp_dtype))
                return fqc::fail(FQ_E_UNSUPPORTED, typed ? "fused comparison type must be numeric"
                                                         : "fused comparison type must be UInt64, Int64 or Float64");
            if (typed) s = rhs_col(lf.rhs_operand, lf.rhs_bits, lf.cmp_dtype, &k.rhs_col, ldt);
            if (s != FQ_OK) return s;
            s = push_cast(ldt, lf.cmp_dtype, k.lhs, typed);
            if (s != FQ_OK) return s;
            if (lf.cmp < FQ_CMP_EQ || lf.cmp > FQ_CMP_GTEQ) return fqc::fail(FQ_E_INVALID, "fq_pred_leaf: bad cmp");
            if (!typed) s = rhs_col(lf.rhs_operand, lf.rhs_bits, lf.cmp_dtype, &k.rhs_col, ldt);
            if (s != FQ_OK) return s;
            k.cmp = lf.cmp;
            k.cmp_dtype = lf.cmp_dtype;
            k.rhs_operand = lf.rhs_operand;
            k.rhs = lf.rhs_bits;
        }
        // validate the postfix program and tabulate it over the 2^n leaf outcomes
        uint32_t truth = 0;
        for (uint32_t combo = 0; combo < (1u << FQ_MAX_PRED_LEAVES); ++combo) {
            bool st[2 * FQ_MAX_PRED_LEAVES];
            int sp = 0;
            for (int i = 0; i < t->n_prog; ++i) {
                const int32_t tok = t->prog[i];
                out.prog[i] = tok;
                if (tok >= 0 && tok < t->n_leaves) {
                    st[sp++] = (combo >> tok) & 1u;
                } else if (tok == FQ_PRED_AND || tok == FQ_PRED_OR) {
                    if (sp < 2) return fqc::fail(FQ_E_INVALID, "fq_pred_tree: malformed program");
                    const bool b = st[--sp], a = st[--sp];
                    st[sp++] = tok == FQ_PRED_AND ? (a && b) : (a || b);
                } else {
                    return fqc::fail(FQ_E_INVALID, "fq_pred_tree: bad program token");
                }
            }
            if (sp != 1) return fqc::fail(FQ_E_INVALID, "fq_pred_tree: malformed program");
            if (st[0]) truth |= 1u << combo;
        }
        out.truth = truth;
    } else if (out.kind != FQ_PRED_NONE) {
        return fqc::fail(FQ_E_INVALID, "fq_pred: bad kind");
    }
    return FQ_OK;
}

fq_status lower_pred(const fq_pred *pred, int32_t col_dtype, int64_t len, bool need_data, KPred &out) {
    return lower_pred_impl(pred, &col_dtype, 0, len, need_data, out);
}

fq_status lower_pred_cols(const fq_pred *pred, const int32_t *cdt, int n_cols, int64_t len, bool need_data,
                          KPred &out) {
    return lower_pred_impl(pred, cdt, n_cols, len, need_data, out);
}

fq_status lower_pred_typed(const fq_pred *pred, const int32_t *cdt, int n_cols, int64_t len, bool need_data,
                           KPred &out) {
    return lower_pred_impl(pred, cdt, n_cols, len, need_data, out, true);
}

template <typename TIn, typename V, int PRED, bool CHAIN>
static fq_status launch_scan(const Launch &L) {
    // vectors in flight per lane: 64 B for 64-bit columns, 16 elements otherwise
    constexpr int U = sizeof(TIn) >= 4 ? 4 : (sizeof(TIn) == 2 ? 2 : 1);
    if (PRED != FQ_PRED_NONE && L.block_mode) {
        hipLaunchKernelGGL((agg_block_kernel<TIn, V, PRED, CHAIN, 8>), dim3(L.grid), dim3(kThreads), 0,
                           L.stream, (const TIn *)L.col, L.n, L.block_rows, L.pred, L.val, L.mask,
                           L.vdtype, L.parts);
    } else {
        // the next tile's loads in flight while this one is reduced, for scans
        // without max/min: sum(number) 1.4132 -> 1.3991 ms per 10 GB, sum+count
        // 1.4094 -> 1.3939; with max or min it costs instead (C3 1.3800 ->
        // 1.3889, max 1.3904 -> 1.3959).  One process each, 6 rounds
        // alternating (profiles/r06_o_*_pf_ab.json); the arithmetic order is
        // the same either way.
        if (PRED == FQ_PRED_NONE && !CHAIN && !(L.mask & (FQ_AGG_MAX | FQ_AGG_MIN)))
            hipLaunchKernelGGL((agg_flat_kernel<TIn, V, PRED, CHAIN, U, true>), dim3(L.grid), dim3(kThreads), 0,
                               L.stream, (const TIn *)L.col, L.n, L.head, L.pred, L.val, L.mask, L.vdtype,
                               L.parts);
        else
            hipLaunchKernelGGL((agg_flat_kernel<TIn, V, PRED, CHAIN, U>), dim3(L.grid), dim3(kThreads), 0,
                               L.stream, (const TIn *)L.col, L.n, L.head, L.pred, L.val, L.mask, L.vdtype,
                               L.parts);
    }
    FQ_HIP_TRY(hipGetLastError());
    return FQ_OK;
}

template <typename TIn, typename V, bool CHAIN>
static fq_status dispatch_pred(const Launch &L) {
    switch (L.pred.kind) {
        case FQ_PRED_NONE: return launch_scan<TIn, V, FQ_PRED_NONE, CHAIN>(L);
        case FQ_PRED_BITMAP: return launch_scan<TIn, V, FQ_PRED_BITMAP, CHAIN>(L);
        case FQ_PRED_EXPR:
            if constexpr (sizeof(TIn) == 8) return launch_scan<TIn, V, FQ_PRED_EXPR, CHAIN>(L);
            return fqc::fail(FQ_E_UNSUPPORTED, "fused predicates need a 64-bit column");
        case FQ_PRED_TREE:
            if constexpr (sizeof(TIn) == 8) return launch_scan<TIn, V, FQ_PRED_TREE, CHAIN>(L);
            return fqc::fail(FQ_E_UNSUPPORTED, "fused predicates need a 64-bit column");
        default: return fqc::fail(FQ_E_INVALID, "fq_pred: bad kind");
    }
}

template <typename V>
static fq_status launch_finalize(const Launch &L, uint64_t blocks, int empty_if_zero, fq_agg_state *d_out) {
    // L.grid == 0: a count-only scan without predicate or expression -- the
    // reference's Count adds block.num_rows() (function_aggregator.rs:60-66),
    // no value is read, so neither is the column
    hipLaunchKernelGGL((agg_finalize_kernel<V>), dim3(1), dim3(kThreads), 0, L.stream, L.parts, L.grid,
                       blocks, L.grid == 0 ? (uint64_t)L.n : 0ull, L.vdtype, empty_if_zero, d_out);
    FQ_HIP_TRY(hipGetLastError());
    return FQ_OK;
}

static fq_status dispatch(int32_t col_dt, const Launch &L, bool chain) {
    const int32_t v = L.vdtype;
    if (!chain) {
        switch (col_dt) {
            case FQ_DT_INT8: return dispatch_pred<int8_t, int8_t, false>(L);
            case FQ_DT_INT16: return dispatch_pred<int16_t, int16_t, false>(L);
            case FQ_DT_INT32: return dispatch_pred<int32_t, int32_t, false>(L);
            case FQ_DT_INT64: return dispatch_pred<int64_t, int64_t, false>(L);
            case FQ_DT_UINT8: return dispatch_pred<uint8_t, uint8_t, false>(L);
            case FQ_DT_UINT16: return dispatch_pred<uint16_t, uint16_t, false>(L);
            case FQ_DT_UINT32: return dispatch_pred<uint32_t, uint32_t, false>(L);
            case FQ_DT_UINT64: return dispatch_pred<uint64_t, uint64_t, false>(L);
            case FQ_DT_FLOAT32: return dispatch_pred<float, float, false>(L);
            case FQ_DT_FLOAT64: return dispatch_pred<double, double, false>(L);
            default: break;
        }
    } else if (col_dt == FQ_DT_UINT64) {
        if (v == FQ_DT_UINT64) return dispatch_pred<uint64_t, uint64_t, true>(L);
        if (v == FQ_DT_INT64) return dispatch_pred<uint64_t, int64_t, true>(L);
        if (v == FQ_DT_FLOAT64) return dispatch_pred<uint64_t, double, true>(L);
    } else if (col_dt == FQ_DT_INT64) {
        if (v == FQ_DT_INT64) return dispatch_pred<int64_t, int64_t, true>(L);
        if (v == FQ_DT_FLOAT64) return dispatch_pred<int64_t, double, true>(L);
    } else if (col_dt == FQ_DT_FLOAT64) {
        if (v == FQ_DT_FLOAT64) return dispatch_pred<double, double, true>(L);
    }
    return fqc::fail(FQ_E_UNSUPPORTED, std::string("aggregate over ") + fqc::dtype_name(col_dt) +
                                           " column with " + fqc::dtype_name(v) +
                                           " value is not supported on the device path");
}

template <typename V>
static fq_status launch_finalize_nullable(const Launch &L, uint64_t blocks, int empty_if_zero, fq_agg_state_n *d_out) {
    hipLaunchKernelGGL((agg_finalize_nullable_kernel<V>), dim3(1), dim3(kThreads), 0, L.stream,
                       (const PartialN *)L.parts, L.grid, blocks, L.grid == 0 ? (uint64_t)L.n : 0ull, L.vdtype,
                       empty_if_zero, d_out);
    FQ_HIP_TRY(hipGetLastError());
    return FQ_OK;
}

static fq_status dispatch_finalize_nullable(const Launch &L, uint64_t blocks, int empty_if_zero, fq_agg_state_n *d_out) {
    switch (L.vdtype) {
        case FQ_DT_INT8: return launch_finalize_nullable<int8_t>(L, blocks, empty_if_zero, d_out);
        case FQ_DT_INT16: return launch_finalize_nullable<int16_t>(L, blocks, empty_if_zero, d_out);
        case FQ_DT_INT32: return launch_finalize_nullable<int32_t>(L, blocks, empty_if_zero, d_out);
        case FQ_DT_INT64: return launch_finalize_nullable<int64_t>(L, blocks, empty_if_zero, d_out);
        case FQ_DT_UINT8: return launch_finalize_nullable<uint8_t>(L, blocks, empty_if_zero, d_out);
        case FQ_DT_UINT16: return launch_finalize_nullable<uint16_t>(L, blocks, empty_if_zero, d_out);
        case FQ_DT_UINT32: return launch_finalize_nullable<uint32_t>(L, blocks, empty_if_zero, d_out);
        case FQ_DT_UINT64: return launch_finalize_nullable<uint64_t>(L, blocks, empty_if_zero, d_out);
        case FQ_DT_FLOAT32: return launch_finalize_nullable<float>(L, blocks, empty_if_zero, d_out);
        case FQ_DT_FLOAT64: return launch_finalize_nullable<double>(L, blocks, empty_if_zero, d_out);
        default: return fqc::fail(FQ_E_INVALID, "finalize: bad dtype");
    }
}

static fq_status dispatch_finalize(const Launch &L, uint64_t blocks, int empty_if_zero, fq_agg_state *d_out) {
    switch (L.vdtype) {
        case FQ_DT_INT8: return launch_finalize<int8_t>(L, blocks, empty_if_zero, d_out);
        case FQ_DT_INT16: return launch_finalize<int16_t>(L, blocks, empty_if_zero, d_out);
        case FQ_DT_INT32: return launch_finalize<int32_t>(L, blocks, empty_if_zero, d_out);
        case FQ_DT_INT64: return launch_finalize<int64_t>(L, blocks, empty_if_zero, d_out);
        case FQ_DT_UINT8: return launch_finalize<uint8_t>(L, blocks, empty_if_zero, d_out);
        case FQ_DT_UINT16: return launch_finalize<uint16_t>(L, blocks, empty_if_zero, d_out);
        case FQ_DT_UINT32: return launch_finalize<uint32_t>(L, blocks, empty_if_zero, d_out);
        case FQ_DT_UINT64: return launch_finalize<uint64_t>(L, blocks, empty_if_zero, d_out);
        case FQ_DT_FLOAT32: return launch_finalize<float>(L, blocks, empty_if_zero, d_out);
        case FQ_DT_FLOAT64: return launch_finalize<double>(L, blocks, empty_if_zero, d_out);
        default: return fqc::fail(FQ_E_INVALID, "finalize: bad dtype");
    }
}

}  // namespace fqk

extern "C" {

size_t fq_aggregate_workspace_bytes(int64_t len) {
    (void)len;
    return fqk::kPartialsBytes;
}

}  // extern "C"

namespace fqk {

// Validates the arguments and prepares the launch shared by fq_aggregate and
// fq_jit_prepare (lowered programs, flat/block mode, grid).
static fq_status plan_scan(const fq_col *col, int64_t block_rows, const fq_pred *pred, const fq_expr *value,
                           uint32_t agg_mask, bool need_data, Launch &L, bool &chain, uint64_t &blocks,
                           int &empty_if_zero) {
    if (!col) return fqc::fail(FQ_E_INVALID, "fq_aggregate: NULL argument");
    if (col->len < 0) return fqc::fail(FQ_E_INVALID, "fq_aggregate: negative length");
    const int esize = fqc::dtype_size(col->dtype);
    if (!fqc::dtype_is_numeric(col->dtype))
        return fqc::internal(std::string("Unsupported data_array_aggregate for data type: ") +
                             fqc::dtype_name(col->dtype));
    if (need_data && col->len > 0 && !col->data) return fqc::fail(FQ_E_INVALID, "fq_aggregate: NULL column data");
    if (((uintptr_t)col->data) % esize)
        return fqc::fail(FQ_E_INVALID, "fq_aggregate: column not aligned to its element size");
    if (block_rows <= 0) block_rows = col->len > 0 ? col->len : 1;

    L = Launch{};
    L.col = col->data;
    L.n = col->len;
    L.block_rows = block_rows;
    L.mask = agg_mask;

    // value expression
    chain = value && value->n_steps > 0;
    int32_t vdt = col->dtype;
    if (chain) {
        fq_status s = lower_expr(*value, col->dtype, L.val, vdt);
        if (s != FQ_OK) return s;
    }
    L.vdtype = vdt;

    // predicate
    fq_status ps = lower_pred(pred, col->dtype, col->len, need_data, L.pred);
    if (ps != FQ_OK) return ps;

    blocks = col->len == 0 ? 0 : (uint64_t)((col->len + block_rows - 1) / block_rows);
    // Block mode only where the per-block emptiness matters (filtered sum over
    // more than one reference block); otherwise stream flat.
    L.block_mode = L.pred.kind != FQ_PRED_NONE && (agg_mask & FQ_AGG_SUM) && blocks > 1;
    empty_if_zero = (L.pred.kind != FQ_PRED_NONE && blocks == 1) ? 1 : 0;

    const int cus = fqc::device_cu_count();
    const int max_grid = cus * 8 < kMaxPartials ? cus * 8 : kMaxPartials;
    if (L.block_mode) {
        const int64_t waves_needed = (int64_t)blocks;
        int64_t grid = (waves_needed + (kThreads / kWave) - 1) / (kThreads / kWave);
        L.grid = (int)(grid < max_grid ? (grid < 1 ? 1 : grid) : max_grid);
        L.head = 0;
    } else {
        const int64_t vec_elems = 16 / esize;
        const uintptr_t mis = ((uintptr_t)col->data) & 15u;
        int64_t head = mis ? (int64_t)((16 - mis) / esize) : 0;
        if (head > col->len) head = col->len;
        L.head = head;
        const int64_t nvec = (col->len - head) / vec_elems;
        const int64_t tile = (int64_t)kThreads * (esize >= 4 ? 4 : (esize == 2 ? 2 : 1));
        int64_t grid = (nvec + tile - 1) / tile;
        if (grid < 1) grid = 1;
        // 2 workgroups (8 waves) per CU streamed fastest (tools/tune_scan.py)
        const int64_t flat_max = (int64_t)cus * scan_wg_per_cu();
        L.grid = (int)(grid < flat_max ? grid : flat_max);
    }
    return FQ_OK;
}

// The same for fq_aggregate_columns / fq_jit_prepare_columns over n_cols >= 2
// checked columns (one column goes through plan_scan).
static fq_status plan_scan_cols(const fq_col *cols, int32_t n_cols, int64_t block_rows, const fq_pred *pred,
                                const fq_expr *value, uint32_t agg_mask, bool need_data, Launch &L, bool &chain,
                                uint64_t &blocks, int &empty_if_zero) {
    const int64_t len = cols[0].len;
    if (block_rows <= 0) block_rows = len > 0 ? len : 1;
    L = Launch{};
    L.col = cols[0].data;
    L.n = len;
    L.block_rows = block_rows;
    L.mask = agg_mask;
    L.n_cols = n_cols;
    for (int j = 0; j < n_cols; ++j) {
        L.cols[j] = cols[j].data;
        L.cdt[j] = cols[j].dtype;
    }
    chain = value && value->n_steps > 0;
    int32_t vdt = L.cdt[0];
    if (chain) {
        fq_status s = lower_expr_cols(*value, L.cdt, n_cols, L.val, vdt);
        if (s != FQ_OK) return s;
    }
    L.vdtype = vdt;
    fq_status ps = lower_pred_cols(pred, L.cdt, n_cols, len, need_data, L.pred);
    if (ps != FQ_OK) return ps;

    blocks = len == 0 ? 0 : (uint64_t)((len + block_rows - 1) / block_rows);
    L.block_mode = L.pred.kind != FQ_PRED_NONE && (agg_mask & FQ_AGG_SUM) && blocks > 1;
    empty_if_zero = (L.pred.kind != FQ_PRED_NONE && blocks == 1) ? 1 : 0;

    // 16-byte loads need the same rows of every column on a 16-byte boundary
    bool same_phase = true, aligned = true;
    for (int j = 0; j < n_cols; ++j) {
        same_phase = same_phase && ((((uintptr_t)cols[j].data) ^ ((uintptr_t)cols[0].data)) & 15u) == 0;
        aligned = aligned && (((uintptr_t)cols[j].data) & 15u) == 0;
    }
    const int cus = fqc::device_cu_count();
    const int max_grid = cus * 8 < kMaxPartials ? cus * 8 : kMaxPartials;
    if (L.block_mode) {
        int64_t grid = ((int64_t)blocks + (kThreads / kWave) - 1) / (kThreads / kWave);
        L.grid = (int)(grid < max_grid ? (grid < 1 ? 1 : grid) : max_grid);
        L.head = 0;
        L.vec = aligned && (block_rows & 1) == 0;
    } else {
        L.vec = same_phase;
        int64_t head = (((uintptr_t)cols[0].data) & 15u) ? 1 : 0;
        if (head > len) head = len;
        L.head = L.vec ? head : 0;
        // a tile: scan_cols_vectors(n_cols) 16-byte vectors of every column per lane
        const int64_t tile_rows = (int64_t)kThreads * scan_cols_vectors(n_cols) * 2;
        int64_t grid = (len + tile_rows - 1) / tile_rows;
        if (grid < 1) grid = 1;
        const int64_t flat_max = (int64_t)cus * scan_wg_per_cu();
        L.grid = (int)(grid < flat_max ? grid : flat_max);
    }
    return FQ_OK;
}

// argument checks of the *_columns entry points (`who` names the caller in the messages)
fq_status check_cols(const fq_col *cols, int32_t n_cols, bool need_data, const char *who) {
    const std::string W = std::string(who) + ": ";
    if (!cols) return fqc::fail(FQ_E_INVALID, W + "NULL argument");
    if (n_cols < 1 || n_cols > FQ_MAX_SCAN_COLS)
        return fqc::fail(FQ_E_INVALID, W + "n_cols must be 1.." + std::to_string(FQ_MAX_SCAN_COLS) +
                                           ", got " + std::to_string(n_cols));
    for (int j = 0; j < n_cols; ++j) {
        if (cols[j].len < 0) return fqc::fail(FQ_E_INVALID, W + "negative length");
        if (cols[j].len != cols[0].len)
            return fqc::fail(FQ_E_INVALID, W + "column " + std::to_string(j) + " has " +
                                               std::to_string(cols[j].len) + " rows, column 0 has " +
                                               std::to_string(cols[0].len));
        if (!is_chain_dtype(cols[j].dtype))
            return fqc::fail(FQ_E_UNSUPPORTED, W + fqc::dtype_name(cols[j].dtype) +
                                                   " column (scans over several columns need UInt64, Int64 or "
                                                   "Float64 columns)");
        if (need_data && cols[j].len > 0 && !cols[j].data)
            return fqc::fail(FQ_E_INVALID, W + "NULL column data");
        if (((uintptr_t)cols[j].data) % 8)
            return fqc::fail(FQ_E_INVALID, W + "column not aligned to its element size");
    }
    return FQ_OK;
}

// the column indices of a one-column program (all must be 0)
static fq_status check_one_col(const fq_col *col, const fq_pred *pred, const fq_expr *value) {
    KProg kp;
    KPred kd;
    int32_t dt = col->dtype;
    if (value && value->n_steps > 0) {
        fq_status s = lower_expr_cols(*value, &col->dtype, 1, kp, dt);
        if (s != FQ_OK) return s;
    }
    return lower_pred_cols(pred, &col->dtype, 1, col->len, false, kd);
}

// fq_aggregate: the scan, then the fold of its partials, both on `stream`
static fq_status aggregate(const fq_col *col, int64_t block_rows, const fq_pred *pred, const fq_expr *value,
                           uint32_t agg_mask, fq_agg_state *d_out, void *d_ws, size_t ws_bytes, hipStream_t stream) {
    if (!col || !d_out || !d_ws) return fqc::fail(FQ_E_INVALID, "fq_aggregate: NULL argument");
    if (ws_bytes < kPartialsBytes) return fqc::fail(FQ_E_INVALID, "fq_aggregate: workspace too small");
    if (agg_mask & ~(uint32_t)(FQ_AGG_MIN | FQ_AGG_MAX | FQ_AGG_SUM | FQ_AGG_COUNT))
        return fqc::fail(FQ_E_INVALID, "fq_aggregate: unknown bits in agg_mask");
    Launch L;
    bool chain = false;
    uint64_t blocks = 0;
    int empty_if_zero = 0;
    fq_status s = plan_scan(col, block_rows, pred, value, agg_mask, true, L, chain, blocks, empty_if_zero);
    if (s != FQ_OK) return s;
    L.stream = (hipStream_t)stream;
    L.parts = (Partial *)d_ws;
    if (agg_mask == FQ_AGG_COUNT && !chain && L.pred.kind == FQ_PRED_NONE) {
        L.grid = 0;  // count(column): rows, not values (see launch_finalize)
        return dispatch_finalize(L, blocks, empty_if_zero, d_out);
    }
    bool jitted = false;
    const bool tree = (chain && prog_has_tree(L.val)) || pred_has_tree(L.pred);
    s = jit_scan(col->dtype, chain, L, &jitted, tree);
    if (s != FQ_OK) return s;
    if (!jitted && tree)
        return fqc::fail(FQ_E_UNSUPPORTED, "fused expression trees run on the hipRTC kernels only (FQ_JIT is off "
                                           "or hipRTC is unavailable)");
    if (!jitted) {
        if (chain || L.pred.kind != FQ_PRED_NONE) jit_count_interp();
        s = dispatch(col->dtype, L, chain);
        if (s != FQ_OK) return s;
    }
    return dispatch_finalize(L, blocks, empty_if_zero, d_out);
}

// fq_aggregate_columns over two or more columns: hipRTC kernels only
static fq_status aggregate_cols(const fq_col *cols, int32_t n_cols, int64_t block_rows, const fq_pred *pred,
                                const fq_expr *value, uint32_t agg_mask, fq_agg_state *d_out, void *d_ws,
                                size_t ws_bytes, hipStream_t stream) {
    if (!d_out || !d_ws) return fqc::fail(FQ_E_INVALID, "fq_aggregate_columns: NULL argument");
    if (ws_bytes < kPartialsBytes) return fqc::fail(FQ_E_INVALID, "fq_aggregate_columns: workspace too small");
    if (agg_mask & ~(uint32_t)(FQ_AGG_MIN | FQ_AGG_MAX | FQ_AGG_SUM | FQ_AGG_COUNT))
        return fqc::fail(FQ_E_INVALID, "fq_aggregate_columns: unknown bits in agg_mask");
    Launch L;
    bool chain = false;
    uint64_t blocks = 0;
    int empty_if_zero = 0;
    fq_status s = plan_scan_cols(cols, n_cols, block_rows, pred, value, agg_mask, true, L, chain, blocks, empty_if_zero);
    if (s != FQ_OK) return s;
    L.stream = stream;
    L.parts = (Partial *)d_ws;
    if (agg_mask == FQ_AGG_COUNT && !chain && L.pred.kind == FQ_PRED_NONE) {
        L.grid = 0;  // count(column): rows, not values (see launch_finalize)
        return dispatch_finalize(L, blocks, empty_if_zero, d_out);
    }
    bool jitted = false;
    s = jit_scan(cols[0].dtype, chain, L, &jitted, true);
    if (s != FQ_OK) return s;
    if (!jitted)
        return fqc::fail(FQ_E_UNSUPPORTED, "scans over several columns run on the hipRTC kernels only (FQ_JIT is off "
                                           "or hipRTC is unavailable)");
    return dispatch_finalize(L, blocks, empty_if_zero, d_out);
}

// ---------------------------------------------------------------------------
// fq_aggregate_typed: columns, steps and comparisons of any numeric type
// ---------------------------------------------------------------------------
static const char *kTypedNeedsJit =
    "scans over narrow or mixed-width columns run on the hipRTC kernels only (FQ_JIT is off or hipRTC is "
    "unavailable)";

fq_status check_cols_typed(const fq_col *cols, int32_t n_cols, bool need_data, const char *who) {
    const std::string W = std::string(who) + ": ";
    if (!cols) return fqc::fail(FQ_E_INVALID, W + "NULL argument");
    if (n_cols < 1 || n_cols > FQ_MAX_SCAN_COLS)
        return fqc::fail(FQ_E_INVALID, W + "n_cols must be 1.." + std::to_string(FQ_MAX_SCAN_COLS) +
                                           ", got " + std::to_string(n_cols));
    for (int j = 0; j < n_cols; ++j) {
        if (cols[j].len < 0) return fqc::fail(FQ_E_INVALID, W + "negative length");
        if (cols[j].len != cols[0].len)
            return fqc::fail(FQ_E_INVALID, W + "column " + std::to_string(j) + " has " +
                                               std::to_string(cols[j].len) + " rows, column 0 has " +
                                               std::to_string(cols[0].len));
        if (!fqc::dtype_is_numeric(cols[j].dtype))
            return fqc::internal(std::string("Unsupported data_array_aggregate for data type: ") +
                                 fqc::dtype_name(cols[j].dtype));
        if (need_data && cols[j].len > 0 && !cols[j].data)
            return fqc::fail(FQ_E_INVALID, W + "NULL column data");
        if (((uintptr_t)cols[j].data) % fqc::dtype_size(cols[j].dtype))
            return fqc::fail(FQ_E_INVALID, W + "column not aligned to its element size");
    }
    return FQ_OK;
}

// every column, step and comparison type 64-bit: the call is fq_aggregate_columns
static bool expr_is_64(const fq_expr *e) {
    if (!e) return true;
    for (int i = 0; i < e->n_steps && i < FQ_MAX_STEPS; ++i)
        if (e->steps[i].op != FQ_OP_PUSH && e->steps[i].op != FQ_OP_LOAD && !is_chain_dtype(e->steps[i].dtype))
            return false;
    return true;
}
bool call_is_64(const fq_col *cols, int32_t n_cols, const fq_pred *pred, const fq_expr *value) {
    for (int j = 0; j < n_cols; ++j)
        if (!is_chain_dtype(cols[j].dtype)) return false;
    if (!expr_is_64(value)) return false;
    if (pred && pred->kind == FQ_PRED_EXPR) return is_chain_dtype(pred->cmp_dtype) && expr_is_64(&pred->lhs);
    if (pred && pred->kind == FQ_PRED_TREE && pred->tree)
        for (int l = 0; l < pred->tree->n_leaves && l < FQ_MAX_PRED_LEAVES; ++l)
            if (!is_chain_dtype(pred->tree->leaves[l].cmp_dtype) || !expr_is_64(&pred->tree->leaves[l].lhs))
                return false;
    return true;
}

static fq_status plan_scan_typed(const fq_col *cols, int32_t n_cols, int64_t block_rows, const fq_pred *pred,
                                 const fq_expr *value, uint32_t agg_mask, bool need_data, Launch &L, bool &chain,
                                 uint64_t &blocks, int &empty_if_zero, bool nullable = false) {
    const int64_t len = cols[0].len;
    if (block_rows <= 0) block_rows = len > 0 ? len : 1;
    L = Launch{};
    L.typed = true;
    L.nullable = nullable;
    L.col = cols[0].data;
    L.n = len;
    L.block_rows = block_rows;
    L.mask = agg_mask;
    L.n_cols = n_cols;
    for (int j = 0; j < n_cols; ++j) {
        L.cols[j] = cols[j].data;
        L.cdt[j] = cols[j].dtype;
    }
    chain = value && value->n_steps > 0;
    int32_t vdt = L.cdt[0];
    if (chain) {
        fq_status s = lower_expr_typed(*value, L.cdt, n_cols, L.val, vdt);
        if (s != FQ_OK) return s;
    }
    L.vdtype = vdt;
    fq_status ps = lower_pred_typed(pred, L.cdt, n_cols, len, need_data, L.pred);
    if (ps != FQ_OK) return ps;

    blocks = len == 0 ? 0 : (uint64_t)((len + block_rows - 1) / block_rows);
    L.block_mode = L.pred.kind != FQ_PRED_NONE && (agg_mask & FQ_AGG_SUM) && blocks > 1;
    empty_if_zero = (L.pred.kind != FQ_PRED_NONE && blocks == 1) ? 1 : 0;
    if (nullable) {  // an unfiltered block whose values are all null is a None sum too
        L.block_mode = (agg_mask & FQ_AGG_SUM) && blocks > 1;
        empty_if_zero = blocks == 1 ? 1 : 0;
    }

    typed_group(L.cdt, n_cols, &L.group, &L.prefetch);
    const int64_t G = L.group;
    // the grouped loads need the same rows of every column at a multiple of G elements
    bool same_phase = true, aligned = true;
    const int64_t phase0 = (int64_t)((((uintptr_t)cols[0].data) / fqc::dtype_size(L.cdt[0])) % G);
    for (int j = 0; j < n_cols; ++j) {
        const int64_t ph = (int64_t)((((uintptr_t)cols[j].data) / fqc::dtype_size(L.cdt[j])) % G);
        same_phase = same_phase && ph == phase0;
        aligned = aligned && ph == 0;
    }
    const int cus = fqc::device_cu_count();
    const int max_grid = cus * 8 < kMaxPartials ? cus * 8 : kMaxPartials;
    if (L.block_mode) {
        int64_t grid = ((int64_t)blocks + (kThreads / kWave) - 1) / (kThreads / kWave);
        L.grid = (int)(grid < max_grid ? (grid < 1 ? 1 : grid) : max_grid);
        L.head = 0;
        L.vec = aligned && (block_rows % G) == 0;
    } else {
        L.vec = same_phase;
        int64_t head = (G - phase0) % G;
        if (head > len) head = len;
        L.head = L.vec ? head : 0;
        const int64_t tile_rows = (int64_t)kThreads * G;
        int64_t grid = (len + tile_rows - 1) / tile_rows;
        if (grid < 1) grid = 1;
        const int64_t flat_max = (int64_t)cus * scan_wg_per_cu();
        L.grid = (int)(grid < flat_max ? grid : flat_max);
    }
    return FQ_OK;
}

bool typed_scan_fits(const int32_t *cdt, int32_t n_cols, const fq_pred *pred, const fq_expr *value) {
    if (!cdt || n_cols < 1 || n_cols > FQ_MAX_SCAN_COLS) return false;
    KProg val;
    KPred kp;
    int32_t vdt = cdt[0];
    if (value && value->n_steps > 0 && lower_expr_typed(*value, cdt, n_cols, val, vdt) != FQ_OK) return false;
    return lower_pred_typed(pred, cdt, n_cols, 0, false, kp) == FQ_OK;
}

}  // namespace fqk

extern "C" {

fq_status fq_aggregate_typed(const fq_col *cols, int32_t n_cols, int64_t block_rows, const fq_pred *pred,
                             const fq_expr *value, uint32_t agg_mask, fq_agg_state *d_out, void *d_ws,
                             size_t ws_bytes, void *stream) {
    using namespace fqk;
    fq_status s = check_cols_typed(cols, n_cols, true, "fq_aggregate_typed");
    if (s != FQ_OK) return s;
    if (call_is_64(cols, n_cols, pred, value))
        return fq_aggregate_columns(cols, n_cols, block_rows, pred, value, agg_mask, d_out, d_ws, ws_bytes, stream);
    if (!d_out || !d_ws) return fqc::fail(FQ_E_INVALID, "fq_aggregate_typed: NULL argument");
    if (ws_bytes < kPartialsBytes) return fqc::fail(FQ_E_INVALID, "fq_aggregate_typed: workspace too small");
    if (agg_mask & ~(uint32_t)(FQ_AGG_MIN | FQ_AGG_MAX | FQ_AGG_SUM | FQ_AGG_COUNT))
        return fqc::fail(FQ_E_INVALID, "fq_aggregate_typed: unknown bits in agg_mask");
    Launch L;
    bool chain = false;
    uint64_t blocks = 0;
    int empty_if_zero = 0;
    s = plan_scan_typed(cols, n_cols, block_rows, pred, value, agg_mask, true, L, chain, blocks, empty_if_zero);
    if (s != FQ_OK) return s;
    L.stream = (hipStream_t)stream;
    L.parts = (Partial *)d_ws;
    if (agg_mask == FQ_AGG_COUNT && !chain && L.pred.kind == FQ_PRED_NONE) {
        L.grid = 0;  // count(column): rows, not values (see launch_finalize)
        return dispatch_finalize(L, blocks, empty_if_zero, d_out);
    }
    bool jitted = false;
    s = jit_scan(cols[0].dtype, chain, L, &jitted, true);
    if (s != FQ_OK) return s;
    if (!jitted) return fqc::fail(FQ_E_UNSUPPORTED, kTypedNeedsJit);
    return dispatch_finalize(L, blocks, empty_if_zero, d_out);
}

fq_status fq_jit_prepare_typed(const fq_col *cols, int32_t n_cols, int64_t block_rows, const fq_pred *pred,
                               const fq_expr *value, uint32_t agg_mask, int32_t *specialised) {
    using namespace fqk;
    if (specialised) *specialised = 0;
    fq_status s = check_cols_typed(cols, n_cols, false, "fq_jit_prepare_typed");
    if (s != FQ_OK) return s;
    if (call_is_64(cols, n_cols, pred, value))
        return fq_jit_prepare_columns(cols, n_cols, block_rows, pred, value, agg_mask, specialised);
    Launch L;
    bool chain = false;
    uint64_t blocks = 0;
    int empty_if_zero = 0;
    s = plan_scan_typed(cols, n_cols, block_rows, pred, value, agg_mask, false, L, chain, blocks, empty_if_zero);
    if (s != FQ_OK) return s;
    bool ok = false;
    s = jit_prepare(cols[0].dtype, chain, L, &ok);
    if (s != FQ_OK) return s;
    if (!ok) return fqc::fail(FQ_E_UNSUPPORTED, kTypedNeedsJit);
    if (specialised) *specialised = 1;
    return FQ_OK;
}

size_t fq_aggregate_nullable_workspace_bytes(int64_t len) {
    (void)len;
    return (size_t)fqk::kMaxPartials * sizeof(fqk::PartialN);
}

fq_status fq_aggregate_nullable(const fq_col *cols, const uint64_t *const *validity, int32_t n_cols,
                                int64_t block_rows, const fq_pred *pred, const fq_expr *value, uint32_t agg_mask,
                                fq_agg_state_n *d_out, void *d_ws, size_t ws_bytes, void *stream) {
    using namespace fqk;
    fq_status s = check_cols_typed(cols, n_cols, true, "fq_aggregate_nullable");
    if (s != FQ_OK) return s;
    if (!validity || !d_out || !d_ws) return fqc::fail(FQ_E_INVALID, "fq_aggregate_nullable: NULL argument");
    for (int j = 0; j < n_cols; ++j)
        if (((uintptr_t)validity[j]) % 8)
            return fqc::fail(FQ_E_INVALID, "fq_aggregate_nullable: validity bitmap " + std::to_string(j) +
                                               " not aligned to 8 bytes");
    if (ws_bytes < fq_aggregate_nullable_workspace_bytes(cols[0].len))
        return fqc::fail(FQ_E_INVALID, "fq_aggregate_nullable: workspace too small");
    if (agg_mask & ~(uint32_t)(FQ_AGG_MIN | FQ_AGG_MAX | FQ_AGG_SUM | FQ_AGG_COUNT))
        return fqc::fail(FQ_E_INVALID, "fq_aggregate_nullable: unknown bits in agg_mask");
    Launch L;
    bool chain = false;
    uint64_t blocks = 0;
    int empty_if_zero = 0;
    s = plan_scan_typed(cols, n_cols, block_rows, pred, value, agg_mask, true, L, chain, blocks, empty_if_zero, true);
    if (s != FQ_OK) return s;
    for (int j = 0; j < n_cols; ++j) {
        L.validity[j] = validity[j];
        L.has_bm[j] = validity[j] != nullptr;
    }
    L.stream = (hipStream_t)stream;
    L.parts = (Partial *)d_ws;  // PartialN behind it (Launch::nullable)
    if (agg_mask == FQ_AGG_COUNT && !chain && L.pred.kind == FQ_PRED_NONE) {
        L.grid = 0;  // count(column): rows, nulls included -- neither the column nor its bitmap is read
        return dispatch_finalize_nullable(L, blocks, empty_if_zero, d_out);
    }
    bool jitted = false;
    s = jit_scan(cols[0].dtype, chain, L, &jitted, true);
    if (s != FQ_OK) return s;
    if (!jitted) return fqc::fail(FQ_E_UNSUPPORTED, kTypedNeedsJit);
    return dispatch_finalize_nullable(L, blocks, empty_if_zero, d_out);
}

fq_status fq_jit_prepare_nullable(const fq_col *cols, const uint8_t *has_validity, int32_t n_cols, int64_t block_rows,
                                  const fq_pred *pred, const fq_expr *value, uint32_t agg_mask,
                                  int32_t *specialised) {
    using namespace fqk;
    if (specialised) *specialised = 0;
    fq_status s = check_cols_typed(cols, n_cols, false, "fq_jit_prepare_nullable");
    if (s != FQ_OK) return s;
    Launch L;
    bool chain = false;
    uint64_t blocks = 0;
    int empty_if_zero = 0;
    s = plan_scan_typed(cols, n_cols, block_rows, pred, value, agg_mask, false, L, chain, blocks, empty_if_zero, true);
    if (s != FQ_OK) return s;
    for (int j = 0; j < n_cols; ++j) L.has_bm[j] = has_validity && has_validity[j];
    bool ok = false;
    s = jit_prepare(cols[0].dtype, chain, L, &ok);
    if (s != FQ_OK) return s;
    if (!ok) return fqc::fail(FQ_E_UNSUPPORTED, kTypedNeedsJit);
    if (specialised) *specialised = 1;
    return FQ_OK;
}

fq_status fq_aggregate_columns(const fq_col *cols, int32_t n_cols, int64_t block_rows, const fq_pred *pred,
                               const fq_expr *value, uint32_t agg_mask, fq_agg_state *d_out, void *d_ws,
                               size_t ws_bytes, void *stream) {
    fq_status s = fqk::check_cols(cols, n_cols, true);
    if (s != FQ_OK) return s;
    if (n_cols == 1) {
        s = fqk::check_one_col(cols, pred, value);
        if (s != FQ_OK) return s;
        return fqk::aggregate(cols, block_rows, pred, value, agg_mask, d_out, d_ws, ws_bytes, (hipStream_t)stream);
    }
    return fqk::aggregate_cols(cols, n_cols, block_rows, pred, value, agg_mask, d_out, d_ws, ws_bytes,
                               (hipStream_t)stream);
}

fq_status fq_jit_prepare_columns(const fq_col *cols, int32_t n_cols, int64_t block_rows, const fq_pred *pred,
                                 const fq_expr *value, uint32_t agg_mask, int32_t *specialised) {
    using namespace fqk;
    if (specialised) *specialised = 0;
    fq_status s = check_cols(cols, n_cols, false);
    if (s != FQ_OK) return s;
    if (n_cols == 1) {
        s = check_one_col(cols, pred, value);
        if (s != FQ_OK) return s;
        return fq_jit_prepare(cols, block_rows, pred, value, agg_mask, specialised);
    }
    Launch L;
    bool chain = false;
    uint64_t blocks = 0;
    int empty_if_zero = 0;
    s = plan_scan_cols(cols, n_cols, block_rows, pred, value, agg_mask, false, L, chain, blocks, empty_if_zero);
    if (s != FQ_OK) return s;
    bool ok = false;
    s = jit_prepare(cols[0].dtype, chain, L, &ok);
    if (s != FQ_OK) return s;
    if (!ok)
        return fqc::fail(FQ_E_UNSUPPORTED, "scans over several columns run on the hipRTC kernels only (FQ_JIT is off "
                                           "or hipRTC is unavailable)");
    if (specialised) *specialised = 1;
    return FQ_OK;
}

fq_status fq_aggregate(const fq_col *col, int64_t block_rows, const fq_pred *pred, const fq_expr *value,
                       uint32_t agg_mask, fq_agg_state *d_out, void *d_ws, size_t ws_bytes, void *stream) {
    return fqk::aggregate(col, block_rows, pred, value, agg_mask, d_out, d_ws, ws_bytes, (hipStream_t)stream);
}

int64_t fq_for32_frames(int64_t len) { return len <= 0 ? 0 : (len + fqk::kFrame - 1) / fqk::kFrame; }

size_t fq_for32_delta_bytes(int64_t len) { return len <= 0 ? 0 : (((size_t)len * 4 + 255) / 256) * 256; }

size_t fq_for32_base_bytes(int64_t len) { return (size_t)fq_for32_frames(len) * 8; }

fq_status fq_for32_encode(const fq_col *col, uint64_t *d_base, uint32_t *d_delta, uint32_t *d_flag, void *stream) {
    using namespace fqk;
    if (!col || !d_flag) return fqc::fail(FQ_E_INVALID, "fq_for32_encode: NULL argument");
    if (col->len < 0) return fqc::fail(FQ_E_INVALID, "fq_for32_encode: negative length");
    if (col->dtype != FQ_DT_UINT64)
        return fqc::fail(FQ_E_UNSUPPORTED, std::string("fq_for32_encode: ") + fqc::dtype_name(col->dtype) +
                                               " column (the encoding is defined for UInt64)");
    if (col->len > 0 && (!col->data || !d_base || !d_delta))
        return fqc::fail(FQ_E_INVALID, "fq_for32_encode: NULL argument");
    if (((uintptr_t)col->data) % 8 || ((uintptr_t)d_base) % 8)
        return fqc::fail(FQ_E_INVALID, "fq_for32_encode: column / base not aligned to 8 bytes");
    if (((uintptr_t)d_delta) % 16) return fqc::fail(FQ_E_INVALID, "fq_for32_encode: delta not aligned to 16 bytes");
    FQ_HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(uint32_t), (hipStream_t)stream));
    if (col->len == 0) return FQ_OK;
    const int64_t frames = fq_for32_frames(col->len);
    const int64_t max_grid = (int64_t)fqc::device_cu_count() * 8;
    const int grid = (int)(frames < max_grid ? frames : max_grid);
    hipLaunchKernelGGL(for32_encode_kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream,
                       (const uint64_t *)col->data, col->len, d_base, d_delta, d_flag);
    FQ_HIP_TRY(hipGetLastError());
    return FQ_OK;
}

}  // extern "C"

namespace fqk {

// fq_aggregate_for32, over `blocks` reference blocks (fq_aggregate_for32_expr
// without predicate and expression passes its block_rows' count)
static fq_status aggregate_for32(const uint32_t *d_delta, const uint64_t *d_base, int64_t len, uint64_t blocks,
                                 uint32_t agg_mask, fq_agg_state *d_out, void *d_ws, size_t ws_bytes, void *stream) {
    if (!d_out || !d_ws) return fqc::fail(FQ_E_INVALID, "fq_aggregate_for32: NULL argument");
    if (len < 0) return fqc::fail(FQ_E_INVALID, "fq_aggregate_for32: negative length");
    if (ws_bytes < kPartialsBytes) return fqc::fail(FQ_E_INVALID, "fq_aggregate_for32: workspace too small");
    if (agg_mask & ~(uint32_t)(FQ_AGG_MIN | FQ_AGG_MAX | FQ_AGG_SUM | FQ_AGG_COUNT))
        return fqc::fail(FQ_E_INVALID, "fq_aggregate_for32: unknown bits in agg_mask");
    if (((uintptr_t)d_delta) % 16) return fqc::fail(FQ_E_INVALID, "fq_aggregate_for32: delta not aligned to 16 bytes");
    if (((uintptr_t)d_base) % 8) return fqc::fail(FQ_E_INVALID, "fq_aggregate_for32: base not aligned to 8 bytes");
    Launch L{};
    L.n = len;
    L.mask = agg_mask;
    L.vdtype = FQ_DT_UINT64;
    L.parts = (Partial *)d_ws;
    L.stream = (hipStream_t)stream;
    if (agg_mask == FQ_AGG_COUNT) {
        L.grid = 0;  // count(column): rows, not values (see launch_finalize)
        return dispatch_finalize(L, blocks, 0, d_out);
    }
    if (len > 0 && (!d_delta || !d_base)) return fqc::fail(FQ_E_INVALID, "fq_aggregate_for32: NULL argument");
    int64_t grid = (len / 4 + kFor32Tile / 4 - 1) / (kFor32Tile / 4);
    if (grid < 1) grid = 1;
    const int64_t flat_max = (int64_t)fqc::device_cu_count() * scan_wg_per_cu();
    L.grid = (int)(grid < flat_max ? grid : flat_max);
    hipLaunchKernelGGL(agg_flat_kernel_for32, dim3(L.grid), dim3(kThreads), 0, L.stream, d_delta, d_base, len,
                       agg_mask, L.parts);
    FQ_HIP_TRY(hipGetLastError());
    return dispatch_finalize(L, blocks, 0, d_out);
}

static bool for32_identity(const fq_pred *pred, const fq_expr *value) {
    return (!pred || pred->kind == FQ_PRED_NONE) && (!value || value->n_steps <= 0);
}

static const char *kFor32NeedsJit =
    "fused scans over 32-bit deltas run on the hipRTC kernel only (FQ_JIT is off or hipRTC is unavailable)";

// The plan of fq_aggregate_for32_expr / fq_jit_prepare_for32 for a call with a
// predicate or an expression: fq_aggregate's over the UInt64 column the deltas
// stand for (lowered programs, flat / block mode, blocks), with the flat grid
// of fq_aggregate_for32.
static fq_status plan_scan_for32(const uint32_t *d_delta, const uint64_t *d_base, int64_t len, int64_t block_rows,
                                 const fq_pred *pred, const fq_expr *value, uint32_t agg_mask, bool need_data,
                                 Launch &L, bool &chain, uint64_t &blocks, int &empty_if_zero) {
    fq_col col{};
    col.data = (void *)d_delta;
    col.dtype = FQ_DT_UINT64;
    col.len = len;
    fq_status s = plan_scan(&col, block_rows, pred, value, agg_mask, need_data, L, chain, blocks, empty_if_zero);
    if (s != FQ_OK) return s;
    L.for32 = true;
    L.for32_base = d_base;
    L.head = 0;
    if (!L.block_mode) L.grid = for32_flat_grid(len, (int64_t)fqc::device_cu_count() * scan_wg_per_cu());
    return FQ_OK;
}

}  // namespace fqk

extern "C" {

fq_status fq_aggregate_for32(const uint32_t *d_delta, const uint64_t *d_base, int64_t len, uint32_t agg_mask,
                             fq_agg_state *d_out, void *d_ws, size_t ws_bytes, void *stream) {
    // one block, as fq_aggregate with block_rows = 0
    return fqk::aggregate_for32(d_delta, d_base, len, len > 0 ? 1 : 0, agg_mask, d_out, d_ws, ws_bytes, stream);
}

fq_status fq_aggregate_for32_expr(const uint32_t *d_delta, const uint64_t *d_base, int64_t len, int64_t block_rows,
                                  const fq_pred *pred, const fq_expr *value, uint32_t agg_mask, fq_agg_state *d_out,
                                  void *d_ws, size_t ws_bytes, void *stream) {
    using namespace fqk;
    if (for32_identity(pred, value)) {
        if (block_rows <= 0) block_rows = len > 0 ? len : 1;
        const uint64_t blocks = len <= 0 ? 0 : (uint64_t)((len + block_rows - 1) / block_rows);
        return aggregate_for32(d_delta, d_base, len, blocks, agg_mask, d_out, d_ws, ws_bytes, stream);
    }
    if (!d_out || !d_ws) return fqc::fail(FQ_E_INVALID, "fq_aggregate_for32_expr: NULL argument");
    if (len < 0) return fqc::fail(FQ_E_INVALID, "fq_aggregate_for32_expr: negative length");
    if (ws_bytes < kPartialsBytes) return fqc::fail(FQ_E_INVALID, "fq_aggregate_for32_expr: workspace too small");
    if (agg_mask & ~(uint32_t)(FQ_AGG_MIN | FQ_AGG_MAX | FQ_AGG_SUM | FQ_AGG_COUNT))
        return fqc::fail(FQ_E_INVALID, "fq_aggregate_for32_expr: unknown bits in agg_mask");
    if (((uintptr_t)d_delta) % 16)
        return fqc::fail(FQ_E_INVALID, "fq_aggregate_for32_expr: delta not aligned to 16 bytes");
    if (((uintptr_t)d_base) % 8) return fqc::fail(FQ_E_INVALID, "fq_aggregate_for32_expr: base not aligned to 8 bytes");
    if (len > 0 && (!d_delta || !d_base)) return fqc::fail(FQ_E_INVALID, "fq_aggregate_for32_expr: NULL argument");
    Launch L;
    bool chain = false;
    uint64_t blocks = 0;
    int empty_if_zero = 0;
    fq_status s = plan_scan_for32(d_delta, d_base, len, block_rows, pred, value, agg_mask, true, L, chain, blocks,
                                  empty_if_zero);
    if (s != FQ_OK) return s;
    L.stream = (hipStream_t)stream;
    L.parts = (Partial *)d_ws;
    bool jitted = false;
    s = jit_scan(FQ_DT_UINT64, chain, L, &jitted, true);  // no interpreting kernel knows the deltas
    if (s != FQ_OK) return s;
    if (!jitted) return fqc::fail(FQ_E_UNSUPPORTED, kFor32NeedsJit);
    return dispatch_finalize(L, blocks, empty_if_zero, d_out);
}

fq_status fq_jit_prepare_for32(int64_t len, int64_t block_rows, const fq_pred *pred, const fq_expr *value,
                               uint32_t agg_mask, int32_t *specialised) {
    using namespace fqk;
    if (specialised) *specialised = 0;
    if (len < 0) return fqc::fail(FQ_E_INVALID, "fq_jit_prepare_for32: negative length");
    if (agg_mask & ~(uint32_t)(FQ_AGG_MIN | FQ_AGG_MAX | FQ_AGG_SUM | FQ_AGG_COUNT))
        return fqc::fail(FQ_E_INVALID, "fq_jit_prepare_for32: unknown bits in agg_mask");
    if (for32_identity(pred, value)) return FQ_OK;  // the precompiled agg_flat_kernel_for32
    Launch L;
    bool chain = false;
    uint64_t blocks = 0;
    int empty_if_zero = 0;
    fq_status s = plan_scan_for32(nullptr, nullptr, len, block_rows, pred, value, agg_mask, false, L, chain, blocks,
                                  empty_if_zero);
    if (s != FQ_OK) return s;
    bool ok = false;
    s = jit_prepare(FQ_DT_UINT64, chain, L, &ok);
    if (s != FQ_OK) return s;
    if (!ok) return fqc::fail(FQ_E_UNSUPPORTED, kFor32NeedsJit);
    if (specialised) *specialised = 1;
    return FQ_OK;
}

fq_status fq_jit_prepare(const fq_col *col, int64_t block_rows, const fq_pred *pred, const fq_expr *value,
                         uint32_t agg_mask, int32_t *specialised) {
    using namespace fqk;
    if (specialised) *specialised = 0;
    Launch L;
    bool chain = false;
    uint64_t blocks = 0;
    int empty_if_zero = 0;
    fq_status s = plan_scan(col, block_rows, pred, value, agg_mask, false, L, chain, blocks, empty_if_zero);
    if (s != FQ_OK) return s;
    bool ok = false;
    s = jit_prepare(col->dtype, chain, L, &ok);
    if (s == FQ_OK && specialised) *specialised = ok ? 1 : 0;
    return s;
}

}  // extern "C"
