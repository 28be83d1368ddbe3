// FilterTransform compaction on gfx950 (arrow filter_record_batch,
// src/transforms/transform_filter.rs:51): keep the rows whose predicate bit
// is set, preserving order.
//
// Three passes over tiles of 256 bitmap words (16,384 rows), in groups of 16:
//   count   one workgroup per group: popcounts of its tiles -> each tile's
//           exclusive prefix inside the group, and the group's total
//   scan    one workgroup: exclusive scan of the group totals
//   scatter one workgroup per tile, LDS scan of its word popcounts, then:
//           8-byte aligned columns: two 8,192-row rounds, each loading row
//           pairs with 16-byte loads, dropping kept rows into an LDS stage
//           at their output offset and writing the round's contiguous output
//           range with aligned 16-byte stores;
//           other widths: each wave walks 64 words, 8 at a time; lane l
//           moves row 64w+l to base + word_offset + popcount(word & lt(l)).
// The bitmap is read twice (1/64 of a u64 column's bytes each time).
#include <hip/hip_runtime.h>

#include "fq_common.h"
#include "fq_device.h"
#include "fq_scan.h"

namespace fqk {

constexpr int kTileWords = 256;

__device__ __forceinline__ uint64_t word_at(const uint64_t *bm, int64_t w, int64_t nwords, int64_t n) {
    if (w >= nwords) return 0;
    uint64_t v = bm[w];
    const int64_t rows = n - w * 64;
    if (rows < 64) v &= (1ull << rows) - 1ull;  // ignore bits past len
    return v;
}

// count: workgroup g covers the kGroupTiles tiles of group g (wave w: tiles
// 4w..4w+3 of the group, all 16 word loads of a lane in flight together);
// writes each tile's exclusive prefix within the group -> intra[tile] and
// the group's total -> gpre[g].
constexpr int kGroupTiles = 16;
constexpr int kWaveTiles = kGroupTiles / (kTileWords / kWave);

__global__ void __launch_bounds__(kTileWords)
    compact_count_kernel(const uint64_t *__restrict__ bm, int64_t n, int64_t ntiles, uint64_t *__restrict__ intra,
                         uint64_t *__restrict__ gpre) {
    const int64_t nwords = (n + 63) / 64;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    const int64_t t0 = (int64_t)blockIdx.x * kGroupTiles + wave * kWaveTiles;
    uint64_t wd[kWaveTiles][kTileWords / kWave];
#pragma unroll
    for (int k = 0; k < kWaveTiles; ++k)
#pragma unroll
        for (int j = 0; j < kTileWords / kWave; ++j)
            wd[k][j] = bm[min((t0 + k) * kTileWords + j * kWave + lane, nwords - 1)];  // all in flight
#pragma unroll
    for (int k = 0; k < kWaveTiles; ++k)
#pragma unroll
        for (int j = 0; j < kTileWords / kWave; ++j) {
            const int64_t w = (t0 + k) * kTileWords + j * kWave + lane;
            const int64_t rows = n - w * 64;
            if (rows <= 0) wd[k][j] = 0;
            else if (rows < 64) wd[k][j] &= (1ull << rows) - 1ull;  // ignore bits past len
        }
    __shared__ uint64_t s_c[kGroupTiles];
#pragma unroll
    for (int k = 0; k < kWaveTiles; ++k) {
        uint64_t c = 0;
#pragma unroll
        for (int j = 0; j < kTileWords / kWave; ++j) c += __popcll(wd[k][j]);
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) c += shfl_xor64(c, off);
        if (lane == 0) s_c[wave * kWaveTiles + k] = c;
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < kGroupTiles) {
        uint64_t pre = 0;
        for (int i = 0; i < t; ++i) pre += s_c[i];
        const int64_t tile = (int64_t)blockIdx.x * kGroupTiles + t;
        if (tile < ntiles) intra[tile] = pre;
        if (t == kGroupTiles - 1) gpre[blockIdx.x] = pre + s_c[t];
    }
}

// exclusive scan of gpre[0..m) in place, gpre[m] = total.  One workgroup;
// the array is taken 16,384 entries per round, 16 consecutive entries per
// thread loaded together (indices clamped, values masked), so a round costs
// one memory round trip.
constexpr int kScanThreads = 1024;
constexpr int kScanPer = 16;

__global__ void __launch_bounds__(kScanThreads) compact_scan_kernel(uint64_t *gpre, int64_t m) {
    constexpr int W = kScanThreads / kWave;
    const int t = threadIdx.x;
    const int lane = t & (kWave - 1);
    const int wave = t / kWave;
    __shared__ uint64_t s_w[W];
    uint64_t run = 0;  // uniform: total of the earlier rounds
    for (int64_t r0 = 0; r0 < m; r0 += (int64_t)kScanThreads * kScanPer) {
        const int64_t i0 = r0 + (int64_t)t * kScanPer;
        uint64_t v[kScanPer];
#pragma unroll
        for (int k = 0; k < kScanPer; ++k) v[k] = gpre[i0 + k < m ? i0 + k : m - 1];
        uint64_t tot = 0;
#pragma unroll
        for (int k = 0; k < kScanPer; ++k) {
            if (i0 + k >= m) v[k] = 0;
            tot += v[k];
        }
        uint64_t incl = tot;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const uint64_t u = shfl_up64(incl, off);
            if (lane >= off) incl += u;
        }
        if (lane == kWave - 1) s_w[wave] = incl;
        __syncthreads();
        uint64_t wbase = 0, rtot = 0;
        for (int w = 0; w < W; ++w) {
            const uint64_t x = s_w[w];
            if (w < wave) wbase += x;
            rtot += x;
        }
        uint64_t p = run + wbase + incl - tot;
#pragma unroll
        for (int k = 0; k < kScanPer; ++k) {
            if (i0 + k < m) gpre[i0 + k] = p;
            p += v[k];
        }
        run += rtot;
        __syncthreads();  // s_w reused by the next round
    }
    if (t == 0) gpre[m] = run;
}

__device__ __forceinline__ uint64_t tile_base(const uint64_t *intra, const uint64_t *gpre, int64_t tile) {
    return gpre[tile / kGroupTiles] + intra[tile];
}

template <typename T>
__global__ void __launch_bounds__(kTileWords)
    compact_scatter_kernel(const T *__restrict__ in, const uint64_t *__restrict__ bm, int64_t n,
                           const uint64_t *__restrict__ intra, const uint64_t *__restrict__ gpre, T *__restrict__ out) {
    const int64_t nwords = (n + 63) / 64;
    const int64_t w0 = (int64_t)blockIdx.x * kTileWords;
    __shared__ uint64_t s_word[kTileWords];
    __shared__ uint32_t s_off[kTileWords];
    __shared__ uint32_t s_wsum[kTileWords / kWave];
    const int t = threadIdx.x;
    const int lane = t & (kWave - 1);
    const int wave = t / kWave;
    const uint64_t word = word_at(bm, w0 + t, nwords, n);
    s_word[t] = word;
    // wave-inclusive scan of popcounts
    uint32_t c = (uint32_t)__popcll(word);
    uint32_t incl = c;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)incl, off, kWave);
        if (lane >= off) incl += v;
    }
    if (lane == kWave - 1) s_wsum[wave] = incl;
    __syncthreads();
    uint32_t wave_base = 0;
    for (int i = 0; i < wave; ++i) wave_base += s_wsum[i];
    s_off[t] = wave_base + incl - c;
    __syncthreads();
    const uint64_t base = tile_base(intra, gpre, blockIdx.x);
    const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    // 8 words per step: all loads of the step are issued before the first
    // store (8 rows per lane in flight); empty words are skipped (uniform).
    constexpr int kStep = 8;
    for (int j = 0; j < kWave; j += kStep) {
        T x[kStep];
        uint64_t wd[kStep];
#pragma unroll
        for (int k = 0; k < kStep; ++k) {
            const int wi = wave * kWave + j + k;
            wd[k] = s_word[wi];
            const int64_t row = (w0 + wi) * 64 + lane;
            x[k] = ((wd[k] >> lane) & 1ull) ? __builtin_nontemporal_load(in + row) : T(0);
        }
#pragma unroll
        for (int k = 0; k < kStep; ++k) {
            const int wi = wave * kWave + j + k;
            if ((wd[k] >> lane) & 1ull) {
                const uint64_t pos = base + s_off[wi] + (uint64_t)__popcll(wd[k] & lt_mask);
                out[pos] = x[k];
            }
        }
    }
}

// 8-byte columns, 16-byte aligned: lane l of a wave loads rows 2l and 2l+1
// of a 128-row word pair with one 16-byte load (lanes 0..31: the pair's first
// word, 32..63: its second), 4 pairs in flight per step; positions come from
// the same LDS word offsets.
typedef unsigned long long u64x2_t __attribute__((ext_vector_type(2)));

template <typename T>
__global__ void __launch_bounds__(kTileWords)
    compact_scatter_vec_kernel(const T *__restrict__ in, const uint64_t *__restrict__ bm, int64_t n,
                               const uint64_t *__restrict__ intra, const uint64_t *__restrict__ gpre, T *__restrict__ out) {
    static_assert(sizeof(T) == 8, "8-byte rows");
    const int64_t nwords = (n + 63) / 64;
    const int64_t w0 = (int64_t)blockIdx.x * kTileWords;
    __shared__ uint64_t s_word[kTileWords];
    __shared__ uint32_t s_off[kTileWords];
    __shared__ uint32_t s_wsum[kTileWords / kWave];
    const int t = threadIdx.x;
    const int lane = t & (kWave - 1);
    const int wave = t / kWave;
    const uint64_t word = word_at(bm, w0 + t, nwords, n);
    s_word[t] = word;
    uint32_t c = (uint32_t)__popcll(word);
    uint32_t incl = c;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)incl, off, kWave);
        if (lane >= off) incl += v;
    }
    if (lane == kWave - 1) s_wsum[wave] = incl;
    __syncthreads();
    uint32_t wave_base = 0;
    for (int i = 0; i < wave; ++i) wave_base += s_wsum[i];
    s_off[t] = wave_base + incl - c;
    __syncthreads();
    const uint64_t base = tile_base(intra, gpre, blockIdx.x);
    const int half = lane >> 5;        // which word of the pair
    const int bl = (lane & 31) * 2;    // bit of this lane's first row in that word
    const uint64_t m_lt = bl == 0 ? 0ull : (~0ull >> (64 - bl));
    const u64x2_t *__restrict__ vin = reinterpret_cast<const u64x2_t *>(in);
    constexpr int kPairs = 4;
    for (int j = 0; j < kWave; j += 2 * kPairs) {
        u64x2_t x[kPairs];
        uint64_t wd[kPairs];
#pragma unroll
        for (int k = 0; k < kPairs; ++k) {
            const int wi = wave * kWave + j + 2 * k + half;
            wd[k] = s_word[wi];
            const int64_t row = (w0 + wave * kWave + j + 2 * k) * 64 + 2 * lane;
            const uint64_t bits = (wd[k] >> bl) & 3ull;
            x[k] = u64x2_t{0, 0};
            if (bits) {
                if (row + 1 < n) {
                    x[k] = __builtin_nontemporal_load(vin + (row >> 1));
                } else {
                    x[k].x = (unsigned long long)__builtin_bit_cast(uint64_t, in[row]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kPairs; ++k) {
            const int wi = wave * kWave + j + 2 * k + half;
            const uint64_t bits = (wd[k] >> bl) & 3ull;
            if (!bits) continue;
            uint64_t pos = base + s_off[wi] + (uint64_t)__popcll(wd[k] & m_lt);
            if (bits & 1ull) out[pos++] = __builtin_bit_cast(T, (uint64_t)x[k].x);
            if (bits & 2ull) out[pos] = __builtin_bit_cast(T, (uint64_t)x[k].y);
        }
    }
}

// 8-byte columns, input and output 16-byte aligned: the tile is compacted in
// two 8,192-row rounds through LDS (64 KB stage, 2 workgroups per CU).  Each thread loads 8 row pairs with
// 16-byte loads (consecutive threads, consecutive pairs), drops the kept rows
// into a 32 KB LDS stage at their offset within the round, and the
// workgroup then writes the round's contiguous output range as aligned
// 16-byte stores (8-byte stores only at its two ends).
constexpr int kRoundWords = 128;
constexpr int kRoundPairs = kRoundWords * 32;

template <typename T>
__global__ void __launch_bounds__(kTileWords)
    compact_scatter_lds_kernel(const T *__restrict__ in, const uint64_t *__restrict__ bm, int64_t n,
                               const uint64_t *__restrict__ intra, const uint64_t *__restrict__ gpre, T *__restrict__ out) {
    static_assert(sizeof(T) == 8, "8-byte rows");
    const int64_t nwords = (n + 63) / 64;
    const int64_t tile = blockIdx.x;
    const int64_t w0 = tile * kTileWords;
    __shared__ uint64_t s_word[kTileWords];
    __shared__ uint32_t s_off[kTileWords + 1];
    __shared__ uint32_t s_wsum[kTileWords / kWave];
    __shared__ uint64_t s_stage[kRoundPairs * 2];
    const int t = threadIdx.x;
    const int lane = t & (kWave - 1);
    const int wave = t / kWave;
    const uint64_t word = word_at(bm, w0 + t, nwords, n);
    s_word[t] = word;
    uint32_t c = (uint32_t)__popcll(word);
    uint32_t incl = c;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)incl, off, kWave);
        if (lane >= off) incl += v;
    }
    if (lane == kWave - 1) s_wsum[wave] = incl;
    __syncthreads();
    uint32_t wave_base = 0;
    for (int i = 0; i < wave; ++i) wave_base += s_wsum[i];
    s_off[t] = wave_base + incl - c;
    if (t == kTileWords - 1) s_off[kTileWords] = wave_base + incl;
    __syncthreads();
    const uint64_t base = tile_base(intra, gpre, tile);
    const u64x2_t *__restrict__ vin = reinterpret_cast<const u64x2_t *>(in);
    u64x2_t *__restrict__ vout = reinterpret_cast<u64x2_t *>(out);
    constexpr int kPer = kRoundPairs / kTileWords;
    for (int rw = 0; rw < kTileWords; rw += kRoundWords) {
        const uint32_t rb = s_off[rw], re = s_off[rw + kRoundWords];
        if (rb == re) continue;  // nothing kept in this round (uniform)
        const int64_t row_r = (w0 + rw) * 64;
        u64x2_t x[kPer];
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const int v = t + kTileWords * i;
            const int64_t row = row_r + 2 * v;
            const uint64_t bits = (s_word[rw + (v >> 5)] >> ((2 * v) & 63)) & 3ull;
            x[i] = u64x2_t{0, 0};
            if (bits) {
                if (row + 1 < n) {
                    x[i] = __builtin_nontemporal_load(vin + (row >> 1));
                } else if (row < n) {
                    x[i].x = (unsigned long long)__builtin_bit_cast(uint64_t, in[row]);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const int v = t + kTileWords * i;
            const int wi = rw + (v >> 5);
            const int bl = (2 * v) & 63;
            const uint64_t wd = s_word[wi];
            const uint64_t bits = (wd >> bl) & 3ull;
            if (!bits) continue;
            const uint64_t m_lt = bl == 0 ? 0ull : (~0ull >> (64 - bl));
            uint32_t pos = s_off[wi] - rb + (uint32_t)__popcll(wd & m_lt);
            if (bits & 1ull) s_stage[pos++] = (uint64_t)x[i].x;
            if (bits & 2ull) s_stage[pos] = (uint64_t)x[i].y;
        }
        __syncthreads();
        const uint64_t g0 = base + rb, g1 = base + re;
        for (uint64_t p = (g0 >> 1) + t; p < ((g1 + 1) >> 1); p += kTileWords) {
            const uint64_t e0 = 2 * p, e1 = e0 + 1;
            if (e0 >= g0 && e1 < g1) {
                __builtin_nontemporal_store(u64x2_t{s_stage[e0 - g0], s_stage[e1 - g0]}, vout + p);
            } else if (e0 >= g0) {
                out[e0] = __builtin_bit_cast(T, s_stage[e0 - g0]);
            } else {
                out[e1] = __builtin_bit_cast(T, s_stage[e1 - g0]);
            }
        }
        __syncthreads();
    }
}

}  // namespace fqk

extern "C" {

size_t fq_filter_workspace_bytes(int64_t len) {
    const int64_t nwords = (len + 63) / 64;
    const int64_t ntiles = (nwords + fqk::kTileWords - 1) / fqk::kTileWords;
    const int64_t ngroups = (ntiles + fqk::kGroupTiles - 1) / fqk::kGroupTiles;
    return (size_t)(ntiles + ngroups + 1) * sizeof(uint64_t);
}

}  // extern "C"

namespace fqk {
namespace {

// block b of a block stream with every row kept holds min(B, n - b * B) rows
__global__ void block_lengths_kernel(int64_t *__restrict__ counts, int64_t nb, int64_t B, int64_t n) {
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nb; b += (int64_t)gridDim.x * blockDim.x)
        counts[b] = b * B + B <= n ? B : n - b * B;
}

// filter_project_blocks_enqueue with a resident workspace: after the
// projection kernel, one thread moves {kept rows, flag words} to d_res (host
// memory the device writes) and zeroes the three workspace words -- one launch
// in place of the next call's memset and this call's copy.
__global__ void project_hand_off_kernel(uint64_t *__restrict__ ws, uint64_t *__restrict__ d_res) {
    if (threadIdx.x != 0) return;
    d_res[0] = ws[0];
    d_res[1] = ws[1];
    ws[0] = 0;
    ws[1] = 0;
    ws[2] = 0;
}

// ---- fq_blocks_compact: a block stream's valid rows into one array ----
// counts[b] -> exclusive offsets in three launches: per-chunk sums of
// kCompactChunk counts, one workgroup scanning the chunk sums, then each chunk
// scanning its counts from its base; a copy kernel moves block b's rows (one
// workgroup per block, lane-consecutive 8-byte rows: coalesced both sides).
constexpr int kCompactChunk = 1024;

__global__ void __launch_bounds__(kCompactChunk)
blocks_chunk_sums_kernel(const int64_t *__restrict__ counts, int64_t nb, int64_t *__restrict__ sums) {
    __shared__ int64_t red[kCompactChunk / kWave];
    const int64_t b = (int64_t)blockIdx.x * kCompactChunk + threadIdx.x;
    int64_t v = b < nb ? counts[b] : 0;
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t t = 0;
        for (int w = 0; w < kCompactChunk / kWave; ++w) t += red[w];
        sums[blockIdx.x] = t;
    }
}

// exclusive scan of `n` values in place by one workgroup; base[n] = the total
__global__ void __launch_bounds__(kCompactChunk) blocks_scan_sums_kernel(int64_t *__restrict__ sums, int64_t n) {
    __shared__ int64_t part[kCompactChunk];
    const int64_t per = (n + kCompactChunk - 1) / kCompactChunk;
    const int64_t lo = threadIdx.x * per, hi = lo + per < n ? lo + per : n;
    int64_t t = 0;
    for (int64_t i = lo; i < hi; ++i) t += sums[i];
    part[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t run = 0;
        for (int i = 0; i < kCompactChunk; ++i) {
            const int64_t x = part[i];
            part[i] = run;
            run += x;
        }
        sums[n] = run;
    }
    __syncthreads();
    int64_t run = part[threadIdx.x];
    for (int64_t i = lo; i < hi; ++i) {
        const int64_t x = sums[i];
        sums[i] = run;
        run += x;
    }
}

__global__ void __launch_bounds__(kCompactChunk)
blocks_offsets_kernel(const int64_t *__restrict__ counts, int64_t nb, const int64_t *__restrict__ sums,
                      int64_t *__restrict__ offs) {
    __shared__ int64_t part[kCompactChunk];
    const int64_t b = (int64_t)blockIdx.x * kCompactChunk + threadIdx.x;
    part[threadIdx.x] = b < nb ? counts[b] : 0;
    __syncthreads();
    for (int o = 1; o < kCompactChunk; o <<= 1) {  // Hillis-Steele inclusive scan
        const int64_t add = threadIdx.x >= (unsigned)o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    if (b < nb) offs[b] = sums[blockIdx.x] + part[threadIdx.x] - counts[b];
    if (b == nb - 1) offs[nb] = sums[blockIdx.x] + part[threadIdx.x];
}

struct CompactCols {
    const uint64_t *in[FQ_MAX_PROJECT];
    uint64_t *out[FQ_MAX_PROJECT];
};

__global__ void __launch_bounds__(256)
blocks_copy_kernel(CompactCols cols, int32_t n_cols, const int64_t *__restrict__ counts,
                   const int64_t *__restrict__ offs, int64_t nb, int64_t block_rows) {
    for (int64_t b = blockIdx.x; b < nb; b += gridDim.x) {
        const int64_t c = counts[b], src = b * block_rows, dst = offs[b];
        for (int j = 0; j < n_cols; ++j)
            for (int64_t r = threadIdx.x; r < c; r += blockDim.x) cols.out[j][dst + r] = cols.in[j][src + r];
    }
}

// Workspace of fq_filter_project: [total][flag words: predicate,
// expressions][the ticket counter, a 128 B line][one look-back status word
// per tile].
struct ProjWs {
    uint64_t *total;
    uint32_t *flags, *ticket;
    uint64_t *status;
    int64_t ntiles;
};

// tile: the look-back tile's rows (0: the 64-bit kernels' over n_cols columns)
ProjWs proj_ws(void *d_ws, int64_t n, int n_cols = 1, int64_t tile = 0) {
    ProjWs w;
    if (tile <= 0) tile = select_tile_rows(n_cols);
    w.ntiles = (n + tile - 1) / tile;
    w.total = (uint64_t *)d_ws;
    w.flags = (uint32_t *)(w.total + 1);
    w.ticket = (uint32_t *)(w.total + 2);
    w.status = w.total + 2 + 16;
    return w;
}

fq_status flag_error(uint32_t f) {
    if (f & 0x80000000u) return fqc::fail(FQ_E_INTERNAL, "fused projection: the offset look-back did not complete");
    if (f & FQ_STATE_DIV_ZERO) return fqc::fail(FQ_E_DIVIDE_BY_ZERO, "Internal Error: Divide by zero error");
    if (f & FQ_STATE_CAST_NULL)
        return fqc::fail(FQ_E_UNSUPPORTED, "cast produced nulls (nulls are not supported on the device path)");
    return FQ_OK;
}

fq_status lower_projection(const fq_col *col, const fq_pred *pred, const fq_expr *values, int32_t n_out, void *const *d_out,
                           void *stream, ProjLaunch &P) {
    if (!col) return fqc::fail(FQ_E_INVALID, "fq_filter_project: NULL column");
    if (col->len > 0 && !col->data) return fqc::fail(FQ_E_INVALID, "fq_filter_project: NULL column data");
    if (fqc::dtype_size(col->dtype) != 8 || col->dtype == FQ_DT_BOOLEAN)
        return fqc::fail(FQ_E_UNSUPPORTED, "fused projection needs a 64-bit numeric column");
    if (n_out < 0 || n_out > FQ_MAX_PROJECT || (n_out > 0 && (!values || !d_out)))
        return fqc::fail(FQ_E_INVALID, "fq_filter_project: bad output list");
    P = ProjLaunch{};
    P.col = col->data;
    P.n = col->len;
    P.stream = (hipStream_t)stream;
    fq_status s = lower_pred(pred, col->dtype, col->len, true, P.pred);
    if (s != FQ_OK) return s;
    P.n_out = n_out;
    for (int j = 0; j < n_out; ++j) {
        if (!d_out[j] && col->len > 0) return fqc::fail(FQ_E_INVALID, "fq_filter_project: NULL output");
        int32_t dt = col->dtype;
        s = lower_expr(values[j], col->dtype, P.vals[j], dt);
        if (s != FQ_OK) return s;
        if (fqc::dtype_size(dt) != 8) return fqc::fail(FQ_E_UNSUPPORTED, "fused projection outputs are 64-bit");
        P.chain[j] = values[j].n_steps > 0;
        P.dtypes[j] = dt;
        P.out[j] = d_out[j];
    }
    return FQ_OK;
}

// The same for the *_columns entry points over n_cols >= 2 checked columns
// (one column goes through the single-column entry point): column references
// are read from the steps and checked, FQ_OP_LOAD is accepted.  need_data =
// false (fq_jit_prepare_project_columns): buffers may be NULL.
fq_status lower_projection_cols(const fq_col *cols, int32_t n_cols, const fq_pred *pred, const fq_expr *values,
                                int32_t n_out, void *const *d_out, void *stream, bool need_data, const char *who,
                                ProjLaunch &P) {
    if (n_out < 0 || n_out > FQ_MAX_PROJECT || (n_out > 0 && (!values || (need_data && !d_out))))
        return fqc::fail(FQ_E_INVALID, std::string(who) + ": bad output list");
    P = ProjLaunch{};
    P.col = cols[0].data;
    P.n = cols[0].len;
    P.stream = (hipStream_t)stream;
    P.n_cols = n_cols;
    for (int j = 0; j < n_cols; ++j) {
        P.cols[j] = cols[j].data;
        P.cdt[j] = cols[j].dtype;
    }
    fq_status s = lower_pred_cols(pred, P.cdt, n_cols, P.n, need_data, P.pred);
    if (s != FQ_OK) return s;
    P.n_out = n_out;
    for (int j = 0; j < n_out; ++j) {
        if (need_data && !d_out[j] && P.n > 0) return fqc::fail(FQ_E_INVALID, std::string(who) + ": NULL output");
        int32_t dt = P.cdt[0];
        s = lower_expr_cols(values[j], P.cdt, n_cols, P.vals[j], dt);
        if (s != FQ_OK) return s;
        P.chain[j] = values[j].n_steps > 0;
        P.dtypes[j] = dt;
        P.out[j] = d_out ? d_out[j] : nullptr;
    }
    return FQ_OK;
}

// the column references of a one-column program through a *_columns entry
// point (all must be 0)
fq_status check_one_col_refs(const fq_col *col, const fq_pred *pred, const fq_expr *values, int32_t n_out) {
    KProg kp;
    KPred kd;
    for (int j = 0; values && j < n_out && j < FQ_MAX_PROJECT; ++j) {
        int32_t dt = col->dtype;
        if (values[j].n_steps > 0) {
            fq_status s = lower_expr_cols(values[j], &col->dtype, 1, kp, dt);
            if (s != FQ_OK) return s;
        }
    }
    return lower_pred_cols(pred, &col->dtype, 1, col->len, false, kd);
}

// The load geometry of a typed launch (after its outputs are known).
void set_typed_geometry(ProjLaunch &P) {
    int wout = 1;
    for (int j = 0; j < P.n_out; ++j) wout = std::max(wout, fqc::dtype_size(P.dtypes[j]));
    typed_project_geometry(P.cdt, P.n_cols, wout, &P.rows, &P.group);
}

// every column, step, comparison and output type of a *_typed call is 64-bit:
// the call is its *_columns twin
bool project_call_is_64(const fq_col *cols, int32_t n_cols, const fq_pred *pred, const fq_expr *values, int32_t n_out) {
    if (!call_is_64(cols, n_cols, pred, nullptr)) return false;
    if (n_out < 0 || n_out > FQ_MAX_PROJECT || (n_out > 0 && !values)) return false;  // the typed lowering reports it
    for (int j = 0; j < n_out; ++j)
        if (!call_is_64(cols, n_cols, nullptr, &values[j]) ||
            (values[j].n_steps > 0 && fqc::dtype_size(values[j].out_dtype) != 8))
            return false;
    return true;
}

// lower_projection_cols for the *_typed entry points: n_cols >= 1 checked
// columns, steps, comparisons and outputs of any numeric type (each checked
// against the coercion of its operands), an output buffer aligned to its
// element.
fq_status lower_projection_typed(const fq_col *cols, int32_t n_cols, const fq_pred *pred, const fq_expr *values,
                                 int32_t n_out, void *const *d_out, void *stream, bool need_data, const char *who,
                                 ProjLaunch &P) {
    if (n_out < 0 || n_out > FQ_MAX_PROJECT || (n_out > 0 && (!values || (need_data && !d_out))))
        return fqc::fail(FQ_E_INVALID, std::string(who) + ": bad output list");
    P = ProjLaunch{};
    P.typed = true;
    P.col = cols[0].data;
    P.n = cols[0].len;
    P.stream = (hipStream_t)stream;
    P.n_cols = n_cols;
    for (int j = 0; j < n_cols; ++j) {
        P.cols[j] = cols[j].data;
        P.cdt[j] = cols[j].dtype;
    }
    fq_status s = lower_pred_typed(pred, P.cdt, n_cols, P.n, need_data, P.pred);
    if (s != FQ_OK) return s;
    P.n_out = n_out;
    for (int j = 0; j < n_out; ++j) {
        if (need_data && !d_out[j] && P.n > 0) return fqc::fail(FQ_E_INVALID, std::string(who) + ": NULL output");
        int32_t dt = P.cdt[0];
        s = lower_expr_typed(values[j], P.cdt, n_cols, P.vals[j], dt);
        if (s != FQ_OK) return s;
        P.chain[j] = values[j].n_steps > 0;
        P.dtypes[j] = dt;
        P.out[j] = d_out ? d_out[j] : nullptr;
        if (((uintptr_t)P.out[j]) % (uintptr_t)fqc::dtype_size(dt))
            return fqc::fail(FQ_E_INVALID, std::string(who) + ": output not aligned to its element size");
    }
    set_typed_geometry(P);
    return FQ_OK;
}

// fq_filter_project / fq_filter_project_columns after the lowering
fq_status filter_project_run(int32_t col_dtype, const ProjLaunch &P, int64_t *out_len, void *d_ws, size_t ws_bytes) {
    fq_status s;
    const std::string who = P.typed ? "fq_filter_project_typed" : P.n_cols > 1 ? "fq_filter_project_columns" : "fq_filter_project";
    if (!jit_project_available())
        return fqc::fail(FQ_E_UNSUPPORTED, who + ": hipRTC unavailable or the JIT is off");
    if ((s = jit_project_prepare(col_dtype, P)) != FQ_OK) return s;
    const int64_t n = P.n;
    if (n == 0) return FQ_OK;
    const ProjWs w = proj_ws(d_ws, n, P.n_cols, project_tile_rows(P));
    const size_t need = (size_t)(2 + 16 + w.ntiles) * sizeof(uint64_t);
    if (!d_ws || ws_bytes < need) return fqc::fail(FQ_E_INVALID, who + ": workspace too small");
    hipStream_t st = P.stream;
    uint64_t local[2] = {0, 0};
    uint64_t *const pinned = fqc::host_staging();
    uint64_t *const host = pinned ? pinned : local;  // kept rows, flag words
    host[0] = host[1] = 0;
    if (P.pred.kind == FQ_PRED_NONE) {
        FQ_HIP_TRY(hipMemsetAsync(w.flags, 0, 2 * sizeof(uint32_t), st));
        if ((s = jit_project_map(col_dtype, P, w.flags + 1)) != FQ_OK) return s;
        FQ_HIP_TRY(hipMemcpyAsync(&host[1], w.flags, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        host[0] = (uint64_t)n;
    } else {
        FQ_HIP_TRY(hipMemsetAsync(d_ws, 0, need, st));
        if ((s = jit_project_select(col_dtype, P, P.pred.kind == FQ_PRED_BITMAP ? P.pred.bitmap : nullptr, w.status,
                                    w.ticket, w.flags, w.total)) != FQ_OK)
            return s;
        FQ_HIP_TRY(hipMemcpyAsync(host, w.total, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));  // total + flag words
    }
    FQ_HIP_TRY(hipStreamSynchronize(st));
    const uint32_t pred_flags = (uint32_t)(host[1] & 0xffffffffu), val_flags = (uint32_t)(host[1] >> 32);
    if ((s = flag_error(pred_flags)) != FQ_OK) return s;  // FilterTransform runs first
    if ((s = flag_error(val_flags)) != FQ_OK) return s;
    *out_len = (int64_t)host[0];
    return FQ_OK;
}

// fq_predicate_bitmap / fq_predicate_bitmap_columns after the lowering
fq_status predicate_bitmap_run(int32_t col_dtype, ProjLaunch &P, uint64_t *d_bitmap, uint32_t *d_flag) {
    fq_status s;
    const std::string who = P.nullable ? "fq_predicate_bitmap_nullable"
                            : P.typed  ? "fq_predicate_bitmap_typed"
                                       : P.n_cols > 1 ? "fq_predicate_bitmap_columns" : "fq_predicate_bitmap";
    if (P.pred.kind != FQ_PRED_EXPR && P.pred.kind != FQ_PRED_TREE)
        return fqc::fail(FQ_E_INVALID, who + ": needs an FQ_PRED_EXPR or FQ_PRED_TREE predicate");
    if (!jit_project_available())
        return fqc::fail(FQ_E_UNSUPPORTED, who + ": hipRTC unavailable or the JIT is off");
    P.n_out = 1;  // the module's shape needs one output; the bits kernel writes none
    P.dtypes[0] = col_dtype;
    if (P.typed) set_typed_geometry(P);
    if ((s = jit_project_prepare(col_dtype, P)) != FQ_OK) return s;
    if (P.n == 0) return FQ_OK;
    if (!d_bitmap || !d_flag) return fqc::fail(FQ_E_INVALID, who + ": NULL buffer");
    FQ_HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(uint32_t), P.stream));
    if ((s = jit_project_bits(col_dtype, P, d_bitmap, d_flag)) != FQ_OK) return s;
    uint32_t local = 0;
    uint64_t *const pinned = fqc::host_staging();
    uint32_t *const h = pinned ? (uint32_t *)pinned : &local;
    FQ_HIP_TRY(hipMemcpyAsync(h, d_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, P.stream));
    FQ_HIP_TRY(hipStreamSynchronize(P.stream));
    return flag_error(*h);
}

}  // namespace
}  // namespace fqk

extern "C" {

size_t fq_filter_project_workspace_bytes(int64_t len) {
    const fqk::ProjWs w = fqk::proj_ws(nullptr, len < 0 ? 0 : len);
    return (size_t)(2 + 16 + w.ntiles) * sizeof(uint64_t);
}

size_t fq_filter_project_columns_workspace_bytes(int64_t len, int32_t n_cols) {
    const fqk::ProjWs w = fqk::proj_ws(nullptr, len < 0 ? 0 : len, n_cols);
    return (size_t)(2 + 16 + w.ntiles) * sizeof(uint64_t);
}

fq_status fq_filter_project(const fq_col *col, const fq_pred *pred, const fq_expr *values, int32_t n_out,
                            void *const *d_out, int64_t *out_len, void *d_ws, size_t ws_bytes, void *stream) {
    using namespace fqk;
    if (!out_len) return fqc::fail(FQ_E_INVALID, "fq_filter_project: NULL out_len");
    *out_len = 0;
    ProjLaunch P;
    fq_status s = lower_projection(col, pred, values, n_out, d_out, stream, P);
    if (s != FQ_OK) return s;
    if (n_out < 1) return fqc::fail(FQ_E_INVALID, "fq_filter_project: no outputs");
    return filter_project_run(col->dtype, P, out_len, d_ws, ws_bytes);
}

fq_status fq_filter_project_columns(const fq_col *cols, int32_t n_cols, const fq_pred *pred, const fq_expr *values,
                                    int32_t n_out, void *const *d_out, int64_t *out_len, void *d_ws, size_t ws_bytes,
                                    void *stream) {
    using namespace fqk;
    if (!out_len) return fqc::fail(FQ_E_INVALID, "fq_filter_project_columns: NULL out_len");
    *out_len = 0;
    fq_status s = check_cols(cols, n_cols, true, "fq_filter_project_columns");
    if (s != FQ_OK) return s;
    if (n_cols == 1) {
        if ((s = check_one_col_refs(cols, pred, values, n_out)) != FQ_OK) return s;
        return fq_filter_project(cols, pred, values, n_out, d_out, out_len, d_ws, ws_bytes, stream);
    }
    ProjLaunch P;
    s = lower_projection_cols(cols, n_cols, pred, values, n_out, d_out, stream, true, "fq_filter_project_columns", P);
    if (s != FQ_OK) return s;
    if (n_out < 1) return fqc::fail(FQ_E_INVALID, "fq_filter_project_columns: no outputs");
    return filter_project_run(cols[0].dtype, P, out_len, d_ws, ws_bytes);
}

size_t fq_filter_project_blocks_workspace_bytes(void) { return 3 * sizeof(uint64_t); }  // total, flags, ticket

}  // extern "C"

namespace fqk {

// a window of a frame-of-reference copy (fq_filter_project_blocks_for32): the
// encoded column's bases and the window's first row in it; the column passed
// beside it holds the deltas' own start and the window's length
struct For32Window {
    const uint64_t *base;
    int64_t first;
};

// typed: the call of fq_filter_project_blocks_typed with a narrow type in it (its columns checked)
// win: the call of fq_filter_project_blocks_for32 (one UInt64 column, its arguments checked)
static fq_status blocks_enqueue(bool typed, const fq_col *cols, int32_t n_cols, int64_t block_rows,
                                const fq_pred *pred, const fq_expr *values, int32_t n_out,
                                void *const *d_out, int64_t *d_counts, uint64_t *h_result,
                                uint64_t *d_result, void *d_ws, size_t ws_bytes, void *ev_start,
                                void *ev_end, void *stream, const For32Window *win = nullptr) {
    const std::string who = win     ? "fq_filter_project_blocks_for32"
                            : typed ? "fq_filter_project_blocks_typed"
                                    : n_cols > 1 ? "fq_filter_project_blocks_columns" : "fq_filter_project_blocks";
    static_assert(FQ_PROJECT_MIN_BLOCK_ROWS == kProjectBlockTile, "the ABI's minimum block is the kernel's tile");
    if (!h_result) return fqc::fail(FQ_E_INVALID, who + ": NULL result words");
    // a resident call's words are the caller's until the hand-off writes them
    // (the engine keeps a sentinel there to poll for)
    if (!d_result) h_result[0] = h_result[1] = 0;
    if (block_rows < FQ_PROJECT_MIN_BLOCK_ROWS)
        return fqc::fail(FQ_E_INVALID, who + ": block_rows below FQ_PROJECT_MIN_BLOCK_ROWS");
    ProjLaunch P;
    fq_status s;
    if (typed) {
        s = lower_projection_typed(cols, n_cols, pred, values, n_out, d_out, stream, true, who.c_str(), P);
    } else if (n_cols == 1) {
        s = lower_projection(cols, pred, values, n_out, d_out, stream, P);
    } else {
        if ((s = check_cols(cols, n_cols, true, "fq_filter_project_blocks_columns")) != FQ_OK) return s;
        s = lower_projection_cols(cols, n_cols, pred, values, n_out, d_out, stream, true,
                                  "fq_filter_project_blocks_columns", P);
    }
    if (s != FQ_OK) return s;
    const fq_col *col = cols;
    if (n_out < 1) return fqc::fail(FQ_E_INVALID, who + ": no outputs");
    if (win) {
        if (P.pred.kind == FQ_PRED_NONE)
            return fqc::fail(FQ_E_UNSUPPORTED, who + ": no predicate (the map kernel reads the plain column)");
        P.for32 = true;
        P.for32_base = win->base;
        P.for32_first = win->first;
    }
    if (!jit_project_available())
        return fqc::fail(FQ_E_UNSUPPORTED, who + ": hipRTC unavailable or the JIT is off");
    if ((s = jit_project_prepare(col->dtype, P)) != FQ_OK) return s;
    const int64_t n = col->len;
    if (n == 0) return FQ_OK;
    if (!d_counts) return fqc::fail(FQ_E_INVALID, who + ": NULL block counts");
    if (!d_ws || ws_bytes < fq_filter_project_blocks_workspace_bytes())
        return fqc::fail(FQ_E_INVALID, who + ": workspace too small");
    uint64_t *const total = (uint64_t *)d_ws;
    uint32_t *const flags = (uint32_t *)(total + 1);
    uint32_t *const ticket = (uint32_t *)(total + 2);
    hipStream_t st = P.stream;
    const int64_t nb = block_rows >= n ? 1 : (n + block_rows - 1) / block_rows;
    const bool resident = d_result != nullptr;
    if (!resident) FQ_HIP_TRY(hipMemsetAsync(d_ws, 0, fq_filter_project_blocks_workspace_bytes(), st));
    if (ev_start) FQ_HIP_TRY(hipEventRecord((hipEvent_t)ev_start, st));
    if (P.pred.kind == FQ_PRED_NONE) {  // every row kept: outputs in place, counts = block lengths
        if ((s = jit_project_map(col->dtype, P, flags + 1)) != FQ_OK) return s;
        hipLaunchKernelGGL(block_lengths_kernel, dim3((unsigned)std::min<int64_t>((nb + 255) / 256, 4096)), dim3(256), 0,
                           st, d_counts, nb, std::min(block_rows, n), n);
        FQ_HIP_TRY(hipGetLastError());
        if (ev_end) FQ_HIP_TRY(hipEventRecord((hipEvent_t)ev_end, st));
        FQ_HIP_TRY(hipMemcpyAsync(&h_result[1], flags, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        h_result[0] = (uint64_t)n;
        // the map kernel used the flag words: zero again for a resident workspace
        if (resident) FQ_HIP_TRY(hipMemsetAsync(d_ws, 0, fq_filter_project_blocks_workspace_bytes(), st));
        return FQ_OK;
    }
    if ((s = jit_project_blocks(col->dtype, P, block_rows, P.pred.kind == FQ_PRED_BITMAP ? P.pred.bitmap : nullptr,
                                d_counts, flags, total, ticket)) != FQ_OK)
        return s;
    if (ev_end) FQ_HIP_TRY(hipEventRecord((hipEvent_t)ev_end, st));
    if (resident) {
        hipLaunchKernelGGL(project_hand_off_kernel, dim3(1), dim3(64), 0, st, total, d_result);
        FQ_HIP_TRY(hipGetLastError());
    } else {
        FQ_HIP_TRY(hipMemcpyAsync(h_result, total, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    }
    return FQ_OK;
}

fq_status filter_project_blocks_enqueue_columns(const fq_col *cols, int32_t n_cols, int64_t block_rows,
                                                const fq_pred *pred, const fq_expr *values, int32_t n_out,
                                                void *const *d_out, int64_t *d_counts, uint64_t *h_result,
                                                uint64_t *d_result, void *d_ws, size_t ws_bytes, void *ev_start,
                                                void *ev_end, void *stream) {
    return blocks_enqueue(false, cols, n_cols, block_rows, pred, values, n_out, d_out, d_counts, h_result, d_result, d_ws,
                          ws_bytes, ev_start, ev_end, stream);
}

fq_status filter_project_blocks_enqueue_typed(const fq_col *cols, int32_t n_cols, int64_t block_rows,
                                              const fq_pred *pred, const fq_expr *values, int32_t n_out,
                                              void *const *d_out, int64_t *d_counts, uint64_t *h_result,
                                              uint64_t *d_result, void *d_ws, size_t ws_bytes, void *ev_start,
                                              void *ev_end, void *stream) {
    fq_status s = check_cols_typed(cols, n_cols, true, "fq_filter_project_blocks_typed");
    if (s != FQ_OK) {
        if (h_result && !d_result) h_result[0] = h_result[1] = 0;
        return s;
    }
    const bool typed = !project_call_is_64(cols, n_cols, pred, values, n_out);
    if (!typed && n_cols == 1 && (s = check_one_col_refs(cols, pred, values, n_out)) != FQ_OK) {
        if (h_result && !d_result) h_result[0] = h_result[1] = 0;
        return s;
    }
    return blocks_enqueue(typed, cols, n_cols, block_rows, pred, values, n_out, d_out, d_counts, h_result, d_result,
                          d_ws, ws_bytes, ev_start, ev_end, stream);
}

fq_status filter_project_blocks_enqueue(const fq_col *col, int64_t block_rows, const fq_pred *pred,
                                        const fq_expr *values, int32_t n_out, void *const *d_out, int64_t *d_counts,
                                        uint64_t *h_result, uint64_t *d_result, void *d_ws, size_t ws_bytes,
                                        void *ev_start, void *ev_end, void *stream) {
    return filter_project_blocks_enqueue_columns(col, 1, block_rows, pred, values, n_out, d_out, d_counts, h_result,
                                                 d_result, d_ws, ws_bytes, ev_start, ev_end, stream);
}

fq_status filter_project_blocks_enqueue_for32(const uint32_t *d_delta, const uint64_t *d_base, int64_t first,
                                              int64_t len, int64_t block_rows, const fq_pred *pred,
                                              const fq_expr *values, int32_t n_out, void *const *d_out,
                                              int64_t *d_counts, uint64_t *h_result, uint64_t *d_result, void *d_ws,
                                              size_t ws_bytes, void *ev_start, void *ev_end, void *stream) {
    if (!h_result) return fqc::fail(FQ_E_INVALID, "fq_filter_project_blocks_for32: NULL result words");
    const char *bad = first < 0                             ? "negative first row"
                      : len < 0                             ? "negative length"
                      : first > INT64_MAX - len             ? "first + len overflows"
                      : len > 0 && (!d_delta || !d_base)    ? "NULL deltas or bases"
                      : len > 0 && !d_counts                ? "NULL block counts"
                      : block_rows < FQ_PROJECT_MIN_BLOCK_ROWS ? "block_rows below FQ_PROJECT_MIN_BLOCK_ROWS"
                                                            : nullptr;
    if (bad) {
        if (h_result && !d_result) h_result[0] = h_result[1] = 0;
        return fqc::fail(FQ_E_INVALID, std::string("fq_filter_project_blocks_for32: ") + bad);
    }
    if (((uintptr_t)d_delta & 3u) || ((uintptr_t)d_base & 7u)) {
        if (h_result && !d_result) h_result[0] = h_result[1] = 0;
        return fqc::fail(FQ_E_INVALID, "fq_filter_project_blocks_for32: deltas or bases not aligned to their element");
    }
    const fq_col col{(void *)d_delta, len, FQ_DT_UINT64, 0};  // the deltas' start; the rows are UInt64
    const For32Window win{d_base, first};
    return blocks_enqueue(false, &col, 1, block_rows, pred, values, n_out, d_out, d_counts, h_result, d_result, d_ws,
                          ws_bytes, ev_start, ev_end, stream, &win);
}

bool typed_project_fits(const int32_t *cdt, int32_t n_cols, const fq_pred *pred, const fq_expr *values, int32_t n_out) {
    if (!cdt || n_cols < 1 || n_cols > FQ_MAX_SCAN_COLS || n_out < 0 || n_out > FQ_MAX_PROJECT || (n_out > 0 && !values))
        return false;
    KProg val;
    KPred kp;
    for (int j = 0; j < n_out; ++j) {
        int32_t dt = cdt[0];
        if (lower_expr_typed(values[j], cdt, n_cols, val, dt) != FQ_OK) return false;
    }
    return lower_pred_typed(pred, cdt, n_cols, 0, false, kp) == FQ_OK;
}

fq_status filter_project_blocks_result(const uint64_t *h_result, int64_t *out_len) {
    if (!h_result || !out_len) return fqc::fail(FQ_E_INVALID, "fq_filter_project_blocks: NULL result");
    *out_len = 0;
    const uint32_t pred_flags = (uint32_t)(h_result[1] & 0xffffffffu), val_flags = (uint32_t)(h_result[1] >> 32);
    fq_status s;
    if ((s = flag_error(pred_flags)) != FQ_OK) return s;  // FilterTransform runs first
    if ((s = flag_error(val_flags)) != FQ_OK) return s;
    *out_len = (int64_t)h_result[0];
    return FQ_OK;
}

}  // namespace fqk

extern "C" {

fq_status fq_filter_project_blocks(const fq_col *col, int64_t block_rows, const fq_pred *pred, const fq_expr *values,
                                   int32_t n_out, void *const *d_out, int64_t *d_counts, int64_t *out_len, void *d_ws,
                                   size_t ws_bytes, void *stream) {
    if (!out_len) return fqc::fail(FQ_E_INVALID, "fq_filter_project_blocks: NULL out_len");
    *out_len = 0;
    uint64_t local[2] = {0, 0};
    uint64_t *const pinned = fqc::host_staging();
    uint64_t *const host = pinned ? pinned : local;  // kept rows, flag words
    fq_status s = fqk::filter_project_blocks_enqueue(col, block_rows, pred, values, n_out, d_out, d_counts, host,
                                                     nullptr, d_ws, ws_bytes, nullptr, nullptr, stream);
    if (s != FQ_OK) return s;
    FQ_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return fqk::filter_project_blocks_result(host, out_len);
}

fq_status fq_filter_project_blocks_columns(const fq_col *cols, int32_t n_cols, int64_t block_rows, const fq_pred *pred,
                                           const fq_expr *values, int32_t n_out, void *const *d_out,
                                           int64_t *d_counts, int64_t *out_len, void *d_ws, size_t ws_bytes,
                                           void *stream) {
    using namespace fqk;
    if (!out_len) return fqc::fail(FQ_E_INVALID, "fq_filter_project_blocks_columns: NULL out_len");
    *out_len = 0;
    fq_status s = check_cols(cols, n_cols, true, "fq_filter_project_blocks_columns");
    if (s != FQ_OK) return s;
    if (n_cols == 1) {
        if ((s = check_one_col_refs(cols, pred, values, n_out)) != FQ_OK) return s;
        return fq_filter_project_blocks(cols, block_rows, pred, values, n_out, d_out, d_counts, out_len, d_ws, ws_bytes,
                                        stream);
    }
    uint64_t local[2] = {0, 0};
    uint64_t *const pinned = fqc::host_staging();
    uint64_t *const host = pinned ? pinned : local;  // kept rows, flag words
    s = filter_project_blocks_enqueue_columns(cols, n_cols, block_rows, pred, values, n_out, d_out, d_counts, host,
                                              nullptr, d_ws, ws_bytes, nullptr, nullptr, stream);
    if (s != FQ_OK) return s;
    FQ_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return filter_project_blocks_result(host, out_len);
}

fq_status fq_filter_project_blocks_for32(const uint32_t *d_delta, const uint64_t *d_base, int64_t first, int64_t len,
                                         int64_t block_rows, const fq_pred *pred, const fq_expr *values, int32_t n_out,
                                         void *const *d_out, int64_t *d_counts, int64_t *out_len, void *d_ws,
                                         size_t ws_bytes, void *stream) {
    if (!out_len) return fqc::fail(FQ_E_INVALID, "fq_filter_project_blocks_for32: NULL out_len");
    *out_len = 0;
    uint64_t local[2] = {0, 0};
    uint64_t *const pinned = fqc::host_staging();
    uint64_t *const host = pinned ? pinned : local;  // kept rows, flag words
    fq_status s = fqk::filter_project_blocks_enqueue_for32(d_delta, d_base, first, len, block_rows, pred, values, n_out,
                                                           d_out, d_counts, host, nullptr, d_ws, ws_bytes, nullptr,
                                                           nullptr, stream);
    if (s != FQ_OK) return s;
    FQ_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return fqk::filter_project_blocks_result(host, out_len);
}

fq_status fq_jit_prepare_project_for32(int64_t block_rows, const fq_pred *pred, const fq_expr *values, int32_t n_out,
                                       int32_t *specialised) {
    using namespace fqk;
    if (specialised) *specialised = 0;
    if (block_rows < FQ_PROJECT_MIN_BLOCK_ROWS)
        return fqc::fail(FQ_E_INVALID, "fq_jit_prepare_project_for32: block_rows below FQ_PROJECT_MIN_BLOCK_ROWS");
    if (n_out < 1 || n_out > FQ_MAX_PROJECT)
        return fqc::fail(FQ_E_INVALID, "fq_jit_prepare_project_for32: n_out must be 1.." + std::to_string(FQ_MAX_PROJECT) +
                                           ", got " + std::to_string(n_out));
    const fq_col c0{nullptr, 0, FQ_DT_UINT64, 0};  // the shape only: no buffers needed
    void *none[FQ_MAX_PROJECT] = {};
    ProjLaunch P;
    fq_status s = lower_projection(&c0, pred, values, n_out, none, nullptr, P);
    if (s != FQ_OK) return s;
    if (P.pred.kind == FQ_PRED_NONE)
        return fqc::fail(FQ_E_UNSUPPORTED, "fq_jit_prepare_project_for32: no predicate (the map kernel reads the plain column)");
    if (!jit_project_available()) return FQ_OK;  // the caller's plain path answers
    P.for32 = true;
    if ((s = jit_project_prepare(FQ_DT_UINT64, P)) != FQ_OK) return s;
    if (specialised) *specialised = 1;
    return FQ_OK;
}

size_t fq_blocks_compact_workspace_bytes(int64_t n_blocks) {
    const int64_t nb = n_blocks < 1 ? 1 : n_blocks;
    const int64_t chunks = (nb + fqk::kCompactChunk - 1) / fqk::kCompactChunk;
    return (size_t)(nb + 1 + chunks + 1) * sizeof(int64_t);
}

fq_status fq_blocks_compact(int32_t n_cols, const void *const *d_in, int64_t len, int64_t block_rows,
                            const int64_t *d_counts, void *const *d_out, int64_t *out_len, void *d_ws, size_t ws_bytes,
                            void *stream) {
    using namespace fqk;
    if (out_len) *out_len = 0;
    if (n_cols < 0 || n_cols > FQ_MAX_PROJECT || (n_cols > 0 && (!d_in || !d_out)))
        return fqc::fail(FQ_E_INVALID, "fq_blocks_compact: bad column list");
    if (len < 0 || block_rows < 1) return fqc::fail(FQ_E_INVALID, "fq_blocks_compact: bad geometry");
    if (len == 0) return FQ_OK;
    const int64_t nb = (len + block_rows - 1) / block_rows;
    if (!d_counts || !d_ws) return fqc::fail(FQ_E_INVALID, "fq_blocks_compact: NULL buffer");
    if (ws_bytes < fq_blocks_compact_workspace_bytes(nb))
        return fqc::fail(FQ_E_INVALID, "fq_blocks_compact: workspace too small");
    CompactCols cols{};
    for (int j = 0; j < n_cols; ++j) {
        if (!d_in[j] || !d_out[j]) return fqc::fail(FQ_E_INVALID, "fq_blocks_compact: NULL column");
        cols.in[j] = (const uint64_t *)d_in[j];
        cols.out[j] = (uint64_t *)d_out[j];
    }
    hipStream_t st = (hipStream_t)stream;
    int64_t *const offs = (int64_t *)d_ws;  // nb + 1
    int64_t *const sums = offs + nb + 1;    // chunks + 1
    const int64_t chunks = (nb + kCompactChunk - 1) / kCompactChunk;
    hipLaunchKernelGGL(blocks_chunk_sums_kernel, dim3((unsigned)chunks), dim3(kCompactChunk), 0, st, d_counts, nb, sums);
    FQ_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(blocks_scan_sums_kernel, dim3(1), dim3(kCompactChunk), 0, st, sums, chunks);
    FQ_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(blocks_offsets_kernel, dim3((unsigned)chunks), dim3(kCompactChunk), 0, st, d_counts, nb, sums,
                       offs);
    FQ_HIP_TRY(hipGetLastError());
    if (n_cols > 0) {
        hipLaunchKernelGGL(blocks_copy_kernel, dim3((unsigned)std::min<int64_t>(nb, 1 << 20)), dim3(256), 0, st, cols,
                           n_cols, d_counts, offs, nb, block_rows);
        FQ_HIP_TRY(hipGetLastError());
    }
    if (!out_len) return FQ_OK;
    uint64_t local = 0;
    uint64_t *const pinned = fqc::host_staging();
    uint64_t *const total = pinned ? pinned : &local;
    FQ_HIP_TRY(hipMemcpyAsync(total, offs + nb, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    FQ_HIP_TRY(hipStreamSynchronize(st));
    *out_len = (int64_t)*total;
    return FQ_OK;
}

fq_status fq_predicate_bitmap(const fq_col *col, const fq_pred *pred, uint64_t *d_bitmap, uint32_t *d_flag,
                              void *stream) {
    using namespace fqk;
    ProjLaunch P;
    fq_status s = lower_projection(col, pred, nullptr, 0, nullptr, stream, P);
    if (s != FQ_OK) return s;
    return predicate_bitmap_run(col->dtype, P, d_bitmap, d_flag);
}

fq_status fq_predicate_bitmap_columns(const fq_col *cols, int32_t n_cols, const fq_pred *pred, uint64_t *d_bitmap,
                                      uint32_t *d_flag, void *stream) {
    using namespace fqk;
    fq_status s = check_cols(cols, n_cols, true, "fq_predicate_bitmap_columns");
    if (s != FQ_OK) return s;
    if (n_cols == 1) {
        if ((s = check_one_col_refs(cols, pred, nullptr, 0)) != FQ_OK) return s;
        return fq_predicate_bitmap(cols, pred, d_bitmap, d_flag, stream);
    }
    ProjLaunch P;
    s = lower_projection_cols(cols, n_cols, pred, nullptr, 0, nullptr, stream, true, "fq_predicate_bitmap_columns", P);
    if (s != FQ_OK) return s;
    return predicate_bitmap_run(cols[0].dtype, P, d_bitmap, d_flag);
}

fq_status fq_jit_prepare_project_columns(const fq_col *cols, int32_t n_cols, int64_t block_rows, const fq_pred *pred,
                                         const fq_expr *values, int32_t n_out, int32_t *specialised) {
    using namespace fqk;
    if (specialised) *specialised = 0;
    fq_status s = check_cols(cols, n_cols, false, "fq_jit_prepare_project_columns");
    if (s != FQ_OK) return s;
    if (block_rows != 0 && block_rows < FQ_PROJECT_MIN_BLOCK_ROWS)
        return fqc::fail(FQ_E_INVALID, "fq_jit_prepare_project_columns: block_rows below FQ_PROJECT_MIN_BLOCK_ROWS");
    if (n_out < 1 || n_out > FQ_MAX_PROJECT)
        return fqc::fail(FQ_E_INVALID, "fq_jit_prepare_project_columns: n_out must be 1.." +
                                           std::to_string(FQ_MAX_PROJECT) + ", got " + std::to_string(n_out));
    // one column: the single-column module (column references all 0, ignored by its lowering)
    ProjLaunch P;
    if (n_cols == 1) {
        if ((s = check_one_col_refs(cols, pred, values, n_out)) != FQ_OK) return s;
        fq_col c0 = cols[0];
        void *none[FQ_MAX_PROJECT] = {};
        c0.len = 0;  // the shape only: no buffers needed
        s = lower_projection(&c0, pred, values, n_out, none, nullptr, P);
    } else {
        s = lower_projection_cols(cols, n_cols, pred, values, n_out, nullptr, nullptr, false,
                                  "fq_jit_prepare_project_columns", P);
    }
    if (s != FQ_OK) return s;
    if (!jit_project_available()) return FQ_OK;  // the caller's unfused path answers
    if ((s = jit_project_prepare(cols[0].dtype, P)) != FQ_OK) return s;
    if (specialised) *specialised = 1;
    return FQ_OK;
}

size_t fq_filter_project_typed_workspace_bytes(int64_t len, const fq_col *cols, int32_t n_cols) {
    if (len < 0) len = 0;
    // enough for the 64-bit twin and for the typed tile of these columns with an 8-byte output (the smallest)
    size_t need = fq_filter_project_columns_workspace_bytes(len, n_cols);
    if (cols && n_cols >= 1 && n_cols <= FQ_MAX_SCAN_COLS) {
        int32_t cdt[FQ_MAX_SCAN_COLS];
        for (int j = 0; j < n_cols; ++j) cdt[j] = fqc::dtype_is_numeric(cols[j].dtype) ? cols[j].dtype : FQ_DT_UINT64;
        int rows = 0, group = 0;
        fqk::typed_project_geometry(cdt, n_cols, 8, &rows, &group);
        const fqk::ProjWs w = fqk::proj_ws(nullptr, len, n_cols, (int64_t)fqk::select_threads() * rows);
        need = std::max(need, (size_t)(2 + 16 + w.ntiles) * sizeof(uint64_t));
    }
    return need;
}

fq_status fq_filter_project_typed(const fq_col *cols, int32_t n_cols, const fq_pred *pred, const fq_expr *values,
                                  int32_t n_out, void *const *d_out, int64_t *out_len, void *d_ws, size_t ws_bytes,
                                  void *stream) {
    using namespace fqk;
    if (!out_len) return fqc::fail(FQ_E_INVALID, "fq_filter_project_typed: NULL out_len");
    *out_len = 0;
    fq_status s = check_cols_typed(cols, n_cols, true, "fq_filter_project_typed");
    if (s != FQ_OK) return s;
    if (project_call_is_64(cols, n_cols, pred, values, n_out))
        return fq_filter_project_columns(cols, n_cols, pred, values, n_out, d_out, out_len, d_ws, ws_bytes, stream);
    ProjLaunch P;
    s = lower_projection_typed(cols, n_cols, pred, values, n_out, d_out, stream, true, "fq_filter_project_typed", P);
    if (s != FQ_OK) return s;
    if (n_out < 1) return fqc::fail(FQ_E_INVALID, "fq_filter_project_typed: no outputs");
    return filter_project_run(cols[0].dtype, P, out_len, d_ws, ws_bytes);
}

fq_status fq_filter_project_blocks_typed(const fq_col *cols, int32_t n_cols, int64_t block_rows, const fq_pred *pred,
                                         const fq_expr *values, int32_t n_out, void *const *d_out, int64_t *d_counts,
                                         int64_t *out_len, void *d_ws, size_t ws_bytes, void *stream) {
    using namespace fqk;
    if (!out_len) return fqc::fail(FQ_E_INVALID, "fq_filter_project_blocks_typed: NULL out_len");
    *out_len = 0;
    fq_status s = check_cols_typed(cols, n_cols, true, "fq_filter_project_blocks_typed");
    if (s != FQ_OK) return s;
    if (project_call_is_64(cols, n_cols, pred, values, n_out))
        return fq_filter_project_blocks_columns(cols, n_cols, block_rows, pred, values, n_out, d_out, d_counts, out_len,
                                                d_ws, ws_bytes, stream);
    uint64_t local[2] = {0, 0};
    uint64_t *const pinned = fqc::host_staging();
    uint64_t *const host = pinned ? pinned : local;  // kept rows, flag words
    s = filter_project_blocks_enqueue_typed(cols, n_cols, block_rows, pred, values, n_out, d_out, d_counts, host, nullptr,
                                            d_ws, ws_bytes, nullptr, nullptr, stream);
    if (s != FQ_OK) return s;
    FQ_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return filter_project_blocks_result(host, out_len);
}

fq_status fq_predicate_bitmap_typed(const fq_col *cols, int32_t n_cols, const fq_pred *pred, uint64_t *d_bitmap,
                                    uint32_t *d_flag, void *stream) {
    using namespace fqk;
    fq_status s = check_cols_typed(cols, n_cols, true, "fq_predicate_bitmap_typed");
    if (s != FQ_OK) return s;
    if (call_is_64(cols, n_cols, pred, nullptr))
        return fq_predicate_bitmap_columns(cols, n_cols, pred, d_bitmap, d_flag, stream);
    ProjLaunch P;
    s = lower_projection_typed(cols, n_cols, pred, nullptr, 0, nullptr, stream, true, "fq_predicate_bitmap_typed", P);
    if (s != FQ_OK) return s;
    return predicate_bitmap_run(cols[0].dtype, P, d_bitmap, d_flag);
}

fq_status fq_jit_prepare_project_typed(const fq_col *cols, int32_t n_cols, int64_t block_rows, const fq_pred *pred,
                                       const fq_expr *values, int32_t n_out, int32_t *specialised) {
    using namespace fqk;
    if (specialised) *specialised = 0;
    fq_status s = check_cols_typed(cols, n_cols, false, "fq_jit_prepare_project_typed");
    if (s != FQ_OK) return s;
    if (project_call_is_64(cols, n_cols, pred, values, n_out))
        return fq_jit_prepare_project_columns(cols, n_cols, block_rows, pred, values, n_out, specialised);
    if (block_rows != 0 && block_rows < FQ_PROJECT_MIN_BLOCK_ROWS)
        return fqc::fail(FQ_E_INVALID, "fq_jit_prepare_project_typed: block_rows below FQ_PROJECT_MIN_BLOCK_ROWS");
    if (n_out < 1 || n_out > FQ_MAX_PROJECT)
        return fqc::fail(FQ_E_INVALID, "fq_jit_prepare_project_typed: n_out must be 1.." +
                                           std::to_string(FQ_MAX_PROJECT) + ", got " + std::to_string(n_out));
    ProjLaunch P;
    s = lower_projection_typed(cols, n_cols, pred, values, n_out, nullptr, nullptr, false,
                               "fq_jit_prepare_project_typed", P);
    if (s != FQ_OK) return s;
    if (!jit_project_available()) return FQ_OK;  // the caller's unfused path answers
    if ((s = jit_project_prepare(cols[0].dtype, P)) != FQ_OK) return s;
    if (specialised) *specialised = 1;
    return FQ_OK;
}

}  // extern "C"

namespace fqk {
namespace {

// The validity arguments of the *_nullable projection entry points: the array itself non-NULL, each entry NULL or
// 8-byte aligned.  Marks P (lowered by lower_projection_typed) nullable: every shape runs the typed kernels.
fq_status set_nullable(const uint64_t *const *validity, const uint8_t *has_validity, int32_t n_cols, const std::string &who,
                       ProjLaunch &P) {
    P.nullable = true;
    for (int j = 0; j < n_cols; ++j) {
        if (validity && ((uintptr_t)validity[j]) % 8)
            return fqc::fail(FQ_E_INVALID, who + ": validity bitmap " + std::to_string(j) + " not aligned to 8 bytes");
        P.validity[j] = validity ? validity[j] : nullptr;
        P.has_bm[j] = validity ? validity[j] != nullptr : (has_validity && has_validity[j]);
    }
    return FQ_OK;
}

const char *const kNullableNeedsJit = ": hipRTC unavailable or the JIT is off (there is no unfused path over nulls)";

}  // namespace
}  // namespace fqk

extern "C" {

fq_status fq_filter_project_blocks_nullable(const fq_col *cols, const uint64_t *const *validity, int32_t n_cols,
                                            int64_t block_rows, const fq_pred *pred, const fq_expr *values,
                                            int32_t n_out, void *const *d_out, uint64_t *const *d_out_validity,
                                            int64_t *d_counts, int64_t *out_len, void *d_ws, size_t ws_bytes,
                                            void *stream) {
    using namespace fqk;
    const std::string who = "fq_filter_project_blocks_nullable";
    if (!out_len) return fqc::fail(FQ_E_INVALID, who + ": NULL out_len");
    *out_len = 0;
    fq_status s = check_cols_typed(cols, n_cols, true, who.c_str());
    if (s != FQ_OK) return s;
    if (!validity) return fqc::fail(FQ_E_INVALID, who + ": NULL validity array");
    if (block_rows < FQ_PROJECT_MIN_BLOCK_ROWS)
        return fqc::fail(FQ_E_INVALID, who + ": block_rows below FQ_PROJECT_MIN_BLOCK_ROWS");
    ProjLaunch P;
    s = lower_projection_typed(cols, n_cols, pred, values, n_out, d_out, stream, true, who.c_str(), P);
    if (s != FQ_OK) return s;
    if (n_out < 1) return fqc::fail(FQ_E_INVALID, who + ": no outputs");
    if ((s = set_nullable(validity, nullptr, n_cols, who, P)) != FQ_OK) return s;
    if (!d_out_validity) return fqc::fail(FQ_E_INVALID, who + ": NULL output validity array");
    for (int j = 0; j < n_out; ++j) {
        P.out_validity[j] = d_out_validity[j];
        if (((uintptr_t)d_out_validity[j]) % 8)
            return fqc::fail(FQ_E_INVALID, who + ": output validity bitmap " + std::to_string(j) + " not aligned to 8 bytes");
        if (!d_out_validity[j] && project_output_nullable(P, j))
            return fqc::fail(FQ_E_INVALID, who + ": NULL validity bitmap of output " + std::to_string(j) + ", which can hold nulls");
    }
    if (!jit_project_available()) return fqc::fail(FQ_E_UNSUPPORTED, who + kNullableNeedsJit);
    if ((s = jit_project_prepare(cols[0].dtype, P)) != FQ_OK) return s;
    const int64_t n = cols[0].len;
    if (n == 0) return FQ_OK;
    if (!d_counts) return fqc::fail(FQ_E_INVALID, who + ": NULL block counts");
    if (!d_ws || ws_bytes < fq_filter_project_blocks_workspace_bytes())
        return fqc::fail(FQ_E_INVALID, who + ": workspace too small");
    uint64_t *const total = (uint64_t *)d_ws;
    uint32_t *const flags = (uint32_t *)(total + 1);
    uint32_t *const ticket = (uint32_t *)(total + 2);
    hipStream_t st = P.stream;
    FQ_HIP_TRY(hipMemsetAsync(d_ws, 0, fq_filter_project_blocks_workspace_bytes(), st));
    // the kernel ORs the kept rows' bits into zeroed words
    for (int j = 0; j < n_out; ++j)
        if (P.out_validity[j]) FQ_HIP_TRY(hipMemsetAsync(P.out_validity[j], 0, (size_t)((n + 63) / 64) * 8, st));
    // FQ_PRED_NONE keeps every row through the block kernel too (the module has no map kernel)
    if ((s = jit_project_blocks(cols[0].dtype, P, block_rows, P.pred.kind == FQ_PRED_BITMAP ? P.pred.bitmap : nullptr,
                                d_counts, flags, total, ticket)) != FQ_OK)
        return s;
    uint64_t local[2] = {0, 0};
    uint64_t *const pinned = fqc::host_staging();
    uint64_t *const host = pinned ? pinned : local;  // kept rows, flag words
    FQ_HIP_TRY(hipMemcpyAsync(host, total, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    FQ_HIP_TRY(hipStreamSynchronize(st));
    return filter_project_blocks_result(host, out_len);
}

fq_status fq_predicate_bitmap_nullable(const fq_col *cols, const uint64_t *const *validity, int32_t n_cols,
                                       const fq_pred *pred, uint64_t *d_bitmap, uint32_t *d_flag, void *stream) {
    using namespace fqk;
    const std::string who = "fq_predicate_bitmap_nullable";
    fq_status s = check_cols_typed(cols, n_cols, true, who.c_str());
    if (s != FQ_OK) return s;
    if (!validity) return fqc::fail(FQ_E_INVALID, who + ": NULL validity array");
    ProjLaunch P;
    s = lower_projection_typed(cols, n_cols, pred, nullptr, 0, nullptr, stream, true, who.c_str(), P);
    if (s != FQ_OK) return s;
    if ((s = set_nullable(validity, nullptr, n_cols, who, P)) != FQ_OK) return s;
    if (!jit_project_available()) return fqc::fail(FQ_E_UNSUPPORTED, who + kNullableNeedsJit);
    return predicate_bitmap_run(cols[0].dtype, P, d_bitmap, d_flag);
}

fq_status fq_jit_prepare_project_nullable(const fq_col *cols, const uint8_t *has_validity, int32_t n_cols,
                                          int64_t block_rows, const fq_pred *pred, const fq_expr *values, int32_t n_out,
                                          int32_t *specialised) {
    using namespace fqk;
    const std::string who = "fq_jit_prepare_project_nullable";
    if (specialised) *specialised = 0;
    fq_status s = check_cols_typed(cols, n_cols, false, who.c_str());
    if (s != FQ_OK) return s;
    if (block_rows < FQ_PROJECT_MIN_BLOCK_ROWS)
        return fqc::fail(FQ_E_INVALID, who + ": block_rows below FQ_PROJECT_MIN_BLOCK_ROWS (the contiguous form is not built)");
    if (n_out < 1 || n_out > FQ_MAX_PROJECT)
        return fqc::fail(FQ_E_INVALID, who + ": n_out must be 1.." + std::to_string(FQ_MAX_PROJECT) + ", got " +
                                           std::to_string(n_out));
    ProjLaunch P;
    s = lower_projection_typed(cols, n_cols, pred, values, n_out, nullptr, nullptr, false, who.c_str(), P);
    if (s != FQ_OK) return s;
    (void)set_nullable(nullptr, has_validity, n_cols, who, P);
    if (!jit_project_available()) return fqc::fail(FQ_E_UNSUPPORTED, who + kNullableNeedsJit);
    if ((s = jit_project_prepare(cols[0].dtype, P)) != FQ_OK) return s;
    if (specialised) *specialised = 1;
    return FQ_OK;
}

fq_status fq_filter_compact(const fq_col *in, const uint64_t *d_bitmap, void *d_out, int64_t *out_len,
                            void *d_ws, size_t ws_bytes, void *stream) {
    using namespace fqk;
    if (!in || !out_len) return fqc::fail(FQ_E_INVALID, "fq_filter_compact: NULL argument");
    const int64_t n = in->len;
    *out_len = 0;
    if (n == 0) return FQ_OK;
    if (!in->data || !d_bitmap || !d_out || !d_ws)
        return fqc::fail(FQ_E_INVALID, "fq_filter_compact: NULL buffer");
    if (ws_bytes < fq_filter_workspace_bytes(n))
        return fqc::fail(FQ_E_INVALID, "fq_filter_compact: workspace too small");
    const int esz = in->dtype == FQ_DT_BOOLEAN ? 0 : fqc::dtype_size(in->dtype);
    if (esz == 0) return fqc::fail(FQ_E_UNSUPPORTED, "fq_filter_compact: column type not supported");
    hipStream_t st = (hipStream_t)stream;
    const int64_t nwords = (n + 63) / 64;
    const int64_t ntiles = (nwords + kTileWords - 1) / kTileWords;
    const int64_t ngroups = (ntiles + kGroupTiles - 1) / kGroupTiles;
    uint64_t *intra = (uint64_t *)d_ws;
    uint64_t *gpre = intra + ntiles;
    hipLaunchKernelGGL(compact_count_kernel, dim3((unsigned)ngroups), dim3(kTileWords), 0, st, d_bitmap, n, ntiles,
                       intra, gpre);
    FQ_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, gpre, ngroups);
    FQ_HIP_TRY(hipGetLastError());
    switch (esz) {
        case 1:
            hipLaunchKernelGGL(compact_scatter_kernel<uint8_t>, dim3((unsigned)ntiles), dim3(kTileWords), 0, st,
                               (const uint8_t *)in->data, d_bitmap, n, intra, gpre, (uint8_t *)d_out);
            break;
        case 2:
            hipLaunchKernelGGL(compact_scatter_kernel<uint16_t>, dim3((unsigned)ntiles), dim3(kTileWords), 0, st,
                               (const uint16_t *)in->data, d_bitmap, n, intra, gpre, (uint16_t *)d_out);
            break;
        case 4:
            hipLaunchKernelGGL(compact_scatter_kernel<uint32_t>, dim3((unsigned)ntiles), dim3(kTileWords), 0, st,
                               (const uint32_t *)in->data, d_bitmap, n, intra, gpre, (uint32_t *)d_out);
            break;
        default:
            if (((uintptr_t)in->data & 15u) == 0 && ((uintptr_t)d_out & 15u) == 0)
                hipLaunchKernelGGL(compact_scatter_lds_kernel<uint64_t>, dim3((unsigned)ntiles), dim3(kTileWords), 0,
                                   st, (const uint64_t *)in->data, d_bitmap, n, intra, gpre, (uint64_t *)d_out);
            else if (((uintptr_t)in->data & 15u) == 0)
                hipLaunchKernelGGL(compact_scatter_vec_kernel<uint64_t>, dim3((unsigned)ntiles), dim3(kTileWords), 0,
                                   st, (const uint64_t *)in->data, d_bitmap, n, intra, gpre, (uint64_t *)d_out);
            else
                hipLaunchKernelGGL(compact_scatter_kernel<uint64_t>, dim3((unsigned)ntiles), dim3(kTileWords), 0,
                                   st, (const uint64_t *)in->data, d_bitmap, n, intra, gpre, (uint64_t *)d_out);
            break;
    }
    FQ_HIP_TRY(hipGetLastError());
    uint64_t local = 0;
    uint64_t *const pinned = fqc::host_staging();
    uint64_t *const total = pinned ? pinned : &local;
    FQ_HIP_TRY(hipMemcpyAsync(total, gpre + ngroups, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    FQ_HIP_TRY(hipStreamSynchronize(st));
    *out_len = (int64_t)*total;
    return FQ_OK;
}

}  // extern "C"
