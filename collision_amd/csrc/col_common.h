// Shared device/host helpers for libcollision_hip.so (gfx950 only: 64-lane waves).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/collision_hip.h"
#include "../../include/collision_hip_debug.h"

#define COL_WAVE 64

#define COL_HIP(expr)                                  \
    do {                                               \
        hipError_t e_ = (expr);                        \
        if (e_ != hipSuccess) return (int)e_;          \
    } while (0)

// launch check: hipGetLastError after a <<<>>> launch
#define COL_LAUNCH_OK()                                \
    do {                                               \
        hipError_t e_ = hipGetLastError();             \
        if (e_ != hipSuccess) return (int)e_;          \
    } while (0)

// ---- constants shared between translation units ----
#define COL_MINMAX_PARTS 256    // col_minmax4_stage1_zero / _dev leave at most this many partial results
// col_radix_sort_msd: one workgroup finishes one of 256 top-digit buckets in LDS -- 8192 pairs per bucket for
// inputs up to COL_MSD_SMALL_N codes, 16384 up to COL_MSD_MAX_N (uniform scenes: n / 256 per bucket +- 4 sigma)
#define COL_MSD_SMALL_N 1900000u
#define COL_MSD_MAX_N 4050000u
// the Morton kernel's tile under the MSD plan that gathers its buckets from sorted tiles (col_radix_sort_msd_gather): 4096
// codes from COL_GATHER_BIG_FROM codes on (pieces of ~16 pairs instead of ~4: a 128-byte line of a sorted tile then serves
// two or three buckets instead of eight), 1024 below, where 4096-code tiles would leave CUs idle
#define COL_GATHER_BIG_FROM (768u << 10)
#define COL_MSD_GROUP 32u       // tiles per group sum of the fused MSD pass (radix.hip: MSD_GROUP)
#define COL_MSD_GROUPS 32u      // group sums per digit: the fused pass takes at most COL_MSD_GROUP * COL_MSD_GROUPS tiles
#define COL_REGION_BOXES 8      // boxes per rank region on the multi-GPU path (multi.hip: k_region)

// ---- internal entry points, one block per defining file (hidden: not part of the public headers) ----
// DEVICE-SIDE COUNT (round 4, the multi-GPU step): `n_dev` (may be NULL) points at a device word that holds the real number
// of spheres; `n` is then a host-known upper bound that sizes grids and scratch, and every kernel works on min(n, *n_dev).
// reduce.hip -- stage 1 of col_reduce(MINMAX, width 4) only: `parts` partial results of [min row, max row] are left in
// `partials` (at most COL_MINMAX_PARTS of them); also clears nzero words at `zero` (may be NULL)
extern "C" int col_minmax4_stage1_zero(void *stream, const void *rows, uint64_t n, int coord_bytes, void *partials, uint32_t *parts,
                                       uint32_t *zero, uint32_t nzero);
// morton.hip -- col_morton plus two by-products for col_collide: packed (x, y, z, r) rows and a zeroed word
extern "C" int col_morton_ex(void *stream, const void *coords, const void *radii, const void *range, uint32_t n,
                             uint32_t padded, int coord_bytes, uint32_t *codes, uint32_t *ids, void *packed,
                             uint32_t *zero_word, uint32_t *publish);
// ... that folds the bounds partials itself (no stage-2 launch) and also writes a histogram for the radix sort (digit = bits
// hist_shift..hist_shift+7: 0 for the LSD sort's pass 0, 22 for the MSD sort's bucket digit), `tile` = 1024, 4096 or 8192
// codes per block (the sort's tile, col_radix_tile), digit-major hist[d * nblocks + b] like k_hist; with `gsum` (the MSD plan
// without a scan launch, col_radix_sort_msd_fused) tile-major hist[b * 256 + d] instead, each count also added into
// gsum[(b / COL_MSD_GROUP) * 256 + d], which must be zero on entry (col_minmax4_stage1_zero clears it in the launch before).
// sorted (1024- or 4096-code tiles, with gsum only): the tile leaves SORTED by the digit, see morton.hip
extern "C" int col_morton_tile(void *stream, const void *coords, const void *radii, const void *partials, uint32_t parts,
                               uint32_t n, uint32_t padded, int coord_bytes, uint32_t *codes, uint32_t *ids, void *packed,
                               uint32_t *zero_word, uint32_t *hist0, uint32_t tile, uint32_t nblocks, int hist_shift,
                               uint32_t *publish, const uint32_t *n_dev, uint32_t *gsum, int sorted);
// radix.hip -- col_radix_sort; have_hist0 = 1: the pass-0 histogram is already at the start of `scratch`
extern "C" int col_radix_sort_ex(void *stream, const void *keys, void *keys_out, const void *vals, void *vals_out,
                                 uint64_t n, int key_bytes, int val_bytes, void *scratch, int copy_back, int have_hist0);
// (u32 key, u32 value) pairs whose keys are below 2^(8 * passes): only that many digit passes
extern "C" int col_radix_sort_low_passes(void *stream, const uint32_t *keys, uint32_t *keys_out, const uint32_t *vals,
                                         uint32_t *vals_out, uint64_t n, void *scratch, int passes);
// col_radix_sort_msd without the scan launch, on what col_morton_tile(gsum) left; `fused`: col_radix_msd_fused_bytes() bytes
extern "C" size_t col_radix_msd_fused_bytes(void);
extern "C" int col_radix_sort_msd_fused(void *stream, const uint32_t *keys, uint32_t *keys_out, const uint32_t *vals, uint32_t *vals_out,
                                        uint64_t n, void *scratch, uint32_t *oversize, const uint32_t *n_real_dev, uint32_t *fused);
// ... and the MSD finish that gathers its buckets from col_morton_tile(sorted)'s tiles (k_bucket_sort GATHER): no global pass
extern "C" int col_radix_sort_msd_gather(void *stream, const uint32_t *tile_keys, uint32_t *keys_out, const uint32_t *tile_vals,
                                         uint32_t *vals_out, uint32_t n_bound, uint64_t padded, void *scratch, uint32_t *oversize,
                                         const uint32_t *n_dev, const uint32_t *gsum, uint32_t tile);
// the largest top-digit bucket of n sorted codes -> *word (col_bucket_report_block below)
extern "C" int col_radix_bucket_report(void *stream, const uint32_t *sorted_codes, uint64_t n, uint32_t *word);
// lbvh.hip -- col_lbvh with `packed` rows (optional, see col_morton_ex) and with what the build does for the walk that
// follows it.  Host side only: the kernels take these one by one.
struct col_walk_prep {
    uint32_t *zero = nullptr;            // words the last kernel clears (the walk's packet counters / chunk header), or NULL
    uint32_t nzero = 8;                  // how many: 8 (the packet counters) or 16 (the chunked walk's whole header)
    const uint32_t *n_dev = nullptr;     // device-side count, or NULL
    uint32_t *walk_order = nullptr;      // the walk's cost / order arrays (WALK ORDER below), or NULL
    int order_mode = 0;                  // 1: a dense scene -- longest walks first; 0: only deal the long walks of a small launch
    uint32_t *report_word = nullptr;     // col_radix_bucket_report's word: the report rides in k_chunk's launch (one extra
    uint32_t report_n = 0;               // workgroup), report_n = length of `codes` with its pads
};
extern "C" int col_lbvh_ex(void *stream, const uint32_t *codes, const uint32_t *ids, const void *coords, const void *radii,
                           const void *packed, col_node *nodes, void *bounds, void *scratch, uint32_t n, int coord_bytes,
                           const col_walk_prep &w);
// bvh.hip -- the whole path's walks: col_traverse with the dynamic packet order (`sched`: eight zeroed words, or NULL) and
// col_traverse_chunked with a header that is already clear (hdr_cleared), both with a device-side count and a walk order
extern "C" int col_traverse_walk(void *stream, uint32_t *pairs, uint32_t *counter, uint32_t capacity, const void *bounds,
                                 uint32_t n, int coord_bytes, uint32_t *sched, const uint32_t *n_dev, uint32_t *walk_order);
extern "C" int col_traverse_chunked_walk(void *stream, uint32_t *pairs, uint32_t *counter, uint32_t capacity, const void *bounds,
                                         uint32_t n, int coord_bytes, void *scratch, const uint32_t *n_dev, uint32_t *walk_order, int hdr_cleared);
extern "C" int col_traverse_dynamic_order(uint32_t n);      // 1: col_collide's exact walk of n spheres takes the dynamic packet order
// ghost spheres as packets of 64 Morton-sorted queries (multi.hip: col_traverse_ghost_slots)
extern "C" int col_traverse_ghost_packets(void *stream, uint32_t *pairs, uint32_t *counter, uint32_t capacity, const void *bounds,
                                          uint32_t n, int coord_bytes, const uint32_t *rec, const uint32_t *order, const uint32_t *count,
                                          uint32_t max_ghosts, const uint32_t *local_gids, const uint32_t *n_dev);

static inline hipStream_t col_stream(void *s) { return (hipStream_t)s; }

static inline uint64_t col_ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }
static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }      // scratch segments start 256-byte aligned

#ifdef __HIPCC__
typedef unsigned long long u64;
typedef unsigned int u32;
// The largest top-digit bucket (code bits 22..29, the MSD plan's bucket digit) of `n` sorted 30-bit codes (pads 0xFFFFFFFF
// behind them) -> *word, bit 31 set (col_radix_bucket_report, radix.hip).  One 256-thread block; s_start: 257 LDS words.
// A device function because the whole path lets it ride in k_chunk's launch (lbvh.hip) instead of a launch of its own.
__device__ __forceinline__ void col_bucket_report_block(const u32 *__restrict__ sorted, u32 n, u32 *word, u32 *s_start) {
    const u32 d = threadIdx.x;
    const u32 want = d << 22;
    u32 lo = 0, hi = n;                        // first position whose code is >= want
    while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (sorted[mid] < want) lo = mid + 1; else hi = mid;
    }
    s_start[d] = lo;
    if (d == 0) {                              // end of bucket 255: the first pad (0xFFFFFFFF) or n
        u32 l2 = 0, h2 = n;
        while (l2 < h2) {
            const u32 mid = l2 + ((h2 - l2) >> 1);
            if (sorted[mid] < (1u << 30)) l2 = mid + 1; else h2 = mid;
        }
        s_start[256] = l2;
    }
    __syncthreads();
    u32 cnt = s_start[d + 1] - s_start[d];
#pragma unroll
    for (int o = COL_WAVE / 2; o > 0; o >>= 1) cnt = max(cnt, (u32)__shfl_xor((int)cnt, o, COL_WAVE));
    __syncthreads();
    if ((d & 63u) == 0) s_start[d >> 6] = cnt;
    __syncthreads();
    if (d == 0) {
        const u32 m = max(max(s_start[0], s_start[1]), max(s_start[2], s_start[3]));
        __hip_atomic_store(word, 0x80000000u | min(m, 0x7FFFFFFFu), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__device__ __forceinline__ u32 lane_id() { return __lane_id(); }

// the real count behind a host-known bound (see col_morton_tile): a wave-uniform (scalar) load
__device__ __forceinline__ u32 count_of(u32 n, const u32 *__restrict__ n_dev) { return n_dev ? min(n, *n_dev) : n; }

// number of set bits of `mask` strictly below this lane
__device__ __forceinline__ u32 mbcnt(u64 mask) {
    return __builtin_amdgcn_mbcnt_hi((u32)(mask >> 32), __builtin_amdgcn_mbcnt_lo((u32)mask, 0u));
}

// lanes of this wave whose 8-bit digit equals mine ("match-any").  For every bit the ballot of
// that bit is XORed with my own bit replicated over the word: the result marks the lanes that
// DIFFER from me in that bit; the eight results are ORed (v_or3) and complemented.  12 VALU per
// 32-lane half instead of 16 for the and-chain formulation.
__device__ __forceinline__ u64 match8(u32 d) {
    // Three batches (masks, ballots, folds) instead of bit by bit: a v_cmp result needs two wait states
    // before a VALU instruction may read it as an SGPR operand, and seven other compares hide them.
    u32 m[8];
    u64 bal[8];
#pragma unroll
    for (int b = 0; b < 8; b++) {
        m[b] = (u32)__builtin_amdgcn_sbfe(d, b, 1);                         // my bit, replicated
        // (opaque to the optimiser: it otherwise derives the comparison from d again -- shift + sign test --
        // instead of comparing the mask it already has: 5 instead of 4 VALU per bit)
        asm("" : "+v"(m[b]));
    }
#pragma unroll
    for (int b = 0; b < 8; b++) bal[b] = __builtin_amdgcn_ballot_w64(m[b] != 0);
    u32 dlo = 0, dhi = 0;
#pragma unroll
    for (int b = 0; b < 8; b++) {
        // acc | (ballot ^ mine) in one v_bitop3 per half (truth table 0xF6 for (acc, ballot, mine))
        dlo = __builtin_amdgcn_bitop3_b32(dlo, (u32)bal[b], m[b], 0xF6);
        dhi = __builtin_amdgcn_bitop3_b32(dhi, (u32)(bal[b] >> 32), m[b], 0xF6);
    }
    return ~(((u64)dhi << 32) | dlo);
}

// inclusive wave scan (add) via shuffles; wave = 64 lanes
__device__ __forceinline__ u32 wave_incl_scan(u32 v) {
    const u32 lane = lane_id();
#pragma unroll
    for (int o = 1; o < COL_WAVE; o <<= 1) {
        u32 t = __shfl_up(v, o, COL_WAVE);
        if (lane >= (u32)o) v += t;
    }
    return v;
}

__device__ __forceinline__ u32 wave_sum(u32 v) {
#pragma unroll
    for (int o = COL_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, COL_WAVE);
    return v;
}

// Exclusive scan of one value per thread over a block of NT threads.
// `warp_sums` is NT/64 words of LDS.  Returns the exclusive prefix; *total gets the block sum.
template <int NT>
__device__ __forceinline__ u32 block_excl_scan(u32 v, u32 *warp_sums, u32 *total) {
    constexpr int NW = NT / COL_WAVE;
    const u32 lane = lane_id(), w = threadIdx.x / COL_WAVE;
    u32 incl = wave_incl_scan(v);
    if (lane == COL_WAVE - 1) warp_sums[w] = incl;
    __syncthreads();
    u32 base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < NW; i++) {
        u32 s = warp_sums[i];
        if ((u32)i < w) base += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return base + incl - v;
}
// ---- traversal links (lane w of every node's Bound record, bvh.hip): `skip`, and `down` = left child (internal
// node) or sphere id (leaf).  LEAF BLOCKS: lbvh.hip lets an internal node that covers at most COL_LEAF_BLOCK
// consecutive sorted leaves [lo, hi] AND is dense (its box is at most a few leaf boxes wide on every axis, so a query
// that meets the node meets a good part of its leaves) carry COL_LINK_MARK | lo << 4 | (hi - lo) in `down` instead:
// a walk that hits it tests its leaves -- consecutive 32-byte records from leaf_start + lo -- straight away instead
// of descending (two dependent record fetches per leaf).  Only written while lo fits 27 bits
// (n <= COL_LEAF_BLOCK_MAX_N); larger trees carry plain child links and walkers must not interpret bit 31.
#define COL_LEAF_BLOCK 16u
#define COL_LINK_MARK 0x80000000u
#define COL_LEAF_BLOCK_MAX_N (1u << 27)
__device__ __forceinline__ u32 block_link(u32 lo, u32 hi) { return COL_LINK_MARK | (lo << 4) | (hi - lo); }
// where a walk goes on from a hit internal node with link `down`: its left child, or (leaf block) its first leaf --
// the skip links of the leaves then lead through the whole block (nested blocks are entered the same way)
__device__ __forceinline__ u32 descend_link(u32 down, u32 leaf_start, bool marks) {
    return (marks && (down & COL_LINK_MARK)) ? leaf_start + ((down >> 4) & 0x7FFFFFFu) : down;
}
// ---- WALK ORDER (round 4): the traversal's dynamic packet order hands out an XCD's walks LONGEST FIRST, by what each packet's
// walk took in the PREVIOUS call on the same scratch (any order is correct; a scene that changes little from call to call -- a
// simulation, a benchmark loop -- gets the makespan of a longest-first list schedule instead of a tail of late long walks).
// walk_order = cost[npk] then perm[npk] (u32 each, npk = packets of the BOUND n) then eight words "perm in use on XCD x": k_traverse
// writes a packet's walk time into cost[]; the tree build's last launch (k_cross: 8 x COL_ORDER_SLICES extra workgroups) turns the
// previous costs into perm[] per XCD range, and k_traverse maps walk unit u to packet perm[u] & 0x7FFFFFFF (bit 31: a long walk,
// run at raised wave priority).  Two modes (lbvh.hip): a DENSE scene (chunked pair allocation: its walks differ by 5 x) gets eight
// classes by cost / mean, longest first; any other scene of up to COL_DEAL_MAX_N spheres (a launch of two or three rounds) only
// has its few long walks dealt over the first round's batches, everything else in natural order.  Larger sparse scenes: nothing
// (walk_order = NULL -- no times recorded, no order: both cost more there than they gain).
#define COL_DEAL_MAX_N 1310720u     // 8 XCDs x 2560 packets x 64
#define COL_TRAV_WAVES 16u      // packets per batch of the dynamic order = waves per k_traverse workgroup (bvh.hip TW)
#define COL_TRAV_FIRST_BATCHES 64      // workgroups of the traversal's grid per XCD (512 / 8): the batches that start at once
__device__ __forceinline__ void xcd_packet_range(u32 npackets, u32 x, u32 &p_lo, u32 &p_end) {
    const u32 ng = (npackets + COL_TRAV_WAVES - 1) / COL_TRAV_WAVES;
    p_lo = (u32)(((u64)ng * x) >> 3) * COL_TRAV_WAVES;
    p_end = min((u32)(((u64)ng * (x + 1)) >> 3) * COL_TRAV_WAVES, npackets);
}
// ---- Karras' sequential search (collision.cl:65-121), one node per thread; shared by bvh.hip (k_build) and lbvh.hip
// (k_chunk_wide).  `code(j)` fetches sorted code j, 0 <= j < n: how -- global memory, an LDS window -- is the caller's.
// delta(i, j): common-prefix length of codes i and j (ci = code(i)), index bits as the tie-break for equal codes, -1 outside [0, n)
template <typename Code> __device__ __forceinline__ int karras_delta(Code code, u32 n, u32 i, u32 ci, int64_t j) {
    if (j < 0 || j >= (int64_t)n) return -1;
    const u32 cj = code(j);
    return ci != cj ? __clz((int)(ci ^ cj)) : 32 + __clz((int)(i ^ (u32)j));
}
// The right child whose range starts at leaf k (1 <= k <= n-1): internal node k if that node's range runs forward from k,
// otherwise the single leaf k.
template <typename Code> __device__ __forceinline__ u32 right_child_at(Code code, u32 n, u32 k) {
    if (k + 1 >= n) return (n - 1) + k;
    const u32 ck = code((int64_t)k);
    const bool fwd = karras_delta(code, n, k, ck, (int64_t)k + 1) > karras_delta(code, n, k, ck, (int64_t)k - 1);
    return fwd ? k : (n - 1) + k;
}
// internal node i (i + 1 < n, ci = code(i)): its other end j and its split gamma (the last leaf of its left child)
template <typename Code> __device__ __forceinline__ void karras_search(Code code, u32 n, u32 i, u32 ci, u32 &j, u32 &gamma) {
    const int dir = karras_delta(code, n, i, ci, (int64_t)i + 1) > karras_delta(code, n, i, ci, (int64_t)i - 1) ? 1 : -1;
    const int delta_min = karras_delta(code, n, i, ci, (int64_t)i - dir);
    int64_t len_max = 2;
    while (karras_delta(code, n, i, ci, (int64_t)i + dir * len_max) > delta_min) len_max *= 2;
    int64_t len = 0;
    for (int64_t t = len_max / 2; t > 0; t /= 2)
        if (karras_delta(code, n, i, ci, (int64_t)i + dir * (len + t)) > delta_min) len += t;
    j = (u32)((int64_t)i + dir * len);
    const int delta_node = karras_delta(code, n, i, ci, (int64_t)j);
    int64_t s = 0, t = len;
    do {
        t = (t + 1) / 2;
        if (karras_delta(code, n, i, ci, (int64_t)i + dir * (s + t)) > delta_node) s += t;
    } while (t > 1);
    gamma = dir > 0 ? (u32)(i + s) : (u32)(i - s - 1);
}
// ---- 30-bit Morton codes (collision.cl:14-31); shared by morton.hip and multi.hip ----
__device__ __forceinline__ u32 expand_bits(u32 v) {   // collision.cl:14-20
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}
template <typename T> __device__ __forceinline__ T tmax(T a, T b);
template <> __device__ __forceinline__ float tmax(float a, float b) { return fmaxf(a, b); }
template <> __device__ __forceinline__ double tmax(double a, double b) { return fmax(a, b); }
template <typename T> __device__ __forceinline__ T tmin(T a, T b);
template <> __device__ __forceinline__ float tmin(float a, float b) { return fminf(a, b); }
template <> __device__ __forceinline__ double tmin(double a, double b) { return fmin(a, b); }
// collision.cl:22-31: q = (uint) clamp(((p - min) / (max - min)) * 1023, 0, 1023); NaN -> 0.
template <typename T>
__device__ __forceinline__ u32 quantize(T p, T mn, T mx) {
    T t = (p - mn) / (mx - mn);
    t = t * (T)1023;
    t = tmin(tmax(t, (T)0), (T)1023);
    return (u32)t;
}
template <typename T>
__device__ __forceinline__ u32 morton30(T x, T y, T z, T mnx, T mny, T mnz, T mxx, T mxy, T mxz) {
    return (expand_bits(quantize(x, mnx, mxx)) << 2) + (expand_bits(quantize(y, mny, mxy)) << 1) +
           expand_bits(quantize(z, mnz, mxz));
}
#endif

