// Fused Karras build + AABB refit for the production path (col_collide).
// Replaces fillInternal + generateBVH + leafBounds + internalBounds
// (collision/collision.cl:55-162, enqueued at collision/collision.py:171-190) and produces the
// same `nodes` and `bounds` arrays as bvh.hip's k_build + k_refit (which stay as the
// reference-shaped, tree-generic kernels for the kernel-level parity tests).
//
// Why not walk the tree: internalBounds hands child boxes from one workgroup to another through
// a flag atomic (collision.cl:152-161).  On MI355X that needs an agent-scope release + acquire
// per level per wave (8 XCDs, non-coherent L2s) and cost 6.3 ms at 1 M spheres.  An LBVH node
// covers a CONTIGUOUS range [first, last] of sorted leaves, so its box is a range-min/max query
// over the leaf boxes, and min/max are exact and idempotent: any grouping gives the reference's
// bits.  So there is no inter-workgroup hand-off at all:
//
//   k_chunk   one block per 256 consecutive sorted leaves: leaf boxes -> LDS; Karras topology for
//             internal nodes [c*256, c*256+256); a node whose range stays inside the chunk is built
//             bottom-up in LDS from the chunk's adjacent deltas (the climb), merges its children and
//             publishes its box; every node is written as one 32-byte record (box + traversal links)
//             per thread.  A node that crosses the chunk boundary stores the half of its range that
//             lies in this chunk (`partial`: the prefix / suffix unions of the chunk's leaf boxes);
//             Karras' search for its other end, split and links runs in a search workgroup of the
//             same launch (a wave per chunk, sorted codes staged in an LDS window chunk +- 256 for
//             the dependent probes).  (From 2^30 leaves on k_chunk_wide takes its place: 64-bit positions, Karras'
//             search for every node in the chunk's own workgroup, which waits in LDS for the children.)
//   k_group   (above COL_MSD_MAX_N / 256 chunks only; 1-2 tiny launches) sparse tables over chunk totals,
//             256 chunks per group, then over group totals, ...
//   k_cross   the ~1-2 % of nodes that cross chunks: partial[first] U partial[last] U the whole chunks in
//             between -- read straight from the chunk totals k_chunk wrote (short ranges by the node's thread,
//             longer ones by a wave or by the whole workgroup), or, where k_group ran, O(1) table look-ups.  k_chunk lists them per chunk (CROSS_CAP words),
//             k_cross runs one thread per list slot (round 3: 76 -> 43 us at 16 M spheres; a thread per NODE left
//             one or two busy lanes per wave).
//
// partial[] is indexed by NODE index: a crossing node that runs forward from `first` owns
// partial[first]; the far end `last` of that node is the index of the backward crossing node
// that ends at `last` (its nearest left-child ancestor-or-self chain: Karras gives a left child
// the index of its last leaf), which stored the prefix box of its chunk up to `last` -- exactly
// the piece the forward node is missing.  Symmetrically for backward nodes; leaf n-1 (no
// internal node has that index) stores its prefix itself.
#include "col_common.h"
#include <math.h>

namespace {

constexpr u32 END = 0xFFFFFFFFu;
constexpr int C = 256;          // leaves per chunk == threads per block
constexpr int LV = 9;           // table levels 0..8 (2^8 = 256)

template <typename T> struct BT;
template <> struct BT<float> { typedef float4 V4; typedef uint32_t Bits; };
template <> struct BT<double> { typedef double4 V4; typedef uint64_t Bits; };

template <typename T> struct Box { T lo[3], hi[3]; };

template <typename T> __device__ __forceinline__ Box<T> box_empty() {
    Box<T> b;
#pragma unroll
    for (int a = 0; a < 3; a++) { b.lo[a] = (T)INFINITY; b.hi[a] = -(T)INFINITY; }
    return b;
}
// min / max as ONE instruction.  `o < a ? o : a` compiles to v_cmp + two wait states + v_cndmask on gfx950 (a VALU
// instruction may not read an SGPR mask a VALU instruction has just written), and box unions are a third of k_chunk's
// vector instructions.  v_min / v_max return the same bits as the compare-and-select for every pair of ordinary
// numbers; they differ only where the reference's own `min(x, y)` (collision.cl:157: "y < x ? y : x") depends on the
// ORDER of its arguments -- a tie between +0 and -0 (the instruction: -0 for min, +0 for max, whatever the order) and
// NaN coordinates (ignored unless both are NaN) -- i.e. where a range-query refit could not promise the tree-order
// result anyway; no fixture of the reference has either.
__device__ __forceinline__ float hw_min(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float hw_max(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ double hw_min(double a, double b) { double r; asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ double hw_max(double a, double b) { double r; asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
template <typename T> __device__ __forceinline__ void box_merge(Box<T> &a, const Box<T> &o) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        a.lo[k] = hw_min(a.lo[k], o.lo[k]);
        a.hi[k] = hw_max(a.hi[k], o.hi[k]);
    }
}
// (component by component: a reference to one of two boxes would keep both in memory)
template <typename T> __device__ __forceinline__ Box<T> box_select(bool c, const Box<T> &a, const Box<T> &b) {
    Box<T> r;
#pragma unroll
    for (int k = 0; k < 3; k++) { r.lo[k] = c ? a.lo[k] : b.lo[k]; r.hi[k] = c ? a.hi[k] : b.hi[k]; }
    return r;
}

// global table / partial entry: two vec4 rows (lo.xyz, -) (hi.xyz, -)
template <typename T> __device__ __forceinline__ void box_store(T *base, uint64_t entry, const Box<T> &b) {
    typedef typename BT<T>::V4 V4;
    V4 *p = reinterpret_cast<V4 *>(base) + 2 * entry;
    V4 lo, hi;
    lo.x = b.lo[0]; lo.y = b.lo[1]; lo.z = b.lo[2]; lo.w = (T)0;
    hi.x = b.hi[0]; hi.y = b.hi[1]; hi.z = b.hi[2]; hi.w = (T)0;
    p[0] = lo; p[1] = hi;
}
template <typename T> __device__ __forceinline__ Box<T> box_load(const T *base, uint64_t entry) {
    typedef typename BT<T>::V4 V4;
    const V4 *p = reinterpret_cast<const V4 *>(base) + 2 * entry;
    const V4 lo = p[0], hi = p[1];
    Box<T> b;
    b.lo[0] = lo.x; b.lo[1] = lo.y; b.lo[2] = lo.z;
    b.hi[0] = hi.x; b.hi[1] = hi.y; b.hi[2] = hi.z;
    return b;
}

// LDS sparse table, structure of arrays: t[level][component][pos]
template <typename T> struct Table { T v[LV][6][C]; };

template <typename T> __device__ __forceinline__ void tab_put(Table<T> &t, int l, int pos, const Box<T> &b) {
#pragma unroll
    for (int k = 0; k < 3; k++) { t.v[l][k][pos] = b.lo[k]; t.v[l][3 + k][pos] = b.hi[k]; }
}
template <typename T> __device__ __forceinline__ Box<T> tab_get(const Table<T> &t, int l, int pos) {
    Box<T> b;
#pragma unroll
    for (int k = 0; k < 3; k++) { b.lo[k] = t.v[l][k][pos]; b.hi[k] = t.v[l][3 + k][pos]; }
    return b;
}
// level l from level l-1 (all 256 threads, barrier inside)
template <typename T> __device__ __forceinline__ void tab_build(Table<T> &t, int tid) {
    for (int l = 1; l < LV; l++) {
        __syncthreads();
        Box<T> b = tab_get(t, l - 1, tid);
        const int o = tid + (1 << (l - 1));
        if (o < C) box_merge(b, tab_get(t, l - 1, o));
        tab_put(t, l, tid, b);
    }
    __syncthreads();
}
// union of entries [a, b], 0 <= a <= b < 256
template <typename T> __device__ __forceinline__ Box<T> tab_query(const Table<T> &t, int a, int b) {
    const int k = 31 - __clz(b - a + 1);
    Box<T> r = tab_get(t, k, a);
    box_merge(r, tab_get(t, k, b - (1 << k) + 1));
    return r;
}

// same query against a global table laid out [group][level][256] of 2 x vec4 entries
template <typename T> __device__ __forceinline__ Box<T> gtab_query(const T *tab, uint64_t group, int a, int b) {
    const int k = 31 - __clz(b - a + 1);
    const uint64_t base = (group * LV + k) * C;
    Box<T> r = box_load(tab, base + a);
    box_merge(r, box_load(tab, base + b - (1 << k) + 1));
    return r;
}

// Sorted codes seen through an LDS window [w0, w0 + WIN) around the chunk: almost every Karras
// probe of a node stays within a few hundred leaves of it, so the dependent-load chains of the
// search run at LDS latency; probes outside the window fall back to global memory.
constexpr int HALO = 256;
constexpr int WIN = C + 2 * HALO;
// (an LDS pointer by type: as a generic pointer the two sides of a window-or-global read become ONE flat_load)
typedef __attribute__((address_space(3))) const u32 LdsWord;
// v_ffbh_u32: leading zeros, 0xFFFFFFFF for 0
__device__ __forceinline__ u32 ffbh_raw(u32 x) { u32 r; asm("v_ffbh_u32 %0, %1" : "=v"(r) : "v"(x)); return r; }
// collision.cl:65-77 for two codes that are in range, the tie rule as an unsigned minimum -- clz(ci ^ cj) is 0xFFFFFFFF exactly
// when the codes are equal, and then 32 + clz(i ^ j) (j != i in every probe, so that is at most 63) is the smaller one
__device__ __forceinline__ u32 delta_of(u32 i, u32 ci, u32 j, u32 cj) { return min(ffbh_raw(ci ^ cj), 32u + ffbh_raw(i ^ j)); }
// SEARCH WAVE's probes (32-bit positions: below 2^30 leaves i +- 2 * range cannot overflow them, and 32-bit index arithmetic
// is half the vector instructions).  The plain form -- range check, window or global memory, equal codes -- compiles to three
// nested per-lane branches: ~40 instructions per probe, a third of them scalar EXEC bookkeeping, and a wave makes ~28 probes.
// Here: one wave-uniform branch (does ANY lane's probe leave the code window?  almost never) and an unconditional LDS read.
struct CodeWindow {
    const u32 *__restrict__ g;
    LdsWord *win;
    int32_t w0;
    // code j; `inb`: this lane asks and 0 <= j < n (any other lane gets a word it must not use)
    __device__ __forceinline__ u32 at(int32_t j, bool inb) const {
        const u32 o = (u32)(j - w0);
        const bool inwin = o < (u32)WIN;
        if (__builtin_amdgcn_ballot_w64(inb && !inwin) == 0) return win[inb ? o : 0u];
        return inb ? (inwin ? win[o] : g[j]) : 0u;
    }
    __device__ __forceinline__ u32 delta(u32 i, u32 ci, int32_t j, bool inb) const { return delta_of(i, ci, (u32)j, at(j, inb)); }
};

template <typename T>
__device__ __forceinline__ void record_store(T *bounds, uint64_t node, const Box<T> &b, u32 skip, u32 down) {
    typedef typename BT<T>::V4 V4;
    typedef typename BT<T>::Bits Bits;
    V4 lo, hi;
    lo.x = b.lo[0]; lo.y = b.lo[1]; lo.z = b.lo[2];
    hi.x = b.hi[0]; hi.y = b.hi[1]; hi.z = b.hi[2];
    const Bits s = (Bits)skip, d = (Bits)down;
    lo.w = *reinterpret_cast<const T *>(&s);
    hi.w = *reinterpret_cast<const T *>(&d);
    V4 *p = reinterpret_cast<V4 *>(bounds) + 2 * node;
    p[0] = lo; p[1] = hi;
}
template <typename T> __device__ __forceinline__ void links_store(T *bounds, uint64_t node, u32 skip, u32 down) {
    typedef typename BT<T>::Bits Bits;
    Bits *p = reinterpret_cast<Bits *>(bounds) + 8 * node;
    p[3] = (Bits)skip;
    p[7] = (Bits)down;
}

// LDS image of one chunk in k_chunk: the leaves, the finished boxes of the in-chunk internal nodes, the climb's tables.
// The image is PACKED so that more workgroups than the CU's 32 wave slots admit fit its LDS (f32: 11.4 KB, under the 12 KB
// of a search workgroup's windows; f64: 21.6 KB): a wave slot that a finished wave frees is only of use to a NEW
// workgroup if the LDS has room for it.
//   leaf[4][C]  the leaf's sphere (x, y, z, r), not its box: the box is c -+ r wherever it is read -- the same two IEEE
//               operations on the same operands as in the leaf's own thread, so the same bits -- and a third less LDS
//   meet        two 16-bit places per word (a value is a far end + 1 <= 256; the first arrival ORs it into a zero place and
//               sees zero, the second sees the first's value -- and spoils the place, which nobody reads again)
//   adj         one signed byte per delta (-1 .. 63)
//   oe, split   other end and split of node c0 + t as chunk-local positions in a byte each; oe[t] == t = not an
//               in-chunk node (a node's range holds two leaves or more: its other end is never itself)
template <typename T> struct ChunkLds {
    T leaf[4][C];
    T node[6][C];
    T wave_tot[2][C / COL_WAVE][6];     // per-wave totals for the prefix / suffix scans
    u32 meet[C / 2];
    u32 ncross;                         // nodes of this chunk that cross its boundary, so far (see CROSS_CAP)
    signed char adj[C + 4];             // adj[1 + t] = delta(p, p + 1) of the chunk's position t, adj[0] = delta(c0 - 1, c0), adj[C + 1]: see k_chunk
    unsigned char oe[C], split[C];
};
// ... and in k_chunk_wide: the same leaves, node boxes and wave totals; a ready flag per node (ready[C] = 1 for ever: the
// 'flag' of a child that is a leaf); the sorted codes c0 - HALO .. c0 + C + HALO
template <typename T> struct WideLds {
    T leaf[4][C];
    T node[6][C];
    T wave_tot[2][C / COL_WAVE][6];
    u32 ready[C + 1];
    u32 ncross;
    u32 win[WIN];
};
template <typename T> __device__ __forceinline__ Box<T> leaf_get(const T (&a)[4][C], int pos) {
    const T x = a[0][pos], y = a[1][pos], z = a[2][pos], r = a[3][pos];
    Box<T> b;
    b.lo[0] = x - r; b.lo[1] = y - r; b.lo[2] = z - r;
    b.hi[0] = x + r; b.hi[1] = y + r; b.hi[2] = z + r;
    return b;
}
// The 1-2 % of nodes that cross a chunk boundary are listed per chunk for k_cross: CROSS_CAP words per chunk, END = free;
// a chunk with more than CROSS_CAP - 1 of them (deep trees: duplicate codes) sets the last word to CROSS_DENSE and k_cross
// goes through all its nodes instead.  (32 since the end of round 4.  tests/analysis/crossing_nodes_per_chunk.py: a chunk has 8.3
// crossing nodes on average, at most 14 on config 2 -- and up to 21 on config 3, where 13 of the 3907 chunks had more than 15: a
// handful of dense chunks, sixteen dependent rounds each, were enough to hold k_cross for 15 us instead of 5.7; whole step 0.515 ->
// 0.505 ms; 64 gains nothing more and costs the 16 M launch 1 %.)
constexpr u32 CROSS_CAP = 32, CROSS_DENSE = 0xFFFFFFFEu;
template <typename T> __device__ __forceinline__ Box<T> soa_get(const T (&a)[6][C], int pos) {
    Box<T> b;
#pragma unroll
    for (int k = 0; k < 3; k++) { b.lo[k] = a[k][pos]; b.hi[k] = a[3 + k][pos]; }
    return b;
}
template <typename T> __device__ __forceinline__ void soa_put(T (&a)[6][C], int pos, const Box<T> &b) {
#pragma unroll
    for (int k = 0; k < 3; k++) { a[k][pos] = b.lo[k]; a[3 + k][pos] = b.hi[k]; }
}
template <typename T> __device__ __forceinline__ Box<T> box_shfl_up(const Box<T> &b, int o) {
    Box<T> r;
#pragma unroll
    for (int k = 0; k < 3; k++) { r.lo[k] = __shfl_up(b.lo[k], o, COL_WAVE); r.hi[k] = __shfl_up(b.hi[k], o, COL_WAVE); }
    return r;
}
template <typename T> __device__ __forceinline__ Box<T> box_shfl_down(const Box<T> &b, int o) {
    Box<T> r;
#pragma unroll
    for (int k = 0; k < 3; k++) { r.lo[k] = __shfl_down(b.lo[k], o, COL_WAVE); r.hi[k] = __shfl_down(b.hi[k], o, COL_WAVE); }
    return r;
}

// Inclusive prefix (lanes 0..l) and suffix (lanes l..63) unions of a wave's f32 boxes on the DPP network: per value one
// v_min / v_max_f32_dpp per step (row_shr 1, 2, 4, 8 inside the rows of 16 -- a lane the shift does not reach keeps its
// value --, then row_bcast:15 into rows 1 and 3 and row_bcast:31 into rows 2 and 3), and for the suffix row_shl 1, 2, 4, 8
// and three rounds "first lane of row 3 / 2 / 1 -> the rows below it" (v_readlane + a v_min / v_max under a narrowed EXEC:
// there is no broadcast towards lower rows).  96 vector instructions and no LDS for the twelve scans instead of
// 144 ds_bpermute + ~240 VALU.  The six values are interleaved, so dependent DPP steps are six instructions apart (two
// wait states are needed after the VALU write of a DPP source, and after a VALU write of an SGPR that a VALU reads);
// s_nop 1 at both ends because the compiler does not track these hazards across the asm boundary.  Needs a full wave.
#define COL_SCAN6(ctrl)                                                                                                       \
    "v_min_f32_dpp %0, %0, %0 " ctrl "\n\tv_min_f32_dpp %1, %1, %1 " ctrl "\n\tv_min_f32_dpp %2, %2, %2 " ctrl "\n\t"        \
    "v_max_f32_dpp %3, %3, %3 " ctrl "\n\tv_max_f32_dpp %4, %4, %4 " ctrl "\n\tv_max_f32_dpp %5, %5, %5 " ctrl "\n\t"
#define COL_DOWN6(src_lane)                                                                                                   \
    "v_readlane_b32 %6, %0, " src_lane "\n\tv_readlane_b32 %7, %1, " src_lane "\n\tv_readlane_b32 %8, %2, " src_lane "\n\t"   \
    "v_readlane_b32 %9, %3, " src_lane "\n\tv_readlane_b32 %10, %4, " src_lane "\n\tv_readlane_b32 %11, %5, " src_lane "\n\t"
#define COL_APPLY6                                                                                                            \
    "v_min_f32 %0, %6, %0\n\tv_min_f32 %1, %7, %1\n\tv_min_f32 %2, %8, %2\n\t"                                               \
    "v_max_f32 %3, %9, %3\n\tv_max_f32 %4, %10, %4\n\tv_max_f32 %5, %11, %5\n\t"
__device__ __forceinline__ void wave_prefix_union(Box<float> &b) {
    asm volatile("s_nop 1\n\t"
                 COL_SCAN6("row_shr:1 row_mask:0xf bank_mask:0xf")
                 COL_SCAN6("row_shr:2 row_mask:0xf bank_mask:0xf")
                 COL_SCAN6("row_shr:4 row_mask:0xf bank_mask:0xf")
                 COL_SCAN6("row_shr:8 row_mask:0xf bank_mask:0xf")
                 COL_SCAN6("row_bcast:15 row_mask:0xa bank_mask:0xf")
                 COL_SCAN6("row_bcast:31 row_mask:0xc bank_mask:0xf")
                 "s_nop 1"
                 : "+v"(b.lo[0]), "+v"(b.lo[1]), "+v"(b.lo[2]), "+v"(b.hi[0]), "+v"(b.hi[1]), "+v"(b.hi[2]));
}
__device__ __forceinline__ void wave_suffix_union(Box<float> &b) {
    u32 t0, t1, t2, t3, t4, t5;
    u64 save;
    asm volatile("s_nop 1\n\t"
                 COL_SCAN6("row_shl:1 row_mask:0xf bank_mask:0xf")
                 COL_SCAN6("row_shl:2 row_mask:0xf bank_mask:0xf")
                 COL_SCAN6("row_shl:4 row_mask:0xf bank_mask:0xf")
                 COL_SCAN6("row_shl:8 row_mask:0xf bank_mask:0xf")
                 "s_mov_b64 %12, exec\n\t"
                 "s_nop 1\n\t"
                 COL_DOWN6("48")                                   // row 3's total -> rows 0..2
                 "s_mov_b32 exec_lo, -1\n\ts_mov_b32 exec_hi, 0xffff\n\t"
                 COL_APPLY6
                 COL_DOWN6("32")                                   // rows 2..3 -> rows 0..1
                 "s_mov_b32 exec_hi, 0\n\t"
                 COL_APPLY6
                 COL_DOWN6("16")                                   // rows 1..3 -> row 0
                 "s_mov_b32 exec_lo, 0xffff\n\t"
                 COL_APPLY6
                 "s_mov_b64 exec, %12\n\t"
                 "s_nop 1"
                 : "+v"(b.lo[0]), "+v"(b.lo[1]), "+v"(b.lo[2]), "+v"(b.hi[0]), "+v"(b.hi[1]), "+v"(b.hi[2]),
                   "=&s"(t0), "=&s"(t1), "=&s"(t2), "=&s"(t3), "=&s"(t4), "=&s"(t5), "=&s"(save));
}
#undef COL_SCAN6
#undef COL_DOWN6
#undef COL_APPLY6
// The same scans for float64 boxes (round 4: the f64 kernel shuffled its twelve doubles through 144 x 2 ds_bpermute and took
// 76.6 us at 1 M spheres against 51 for f32).  There is no v_min_f64 with a DPP operand, so a step moves the two words of a
// value with v_mov_b32_dpp (a lane the shift does not reach keeps its own value: `old` = the source) and merges with
// v_min / v_max_f64; hipcc places the wait states of the builtins itself.
template <int CTRL, int ROW_MASK> __device__ __forceinline__ double dpp_d(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = (int)(u32)b, hi = (int)(u32)((u64)b >> 32);
    const u32 l2 = (u32)__builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xF, false);
    const u32 h2 = (u32)__builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xF, false);
    return __longlong_as_double((long long)(((u64)h2 << 32) | l2));
}
template <int CTRL, int ROW_MASK> __device__ __forceinline__ void box_dpp_merge(Box<double> &b) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        b.lo[k] = hw_min(b.lo[k], dpp_d<CTRL, ROW_MASK>(b.lo[k]));
        b.hi[k] = hw_max(b.hi[k], dpp_d<CTRL, ROW_MASK>(b.hi[k]));
    }
}
__device__ __forceinline__ double readlane_d(double v, int l) {
    const long long b = __double_as_longlong(v);
    const u32 lo = (u32)__builtin_amdgcn_readlane((int)(u32)b, l), hi = (u32)__builtin_amdgcn_readlane((int)(u32)((u64)b >> 32), l);
    return __longlong_as_double((long long)(((u64)hi << 32) | lo));
}
__device__ __forceinline__ void wave_prefix_union(Box<double> &b) {
    box_dpp_merge<0x111, 0xF>(b);       // row_shr:1, 2, 4, 8 inside the rows of 16
    box_dpp_merge<0x112, 0xF>(b);
    box_dpp_merge<0x114, 0xF>(b);
    box_dpp_merge<0x118, 0xF>(b);
    box_dpp_merge<0x142, 0xA>(b);       // row_bcast:15 -> rows 1, 3
    box_dpp_merge<0x143, 0xC>(b);       // row_bcast:31 -> rows 2, 3
}
__device__ __forceinline__ void wave_suffix_union(Box<double> &b) {
    box_dpp_merge<0x101, 0xF>(b);       // row_shl:1, 2, 4, 8
    box_dpp_merge<0x102, 0xF>(b);
    box_dpp_merge<0x104, 0xF>(b);
    box_dpp_merge<0x108, 0xF>(b);
    const u32 lane = lane_id();
#pragma unroll
    for (int first = 48; first >= 16; first -= 16) {      // row 3's total -> rows 0..2, rows 2..3 -> rows 0..1, rows 1..3 -> row 0
        Box<double> t;
#pragma unroll
        for (int k = 0; k < 3; k++) { t.lo[k] = readlane_d(b.lo[k], first); t.hi[k] = readlane_d(b.hi[k], first); }
        if (lane < (u32)first) box_merge(b, t);
    }
}

// node records without the `parent` word, which the parent's thread writes (collision.cl:119-120)
struct __attribute__((packed, aligned(4))) LeafTail { u32 right_edge, id; };
struct __attribute__((packed, aligned(4))) InnerTail { u32 right_edge, child_a, child_b; };

// WALK ORDER (col_common.h), workgroup `ob` of the 8 x COL_ORDER_SLICES that order the packets of the traversal that follows: part of
// k_chunk's launch (the first workgroups of its grid: done long before the launch is) or, with k_chunk_wide, of
// k_cross's (where they were first, and made that launch 11 us instead of 5 at 1 M spheres).  n: this call's number of leaves.
constexpr u32 COL_ORDER_SLICES = 8;     // workgroups per XCD that order its packets
constexpr u32 COL_DEAL_UPTO = COL_DEAL_MAX_N / 512;      // packets per XCD up to which a sparse scene's long walks are dealt
__device__ __forceinline__ void order_packets(u32 ob, u32 n, u32 n_bound, u32 *__restrict__ walk_order, int order_mode) {
    // WALK ORDER (col_common.h): COL_ORDER_SLICES workgroups per XCD look at the costs the previous call's walks left for the
    // XCD's packets and decide this call's order.  The statistics come from a sample of at most 1024 packets (every
    // workgroup of the XCD takes the same one: 16 M spheres are 31 250 packets per XCD, and reading them all in one
    // workgroup made this launch 105 us instead of 42).
    __shared__ unsigned long long s_sum;
    __shared__ u32 s_cnt[8], s_cur[8];
    const u32 x = ob & 7u, g = ob >> 3, npk_bound = (n_bound + 63u) / 64u;
    const u32 *cost = walk_order;
    u32 *perm = walk_order + npk_bound;
    u32 p_lo, p_end;
    xcd_packet_range((n + 63u) / 64u, x, p_lo, p_end);
    if (threadIdx.x == 0) s_sum = 0;
    if (threadIdx.x < 8) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const u32 cnt = p_end > p_lo ? p_end - p_lo : 0u;
    const u32 stride = (cnt + 1023u) / 1024u, nsamp = stride ? (cnt + stride - 1u) / stride : 0u;
    u32 sample[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {                  // (the four loads of a thread go out together: each is a round trip to memory)
        const u32 e = threadIdx.x + 256u * k;
        sample[k] = e < nsamp ? min(cost[p_lo + e * stride], 1u << 24) : 0u;        // (a first call's garbage, capped)
    }
    unsigned long long mine = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) mine += sample[k];
    atomicAdd(&s_sum, mine);
    __syncthreads();
    const unsigned long long mean = nsamp ? max(s_sum / nsamp, 1ull) : 1ull;
    u32 *use_perm = walk_order + 2u * npk_bound + x;       // read by k_traverse's workgroups of this XCD
    if (!cnt) { if (threadIdx.x == 0 && g == 0) *use_perm = 0; return; }
    // Which order: decided by the caller (col_common.h, WALK ORDER).  The walks' times themselves do not tell a dense scene from a
    // large sparse one -- a walk of a 16 M-sphere uniform scene takes 25 us among its 8191 neighbours, and a longest-first order
    // there (it scatters a batch's 16 neighbouring packets, which walk nearly the same nodes, over the XCD's range) cost the
    // traversal 15 %.
    if (order_mode != 1) {
        if (g) return;
        // Moderate scenes (config 2: walks of 7..38 us around a mean of 13, the same packets long in every call): the kernel
        // ends when the last long walk does, so the long walks (>= 1.5 x the mean: one packet in twelve) must START in the
        // first round -- but SPREAD over it: a CU's scalar unit is what its 32 walks share, and long walks in a row (a
        // longest-first list puts sixteen into one workgroup) only slow each other down.  So they are dealt over the leading
        // slots of the XCD's first COL_TRAV_FIRST_BATCHES batches (one per workgroup of the traversal's grid), the longest
        // class (>= 2 x) first; every other packet keeps its natural order in the slots that remain.
        // ... and only where the launch is a few rounds long (up to COL_DEAL_UPTO packets on the XCD: 1.3 M spheres): the order costs
        // every packet a dependent load of its number (1 M: - 1.6 us net of that; 2 M: + 6 us, `gpurun_out/order_ab_6.txt`)
        const u32 nb1 = min(cnt / (u32)COL_TRAV_WAVES, (u32)COL_TRAV_FIRST_BATCHES);
        if (nb1 == 0 || cnt > COL_DEAL_UPTO) {
            if (threadIdx.x == 0) *use_perm = 0;          // natural order: k_traverse does not read perm[]
            return;
        }
        const u32 thr2 = (u32)min(2ull * mean, 0xFFFFFFFFull), thr1 = (u32)min(mean + mean / 2, 0xFFFFFFFFull);
        if (threadIdx.x < 2) s_cur[threadIdx.x] = 0;
        constexpr int PER = (int)(COL_DEAL_UPTO + 255u) / 256;       // a thread's packets: PER consecutive ones from p_lo + PER * threadIdx.x
        u32 mycost[PER];
        const u32 q0 = p_lo + (u32)PER * threadIdx.x;
#pragma unroll
        for (int k = 0; k < PER; k++) mycost[k] = q0 + k < p_end ? min(cost[q0 + k], 1u << 24) : 0u;
        u32 my_shorts = 0;
#pragma unroll
        for (int k = 0; k < PER; k++) {
            if (q0 + k >= p_end) continue;
            if (mycost[k] >= thr1) atomicAdd(&s_cnt[mycost[k] >= thr2 ? 0 : 1], 1u);
            else my_shorts++;
        }
        __syncthreads();
        const u32 l2 = s_cnt[0], l = l2 + s_cnt[1];
        if (l == 0 || l > 8u * nb1) {
            if (threadIdx.x == 0) *use_perm = 0;
            return;
        }
        if (threadIdx.x == 0) *use_perm = 1;
        const u32 per = l / nb1, rem = l % nb1;                      // batch j starts with per + (j < rem) long walks
        const u32 cap_a = (u32)COL_TRAV_WAVES - per - 1u, cap_b = (u32)COL_TRAV_WAVES - per, in_a = rem * cap_a, in_ab = in_a + (nb1 - rem) * cap_b;
        __shared__ u32 s_ws[4];
        u32 tot;
        u32 r = block_excl_scan<256>(my_shorts, s_ws, &tot);       // (one scan: the threads' runs of packets are in natural order)
#pragma unroll
        for (int k = 0; k < PER; k++) {
            const u32 q = q0 + k, c = mycost[k];
            if (q >= p_end) continue;
            u32 pos;
            if (c < thr1) {
                if (r < in_a) pos = (r / cap_a) * (u32)COL_TRAV_WAVES + per + 1u + r % cap_a;
                else if (r < in_ab) pos = (rem + (r - in_a) / cap_b) * (u32)COL_TRAV_WAVES + per + (r - in_a) % cap_b;
                else pos = nb1 * (u32)COL_TRAV_WAVES + (r - in_ab);
                r++;
            } else {
                const u32 kk = c >= thr2 ? atomicAdd(&s_cur[0], 1u) : l2 + atomicAdd(&s_cur[1], 1u);
                pos = (kk % nb1) * (u32)COL_TRAV_WAVES + kk / nb1;
            }
            perm[p_lo + pos] = c < thr1 ? q : q | 0x80000000u;        // (bit 31: walked at raised priority)
        }
        return;
    }
    // Longest first: eight classes by cost * 4 / mean (capped), the longest class first, any order inside a class (an LDS
    // cursor).  From 4096 packets the XCD's range is cut into COL_ORDER_SLICES slices, a workgroup each, and the slices' orders
    // are interleaved (element k of slice g goes to place k * slices + g): longest first up to the slices' differences.
    const u32 slices = cnt >= 4096u ? (u32)COL_ORDER_SLICES : 1u;
    if (g >= slices) return;
    if (threadIdx.x == 0 && g == 0) *use_perm = 1;
    const u32 len = cnt / slices, longer = cnt % slices;                       // slice g: len + (g < longer) packets
    const u32 s_lo = p_lo + g * len + min(g, longer), s_end = s_lo + len + (g < longer ? 1u : 0u);
    // (four loads of a thread go out together in both passes: each is a round trip to memory)
    auto cls_of = [&](u32 c) -> u32 { return (u32)min(7ull, (unsigned long long)c * 4ull / mean); };
    for (u32 base = s_lo; base < s_end; base += 1024) {
        u32 c[4];
#pragma unroll
        for (int k = 0; k < 4; k++) { const u32 q = base + 256u * k + threadIdx.x; c[k] = q < s_end ? min(cost[q], 1u << 24) : 0u; }
#pragma unroll
        for (int k = 0; k < 4; k++) if (base + 256u * k + threadIdx.x < s_end) atomicAdd(&s_cnt[cls_of(c[k])], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) { u32 acc = 0; for (int k = 7; k >= 0; k--) { s_cur[k] = acc; acc += s_cnt[k]; } }
    __syncthreads();
    for (u32 base = s_lo; base < s_end; base += 1024) {
        u32 c[4];
#pragma unroll
        for (int k = 0; k < 4; k++) { const u32 q = base + 256u * k + threadIdx.x; c[k] = q < s_end ? min(cost[q], 1u << 24) : 0u; }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const u32 q = base + 256u * k + threadIdx.x;
            if (q >= s_end) continue;
            const u32 cls = cls_of(c[k]);
            const u32 kk = atomicAdd(&s_cur[cls], 1u);
            perm[p_lo + (kk < len ? kk * slices + g : len * slices + g)] = cls >= 6u ? q | 0x80000000u : q;
        }
    }
    return;
}

// LDS of the production k_chunk: what a workgroup holds depends on its place in the grid -- a chunk's image, a code window for
// each of the four chunks a search workgroup serves, or the bucket report's 257 words
template <typename T> union ProdLds {
    ChunkLds<T> chunk;
    u32 win[C / COL_WAVE][WIN];
    u32 report[C + 1];
};
// PLACES.  k_chunk's grid behind its order_packets workgroups holds chunk workgroups and search workgroups (SEARCH WAVE below: a
// wave per chunk, four chunks to a workgroup).  blockIdx % 8 is the XCD, each XCD builds one contiguous run of the chunks, and a
// chunk's searcher runs on the chunk's XCD: it reads its code window from the same L2.  Two layouts, chosen by the chunk count:
//   searchers first  [all search workgroups][all chunk workgroups]   the fastest step at 1 M spheres and on config 3; at 16 M the
//                    searchers are 7.6 rounds of resident waves before the first chunk starts: col_lbvh + 6.7 %
//   groups of 40     [32 chunk workgroups][8 search workgroups, one per XCD: the searchers of the group's own 32 chunks]
//                    the fastest from 2 M spheres up
// Searchers first up to SEARCH_FIRST_MAX_CHUNKS chunks -- they are then less than one round of the CUs' wave places --, groups
// above.  (Timed and dropped, EXPERIMENTS R8: all searchers LAST only fill the drain of the last round, slower than no split;
// groups with their searchers in FRONT equal the groups kept.)
constexpr u32 SEARCH_FIRST_MAX_CHUNKS = 1500000 / C;           // between the measured sizes: 1 M (searchers first wins) and 2 M (groups)
constexpr u32 SEARCH_CHUNKS = C / COL_WAVE;                     // chunks per search workgroup
constexpr u32 PLACE_CHUNKS = 8u * SEARCH_CHUNKS, PLACE_GROUP = PLACE_CHUNKS + 8u;      // 32 chunk workgroups and their 8 search workgroups
// number of chunk + search workgroups for `chunks` chunks (a bound, under a device-side count)
__host__ __device__ __forceinline__ u32 place_blocks(u32 chunks) {
    if (chunks > SEARCH_FIRST_MAX_CHUNKS) return PLACE_GROUP * ((chunks + PLACE_CHUNKS - 1u) / PLACE_CHUNKS);
    // (a multiple of 8 search workgroups, so that every XCD gets the same number)
    return chunks + 8u * (((chunks + 7u) / 8u + SEARCH_CHUNKS - 1u) / SEARCH_CHUNKS);
}
// workgroup v of those: a chunk workgroup (its number `bid` among them; bid % 8 is its XCD) or search workgroup `m` of XCD `xcd`
struct Place { bool searcher; u32 bid, xcd, m; };
__device__ __forceinline__ Place place_of(u32 v, u32 chunks) {
    Place pl;
    if (chunks > SEARCH_FIRST_MAX_CHUNKS) {
        const u32 grp = v / PLACE_GROUP, within = v % PLACE_GROUP;
        pl.searcher = within >= PLACE_CHUNKS;
        pl.bid = grp * PLACE_CHUNKS + within;
        pl.xcd = within & 7u;
        pl.m = grp;
    } else {
        const u32 nsearch = place_blocks(chunks) - chunks;
        pl.searcher = v < nsearch;
        pl.bid = v - nsearch;
        pl.xcd = v & 7u;
        pl.m = v >> 3;
    }
    return pl;
}
// XCD-aware order: blockIdx % 8 is the XCD (each with its own L2).  Every XCD builds one contiguous run of the nb chunks -- the
// same eighth of the sorted leaves whose packets it walks in k_traverse, and neighbouring chunks read overlapping codes: XCD x's
// run has xcd_chunks(nb, x) chunks, xcd_chunk(nb, x, k) is its k-th.  Same bits; whole path, interleaved A/B of two builds on one
// box: 1 M uniform 0.1706-0.1736 against 0.1744-0.1757 ms, 2 M 0.293-0.296 against 0.298-0.301, 16 M and config 3 unchanged; a
// clustered scene at 2 M loses 2.5 % (the deep chunks of a cluster all go to one XCD; strips of 16 chunks going round the XCDs
// avoid that and gain 0.4 % instead of 1.5 %: not taken).
__device__ __forceinline__ u32 xcd_chunks(u32 nb, u32 x) { return nb / 8 + (x < nb % 8 ? 1u : 0u); }
__device__ __forceinline__ u32 xcd_chunk(u32 nb, u32 x, u32 k) { const u32 q = nb / 8, r = nb % 8; return x * q + (x < r ? x : r) + k; }

// ---- what k_chunk and k_chunk_wide share: a chunk workgroup's leaves and the words a finished node leaves behind ----
// leaf tid of the chunk (sphere `id`; valid: it exists): its sphere into the LDS image, returns its box (empty if not valid).
// collision.cl:128-141 (leafBounds)
template <typename T>
__device__ __forceinline__ Box<T> leaf_in(const T *__restrict__ coords, const T *__restrict__ radii, const T *__restrict__ packed,
                                          bool valid, u32 id, int tid, T (&image)[4][C]) {
    typedef typename BT<T>::V4 V4;
    Box<T> leaf = box_empty<T>();
    if (valid) {
        V4 c;
        T r;
        if (packed) {                 // (x, y, z, r) rows written by col_morton_ex: one gather per leaf
            c = reinterpret_cast<const V4 *>(packed)[id];
            r = c.w;
        } else {
            c = reinterpret_cast<const V4 *>(coords)[id];
            r = radii[id];
        }
        leaf.lo[0] = c.x - r; leaf.lo[1] = c.y - r; leaf.lo[2] = c.z - r;
        leaf.hi[0] = c.x + r; leaf.hi[1] = c.y + r; leaf.hi[2] = c.z + r;
        image[0][tid] = c.x; image[1][tid] = c.y; image[2][tid] = c.z; image[3][tid] = r;      // (a place beyond n is never read)
    }
    return leaf;
}
// The chunk-wide prefix / suffix unions from the waves' inclusive ones: every wave has left its totals, and behind a barrier
// every thread folds in the totals of the waves before / behind its own.
template <typename T>
__device__ __forceinline__ void wave_totals_fold(const T (&wave_tot)[2][C / COL_WAVE][6], int w, Box<T> &pre, Box<T> &suf) {
    for (int ww = 0; ww < C / COL_WAVE; ww++) {
        Box<T> t;
#pragma unroll
        for (int k = 0; k < 3; k++) { t.lo[k] = wave_tot[ww < w ? 0 : 1][ww][k]; t.hi[k] = wave_tot[ww < w ? 0 : 1][ww][3 + k]; }
        if (ww < w) box_merge(pre, t);
        if (ww > w) box_merge(suf, t);
    }
}
// node i with its other end j and its split gamma: the node record's tail and the children's parent words (NODES); returns the
// left child (collision.cl:104-120)
template <bool NODES>
__device__ __forceinline__ u32 node_children(col_node *__restrict__ nodes, u32 leaf_start, u32 i, u32 j, u32 gamma) {
    const u32 lo = min(i, j), hi = max(i, j);
    const bool a_leaf = lo == gamma, b_leaf = hi == gamma + 1;
    const u32 child_a = a_leaf ? leaf_start + gamma : gamma;
    const u32 child_b = b_leaf ? leaf_start + gamma + 1 : gamma + 1;
    if constexpr (NODES) {
        InnerTail tail = {hi, child_a, child_b};
        *reinterpret_cast<InnerTail *>(&nodes[i].right_edge) = tail;
        nodes[child_a].parent = i;
        nodes[child_b].parent = i;
    }
    return child_a;
}
// a node whose range [i, j] lies in chunk c0 / C: its record with the box, marked as a leaf block if it is small and dense
template <typename T>
__device__ __forceinline__ void record_out(T *__restrict__ bounds, const T (&image)[4][C], u32 c0, u32 n, T block_k,
                                           u32 i, u32 j, u32 skip, u32 child_a, const Box<T> &box) {
    // leaf block (col_common.h): a small DENSE node -- on every axis at most block_k times as wide as its first
    // leaf -- is marked for the packet walk.  Sparse scenes (BASELINE config 2: leaf boxes a fifth of the
    // spacing) get no marks and walk as before; where spheres overlap in heaps (config 3) nearly every node
    // of <= 16 leaves qualifies.
    const u32 lo = min(i, j), hi = max(i, j);
    u32 down = child_a;
    if (hi - lo < COL_LEAF_BLOCK && n <= COL_LEAF_BLOCK_MAX_N && block_k > (T)0) {
        const Box<T> first = leaf_get(image, (int)(lo - c0));
        bool dense = true;
#pragma unroll
        for (int k = 0; k < 3; k++) dense = dense && (box.hi[k] - box.lo[k]) <= block_k * (first.hi[k] - first.lo[k]);
        if (dense) down = block_link(lo, hi);
    }
    record_store(bounds, (uint64_t)i, box, skip, down);
}
// a node that crosses its chunk's boundary leaves this chunk's half of its range (`half`: the suffix from i if it runs forward,
// the prefix up to i if backward) and its number for k_cross; returns its slot in the chunk's list (CROSS_CAP - 1 or more: no
// slot, the chunk is dense)
template <typename T>
__device__ __forceinline__ u32 crossing_out(T *__restrict__ partial, u32 *__restrict__ cross, u32 *ncross, u32 chunk, u32 i, const Box<T> &half) {
    box_store(partial, i, half);
    const u32 slot = atomicAdd(ncross, 1u);
    cross[(uint64_t)chunk * CROSS_CAP + (slot < CROSS_CAP - 1 ? slot : CROSS_CAP - 1)] = slot < CROSS_CAP - 1 ? i : CROSS_DENSE;
    return slot;
}

// SEARCH WAVE (round 8).  Karras' search for the nodes of chunk c0 / C whose range crosses the chunk's boundary -- their other end,
// split, children and skip link are functions of the sorted codes and n alone, final before the launch --, by ONE wave of a search
// workgroup of k_chunk's grid instead of the chunk's own workgroup, which ends at the stores behind its climb: the probes beyond the
// code window are dependent round trips to global memory, and a chunk workgroup kept its place on the CU (LDS, four wave slots)
// while one or two of its waves made them.  Which nodes cross is decided by the chunk's 257 adjacent deltas: node t, with
// dp = adj[t] = delta(c0 + t - 1, c0 + t) and dn = adj[t + 1], runs forward iff dn > dp and crosses iff every delta between it and
// the chunk's edge on that side -- adj[t + 1 .. 256] forward, adj[0 .. t] backward -- exceeds min(dn, dp) (-1: no such neighbour):
// a suffix and a prefix minimum, four places per lane.  These are exactly the nodes the climb leaves unnamed
// (tests/test_crossing_criterion.py).  Every word has one writer: this wave writes other_end[i], the skip and down words of record
// i and, with NODES, the node's tail and its children's parent words, for crossing nodes i only; the chunk's workgroup writes none
// of them.  No barrier, no atomics, nothing read that this launch writes.
template <typename T, bool NODES>
__device__ __forceinline__ void search_wave(const u32 *__restrict__ gcodes, col_node *__restrict__ nodes, T *__restrict__ bounds,
                                            u32 *__restrict__ other_end, u32 n, u32 c0, u32 *win) {
    typedef int32_t I;
    const u32 lane = lane_id(), leaf_start = n - 1;
    const CodeWindow codes = {gcodes, (LdsWord *)win, (I)c0 - HALO};
    // the code window: every load first, one wait (see k_chunk)
    u32 wcode[WIN / COL_WAVE];
#pragma unroll
    for (int k = 0; k < WIN / COL_WAVE; k++) {
        const I j = codes.w0 + (I)lane + k * COL_WAVE;
        const bool in = j >= 0 && j < (I)n;
        const u32 v = gcodes[in ? j : (I)0];
        wcode[k] = in ? v : 0u;
    }
#pragma unroll
    for (int k = 0; k < WIN / COL_WAVE; k++) win[lane + k * COL_WAVE] = wcode[k];
    // (LDS instructions of one wave are carried out in order: the compiler only has to keep that order)
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
    auto adj_at = [&](u32 u) -> int {                       // delta(c0 + u - 1, c0 + u), 0 <= u <= C + 1
        const u32 pos = c0 + u;
        if (pos < 1u || pos >= n) return -1;
        return (int)delta_of(pos - 1u, codes.win[HALO + u - 1u], pos, codes.win[HALO + u]);
    };
    int a[5];                                               // adj[4 * lane + e]
#pragma unroll
    for (int e = 0; e < 5; e++) a[e] = adj_at(4u * lane + (u32)e);
    // exclusive prefix minimum over the lanes' adj[4 l .. 4 l + 3], exclusive suffix minimum over their adj[4 l + 1 .. 4 l + 4]
    int pre = min(min(a[0], a[1]), min(a[2], a[3])), suf = min(min(a[1], a[2]), min(a[3], a[4]));
#pragma unroll
    for (int o = 1; o < COL_WAVE; o <<= 1) {
        const int up = __shfl_up(pre, o, COL_WAVE), dn = __shfl_down(suf, o, COL_WAVE);
        if (lane >= (u32)o) pre = min(pre, up);
        if (lane + (u32)o < (u32)COL_WAVE) suf = min(suf, dn);
    }
    pre = __shfl_up(pre, 1, COL_WAVE);
    suf = __shfl_down(suf, 1, COL_WAVE);
    if (lane == 0) pre = 0x7FFFFFFF;
    if (lane == COL_WAVE - 1) suf = 0x7FFFFFFF;
    u64 todo[4];                                            // todo[e]: lanes whose node 4 * lane + e crosses
#pragma unroll
    for (int e = 0; e < 4; e++) {
        int before = pre, behind = suf;                    // min adj[0 .. t], min adj[t + 1 .. C]
        for (int k = 0; k <= e; k++) before = min(before, a[k]);
        for (int k = e + 1; k < 5; k++) behind = min(behind, a[k]);
        const int dp = a[e], dn = a[e + 1];
        const bool inner = c0 + 4u * lane + (u32)e < leaf_start;
        todo[e] = __builtin_amdgcn_ballot_w64(inner && (dn > dp ? behind > dp : before > dn));
    }
    const u32 cnt = (u32)(__builtin_popcountll(todo[0]) + __builtin_popcountll(todo[1]) + __builtin_popcountll(todo[2]) +
                          __builtin_popcountll(todo[3]));
    if (cnt == 0) return;
    // A wave shares its lanes among its nodes -- 64, 32, 16 or 8 lanes per node -- and every step of the three searches (each looks
    // for the end of a run of "yes": delta(i, i + dir * x) > threshold is monotone in x) asks that many places at once: the powers
    // of two, then equal parts of what is left.  A fifth of the round trips of a search per lane, ~35 instructions per step for the
    // whole wave.
    const u32 lpn_log = cnt <= 1 ? 6u : cnt <= 2 ? 5u : cnt <= 4 ? 4u : 3u, lpn = 1u << lpn_log, groups = 64u >> lpn_log;
    const u32 g = lane >> lpn_log, sub = lane & (lpn - 1u);
    auto group_count = [&](bool yes) -> I {                 // how many lanes of my group say yes
        u64 m = __builtin_amdgcn_ballot_w64(yes) >> (g << lpn_log);
        if (lpn < 64u) m &= (1ull << lpn) - 1ull;
        return (I)__builtin_popcountll(m);
    };
    for (u32 base = 0; base < cnt; base += groups) {
        const bool on = base + g < cnt;                      // my group has a node this round
        // node number base + g of the wave's list: todo[0]'s lanes, then todo[1]'s, ...
        u32 e_sel = 0, skip_bits = base + g;
        u64 m = todo[0];
#pragma unroll
        for (u32 e = 0; e < 3; e++) {
            const u32 c = (u32)__builtin_popcountll(todo[e]);
            if (on && e_sel == e && skip_bits >= c) { skip_bits -= c; e_sel = e + 1; m = todo[e + 1]; }
        }
        for (u32 b = 0; b < skip_bits && on; b++) m &= m - 1ull;
        const u32 t = on ? 4u * (u32)__builtin_ctzll(m) + e_sel : lane;
        const u32 i = c0 + t, ci = codes.win[HALO + t];
        const int dn = adj_at(t + 1u), dp = adj_at(t);       // delta(i, i + 1), delta(i - 1, i)
        const int dir = dn > dp ? 1 : -1, delta_min = min(dn, dp);
        // is place x (0 = none) in the run?  one load per lane; LDS if every lane's place is in the window
        auto yes_at = [&](I x, int thr) -> bool {
            const I jk = (I)i + dir * x;
            const bool inb = on && x > 0 && (u32)jk < n;
            const u32 d = codes.delta(i, ci, jk, inb);        // (every lane: a wave-uniform branch inside)
            return inb && (int)d > thr;
        };
        // the first power of two that is not in the range any more
        I hi = 2;
        {
            bool more = on;
            int e0 = 1;
            while (__builtin_amdgcn_ballot_w64(more)) {
                const int e = e0 + (int)sub;
                const I x = (more && e < 31 && (1u << e) <= n) ? (I)(1u << e) : (I)0;
                const I yes = group_count(yes_at(x, delta_min));
                if (more) {
                    hi = (I)(1u << (e0 + yes));
                    more = yes == (I)lpn && e0 + (int)lpn < 31;
                    e0 += (int)lpn;
                }
            }
        }
        // the end of a run of yes between lo (in) and hi (out)
        auto run_end = [&](I lo, I hi, int thr) -> I {
            while (__builtin_amdgcn_ballot_w64(on && hi - lo > 1)) {
                const bool act = on && hi - lo > 1;
                const I step = (hi - lo + (I)lpn) / ((I)lpn + 1);
                const I x = lo + ((I)sub + 1) * step;
                const I yes = group_count(yes_at(act && x < hi ? x : (I)0, thr));
                if (act) { lo += yes * step; hi = min(hi, lo + step); }
            }
            return lo;
        };
        const I len = run_end(hi / 2, hi, delta_min);
        const u32 j = (u32)((I)i + dir * len);
        const bool j_in = j < n;                             // (a group without a node: any j)
        const u32 dj = codes.delta(i, ci, (I)j, j_in);
        const int delta_node = j_in ? (int)dj : -1;
        const I s = run_end((I)0, len, delta_node);
        const u32 gamma = dir > 0 ? (u32)(i + s) : (u32)(i - s - 1);
        if (on && sub == 0) {
            const u32 top = max(i, j);
            const u32 child_a = node_children<NODES>(nodes, leaf_start, i, j, gamma);
            other_end[i] = j;
            u32 skip = END;
            if (top + 1 < n) {
                const u32 k = top + 1;
                if (k + 1 >= n) skip = (n - 1) + k;
                else {
                    // is the right child that starts at leaf k an internal node: its three codes in ONE round trip
                    const u32 ck = codes.at((I)k, true), cm = codes.at((I)k - 1, true), cp = codes.at((I)k + 1, true);
                    skip = delta_of(k, ck, k + 1u, cp) > delta_of(k, ck, k - 1u, cm) ? k : (n - 1) + k;
                }
            }
            links_store(bounds, (uint64_t)i, skip, child_a);
        }
    }
}

// The production tree build: 32-bit positions (n < 2^30), DPP scans, adjacent deltas and the climb in LDS.  Its grid is
// [order_packets workgroups][chunk and search workgroups: PLACES][the bucket report's workgroup]; a chunk workgroup builds the
// leaves and the in-chunk nodes of one chunk and keeps no code window -- what it reads of the codes are its own 256, one before
// and two behind.
// NODES = false: the caller passed no `nodes` array (nothing on the collide path reads it: the walk runs on `bounds`, k_cross
// on other_end[] of the crossing nodes).  The instance has no store into nodes[] and writes other_end[i] for crossing nodes
// only -- 5 of a thread's 7 global stores and 36 of the 100 bytes per sphere; bounds, partial, cross and the chunk totals are
// the same bits.
template <typename T, bool NODES>
__global__ __launch_bounds__(C) void k_chunk(const u32 *__restrict__ gcodes, const u32 *__restrict__ ids,
                                             const T *__restrict__ coords, const T *__restrict__ radii,
                                             const T *__restrict__ packed,
                                             col_node *__restrict__ nodes, T *__restrict__ bounds,
                                             u32 *__restrict__ other_end, T *__restrict__ partial, u32 *__restrict__ cross,
                                             T *__restrict__ tab1, u32 n_bound, T block_k, const u32 *__restrict__ n_dev,
                                             u32 *__restrict__ walk_order, int order_mode, u32 *report_word, u32 report_n) {
    const u32 n = count_of(n_bound, n_dev);  // (device-side count, col_common.h: the grid is sized for the bound)
    __shared__ ProdLds<T> lds_mem;
    ChunkLds<T> &lds = lds_mem.chunk;
    const int tid = threadIdx.x, lane = tid & (COL_WAVE - 1), w = tid / COL_WAVE;
    // with a walk order the first 8 x COL_ORDER_SLICES workgroups of the grid make it -- see order_packets
    const u32 nord = walk_order ? 8u * COL_ORDER_SLICES : 0u;
    if (blockIdx.x < nord) {
        order_packets(blockIdx.x, n, n_bound, walk_order, order_mode);
        return;
    }
    // the LSD plan's bucket report -- how clustered are the codes, for the caller's next choice of plan -- is the LAST workgroup
    // of the grid: twenty dependent loads that as a launch of their own take 8.8 us on config 3
    if (report_word && blockIdx.x == gridDim.x - 1u) {
        col_bucket_report_block(gcodes, report_n, report_word, lds_mem.report);
        return;
    }
    // Chunk workgroups and search workgroups are both sized for the bound and, under a device-side count, clamped the same way:
    // the first `nb` chunk workgroups -- dealt round-robin over the XCDs like all workgroups -- share the real chunks, the
    // others and the searchers of chunks at or beyond the real count leave.  (With the bound's chunk count in xcd_chunk two of
    // eight XCDs sat idle at a bound of 1.3 n: 70 instead of 51 us.)
    const u32 bound_chunks = (n_bound + (u32)C - 1) / (u32)C;
    const Place pl = place_of(blockIdx.x - nord, bound_chunks);
    const u32 nb = n_dev ? (n + (u32)C - 1) / (u32)C : bound_chunks;
    if (pl.searcher) {
        const u32 k = pl.m * SEARCH_CHUNKS + (u32)w;
        if (k >= xcd_chunks(nb, pl.xcd)) return;   // (n == 0 included)
        search_wave<T, NODES>(gcodes, nodes, bounds, other_end, n, xcd_chunk(nb, pl.xcd, k) * (u32)C, lds_mem.win[w]);
        return;
    }
    if (pl.bid >= nb) return;            // (n == 0 included)
    const u32 chunk = xcd_chunk(nb, pl.bid & 7u, pl.bid >> 3);
    const u32 c0 = chunk * C;
    const u32 p = c0 + tid;
    const bool valid = p < n;
    // Every independent load of the block first -- the leaf's code, its two neighbours, the code behind the chunk and the
    // leaf's id, at clamped addresses so that none sits behind a branch -- and ONE wait: with the row gather two dependent
    // round trips per block.
    // (The signed range test and the two clamps -- the code and, below, the id of a place beyond n are 0 -- are the form this
    // load has had since it was one step of a window loop; nothing reads the clamped values, but `gcodes[valid ? p : 0u]`
    // alone, seven instructions less, made col_lbvh 1 us slower at 16 M spheres on each of three boxes: EXPERIMENTS R10.4.)
    const int32_t jme = (int32_t)c0 + tid;
    const bool in = jme >= 0 && jme < (int32_t)n;
    const u32 cme_ld = gcodes[in ? jme : 0];
    const u32 cme = in ? cme_ld : 0u;
    u32 id = ids[valid ? p : 0u];
    // Adjacent deltas: delta(p - 1, p) and delta(p, p + 1).  Karras' direction of node p is the larger of these two numbers,
    // and "is the right child that starts at leaf k an internal node" is adj[k] > adj[k - 1] wherever k - 1 and k lie in this
    // chunk: no code read, no probe.
    int d_prev = -1, d_next = -1;
    const bool has_prev = valid && p >= 1u, has_next = p + 1u < n;
    const u32 cprev = gcodes[has_prev ? p - 1u : 0u], cnext = gcodes[has_next ? p + 1u : 0u];
    if (has_prev) d_prev = (int)delta_of(p, cme, p - 1u, cprev);
    if (has_next) d_next = (int)delta_of(p, cme, p + 1u, cnext);
    lds.adj[1 + tid] = (signed char)d_next;
    if (tid == 0) lds.adj[0] = (signed char)d_prev;
    // adj[C + 1] = delta(c0 + C, c0 + C + 1): with it "is the right child that starts behind the chunk's last leaf an internal
    // node" -- the skip link of that leaf and of a node that ends there -- is adj[C + 1] > adj[C] like everywhere else in the
    // chunk.  One more load, the same address in every lane.
    const u32 k2 = c0 + (u32)C + 1u;
    const u32 c2 = gcodes[k2 < n ? k2 : 0u];
    if (tid == C - 1) lds.adj[C + 1] = k2 < n ? (signed char)delta_of(k2 - 1u, cnext, k2, c2) : (signed char)-1;
    if (tid < C / 2) lds.meet[tid] = 0;
    lds.oe[tid] = (unsigned char)tid;
    if (tid < (int)CROSS_CAP) cross[(uint64_t)chunk * CROSS_CAP + tid] = END;       // (complete before the barrier below: the fence of __syncthreads)
    if (tid == 0) lds.ncross = 0;
    const u32 leaf_start = n - 1;

    // leaves: collision.cl:55-63 (fillInternal) + collision.cl:128-141 (leafBounds)
    if (!valid) id = 0;
    const Box<T> leaf = leaf_in(coords, radii, packed, valid, id, tid, lds.leaf);
    // inclusive prefix / suffix unions over the chunk: DPP scans in the waves (every lane of the block is still here: full
    // waves), then the 4 wave totals
    Box<T> pre = leaf, suf = leaf;
    wave_prefix_union(pre);
    wave_suffix_union(suf);
    // (written out here and in k_chunk_wide: as a function of both boxes hipcc makes ONE store through a selected pointer of
    // the two, and pre and suf live in scratch -- EXPERIMENTS R10.2)
    if (lane == COL_WAVE - 1) { for (int k = 0; k < 3; k++) { lds.wave_tot[0][w][k] = pre.lo[k]; lds.wave_tot[0][w][3 + k] = pre.hi[k]; } }
    if (lane == 0) { for (int k = 0; k < 3; k++) { lds.wave_tot[1][w][k] = suf.lo[k]; lds.wave_tot[1][w][3 + k] = suf.hi[k]; } }
    __syncthreads();       // adjacent deltas, leaf spheres, meeting places and wave totals are in LDS
    wave_totals_fold(lds.wave_tot, w, pre, suf);

    if (valid) {
        if constexpr (NODES) {
            LeafTail tail = {p, id};
            *reinterpret_cast<LeafTail *>(&nodes[leaf_start + p].right_edge) = tail;
        }
        u32 skip_leaf = END;
        if (p + 1 < n) {
            const u32 k = p + 1;
            if (k + 1 >= n) skip_leaf = (n - 1) + k;
            else skip_leaf = lds.adj[tid + 2] > d_next ? k : (n - 1) + k;       // (the chunk's last leaf: adj[C + 1])
        }
        record_store(bounds, (uint64_t)leaf_start + p, leaf, skip_leaf, id);
    }
    if (tid == 0)          // chunk total -> level 0 of the first group table
        box_store(tab1, ((uint64_t)(chunk / C) * LV + 0) * C + (chunk % C), suf);
    if (p == n - 1 && n > (u32)C) box_store(partial, p, pre);      // prefix of the last leaf
    // The climb: the in-chunk nodes bottom-up instead of Karras' searches.  For sorted keys delta(i, j) is the minimum of the
    // adjacent deltas between i and j (equal codes included: their deltas 32 + clz(i ^ j) are the common prefix of the keys
    // (code, position)), so the tree is the Cartesian tree of adj[]: a finished range [l, r] is the LEFT child of its parent --
    // Karras' node r -- if delta(r, r + 1) > delta(l - 1, l), else the right child -- node l --, and the two children of the node
    // that splits behind position g meet at meet[g]: the first leaves its far end there and stops, the second takes over the
    // union and goes on (Apetrei 2014, inside one chunk and in LDS).  One round costs what ONE of a search's probes does, a
    // thread climbs as far as it arrives second, and the boxes are merged on the way: no search, no waiting for children.  A
    // range whose sibling lies outside the chunk stops; its parent crosses the boundary and is found by the chunk's search
    // wave, like every node that the climb has not named (oe[t] == t).
    if (valid) {
        int l = tid, r = tid, my_split = 0;
        bool is_leaf = true;
        Box<T> box = leaf;
        for (;;) {
            const int dl = lds.adj[l], dr = lds.adj[r + 1];
            const bool right = dr > dl;
            if (!is_leaf) {
                const int node = right ? r : l;
                soa_put(lds.node, node, box);
                lds.oe[node] = (unsigned char)(right ? l : r);
                lds.split[node] = (unsigned char)my_split;
            }
            const int g = right ? r : l - 1;
            if ((dl & dr) < 0 || g < 0 || g >= C - 1) break;       // the root; or the sibling lies outside the chunk
            // (LDS instructions of one wave are carried out in order: the box is in lds.node before the exchange, and the reads
            // below come after it -- the compiler only has to keep that order)
            asm volatile("" ::: "memory");
            const u32 place = 16u * ((u32)g & 1u);
            const u32 old = (__hip_atomic_fetch_or(&lds.meet[g >> 1], ((u32)(right ? l : r) + 1u) << place, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >> place) & 0xFFFFu;
            asm volatile("" ::: "memory");
            if (old == 0) break;                                    // first: the sibling will take it from here
            const int far = (int)old - 1;
            Box<T> sib;
            if (right) { sib = far == g + 1 ? leaf_get(lds.leaf, g + 1) : soa_get(lds.node, g + 1); r = far; }
            else { sib = far == g ? leaf_get(lds.leaf, g) : soa_get(lds.node, g); l = far; }
            box_merge(box, sib);
            my_split = g;
            is_leaf = false;
        }
    }
    __syncthreads();       // (every thread of the workgroup: `valid` guards the climb, not the barrier)
    // A node the climb has named: everything is known, and its record goes out.  The others -- three in a hundred: their ranges
    // cross the chunk's boundary -- leave their half box and their number for k_cross (the direction is in adj[]), and that is
    // where this workgroup ends: what those nodes still need is Karras' search, which needs nothing this workgroup computes and
    // whose probes beyond a code window are dependent round trips to global memory (SEARCH WAVE above).
    if (p >= leaf_start) return;
    if (lds.oe[tid] != (unsigned char)tid) {
        const u32 j = c0 + lds.oe[tid], hi = max(p, j);
        const u32 child_a = node_children<NODES>(nodes, leaf_start, p, j, c0 + lds.split[tid]);
        if constexpr (NODES) other_end[p] = j;
        u32 skip = END;
        if (hi + 1 < n) {
            const u32 k = hi + 1;
            if (k + 1 >= n) skip = (n - 1) + k;
            // (a named node's range lies in the chunk: c0 <= hi < c0 + C, and behind its last leaf adj[C + 1] answers)
            else skip = lds.adj[k - c0 + 1] > lds.adj[hi - c0 + 1] ? k : (n - 1) + k;
        }
        record_out(bounds, lds.leaf, c0, n, block_k, p, j, skip, child_a, soa_get(lds.node, tid));
    } else {
        const u32 slot = crossing_out(partial, cross, &lds.ncross, chunk, p, box_select(d_next > d_prev, suf, pre));
        if constexpr (!NODES) {
            // A dense chunk: k_cross goes through ALL its nodes and tells the crossing ones by other_end[], so the words the
            // named nodes did not write are due after all.  The one thread that finds the list full writes them from oe[]
            // (final since the climb's barrier); a chunk in thousands, on clustered scenes only.
            if (slot == CROSS_CAP - 1)
#pragma unroll 1
                for (u32 t = 0; t < (u32)C && c0 + t < leaf_start; t++)
                    if (lds.oe[t] != (unsigned char)t) other_end[c0 + t] = c0 + lds.oe[t];
        }
    }
}

// The wide-index tree build: 64-bit positions, for n >= 2^30 (and at every size under col_debug_lbvh bit 10, where the tests
// use it as a second implementation of k_chunk).  A grid of exactly the chunks' workgroups; each stages a code window, runs
// Karras' search for every node of its chunk in that node's thread, and waits in LDS until the children of an in-chunk node are
// final.  k_cross orders the traversal's packets and the bucket report is a launch of its own.  It writes every word of
// other_end[], with or without NODES: it has no oe[] to make up for them in a dense chunk.
template <typename T, bool NODES>
__global__ __launch_bounds__(C) void k_chunk_wide(const u32 *__restrict__ gcodes, const u32 *__restrict__ ids,
                                                  const T *__restrict__ coords, const T *__restrict__ radii,
                                                  const T *__restrict__ packed,
                                                  col_node *__restrict__ nodes, T *__restrict__ bounds,
                                                  u32 *__restrict__ other_end, T *__restrict__ partial, u32 *__restrict__ cross,
                                                  T *__restrict__ tab1, u32 n_bound, T block_k, const u32 *__restrict__ n_dev) {
    typedef int64_t I;      // a (possibly out-of-range) leaf position: i +- 2 * range overflows 32 bits from 2^30 leaves
    const u32 n = count_of(n_bound, n_dev);
    __shared__ WideLds<T> lds;
    const int tid = threadIdx.x, lane = tid & (COL_WAVE - 1), w = tid / COL_WAVE;
    // (with a device-side count the grid is sized for the bound: the first `nb` workgroups share the real chunks, the others leave)
    const u32 bid = blockIdx.x, nb = n_dev ? (n + (u32)C - 1) / (u32)C : gridDim.x;
    if (bid >= nb) return;            // (n == 0 included)
    const u32 chunk = xcd_chunk(nb, bid & 7u, bid >> 3);
    const u32 c0 = chunk * C;
    const u32 p = c0 + tid;
    const bool valid = p < n;
    // Every independent load of the block first -- the three words of the code window and the leaf's id, at clamped
    // addresses so that none sits behind a branch -- and ONE wait.  As a loop with the LDS store inside, hipcc waits for
    // each window load before it issues the next: with the id and the row gather five dependent round trips per block
    // instead of two.
    const I w0 = (I)c0 - HALO;
    u32 wcode[WIN / C];
#pragma unroll
    for (int k = 0; k < WIN / C; k++) {
        const I j = w0 + tid + k * C;
        const bool in = j >= 0 && j < (I)n;
        const u32 v = gcodes[in ? j : (I)0];
        wcode[k] = in ? v : 0u;
    }
    const u32 id = ids[valid ? p : 0u];
#pragma unroll
    for (int k = 0; k < WIN / C; k++) lds.win[tid + k * C] = wcode[k];
    lds.ready[tid] = 0;
    if (tid < (int)CROSS_CAP) cross[(uint64_t)chunk * CROSS_CAP + tid] = END;       // (complete before the barrier below: the fence of __syncthreads)
    if (tid == 0) { lds.ncross = 0; lds.ready[C] = 1u; }
    const u32 leaf_start = n - 1;
    // code j, 0 <= j < n: from the window, else from global memory
    LdsWord *win = (LdsWord *)lds.win;
    const auto code = [=](I j) -> u32 {
        const I o = j - w0;
        return (o >= 0 && o < WIN) ? win[o] : gcodes[j];
    };

    // leaves: collision.cl:55-63 (fillInternal) + collision.cl:128-141 (leafBounds)
    const Box<T> leaf = leaf_in(coords, radii, packed, valid, id, tid, lds.leaf);
    // inclusive prefix / suffix unions over the chunk (wave shuffles, then the 4 wave totals)
    Box<T> pre = leaf, suf = leaf;
#pragma unroll
    for (int o = 1; o < COL_WAVE; o <<= 1) {
        const Box<T> up = box_shfl_up(pre, o), dn = box_shfl_down(suf, o);
        if (lane >= o) box_merge(pre, up);
        if (lane + o < COL_WAVE) box_merge(suf, dn);
    }
    if (lane == COL_WAVE - 1) { for (int k = 0; k < 3; k++) { lds.wave_tot[0][w][k] = pre.lo[k]; lds.wave_tot[0][w][3 + k] = pre.hi[k]; } }
    if (lane == 0) { for (int k = 0; k < 3; k++) { lds.wave_tot[1][w][k] = suf.lo[k]; lds.wave_tot[1][w][3 + k] = suf.hi[k]; } }
    __syncthreads();       // code window, leaf spheres, ready flags and wave totals are in LDS
    wave_totals_fold(lds.wave_tot, w, pre, suf);

    if (valid) {
        if constexpr (NODES) {
            LeafTail tail = {p, id};
            *reinterpret_cast<LeafTail *>(&nodes[leaf_start + p].right_edge) = tail;
        }
        record_store(bounds, (uint64_t)leaf_start + p, leaf, p + 1 < n ? right_child_at(code, n, p + 1) : END, id);
    }
    if (tid == 0)          // chunk total -> level 0 of the first group table
        box_store(tab1, ((uint64_t)(chunk / C) * LV + 0) * C + (chunk % C), suf);
    if (p == n - 1 && n > (u32)C) box_store(partial, p, pre);      // prefix of the last leaf
    if (p >= leaf_start) return;                      // no barrier below this line
    // Karras' search (collision.cl:81-121) for node i = c0 + tid: its other end and its split, then the node record's tail,
    // the children's parent words and the links
    const u32 i = p;
    u32 j, gamma;
    karras_search(code, n, i, win[HALO + tid], j, gamma);       // (the chunk's own codes are always in the window)
    const u32 lo = min(i, j), hi = max(i, j);
    const u32 child_a = node_children<NODES>(nodes, leaf_start, i, j, gamma);
    other_end[i] = j;
    const u32 skip = hi + 1 < n ? right_child_at(code, n, hi + 1) : END;
    if (lo >= c0 && hi < c0 + C) {
        // Both children live in this chunk.  Wait (in LDS, workgroup scope) until their boxes are
        // final, merge, publish.  The tree is at most 64 levels deep, so this ends after <= 64
        // rounds; finished lanes idle at the loop exit while the others retry.
        const bool a_leaf = lo == gamma, b_leaf = hi == gamma + 1;
        const int la = (int)(gamma - c0), lb = la + 1;
        Box<T> box;
        const int fa = a_leaf ? C : la, fb = b_leaf ? C : lb;      // both flags are read every round, unconditionally
        for (bool done = false; !done;) {
            // (relaxed loads + ONE acquire fence on success: two acquire loads are two serial LDS round trips per round)
            const u32 ra = __hip_atomic_load(&lds.ready[fa], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const u32 rb = __hip_atomic_load(&lds.ready[fb], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (ra & rb) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                box = a_leaf ? leaf_get(lds.leaf, la) : soa_get(lds.node, la);
                box_merge(box, b_leaf ? leaf_get(lds.leaf, lb) : soa_get(lds.node, lb));
                soa_put(lds.node, tid, box);
                __hip_atomic_store(&lds.ready[tid], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                done = true;
            }
        }
        record_out(bounds, lds.leaf, c0, n, block_k, i, j, skip, child_a, box);
    } else {
        links_store(bounds, (uint64_t)i, skip, child_a);
        crossing_out(partial, cross, &lds.ncross, chunk, i, box_select(j > i, suf, pre));
    }
}

// Sparse table over `count` level-0 entries, 256 per group; group totals go to level 0 of `next`.
template <typename T>
__global__ __launch_bounds__(C) void k_group(T *__restrict__ tab, u32 count, T *__restrict__ next, u32 n_bound, const u32 *__restrict__ n_dev,
                                             int level) {
    if (n_dev) {                            // device-side count: this level's real number of entries (chunks, groups, ...)
        u32 c = count_of(n_bound, n_dev);
        for (int k = 0; k <= level; k++) c = (c + C - 1) / C;
        count = min(count, c);
    }
    __shared__ Table<T> t;
    const int tid = threadIdx.x;
    const u32 g = blockIdx.x;
    const u32 e = g * C + tid;
    const uint64_t base = (uint64_t)g * LV * C;
    Box<T> b = e < count ? box_load(tab, base + tid) : box_empty<T>();
    if (e >= count) box_store(tab, base + tid, b);
    tab_put(t, 0, tid, b);
    tab_build(t, tid);
    for (int l = 1; l < LV; l++) box_store(tab, base + (uint64_t)l * C + tid, tab_get(t, l, tid));
    if (tid == 0 && next) box_store(next, ((uint64_t)(g / C) * LV + 0) * C + (g % C), tab_get(t, LV - 1, 0));
}

struct Tabs { void *t[3]; };

// `lin`: the table level whose sparse table was not built because it has at most LIN entries (one
// launch less on inputs up to 2 M leaves); a range on that level is a short scan of its level-0 row.
constexpr u32 LIN = 32;

template <typename T>
__device__ __forceinline__ void cross_node(T *__restrict__ bounds, const u32 *__restrict__ other_end, const T *__restrict__ partial,
                                           const Tabs &tabs, u32 i, int lin) {
    const u32 j = other_end[i];
    const u32 first = min(i, j), last = max(i, j);
    int64_t a = first / C, b = last / C;
    if (a == b) return;
    Box<T> box = box_load(partial, first);
    box_merge(box, box_load(partial, last));
    a += 1; b -= 1;                      // whole chunks strictly between the two ends
    for (int h = 0; h < 3 && a <= b; h++) {
        const T *tab = (const T *)tabs.t[h];
        if (h == lin) {                  // single group, level 0 only: entry e sits at index e
            for (int64_t e = a; e <= b; e++) box_merge(box, box_load(tab, (uint64_t)e));
            break;
        }
        const int64_t ga = a / C, gb = b / C;
        if (ga == gb) {
            box_merge(box, gtab_query(tab, (uint64_t)ga, (int)(a % C), (int)(b % C)));
            break;
        }
        box_merge(box, gtab_query(tab, (uint64_t)ga, (int)(a % C), C - 1));
        box_merge(box, gtab_query(tab, (uint64_t)gb, 0, (int)(b % C)));
        a = ga + 1; b = gb - 1;
    }
    // links (lane w) were written by k_chunk: store xyz only
    T *row = bounds + 8ull * i;
    row[0] = box.lo[0]; row[1] = box.lo[1]; row[2] = box.lo[2];
    row[4] = box.hi[0]; row[5] = box.hi[1]; row[6] = box.hi[2];
}

// The direct form (DIRECT, up to CROSS_DIRECT_MAX_CHUNKS chunks): no tables, so no k_group launch.  The whole chunks strictly
// between a crossing node's two ends are read from the chunk totals themselves (level 0 of the first table, written by k_chunk
// before this launch).  The crossing nodes are a laminar family, so all their ranges together are about nchunks * log2(nchunks)
// boxes (47 k x 32 B at 1 M spheres) -- less than the tables k_group would write.  Min / max are idempotent: reading an entry
// twice (the clamped loads below) cannot change a bit.
constexpr u32 CROSS_SHORT = 8;                            // a range of at most this many chunks: the slot's own thread reads it
constexpr u32 CROSS_LIST = (256 / CROSS_CAP) * C;         // longer ranges of a workgroup, at most every node of its 8 chunks
constexpr u32 CROSS_DIRECT_MAX_CHUNKS = COL_MSD_MAX_N / C;

// chunk e's total box: level-0 entry e of the first table, [group][level][256]
__device__ __forceinline__ uint64_t chunk_total_at(u32 e) { return (uint64_t)(e / C) * (LV * C) + e % C; }

template <typename T>
__device__ __forceinline__ void cross_store(T *__restrict__ bounds, u32 i, const Box<T> &box) {
    // links (lane w) were written by k_chunk: store xyz only
    T *row = bounds + 8ull * i;
    row[0] = box.lo[0]; row[1] = box.lo[1]; row[2] = box.lo[2];
    row[4] = box.hi[0]; row[5] = box.hi[1]; row[6] = box.hi[2];
}

// CROSS_MID: the longest range one wave reads in a single round trip (CROSS_MID_U entries in flight per lane); anything longer is
// read by the whole workgroup, CrossU<T>::U entries per thread and round trip (the root of a 1 M scene: 3905 entries, 15.3 per thread)
template <typename T> struct CrossU { static constexpr u32 U = sizeof(T) == 4 ? 16 : 8; };
constexpr u32 CROSS_MID_U = 8, CROSS_MID = COL_WAVE * CROSS_MID_U;
struct CrossLds {
    uint2 list[CROSS_LIST];                       // (node, other end): wave-sized ranges from the front, longer ones from the back
    u32 nmid, nhuge;
    double part[256 / COL_WAVE][6];               // the waves' results for a huge node
};

// node i with a short range is finished here; a longer one is listed for the waves of the workgroup / the workgroup
template <typename T>
__device__ __forceinline__ void cross_direct(T *__restrict__ bounds, const u32 *__restrict__ other_end, const T *__restrict__ partial,
                                             const T *__restrict__ tab0, u32 i, CrossLds &lds) {
    const u32 j = other_end[i];
    const u32 first = min(i, j), last = max(i, j);
    const u32 a = first / C + 1, b = last / C;             // whole chunks [a, b) strictly between the two ends
    if (b < a) return;                                     // both ends in one chunk: k_chunk finished this node
    if (b - a > CROSS_MID) { lds.list[CROSS_LIST - 1 - atomicAdd(&lds.nhuge, 1u)] = make_uint2(i, j); return; }
    if (b - a > CROSS_SHORT) { lds.list[atomicAdd(&lds.nmid, 1u)] = make_uint2(i, j); return; }
    Box<T> box = box_load(partial, first);
    box_merge(box, box_load(partial, last));
    if (b > a) {
        Box<T> v[CROSS_SHORT];
#pragma unroll
        for (u32 k = 0; k < CROSS_SHORT; k++) v[k] = box_load(tab0, chunk_total_at(min(a + k, b - 1)));    // independent loads, one round trip
#pragma unroll
        for (u32 k = 0; k < CROSS_SHORT; k++) box_merge(box, v[k]);
    }
    cross_store(bounds, i, box);
}

template <typename T> __device__ __forceinline__ void box_wave_union(Box<T> &box) {
#pragma unroll
    for (int o = COL_WAVE / 2; o > 0; o >>= 1) {
        Box<T> r;
#pragma unroll
        for (int k = 0; k < 3; k++) { r.lo[k] = __shfl_xor(box.lo[k], o, COL_WAVE); r.hi[k] = __shfl_xor(box.hi[k], o, COL_WAVE); }
        box_merge(box, r);
    }
}

// entries e0, e0 + stride, ... (U of them, all loads issued before the first use; clamped to b - 1) merged into box
template <typename T, u32 U>
__device__ __forceinline__ void cross_batch(const T *__restrict__ tab0, u32 e0, u32 stride, u32 b, Box<T> &box) {
    Box<T> v[U];
#pragma unroll
    for (u32 k = 0; k < U; k++) v[k] = box_load(tab0, chunk_total_at(min(e0 + stride * k, b - 1)));
#pragma unroll
    for (u32 k = 0; k < U; k++) box_merge(box, v[k]);
}

// a listed node of up to CROSS_MID chunks, one per wave: one round trip
template <typename T>
__device__ __forceinline__ void cross_direct_wave(T *__restrict__ bounds, const T *__restrict__ partial,
                                                  const T *__restrict__ tab0, uint2 ij, u32 lane) {
    const u32 first = min(ij.x, ij.y), last = max(ij.x, ij.y);
    const u32 a = first / C + 1, b = last / C;
    Box<T> box = box_load(partial, first);
    box_merge(box, box_load(partial, last));
    cross_batch<T, CROSS_MID_U>(tab0, a + lane, COL_WAVE, b, box);
    box_wave_union(box);
    if (lane == 0) cross_store(bounds, ij.x, box);
}

// a listed node of more than CROSS_MID chunks, by the whole workgroup (uniform control flow: barriers inside)
template <typename T>
__device__ __forceinline__ void cross_direct_block(T *__restrict__ bounds, const T *__restrict__ partial,
                                                   const T *__restrict__ tab0, uint2 ij, CrossLds &lds) {
    constexpr u32 U = CrossU<T>::U;
    const u32 tid = threadIdx.x, lane = tid % COL_WAVE, w = tid / COL_WAVE;
    const u32 first = min(ij.x, ij.y), last = max(ij.x, ij.y);
    const u32 a = first / C + 1, b = last / C;
    Box<T> box = box_load(partial, first);
    box_merge(box, box_load(partial, last));
    for (u32 e0 = a; e0 < b; e0 += 256 * U) cross_batch<T, U>(tab0, e0 + tid, 256, b, box);      // (b - a > CROSS_MID: every thread has an entry)
    box_wave_union(box);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) { lds.part[w][k] = (double)box.lo[k]; lds.part[w][3 + k] = (double)box.hi[k]; }     // (exact: T is float or double)
    }
    __syncthreads();
    if (tid == 0) {
        for (u32 ww = 1; ww < 256 / COL_WAVE; ww++) {
            Box<T> o;
#pragma unroll
            for (int k = 0; k < 3; k++) { o.lo[k] = (T)lds.part[ww][k]; o.hi[k] = (T)lds.part[ww][3 + k]; }
            box_merge(box, o);
        }
        cross_store(bounds, ij.x, box);
    }
    __syncthreads();
}

// One thread per (chunk, list slot): CROSS_CAP threads per chunk instead of one per node -- a wave of the per-node version
// had one or two crossing nodes among its 64 and ran their table look-ups at that utilisation (76 us at 16 M spheres).
template <typename T, bool DIRECT = false>
__global__ __launch_bounds__(256) void k_cross(T *__restrict__ bounds, const u32 *__restrict__ other_end,
                                               const T *__restrict__ partial, const u32 *__restrict__ cross, Tabs tabs, u32 n,
                                               u32 nchunks, int lin, u32 *__restrict__ zero8, const u32 *__restrict__ n_dev,
                                               u32 *__restrict__ walk_order, u32 cross_blocks, int order_mode, u32 nzero) {
    const u32 n_bound = n;
    if (n_dev) { n = count_of(n, n_dev); nchunks = min(nchunks, (n + (u32)C - 1) / (u32)C); }
    if (blockIdx.x >= cross_blocks) {
        order_packets(blockIdx.x - cross_blocks, n, n_bound, walk_order, order_mode);
        return;
    }
    const u32 t = blockIdx.x * 256 + threadIdx.x;
    if (zero8 && t < nzero) zero8[t] = 0;      // the packet counters (or the whole chunk header) of the traversal that follows (bvh.hip), no launch of their own
    const u32 chunk = t / CROSS_CAP, slot = t % CROSS_CAP;
    if constexpr (DIRECT) {
        // every entry read below belongs to a chunk under the real chunk count: the ranges are those of real nodes
        // (listed by a real chunk's k_chunk workgroup, or i + 1 < n), and a node's last leaf is below n
        __shared__ CrossLds lds;
        const T *tab0 = (const T *)tabs.t[0];
        if (threadIdx.x == 0) { lds.nmid = 0; lds.nhuge = 0; }
        __syncthreads();
        if (chunk < nchunks) {
            if (cross[(uint64_t)chunk * CROSS_CAP + CROSS_CAP - 1] == CROSS_DENSE) {
                for (u32 k = slot; k < (u32)C; k += CROSS_CAP) {
                    const u32 i = chunk * C + k;
                    if (i + 1 < n) cross_direct(bounds, other_end, partial, tab0, i, lds);
                }
            } else {
                const u32 i = cross[(uint64_t)chunk * CROSS_CAP + slot];
                if (i != END) cross_direct(bounds, other_end, partial, tab0, i, lds);
            }
        }
        __syncthreads();
        const u32 nhuge = lds.nhuge, nmid = lds.nmid;
        for (u32 q = 0; q < nhuge; q++) cross_direct_block(bounds, partial, tab0, lds.list[CROSS_LIST - 1 - q], lds);
        for (u32 q = threadIdx.x / COL_WAVE; q < nmid; q += 256 / COL_WAVE)
            cross_direct_wave(bounds, partial, tab0, lds.list[q], threadIdx.x % COL_WAVE);
        return;
    }
    if (chunk >= nchunks) return;
    if (cross[(uint64_t)chunk * CROSS_CAP + CROSS_CAP - 1] == CROSS_DENSE) {
        for (u32 k = slot; k < (u32)C; k += CROSS_CAP) {
            const u32 i = chunk * C + k;
            if (i + 1 < n) cross_node(bounds, other_end, partial, tabs, i, lin);
        }
        return;
    }
    const u32 i = cross[(uint64_t)chunk * CROSS_CAP + slot];
    if (i != END) cross_node(bounds, other_end, partial, tabs, i, lin);
}

// col_debug_lbvh, process-wide: k_chunk_wide at every size / the walk order forced / the tables at every size
constexpr int DBG_WIDE = 1024, DBG_ORDER = 4096, DBG_TABLES = 32768;
int g_dbg = 0;
float g_block_k = 3.0f;   // leaf-block density criterion (col_debug_leaf_blocks): node width <= k x leaf width; 0 = no marks

struct Layout {
    size_t other_end, partial, cross, tab[3], total;
    u32 count[3];    // level-0 entries of each table: chunks, groups, groups of groups
};

Layout layout(uint32_t n, int coord_bytes) {
    Layout L;
    const size_t entry = 8 * (size_t)coord_bytes;       // two vec4 rows
    size_t off = 0;
    L.other_end = off; off += align256((size_t)n * 4);
    L.partial = off;   off += align256((size_t)n * entry);
    u32 cnt = (u32)col_ceil_div(n, C);
    L.cross = off;     off += align256((size_t)cnt * CROSS_CAP * 4);
    for (int h = 0; h < 3; h++) {
        L.count[h] = cnt;
        const size_t groups = col_ceil_div(cnt, C);
        L.tab[h] = off; off += align256(groups * LV * C * entry);
        cnt = (u32)groups;
    }
    L.total = off;
    return L;
}

template <typename T>
int run(hipStream_t s, const u32 *codes, const u32 *ids, const T *coords, const T *radii, const T *packed,
        col_node *nodes, T *bounds, char *scratch, u32 n, const col_walk_prep &w) {
    u32 *report_word = w.report_word;
    const Layout L = layout(n, sizeof(T));
    u32 *other_end = (u32 *)(scratch + L.other_end);
    T *partial = (T *)(scratch + L.partial);
    u32 *cross = (u32 *)(scratch + L.cross);
    Tabs tabs;
    for (int h = 0; h < 3; h++) tabs.t[h] = scratch + L.tab[h];
    const u32 nchunks = L.count[0];
    bool ordered_by_chunk = false;       // the production k_chunk orders the traversal's packets itself; otherwise k_cross does
    if (n < (1u << 30) && !(g_dbg & DBG_WIDE)) {
        // [order_packets workgroups][chunk and search workgroups: PLACES][report workgroup]
        const dim3 grid((w.walk_order ? 8u * COL_ORDER_SLICES : 0u) + place_blocks(nchunks) + (report_word ? 1u : 0u));
        if (nodes)
            k_chunk<T, true><<<grid, dim3(C), 0, s>>>(
                codes, ids, coords, radii, packed, nodes, bounds, other_end, partial, cross, (T *)tabs.t[0], n, (T)g_block_k, w.n_dev, w.walk_order, w.order_mode,
                report_word, w.report_n);
        else                            // no Node array asked for: the instance without its stores
            k_chunk<T, false><<<grid, dim3(C), 0, s>>>(
                codes, ids, coords, radii, packed, nullptr, bounds, other_end, partial, cross, (T *)tabs.t[0], n, (T)g_block_k, w.n_dev, w.walk_order, w.order_mode,
                report_word, w.report_n);
        ordered_by_chunk = true;
        report_word = nullptr;          // done in that launch
    } else if (nodes)
        k_chunk_wide<T, true><<<dim3(nchunks), dim3(C), 0, s>>>(codes, ids, coords, radii, packed, nodes, bounds, other_end, partial, cross,
                                                                 (T *)tabs.t[0], n, (T)g_block_k, w.n_dev);
    else
        k_chunk_wide<T, false><<<dim3(nchunks), dim3(C), 0, s>>>(codes, ids, coords, radii, packed, nullptr, bounds, other_end, partial, cross,
                                                                  (T *)tabs.t[0], n, (T)g_block_k, w.n_dev);
    COL_LAUNCH_OK();
    if (report_word) {                  // (k_chunk_wide has no report workgroup: the report's own launch)
        const int rc = col_radix_bucket_report((void *)s, codes, w.report_n, report_word);
        if (rc) return rc;
    }
    if (nchunks < 2) {                  // every node lives inside the single chunk: no k_cross, so clear the packet counters here
        if (w.zero) COL_HIP(hipMemsetAsync(w.zero, 0, w.nzero * sizeof(u32), s));
        return COL_OK;
    }
    const unsigned cross_blocks = (unsigned)col_ceil_div((uint64_t)nchunks * CROSS_CAP, 256);
    const dim3 cross_grid(cross_blocks + (w.walk_order && !ordered_by_chunk ? 8u * COL_ORDER_SLICES : 0u));
    if (nchunks <= CROSS_DIRECT_MAX_CHUNKS && !(g_dbg & DBG_TABLES)) {     // k_cross reads the chunk totals itself: no tables, no k_group
        k_cross<T, true><<<cross_grid, dim3(256), 0, s>>>(bounds, other_end, partial, cross, tabs, n, nchunks, -1, w.zero,
                                                          w.n_dev, w.walk_order, cross_blocks, w.order_mode, w.nzero);
        COL_LAUNCH_OK();
        return COL_OK;
    }
    int lin = -1;
    for (int h = 0; h < 3; h++) {
        if (h > 0 && L.count[h] <= LIN) { lin = h; break; }      // k_cross scans this level's few entries itself
        const u32 groups = (u32)col_ceil_div(L.count[h], C);
        k_group<T><<<dim3(groups), dim3(C), 0, s>>>((T *)tabs.t[h], L.count[h], h + 1 < 3 ? (T *)tabs.t[h + 1] : nullptr, n, w.n_dev, h);
        COL_LAUNCH_OK();
        if (groups < 2) break;
    }
    k_cross<T><<<cross_grid, dim3(256), 0, s>>>(bounds, other_end, partial, cross, tabs, n, nchunks, lin, w.zero,
                                                w.n_dev, w.walk_order, cross_blocks, w.order_mode, w.nzero);
    COL_LAUNCH_OK();
    return COL_OK;
}

}  // namespace

extern "C" {

int col_debug_lbvh(int mode) {
    if (mode & ~(DBG_WIDE | DBG_ORDER | DBG_TABLES)) return COL_EINVAL;
    g_dbg = mode;
    return COL_OK;
}
int col_lbvh_order_forced(void) { return (g_dbg & DBG_ORDER) ? 1 : 0; }
void col_debug_leaf_blocks(float k) { g_block_k = k; }

size_t col_lbvh_scratch_bytes(uint32_t n, int coord_bytes) { return layout(n, coord_bytes).total + 256; }

// `packed`: optional (x, y, z, r) rows indexed like coords (see col_morton_ex); coords/radii are then unused.
int col_lbvh_ex(void *stream, const uint32_t *codes, const uint32_t *ids, const void *coords, const void *radii,
                const void *packed, col_node *nodes, void *bounds, void *scratch, uint32_t n, int coord_bytes, const col_walk_prep &w) {
    if (n == 0) return COL_OK;
    if (n >= 0x80000000u || w.nzero > 256u) return COL_EINVAL;
    if (!scratch) return COL_ENOSCRATCH;
    if (coord_bytes == 4)
        return run<float>(col_stream(stream), codes, ids, (const float *)coords, (const float *)radii, (const float *)packed, nodes, (float *)bounds, (char *)scratch, n, w);
    if (coord_bytes == 8)
        return run<double>(col_stream(stream), codes, ids, (const double *)coords, (const double *)radii, (const double *)packed, nodes, (double *)bounds, (char *)scratch, n, w);
    return COL_EINVAL;
}

int col_lbvh(void *stream, const uint32_t *codes, const uint32_t *ids, const void *coords, const void *radii,
             col_node *nodes, void *bounds, void *scratch, uint32_t n, int coord_bytes) {
    return col_lbvh_ex(stream, codes, ids, coords, radii, nullptr, nodes, bounds, scratch, n, coord_bytes, col_walk_prep{});
}

}  // extern "C"
