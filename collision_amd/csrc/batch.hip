// Batched collider: B independent small scenes, concatenated in the caller's arrays, in one kernel launch.
// Scene s gets what Collider.get_collisions (collision/collision.py:130-198) gives for that scene alone: its own
// scene bounds, its own 30-bit Morton codes, its own stable sort, its own pair list -- nothing is shared between scenes.
//
// k_batch<T, NT, SPW>: a workgroup of NT * SPW threads holds SPW scenes of at most NT spheres each, one sphere per
// thread, and the whole pipeline stays in LDS:
//   1. min / max of the scene's centres (wave shuffles, then one LDS row per wave);
//   2. Morton codes with quantize() of col_common.h -- the arithmetic of k_morton_tile (IEEE divide, no contraction;
//      a degenerate axis gives 0 / 0 = NaN and so code 0);
//   3. a stable RANK sort: key = code << 10 | local id (distinct keys), rank = number of smaller keys of the scene,
//      every key read as an LDS broadcast.  n key compares per sphere is a fraction of what step 4 costs;
//      a radix sort of 30-bit keys would need four ranking passes with their barriers for at most 1024 keys;
//   4. pair finding as a sweep over the sorted leaf boxes (c - r, c + r in the coordinate type): the thread at sorted
//      position q tests every p > q, the box of p read as an LDS broadcast (p is wave-uniform; 16-byte aligned records:
//      two / three ds_read_b128 per box).  The oracle's walk reports exactly the pairs q < p whose leaf boxes overlap (an
//      ancestor's box contains its leaves' boxes exactly), so no tree is needed for the same pair set, and a scene of
//      at most 1024 boxes has no room for a tree to pay: n (n - 1) / 2 strict AABB tests (collision.cl:164-166) per scene;
//   5. output: hits are staged in a workgroup-wide LDS list (slot from an LDS counter), ONE atomic on the pair counter
//      per workgroup reserves the list space of all its scenes, and the list is flushed with consecutive threads storing
//      consecutive rows.  A workgroup with more hits than the list holds (4 per sphere: dense and degenerate scenes)
//      scans its threads' hit counts instead and every thread walks its row again, storing its pairs itself.
// Every barrier is in uniform control flow: empty, skipped and missing scenes walk through the same sequence.
#include "col_common.h"

namespace {

template <typename T> struct alignas(4 * sizeof(T)) BVec4 { T x, y, z, w; };
template <> struct alignas(16) BVec4<double> { double x, y, z, w; };

// A leaf box as the sweep reads it: whole 16-byte LDS words (ds_read_b128, 4 LDS cycles; a 12-byte read takes 8).
// float: two words, and their fourth lanes carry what the sweep needs besides the box -- the box's sorted position (as a
// float: exact below 2^24), compared in the same breath as the coordinates, and the sphere's local id for a hit -- so both
// words are read whole.  double: three words, position and id stay outside (the loop counter, s_id).
template <typename T> struct Box;
template <> struct alignas(16) Box<float> { float lo[3], pos, hi[3], idf; };
template <> struct alignas(16) Box<double> { double lo[3], hi[3]; };

// collision.cl:164-166 checkOverlap(query a, other b): strict on all three axes
template <typename T> __device__ __forceinline__ bool box_overlap(const Box<T> &a, const Box<T> &b) {
    return (a.hi[0] > b.lo[0]) & (a.lo[0] < b.hi[0]) & (a.hi[1] > b.lo[1]) & (a.lo[1] < b.hi[1]) & (a.hi[2] > b.lo[2]) &
           (a.lo[2] < b.hi[2]);
}
// is b, read from sorted position p, behind the query a at position t?
__device__ __forceinline__ bool box_behind(const Box<float> &a, const Box<float> &b, u32 t, u32 p) { return b.pos > a.pos; }
__device__ __forceinline__ bool box_behind(const Box<double> &a, const Box<double> &b, u32 t, u32 p) { return p > t; }
// the local id of the sphere whose box b was read from sorted position p (ids: the scene's sorted ids)
__device__ __forceinline__ u32 box_id(const Box<float> &b, const unsigned short *ids, u32 p) { return __float_as_uint(b.idf); }
__device__ __forceinline__ u32 box_id(const Box<double> &b, const unsigned short *ids, u32 p) { return ids[p]; }
__device__ __forceinline__ void box_tag(Box<float> &b, u32 pos, u32 id) { b.pos = (float)pos; b.idf = __uint_as_float(id); }
__device__ __forceinline__ void box_tag(Box<double> &b, u32 pos, u32 id) {}

constexpr u32 SWEEP = 4;            // boxes per round of the sweep

template <typename T, int NT, int SPW>
__global__ __launch_bounds__(NT *SPW) void k_batch(const BVec4<T> *__restrict__ coords, const T *__restrict__ radii,
                                                   const u32 *__restrict__ offsets, u32 n_scenes, u32 total, u32 max_scene,
                                                   u32 *__restrict__ codes_out, u32 *__restrict__ ids_out,
                                                   u32 *__restrict__ counter, u32 *__restrict__ scene_counts,
                                                   u32 *__restrict__ pairs, u32 capacity) {
    constexpr int BT = NT * SPW, NW = BT / 64, WPS = NT / 64;      // threads, waves, waves per scene
    constexpr u32 STAGE = 4 * BT;                                  // staged hits per workgroup
    static_assert(NT % 64 == 0 && NT <= 1024 && BT <= 1024, "a wave never spans two scenes; positions fit 10 bits");
    __shared__ Box<T> s_box[BT + SWEEP];         // leaf boxes in sorted order (+ what the last round of a sweep reads past them)
    // the keys of the sort (code << 10 | local id, in input order), then -- they are dead by then -- the staged hits
    // (position of q in the workgroup << 10 | local id of p)
    __shared__ __attribute__((aligned(16))) u32 s_stage[STAGE];
    u64 *s_key = reinterpret_cast<u64 *>(s_stage);
    __shared__ unsigned short s_id[BT];          // local ids in sorted order
    __shared__ T s_fold[NW][6];
    __shared__ u32 s_ws[NW];
    __shared__ u32 s_o0[SPW];
    __shared__ u32 s_base, s_staged;
    const u32 tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const u32 slot = (u32)__builtin_amdgcn_readfirstlane((int)(tid / NT)), t = tid % NT;
    const u32 s = blockIdx.x * SPW + slot;

    // ---- the scene of this slot (wave-uniform)
    u32 o0 = 0, n = 0;
    bool skipped = false;
    if (s < n_scenes) {
        o0 = offsets[s];
        const u32 o1 = offsets[s + 1];
        n = o1 - o0;
        skipped = o0 > o1 || n > max_scene || o1 > total;      // rows [o0, o1) of a scene that runs lie inside [0, total)
        if (skipped) n = 0;
    }
    o0 = (u32)__builtin_amdgcn_readfirstlane((int)o0);
    n = (u32)__builtin_amdgcn_readfirstlane((int)n);
    const bool live = t < n;
    const u32 sb = slot * NT;               // this scene's part of the LDS arrays
    if (t == 0) s_o0[slot] = o0;
    if (tid == 0) s_staged = 0;

    // ---- 1. scene bounds
    T x = 0, y = 0, z = 0, r = 0;
    if (live) {
        const BVec4<T> c = coords[(size_t)o0 + t];
        x = c.x; y = c.y; z = c.z;
        r = radii[(size_t)o0 + t];
    }
    T acc[6] = {live ? x : (T)INFINITY, live ? y : (T)INFINITY, live ? z : (T)INFINITY,
                live ? x : -(T)INFINITY, live ? y : -(T)INFINITY, live ? z : -(T)INFINITY};
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const T lo = __shfl_xor(acc[k], o, 64), hi = __shfl_xor(acc[3 + k], o, 64);
            acc[k] = lo < acc[k] ? lo : acc[k];
            acc[3 + k] = hi > acc[3 + k] ? hi : acc[3 + k];
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 6; k++) s_fold[w][k] = acc[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 6; k++) acc[k] = s_fold[slot * WPS][k];
    for (int ww = 1; ww < WPS; ww++) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const T lo = s_fold[slot * WPS + ww][k], hi = s_fold[slot * WPS + ww][3 + k];
            acc[k] = lo < acc[k] ? lo : acc[k];
            acc[3 + k] = hi > acc[3 + k] ? hi : acc[3 + k];
        }
    }

    // ---- 2. Morton code, 3. stable rank sort
    const u32 code = morton30(x, y, z, acc[0], acc[1], acc[2], acc[3], acc[4], acc[5]);
    const u64 key = ((u64)code << 10) | t;
    s_key[tid] = key;
    __syncthreads();
    // positions from n on (and the SWEEP records behind the last scene) hold EMPTY boxes (lo = +inf, hi = -inf: nothing
    // overlaps them): the sweep reads whole rounds, and no thread's query is uninitialised memory
    Box<T> b;
#pragma unroll
    for (int k = 0; k < 3; k++) { b.lo[k] = (T)INFINITY; b.hi[k] = -(T)INFINITY; }
    box_tag(b, BT + tid, 0u);
    if (tid < SWEEP) s_box[BT + tid] = b;
    u32 rank = t;
    if (live) {
        const u64 *kp = s_key + sb;
        rank = 0;
#pragma unroll 8
        for (u32 j = 0; j < n; j++) rank += kp[j] < key ? 1u : 0u;
        b.lo[0] = x - r; b.lo[1] = y - r; b.lo[2] = z - r;
        b.hi[0] = x + r; b.hi[1] = y + r; b.hi[2] = z + r;
        if (codes_out) codes_out[(size_t)o0 + rank] = code;
        if (ids_out) ids_out[(size_t)o0 + rank] = t;
    }
    box_tag(b, rank, t);
    s_box[sb + rank] = b;
    s_id[sb + rank] = (unsigned short)t;
    __syncthreads();                        // the boxes are in place, and every key has been read: its words become the staged list

    // ---- 4. the sweep: this thread is the query at sorted position t
    const Box<T> *bp = s_box + sb;
    const unsigned short *idp = s_id + sb;
    const Box<T> a = bp[t];
    u32 cnt = 0;
    const u32 pstart = (u32)__builtin_amdgcn_readfirstlane((int)(t & ~63u)) + 1u;
    // SWEEP boxes per round: their reads are in flight together and the wave branches once, on "any hit in the round"
    for (u32 p0 = pstart; p0 < n; p0 += SWEEP) {
        Box<T> c[SWEEP];
        bool hit[SWEEP], any = false;
#pragma unroll
        for (u32 k = 0; k < SWEEP; k++) {
            c[k] = bp[p0 + k];
            const bool behind = box_behind(a, c[k], t, p0 + k), over = box_overlap(a, c[k]);
            hit[k] = behind & over & (p0 + k < n);      // (a full scene's last round reads into the NEXT scene's boxes)
            any |= hit[k];
        }
        if (any) {
#pragma unroll
            for (u32 k = 0; k < SWEEP; k++) {
                if (hit[k]) {
                    const u32 e = atomicAdd(&s_staged, 1u);
                    if (e < STAGE) s_stage[e] = (tid << 10) | box_id(c[k], idp, p0 + k);
                    cnt++;
                }
            }
        }
    }

    // ---- 5. list space: one atomic per workgroup
    const u32 incl = wave_incl_scan(cnt);
    if (lane == 63) s_ws[w] = incl;
    __syncthreads();
    u32 before = 0, scene_total = 0, block_total = 0;
#pragma unroll
    for (int i = 0; i < NW; i++) {
        const u32 v = s_ws[i];
        block_total += v;
        if ((u32)i < w) before += v;
        if ((u32)i / WPS == slot) scene_total += v;
    }
    if (tid == 0) s_base = block_total ? atomicAdd(counter, block_total) : 0u;
    if (t == 0 && s < n_scenes) scene_counts[s] = skipped ? COL_BATCH_SKIPPED : scene_total;
    __syncthreads();
    const u64 base = s_base;
    if (base >= capacity) return;
    if (block_total <= STAGE) {             // the staged list holds every hit: consecutive threads, consecutive rows
        for (u32 i = tid; i < block_total; i += BT) {
            const u64 row = base + i;
            if (row >= capacity) break;
            const u32 e = s_stage[i], q = e >> 10;      // q's position in the workgroup, p's local id
            const u32 off = s_o0[q / NT];
            pairs[2 * row] = off + s_id[q];
            pairs[2 * row + 1] = off + (e & 1023u);
        }
        return;
    }
    // more hits than the list holds: this thread's rows start at its place in the scan (waves are in scene order)
    u64 row = base + before + (incl - cnt);
    if (cnt == 0 || row >= capacity) return;
    const u32 idq = s_id[sb + t];
    for (u32 p = t + 1; p < n; p++) {
        if (box_overlap(a, bp[p])) {
            if (row >= capacity) return;
            pairs[2 * row] = o0 + idq;
            pairs[2 * row + 1] = o0 + s_id[sb + p];
            row++;
        }
    }
}

template <typename T, int NT, int SPW>
int launch_batch(hipStream_t st, const void *coords, const void *radii, const u32 *offsets, u32 n_scenes, u32 total, u32 max_scene,
                 u32 *codes_out, u32 *ids_out, u32 *counter, u32 *scene_counts, u32 *pairs, u32 capacity) {
    const dim3 grid((unsigned)col_ceil_div(n_scenes, SPW)), block(NT * SPW);
    k_batch<T, NT, SPW><<<grid, block, 0, st>>>((const BVec4<T> *)coords, (const T *)radii, offsets, n_scenes, total, max_scene,
                                                 codes_out, ids_out, counter, scene_counts, pairs, capacity);
    COL_LAUNCH_OK();
    return COL_OK;
}

// the size class: the smallest instance whose scenes hold max_scene spheres
template <typename T>
int batch_class(hipStream_t st, const void *coords, const void *radii, const u32 *offsets, u32 n_scenes, u32 total, u32 max_scene,
                u32 *codes_out, u32 *ids_out, u32 *counter, u32 *scene_counts, u32 *pairs, u32 capacity) {
    if (max_scene <= 64)
        return launch_batch<T, 64, 8>(st, coords, radii, offsets, n_scenes, total, max_scene, codes_out, ids_out, counter, scene_counts, pairs, capacity);
    if (max_scene <= 256)
        return launch_batch<T, 256, 4>(st, coords, radii, offsets, n_scenes, total, max_scene, codes_out, ids_out, counter, scene_counts, pairs, capacity);
    if (max_scene <= 512)
        return launch_batch<T, 512, 2>(st, coords, radii, offsets, n_scenes, total, max_scene, codes_out, ids_out, counter, scene_counts, pairs, capacity);
    return launch_batch<T, 1024, 1>(st, coords, radii, offsets, n_scenes, total, max_scene, codes_out, ids_out, counter, scene_counts, pairs, capacity);
}

}  // namespace

extern "C" {

uint32_t col_collide_batch_max_scene(int coord_bytes) { return coord_bytes == 4 || coord_bytes == 8 ? 1024u : 0u; }

// everything lives in LDS: no scratch (the argument stays in the ABI for an instance that needs some)
size_t col_collide_batch_scratch_bytes(uint32_t n_scenes, uint32_t total, uint32_t max_scene, int coord_bytes) {
    (void)n_scenes; (void)total; (void)max_scene; (void)coord_bytes;
    return 0;
}

int col_collide_batch(void *stream, const void *coords, const void *radii, const uint32_t *offsets, uint32_t n_scenes,
                      uint32_t total, uint32_t max_scene, int coord_bytes, uint32_t *codes_out, uint32_t *ids_out, void *scratch,
                      uint32_t *counter, uint32_t *scene_counts, uint32_t *pairs, uint32_t capacity) {
    (void)scratch;
    if (coord_bytes != 4 && coord_bytes != 8) return COL_EINVAL;
    if (max_scene == 0 || max_scene > col_collide_batch_max_scene(coord_bytes)) return COL_EINVAL;
    if (!pairs && capacity > 0) return COL_EINVAL;
    if (!counter || !scene_counts || !offsets) return COL_EINVAL;
    if (n_scenes == 0) return COL_OK;
    hipStream_t st = col_stream(stream);
    COL_HIP(hipMemsetAsync(counter, 0, sizeof(uint32_t), st));      // launch 1 of 2; scene_counts: every word is stored by the kernel
    if (coord_bytes == 4)
        return batch_class<float>(st, coords, radii, offsets, n_scenes, total, max_scene, codes_out, ids_out, counter, scene_counts, pairs, capacity);
    return batch_class<double>(st, coords, radii, offsets, n_scenes, total, max_scene, codes_out, ids_out, counter, scene_counts, pairs, capacity);
}

}  // extern "C"
