// col_collide: the whole path -- bounds, Morton codes, sort, tree, walk -- as one chain of launches.  Host code only: the
// kernels live in reduce.hip, morton.hip, radix.hip, lbvh.hip and bvh.hip, behind include/collision_hip.h and col_common.h.
#include "col_common.h"

namespace {

// The whole path's scratch: offsets from its 256-byte aligned base (callers pass aligned buffers, collision_hip.h; `total`
// allows for one that is not).  The size query and the carve both read this table; nothing else adds up sizes.
struct CollideLayout {
    size_t reduce, sort, lbvh, packed, walk, walk_sched, walk_order, msd, total;
};
CollideLayout collide_layout(uint32_t n, uint32_t padded, int coord_bytes) {
    CollideLayout L;
    L.reduce = 256;                // the bounds partials, behind 256 unused bytes (once the scene's range, which the Morton kernel now folds itself)
    L.sort = align256(L.reduce + col_reduce_scratch_bytes(coord_bytes == 8 ? COL_F64 : COL_F32, 4));      // histogram first
    L.lbvh = align256(L.sort + col_radix_scratch_bytes(padded, 4, 4));
    L.packed = align256(L.lbvh + col_lbvh_scratch_bytes(n, coord_bytes));      // (x, y, z, r) rows
    L.walk = align256(L.packed + (size_t)n * 4 * coord_bytes);                 // the chunked walk's header |
    L.walk_sched = L.walk + col_traverse_chunked_scratch_bytes();              // 256 bytes of packet counters |
    L.walk_order = L.walk_sched + 256;                                         // cost[] and perm[] (col_common.h)
    L.msd = align256(L.walk_order + 8 * ((size_t)n / 64 + 1) + 256);           // the MSD plan's group sums + bucket starts
    L.total = L.msd + col_radix_msd_fused_bytes() + 255;
    return L;
}

}  // namespace

extern "C" {

size_t col_collide_scratch_bytes(uint32_t n, uint32_t padded, int coord_bytes) { return collide_layout(n, padded, coord_bytes).total; }

int col_collide(void *stream, const void *coords, const void *radii, uint32_t n, uint32_t padded, int coord_bytes,
                uint32_t *codes0, uint32_t *codes1, uint32_t *ids0, uint32_t *ids1, col_node *nodes, void *bounds,
                uint32_t *flags, void *scratch, uint32_t *counter, uint32_t *pairs, uint32_t capacity) {
    return col_collide_plan_dev(stream, coords, radii, n, padded, coord_bytes, codes0, codes1, ids0, ids1, nodes, bounds, flags,
                                scratch, counter, pairs, capacity, COL_SORT_LSD, nullptr, nullptr, 0, nullptr);
}

int col_collide_plan(void *stream, const void *coords, const void *radii, uint32_t n, uint32_t padded, int coord_bytes,
                     uint32_t *codes0, uint32_t *codes1, uint32_t *ids0, uint32_t *ids1, col_node *nodes, void *bounds,
                     uint32_t *flags, void *scratch, uint32_t *counter, uint32_t *pairs, uint32_t capacity,
                     int sort_plan, uint32_t *oversize) {
    return col_collide_plan_dev(stream, coords, radii, n, padded, coord_bytes, codes0, codes1, ids0, ids1, nodes, bounds, flags,
                                scratch, counter, pairs, capacity, sort_plan, oversize, nullptr, 0, nullptr);
}

// col_collide_plan with the bounds partials of `coords` already computed (col_minmax4_stage1_dev: `parts` records of
// [min row, max row] at `partials`; NULL = compute them here).
int col_collide_plan_partials(void *stream, const void *coords, const void *radii, uint32_t n, uint32_t padded, int coord_bytes,
                              uint32_t *codes0, uint32_t *codes1, uint32_t *ids0, uint32_t *ids1, col_node *nodes, void *bounds,
                              uint32_t *flags, void *scratch, uint32_t *counter, uint32_t *pairs, uint32_t capacity,
                              int sort_plan, uint32_t *oversize, const void *partials, uint32_t parts) {
    return col_collide_plan_dev(stream, coords, radii, n, padded, coord_bytes, codes0, codes1, ids0, ids1, nodes, bounds, flags, scratch,
                                counter, pairs, capacity, sort_plan, oversize, partials, parts, nullptr);
}

// The whole path with the number of spheres ON THE DEVICE (include/collision_hip.h): n is a host-known bound that sizes grids,
// scratch and the sort (rows from *n_dev on become pads), every kernel works on min(n, *n_dev).  Needs the bounds partials
// (col_minmax4_stage1_dev reads the same word).
int col_collide_plan_dev(void *stream, const void *coords, const void *radii, uint32_t n, uint32_t padded, int coord_bytes,
                         uint32_t *codes0, uint32_t *codes1, uint32_t *ids0, uint32_t *ids1, col_node *nodes, void *bounds,
                         uint32_t *flags, void *scratch, uint32_t *counter, uint32_t *pairs, uint32_t capacity,
                         int sort_plan, uint32_t *oversize, const void *partials, uint32_t parts, const uint32_t *n_dev) {
    if (coord_bytes != 4 && coord_bytes != 8) return COL_EINVAL;
    if (n_dev && !partials) return COL_EINVAL;
    if (partials && (parts == 0 || parts > COL_MINMAX_PARTS)) return COL_EINVAL;
    if (padded < n || (capacity > 0 && !pairs)) return COL_EINVAL;
    if (!scratch) return COL_ENOSCRATCH;
    // a forced radix tile class (diagnostics) would not match the histogram the fused Morton kernel writes
    if (col_radix_tile_override_active()) return COL_EINVAL;
    hipStream_t s = col_stream(stream);
    if (n == 0) {
        COL_HIP(hipMemsetAsync(counter, 0, sizeof(uint32_t), s));             // collision.py:151-154
        return COL_OK;
    }
    (void)flags;   // the arrival counters of internalBounds (collision.py:147-150) are not needed: see lbvh.hip
    const CollideLayout L = collide_layout(n, padded, coord_bytes);
    char *base = (char *)align256((uintptr_t)scratch);
    void *red_scratch = base + L.reduce, *sort_scratch = base + L.sort, *packed = base + L.packed;
    uint32_t *msd_fused = (uint32_t *)(base + L.msd);
    // sort_plan: bit 0 = the sort (COL_SORT_LSD / COL_SORT_MSD), bit 1 = COL_TRAVERSE_CHUNKED (dense scenes)
    const bool chunked = (sort_plan & COL_TRAVERSE_CHUNKED) != 0;
    sort_plan &= 1;
    uint32_t *publish = oversize ? oversize + 2 : nullptr;      // the previous call's pair count, for the caller's next choice
    int rc;
    // The front end is fused for every tile class of a (u32, u32) sort (col_radix_tile without a forced class: 1024, 4096
    // or 8192): the Morton kernel folds the bounds partials itself and counts the digits of the sort's first pass (the
    // histogram sits at the start of the sort scratch): two launches less.
    const uint32_t tile = col_radix_tile(padded, 4, 4);
    if (tile != 1024 && tile != 4096 && tile != 8192) return COL_EINVAL;
    // The MSD plan applies up to COL_MSD_MAX_N, without a scan launch (col_radix_sort_msd_fused: the Morton kernel also adds its
    // counts into group sums, cleared by the bounds kernel when it runs here, else by a memset); the 1024-pair tile class has no
    // global pass either (col_radix_sort_msd_gather: the Morton kernel leaves every tile sorted by the bucket digit).
    const bool msd = sort_plan == COL_SORT_MSD && padded <= COL_MSD_MAX_N;
    const bool gather = msd && tile == 1024;
    const uint32_t mtile = gather && padded >= COL_GATHER_BIG_FROM ? 4096u : tile;      // the Morton kernel's tile (col_common.h)
    const uint32_t nsums = msd ? (uint32_t)(col_radix_msd_fused_bytes() / sizeof(uint32_t)) : 0u;
    if (msd && col_ceil_div(padded, tile) > (uint64_t)COL_MSD_GROUP * COL_MSD_GROUPS) return COL_EINVAL;    // (more tiles than group sums: no tile class does that)
    if (!partials) {
        if ((rc = col_minmax4_stage1_zero(stream, coords, n, coord_bytes, red_scratch, &parts, msd_fused, nsums))) return rc;
        partials = red_scratch;
    } else if (msd)
        COL_HIP(hipMemsetAsync(msd_fused, 0, nsums * sizeof(uint32_t), s));
    if ((rc = col_morton_tile(stream, coords, radii, partials, parts, n, padded, coord_bytes, codes0, ids0, packed,
                              counter, (uint32_t *)sort_scratch, mtile, (uint32_t)col_ceil_div(padded, mtile), msd ? 22 : 0,
                              publish, n_dev, msd ? msd_fused : nullptr, gather ? 1 : 0))) return rc;
    if (gather) rc = col_radix_sort_msd_gather(stream, codes0, codes1, ids0, ids1, n, padded, sort_scratch, oversize, n_dev, msd_fused, mtile);
    else if (msd) rc = col_radix_sort_msd_fused(stream, codes0, codes1, ids0, ids1, padded, sort_scratch, oversize, n_dev, msd_fused);
    else rc = col_radix_sort_ex(stream, codes0, codes1, ids0, ids1, padded, 4, 4, sort_scratch, 0, 1);
    if (rc) return rc;
    // How the walk is scheduled, and what the tree build's last launch prepares for it (col_walk_prep).  The exact walk takes
    // its packets in dynamic order (`sched`: eight counters) where col_traverse_dynamic_order(n) says so (bvh.hip, with the
    // measurements); the chunked walk always does, with the counters in its header.  WALK ORDER (col_common.h): a dense scene --
    // chunked, or col_debug_lbvh's bit -- orders its walks longest first (order_mode 1), a sparse one of up to COL_DEAL_MAX_N
    // spheres under the dynamic order only deals its long walks over the first round, larger sparse scenes record and order
    // nothing; never for a tree of one chunk (no k_cross).  The build clears what the walk counts in: the chunked walk's
    // 64-byte header (its memset was a launch of 4.8 us), else the eight packet counters.
    uint32_t *sched = !chunked && col_traverse_dynamic_order(n) ? (uint32_t *)(base + L.walk_sched) : nullptr;
    col_walk_prep w;
    w.order_mode = chunked || col_lbvh_order_forced() ? 1 : 0;
    if (n > 256 && (chunked || (sched && (n <= COL_DEAL_MAX_N || w.order_mode)))) w.walk_order = (uint32_t *)(base + L.walk_order);
    w.zero = chunked ? (uint32_t *)(base + L.walk) : sched;
    w.nzero = chunked ? 16u : 8u;
    w.n_dev = n_dev;
    // the LSD plan was taken where the MSD plan could apply: tell the caller how clustered the codes are (oversize[1]);
    // the report rides in the tree build's first launch (lbvh.hip)
    if (!msd && oversize && padded <= COL_MSD_MAX_N) w.report_word = oversize + 1;
    w.report_n = padded;
    if ((rc = col_lbvh_ex(stream, codes1, ids1, coords, radii, packed, nodes, bounds, base + L.lbvh, n, coord_bytes, w))) return rc;
    if (chunked)
        return col_traverse_chunked_walk(stream, pairs, counter, capacity, bounds, n, coord_bytes, base + L.walk, n_dev, w.walk_order, 1);
    if (n < 2) return COL_OK;
    return col_traverse_walk(stream, pairs, counter, capacity, bounds, n, coord_bytes, sched, n_dev, w.walk_order);
}

}  // extern "C"
