/*
 * collision_hip_debug.h -- diagnostics entry points of libcollision_hip.so.  NOT part of the drop-in ABI
 * (include/collision_hip.h): nothing a maintainer of the reference binds.  They exist for bench.py's
 * roofline leg, for the counting traversal of collision_amd/stages.py, for tools/ and for the tests that force a code
 * path at a size where the library would not choose it.  The col_debug_* setters are PROCESS-WIDE and unsynchronised:
 * they change the host-side choice between production kernels (tile class, tree-build instance, packet order) for every
 * caller in the process; no kernel carries diagnostics code for them.  Set them from one thread while no work is in
 * flight; col_collide / col_collide_plan refuse to run under a forced tile class.  A setter returns COL_EINVAL for a
 * value it does not list and leaves its state unchanged.  (An experiment is an A/B of two builds: tools/ab_builds.sh.)
 */
#ifndef COLLISION_HIP_DEBUG_H
#define COLLISION_HIP_DEBUG_H

#include "collision_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

int col_debug_xcc_census(void *stream, uint32_t *out, uint32_t nblocks);   /* diagnostics: XCC id per workgroup */
int col_debug_traverse(int variant);    /* 0 = default; 32768: col_collide's dynamic packet order at every size instead of from
                                         * 400 000 spheres on (tests) */
int col_debug_lbvh(int mode);           /* 0 = default, or a sum of: 1024: k_chunk_wide, the tree build's 64-bit-index chunk kernel,
                                         * which otherwise serves n >= 2^30 only, at every size (tests); 4096: the traversal's
                                         * longest-first walk order whatever the scene (tests); 32768: k_group's tables and
                                         * k_cross's table look-ups at every size, instead of the direct unions up to the MSD size range
                                         * (tests) */
void col_debug_leaf_blocks(float k);    /* leaf-block criterion of the fused LBVH build, process-wide: a node of <= 16 leaves is marked when it is at
                                         * most k leaf boxes wide on every axis; default 3, 0 = no marks, a huge k = every small node */
int col_debug_radix_tile(int tile);     /* force the tile class (1024, 4096, 8192, 16384; 0 = automatic).  Set it BEFORE sizing
                                           scratch with col_radix_scratch_bytes / col_radix_tile: the histogram layout follows it. */
int col_lbvh_order_forced(void);        /* 1 while col_debug_lbvh bit 4096 is set: col_collide then takes order_mode 1 at every size */
int col_radix_tile_override_active(void);   /* 1 while col_debug_radix_tile forces a tile class */
/* copies `bytes` (a multiple of 128 KiB) from `in` to `out`: shape 0 = float4 copy, one vector per thread; shape 1 = the scatter
 * pass's tile shape (64 KB per 512-thread workgroup through LDS, coalesced stores) without any ranking: bench.py's
 * roofline.copy_ceiling, measured beside the pass */
int col_debug_copy(void *stream, const void *in, void *out, uint64_t bytes, int shape);
/* Diagnostics build of the traversal -- same pairs, same counter semantics -- that also counts its work.
 * stats: 8 x uint64, zeroed by the caller (steps, descents, leaf tests, leaf hits, steps within 1k/2k/4k/8k positions
 * of the block start) */
int col_traverse_stats(void *stream, uint32_t *pairs, uint32_t *counter, uint32_t capacity,
                       const void *bounds, uint32_t n, int coord_bytes, uint64_t *stats, int mode);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* COLLISION_HIP_DEBUG_H */
