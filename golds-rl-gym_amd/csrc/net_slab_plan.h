// How many slabs a split-M weight-gradient launch (gemm_tn) writes, and how many rows of M each one covers.  Plain C++ (no HIP), so
// that a host program can hold the rule to its inputs (tests/test_slab_plan.py).
#pragma once
#include <stddef.h>

namespace grl {

struct SlabPlan {
    int chunks;      // slabs = row ranges = grid.z of the launch; < 1: not even one slab fits the buffer
    int mc;          // rows per range, a multiple of 32; 0 when the rows are dealt to the ranges on the device
};

// wg_target / tiles workgroups' worth of ranges, at least min_chunks (short K loops where only part of the rows is live), at most 1024
// and at most what ONE request of the slab buffer can hold.  rows > 0: the ranges are mc rows each and chunks is what covers the rows
// at that mc.  rows == 0: the device deals the rows, chunks stays as sized.
// The cap of 1024 came with tn_launch and slot_wgrad_launch; the trunk-skip weight gradients of dense1 (per env), conv3 and conv2 were
// written without it.  It never binds there: their tiles are 196, 9 and 4, the target (GRL_TN_WGS) is <= 4096, and they have no floor.
inline SlabPlan slab_plan(int wg_target, int tiles, int min_chunks, int rows, size_t floats_per_chunk, size_t slab_floats) {
    int chunks = (wg_target + tiles - 1) / tiles;
    if (min_chunks > chunks) chunks = min_chunks;
    if (chunks > 1024) chunks = 1024;
    if ((size_t)chunks * floats_per_chunk > slab_floats) chunks = (int)(slab_floats / floats_per_chunk);
    if (chunks < 1 || rows == 0) return {chunks, 0};
    const int mc = ((rows + chunks - 1) / chunks + 31) / 32 * 32;
    return {(rows + mc - 1) / mc, mc};
}

}  // namespace grl
