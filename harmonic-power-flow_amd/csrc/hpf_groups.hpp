// The split of a batch's slots over the scenario groups (one stream each, hpf_lib.hip: enqueue_iterations): how many groups a count of slots
// gets and where each begins.  Batch results stay bit-identical only while every caller splits alike, so this is the one copy.  Plain C++ (no
// HIP): the host tests compile it on its own.
#pragma once

namespace hpf {

// groups of `count` slots of a handle set to n_groups: only the radial block-tree step runs in groups
inline int group_count(bool radial_block_tree, int n_groups, int count) {
    if (!radial_block_tree) return 1;
    int g = n_groups;
    while (g > 1 && count < 32 * g) --g;       // at least 32 scenarios per group (below that the launches of a group no longer fill their levels: tools/groups_sweep.py)
    return g < 1 ? 1 : g;
}

// first slot of group g of G (g >= G: count).  Boundaries on multiples of 16 slots: the scenario-batched workgroups of the tree kernels take 16
// scenarios each, an even split of e.g. 128 into 43 + 43 + 42 would run 3 x 3 tiles with ragged ends instead of 3 + 2 + 3 full ones
inline int group_bound(int count, int G, int g) {
    return g >= G ? count : (int)(16 * (((long long)count * g / G + 8) / 16));
}

}  // namespace hpf
