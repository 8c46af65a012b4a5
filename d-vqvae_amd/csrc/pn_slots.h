// Slots, ids and groups of the filtered PointNet trunk (pointnet_filter.hip): which point a (wave, lane, accumulator register) of
// pn_trunk_filter_kernel scores, the id the top-two chain leaves in a score's low mantissa bits, and the sixteen points of a flagged
// group -- shared by the trunk kernel and pn_exact_kernel, and compiled for the host by tests/test_pointnet_trunk_layout.py.
//
// A tile has 256 slots = 4 waves x 4 row blocks of 16 points (slot = 64 wave + 16 rb + row).  conv1 / conv2 see a wave's 64 points as
// two 32-point blocks (pb = rb >> 1; lanes l and l + 32 work on point 32 pb + (l & 31)); conv3 runs v_mfma_f32_16x16x32_f16 per row
// block and 16-channel column block: lane (quarter q = lane >> 4, column lane & 15) holds, for ONE channel, the scores of rows
// 4 q + e (e = 0 .. 3: accumulator register) of every row block -- sixteen scores per column block, one top-two chain, one GROUP
// (wave, quarter).  The tail tile is one 32-point block per wave: row blocks 0 and 1; the slots of row blocks 2 and 3 repeat them.
#pragma once
#if defined(__HIPCC__) || defined(__CUDACC__)
#define PN_SLOTS_FN __host__ __device__ inline
#else
#define PN_SLOTS_FN inline
#endif

constexpr int PN_TILE_SLOTS = 256;                         // slots of a tile
constexpr int PN_TAIL_SLOTS = 32;                          // points of a tail tile (1 .. 32 points beyond a multiple of 256)
constexpr int PN_GROUPS = 16;                              // 16-point groups of a tile: 4 waves x 4 lane quarters

// Points are dealt to the tiles round robin and to the 256 slots of a tile through a multiplicative permutation: neighbours in
// the cloud's order -- often neighbours in space, i.e. near ties -- land in different waves.  ``deal`` tiles share the first
// 256 * deal points this way.  A cloud with 1 .. 32 points beyond a multiple of 256 (the 778 hand vertices: 3 * 256 + 10) gets them
// as a TAIL tile (index deal) of ONE 32-point block instead of a fourth full tile that is three quarters padding: point
// 256 * deal + (slot & 31) (callers fold indices >= N back with % N, as for every padding slot).
PN_SLOTS_FN int point_of_slot(int tile, int slot, int deal) {
    return tile < deal ? ((slot * 67) & 255) * deal + tile : 256 * deal + (slot & 31);
}
// slot of (wave, row block, lane quarter, accumulator register)
PN_SLOTS_FN int pn_slot(int wave, int rb, int q, int e) { return 64 * wave + 16 * rb + 4 * q + e; }
// the id the chain writes (bits [3:0]: row block, register) and the id of a published score: + [5:4] lane quarter, [7:6] wave
PN_SLOTS_FN unsigned pn_chain_id(int rb, int e) { return (unsigned)(4 * rb + e); }
PN_SLOTS_FN unsigned pn_group_tag(int wave, int q) { return (unsigned)((wave << 6) | (q << 4)); }
PN_SLOTS_FN int slot_of_id(unsigned id) { return pn_slot((id >> 6) & 3, (id >> 2) & 3, (id >> 4) & 3, id & 3); }
// group (flag bit) of a published id, and the k-th (0 .. 15) slot of a group: the sixteen points one lane scored for a channel
PN_SLOTS_FN int pn_group_of_id(unsigned id) { return (int)(4 * ((id >> 6) & 3) + ((id >> 4) & 3)); }
PN_SLOTS_FN int pn_group_slot(int group, int k) { return pn_slot(group >> 2, k >> 2, group & 3, k & 3); }
