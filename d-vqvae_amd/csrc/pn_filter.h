// Host side of the PointNet trunks (pointnet.hip, pointnet_filter.hip): the tile geometry and scratch layout of the filtered trunk, the
// DVQ_PN_ABL diagnostics bits, and the argument structs and prototypes of the launchers.  The geometry and the enum compile as plain
// C++ (tests/test_pointnet_trunk_layout.py builds them into a host program); what needs HIP or dvq.h types is behind __HIPCC__.
#pragma once
#include <stddef.h>
#include "pn_slots.h"

constexpr int PN_MAX_TILES = 64;                           // tiles of a sample the exact stage keeps maxima for
constexpr int PN_MAX_POINTS = PN_MAX_TILES * PN_TILE_SLOTS;   // the filtered trunk takes at most 16 384 points

// One sample of N points on the filtered trunk, and the bytes PER SAMPLE of every array of a scratch set.
struct PnGeometry {
    int tiles;        // 256-point tiles = tile records of a sample, a tail tile included
    int deal;         // tiles the points are dealt to (pn_slots.h); deal == tiles - 1: the last tile is a 32-point tail tile
    int Npad;         // rows of a sample's h2 block: N rounded up to whole tiles
    long slots;       // slots the filtered trunk evaluates: 256 per dealt tile + 32 of a tail tile
    size_t h2;        // conv2 rows [Npad][128] fp32
    size_t rec4;      // tile records [tiles][1024] float4: the three largest scores + group flags
    size_t rec2;      // tile records [tiles][1024] float2: the fourth and fifth score
    size_t tstat;     // tile maxima [tiles][4] words
    size_t cbuf;      // centre [128] fp32
    bool has_tail() const { return deal < tiles; }
    // ``part`` = rec4 + rec2 (96 B per padded point); the fused and the unfused trunk use it as [Npad / 128][1024] floats, a third of it
    size_t part() const { return rec4 + rec2; }
    size_t per_sample() const { return h2 + part() + tstat + cbuf; }
};
// 1 .. 32 points beyond a multiple of 256 (the 778 MANO vertices: 3 x 256 + 10) become a tail tile of one block, four samples per
// workgroup, instead of a last full tile of padding (tail_enabled = DVQ_PN_TAIL, default on; the features are the same bit for bit)
inline PnGeometry pn_geometry(int N, bool tail_enabled) {
    PnGeometry g;
    g.tiles = (N + PN_TILE_SLOTS - 1) / PN_TILE_SLOTS;
    const int over = N - PN_TILE_SLOTS * (g.tiles - 1);
    g.deal = (g.tiles >= 2 && over <= PN_TAIL_SLOTS && tail_enabled) ? g.tiles - 1 : g.tiles;
    g.Npad = g.tiles * PN_TILE_SLOTS;
    g.slots = (long)PN_TILE_SLOTS * g.deal + (g.has_tail() ? PN_TAIL_SLOTS : 0);
    g.h2 = (size_t)g.Npad * 128 * 4;
    g.rec4 = (size_t)g.tiles * 1024 * 16;
    g.rec2 = (size_t)g.tiles * 1024 * 8;
    g.tstat = (size_t)g.tiles * 16;
    g.cbuf = 128 * 4;
    return g;
}
// Byte offsets of the arrays of ONE scratch set for launches of up to ``samples`` samples (each array 256-byte aligned; part2 sits
// directly behind the float4 records: together they are ``part``)
struct PnSetLayout { size_t h2, part, part2, tstat, cbuf, bytes; };
inline PnSetLayout pn_set_layout(const PnGeometry& g, size_t samples) {
    auto up = [](size_t n) { return (n + 255) / 256 * 256; };
    const size_t part = up(samples * g.h2), tstat = part + up(samples * g.part()), cbuf = tstat + up(samples * g.tstat);
    return {0, part, part + samples * g.rec4, tstat, cbuf, cbuf + up(samples * g.cbuf)};
}

// DVQ_PN_ABL (diagnostics build only, -DDVQ_DIAG): a sum of these bits.  "trunk" = pn_trunk_filter_kernel (full-tile instances unless
// said otherwise), "exact" = pn_exact_kernel, "front" / "back" = the launchers.  Everything outside PN_ABL_VALID is a timing ablation:
// the features are INVALID.  (Bit 8 is retired: nothing reads it.)
enum PnAbl : int {
    PN_ABL_NO_H2_STORE = 1,         // trunk (both): the conv2 rows are not stored
    PN_ABL_NO_CONV3 = 2,            // trunk: no conv3 loop
    PN_ABL_FEW_ROWS = 16,           // exact: every candidate is one of 64 rows (rows cached)
    PN_ABL_NO_GROUPS = 32,          // exact: no flagged groups (phase C)
    PN_ABL_NO_DOTS = 64,            // exact: no candidate dots (phase B)
    PN_ABL_NO_CHAIN = 128,          // trunk (both): no top-two chain behind the MFMAs
    PN_ABL_NO_PUBLISH = 256,        // trunk: no tile records published
    PN_ABL_NO_HANDOVER = 512,       // trunk: the pairs are not handed over through the ring
    PN_ABL_NO_W3_LOADS = 1024,      // trunk: W3 chunks neither loaded nor staged
    PN_ABL_STAMPS = 4096,           // trunk (both): phase durations into word 3 of the tile maxima (no non-finite flag); exact: phase cycles into the statistics; back prints both (DVQ_PN_STATS=1)
    PN_ABL_CLOCK = 8192,            // trunk (both), with STAMPS: the in-kernel clock in MHz instead; back prints it
    PN_ABL_NO_CHUNK_BARRIER = 16384,   // trunk: no barrier at the head of a chunk
    PN_ABL_INJECT_LIE = 32768,      // trunk (both): FAULT INJECTION, a record that lies about its tile (tests/test_gpu_parity.py)
    PN_ABL_INJECT_LOST = 65536,     // trunk (both): FAULT INJECTION, a hand-over that does not happen (tests/test_gpu_parity.py)
    PN_ABL_CONSUMER = 131072,       // trunk (both): no conv1 / conv2, rows from thin air
    PN_ABL_SPLIT = 262144,          // front (C = 4): producer and consumer halves of the trunk as two launches on two streams
    PN_ABL_ONE_PER_CU = 524288,     // front: 100 KB of LDS asked for, ONE workgroup per CU
    PN_ABL_NO_RULE1 = 1048576,      // exact: flagged groups are not gated on what their hidden points can reach (the counts without rule 1)
    PN_ABL_NO_RULE2 = 2097152,      // exact: the anchor's exact score does not raise the lower bound (the counts without rule 2)
    // bits that leave the features valid: the exact stage's consistency check runs only under these
    PN_ABL_VALID = PN_ABL_STAMPS | PN_ABL_CLOCK | PN_ABL_INJECT_LIE | PN_ABL_INJECT_LOST | PN_ABL_ONE_PER_CU | PN_ABL_NO_RULE1 | PN_ABL_NO_RULE2
};

constexpr size_t PN_STATS_BYTES = 128;                     // the exact stage's statistics (DVQ_PN_STATS): sixteen 64-bit counters

// One scratch set (pointnet.hip's plan() places it by pn_set_layout)
struct PnSlot { float *h2, *part, *cbuf; void* part2; unsigned* tstat; };

#ifdef __HIPCC__
#include "dvq_internal.h"

// the conv layers of one trunk (BatchNorm folded); w2p / w3p: bf16 planes, w3f: filter image (all optional, include/dvq.h)
struct PnTrunkWeights {
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    const uint16_t *w2p, *w3p;
    const void* w3f;
    int relu3;                                             // ReLU after the last layer: the STN's trunk has one, the main trunk none
};
inline PnTrunkWeights pn_stn_trunk(const dvq_pointnet_weights* w) {
    return {w->s_w1, w->s_b1, w->s_w2, w->s_b2, w->s_w3, w->s_b3, w->s_w2p, w->s_w3p, w->s_w3f, 1};
}
inline PnTrunkWeights pn_main_trunk(const dvq_pointnet_weights* w) {
    return {w->w1, w->b1, w->w2, w->b2, w->w3, w->b3, w->w2p, w->w3p, w->w3f, 0};
}
// the clouds of one launch: pc [B][C][N], trans [B][9] (xyz @ trans in front of conv1) or null
struct PnBatch { const float *pc, *trans; int C, N; long B; };

// pointnet.hip: the fused six-product trunk -> partial [B][ceil(N / 128)][1024] column maxima
int dvq_launch_pn_trunk(const PnBatch& in, const PnTrunkWeights& w, float* partial, hipStream_t st);
// pointnet_filter.hip.  front = centres + trunk kernel(s) into the scratch set, back = pn_exact_kernel from it -> feat: two halves,
// so that the caller may put them on different streams
int dvq_launch_pn_filter_front(const PnBatch& in, const PnTrunkWeights& w, const PnSlot& sl, unsigned long long* stats, hipStream_t st);
int dvq_launch_pn_filter_back(const PnBatch& in, const PnTrunkWeights& w, const PnSlot& sl, float* feat, long ld_feat,
                              unsigned long long* stats, hipStream_t st);
size_t dvq_pn_filter_image_bytes();
int dvq_launch_pn_filter_pack(const float* w2, const float* w3, void* image, hipStream_t st);
int dvq_pn_fault_counters(unsigned long long* out2, int reset);
#endif
