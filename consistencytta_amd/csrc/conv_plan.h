// conv_gemm dispatch, host side: the tile table, the tile ids the rules name, and the PLAN of one ctta_conv_gemm call --
// everything that decides what reaches the device, worked out without touching it (conv_plan.hip).  conv_gemm.hip launches
// from the plan; ctta_conv_plan shows it to tests and tools.
#pragma once
#include "conv_epilogue.h"

// ------------------------------------------------------------------------------------------
// The tile variants: T(BM, BN, BK, WM, WN, MODE, STAGES) one tile per workgroup, TK(..., KIND, TAG) the others.
// Ids are 1-based positions in this list; tests and tools address tiles by id, so the order is fixed.
#define CTTA_CONV_TILE_TABLE(T, TK) \
  T(128, 128, 64, 2, 2, 0, 2)  /* 1   register-staged (support in_act) */ \
  T(128, 128, 32, 2, 2, 0, 2)  /* 2 */ \
  T(256, 64, 64, 4, 1, 0, 2)   /* 3 */ \
  T(256, 32, 64, 4, 1, 0, 2)   /* 4 */ \
  T(64, 64, 64, 2, 2, 0, 2)    /* 5 */ \
  T(64, 128, 64, 2, 2, 0, 2)   /* 6 */ \
  T(256, 128, 64, 4, 2, 0, 2)  /* 7 */ \
  T(128, 64, 64, 2, 2, 0, 2)   /* 8 */ \
  T(128, 128, 64, 2, 2, 1, 2)  /* 9   direct-to-LDS, generic gather: twins of 1..8 */ \
  T(128, 128, 32, 2, 2, 1, 2)  /* 10 */ \
  T(256, 64, 64, 4, 1, 1, 2)   /* 11 */ \
  T(256, 32, 64, 4, 1, 1, 2)   /* 12 */ \
  T(64, 64, 64, 2, 2, 1, 2)    /* 13 */ \
  T(64, 128, 64, 2, 2, 1, 2)   /* 14 */ \
  T(256, 128, 64, 4, 2, 1, 2)  /* 15 */ \
  T(128, 64, 64, 2, 2, 1, 2)   /* 16 */ \
  T(128, 128, 64, 2, 2, 2, 2)  /* 17  direct-to-LDS, descriptor fast path: twins of 1..8 */ \
  T(128, 128, 32, 2, 2, 2, 2)  /* 18 */ \
  T(256, 64, 64, 4, 1, 2, 2)   /* 19 */ \
  T(256, 32, 64, 4, 1, 2, 2)   /* 20 */ \
  T(64, 64, 64, 2, 2, 2, 2)    /* 21 */ \
  T(64, 128, 64, 2, 2, 2, 2)   /* 22 */ \
  T(256, 128, 64, 4, 2, 2, 2)  /* 23 */ \
  T(128, 64, 64, 2, 2, 2, 2)   /* 24 */ \
  T(128, 128, 32, 2, 2, 1, 4)  /* 25  multi-stage rings (counted vmcnt) */ \
  T(128, 128, 32, 2, 2, 2, 3)  /* 26 */ \
  T(64, 128, 64, 2, 2, 2, 3)   /* 27 */ \
  T(256, 128, 32, 4, 2, 2, 2)  /* 28 */ \
  T(256, 256, 64, 2, 4, 2, 2)  /* 29  8 waves, 128x64 per wave */ \
  T(256, 256, 32, 2, 4, 2, 2)  /* 30 */ \
  T(256, 128, 64, 2, 2, 2, 2)  /* 31  4 waves, 128x64 per wave */ \
  T(256, 128, 32, 2, 2, 2, 2)  /* 32 */ \
  T(256, 256, 32, 2, 4, 2, 3)  /* 33  deeper rings for the big tile (96 / 128 KB) */ \
  T(256, 256, 32, 2, 4, 2, 4)  /* 34 */ \
  T(512, 128, 32, 4, 2, 2, 2)  /* 35  N = 128 layers: 8 waves of 128x64 (the big tile's wave shape) over 512 rows */ \
  T(512, 128, 64, 4, 2, 2, 2)  /* 36  ... with BK = 64: the whole 160 KB of LDS */ \
  T(64, 128, 64, 2, 2, 2, 4)   /* 37  deeper rings for thin K-heavy launches (latency-bound: one K tile in flight per */ \
  T(128, 128, 64, 2, 2, 2, 3)  /* 38  workgroup is ~1.1 us per K step whatever the tile) */ \
  T(128, 64, 64, 2, 2, 2, 3)   /* 39 */ \
  T(128, 128, 64, 2, 2, 2, 4)  /* 40 */ \
  TK(256, 256, 64, 2, 4, 2, 2, 2, "_sk")  /* 41  stream-K (one persistent launch, in-launch fold): twins of 29 / 31 / 17 */ \
  TK(256, 128, 64, 2, 2, 2, 2, 2, "_sk")  /* 42 */ \
  TK(128, 128, 64, 2, 2, 2, 2, 2, "_sk")  /* 43 */

struct TileShape {
  const char* name;
  int bm, bn, bk;
  int wm, wn;
  int mode;
  int stages;
  int kind;     // 0: one tile per workgroup; 2: stream-K (one persistent launch)
};
#define CTTA_TILE_SHAPE_(BM, BN, BK, WM, WN, G, S) {#BM "x" #BN "x" #BK "_w" #WM "x" #WN "_m" #G "_s" #S, BM, BN, BK, WM, WN, G, S, 0},
#define CTTA_TILE_SHAPE_K_(BM, BN, BK, WM, WN, G, S, KIND, TAG) \
  {#BM "x" #BN "x" #BK "_w" #WM "x" #WN "_m" #G "_s" #S TAG, BM, BN, BK, WM, WN, G, S, KIND},
constexpr TileShape kTiles[] = {CTTA_CONV_TILE_TABLE(CTTA_TILE_SHAPE_, CTTA_TILE_SHAPE_K_)};
constexpr int kNumVariants = sizeof(kTiles) / sizeof(kTiles[0]);

// The ids the dispatch rules name.
enum : int {
  kTile128x128x64 = 1,      // register-staged ids: what pick_tile returns before the staging twin is chosen
  kTile128x128x32 = 2,
  kTile256x32x64 = 4,
  kTile64x64x64 = 5,
  kTile64x128x64 = 6,
  kTile128x64x64 = 8,
  kTwinLds = 8,             // + this: the direct-to-LDS twin with the generic gather (ids 1..8 only)
  kTwinFast = 16,           // + this: the direct-to-LDS twin on the descriptor fast path (ids 1..8 only)
  kTile64x128x64Ring3 = 27, // 64x128x64 on the fast path with a 3-stage ring
  kTile256x128x32 = 28,     // 8 waves of 64x64
  kBigTile = 29,            // 256x256x64, 8 waves of 128x64
  kTile512x128x64 = 36,
  kBigTileSk = 41,          // the big tile's stream-K twin
  kHaloProfCode = 39,       // what conv1d_halo_kernel launches are profiled as (predates tile 39; tools read it)
};
constexpr bool tile_is(int id, int bm, int bn, int bk, int wm, int wn, int mode, int stages, int kind) {
  return id >= 1 && id <= kNumVariants && kTiles[id - 1].bm == bm && kTiles[id - 1].bn == bn && kTiles[id - 1].bk == bk &&
         kTiles[id - 1].wm == wm && kTiles[id - 1].wn == wn && kTiles[id - 1].mode == mode && kTiles[id - 1].stages == stages &&
         kTiles[id - 1].kind == kind;
}
constexpr bool twins_ok() {   // ids 1..8 + kTwinLds / kTwinFast: the same tile in staging mode 1 / 2
  for (int i = 1; i <= 8; ++i) {
    const TileShape& t = kTiles[i - 1];
    if (!tile_is(i, t.bm, t.bn, t.bk, t.wm, t.wn, 0, 2, 0) || !tile_is(i + kTwinLds, t.bm, t.bn, t.bk, t.wm, t.wn, 1, 2, 0) ||
        !tile_is(i + kTwinFast, t.bm, t.bn, t.bk, t.wm, t.wn, 2, 2, 0))
      return false;
  }
  return true;
}
static_assert(kNumVariants == 43, "tile ids are public: tests and tools address tiles by number");
static_assert(twins_ok(), "ids 9..16 / 17..24 must be the staging twins of 1..8");
static_assert(tile_is(kTile128x128x64, 128, 128, 64, 2, 2, 0, 2, 0) && tile_is(kTile128x128x32, 128, 128, 32, 2, 2, 0, 2, 0) &&
              tile_is(kTile256x32x64, 256, 32, 64, 4, 1, 0, 2, 0) && tile_is(kTile64x64x64, 64, 64, 64, 2, 2, 0, 2, 0) &&
              tile_is(kTile64x128x64, 64, 128, 64, 2, 2, 0, 2, 0) && tile_is(kTile128x64x64, 128, 64, 64, 2, 2, 0, 2, 0),
              "register-staged tile names");
static_assert(tile_is(kTile64x128x64Ring3, 64, 128, 64, 2, 2, 2, 3, 0) && tile_is(kTile256x128x32, 256, 128, 32, 4, 2, 2, 2, 0) &&
              tile_is(kBigTile, 256, 256, 64, 2, 4, 2, 2, 0) && tile_is(kTile512x128x64, 512, 128, 64, 4, 2, 2, 2, 0) &&
              tile_is(kBigTileSk, 256, 256, 64, 2, 4, 2, 2, 2),
              "fast-path tile names");

// ------------------------------------------------------------------------------------------
// What a plan may know about the process.  ctta_conv_gemm fills it from the live process, ctta_conv_plan from its caller.
struct ConvPlanEnv {
  int cu_count;
  int xcd, splitk, streamk, streamk_grid;     // option values (CttaOption)
  bool no_splitk;                             // ctta_conv_suppress_splitk
  bool stamps;                                // ctta_conv_debug_stamps bound a buffer
  // The split-K / stream-K workspace, looked up on FIRST USE: the per-device default workspace is allocated by the lookup, and
  // only launches that reach for it may create it.  `lookup` fills the three fields below; null: they are given.
  void (*lookup)(ConvPlanEnv*);
  bool ws_ok;                                 // there is a workspace
  size_t ws_bytes;
  bool ws_hdr;                                // ... and its stream-K header was zeroed by its owner
  float* ws;                                  // (for the launch step; the plan never looks at it)

  bool splitk_on() const { return splitk != 0 && !no_splitk; }
  bool workspace() {
    if (lookup) { lookup(this); lookup = nullptr; }
    return ws_ok;
  }
};

// One ctta_conv_gemm call, decided.  The ConvParams are finished but for the pointers to process resources that the launch
// step binds: zero, stamps, sk_hdr / sk_slots and the split-K first pass's out.
struct ConvPlan {
  int vid, kind;            // tile id (0 on the halo path) and its TileShape::kind
  bool halo;                // conv1d_halo_kernel<32, 256> instead of a tile
  int prof_code;            // profiler variant: vid, vid + 100 with the generic epilogue, kHaloProfCode
  long long M, K;
  int groups;
  unsigned gx, gy, gz;      // grid of the (first) launch
  ConvParams p;             // the launch -- with splits > 1: the epilogue that splitk_finish_kernel runs
  int splits;               // > 1: two-pass split-K
  ConvParams q;             // splits > 1: the first pass (raw fp32 partial sums into the workspace)
  int ld, finish_blocks;    // splits > 1: slab row stride and the grid of splitk_finish_kernel
  int tail_rows, tail_vid;  // > 0: the ragged last row tile runs as a second launch on tail_vid
  unsigned tail_gx, tail_gy;
  ConvParams t;
};
ctta_status ctta_conv_make_plan(const ctta_conv_desc* d, ConvPlanEnv& env, ConvPlan& pl);
