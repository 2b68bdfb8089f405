// norm_plan.h — the numbers of the GroupNorm / LayerNorm kernels and who decides between them (norm_plan.cpp: host
// arithmetic only, no HIP).  norms.hip holds the kernels, sizes them by the constants below and launches what the planner
// answers.  Plain constants and structs: read by the device and by the host compile.
#pragma once
#include <stddef.h>
#include <stdint.h>

// ---- GroupNorm: the streaming pipeline (gn_stats | gn_finalize_cs -> gn_apply) ------------------------------------------
constexpr int GN_THREADS = 256;
constexpr int GN_MAX_SLOTS = 3;   // float4 slots per thread
constexpr int GN_MAX_C = 4 * GN_MAX_SLOTS * GN_THREADS;   // 3072: also the floats per plane of gn_stats' LDS staging
constexpr int GN_G = 32;          // groups supported per launch (reference always uses 32)
constexpr int GN_MAX_NSPLIT = 1024;      // slabs per batch at most: sizes the workspace for every C
constexpr int GN_CS_ROWS = 64;           // rows per slab of a producer's column statistics (vgen_tapgemm colstats)
constexpr int GN_CS_ITEMS_256 = 2048;    // (slab, channel) items per group up to which gn_finalize_cs runs 256 threads, above 1024
// ---- single launch, slice resident in LDS (gn_fused) ---------------------------------------------------------------------
constexpr int GNF_THREADS = 512;         // r04 same-box A/B of the whole step: 256 threads +0.3 %, 1024 +0.35 % (profiles/r04f_ab_gnf_threads.jsonl)
constexpr int GNF_LDS_FLOATS = 24576;    // 96 KiB of the CU's 160 KiB
// ---- single launch, slice resident in registers (gn_regs) ----------------------------------------------------------------
constexpr int GNR_THREADS = 1024;
constexpr int GNR_NIT = 36;              // float2 items per thread
constexpr int GNR_MAX_BLOCKS = 1024;     // one block per (batch, group): more of them and the streaming pipeline wins

enum GnPath { GN_FUSED = 0, GN_REGS = 1, GN_STREAM = 2, GN_CS256 = 3, GN_CS1024 = 4 };

struct GnPlan {
  int path;
  int nsplit;          // slabs per batch of gn_stats / gn_apply (0: single launch)
  size_t lds_bytes;    // dynamic LDS of gn_fused: the staged (batch, group) slice
  int64_t part_floats; // workspace: part[nb][nsplit][groups][3], then stat[nb][C][2] at this offset
};

// what vgen_groupnorm / vgen_groupnorm_cs were called with, as far as validation and planning read it
struct GnArgs {
  const void *x1, *cs1, *x2, *cs2, *y, *raw, *ws;
  int32_t C1, C2, groups, dtype;
  int64_t nb, S;
  size_t ws_bytes;
  bool want_cs;        // the _cs entry: statistics are required, S in whole slabs
};

// every argument check of the two entries, in their order: 0, VGEN_E_BADARG or VGEN_E_WORKSPACE with vgen_last_error() set
int gn_validate(const GnArgs& a);
// the dispatch rule; sizes as gn_validate admits them
GnPlan gn_plan(int64_t nb, int64_t S, int C1, int C2, int groups, bool has_cs);

// ---- LayerNorm: LPR lanes per row, float4 slots sub, sub + LPR, ... ---------------------------------------------------------
constexpr int LN_THREADS = 256;
constexpr int LN_MAX_SLOTS = 8;          // float4 slots per lane: d <= 4 * 8 * LPR
constexpr int LN_MAX_D = 64 * 4 * LN_MAX_SLOTS;
constexpr int LN_STREAM_GRID = 2048;     // blocks of the streaming kernel at most (8 per CU); they walk the row groups
// the widths with a streaming kernel, d = NS * 4 * LPR exactly (16-bit outputs only)
struct LnWidth {
  int d, lpr, ns;
};
constexpr LnWidth LN_STREAM[] = {{320, 16, 5}, {512, 16, 8}, {640, 32, 5}, {1024, 32, 8}, {1280, 64, 5}, {2048, 64, 8}};

struct LnPlan {
  int lpr;             // 16 / 32 / 64
  int ns;              // float4 slots per lane of the streaming kernel; 0: the one-shot kernel
  unsigned grid;
};

int ln_validate(const void* x, int64_t M, int32_t d, const void* gamma, const void* beta, const void* y, int32_t dtype);
LnPlan ln_plan(int64_t M, int d, int dtype);   // M > 0
