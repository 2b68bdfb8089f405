// tapgemm_plan.h — what a tap-GEMM launch looks like and who decides it (tapgemm_plan.cpp: host arithmetic only, no HIP).
// tapgemm.hip and panelgemm.hip hold the kernels and launch what the planner answers.
#pragma once
#include "../../include/vgen_hip.h"

// ---- the block shapes -------------------------------------------------------------------------------------------------
// One kernel template (tapgemm.hip: BM x BN tile, BK K-elements per stage of a 3-stage LDS ring, WM x WN waves) in five
// block shapes, and the panel kernel of panelgemm.hip.  kShapes below is the ONE statement of what each shape is: the
// legality rule, the cost model, the start stagger and the dispatch of tapgemm.hip all read it.
//   "pp"    256 x BN, BK 64, 4x2 waves (512 threads), ONE block per CU, ping-pong wave groups — the long-K shape: convs,
//           big linears.  Takes dual-W launches (vgen_tapgemm_args.dualw).
//   "dual"  256 x BN, BK 32, 2x2 waves (wave tile 128 x BN/2), lock-step K-steps, ring of 24-26 KiB stages, TWO blocks per
//           CU (<= 80 KiB LDS, <= 256 VGPRs each).  The two blocks are not barrier-coupled: one block's prologue (index
//           math, first DMA latency), fragment reads and epilogue run under the other's MFMAs — the short-K linears of the
//           transformer blocks (5-20 K-steps per tile) spend 60-80 % of a "pp" tile in exactly those phases (profiles/).
//           The 128-row wave tile also reads 25 % fewer LDS bytes per MFMA than the 64 x 64 one.  No dual-W K-steps.
//   "pp128" 128 x BN, otherwise "pp": for under-filled launches.  32-row wave tiles: a 64-row statistics slab would span two
//           waves, so no column statistics.
//   "panel" panelgemm.hip: the W-panel-resident shape of the K = 320 / 640 linears; never a row of the plan table, never
//           proposed by the cost model: vgen_panel_bn() below says which launches take it and with which panel width.
//   "pp256" 256 x 256, BK 32, 8 waves (64 x 128 wave tiles), ping-pong, 3 x 32 KiB ring: 128 FLOP per staged byte instead
//           of 85-98 — for N % 256 == 0 launches with 16-bit outputs (GEGLU up-projections, the K = 1280 q/k/v); 214
//           VGPRs, so only the paired-16-byte-store epilogue is instantiated for it (fp32 outputs through split-K only).
//   "q128"  128 x BN, BK 32, 4 waves (64 x BN/2 wave tiles), lock-step, 3 x (128 + BN) x 64 B ring (48-55 KiB): two
//           INDEPENDENT blocks per CU — for the under-filled 8 x 14 / 4 x 7 levels, where one 8-wave block per CU leaves
//           every stall of its short K loop uncovered.
// BN = 128 (N % 128 == 0), 160 (N = 320 / 960 ...: exact tiles instead of 2.5 x 128; not under GEGLU, whose tiles pair 16
// value with 16 gate columns) or 64 (small / odd N).  pp256 and q128 (r06) are reached through the measured plan table or
// a forced plan only.
// r04: 224-row tiles (every row count of the t2v UNet is 7 * 2^k, so 256-row tiles fill the last round over the CUs at
// most 87.5 %) were built as a dual 224 x BN shape and a 224 x 320 ping-pong shape, passed every parity case they are legal
// for, and measured +0.5 % (mixed) / +1.4 % (single-pass) SLOWER on the whole step in a same-box A/B
// (profiles/r04a_ab_libs.jsonl); so was the buffer-resource LDS-DMA (+0.1 / +0.6 %).  Both were removed again (history:
// commits 34443ca, 6b9d39a).
enum Shape { SHAPE_PP = 0, SHAPE_DUAL = 1, SHAPE_PP128 = 2, SHAPE_PANEL = 3, SHAPE_PP256 = 4, SHAPE_Q128 = 5, NUM_SHAPES = 6 };

struct ShapeDesc {
  const char* name;
  int bm, bk, wm, wn;       // block tile rows, K elements per ring stage, waves along M x N (bm = 0: not the streaming kernel)
  bool pp;                  // ping-pong wave groups (8 waves), else lock-step K-steps
  int bpc;                  // co-resident blocks per CU: 2 for the 4-wave blocks (the kernel's __launch_bounds__ rule)
  int bns[3];               // the column tiles BN it takes
  bool dualw, colstats;     // takes dual-W launches / writes column statistics
  bool out16_only;          // no fp32 / scalar epilogue: vectorisable 16-bit outputs, anything the split-K reducer takes
  bool modelled;            // proposed by the cost model
  // cost model, microseconds (constants fitted to profiles/r01_*_tapgemm_shapes.json), by BN = 128 / 160 / 64:
  double t_k[3];            //   per 64-element K-step of one block (bpc = 2: while sharing its CU)
  double t_tile;            //   fixed per tile
  double t_k_alone[3];      //   bpc = 2, launch of <= 256 blocks: per K-step of a block alone on its CU ...
  double t_tile_alone;      //   ... and its fixed part
  double stagger_us;        // start stagger (tapgemm.hip launch()): estimated us per K-step and tile column
};

constexpr ShapeDesc kShapes[NUM_SHAPES] = {
    // name     bm  bk wm wn  pp    bpc  bns              dualw  colst  out16  model  t_k                 t_tile t_k_alone           t_tile_alone stagger
    {"pp",     256, 64, 4, 2, true,  1, {128, 160, 64},   true,  true,  false, true,  {0.85, 1.15, 0.60}, 8.0,   {0, 0, 0},          0.0,         0.0060},
    {"dual",   256, 32, 2, 2, false, 2, {128, 160, 64},   false, true,  false, true,  {2.20, 2.50, 1.40}, 9.0,   {1.10, 1.30, 0.75}, 10.0,        0.0150},
    {"pp128",  128, 64, 4, 2, true,  1, {128, 160, 64},   true,  false, false, true,  {0.62, 0.80, 0.45}, 6.0,   {0, 0, 0},          0.0,         0.0050},
    {"panel",    0,  0, 8, 1, false, 1, {160, 80, 64},    true,  false, false, false, {0, 0, 0},          0.0,   {0, 0, 0},          0.0,         0.0},
    {"pp256",  256, 32, 4, 2, true,  1, {256, 0, 0},      false, false, true,  false, {0, 0, 0},          0.0,   {0, 0, 0},          0.0,         0.0060},
    {"q128",   128, 32, 2, 2, false, 2, {128, 160, 64},   false, true,  false, false, {0, 0, 0},          0.0,   {0, 0, 0},          0.0,         0.0050},
};

// a dual-W pair = an ordinary K-step + an odd step that reads 10 of 18 fragments and issues 3 of 7 DMA pieces
constexpr double DUALW_KSTEP_FACTOR = 1.6;

// Source of padding / out-of-range rows in tapgemm.hip: a zero REGION long enough for a pointer to walk a whole K extent
// through it (K * 2 bytes — twice that on the W side of a dual-W launch — <= 256 KiB - 128, vgen_tapgemm_validate), so every
// DMA source pointer advances by the same ROW_BYTES per K-tile whether its row is live or not — no per-piece increment
// registers (7 VGPRs on the dual shape, which sat at 256 VGPRs with 3 spills).  256 KiB: K <= 131008 for a plain launch,
// <= 65504 with dual-W — the VAE's P.V product over a 90 x 160 latent (K = 14400) and the widest decoder conv of the UNet
// (K = 9 * 2560, dual-W) fit with room (r02's 64 KiB bound did not: ADVICE r02).
constexpr int ZERO_BYTES = 262144;

// ---- quantities of a launch that the planner and launch() both need ---------------------------------------------------
// (the kernel and the reducer keep their own expressions of KT and n_out: device code is pinned by the ISA fingerprint)
inline int tap_kt(const vgen_tapgemm_args& a) { return a.taps * (a.C1 / 64) + a.C2 / 64; }   // 64-element K-steps
inline int tap_n_out(const vgen_tapgemm_args& a) { return a.epilogue == VGEN_EPI_GEGLU ? a.N / 2 : a.N; }
// The PLANNER's "every epilogue access is a whole 4-vector": it gates split-K (the reducer has no scalar path) and pp256.
// Deliberately NOT shared with the kernel's `vec`, which is a different predicate (no N % 4 term, masks instead of
// remainders) and part of the pinned device code: the kernel picks an epilogue path with its own, the planner a plan with
// this one.
inline bool tap_vec(const vgen_tapgemm_args& a) {
  return (a.N % 4 == 0) && (tap_n_out(a) % 4 == 0) && (a.ldo % 4 == 0) && (a.residual == nullptr || a.ldr % 4 == 0) &&
         (a.rowbias == nullptr || a.rowbias_ld % 4 == 0);
}

struct Plan {
  int shape;
  int bn;
  int splitk;
};

// The plan of a launch: a measured table entry first (r06: it may also take a K = 320 / 640 linear AWAY from the panel
// shape), then the panel shape for the launches it takes, then the cost model.
Plan full_plan(const vgen_tapgemm_args& a);
// which launches take the panel shape: the column-panel width, 0 = not this shape
int vgen_panel_bn(const vgen_tapgemm_args& a);
// every argument check of vgen_tapgemm: 0, or VGEN_E_BADARG with vgen_last_error() set; nothing is launched
int vgen_tapgemm_validate(const vgen_tapgemm_args& a);
