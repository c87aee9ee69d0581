// sweep_policy.hpp -- which kernel form an indirect sweep runs: what every form is built for, and the rules that pick one.
// Device-free (no HIP, no lto_ctx): tests/cabi/sweep_policy_check.cpp builds it with g++ and pins the choices on a CPU.  The
// predicates are the ONLY statement of what a form is built for -- the plan setters of lto_indirect_plan.hip validate through them, the rules
// below choose through them, the launchers of the kernel units refuse through them.  A new form: one predicate, one line in the
// rule that should pick it, one case in launch_stm / launch_defect (lto_indirect_plan.hip).
#pragma once
#include <algorithm>
#include "../../include/lto.h"

namespace lto {

// pm: bit mask of the control-law classes present in a batch, bit c = class c of dynamics.hpp PMode (kernels.hpp asserts the numbering)
constexpr int kThrustLimitedClasses = (1 << 0) | (1 << 1);   // PM_P0, PM_P1: the always-thrust-limited laws, p = 0 and p = 1
constexpr int kOtherClasses = (1 << 2) | (1 << 3);           // PM_P2, PM_PGEN

// RK4 STM sweeps with >= 6 steps, 12-dim: microseconds per round of the form whose lane is a whole segment (kernels_indirect_lane.hip;
// a round = 256 segments per CU) at 64 steps on MI355X, for AUTO's comparison with the pipelines' round costs (default of
// lto_ctx::lane_round_us; lto_calibrate_kernels measures it on the context's own device).
constexpr double kLaneRoundUs = 505.0;      // round 6 (explicit register parking, matrices from the base evaluations' by-products): was 590
// us per round at 64 steps, MI355X: [12-dim | 14-dim][eight-wave (16 x CUs) | 48-segment (48 x CUs) | per-lane with 3 columns (64 x CUs) |
// 44-segment (44 x CUs) | 32-segment (32 x CUs)]; lto_calibrate_kernels replaces them with the context's own device's
constexpr double kRoundCostDefault[2][5] = {{63.0, 165.0, 246.0, 139.0, 111.0}, {72.0, 191.0, 1e300, 1e300, 128.0}};

/* ------------------------------------------------------------------------------ what each form is built for */
// The reference's setting, 12-dim DOP853: the forms with two lanes per state or per segment and what hangs on them -- record staging
// and LTO_LAYOUT_BLOCKS (the kernels that write per-segment records), the warm start.
inline bool reference_setting(int ndim, int method) { return ndim == 12 && method == LTO_DOP853_ADAPTIVE; }
inline bool indirect_records_available(int ndim, int method) { return reference_setting(ndim, method); }
inline bool indirect_warm_start_available(int ndim, int method) { return reference_setting(ndim, method); }
// STM sweep.  Per-lane (kernels_indirect.hip, kernels_indirect14.hip): RK4 -- the 13-stage methods have no per-lane STM form; its
// form with the whole STM of a one-step segment in the lane (kernels_indirect_stream.hip); whole-segment lanes (kernels_indirect_lane.hip)
inline bool indirect_stm_per_lane_available(int method) { return method == LTO_RK4; }
inline bool indirect_stm_stream_available(int ndim, int method, int steps, long S) {
  return (ndim == 12 || ndim == 14) && method == LTO_RK4 && steps == 1 && S < (1L << 29);
}
inline bool indirect_stm_lane_available(int ndim, int method, long S) { return ndim == 12 && method == LTO_RK4 && S < (1L << 29); }
// the three pipelines (kernels_indirect_pipe8 / _pipe32 / _pipe48.hip): fixed-step RK4; the 32-segment form pairs stages, 14-dim only
// for the always-thrust-limited laws
inline bool indirect_stm_pipeline_available(int method) { return method == LTO_RK4; }
inline bool indirect_stm_pipe32_available(int ndim, int pm) { return ndim == 12 || (ndim == 14 && !(pm & kOtherClasses)); }
// two lanes per state (kernels_indirect_coop2.hip, kernels_indirect_coop2_14.hip): DOP853; 12-dim, and 14-dim with p = 0 or p = 1
inline bool indirect_stm_coop2_14_available(int pm) { return (pm & ~kThrustLimitedClasses) == 0; }
inline bool indirect_stm_coop2_available(int ndim, int method, int pm) {
  return method == LTO_DOP853_ADAPTIVE && (ndim == 12 || indirect_stm_coop2_14_available(pm));
}
// one-piece cooperative kernel (kernels_indirect_coop.hip): the 13-stage methods, except where coop2 is the only form (12-dim DOP853)
inline bool indirect_stm_coop_available(int ndim, int method) { return method != LTO_RK4 && !reference_setting(ndim, method); }
// Defect-only sweep (kernels_indirect_defect2.hip).  Two lanes per segment: the reference's setting; four: that, and 14-dim DOP853
// for the always-thrust-limited laws (round 6, the dynamics of coop2_14)
inline bool indirect_defect2_available(int ndim, int method) { return reference_setting(ndim, method); }
inline bool indirect_defect4_14_available(int ndim, int method, int pm) {
  return ndim == 14 && method == LTO_DOP853_ADAPTIVE && indirect_stm_coop2_14_available(pm);
}
inline bool indirect_defect4_available(int ndim, int method, int pm) {
  return reference_setting(ndim, method) || indirect_defect4_14_available(ndim, method, pm);
}

/* ------------------------------------------------------------------------------ STM sweep: which family runs */
/* What LTO_KERNEL_AUTO resolves to for an STM sweep: a pure function of the plan's shape and the cost table (no device, no context
 * state), so that the choice at sizes this build never ran on -- the per-rank batches of an 8-GPU run -- can be pinned by a CPU test
 * (tests/test_auto_kernel.py).  cost: us per round at 64 steps of the eight-wave / 48-segment / (unused) / 44-segment / 32-segment
 * pipelines for this dimension; per_lane3_us: the 12-dim per-lane kernel with three columns, rounds of 64 x CUs (only for RK4 with
 * 2 ... 5 steps); lane_us: the whole-segment lanes, rounds of 256 x CUs.
 * RK4 with >= 6 steps: the pipelines -- the eight-wave form while the batch is one round of it (16 segments per CU), above that the
 * family whose rounds are cheapest for THIS segment count, a partly filled round costing a whole one.  (Round 6: the per-lane kernel
 * left this table -- its rounds, 246 us per 64 x CUs, never beat the 32-segment pipeline's, 2 x 111 us.)  RK4 with fewer steps: the
 * per-lane kernel (fill and drain phases outweigh the pipelines' shorter phase), on a full chip its whole-segment forms.  13-stage
 * methods: the cooperative kernels; 12-dim DOP853 (the reference's setting) the two-lanes-per-state form. */
inline int auto_stm_kernel(int ndim, int method, int steps, int pm, long S, long cus, bool ordered, int cols_per_lane, const double* cost,
                           double per_lane3_us, double lane_us) {
  const auto rounds = [&](long per_round) { return (double)((S + per_round - 1) / per_round); };
  if (method != LTO_RK4)      // DOP853: the two-lanes-per-state forms (12-dim; 14-dim for batches of the always-thrust-limited laws, round 6)
    return indirect_stm_coop2_available(ndim, method, pm) ? LTO_KERNEL_COOP2 : LTO_KERNEL_COOP;
  if (steps < 6) {
    if (steps >= 2 && indirect_stm_lane_available(ndim, method, S) && !ordered && cols_per_lane == 0 &&
        rounds(256 * cus) * lane_us < rounds(64 * cus) * per_lane3_us)
      return LTO_KERNEL_LANE;
    return LTO_KERNEL_PER_LANE;
  }
  if (S <= 16 * cus) return LTO_KERNEL_PIPE8;
  const double t8 = rounds(16 * cus) * cost[0];
  const double t48 = std::min(rounds(48 * cus) * cost[1], ndim == 12 ? rounds(44 * cus) * cost[3] : 1e300);
  const double t32 = indirect_stm_pipe32_available(ndim, pm) ? rounds(32 * cus) * cost[4] : 1e300;
  int kern = (t32 < t8 && t32 < t48) ? LTO_KERNEL_PIPE32 : (t48 <= t8 ? LTO_KERNEL_PIPE48 : LTO_KERNEL_PIPE8);
  // the whole-segment lanes (kernels_indirect_lane.hip, 12-dim): rounds of 256 x CUs segments -- four wavefronts of 64 per CU, one per
  // SIMD.  A partly filled round costs a whole one, so the pipelines keep the sizes just above a multiple of their own, smaller rounds.
  if (indirect_stm_lane_available(ndim, method, S) && !ordered && rounds(256 * cus) * lane_us < std::min(std::min(t8, t48), t32)) kern = LTO_KERNEL_LANE;
  return kern;
}

// One-step RK4 STM sweeps (SURVEY 8d's HBM-bound corner): from this many segments AUTO's per-lane family runs the form whose lane is
// a whole segment (kernels_indirect_stream.hip): one wavefront of 64 segments per SIMD of an MI355X.  Below, the per-(segment,
// column group) lanes fill the chip with four to twelve times the wavefronts and the sweep is latency-bound either way.
constexpr long kStreamMinSegments = 65536;

struct StmChoice {
  int kernel;     // the family that runs: what lto_indirect_plan_last_kernel reports (never LTO_KERNEL_AUTO)
  bool seg44;     // LTO_KERNEL_PIPE48, 12-dim: its 44-segment form
  bool stream;    // LTO_KERNEL_PER_LANE: its whole-STM-in-the-lane form (one RK4 step)
};

// The STM sweep of a plan of this shape with selector `forced` (LTO_KERNEL_*, lto_indirect_plan_set_kernel).  round_cost: the
// context's [12-dim | 14-dim][5] table (kRoundCostDefault), lane_us its lane_round_us.
//
// Kernel choice (DESIGN.md "Kernels"; measured on MI355X with tools/probe_kernels.py, profiles/r03_probe_kernels.txt).
// RK4 with >= 6 steps per segment: the three-role pipeline kernels.  A workgroup of the eight-wave form owns 16 segments and a
// CU holds one (91 KB of LDS), so up to 16 x CUs segments (4 096 on MI355X) the sweep is one round -- 14-dim 76 us, 12-dim 66 us
// against 106 / 89 us (four-wave form, removed), 173 / 136 us per-lane, 238 / 116 us cooperative -- and above that every family
// runs in rounds of the segments the chip holds at once, a partly filled round costing a whole one: the family with the
// cheapest rounds for THIS segment count wins (lto_ctx::round_cost: us per round at 64 steps; the ratios do not depend on the step count): the
// eight-wave form in rounds of 16 x CUs, the 48-segment / 16-wave form in rounds of 48 x CUs (12-dim: 44 x CUs), for 12-dim also the per-lane
// kernel with 3 columns per lane in rounds of 64 x CUs.  13-stage methods: the wave-specialised kernel (DOP853 @1e-13,
// 4 096 segments: 0.32 ms vs 1.9 ms per-lane), for the reference's setting (12-dim, DOP853) its two-lanes-per-state form.
inline StmChoice resolve_stm(int ndim, int method, int steps, int pm, long S, int forced, int cols_per_lane, bool ordered, int p48_form,
                             long cus, const double (*round_cost)[5], double lane_us) {
  const double* cost = round_cost[ndim == 14 ? 1 : 0];
  const auto auto_kernel = [&](int steps_, int cols_) {
    return auto_stm_kernel(ndim, method, steps_, pm, S, cus, ordered, cols_, cost, round_cost[0][2], lane_us);
  };
  int kern = forced == LTO_KERNEL_AUTO ? auto_kernel(steps, cols_per_lane) : forced;
  // Families that are gone since round 6 resolve to the one that took over (results agree to round-off, lto_indirect_plan_last_kernel
  // says what ran): the 13-stage methods have no per-lane STM form any more, RK4 no cooperative form, and 12-dim DOP853 only the
  // two-lanes-per-state cooperative form.
  if (kern == LTO_KERNEL_PER_LANE && !indirect_stm_per_lane_available(method)) kern = LTO_KERNEL_COOP;
  // (include/lto.h words the RK4 case loosely, "runs the pipeline AUTO would take": below 6 steps AUTO takes the per-lane family, and
  // a forced LTO_KERNEL_COOP is resolved as if the plan had 6 steps and cols_per_lane = 0.  Kept as it was.)
  if (kern == LTO_KERNEL_COOP && !indirect_stm_coop_available(ndim, method))
    kern = method == LTO_RK4 ? auto_kernel(steps < 6 ? 6 : steps, 0) : LTO_KERNEL_COOP2;
  StmChoice ch = {kern, false, false};
  // the large-batch pipeline has two forms for 12-dim (48 or 44 segments per workgroup, kernels_indirect_pipe48.hip): the cheaper
  // rounds for this segment count, whether AUTO or the caller chose the family
  if (kern == LTO_KERNEL_PIPE48 && ndim == 12) {
    const auto rounds = [&](long per_round) { return (double)((S + per_round - 1) / per_round); };
    ch.seg44 = p48_form ? p48_form == 44 : rounds(44 * cus) * round_cost[0][3] < rounds(48 * cus) * round_cost[0][1];
  }
  // one RK4 step on a full chip: lane = segment, HBM-bound (kernels_indirect_stream.hip)
  if (kern == LTO_KERNEL_PER_LANE)
    ch.stream = !ordered && (cols_per_lane == ndim || (cols_per_lane == 0 && S >= kStreamMinSegments &&
                                                       indirect_stm_stream_available(ndim, method, steps, S)));
  return ch;
}

/* ------------------------------------------------------------------------------ defect-only sweep: lanes per segment */
// The previous sweep's trial-step statistics (k_step_stats: sum and max over `count` segments) as a verdict on the lanes per segment
// of the next one, 0 = none: max <= 3 x mean, no tail worth shortening -- the sweep is throughput-bound once the chip is full.
inline int defect_stats_verdict(long long sum, long long max, long long count, long S, long cus) {
  if (count == S && sum > 0 && max * (long long)S <= 3 * sum) return (S <= 160L * cus) ? 2 : 1;
  return 0;
}
// Whether a plan's defect sweeps take (and leave) such statistics: AUTO's own choice for the reference's setting, on a full chip
inline bool defect_stats_wanted(int ndim, int method, int forced, int lanes_set, long S, long cus) {
  return reference_setting(ndim, method) && forced == LTO_KERNEL_AUTO && !lanes_set && S >= 64L * cus;
}

// Lanes per segment of a defect-only sweep: 4 / 2 (kernels_indirect_defect2.hip) or 1 (the per-lane kernel).  forced: the plan's
// LTO_KERNEL_* selector; lanes_set: lto_indirect_plan_set_defect_lanes (0 = choose); stats_verdict: the latched
// defect_stats_verdict (0 = none); out_blocks: LTO_LAYOUT_BLOCKS.
//
// The reference's setting (12-dim, DOP853).  Two lanes per segment (tools/probe_defect2.py: 29 segments 99 -> 73 us, 4 096:
// 119 -> 88 us, 65 536 ordered: 0.43 -> 0.32 ms, 262 144: 0.44 -> 0.38 ms; 524 288: 0.60 -> 0.73 ms, so one lane beyond);
// round 3: four lanes per segment (a DPP quad, 16 segments per wavefront) up to eight wavefronts per SIMD -- 4 096 segments:
// 90 -> 77 us, 65 536 ordered: 0.31 -> 0.27 ms, 131 072: 0.32 -> 0.30 ms; 262 144: 0.39 -> 0.52 ms, so two lanes there.
// LTO_KERNEL_PER_LANE / LTO_KERNEL_COOP2 on the plan, or lto_indirect_plan_set_defect_lanes, force one form.
inline int defect_lanes(int ndim, int method, int pm, long S, int forced, int lanes_set, int stats_verdict, bool out_blocks, long cus) {
  const bool simd_per_16 = (S + 15) / 16 <= 32L * cus;
  int lanes = 1;
  // the same integrator setting on the 14-dim system (always-thrust-limited laws): the quad form while the chip has a SIMD per 16
  // segments to spare, as for 12-dim (round 6)
  if (indirect_defect4_14_available(ndim, method, pm))
    lanes = lanes_set ? lanes_set : ((forced == LTO_KERNEL_AUTO || forced == LTO_KERNEL_COOP2) && simd_per_16) ? 4 : 1;
  if (reference_setting(ndim, method)) {
    if (lanes_set) lanes = lanes_set;
    else if (forced == LTO_KERNEL_COOP2) lanes = 2;
    else if (forced == LTO_KERNEL_AUTO) {
      lanes = simd_per_16 ? 4 : (S <= 262144 ? 2 : 1);
      // Those thresholds come from the C5 study, where the slowest segment takes 8 x the mean number of trial steps and sets the
      // sweep's time: more lanes per segment = a shorter stream for it.  A sweep whose segments all take about the same number
      // of steps (the 20 trial trajectories of a line search) is throughput-bound once the chip is full, and fewer lanes per
      // segment issue fewer instructions per segment (tools/probe_linesearch_lanes.py, 20 x 4 096 segments: 166 / 147 / 124 us
      // with 4 / 2 / 1 lanes; 20 x 1 024: 73 / 61 / 94).  The previous sweep's statistics say which case this is
      // (lto_indirect_defect_dev reads and latches them).
      if (stats_verdict && S >= 64L * cus) lanes = stats_verdict;
    }
  }
  if (out_blocks && lanes == 1) lanes = 2;          // the one-lane kernel writes struct-of-arrays only
  return lanes;
}

}  // namespace lto
