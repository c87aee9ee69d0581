// CPU check of lowthrustopt_amd/csrc/sweep_policy.hpp (which kernel form an indirect sweep runs): built and run by
// tests/test_sweep_policy.py with g++, no GPU.  Literal expectations at 256 CUs and the default cost table; `auto <ndim> <method>
// <steps> <pm> <S>` on the command line prints what resolve_stm gives for LTO_KERNEL_AUTO (the rows of tests/test_auto_kernel.py).
#include <cstdio>
#include <cstdlib>
#include "../../lowthrustopt_amd/csrc/sweep_policy.hpp"

using namespace lto;

static const long CUS = 256;
static const int P0 = 1, P1 = 2, P2 = 4, PGEN = 8;     // one bit per control-law class

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL line %d: %s\n", __LINE__, #cond); ++fails; } } while (0)

static StmChoice stm(int ndim, int method, int steps, int pm, long S, int forced, int cols = 0, bool ordered = false, int p48_form = 0) {
  return resolve_stm(ndim, method, steps, pm, S, forced, cols, ordered, p48_form, CUS, kRoundCostDefault, kLaneRoundUs);
}
static int lanes(int ndim, int method, int pm, long S, int forced, int set = 0, int verdict = 0, bool blocks = false) {
  return defect_lanes(ndim, method, pm, S, forced, set, verdict, blocks, CUS);
}

int main(int argc, char** argv) {
  if (argc == 7 && std::atoi(argv[1]) == 0) {          // auto <ndim> <method> <steps> <pm> <S>
    const StmChoice ch = stm(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atol(argv[6]), LTO_KERNEL_AUTO);
    std::printf("%d\n", ch.kernel);
    return 0;
  }
  const int RK4 = LTO_RK4, DOP = LTO_DOP853_ADAPTIVE;

  // forced selectors whose family is gone resolve to the one that took over
  CHECK(stm(12, RK4, 3, P1, 29, LTO_KERNEL_COOP).kernel == LTO_KERNEL_PIPE8);             // resolved as if the plan had 6 steps
  CHECK(stm(12, RK4, 64, P1, 8192, LTO_KERNEL_COOP).kernel == LTO_KERNEL_PIPE32);
  CHECK(stm(12, LTO_RKF78_ADAPTIVE, 0, P1, 29, LTO_KERNEL_PER_LANE).kernel == LTO_KERNEL_COOP);
  CHECK(stm(12, LTO_RKF78_FIXED, 4, P1, 29, LTO_KERNEL_PER_LANE).kernel == LTO_KERNEL_COOP);
  CHECK(stm(12, DOP, 0, P1, 29, LTO_KERNEL_COOP).kernel == LTO_KERNEL_COOP2);
  CHECK(stm(14, DOP, 0, P2, 29, LTO_KERNEL_AUTO).kernel == LTO_KERNEL_COOP);
  CHECK(stm(14, DOP, 0, P0 | P1, 29, LTO_KERNEL_AUTO).kernel == LTO_KERNEL_COOP2);
  CHECK(stm(14, DOP, 0, P1 | PGEN, 29, LTO_KERNEL_AUTO).kernel == LTO_KERNEL_COOP);
  CHECK(stm(12, RK4, 64, P1, 29, LTO_KERNEL_PIPE48).kernel == LTO_KERNEL_PIPE48);          // a family that exists runs as asked

  // LTO_KERNEL_PIPE48, 12-dim: the form with the cheaper rounds; p48_form overrides; 14-dim: always 48
  const auto rounds = [](long S, long per) { return (double)((S + per - 1) / per); };
  for (long S : {11264L, 12288L, 24576L}) {
    const bool want = rounds(S, 44 * CUS) * kRoundCostDefault[0][3] < rounds(S, 48 * CUS) * kRoundCostDefault[0][1];
    CHECK(stm(12, RK4, 64, P1, S, LTO_KERNEL_PIPE48).seg44 == want);
    CHECK(stm(12, RK4, 64, P1, S, LTO_KERNEL_PIPE48, 0, false, 44).seg44 == true);
    CHECK(stm(12, RK4, 64, P1, S, LTO_KERNEL_PIPE48, 0, false, 48).seg44 == false);
    CHECK(stm(14, RK4, 64, P1, S, LTO_KERNEL_PIPE48).seg44 == false);
    CHECK(stm(14, RK4, 64, P1, S, LTO_KERNEL_PIPE48, 0, false, 44).seg44 == false);
  }
  CHECK(stm(12, RK4, 64, P1, 11264, LTO_KERNEL_PIPE48).seg44 == true);     // 1 round of 44 x 256 at 139 us against 1 of 48 x 256 at 165
  CHECK(stm(12, RK4, 64, P1, 12288, LTO_KERNEL_PIPE48).seg44 == false);    // 2 x 139 against 1 x 165
  CHECK(stm(12, RK4, 64, P1, 24576, LTO_KERNEL_PIPE48).seg44 == false);    // 3 x 139 against 2 x 165
  CHECK(stm(12, RK4, 6, P1, 11264, LTO_KERNEL_AUTO).kernel == LTO_KERNEL_PIPE48 && stm(12, RK4, 6, P1, 11264, LTO_KERNEL_AUTO).seg44);

  // the stream corner of the per-lane family: one RK4 step, unordered, from 65 536 segments; cols_per_lane = ndim asks for it
  for (int ndim : {12, 14}) {
    CHECK(stm(ndim, RK4, 1, P1, 65535, LTO_KERNEL_AUTO).kernel == LTO_KERNEL_PER_LANE && !stm(ndim, RK4, 1, P1, 65535, LTO_KERNEL_AUTO).stream);
    CHECK(stm(ndim, RK4, 1, P1, 65536, LTO_KERNEL_AUTO).kernel == LTO_KERNEL_PER_LANE && stm(ndim, RK4, 1, P1, 65536, LTO_KERNEL_AUTO).stream);
    CHECK(stm(ndim, RK4, 1, P1, 65536, LTO_KERNEL_PER_LANE).stream);
    CHECK(stm(ndim, RK4, 1, P1, 29, LTO_KERNEL_AUTO, ndim).stream && stm(ndim, RK4, 1, P1, 1048576, LTO_KERNEL_AUTO, ndim).stream);
    CHECK(!stm(ndim, RK4, 1, P1, 65536, LTO_KERNEL_AUTO, 1).stream);
    CHECK(!stm(ndim, RK4, 1, P1, 65536, LTO_KERNEL_AUTO, 0, true).stream && !stm(ndim, RK4, 1, P1, 65536, LTO_KERNEL_AUTO, ndim, true).stream);
    CHECK(!stm(ndim, RK4, 2, P1, 14 * 65536, LTO_KERNEL_PER_LANE).stream);
  }
  CHECK(!stm(12, RK4, 64, P1, 65536, LTO_KERNEL_PIPE8).stream && !stm(12, DOP, 0, P1, 65536, LTO_KERNEL_AUTO).stream);

  // defect lanes, 12-dim DOP853
  CHECK(lanes(12, DOP, P1, 29, LTO_KERNEL_AUTO) == 4);
  CHECK(lanes(12, DOP, P1, 131072, LTO_KERNEL_AUTO) == 4 && lanes(12, DOP, P1, 131073, LTO_KERNEL_AUTO) == 2);
  CHECK(lanes(12, DOP, P1, 262144, LTO_KERNEL_AUTO) == 2 && lanes(12, DOP, P1, 262145, LTO_KERNEL_AUTO) == 1);
  CHECK(lanes(12, DOP, P2 | PGEN, 131072, LTO_KERNEL_AUTO) == 4);
  CHECK(lanes(12, DOP, P1, 29, LTO_KERNEL_COOP2) == 2 && lanes(12, DOP, P1, 524288, LTO_KERNEL_COOP2) == 2);
  CHECK(lanes(12, DOP, P1, 29, LTO_KERNEL_PER_LANE) == 1 && lanes(12, DOP, P1, 29, LTO_KERNEL_COOP) == 1);
  for (int set : {1, 2, 4}) {
    CHECK(lanes(12, DOP, P1, 29, LTO_KERNEL_AUTO, set) == set && lanes(12, DOP, P1, 524288, LTO_KERNEL_PER_LANE, set) == set);
    CHECK(lanes(12, DOP, P1, 65536, LTO_KERNEL_AUTO, set, 1) == set);           // ... and no verdict overrides it
  }
  // a latched verdict overrides AUTO's own choice only on a full chip, S >= 64 x CUs = 16 384
  CHECK(lanes(12, DOP, P1, 16384, LTO_KERNEL_AUTO, 0, 1) == 1 && lanes(12, DOP, P1, 16384, LTO_KERNEL_AUTO, 0, 2) == 2);
  CHECK(lanes(12, DOP, P1, 16383, LTO_KERNEL_AUTO, 0, 1) == 4 && lanes(12, DOP, P1, 16383, LTO_KERNEL_AUTO, 0, 2) == 4);
  CHECK(lanes(12, DOP, P1, 262145, LTO_KERNEL_AUTO, 0, 2) == 2);
  CHECK(lanes(12, DOP, P1, 65536, LTO_KERNEL_COOP2, 0, 1) == 2 && lanes(12, DOP, P1, 65536, LTO_KERNEL_PER_LANE, 0, 2) == 1);
  // 14-dim DOP853: the quad form for p = 0 / 1 while the chip has a SIMD per 16 segments, else one lane
  CHECK(lanes(14, DOP, P0 | P1, 131072, LTO_KERNEL_AUTO) == 4 && lanes(14, DOP, P1, 131073, LTO_KERNEL_AUTO) == 1);
  CHECK(lanes(14, DOP, P1, 131072, LTO_KERNEL_COOP2) == 4 && lanes(14, DOP, P1, 29, LTO_KERNEL_PER_LANE) == 1);
  CHECK(lanes(14, DOP, P1, 524288, LTO_KERNEL_AUTO, 4) == 4 && lanes(14, DOP, P1, 29, LTO_KERNEL_AUTO, 1) == 1);
  CHECK(lanes(14, DOP, P1, 65536, LTO_KERNEL_AUTO, 0, 2) == 4);                            // no statistics on 14-dim plans
  CHECK(lanes(14, DOP, P2, 29, LTO_KERNEL_AUTO) == 1 && lanes(14, DOP, P1 | PGEN, 29, LTO_KERNEL_AUTO) == 1);
  // every other integrator: one lane
  for (int ndim : {12, 14})
    for (int method : {LTO_RK4, LTO_RKF78_FIXED, LTO_RKF78_ADAPTIVE})
      for (int forced : {LTO_KERNEL_AUTO, LTO_KERNEL_COOP2, LTO_KERNEL_PER_LANE})
        CHECK(lanes(ndim, method, P1, 29, forced) == 1 && lanes(ndim, method, P1, 65536, forced, 0, 2) == 1);
  // LTO_LAYOUT_BLOCKS: the one-lane kernel writes struct-of-arrays only
  CHECK(lanes(12, DOP, P1, 262145, LTO_KERNEL_AUTO, 0, 0, true) == 2 && lanes(12, DOP, P1, 29, LTO_KERNEL_PER_LANE, 0, 0, true) == 2);
  CHECK(lanes(12, DOP, P1, 29, LTO_KERNEL_AUTO, 1, 0, true) == 2 && lanes(12, DOP, P1, 29, LTO_KERNEL_AUTO, 0, 0, true) == 4);

  // statistics: which sweeps take them, and the verdict -- max <= 3 x mean over all S segments: 2 lanes up to 160 x CUs = 40 960, then 1
  CHECK(defect_stats_wanted(12, DOP, LTO_KERNEL_AUTO, 0, 16384, CUS) && !defect_stats_wanted(12, DOP, LTO_KERNEL_AUTO, 0, 16383, CUS));
  CHECK(!defect_stats_wanted(12, DOP, LTO_KERNEL_COOP2, 0, 65536, CUS) && !defect_stats_wanted(12, DOP, LTO_KERNEL_AUTO, 2, 65536, CUS));
  CHECK(!defect_stats_wanted(14, DOP, LTO_KERNEL_AUTO, 0, 65536, CUS) && !defect_stats_wanted(12, RK4, LTO_KERNEL_AUTO, 0, 65536, CUS));
  CHECK(defect_stats_verdict(10L * 40960, 30, 40960, 40960, CUS) == 2 && defect_stats_verdict(10L * 40961, 30, 40961, 40961, CUS) == 1);
  CHECK(defect_stats_verdict(10L * 40960, 31, 40960, 40960, CUS) == 0);                    // a tail: max > 3 x mean
  CHECK(defect_stats_verdict(10L * 40960, 30, 40959, 40960, CUS) == 0);                    // not every segment counted
  CHECK(defect_stats_verdict(0, 0, 40960, 40960, CUS) == 0);
  CHECK(defect_stats_verdict(81920L * 7, 21, 81920, 81920, CUS) == 1 && defect_stats_verdict(81920L * 7, 21, 81920, 81920, 512) == 2);

  // what each form is built for, as the plan setters ask it
  CHECK(reference_setting(12, DOP) && !reference_setting(14, DOP) && !reference_setting(12, LTO_RKF78_ADAPTIVE));
  CHECK(indirect_records_available(12, DOP) && !indirect_records_available(14, DOP) && indirect_warm_start_available(12, DOP) && !indirect_warm_start_available(12, RK4));
  CHECK(indirect_stm_coop2_available(12, DOP, PGEN) && indirect_stm_coop2_available(14, DOP, P0 | P1) && !indirect_stm_coop2_available(14, DOP, P2) &&
        !indirect_stm_coop2_available(12, LTO_RKF78_ADAPTIVE, P1) && !indirect_stm_coop2_available(12, RK4, P1));
  CHECK(indirect_stm_coop_available(14, DOP) && indirect_stm_coop_available(12, LTO_RKF78_FIXED) && !indirect_stm_coop_available(12, DOP) && !indirect_stm_coop_available(14, RK4));
  CHECK(indirect_stm_pipeline_available(RK4) && !indirect_stm_pipeline_available(DOP) && indirect_stm_per_lane_available(RK4) && !indirect_stm_per_lane_available(LTO_RKF78_FIXED));
  CHECK(indirect_stm_pipe32_available(12, PGEN) && indirect_stm_pipe32_available(14, P0 | P1) && !indirect_stm_pipe32_available(14, P1 | P2) && !indirect_stm_pipe32_available(14, PGEN));
  CHECK(indirect_stm_lane_available(12, RK4, 1L << 20) && !indirect_stm_lane_available(14, RK4, 29) && !indirect_stm_lane_available(12, DOP, 29) && !indirect_stm_lane_available(12, RK4, 1L << 29));
  CHECK(indirect_stm_stream_available(12, RK4, 1, 29) && indirect_stm_stream_available(14, RK4, 1, 29) && !indirect_stm_stream_available(12, RK4, 2, 29) &&
        !indirect_stm_stream_available(12, DOP, 1, 29) && !indirect_stm_stream_available(12, RK4, 1, 1L << 29));
  CHECK(indirect_defect2_available(12, DOP) && !indirect_defect2_available(14, DOP) && !indirect_defect2_available(12, RK4));
  CHECK(indirect_defect4_available(12, DOP, PGEN) && indirect_defect4_available(14, DOP, P0) && !indirect_defect4_available(14, DOP, P2) && !indirect_defect4_available(14, LTO_RKF78_ADAPTIVE, P1));

  if (fails) return 1;
  std::printf("sweep policy ok\n");
  return 0;
}
