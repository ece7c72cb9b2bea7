// A program of its own for tests/test_search_plan_cpu.py::test_the_replay_is_clean_under_asan_and_ubsan: replays the first eight transitions
// of that file (first search, AUTO contracting and handing over, a cache-aware round, the fixed point, an exchange, a cutoff change, a
// fixed-mask change, forget) through the functions of tests/plan_harness.cpp, built with -fsanitize=address,undefined.  The plans are
// checked in the Python test; here a few key fields are, and every access the planner makes is under the sanitizers.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "plan_harness.cpp"

#define CHECK(cond) do { if (!(cond)) { std::printf("CHECK failed at line %d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

namespace {
const int kSrc[4] = {0, 1, 1, 2}, kDst[4] = {1, 0, 2, 1}, kN[3] = {100, 200, 300};
const int AUTO = 0, GRID = 2, TILE = 3;

struct Replay {
  void* h; int exchange, world; PlanOut out; unsigned char fixed[3] = {1, 0, 0};
  Replay(int exchange_, int world_) : exchange(exchange_), world(world_) {
    const unsigned char owned[4] = {1, 1, 1, 1};
    h = plan_new(3, 4, kSrc, kDst, owned);
    for (int k = 0; k < 3; ++k) plan_set_frame(h, k, kN[k], 1.0, 0.1, 5);
  }
  ~Replay() { plan_free(h); }
  int plan(double x1, float cutoff = 0.05f, int method = AUTO) {
    double P[48] = {0};
    for (int k = 0; k < 3; ++k) for (int i = 0; i < 4; ++i) P[16 * k + 5 * i] = 1.0;
    P[16 + 12] = x1;
    return plan_run(h, P, fixed, cutoff, method, exchange, world, &out);
  }
  int finish(double d, unsigned tie = 0, unsigned far = 0) {
    int ints[24]; double reals[12]; int need[8];
    plan_rows(h, ints, reals, need);
    plan_queued(h);
    double res[9] = {0}, scales[4] = {0};
    for (int e = 0; e < 4; ++e) if (ints[6 * e]) { res[2 * e] = kN[kSrc[e]] / 2; res[2 * e + 1] = d * d; scales[e] = (double)(float)(std::sqrt(d * d) * 1.5); }
    res[8] = out.spec_arm * world;
    return plan_arrived(h, tie, far, res, scales, 0);
  }
  void to_fixed_point() {
    const double x[5] = {0.30, 0.20, 0.12, 0.11, 0.106}, d[5] = {0.2, 0.09, 0.08, 0.079, 0.07};
    for (int r = 0; r < 5; ++r) {
      CHECK(plan(x[r]) == 0 && out.method == TILE);
      CHECK(out.tile_lb == (r >= 3) && out.tile_cached == (r == 4));
      finish(d[r]);
    }
    CHECK(plan(0.106) == 0 && out.method == GRID && out.nothing_can_change && out.tie_skip && !out.far_skip && out.far_narrow);
    finish(0.07);
  }
};
}  // namespace

int main() {
  {   // 1-4: a registration to its fixed point
    Replay R(0, 1);
    R.to_fixed_point();
    CHECK(R.plan(0.106) == 0 && R.out.far_skip && R.out.sel_skip && R.out.use_bracket);
    R.finish(0.07);
    // 6: cutoff change
    CHECK(R.plan(0.106, 0.02f) == 0 && !R.out.all_unchanged && R.out.method == TILE && R.out.tile_cached);
    R.finish(0.02);
    // 7: fixed-mask change and back
    R.fixed[2] = 1;
    CHECK(R.plan(0.106, 0.02f) == 0 && !R.out.same_active_set);
    R.finish(0.02);
    R.fixed[2] = 0;
    CHECK(R.plan(0.106, 0.02f) == 0 && !R.out.same_active_set);
    R.finish(0.02);
    // an explicit list, a solve, a forced method, an unknown one
    plan_explicit(R.h, 2, 50, 0.1f);
    plan_solved(R.h, 1, 0, 1, 1);
    CHECK(R.plan(0.106, 0.02f, GRID) == 0 && R.out.method == GRID && R.out.spec_arm && !R.out.use_bracket);
    R.finish(0.02);
    CHECK(R.plan(0.106, 0.02f, 99) == MVICP_ERR_ARG);
    // 8: forget
    plan_forget(R.h);
    CHECK(R.plan(0.106) == 0 && R.out.method == TILE && !R.out.same_active_set && !R.out.use_bracket && !R.out.spec_arm);
    R.finish(0.2);
    CHECK(plan_set_option(R.h, "tie_rule", 0.0) == 0 && plan_set_option(R.h, "no_such_option", 1.0) == -1);
    CHECK(R.plan(0.106) == 0 && !R.out.tie_launched && !R.out.same_active_set);
  }
  {   // 5: the same with an exchange configured (two ranks, eager tie trees)
    Replay R(1, 2);
    CHECK(R.plan(0.30) == 0 && R.out.n_tie_need == 3);
    R.finish(0.2);
    plan_forget(R.h);
    R.to_fixed_point();
    plan_solved(R.h, 1, 0, 0, 1);
    CHECK(R.plan(0.106) == 0 && !R.out.sel_skip && !R.out.spec2_plan && R.out.spec_arm);
    CHECK(R.finish(0.07) == 1);
  }
  std::printf("PLAN_REPLAY_OK\n");
  return 0;
}
