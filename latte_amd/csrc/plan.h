// The plan table of the linear samplers (Euler, Euler-ancestral, Heun, DPM-Solver++): what latte_sample_plan_loop and
// latte_t2v_guided_linear_loop share.  Host code only.  The table is latte_amd/schedulers.py: engine_plan(); its layout is documented at
// latte_sample_plan_loop in include/latte_amd.h.
#pragma once
#include "common.h"

namespace latte {

// columns of a plan row: the ONE definition on the C++ side
enum PlanCol { P_T = 0, P_IN, P_MX, P_MEPS, P_CX, P_C0, P_C1, P_C2, P_C3, P_CN, P_PUSH, P_RSV };
static_assert(P_RSV + 1 == LATTE_PLAN_COLS, "plan columns");

struct PlanInfo {
  std::vector<int64_t> ts;   // timestep of every row
  bool scaled = false;       // some in_scale != 1: the denoiser reads in_scale * x kept beside x
};

// Every check of the table, all rows before anything is launched or copied: n_evals <= max_evals; per row finite entries, an integral
// timestep >= 0 (and < t_limit unless t_limit == 0), push in {0, 1}, reserved 0, c_noise == 0 unless noise is given or may be drawn,
// c_j (j >= 1) only after j rows with push.  Messages start with "<who>: ".
int plan_check(const char* who, const double* plan, int n_evals, int max_evals, int64_t t_limit, bool noise_given, bool may_draw_noise,
               PlanInfo* info);

// coefficients of row k narrowed to fp32; in_scale_next is the NEXT row's in_scale (1 after the last row, whose x is the result)
LinearStep plan_step(const double* plan, int k, int n_evals, float scale);

// The three remembered outputs m0 of earlier rows: h1 the newest.  A row with push writes write() -- the oldest slot, which may be
// read as h3 by the same launch -- and then push() makes it h1.
struct HistRing {
  float* slot[3];
  int newest = 0;
  float* h1() const { return slot[newest]; }
  float* h2() const { return slot[(newest + 2) % 3]; }
  float* h3() const { return slot[(newest + 1) % 3]; }
  float* write() const { return h3(); }
  void push() { newest = (newest + 1) % 3; }
};

}  // namespace latte
