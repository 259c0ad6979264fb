// Plan walker of the linear samplers (plan.h).
#include "plan.h"

#include <cmath>

#include "../../include/latte_amd_debug.h"

namespace latte {

int plan_check(const char* who, const double* plan, int n_evals, int max_evals, int64_t t_limit, bool noise_given, bool may_draw_noise,
               PlanInfo* info) {
  const std::string w = std::string(who) + ": ";
  if (n_evals > max_evals) return fail(LATTE_ERR_INVALID, w + "more than " + std::to_string(max_evals) + " evaluations");
  info->ts.resize(n_evals);
  info->scaled = false;
  int pushed = 0;
  for (int k = 0; k < n_evals; ++k) {
    const double* r = plan + (size_t)k * LATTE_PLAN_COLS;
    const std::string row = std::to_string(k);
    for (int j = 0; j < LATTE_PLAN_COLS; ++j)
      if (!std::isfinite(r[j])) return fail(LATTE_ERR_INVALID, w + "non-finite plan entry in row " + row);
    if (r[P_T] < 0.0 || r[P_T] >= 9.0e15 || r[P_T] != std::floor(r[P_T]))
      return fail(LATTE_ERR_INVALID, w + "timestep of row " + row + " is not a non-negative integer");
    if (t_limit && r[P_T] >= (double)t_limit)
      return fail(LATTE_ERR_INVALID, w + "timestep of row " + row + " is outside the trained range [0, " + std::to_string(t_limit) + ")");
    if ((r[P_PUSH] != 0.0 && r[P_PUSH] != 1.0) || r[P_RSV] != 0.0)
      return fail(LATTE_ERR_INVALID, w + "push must be 0 or 1 and the reserved column 0 (row " + row + ")");
    if (r[P_CN] != 0.0 && !noise_given && !may_draw_noise)
      return fail(LATTE_ERR_INVALID, w + "row " + row + " has c_noise != 0 but no noise was passed");
    for (int j = 1; j <= 3; ++j)
      if (r[P_C0 + j] != 0.0 && pushed < j)
        return fail(LATTE_ERR_INVALID, w + "row " + row + " reads history slot " + std::to_string(j) + " before " + std::to_string(j) +
                                           " rows with push have run");
    info->ts[k] = (int64_t)r[P_T];
    info->scaled = info->scaled || r[P_IN] != 1.0;
    pushed += r[P_PUSH] != 0.0;
  }
  return LATTE_OK;
}

LinearStep plan_step(const double* plan, int k, int n_evals, float scale) {
  const double* r = plan + (size_t)k * LATTE_PLAN_COLS;
  const bool last = k + 1 == n_evals;
  return LinearStep{scale, (float)r[P_MX], (float)r[P_MEPS], (float)r[P_CX], (float)r[P_C0], (float)r[P_C1], (float)r[P_C2], (float)r[P_C3],
                    (float)r[P_CN], last ? 1.0f : (float)r[LATTE_PLAN_COLS + P_IN], r[P_PUSH] != 0.0 ? 1 : 0};
}

}  // namespace latte

extern "C" int latte_debug_plan_check(const double* plan, int n_evals, int max_evals, int64_t t_limit, int noise_given, int may_draw_noise) {
  if (!plan || n_evals <= 0) return latte::fail(LATTE_ERR_INVALID, "plan_check: bad arguments");
  latte::PlanInfo info;
  return latte::plan_check("plan_check", plan, n_evals, max_evals, t_limit, noise_given != 0, may_draw_noise != 0, &info);
}
