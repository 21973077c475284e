// Stand-alone check of the adjoint marches' backward schedule (flowcontrol_amd/csrc/fc_adjoint_schedule.hpp) -- TEST INFRASTRUCTURE,
// driven by tests/test_adjoint_schedule_host.py.  No device.  The expected table is derived the other way round, from the forward
// recurrence: forward step j on slot s_j reads x_{j-1} with (cm_n, cc_n)(s_j) and x_{j-2} with (cm_nn, cc_nn)(s_j), so the weight of
// adjoint level mu_j on the state x_m is collected by looping over the forward steps.  Backward step m holds mu_{m+1} (the newer level)
// and mu_{m+2}; the two products behind the loop hold mu_1 and mu_2.  Equality is exact.  Prints one line per check, "<name> ok" or
// "<name> FAILED <what>", and exits non-zero if a check failed.
#include <cstdio>
#include <string>
#include <vector>

#include "fc_adjoint_schedule.hpp"

static int failures = 0;

static void check(const std::string& name, bool ok, const std::string& what = "") {
  if (ok) {
    std::printf("%s ok\n", name.c_str());
  } else {
    std::printf("%s FAILED %s\n", name.c_str(), what.c_str());
    ++failures;
  }
}

struct Weight {
  double cm = 0.0, cc = 0.0;
};

static bool same(const StepCoeffs& c, const Weight& newer, const Weight& older) {
  return c.cm_n == newer.cm && c.cc_n == newer.cc && c.cm_nn == older.cm && c.cc_nn == older.cc;
}

int main() {
  const int BDF1 = 0, BDF2 = 1;
  const double dt = 0.005;
  struct Set {
    const char* name;
    StepCoeffs c[2];  // by slot
  };
  const Set sets[] = {
      {"lin", {{1.0 / dt, 0.0, 0.0, 0.0}, {2.0 / dt, -0.5 / dt, 0.0, 0.0}}},
      {"nl", {{1.0 / dt, 0.0, -1.0, 0.0}, {2.0 / dt, -0.5 / dt, -2.0, 1.0}}},
      {"distinct", {{3.0, 5.0, 7.0, 11.0}, {13.0, 17.0, 19.0, 23.0}}},  // no two fields equal: a swapped field shows
  };
  for (const Set& set : sets)
    for (int first : {BDF1, BDF2})
      for (int n : {1, 2, 3, 4, 7}) {
        // w[m + 1][j]: the weight of mu_j on x_m, m = -1 .. n, j = 1 .. n + 2 (levels beyond n stay zero)
        std::vector<std::vector<Weight>> w((size_t)n + 2, std::vector<Weight>((size_t)n + 3));
        std::vector<int> slot_of((size_t)n + 1, -1);
        for (int j = 1; j <= n; ++j) {
          const int s = j == 1 ? first : BDF2;
          slot_of[(size_t)j] = s;
          w[(size_t)(j - 1) + 1][(size_t)j] = {set.c[s].cm_n, set.c[s].cc_n};    // step j read x_{j-1}
          w[(size_t)(j - 2) + 1][(size_t)j] = {set.c[s].cm_nn, set.c[s].cc_nn};  // ... and x_{j-2}
        }
        const FcAdjointSchedule S{n, first, BDF2, set.c[first], set.c[BDF2]};
        const std::string tag = std::string(set.name) + "_bdf" + std::to_string(first + 1) + "_n" + std::to_string(n);
        bool steps = true;
        for (int m = n; m >= 1; --m) {
          const FcAdjointSchedule::Item it = S.step(m);
          steps = steps && it.slot == slot_of[(size_t)m] && it.column == m + 1 && it.energy_row == m - 1 &&
                  same(it.c, w[(size_t)m + 1][(size_t)m + 1], w[(size_t)m + 1][(size_t)m + 2]);
        }
        check(tag + "_steps", steps);
        const FcAdjointSchedule::Item d0 = S.dx0(), d1 = S.dxm1();
        check(tag + "_dx0", d0.slot == -1 && d0.column == 1 && d0.energy_row == -1 && same(d0.c, w[1][1], w[1][2]));
        check(tag + "_dxm1", d1.slot == -1 && d1.column == 0 && d1.energy_row == -1 && same(d1.c, w[0][1], w[0][2]));
      }
  std::printf("%s\n", failures ? "CHECK FAILED" : "CHECK OK");
  return failures ? 1 : 0;
}
