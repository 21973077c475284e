// fc_adjoint_schedule.hpp -- the backward schedule of the four adjoint marches: the order slot backward step m solves on,
// the coefficients that weigh the two masked adjoint levels in its right-hand side, the tape column of x_m and its energy row -- and
// the same for the two state-gradient products behind the loop.  Host only, no project header, nothing of the device (it is tested
// alone: tests/support/adjoint_schedule_host_check.cpp).  The coefficients belong to the forward step that CONSUMED the state: step j
// read x_{j-1} with (cm_n, cc_n) and x_{j-2} with (cm_nn, cc_nn) of its slot; step 1 ran on `first_slot`, every later one on
// `later_slot`.  (The convective coefficients cc are 0 on a linearised handle.)
#pragma once

struct StepCoeffs {
  double cm_n, cm_nn, cc_n, cc_nn;
};

struct FcAdjointSchedule {
  int n_steps, first_slot, later_slot;
  StepCoeffs c1, c2;  // the coefficients of first_slot and of later_slot

  struct Item {
    int slot;        // order slot of the transposed solve (-1: a product, no solve)
    StepCoeffs c;    // weights of (mu_{m+1}, mu_{m+2}) in the right-hand side
    int column;      // tape column of x_m: m + 1
    int energy_row;  // row of the energy weights: m - 1 (-1: no energy term, dE_0 is not in the sum)
  };

  // backward step m, n_steps >= m >= 1
  Item step(int m) const {
    const bool next = m + 1 <= n_steps, next2 = m + 2 <= n_steps;
    return {m == 1 ? first_slot : later_slot, {next ? c2.cm_n : 0.0, next2 ? c2.cm_nn : 0.0, next ? c2.cc_n : 0.0, next2 ? c2.cc_nn : 0.0}, m + 1, m - 1};
  }
  // dJ/dx_0 = M Z (cm_n(1) mu_1 + cm_nn(2) mu_2) + J(x_0)^T Z (cc_n(1) mu_1 + cc_nn(2) mu_2)
  Item dx0() const {
    const bool two = n_steps >= 2;
    return {-1, {c1.cm_n, two ? c2.cm_nn : 0.0, c1.cc_n, two ? c2.cc_nn : 0.0}, 1, -1};
  }
  // dJ/dx_{-1} = M Z cm_nn(1) mu_1 + J(x_{-1})^T Z cc_nn(1) mu_1
  Item dxm1() const { return {-1, {c1.cm_nn, 0.0, c1.cc_nn, 0.0}, 0, -1}; }
};
