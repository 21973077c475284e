// fc_adjoint_tape.hpp -- host bookkeeping of the adjoint state tape (fc_adjoint_tape_reserve / _begin).  The tape holds the
// forward trajectory the adjoint of the NONLINEAR stepper reads: capacity + 2 columns of N doubles on the device, column 0 = x_{-1},
// column j + 1 = x_j (x_0: the state fc_adjoint_tape_begin found).  This header knows nothing of the device: it counts the columns, keeps
// the order slot of every taped step and answers whether the tape covers a given run.  Host only, standard headers only (it is tested
// alone: tests/support/adjoint_tape_host_check.cpp).
#pragma once

#include <string>
#include <vector>

struct FcAdjointTape {
  int capacity = 0;        // steps the tape can hold (0: no tape); the device array has capacity + 2 columns
  bool begun = false;      // columns 0 and 1 hold the two time levels a run starts from; false again after invalidate()
  int lost = 0;            // steps beyond the capacity since begin(): nothing was written for them
  std::vector<int> slots;  // order slot of taped step j at [j - 1]

  int count() const { return (int)slots.size(); }
  bool overflowed() const { return lost > 0; }
  int columns() const { return capacity > 0 ? capacity + 2 : 0; }

  // a new, empty tape of `cap` steps (0: none); not begun
  void reserve(int cap) {
    capacity = cap > 0 ? cap : 0;
    invalidate();
  }
  // the state changed behind the tape's back, or its numbering did: what the columns hold is no trajectory any more
  void invalidate() {
    begun = false;
    lost = 0;
    slots.clear();
  }
  // the caller has just written the present (x_{-1}, x_0) into columns 0 and 1; false without a tape
  bool begin() {
    if (capacity == 0) return false;
    invalidate();
    begun = true;
    return true;
  }
  // a step on `order_slot` has advanced the state: the column to write the new state into, or -1 when nothing is to be written (no
  // tape, not begun, or full -- the step is then counted as lost)
  int push(int order_slot) {
    if (capacity == 0 || !begun) return -1;
    if (lost > 0 || count() >= capacity) {
      ++lost;
      return -1;
    }
    slots.push_back(order_slot);
    return count() + 1;
  }
  // the last step was withdrawn (fc_undo_step).  A step withdrawn from in front of begin() ends the tape.
  void pop() {
    if (capacity == 0 || !begun) return;
    if (lost > 0) {
      --lost;
      return;
    }
    if (slots.empty()) {
      invalidate();
      return;
    }
    slots.pop_back();
  }
  // does the tape hold exactly a run of n_steps steps whose first step ran on first_slot and whose later ones ran on later_slot?
  // `why` (optional) receives the reason when it does not.
  bool covers(int n_steps, int first_slot, int later_slot, std::string* why = nullptr) const {
    std::string r;
    if (capacity == 0)
      r = "no tape is reserved";
    else if (!begun)
      r = "the tape is not begun (or was ended by a change of the state, the permutation or the solver structure)";
    else if (overflowed())
      r = "the tape overflowed: " + std::to_string(count() + lost) + " steps since it was begun, capacity " + std::to_string(capacity);
    else if (count() != n_steps)
      r = "the tape holds " + std::to_string(count()) + " steps, the run has " + std::to_string(n_steps);
    else if (n_steps > 0 && slots[0] != first_slot)
      r = "the first taped step ran on order slot " + std::to_string(slots[0]) + ", not on " + std::to_string(first_slot);
    else
      for (int j = 1; j < n_steps; ++j)
        if (slots[(size_t)j] != later_slot) {
          r = "taped step " + std::to_string(j + 1) + " ran on order slot " + std::to_string(slots[(size_t)j]) + ", not on " + std::to_string(later_slot);
          break;
        }
    if (why) *why = r;
    return r.empty();
  }
};
