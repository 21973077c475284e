// fc_adjoint_loop_tape.hpp -- host bookkeeping of the closed-loop tape (fc_adjoint_loop_reserve / _begin), the sibling of
// fc_adjoint_segments.hpp.  The loop tape holds what the adjoint of a closed loop reads of the forward run: one row per closed-loop step m,
//     [ xi_{m-1} (nx) | y_{m-1} (n_sens) | v_m (n_act) ]
// -- the controller state BEFORE its update, the measurement the controller read and the UNCLAMPED control -- written by fc_ctrl_step.
// This header knows nothing of the device: it counts the rows, keeps the order slot of every taped step, the row of the loop signals the
// first taped step read and the step counter the next taped step must find (a step taken outside the closed loop ends the tape), and
// answers whether the tape holds exactly a given run.  Host only, standard headers only (it is tested alone:
// tests/support/adjoint_loop_tape_host_check.cpp).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

struct FcLoopTape {
  int capacity = 0;          // steps the tape can hold (0: no tape)
  bool begun = false;        // false again after end()
  int lost = 0;              // steps beyond the capacity since begin(): nothing was written for them
  bool bad = false;          // a taped forward call reported a non-finite velocity: the rows behind that step were never written
  int64_t row0 = -1;         // row of the loop signals that the first taped step read (-1: no signals were set)
  uint64_t next_step = 0;    // the handle's step counter as the next taped step must find it
  std::vector<int> slots;    // order slot of taped step m at [m - 1]
  std::string ended_by;      // what ended the tape (empty: nothing did)

  int count() const { return (int)slots.size(); }
  bool overflowed() const { return lost > 0; }

  // a new, empty tape of `cap` steps (0: none); not begun
  void reserve(int cap) {
    capacity = cap > 0 ? cap : 0;
    clear();
    ended_by.clear();
  }
  // the bank, its state, the signals, the limits, the flow state or the solver's numbering changed: the rows are no run any more
  void end(const char* why) {
    if (capacity == 0) return;
    if (begun) ended_by = why ? why : "";
    clear();
  }
  // the next closed-loop step starts a new tape; false without a reserve
  bool begin(uint64_t step_counter) {
    if (capacity == 0) return false;
    clear();
    ended_by.clear();
    begun = true;
    next_step = step_counter;
    return true;
  }
  // a closed-loop step on `order_slot` is about to be enqueued: the row to write (0-based), or -1 when nothing is to be written (no
  // tape, not begun, ended, or full -- the step is then counted as lost).  `step_counter`: the handle's counter before the step;
  // `signal_row`: the row of the loop signals the step reads (-1: none).
  int push(int order_slot, uint64_t step_counter, int64_t signal_row) {
    if (capacity == 0 || !begun) return -1;
    if (step_counter != next_step) {
      end("a time step outside the closed loop advanced the state");
      return -1;
    }
    ++next_step;
    if (lost > 0 || count() >= capacity) {
      ++lost;
      return -1;
    }
    if (slots.empty()) row0 = signal_row;
    slots.push_back(order_slot);
    return count() - 1;
  }
  void mark_bad() {
    if (begun) bad = true;
  }
  // does the tape hold exactly a run of n_steps steps whose first step ran on first_slot and whose later ones ran on later_slot?
  // `why` (optional) receives the reason when it does not.
  bool covers(int n_steps, int first_slot, int later_slot, std::string* why = nullptr) const {
    std::string r;
    if (capacity == 0)
      r = "no loop tape is reserved";
    else if (!begun)
      r = ended_by.empty() ? std::string("the loop tape is not begun") : "the loop tape was ended: " + ended_by;
    else if (overflowed())
      r = "the loop tape overflowed: " + std::to_string(count() + lost) + " steps since it was begun, capacity " + std::to_string(capacity);
    else if (bad)
      r = "the taped forward run went non-finite";
    else if (count() != n_steps)
      r = "the loop tape holds " + std::to_string(count()) + " steps, the run has " + std::to_string(n_steps);
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

 private:
  void clear() {
    begun = false;
    lost = 0;
    bad = false;
    row0 = -1;
    next_step = 0;
    slots.clear();
  }
};
