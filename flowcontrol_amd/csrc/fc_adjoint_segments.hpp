// fc_adjoint_segments.hpp -- host bookkeeping of the adjoint state tape, dense (fc_adjoint_tape_reserve) and checkpointed
// (fc_adjoint_tape_reserve_sparse; DESIGN §5.4 "Checkpointed tape": one record).  For a run of n steps and a spacing c >= 1 the tape keeps
//   * checkpoint j = the pair (x_{jc-1}, x_{jc}), j = 0 .. ceil(n / c) - 1: two columns each, for the whole run, and
//   * ONE dense segment buffer of c + 2 columns: while it holds segment j (steps jc + 1 .. min((j + 1) c, n)), column 0 = x_{jc-1},
//     column 1 = x_{jc}, column i + 1 = x_{jc+i}.
// A backward march walks the segments from the last to the first; every segment but the one the forward run left in the buffer is
// recomputed from its checkpoint first.  The DENSE tape is the one-segment case, reserve(n, n): the buffer's n + 2 columns are the whole
// trajectory (column 0 = x_{-1}, column m + 1 = x_m), no step opens a checkpoint and no march replays.  This header knows nothing of
// the device: it counts, keeps the order slot of every taped step and answers where a forward step writes, which buffer column a
// backward step reads and which segments a march replays.  Host only, standard headers only (it is tested alone:
// tests/support/adjoint_segments_host_check.cpp, and its one-segment form against a model of the dense tape in adjoint_tape_host_check.cpp).
#pragma once

#include <string>
#include <vector>

struct FcAdjointSegments {
  int capacity = 0;        // steps the tape can hold (0: no tape)
  int every = 0;           // c: steps per segment (0: no tape)
  bool begun = false;      // checkpoint 0 and buffer columns 0, 1 hold the two time levels a run starts from
  int lost = 0;            // steps beyond the capacity since begin(): nothing was written for them
  int resident = 0;        // the segment the buffer holds
  std::vector<int> slots;  // order slot of taped step m at [m - 1]

  static int ceil_div(int a, int b) { return (a + b - 1) / b; }
  // what a run of n steps with spacing c holds, in columns: 2 ceil(n / c) + c + 2
  static int columns_for(int n, int c) { return n > 0 && c > 0 ? 2 * ceil_div(n, c) + c + 2 : 0; }

  int count() const { return (int)slots.size(); }
  bool overflowed() const { return lost > 0; }
  int checkpoints() const { return capacity > 0 ? ceil_div(capacity, every) : 0; }  // pairs the store has room for
  int buffer_columns() const { return capacity > 0 ? every + 2 : 0; }
  int columns() const { return columns_for(capacity, every); }

  // segment of step m >= 1, and the segments of a run of n steps
  int segment_of(int m) const { return (m - 1) / every; }
  int n_segments(int n) const { return n > 0 ? ceil_div(n, every) : 0; }
  int seg_first(int j) const { return j * every + 1; }
  int seg_last(int j, int n) const { return (j + 1) * every < n ? (j + 1) * every : n; }
  int seg_len(int j, int n) const { return seg_last(j, n) - seg_first(j) + 1; }
  // the buffer column of GLOBAL tape column g (x_m sits in g = m + 1, x_{-1} in g = 0) while the buffer holds segment j
  int local_column(int g, int j) const { return g - j * every; }

  // a new, empty tape of `cap` steps in segments of `c` (either 0: none); not begun
  void reserve(int cap, int c) {
    capacity = (cap > 0 && c > 0) ? cap : 0;
    every = capacity > 0 ? c : 0;
    invalidate();
  }
  // the state changed behind the tape's back, or its numbering did: what the columns hold is no trajectory any more
  void invalidate() {
    begun = false;
    lost = 0;
    resident = 0;
    slots.clear();
  }
  // the caller has just written the present (x_{-1}, x_0) into buffer columns 0, 1 and into checkpoint 0; false without a tape
  bool begin() {
    if (capacity == 0) return false;
    invalidate();
    begun = true;
    return true;
  }

  // Where a forward step writes.  column: the buffer column of the new state (-1: nothing is written).  checkpoint >= 0: the step opens
  // segment `checkpoint` -- BEFORE the new state is written, buffer columns (c, c + 1) go to that pair of the store and to columns (0, 1).
  // row: the row of the control tape (m - 1).
  struct Write {
    int column, checkpoint, row;
  };
  // the step push() would tape next (0: it would not be taped) -- the control row is appended in front of the step's launches
  int next_step() const {
    if (capacity == 0 || !begun || lost > 0 || count() >= capacity) return 0;
    if (count() > 0 && resident != segment_of(count())) return 0;
    return count() + 1;
  }
  // a step on `order_slot` has advanced the state.  A step behind a march that left another segment in the buffer ends the tape: its
  // segment's columns are gone.
  Write push(int order_slot) {
    const Write none{-1, -1, -1};
    if (capacity == 0 || !begun) return none;
    if (lost > 0 || count() >= capacity) {
      ++lost;
      return none;
    }
    if (count() > 0 && resident != segment_of(count())) {
      invalidate();
      return none;
    }
    slots.push_back(order_slot);
    const int m = count(), j = segment_of(m);
    Write w{local_column(m + 1, j), -1, m - 1};
    if (j != resident) w.checkpoint = j, resident = j;
    return w;
  }
  // the last step was withdrawn (fc_undo_step): its column inside the segment is free again.  A step withdrawn from in front of
  // begin() ends the tape, and so does one that opened a segment (the previous segment's columns are overwritten) or one whose
  // segment the buffer no longer holds.
  void pop() {
    if (capacity == 0 || !begun) return;
    if (lost > 0) {
      --lost;
      return;
    }
    const int m = count();
    if (m == 0 || resident != segment_of(m) || (m > 1 && segment_of(m - 1) != segment_of(m))) {
      invalidate();
      return;
    }
    slots.pop_back();
  }

  // The march over a run of n steps: segments n_segments(n) - 1 .. 0; replay(j, n): segment j is recomputed from checkpoint j first.
  // What the buffer holds serves only the segment the march starts with -- the one the forward run left there: every replay
  // overwrites it.  (A march over a run of several segments leaves segment 0 behind: marched again, every segment is recomputed.)
  bool replay(int j, int n) const { return !(j == resident && j == n_segments(n) - 1); }
  // forward steps a march over n steps recomputes
  int replayed_steps(int n) const {
    int r = 0;
    for (int j = n_segments(n) - 1; j >= 0; --j)
      if (replay(j, n)) r += seg_len(j, n);
    return r;
  }
  // a march has walked down to segment 0: that is what the buffer holds now
  void marched() { resident = 0; }

  // does the tape hold exactly a run of n_steps steps whose first step ran on first_slot and whose later ones ran on later_slot?
  // `why` (optional) receives the reason when it does not (the dense tape's wording).
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
