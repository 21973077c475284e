// Stand-alone check of the DENSE adjoint state tape's host bookkeeping -- TEST INFRASTRUCTURE, driven by tests/test_adjoint_tape_host.py.
// The dense tape is the one-segment form of FcAdjointSegments (flowcontrol_amd/csrc/fc_adjoint_segments.hpp): reserve(n, n).  No device:
// the header counts columns, keeps the order slot of every taped step and says whether the tape covers a run.  Two parts:
//   * the checks the dense tape's own type had, on the one-segment form: one line per check, "<name> ok" or "<name> FAILED <what>", and
//     "refusal <key>: <reason>" for every refusal reason of covers();
//   * DenseTapeModel below -- the body of that former type, kept here as the model -- against the one-segment form over seeded random
//     begin / push / pop / invalidate / marched sequences: every field, every returned column and covers() with its reason after
//     every operation.
// Exits non-zero if a check failed.
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "fc_adjoint_segments.hpp"

// the dense tape as it was written on its own: capacity + 2 columns, column 0 = x_{-1}, column j + 1 = x_j
struct DenseTapeModel {
  int capacity = 0;
  bool begun = false;
  int lost = 0;
  std::vector<int> slots;

  int count() const { return (int)slots.size(); }
  bool overflowed() const { return lost > 0; }
  int columns() const { return capacity > 0 ? capacity + 2 : 0; }
  void reserve(int cap) {
    capacity = cap > 0 ? cap : 0;
    invalidate();
  }
  void invalidate() {
    begun = false;
    lost = 0;
    slots.clear();
  }
  bool begin() {
    if (capacity == 0) return false;
    invalidate();
    begun = true;
    return true;
  }
  int push(int order_slot) {
    if (capacity == 0 || !begun) return -1;
    if (lost > 0 || count() >= capacity) {
      ++lost;
      return -1;
    }
    slots.push_back(order_slot);
    return count() + 1;
  }
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

static int failures = 0;

static void check(const char* name, bool ok, const std::string& what = "") {
  if (ok) {
    std::printf("%s ok\n", name);
  } else {
    std::printf("%s FAILED %s\n", name, what.c_str());
    ++failures;
  }
}

static std::string refusal(const FcAdjointSegments& t, int n, int first, int later) {
  std::string why;
  const bool ok = t.covers(n, first, later, &why);
  return ok ? std::string() : why;
}

// the one-segment form and the model agree in every field and in covers() for every n in 0 .. 7 and both first slots; "" if they do
static std::string difference(const FcAdjointSegments& t, const DenseTapeModel& m) {
  if (t.capacity != m.capacity || t.every != m.capacity) return "capacity / every";
  if (t.begun != m.begun || t.lost != m.lost || t.slots != m.slots || t.count() != m.count() || t.overflowed() != m.overflowed()) return "begun / lost / slots";
  if (t.resident != 0) return "resident";
  if (t.buffer_columns() != m.columns()) return "buffer_columns";
  for (int n = 0; n <= 7; ++n)
    for (int first = 0; first < 2; ++first) {
      std::string a, b;
      if (t.covers(n, first, 1, &a) != m.covers(n, first, 1, &b) || a != b) return "covers(" + std::to_string(n) + ", " + std::to_string(first) + "): '" + a + "' / '" + b + "'";
    }
  for (int n = 1; n <= m.capacity; ++n)  // a march over the dense tape has nothing to replay
    if (t.n_segments(n) != 1 || t.replay(0, n) || t.replayed_steps(n) != 0 || t.seg_first(0) != 1 || t.seg_last(0, n) != n || t.local_column(n + 1, 0) != n + 1)
      return "segments of a run of " + std::to_string(n);
  return "";
}

// seeded random sequences on both; the first difference, with the sequence and operation it showed at
static std::string random_comparison(int n_sequences, int n_ops, long long* n_done) {
  std::mt19937 rng(20240607u);
  for (int s = 0; s < n_sequences; ++s) {
    const int cap = (int)(rng() % 7u);  // 0 .. 6
    FcAdjointSegments t;
    DenseTapeModel m;
    t.reserve(cap, cap), m.reserve(cap);
    std::string d = difference(t, m);
    for (int i = 0; i < n_ops && d.empty(); ++i, ++*n_done) {
      const unsigned op = rng() % 16u;  // pushes dominate, so that tapes fill and overflow
      if (op == 0) {
        if (t.begin() != m.begin()) d = "begin()";
      } else if (op == 1) {
        t.invalidate(), m.invalidate();
      } else if (op == 2) {
        t.marched();  // (the model has no such call: a march changes nothing of a dense tape)
      } else if (op < 7) {
        t.pop(), m.pop();
      } else {
        const int slot = (int)(rng() % 2u);
        const FcAdjointSegments::Write w = t.push(slot);
        const int col = m.push(slot);
        if (w.column != col || w.checkpoint != -1 || w.row != (col < 0 ? -1 : m.count() - 1)) d = "push(): column " + std::to_string(w.column) + " / " + std::to_string(col);
        if (t.next_step() != ((m.capacity > 0 && m.begun && m.lost == 0 && m.count() < m.capacity) ? m.count() + 1 : 0)) d = "next_step()";
      }
      if (d.empty()) d = difference(t, m);
      if (!d.empty()) d = "sequence " + std::to_string(s) + " (capacity " + std::to_string(cap) + "), operation " + std::to_string(i) + ": " + d;
    }
    if (!d.empty()) return d;
  }
  return "";
}

int main() {
  const int BDF1 = 0, BDF2 = 1;
  {  // no tape: every call is a no-op, nothing is to be written
    FcAdjointSegments t;
    check("none_push", t.push(BDF1).column == -1 && t.count() == 0 && !t.overflowed() && t.buffer_columns() == 0);
    t.pop();
    check("none_begin", !t.begin() && !t.begun);
    const std::string r = refusal(t, 1, BDF1, BDF2);
    std::printf("refusal none: %s\n", r.c_str());
    check("none_covers", !r.empty());
  }
  {  // reserved, not begun: steps are not taped
    FcAdjointSegments t;
    t.reserve(3, 3);
    check("reserved_columns", t.buffer_columns() == 5 && t.capacity == 3 && !t.begun);
    check("reserved_push", t.push(BDF2).column == -1 && t.count() == 0 && !t.overflowed());
    const std::string r = refusal(t, 0, BDF1, BDF2);
    std::printf("refusal not_begun: %s\n", r.c_str());
    check("reserved_covers", !r.empty());
  }
  {  // begin, push to the capacity, overflow, pop back
    FcAdjointSegments t;
    t.reserve(3, 3);
    check("begin", t.begin() && t.begun && t.count() == 0);
    check("push_columns", t.push(BDF1).column == 2 && t.push(BDF2).column == 3 && t.push(BDF2).column == 4 && t.count() == 3);
    check("covers_full", t.covers(3, BDF1, BDF2) && refusal(t, 3, BDF1, BDF2).empty());
    check("overflow", t.push(BDF2).column == -1 && t.overflowed() && t.count() == 3 && t.lost == 1);
    check("overflow_again", t.push(BDF2).column == -1 && t.lost == 2 && t.count() == 3);
    std::string r = refusal(t, 3, BDF1, BDF2);
    std::printf("refusal overflowed: %s\n", r.c_str());
    check("overflow_covers", !r.empty());
    t.pop();
    check("pop_lost", t.overflowed() && t.lost == 1 && t.count() == 3);
    t.pop();
    check("pop_lost_all", !t.overflowed() && t.count() == 3 && t.covers(3, BDF1, BDF2));
    t.pop();
    check("pop_column", t.count() == 2 && t.push(BDF2).column == 4 && t.count() == 3);
    r = refusal(t, 2, BDF1, BDF2);
    std::printf("refusal count: %s\n", r.c_str());
    check("count_covers", !r.empty() && !t.covers(4, BDF1, BDF2));
    r = refusal(t, 3, BDF2, BDF2);
    std::printf("refusal first_slot: %s\n", r.c_str());
    check("first_slot_covers", !r.empty());
  }
  {  // a later step that did not run on BDF2
    FcAdjointSegments t;
    t.reserve(4, 4);
    t.begin();
    t.push(BDF2), t.push(BDF2), t.push(BDF1);
    const std::string r = refusal(t, 3, BDF2, BDF2);
    std::printf("refusal later_slot: %s\n", r.c_str());
    check("later_slot_covers", !r.empty() && t.covers(2, BDF2, BDF2) == false);
    t.pop();
    check("later_slot_popped", t.covers(2, BDF2, BDF2));
  }
  {  // invalidate ends the tape and keeps the reservation; begin starts over; a step withdrawn from in front of begin ends it too
    FcAdjointSegments t;
    t.reserve(2, 2);
    t.begin();
    t.push(BDF1);
    t.invalidate();
    check("invalidate", !t.begun && t.count() == 0 && t.capacity == 2 && t.push(BDF2).column == -1 && !t.overflowed());
    check("invalidate_covers", !refusal(t, 0, BDF1, BDF2).empty());
    check("begin_again", t.begin() && t.push(BDF1).column == 2 && t.covers(1, BDF1, BDF2));
    t.begin();
    check("begin_resets", t.count() == 0 && !t.overflowed() && t.begun);
    t.pop();
    check("pop_before_begin", !t.begun && t.push(BDF1).column == -1);
    t.begin();
    t.push(BDF1), t.push(BDF2), t.push(BDF2);
    check("begin_clears_overflow_setup", t.overflowed());
    t.begin();
    check("begin_clears_overflow", !t.overflowed() && t.count() == 0);
    t.reserve(0, 0);
    check("release", t.capacity == 0 && t.buffer_columns() == 0 && !t.begun && t.push(BDF1).column == -1);
    t.reserve(-5, -5);
    check("negative_capacity", t.capacity == 0);
  }
  {  // many steps: the slots vector grows and shrinks without trouble
    FcAdjointSegments t;
    t.reserve(1000, 1000);
    t.begin();
    bool ok = true;
    for (int j = 1; j <= 1000; ++j) ok = ok && t.push(j == 1 ? BDF1 : BDF2).column == j + 1;
    check("long_run", ok && t.covers(1000, BDF1, BDF2) && !t.covers(1000, BDF2, BDF2));
    for (int j = 0; j < 1000; ++j) t.pop();
    check("long_pop", t.count() == 0 && t.begun && t.covers(0, BDF1, BDF2));
  }
  {  // the model of the dense tape and the one-segment form, operation by operation
    long long n_done = 0;
    const std::string d = random_comparison(20000, 60, &n_done);
    std::printf("model comparison: %lld operations\n", n_done);
    check("model_comparison", d.empty() && n_done == 20000LL * 60, d);
  }
  std::printf("%s\n", failures ? "CHECK FAILED" : "CHECK OK");
  return failures ? 1 : 0;
}
