// Stand-alone check of the closed-loop tape's host bookkeeping (flowcontrol_amd/csrc/fc_adjoint_loop_tape.hpp) -- TEST INFRASTRUCTURE,
// driven by tests/test_adjoint_loop_tape_host.py.  No device: the header counts rows, keeps the order slot of every taped step, the
// signal row of the first one and the step counter, and says whether the tape holds a run.  Prints one line per check, "<name> ok" or
// "<name> FAILED <what>", and "refusal <key>: <reason>" for every refusal reason of covers(); exits non-zero if a check failed.
#include <cstdio>
#include <string>
#include <vector>

#include "fc_adjoint_loop_tape.hpp"

static int failures = 0;

static void check(const char* name, bool ok, const std::string& what = "") {
  if (ok) {
    std::printf("%s ok\n", name);
  } else {
    std::printf("%s FAILED %s\n", name, what.c_str());
    ++failures;
  }
}

static std::string refusal(const FcLoopTape& t, int n, int first, int later) {
  std::string why;
  const bool ok = t.covers(n, first, later, &why);
  return ok ? std::string() : why;
}

int main() {
  const int BDF1 = 0, BDF2 = 1;
  {  // no tape: every call is a no-op
    FcLoopTape t;
    check("none_push", t.push(BDF1, 0, -1) == -1 && t.count() == 0 && !t.overflowed());
    check("none_begin", !t.begin(0) && !t.begun);
    t.end("x");
    t.mark_bad();
    check("none_end", !t.begun && !t.bad && t.ended_by.empty());
    const std::string r = refusal(t, 1, BDF1, BDF2);
    std::printf("refusal none: %s\n", r.c_str());
    check("none_covers", !r.empty());
  }
  {  // reserved, not begun: steps are not taped
    FcLoopTape t;
    t.reserve(3);
    check("reserved", t.capacity == 3 && !t.begun && t.count() == 0);
    check("reserved_push", t.push(BDF2, 7, 0) == -1 && t.count() == 0 && !t.overflowed());
    const std::string r = refusal(t, 0, BDF1, BDF2);
    std::printf("refusal not_begun: %s\n", r.c_str());
    check("reserved_covers", !r.empty());
  }
  {  // begin, push to the capacity across two calls, overflow
    FcLoopTape t;
    t.reserve(3);
    check("begin", t.begin(10) && t.begun && t.count() == 0 && t.next_step == 10);
    check("push_rows", t.push(BDF1, 10, 4) == 0 && t.push(BDF2, 11, 5) == 1 && t.push(BDF2, 12, 6) == 2 && t.count() == 3);
    check("row0", t.row0 == 4 && t.next_step == 13);
    check("covers_full", t.covers(3, BDF1, BDF2) && refusal(t, 3, BDF1, BDF2).empty());
    std::string r = refusal(t, 2, BDF1, BDF2);
    std::printf("refusal count: %s\n", r.c_str());
    check("count_covers", !r.empty() && !t.covers(4, BDF1, BDF2));
    r = refusal(t, 3, BDF2, BDF2);
    std::printf("refusal first_slot: %s\n", r.c_str());
    check("first_slot_covers", !r.empty());
    check("overflow", t.push(BDF2, 13, 7) == -1 && t.overflowed() && t.count() == 3 && t.lost == 1);
    check("overflow_again", t.push(BDF2, 14, 8) == -1 && t.lost == 2 && t.count() == 3);
    r = refusal(t, 3, BDF1, BDF2);
    std::printf("refusal overflowed: %s\n", r.c_str());
    check("overflow_covers", !r.empty() && !t.covers(5, BDF1, BDF2));
    check("begin_clears_overflow", t.begin(15) && !t.overflowed() && t.count() == 0 && t.row0 == -1);
  }
  {  // a later step that did not run on BDF2
    FcLoopTape t;
    t.reserve(4);
    t.begin(0);
    t.push(BDF2, 0, -1), t.push(BDF2, 1, -1), t.push(BDF1, 2, -1);
    const std::string r = refusal(t, 3, BDF2, BDF2);
    std::printf("refusal later_slot: %s\n", r.c_str());
    check("later_slot_covers", !r.empty() && !t.covers(2, BDF2, BDF2));
    check("no_signals_row0", t.row0 == -1);
  }
  {  // a non-finite forward run
    FcLoopTape t;
    t.reserve(4);
    t.begin(3);
    t.push(BDF1, 3, 0), t.push(BDF2, 4, 1);
    check("good_run", t.covers(2, BDF1, BDF2));
    t.mark_bad();
    const std::string r = refusal(t, 2, BDF1, BDF2);
    std::printf("refusal bad: %s\n", r.c_str());
    check("bad_covers", !r.empty());
    check("begin_clears_bad", t.begin(5) && !t.bad);
  }
  {  // end() ends the tape, keeps the reservation and says why; begin starts over
    FcLoopTape t;
    t.reserve(2);
    t.begin(0);
    t.push(BDF1, 0, -1);
    t.end("fc_set_controllers");
    check("end", !t.begun && t.count() == 0 && t.capacity == 2 && t.push(BDF2, 1, -1) == -1 && !t.overflowed());
    const std::string r = refusal(t, 1, BDF1, BDF2);
    std::printf("refusal ended: %s\n", r.c_str());
    check("end_covers", !r.empty());
    t.end("something later");  // (not begun: the first reason stays)
    check("end_keeps_reason", t.ended_by == "fc_set_controllers");
    check("begin_again", t.begin(1) && t.ended_by.empty() && t.push(BDF1, 1, -1) == 0 && t.covers(1, BDF1, BDF2));
    t.reserve(0);
    check("release", t.capacity == 0 && !t.begun && t.push(BDF1, 2, -1) == -1);
    t.reserve(-5);
    check("negative_capacity", t.capacity == 0);
  }
  {  // a step outside the closed loop moves the counter: the next taped step ends the tape
    FcLoopTape t;
    t.reserve(5);
    t.begin(100);
    t.push(BDF1, 100, -1), t.push(BDF2, 101, -1);
    check("foreign_step", t.push(BDF2, 103, -1) == -1 && !t.begun && t.count() == 0);
    const std::string r = refusal(t, 2, BDF1, BDF2);
    std::printf("refusal foreign_step: %s\n", r.c_str());
    check("foreign_step_covers", !r.empty());
  }
  {  // many steps
    FcLoopTape t;
    t.reserve(1000);
    t.begin(0);
    bool ok = true;
    for (int j = 0; j < 1000; ++j) ok = ok && t.push(j == 0 ? BDF1 : BDF2, (uint64_t)j, j) == j;
    check("long_run", ok && t.covers(1000, BDF1, BDF2) && !t.covers(1000, BDF2, BDF2) && t.row0 == 0);
  }
  std::printf("%s\n", failures ? "CHECK FAILED" : "CHECK OK");
  return failures ? 1 : 0;
}
