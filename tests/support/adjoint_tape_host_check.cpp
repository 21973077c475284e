// Stand-alone check of the adjoint state tape's host bookkeeping (flowcontrol_amd/csrc/fc_adjoint_tape.hpp) -- TEST INFRASTRUCTURE,
// driven by tests/test_adjoint_tape_host.py.  No device: the header counts columns, keeps the order slot of every taped step and says
// whether the tape covers a run.  Prints one line per check, "<name> ok" or "<name> FAILED <what>", and "refusal <key>: <reason>" for
// every refusal reason of covers(); exits non-zero if a check failed.
#include <cstdio>
#include <string>
#include <vector>

#include "fc_adjoint_tape.hpp"

static int failures = 0;

static void check(const char* name, bool ok, const std::string& what = "") {
  if (ok) {
    std::printf("%s ok\n", name);
  } else {
    std::printf("%s FAILED %s\n", name, what.c_str());
    ++failures;
  }
}

static std::string refusal(const FcAdjointTape& t, int n, int first, int later) {
  std::string why;
  const bool ok = t.covers(n, first, later, &why);
  return ok ? std::string() : why;
}

int main() {
  const int BDF1 = 0, BDF2 = 1;
  {  // no tape: every call is a no-op, nothing is to be written
    FcAdjointTape t;
    check("none_push", t.push(BDF1) == -1 && t.count() == 0 && !t.overflowed() && t.columns() == 0);
    t.pop();
    check("none_begin", !t.begin() && !t.begun);
    const std::string r = refusal(t, 1, BDF1, BDF2);
    std::printf("refusal none: %s\n", r.c_str());
    check("none_covers", !r.empty());
  }
  {  // reserved, not begun: steps are not taped
    FcAdjointTape t;
    t.reserve(3);
    check("reserved_columns", t.columns() == 5 && t.capacity == 3 && !t.begun);
    check("reserved_push", t.push(BDF2) == -1 && t.count() == 0 && !t.overflowed());
    const std::string r = refusal(t, 0, BDF1, BDF2);
    std::printf("refusal not_begun: %s\n", r.c_str());
    check("reserved_covers", !r.empty());
  }
  {  // begin, push to the capacity, overflow, pop back
    FcAdjointTape t;
    t.reserve(3);
    check("begin", t.begin() && t.begun && t.count() == 0);
    check("push_columns", t.push(BDF1) == 2 && t.push(BDF2) == 3 && t.push(BDF2) == 4 && t.count() == 3);
    check("covers_full", t.covers(3, BDF1, BDF2) && refusal(t, 3, BDF1, BDF2).empty());
    check("overflow", t.push(BDF2) == -1 && t.overflowed() && t.count() == 3 && t.lost == 1);
    check("overflow_again", t.push(BDF2) == -1 && t.lost == 2 && t.count() == 3);
    std::string r = refusal(t, 3, BDF1, BDF2);
    std::printf("refusal overflowed: %s\n", r.c_str());
    check("overflow_covers", !r.empty());
    t.pop();
    check("pop_lost", t.overflowed() && t.lost == 1 && t.count() == 3);
    t.pop();
    check("pop_lost_all", !t.overflowed() && t.count() == 3 && t.covers(3, BDF1, BDF2));
    t.pop();
    check("pop_column", t.count() == 2 && t.push(BDF2) == 4 && t.count() == 3);
    r = refusal(t, 2, BDF1, BDF2);
    std::printf("refusal count: %s\n", r.c_str());
    check("count_covers", !r.empty() && !t.covers(4, BDF1, BDF2));
    r = refusal(t, 3, BDF2, BDF2);
    std::printf("refusal first_slot: %s\n", r.c_str());
    check("first_slot_covers", !r.empty());
  }
  {  // a later step that did not run on BDF2
    FcAdjointTape t;
    t.reserve(4);
    t.begin();
    t.push(BDF2), t.push(BDF2), t.push(BDF1);
    const std::string r = refusal(t, 3, BDF2, BDF2);
    std::printf("refusal later_slot: %s\n", r.c_str());
    check("later_slot_covers", !r.empty() && t.covers(2, BDF2, BDF2) == false);
    t.pop();
    check("later_slot_popped", t.covers(2, BDF2, BDF2));
  }
  {  // invalidate ends the tape and keeps the reservation; begin starts over; a step withdrawn from in front of begin ends it too
    FcAdjointTape t;
    t.reserve(2);
    t.begin();
    t.push(BDF1);
    t.invalidate();
    check("invalidate", !t.begun && t.count() == 0 && t.capacity == 2 && t.push(BDF2) == -1 && !t.overflowed());
    check("invalidate_covers", !refusal(t, 0, BDF1, BDF2).empty());
    check("begin_again", t.begin() && t.push(BDF1) == 2 && t.covers(1, BDF1, BDF2));
    t.begin();
    check("begin_resets", t.count() == 0 && !t.overflowed() && t.begun);
    t.pop();
    check("pop_before_begin", !t.begun && t.push(BDF1) == -1);
    t.begin();
    t.push(BDF1), t.push(BDF2), t.push(BDF2);
    check("begin_clears_overflow_setup", t.overflowed());
    t.begin();
    check("begin_clears_overflow", !t.overflowed() && t.count() == 0);
    t.reserve(0);
    check("release", t.capacity == 0 && t.columns() == 0 && !t.begun && t.push(BDF1) == -1);
    t.reserve(-5);
    check("negative_capacity", t.capacity == 0);
  }
  {  // many steps: the slots vector grows and shrinks without trouble
    FcAdjointTape t;
    t.reserve(1000);
    t.begin();
    bool ok = true;
    for (int j = 1; j <= 1000; ++j) ok = ok && t.push(j == 1 ? BDF1 : BDF2) == j + 1;
    check("long_run", ok && t.covers(1000, BDF1, BDF2) && !t.covers(1000, BDF2, BDF2));
    for (int j = 0; j < 1000; ++j) t.pop();
    check("long_pop", t.count() == 0 && t.begun && t.covers(0, BDF1, BDF2));
  }
  std::printf("%s\n", failures ? "CHECK FAILED" : "CHECK OK");
  return failures ? 1 : 0;
}
