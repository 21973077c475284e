// Stand-alone check of the checkpointed state tape's host bookkeeping (flowcontrol_amd/csrc/fc_adjoint_segments.hpp) -- TEST
// INFRASTRUCTURE, driven by tests/test_adjoint_segments_host.py.  No device: the "states" are their indices (x_m is the number m), the
// segment buffer and the checkpoint store are arrays of such numbers that are written exactly where the header says, and a march over
// them must read x_m at backward step m.  For every n in 1 .. 40 and c in 1 .. n + 2 it prints
//   "case <n> <c> <columns> <replayed> | <forward writes: column:checkpoint ...> | <march: m:column ...> | <segments: j:replay ...>"
// (the Python test restates these tables on its own) and "<name> ok" / "<name> FAILED <what>" per check; "refusal <key>: <reason>" for
// every refusal reason of covers().  Exits non-zero if a check failed.
#include <cstdio>
#include <string>
#include <vector>

#include "fc_adjoint_segments.hpp"

static int failures = 0;

static void check(const std::string& name, bool ok, const std::string& what = "") {
  if (ok) {
    std::printf("%s ok\n", name.c_str());
  } else {
    std::printf("%s FAILED %s\n", name.c_str(), what.c_str());
    ++failures;
  }
}

static std::string refusal(const FcAdjointSegments& t, int n, int first, int later) {
  std::string why;
  return t.covers(n, first, later, &why) ? std::string() : why;
}

constexpr int kNone = -1000;  // a column nobody has written

// the device side of the tape, with state indices for states
struct Store {
  std::vector<int> buf, ckpt;
  explicit Store(const FcAdjointSegments& t) : buf((size_t)t.buffer_columns(), kNone), ckpt(2 * (size_t)t.checkpoints(), kNone) {}
  void begin() { buf[0] = ckpt[0] = -1, buf[1] = ckpt[1] = 0; }
  // what a forward or replayed step m does with a Write
  void write(const FcAdjointSegments& t, const FcAdjointSegments::Write& w, int m) {
    if (w.checkpoint >= 0) {
      ckpt[2 * (size_t)w.checkpoint] = buf[(size_t)t.every], ckpt[2 * (size_t)w.checkpoint + 1] = buf[(size_t)t.every + 1];
      buf[0] = ckpt[2 * (size_t)w.checkpoint], buf[1] = ckpt[2 * (size_t)w.checkpoint + 1];
    }
    buf[(size_t)w.column] = m;
  }
};

static bool walk(const FcAdjointSegments& t, Store& s, int n, int replayed, std::string* march_out, std::string* segs_out);

static bool one_case(int n, int c) {
  const int BDF1 = 0, BDF2 = 1;
  FcAdjointSegments t;
  t.reserve(n, c);
  bool ok = t.columns() == 2 * ((n + c - 1) / c) + c + 2 && t.columns() == FcAdjointSegments::columns_for(n, c);
  Store s(t);
  t.begin();
  s.begin();
  std::string line = "case " + std::to_string(n) + " " + std::to_string(c) + " " + std::to_string(t.columns());
  std::string writes, march, segs;
  for (int m = 1; m <= n; ++m) {
    ok = ok && t.next_step() == m;
    const FcAdjointSegments::Write w = t.push(m == 1 ? BDF1 : BDF2);
    ok = ok && w.column >= 2 && w.column < t.buffer_columns() && w.row == m - 1;
    ok = ok && (w.checkpoint < 0 || (w.checkpoint < t.checkpoints() && w.checkpoint == t.segment_of(m)));
    if (!ok) return false;
    s.write(t, w, m);
    writes += " " + std::to_string(w.column) + ":" + std::to_string(w.checkpoint);
  }
  ok = ok && t.covers(n, BDF1, BDF2) && t.next_step() == 0;
  const int S = t.n_segments(n);
  ok = ok && t.resident == S - 1;
  const int replayed = t.replayed_steps(n);
  ok = ok && replayed == n - t.seg_len(S - 1, n);
  ok = ok && walk(t, s, n, replayed, &march, &segs);
  t.marched();
  // a second march finds segment 0 in the buffer, which only a run of one segment can use: every segment is recomputed
  ok = ok && t.resident == 0 && t.replayed_steps(n) == (S == 1 ? 0 : n) && walk(t, s, n, t.replayed_steps(n), nullptr, nullptr);
  std::printf("%s %d |%s |%s |%s\n", line.c_str(), replayed, writes.c_str(), march.c_str(), segs.c_str());
  return ok;
}

// the march: segments S - 1 .. 0; a replayed one starts from its checkpoint and rewrites columns 2 ..
static bool walk(const FcAdjointSegments& t, Store& s, int n, int replayed, std::string* march_out, std::string* segs_out) {
  const int c = t.every, S = t.n_segments(n);
  std::string march, segs;
  bool ok = true;
  int expect = n, done = 0;
  for (int j = S - 1; j >= 0; --j) {
    segs += " " + std::to_string(j) + ":" + (t.replay(j, n) ? "1" : "0");
    if (t.replay(j, n)) {
      ok = ok && s.ckpt[2 * (size_t)j] == (j == 0 ? -1 : j * c - 1) && s.ckpt[2 * (size_t)j + 1] == j * c;  // the pair the forward run stored
      s.buf[0] = s.ckpt[2 * (size_t)j], s.buf[1] = s.ckpt[2 * (size_t)j + 1];
      for (int m = t.seg_first(j); m <= t.seg_last(j, n); ++m) {
        // a replayed step reads the two columns in front of its own
        const int col = t.local_column(m + 1, j);
        ok = ok && col >= 2 && col < t.buffer_columns() && s.buf[(size_t)col - 1] == m - 1 && s.buf[(size_t)col - 2] == (m == 1 ? -1 : m - 2);
        if (!ok) return false;
        s.buf[(size_t)col] = m;
        ++done;
      }
    }
    for (int m = t.seg_last(j, n); m >= t.seg_first(j); --m) {
      const int col = t.local_column(m + 1, j);
      ok = ok && m == expect && col >= 0 && col < t.buffer_columns() && s.buf[(size_t)col] == m;  // every m once, descending, reading x_m
      if (!ok) return false;
      --expect;
      march += " " + std::to_string(m) + ":" + std::to_string(col);
    }
  }
  ok = ok && expect == 0 && done == replayed;
  // the two state-gradient products behind the loop read x_0 and x_{-1} in segment 0
  ok = ok && s.buf[(size_t)t.local_column(1, 0)] == 0 && s.buf[(size_t)t.local_column(0, 0)] == -1;
  if (march_out) *march_out = march;
  if (segs_out) *segs_out = segs;
  return ok;
}

int main() {
  const int BDF1 = 0, BDF2 = 1;
  for (int n = 1; n <= 40; ++n)
    for (int c = 1; c <= n + 2; ++c) check("case_n" + std::to_string(n) + "_c" + std::to_string(c), one_case(n, c));
  {  // no tape: every call is a no-op
    FcAdjointSegments t;
    check("none_push", t.push(BDF1).column == -1 && t.count() == 0 && !t.overflowed() && t.columns() == 0 && t.next_step() == 0);
    t.pop();
    check("none_begin", !t.begin() && !t.begun);
    const std::string r = refusal(t, 1, BDF1, BDF2);
    std::printf("refusal none: %s\n", r.c_str());
    check("none_covers", !r.empty());
    t.reserve(5, 0);
    check("every_zero", t.capacity == 0 && t.columns() == 0);
    t.reserve(0, 3);
    check("capacity_zero", t.capacity == 0 && t.every == 0);
  }
  {  // reserved, not begun
    FcAdjointSegments t;
    t.reserve(7, 3);
    check("reserved_columns", t.columns() == 11 && t.checkpoints() == 3 && t.buffer_columns() == 5 && !t.begun);
    check("reserved_push", t.push(BDF2).column == -1 && t.count() == 0 && !t.overflowed());
    const std::string r = refusal(t, 0, BDF1, BDF2);
    std::printf("refusal not_begun: %s\n", r.c_str());
    check("reserved_covers", !r.empty());
  }
  {  // overflow and pop
    FcAdjointSegments t;
    t.reserve(3, 2);
    check("begin", t.begin() && t.begun && t.count() == 0);
    check("push_columns", t.push(BDF1).column == 2 && t.push(BDF2).column == 3 && t.push(BDF2).checkpoint == 1 && t.count() == 3);
    check("overflow", t.push(BDF2).column == -1 && t.overflowed() && t.count() == 3 && t.lost == 1 && t.next_step() == 0);
    std::string r = refusal(t, 3, BDF1, BDF2);
    std::printf("refusal overflowed: %s\n", r.c_str());
    check("overflow_covers", !r.empty());
    t.pop();
    check("pop_lost", !t.overflowed() && t.count() == 3 && t.covers(3, BDF1, BDF2));
    r = refusal(t, 2, BDF1, BDF2);
    std::printf("refusal count: %s\n", r.c_str());
    check("count_covers", !r.empty());
    r = refusal(t, 3, BDF2, BDF2);
    std::printf("refusal first_slot: %s\n", r.c_str());
    check("first_slot_covers", !r.empty());
    t.pop();  // step 3 opened segment 1: the tape ends
    check("pop_across_boundary", !t.begun && t.count() == 0 && t.push(BDF2).column == -1);
  }
  {  // pop inside a segment frees the column; a later step that did not run on BDF2
    FcAdjointSegments t;
    t.reserve(6, 3);
    t.begin();
    t.push(BDF2), t.push(BDF2);
    t.pop();
    check("pop_inside", t.begun && t.count() == 1 && t.next_step() == 2);
    const FcAdjointSegments::Write w = t.push(BDF1);
    check("pop_inside_column", w.column == 3 && w.checkpoint == -1 && w.row == 1);
    const std::string r = refusal(t, 2, BDF2, BDF2);
    std::printf("refusal later_slot: %s\n", r.c_str());
    check("later_slot_covers", !r.empty());
    t.pop(), t.pop();
    check("pop_to_begin", t.begun && t.count() == 0);
    t.pop();
    check("pop_before_begin", !t.begun);
  }
  {  // behind a march that left segment 0 in the buffer the run cannot go on, and its last step cannot be withdrawn
    FcAdjointSegments t;
    t.reserve(8, 2);
    t.begin();
    for (int m = 1; m <= 5; ++m) t.push(m == 1 ? BDF1 : BDF2);
    t.marched();
    check("marched_next", t.next_step() == 0 && t.covers(5, BDF1, BDF2));
    FcAdjointSegments u = t;
    check("marched_push", u.push(BDF2).column == -1 && !u.begun);
    u = t;
    u.pop();
    check("marched_pop", !u.begun);
    FcAdjointSegments v;  // one segment: the march leaves the buffer as it was
    v.reserve(4, 9);
    v.begin();
    v.push(BDF1), v.push(BDF2);
    check("one_segment", v.replayed_steps(2) == 0 && !v.replay(0, 2));
    v.marched();
    check("one_segment_goes_on", v.next_step() == 3 && v.push(BDF2).column == 4);
  }
  {  // invalidate keeps the reservation; reserve(0) releases
    FcAdjointSegments t;
    t.reserve(4, 2);
    t.begin();
    t.push(BDF1);
    t.invalidate();
    check("invalidate", !t.begun && t.count() == 0 && t.capacity == 4 && t.every == 2 && t.push(BDF2).column == -1);
    check("begin_again", t.begin() && t.push(BDF1).column == 2 && t.covers(1, BDF1, BDF2));
    t.reserve(0, 0);
    check("release", t.capacity == 0 && t.columns() == 0 && !t.begun);
    t.reserve(-5, 2);
    check("negative_capacity", t.capacity == 0);
  }
  std::printf("%s\n", failures ? "CHECK FAILED" : "CHECK OK");
  return failures ? 1 : 0;
}
