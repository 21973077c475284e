// CPU check of the step-record protocol (flowcontrol_amd/csrc/fc_record.hpp): records are built with the fold the kernels use
// and handed to the readers fc_hip.hip calls.  Prints "key accepted tried" lines; tests/test_record_host.py asserts on them.
#include <cstdio>
#include <vector>

#include "../../flowcontrol_amd/csrc/fc_record.hpp"

using namespace fc_rec;

static double noise(unsigned& state) {  // distinct, finite, non-trivial bit patterns
  state = state * 1664525u + 1013904223u;
  return 1.0 + (double)(state >> 8) / 16777216.0 + (double)(state & 255u) * 1e-9;
}

// what fc_publish does: the payload, the two checksums of fold_step, the sequence word
static void publish_step(double* rec, const std::vector<double>& y, double E, double r2, double b2, double flag, double seq) {
  const int n_sens = (int)y.size();
  const Fold f = fold_step(seq, n_sens, [&](int q) { return rec[kY + q] = y[(size_t)q]; }, E, r2, b2, flag);
  rec[kE] = E, rec[kR2] = r2, rec[kB2] = b2, rec[kFlag] = flag;
  rec[kXor] = from_bits(f.x), rec[kSum] = from_bits(f.w), rec[kSeq] = seq;
}
// what fc_publish_late does
static void publish_late(double* rec, double E, double r2, double b2, double gave_up, double seq) {
  const Fold f = fold_late(seq, E, r2, b2, gave_up);
  rec[kLateE] = E, rec[kLateR2] = r2, rec[kLateB2] = b2, rec[kLateGaveUp] = gave_up;
  rec[kLateXor] = from_bits(f.x), rec[kLateSum] = from_bits(f.w), rec[kLateSeq] = seq;
}

struct Tally {
  const char* key;
  int accepted = 0, tried = 0;
  void operator()(bool ok) { accepted += ok ? 1 : 0, ++tried; }
  ~Tally() { std::printf("%s %d %d\n", key, accepted, tried); }
};

// every way the test damages one word: another value, one flipped mantissa bit, the sign bit, zero
static std::vector<double> damaged(double v, unsigned& rng) {
  return {noise(rng), from_bits(bits(v) ^ 1ull), from_bits(bits(v) ^ (1ull << 63)), v == 0.0 ? 1.0 : 0.0};
}

static void check_step(int n_sens, unsigned seed) {
  unsigned rng = seed;
  std::vector<double> page((size_t)kRecStride);
  for (double& w : page) w = noise(rng);
  std::vector<double> y((size_t)n_sens);
  for (double& v : y) v = noise(rng);
  const double seq = 41.0;
  publish_step(page.data(), y, noise(rng), noise(rng), noise(rng), 1.0, seq);
  std::vector<int> payload;
  for (int q = 0; q < n_sens; ++q) payload.push_back(kY + q);
  for (int w : {kE, kR2, kB2, kFlag}) payload.push_back(w);
  {
    Tally t{"step_intact"};
    t(step_record_ok(page.data(), n_sens, seq));
  }
  {  // the previous step's record is still there / the sequence word arrived and nothing else did
    Tally t{"step_stale_seq"};
    t(step_record_ok(page.data(), n_sens, seq + 1.0));
    std::vector<double> r = page;
    r[kSeq] = seq - 1.0;
    t(step_record_ok(r.data(), n_sens, seq));
    r[kSeq] = seq + 1.0;
    t(step_record_ok(r.data(), n_sens, seq + 1.0));
  }
  {
    Tally t{"step_payload_word"};
    for (int w : payload)
      for (double v : damaged(page[(size_t)w], rng)) {
        std::vector<double> r = page;
        r[(size_t)w] = v;
        t(step_record_ok(r.data(), n_sens, seq));
      }
  }
  {
    Tally t{"step_checksum_word"};
    for (int w : {kXor, kSum})
      for (double v : damaged(page[(size_t)w], rng)) {
        std::vector<double> r = page;
        r[(size_t)w] = v;
        t(step_record_ok(r.data(), n_sens, seq));
      }
  }
  {  // two payload words exchanged: the XOR alone cannot see it (xor_blind counts that), the odd-weighted sum does
    Tally t{"step_exchanged"}, blind{"step_exchanged_xor_blind"};
    for (size_t i = 0; i < payload.size(); ++i)
      for (size_t j = i + 1; j < payload.size(); ++j) {
        std::vector<double> r = page;
        std::swap(r[(size_t)payload[i]], r[(size_t)payload[j]]);
        t(step_record_ok(r.data(), n_sens, seq));
        const Fold f = fold_step(seq, n_sens, [&](int q) { return r[(size_t)(kY + q)]; }, r[kE], r[kR2], r[kB2], r[kFlag]);
        blind(f.x == bits(r[kXor]));
      }
  }
  {  // nothing but the named words counts: controls, force amplitudes, unused sensor words, gaps, the late records
    Tally t{"step_other_words"};
    std::vector<bool> named((size_t)kRecStride, false);
    for (int w : payload) named[(size_t)w] = true;
    for (int w : {kSeq, kXor, kSum}) named[(size_t)w] = true;
    std::vector<double> r = page;
    for (int w = 0; w < kRecStride; ++w)
      if (!named[(size_t)w]) {
        r[(size_t)w] = noise(rng);
        t(step_record_ok(r.data(), n_sens, seq));
      }
  }
}

static void check_late(unsigned seed) {
  unsigned rng = seed;
  std::vector<double> page((size_t)kLateWords);
  for (double& w : page) w = noise(rng);
  const double seq = 7.0;
  publish_late(page.data(), noise(rng), noise(rng), noise(rng), 1.0, seq);
  const std::vector<int> payload = {kLateE, kLateR2, kLateB2, kLateGaveUp};
  {
    Tally t{"late_intact"};
    t(late_record_ok(page.data(), seq));
  }
  {
    Tally t{"late_stale_seq"};
    t(late_record_ok(page.data(), seq + 2.0));  // (the same parity, two steps on)
    std::vector<double> r = page;
    r[kLateSeq] = seq - 2.0;
    t(late_record_ok(r.data(), seq));
    r[kLateSeq] = seq + 2.0;
    t(late_record_ok(r.data(), seq + 2.0));
  }
  {
    Tally t{"late_payload_word"};
    for (int w : payload)
      for (double v : damaged(page[(size_t)w], rng)) {
        std::vector<double> r = page;
        r[(size_t)w] = v;
        t(late_record_ok(r.data(), seq));
      }
  }
  {
    Tally t{"late_checksum_word"};
    for (int w : {kLateXor, kLateSum})
      for (double v : damaged(page[(size_t)w], rng)) {
        std::vector<double> r = page;
        r[(size_t)w] = v;
        t(late_record_ok(r.data(), seq));
      }
  }
  {
    Tally t{"late_exchanged"};
    for (size_t i = 0; i < payload.size(); ++i)
      for (size_t j = i + 1; j < payload.size(); ++j) {
        std::vector<double> r = page;
        std::swap(r[(size_t)payload[i]], r[(size_t)payload[j]]);
        t(late_record_ok(r.data(), seq));
      }
  }
  {
    Tally t{"late_other_words"};
    std::vector<double> r = page;
    for (int w = 0; w < kLateWords; ++w)
      if (w != kLateSeq && w != kLateXor && w != kLateSum && w != kLateE && w != kLateR2 && w != kLateB2 && w != kLateGaveUp) {
        r[(size_t)w] = noise(rng);
        t(late_record_ok(r.data(), seq));
      }
  }
}

int main() {
  // the fold itself: seq with weight 1, then 3, 5, ... over the words in order
  {
    Fold f(2.0);
    f.add(3.0);
    f.add(5.0);
    const u64 x = bits(2.0) ^ bits(3.0) ^ bits(5.0), w = bits(2.0) + 3 * bits(3.0) + 5 * bits(5.0);
    std::printf("fold %d 1\n", (f.x == x && f.w == w && f.k == 7) ? 1 : 0);
  }
  for (int n_sens : {0, 1, 3, kMaxSens}) check_step(n_sens, 12345u + (unsigned)n_sens);
  check_late(99u);
  return 0;
}
