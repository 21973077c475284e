// fc_record.hpp — the step record: one definition of its layout, its checksum fold and its host-side readers.
//
// Every time step ends with ONE thread publishing a record into a pinned, host-mapped page that the host polls instead of
// synchronising the stream.  The same page carries the controls in.  The batched path repeats the record per simulation, the
// overlapped tail adds a "late record" per step parity, and a closed-loop run keeps a copy of the page in device memory
// (fc_ctrl_step reads and writes it).  Kernels, host code and tests take every word offset from here.
//
// No HIP dependency: included by device code, by fc_hip.hip host code and by plain C++ (tests/support/record_host_check.cpp).
#pragma once

#ifdef __HIPCC__
#define FC_REC_HD __host__ __device__
#else
#define FC_REC_HD
#endif

namespace fc_rec {

typedef unsigned long long u64;

// ── one simulation's record (word = double) ─────────────────────────────────────────────────────────────────────────
constexpr int kCtrl = 0;     // controls in: u[n_act]
constexpr int kForce = 32;   // body-force amplitudes in: [n_act] (CN: mean of new and old control)
constexpr int kY = 64;       // sensors out: y[n_sens]
constexpr int kE = 128;      // energy
constexpr int kR2 = 129;     // sum r^2 of the residual monitor
constexpr int kB2 = 130;     // sum b^2
constexpr int kFlag = 136;   // non-finite flag (bit 0; partitioned runs sum the word over the ranks)
constexpr int kSeq = 137;    // sequence number of the step that wrote the record
constexpr int kXor = 138;    // checksum: XOR of the folded words' bit patterns
constexpr int kSum = 139;    // checksum: odd-weighted sum modulo 2^64
constexpr int kLateRecB = 144;  // late record of a batched simulation inside its record: + kLateWords x step parity
constexpr int kRecStride = 160;  // doubles per simulation: the page is this layout, repeated

// ── a late record (overlapped tail: residual monitor and energy follow the step record) ─────────────────────────────
constexpr int kLateE = 0, kLateR2 = 1, kLateB2 = 2, kLateSeq = 3, kLateXor = 4, kLateSum = 5;
constexpr int kLateGaveUp = 6;  // the side stream's gate stopped waiting for the step's solve: the three values are not valid
constexpr int kLateWords = 8;

// ── the page ────────────────────────────────────────────────────────────────────────────────────────────────────────
constexpr int kMaxSims = 32;       // records in the page
constexpr int kSeqSlot = 8000;     // batched steps read their sequence number here: + step parity (graph replay: no kernel argument)
constexpr int kLateRec = 8010;     // the single simulation's late records: + kLateWords x step parity
constexpr int kPinDoubles = 8192;  // page size
constexpr int kMaxAct = 32, kMaxSens = 64;  // what one record holds

// ── the partitioned step's tail buffer: each rank's share, summed over the ranks by one all-reduce, then published ──
constexpr int kTailY = 0, kTailE = 64, kTailR2 = 65, kTailB2 = 66, kTailFlag = 72;
constexpr int kTailDoubles = 80;  // exchanged length
constexpr int kTailAlloc = 128;   // allocated (and cleared) length

static_assert(kForce - kCtrl >= kMaxAct && kY - kForce >= kMaxAct, "controls and force amplitudes: n_act <= 32 words each");
static_assert(kE - kY >= kMaxSens, "sensors: n_sens <= 64 words");
// fc_publish and FcCtrlIO::rec_E address (E, r^2, b^2) and (seq, xor, sum) as consecutive words behind one pointer
static_assert(kR2 == kE + 1 && kB2 == kE + 2, "E, r^2, b^2 are consecutive");
static_assert(kXor == kSeq + 1 && kSum == kSeq + 2, "seq and its two checksums are consecutive");
static_assert(kB2 < kFlag && kFlag < kSeq && kSum < kLateRecB, "record words do not overlap");
static_assert(kLateRecB + 2 * kLateWords <= kRecStride, "both parities' late records fit inside a simulation's record");
static_assert(kLateE < kLateSeq && kLateR2 < kLateSeq && kLateB2 < kLateSeq && kLateSum < kLateGaveUp && kLateGaveUp < kLateWords,
              "late record words do not overlap");
static_assert(kRecStride * kMaxSims <= kSeqSlot, "the records end before the sequence slots");
static_assert(kSeqSlot + 2 <= kLateRec, "both parities' sequence slots end before the late records");
static_assert(kLateRec + 2 * kLateWords <= kPinDoubles, "the late records fit inside the page");
static_assert(kTailE - kTailY >= kMaxSens && kTailR2 == kTailE + 1 && kTailB2 == kTailE + 2 && kTailB2 < kTailFlag &&
                  kTailFlag < kTailDoubles && kTailDoubles <= kTailAlloc,
              "tail buffer words do not overlap");

// ── the checksums ───────────────────────────────────────────────────────────────────────────────────────────────────
// The device writes a record with no fence, so its words may become visible to the host in any order.  Two checksums over
// the bit patterns of the sequence number and of every payload word go with it: an XOR, and a position-weighted sum modulo
// 2^64 with odd weights 1, 3, 5, ... (odd: invertible, and two torn words that cancel in the XOR do not cancel in the sum).
// A reader accepts a record only when the sequence word is the expected one AND both checksums fit the words it read.
FC_REC_HD inline u64 bits(double v) {
  u64 u;
  __builtin_memcpy(&u, &v, sizeof u);
  return u;
}
FC_REC_HD inline double from_bits(u64 u) {
  double v;
  __builtin_memcpy(&v, &u, sizeof v);
  return v;
}
struct Fold {
  u64 x, w, k;
  FC_REC_HD explicit Fold(double seq) : x(bits(seq)), w(x), k(3) {}
  FC_REC_HD void add(double v) {
    const u64 b = bits(v);
    x ^= b;
    w += k * b;
    k += 2;
  }
};
// The word ORDER of the two folds, stated here and nowhere else.
// step record: seq, the sensors in index order (sensor(q) is called once per q, ascending), E, r^2, b^2, flag
template <class Sensor>
FC_REC_HD inline Fold fold_step(double seq, int n_sens, Sensor&& sensor, double E, double r2, double b2, double flag) {
  Fold f(seq);
  for (int q = 0; q < n_sens; ++q) f.add(sensor(q));
  f.add(E);
  f.add(r2);
  f.add(b2);
  f.add(flag);
  return f;
}
// late record: seq, E, r^2, b^2, gate-gave-up
FC_REC_HD inline Fold fold_late(double seq, double E, double r2, double b2, double gave_up) {
  Fold f(seq);
  f.add(E);
  f.add(r2);
  f.add(b2);
  f.add(gave_up);
  return f;
}

// ── host-side readers (rec: one simulation's record / one late record, possibly still being written) ───────────────
inline bool step_record_ok(const volatile double* rec, int n_sens, double seq) {
  if (rec[kSeq] != seq) return false;
  const Fold f = fold_step(seq, n_sens, [rec](int q) { return (double)rec[kY + q]; }, rec[kE], rec[kR2], rec[kB2], rec[kFlag]);
  return f.x == bits(rec[kXor]) && f.w == bits(rec[kSum]);
}
inline bool late_record_ok(const volatile double* rec, double seq) {
  if (rec[kLateSeq] != seq) return false;
  const Fold f = fold_late(seq, rec[kLateE], rec[kLateR2], rec[kLateB2], rec[kLateGaveUp]);
  return f.x == bits(rec[kLateXor]) && f.w == bits(rec[kLateSum]);
}

}  // namespace fc_rec
