// Run-time value -> template argument, for the kernel launches of fc_hip.hip and fc_shifted_solver.hpp, and the ONE declaration of
// every list of template instances those launches choose from.  Host only, standard headers only.
//
//   pick(BatchWidths{}, KB, [&](auto K) { hipLaunchKernelGGL((fc_nd_fold_b<K>), ...); });
//   pick(SweepGeoms{}, lanes, sub, [&](auto L, auto SB) { ... fc_nd_sweep<L, SB> ... });
//   pick_bool(nt, [&](auto NT) { ... fc_nd_flat_block<U, NT> ... });
//
// The functor is a generic lambda: its arguments are std::integral_constant / std::bool_constant values, usable as template arguments,
// and it is instantiated for the listed entries only -- a kernel instance exists because its entry stands in a list below.  Every
// picker says whether an entry matched; what a miss means (refuse, or fall through to a last instance) is the caller's.
#pragma once

#include <type_traits>

namespace fc_dispatch {

template <int... V>
struct IntList {};
template <int A, int B>
struct Pair {};
template <class... P>
struct PairList {};

// f(std::integral_constant<int, V>{}) for the entry equal to v
template <int... V, class F>
bool pick(IntList<V...>, int v, F&& f) {
  return ((v == V ? (f(std::integral_constant<int, V>{}), true) : false) || ...);
}

// f(std::integral_constant<int, A>{}, std::integral_constant<int, B>{}) for the entry equal to (a, b)
template <int... A, int... B, class F>
bool pick(PairList<Pair<A, B>...>, int a, int b, F&& f) {
  return ((a == A && b == B ? (f(std::integral_constant<int, A>{}, std::integral_constant<int, B>{}), true) : false) || ...);
}

// f(std::true_type{}) or f(std::false_type{})
template <class F>
bool pick_bool(bool v, F&& f) {
  if (v)
    f(std::true_type{});
  else
    f(std::false_type{});
  return true;
}

// ── the instance lists ──────────────────────────────────────────────────────────────────────────────────────────────────────────
// padded batch widths KB (fc_batch.hip.h, the block kernels of fc_shifted.hip.h)
using BatchWidths = IntList<4, 8, 16, 32>;
// fc_nd_sweep, fp64 factors: (LANES, SUB)
using SweepGeoms = PairList<Pair<8, 4>, Pair<8, 8>, Pair<16, 4>, Pair<16, 8>, Pair<16, 16>, Pair<32, 4>, Pair<32, 8>, Pair<32, 16>, Pair<32, 32>,
                            Pair<64, 4>, Pair<64, 8>, Pair<64, 16>, Pair<64, 32>, Pair<64, 64>, Pair<256, 16>, Pair<256, 32>, Pair<256, 64>,
                            Pair<256, 256>>;
// fc_nd_down_block, down-sweep: (LPR, RPS)
using BlockDownGeoms = PairList<Pair<16, 1>, Pair<16, 2>, Pair<32, 1>, Pair<32, 2>, Pair<32, 4>, Pair<64, 1>, Pair<64, 2>, Pair<64, 4>, Pair<64, 8>>;
// fc_nd_down_block, column form of the up-sweep: the small nodes near the leaves add (8, 1), (8, 2), (16, 4)
using BlockUpColumnGeoms = PairList<Pair<8, 1>, Pair<8, 2>, Pair<16, 4>, Pair<16, 1>, Pair<16, 2>, Pair<32, 1>, Pair<32, 2>, Pair<32, 4>, Pair<64, 1>,
                                    Pair<64, 2>, Pair<64, 4>, Pair<64, 8>>;
// fc_nd_flat_block: loads per thread
using FlatLoads = IntList<4, 8, 12, 16>;
// compressed factors (fp32 / bf16 values): the reduced geometries of pick_sweep
using SweepGeomsCompressed = PairList<Pair<16, 4>, Pair<64, 16>, Pair<256, 64>>;
using BlockGeomsCompressed = PairList<Pair<16, 2>, Pair<32, 4>, Pair<64, 8>>;
// lanes per row of the CSR products; the last entry is the one any other lane count falls through to
using SpmvLanes = IntList<4, 8, 16, 32, 64>;  // fc_spmv_csr
using PcLanes = IntList<1, 4, 8, 16, 32>;     // fc_pc_csr
using ShiftedSpmvLanes = IntList<8, 16, 32>;  // fc_shifted_spmv

}  // namespace fc_dispatch
