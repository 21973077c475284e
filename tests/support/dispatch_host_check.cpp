// CPU check of the launch dispatcher (flowcontrol_amd/csrc/fc_dispatch.hpp): every instance list is printed ("list NAME entries") and
// driven through its picker ("NAME passed tried" per property).  tests/test_dispatch_host.py asserts on both.
#include <algorithm>
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "../../flowcontrol_amd/csrc/fc_dispatch.hpp"

using namespace fc_dispatch;

template <int... V>
static std::vector<int> entries(IntList<V...>) {
  return {V...};
}
template <int... A, int... B>
static std::vector<std::pair<int, int>> entries(PairList<Pair<A, B>...>) {
  return {{A, B}...};
}

struct Tally {
  int passed = 0, tried = 0;
  void operator()(bool ok) { passed += ok ? 1 : 0, ++tried; }
};
static void report(const char* list, const char* what, const Tally& t) { std::printf("%s %s %d %d\n", list, what, t.passed, t.tried); }

template <class List>
static void check_values(const char* name, List list) {
  const std::vector<int> vs = entries(list);
  std::printf("list %s", name);
  for (int v : vs) std::printf(" %d", v);
  std::printf("\n");
  Tally hit, miss;
  for (int v : vs) {
    int calls = 0, got = -1;
    const bool found = pick(list, v, [&](auto K) {
      constexpr int k = K;  // (a compile-time constant: usable as a template argument)
      static_assert(k == decltype(K)::value, "");
      ++calls, got = k;
    });
    hit(found && calls == 1 && got == v);
  }
  // one below, one above and half-way between the entries
  std::set<int> others;
  for (size_t i = 0; i < vs.size(); ++i) {
    others.insert(vs[i] - 1), others.insert(vs[i] + 1);
    for (size_t j = 0; j < i; ++j) others.insert((vs[i] + vs[j]) / 2);
  }
  for (int v : others) {
    if (std::find(vs.begin(), vs.end(), v) != vs.end()) continue;
    int calls = 0;
    const bool found = pick(list, v, [&](auto) { ++calls; });
    miss(!found && calls == 0);
  }
  report(name, "hit", hit), report(name, "miss", miss);
}

template <class List>
static void check_pairs(const char* name, List list) {
  const std::vector<std::pair<int, int>> ps = entries(list);
  std::printf("list %s", name);
  for (auto p : ps) std::printf(" %d:%d", p.first, p.second);
  std::printf("\n");
  auto listed = [&](int a, int b) { return std::find(ps.begin(), ps.end(), std::make_pair(a, b)) != ps.end(); };
  auto misses = [&](int a, int b) {
    int calls = 0;
    const bool found = pick(list, a, b, [&](auto, auto) { ++calls; });
    return !found && calls == 0;
  };
  Tally hit, transposed, miss;
  std::set<int> firsts, seconds;
  for (auto p : ps) {
    int calls = 0, ga = -1, gb = -1;
    const bool found = pick(list, p.first, p.second, [&](auto A, auto B) {
      constexpr int a = A, b = B;
      static_assert(a == decltype(A)::value && b == decltype(B)::value, "");
      ++calls, ga = a, gb = b;
    });
    hit(found && calls == 1 && ga == p.first && gb == p.second);
    if (!listed(p.second, p.first)) transposed(misses(p.second, p.first));
    firsts.insert({p.first - 1, p.first, p.first + 1}), seconds.insert({p.second - 1, p.second, p.second + 1});
  }
  // every combination of the entries' members and their neighbours that is not itself an entry
  for (int a : firsts)
    for (int b : seconds)
      if (!listed(a, b)) miss(misses(a, b));
  report(name, "hit", hit), report(name, "transposed", transposed), report(name, "miss", miss);
}

int main() {
  check_values("BatchWidths", BatchWidths{});
  check_pairs("SweepGeoms", SweepGeoms{});
  check_pairs("BlockDownGeoms", BlockDownGeoms{});
  check_pairs("BlockUpColumnGeoms", BlockUpColumnGeoms{});
  check_values("FlatLoads", FlatLoads{});
  check_pairs("SweepGeomsCompressed", SweepGeomsCompressed{});
  check_pairs("BlockGeomsCompressed", BlockGeomsCompressed{});
  check_values("SpmvLanes", SpmvLanes{});
  check_values("PcLanes", PcLanes{});
  check_values("ShiftedSpmvLanes", ShiftedSpmvLanes{});
  // an empty list matches nothing
  Tally empty;
  empty(!pick(IntList<>{}, 4, [](auto) {}) && !pick(PairList<>{}, 4, 4, [](auto, auto) {}));
  report("Empty", "miss", empty);
  // the bool picker delivers both constants
  Tally both;
  for (bool v : {false, true}) {
    int calls = 0;
    bool got = !v;
    const bool found = pick_bool(v, [&](auto B) {
      constexpr bool b = B;
      static_assert(b == decltype(B)::value, "");
      ++calls, got = b;
    });
    both(found && calls == 1 && got == v);
  }
  report("Bool", "hit", both);
  return 0;
}
