// Host-only replay of the LDS bank rules on the E tables' index formula (csrc/qmpc_etab.h), for tests/test_etab_layout_cpu.py.
//
// stdin: one case per line, 65 integers: the row u (0..11) each of the 64 lanes of a wave reads, then the wave-uniform column v.
// stdout: one JSON object with, per scheme, the WORST number of distinct addresses that meet on one bank inside one lane group
// (1 = no conflict; an N-way conflict costs the group N LDS cycles).
//
//   pairs_b128        the interleaved, padded layout read by one 16-byte load per lane: four groups of 16 lanes
//                     {0-3,12-15,20-27}, {4-11,16-19,28-31}, {32-35,44-47,52-59}, {36-43,48-51,60-63}, bank = (a / 4) mod 64
//   plain_read2_b64   the layout it replaced (two 12 x 12 tables of doubles, 144 apart) read by a two-address 8-byte load: two
//                     accesses, each four groups of 16 contiguous lanes, bank = (a / 4) mod 32
//   plain_read_b64    the same layout read by single 8-byte loads: two groups of 32 lanes, bank = (a / 4) mod 64
#include <cstdio>
#include <set>
#include <vector>

#include "qmpc_etab.h"

static_assert(qmpc_e_pair(QMPC_E_DIM - 1, QMPC_E_DIM - 1) < QMPC_E_PAIRS, "the last pair lies inside the storage");

// worst distinct-address count on a bank over the lane groups; `bytes` per lane at byte address addr[lane]
static int worst(const std::vector<std::vector<int>>& groups, const int* addr, int bytes, int banks) {
  int w = 0;
  for (const auto& g : groups) {
    std::vector<std::set<int>> on(banks);
    for (int lane : g)
      for (int b = 0; b < bytes; b += 4) on[((addr[lane] + b) / 4) % banks].insert(addr[lane]);
    for (const auto& s : on) w = (int)s.size() > w ? (int)s.size() : w;
  }
  return w;
}

static std::vector<int> run(int a, int b) {
  std::vector<int> r;
  for (int i = a; i <= b; ++i) r.push_back(i);
  return r;
}
static std::vector<int> cat(std::vector<int> a, const std::vector<int>& b, const std::vector<int>& c) {
  a.insert(a.end(), b.begin(), b.end());
  a.insert(a.end(), c.begin(), c.end());
  return a;
}

int main() {
  const std::vector<std::vector<int>> g128 = {cat(run(0, 3), run(12, 15), run(20, 27)), cat(run(4, 11), run(16, 19), run(28, 31)),
                                              cat(run(32, 35), run(44, 47), run(52, 59)), cat(run(36, 43), run(48, 51), run(60, 63))};
  const std::vector<std::vector<int>> g16 = {run(0, 15), run(16, 31), run(32, 47), run(48, 63)};
  const std::vector<std::vector<int>> g32 = {run(0, 31), run(32, 63)};
  int w_pairs = 0, w_read2 = 0, w_read = 0, cases = 0;
  for (;;) {
    int u[64], v;
    for (int l = 0; l < 64; ++l)
      if (std::scanf("%d", &u[l]) != 1) goto done;
    if (std::scanf("%d", &v) != 1) break;
    int ap[64], a0[64], a1[64];
    for (int l = 0; l < 64; ++l) {
      if (u[l] < 0 || u[l] >= QMPC_E_DIM || v < 0 || v >= QMPC_E_DIM) return 2;
      ap[l] = QMPC_E_PAIR_BYTES * qmpc_e_pair(u[l], v);
      a0[l] = 8 * qmpc_e_plain(u[l], v);
      a1[l] = 8 * (QMPC_E_DIM * QMPC_E_DIM + qmpc_e_plain(u[l], v));
    }
    auto up = [](int& w, int x) { w = x > w ? x : w; };
    up(w_pairs, worst(g128, ap, 16, 64));
    up(w_read2, worst(g16, a0, 8, 32));
    up(w_read2, worst(g16, a1, 8, 32));
    up(w_read, worst(g32, a0, 8, 64));
    up(w_read, worst(g32, a1, 8, 64));
    ++cases;
  }
done:
  std::printf("{\"cases\": %d, \"pairs_b128\": %d, \"plain_read2_b64\": %d, \"plain_read_b64\": %d}\n", cases, w_pairs, w_read2, w_read);
  return 0;
}
