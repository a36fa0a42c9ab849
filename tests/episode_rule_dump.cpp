// episode_rule_dump.cpp -- the decision and the draw of include/qmpc_episode.h on the CPU (tests/test_episode_cpu.py
// builds this with AddressSanitizer and UBSan for the host and runs it; it is never loaded into python).  It feeds
// quadruped_ctrl_amd/csrc/qmpc_episode_rule.h
//   C lines: a pose near every threshold -- each threshold at its boundary and one ulp either side --, NaN and +-inf in
//     every field of p, q and of each threshold, the age at max_ticks - 1, max_ticks, max_ticks + 1 and at the end of
//     int, elapsed 1 and 13, under every single cause, all of them and none, and prints
//       C  causes max_ticks cos_tilt_min z_min range  safe  p0 p1 p2  q0 q1 q2 q3  ground  s0 s1  age_in elapsed
//          -> age cause dx dy height tilt
//   G lines: the gait column of a command row, hostile values included:  G value -> gait number
//   D lines: draws for n_spawn in {1, 7}, n_commands in {0, 1, 5}, robots up to 2^20 and episode indices 0, 1, 2^31 - 1
//     (and 4096 consecutive pairs for the coverage test), READS the drawn rows from heap arrays of exactly the tables'
//     sizes -- a row outside its table is an AddressSanitizer report -- and prints
//       D  key0 key1 b episode n_spawn n_commands -> spawn_row command_row offset_shared offset_per_robot
#include <climits>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../quadruped_ctrl_amd/csrc/qmpc_episode_rule.h"

namespace {

const double inf = std::numeric_limits<double>::infinity(), nan_ = std::numeric_limits<double>::quiet_NaN();

struct Case {
  qmpc_episode_rule R;
  int safe;
  double p[3], q[4], ground, start[2];
  int age, elapsed;
};

void run(const Case& c) {
  QmpcEpisodeFacts F;
  const int age = qmpc_episode_age(c.age, c.elapsed);
  const int cause = qmpc_episode_cause(c.R, c.safe, c.p, c.q, c.ground, c.start, age, &F);
  std::printf("C %d %d %.17g %.17g %.17g  %d  %.17g %.17g %.17g  %.17g %.17g %.17g %.17g  %.17g  %.17g %.17g  %d %d  %d %d "
              "%.17g %.17g %.17g %.17g\n",
              c.R.causes, c.R.max_ticks, c.R.cos_tilt_min, c.R.z_min, c.R.range, c.safe, c.p[0], c.p[1], c.p[2], c.q[0],
              c.q[1], c.q[2], c.q[3], c.ground, c.start[0], c.start[1], c.age, c.elapsed, age, cause, F.dx, F.dy, F.height,
              F.tilt);
}

// the case under every cause set and both values of elapsed, with the age landing on `land` after the increment
void sweep(Case c, int land) {
  const int sets[] = {63, 0, 1, 2, 4, 8, 16, 32, 1 | 32, 2 | 4 | 8};
  for (const int s : sets)
    for (const int elapsed : {1, 13})
      for (const int safe : {1, 0}) {
        c.R.causes = s;
        c.elapsed = elapsed;
        c.age = land - elapsed;
        c.safe = safe;
        run(c);
      }
}

}  // namespace

int main() {
  Case base{};
  base.R = qmpc_episode_rule{63, 40, 0.8, 0.18, 0.5};
  base.safe = 1;
  const double p[3] = {0.37, -0.21, 0.26}, q[4] = {0.94, 0.17, -0.23, 0.11}, start[2] = {0.1, 0.05};
  for (int k = 0; k < 3; ++k) base.p[k] = p[k];
  for (int k = 0; k < 4; ++k) base.q[k] = q[k];
  base.ground = 0.03;
  for (int k = 0; k < 2; ++k) base.start[k] = start[k];
  // the facts of the base pose, for the thresholds' boundaries
  QmpcEpisodeFacts F;
  qmpc_episode_cause(base.R, 1, base.p, base.q, base.ground, base.start, 0, &F);
  const std::vector<double> hostile = {nan_, -nan_, inf, -inf};
  const auto around = [](double x) { return std::vector<double>{x, std::nextafter(x, -inf), std::nextafter(x, inf)}; };
  // every threshold at its boundary and one ulp either side, and hostile
  for (const int land : {39, 40, 41}) {
    sweep(base, land);
    for (double v : around(F.tilt)) { Case c = base; c.R.cos_tilt_min = v; sweep(c, land); }
    for (double v : around(F.height)) { Case c = base; c.R.z_min = v; sweep(c, land); }
    for (double v : around(std::fabs(F.dx))) { Case c = base; c.R.range = v; sweep(c, land); }
    for (double v : around(std::fabs(F.dy))) { Case c = base; c.R.range = v; c.p[0] = c.start[0]; sweep(c, land); }
    for (double v : hostile) {
      { Case c = base; c.R.cos_tilt_min = v; sweep(c, land); }
      { Case c = base; c.R.z_min = v; sweep(c, land); }
      { Case c = base; c.R.range = v; sweep(c, land); }
      for (int k = 0; k < 3; ++k) { Case c = base; c.p[k] = v; sweep(c, land); }
      for (int k = 0; k < 4; ++k) { Case c = base; c.q[k] = v; sweep(c, land); }
      { Case c = base; c.ground = v; sweep(c, land); }
      for (int k = 0; k < 2; ++k) { Case c = base; c.start[k] = v; sweep(c, land); }
    }
  }
  // a robot on the other side of its start (the range is on |dx|, |dy|), and the end of int
  { Case c = base; c.p[0] = -0.9; c.p[1] = 0.05; sweep(c, 10); }
  { Case c = base; c.p[1] = 2.0; sweep(c, 10); }
  for (const int elapsed : {1, 13})
    for (const int age : {INT_MAX, INT_MAX - 1, INT_MAX - 13, INT_MAX - 14, 0}) {
      Case c = base;
      c.age = age;
      c.elapsed = elapsed;
      c.R.max_ticks = INT_MAX;
      run(c);
    }
  { Case c = base; c.R.max_ticks = 0; c.age = 0; c.elapsed = 1; run(c); c.R.max_ticks = -5; run(c); c.R.max_ticks = INT_MIN; run(c); }

  // ---- the gait column: G value -> gait number
  for (const double g : {0.0, -0.0, 0.5, 0.999, 1.0, 4.0, 11.9, 30.0, 31.0, 31.5, 32.0, -1.0, -1e-300, 1e9, -1e9, 2147483647.0,
                         2147483648.0, -2147483649.0, 1e300, -1e300, inf, -inf, nan_, -nan_})
    std::printf("G %.17g %d\n", g, (int)qmpc_episode_gait(g));

  // ---- draws
  double sum = 0.0;
  const int n_per = 4096;  // robots that own rows of the per-robot table (those beyond read the shared one only)
  for (const int S : {1, 7})
    for (const int Cn : {0, 1, 5}) {
      const size_t ns = (size_t)S * 3, nc = (size_t)(Cn > 0 ? Cn : 1) * 4;
      double* shared = new double[ns];  // exactly the tables: one element past them is a heap overflow
      double* per = new double[(size_t)n_per * ns];
      double* cmd = new double[nc];
      for (size_t k = 0; k < ns; ++k) shared[k] = (double)k;
      for (size_t k = 0; k < (size_t)n_per * ns; ++k) per[k] = (double)k;
      for (size_t k = 0; k < nc; ++k) cmd[k] = (double)k;
      const auto draw = [&](uint32_t k0, uint32_t k1, int b, int e) {
        int sr, cr;
        qmpc_episode_draw(k0, k1, b, e, S, Cn, &sr, &cr);
        const size_t o0 = qmpc_episode_spawn_at(b, sr, S, 0), o1 = qmpc_episode_spawn_at(b, sr, S, QMPC_EP_SPAWN_PER_ROBOT);
        sum += shared[o0] + shared[o0 + 1] + shared[o0 + 2];
        if (b < n_per) sum += per[o1] + per[o1 + 1] + per[o1 + 2];
        for (int k = 0; k < 4; ++k) sum += cmd[(size_t)cr * 4 + k];
        std::printf("D %u %u %d %d %d %d  %d %d %zu %zu\n", k0, k1, b, e, S, Cn, sr, cr, o0, o1);
      };
      const uint32_t keys[][2] = {{0u, 0u}, {0xFFFFFFFFu, 0xFFFFFFFFu}, {0x243F6A88u, 0x85A308D3u}};
      for (const auto& key : keys)
        for (const int b : {0, 1, 63, 64, 95, 4095, 4096, 65535, 1 << 20})
          for (const int e : {0, 1, 2, INT_MAX}) draw(key[0], key[1], b, e);
      // 4096 consecutive (b, episode) pairs: 64 robots x 64 episodes (the coverage test reads S = 7, C = 5)
      for (int b = 0; b < 64; ++b)
        for (int e = 1; e <= 64; ++e) draw(0x243F6A88u, 0x85A308D3u, b, e);
      delete[] shared;
      delete[] per;
      delete[] cmd;
    }
  std::fprintf(stderr, "checksum %.17g\n", sum);
  return 0;
}
