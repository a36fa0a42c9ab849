// field_index_dump.cpp -- the index logic of include/qmpc_field.h on the CPU (tests/test_field_cpu.py builds this with
// AddressSanitizer and UBSan for the host and runs it; it is never loaded into python).  For every bank shape given on
// the command line as "nx ny count" triples it feeds quadruped_ctrl_amd/csrc/qmpc_field_index.h the hostile values below as u, v and
// map in every combination, READS the four taps from a heap array of exactly count * ny * nx floats -- so that a tap
// outside the bank is an AddressSanitizer report and a float-to-int conversion out of range an UBSan one -- and prints
//     nx ny count  u v map  m i j  a b  in_x in_y  t00 t10 t01 t11
// with the taps as offsets into the whole bank.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../quadruped_ctrl_amd/csrc/qmpc_field_index.h"

int main(int argc, char** argv) {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  double sum = 0.0;
  for (int arg = 1; arg + 2 < argc; arg += 3) {
    const int nx = std::atoi(argv[arg]), ny = std::atoi(argv[arg + 1]), count = std::atoi(argv[arg + 2]);
    const std::vector<double> hostile = {0.0, -0.0, 0.5, 1e9, -1e9, 1e300, -1e300, inf, -inf, nan, -nan, 5e-324, -5e-324,
                                         2147483647.0, 2147483648.0, -2147483649.0, 4294967296.0, 1.8446744073709552e19};
    // ... and for an axis of n: every exact grid line with its two neighbours, and 1e-9 inside / outside each edge
    auto axis = [&](int n) {
      std::vector<double> vals = hostile;
      for (int k = 0; k <= n; ++k) {
        const double g = (double)k;
        vals.push_back(g);
        vals.push_back(std::nextafter(g, -inf));
        vals.push_back(std::nextafter(g, inf));
      }
      for (const double e : {-1e-9, 1e-9, (double)(n - 1) - 1e-9, (double)(n - 1) + 1e-9, -1.0, (double)-n}) vals.push_back(e);
      return vals;
    };
    const std::vector<double> us = axis(nx), vs = axis(ny), maps = axis(count);
    const size_t total = (size_t)count * (size_t)ny * (size_t)nx;
    float* z = new float[total];  // exactly the bank: one element past it is a heap overflow
    for (size_t k = 0; k < total; ++k) z[k] = (float)k;
    for (const double u : us)
      for (const double v : vs)
        for (const double map : maps) {
          double a, b;
          bool in_x, in_y;
          const int m = qmpc_field_map(map, count);
          const int i = qmpc_field_axis(u, nx, &a, &in_x);
          const int j = qmpc_field_axis(v, ny, &b, &in_y);
          const size_t t00 = qmpc_field_base(m, nx, ny) + qmpc_field_tap(i, j, nx);
          const size_t t10 = t00 + 1, t01 = t00 + (size_t)nx, t11 = t00 + (size_t)nx + 1;
          sum += (double)z[t00] + (double)z[t10] + (double)z[t01] + (double)z[t11];
          std::printf("%d %d %d  %.17g %.17g %.17g  %d %d %d  %.17g %.17g  %d %d  %zu %zu %zu %zu\n", nx, ny, count, u, v, map,
                      m, i, j, a, b, (int)in_x, (int)in_y, t00, t10, t01, t11);
        }
    delete[] z;
  }
  std::fprintf(stderr, "checksum %.17g\n", sum);
  return 0;
}
