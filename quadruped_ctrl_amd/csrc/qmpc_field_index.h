// qmpc_field_index.h -- the index logic of include/qmpc_field.h in plain C++, __host__ and __device__: the kernels of
// qmpc_field.hip sample the bank through it, and a CPU program (tests/field_index_dump.cpp) compiles it under the
// sanitizers.  Every clamp comes before its float-to-int conversion, so no index leaves the bank for any input bits:
//   0 <= m <= count - 1,   0 <= i <= nx - 2,   0 <= j <= ny - 2   (nx, ny >= 2 and count >= 1 by qmpc_plant_set_field),
// and the four taps m ny nx + (j, j + 1) nx + (i, i + 1) lie inside [0, count ny nx).
#ifndef QMPC_FIELD_INDEX_H
#define QMPC_FIELD_INDEX_H

#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define QMPC_FIELD_HD __host__ __device__ __forceinline__
#else
#define QMPC_FIELD_HD inline
#endif

// map -> m: clamped to [0, count - 1] (a NaN to 0), then truncated
QMPC_FIELD_HD int qmpc_field_map(double map, int count) {
  const double top = (double)(count - 1);
  if (!(map >= 0.0)) map = 0.0;
  if (map > top) map = top;
  return (int)map;
}

// One axis: u = (x - o) / cell in cells -> the cell i in [0, n - 2], the weight a = u - i in [0, 1], and whether u lies
// on the map (the gradient along this axis is 0 where it does not).  Returns i.
QMPC_FIELD_HD int qmpc_field_axis(double u, int n, double* a, bool* in) {
  const double top = (double)(n - 1);
  *in = (u >= 0.0) && (u <= top);
  if (!(u >= 0.0)) u = 0.0;
  if (u > top) u = top;
  double fi = floor(u);
  if (fi > (double)(n - 2)) fi = (double)(n - 2);
  *a = u - fi;
  return (int)fi;
}

// The offset of tap z00 inside map m's ny x nx samples; z10 is + 1, z01 is + nx, z11 is + nx + 1
QMPC_FIELD_HD size_t qmpc_field_tap(int i, int j, int nx) { return (size_t)j * (size_t)nx + (size_t)i; }
// The offset of map m inside the bank
QMPC_FIELD_HD size_t qmpc_field_base(int m, int nx, int ny) { return (size_t)m * ((size_t)ny * (size_t)nx); }

#endif
