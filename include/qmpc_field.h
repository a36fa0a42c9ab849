/*
 * qmpc_field.h -- height-field terrain from memory under the reduced-order plant of qmpc_plant.h.  Same library, same
 * handle, same ABI version: nothing of qmpc_plant.h, qmpc_plant_vary.h, qmpc_terrain.h or qmpc_contact.h changes, and a
 * plant with no field bound steps exactly as those headers describe, with the kernels it always launched and the
 * arguments it always gave them.
 *
 * The reference's simulation offers rough ground: `random1`, 256 x 256 samples on 0.05 m cells where each 2 x 2 block
 * shares one height drawn from uniform(0, 0.06) m, and `random2`, a height map read from a file.  Here a plant gets a
 * BANK of such maps in device memory, and every robot of the fleet its own placement on one of them.  The field is
 * added to qmpc_terrain.h's analytic ground, so a robot can walk rough stairs; with no terrain rows bound the analytic
 * term is 0.  The controller and the solve are not told.
 *
 * The bank z[count][ny][nx] (float, x fastest) and the placements place[B][4] (double) are caller-owned DEVICE arrays
 * read at every launch: the pointers are captured, the values are not, so samples and rows can be rewritten on the
 * stream between steps or between replays of a captured graph, like qmpc_terrain.h's rows.  Row b = (map, ox, oy, zs):
 * robot b stands on map `map`, whose sample (0, 0) lies at world (ox, oy), scaled by zs.
 *
 * The field of robot b at world (x, y) (fp64, no contraction, one operation at a time; restated in
 * tests/plant_model_field.py; the index logic is quadruped_ctrl_amd/csrc/qmpc_field_index.h, which a CPU program can
 * compile).  Every clamp comes before its float-to-int conversion, so no index leaves the bank for any input bits:
 *     m    = map;  if !(m >= 0) then m = 0 (a NaN too);  if m > count - 1 then m = count - 1;  truncated to an integer
 *     u    = (x - ox) / cell
 *     in_x = (u >= 0) && (u <= nx - 1)
 *     if !(u >= 0) then u = 0 (a NaN lands on column 0);  if u > nx - 1 then u = nx - 1   (the edge sample extends outward)
 *     i    = floor(u);  if i > nx - 2 then i = nx - 2;   a = u - i
 *     v, in_y, j, b: the same from y, oy and ny
 *     z00 = z[m][j][i], z10 = z[m][j][i + 1], z01 = z[m][j + 1][i], z11 = z[m][j + 1][i + 1], widened to double
 *     d0 = z10 - z00;  d1 = z11 - z01;  e0 = z00 + a d0;  e1 = z01 + a d1;  e = e1 - e0
 *     f  = zs (e0 + b e)
 *     fx = zs ((d0 + b (d1 - d0)) / cell) where in_x, else 0
 *     fy = zs (e / cell)                  where in_y, else 0
 * f, fx and fy come from one set of four taps.  The surface and its slope are
 *     height(x, y) = qmpc_terrain.h's height(x, y)   when f == 0 (either sign), otherwise that + f
 *     g_x = gx when fx == 0 (either sign), otherwise gx + fx;   g_y likewise from gy and fy
 * (gx = gy = 0 and an analytic height of 0 with no rows bound).  The zero cases are what keeps a bank of all-zero samples
 * bit-neutral: h + 0.0 would turn a height of -0.0 into +0.0, and -0.0 + 0.0 a slope of -0.0 into +0.0, and the existing
 * plant relies on n_x = -gx / norm = -0.0 for a zero slope.
 *
 * The model changes the numbered steps of qmpc_terrain.h and qmpc_contact.h only while a field is bound, for robot b:
 *   height.  The field's height enters every place the two headers say height(...): qmpc_terrain.h's touch-down (1), swing
 *       clamp (3), ground_b (4) and the reset's placement of body and feet; qmpc_contact.h's edges (1), the height a
 *       sliding foot is re-projected to (2), the `touching` test and the pinning height (3), the swing clamp and ground_b.
 *   normal.  The contact normal is per FOOT: n = (-g_x, -g_y, 1) / sqrt((g_x g_x + g_y g_y) + 1) with g at the foot's
 *       pinned (c_x, c_y).  It is evaluated after step 1's edges (qmpc_terrain.h 1 / qmpc_contact.h 1), for every foot,
 *       from the same taps as the touch-down's height, and used by the cone of every substep (2a / 2).  With
 *       QMPC_CONTACT_SLIP it is evaluated again after each slide move, at the new (c_x, c_y), from the taps of the
 *       re-projection.  A foot pinned in step 3 gets its normal in the next step's step 1.
 *   flags.  A step uses the OR of the terrain binding's flags and the field binding's flags (QMPC_TERRAIN_*).
 *   Reset (qmpc_plant_reset keeps the binding): qmpc_terrain.h's reset on the summed surface.  qmpc_plant_init unbinds.
 *       The flow is init -> set_field (and set_terrain, set_contact) -> reset(all).
 * Bit neutrality: a bank of all-zero samples under flags 0, with finite placements, changes no bit of any output
 * relative to the same plant without the field -- on flat ground, on terrain rows and with contact on.
 * A non-finite value, or an out-of-range map, affects that robot only.
 *
 * Still out of scope: risers and lateral collisions; body-ground collision; telling the controller about the ground.
 *
 * Errors as in qmpc_plant.h: QMPC_ERR_STATE before qmpc_plant_init; QMPC_ERR_ARG for a batch other than the plant's,
 * nx < 2, ny < 2, count < 1, a cell that is not finite and > 0, a null z or place, unknown flag bits or a null view.
 */
#ifndef QMPC_FIELD_H
#define QMPC_FIELD_H

#include "qmpc_terrain.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  const float* z;  /* z[count][ny][nx], x fastest, DEVICE, caller-owned */
  int nx, ny, count;
  double cell;     /* metres between samples, both axes */
} qmpc_field_bank;

/* Bind the bank and place_dev[B][4] (device, double: map, ox, oy, zs) with QMPC_TERRAIN_* flags, or unbind with
 * bank == NULL (host state only: nothing is enqueued, nothing is copied).  Every later qmpc_plant_step and
 * qmpc_plant_reset reads the rows and the samples at launch. */
int qmpc_plant_set_field(qmpc_handle h, int batch, const qmpc_field_bank* bank, const double* place_dev, int flags);

/* The binding as set (bank.z == NULL: no field). */
typedef struct {
  qmpc_field_bank bank;
  const double* place;
  int flags;
  int batch;
} qmpc_field_view;
int qmpc_field_view_get(qmpc_handle h, qmpc_field_view* v);

#ifdef __cplusplus
}
#endif
#endif /* QMPC_FIELD_H */
