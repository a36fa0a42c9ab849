/*
 * qmpc_terrain.h -- per-robot slopes and stairs under the reduced-order plant of qmpc_plant.h.  Same library, same
 * handle, same ABI version: nothing of qmpc_plant.h or qmpc_plant_vary.h changes, and a plant with no terrain bound
 * stands on flat ground at z = 0 and steps exactly as those headers describe, with the kernels it always launched.
 *
 * The reference's own simulation walks over four boxes of 0.2 m depth and 0.01 .. 0.04 m height; its controller climbs
 * them blind, because its Kalman filter measures the body's height against the stance feet.  Here every robot of a
 * fleet gets its own ground: an inclined plane plus a flight of stairs, analytic, with no height-field memory.  The
 * controller and the solve are not told.
 *
 * Terrain is read from a caller-owned DEVICE array terrain[B][8] (double) at every launch: the pointer is captured, the
 * values are not, so rows can be rewritten on the stream between steps or between replays of a captured graph, like
 * qmpc_plant_vary.h's force.  Row b = (z0, gx, gy, rise, run, count, s0, psi):
 *
 *     height(x, y) = ((z0 + gx x) + gy y) + rise k
 *     k = 0                                                                 when count <= 0 or not run > 0
 *     k = clamp(floor(((x cos psi + y sin psi) - s0) / run) + 1, 0, count)  otherwise
 *
 * i.e. a plane through (0, 0, z0) with slopes gx, gy, plus `count` treads of depth `run` and height `rise` (signed:
 * negative is downstairs) that start at abscissa s0 along heading psi.  Treads inherit the plane's slope.  The contact
 * normal is n = (-gx, -gy, 1) / sqrt((gx gx + gy gy) + 1) everywhere: a height field has no risers.
 *
 * The model (fp64, no contraction, one operation at a time; restated in tests/plant_model_terrain.py) changes the
 * numbered steps of qmpc_plant.h only while terrain is bound, for robot b:
 *   1.  Touch-down.  On a swing -> stance edge c_z = height(c_x, c_y) instead of 0.  Contact stays scheduled: the gait
 *       decides which feet stand, not the ground.
 *       support_b = mean c_z of the feet in stance after this step, ((s_0 + s_1) + (s_2 + s_3)) / their number with
 *       s_i = c_i,z of a stance foot and 0 of a swing foot; with no foot in stance it keeps its previous value (device
 *       state, set by reset).
 *   2a. Stance force: the cone is taken about n.  fn = (f_x n_x + f_y n_y) + f_z n_z; f = 0 unless fn > 0;
 *       t = f - fn n; if |t| = sqrt((t_x^2 + t_y^2) + t_z^2) > mu fn then f_k = fn n_k + t_k (mu fn / |t|), otherwise f
 *       is left untouched.  (mu is qmpc_plant_vary.h's mu_b where bound.)  n_x = -gx / norm, so a zero slope gives -0.0,
 *       the additive identity: an all-zero row reproduces the flat plant bit for bit.
 *   3.  Swing feet, only with QMPC_TERRAIN_CLAMP_SWING: after the foot is placed at the commanded position, if c_z <
 *       height(c_x, c_y) then c_z = height(c_x, c_y), and r = rBody (c - p) - hip for the read-out, so the encoders see
 *       the shortened leg; rdot stays v_des.  (The flat plant lets a swing foot dip below 0 -- the controller aims at
 *       -0.003 -- so without the flag zero terrain is bit-neutral.)
 *   4.  Read-out.  ground_b = height(p_x, p_y) at the new pose.  With QMPC_TERRAIN_REBASE_Z column 6 of the state row
 *       (the plant's own copy and the caller's) is p_z - support_b: the height above the stance feet, which is what the
 *       Kalman filter estimates, so that qmpc_ctrl_tick_state walks on terrain without its body target sinking into a
 *       hill.  The view's p stays world truth.
 *   Statistics (qmpc_plant_vary.h): z_min and z_max fold the state row's column 6, re-based when the flag is set.
 *   Reset (qmpc_plant_reset keeps the binding): the masked robots are placed on the terrain -- the body level at
 *       (x0, y0, 0.29 + height(x0, y0)), each foot at its usual body-frame xy with c_z = height(c_x, c_y), support the
 *       mean of the four feet, ground = height(x0, y0).  qmpc_plant_init unbinds: a new plant is the flat plant.  The
 *       flow is therefore init -> set_terrain -> reset(all).
 * A non-finite value, or run <= 0 with count > 0, affects that robot only.
 *
 * Still out of scope: risers and lateral collisions; pitch adaptation of the controller to a slope.  (Contact decided by
 * the ground -- early or late touch-down -- and slip are qmpc_contact.h, height maps from memory are qmpc_field.h, both
 * opt-in.)
 *
 * Errors as in qmpc_plant.h: QMPC_ERR_STATE before qmpc_plant_init; QMPC_ERR_ARG for a batch other than the plant's,
 * unknown flag bits or a null view.
 */
#ifndef QMPC_TERRAIN_H
#define QMPC_TERRAIN_H

#include "qmpc_plant.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { QMPC_TERRAIN_CLAMP_SWING = 1, QMPC_TERRAIN_REBASE_Z = 2 };

/* Bind terrain_dev[B][8] (device, double) and the flags, or unbind with NULL (host state only: nothing is enqueued,
 * nothing is copied).  Every later qmpc_plant_step and qmpc_plant_reset reads the rows at launch. */
int qmpc_plant_set_terrain(qmpc_handle h, int batch, const double* terrain_dev, int flags);

/* Device views, [B] each (allocated once for the handle's max_batch by qmpc_plant_init, valid until the handle is
 * destroyed; read-only by contract), the rows as bound (NULL: flat ground) and the flags. */
typedef struct {
  const double* ground;   /* [B] height(p_x, p_y) at the last pose written on terrain */
  const double* support;  /* [B] mean height of the stance feet */
  const double* terrain;  /* [B][8] the caller's rows, or NULL */
  int flags;
  int batch;
} qmpc_terrain_view;
int qmpc_terrain_view_get(qmpc_handle h, qmpc_terrain_view* v);

#ifdef __cplusplus
}
#endif
#endif /* QMPC_TERRAIN_H */
