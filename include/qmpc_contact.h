/*
 * qmpc_contact.h -- contact decided by the ground under the reduced-order plant of qmpc_plant.h: early and late
 * touch-down, and feet that slip.  Same library, same handle, same ABI version: nothing of qmpc_plant.h,
 * qmpc_plant_vary.h or qmpc_terrain.h changes, and a plant whose contact flags are 0 steps exactly as those headers
 * describe, with the kernels it always launched and the arguments it always gave them.
 *
 * In those headers contact is scheduled: a foot the gait says stands is put on the surface, a foot the gait says swings
 * passes through a tread, and a force outside the friction cone is cut back while the foot stays put.  A controller
 * cannot fall over its own feet on such a plant, and the swing-leg torques it computes are never exercised.  Here, per
 * plant and opt-in, the ground decides.  The controller and the solve are not told.
 *
 * Notation.  s_i: the gait's schedule of foot i (contact_state > 0).  pi_i: the plant's pinned flag, device state -- the
 * plant view's `stance`, which with contact on is the physical flag and no longer the schedule.  height(x, y) and n are
 * qmpc_terrain.h's; with no terrain bound the ground is height = 0 with n = (0, 0, 1) (an all-zero row, flags 0).
 * dt = 1 / freq, h = dt / substeps.  Fp64, no contraction, one operation at a time; restated in
 * tests/plant_model_contact.py.  A flag that is off leaves today's rule for its case in force.
 *
 *   1.  Edges, before the substeps.
 *       s = 1, pi = 0: without QMPC_CONTACT_LATE, or when c_z <= height(c_x, c_y): c_z = height(c_x, c_y), pi = 1.
 *                      Otherwise the foot stays unpinned (it is late) and carries no load.
 *       s = 0, pi = 1: without QMPC_CONTACT_EARLY pi = 0; with it the foot stays pinned until step 3 releases it.
 *       support_b = mean c_z of the feet with pi = 1 after this step, ((z_0 + z_1) + (z_2 + z_3)) / their number with
 *       z_i = 0 for an unpinned foot; with none it keeps its previous value.
 *   2.  Substeps.  A foot with pi = 1 pushes with J^-T tau of its own three torques whatever the schedule says, so a
 *       stubbed swing foot loads the body with the swing leg's PD torque.  The force is unilateral and the cone is taken
 *       about n, as in qmpc_terrain.h 2a: fn, t = f - fn n, |t|, cap = mu fn (mu is qmpc_plant_vary.h's mu_b where
 *       bound).  With QMPC_CONTACT_SLIP, when |t| > cap (and fn > 0) the force is cut back as always and the foot slides
 *       against the friction it receives:
 *           sv = slip_gain (|t| - cap);  if sv > slip_vmax then sv = slip_vmax;   cdot_k = -(sv (t_k / |t|))
 *           after p += h v of the same substep:  c_x += h cdot_x,  c_y += h cdot_y,  c_z = height(c_x, c_y)
 *           slip_b += (d_0 + d_1) + (d_2 + d_3),  d_i = h sv of a sliding foot and 0 of any other
 *       A foot that is not saturated does not move, and cdot = 0 for it.
 *   3.  Unpinned feet and release, at the new pose; R = R(q), rBody = R^T.
 *       A foot with s = 1 and pi = 1 keeps its place.  For every other foot the command is evaluated:
 *           late foot (s = 1, pi = 0; it exists only with QMPC_CONTACT_LATE): drop_i += drop_speed dt and
 *                      r = clamp(p_des_i - drop_i (rBody e_z)), the leg extends along the world's vertical;
 *           swing foot (s = 0): r = clamp(p_des_i); (clamp: the radial reach clamp of qmpc_plant.h)
 *           c* = p + R (hip_i + r);  touching = c*_z <= height(c*_x, c*_y).
 *       A late foot, and with QMPC_CONTACT_EARLY a swing foot, that is touching: if pi = 0 it is pinned at
 *       (c*_x, c*_y, height(c*_x, c*_y)), pi = 1; if pi = 1 it stays where it is.  Otherwise c = c*, pi = 0 (and without
 *       QMPC_CONTACT_EARLY qmpc_terrain.h's QMPC_TERRAIN_CLAMP_SWING acts on c as it always did).
 *       early_b counts every foot-tick that ends with s = 0, pi = 1; late_b every foot-tick spent in the late branch.
 *       drop_i = 0 whenever the foot ends the tick pinned or is scheduled to swing.  In stance the controller's p_des is
 *       its last swing target (ConvexMPCLocomotion.cpp:439-448), so a late foot's command is defined.
 *   4.  Read-out.  Pinned foot: r = rBody (c - p) - hip, rdot = (-(rBody v) - omega x (rBody (c - p))) + rBody cdot with
 *       the cdot of the last substep.  Unpinned foot: r of step 3 (after the terrain's swing clamp where it acted),
 *       rdot = v_des.  grf is the last substep's.  QMPC_TERRAIN_REBASE_Z and the statistics use the support of step 1;
 *       ground_b = height(p_x, p_y).
 *   qmpc_plant_init switches contact off, as it unbinds terrain.  qmpc_plant_reset keeps it on; while it is on it zeroes
 *   early, late, slip and drop of the masked robots (and support and ground when no terrain is bound).
 * A non-finite value affects its own robot only.
 *
 * The parameters are modelling choices the caller may change, not measurements.  The defaults of the Python binding:
 *   drop_speed 1 m/s: the mean speed at which a stance force of about 45 N extends a leg of about 1 kg over a 0.04 m
 *                     step;  slip_gain 0.01 m/s per newton of excess tangential demand;  slip_vmax 1 m/s.
 *
 * Still out of scope: risers and lateral collisions; leg inertia; contact sensing in the sensor model; telling the
 * controller about contact.
 *
 * Errors as in qmpc_plant.h: QMPC_ERR_STATE before qmpc_plant_init; QMPC_ERR_ARG for a batch other than the plant's,
 * unknown flag bits, a drop_speed, slip_gain or slip_vmax that is not finite and >= 0, or a null view.
 */
#ifndef QMPC_CONTACT_H
#define QMPC_CONTACT_H

#include "qmpc_terrain.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { QMPC_CONTACT_EARLY = 1, QMPC_CONTACT_LATE = 2, QMPC_CONTACT_SLIP = 4 };

typedef struct {
  int flags;          /* QMPC_CONTACT_* */
  double drop_speed;  /* m/s: how fast a late foot is lowered */
  double slip_gain;   /* m/s per newton beyond the cone */
  double slip_vmax;   /* m/s: the sliding speed's cap */
} qmpc_contact_params;

/* Host state only: nothing is enqueued, the scalars travel as kernel arguments of every later qmpc_plant_step.
 * prm == NULL or flags == 0: off. */
int qmpc_plant_set_contact(qmpc_handle h, int batch, const qmpc_contact_params* prm);

/* Device views (allocated once for the handle's max_batch by qmpc_plant_init, valid until the handle is destroyed;
 * read-only by contract) and the parameters as set. */
typedef struct {
  const int32_t* early;  /* [B]    foot-ticks spent pinned while the gait scheduled swing */
  const int32_t* late;   /* [B]    foot-ticks spent unpinned while the gait scheduled stance */
  const double* slip;    /* [B]    metres slid, summed over the four feet */
  const double* drop;    /* [B][4] how far each late foot has been lowered below its command */
  qmpc_contact_params params;
  int batch;
} qmpc_contact_view;
int qmpc_contact_view_get(qmpc_handle h, qmpc_contact_view* v);

#ifdef __cplusplus
}
#endif
#endif /* QMPC_CONTACT_H */
