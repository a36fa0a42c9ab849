/*
 * qmpc_act.h -- actuators on the device between the controller's effort and the reduced-order plant of qmpc_plant.h: a
 * motor model, a command latency, and energy / saturation accumulators per robot.  Same library, same handle, same ABI
 * version: nothing of the other headers changes, and until qmpc_act_init nothing of this one is active.
 *
 * One qmpc_act per control period turns effort[B][12] as qmpc_ctrl_tick* wrote it into the torque the joints receive.
 * A run of
 *     qmpc_ctrl_tick_state -> qmpc_act -> qmpc_plant_step            (or qmpc_ctrl_tick ... qmpc_sense on the sensor path)
 * is a closed loop with no host in it.  qmpc_act allocates nothing and only enqueues one kernel, so the loop can be
 * captured into a graph (in lockstep a captured block holds a multiple of 13 ticks, see qmpc_ctrl.h); the ring and the
 * counters are device state and go on across replays.
 *
 * THE MODEL (fp64, no contraction, one operation at a time, nothing transcendental; restated in tests/act_model.py, which
 * agrees with the kernel bit for bit).  The motor is the reference's ActuatorModel<T>::getTorque
 * (src/Dynamics/ActuatorModel.h:54-71), which the reference ships and never calls; the defaults are the Mini Cheetah's
 * (src/Dynamics/MiniCheetah.h:28-46, assembled per joint type in Quadruped::buildActuatorModels).  For robot b and joint
 * k = 3 leg + j with g = gear[j], qd = the plant's own joint rate (qmpc_plant_view.motor, columns 12..23: the true rate,
 * not a sensed one), V_b, tmax_b, damp_b, dry_b the robot's bound values or else the config's:
 *     tau_cmd = ring[row][b][k]                      (LATENCY below)
 *     tm   = tau_cmd / g
 *     ides = tm / (kt * 1.5)
 *     bemf = ((qd * g) * kt) * 2.0
 *     vdes = ides * R + bemf
 *     vact = coerce(vdes, -V_b, V_b)                 (the reference's coerce: two compares; a NaN passes through)
 *     tam  = ((kt * 1.5) * (vact - bemf)) / R
 *     tc   = coerce(tam, -tmax_b, tmax_b)
 *     tau  = g * tc;   tau = strength_b * tau        (only when strength is bound)
 *     if friction:  tau = (tau - damp_b * qd) - dry_b * sgn(qd)       sgn(x) = (0 < x) - (x < 0): sgn(+-0) = sgn(NaN) = 0
 * effort_out[b][k] = tau.
 *
 * LATENCY.  ring[max_delay + 1][B][12] holds the last commands.  Per robot, head_b (the row this period's command goes
 * into: the robot's call count modulo max_delay + 1) and age_b (periods since qmpc_act_init or the robot's last
 * qmpc_act_reset, saturated at max_delay) are device state.  A call stores effort_in[b] in row head_b, then applies
 *     row = (head_b - min(clamp(delay_b, 0, max_delay), age_b)) mod (max_delay + 1),
 * then head_b and age_b advance by one.  So until delay_b periods have passed since init or reset the robot receives its
 * OLDEST stored command, not zeros: a robot that starts standing does not drop.  With max_delay = 0 the ring is one row
 * and the path is the motor alone.
 *
 * ACCUMULATORS per robot, updated in the same launch (these are THIS LIBRARY'S definitions, not the reference's, which
 * has none):
 *     n         calls
 *     n_vsat    joint-periods with vact != vdes        n_tsat    joint-periods with tc != tam
 *     tau_peak  the largest |tau| (a NaN never enters)
 *     e_heat   += dt * S,  S = sum_k ((1.5 * i_k) * i_k) * R  with  i_k = tc / (kt * 1.5)        (joules in the windings)
 *     e_mech   += dt * sum_k tau_k * qd_k                                                        (work on the joints)
 *     e_pos    += dt * sum_k max(tau_k * qd_k, 0)                                                (a NaN counts 0)
 * with dt = 1 / freq of qmpc_ctrl_init.  Every sum starts at 0.0 and runs k = 0 .. 11 left to right into a per-period
 * subtotal, which is then multiplied by dt and added: the order is part of the contract, because the comparison with
 * the model is bit for bit.  The sums run over ALL twelve joints, swing legs included -- whose torque the massless-leg
 * plant ignores (except on an early touch-down with qmpc_contact.h): the energies are what the motors would spend, not
 * what the plant's body receives.
 *
 * WHAT THE REFERENCE PIPELINE STANDS (CPU restatement with the reference's qpOASES: tests/act_loop.py, recorded in
 * tests/golden/act_closed_loop_cpu.json; the 16 commands of the closed-loop tests, 650 ticks at 500 Hz, every robot the
 * same actuator).  The Mini Cheetah's motor keeps 16 of 16 robots safe in both robot modes.
 *     motor-side torque cap (N m)   mode 0: 16 safe at 1.5 and 1.25, 14 at 1.0, 8 at 0.75     mode 1: 16 safe at 1.5, 1.25 and 1.0, 11 at 0.75
 *     latency (ticks)               mode 0: 16 safe at 8 and 12 (24 ms; roll up to 0.33 rad), 11 at 16     mode 1: 16 safe at 8 and 12, 13 at 16
 *     battery (V)                   mode 0: 16 safe at 4 and 2 (sagging to 0.18 m at 2), 8 at 1     mode 1: 16 safe at 4 and 2, 11 at 1
 * At the default motor no joint-period is at the voltage limit and at most 2 of 124800 are at the torque cap; at 4 V some
 * 9000 are at the voltage limit and the walk is unchanged.
 * The voltage limit bites so late because it acts mostly on fast swing joints, whose torque the plant ignores.
 *
 * Out of scope: leg mass and rotor inertia, per-joint (as opposed to per-robot) parameters, a thermal model.
 *
 * Errors as in qmpc_sense.h: QMPC_ERR_STATE before qmpc_plant_init, and before qmpc_act_init for every call but
 * qmpc_act_init and qmpc_act_config_default; QMPC_ERR_ARG for a null handle, a batch other than the plant's, a null
 * effort pointer, config or view, max_delay outside 0 .. 64, a kt, R or gear that is not positive, or an effort_out that
 * overlaps the plant's motor buffer (the kernel reads the rates there while it writes the output).  A later
 * qmpc_plant_init with the same batch keeps the actuators; with another batch they must be initialised again.
 */
#ifndef QMPC_ACT_H
#define QMPC_ACT_H

#include "qmpc_plant.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QMPC_ACT_MAX_DELAY 64

typedef struct {
  double gear[3];  /* abad, hip, knee */
  double kt;       /* motor torque constant, N m / A */
  double R;        /* winding resistance, ohm */
  double battery_v;
  double damping;      /* at the joint, N m s / rad */
  double dry_friction; /* at the joint, N m */
  double tau_max;      /* motor-side torque cap, N m */
  int friction;        /* ActuatorModel::_frictionEnabled */
  int max_delay;       /* 0 .. QMPC_ACT_MAX_DELAY ticks: the ring holds max_delay + 1 rows */
} qmpc_act_config;

/* MiniCheetah.h's values: gear 6 / 6 / 9.33, kt 0.05, R 0.173, 24 V, damping 0.01, dry friction 0.2, cap 3 N m;
 * friction 1, max_delay 0. */
int qmpc_act_config_default(qmpc_act_config* cfg);

/* After qmpc_plant_init.  cfg == NULL: the default.  Allocates for the handle's max_batch -- the ring, head, age and the
 * accumulators; once, and again only when a later call asks for a longer ring --, zeroes all of it on the stream, keeps
 * the config and unbinds the parameters. */
int qmpc_act_init(qmpc_handle h, int batch, const qmpc_act_config* cfg, void* stream);

/* Caller-owned DEVICE arrays, one element per robot.  A NULL member: the config's value; strength: the factor is
 * absent; delay: 0. */
typedef struct {
  const double* battery_v;
  const double* tau_max;
  const double* strength;
  const double* damping;
  const double* dry_friction;
  const int32_t* delay; /* ticks; clamped to 0 .. max_delay */
} qmpc_act_params;

/* Bind the arrays (host state only: nothing is enqueued, nothing is copied).  Every later qmpc_act reads them at
 * launch: the pointers are captured, the values are not (qmpc_plant_set_params' contract, including: a non-finite value
 * affects that robot only).  prm == NULL or six NULL members unbind. */
int qmpc_act_set_params(qmpc_handle h, int batch, const qmpc_act_params* prm);

/* For the robots where mask_a[b] | mask_b[b] (uint8, device; either may be NULL, both NULL: all robots) is non-zero:
 * age = 0, so the robot's next command is applied at once and its ring fills again; with stats != 0 also the
 * accumulators' initial values (all zero).  One small kernel. */
int qmpc_act_reset(qmpc_handle h, int batch, const uint8_t* mask_a, const uint8_t* mask_b, int stats, void* stream);

/* One control period: effort_in[B][12] -> effort_out[B][12] (device, double).  One kernel launch, nothing else.
 * effort_out == effort_in is allowed: every element is read before the same work item writes it. */
int qmpc_act(qmpc_handle h, int batch, const double* effort_in, double* effort_out, void* stream);

/* Device views of the state (valid until the handle is destroyed or a qmpc_act_init with a longer ring); read-only by
 * contract. */
typedef struct {
  const double* ring;     /* [max_delay + 1][B][12] */
  const int32_t* head;    /* [B] */
  const int32_t* age;     /* [B] */
  const int32_t* n;       /* [B] */
  const int64_t* n_vsat;  /* [B] */
  const int64_t* n_tsat;  /* [B] */
  const double* tau_peak; /* [B] */
  const double* e_heat;   /* [B] */
  const double* e_mech;   /* [B] */
  const double* e_pos;    /* [B] */
  qmpc_act_config config;
  double dt;
  int batch;
} qmpc_act_view;
int qmpc_act_view_get(qmpc_handle h, qmpc_act_view* v);

#ifdef __cplusplus
}
#endif
#endif /* QMPC_ACT_H */
