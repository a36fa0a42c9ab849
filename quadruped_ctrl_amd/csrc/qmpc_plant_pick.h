// qmpc_plant_pick.h -- which kernel steps the plant and which one resets it, as a pure function of what is bound.  No
// HIP, no device: tests/plant_pick_dump.cpp includes this header alone and prints the choice for every combination.
//
// The two lists below are the only lists of the plant's step and reset kernels: qmpc_plant.h declares one launcher per
// entry, qmpc_capi_plant.cpp builds its launcher tables from them in the enums' order.  A new step kernel is one entry in
// QMPC_PLANT_STEP_KINDS, its launcher, and its line in qmpc_plant_pick.
#ifndef QMPC_PLANT_PICK_H
#define QMPC_PLANT_PICK_H

// X(ENUM suffix, launcher infix): qmpc_launch_<infix>_step
#define QMPC_PLANT_STEP_KINDS(X)                                                                  \
  X(PLANT, plant)                 /* qmpc_plant.hip: flat ground, scheduled contact */            \
  X(TERRAIN, terrain)             /* qmpc_terrain.hip: rows bound, scheduled contact */           \
  X(CONTACT, contact)             /* qmpc_contact.hip: contact decided by the ground, any rows */ \
  X(FIELD, field)                 /* qmpc_field.hip: a bank bound, scheduled contact */           \
  X(FIELD_CONTACT, field_contact) /* qmpc_field.hip: a bank bound, contact decided by the ground */
// ... qmpc_launch_<infix>_init
#define QMPC_PLANT_RESET_KINDS(X) \
  X(PLANT, plant)     /* flat */  \
  X(TERRAIN, terrain) /* rows */  \
  X(FIELD, field)     /* a bank, with or without rows */

#define QMPC_PLANT_PICK_ENUM(NAME, name) QMPC_STEP_##NAME,
enum QmpcPlantStepKind { QMPC_PLANT_STEP_KINDS(QMPC_PLANT_PICK_ENUM) QMPC_STEP_KINDS };
#undef QMPC_PLANT_PICK_ENUM
#define QMPC_PLANT_PICK_ENUM(NAME, name) QMPC_RESET_##NAME,
enum QmpcPlantResetKind { QMPC_PLANT_RESET_KINDS(QMPC_PLANT_PICK_ENUM) QMPC_RESET_KINDS };
#undef QMPC_PLANT_PICK_ENUM

struct QmpcPlantPick {
  QmpcPlantStepKind step;
  QmpcPlantResetKind reset;
  bool contact;  // the contact counters are in use: a reset zeroes the masked robots'
};

// field: a height-field bank is bound (include/qmpc_field.h); contact: the contact flags are not 0
// (include/qmpc_contact.h); rows: terrain rows are bound (include/qmpc_terrain.h).  A field takes its own kernels
// whatever else is bound; without one, contact decided by the ground takes qmpc_contact.hip's step on any rows; without
// either, rows decide between the terrain and the flat step.  The reset stands the robots on the ground and does not
// depend on who decides contact.
inline QmpcPlantPick qmpc_plant_pick(bool field, bool contact, bool rows) {
  QmpcPlantPick p;
  p.step = field ? (contact ? QMPC_STEP_FIELD_CONTACT : QMPC_STEP_FIELD)
                 : contact ? QMPC_STEP_CONTACT : rows ? QMPC_STEP_TERRAIN : QMPC_STEP_PLANT;
  p.reset = field ? QMPC_RESET_FIELD : rows ? QMPC_RESET_TERRAIN : QMPC_RESET_PLANT;
  p.contact = contact;
  return p;
}

#endif
