// qmpc_sense.h -- launch arguments of the sensor model (include/qmpc_sense.h), shared by qmpc_sense.hip (kernels) and
// qmpc_capi_stages.cpp (entry points).
#ifndef QMPC_SENSE_DEV_H
#define QMPC_SENSE_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>

// by value; the six parameter pointers are the caller's arrays as bound (null: that term is absent)
struct QmpcSenseArgs {
  const double* state;  // [B][16] the plant's last read-out (QmpcPlantDev::state)
  const double* motor;  // [B][24] (QmpcPlantDev::motor)
  int* n;               // [B] readings taken in this epoch
  int* epoch;           // [B] resets
  const double* acc_bias;    // [B][3]
  const double* gyro_bias;   // [B][3]
  const double* acc_sigma;   // [B]
  const double* gyro_sigma;  // [B]
  const double* q_sigma;     // [B]
  const double* qd_sigma;    // [B]
  uint32_t key0, key1;  // the seed's low and high word
};

// channel numbers of a robot (the third counter word of the generator)
enum { QMPC_SENSE_CH_ACC = 0, QMPC_SENSE_CH_GYRO = 3, QMPC_SENSE_CH_Q = 6, QMPC_SENSE_CH_QD = 18 };

// Launchers of qmpc_sense.hip, declared once for the file that defines them and for qmpc_capi_stages.cpp, which calls them: a
// signature that drifts fails to compile.
extern "C" hipError_t qmpc_launch_sense(const QmpcSenseArgs* A, double* imu_out, double* motor_out, int batch, int noisy,
                                        hipStream_t stream);
extern "C" hipError_t qmpc_launch_sense_reset(const QmpcSenseArgs* A, const uint8_t* mask, int batch,
                                              hipStream_t stream);

#endif
