// The kernels of the plan record as a translation unit of their own: plan_record_kernel and
// plan_prediction_score_kernel get a code object of their own, loaded when one of them is first launched, and the library's other
// code objects are what they were before these kernels existed.  jsim_mpc.hip declares the two and launches them.  The checkpoint
// kernels (checkpoint.inc) live here for the same reason.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "jsim_mpc.h"

#include "recorder_walk.inc" // RecorderBuf, the walk, jct_state_at
#include "pymod.inc"         // jpl_pymod

#define JSIM_PLAN_TU 1
#include "plan_predictions.inc"
#include "checkpoint.inc"    // the checkpoint kernels: beside the plan record's, for the same reason
