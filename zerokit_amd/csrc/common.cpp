#include "common.h"

#include <stdlib.h>

// The prover creates eight HIP streams (two graph interpreters, mat-vec/NTT, the two table walks, back end, proof values,
// wipes).  ROCclr multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues and streams that share a queue serialise,
// so a big batch keeps all eight busy only where the process has eight queues and four at four to seven (prover_plan.h:
// stream_plan).  The library reads that variable and leaves setting it to the host program and its environment: the
// hardware queues of a card are shared by every process on it.
namespace rlnamd {
void require_gpu() {
  static int checked = 0;
  if (checked == 1) return;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0)
    throw Error("no HIP device available: this library has no CPU fallback (MI355X / gfx950 required)");
  hipDeviceProp_t prop;
  RLN_HIP(hipGetDeviceProperties(&prop, 0));
  checked = 1;
}
}  // namespace rlnamd
