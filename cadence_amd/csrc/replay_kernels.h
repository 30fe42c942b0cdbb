// replay_kernels.h -- the kernels replay_kernel.hip defines and capi.hip launches, declared once: a definition
// that drifts from its declaration fails to compile instead of failing to link.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cadence_replay.h"

namespace crr {
template <bool WAVE_TAIL, bool EMIT>
__global__ void replay_lds_kernel(crr_inputs in, crr_outputs out, int phase, uint32_t lo, uint32_t hi);
template <bool WAVE_TAIL, bool EMIT, bool LANES = false>
__global__ void replay_lds_small_kernel(crr_inputs in, crr_outputs out, int phase, uint32_t lo, uint32_t hi);
__global__ void replay_wide_kernel(crr_inputs in, crr_outputs out, int phase, uint32_t lo, uint32_t hi);
template <bool EMIT, bool RESUME>
__global__ void replay_compact1_kernel(crr_inputs in, crr_outputs out, int phase, uint32_t lo, uint32_t hi);
template <bool EMIT, bool RESUME>
__global__ void replay_compact2_kernel(crr_inputs in, crr_outputs out, int phase, uint32_t lo, uint32_t hi);
template <bool EMIT, bool RESUME>
__global__ void replay_compact3_kernel(crr_inputs in, crr_outputs out, int phase, uint32_t lo, uint32_t hi);
__global__ void replay_big_kernel(crr_inputs in, crr_outputs out, int phase, uint32_t lo, uint32_t hi);
template <bool EMIT, bool RESUME>
__global__ void replay_tail_kernel(crr_inputs in, crr_outputs out, int phase, uint32_t lo, uint32_t hi);
__global__ void replay_global_kernel(crr_inputs in, crr_outputs out, int phase, int retry_only);
__global__ void tail_gate_kernel(const uint32_t* scratch, uint32_t need);
__global__ void replay_retry_kernel(crr_inputs in, crr_outputs out, int phase);
__global__ void checksum_kernel(crr_inputs in, crr_outputs out, uint32_t* checksums);
__global__ void token_crc_kernel(crr_inputs in, uint32_t* out);
}  // namespace crr
