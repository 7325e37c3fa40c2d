// Time maps (include/rocoder_hip.h: rc_engine_set_time_map): the gather stage in front of the hops. It belongs
// to no kernel family: no hop kernel reads a table of positions, they run unchanged at a step of N on the rows this stage
// writes, and neither this header nor rc_timemap.hip enters rc_kernel_id().
#ifndef RC_TIMEMAP_H
#define RC_TIMEMAP_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rc {

constexpr uint32_t TM_MAX_N = 1u << 22;          // the engine's longest window
constexpr int64_t TM_MAX_POS = (int64_t)1 << 48;  // |hop_pos[k]| above this is refused by the setter (and never reaches here)

// Hop k in [hop_first, hop_first + hop_count) of channel c in [0, channels) goes to v + c * v_stride + (k - hop_first) * N:
//   v[...][n] = x[c * in_stride + hop_pos[k] + n]  where 0 <= hop_pos[k] + n < in_len,  +0.0f elsewhere,   0 <= n < N.
// hop_pos is the DEVICE table of the whole map (entry k at hop_pos[k]). x may be null with in_len == 0. x needs float
// alignment only and any stride >= in_len; no address outside [x + c * in_stride, + in_len) is formed. The 16-byte stores
// run where v is 16-byte aligned, v_stride a multiple of 4 and N a multiple of 4; otherwise a float-per-thread kernel
// writes the same values.
struct TimeMapGatherParams {
    const float *x;
    uint64_t in_stride, in_len;
    const int64_t *hop_pos;
    uint64_t hop_first, hop_count;
    uint32_t channels, N;
    float *v;
    uint64_t v_stride;
};

// hipErrorInvalidValue, and no launch: N odd, below 4 or above TM_MAX_N; a null v or hop_pos; a null x with in_len > 0;
// more than 65535 channels; in_stride < in_len or v_stride < hop_count * N with more than one channel; rows of 2^31 floats
// or more; in_len >= 2^62. hop_count == 0 or channels == 0: nothing to do, hipSuccess. The grid follows from (hop_count,
// channels, N) alone.
hipError_t launch_time_map_gather(const TimeMapGatherParams &p, hipStream_t s);

}  // namespace rc

#endif
