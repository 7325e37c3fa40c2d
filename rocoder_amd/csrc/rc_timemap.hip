// The gather stage of a time map (rc_timemap.h): hop k's N samples from wherever hop_pos[k] points, zero
// outside the input, into rows on which every hop kernel runs unchanged at a step of N.
//
// A work item is one 16-byte group of the destination: row c is hop_count * N / 4 such groups, group i belongs to hop
// i / (N / 4). With N >= 256 a wave's 64 groups lie in one hop (N / 4 is then a multiple of 64 for the power-of-two
// windows), so the position and the class of the hop - inside, outside, across an end - are wave-uniform and the branch
// does not diverge. A hop wholly inside [0, in_len) loads each group with ONE 16-byte load at the float alignment the
// position happens to have (global memory takes a dwordx4 at 4-byte alignment) and tests nothing per sample; a hop wholly
// outside stores zeros and reads nothing; only a hop across an end tests its samples one by one. A thread carries four
// groups 256 apart and issues its loads in front of its stores. The kernel moves N floats in and N floats out per hop and
// channel and does nothing else: it is bound by HBM.
#include "rc_timemap.h"

namespace rc {
namespace {

constexpr uint32_t kThreads = 256, kGroups = 4;  // groups per thread

__device__ __forceinline__ float4 gather_group(const TimeMapGatherParams &p, uint64_t x_off, uint32_t i, uint32_t groups_per_hop) {
    const uint32_t hop = i / groups_per_hop, n = (i - hop * groups_per_hop) * 4u;
    const int64_t pos = p.hop_pos[p.hop_first + hop], N = (int64_t)p.N, in_len = (int64_t)p.in_len;
    float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (pos >= 0 && pos + N <= in_len) {
        __builtin_memcpy(&q, p.x + (x_off + (uint64_t)pos + n), sizeof q);
    } else if (pos < in_len && pos + N > 0) {  // across an end: the address of a sample is formed only where it exists
        const int64_t j = pos + (int64_t)n;
        if (j >= 0 && j < in_len) q.x = p.x[x_off + (uint64_t)j];
        if (j + 1 >= 0 && j + 1 < in_len) q.y = p.x[x_off + (uint64_t)(j + 1)];
        if (j + 2 >= 0 && j + 2 < in_len) q.z = p.x[x_off + (uint64_t)(j + 2)];
        if (j + 3 >= 0 && j + 3 < in_len) q.w = p.x[x_off + (uint64_t)(j + 3)];
    }
    return q;
}

__global__ __launch_bounds__(kThreads) void time_map_gather_kernel(TimeMapGatherParams p, uint32_t groups_per_hop, uint32_t groups_per_row) {
    const uint32_t c = blockIdx.y;
    const uint64_t x_off = (uint64_t)c * p.in_stride;
    float4 *const vc = reinterpret_cast<float4 *>(p.v + (uint64_t)c * p.v_stride);
    const uint32_t i0 = blockIdx.x * (kThreads * kGroups) + threadIdx.x;
    float4 q[kGroups];
#pragma unroll
    for (uint32_t u = 0; u < kGroups; ++u) {
        const uint32_t i = i0 + u * kThreads;
        if (i < groups_per_row) q[u] = gather_group(p, x_off, i, groups_per_hop);
    }
#pragma unroll
    for (uint32_t u = 0; u < kGroups; ++u) {
        const uint32_t i = i0 + u * kThreads;
        if (i < groups_per_row) vc[i] = q[u];
    }
}

// N % 4 == 2, or rows the caller did not align: a float per thread
__global__ __launch_bounds__(kThreads) void time_map_gather_floats_kernel(TimeMapGatherParams p, uint32_t floats_per_row) {
    const uint32_t c = blockIdx.y;
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= floats_per_row) return;
    const uint32_t hop = i / p.N, n = i - hop * p.N;
    const int64_t j = p.hop_pos[p.hop_first + hop] + (int64_t)n;
    float val = 0.0f;
    if (j >= 0 && j < (int64_t)p.in_len) val = p.x[(uint64_t)c * p.in_stride + (uint64_t)j];
    p.v[(uint64_t)c * p.v_stride + i] = val;
}

}  // namespace

hipError_t launch_time_map_gather(const TimeMapGatherParams &p, hipStream_t s) {
    if (p.N < 4 || (p.N & 1u) || p.N > TM_MAX_N) return hipErrorInvalidValue;
    if (p.channels > 65535u || p.in_len >= ((uint64_t)1 << 62)) return hipErrorInvalidValue;
    if (p.hop_count == 0 || p.channels == 0) return hipSuccess;
    if (!p.v || !p.hop_pos || (!p.x && p.in_len)) return hipErrorInvalidValue;
    if (p.hop_count >= ((uint64_t)1 << 31) / p.N) return hipErrorInvalidValue;  // (32-bit indices inside a row)
    const uint64_t row = p.hop_count * p.N;
    if (p.channels > 1 && (p.in_stride < p.in_len || p.v_stride < row)) return hipErrorInvalidValue;
    const bool groups = p.N % 4 == 0 && ((uintptr_t)p.v & 15u) == 0 && (p.channels == 1 || p.v_stride % 4 == 0);
    if (groups) {
        const uint32_t per_row = (uint32_t)(row / 4), per_block = kThreads * kGroups;
        hipLaunchKernelGGL(time_map_gather_kernel, dim3((per_row + per_block - 1) / per_block, p.channels), dim3(kThreads), 0, s, p, p.N / 4,
                           per_row);
    } else {
        hipLaunchKernelGGL(time_map_gather_floats_kernel, dim3(((uint32_t)row + kThreads - 1) / kThreads, p.channels), dim3(kThreads), 0, s, p,
                           (uint32_t)row);
    }
    return hipGetLastError();
}

}  // namespace rc
