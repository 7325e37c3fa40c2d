// The look-ahead peak limiter on planar float rows (rc_engine_set_output_limiter; the definition is stated in
// include/rocoder_hip.h and, as the launcher sees it, at FramesLimitParams in rc_frames.h).
//
// Mapping. One fused kernel; a workgroup of kLimitThreads takes kLimitTile consecutive frames, every channel.
// Everything between the read and the write of a sample is per frame and lives in LDS:
//   1  rq of the frames [tile - 2 L, tile + count + 2 L): a channel maximum per frame, coalesced row reads
//   2  the sliding minimum over T = 2 L + 1 frames by log-step doubling: M_k[j] = min rq[j .. j + 2^k), one pass per k,
//      each thread holding its elements in registers between the read and the write of a pass, and then
//      m[j] = min(M_k[j], M_k[j + T - 2^k]) for the largest 2^k <= T
//   3  the prefix sums of m in two halves: a u32 prefix inside every 64-word block (a wave scan; below 64 * 2^24) and a
//      u64 base per block, so that S[t] = P[i + T] - P[i] is exact in 64 bits
//   4  g = (float)S / (float)(T * ONE) and y = clamp(x * drive * g) for every channel of the frame: the one read and the one
//      write of the sample
// Minimum and sum are integer operations: a frame's g does not depend on the tile, the launch or the chunk. The kernel is
// built twice: for look-aheads up to 256 frames with 40 KB of LDS, so that two workgroups share a CU, and up to 2048 with 84 KB.
#include "rc_frames.h"

namespace rc {
namespace {

constexpr uint32_t kLimitThreads = 1024;
constexpr uint32_t kLimitTile = 4096;
constexpr uint32_t kLimitOne = 1u << 24;
constexpr uint32_t kLimitShortLookahead = 256;  // up to here the kernel is built with 40 KB of LDS: two workgroups a CU
constexpr uint32_t kLimitWaves = kLimitThreads / 64;
constexpr uint64_t kMaxLimitPerLaunch = (uint64_t)1 << 27;  // frames: a multiple of the tile
static_assert(kMaxLimitPerLaunch % kLimitTile == 0, "tile shapes");

// rq of absolute frame a (ONE outside the job; a frame the launch was not given counts as outside: the launcher has
// refused every range that needs one, the test keeps a wrong call in bounds)
__device__ __forceinline__ uint32_t limit_rq(const FramesLimitParams &p, int64_t a) {
    if (a < 0 || (uint64_t)a >= p.n || (uint64_t)a < p.src0 || (uint64_t)a - p.src0 >= p.src_len) return kLimitOne;
    const float *x = p.src + ((uint64_t)a - p.src0);
    float amax = 0.0f;
    for (uint32_t c = 0; c < p.channels; ++c) {
        const float av = fabsf(__fmul_rn(x[(uint64_t)c * p.stride], p.drive));
        if (av < __builtin_inff() && av > amax) amax = av;  // (a NaN fails both tests)
    }
    const float r = amax > p.ceiling ? __fdiv_rn(p.ceiling, amax) : 1.0f;
    return (uint32_t)__fmul_rn(r, 16777216.0f);
}

// MAXL: the largest look-ahead this instance holds in LDS - 84 KB at 2048, 40 KB at 256. The arithmetic is the same.
template <uint32_t MAXL>
__global__ __launch_bounds__(kLimitThreads) void frames_limit_kernel(FramesLimitParams p) {
    constexpr uint32_t kLimitRq = kLimitTile + 4 * MAXL;      // words of rq a tile can need
    constexpr uint32_t kLimitM = kLimitTile + 2 * MAXL;       // words of m
    constexpr uint32_t kLimitPer = kLimitRq / kLimitThreads;  // elements of a doubling pass a thread holds
    constexpr uint32_t kLimitBlocks = kLimitM / 64 + 1;       // 64-word blocks of the prefix sums
    static_assert(kLimitRq % kLimitThreads == 0, "tile shapes");
    __shared__ uint32_t a_buf[kLimitRq + 64];  // rq, the doubling passes in place; then the in-block prefix of m
    __shared__ uint32_t m_buf[kLimitM];
    __shared__ uint64_t base[kLimitBlocks + 1];
    __shared__ uint32_t block_total[kLimitBlocks + 1];
    __shared__ uint32_t wave_min[kLimitWaves], wave_cnt[kLimitWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t tt = p.t0 + (uint64_t)blockIdx.x * kLimitTile;  // the tile's first frame
    const uint32_t count = (uint32_t)(p.t1 - tt < kLimitTile ? p.t1 - tt : kLimitTile);
    const uint32_t L = p.L, T = 2 * L + 1;
    const uint32_t len_a = count + 4 * L, len_m = count + 2 * L;

    // 1: a_buf[s] = rq of frame tt - 2 L + s
    for (uint32_t s = tid; s < len_a; s += kLimitThreads) a_buf[s] = limit_rq(p, (int64_t)tt - 2 * (int64_t)L + (int64_t)s);
    __syncthreads();

    // 2: M_k in place. An element past len_a belongs to no window that is needed: it is left out of the minimum.
    uint32_t w = 1;  // 2^k
    while (2 * w <= T) {
        uint32_t hold[kLimitPer];
#pragma unroll
        for (uint32_t i = 0; i < kLimitPer; ++i) {
            const uint32_t j = tid + i * kLimitThreads;
            uint32_t v = kLimitOne;
            if (j < len_a) {
                v = a_buf[j];
                if (j + w < len_a) v = min(v, a_buf[j + w]);
            }
            hold[i] = v;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t i = 0; i < kLimitPer; ++i) {
            const uint32_t j = tid + i * kLimitThreads;
            if (j < len_a) a_buf[j] = hold[i];
        }
        __syncthreads();
        w *= 2;
    }
    // m_buf[j] = m of frame tt - L + j = min rq over a_buf[j .. j + T)
    for (uint32_t j = tid; j < len_m; j += kLimitThreads) m_buf[j] = min(a_buf[j], a_buf[j + T - w]);
    __syncthreads();

    // 3: P[x] = sum of m_buf[j], j < x, for x <= len_m, as base[x / 64] + a_buf[x]. A wave scans a block of 64 words.
    const uint32_t n_blocks = len_m / 64 + 1;
    for (uint32_t b = wave; b < n_blocks; b += kLimitWaves) {
        const uint32_t j = b * 64 + lane;
        const uint32_t own = j < len_m ? m_buf[j] : 0u;
        uint32_t inc = own;  // inclusive scan across the wave
        for (uint32_t off = 1; off < 64; off <<= 1) {
            const uint32_t up = __shfl_up(inc, off);
            if (lane >= off) inc += up;
        }
        a_buf[j] = inc - own;
        if (lane == 63) block_total[b] = inc;
    }
    __syncthreads();
    if (tid == 0) {
        uint64_t run = 0;
        for (uint32_t b = 0; b < n_blocks; ++b) {
            base[b] = run;
            run += block_total[b];
        }
    }
    __syncthreads();

    // 4: the frames of the tile
    const uint64_t full = (uint64_t)T << 24;
    const float full_f = __ull2float_rn(full);  // exact
    uint32_t min_bits = 0x3F800000u, limited = 0;
    for (uint32_t i = tid; i < count; i += kLimitThreads) {
        const uint32_t hi = i + T;
        const uint64_t S = (base[hi >> 6] + a_buf[hi]) - (base[i >> 6] + a_buf[i]);
        const float g = __fdiv_rn(__ull2float_rn(S), full_f);
        limited += S < full ? 1u : 0u;
        min_bits = min(min_bits, __float_as_uint(g));
        const uint64_t t = tt + i;
        // (the launcher has seen to it that a frame of the range is one of src; the test keeps a wrong call in bounds)
        if (t < p.src0 || t - p.src0 >= p.src_len) continue;
        const float *x = p.src + (t - p.src0);
        float *y = p.dst + (t - p.t0);
        for (uint32_t c = 0; c < p.channels; ++c) {
            float v = __fmul_rn(__fmul_rn(x[(uint64_t)c * p.stride], p.drive), g);
            if (v > p.ceiling) v = p.ceiling;
            else if (v < -p.ceiling) v = -p.ceiling;  // (a NaN fails both tests and stays)
            y[(uint64_t)c * p.dst_stride] = v;
        }
    }
    // one atomic of each kind per workgroup that has something to report
    for (uint32_t off = 32; off; off >>= 1) {
        min_bits = min(min_bits, (uint32_t)__shfl_down(min_bits, off));
        limited += __shfl_down(limited, off);
    }
    if (lane == 0) {
        wave_min[wave] = min_bits;
        wave_cnt[wave] = limited;
    }
    __syncthreads();
    if (tid == 0) {
        for (uint32_t k = 1; k < kLimitWaves; ++k) {
            min_bits = min(min_bits, wave_min[k]);
            limited += wave_cnt[k];
        }
        if (min_bits < 0x3F800000u) atomicMin(&p.stats->min_gain_bits, min_bits);
        if (limited) atomicAdd((unsigned long long *)&p.stats->limited, (unsigned long long)limited);
    }
}

}  // namespace

hipError_t launch_frames_limit(const FramesLimitParams &p, hipStream_t s) {
    if (p.t1 <= p.t0) return hipSuccess;
    if (!p.src || !p.dst || !p.stats || p.channels == 0 || p.channels > 65535u || p.L > kLimitMaxLookahead || p.t1 > p.n ||
        !(p.drive > 0.0f && p.drive < __builtin_inff()) || !(p.ceiling > 0.0f && p.ceiling < __builtin_inff()) ||
        p.n > (UINT64_MAX >> 2) || p.src0 + p.src_len < p.src0)
        return hipErrorInvalidValue;
    // the range needs the frames [t0 - 2 L, t1 + 2 L) of the rows; those of them inside [0, n) must be frames of src
    const uint64_t halo = 2 * (uint64_t)p.L;
    const uint64_t need_lo = p.t0 > halo ? p.t0 - halo : 0, need_hi = p.t1 + halo < p.n ? p.t1 + halo : p.n;
    if (need_lo < need_hi && (need_lo < p.src0 || need_hi > p.src0 + p.src_len)) return hipErrorInvalidValue;
    for (uint64_t done = p.t0; done < p.t1; done += kMaxLimitPerLaunch) {
        FramesLimitParams q = p;
        q.dst = p.dst + (done - p.t0);
        q.t0 = done;
        q.t1 = p.t1 - done < kMaxLimitPerLaunch ? p.t1 : done + kMaxLimitPerLaunch;
        const uint32_t tiles = (uint32_t)((q.t1 - q.t0 + kLimitTile - 1) / kLimitTile);
        if (p.L <= kLimitShortLookahead) frames_limit_kernel<kLimitShortLookahead><<<dim3(tiles), dim3(kLimitThreads), 0, s>>>(q);
        else frames_limit_kernel<kLimitMaxLookahead><<<dim3(tiles), dim3(kLimitThreads), 0, s>>>(q);
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

}  // namespace rc
