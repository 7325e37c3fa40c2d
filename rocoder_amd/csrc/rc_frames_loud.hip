// The two measurements of rc_engine_stretch_frames_loud on the finished planar rows of a job (the definition is stated in
// include/rocoder_hip.h, the launchers' contracts in rc_frames.h): K-weighted sub-block energies and the true peak.
//
// Energies. The K-weighting is a recurrence, and two facts make it parallel. It is linear: kLoudRun frames map
// the state they meet affinely to the state they leave, and the linear part is the same matrix for every run, a power of
// the state-transition matrix A. And it forgets: a state dies out by 1.6e-12 of a sub-block's energy within two sub-blocks,
// so a workgroup owns a span of sub-blocks of one row, starts from a zero state kLoudWarm sub-blocks in front of it (at
// frame 0 where the row starts sooner: then it IS the definition) and no state crosses workgroups.
// A workgroup walks its frames in chunks of kLoudChunk = 256 lanes x kLoudRun frames, staged through LDS with coalesced
// loads. Per chunk: (1) every lane runs its 16 frames from a zero state - lane 0 from the state the last chunk left - and
// keeps its end state; (2) a Kogge-Stone scan over the lanes, eight steps through LDS, v[i] = A^(16 d) v[i - d] + v[i] with
// the host's f64 powers, turns them into the true end state of every lane; (3) every lane runs its frames again from the
// end state of the lane in front of it, squares and sums, apart for the two sub-blocks a run can touch; (4) one thread
// per sub-block of the chunk adds the lanes' sums in lane order to the sub-block's f64 accumulator in LDS. Every sum has
// a fixed order and every energy word is stored once: no atomics, and a job measured twice gives the same words.
// All of it is f64: the high-pass's poles lie 0.005 from the unit circle at 48 kHz and 3e-4 from it at 768 kHz, where an
// f32 recurrence amplifies its own rounding by 1e5. The kernel stays latency-bound on two dependent FMAs a frame.
//
// True peak. A workgroup takes kTpTile frames of one row and stages them with the 31 + 32 frames around them, zeros
// outside [0, n), and the 4 x 64 table in LDS. A lane holds four frames 256 apart and their four phases: sixteen chains
// acc = fmaf(h[p][j], y[q - 31 + j], acc), j ascending from +0 - the resampler's definition at the step 1/4 - fed by four
// conflict-free LDS reads and four broadcast reads a tap. Nothing of the 4 n oversampled frames is stored: the finite
// magnitudes, the row's own included, join the peak word by one atomicMax per workgroup, as launch_frames_peak's do.
#include "rc_frames.h"

namespace rc {
namespace {

constexpr uint32_t kLoudChunk = kFramesThreads * kLoudRun;        // 4096 frames
constexpr uint32_t kLoudMaxSpan = 32;                             // frames_loud_span's upper end
constexpr uint32_t kLoudChunkSubs = kLoudChunk / kLoudMinSub + 3;  // sub-blocks a chunk can touch (7), rounded up
constexpr uint32_t kLoudMaxSub = 1u << 20;                        // (span + warm) * sub stays far below 2^32
constexpr uint32_t kLoudSpansPerLaunch = 1u << 20;

struct LoudState {
    double s1, s2, u1, u2;
};

// one frame of the two biquads, direct form II transposed; returns the K-weighted sample
__device__ __forceinline__ double loud_step(const double *cf, LoudState &s, double x) {
    const double y1 = fma(cf[0], x, s.s1);
    s.s1 = fma(-cf[3], y1, fma(cf[1], x, s.s2));
    s.s2 = fma(-cf[4], y1, cf[2] * x);
    const double y2 = fma(cf[5], y1, s.u1);
    s.u1 = fma(-cf[8], y2, fma(cf[6], y1, s.u2));
    s.u2 = fma(-cf[9], y2, cf[7] * y1);
    return y2;
}

__global__ __launch_bounds__(kFramesThreads) void frames_loud_energy_kernel(FramesLoudEnergyParams p, uint32_t span, uint64_t first_span) {
    __shared__ float x[kLoudChunk + kLoudChunk / 16];  // frame i of the chunk at i + i / 16: a lane's run starts 17 floats after its neighbour's
    __shared__ double st[2][kFramesThreads][4];
    __shared__ double part[2][kFramesThreads];
    __shared__ double eacc[kLoudMaxSpan];
    const uint32_t tid = threadIdx.x, sub = p.sub;
    const uint64_t j0 = (first_span + blockIdx.x) * span;
    if (j0 >= p.nb) return;  // (the whole workgroup)
    const uint64_t j1 = p.nb - j0 < span ? p.nb : j0 + span;
    const uint64_t jb = j0 > kLoudWarm ? j0 - kLoudWarm : 0;  // the sub-block the recurrence starts at
    const float *row = p.planar + (uint64_t)blockIdx.y * p.stride + jb * sub;
    // frames relative to jb * sub from here on: 32 bits hold (span + warm) * sub
    const uint32_t rel_end = (uint32_t)(j1 - jb) * sub;
    const uint32_t jm = (uint32_t)(j0 - jb), jn = (uint32_t)(j1 - jb);  // the measured sub-blocks, relative to jb
    if (tid < kLoudMaxSpan) eacc[tid] = 0.0;
    LoudState in{0.0, 0.0, 0.0, 0.0};  // the state in front of the chunk, in every lane
    for (uint32_t tc = 0; tc < rel_end; tc += kLoudChunk) {
        __syncthreads();  // (the last chunk's reads of x, st and part are over)
#pragma unroll
        for (uint32_t k = 0; k < kLoudRun; ++k) {
            const uint32_t i = tid + k * kFramesThreads, t = tc + i;
            x[i + i / 16] = t < rel_end ? row[t] : 0.0f;
        }
        __syncthreads();
        float xs[kLoudRun];
#pragma unroll
        for (uint32_t k = 0; k < kLoudRun; ++k) xs[k] = x[tid * (kLoudRun + 1) + k];
        // (1) the run from a zero state; lane 0 carries the chunk's incoming state
        LoudState s = tid == 0 ? in : LoudState{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (uint32_t k = 0; k < kLoudRun; ++k) (void)loud_step(p.coef, s, (double)xs[k]);
        double v[4] = {s.s1, s.s2, s.u1, s.u2};
        // (2) inclusive scan: after the step with d, v is the end state of lane tid had lane tid - 2 d + 1 started from zero
        uint32_t cur = 0;
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) {
            const uint32_t d = 1u << k;
            st[cur][tid][0] = v[0];
            st[cur][tid][1] = v[1];
            st[cur][tid][2] = v[2];
            st[cur][tid][3] = v[3];
            __syncthreads();
            if (tid >= d) {
                const double *w = st[cur][tid - d];
                const double w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
                const double *m = p.step[k];
#pragma unroll
                for (uint32_t r = 0; r < 4; ++r) v[r] = fma(m[4 * r], w0, fma(m[4 * r + 1], w1, fma(m[4 * r + 2], w2, fma(m[4 * r + 3], w3, v[r]))));
            }
            cur ^= 1u;
        }
        st[cur][tid][0] = v[0];
        st[cur][tid][1] = v[1];
        st[cur][tid][2] = v[2];
        st[cur][tid][3] = v[3];
        __syncthreads();
        // (3) the run again, from the end state of the lane in front
        if (tid) {
            const double *w = st[cur][tid - 1];
            s = LoudState{w[0], w[1], w[2], w[3]};
        } else
            s = in;
        {
            const double *w = st[cur][kFramesThreads - 1];
            in = LoudState{w[0], w[1], w[2], w[3]};
        }
        const uint32_t t_lo = tc + tid * kLoudRun;
        const uint32_t tb = (t_lo / sub + 1u) * sub;  // the first frame of the sub-block behind the one the run starts in
        const uint32_t lim1 = t_lo >= rel_end ? 0u : rel_end - t_lo < kLoudRun ? rel_end - t_lo : kLoudRun;
        const uint32_t lim0 = tb - t_lo < lim1 ? tb - t_lo : lim1;
        double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
        for (uint32_t k = 0; k < kLoudRun; ++k) {
            const double y = loud_step(p.coef, s, (double)xs[k]);
            if (k < lim0) acc0 = fma(y, y, acc0);
            else if (k < lim1) acc1 = fma(y, y, acc1);
        }
        part[0][tid] = acc0;
        part[1][tid] = acc1;
        __syncthreads();
        // (4) the sub-blocks of the chunk, one thread each, lanes in ascending order
        if (tid < kLoudChunkSubs) {
            const uint32_t j = tc / sub + tid;
            const uint64_t lo64 = (uint64_t)j * sub, hi64 = lo64 + sub;
            const uint32_t chunk_end = tc + kLoudChunk < rel_end ? tc + kLoudChunk : rel_end;
            if (j >= jm && j < jn && lo64 < chunk_end) {
                const uint32_t lo = (uint32_t)lo64 > tc ? (uint32_t)lo64 : tc, hi = hi64 < chunk_end ? (uint32_t)hi64 : chunk_end;
                uint32_t i = (lo - tc) / kLoudRun;
                const uint32_t i_last = (hi - 1u - tc) / kLoudRun;
                double acc = eacc[j - jm];
                if (tc + i * kLoudRun < (uint32_t)lo64) acc += part[1][i++];  // a run that began in the sub-block in front
                for (; i <= i_last; ++i) acc += part[0][i];
                eacc[j - jm] = acc;
            }
        }
    }
    __syncthreads();
    if (tid < jn - jm) p.energy[(uint64_t)blockIdx.y * p.e_stride + j0 + tid] = (float)eacc[tid];
}

constexpr uint32_t kTpTile = 1024, kTpTaps = 64, kTpLead = 31;  // rc_resample_table(1, 4): W = 32, T = 64, k0 = q - 31
constexpr uint32_t kTpPer = kTpTile / kFramesThreads;
constexpr uint64_t kTpTilesPerLaunch = (uint64_t)1 << 17;

__device__ __forceinline__ uint32_t finite_bits(float v) {
    const uint32_t b = __float_as_uint(v) & 0x7fffffffu;
    return b < 0x7f800000u ? b : 0u;
}

__global__ __launch_bounds__(kFramesThreads) void frames_true_peak_kernel(FramesTruePeakParams p, uint64_t first_tile) {
    __shared__ float span[kTpTile + kTpTaps];
    __shared__ float h[4 * kTpTaps];
    __shared__ uint32_t wave_max[kFramesThreads / 64];
    const uint32_t tid = threadIdx.x;
    const uint64_t t0 = (first_tile + blockIdx.x) * kTpTile;
    if (t0 >= p.n) return;  // (the whole workgroup)
    const uint32_t count = (uint32_t)(p.n - t0 < kTpTile ? p.n - t0 : kTpTile);
    const float *row = p.planar + (uint64_t)blockIdx.y * p.stride;
    for (uint32_t s = tid; s < kTpTile + kTpTaps; s += kFramesThreads) {
        const int64_t a = (int64_t)t0 - (int64_t)kTpLead + (int64_t)s;
        span[s] = a >= 0 && (uint64_t)a < p.n ? row[a] : 0.0f;
    }
    static_assert(4 * kTpTaps == kFramesThreads, "one table entry a thread");
    h[tid] = p.table[tid];
    __syncthreads();
    float acc[kTpPer][4];
#pragma unroll
    for (uint32_t k = 0; k < kTpPer; ++k) acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0.0f;
#pragma unroll 4
    for (uint32_t j = 0; j < kTpTaps; ++j) {
        const float h0 = h[j], h1 = h[kTpTaps + j], h2 = h[2 * kTpTaps + j], h3 = h[3 * kTpTaps + j];
#pragma unroll
        for (uint32_t k = 0; k < kTpPer; ++k) {
            const float v = span[tid + k * kFramesThreads + j];
            acc[k][0] = fmaf(h0, v, acc[k][0]);
            acc[k][1] = fmaf(h1, v, acc[k][1]);
            acc[k][2] = fmaf(h2, v, acc[k][2]);
            acc[k][3] = fmaf(h3, v, acc[k][3]);
        }
    }
    uint32_t m = 0;
#pragma unroll
    for (uint32_t k = 0; k < kTpPer; ++k) {
        const uint32_t i = tid + k * kFramesThreads;
        if (i < count) {
            m = max(m, finite_bits(span[i + kTpLead]));
            m = max(max(m, finite_bits(acc[k][0])), max(finite_bits(acc[k][1]), max(finite_bits(acc[k][2]), finite_bits(acc[k][3]))));
        }
    }
    for (uint32_t off = 32; off; off >>= 1) m = max(m, (uint32_t)__shfl_down(m, off));
    if ((tid & 63u) == 0) wave_max[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        for (uint32_t w = 1; w < kFramesThreads / 64; ++w) m = max(m, wave_max[w]);
        if (m) atomicMax(&p.norm->peak_bits, m);
    }
}

}  // namespace

hipError_t launch_frames_loud_energy(const FramesLoudEnergyParams &p, hipStream_t s) {
    if (p.nb == 0) return hipSuccess;
    if (!p.planar || !p.energy || p.channels == 0 || p.channels > 65535u || p.sub < kLoudMinSub || p.sub > kLoudMaxSub ||
        p.nb > p.n / p.sub || p.e_stride < p.nb || p.stride < p.n)
        return hipErrorInvalidValue;
    const uint32_t span = frames_loud_span(p.channels, p.nb);
    static_assert(kLoudMaxSpan >= 32 && kLoudChunkSubs <= kFramesThreads, "frames_loud_span's range");
    const uint64_t spans = (p.nb + span - 1) / span;
    for (uint64_t done = 0; done < spans; done += kLoudSpansPerLaunch) {
        const uint32_t now = (uint32_t)(spans - done < kLoudSpansPerLaunch ? spans - done : kLoudSpansPerLaunch);
        frames_loud_energy_kernel<<<dim3(now, p.channels), dim3(kFramesThreads), 0, s>>>(p, span, done);
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

hipError_t launch_frames_true_peak(const FramesTruePeakParams &p, hipStream_t s) {
    if (p.n == 0) return hipSuccess;
    if (!p.planar || !p.table || !p.norm || p.channels == 0 || p.channels > 65535u || p.stride < p.n || p.n > (UINT64_MAX >> 4))
        return hipErrorInvalidValue;
    const uint64_t tiles = (p.n + kTpTile - 1) / kTpTile;
    for (uint64_t done = 0; done < tiles; done += kTpTilesPerLaunch) {
        const uint32_t now = (uint32_t)(tiles - done < kTpTilesPerLaunch ? tiles - done : kTpTilesPerLaunch);
        frames_true_peak_kernel<<<dim3(now, p.channels), dim3(kFramesThreads), 0, s>>>(p, done);
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

}  // namespace rc
