// gfx950 kernels of the phase-coherent resynthesis (rc_phase.h): phase_prep, phase_scan, phase_walk and
// phase_apply, between MODE_FORWARD and MODE_RESYNTH_KEEP of run_chunk. Vector code only; phases are uint32_t in units
// of 2^-32 turn. What a kernel reads from global memory was written by an earlier launch (stream order) - within a
// launch the threads of a workgroup meet in LDS only - and no pointer here is __restrict__ or read through __ldg.
#include "rc_phase.h"

namespace rc {
namespace {

constexpr int PH_ITEMS = 9;  // bins per thread of the scan kernels: T = max(64, H / 8) threads, 9 T >= H + 1 from H = 8 on

__device__ __forceinline__ uint32_t phase_turn(float2 x) {
    const float rev = atan2f(x.y, x.x) * 0.15915494309189535f;         // [-0.5, 0.5] turn
    return (uint32_t)(int64_t)__float2ll_rn(rev * 4294967296.0f);      // mod 2^32
}

// One workgroup per (hop, channel). LDS: m2[H + 1], then in its place the peak indices lo[] / hi[] (int16) that the
// max-scan / min-scan turn into the nearest peak below / above every bin; behind them one word per thread and scan.
__global__ __launch_bounds__(256) void phase_prep_kernel(const PhasePrepParams p) {
    const uint32_t N = p.n, H = N / 2, nb = H + 1, T = blockDim.x, t = threadIdx.x;
    const size_t r = blockIdx.x, ch = blockIdx.y;
    extern __shared__ __attribute__((aligned(16))) uint32_t sm[];
    float *m2 = (float *)sm;
    int16_t *lo = (int16_t *)sm, *hi = lo + nb;
    int *seglo = (int *)(sm + nb), *seghi = seglo + T;
    const float2 *cur = p.spec + (ch * (size_t)(p.halo + p.hop_count) + p.halo + r) * N;
    const bool has_prev = p.halo + r >= 1;
    const float2 *prev = has_prev ? cur - N : cur;
    uint32_t *P = p.pe + (ch * (size_t)p.hop_count + r) * (2 * (size_t)nb), *E = P + nb;
    const uint32_t unit = (uint32_t)(0x100000000ull / N), step = p.step;
    const bool whole = H % step == 0;  // H / step an integer: the scaled deviation is a product
    const int64_t ratio = H / step;
    for (uint32_t j = t; j < nb; j += T) {
        const float2 x = cur[j];
        m2[j] = x.x * x.x + x.y * x.y;
        uint32_t e = 0;
        if (has_prev) {
            const uint32_t a1 = phase_turn(x), a0 = phase_turn(prev[j]);
            const uint32_t expect = (uint32_t)(((uint64_t)j * step) & (N - 1)) * unit;
            const int64_t dev = (int32_t)(a1 - a0 - expect);  // the principal argument
            int64_t q;
            if (whole) q = dev * ratio;
            else {
                const int64_t num = dev * (int64_t)H;
                q = num / (int64_t)step;
                if (num % (int64_t)step < 0) --q;  // floor
            }
            e = a0 - a1 + ((j & 1u) << 31) + (uint32_t)q;
        }
        E[j] = e;
    }
    if (!p.locked || !has_prev) {  // (uniform: every bin owns itself)
        for (uint32_t j = t; j < nb; j += T) P[j] = j;
        return;
    }
    __syncthreads();
    uint64_t mask = 0;  // this thread's peak flags, bin t + i T at bit i (at most 33 of them)
    for (uint32_t j = t, i = 0; j < nb; j += T, ++i) {
        bool pk = j >= 1 && j + 1 <= H;
        if (pk) {
            const float c = m2[j];
            pk = c > m2[j - 1] && c > m2[j + 1] && (j < 2 || c > m2[j - 2]) && (j + 2 > H || c > m2[j + 2]);
        }
        mask |= (uint64_t)pk << i;
    }
    __syncthreads();
    for (uint32_t j = t, i = 0; j < nb; j += T, ++i) {
        const bool pk = (mask >> i) & 1;
        lo[j] = pk ? (int16_t)j : (int16_t)-1;
        hi[j] = pk ? (int16_t)j : (int16_t)0x7fff;
    }
    __syncthreads();
    const uint32_t S = (nb + T - 1) / T;  // bins per segment: thread t scans [t S, (t + 1) S)
    const int j0 = (int)min(t * S, nb), j1 = (int)min(t * S + S, nb);
    int up = -1, down = 0x7fff;
    for (int j = j0; j < j1; ++j) {
        up = max(up, (int)lo[j]);
        lo[j] = (int16_t)up;
    }
    for (int j = j1 - 1; j >= j0; --j) {
        down = min(down, (int)hi[j]);
        hi[j] = (int16_t)down;
    }
    seglo[t] = up;
    seghi[t] = down;
    __syncthreads();
    for (uint32_t d = 1; d < T; d <<= 1) {  // inclusive scans over the segments: max from below, min from above
        int a = seglo[t], b = seghi[t];
        if (t >= d) a = max(a, seglo[t - d]);
        if (t + d < T) b = min(b, seghi[t + d]);
        __syncthreads();
        seglo[t] = a;
        seghi[t] = b;
        __syncthreads();
    }
    for (uint32_t j = t; j < nb; j += T) {
        const uint32_t seg = j / S;
        int L = lo[j], R = hi[j];
        if (seg > 0) L = max(L, seglo[seg - 1]);
        if (seg + 1 < T) R = min(R, seghi[seg + 1]);
        int own = (int)j;  // a hop without a peak: every bin owns itself
        if (L >= 0 && R < 0x7fff) own = ((int)j - L <= R - (int)j) ? L : R;  // the lower one on a tie
        else if (L >= 0) own = L;
        else if (R < 0x7fff) own = R;
        P[j] = (uint32_t)own;
    }
}

// One workgroup per (block of hops, channel): the composed map (Q, s) from the block's start in LDS, a barrier between
// the gathers of a hop and the stores that replace its row
__global__ __launch_bounds__(1024) void phase_scan_kernel(const PhaseScanParams p) {
    const uint32_t H = p.n / 2, nb = H + 1, T = blockDim.x, t = threadIdx.x;
    const size_t ch = blockIdx.y;
    extern __shared__ __attribute__((aligned(16))) uint32_t sm[];
    uint32_t *S = sm;
    uint16_t *Q = (uint16_t *)(sm + nb);
    const int64_t r0 = (int64_t)blockIdx.x * p.block, r1 = r0 + (int64_t)p.block < p.hop_count ? r0 + (int64_t)p.block : p.hop_count;
    for (uint32_t j = t; j < nb; j += T) {
        S[j] = 0;
        Q[j] = (uint16_t)j;
    }
    __syncthreads();
    uint32_t *row = p.pe + (ch * (size_t)p.hop_count + (size_t)r0) * (2 * (size_t)nb);
    for (int64_t r = r0; r < r1; ++r, row += 2 * (size_t)nb) {
        uint32_t q[PH_ITEMS], s[PH_ITEMS];
#pragma unroll
        for (int i = 0; i < PH_ITEMS; ++i) {
            const uint32_t j = t + (uint32_t)i * T;
            q[i] = s[i] = 0;
            if (j < nb) {
                const uint32_t pj = row[j];
                q[i] = Q[pj];
                s[i] = S[pj] + row[nb + pj];
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PH_ITEMS; ++i) {
            const uint32_t j = t + (uint32_t)i * T;
            if (j < nb) {
                Q[j] = (uint16_t)q[i];
                S[j] = s[i];
                row[j] = q[i];
                row[nb + j] = s[i];
            }
        }
        __syncthreads();
    }
}

// One workgroup per channel: the carried state through the blocks' last rows
__global__ __launch_bounds__(1024) void phase_walk_kernel(const PhaseWalkParams p) {
    const uint32_t H = p.n / 2, nb = H + 1, T = blockDim.x, t = threadIdx.x;
    const size_t ch = blockIdx.x;
    extern __shared__ __attribute__((aligned(16))) uint32_t sm[];
    uint32_t *TH = sm;
    uint32_t *theta = p.theta + ch * nb;
    for (uint32_t j = t; j < nb; j += T) TH[j] = theta[j];
    __syncthreads();
    const int64_t n_blocks = (p.hop_count + p.block - 1) / p.block;
    for (int64_t b = 0; b < n_blocks; ++b) {
        uint32_t *base = p.base + (ch * (size_t)n_blocks + (size_t)b) * nb;
        const int64_t last = ((b + 1) * (int64_t)p.block < p.hop_count ? (b + 1) * (int64_t)p.block : p.hop_count) - 1;
        const uint32_t *row = p.pe + (ch * (size_t)p.hop_count + (size_t)last) * (2 * (size_t)nb);
        uint32_t v[PH_ITEMS];
#pragma unroll
        for (int i = 0; i < PH_ITEMS; ++i) {
            const uint32_t j = t + (uint32_t)i * T;
            v[i] = 0;
            if (j < nb) {
                base[j] = TH[j];
                v[i] = TH[row[j]] + row[nb + j];
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PH_ITEMS; ++i) {
            const uint32_t j = t + (uint32_t)i * T;
            if (j < nb) TH[j] = v[i];
        }
        __syncthreads();
    }
    for (uint32_t j = t; j < nb; j += T) theta[j] = TH[j];
}

// grid (bins / 256, hops, channels)
__global__ __launch_bounds__(256) void phase_apply_kernel(const PhaseApplyParams p) {
    const uint32_t N = p.n, H = N / 2, nb = H + 1;
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nb) return;
    const size_t r = blockIdx.y, ch = blockIdx.z;
    const size_t n_blocks = (size_t)((p.hop_count + p.block - 1) / p.block);
    const uint32_t *row = p.pe + (ch * (size_t)p.hop_count + r) * (2 * (size_t)nb);
    const uint32_t *base = p.base + (ch * n_blocks + r / p.block) * nb;
    const uint32_t theta = base[row[j]] + row[nb + j];
    const float2 x = p.spec[(ch * (size_t)(p.halo + p.hop_count) + p.halo + r) * N + j];
    float2 z = x;
    if (theta) {
        // v_sin / v_cos take revolutions. The nearest quarter turn comes off in integers, so the argument is within an
        // eighth of a turn and its conversion to f32 is good to 2^-28 turn; the quarter turns are swaps and signs
        const uint32_t quarter = (theta + 0x20000000u) >> 30;
        const float rev = (float)(int32_t)(theta - (quarter << 30)) * 2.3283064365386963e-10f;
        const float cr = __builtin_amdgcn_cosf(rev), sr = __builtin_amdgcn_sinf(rev);
        const float c = (quarter & 1) ? ((quarter & 2) ? sr : -sr) : ((quarter & 2) ? -cr : cr);
        const float s = (quarter & 1) ? ((quarter & 2) ? -cr : cr) : ((quarter & 2) ? -sr : sr);
        z = make_float2(x.x * c - x.y * s, x.x * s + x.y * c);
    }
    float2 *out = p.out + (ch * (size_t)p.hop_count + r) * N;
    out[j] = z;
    if (j > 0 && j < H) out[N - j] = make_float2(z.x, -z.y);
}

uint32_t scan_threads(uint32_t n) { return n / 16 > 64 ? n / 16 : 64; }  // max(64, H / 8)
bool phase_n_ok(uint32_t n) { return n >= 32 && n <= kPhaseMaxN && (n & (n - 1)) == 0; }

}  // namespace

hipError_t launch_phase_prep(const PhasePrepParams &p, hipStream_t s) {
    if (!phase_n_ok(p.n) || p.step == 0 || p.halo > 1 || p.hop_count <= 0 || p.n_channels == 0) return hipErrorInvalidValue;
    const uint32_t nb = p.n / 2 + 1, T = nb > 256 ? 256 : 64;
    hipLaunchKernelGGL(phase_prep_kernel, dim3((uint32_t)p.hop_count, p.n_channels), dim3(T), (nb + 2 * T) * sizeof(uint32_t), s, p);
    return hipGetLastError();
}

hipError_t launch_phase_scan(const PhaseScanParams &p, hipStream_t s) {
    if (!phase_n_ok(p.n) || p.block == 0 || p.hop_count <= 0 || p.n_channels == 0) return hipErrorInvalidValue;
    const uint32_t nb = p.n / 2 + 1;
    const size_t lds = (nb + (nb + 1) / 2) * sizeof(uint32_t);
    hipLaunchKernelGGL(phase_scan_kernel, dim3((uint32_t)phase_blocks(p.hop_count, p.block), p.n_channels), dim3(scan_threads(p.n)), lds, s, p);
    return hipGetLastError();
}

hipError_t launch_phase_walk(const PhaseWalkParams &p, hipStream_t s) {
    if (!phase_n_ok(p.n) || p.block == 0 || p.hop_count <= 0 || p.n_channels == 0) return hipErrorInvalidValue;
    const uint32_t nb = p.n / 2 + 1;
    hipLaunchKernelGGL(phase_walk_kernel, dim3(p.n_channels), dim3(scan_threads(p.n)), nb * sizeof(uint32_t), s, p);
    return hipGetLastError();
}

hipError_t launch_phase_apply(const PhaseApplyParams &p, hipStream_t s) {
    if (!phase_n_ok(p.n) || p.block == 0 || p.halo > 1 || p.hop_count <= 0 || p.hop_count > 65535 || p.n_channels == 0 || p.n_channels > 65535)
        return hipErrorInvalidValue;
    const uint32_t nb = p.n / 2 + 1;
    hipLaunchKernelGGL(phase_apply_kernel, dim3((nb + 255) / 256, (uint32_t)p.hop_count, p.n_channels), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace rc
