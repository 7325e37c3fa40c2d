// Long-window path (rc_long.h): window lengths 65538 .. 2^22 as batched four-step FFTs through HBM,
// many workgroups per hop, and an overlap-add whose hops are spread over the chip.
#include "rc_dev.hpp"
#include "rc_long.h"

namespace rc {
namespace {

__device__ __forceinline__ float2 conj2(float2 a) { return make_float2(a.x, -a.y); }

// W_P^m, m < P, from the two-level table (both levels rounded from f64)
__device__ __forceinline__ float2 lw_twiddle(const LongParams &p, uint32_t m) {
    return cmul(ldg2((GV2)p.tw_hi + (m >> LW_TW_LO_BITS)), ldg2((GV2)p.tw_lo + (m & ((1u << LW_TW_LO_BITS) - 1))));
}
// position of transform output k in the work buffer: four-step order for the power-of-two transforms, natural for
// the chirp-z ones (their last column pass writes natural order)
__device__ __forceinline__ uint32_t lw_pos(const LongParams &p, uint32_t k) {
    if (p.chirp) return k;
    return ((k & ((1u << p.log2r) - 1)) << p.log2c) | (k >> p.log2r);
}
__device__ __forceinline__ size_t lw_row(const LongParams &p, int64_t hl, uint32_t ch) {
    return (size_t)ch * (size_t)p.hop_count + (size_t)hl;
}
__device__ __forceinline__ GF lw_src(const LongParams &p, int64_t hl, uint32_t ch) {
    const int64_t hop = p.hop_first + hl;
    GF xc = (GF)p.x + (size_t)ch * p.in_stride;
    GF xt = (GF)p.xtail + (size_t)ch * p.tail_stride;
    return (hop >= p.tail_hop_first) ? xt + (hop * (int64_t)p.step - p.tail_origin)
                                     : xc + (hop * (int64_t)p.step - p.in_origin);
}
__device__ __forceinline__ uint32_t brev(uint32_t v, uint32_t bits) { return __brev(v) >> (32 - bits); }

// Radix-2 DIF stages (natural -> bit-reversed order) of 2^l2-point FFTs on G interleaved sequences in LDS (element i of
// sequence g at a[i G + g]); tw = exp(-2 pi i k / 2^l2), k < 2^(l2-1); INV: conjugate twiddles (unnormalised inverse)
template <uint32_t G, bool INV>
__device__ __forceinline__ void lds_dif(float2 *a, uint32_t l2, GV2 tw) {
    const uint32_t T = blockDim.x, tid = threadIdx.x, nb = (G << l2) / 2;
    for (int s = (int)l2 - 1; s >= 0; --s) {
        const uint32_t half = 1u << s;
        for (uint32_t b = tid; b < nb; b += T) {
            const uint32_t g = b % G, bb = b / G;
            const uint32_t lo = bb & (half - 1), i = (((bb >> s) << (s + 1)) | lo) * G + g, j = i + half * G;
            float2 w = ldg2(tw + ((size_t)lo << (l2 - 1 - s)));
            if (INV) w.y = -w.y;
            const float2 u = a[i], v = a[j];
            a[i] = make_float2(u.x + v.x, u.y + v.y);
            a[j] = cmul(make_float2(u.x - v.x, u.y - v.y), w);
        }
        __syncthreads();
    }
}
// Radix-2 DIT stages with conjugate twiddles (bit-reversed -> natural order): the unnormalised inverse, one sequence
__device__ __forceinline__ void lds_dit_inv(float2 *a, uint32_t l2, GV2 tw) {
    const uint32_t T = blockDim.x, tid = threadIdx.x, nb = 1u << (l2 - 1);
    for (uint32_t s = 0; s < l2; ++s) {
        const uint32_t half = 1u << s;
        for (uint32_t b = tid; b < nb; b += T) {
            const uint32_t lo = b & (half - 1), i = ((b >> s) << (s + 1)) | lo, j = i + half;
            const float2 w = ldg2(tw + ((size_t)lo << (l2 - 1 - s)));
            const float2 u = a[i], v = cmul(a[j], conj2(w));
            a[i] = make_float2(u.x + v.x, u.y + v.y);
            a[j] = make_float2(u.x - v.x, u.y - v.y);
        }
        __syncthreads();
    }
}

// ---- column passes ----------------------------------------------------------------------------------------------
enum ColIn { CI_SAMPLES = 0, CI_CHIRP_SAMPLES = 1, CI_CHIRP_CONJ = 2, CI_WK = 3 };
enum ColOut { CO_TWIDDLE = 0, CO_Y = 1, CO_Z_CHIRP = 2, CO_Y_CHIRP = 3 };
// grid (C / LW_G, hops, channels), 256 threads, R x LW_G x 8 B of LDS. Every workgroup owns its LW_G columns of the
// hop's work buffer, so reading them all before writing any makes the pass in place.
//   in:  CI_SAMPLES        z[n] from the hop's samples (power-of-two N)
//        CI_CHIRP_SAMPLES  z[n] c[n] for n < M, 0 above (chirp-z forward)
//        CI_CHIRP_CONJ     conj(G[n]) c[n] for n < M, 0 above, G natural in the work buffer (chirp-z inverse)
//        CI_WK             the work buffer as it is (after an inverse row pass)
//   out: CO_TWIDDLE        forward: R-point FFT, times W_P^(c k1), to (k1, c)
//        CO_Y              inverse: y[2n], y[2n+1] = (Re, Im) g[n] / M x window (power-of-two N)
//        CO_Z_CHIRP        inverse: Z[n] = v[n] c[n] for n < M, natural order (chirp-z forward, done)
//        CO_Y_CHIRP        inverse: (y[2n], y[2n+1]) = conj(v[n] c[n]) / M x window (chirp-z inverse, done)
template <int IN, int OUT>
__global__ __launch_bounds__(256) void lw_col_kernel(const LongParams p) {
    extern __shared__ __attribute__((aligned(16))) float2 a[];
    constexpr bool INV = OUT != CO_TWIDDLE;
    const uint32_t l2r = p.log2r, l2c = p.log2c, c0 = blockIdx.x * LW_G, M = p.n / 2, cnt = LW_G << l2r;
    const int64_t hl = blockIdx.y;
    const uint32_t ch = blockIdx.z;
    const size_t row = lw_row(p, hl, ch);
    GV2W wk = (GV2W)p.wk + (row << (l2r + l2c));
    GF win = (GF)p.window;
    GF src = nullptr;
    if (IN == CI_SAMPLES || IN == CI_CHIRP_SAMPLES) src = lw_src(p, hl, ch);
    for (uint32_t idx = threadIdx.x; idx < cnt; idx += blockDim.x) {
        const uint32_t r = idx / LW_G, g = idx % LW_G;
        const uint32_t n = (r << l2c) + c0 + g;
        float2 v;
        if (IN == CI_SAMPLES) {
            v = make_float2(src[2 * (size_t)n] * win[2 * (size_t)n], src[2 * (size_t)n + 1] * win[2 * (size_t)n + 1]);
        } else if (IN == CI_CHIRP_SAMPLES) {
            v = n < M ? cmul(make_float2(src[2 * (size_t)n] * win[2 * (size_t)n], src[2 * (size_t)n + 1] * win[2 * (size_t)n + 1]),
                             ldg2((GV2)p.chirp_c + n))
                      : make_float2(0.f, 0.f);
        } else if (IN == CI_CHIRP_CONJ) {
            v = n < M ? cmul(conj2(ldg2((GV2)wk + n)), ldg2((GV2)p.chirp_c + n)) : make_float2(0.f, 0.f);
        } else {
            v = ldg2((GV2)wk + n);
        }
        a[idx] = v;
    }
    __syncthreads();
    lds_dif<LW_G, INV>(a, l2r, (GV2)p.tw_r);
    GFW y = (GFW)p.ybuf + row * (size_t)p.n;
    const float inv_m = 1.0f / (float)M;
    for (uint32_t idx = threadIdx.x; idx < cnt; idx += blockDim.x) {
        const uint32_t k = idx / LW_G, g = idx % LW_G, c = c0 + g;
        const float2 v = a[brev(k, l2r) * LW_G + g];
        const uint32_t n = (k << l2c) + c;  // forward: position (k1 = k, c); inverse: sample n = C r + c, r = k
        if (OUT == CO_TWIDDLE) {
            stg2(wk + n, cmul(v, lw_twiddle(p, c * k)));
        } else if (OUT == CO_Y) {
            y[2 * (size_t)n] = v.x * inv_m * win[2 * (size_t)n];
            y[2 * (size_t)n + 1] = v.y * inv_m * win[2 * (size_t)n + 1];
        } else if (n < M) {
            const float2 z = cmul(v, ldg2((GV2)p.chirp_c + n));
            if (OUT == CO_Z_CHIRP) {
                stg2(wk + n, z);
            } else {
                y[2 * (size_t)n] = z.x * inv_m * win[2 * (size_t)n];
                y[2 * (size_t)n + 1] = -z.y * inv_m * win[2 * (size_t)n + 1];
            }
        }
    }
}

// ---- row passes -------------------------------------------------------------------------------------------------
enum RowMode { RM_FWD = 0, RM_INV = 1, RM_CONV = 2 };
// grid (R, hops, channels), 512 threads, C x 8 B of LDS; row k1 in place
//   RM_FWD   C-point FFT over c: (k1, k2) = X[k1 + R k2]
//   RM_INV   inverse C-point FFT over k2, times conj W_P^(c k1): (k1, c), ready for the inverse column pass
//   RM_CONV  (chirp-z) RM_FWD, times FFT_P(conj chirp) / P, then RM_INV: the circular convolution's middle
template <int MODE>
__global__ __launch_bounds__(512) void lw_row_kernel(const LongParams p) {
    extern __shared__ __attribute__((aligned(16))) float2 a[];
    const uint32_t l2c = p.log2c, C = 1u << l2c, k1 = blockIdx.x;
    const size_t row = lw_row(p, blockIdx.y, blockIdx.z);
    GV2W base = (GV2W)p.wk + (row << (p.log2r + l2c)) + ((size_t)k1 << l2c);
    for (uint32_t i = threadIdx.x; i < C; i += blockDim.x) a[i] = ldg2((GV2)base + i);
    __syncthreads();
    lds_dif<1, MODE == RM_INV>(a, l2c, (GV2)p.tw_c);
    if (MODE == RM_FWD) {
        for (uint32_t k2 = threadIdx.x; k2 < C; k2 += blockDim.x) stg2(base + k2, a[brev(k2, l2c)]);
        return;
    }
    if (MODE == RM_CONV) {
        GV2 b = (GV2)p.chirp_b + ((size_t)k1 << l2c);
        for (uint32_t i = threadIdx.x; i < C; i += blockDim.x) a[i] = cmul(a[i], ldg2(b + brev(i, l2c)));
        __syncthreads();
        lds_dit_inv(a, l2c, (GV2)p.tw_c);
    }
    for (uint32_t c = threadIdx.x; c < C; c += blockDim.x) {
        const float2 v = MODE == RM_CONV ? a[c] : a[brev(c, l2c)];
        stg2(base + c, cmul(v, conj2(lw_twiddle(p, c * k1))));
    }
}

// ---- per-bin stages ---------------------------------------------------------------------------------------------
// real split of Z = DFT_M(z) into bin j of the N-point spectrum: zj = Z[j mod M], zm = Z[(M - j) mod M] (as §5.6)
__device__ __forceinline__ float2 lw_split_bin(float2 zj, float2 zm, float2 w) {
    const float2 E = make_float2(0.5f * (zj.x + zm.x), 0.5f * (zj.y - zm.y));
    const float2 O = make_float2(0.5f * (zj.y + zm.y), -0.5f * (zj.x - zm.x));  // (zj - conj zm) / (2 i)
    const float2 t = cmul(O, w);
    return make_float2(E.x + t.x, E.y + t.y);
}
// packed bin k of the inverse from the resynthesised bins Y[k], Y[N - k], Y[k + M], Y[M - k]: the Hermitian part
// (Re(IFFT(Y)) = IFFT((Y + conj(mirror Y)) / 2), src/fft.rs:69-73), merged to G = E + i O (as §5.6)
__device__ __forceinline__ float2 lw_merge_bin(float2 z0, float2 z0m, float2 z1, float2 z1m, float2 w) {
    const float2 h0 = make_float2(0.5f * (z0.x + z0m.x), 0.5f * (z0.y - z0m.y));
    const float2 h1 = make_float2(0.5f * (z1.x + z1m.x), 0.5f * (z1.y - z1m.y));
    const float2 E = make_float2(0.5f * (h0.x + h1.x), 0.5f * (h0.y + h1.y));
    const float2 D = make_float2(0.5f * (h0.x - h1.x), 0.5f * (h0.y - h1.y));
    const float2 O = cmul(D, conj2(w));
    return make_float2(E.x - O.y, E.y + O.x);
}
// frozen phase spec (rc_phase_theta): bins b < N/2 take the top 23 bits of hash(b), bins b + N/2 its low 16
__device__ __forceinline__ float2 lw_phasor(float m, uint32_t h, bool upper) {
    const float u = upper ? (float)(h & 0xFFFFu) * (1.0f / 65536.0f) : (float)(h >> 9) * (1.0f / 8388608.0f);
    const float th = u * 3.14159274101257324219f;
    float sn, cs;
    sincosf(th, &sn, &cs);
    return make_float2(m * cs, m * sn);  // src/fft.rs:65-68
}
__device__ __forceinline__ float lw_abs(float2 x) { return sqrtf(x.x * x.x + x.y * x.y); }

// stage 0's tail: bins j and N - j of the natural-order spectrum, j <= M. grid ((M + 256) / 256, hops, channels)
__global__ __launch_bounds__(256) void lw_split_kernel(const LongParams p) {
    const uint32_t M = p.n / 2, j = blockIdx.x * 256 + threadIdx.x;
    if (j > M) return;
    const size_t row = lw_row(p, blockIdx.y, blockIdx.z);
    GV2 Z = (GV2)p.wk + (row << (p.log2r + p.log2c));
    const float2 zj = ldg2(Z + lw_pos(p, j == M ? 0 : j)), zm = ldg2(Z + lw_pos(p, j == 0 ? 0 : M - j));
    const float2 x = lw_split_bin(zj, zm, ldg2((GV2)p.tw_n + j));
    GV2W X = (GV2W)p.spec + row * (size_t)p.n;
    stg2(X + j, x);
    if (j > 0 && j < M) stg2(X + (p.n - j), conj2(x));
}
// stage 1: |X[k]| x phasor in place on all N bins. grid (N / 256, hops, channels)
__global__ __launch_bounds__(256) void lw_phase_kernel(const LongParams p) {
    const uint32_t N = p.n, half = N / 2, k = blockIdx.x * 256 + threadIdx.x;
    if (k >= N) return;
    const int64_t hl = blockIdx.y;
    const uint32_t ch = blockIdx.z;
    const PhaseKey key = make_phase_key(p.seed_mixed, p.ch_first + ch, p.hop_first + hl);
    const bool upper = k >= half;
    const uint32_t h = phase_hash_x((upper ? k - half : k) * key.mul + key.k0);
    GV2W z = (GV2W)p.spec + lw_row(p, hl, ch) * (size_t)N + k;
    stg2(z, lw_phasor(lw_abs(ldg2((GV2)z)), h, upper));
}
// stage 2's head: packed bin k < M from the natural-order spectrum to its work-buffer position. grid (M / 256 ...)
__global__ __launch_bounds__(256) void lw_merge_kernel(const LongParams p) {
    const uint32_t N = p.n, M = N / 2, k = blockIdx.x * 256 + threadIdx.x;
    if (k >= M) return;
    const size_t row = lw_row(p, blockIdx.y, blockIdx.z);
    GV2 Y = (GV2)p.spec + row * (size_t)N;
    const float2 g = lw_merge_bin(ldg2(Y + k), ldg2(Y + (k ? N - k : 0)), ldg2(Y + k + M), ldg2(Y + M - k), ldg2((GV2)p.tw_n + k));
    stg2((GV2W)p.wk + (row << (p.log2r + p.log2c)) + lw_pos(p, k), g);
}
// The plain stretch's per-bin-pair stage: Z[j], Z[M - j] -> the four bins j, M - j, M + j, N - j (split, magnitude,
// phase) -> packed bins G[j], G[M - j] of the inverse, in place. j = 0 stands for the bins 0 and M.
// Power-of-two N: thread q is four-step position q of rows k1 <= R/2 (row k1 pairs with row R - k1, so both reads are
// contiguous; rows 0 and R/2 pair with themselves, and there the thread of the smaller j does the pair).
// Chirp-z: thread q is j = q <= M/2, natural order. grid (((R/2 + 1) C or M/2 + 1) / 256, hops, channels)
__global__ __launch_bounds__(256) void lw_pair_kernel(const LongParams p) {
    const uint32_t N = p.n, M = N / 2, q = blockIdx.x * 256 + threadIdx.x;
    uint32_t j;
    if (p.chirp) {
        if (q > M / 2) return;
        j = q;
    } else {
        const uint32_t R = 1u << p.log2r, k1 = q >> p.log2c, k2 = q & ((1u << p.log2c) - 1);
        if (k1 > R / 2) return;
        j = k1 + (k2 << p.log2r);
        const uint32_t jm = j ? M - j : 0;
        if ((k1 == 0 || k1 == R / 2) && j > jm) return;
    }
    const int64_t hl = blockIdx.y;
    const uint32_t ch = blockIdx.z;
    GV2W Z = (GV2W)p.wk + (lw_row(p, hl, ch) << (p.log2r + p.log2c));
    const uint32_t jm = j ? M - j : 0, pj = lw_pos(p, j), pm = lw_pos(p, jm);
    const float2 zj = ldg2((GV2)Z + pj), zm = ldg2((GV2)Z + pm);
    GV2 twn = (GV2)p.tw_n;
    const float A = lw_abs(lw_split_bin(zj, zm, ldg2(twn + j)));        // |X[j]| = |X[N - j]|
    const float B = lw_abs(lw_split_bin(zm, zj, ldg2(twn + (M - j))));  // |X[M - j]| = |X[M + j]| (j = 0: |X[M]|)
    const PhaseKey key = make_phase_key(p.seed_mixed, p.ch_first + ch, p.hop_first + hl);
    const uint32_t hj = phase_hash_x(j * key.mul + key.k0);
    if (j == 0) {
        const float2 y0 = lw_phasor(A, hj, false), ym = lw_phasor(B, hj, true);
        stg2(Z + pj, lw_merge_bin(y0, y0, ym, ym, ldg2(twn)));
        return;
    }
    const uint32_t hm = phase_hash_x((M - j) * key.mul + key.k0);
    const float2 yj = lw_phasor(A, hj, false), ymj = lw_phasor(B, hm, false);  // bins j, M - j
    const float2 ypj = lw_phasor(B, hj, true), ynj = lw_phasor(A, hm, true);   // bins M + j, N - j
    stg2(Z + pj, lw_merge_bin(yj, ynj, ypj, ymj, ldg2(twn + j)));
    if (jm != j) stg2(Z + pm, lw_merge_bin(ymj, ypj, ynj, yj, ldg2(twn + (M - j))));
}

// ---- overlap-add ------------------------------------------------------------------------------------------------
// ola_kernel's arithmetic, operation for operation; grid (pieces of LW_OLA_PIECE samples, hops, channels)
constexpr uint32_t LW_OLA_PIECE = 2048;
__global__ __launch_bounds__(256) void lw_ola_kernel(const OlaParams p) {
    const uint32_t N = p.n, H = N / 2;
    const int64_t hop_local = blockIdx.y;
    const uint32_t ch = blockIdx.z;
    const int64_t k = p.hop_first + hop_local;
    GF yk = (GF)p.ybuf + ((size_t)ch * p.hop_count + (size_t)hop_local) * N;
    GF prev = hop_local > 0 ? yk - N + H : (GF)p.tail + (size_t)ch * H;
    GF env = (GF)p.env;
    GFW outc = (GFW)p.out + (size_t)ch * p.out_stride;
    const uint32_t i0 = blockIdx.x * LW_OLA_PIECE;
    if (p.pitch >= 1) {
        const uint32_t i1 = min(H, i0 + LW_OLA_PIECE);
        const int64_t g0 = k * (int64_t)H;
        for (uint32_t i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
            const int64_t g = g0 + i;
            if (p.pitch == 1 || g % p.pitch == 0) outc[g / p.pitch - p.out_origin] = (yk[i] + prev[i]) * env[i] * p.amp;
        }
    } else {
        const uint32_t f = (uint32_t)(-p.pitch), S = p.samples_needed, m1 = min((S - 1) * f, i0 + LW_OLA_PIECE);
        GFW dst = outc + (k * (int64_t)p.window_out_len - p.out_origin);
        for (uint32_t m = i0 + threadIdx.x; m < m1; m += blockDim.x) {
            const uint32_t i = m / f, j = m - i * f;
            const float cur = (yk[i] + prev[i]) * env[i] * p.amp;
            const float nxt = (yk[i + 1] + prev[i + 1]) * env[i + 1] * p.amp;
            dst[m] = cur + (nxt - cur) * ((float)j / (float)f);  // math::lerp, src/math.rs:28-30
        }
    }
}
__global__ __launch_bounds__(256) void lw_save_tail_kernel(const OlaParams p) {
    const uint32_t N = p.n, H = N / 2, ch = blockIdx.y;
    GF yl = (GF)p.ybuf + ((size_t)ch * p.hop_count + (size_t)(p.hop_count - 1)) * N + H;
    GFW t = (GFW)p.tail + (size_t)ch * H;
    const uint32_t i0 = blockIdx.x * LW_OLA_PIECE, i1 = min(H, i0 + LW_OLA_PIECE);
    for (uint32_t i = i0 + threadIdx.x; i < i1; i += blockDim.x) t[i] = yl[i];
}

}  // namespace

hipError_t launch_long(int stage, const LongParams &p, hipStream_t s) {
    if (stage < 0 || stage > 3 || p.hop_count <= 0 || p.n_channels == 0) return hipErrorInvalidValue;
    if (p.log2r < LW_MIN_LOG2R || p.log2r > LW_MAX_LOG2R || p.log2c > LW_MAX_LOG2C || p.n < 4 || p.n % 2 || p.n > LW_MAX_N)
        return hipErrorInvalidValue;
    const uint32_t l2p = p.log2r + p.log2c, M = p.n / 2;
    if (p.chirp ? (2ull * M - 1 > (1ull << l2p) || !p.chirp_c || !p.chirp_b) : M != (1u << l2p)) return hipErrorInvalidValue;
    if ((stage != 1 && !p.wk) || (stage <= 2 && !p.spec) || (stage >= 2 && !p.ybuf)) return hipErrorInvalidValue;
    const uint32_t R = 1u << p.log2r, C = 1u << p.log2c;
    const int64_t per = 32768;  // grid.y limit
    for (int64_t h0 = 0; h0 < p.hop_count; h0 += per) {
        // hop index inside the launch = blockIdx.y + h0: shift the bases and the first hop instead of the index
        LongParams q = p;
        q.hop_first = p.hop_first + h0;
        const size_t sh = (size_t)h0;
        if (q.spec) q.spec = p.spec + sh * p.n;
        if (q.ybuf) q.ybuf = p.ybuf + sh * p.n;
        if (q.wk) q.wk = p.wk + (sh << l2p);
        // (the channel stride of every buffer stays hop_count rows: q.hop_count is left as it is)
        const unsigned ny = (unsigned)std::min<int64_t>(per, p.hop_count - h0);
        const dim3 gcol(C / LW_G, ny, p.n_channels), grow(R, ny, p.n_channels), b256(256), b512(512);
        const size_t lcol = sizeof(float2) * ((size_t)LW_G << p.log2r), lrow = sizeof(float2) * (size_t)C;
        auto forward = [&]() {
            if (!p.chirp) {
                hipLaunchKernelGGL((lw_col_kernel<CI_SAMPLES, CO_TWIDDLE>), gcol, b256, lcol, s, q);
                hipLaunchKernelGGL((lw_row_kernel<RM_FWD>), grow, b512, lrow, s, q);
            } else {
                hipLaunchKernelGGL((lw_col_kernel<CI_CHIRP_SAMPLES, CO_TWIDDLE>), gcol, b256, lcol, s, q);
                hipLaunchKernelGGL((lw_row_kernel<RM_CONV>), grow, b512, lrow, s, q);
                hipLaunchKernelGGL((lw_col_kernel<CI_WK, CO_Z_CHIRP>), gcol, b256, lcol, s, q);
            }
        };
        auto inverse = [&]() {
            if (!p.chirp) {
                hipLaunchKernelGGL((lw_row_kernel<RM_INV>), grow, b512, lrow, s, q);
                hipLaunchKernelGGL((lw_col_kernel<CI_WK, CO_Y>), gcol, b256, lcol, s, q);
            } else {
                hipLaunchKernelGGL((lw_col_kernel<CI_CHIRP_CONJ, CO_TWIDDLE>), gcol, b256, lcol, s, q);
                hipLaunchKernelGGL((lw_row_kernel<RM_CONV>), grow, b512, lrow, s, q);
                hipLaunchKernelGGL((lw_col_kernel<CI_WK, CO_Y_CHIRP>), gcol, b256, lcol, s, q);
            }
        };
        if (stage == 0) {
            forward();
            hipLaunchKernelGGL(lw_split_kernel, dim3((M + 256) / 256, ny, p.n_channels), b256, 0, s, q);
        } else if (stage == 1) {
            hipLaunchKernelGGL(lw_phase_kernel, dim3((p.n + 255) / 256, ny, p.n_channels), b256, 0, s, q);
        } else if (stage == 2) {
            hipLaunchKernelGGL(lw_merge_kernel, dim3((M + 255) / 256, ny, p.n_channels), b256, 0, s, q);
            inverse();
        } else {
            forward();
            const uint32_t threads = p.chirp ? M / 2 + 1 : (R / 2 + 1) * C;
            hipLaunchKernelGGL(lw_pair_kernel, dim3((threads + 255) / 256, ny, p.n_channels), b256, 0, s, q);
            inverse();
        }
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_long_ola(const OlaParams &p, hipStream_t s, bool tail_only) {
    // (a chunk of the engine holds at most 32768 hops: one launch, grid.y = hops)
    if (p.hop_count <= 0 || p.hop_count > 65535 || p.n_channels == 0 || p.n < 4 || p.n % 2) return hipErrorInvalidValue;
    const uint32_t H = p.n / 2;
    if (!tail_only) {
        const uint64_t work = p.pitch >= 1 ? H : (uint64_t)(p.samples_needed - 1) * (uint64_t)(-p.pitch);
        const unsigned nx = (unsigned)std::max<uint64_t>(1, (work + LW_OLA_PIECE - 1) / LW_OLA_PIECE);
        hipLaunchKernelGGL(lw_ola_kernel, dim3(nx, (unsigned)p.hop_count, p.n_channels), dim3(256), 0, s, p);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(lw_save_tail_kernel, dim3((H + LW_OLA_PIECE - 1) / LW_OLA_PIECE, p.n_channels), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace rc
