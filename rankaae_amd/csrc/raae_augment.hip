// The augmentations of a training batch, behind the step head (raae_step_begin, raae_optim.hip): the energy shift
// (`spec_shift`), the Gaussian broadening (`spec_broaden`) and the gain and tilt (`spec_gain`, `spec_tilt`).
#include "raae_common.h"
#include "raae_philox.h"

namespace {

using raae::normal4;

// ---- the per-row draws: u = (h >> 8) * 2^-24 with h = lowbias32(lowbias32(b + off + k1) ^ k2), the step's dropout
// hash at an index no tape element has.  Four ranges of `off`, 2^29 rows wide each, disjoint from one another and from
// the dropout elements (< 2^31), the last one ending at 2^32 - 1 ----
constexpr uint32_t SPEC_SHIFT_OFF = 0x80000000u;
constexpr uint32_t SPEC_GAIN_OFF = 0xA0000000u;
constexpr uint32_t SPEC_BROADEN_OFF = 0xC0000000u;
constexpr uint32_t SPEC_TILT_OFF = 0xE0000000u;
constexpr int SPEC_NORM_BMAX = 1 << 29;
__device__ __forceinline__ float spec_row_unit(uint32_t b, uint32_t off, uint32_t k1, uint32_t k2) {
#pragma clang fp contract(off)
    const uint32_t h = raae::lowbias32(raae::lowbias32(b + off + k1) ^ k2);
    return (float)(h >> 8) * (1.0f / 16777216.0f);                // exact: 24 bits
}
// (2 u - 1) * m for the draw at hash index b + off
__device__ __forceinline__ float spec_row_draw(uint32_t b, uint32_t off, uint32_t k1, uint32_t k2, float m) {
#pragma clang fp contract(off)
    return (2.f * spec_row_unit(b, off, k1, k2) - 1.f) * m;       // (2 u - 1 is exact; the product is the only rounding)
}

// ---- energy-shift augmentation (config key `spec_shift`): the batch rows resampled at l + delta_b, then the noise ----
// Runs BEHIND the step head and reads the counter, the seed, the hash keys and the row cursor as the head published
// them (no + 1, no + stride here).  Row b draws delta_b = (2 u_b - 1) * s at index SPEC_SHIFT_OFF + b.
// Every rounding is written out and the draw and the function below are compiled with contraction off (a product fused
// into the sum that follows it would skip a rounding: x = l + delta_b must see the ROUNDED delta_b), so the float4 body
// and the scalar body give the same bits and a float64 reference can follow them: delta_b is one multiply,
// x = clamp(l + delta_b) one add, f = x - floor(x) is exact, the interpolation a subtraction, a product and a sum.  The
// noise term is the head's expression with the head's Gaussian numbering.  Out of place, no LDS, no atomics: a replay
// is bitwise.
struct SpecAugArgs {
    const float* spec; const long* idx; const int* cursor; const unsigned long long* rng_state; int B; int L;
    float max_shift; float spec_noise; long noise_goff; float* spec_out;
};
__device__ __forceinline__ float spec_shift_delta(uint32_t b, uint32_t k1, uint32_t k2, float s) {
    return spec_row_draw(b, SPEC_SHIFT_OFF, k1, k2, s);
}
__device__ __forceinline__ float spec_shift_sample(const float* row, int l, int L, float delta) {
#pragma clang fp contract(off)
    const float x = fminf(fmaxf((float)l + delta, 0.f), (float)(L - 1));
    const float fl = floorf(x);
    const int i0 = (int)fl, i1 = min(i0 + 1, L - 1);
    const float f = x - fl;                                       // exact (Sterbenz / x < 2^24)
    const float v0 = row[i0];
    // f == 0: the sample itself (v0 + 0 * (v1 - v0) would turn -0 into +0 and an Inf neighbour into NaN)
    const float d = row[i1] - v0, p = f * d;
    return f == 0.f ? v0 : v0 + p;
}
__device__ __forceinline__ void spec_augment_body(const SpecAugArgs& a) {
    const unsigned long long ctr = a.rng_state[0], seed = a.rng_state[1];
    const uint32_t k1 = reinterpret_cast<const unsigned*>(a.rng_state + 2)[0];
    const uint32_t k2 = reinterpret_cast<const unsigned*>(a.rng_state + 2)[1];
    const long* idx = a.idx + (a.cursor[0] - a.B);
    const long nthreads = (long)gridDim.x * 256, t0 = (long)blockIdx.x * 256 + threadIdx.x;
    const long n = (long)a.B * a.L;
    // four samples of one row per thread and one float4 store when the rows are whole quads and spec_out is 16-byte
    // aligned (decided HERE, per plane: the trials of a batch launch one instance with one grid); else one per thread
    if ((a.L & 3) == 0 && ((uintptr_t)a.spec_out & 15) == 0) {
        for (long i4 = t0; i4 * 4 < n; i4 += nthreads) {
            const long i = i4 * 4;
            const int b = (int)(i / a.L), l = (int)(i - (long)b * a.L);
            const float* row = a.spec + (size_t)idx[b] * a.L;
            const float delta = spec_shift_delta((uint32_t)b, k1, k2, a.max_shift);
            float4 v;
            v.x = spec_shift_sample(row, l, a.L, delta); v.y = spec_shift_sample(row, l + 1, a.L, delta);
            v.z = spec_shift_sample(row, l + 2, a.L, delta); v.w = spec_shift_sample(row, l + 3, a.L, delta);
            if (a.spec_noise != 0.f) {
                float z[4];
                normal4((a.noise_goff + i) >> 2, ctr, seed, z);
                v.x += z[0] * a.spec_noise; v.y += z[1] * a.spec_noise; v.z += z[2] * a.spec_noise; v.w += z[3] * a.spec_noise;
            }
            *reinterpret_cast<float4*>(a.spec_out + i) = v;
        }
    } else {
        for (long i = t0; i < n; i += nthreads) {
            const int b = (int)(i / a.L), l = (int)(i - (long)b * a.L);
            const float* row = a.spec + (size_t)idx[b] * a.L;
            float v = spec_shift_sample(row, l, a.L, spec_shift_delta((uint32_t)b, k1, k2, a.max_shift));
            if (a.spec_noise != 0.f) { float z[4]; normal4((a.noise_goff + i) >> 2, ctr, seed, z); v += z[(a.noise_goff + i) & 3] * a.spec_noise; }
            a.spec_out[i] = v;
        }
    }
}
__global__ __launch_bounds__(256) void spec_augment_kernel(SpecAugArgs a) { spec_augment_body(a); }
__global__ __launch_bounds__(256) void spec_augment_kernel_m(const SpecAugArgs* t) {
    const SpecAugArgs a = t[blockIdx.z];
    spec_augment_body(a);
}

// ---- resolution augmentation (config key `spec_broaden`): row b convolved with a Gaussian of its own width, then the
// shift, then the noise ----
// Behind the step head on the same state, like the kernel above.  Row b draws sigma_b = v_b * s, v_b the unit draw at
// index SPEC_BROADEN_OFF + b.  A convolution reads its neighbours, so this is the one augmentation body that stages
// (spec_staged_body below, which also serves the normalisation kernels): ONE workgroup works on ONE row at a time, in
// three stages with a barrier between them --
//   1. the row with R = ceil(3 s) replicated samples at either end -> LDS (`in`, L + 2 R floats), and the 2 R + 1
//      weights w_j = expf(-(float)(j j) * q), q = 1 / (2 sigma sigma), w_0 = 1 -> LDS (one thread each);
//   2. thread t, for l = t, t + 256, ...: g[l] = (sum_j w_j in[l + j]) / (sum_j w_j) -> LDS, both sums in ascending j,
//      the first as ONE fmaf per tap (acc = fmaf(w_j, in, acc): one rounding per tap, and a product that cannot be
//      contracted differently in another body -- there is one body), the second a plain fp32 sum every thread repeats
//      beside it (the weight is in a register anyway; no reduction, no second barrier).  Lanes read consecutive LDS
//      words and one broadcast word per tap: conflict free;
//   3. out[b][l] = spec_shift_sample(g, l, delta_b) + noise: the functions of the kernel above, unchanged, on the LDS
//      row.  A thread takes one QUAD of the step's Gaussian numbering (one Philox block) and the up to four samples of
//      the row inside it, whatever L and the row's offset are: one body, no alignment case.
// sigma_b == 0 (v_b == 0, or s == 0): stage 1 copies the row to g as it is and stage 2 is skipped -- the bits survive,
// no 0 / 0.  expf, not __expf: the weights are specified to expf's accuracy.  q, the weights and sigma_b are computed
// with contraction off; R is one value per plane (from its own argument block), the LDS image is laid out for R = 64
// whatever R is, so that the planes of a batch share one launch geometry.  No atomics, fixed summation order: the
// result does not depend on the grid, and a replay is bitwise the eager call.
constexpr int SPEC_BROADEN_RMAX = 64;
constexpr int SPEC_BROADEN_LMAX = 8192;
struct SpecAug2Args {
    static constexpr bool NORM = false;
    const float* spec; const long* idx; const int* cursor; const unsigned long long* rng_state; int B; int L;
    float max_sigma; float max_shift; float spec_noise; long noise_goff; float* spec_out;
};
__host__ __device__ __forceinline__ float spec_broaden_radius_f(float s) {
#pragma clang fp contract(off)
    return ceilf(3.f * s);                                        // (one fp32 product, then the ceiling)
}
// the range check, in floating point BEFORE any conversion: 3 s may be beyond every int, or Inf for a finite s (false
// for a NaN, too)
__host__ __forceinline__ bool spec_broaden_radius_ok(float s) { return s >= 0.f && spec_broaden_radius_f(s) <= (float)SPEC_BROADEN_RMAX; }
// (the entry point has checked the range: the conversion is exact)
__device__ __forceinline__ int spec_broaden_radius(float s) { return (int)spec_broaden_radius_f(s); }
__device__ __forceinline__ float spec_broaden_sigma(uint32_t b, uint32_t k1, uint32_t k2, float s) {
#pragma clang fp contract(off)
    return spec_row_unit(b, SPEC_BROADEN_OFF, k1, k2) * s;        // the only rounding
}
__device__ __forceinline__ float spec_broaden_q(float sigma) {
#pragma clang fp contract(off)
    const float s2 = sigma * sigma;                               // rounds
    return 1.0f / (2.f * s2);                                     // 2 s2 is exact; the (correctly rounded) division rounds
}
__device__ __forceinline__ float spec_broaden_weight(int j, float q) {
#pragma clang fp contract(off)
    const float t = (float)(j * j) * q;                           // j j <= 4096 is exact; the product rounds
    return j == 0 ? 1.f : expf(-t);
}

// ---- normalisation augmentation (config keys `spec_gain`, `spec_tilt`): row b scaled by g_b and tilted by a linear
// ramp c_b r_l, between the shift and the noise ----
// The body above with one more stage, present at compile time only in the instances of SpecAug3Args (NORM): resolution,
// axis, NORMALISATION, detector.  Row b draws twice more, at SPEC_GAIN_OFF + b and SPEC_TILT_OFF + b:
//   g_b = 1 + (2 u_b - 1) a      2 u - 1 exact; the product rounds; the sum rounds
//   c_b = (2 u'_b - 1) t         the product rounds
//   r_l = float(2 l - (L - 1)) / float(L - 1)     the integer is exact (|.| < 2^13); the division rounds; L == 1: r = 0
//   v   = g_b x;  p = c_b r_l;  v = v + p          three roundings, x the shifted sample
// all compiled with contraction off (a product fused into the sum would skip its rounding), so a fp32 emulation on the
// host reproduces the stage bit for bit.  a == 0 gives g_b = 1 and v = x, t == 0 gives p = +-0 and v + p = v (up to
// the sign of a zero, which is why the stage is not run with a = t = 0 for SpecAug2Args): no case is skipped.  g_b, c_b
// are one value per row, computed by every thread from the hash (two scalars: nothing to stage, no barrier); r_l is
// computed where it is used.  Stage 3's quad-per-thread layout has a lane read LDS words 4 t + k (32-bit reads at a
// stride of four words: four lanes share a bank, which a row of a few hundred samples does not feel; a lane-consecutive
// layout would draw every Philox block four times).  The noise term stays in the default contraction context.
struct SpecAug3Args {
    static constexpr bool NORM = true;
    const float* spec; const long* idx; const int* cursor; const unsigned long long* rng_state; int B; int L;
    float max_sigma; float max_shift; float max_gain; float max_tilt; float spec_noise; long noise_goff; float* spec_out;
};
__device__ __forceinline__ float spec_norm_gain(uint32_t b, uint32_t k1, uint32_t k2, float a) {
#pragma clang fp contract(off)
    const float d = spec_row_draw(b, SPEC_GAIN_OFF, k1, k2, a);
    return 1.f + d;                                               // rounds
}
__device__ __forceinline__ float spec_norm_ramp(int l, int L) {
#pragma clang fp contract(off)
    return L == 1 ? 0.f : (float)(2 * l - (L - 1)) / (float)(L - 1);      // (the correctly rounded division rounds)
}
__device__ __forceinline__ float spec_norm_apply(float x, float g, float c, float r) {
#pragma clang fp contract(off)
    const float v = g * x, p = c * r;                             // each rounds
    return v + p;                                                 // rounds
}

// the row-staged body: Args is SpecAug2Args or SpecAug3Args
template <typename Args>
__device__ __forceinline__ void spec_staged_body(const Args& a) {
    extern __shared__ float s_aug[];
    const int L = a.L, R = spec_broaden_radius(a.max_sigma), tid = threadIdx.x;
    float* s_in = s_aug;                                          // L + 2 R of the L + 2 RMAX
    float* s_w = s_aug + L + 2 * SPEC_BROADEN_RMAX;               // 2 R + 1 of the 2 RMAX + 4
    float* s_g = s_w + 2 * SPEC_BROADEN_RMAX + 4;                 // L
    const unsigned long long ctr = a.rng_state[0], seed = a.rng_state[1];
    const uint32_t k1 = reinterpret_cast<const unsigned*>(a.rng_state + 2)[0];
    const uint32_t k2 = reinterpret_cast<const unsigned*>(a.rng_state + 2)[1];
    const long* idx = a.idx + (a.cursor[0] - a.B);
    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const float* row = a.spec + (size_t)idx[b] * L;
        const float sigma = spec_broaden_sigma((uint32_t)b, k1, k2, a.max_sigma);
        if (sigma == 0.f) {                                       // (the whole workgroup agrees: one row, one sigma)
            for (int l = tid; l < L; l += 256) s_g[l] = row[l];
        } else {
            for (int i = tid; i < L + 2 * R; i += 256) s_in[i] = row[min(max(i - R, 0), L - 1)];
            if (tid <= 2 * R) s_w[tid] = spec_broaden_weight(tid - R, spec_broaden_q(sigma));
            __syncthreads();
            for (int l = tid; l < L; l += 256) {
                float acc = 0.f, wsum = 0.f;
                for (int j = 0; j <= 2 * R; ++j) {
                    const float w = s_w[j];
                    wsum += w;
                    acc = fmaf(w, s_in[l + j], acc);
                }
                s_g[l] = acc / wsum;
            }
        }
        __syncthreads();
        const float delta = spec_shift_delta((uint32_t)b, k1, k2, a.max_shift);
        float gain = 1.f, tilt = 0.f;
        if constexpr (Args::NORM) {
            gain = spec_norm_gain((uint32_t)b, k1, k2, a.max_gain);
            tilt = spec_row_draw((uint32_t)b, SPEC_TILT_OFF, k1, k2, a.max_tilt);
        }
        const long e0 = a.noise_goff + (long)b * L;               // the row's first element in the Gaussian numbering
        float* out = a.spec_out + (size_t)b * L;
        for (long q4 = (e0 >> 2) + tid; q4 * 4 < e0 + L; q4 += 256) {
            float z[4] = {0.f, 0.f, 0.f, 0.f};
            if (a.spec_noise != 0.f) normal4(q4, ctr, seed, z);
            const long l0 = q4 * 4 - e0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long l = l0 + k;
                if (l < 0 || l >= L) continue;
                float v = spec_shift_sample(s_g, (int)l, L, delta);
                if constexpr (Args::NORM) v = spec_norm_apply(v, gain, tilt, spec_norm_ramp((int)l, L));
                if (a.spec_noise != 0.f) v += z[k] * a.spec_noise;
                out[l] = v;
            }
        }
        __syncthreads();                                          // (the next row overwrites the LDS image)
    }
}
__global__ __launch_bounds__(256) void spec_augment2_kernel(SpecAug2Args a) { spec_staged_body(a); }
__global__ __launch_bounds__(256) void spec_augment2_kernel_m(const SpecAug2Args* t) {
    const SpecAug2Args a = t[blockIdx.z];
    spec_staged_body(a);
}
__global__ __launch_bounds__(256) void spec_augment3_kernel(SpecAug3Args a) { spec_staged_body(a); }
__global__ __launch_bounds__(256) void spec_augment3_kernel_m(const SpecAug3Args* t) {
    const SpecAug3Args a = t[blockIdx.z];
    spec_staged_body(a);
}

// what the three entry points refuse alike (max_sigma = 0 from the one that does not broaden)
bool spec_args_ok(const float* spec, const long* idx, const int* cursor, const unsigned long long* rng_state,
                  const float* spec_out, int B, double max_sigma, double max_shift, double spec_noise) {
    const float sg = (float)max_sigma, s = (float)max_shift, sn = (float)spec_noise;
    return spec && idx && cursor && rng_state && spec_out && B >= 1
        && max_shift >= 0.0 && s < INFINITY && sn == sn                // (false for a NaN or Inf max_shift)
        && max_sigma >= 0.0 && sg < INFINITY                           // (likewise)
        && spec_broaden_radius_ok(sg);                                 // (a float comparison: 1e10 or 3e38 is refused here)
}

// the launch of a row-staged kernel and its batched twin: one workgroup per row, at most 1024, above which the kernel
// grid-strides over rows; the LDS image is sized for the largest radius whatever this plane's is (one geometry per
// shape: the trials of a batch agree)
template <auto SINGLE, auto MULTI, typename Args>
int spec_staged_launch(const Args& a, hipStream_t stream) {
    const size_t lds = sizeof(float) * (size_t)(2 * a.L + 4 * SPEC_BROADEN_RMAX + 4);
    // the image of the longest row is 65.0 KiB: the runtime wants to be told about more than 64 KiB, once per kernel
    // (the first call does it, for the largest L, whatever its own L is: no runtime call per launch or inside a capture
    // after that)
    static const hipError_t lds_limit = [] {
        const int most = (int)(sizeof(float) * (2 * SPEC_BROADEN_LMAX + 4 * SPEC_BROADEN_RMAX + 4));
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(SINGLE), hipFuncAttributeMaxDynamicSharedMemorySize, most);
        if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(MULTI), hipFuncAttributeMaxDynamicSharedMemorySize, most);
        return e;
    }();
    if (lds_limit != hipSuccess) return (int)lds_limit;
    raae::launch(SINGLE, MULTI, dim3(a.B < 1024 ? a.B : 1024), dim3(256), lds, stream, a);
    RAAE_LAUNCH_RET();
}

}  // namespace

extern "C" int raae_spec_augment(const float* spec, const long* idx, const int* cursor, const unsigned long long* rng_state,
                                 int B, int L, double max_shift, double spec_noise, long noise_goff, float* spec_out,
                                 void* stream) {
    RAAE_CHECK_ARG(spec_args_ok(spec, idx, cursor, rng_state, spec_out, B, 0.0, max_shift, spec_noise) && L >= 2);
    RAAE_CHECK_ARG((noise_goff & 3) == 0 && noise_goff >= 0);
    const SpecAugArgs a = {spec, idx, cursor, rng_state, B, L, (float)max_shift, (float)spec_noise, noise_goff, spec_out};
    // sized by B * L, four elements per thread whichever body runs (one geometry per shape: trials of a batch agree),
    // at most 1024 workgroups, above which the kernel grid-strides
    long g = (((long)B * L + 3) / 4 + 255) / 256;
    if (g > 1024) g = 1024;
    raae::launch(spec_augment_kernel, spec_augment_kernel_m, dim3((int)g), dim3(256), 0, (hipStream_t)stream, a);
    RAAE_LAUNCH_RET();
}

extern "C" int raae_spec_augment2(const float* spec, const long* idx, const int* cursor, const unsigned long long* rng_state,
                                  int B, int L, double max_sigma, double max_shift, double spec_noise, long noise_goff,
                                  float* spec_out, void* stream) {
    RAAE_CHECK_ARG(spec_args_ok(spec, idx, cursor, rng_state, spec_out, B, max_sigma, max_shift, spec_noise));
    RAAE_CHECK_ARG(L >= 2 && L <= SPEC_BROADEN_LMAX && (noise_goff & 3) == 0 && noise_goff >= 0);
    const SpecAug2Args a = {spec, idx, cursor, rng_state, B, L, (float)max_sigma, (float)max_shift, (float)spec_noise,
                            noise_goff, spec_out};
    return spec_staged_launch<spec_augment2_kernel, spec_augment2_kernel_m>(a, (hipStream_t)stream);
}

extern "C" int raae_spec_augment3(const float* spec, const long* idx, const int* cursor, const unsigned long long* rng_state,
                                  int B, int L, double max_sigma, double max_shift, double max_gain, double max_tilt,
                                  double spec_noise, long noise_goff, float* spec_out, void* stream) {
    RAAE_CHECK_ARG(spec_args_ok(spec, idx, cursor, rng_state, spec_out, B, max_sigma, max_shift, spec_noise));
    // (B <= 2^29: the gain draws at 0xA0000000 + b end below the broaden draws, the tilt draws at 0xE0000000 + b below 2^32)
    RAAE_CHECK_ARG(B <= SPEC_NORM_BMAX && L >= 1 && L <= SPEC_BROADEN_LMAX);
    const float gn = (float)max_gain, tl = (float)max_tilt;
    RAAE_CHECK_ARG(max_gain >= 0.0 && gn < 1.f);                       // (as the kernel sees it: 1 - 1e-12 rounds to 1; false for a NaN)
    RAAE_CHECK_ARG(max_tilt >= 0.0 && tl < INFINITY);                  // (false for a NaN or Inf, and for a finite double beyond fp32)
    RAAE_CHECK_ARG(noise_goff >= 0);                                   // (any alignment: the body takes whole quads of the numbering)
    const SpecAug3Args a = {spec, idx, cursor, rng_state, B, L, (float)max_sigma, (float)max_shift, gn, tl, (float)spec_noise,
                            noise_goff, spec_out};
    return spec_staged_launch<spec_augment3_kernel, spec_augment3_kernel_m>(a, (hipStream_t)stream);
}
