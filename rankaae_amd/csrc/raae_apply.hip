// Applying trained models to spectra they were not trained on (rankaae_amd/apply.py): the two per-row pieces of device
// work next to the eval forwards, which are the report step's (rankaae_amd/report.py).
//   raae_resample_rows    foreign rows [n][Ls] onto the model's energy grid [n][L], by a host-made plan (idx, w)
//   raae_ensemble_stats   the J models' styles and reconstructions of a chunk of rows -> mean and spread over the
//                         models of every style and of every descriptor the calibrations predict, the per-model and the
//                         mean reconstruction error
// Both have the one-argument-block form of raae_common.h (raae::launch), no atomics and a fixed summation order: a second
// call on the same inputs writes the same bytes.
#include "raae_common.h"

namespace {

// ---- resampling ------------------------------------------------------------------------------------------------------
// out[r][l] = a + w[l] (b - a),  a = src[r][idx[l]],  b = src[r][idx[l] + 1].
// The plan is per column, not per row: a thread keeps its column's (idx, w) in registers and walks kResRows rows, so the
// plan is read once per kResRows rows.  Grid (ceil(L / 256), ceil(n / kResRows)), capped in y, above which the workgroups
// stride over row groups.  The reads are a monotone gather straight from global memory: neighbouring lanes read
// neighbouring or equal addresses, a and b of one lane are adjacent words, so every cache line of the row's used range
// comes from HBM once and is then served by the vector cache.  A row is up to 256 KiB -- more than a workgroup's LDS --
// and where Ls >> L most of it is never read, so staging the row would move more bytes, not fewer.  (Not measured.)
// Exactness: w == 0 returns a and w == 1 returns b through a select, not through arithmetic (fmaf(0, b - a, a) would
// turn an infinite b - a into NaN and fmaf(1, b - a, a) rounds b - a first); every other w is one fmaf.
constexpr int kResRows = 4;
struct ResampleArgs {
    const float* src; const int* idx; const float* w; float* out;
    int n, Ls, lds, L, ldo;
};
__device__ __forceinline__ void resample_rows_body(const ResampleArgs& a) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= a.L) return;
    // (the host contract is 0 <= idx <= Ls - 2; a plan that breaks it must not read outside the row)
    const int i0 = min(max(a.idx[l], 0), a.Ls - 2);
    const float w = a.w[l];
    for (long r0 = (long)blockIdx.y * kResRows; r0 < a.n; r0 += (long)gridDim.y * kResRows) {
#pragma unroll
        for (int u = 0; u < kResRows; ++u) {
            const long r = r0 + u;
            if (r >= a.n) break;
            const float* row = a.src + (size_t)r * a.lds;
            const float va = row[i0], vb = row[i0 + 1];
            const float v = fmaf(w, vb - va, va);
            a.out[(size_t)r * a.ldo + l] = w == 0.f ? va : (w == 1.f ? vb : v);
        }
    }
}

// ---- ensemble statistics ---------------------------------------------------------------------------------------------
// One workgroup (4 waves) per row, striding over rows above 65535.  The only part with bandwidth in it is the error
// pass, J L floats per row: wave w takes models w, w + 4, ..., its 64 lanes stride over the L points (coalesced 256-byte
// reads of `recon`, the row of `spec` stays in the vector cache), sum |recon - spec| in double (the difference in fp32,
// as raae_select_scores' error pass and scikit-learn on fp32 arrays form it) and meet in an xor tree.  The J errors go
// through LDS to the thread that averages them, in model order.  Behind the barrier thread c < k forms style c's mean
// and sample standard deviation over the models, thread 64 + i descriptor i's over the models with a fit for it, each
// in two passes (mean, then squared deviations) in double and in model order, re-reading its J inputs instead of keeping
// them (a runtime-indexed private array would live in scratch memory).
struct EnsembleArgs {
    const float* const* z;          // [J] -> [n][k]
    const float* spec;              // [n][L]
    const float* const* recon;      // [J] -> [n][L]
    const double* calib;            // [J][n_aux][4]
    double* z_mean; double* z_std; double* d_mean; double* d_std; double* d_used; double* mae; double* mae_mean;
    int J, n, k, n_aux, L;
    long ld_mae;
};
__device__ __forceinline__ double ens_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
// the descriptor a calibration row {kind, p0, p1, 0} reads off a style (kind != 0)
__device__ __forceinline__ double ens_predict(const double* c, double z) {
    return c[0] == 1.0 ? (z - c[2]) / c[1] : 4.0 + (double)(z > c[1]) + (double)(z > c[2]);
}
__device__ __forceinline__ void ensemble_stats_body(const EnsembleArgs& a) {
    __shared__ double sh_mae[64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int row = blockIdx.x; row < a.n; row += gridDim.x) {
        const float* x = a.spec + (size_t)row * a.L;
        for (int j = wave; j < a.J; j += 4) {
            const float* y = a.recon[j] + (size_t)row * a.L;
            double s = 0.0;
#pragma unroll 4
            for (int l = lane; l < a.L; l += 64) s += (double)fabsf(y[l] - x[l]);
            s = raae::wave_sum(s);
            if (lane == 0) {
                const double m = s / (double)a.L;
                a.mae[(size_t)j * a.ld_mae + row] = m;
                sh_mae[j] = m;
            }
        }
        __syncthreads();
        if (tid < a.k) {
            double s = 0.0;
            for (int j = 0; j < a.J; ++j) s += (double)a.z[j][(size_t)row * a.k + tid];
            const double mean = s / (double)a.J;
            double q = 0.0;
            for (int j = 0; j < a.J; ++j) { const double d = (double)a.z[j][(size_t)row * a.k + tid] - mean; q += d * d; }
            a.z_mean[(size_t)row * a.k + tid] = mean;
            a.z_std[(size_t)row * a.k + tid] = a.J > 1 ? sqrt(q / (double)(a.J - 1)) : 0.0;
        } else if (tid >= 64 && tid < 64 + a.n_aux) {
            const int i = tid - 64;
            int used = 0;
            double s = 0.0;
            if (i < a.k) {                   // descriptor i is read off style i: none without that style
                for (int j = 0; j < a.J; ++j) {
                    const double* c = a.calib + ((size_t)j * a.n_aux + i) * 4;
                    if (c[0] == 0.0) continue;
                    ++used;
                    s += ens_predict(c, (double)a.z[j][(size_t)row * a.k + i]);
                }
            }
            double mean = ens_nan(), sd = ens_nan();
            if (used > 0) {
                mean = s / (double)used;
                double q = 0.0;
                for (int j = 0; j < a.J; ++j) {
                    const double* c = a.calib + ((size_t)j * a.n_aux + i) * 4;
                    if (c[0] == 0.0) continue;
                    const double d = ens_predict(c, (double)a.z[j][(size_t)row * a.k + i]) - mean;
                    q += d * d;
                }
                sd = used > 1 ? sqrt(q / (double)(used - 1)) : 0.0;
            }
            a.d_mean[(size_t)row * a.n_aux + i] = mean;
            a.d_std[(size_t)row * a.n_aux + i] = sd;
            if (row == 0) a.d_used[i] = (double)used;
        } else if (tid == 128) {
            double s = 0.0;
            for (int j = 0; j < a.J; ++j) s += sh_mae[j];
            a.mae_mean[row] = s / (double)a.J;
        }
        __syncthreads();                     // (the next row overwrites sh_mae)
    }
}

#define APPLY_KERNEL_PAIR(NAME, ARGS)                                                                            \
    __global__ __launch_bounds__(256) void NAME##_kernel(ARGS a) { NAME##_body(a); }                             \
    __global__ __launch_bounds__(256) void NAME##_kernel_m(const ARGS* t) {  /* raae::launch's second form */    \
        const ARGS a = t[blockIdx.z];                                                                            \
        NAME##_body(a);                                                                                          \
    }
APPLY_KERNEL_PAIR(resample_rows, ResampleArgs)
APPLY_KERNEL_PAIR(ensemble_stats, EnsembleArgs)

}  // namespace

extern "C" int raae_resample_rows(const float* src, int n, int Ls, int ld_src, const int* idx, const float* w, int L,
                                  float* out, int ld_out, void* stream) {
    RAAE_CHECK_ARG(src && idx && w && out);
    RAAE_CHECK_ARG(n >= 1 && Ls >= 2 && Ls <= 65536 && L >= 1 && L <= 4096 && ld_src >= Ls && ld_out >= L);
    const ResampleArgs a = {src, idx, w, out, n, Ls, ld_src, L, ld_out};
    const int gy = raae::cdiv(n, kResRows);
    raae::launch(resample_rows_kernel, resample_rows_kernel_m, dim3(raae::cdiv(L, 256), gy < 65535 ? gy : 65535), dim3(256),
                 0, (hipStream_t)stream, a);
    RAAE_LAUNCH_RET();
}

extern "C" int raae_ensemble_stats(const float* const* z, const float* spec, const float* const* recon, const double* calib,
                                   int J, int n, int k, int n_aux, int L, double* z_mean, double* z_std, double* d_mean,
                                   double* d_std, double* d_used, double* mae, long ld_mae, double* mae_mean, void* stream) {
    RAAE_CHECK_ARG(z && spec && recon && z_mean && z_std && mae && mae_mean);
    RAAE_CHECK_ARG(J >= 1 && J <= 64 && n >= 1 && k >= 1 && k <= 16 && n_aux >= 0 && n_aux <= 16 && L >= 1 && ld_mae >= n);
    RAAE_CHECK_ARG(n_aux == 0 || (calib && d_mean && d_std && d_used));
    const EnsembleArgs a = {z, spec, recon, calib, z_mean, z_std, d_mean, d_std, d_used, mae, mae_mean, J, n, k, n_aux, L, ld_mae};
    raae::launch(ensemble_stats_kernel, ensemble_stats_kernel_m, dim3(n < 65535 ? n : 65535), dim3(256), 0,
                 (hipStream_t)stream, a);
    RAAE_LAUNCH_RET();
}
