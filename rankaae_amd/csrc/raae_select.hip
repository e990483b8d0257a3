// Model-selection scores of a trained model on the device: what the reference's report step computes per
// `training/job_*/final.pt` on a host copy with scipy / scikit-learn (sc/report/analysis.py:394-450, evaluate_model),
// unrounded.  Inputs stay in HBM: the validation styles [n, k] (fp32), the descriptors [n, n_aux] (float64, as the
// reference sees them), the spectra in and out [n, L] (fp32).  Output: one block of doubles (RAAE_SEL_* in the header).
//
// Four launches, each with the one-model-per-grid-plane form of raae_common.h (raae::launch), so J models of one
// architecture are scored by one gridDim.z = J sequence:
//   sel_rank_kernel   average ranks of every style column and every descriptor column but column 1, by counting -- the
//                     scheme of style_rank_kernel (raae_metrics.hip), here on doubles because the descriptors are doubles
//   sel_mae_kernel    mean absolute error of each spectrum, one wave per row
//   sel_sweep_kernel  coordination-number sweeps: workgroup (t, s) counts, over the n rows, the binary confusion of
//                     `style_1 < th_t` against `class < 1` (s = 0) or of `style_1 > th_t` against `class > 1` (s = 1)
//   sel_stat_kernel   workgroup 0: mean / population std of the n MAEs; workgroup 1: max_i |rho(style_i, style_last)|;
//                     workgroup 2 + i: descriptor i -- Spearman, linregress, degree-2 fit (i != 1), or the two arg-max
//                     thresholds, the 3x3 confusion matrix and the support-weighted F1 (i == 1)
// Counts are integers; every floating sum is double, strided per thread, then a wave64 shuffle tree, then the four
// wave totals in order: no atomics, so a replay is bitwise repeatable.  Inputs are taken to be finite (the reference
// masks NaN rows out before its statistics; a model that produces NaN styles has no place in a ranking).
//
// raae_select_scores_masked: a descriptor cell that is not finite (NaN) is a missing label.  The same four bodies are
// instantiated a second time on SelArgsM; there every per-descriptor score of descriptor i is formed over S_i, the rows
// whose cell i is labelled (m_i of them; fewer than 3: the slice is zeros), which takes the average ranks of style i
// among the rows of S_i (rank_zs, n_aux more columns of the rank kernel).  The head of the block uses all rows and is
// bitwise what raae_select_scores writes.
#include "raae_common.h"

namespace {

constexpr int kTile = 2048;
// degree-2 fit: the share of sum u^4 below which the variance of u^2 counts as none (rounding leaves ~1e-15 of it where
// the descriptor has two distinct values; three values, one of them on a single row of 2^20, still leave 1e-6)
constexpr double kSelRankTol = 1e-10;

struct SelArgs {
    const float* z; const double* aux; const float* sin; const float* sout; const double* th;
    double* rank_z; double* rank_d; double* mae; int* sweep; double* out;
    int n, k, n_aux, L, n_th;
};
struct SelArgsM : SelArgs { double* rank_zs; };      // [n_aux][n]: ranks of style i among the rows labelled for descriptor i
template <class A> constexpr bool kMasked = false;
template <> constexpr bool kMasked<SelArgsM> = true;
// the exponent bits, not x == x: the test must hold under -ffinite-math-only too
__device__ __forceinline__ bool labelled(double x) { return (__double2hiint(x) & 0x7ff00000) != 0x7ff00000; }

// ---- block-wide reductions (256 threads = 4 waves); the result is valid in every thread --------------------------------
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* sh) {       // sh: >= 4 NV doubles
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int u = 0; u < NV; ++u) v[u] = raae::wave_sum(v[u]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int u = 0; u < NV; ++u) sh[u * 4 + w] = v[u];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NV; ++u) v[u] = ((sh[u * 4] + sh[u * 4 + 1]) + sh[u * 4 + 2]) + sh[u * 4 + 3];
}
template <int NV>
__device__ __forceinline__ void block_sum(int (&v)[NV], int* sh) {              // sh: >= 4 NV ints
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int u = 0; u < NV; ++u) v[u] = raae::wave_sum(v[u]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int u = 0; u < NV; ++u) sh[u * 4 + w] = v[u];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NV; ++u) v[u] = sh[u * 4] + sh[u * 4 + 1] + sh[u * 4 + 2] + sh[u * 4 + 3];
}
__device__ __forceinline__ double block_min(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmin(fmin(sh[0], sh[1]), fmin(sh[2], sh[3]));
}

// ---- ranks: grid (ceil(n / 256), k + n_aux); column c < k is style c, column k + i is descriptor i ----------------------
template <class A>
__device__ __forceinline__ void sel_rank_body(const A& a) {
    __shared__ __attribute__((aligned(16))) double tile[kTile];
    int c = blockIdx.y;
    const int tid = threadIdx.x, n = a.n;
    // masked form, columns k + n_aux + i: style i among the rows labelled for descriptor i
    const bool sub = kMasked<A> && c >= a.k + a.n_aux;
    const int dsub = c - a.k - a.n_aux;
    if (sub) c = dsub;
    if (sub ? dsub == 1 : c == a.k + 1) return;          // the coordination number is classified, never ranked
    const bool st = c < a.k;
    const int ld = st ? a.k : a.n_aux, col = st ? c : c - a.k;
    auto at = [&](int j) -> double {
        const double v = st ? (double)a.z[(size_t)j * ld + col] : a.aux[(size_t)j * ld + col];
        if constexpr (kMasked<A>) {
            // an unlabelled row stands at +infinity: below no one, equal to no labelled value.  (Its own rank is never read.)
            const double lab = sub ? a.aux[(size_t)j * a.n_aux + dsub] : (st ? 0.0 : v);
            if (!labelled(lab)) return __builtin_huge_val();
        }
        return v;
    };
    const int i = blockIdx.x * 256 + tid;
    const double xi = i < n ? at(i) : 0.0;
    int less = 0, eq = 0;
    for (int j0 = 0; j0 < n; j0 += kTile) {
        const int m = min(kTile, n - j0);
        __syncthreads();
        for (int t = tid; t < m; t += 256) tile[t] = at(j0 + t);
        __syncthreads();
        int jj = 0;
        for (; jj + 2 <= m; jj += 2) {
            const double2 v = *reinterpret_cast<const double2*>(tile + jj);
            less += (v.x < xi) + (v.y < xi);
            eq += (v.x == xi) + (v.y == xi);
        }
        for (; jj < m; ++jj) {
            const double v = tile[jj];
            less += v < xi;
            eq += v == xi;
        }
    }
    if (i < n) {
        double* rank = st ? a.rank_z + (size_t)c * n : a.rank_d + (size_t)col * n;
        if constexpr (kMasked<A>) { if (sub) rank = a.rank_zs + (size_t)dsub * n; }
        rank[i] = (double)less + 0.5 * (double)(eq + 1);
    }
}

// ---- MAE of each spectrum: grid (ceil(n / 4)), one wave per row (sklearn: mean |y_pred - y_true|, fp32 difference) -----
template <class A>
__device__ __forceinline__ void sel_mae_body(const A& a) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= a.n) return;
    const float* x = a.sin + (size_t)row * a.L;
    const float* y = a.sout + (size_t)row * a.L;
    double s = 0.0;
    for (int l = lane; l < a.L; l += 64) s += (double)fabsf(y[l] - x[l]);
    s = raae::wave_sum(s);
    if (lane == 0) a.mae[row] = s / (double)a.L;
}

// class of a coordination number as the reference forms it: (cn - 4).astype(int), i.e. truncation toward zero
__device__ __forceinline__ double cn_class(double cn) { return trunc(cn - 4.0); }

// ---- threshold sweeps: grid (n_th, 2).  sweep[s][t] = {2 TP, 2 TP + FP + FN}: F1 is their quotient, 0 where the
// denominator is 0 (zero_division=0) --------------------------------------------------------------------------------------
template <class A>
__device__ __forceinline__ void sel_sweep_body(const A& a) {
    __shared__ int sh[12];
    const int t = blockIdx.x, s = blockIdx.y, n = a.n;
    const double th = a.th[t];
    int c[3] = {0, 0, 0};                                // TP, predicted positives, actual positives
    for (int i = threadIdx.x; i < n; i += 256) {
        const double z = (double)a.z[(size_t)i * a.k + 1];        // numpy promotes the fp32 style to the float64 threshold
        if constexpr (kMasked<A>) { if (!labelled(a.aux[(size_t)i * a.n_aux + 1])) continue; }
        const double cls = cn_class(a.aux[(size_t)i * a.n_aux + 1]);
        const int p = s == 0 ? z < th : z > th;
        const int q = s == 0 ? cls < 1.0 : cls > 1.0;
        c[0] += p & q; c[1] += p; c[2] += q;
    }
    block_sum<3>(c, sh);
    if (threadIdx.x == 0) {
        int* o = a.sweep + ((size_t)s * a.n_th + t) * 2;
        o[0] = 2 * c[0];
        o[1] = c[1] + c[2];
    }
}

// first maximum of sweep s over the thresholds: fractions compared exactly by cross-multiplication (num <= 2 n,
// den <= 2 n: the products fit 64 bits), ties to the lower index -- numpy.argmax of the host's list of quotients
__device__ __forceinline__ int sweep_argmax(const SelArgs& a, int s, int* sh) {
    const int tid = threadIdx.x;
    long long bn = 0, bd = 1;
    int bi = 0x7fffffff;
    for (int t = tid; t < a.n_th; t += 256) {
        const int* o = a.sweep + ((size_t)s * a.n_th + t) * 2;
        const long long num = o[1] > 0 ? o[0] : 0, den = o[1] > 0 ? o[1] : 1;
        if (bi == 0x7fffffff || num * bd > bn * den) { bn = num; bd = den; bi = t; }
    }
    __syncthreads();
    sh[tid] = (int)bn; sh[256 + tid] = (int)bd; sh[512 + tid] = bi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            const long long n0 = sh[tid], d0 = sh[256 + tid], n1 = sh[tid + o], d1 = sh[256 + tid + o];
            const int i0 = sh[512 + tid], i1 = sh[512 + tid + o];
            const bool take = i1 != 0x7fffffff && (i0 == 0x7fffffff || n1 * d0 > n0 * d1 || (n1 * d0 == n0 * d1 && i1 < i0));
            if (take) { sh[tid] = (int)n1; sh[256 + tid] = (int)d1; sh[512 + tid] = i1; }
        }
        __syncthreads();
    }
    const int best = sh[512];
    __syncthreads();
    return best;
}

template <class A>
__device__ __forceinline__ void sel_stat_body(const A& a) {
    __shared__ double shd[13 * 4];
    __shared__ int shi[3 * 256];
    const int tid = threadIdx.x, w = blockIdx.x, n = a.n, k = a.k;
    double dn = (double)n;
    if (w == 0) {
        // Reconstruct Err: np.mean / np.std (population) of the per-spectrum MAEs
        double s[1] = {0.0};
        for (int i = tid; i < n; i += 256) s[0] += a.mae[i];
        block_sum<1>(s, shd);
        const double mean = s[0] / dn;
        double q[1] = {0.0};
        for (int i = tid; i < n; i += 256) { const double d = a.mae[i] - mean; q[0] += d * d; }
        block_sum<1>(q, shd);
        if (tid == 0) { a.out[0] = mean; a.out[1] = sqrt(q[0] / dn); a.out[3] = 0.0; }
        return;
    }
    double rmean = 0.5 * (dn + 1.0);                     // average ranks always sum to n (n + 1) / 2
    if (w == 1) {
        // Inter-style Corr: max_i |spearman(style_i, style_{k-1})|, i < k - 1 (analysis.py:321-325)
        const double* rl = a.rank_z + (size_t)(k - 1) * n;
        double best = 0.0;
        for (int c = 0; c < k - 1; ++c) {
            const double* rc = a.rank_z + (size_t)c * n;
            double t[3] = {0.0, 0.0, 0.0};
            for (int i = tid; i < n; i += 256) {
                const double u = rc[i] - rmean, v = rl[i] - rmean;
                t[0] += u * u; t[1] += v * v; t[2] += u * v;
            }
            block_sum<3>(t, shd);
            double r = t[2] / sqrt(t[0]) / sqrt(t[1]);
            r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
            best = fmax(best, fabs(r));
        }
        if (tid == 0) a.out[2] = best;
        return;
    }
    const int d = w - 2;
    double* o = a.out + RAAE_SEL_HEAD + (size_t)RAAE_SEL_STRIDE * d;
    // masked form: row i takes part iff its cell of descriptor d is labelled; dn becomes the number of such rows
    auto V = [&](int i) -> bool {
        if constexpr (kMasked<A>) return labelled(a.aux[(size_t)i * a.n_aux + d]);
        return true;
    };
    if constexpr (kMasked<A>) {
        int m[1] = {0};
        for (int i = tid; i < n; i += 256) m[0] += V(i);
        block_sum<1>(m, shi);
        __syncthreads();                                 // shi is reused below
        if (m[0] < 3) {                                  // uniform: no score from fewer than three labelled rows
            for (int u = tid; u < RAAE_SEL_STRIDE; u += 256) o[u] = 0.0;
            return;
        }
        dn = (double)m[0];
        rmean = 0.5 * (dn + 1.0);
    }
    if (d == 1) {
        // coordination number (get_confusion_matrix, analysis.py:234-269)
        for (int u = tid; u < RAAE_SEL_STRIDE; u += 256) o[u] = 0.0;
        // more than three distinct classes: the reference returns None.  Walk up the distinct values, smallest first.
        const double inf = __builtin_huge_val();
        double floor_ = -inf;
        int distinct = 0;
        for (int pass = 0; pass < 4; ++pass) {
            double m = inf;
            for (int i = tid; i < n; i += 256) {
                if (!V(i)) continue;
                const double c = cn_class(a.aux[(size_t)i * a.n_aux + 1]);
                if (c > floor_) m = fmin(m, c);
            }
            m = block_min(m, shd);
            if (m == inf) break;
            ++distinct;
            floor_ = m;
        }
        if (distinct > 3) return;                        // o[0] = 0: no result
        const int i45 = sweep_argmax(a, 0, shi), i56 = sweep_argmax(a, 1, shi);
        const double t45 = a.th[i45], t56 = a.th[i56];
        // cm[true class 0..2][predicted 0..2], and how often each class is predicted at all (rows whose true class
        // lies outside 0..2 still count as false positives of what they are predicted as)
        int c[12];
#pragma unroll
        for (int u = 0; u < 12; ++u) c[u] = 0;
        for (int i = tid; i < n; i += 256) {
            if (!V(i)) continue;
            const double z = (double)a.z[(size_t)i * k + 1];
            const double cls = cn_class(a.aux[(size_t)i * a.n_aux + 1]);
            const int p = (z > t45) + (z > t56);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                c[9 + q] += p == q;
#pragma unroll
                for (int r = 0; r < 3; ++r) c[r * 3 + q] += (cls == (double)r) & (p == q);
            }
        }
        {
            int c0[3] = {c[0], c[1], c[2]}, c1[3] = {c[3], c[4], c[5]}, c2[3] = {c[6], c[7], c[8]}, c3[3] = {c[9], c[10], c[11]};
            block_sum<3>(c0, shi); block_sum<3>(c1, shi); block_sum<3>(c2, shi); block_sum<3>(c3, shi);
#pragma unroll
            for (int u = 0; u < 3; ++u) { c[u] = c0[u]; c[3 + u] = c1[u]; c[6 + u] = c2[u]; c[9 + u] = c3[u]; }
        }
        if (tid == 0) {
            // f1_score(average="weighted"): sum_l support_l F1_l / sum_l support_l over the labels in ascending order;
            // a label outside 0..2 is never predicted, its F1 is 0 and only its support counts: the divisor is n
            double acc = 0.0;
            for (int l = 0; l < 3; ++l) {
                const int support = c[l * 3] + c[l * 3 + 1] + c[l * 3 + 2], den = support + c[9 + l];
                const double f = den > 0 ? (double)(2 * c[l * 3 + l]) / (double)den : 0.0;
                acc += f * (double)support;
            }
            o[0] = 1.0; o[1] = acc / dn; o[2] = (double)i45; o[3] = (double)i56; o[4] = t45; o[5] = t56;
            for (int u = 0; u < 9; ++u) o[6 + u] = (double)c[u];
        }
        return;
    }
    // get_descriptor_style_correlation as evaluate_model calls it: x = descriptor, y = style (analysis.py:445)
    const double* rx = a.rank_d + (size_t)d * n;
    const double* ry = a.rank_z + (size_t)d * n;
    if constexpr (kMasked<A>) ry = a.rank_zs + (size_t)d * n;
    auto X = [&](int i) -> double { return a.aux[(size_t)i * a.n_aux + d]; };
    auto Y = [&](int i) -> double { return (double)a.z[(size_t)i * k + d]; };
    double s[2] = {0.0, 0.0};
    const double inf = __builtin_huge_val();
    double lo = inf, nhi = inf;
    for (int i = tid; i < n; i += 256) {
        if (!V(i)) continue;
        const double x = X(i);
        s[0] += x; s[1] += Y(i);
        lo = fmin(lo, x); nhi = fmin(nhi, -x);
    }
    block_sum<2>(s, shd);
    lo = block_min(lo, shd);
    const double hi = -block_min(nhi, shd);
    const double xm = s[0] / dn, ym = s[1] / dn;
    // Polynomial.fit maps [min x, max x] onto [-1, 1]: u = off + scl x
    const double scl = 2.0 / (hi - lo), off = -(hi + lo) / (hi - lo);
    double t[13];
#pragma unroll
    for (int u = 0; u < 13; ++u) t[u] = 0.0;
    for (int i = tid; i < n; i += 256) {
        if (!V(i)) continue;
        const double x = X(i), y = Y(i), dx = x - xm, dy = y - ym;
        t[0] += dx * dx; t[1] += dx * dy; t[2] += dy * dy;
        const double p = rx[i] - rmean, q = ry[i] - rmean;
        t[3] += p * p; t[4] += q * q; t[5] += p * q;
        const double u = off + scl * x, u2 = u * u;
        t[6] += u; t[7] += u2; t[8] += u2 * u; t[9] += u2 * u2;
        t[10] += y; t[11] += u * y; t[12] += u2 * y;
    }
    block_sum<13>(t, shd);
    // normal equations of the degree-2 least squares in u (symmetric positive definite, |u| <= 1): elimination in place
    double m00 = dn, m01 = t[6], m02 = t[7], m11 = t[7], m12 = t[8], m22 = t[9];
    double b0 = t[10], b1 = t[11], b2 = t[12];
    {
        const double f1 = m01 / m00, f2 = m02 / m00;
        m11 -= f1 * m01; m12 -= f1 * m02; b1 -= f1 * b0;
        m22 -= f2 * m02; b2 -= f2 * b0;
        if (m22 <= kSelRankTol * t[9]) {
            // m22 is now n Var(u^2): none means u^2 == 1 on every row, a descriptor with two distinct values.  The basis
            // {1, u, u^2} has rank 2 there, and Polynomial.fit's SVD answers with the minimum-norm coefficients: the line
            // c + a1 u through the two group means, its constant shared evenly between the columns 1 and u^2.  Stated
            // as the reduced system whose solution that is (a2 = c / 2, hence a0 = c - a2), so that the lines below --
            // and with them every result on a full-rank column -- stay as they were.
            m12 = 0.0; m22 = 1.0;
            b2 = 0.5 * ((b0 - m01 * (b1 / m11)) / m00);
        }
        const double f3 = m12 / m11;                     // (row 2, column 1) equals (1, 2) after the first step: symmetric
        m22 -= f3 * m12; b2 -= f3 * b1;
    }
    const double a2 = b2 / m22, a1 = (b1 - m12 * a2) / m11, a0 = (b0 - m01 * a1 - m02 * a2) / m00;
    double e[2] = {0.0, 0.0};
    for (int i = tid; i < n; i += 256) {
        if (!V(i)) continue;
        const double u = off + scl * X(i), f = a0 + u * (a1 + u * a2), r = Y(i) - f;
        e[0] += f; e[1] += r * r;
    }
    block_sum<2>(e, shd);
    const double fm = e[0] / dn;
    double g[2] = {0.0, 0.0};
    for (int i = tid; i < n; i += 256) {
        if (!V(i)) continue;
        const double u = off + scl * X(i), df = a0 + u * (a1 + u * a2) - fm;
        g[0] += df * df; g[1] += df * (Y(i) - ym);
    }
    block_sum<2>(g, shd);
    if (tid == 0) {
        auto clip = [](double r) { return r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r); };
        o[0] = clip(t[5] / sqrt(t[3]) / sqrt(t[4]));                         // Spearman: Pearson of the average ranks
        // scipy.stats.linregress: the covariances are divided by n, which cancels everywhere below
        const double r = (t[0] == 0.0 || t[2] == 0.0) ? 0.0 : clip(t[1] / sqrt(t[0] * t[2]));
        const double slope = t[1] / t[0];
        o[1] = slope; o[2] = ym - slope * xm; o[3] = r * r;
        o[4] = a0 + a1 * off + a2 * off * off;                               // p.convert().coef: the unscaled basis
        o[5] = a1 * scl + 2.0 * a2 * off * scl;
        o[6] = a2 * scl * scl;
        o[7] = e[1] / dn;                                                    // residue: SSE / n
        const double rq = (g[0] == 0.0 || t[2] == 0.0) ? 0.0 : clip(g[1] / sqrt(g[0] * t[2]));
        o[8] = rq * rq;                                                      // r^2 of fitted values against the style
        for (int u = 9; u < RAAE_SEL_STRIDE; ++u) o[u] = 0.0;
    }
}

#define SEL_KERNEL_PAIR(NAME, ARGS)                                                                              \
    __global__ __launch_bounds__(256) void NAME##_kernel(ARGS a) { NAME##_body(a); }                             \
    __global__ __launch_bounds__(256) void NAME##_kernel_m(const ARGS* t) {        /* one model per grid plane */ \
        const ARGS a = t[blockIdx.z];                                                                            \
        NAME##_body(a);                                                                                          \
    }
#define sel_rank_masked_body sel_rank_body
#define sel_sweep_masked_body sel_sweep_body
#define sel_stat_masked_body sel_stat_body
SEL_KERNEL_PAIR(sel_rank, SelArgs)
SEL_KERNEL_PAIR(sel_mae, SelArgs)
SEL_KERNEL_PAIR(sel_sweep, SelArgs)
SEL_KERNEL_PAIR(sel_stat, SelArgs)
SEL_KERNEL_PAIR(sel_rank_masked, SelArgsM)
SEL_KERNEL_PAIR(sel_sweep_masked, SelArgsM)
SEL_KERNEL_PAIR(sel_stat_masked, SelArgsM)

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

extern "C" long raae_select_work_bytes(int n, int k, int n_aux, int n_thresh) {
    if (n < 1 || k < 1 || n_aux < 0 || n_thresh < 0) return -1;
    return (long)(align256(sizeof(double) * (size_t)n * (size_t)(k + n_aux + 1)) + align256(sizeof(int) * 4 * (size_t)n_thresh));
}

// `extra`: rank columns behind the k + n_aux + 1 the unmasked form uses
static void sel_fill(SelArgs& a, const float* styles, int n, int k, const double* aux, int n_aux, const float* spec_in,
                     const float* spec_out, int L, const double* thresh, int n_thresh, void* work, double* out, int extra) {
    a.z = styles; a.aux = aux; a.sin = spec_in; a.sout = spec_out; a.th = thresh;
    a.rank_z = (double*)work;
    a.rank_d = a.rank_z + (size_t)k * n;
    a.mae = a.rank_d + (size_t)n_aux * n;
    a.sweep = (int*)((char*)work + align256(sizeof(double) * (size_t)n * (size_t)(k + n_aux + 1 + extra)));
    a.out = out;
    a.n = n; a.k = k; a.n_aux = n_aux; a.L = L; a.n_th = n_thresh;
}

extern "C" int raae_select_scores(const float* styles, int n, int k, const double* aux, int n_aux, const float* spec_in,
                                  const float* spec_out, int L, const double* thresh, int n_thresh, void* work,
                                  double* out, void* stream) {
    RAAE_CHECK_ARG(styles && aux && spec_in && spec_out && work && out);
    RAAE_CHECK_ARG(n >= 3 && k >= 2 && k <= 64 && n_aux >= 1 && n_aux <= k && L >= 1);
    RAAE_CHECK_ARG(n_aux < 2 || (thresh && n_thresh >= 1 && n_thresh <= 65535));
    SelArgs a;
    sel_fill(a, styles, n, k, aux, n_aux, spec_in, spec_out, L, thresh, n_thresh, work, out, 0);
    const hipStream_t st = (hipStream_t)stream;
    raae::launch(sel_rank_kernel, sel_rank_kernel_m, dim3(raae::cdiv(n, 256), k + n_aux), dim3(256), 0, st, a);
    raae::launch(sel_mae_kernel, sel_mae_kernel_m, dim3(raae::cdiv(n, 4)), dim3(256), 0, st, a);
    if (n_aux >= 2)
        raae::launch(sel_sweep_kernel, sel_sweep_kernel_m, dim3(n_thresh, 2), dim3(256), 0, st, a);
    raae::launch(sel_stat_kernel, sel_stat_kernel_m, dim3(2 + n_aux), dim3(256), 0, st, a);
    RAAE_LAUNCH_RET();
}

extern "C" long raae_select_masked_work_bytes(int n, int k, int n_aux, int n_thresh) {
    if (n < 1 || k < 1 || n_aux < 0 || n_thresh < 0) return -1;
    return (long)(align256(sizeof(double) * (size_t)n * (size_t)(k + 2 * n_aux + 1)) + align256(sizeof(int) * 4 * (size_t)n_thresh));
}

extern "C" int raae_select_scores_masked(const float* styles, int n, int k, const double* aux, int n_aux, const float* spec_in,
                                         const float* spec_out, int L, const double* thresh, int n_thresh, void* work,
                                         double* out, void* stream) {
    RAAE_CHECK_ARG(styles && aux && spec_in && spec_out && work && out);
    RAAE_CHECK_ARG(n >= 3 && k >= 2 && k <= 64 && n_aux >= 1 && n_aux <= k && L >= 1);
    RAAE_CHECK_ARG(n_aux < 2 || (thresh && n_thresh >= 1 && n_thresh <= 65535));
    SelArgsM a;
    sel_fill(a, styles, n, k, aux, n_aux, spec_in, spec_out, L, thresh, n_thresh, work, out, n_aux);
    a.rank_zs = a.mae + n;
    const hipStream_t st = (hipStream_t)stream;
    raae::launch(sel_rank_masked_kernel, sel_rank_masked_kernel_m, dim3(raae::cdiv(n, 256), k + 2 * n_aux), dim3(256), 0, st, a);
    raae::launch(sel_mae_kernel, sel_mae_kernel_m, dim3(raae::cdiv(n, 4)), dim3(256), 0, st, (const SelArgs&)a);
    if (n_aux >= 2)
        raae::launch(sel_sweep_masked_kernel, sel_sweep_masked_kernel_m, dim3(n_thresh, 2), dim3(256), 0, st, a);
    raae::launch(sel_stat_masked_kernel, sel_stat_masked_kernel_m, dim3(2 + n_aux), dim3(256), 0, st, a);
    RAAE_LAUNCH_RET();
}
