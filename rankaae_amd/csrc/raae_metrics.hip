// Model-selection metrics of the validation styles on the device: the Shapiro-Wilk W of every
// style column and Spearman's rho of every column pair, which the reference obtains per epoch with
// scipy.stats.shapiro / scipy.stats.spearmanr on a host copy (sc/clustering/trainer.py:286-292).
//
// Two launches.  style_rank_kernel gives every element its average rank and its slot in the sorted column by
// counting (exact for ties, no sort network, any n); style_stat_kernel then forms, one workgroup per column or
// column pair, the W statistic with the arithmetic of Royston's AS R94 as scipy 1.15.3 runs it (squared
// correlation of the sorted, range-scaled sample with the coefficient vector, reported as 1 - (1 - W)) and the
// Pearson correlation of the rank vectors.  All sums are double, in a fixed order (strided per thread, then a
// tree), so a replay is bitwise repeatable.
#include "raae_common.h"

namespace {

constexpr int kTile = 2048;

// grid (ceil(n / 256), k).  rank[c][i] = #{x_j < x_i} + (#{x_j == x_i} + 1) / 2; the element's slot in the sorted
// column is #{x_j < x_i} + #{j < i : x_j == x_i}; sorted[c][slot] = x_i - pivot_c (scipy subtracts x[n / 2],
// "the median or a nearby value", before the W arithmetic).
struct StyleRankArgs { const float* z; int n; int k; double* rank; double* sorted; };
__device__ __forceinline__ void style_rank_body(const float* __restrict__ z, int n, int k,
                                                double* __restrict__ rank, double* __restrict__ sorted) {
    __shared__ float tile[kTile];
    const int c = blockIdx.y, tid = threadIdx.x;
    const int i = blockIdx.x * 256 + tid;
    const float xi = i < n ? z[(size_t)i * k + c] : 0.f;
    int less = 0, eq = 0, eqb = 0;
    for (int j0 = 0; j0 < n; j0 += kTile) {
        const int m = min(kTile, n - j0);
        __syncthreads();
        for (int t = tid; t < m; t += 256) tile[t] = z[(size_t)(j0 + t) * k + c];
        __syncthreads();
        const int before = min(max(i - j0, 0), m);        // elements of this tile with index < i
        int jj = 0;
        for (; jj + 4 <= m; jj += 4) {
            const float4 v = *reinterpret_cast<const float4*>(tile + jj);
            less += (v.x < xi) + (v.y < xi) + (v.z < xi) + (v.w < xi);
            const int e0 = v.x == xi, e1 = v.y == xi, e2 = v.z == xi, e3 = v.w == xi;
            eq += e0 + e1 + e2 + e3;
            eqb += (e0 & (jj < before)) + (e1 & (jj + 1 < before)) + (e2 & (jj + 2 < before)) + (e3 & (jj + 3 < before));
        }
        for (; jj < m; ++jj) {
            const float v = tile[jj];
            less += v < xi;
            const int e = v == xi;
            eq += e;
            eqb += e & (jj < before);
        }
    }
    // The slot stays in [0, n) for any input, NaN included: it counts the disjoint sets {j : x_j < x_i} and
    // {j < i : x_j == x_i}, neither of which holds j = i, and every comparison with a NaN is false (a NaN element and
    // its neighbours may then share a slot -- a wrong W, never a store out of the column).  A diverged trial's grid
    // plane of a TrialBatch keeps running this kernel.
    if (i < n) {
        const double pivot = (double)z[(size_t)(n / 2) * k + c];
        rank[(size_t)c * n + i] = (double)less + 0.5 * (double)(eq + 1);
        sorted[(size_t)c * n + less + eqb] = (double)xi - pivot;
    }
}

template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* red) {
    const int tid = threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NV; ++u) red[u * 256 + tid] = v[u];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
#pragma unroll
            for (int u = 0; u < NV; ++u) red[u * 256 + tid] += red[u * 256 + tid + o];
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < NV; ++u) v[u] = red[u * 256];
}

__global__ __launch_bounds__(256) void style_rank_kernel(StyleRankArgs a) { style_rank_body(a.z, a.n, a.k, a.rank, a.sorted); }
__global__ __launch_bounds__(256) void style_rank_kernel_m(const StyleRankArgs* t) {       // one trial per grid plane
    const StyleRankArgs a = t[blockIdx.z];
    style_rank_body(a.z, a.n, a.k, a.rank, a.sorted);
}

// grid (k + k (k - 1) / 2).  Workgroups < k: W of column blockIdx.x; the others: rho of pair (p, q), p < q, in
// itertools.combinations order.  out = [W_0 .. W_{k-1}, rho_(0,1), rho_(0,2), ...].
struct StyleStatArgs { const double* rank; const double* sorted; const double* a; int n; int k; double* out; };
__device__ __forceinline__ void style_stat_body(const double* __restrict__ rank,
                                                const double* __restrict__ sorted,
                                                const double* __restrict__ a, int n, int k,
                                                double* __restrict__ out) {
    __shared__ double red[3 * 256];
    const int tid = threadIdx.x, w = blockIdx.x;
    if (w < k) {
        const double* y = sorted + (size_t)w * n;
        const double range = y[n - 1] - y[0];
        if (range < 1e-19) {                          // AS R94 ifault 6: W is reported as 1
            if (tid == 0) out[w] = 1.0;
            return;
        }
        // antisymmetric coefficient of order statistic i: -a[i] below the middle, +a[n-1-i] above, 0 at it
        auto coef = [&](int i) -> double {
            const int j = n - 1 - i;
            return i < j ? -a[i] : (i > j ? a[j] : 0.0);
        };
        double s[2] = {0.0, 0.0};
        for (int i = tid; i < n; i += 256) { s[0] += y[i] / range; s[1] += coef(i); }
        block_sum<2>(s, red);
        const double sx = s[0] / (double)n, sa = s[1] / (double)n;
        double t[3] = {0.0, 0.0, 0.0};
        for (int i = tid; i < n; i += 256) {
            const double asa = coef(i) - sa, xsx = y[i] / range - sx;
            t[0] += asa * asa; t[1] += xsx * xsx; t[2] += asa * xsx;
        }
        block_sum<3>(t, red);
        if (tid == 0) {
            const double ssassx = sqrt(t[0] * t[1]);
            const double w1 = (ssassx - t[2]) * (ssassx + t[2]) / (t[0] * t[1]);
            out[w] = 1.0 - w1;
        }
        return;
    }
    int p = 0, rest = w - k;
    while (rest >= k - 1 - p) { rest -= k - 1 - p; ++p; }
    const int q = p + 1 + rest;
    const double* rp = rank + (size_t)p * n;
    const double* rq = rank + (size_t)q * n;
    const double mean = 0.5 * (double)(n + 1);        // average ranks always sum to n (n + 1) / 2
    double t[3] = {0.0, 0.0, 0.0};
    for (int i = tid; i < n; i += 256) {
        const double u = rp[i] - mean, v = rq[i] - mean;
        t[0] += u * u; t[1] += v * v; t[2] += u * v;
    }
    block_sum<3>(t, red);
    if (tid == 0) {
        double r = t[2] / sqrt(t[0]) / sqrt(t[1]);     // numpy.corrcoef: divide by each deviation, then clip
        r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
        out[w] = r;
    }
}

// out[g][l] = mean_s x[g][s][l]: the n_sampling average of the report's decoder sweeps (sc/report/analysis.py:78-86).
// One thread per output column element; the sum runs in sample order in double.
__global__ __launch_bounds__(256) void style_stat_kernel(StyleStatArgs a) { style_stat_body(a.rank, a.sorted, a.a, a.n, a.k, a.out); }
__global__ __launch_bounds__(256) void style_stat_kernel_m(const StyleStatArgs* t) {
    const StyleStatArgs a = t[blockIdx.z];
    style_stat_body(a.rank, a.sorted, a.a, a.n, a.k, a.out);
}

__global__ __launch_bounds__(256) void group_mean_kernel(const float* __restrict__ x, int groups, int per, int L,
                                                         float* __restrict__ out) {
    const long n = (long)groups * L;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const long g = i / L, l = i - g * L;
        const float* p = x + g * (long)per * L + l;
        double acc = 0.0;
        for (int s = 0; s < per; ++s) acc += (double)p[(long)s * L];
        out[i] = (float)(acc / (double)per);
    }
}

// ---- Kendall's tau-b of style k against descriptor k (ABI 30; config key `rank_metrics`) --------------------------------
// What scipy.stats.kendalltau(d_k, z_k, variant="b") returns on the rows labelled for descriptor k, from exact pair
// counts.  kendall_pairs_kernel: grid (T * S, n_aux), T = ceil(n / 256) row tiles.  A thread owns one row of its row
// tile and meets the rows of a column tile staged in LDS (every lane reads the same address: a broadcast).  The
// unordered tile pairs are dealt out cyclically: row tile ti takes the column tiles (ti + o) mod T, o = 0 .. T / 2 (for
// an even T the offset T / 2 belongs to the lower half of the row tiles alone), so every tile pair is met once, every
// row tile does the same work, and the partials grow with T, not T^2; split s of S takes the offsets s, s + S, ...
// The diagonal tile (o = 0) counts j behind i only.  Rows without a label (a descriptor cell that is not finite) never
// reach the LDS tile: the stage compacts the labelled rows in row order, which also keeps "behind" meaningful there.
//
// A pair is classified by <, >, == of the stored values, taken on their order-preserving integer keys (the bits, with
// the magnitude of a negative value inverted, and -0 as +0): the same order and the same ties as the float comparisons
// for every value that is not NaN, with no arithmetic on the values and no dependence on the denormal mode -- two
// subnormals one ulp apart are ordered.  A NaN style is just some key: counts without meaning, nothing out of bounds.
constexpr int kKtTile = 256;
constexpr int kKtMaxSplit = 8;
struct KendallPart { long long c[6]; };     // C, D, Tx, Ty, Txy of the workgroup's pairs; labelled rows of its row tile

__device__ __forceinline__ int kendall_key(float x) {
    int b = __float_as_int(x);
    b = b < 0 ? b ^ 0x7fffffff : b;
    return b == -1 ? 0 : b;                 // -0.0 (0x80000000 -> -1) ties with +0.0
}
__device__ __forceinline__ bool kendall_labelled(float d) { return (__float_as_uint(d) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ long long kendall_block_sum(long long v, long long* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

struct KendallPairsArgs { const float* d; int ldd; const float* z; int ldz; int n; int T; int S; KendallPart* part; };
__device__ __forceinline__ void kendall_pairs_body(const float* __restrict__ d, int ldd, const float* __restrict__ z,
                                                   int ldz, int n, int T, int S, KendallPart* __restrict__ part) {
    __shared__ int2 tile[kKtTile];          // {descriptor key, style key} of the column tile's labelled rows
    __shared__ int wave_n[4];
    __shared__ long long red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ti = blockIdx.x / S, s = blockIdx.x - ti * S, k = blockIdx.y;
    const int i = ti * kKtTile + tid;
    int di = 0, zi = 0;
    bool vi = false;
    if (i < n) {
        const float dv = d[(size_t)i * ldd + k];
        vi = kendall_labelled(dv);
        di = kendall_key(dv); zi = kendall_key(z[(size_t)i * ldz + k]);
    }
    const int H = T / 2;
    const int omax = ((T & 1) || ti < H) ? H : H - 1;
    int nc = 0, nd = 0, ntx = 0, nty = 0, ntxy = 0;
    for (int o = s; o <= omax; o += S) {
        const int tj = ti + o < T ? ti + o : ti + o - T;
        const int j = tj * kKtTile + tid;
        int dj = 0, zj = 0;
        bool vj = false;
        if (j < n) {
            const float dv = d[(size_t)j * ldd + k];
            vj = kendall_labelled(dv);
            dj = kendall_key(dv); zj = kendall_key(z[(size_t)j * ldz + k]);
        }
        const unsigned long long live = __ballot(vj);
        if (lane == 0) wave_n[wave] = __popcll(live);
        __syncthreads();                    // the counts are there, and every wave has left the previous tile
        int pos = __popcll(live & ((1ull << lane) - 1ull)), nv = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { const int c = wave_n[w]; pos += w < wave ? c : 0; nv += c; }
        if (vj) tile[pos] = make_int2(dj, zj);
        __syncthreads();
        // diagonal tile: row i is the tile's row `pos` (tj == ti, so vj == vi), and pairs with the rows behind it
        const int first = vi ? (o == 0 ? pos + 1 : 0) : nv;
#pragma unroll 4
        for (int jj = first; jj < nv; ++jj) {
            const int2 t = tile[jj];
            const bool dl = t.x < di, dg = t.x > di, zl = t.y < zi, zg = t.y > zi;
            const bool de = !(dl | dg), ze = !(zl | zg);
            nc += (dl & zl) | (dg & zg);
            nd += (dl & zg) | (dg & zl);
            ntx += de & !ze;
            nty += ze & !de;
            ntxy += de & ze;
        }
    }
    const long long lab = (s == 0 && vi) ? 1 : 0;
    const long long t0 = kendall_block_sum(nc, red), t1 = kendall_block_sum(nd, red), t2 = kendall_block_sum(ntx, red);
    const long long t3 = kendall_block_sum(nty, red), t4 = kendall_block_sum(ntxy, red), t5 = kendall_block_sum(lab, red);
    if (tid == 0) {
        KendallPart p;
        p.c[0] = t0; p.c[1] = t1; p.c[2] = t2; p.c[3] = t3; p.c[4] = t4; p.c[5] = t5;
        part[(size_t)k * gridDim.x + blockIdx.x] = p;
    }
}
__global__ __launch_bounds__(256) void kendall_pairs_kernel(KendallPairsArgs a) {
    kendall_pairs_body(a.d, a.ldd, a.z, a.ldz, a.n, a.T, a.S, a.part);
}
__global__ __launch_bounds__(256) void kendall_pairs_kernel_m(const KendallPairsArgs* t) {
    const KendallPairsArgs a = t[blockIdx.z];
    kendall_pairs_body(a.d, a.ldd, a.z, a.ldz, a.n, a.T, a.S, a.part);
}

// grid (n_aux): workgroup k adds descriptor k's partials (integers: any order gives the same sums; this one is fixed)
// and forms tau in double in scipy's order of operations.
struct KendallFinArgs { const KendallPart* part; int nparts; long long* counts; double* tau; };
__device__ __forceinline__ void kendall_finish_body(const KendallPart* __restrict__ part, int nparts,
                                                    long long* __restrict__ counts, double* __restrict__ tau) {
    __shared__ long long red[4];
    const int tid = threadIdx.x, k = blockIdx.x;
    const KendallPart* p = part + (size_t)k * nparts;
    long long a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0, a5 = 0;
    for (int w = tid; w < nparts; w += 256) {
        const KendallPart v = p[w];
        a0 += v.c[0]; a1 += v.c[1]; a2 += v.c[2]; a3 += v.c[3]; a4 += v.c[4]; a5 += v.c[5];
    }
    const long long C_ = kendall_block_sum(a0, red), D_ = kendall_block_sum(a1, red), Tx = kendall_block_sum(a2, red);
    const long long Ty = kendall_block_sum(a3, red), Txy = kendall_block_sum(a4, red), m = kendall_block_sum(a5, red);
    if (tid == 0) {
        long long* c = counts + (size_t)k * 6;
        c[0] = C_; c[1] = D_; c[2] = Tx; c[3] = Ty; c[4] = Txy; c[5] = m;
        const long long tot = m * (m - 1) / 2, fx = tot - (Tx + Txy), fy = tot - (Ty + Txy);
        double t = __longlong_as_double(0x7ff8000000000000LL);       // fewer than two rows, or a constant column
        if (m >= 2 && fx != 0 && fy != 0) t = (double)(C_ - D_) / sqrt((double)fx) / sqrt((double)fy);
        tau[k] = t;
    }
}
__global__ __launch_bounds__(256) void kendall_finish_kernel(KendallFinArgs a) { kendall_finish_body(a.part, a.nparts, a.counts, a.tau); }
__global__ __launch_bounds__(256) void kendall_finish_kernel_m(const KendallFinArgs* t) {
    const KendallFinArgs a = t[blockIdx.z];
    kendall_finish_body(a.part, a.nparts, a.counts, a.tau);
}

// column-tile splits per row tile: enough workgroups for the chip while there are few row tiles, one from ~200 row tiles
// on (the partials stay linear in n: T * S <= min(kKtMaxSplit * T, 1024 / n_aux + T) per descriptor)
static int kendall_split(int T, int n_aux) {
    const int want = raae::cdiv(1024, (long)T * n_aux), most = T / 2 + 1;
    const int s = want < most ? want : most;
    return s < 1 ? 1 : (s > kKtMaxSplit ? kKtMaxSplit : s);
}

}  // namespace

extern "C" long raae_kendall_tau_work_bytes(int n, int n_aux) {
    if (n < 1 || n_aux < 1 || n_aux > 16) return 0;
    const int T = raae::cdiv(n, kKtTile);
    return (long)T * kendall_split(T, n_aux) * n_aux * (long)sizeof(KendallPart);
}

extern "C" int raae_kendall_tau(const float* d, int ldd, const float* z, int ldz, int n, int n_aux, void* work,
                                long long* counts, double* tau, void* stream) {
    RAAE_CHECK_ARG(d && z && work && counts && tau && n >= 1 && n_aux >= 1 && n_aux <= 16 && ldd >= n_aux && ldz >= n_aux);
    const int T = raae::cdiv(n, kKtTile), S = kendall_split(T, n_aux);
    const KendallPairsArgs pa = {d, ldd, z, ldz, n, T, S, (KendallPart*)work};
    raae::launch(kendall_pairs_kernel, kendall_pairs_kernel_m, dim3(T * S, n_aux), dim3(256), 0, (hipStream_t)stream, pa);
    const KendallFinArgs fa = {(const KendallPart*)work, T * S, counts, tau};
    raae::launch(kendall_finish_kernel, kendall_finish_kernel_m, dim3(n_aux), dim3(256), 0, (hipStream_t)stream, fa);
    RAAE_LAUNCH_RET();
}

extern "C" int raae_group_mean(const float* x, int groups, int per, int L, float* out, void* stream) {
    RAAE_CHECK_ARG(x && out && groups > 0 && per > 0 && L > 0);
    const long n = (long)groups * L;
    const int grid = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    RAAE_PLAIN_LAUNCH(group_mean_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, groups, per, L, out);
    RAAE_LAUNCH_RET();
}

extern "C" int raae_style_metrics(const float* z, int n, int k, const double* a_coef, double* work, double* out,
                                  void* stream) {
    RAAE_CHECK_ARG(z && a_coef && work && out && n >= 3 && k >= 1 && k <= 64);
    double* rank = work;
    double* sorted = work + (size_t)k * n;
    const StyleRankArgs ra = {z, n, k, rank, sorted};
    raae::launch(style_rank_kernel, style_rank_kernel_m, dim3(raae::cdiv(n, 256), k), dim3(256), 0, (hipStream_t)stream, ra);
    const StyleStatArgs sa = {rank, sorted, a_coef, n, k, out};
    raae::launch(style_stat_kernel, style_stat_kernel_m, dim3(k + k * (k - 1) / 2), dim3(256), 0, (hipStream_t)stream, sa);
    RAAE_LAUNCH_RET();
}
