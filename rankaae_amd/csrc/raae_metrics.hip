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
#include <cmath>

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

// ---- style decorrelation penalty (ABI 31; config key `style_decorr`) ----------------------------------------------------
// D(z) = 1 / (k (k - 1)) * sum_{i != j} C_ij^2, C the Pearson correlation matrix of the k style columns over the b rows,
// and dz += w * dD/dz.  With x = z - mean, G = x^T x (the centred Gram matrix), s_i = sqrt(G_ii), C_ij = G_ij / (s_i s_j)
// and q_i = sum_{j != i} C_ij^2 the exact derivative (through the centring and the normalisation) is one k x k matrix
// applied to every centred row:
//     dD/dz[r][i] = sum_j M_ij x[r][j],   M_ij = 4 C_ij / (k (k - 1) s_i s_j)  (i != j),   M_ii = -4 q_i / (k (k - 1) s_i^2)
// A column with s_i == 0 has C_i. = 0 and a zero row and column of M: no gradient, nothing that is not finite.
//
// Everything is double: the means first, then the centred sums; the one fp32 rounding is the store of dz.  Every sum has
// a fixed order (strided per thread, then the slices in index order), there are no atomics: a replay gives the same bits.
// 256 threads; the k x k matrix, the per-column scalars and the workgroup's rows (as fp32) live in LDS, ~52 KB.
//
// One launch where the b * k styles fit the LDS stage (kDcStage floats: 256 x 6, 256 x 16, 64 x 64).  Otherwise two: the
// rows are cut into chunks of min(256, kDcStage / k); decorr_chunk_kernel leaves every chunk's column sums, means and
// Gram matrix centred on the CHUNK's means in `work`; every workgroup of decorr_apply_kernel then adds them as the
// pairwise update of Chan, Golub and LeVeque does, G = sum_c G_c + n_c (m_c - m)(m_c - m)^T -- centred sums again, no
// raw moments -- in chunk order (every workgroup the same bits), and applies M to its own chunk.
constexpr int kDcStage = 4096;
constexpr int kDcRows = 256;
struct DecorrArgs {
    const float* z; int ldz; int b; int k; double w; double* work; double* stats; float* dz; int lddz;
    int rows; int nchunk;               // rows per workgroup (>= b: the one-launch form) and the number of workgroups
};

// rows [r0, r0 + n) of z -> zs [n][k]
__device__ __forceinline__ void decorr_stage(const float* __restrict__ z, int ldz, int r0, int n, int k, float* zs) {
    for (int e = threadIdx.x; e < n * k; e += 256) {
        const int r = e / k, c = e - r * k;
        zs[e] = z[(size_t)(r0 + r) * ldz + c];
    }
    __syncthreads();
}

// column sums, means and the Gram matrix centred on those means of the n staged rows.  A sum over the rows is cut into
// as many slices as 256 threads allow (slice s takes rows s, s + nsl, ...); the slices meet in index order.
__device__ __forceinline__ void decorr_chunk_stats(const float* zs, int n, int k, double* part, double* sum, double* mean,
                                                   double* mat) {
    const int tid = threadIdx.x;
    {
        const int nsl = 256 / k, sl = tid / k, c = tid - sl * k;
        if (sl < nsl) {
            double a = 0.0;
            for (int r = sl; r < n; r += nsl) a += (double)zs[r * k + c];
            part[sl * k + c] = a;
        }
        __syncthreads();
        if (tid < k) {
            double s = 0.0;
            for (int q = 0; q < nsl; ++q) s += part[q * k + tid];
            sum[tid] = s;
            mean[tid] = s / (double)n;
        }
        __syncthreads();
    }
    const int P = k * k;
    if (P <= 256) {
        const int nsl = 256 / P, sl = tid / P, e = tid - sl * P;
        if (sl < nsl) {
            const int i = e / k, j = e - i * k;
            const double mi = mean[i], mj = mean[j];
            double a = 0.0;
            for (int r = sl; r < n; r += nsl) a += ((double)zs[r * k + i] - mi) * ((double)zs[r * k + j] - mj);
            part[sl * P + e] = a;
        }
        __syncthreads();
        if (tid < P) {
            double s = 0.0;
            for (int q = 0; q < nsl; ++q) s += part[q * P + tid];
            mat[tid] = s;
        }
    } else {
        for (int e = tid; e < P; e += 256) {
            const int i = e / k, j = e - i * k;
            const double mi = mean[i], mj = mean[j];
            double a = 0.0;
            for (int r = 0; r < n; ++r) a += ((double)zs[r * k + i] - mi) * ((double)zs[r * k + j] - mj);
            mat[e] = a;
        }
    }
    __syncthreads();
}

// mat: G -> M in place (both symmetric); returns D in every thread.  sd, q: k doubles each.
__device__ __forceinline__ double decorr_finish(double* mat, int k, double* sd, double* q) {
    const int tid = threadIdx.x;
    if (tid < k) sd[tid] = sqrt(mat[tid * k + tid]);
    __syncthreads();
    if (tid < k) {
        const double si = sd[tid];
        double a = 0.0;
        for (int j = 0; j < k; ++j) {
            const double sj = sd[j];
            const double c = (j != tid && si > 0.0 && sj > 0.0) ? mat[tid * k + j] / (si * sj) : 0.0;
            a += c * c;
        }
        q[tid] = a;
    }
    __syncthreads();
    const double kk = (double)k * (double)(k - 1);
    for (int e = tid; e < k * k; e += 256) {
        const int i = e / k, j = e - i * k;
        const double si = sd[i], sj = sd[j];
        double m = 0.0;
        if (si > 0.0 && sj > 0.0) m = i == j ? -4.0 * q[i] / (kk * si * si) : 4.0 * (mat[e] / (si * sj)) / (kk * si * sj);
        mat[e] = m;
    }
    double D = 0.0;
    for (int i = 0; i < k; ++i) D += q[i];
    __syncthreads();
    return D / kk;
}

// dz[r0 + r][i] = fl32(dz[r0 + r][i] + w * sum_j M_ij (zs[r][j] - mean[j])) for the n staged rows; an element whose
// gradient is exactly zero (a constant column) is not written
__device__ __forceinline__ void decorr_apply(const float* zs, int n, int k, const double* mat, const double* mean, double w,
                                             float* __restrict__ dz, int lddz, int r0) {
    for (int e = threadIdx.x; e < n * k; e += 256) {
        const int r = e / k, i = e - r * k;
        double g = 0.0;
        for (int j = 0; j < k; ++j) g += mat[j * k + i] * ((double)zs[r * k + j] - mean[j]);
        const double wg = w * g;
        if (wg != 0.0) {
            float* p = dz + (size_t)(r0 + r) * lddz + i;
            *p = (float)((double)*p + wg);
        }
    }
}

__device__ __forceinline__ void decorr_write_stats(double* stats, double D) {
    stats[0] = D;
    stats[1] += D;
    stats[2] += 1.0;
}

// the one-launch form: grid (1)
__device__ __forceinline__ void decorr_one_body(const DecorrArgs& a) {
    __shared__ double mat[64 * 64], part[256], sum[64], mean[64], sd[64], q[64];
    __shared__ float zs[kDcStage];
    if (a.k == 1 || a.b == 1) {                 // D = 0, no gradient (k == 1 comes here at every b: nothing is staged)
        if (threadIdx.x == 0) decorr_write_stats(a.stats, 0.0);
        return;
    }
    decorr_stage(a.z, a.ldz, 0, a.b, a.k, zs);
    decorr_chunk_stats(zs, a.b, a.k, part, sum, mean, mat);
    const double D = decorr_finish(mat, a.k, sd, q);
    if (threadIdx.x == 0) decorr_write_stats(a.stats, D);
    if (a.w != 0.0) decorr_apply(zs, a.b, a.k, mat, mean, a.w, a.dz, a.lddz, 0);
}
__global__ __launch_bounds__(256) void decorr_one_kernel(DecorrArgs a) { decorr_one_body(a); }
__global__ __launch_bounds__(256) void decorr_one_kernel_m(const DecorrArgs* t) {
    const DecorrArgs a = t[blockIdx.z];
    decorr_one_body(a);
}

// the two-launch form, first launch: grid (nchunk); work [nchunk][k sums | k means | k * k Gram]
__device__ __forceinline__ void decorr_chunk_body(const DecorrArgs& a) {
    __shared__ double mat[64 * 64], part[256], sum[64], mean[64];
    __shared__ float zs[kDcStage];
    const int k = a.k, r0 = blockIdx.x * a.rows, n = min(a.rows, a.b - r0);
    decorr_stage(a.z, a.ldz, r0, n, k, zs);
    decorr_chunk_stats(zs, n, k, part, sum, mean, mat);
    double* out = a.work + (size_t)blockIdx.x * (2 * k + k * k);
    for (int e = threadIdx.x; e < k; e += 256) { out[e] = sum[e]; out[k + e] = mean[e]; }
    for (int e = threadIdx.x; e < k * k; e += 256) out[2 * k + e] = mat[e];
}
__global__ __launch_bounds__(256) void decorr_chunk_kernel(DecorrArgs a) { decorr_chunk_body(a); }
__global__ __launch_bounds__(256) void decorr_chunk_kernel_m(const DecorrArgs* t) {
    const DecorrArgs a = t[blockIdx.z];
    decorr_chunk_body(a);
}

// second launch: grid (nchunk)
__device__ __forceinline__ void decorr_apply_body(const DecorrArgs& a) {
    __shared__ double mat[64 * 64], mean[64], sd[64], q[64];
    __shared__ float zs[kDcStage];
    const int tid = threadIdx.x, k = a.k, r0 = blockIdx.x * a.rows, n = min(a.rows, a.b - r0);
    const size_t stride = (size_t)(2 * k + k * k);
    decorr_stage(a.z, a.ldz, r0, n, k, zs);
    if (tid < k) {
        double s = 0.0;
        for (int c = 0; c < a.nchunk; ++c) s += a.work[c * stride + tid];
        mean[tid] = s / (double)a.b;
    }
    __syncthreads();
    for (int e = tid; e < k * k; e += 256) {
        const int i = e / k, j = e - i * k;
        const double mi = mean[i], mj = mean[j];
        double g = 0.0;
        for (int c = 0; c < a.nchunk; ++c) {
            const double* wc = a.work + c * stride;
            const double nc = (double)min(a.rows, a.b - c * a.rows);
            g += wc[2 * k + e] + nc * ((wc[k + i] - mi) * (wc[k + j] - mj));
        }
        mat[e] = g;
    }
    __syncthreads();
    const double D = decorr_finish(mat, k, sd, q);
    if (blockIdx.x == 0 && tid == 0) decorr_write_stats(a.stats, D);
    if (a.w != 0.0) decorr_apply(zs, n, k, mat, mean, a.w, a.dz, a.lddz, r0);
}
__global__ __launch_bounds__(256) void decorr_apply_kernel(DecorrArgs a) { decorr_apply_body(a); }
__global__ __launch_bounds__(256) void decorr_apply_kernel_m(const DecorrArgs* t) {
    const DecorrArgs a = t[blockIdx.z];
    decorr_apply_body(a);
}

// rows per workgroup: b itself where one workgroup stages all of them
static int decorr_rows(int b, int k) {
    if (k == 1 || (long)b * k <= kDcStage) return b;
    const int fit = kDcStage / k;
    return fit < kDcRows ? fit : kDcRows;
}

}  // namespace

extern "C" long raae_style_decorr_work_bytes(int b, int k) {
    if (b < 1 || k < 1 || k > 64) return 0;
    return (long)raae::cdiv(b, decorr_rows(b, k)) * (2 * k + k * k) * (long)sizeof(double);
}

extern "C" int raae_style_decorr_fwd_bwd(const float* z, int ldz, int b, int k, double w, void* work, double* stats, float* dz,
                                         int lddz, void* stream) {
    RAAE_CHECK_ARG(z && work && stats && dz && b >= 1 && k >= 1 && k <= 64 && ldz >= k && lddz >= k && std::isfinite(w));
    const int rows = decorr_rows(b, k), nchunk = raae::cdiv(b, rows);
    const DecorrArgs a = {z, ldz, b, k, w, (double*)work, stats, dz, lddz, rows, nchunk};
    if (nchunk == 1) {
        raae::launch(decorr_one_kernel, decorr_one_kernel_m, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
    } else {
        raae::launch(decorr_chunk_kernel, decorr_chunk_kernel_m, dim3(nchunk), dim3(256), 0, (hipStream_t)stream, a);
        raae::launch(decorr_apply_kernel, decorr_apply_kernel_m, dim3(nchunk), dim3(256), 0, (hipStream_t)stream, a);
    }
    RAAE_LAUNCH_RET();
}

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
