// LDS-tiled versions of the conv-family kernels (included inside raae_conv.hip's anonymous
// namespace).  A workgroup stages whole samples -- S at a time, all channels, the PReLU /
// BatchNorm / dropout view or the BatchNorm-backward gradient applied ONCE per element while
// staging -- and computes every output of those samples from LDS: the conv windows are read
// from the staged (halo-padded) tile, never re-fetched from HBM.  Workgroups grid-stride over
// sample groups; BatchNorm partials and parameter-gradient slabs are per workgroup (fixed order).
//
// Thread mapping: a thread is bound to ONE channel for the whole kernel (c = tid / tpc with
// tpc = 256 / C threads per channel) and walks the (sample, position) space of that channel.
// Per-channel sums are then plain per-thread registers (no select chains), lanes of a wave read
// consecutive LDS addresses (conflict-free) and the channel's weights are wave-uniform broadcasts.

#define CT_MAXCH 8           // most channels a tiled kernel handles (more => generic kernels)

struct ChanMap { int c, j, tpc; bool active; };
__device__ __forceinline__ ChanMap chan_map(int C) {
    ChanMap m;
    m.tpc = 256 / C;
    m.c = threadIdx.x / m.tpc;
    m.j = threadIdx.x - m.c * m.tpc;
    m.active = m.c < C;
    return m;
}
// q -> (q / L, q % L); sh = log2(L) when L is a power of two, else -1
__device__ __forceinline__ void split(int q, int L, int sh, int* hi, int* lo) {
    if (sh >= 0) { *hi = q >> sh; *lo = q & (L - 1); }
    else { *hi = q / L; *lo = q - *hi * L; }
}

// ---- staging a view tile in two halves: tile_issue() requests the first four elements of this thread and its
// halo element (raw values, independent of any statistic), tile_commit() transforms and stores them and then
// handles whatever is left.  (Measured: calling tile_issue() before a kernel's statistic prologue does not pay
// at one wave per SIMD -- the extra address arithmetic costs what the overlapped round trip saves -- so today
// the two halves are only used back to back, as a batched replacement of the element-by-element loop.)
struct TilePre { float xr[4], xm[4]; int off[4]; float hraw, hmask; int hq, hs, hh, nh; };

__device__ __forceinline__ void tile_issue(TilePre& p, const raae_view_t& v, int C, int L, int sh, int pad, int replicate,
                                           int b0, int nb) {
    const ChanMap m = chan_map(C);
    p.nh = 0; p.hq = m.j; p.hs = 0; p.hh = 0; p.hraw = 0.f; p.hmask = 1.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) { p.off[r] = -1; p.xr[r] = 0.f; p.xm[r] = 1.f; }
    if (!m.active) return;
    const int Lp = L + 2 * pad;
    const int n = nb * L;
    const size_t base = ((size_t)b0 * C + m.c) * L;               // sample s of this channel: + s*C*L
    p.nh = pad > 0 ? nb * 2 * pad : 0;                            // halo elements of this channel
    if (p.hq < p.nh) {
        p.hs = p.hq / (2 * pad); p.hh = p.hq - p.hs * 2 * pad;
        if (replicate) {
            const size_t gi = base + (size_t)p.hs * C * L + (p.hh < pad ? 0 : L - 1);
            p.hraw = v.raw[gi];
            if (v.mask) p.hmask = v.mask[gi];
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int q = m.j + r * m.tpc;
        int s, l;
        split(q < n ? q : 0, L, sh, &s, &l);
        const size_t gi = base + (size_t)s * C * L + l;
        p.xr[r] = v.raw[gi];
        p.xm[r] = v.mask ? v.mask[gi] : 1.f;
        p.off[r] = q < n ? (s * C + m.c) * Lp + pad + l : -1;
    }
}

__device__ __forceinline__ void tile_commit(float* tile, const TilePre& p, const raae_view_t& v, const ViewStats* st, int C,
                                            int L, int sh, int pad, int replicate, int b0, int nb) {
    const ChanMap m = chan_map(C);
    if (!m.active) return;
    const int Lp = L + 2 * pad;
    const int n = nb * L;
    const float sl = v.slope ? v.slope[m.c] : 1.f;
    const float mu = v.has_bn ? st->mean[m.c] : 0.f, rs = v.has_bn ? st->rstd[m.c] : 1.f;
    const size_t base = ((size_t)b0 * C + m.c) * L;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (p.off[r] < 0) continue;
        float x = p.xr[r];
        if (v.slope) x = prelu(x, sl);
        if (v.has_bn) x = (x - mu) * rs;
        tile[p.off[r]] = x * p.xm[r];
    }
    if (p.hq < p.nh) {
        float x = 0.f;
        if (replicate) {
            x = p.hraw;
            if (v.slope) x = prelu(x, sl);
            if (v.has_bn) x = (x - mu) * rs;
            x *= p.hmask;
        }
        tile[(p.hs * C + m.c) * Lp + (p.hh < pad ? p.hh : L + p.hh)] = x;
    }
    for (int q0 = m.j + 4 * m.tpc; q0 < n; q0 += 4 * m.tpc) {     // more than four elements per thread
        float xr[4], xm[4];
        int off[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q = q0 + r * m.tpc;
            int s, l;
            split(q < n ? q : q0, L, sh, &s, &l);
            const size_t gi = base + (size_t)s * C * L + l;
            xr[r] = v.raw[gi];
            xm[r] = v.mask ? v.mask[gi] : 1.f;
            off[r] = q < n ? (s * C + m.c) * Lp + pad + l : -1;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (off[r] < 0) continue;
            float x = xr[r];
            if (v.slope) x = prelu(x, sl);
            if (v.has_bn) x = (x - mu) * rs;
            tile[off[r]] = x * xm[r];
        }
    }
    for (int hq = p.hq + m.tpc; hq < p.nh; hq += m.tpc) {         // more halo elements than threads: rare
        const int s = hq / (2 * pad), h = hq - s * 2 * pad;
        float x = 0.f;
        if (replicate) x = view_at(v, st, m.c, base + (size_t)s * C * L + (h < pad ? 0 : L - 1));
        tile[(s * C + m.c) * Lp + (h < pad ? h : L + h)] = x;
    }
}

// ---- 16-byte staging (rows whose length is a multiple of four, 16-byte aligned tensors).
// A thread stays bound to its channel and walks QUADS of four consecutive positions, U of them per trip with every
// global load of the trip issued before the first use: at large batches a workgroup stages tens of kilobytes per
// group and the element-by-element loop was one dependent memory round trip per element and lane (measured at
// B = 4096: 10.8 us for the 32 KB elementwise stage of one four-sample group).
__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
__device__ __forceinline__ bool view_vec_ok(const raae_view_t& v, int L) {
    return (L & 3) == 0 && aligned16(v.raw) && aligned16(v.mask);
}
__device__ __forceinline__ float4 prelu4(float4 x, float a) {
    return make_float4(prelu(x.x, a), prelu(x.y, a), prelu(x.z, a), prelu(x.w, a));
}

template <int U>
__device__ __forceinline__ void stage_view_tile_v4(float* tile, const raae_view_t& v, const ViewStats* st, int C, int L,
                                                   int sh, int pad, int replicate, int b0, int nb) {
    const ChanMap m = chan_map(C);
    if (!m.active) return;
    const int L4 = L >> 2, sh4 = sh >= 2 ? sh - 2 : -1, Lp = L + 2 * pad;
    const int n4 = nb * L4;
    const bool has_slope = v.slope != nullptr, has_bn = v.has_bn != 0, has_mask = v.mask != nullptr;
    const float sl = has_slope ? v.slope[m.c] : 1.f;
    const float mu = has_bn ? st->mean[m.c] : 0.f, rs = has_bn ? st->rstd[m.c] : 1.f;
    const size_t base = ((size_t)b0 * C + m.c) * L;
    const float4* src = reinterpret_cast<const float4*>(v.raw + base);
    const float4* msk = has_mask ? reinterpret_cast<const float4*>(v.mask + base) : nullptr;
    const bool st16 = ((Lp | pad) & 3) == 0;             // tile rows and their first element on 16-byte boundaries
    for (int q0 = m.j; q0 < n4; q0 += U * m.tpc) {
        float4 x[U], mk[U];
        int row[U], l4[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int q = q0 + u * m.tpc;
            int s, l;
            split(q < n4 ? q : q0, L4, sh4, &s, &l);
            const size_t gi = (size_t)s * C * L4 + l;
            x[u] = src[gi];
            if (has_mask) mk[u] = msk[gi];
            row[u] = q < n4 ? s * C + m.c : -1;
            l4[u] = l;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (row[u] < 0) continue;
            float4 y = x[u];
            if (has_slope) y = prelu4(y, sl);
            if (has_bn) y = make_float4((y.x - mu) * rs, (y.y - mu) * rs, (y.z - mu) * rs, (y.w - mu) * rs);
            if (has_mask) y = make_float4(y.x * mk[u].x, y.y * mk[u].y, y.z * mk[u].z, y.w * mk[u].w);
            float* r = tile + row[u] * Lp + pad;
            if (st16) *reinterpret_cast<float4*>(r + 4 * l4[u]) = y;
            else { r[4 * l4[u]] = y.x; r[4 * l4[u] + 1] = y.y; r[4 * l4[u] + 2] = y.z; r[4 * l4[u] + 3] = y.w; }
            if (pad > 0 && l4[u] == 0) {
                const float e = replicate ? y.x : 0.f;
                for (int k = 1; k <= pad; ++k) r[-k] = e;
            }
            if (pad > 0 && l4[u] == L4 - 1) {
                const float e = replicate ? y.w : 0.f;
                for (int k = 0; k < pad; ++k) r[L + k] = e;
            }
        }
    }
}

// stage nb samples of a view into tile[s][c][Lp], Lp = L + 2*pad (halo: replicate or zero)
// BIG: instance for large batches (>= 1024 rows); the launch-bound small-batch instances do not carry the 16-byte
// path at all (its mere presence cost the 256-row weight-gradient kernels 4-5 us each: registers, code size)
template <bool BIG>
__device__ __forceinline__ void stage_view_tile(float* tile, const raae_view_t& v, const ViewStats* st, int C, int L,
                                                int sh, int pad, int replicate, int b0, int nb) {
    if constexpr (BIG) {
        if (view_vec_ok(v, L) && nb * L >= 512) {       // uniform: large tiles take the 16-byte path
            stage_view_tile_v4<4>(tile, v, st, C, L, sh, pad, replicate, b0, nb);
            return;
        }
    }
    TilePre p;
    tile_issue(p, v, C, L, sh, pad, replicate, b0, nb);
    tile_commit(tile, p, v, st, C, L, sh, pad, replicate, b0, nb);
}

// stage dL/d(raw) of nb samples into tile[s][c][L]; optionally dA*raw[raw<=0] into tile_s (for dslope)
// four consecutive elements of grad_at(): dL/d raw (and dA = gradient w.r.t. the activation output, raw) from
// already loaded operands -- the arithmetic of grad_at, element by element
struct Grad4 { float4 dr, da, raw; };
struct Grad1 { float dr, da; };
__device__ __forceinline__ Grad1 grad_elem(const raae_grad_t& g, float gv, float raw, float u, bool has_u, float sl,
                                           float mu, float rs, float m1, float m2) {
    Grad1 o;
    o.da = gv;
    if (g.has_bn) {
        const float uu = has_u ? u : (g.slope ? prelu(raw, sl) : raw);
        const float y = (uu - mu) * rs;
        o.da = rs * (gv - m1 - y * m2);
    }
    o.dr = o.da;
    if (g.slope) o.dr = raw > 0.f ? o.da : o.da * sl;
    else if (g.act == RAAE_OUT_SOFTPLUS) o.dr = o.da * (1.f - expf(-2.f * raw));
    else if (g.act == RAAE_OUT_RELU) o.dr = raw > 0.f ? o.da : 0.f;
    return o;
}
// (values only, no pointers into the result: an address taken inside a float4 keeps the struct in scratch memory)
__device__ __forceinline__ Grad4 grad_quad(const raae_grad_t& g, float4 gv, float4 raw, float4 u, bool has_u, float sl,
                                           float mu, float rs, float m1, float m2) {
    const Grad1 a = grad_elem(g, gv.x, raw.x, u.x, has_u, sl, mu, rs, m1, m2);
    const Grad1 b = grad_elem(g, gv.y, raw.y, u.y, has_u, sl, mu, rs, m1, m2);
    const Grad1 c = grad_elem(g, gv.z, raw.z, u.z, has_u, sl, mu, rs, m1, m2);
    const Grad1 d = grad_elem(g, gv.w, raw.w, u.w, has_u, sl, mu, rs, m1, m2);
    Grad4 o;
    o.dr = make_float4(a.dr, b.dr, c.dr, d.dr);
    o.da = make_float4(a.da, b.da, c.da, d.da);
    o.raw = raw;
    return o;
}
__device__ __forceinline__ bool grad_vec_ok(const raae_grad_t& g, int L) {
    return (L & 3) == 0 && aligned16(g.g) && aligned16(g.raw) && aligned16(g.u);
}

template <int U>
__device__ __forceinline__ void stage_grad_tile_v4(float* tile, float* tile_s, const raae_grad_t& g, const GradStats* st,
                                                   int C, int L, int sh, int b0, int nb) {
    const ChanMap m = chan_map(C);
    if (!m.active) return;
    const int L4 = L >> 2, sh4 = sh >= 2 ? sh - 2 : -1;
    const int n4 = nb * L4;
    const bool has_raw = g.raw != nullptr, has_u = g.u != nullptr, has_bn = g.has_bn != 0;
    const float sl = g.slope ? g.slope[m.c] : 1.f;
    const float mu = has_bn ? st->mean[m.c] : 0.f, rs = has_bn ? st->rstd[m.c] : 1.f;
    const float m1 = has_bn ? st->m1[m.c] : 0.f, m2 = has_bn ? st->m2[m.c] : 0.f;
    const size_t base = ((size_t)b0 * C + m.c) * L;
    const float4* pg = reinterpret_cast<const float4*>(g.g + base);
    const float4* pr = has_raw ? reinterpret_cast<const float4*>(g.raw + base) : nullptr;
    const float4* pu = has_u ? reinterpret_cast<const float4*>(g.u + base) : nullptr;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int q0 = m.j; q0 < n4; q0 += U * m.tpc) {
        float4 gv[U], rv[U], uv[U];
        int o[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int q = q0 + u * m.tpc;
            int s, l;
            split(q < n4 ? q : q0, L4, sh4, &s, &l);
            const size_t gi = (size_t)s * C * L4 + l;
            gv[u] = pg[gi];
            rv[u] = has_raw ? pr[gi] : zero4;
            uv[u] = (has_u && has_bn) ? pu[gi] : zero4;
            o[u] = q < n4 ? (s * C + m.c) * L + 4 * l : -1;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (o[u] < 0) continue;
            const Grad4 r = grad_quad(g, gv[u], rv[u], uv[u], has_u, sl, mu, rs, m1, m2);
            *reinterpret_cast<float4*>(tile + o[u]) = r.dr;
            if (tile_s) *reinterpret_cast<float4*>(tile_s + o[u]) = make_float4(
                r.raw.x <= 0.f ? r.da.x * r.raw.x : 0.f, r.raw.y <= 0.f ? r.da.y * r.raw.y : 0.f,
                r.raw.z <= 0.f ? r.da.z * r.raw.z : 0.f, r.raw.w <= 0.f ? r.da.w * r.raw.w : 0.f);
        }
    }
}

template <bool BIG>
__device__ __forceinline__ void stage_grad_tile(float* tile, float* tile_s, const raae_grad_t& g, const GradStats* st,
                                                int C, int L, int sh, int b0, int nb) {
    if constexpr (BIG) {
        if (grad_vec_ok(g, L) && nb * L >= 512 && ((C * L) & 3) == 0) {
            stage_grad_tile_v4<4>(tile, tile_s, g, st, C, L, sh, b0, nb);
            return;
        }
    }
    const ChanMap m = chan_map(C);
    if (!m.active) return;
    const int n = nb * L;
    for (int q = m.j; q < n; q += m.tpc) {
        int s, l;
        split(q, L, sh, &s, &l);
        float da, raw;
        const int o = (s * C + m.c) * L + l;
        tile[o] = grad_at(g, st, m.c, (size_t)b0 * C * L + o, &da, &raw);
        if (tile_s) tile_s[o] = raw <= 0.f ? da * raw : 0.f;
    }
}

// per-channel totals of per-thread partials (a, b): fixed order; out[c*2] = sum a, out[c*2+1] = sum b.
// All 256 threads call it.  scr: LDS [2][256] doubles, scr2: LDS [2][CT_MAXCH*8] doubles.
__device__ __forceinline__ void chan_reduce(double a, double b, int C, const ChanMap& m, double* out, double* scr,
                                            double* scr2) {
    __syncthreads();
    if ((m.tpc & (m.tpc - 1)) == 0) {
        // C a power of two: a channel is a run of whole lanes -> xor-shuffle tree, LDS only across waves
        const int w = m.tpc < 64 ? m.tpc : 64;
        for (int o = w >> 1; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
        if (m.tpc <= 64) {
            if (m.j == 0) { out[m.c * 2] = a; out[m.c * 2 + 1] = b; }
            return;
        }
        if ((threadIdx.x & 63) == 0) { scr[threadIdx.x >> 6] = a; scr[4 + (threadIdx.x >> 6)] = b; }
        __syncthreads();
        if (threadIdx.x < C) {
            const int nwv = m.tpc >> 6;
            double sa = 0.0, sb = 0.0;
            for (int k = 0; k < nwv; ++k) { sa += scr[threadIdx.x * nwv + k]; sb += scr[4 + threadIdx.x * nwv + k]; }
            out[threadIdx.x * 2] = sa; out[threadIdx.x * 2 + 1] = sb;
        }
        return;
    }
    scr[threadIdx.x] = m.active ? a : 0.0;
    scr[256 + threadIdx.x] = m.active ? b : 0.0;
    __syncthreads();
    if (threadIdx.x < C * 8) {
        const int c = threadIdx.x >> 3, part = threadIdx.x & 7;
        double sa = 0.0, sb = 0.0;
        for (int k = part; k < m.tpc; k += 8) { sa += scr[c * m.tpc + k]; sb += scr[256 + c * m.tpc + k]; }
        scr2[threadIdx.x] = sa; scr2[CT_MAXCH * 8 + threadIdx.x] = sb;
    }
    __syncthreads();
    if (threadIdx.x < C) {
        double sa = 0.0, sb = 0.0;
        for (int k = 0; k < 8; ++k) { sa += scr2[threadIdx.x * 8 + k]; sb += scr2[CT_MAXCH * 8 + threadIdx.x * 8 + k]; }
        out[threadIdx.x * 2] = sa; out[threadIdx.x * 2 + 1] = sb;
    }
}


// Per-channel totals of NV (power of two, <= 8) per-thread doubles in one pass: res[c * NV + k] (LDS).  Channel
// counts that make a channel a run of >= NV whole lanes take a halving butterfly (NV + log2(lanes/NV) shuffles
// instead of NV * log2(lanes)); other counts fall back to pairs through chan_reduce.  All 256 threads call
// it; the caller puts a barrier before reading res.
template <int NV>
__device__ __forceinline__ void chan_reduce_n(double (&v)[NV], int C, const ChanMap& m, double* res, double* scr,
                                              double* scr2) {
    __syncthreads();
    if ((m.tpc & (m.tpc - 1)) == 0 && m.tpc >= NV) {
        const int lane = threadIdx.x & 63;
        raae::group_multi_sum<NV>(v, lane, m.tpc < 64 ? m.tpc : 64);
        const int slot = raae::group_multi_slot<NV>(lane);
        if (m.tpc <= 64) {
            if (m.j < NV) res[m.c * NV + slot] = v[0];
            return;
        }
        if (lane < NV) scr[(threadIdx.x >> 6) * NV + slot] = v[0];
        __syncthreads();
        if ((int)threadIdx.x < C * NV) {
            const int c = threadIdx.x / NV, k = threadIdx.x - c * NV, nwv = m.tpc >> 6;
            double t = 0.0;
            for (int i = 0; i < nwv; ++i) t += scr[(c * nwv + i) * NV + k];
            res[c * NV + k] = t;
        }
        return;
    }
    __shared__ double pair_out[2 * CT_MAXCH];
#pragma unroll
    for (int k = 0; k < NV; k += 2) {
        chan_reduce(v[k], v[k + 1], C, m, pair_out, scr, scr2);
        __syncthreads();
        if ((int)threadIdx.x < C) { res[threadIdx.x * NV + k] = pair_out[threadIdx.x * 2]; res[threadIdx.x * NV + k + 1] = pair_out[threadIdx.x * 2 + 1]; }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ conv forward (tiled)
struct ConvFwdTArgs { ConvFwdArgs a; int S; int ngroups; int sh_in; int sh_out; };

template <bool BIG>
__global__ __launch_bounds__(256) void conv_fwd_tiled_kernel(ConvFwdTArgs t) {
    extern __shared__ __attribute__((aligned(16))) float dyn[];
    __shared__ ViewStats vs;
    __shared__ float s_w[1024 + CV_MAXC];
    __shared__ double scr[512], scr2[2 * CT_MAXCH * 8];
    const ConvFwdArgs& a = t.a;
    const raae_conv_t& cv = a.cv;
    const int cig = cv.Cin / cv.groups, cog = cv.Cout / cv.groups;
    const int nW = cv.transposed ? cv.Cin * cog * cv.K : cv.Cout * cig * cv.K;
    view_prologue(a.in, cv.Cin, &vs, blockIdx.x == 0);
    for (int i = threadIdx.x; i < nW; i += 256) s_w[i] = a.w[i];
    for (int i = threadIdx.x; i < cv.Cout; i += 256) s_w[1024 + i] = a.bias[i];
    __syncthreads();
    const int pad = cv.transposed ? 0 : cv.pad;
    const int Lp = cv.Lin + 2 * pad;
    const ChanMap m = chan_map(cv.Cout);
    const int co = m.c, g = m.active ? co / cog : 0, col = co - g * cog;
    const float bias = m.active ? s_w[1024 + co] : 0.f;
    const float oslope = (m.active && a.stats_kind == RAAE_OUT_STATS_PRELU) ? a.out_slope[co] : 1.f;
    double s_acc = 0.0, q_acc = 0.0;
    for (int grp = blockIdx.x; grp < t.ngroups; grp += gridDim.x) {
        const int b0 = grp * t.S, nb = min(t.S, a.B - b0);
        __syncthreads();
        stage_view_tile<BIG>(dyn, a.in, &vs, cv.Cin, cv.Lin, t.sh_in, pad, cv.pad_replicate, b0, nb);
        __syncthreads();
        if (!m.active) continue;
        const int n = nb * cv.Lout;
        for (int q = m.j; q < n; q += m.tpc) {
            int s, l;
            split(q, cv.Lout, t.sh_out, &s, &l);
            float acc = bias;
            const float* xs = dyn + (s * cv.Cin + g * cig) * Lp;
            if (cv.transposed) {
                const int li = l / cv.stride, tt = l - li * cv.stride;
                const float* wr = s_w + ((g * cig) * cog + col) * cv.K + tt;
                for (int cil = 0; cil < cig; ++cil) acc += wr[cil * cog * cv.K] * xs[cil * Lp + li];
            } else {
                const float* wr = s_w + co * cig * cv.K;
                const float* xr = xs + l * cv.stride;
                for (int cil = 0; cil < cig; ++cil) {
                    for (int tt = 0; tt < cv.K; ++tt) acc += wr[tt] * xr[tt];
                    wr += cv.K; xr += Lp;
                }
            }
            float o = acc;
            if (a.act == RAAE_OUT_SOFTPLUS) o = raae::softplus2(acc);
            else if (a.act == RAAE_OUT_RELU) o = fmaxf(acc, 0.f);
            a.out[((size_t)(b0 + s) * cv.Cout + co) * cv.Lout + l] = o;
            if (a.stats_kind != RAAE_OUT_RAW) {
                const float v = (a.stats_kind == RAAE_OUT_STATS_PRELU) ? prelu(acc, oslope) : acc;
                s_acc += (double)v; q_acc += (double)v * (double)v;
            }
        }
    }
    if (a.stats_kind != RAAE_OUT_RAW)
        chan_reduce(s_acc, q_acc, cv.Cout, m, a.out_partials + (size_t)blockIdx.x * cv.Cout * 2, scr, scr2);
}

// ------------------------------------------------------------------ conv backward data (tiled)
struct ConvBwdDataTArgs { ConvBwdDataArgs a; int S; int ngroups; int sh_in; int sh_out; };

template <bool BIG>
__global__ __launch_bounds__(256) void conv_bwd_data_tiled_kernel(ConvBwdDataTArgs t) {
    extern __shared__ __attribute__((aligned(16))) float dyn[];
    __shared__ ViewStats vs;
    __shared__ GradStats gs;
    __shared__ float s_w[1024];
    __shared__ double scr[512], scr2[2 * CT_MAXCH * 8];
    const ConvBwdDataArgs& a = t.a;
    const raae_conv_t& cv = a.cv;
    const int cig = cv.Cin / cv.groups, cog = cv.Cout / cv.groups;
    const int nW = cv.transposed ? cv.Cin * cog * cv.K : cv.Cout * cig * cv.K;
    view_grad_prologue(a.in, cv.Cin, &vs, a.go, cv.Cout, &gs);
    for (int i = threadIdx.x; i < nW; i += 256) s_w[i] = a.w[i];
    __syncthreads();
    const ChanMap m = chan_map(cv.Cin);
    const int ci = m.c, g = m.active ? ci / cig : 0, cil = ci - g * cig;
    double s_acc = 0.0, q_acc = 0.0;
    for (int grp = blockIdx.x; grp < t.ngroups; grp += gridDim.x) {
        const int b0 = grp * t.S, nb = min(t.S, a.B - b0);
        __syncthreads();
        stage_grad_tile<BIG>(dyn, nullptr, a.go, &gs, cv.Cout, cv.Lout, t.sh_out, b0, nb);
        __syncthreads();
        if (!m.active) continue;
        const int n = nb * cv.Lin;
        for (int q = m.j; q < n; q += m.tpc) {
            int s, li;
            split(q, cv.Lin, t.sh_in, &s, &li);
            float acc = 0.f;
            const float* gsm = dyn + (s * cv.Cout + g * cog) * cv.Lout;
            if (cv.transposed) {
                const float* gr = gsm + li * cv.stride;
                const float* wr = s_w + ci * cog * cv.K;
                for (int col = 0; col < cog; ++col) {
                    for (int tt = 0; tt < cv.K; ++tt) acc += wr[tt] * gr[tt];
                    wr += cv.K; gr += cv.Lout;
                }
            } else {
                int p0 = li + cv.pad, p1 = li + cv.pad;
                if (cv.pad_replicate) {
                    if (li == 0) p0 = 0;
                    if (li == cv.Lin - 1) p1 = cv.Lin - 1 + 2 * cv.pad;
                }
                for (int p = p0; p <= p1; ++p) {
                    // outputs l with l*stride + t = p, 0 <= t < K  =>  l in [ceil((p-K+1)/s), floor(p/s)]
                    int lmax = p / cv.stride;
                    int lmin = p - cv.K + 1;
                    lmin = lmin <= 0 ? 0 : (lmin + cv.stride - 1) / cv.stride;
                    if (lmax > cv.Lout - 1) lmax = cv.Lout - 1;
                    const float* gr = gsm;
                    const float* wr = s_w + (g * cog * cig + cil) * cv.K + (p - lmin * cv.stride);
                    for (int col = 0; col < cog; ++col) {
                        int wo = 0;
                        for (int l = lmin; l <= lmax; ++l, wo -= cv.stride) acc += wr[wo] * gr[l];
                        gr += cv.Lout; wr += cig * cv.K;
                    }
                }
            }
            const size_t idx = ((size_t)(b0 + s) * cv.Cin + ci) * cv.Lin + li;
            if (a.in.mask) acc *= a.in.mask[idx];
            if (a.accumulate) acc += a.din[idx];
            a.din[idx] = acc;
            if (a.din_partials) {
                const float y = view_y(a.in, &vs, ci, idx);
                s_acc += (double)acc; q_acc += (double)acc * (double)y;
            }
        }
    }
    if (a.din_partials)
        chan_reduce(s_acc, q_acc, cv.Cin, m, a.din_partials + (size_t)blockIdx.x * cv.Cin * 2, scr, scr2);
}


// Weight gradient of a non-transposed conv by (output channel, input channel) PAIR: the lanes of a pair take
// blocks of four consecutive output positions; per block the K + 3*stride input window and four gradients
// are read once and feed 4*K multiply-adds into K register accumulators (0.45 LDS reads per multiply-add; the
// one-thread-per-weight loop needs 2).  acc[t] += sum_{s, l in this lane's blocks} g[s][l] * x[s][l*S + t].
template <int K, int S>
__device__ __forceinline__ void wgrad_pair_blocks(const float* Gt, const float* Xt, int nb, int gper, int xper, int span,
                                                  int part, int lpp, float (&acc)[K]) {
    for (int s = 0; s < nb; ++s) {
        const float* g = Gt + s * gper;
        const float* x = Xt + s * xper;
        for (int l0 = part * 4; l0 < span; l0 += 4 * lpp) {
            if (l0 + 4 <= span) {
                float gv[4], xw[K + 3 * S];
#pragma unroll
                for (int r = 0; r < 4; ++r) gv[r] = g[l0 + r];
#pragma unroll
                for (int i = 0; i < K + 3 * S; ++i) xw[i] = x[l0 * S + i];
#pragma unroll
                for (int t = 0; t < K; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[t] = fmaf(gv[r], xw[r * S + t], acc[t]);
            } else {
                for (int l = l0; l < span; ++l) {
                    const float gv = g[l];
#pragma unroll
                    for (int t = 0; t < K; ++t) acc[t] = fmaf(gv, x[l * S + t], acc[t]);
                }
            }
        }
    }
}

// ------------------------------------------------------------------ conv backward weights (tiled, slabs)
struct ConvBwdWTArgs { ConvBwdWArgs a; int S; int ngroups; long slab_stride; int sh_in; int sh_out; };

// thread e (+256 j) owns weight element e; the channel mapping sums dbias / dslope.
// (bid, nblk) = this workgroup's index / count within the task (a task may be one of several in a launch).
// KIND >= 0 / WHICH in 1..4: the conv is cv1 / cv2 / cve / cvs of block shape kBlk[KIND] -- a compile-time constant
// (pair path, tap counts and index splits fold); otherwise it is read from the arguments.
#if defined(RAAE_STAMPS) && defined(RAAE_STAMPS_WGRAD)
// per-stage clock of the FIRST workgroup of weight-gradient task t (t < 4) of a launch into stamp slot t
// (tools/stamps.py); only the instance of block shape RAAE_STAMP_WKIND records; the block kernels' stamps are off
#ifndef RAAE_STAMP_WKIND
#define RAAE_STAMP_WKIND 6
#endif
__shared__ int s_wslot;
#define WSTAMP(i) do { __syncthreads(); if (threadIdx.x == 0 && s_wslot >= 0 && s_wslot < 4) { \
        const long long now_ = wall_clock64(); const int gc_ = 2, k_ = s_wslot; d_stamps[k_][gc_][i] = now_; \
        if ((i) > 0) { d_stage_sum[k_][gc_][i] += (unsigned long long)(now_ - d_stage_prev[k_]); d_stage_cnt[k_][gc_][i] += 1ull; } \
        d_stage_prev[k_] = now_; } } while (0)
#else
#define WSTAMP(i)
#endif
template <int KIND = -1, int WHICH = 0, bool BIG = false>
__device__ __forceinline__ void conv_bwd_weight_task(const ConvBwdWTArgs& t, const int bid, const int nblk, float* dyn) {
    __shared__ ViewStats vs;
    __shared__ GradStats gs;
    __shared__ double scr[512], scr2[2 * CT_MAXCH * 8], res[2 * CT_MAXCH];
    const ConvBwdWArgs& a = t.a;
    constexpr int KB = KIND < 0 ? 0 : KIND;
    const raae_conv_t cv = (KIND >= 0 && WHICH == 1) ? kBlk[KB].cv1 : (KIND >= 0 && WHICH == 2) ? kBlk[KB].cv2 :
                           (KIND >= 0 && WHICH == 3) ? kBlk[KB].cve : (KIND >= 0 && WHICH == 4) ? kBlk[KB].cvs : a.cv;
    const int sh_in = (KIND >= 0 && WHICH > 0) ? clg2(cv.Lin) : t.sh_in, sh_out = (KIND >= 0 && WHICH > 0) ? clg2(cv.Lout) : t.sh_out;
    const int cig = cv.Cin / cv.groups, cog = cv.Cout / cv.groups;
    WSTAMP(0);
    view_grad_prologue(a.in, cv.Cin, &vs, a.go, cv.Cout, &gs);
    WSTAMP(1);
    const int pad = cv.transposed ? 0 : cv.pad;
    const int Lp = cv.Lin + 2 * pad;
    float* Gt = dyn;                                         // [S][Cout][Lout]
    float* At = Gt + t.S * cv.Cout * cv.Lout;                // [S][Cout][Lout]  dA*raw[raw<=0]
    float* Xt = At + (a.dslope ? t.S * cv.Cout * cv.Lout : 0);   // [S][Cin][Lp]
    double wacc[4] = {0.0, 0.0, 0.0, 0.0};
    int e_go[4], e_xo[4];        // offsets inside one sample of Gt / Xt (channel row + tap); -1 = none
    // Few weights (nw <= 128): P = 256 / nextpow2(nw) lanes share a weight element, lane `part` takes the
    // positions part, part+P, ... and an xor-shuffle tree joins them (the 4 -> 1 head conv has 4 weights:
    // one thread per weight left 252 lanes idle behind a 65 536-term dot product).
    int P = 1;
    if (a.nw <= 128) { int np = 1; while (np < a.nw) np <<= 1; P = 256 / np; }
    const int part = threadIdx.x & (P - 1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = P > 1 ? (j == 0 ? (int)(threadIdx.x / P) : a.nw) : (int)threadIdx.x + 256 * j;
        e_go[j] = -1; e_xo[j] = 0;
        if (e < a.nw) {
            int co, ci, tt;
            if (cv.transposed) {
                tt = e % cv.K; const int col = (e / cv.K) % cog; ci = e / (cv.K * cog);
                co = (ci / cig) * cog + col;
                e_go[j] = co * cv.Lout + tt; e_xo[j] = ci * Lp;
            } else {
                tt = e % cv.K; const int cil = (e / cv.K) % cig; co = e / (cv.K * cig);
                ci = (co / cog) * cig + cil;
                e_go[j] = co * cv.Lout; e_xo[j] = ci * Lp + tt;
            }
        }
    }
    const int gper = cv.Cout * cv.Lout, xper = cv.Cin * Lp;
    const int span = cv.transposed ? cv.Lin : cv.Lout;
    const ChanMap m = chan_map(cv.Cout);
    double bacc = 0.0, sacc = 0.0;
    // ---- pair path (non-transposed convs with a template instance for their K and stride)
    const int ks = cv.transposed ? -1 : cv.K * 16 + cv.stride;
    const int npair = cv.Cout * cig;
    int lpp = 1;
    { int np2 = 1; while (np2 < npair) np2 <<= 1; lpp = 256 / np2; }
    // worth it when a pair has >= 16 lanes (butterfly join) and every lane gets at least one block of positions
    const bool by_pair = (ks == 11 * 16 + 1 || ks == 11 * 16 + 2 || ks == 7 * 16 + 2 || ks == 5 * 16 + 1 ||
                          ks == 5 * 16 + 2 || ks == 4 * 16 + 4 || ks == 2 * 16 + 2 || ks == 1 * 16 + 1) &&
                         lpp >= 16 && span >= 4 * lpp;
    const int pair = threadIdx.x / lpp, ppart = threadIdx.x - pair * lpp;
    const int pco = pair / cig, pci = (pco / cog) * cig + (pair - pco * cig);
    double pacc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) pacc[i] = 0.0;
    WSTAMP(2);
    for (int grp = bid; grp < t.ngroups; grp += nblk) {
        const int b0 = grp * t.S, nb = min(t.S, a.B - b0);
        __syncthreads();
        stage_grad_tile<BIG>(Gt, a.dslope ? At : nullptr, a.go, &gs, cv.Cout, cv.Lout, sh_out, b0, nb);
        stage_view_tile<BIG>(Xt, a.in, &vs, cv.Cin, cv.Lin, sh_in, pad, cv.pad_replicate, b0, nb);
        __syncthreads();
        WSTAMP(3);
        if (by_pair) {
            if (pair < npair) {
                const float* gp = Gt + pco * cv.Lout;
                const float* xp = Xt + pci * Lp;
#define RAAE_WG_CASE(K_, S_) case K_ * 16 + S_: { float acc[K_]; \
                    _Pragma("unroll") for (int i = 0; i < K_; ++i) acc[i] = 0.f; \
                    wgrad_pair_blocks<K_, S_>(gp, xp, nb, gper, xper, span, ppart, lpp, acc); \
                    _Pragma("unroll") for (int i = 0; i < K_; ++i) pacc[i] += (double)acc[i]; } break;
                switch (ks) {
                    RAAE_WG_CASE(11, 1) RAAE_WG_CASE(11, 2) RAAE_WG_CASE(7, 2) RAAE_WG_CASE(5, 1) RAAE_WG_CASE(5, 2)
                    RAAE_WG_CASE(4, 4) RAAE_WG_CASE(2, 2) RAAE_WG_CASE(1, 1)
                    default: break;          // by_pair is false for every other (K, stride)
                }
#undef RAAE_WG_CASE
            }
        } else
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (e_go[j] < 0) continue;
            float acc = 0.f;
            const float* gr = Gt + e_go[j];
            const float* xr = Xt + e_xo[j];
            for (int sidx = 0; sidx < nb; ++sidx) {
                if (cv.transposed) {
#pragma unroll 4
                    for (int li = part; li < span; li += P) acc += xr[li] * gr[li * cv.stride];
                } else {
#pragma unroll 4
                    for (int l = part; l < span; l += P) acc += gr[l] * xr[l * cv.stride];
                }
                gr += gper; xr += xper;
            }
            wacc[j] += (double)acc;
        }
        WSTAMP(4);
        if (m.active) {           // dbias / dslope of channel m.c
            float fb = 0.f, fs = 0.f;
            const int n = nb * cv.Lout;
            for (int q = m.j; q < n; q += m.tpc) {
                int s, l;
                split(q, cv.Lout, sh_out, &s, &l);
                const int o = (s * cv.Cout + m.c) * cv.Lout + l;
                fb += Gt[o];
                if (a.dslope) fs += At[o];
            }
            bacc += (double)fb; sacc += (double)fs;
        }
    }
    WSTAMP(5);
    const size_t slab = (size_t)bid * (size_t)t.slab_stride;
    if (by_pair) {
        // join the lanes of a pair (lpp consecutive lanes, 4 <= lpp <= 64 because Cout * Cin/groups <= 64)
        raae::group_multi_sum<16>(pacc, threadIdx.x & 63, lpp);
        const int tt = raae::group_multi_slot<16>(threadIdx.x & 63);
        if (ppart < 16 && tt < cv.K && pair < npair) a.dw[slab + pair * cv.K + tt] = (float)pacc[0];
    } else if (P > 1) {
        double w0 = wacc[0];
        for (int o = P >> 1; o > 0; o >>= 1) w0 += __shfl_xor(w0, o, 64);      // P <= 64: inside one wave
        const int e = threadIdx.x / P;
        if (part == 0 && e < a.nw) a.dw[slab + e] = (float)w0;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = threadIdx.x + 256 * j;
            if (e < a.nw) a.dw[slab + e] = (float)wacc[j];
        }
    }
    WSTAMP(6);
    chan_reduce(bacc, sacc, cv.Cout, m, res, scr, scr2);
    __syncthreads();
    if (threadIdx.x < cv.Cout) {
        a.dbias[slab + threadIdx.x] = (float)res[threadIdx.x * 2];
        if (a.dslope) a.dslope[slab + threadIdx.x] = (float)res[threadIdx.x * 2 + 1];
    }
    WSTAMP(7);
}

template <bool BIG>
__global__ __launch_bounds__(256) void conv_bwd_weight_tiled_kernel(ConvBwdWTArgs t) {
    extern __shared__ __attribute__((aligned(16))) float dyn[];
#if defined(RAAE_STAMPS) && defined(RAAE_STAMPS_WGRAD)
    if (threadIdx.x == 0) s_wslot = -1;
    __syncthreads();
#endif
    conv_bwd_weight_task<-1, 0, BIG>(t, blockIdx.x, gridDim.x, dyn);
}

// ------------------------------------------------------------------ length-axis Linear (tiled)
struct LenLinFwdTArgs { LenLinFwdArgs a; int S; int ngroups; int sh_in; int sh_e; };

template <bool BIG>
__global__ __launch_bounds__(256) void lenlin_fwd_tiled_kernel(LenLinFwdTArgs t) {
    extern __shared__ __attribute__((aligned(16))) float dyn[];
    __shared__ ViewStats vs;
    __shared__ double scr[512], scr2[2 * CT_MAXCH * 8];
    const LenLinFwdArgs& a = t.a;
    view_prologue(a.in, a.C, &vs, blockIdx.x == 0);
    float* Xt = dyn;                                   // [S][C][Lin]
    float* Wt = Xt + t.S * a.C * a.Lin;                // [E][Lin] + bias[E]
    for (int i = threadIdx.x; i < a.E * a.Lin; i += 256) Wt[i] = a.w[i];
    for (int i = threadIdx.x; i < a.E; i += 256) Wt[a.E * a.Lin + i] = a.bias[i];
    const ChanMap m = chan_map(a.C);
    const float oslope = (m.active && a.stats_kind == RAAE_OUT_STATS_PRELU) ? a.out_slope[m.c] : 1.f;
    double s_acc = 0.0, q_acc = 0.0;
    // long contraction with few outputs: `sub` lanes cooperate on one output (sub = 16 when Lin >= 64)
    const int sub = (a.Lin >= 64 && (m.tpc & 15) == 0) ? 16 : 1;
    const int jj = m.j / sub, lane_sub = m.j - jj * sub, tpo = m.tpc / sub;     // outputs in flight per channel
    for (int grp = blockIdx.x; grp < t.ngroups; grp += gridDim.x) {
        const int b0 = grp * t.S, nb = min(t.S, a.B - b0);
        __syncthreads();
        stage_view_tile<BIG>(Xt, a.in, &vs, a.C, a.Lin, t.sh_in, 0, 0, b0, nb);
        __syncthreads();
        if (!m.active) continue;
        const int n = nb * a.E;                        // outputs of this channel: (s, e)
        const int nloop = (n + tpo - 1) / tpo;
        for (int it = 0; it < nloop; ++it) {
            const int q = jj + it * tpo;
            const bool ok = q < n && jj < tpo;
            int s = 0, e = 0;
            if (ok) split(q, a.E, t.sh_e, &s, &e);
            const float* xr = Xt + (s * a.C + m.c) * a.Lin;
            const float* wr = Wt + e * a.Lin;
            float acc = 0.f;
            if (ok) for (int l = lane_sub; l < a.Lin; l += sub) acc += wr[l] * xr[l];
            if (sub == 16) {
                acc += __shfl_xor(acc, 1, 64); acc += __shfl_xor(acc, 2, 64);
                acc += __shfl_xor(acc, 4, 64); acc += __shfl_xor(acc, 8, 64);
            }
            if (ok && lane_sub == 0) {
                acc += Wt[a.E * a.Lin + e];
                a.out[((size_t)(b0 + s) * a.C + m.c) * a.E + e] = acc;
                if (a.stats_kind != RAAE_OUT_RAW) {
                    const float v = (a.stats_kind == RAAE_OUT_STATS_PRELU) ? prelu(acc, oslope) : acc;
                    s_acc += (double)v; q_acc += (double)v * (double)v;
                }
            }
        }
    }
    if (a.stats_kind != RAAE_OUT_RAW)
        chan_reduce(s_acc, q_acc, a.C, m, a.out_partials + (size_t)blockIdx.x * a.C * 2, scr, scr2);
}

struct LenLinBwdDataTArgs { LenLinBwdDataArgs a; int S; int ngroups; int sh_in; int sh_e; };

template <bool BIG>
__global__ __launch_bounds__(256) void lenlin_bwd_data_tiled_kernel(LenLinBwdDataTArgs t) {
    extern __shared__ __attribute__((aligned(16))) float dyn[];
    __shared__ ViewStats vs;
    __shared__ GradStats gs;
    __shared__ double scr[512], scr2[2 * CT_MAXCH * 8];
    const LenLinBwdDataArgs& a = t.a;
    view_grad_prologue(a.in, a.C, &vs, a.go, a.C, &gs);
    float* Gt = dyn;                                   // [S][C][E]
    float* Wt = Gt + t.S * a.C * a.E;                  // [E][Lin]
    for (int i = threadIdx.x; i < a.E * a.Lin; i += 256) Wt[i] = a.w[i];
    const ChanMap m = chan_map(a.C);
    double s_acc = 0.0, q_acc = 0.0;
    const int sub = (a.E >= 64 && (m.tpc & 15) == 0) ? 16 : 1;    // long contraction over e: 16 lanes per output
    const int jj = m.j / sub, lane_sub = m.j - jj * sub, tpo = m.tpc / sub;
    for (int grp = blockIdx.x; grp < t.ngroups; grp += gridDim.x) {
        const int b0 = grp * t.S, nb = min(t.S, a.B - b0);
        __syncthreads();
        stage_grad_tile<BIG>(Gt, nullptr, a.go, &gs, a.C, a.E, t.sh_e, b0, nb);
        __syncthreads();
        if (!m.active) continue;
        const int n = nb * a.Lin;                      // outputs of this channel: (s, l)
        const int nloop = (n + tpo - 1) / tpo;
        for (int it = 0; it < nloop; ++it) {
            const int q = jj + it * tpo;
            const bool ok = q < n && jj < tpo;
            int s = 0, l = 0;
            if (ok) split(q, a.Lin, t.sh_in, &s, &l);
            const float* gr = Gt + (s * a.C + m.c) * a.E;
            float acc = 0.f;
            if (ok) for (int e = lane_sub; e < a.E; e += sub) acc += Wt[e * a.Lin + l] * gr[e];
            if (sub == 16) {
                acc += __shfl_xor(acc, 1, 64); acc += __shfl_xor(acc, 2, 64);
                acc += __shfl_xor(acc, 4, 64); acc += __shfl_xor(acc, 8, 64);
            }
            if (ok && lane_sub == 0) {
                const size_t idx = ((size_t)(b0 + s) * a.C + m.c) * a.Lin + l;
                if (a.in.mask) acc *= a.in.mask[idx];
                if (a.accumulate) acc += a.din[idx];
                a.din[idx] = acc;
                if (a.din_partials) {
                    const float y = view_y(a.in, &vs, m.c, idx);
                    s_acc += (double)acc; q_acc += (double)acc * (double)y;
                }
            }
        }
    }
    if (a.din_partials)
        chan_reduce(s_acc, q_acc, a.C, m, a.din_partials + (size_t)blockIdx.x * a.C * 2, scr, scr2);
}

struct LenLinBwdWTArgs { LenLinBwdWArgs a; int S; int ngroups; long slab_stride; int sh_in; int sh_e; };

// thread x (+256 j) owns dW element x = e*Lin + l; thread e < E owns dbias[e]; channel map sums dslope[c].
template <bool BIG = false>
__device__ __forceinline__ void lenlin_bwd_weight_task(const LenLinBwdWTArgs& t, const int bid, const int nblk, float* dyn) {
    __shared__ ViewStats vs;
    __shared__ GradStats gs;
    __shared__ double scr[512], scr2[2 * CT_MAXCH * 8], res[2 * CT_MAXCH];
    const LenLinBwdWArgs& a = t.a;
    WSTAMP(0);
    view_grad_prologue(a.in, a.C, &vs, a.go, a.C, &gs);
    WSTAMP(1);
    float* Gt = dyn;                                        // [S][C][E]
    float* At = Gt + t.S * a.C * a.E;                       // [S][C][E]
    float* Xt = At + (a.dslope ? t.S * a.C * a.E : 0);      // [S][C][Lin]
    const int nw = a.E * a.Lin;
    double wacc[4] = {0.0, 0.0, 0.0, 0.0};
    double bacc = 0.0, sacc = 0.0;
    int w_e[4], w_l[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = threadIdx.x + 256 * j;
        w_e[j] = -1; w_l[j] = 0;
        if (x < nw) split(x, a.Lin, t.sh_in, &w_e[j], &w_l[j]);
    }
    const ChanMap m = chan_map(a.C);
    for (int grp = bid; grp < t.ngroups; grp += nblk) {
        const int b0 = grp * t.S, nb = min(t.S, a.B - b0);
        __syncthreads();
        stage_grad_tile<BIG>(Gt, a.dslope ? At : nullptr, a.go, &gs, a.C, a.E, t.sh_e, b0, nb);
        stage_view_tile<BIG>(Xt, a.in, &vs, a.C, a.Lin, t.sh_in, 0, 0, b0, nb);
        __syncthreads();
        WSTAMP(3);
        const int rows = nb * a.C;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (w_e[j] < 0) continue;
            float acc = 0.f;
            const float* gr = Gt + w_e[j];
            const float* xr = Xt + w_l[j];
#pragma unroll 4
            for (int r = 0; r < rows; ++r) acc += gr[r * a.E] * xr[r * a.Lin];
            wacc[j] += (double)acc;
        }
        if (threadIdx.x < a.E) {
            float acc = 0.f;
            for (int r = 0; r < rows; ++r) acc += Gt[r * a.E + threadIdx.x];
            bacc += (double)acc;
        }
        if (a.dslope && m.active) {
            float fs = 0.f;
            const int n = nb * a.E;
            for (int q = m.j; q < n; q += m.tpc) {
                int s, e;
                split(q, a.E, t.sh_e, &s, &e);
                fs += At[(s * a.C + m.c) * a.E + e];
            }
            sacc += (double)fs;
        }
        WSTAMP(4);
    }
    WSTAMP(5);
    const size_t slab = (size_t)bid * (size_t)t.slab_stride;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = threadIdx.x + 256 * j;
        if (x < nw) a.dw[slab + x] = (float)wacc[j];
    }
    if (threadIdx.x < a.E) a.dbias[slab + threadIdx.x] = (float)bacc;
    if (a.dslope) {
        chan_reduce(sacc, 0.0, a.C, m, res, scr, scr2);
        __syncthreads();
        if (threadIdx.x < a.C) a.dslope[slab + threadIdx.x] = (float)res[threadIdx.x * 2];
    }
}

template <bool BIG>
__global__ __launch_bounds__(256) void lenlin_bwd_weight_tiled_kernel(LenLinBwdWTArgs t) {
    extern __shared__ __attribute__((aligned(16))) float dyn[];
#if defined(RAAE_STAMPS) && defined(RAAE_STAMPS_WGRAD)
    if (threadIdx.x == 0) s_wslot = -1;
    __syncthreads();
#endif
    lenlin_bwd_weight_task<BIG>(t, blockIdx.x, gridDim.x, dyn);
}

// Several independent weight-gradient tasks of one residual block in ONE launch: workgroup ranges
// [first[t], first[t+1]) run task t.  All tasks overlap on the chip and share a single launch.
struct WgradMultiArgs { int ntask; int first[7]; int is_conv[6]; int idx[6]; int which[4]; ConvBwdWTArgs conv[4]; LenLinBwdWTArgs lin[2]; };

// `bx`: the workgroup's index among the workgroups of this multi-task launch
template <int KIND, bool BIG = false>
__device__ __forceinline__ void wgrad_multi_body(const WgradMultiArgs& m, const int bx, float* dyn) {
    int t = 0;
    while (t + 1 < m.ntask && bx >= m.first[t + 1]) ++t;
    const int bid = bx - m.first[t], nblk = m.first[t + 1] - m.first[t];
#if defined(RAAE_STAMPS) && defined(RAAE_STAMPS_WGRAD)
    if (threadIdx.x == 0) s_wslot = (bid == 0 && KIND == RAAE_STAMP_WKIND && BIG) ? t : -1;
    __syncthreads();
#endif
    if (m.is_conv[t]) {
        const ConvBwdWTArgs& ct = m.conv[m.idx[t]];
        if (KIND >= 0) {
            constexpr int KB = KIND < 0 ? 0 : KIND;
            const int which = __builtin_amdgcn_readfirstlane(m.which[m.idx[t]]);
            if (which == 1) conv_bwd_weight_task<KIND, 1, BIG>(ct, bid, nblk, dyn);
            else if (which == 2) conv_bwd_weight_task<KIND, 2, BIG>(ct, bid, nblk, dyn);
            else if (which == 3) { if constexpr (kBlk[KB].has_excit != 0) conv_bwd_weight_task<KIND, 3, BIG>(ct, bid, nblk, dyn); }
            else { if constexpr (kBlk[KB].has_short != 0) conv_bwd_weight_task<KIND, 4, BIG>(ct, bid, nblk, dyn); }
        } else {
            conv_bwd_weight_task<-1, 0, BIG>(ct, bid, nblk, dyn);
        }
    } else {
        lenlin_bwd_weight_task<BIG>(m.lin[m.idx[t]], bid, nblk, dyn);
    }
}

template <int KIND, bool BIG = false>
__global__ __launch_bounds__(256) void wgrad_multi_kernel(WgradMultiArgs km) {
    extern __shared__ __attribute__((aligned(16))) float dyn[];
    __shared__ WgradMultiArgs sm;
    const WgradMultiArgs& m = raae::args_to_lds(&sm);
    wgrad_multi_body<KIND, BIG>(m, blockIdx.x, dyn);
}
template <int KIND, bool BIG = false>
__global__ __launch_bounds__(256) void wgrad_multi_kernel_m(const WgradMultiArgs* table) {     // one trial per grid plane
    extern __shared__ __attribute__((aligned(16))) float dyn[];
    __shared__ WgradMultiArgs sm;
    const WgradMultiArgs& m = raae::args_from_table(&sm, table);
    wgrad_multi_body<KIND, BIG>(m, blockIdx.x, dyn);
}

// ------------------------------------------------------------------ grad materialise (sliced)
struct GradMatTArgs { GradMatArgs a; int nsl; long slab_stride; };

__global__ __launch_bounds__(256) void grad_materialize_sliced_kernel(GradMatTArgs t) {
    __shared__ GradStats gs;
    __shared__ double shd[16];
    const GradMatArgs& a = t.a;
    const int c = blockIdx.x % a.C, sl = blockIdx.x / a.C;
    grad_prologue(a.go, a.C, &gs);
    long lo, hi;
    slice_range((long)a.B * a.L, t.nsl, sl, &lo, &hi);
    double acc = 0.0;
    for (long i = lo + threadIdx.x; i < hi; i += 256) {
        const int b = (int)(i / a.L), l = (int)(i - (long)b * a.L);
        const size_t idx = ((size_t)b * a.C + c) * a.L + l;
        float da, raw;
        const float dr = grad_at(a.go, &gs, c, idx, &da, &raw);
        if (a.draw) a.draw[idx] = a.accumulate ? a.draw[idx] + dr : dr;
        if (raw <= 0.f) acc += (double)da * (double)raw;
    }
    if (a.dslope) {
        const double tot = raae::block_sum(acc, shd);
        if (threadIdx.x == 0) a.dslope[(size_t)sl * t.slab_stride + c] = (float)tot;
    }
}
