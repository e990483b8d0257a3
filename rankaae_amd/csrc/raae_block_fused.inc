// Fused residual-block FORWARD kernels (included inside raae_conv.hip's anonymous namespace).
// BatchNorm (batch statistics) is the only grid-wide dependency inside an Encoding/DecodingBlock
// (reference sc/clustering/model.py:24-174), so a block's forward is exactly two kernels:
//   A:  R = bn1(X) staged once per sample ->  T1 = conv1(R) (+stats of PReLU1)      [needs bn1 stats]
//                                              Sh = conv_short(R)
//                                              E1 = fc1(dropout(R)); E2 = fc2(PReLU(E1)) (+stats)
//   B:  T2 = conv2(bn2(PReLU1(T1)));  E3 = conv_excit(bn_e(PReLU(E2)))              [needs bn2 / bn_e stats]
//       Y  = PReLU2(T2) + PReLUs(Sh) | R + PReLUe(E3 | E2)   (+stats of Y for the next BatchNorm)
// Same LDS-tile / channel-bound-thread scheme as raae_conv_tiled.inc.

// one conv / convT output from a staged tile row set.  tile rows have pitch Lp and a halo of `halo`
// elements on the left; `xs` points at channel 0 of the sample; w in torch layout (staged in LDS).
__device__ __forceinline__ float conv_out(const raae_conv_t& cv, const float* w, const float* xs, int Lp, int halo,
                                          int co, int l) {
    const int cig = cv.Cin / cv.groups, cog = cv.Cout / cv.groups;
    const int g = co / cog, col = co - g * cog;
    float acc = 0.f;
    if (cv.transposed) {
        const int li = l / cv.stride, tt = l - li * cv.stride;
        const float* wr = w + ((g * cig) * cog + col) * cv.K + tt;
        const float* xr = xs + (g * cig) * Lp + halo + li;
        for (int cil = 0; cil < cig; ++cil) acc += wr[cil * cog * cv.K] * xr[cil * Lp];
    } else {
        const float* wr = w + co * cig * cv.K;
        const float* xr = xs + (g * cig) * Lp + halo - cv.pad + l * cv.stride;
        for (int cil = 0; cil < cig; ++cil) {
            for (int tt = 0; tt < cv.K; ++tt) acc += wr[tt] * xr[tt];
            wr += cv.K; xr += Lp;
        }
    }
    return acc;
}


// Copy up to four weight arrays global -> LDS with all first-round loads in flight together (four separate
// copy loops are four dependent memory round trips at the head of a ten-microsecond kernel) -- in two halves:
// weights4_issue() requests the first round BEFORE the kernel's statistic prologue, weights4_commit() stores it to
// LDS behind the prologue, so that the round trip of the weights is spent inside the prologue's own (stage stamps at
// 256 rows: 0.6-1.3 us per kernel for the copy when it followed the prologue).
struct WeightRegs { float v0, v1, v2, v3, u2, u3; };
__device__ __forceinline__ WeightRegs weights4_issue(const float* s0, int n0, const float* s1, int n1, const float* s2, int n2,
                                                     const float* s3, int n3) {
    const int t = threadIdx.x;
    WeightRegs r;
    r.v0 = t < n0 ? s0[t] : 0.f; r.v1 = t < n1 ? s1[t] : 0.f; r.v2 = t < n2 ? s2[t] : 0.f; r.v3 = t < n3 ? s3[t] : 0.f;
    // second round of the (usually longer) last two arrays rides along
    r.u2 = t + 256 < n2 ? s2[t + 256] : 0.f; r.u3 = t + 256 < n3 ? s3[t + 256] : 0.f;
    return r;
}
__device__ __forceinline__ void weights4_commit(const WeightRegs& r, float* d0, const float* s0, int n0, float* d1, const float* s1,
                                                int n1, float* d2, const float* s2, int n2, float* d3, const float* s3, int n3) {
    const int t = threadIdx.x;
    if (t < n0) d0[t] = r.v0;
    if (t < n1) d1[t] = r.v1;
    if (t < n2) d2[t] = r.v2;
    if (t < n3) d3[t] = r.v3;
    if (t + 256 < n2) d2[t + 256] = r.u2;
    if (t + 256 < n3) d3[t + 256] = r.u3;
    for (int i = t + 256; i < n0; i += 256) d0[i] = s0[i];
    for (int i = t + 256; i < n1; i += 256) d1[i] = s1[i];
    for (int i = t + 512; i < n2; i += 256) d2[i] = s2[i];
    for (int i = t + 512; i < n3; i += 256) d3[i] = s3[i];
}

#if defined(RAAE_STAMPS) && defined(RAAE_STAMPS_WGRAD)
#define RAAE_STAMP_KIND -3          /* no block kernel stamps: slot 0 belongs to the weight-gradient task (WSTAMP) */
#endif
#ifdef RAAE_STAMPS
// STAMP(k, i): workgroup 0 records the 100 MHz clock at stage boundary i of kernel k (last launch per grid class)
// and adds the time since its previous stamp to a running per-stage total over ALL launches (tools/stamps.py).
#ifndef RAAE_STAMP_KIND
#define RAAE_STAMP_KIND -2          /* -DRAAE_STAMP_KIND=n: only the instance of block shape n records */
#endif
#define STAMP(k, i) do { __syncthreads(); if (blockIdx.x == 0 && threadIdx.x == 0 && (RAAE_STAMP_KIND == -2 || KIND == RAAE_STAMP_KIND)) { \
        const long long now_ = wall_clock64(); \
        const int gc_ = gridDim.x <= 64 ? 0 : (gridDim.x <= 128 ? 1 : 2); \
        d_stamps[k][gc_][i] = now_; \
        if ((i) > 0) { d_stage_sum[k][gc_][i] += (unsigned long long)(now_ - d_stage_prev[k]); d_stage_cnt[k][gc_][i] += 1ull; \
                       if (gc_ == 2) { d_kind_sum[KIND < 0 ? 7 : KIND][k][i] += (unsigned long long)(now_ - d_stage_prev[k]); d_kind_cnt[KIND < 0 ? 7 : KIND][k][i] += 1ull; } } \
        d_stage_prev[k] = now_; } } while (0)
extern "C" int raae_debug_kind_totals(unsigned long long* sum, unsigned long long* cnt) {
    hipError_t e = hipMemcpyFromSymbol(sum, HIP_SYMBOL(d_kind_sum), sizeof(unsigned long long) * 8 * 4 * 16);
    if (e != hipSuccess) return (int)e;
    return (int)hipMemcpyFromSymbol(cnt, HIP_SYMBOL(d_kind_cnt), sizeof(unsigned long long) * 8 * 4 * 16);
}
extern "C" int raae_debug_stamps(long long* out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(d_stamps), sizeof(long long) * 4 * 3 * 16); }
extern "C" int raae_debug_stage_totals(unsigned long long* sum, unsigned long long* cnt) {
    hipError_t e = hipMemcpyFromSymbol(sum, HIP_SYMBOL(d_stage_sum), sizeof(unsigned long long) * 4 * 3 * 16);
    if (e != hipSuccess) return (int)e;
    return (int)hipMemcpyFromSymbol(cnt, HIP_SYMBOL(d_stage_cnt), sizeof(unsigned long long) * 4 * 3 * 16);
}
#else
#define STAMP(k, i)
#endif

// Four outputs of a (non-transposed) conv at once: independent accumulators, taps unrolled for the kernel
// sizes of the model, each weight read once for the four.  The one-output-at-a-time loop was a dependent
// chain of LDS round trips (~100 cycles per multiply-add; 8.6 us for the k=11 4->4 layer at one sample per
// workgroup).  xb[r] points at tap 0 / local input channel 0 of output r; w at this output channel's taps.
template <int K>
__device__ __forceinline__ void conv4_rows(const float* w, const float* const (&xb)[4], int Lp, int cig, float (&acc)[4]) {
    for (int cil = 0; cil < cig; ++cil) {
        float wv[K];
#pragma unroll
        for (int t = 0; t < K; ++t) wv[t] = w[cil * K + t];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float* x = xb[r] + cil * Lp;
#pragma unroll
            for (int t = 0; t < K; ++t) acc[r] = fmaf(wv[t], x[t], acc[r]);
        }
    }
}
__device__ __forceinline__ void conv4(int K, const float* w, const float* const (&xb)[4], int Lp, int cig, float (&acc)[4]) {
    switch (K) {
    case 11: conv4_rows<11>(w, xb, Lp, cig, acc); break;
    case 7: conv4_rows<7>(w, xb, Lp, cig, acc); break;
    case 5: conv4_rows<5>(w, xb, Lp, cig, acc); break;
    case 4: conv4_rows<4>(w, xb, Lp, cig, acc); break;
    case 2: conv4_rows<2>(w, xb, Lp, cig, acc); break;
    case 1: conv4_rows<1>(w, xb, Lp, cig, acc); break;
    default:
        for (int cil = 0; cil < cig; ++cil)
            for (int t = 0; t < K; ++t) {
                const float wv = w[cil * K + t];
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[r] = fmaf(wv, xb[r][cil * Lp + t], acc[r]);
            }
    }
}
// tap-0 pointer of output l of output channel co of a non-transposed conv inside a staged sample tile
__device__ __forceinline__ const float* conv_tap0(const raae_conv_t& cv, const float* xs, int Lp, int halo, int co, int l) {
    const int cig = cv.Cin / cv.groups, cog = cv.Cout / cv.groups;
    return xs + ((co / cog) * cig) * Lp + halo - cv.pad + l * cv.stride;
}

// ---- register-blocked strips for the stride-1 "same" convolutions (odd K, pad (K-1)/2, Lin == Lout: the k = 11
// 4 -> 4 layers on 256 points of the decoder's last block, reference model.py:456-459) -------------------------------
// The one-output-per-thread loops read two LDS words per multiply-add and wait for them with one wave per SIMD: at
// B = 4096 the conv loop was 16-25 us of every 4-sample group.  Here a thread takes FOUR consecutive outputs of its
// channel: per input channel the K + 3 window arrives in aligned 16-byte reads (tile rows have an 8-float margin and
// a pitch of L + 16, so every window starts on a 16-byte boundary) and feeds 4 K multiply-adds into four independent
// accumulators; the K weights of the (output, input) channel pair are wave-uniform LDS broadcasts.
__host__ __device__ constexpr bool strip_conv_ok(const raae_conv_t& cv) {
    return !cv.transposed && cv.stride == 1 && cv.groups == 1 && (cv.K & 1) && cv.K >= 3 && cv.K <= 15 &&
           cv.pad == (cv.K - 1) / 2 && cv.Lin == cv.Lout && (cv.Lin & 3) == 0 && cv.Lin >= 64;
}
constexpr int kStripMargin = 8;
template <int K>
struct Strip {
    static constexpr int PAD = (K - 1) / 2, OFF = (kStripMargin - PAD) & 3, NV4 = (OFF + 3 + K + 3) / 4;
    static_assert(((PAD + OFF) & 3) == 0 && PAD + OFF <= kStripMargin, "window start on a 16-byte boundary inside the margin");
};
// window of one channel row for outputs l0 .. l0+3 (l0 a multiple of 4); `row` points at element 0 of the row
template <int K>
__device__ __forceinline__ void strip_window(const float* row, int l0, float (&xw)[Strip<K>::NV4 * 4]) {
    const float4* p = reinterpret_cast<const float4*>(row + l0 - Strip<K>::PAD - Strip<K>::OFF);
#pragma unroll
    for (int j = 0; j < Strip<K>::NV4; ++j) {
        float4 v = p[j];
        asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w));      // keep the 16-byte read whole
        xw[4 * j] = v.x; xw[4 * j + 1] = v.y; xw[4 * j + 2] = v.z; xw[4 * j + 3] = v.w;
    }
}
// acc[r] += sum_t w[t] * x[l0 + r + t - PAD]          (FLIP false: the convolution itself)
// acc[r] += sum_t w[t] * g[l0 + r + PAD - t]          (FLIP true: its transpose, i.e. the data gradient)
template <int K, bool FLIP>
__device__ __forceinline__ void strip_fma(const float* w, const float (&xw)[Strip<K>::NV4 * 4], float (&acc)[4]) {
#pragma unroll
    for (int t = 0; t < K; ++t) {
        const float wt = w[FLIP ? K - 1 - t : t];
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = fmaf(wt, xw[Strip<K>::OFF + r + t], acc[r]);
    }
}
// halo of a staged tile for conv `cv`: strip-capable convs get the 8-float margin (>= their pad)
__host__ __device__ constexpr int tile_halo(const raae_conv_t& cv) {
    return cv.transposed ? 0 : (strip_conv_ok(cv) ? kStripMargin : cv.pad);
}

typedef raae_block_fwd_a_t BlockFwdAArgs;
__device__ __forceinline__ int conv_nw_dev(const raae_conv_t& cv) {
    return cv.transposed ? cv.Cin * (cv.Cout / cv.groups) * cv.K : cv.Cout * (cv.Cin / cv.groups) * cv.K;
}

// KIND >= 0: instance for kBlk[KIND] -- every shape parameter is a compile-time constant (taps unroll, index splits
// become shifts, dead branches vanish); KIND < 0: generic instance reading the shape from its arguments.
template <int KIND, bool BIG = false>
__device__ __forceinline__ void block_fwd_a_body(const BlockFwdAArgs& a, const int bx, const int gx, float* dyn) {
#define SH(f) (KIND >= 0 ? kBlk[KIND < 0 ? 0 : KIND].f : a.f)
    const raae_conv_t cv1 = SH(cv1), cvs = SH(cvs);
    const int sh_lin = KIND >= 0 ? clg2(SH(Lin)) : a.sh_lin, sh_l1 = KIND >= 0 ? clg2(SH(L1)) : a.sh_l1;
    const int sh_lout = KIND >= 0 ? clg2(SH(Lout)) : a.sh_lout, sh_e = KIND >= 0 ? clg2(SH(E)) : a.sh_e;
    const int halo = KIND >= 0 ? tile_halo(cv1) : a.halo;
    constexpr bool kStrip1 = KIND >= 0 && strip_conv_ok(kBlk[KIND < 0 ? 0 : KIND].cv1);
    __shared__ ViewStats vs;
    __shared__ double scr[512], scr2[2 * CT_MAXCH * 8];
    STAMP(0, 0);
    const int nW1 = conv_nw_dev(cv1), nWs = SH(has_short) ? conv_nw_dev(cvs) : 0;
    const WeightRegs wregs = weights4_issue(a.w1, nW1, a.ws, nWs, a.wf1, SH(E) * SH(Lin), a.wf2, SH(Lout) * SH(E));
    {
        const raae::StatJob jobs[1] = {a.in.has_bn ? raae::stat_job_bn(a.in.bn, SH(Cin), vs.mean, vs.rstd, true)
                                                   : raae::stat_job_none()};
        raae::stat_jobs<1, CT_MAXCH>(jobs, bx == 0);
    }
    STAMP(0, 1);
    const int Lp = SH(Lin) + 2 * halo;
    float* Rt = dyn;                                   // [S][Cin][Lp]
    float* E1t = Rt + a.S * SH(Cin) * Lp;                // [S][Cin][E]   PReLU(E1)
    float* W1 = E1t + a.S * SH(Cin) * SH(E);               // weights
    float* Wsh = W1 + nW1;
    float* Wf1 = Wsh + nWs;                            // [E][Lin]
    float* Wf2 = Wf1 + SH(E) * SH(Lin);                    // [Lout][E]
    weights4_commit(wregs, W1, a.w1, nW1, Wsh, a.ws, nWs, Wf1, a.wf1, SH(E) * SH(Lin), Wf2, a.wf2, SH(Lout) * SH(E));
    const ChanMap mo = chan_map(SH(Cout)), mi = chan_map(SH(Cin));
    const float b1 = mo.active ? a.b1[mo.c] : 0.f, sl1 = mo.active ? a.slope1[mo.c] : 1.f;
    const float bsh = (mo.active && SH(has_short)) ? a.bs[mo.c] : 0.f;
    const float sle1 = mi.active ? a.se1[mi.c] : 1.f, sle2 = mi.active ? a.se2[mi.c] : 1.f;
    const int sub = (SH(Lin) >= 64 && (mi.tpc & 15) == 0) ? 16 : 1;
    const int jj = mi.j / sub, lane_sub = mi.j - jj * sub, tpo = mi.tpc / sub;
    double t1s = 0.0, t1q = 0.0, e2s = 0.0, e2q = 0.0;
    STAMP(0, 2);
    for (int grp = bx; grp < a.ngroups; grp += gx) {
        const int b0 = grp * a.S, nb = min(a.S, a.B - b0);
        __syncthreads();
        STAMP(0, 3);
        stage_view_tile<BIG>(Rt, a.in, &vs, SH(Cin), SH(Lin), sh_lin, halo, cv1.pad_replicate, b0, nb);
        __syncthreads();
        STAMP(0, 4);
        if (mo.active) {
            // conv1 -> T1 (+ statistics of PReLU1(T1))
            const int n1 = nb * SH(L1);
            if constexpr (kStrip1) {
                constexpr int K1 = kBlk[KIND < 0 ? 0 : KIND].cv1.K, CI = kBlk[KIND < 0 ? 0 : KIND].Cin;
                const int L4 = SH(L1) >> 2, n4 = nb * L4;
                const float* w1c = W1 + mo.c * CI * K1;
                for (int q = mo.j; q < n4; q += mo.tpc) {
                    const int sidx = q / L4, l0 = 4 * (q - sidx * L4);
                    float acc[4] = {b1, b1, b1, b1};
#pragma unroll
                    for (int ci = 0; ci < CI; ++ci) {
                        float xw[Strip<K1>::NV4 * 4];
                        strip_window<K1>(Rt + (sidx * CI + ci) * Lp + halo, l0, xw);
                        strip_fma<K1, false>(w1c + ci * K1, xw, acc);
                    }
                    *reinterpret_cast<float4*>(a.T1 + ((size_t)(b0 + sidx) * SH(Cout) + mo.c) * SH(L1) + l0) =
                        make_float4(acc[0], acc[1], acc[2], acc[3]);
                    const float p0 = prelu(acc[0], sl1), p1 = prelu(acc[1], sl1), p2 = prelu(acc[2], sl1), p3 = prelu(acc[3], sl1);
                    t1s += (double)((p0 + p1) + (p2 + p3));
                    t1q += (double)(p0 * p0 + p1 * p1) + (double)(p2 * p2 + p3 * p3);
                }
            } else if (!cv1.transposed) {
                const int cig1 = cv1.Cin / cv1.groups;
                const float* w1c = W1 + mo.c * cig1 * cv1.K;
                for (int q0 = mo.j; q0 < n1; q0 += 4 * mo.tpc) {
                    const float* xb[4];
                    int so[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int q = q0 + r * mo.tpc;
                        int s, l;
                        split(q < n1 ? q : q0, SH(L1), sh_l1, &s, &l);
                        xb[r] = conv_tap0(cv1, Rt + s * SH(Cin) * Lp, Lp, halo, mo.c, l);
                        so[r] = q < n1 ? (s * SH(Cout) + mo.c) * SH(L1) + l : -1;
                    }
                    float acc[4] = {b1, b1, b1, b1};
                    conv4(cv1.K, w1c, xb, Lp, cig1, acc);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (so[r] < 0) continue;
                        a.T1[(size_t)b0 * SH(Cout) * SH(L1) + so[r]] = acc[r];
                        const float pv = prelu(acc[r], sl1);
                        t1s += (double)pv; t1q += (double)pv * (double)pv;
                    }
                }
            } else {
                for (int q = mo.j; q < n1; q += mo.tpc) {
                    int s, l;
                    split(q, SH(L1), sh_l1, &s, &l);
                    const float v = b1 + conv_out(cv1, W1, Rt + s * SH(Cin) * Lp, Lp, halo, mo.c, l);
                    a.T1[((size_t)(b0 + s) * SH(Cout) + mo.c) * SH(L1) + l] = v;
                    const float pv = prelu(v, sl1);
                    t1s += (double)pv; t1q += (double)pv * (double)pv;
                }
            }
            if (SH(has_short)) {
                const int n2 = nb * SH(Lout);
                for (int q = mo.j; q < n2; q += mo.tpc) {
                    int s, l;
                    split(q, SH(Lout), sh_lout, &s, &l);
                    a.Sh[((size_t)(b0 + s) * SH(Cout) + mo.c) * SH(Lout) + l] =
                        bsh + conv_out(cvs, Wsh, Rt + s * SH(Cin) * Lp, Lp, halo, mo.c, l);
                }
            }
        }
        // fc1: E1[s][ci][e] = bf1[e] + sum_l wf1[e][l] * R[s][ci][l] * mask
        constexpr int kE = KIND >= 0 ? kBlk[KIND < 0 ? 0 : KIND].E : 0;
        constexpr bool kFc1Rows = BIG && KIND >= 0 && kE >= 2 && kE <= 4 && kBlk[KIND < 0 ? 0 : KIND].Lin >= 64 &&
                                  kBlk[KIND < 0 ? 0 : KIND].Lin <= 256 && kBlk[KIND < 0 ? 0 : KIND].Cin >= 4;
        if (kFc1Rows && mi.active && sub == 16) {
            // Large batches: the 16 lanes of a (sample, channel) row produce ALL E outputs of that row from one set of
            // operands -- the dropout mask (global memory) and the row are read once instead of once per output, and a
            // four-sample group is one trip instead of E (each trip is a dependent global round trip inside the
            // compute stage; measured alone at 4096 rows: 35.5 -> 33.9 us and 29.8 -> 26.4 us for the two 256-point decoder
            // blocks; the one-channel encoder block 0 is faster with the loop below).  Per output
            // the same products in the same order as the loop below.
            const int nloop = (nb + tpo - 1) / tpo;
            for (int it = 0; it < nloop; ++it) {
                const int srow = jj + it * tpo;
                const bool ok = srow < nb && jj < tpo;
                const int s = ok ? srow : 0;
                const float* xr = Rt + (s * SH(Cin) + mi.c) * Lp + halo;
                const float* mk = a.mask ? a.mask + ((size_t)(b0 + s) * SH(Cin) + mi.c) * SH(Lin) : nullptr;
                float mv[16], xv[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int l = lane_sub + 16 * i;
                    const bool in = ok && l < SH(Lin);
                    mv[i] = (mk && in) ? mk[l] : 1.f;
                    xv[i] = in ? xr[l] : 0.f;
                }
                float acc[kE > 0 ? kE : 1];
#pragma unroll
                for (int e = 0; e < kE; ++e) {
                    const float* wr = Wf1 + e * SH(Lin);
                    float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
#pragma unroll
                    for (int i = 0; i < 16; i += 4) {
                        const int l = lane_sub + 16 * i;
                        const float w0 = l < SH(Lin) ? wr[l] : 0.f, w1 = l + 16 < SH(Lin) ? wr[l + 16] : 0.f;
                        const float w2 = l + 32 < SH(Lin) ? wr[l + 32] : 0.f, w3 = l + 48 < SH(Lin) ? wr[l + 48] : 0.f;
                        p0 = fmaf(w0 * xv[i], mv[i], p0); p1 = fmaf(w1 * xv[i + 1], mv[i + 1], p1);
                        p2 = fmaf(w2 * xv[i + 2], mv[i + 2], p2); p3 = fmaf(w3 * xv[i + 3], mv[i + 3], p3);
                    }
                    float v = (p0 + p1) + (p2 + p3);
                    v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64);
                    v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 8, 64);
                    acc[e] = v;
                }
                if (ok && lane_sub == 0) {
#pragma unroll
                    for (int e = 0; e < kE; ++e) {
                        const float v = acc[e] + a.bf1[e];
                        a.E1[((size_t)(b0 + s) * SH(Cin) + mi.c) * SH(E) + e] = v;
                        E1t[(s * SH(Cin) + mi.c) * SH(E) + e] = prelu(v, sle1);
                    }
                }
            }
        } else
        if (mi.active) {
            const int n = nb * SH(E), nloop = (n + tpo - 1) / tpo;
            for (int it = 0; it < nloop; ++it) {
                const int q = jj + it * tpo;
                const bool ok = q < n && jj < tpo;
                int s = 0, e = 0;
                if (ok) split(q, SH(E), sh_e, &s, &e);
                const float* xr = Rt + (s * SH(Cin) + mi.c) * Lp + halo;
                const float* wr = Wf1 + e * SH(Lin);
                const float* mk = a.mask ? a.mask + ((size_t)(b0 + s) * SH(Cin) + mi.c) * SH(Lin) : nullptr;
                float acc = 0.f;
                if (ok) {
                    if (sub == 16 && SH(Lin) <= 256) {
                        // <= 16 elements per lane: every operand (the dropout mask comes from global memory) is
                        // requested before the first product instead of one dependent round trip per element
                        float mv[16], xv[16], wv[16];
#pragma unroll
                        for (int i = 0; i < 16; ++i) {
                            const int l = lane_sub + 16 * i;
                            const bool in = l < SH(Lin);
                            mv[i] = (mk && in) ? mk[l] : 1.f;
                            xv[i] = in ? xr[l] : 0.f;
                            wv[i] = in ? wr[l] : 0.f;
                        }
                        float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
#pragma unroll
                        for (int i = 0; i < 16; i += 4) {
                            p0 = fmaf(wv[i] * xv[i], mv[i], p0); p1 = fmaf(wv[i + 1] * xv[i + 1], mv[i + 1], p1);
                            p2 = fmaf(wv[i + 2] * xv[i + 2], mv[i + 2], p2); p3 = fmaf(wv[i + 3] * xv[i + 3], mv[i + 3], p3);
                        }
                        acc = (p0 + p1) + (p2 + p3);
                    } else if (mk) {
                        for (int l = lane_sub; l < SH(Lin); l += sub) acc += wr[l] * xr[l] * mk[l];
                    } else {
                        for (int l = lane_sub; l < SH(Lin); l += sub) acc += wr[l] * xr[l];
                    }
                }
                if (sub == 16) {
                    acc += __shfl_xor(acc, 1, 64); acc += __shfl_xor(acc, 2, 64);
                    acc += __shfl_xor(acc, 4, 64); acc += __shfl_xor(acc, 8, 64);
                }
                if (ok && lane_sub == 0) {
                    acc += a.bf1[e];
                    a.E1[((size_t)(b0 + s) * SH(Cin) + mi.c) * SH(E) + e] = acc;
                    E1t[(s * SH(Cin) + mi.c) * SH(E) + e] = prelu(acc, sle1);
                }
            }
        }
        __syncthreads();
        STAMP(0, 5);
        // fc2: E2[s][ci][lo] = bf2[lo] + sum_e wf2[lo][e] * PReLU(E1)[s][ci][e]
        constexpr bool kFc2Cols = BIG && KIND >= 0 && kE >= 1 && kE <= 4 && (kBlk[KIND < 0 ? 0 : KIND].Lout % (256 / kBlk[KIND < 0 ? 0 : KIND].Cin)) == 0 &&
                                  (256 % kBlk[KIND < 0 ? 0 : KIND].Cin) == 0;
        if constexpr (kFc2Cols) {
            // Large batches: a thread's outputs lie in Lout / tpc fixed columns `lo` (q = j + k * tpc with tpc | Lout), so
            // the bias and the E weights of a column are fetched ONCE and the loop over the samples has no global
            // load in it (the q loop below re-reads bf2[lo] -- a dependent global round trip -- for every output:
            // 7.7 us of the 33 us kernel on the 4x256 decoder block at 4096 rows).  Same products, same order.
            if (mi.active) {
                constexpr int LO = kBlk[KIND < 0 ? 0 : KIND].Lout, CI = kBlk[KIND < 0 ? 0 : KIND].Cin, TPC = 256 / CI, NC = LO / TPC;
                float bcol[NC], wcol[NC][kE > 0 ? kE : 1];
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const int lo = mi.j + c * TPC;
                    bcol[c] = a.bf2[lo];
#pragma unroll
                    for (int e = 0; e < kE; ++e) wcol[c][e] = Wf2[lo * kE + e];
                }
                for (int s = 0; s < nb; ++s) {
                    const float* er = E1t + (s * CI + mi.c) * kE;
                    float ev[kE > 0 ? kE : 1];
#pragma unroll
                    for (int e = 0; e < kE; ++e) ev[e] = er[e];
                    float* orow = a.E2 + ((size_t)(b0 + s) * CI + mi.c) * LO;
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        float acc = bcol[c];
#pragma unroll
                        for (int e = 0; e < kE; ++e) acc += wcol[c][e] * ev[e];
                        orow[mi.j + c * TPC] = acc;
                        if (a.pE2) {
                            const float pv = prelu(acc, sle2);
                            e2s += (double)pv; e2q += (double)pv * (double)pv;
                        }
                    }
                }
            }
        } else
        if (mi.active) {
            const int n = nb * SH(Lout);
            for (int q = mi.j; q < n; q += mi.tpc) {
                int s, lo;
                split(q, SH(Lout), sh_lout, &s, &lo);
                float acc = a.bf2[lo];
                const float* er = E1t + (s * SH(Cin) + mi.c) * SH(E);
                const float* wr = Wf2 + lo * SH(E);
                for (int e = 0; e < SH(E); ++e) acc += wr[e] * er[e];
                a.E2[((size_t)(b0 + s) * SH(Cin) + mi.c) * SH(Lout) + lo] = acc;
                if (a.pE2) {
                    const float pv = prelu(acc, sle2);
                    e2s += (double)pv; e2q += (double)pv * (double)pv;
                }
            }
        }
    }
    STAMP(0, 6);
    chan_reduce(t1s, t1q, SH(Cout), mo, a.pT1 + (size_t)bx * SH(Cout) * 2, scr, scr2);
    if (a.pE2) chan_reduce(e2s, e2q, SH(Cin), mi, a.pE2 + (size_t)bx * SH(Cin) * 2, scr, scr2);

    STAMP(0, 7);
}
#undef SH

template <int KIND, bool BIG = false>
__global__ __launch_bounds__(256) void block_fwd_a_kernel(BlockFwdAArgs ka) {
    extern __shared__ __attribute__((aligned(16))) float dyn[];
    __shared__ BlockFwdAArgs sa;
    const BlockFwdAArgs& a = raae::args_to_lds(&sa);
    block_fwd_a_body<KIND, BIG>(a, blockIdx.x, gridDim.x, dyn);
}
// one trial per grid plane (raae_common.h, "batched launches over independent trials"): the same body as the
// single-trial instance of the same <KIND, BIG>, the launch-bound and the large-batch instances alike
template <int KIND, bool BIG = false>
__global__ __launch_bounds__(256) void block_fwd_a_kernel_m(const BlockFwdAArgs* table) {
    extern __shared__ __attribute__((aligned(16))) float dyn[];
    __shared__ BlockFwdAArgs sa;
    const BlockFwdAArgs& a = raae::args_from_table(&sa, table);
    block_fwd_a_body<KIND, BIG>(a, blockIdx.x, gridDim.x, dyn);
}

typedef raae_block_fwd_b_t BlockFwdBArgs;

template <int KIND, bool BIG = false>        // see block_fwd_a_kernel
__device__ __forceinline__ void block_fwd_b_body(const BlockFwdBArgs& a, const int bx, const int gx, float* dyn) {
#define SH(f) (KIND >= 0 ? kBlk[KIND < 0 ? 0 : KIND].f : a.f)
    const raae_conv_t cv2 = SH(cv2), cve = SH(cve);
    const int sh_l1 = KIND >= 0 ? clg2(SH(L1)) : a.sh_l1;
    const int sh_lout = KIND >= 0 ? clg2(SH(Lout)) : a.sh_lout;
    const int halo2 = KIND >= 0 ? tile_halo(cv2) : a.halo2;
    constexpr bool kStrip2 = KIND >= 0 && strip_conv_ok(kBlk[KIND < 0 ? 0 : KIND].cv2) && !kBlk[KIND < 0 ? 0 : KIND].has_excit;
    __shared__ ViewStats vs1, vse, vsr;
    __shared__ double scr[512], scr2[2 * CT_MAXCH * 8];
    STAMP(1, 0);
    const int nW2 = conv_nw_dev(cv2), nWe = SH(has_excit) ? conv_nw_dev(cve) : 0;
    const WeightRegs wregs = weights4_issue(a.w2, nW2, a.we, nWe, nullptr, 0, nullptr, 0);
    {
        const raae::StatJob jobs[3] = {
            raae::stat_job_bn(a.vT1.bn, SH(Cout), vs1.mean, vs1.rstd, true),
            a.vE2.has_bn ? raae::stat_job_bn(a.vE2.bn, SH(Cin), vse.mean, vse.rstd, true) : raae::stat_job_none(),
            (!SH(has_short) && a.vR.has_bn) ? raae::stat_job_bn(a.vR.bn, SH(Cin), vsr.mean, vsr.rstd, false)
                                          : raae::stat_job_none()};
        raae::stat_jobs<3, CT_MAXCH>(jobs, bx == 0);
    }
    STAMP(1, 1);
    const int Lp = SH(L1) + 2 * halo2;
    float* Tt = dyn;                                    // [S][Cout][Lp]
    float* Et = Tt + a.S * SH(Cout) * Lp;                 // [S][Cin][Lout]  (only with conv_excit)
    float* W2 = Et + (SH(has_excit) ? a.S * SH(Cin) * SH(Lout) : 0);
    float* We = W2 + nW2;
    weights4_commit(wregs, W2, a.w2, nW2, We, a.we, nWe, nullptr, nullptr, 0, nullptr, nullptr, 0);
    const ChanMap m = chan_map(SH(Cout));
    const float b2 = m.active ? a.b2[m.c] : 0.f, sl2 = m.active ? a.slope2[m.c] : 1.f;
    const float be = (m.active && SH(has_excit)) ? a.be[m.c] : 0.f;
    const float sl3 = (m.active && SH(has_excit)) ? a.se3[m.c] : 1.f;
    const float sls = (m.active && SH(has_short)) ? a.ss[m.c] : 1.f;
    double ys = 0.0, yq = 0.0;
    STAMP(1, 2);
    for (int grp = bx; grp < a.ngroups; grp += gx) {
        const int b0 = grp * a.S, nb = min(a.S, a.B - b0);
        __syncthreads();
        stage_view_tile<BIG>(Tt, a.vT1, &vs1, SH(Cout), SH(L1), sh_l1, halo2, 0, b0, nb);
        if (SH(has_excit)) stage_view_tile<BIG>(Et, a.vE2, &vse, SH(Cin), SH(Lout), sh_lout, 0, 0, b0, nb);
        __syncthreads();
        STAMP(1, 3);
        if (!m.active) continue;
        const int n = nb * SH(Lout);
        if constexpr (kStrip2) {
            // strips of four outputs: the global operands of the sum (Sh | R, E2) are 16-byte loads requested ahead
            // of the taps
            constexpr int K2 = kBlk[KIND < 0 ? 0 : KIND].cv2.K, CO = kBlk[KIND < 0 ? 0 : KIND].Cout;
            const int L4 = SH(Lout) >> 2, n4 = nb * L4;
            const float* w2c = W2 + m.c * CO * K2;
            const float rmu = (!SH(has_short) && a.vR.has_bn) ? vsr.mean[m.c] : 0.f;
            const float rrs = (!SH(has_short) && a.vR.has_bn) ? vsr.rstd[m.c] : 1.f;
            const float esl = a.vE2.slope ? a.vE2.slope[m.c] : 1.f;
            for (int q = m.j; q < n4; q += m.tpc) {
                const int sidx = q / L4, l0 = 4 * (q - sidx * L4);
                const size_t idx = ((size_t)(b0 + sidx) * SH(Cout) + m.c) * SH(Lout) + l0;
                float4 shq = *reinterpret_cast<const float4*>((SH(has_short) ? a.Sh : a.vR.raw) + idx);
                float4 exq = *reinterpret_cast<const float4*>(a.vE2.raw + idx);
                float acc[4] = {b2, b2, b2, b2};
#pragma unroll
                for (int ci = 0; ci < CO; ++ci) {
                    float xw[Strip<K2>::NV4 * 4];
                    strip_window<K2>(Tt + (sidx * CO + ci) * Lp + halo2, l0, xw);
                    strip_fma<K2, false>(w2c + ci * K2, xw, acc);
                }
                *reinterpret_cast<float4*>(a.T2 + idx) = make_float4(acc[0], acc[1], acc[2], acc[3]);
                if (SH(has_short)) shq = prelu4(shq, sls);
                else if (a.vR.has_bn) shq = make_float4((shq.x - rmu) * rrs, (shq.y - rmu) * rrs, (shq.z - rmu) * rrs, (shq.w - rmu) * rrs);
                if (a.vE2.slope) exq = prelu4(exq, esl);
                const float y0 = prelu(acc[0], sl2) + shq.x + exq.x, y1 = prelu(acc[1], sl2) + shq.y + exq.y;
                const float y2 = prelu(acc[2], sl2) + shq.z + exq.z, y3 = prelu(acc[3], sl2) + shq.w + exq.w;
                *reinterpret_cast<float4*>(a.Y + idx) = make_float4(y0, y1, y2, y3);
                ys += (double)((y0 + y1) + (y2 + y3));
                yq += (double)(y0 * y0 + y1 * y1) + (double)(y2 * y2 + y3 * y3);
            }
            continue;
        }
        if (!cv2.transposed) {
            // four outputs per trip: their global operands (Sh / E2 / R) are requested together, ahead of the taps
            const int cig2 = cv2.Cin / cv2.groups, cige = SH(has_excit) ? cve.Cin / cve.groups : 1;
            const float* w2c = W2 + m.c * cig2 * cv2.K;
            const float* wec = We + m.c * cige * (SH(has_excit) ? cve.K : 1);
            for (int q0 = m.j; q0 < n; q0 += 4 * m.tpc) {
                const float* xb[4];
                const float* eb[4];
                size_t idx[4];
                bool ok[4];
                float shv[4], exv[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int q = q0 + r * m.tpc;
                    ok[r] = q < n;
                    int s, l;
                    split(ok[r] ? q : q0, SH(Lout), sh_lout, &s, &l);
                    idx[r] = ((size_t)(b0 + s) * SH(Cout) + m.c) * SH(Lout) + l;
                    xb[r] = conv_tap0(cv2, Tt + s * SH(Cout) * Lp, Lp, halo2, m.c, l);
                    eb[r] = SH(has_excit) ? conv_tap0(cve, Et + s * SH(Cin) * SH(Lout), SH(Lout), 0, m.c, l) : xb[r];
                    shv[r] = SH(has_short) ? a.Sh[idx[r]] : view_at(a.vR, &vsr, m.c, idx[r]);
                    exv[r] = SH(has_excit) ? 0.f : view_at(a.vE2, &vse, m.c, idx[r]);     // Cin == Cout: PReLU_e2(E2)
                }
                float t2[4] = {b2, b2, b2, b2};
                conv4(cv2.K, w2c, xb, Lp, cig2, t2);
                float e3[4] = {be, be, be, be};
                if (SH(has_excit)) conv4(cve.K, wec, eb, SH(Lout), cige, e3);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (!ok[r]) continue;
                    a.T2[idx[r]] = t2[r];
                    float ex = exv[r];
                    if (SH(has_excit)) { a.E3[idx[r]] = e3[r]; ex = prelu(e3[r], sl3); }
                    const float sh = SH(has_short) ? prelu(shv[r], sls) : shv[r];
                    const float y = prelu(t2[r], sl2) + sh + ex;
                    a.Y[idx[r]] = y;
                    ys += (double)y; yq += (double)y * (double)y;
                }
            }
            continue;
        }
        if (BIG && (SH(Lout) & 3) == 0 && a.S * SH(Lout) >= 256 && aligned16(a.T2) && aligned16(a.Y) && aligned16(a.Sh) &&
            aligned16(a.E3) && aligned16(a.vE2.raw) && aligned16(a.vR.raw)) {
            // large batches, transposed conv2: four consecutive outputs per thread; the global operands of the sum
            // (Sh | R, E2) are 16-byte loads issued ahead of the taps, T2 / E3 / Y leave as 16-byte stores
            const int L4 = SH(Lout) >> 2, n4 = nb * L4;
            const float rmu = (!SH(has_short) && a.vR.has_bn) ? vsr.mean[m.c] : 0.f;
            const float rrs = (!SH(has_short) && a.vR.has_bn) ? vsr.rstd[m.c] : 1.f;
            const float esl = a.vE2.slope ? a.vE2.slope[m.c] : 1.f;
            for (int q = m.j; q < n4; q += m.tpc) {
                const int sidx = q / L4, l0 = 4 * (q - sidx * L4);
                const size_t idx = ((size_t)(b0 + sidx) * SH(Cout) + m.c) * SH(Lout) + l0;
                float4 shq = *reinterpret_cast<const float4*>((SH(has_short) ? a.Sh : a.vR.raw) + idx);
                float4 exq = make_float4(0.f, 0.f, 0.f, 0.f);
                if (!SH(has_excit)) exq = *reinterpret_cast<const float4*>(a.vE2.raw + idx);
                const float* ts = Tt + sidx * SH(Cout) * Lp;
                const float* es = Et + sidx * SH(Cin) * SH(Lout);
                float t2[4], e3[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    t2[r] = b2 + conv_out(cv2, W2, ts, Lp, halo2, m.c, l0 + r);
                    e3[r] = SH(has_excit) ? be + conv_out(cve, We, es, SH(Lout), 0, m.c, l0 + r) : 0.f;
                }
                *reinterpret_cast<float4*>(a.T2 + idx) = make_float4(t2[0], t2[1], t2[2], t2[3]);
                if (SH(has_excit)) {
                    *reinterpret_cast<float4*>(a.E3 + idx) = make_float4(e3[0], e3[1], e3[2], e3[3]);
                    exq = make_float4(prelu(e3[0], sl3), prelu(e3[1], sl3), prelu(e3[2], sl3), prelu(e3[3], sl3));
                } else if (a.vE2.slope) {
                    exq = prelu4(exq, esl);
                }
                if (SH(has_short)) shq = prelu4(shq, sls);
                else if (a.vR.has_bn) shq = make_float4((shq.x - rmu) * rrs, (shq.y - rmu) * rrs, (shq.z - rmu) * rrs, (shq.w - rmu) * rrs);
                const float y0 = prelu(t2[0], sl2) + shq.x + exq.x, y1 = prelu(t2[1], sl2) + shq.y + exq.y;
                const float y2 = prelu(t2[2], sl2) + shq.z + exq.z, y3 = prelu(t2[3], sl2) + shq.w + exq.w;
                *reinterpret_cast<float4*>(a.Y + idx) = make_float4(y0, y1, y2, y3);
                ys += (double)((y0 + y1) + (y2 + y3));
                yq += (double)(y0 * y0 + y1 * y1) + (double)(y2 * y2 + y3 * y3);
            }
            continue;
        }
        for (int q = m.j; q < n; q += m.tpc) {
            int s, l;
            split(q, SH(Lout), sh_lout, &s, &l);
            const size_t idx = ((size_t)(b0 + s) * SH(Cout) + m.c) * SH(Lout) + l;
            const float t2 = b2 + conv_out(cv2, W2, Tt + s * SH(Cout) * Lp, Lp, halo2, m.c, l);
            a.T2[idx] = t2;
            float ex;
            if (SH(has_excit)) {
                const float e3 = be + conv_out(cve, We, Et + s * SH(Cin) * SH(Lout), SH(Lout), 0, m.c, l);
                a.E3[idx] = e3;
                ex = prelu(e3, sl3);
            } else {
                ex = view_at(a.vE2, &vse, m.c, idx);          // Cin == Cout: PReLU_e2(E2)
            }
            const float sh = SH(has_short) ? prelu(a.Sh[idx], sls) : view_at(a.vR, &vsr, m.c, idx);
            const float y = prelu(t2, sl2) + sh + ex;
            a.Y[idx] = y;
            ys += (double)y; yq += (double)y * (double)y;
        }
    }
    STAMP(1, 4);
    chan_reduce(ys, yq, SH(Cout), m, a.pY + (size_t)bx * SH(Cout) * 2, scr, scr2);
    STAMP(1, 5);
}
#undef SH

template <int KIND, bool BIG = false>
__global__ __launch_bounds__(256) void block_fwd_b_kernel(BlockFwdBArgs ka) {
    extern __shared__ __attribute__((aligned(16))) float dyn[];
    __shared__ BlockFwdBArgs sa;
    const BlockFwdBArgs& a = raae::args_to_lds(&sa);
    block_fwd_b_body<KIND, BIG>(a, blockIdx.x, gridDim.x, dyn);
}
template <int KIND, bool BIG = false>
__global__ __launch_bounds__(256) void block_fwd_b_kernel_m(const BlockFwdBArgs* table) {
    extern __shared__ __attribute__((aligned(16))) float dyn[];
    __shared__ BlockFwdBArgs sa;
    const BlockFwdBArgs& a = raae::args_from_table(&sa, table);
    block_fwd_b_body<KIND, BIG>(a, blockIdx.x, gridDim.x, dyn);
}

// =====================================================================================
// Fused residual-block BACKWARD (data gradients).  Mirror of the forward split:
//   B: dY = BNbwd(g; Y)  ->  dT2 = dY PReLU2'(T2), dSh = dY PReLUs'(Sh) | dY, dE3 = dY PReLUe3'(E3) | dE2
//      (materialised once: the weight-gradient kernels and phase A read them as plain gradients),
//      dBn2 = conv2^T dT2 (+ BN-backward sums), dBnE = conv_excit^T dE3 (+ sums), PReLU-slope gradients.
//   A: dT1 = BNbwd(dBn2) PReLU1'(T1), dE2 = BNbwd(dBnE) PReLUe2'(E2), dE1 = (fc2^T dE2) PReLUe1'(E1),
//      dR = conv1^T dT1 + short^T dSh | dSh + mask * fc1^T dE1  (+ BN-backward sums for bn1).
// Parameter gradients of conv/fc weights stay in the per-layer tiled kernels (side streams).

// one element of the transposed conv: sum over outputs that read input (ci, li); gsm = tile [Cout][Lout] of the sample
__device__ __forceinline__ float conv_bwd_elem(const raae_conv_t& cv, const float* w, const float* gsm, int ci, int li) {
    const int cig = cv.Cin / cv.groups, cog = cv.Cout / cv.groups;
    const int g = ci / cig, cil = ci - g * cig;
    float acc = 0.f;
    const float* gg = gsm + (g * cog) * cv.Lout;
    if (cv.transposed) {
        const float* gr = gg + li * cv.stride;
        const float* wr = w + ci * cog * cv.K;
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
            int lmax = p / cv.stride;
            int lmin = p - cv.K + 1;
            lmin = lmin <= 0 ? 0 : (lmin + cv.stride - 1) / cv.stride;
            if (lmax > cv.Lout - 1) lmax = cv.Lout - 1;
            const float* gr = gg;
            const float* wr = w + (g * cog * cig + cil) * cv.K + (p - lmin * cv.stride);
            for (int col = 0; col < cog; ++col) {
                int wo = 0;
                for (int l = lmin; l <= lmax; ++l, wo -= cv.stride) acc += wr[wo] * gr[l];
                gr += cv.Lout; wr += cig * cv.K;
            }
        }
    }
    return acc;
}


// The same element with the kernel size and stride known at compile time.  Interior elements (every tap lands
// inside the output row) run straight-line multiply-adds with immediate offsets and no per-tap predicate --
// ~3 instructions per tap against ~8 plus two integer divisions in the generic loop, which is what this stage
// costs at one wave per SIMD; the few elements near an edge take the generic routine.
// Gradient that reaches PADDED input position p (0 <= p < Lin + 2*pad) of a non-transposed conv: the sum over
// the taps t and outputs l with l*S + t == p.  Positions whose taps all land inside the output row run
// unpredicated; the others (next to an edge, or halo positions) run the same unrolled taps predicated.
template <int K, int S>
__device__ __forceinline__ float conv_bwd_pos_t(const raae_conv_t& cv, const float* w, const float* gsm, int ci, int p) {
    const int cig = cv.Cin / cv.groups, cog = cv.Cout / cv.groups;
    const int g = ci / cig, cil = ci - g * cig;
    const int Lout = cv.Lout;
    constexpr int NJ = (K + S - 1) / S;                 // taps that can hit one input position
    const int lmax = p / S, t0 = p - lmax * S;          // S is a compile-time power of two: shift and mask
    const float* wr = w + (g * cog * cig + cil) * K;
    const float* gg = gsm + (g * cog) * Lout;
    float acc = 0.f;
    if (lmax - (NJ - 1) >= 0 && lmax <= Lout - 1) {
        const bool last = t0 + (NJ - 1) * S < K;        // only the last tap of a position can fall off the kernel
        const float* wt = wr + t0;
        const float* gr = gg + lmax;
        for (int col = 0; col < cog; ++col) {
#pragma unroll
            for (int j = 0; j < NJ - 1; ++j) acc = fmaf(wt[j * S], gr[-j], acc);
            acc += last ? wt[(NJ - 1) * S] * gr[-(NJ - 1)] : 0.f;
            wt += cig * K; gr += Lout;
        }
    } else {
        for (int col = 0; col < cog; ++col) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int l = lmax - j, t = t0 + j * S;
                const bool v = t < K && l >= 0 && l < Lout;
                const float prod = wr[v ? t : 0] * gg[v ? l : 0];
                acc += v ? prod : 0.f;
            }
            wr += cig * K; gg += Lout;
        }
    }
    return acc;
}

// The same element with the kernel size and stride known at compile time (~3 instructions per tap against ~8
// plus two integer divisions in the generic loop, which is what this stage costs at one wave per SIMD).
// OWN: return only the element's own position p = li + pad; the caller adds the replicate-halo positions of
// an edge element (conv_bwd_halo_t).  Otherwise edge elements of a replicate-padded conv take the generic routine.
template <int K, int S, bool TR, bool OWN = false>
__device__ __forceinline__ float conv_bwd_elem_t(const raae_conv_t& cv, const float* w, const float* gsm, int ci, int li) {
    if (TR) {
        const int cog = cv.Cout / cv.groups, cig = cv.Cin / cv.groups;
        const int g = ci / cig;
        float acc = 0.f;
        const float* gr = gsm + (g * cog) * cv.Lout + li * S;
        const float* wr = w + ci * cog * K;
        for (int col = 0; col < cog; ++col) {
#pragma unroll
            for (int tt = 0; tt < K; ++tt) acc = fmaf(wr[tt], gr[tt], acc);
            wr += K; gr += cv.Lout;
        }
        return acc;
    }
    if (!OWN && cv.pad_replicate && (li == 0 || li == cv.Lin - 1)) return conv_bwd_elem(cv, w, gsm, ci, li);
    return conv_bwd_pos_t<K, S>(cv, w, gsm, ci, li + cv.pad);
}
// Replicate padding: the halo positions p < pad read input 0 and the positions p >= Lin + pad read input Lin-1,
// so their gradients belong to those two elements.  Instead of the edge lane walking all of them, the `pad`
// lanes next to each edge take one halo position each and an xor-shuffle over the aligned group of 8 lanes
// (rows start at multiples of 8 lanes: Lin % 8 == 0) delivers the sums.  Returns what to add to this element.
template <int K, int S>
__device__ __forceinline__ float conv_bwd_halo_t(const raae_conv_t& cv, const float* w, const float* gsm, int ci, int li) {
    const int pad = cv.pad, Lin = cv.Lin;
    float hl = li < pad ? conv_bwd_pos_t<K, S>(cv, w, gsm, ci, li) : 0.f;
    float hr = li >= Lin - pad ? conv_bwd_pos_t<K, S>(cv, w, gsm, ci, li + 2 * pad) : 0.f;
    hl += __shfl_xor(hl, 1, 64); hl += __shfl_xor(hl, 2, 64); hl += __shfl_xor(hl, 4, 64);
    hr += __shfl_xor(hr, 1, 64); hr += __shfl_xor(hr, 2, 64); hr += __shfl_xor(hr, 4, 64);
    return (li == 0 ? hl : 0.f) + (li == Lin - 1 ? hr : 0.f);
}
__device__ __forceinline__ float conv_bwd_elem_fast(int kind, const raae_conv_t& cv, const float* w, const float* gsm, int ci, int li) {
    switch (kind) {
    case -1: return conv_bwd_elem(cv, w, gsm, ci, li);
    case 11 * 16 + 1: return conv_bwd_elem_t<11, 1, false>(cv, w, gsm, ci, li);
    case 11 * 16 + 2: return conv_bwd_elem_t<11, 2, false>(cv, w, gsm, ci, li);
    case 7 * 16 + 2: return conv_bwd_elem_t<7, 2, false>(cv, w, gsm, ci, li);
    case 5 * 16 + 1: return conv_bwd_elem_t<5, 1, false>(cv, w, gsm, ci, li);
    case 5 * 16 + 2: return conv_bwd_elem_t<5, 2, false>(cv, w, gsm, ci, li);
    case 1024 + 2 * 16 + 2: return conv_bwd_elem_t<2, 2, true>(cv, w, gsm, ci, li);
    case 1024 + 4 * 16 + 4: return conv_bwd_elem_t<4, 4, true>(cv, w, gsm, ci, li);
    case 1024 + 8 * 16 + 8: return conv_bwd_elem_t<8, 8, true>(cv, w, gsm, ci, li);
    default: return conv_bwd_elem(cv, w, gsm, ci, li);
    }
}
// scalar (uniform) dispatch key of a conv for conv_bwd_elem_fast
__device__ __forceinline__ int conv_kind(const raae_conv_t& cv) {
    return __builtin_amdgcn_readfirstlane((cv.transposed ? 1024 : 0) + cv.K * 16 + cv.stride);
}

typedef raae_block_bwd_b_t BlockBwdBArgs;

// `bx` of `gx`: the workgroup's index / count among the workgroups that run this block's backward phase B (the
// whole grid of block_bwd_b_kernel, the leading range of co_kernel<CoBwdB<KB>, CoWgrad<KW>>)
template <int KIND, bool BIG = false>        // see block_fwd_a_kernel
__device__ __forceinline__ void block_bwd_b_body(const BlockBwdBArgs& a, const int bx, const int gx, float* dyn) {
#define SH(f) (KIND >= 0 ? kBlk[KIND < 0 ? 0 : KIND].f : a.f)
    const raae_conv_t cv2 = SH(cv2), cve = SH(cve);
    const int sh_l1 = KIND >= 0 ? clg2(SH(L1)) : a.sh_l1;
    const int sh_lout = KIND >= 0 ? clg2(SH(Lout)) : a.sh_lout;
    __shared__ GradStats gs;
    __shared__ ViewStats vs1, vse;
    __shared__ double scr[512], scr2[2 * CT_MAXCH * 8];
    STAMP(2, 0);
    const int nW2 = conv_nw_dev(cv2), nWe = SH(has_excit) ? conv_nw_dev(cve) : 0;
    const WeightRegs wregs = weights4_issue(a.w2, nW2, a.we, nWe, nullptr, 0, nullptr, 0);
    {
        const raae::StatJob jobs[4] = {
            a.gy.has_bn ? raae::stat_job_bn(a.gy.bn, SH(Cout), gs.mean, gs.rstd, false) : raae::stat_job_none(),
            a.gy.has_bn ? raae::stat_job_bwd(a.gy.g_partials, a.gy.g_nparts, SH(Cout), a.gy.bn.count, gs.m1, gs.m2)
                        : raae::stat_job_none(),
            raae::stat_job_bn(a.vT1.bn, SH(Cout), vs1.mean, vs1.rstd, false),
            SH(has_excit) ? raae::stat_job_bn(a.vE2.bn, SH(Cin), vse.mean, vse.rstd, false) : raae::stat_job_none()};
        raae::stat_jobs<4, CT_MAXCH>(jobs, false);
    }
    STAMP(2, 1);
    // strip-capable conv2: the dT2 tile rows carry an 8-float zero margin on both sides (strip_window)
    constexpr bool kStripB = KIND >= 0 && strip_conv_ok(kBlk[KIND < 0 ? 0 : KIND].cv2);
    constexpr int GM = kStripB ? kStripMargin : 0;
    const int GP = SH(Lout) + 2 * GM;
    float* Gt = dyn;                                      // dT2 [S][Cout][GP]
    float* Et = Gt + a.S * SH(Cout) * GP;                   // dE3 [S][Cout][Lout]   (has_excit)
    if (GM > 0) for (int i = threadIdx.x; i < a.S * SH(Cout) * 2 * GM; i += 256) {
        const int row = i / (2 * GM), k = i - row * 2 * GM;
        Gt[row * GP + (k < GM ? k : SH(Lout) + k)] = 0.f;
    }
    float* W2 = Et + (SH(has_excit) ? a.S * SH(Cout) * SH(Lout) : 0);
    float* We = W2 + nW2;
    weights4_commit(wregs, W2, a.w2, nW2, We, a.we, nWe, nullptr, nullptr, 0, nullptr, nullptr, 0);
    const ChanMap mo = chan_map(SH(Cout)), mi = chan_map(SH(Cin));
    const int kind2 = conv_kind(cv2);
    const float sl2 = mo.active ? a.slope2[mo.c] : 1.f;
    const float sls = (mo.active && SH(has_short)) ? a.ss[mo.c] : 1.f;
    const float sle = mo.active ? a.se[mo.c] : 1.f;       // slope of E3 (has_excit) or of E2 (Cin == Cout)
    double d2 = 0.0, dss = 0.0, dse = 0.0, p2s = 0.0, p2q = 0.0, pes = 0.0, peq = 0.0;
    // uniform: rows of whole quads, 16-byte aligned tensors, and a group large enough for the wide path to pay
    const bool vec1 = BIG && (SH(Lout) & 3) == 0 && a.S * SH(Lout) >= 256 && aligned16(a.gy.g) && aligned16(a.gy.u) &&
                      aligned16(a.T2) && aligned16(a.Sh) && aligned16(a.Ex) && aligned16(a.dT2) && aligned16(a.dSh) &&
                      aligned16(a.dEx);
    STAMP(2, 2);
    for (int grp = bx; grp < a.ngroups; grp += gx) {
        const int b0 = grp * a.S, nb = min(a.S, a.B - b0);
        __syncthreads();
        STAMP(2, 3);
        if (mo.active && vec1) {
            // 16-byte path: quads of four consecutive positions, two per trip, every load of the trip issued first
            const int L4 = SH(Lout) >> 2, sh4 = sh_lout >= 2 ? sh_lout - 2 : -1, n4 = nb * L4;
            const size_t base = ((size_t)b0 * SH(Cout) + mo.c) * SH(Lout);
            const float gmu = a.gy.has_bn ? gs.mean[mo.c] : 0.f, grs = a.gy.has_bn ? gs.rstd[mo.c] : 1.f;
            const float gm1 = a.gy.has_bn ? gs.m1[mo.c] : 0.f, gm2 = a.gy.has_bn ? gs.m2[mo.c] : 0.f;
            constexpr int U = 2;
            for (int q0 = mo.j; q0 < n4; q0 += U * mo.tpc) {
                float4 gv[U], uv[U], tv[U], sv[U], ev[U];
                size_t gi[U];
                int o[U], og[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int q = q0 + u * mo.tpc;
                    int s, l;
                    split(q < n4 ? q : q0, L4, sh4, &s, &l);
                    gi[u] = base + (size_t)s * SH(Cout) * SH(Lout) + 4 * l;
                    o[u] = q < n4 ? (s * SH(Cout) + mo.c) * SH(Lout) + 4 * l : -1;
                    og[u] = (s * SH(Cout) + mo.c) * GP + GM + 4 * l;
                    gv[u] = *reinterpret_cast<const float4*>(a.gy.g + gi[u]);
                    if (a.gy.has_bn) uv[u] = *reinterpret_cast<const float4*>(a.gy.u + gi[u]);
                    tv[u] = *reinterpret_cast<const float4*>(a.T2 + gi[u]);
                    if (SH(has_short)) sv[u] = *reinterpret_cast<const float4*>(a.Sh + gi[u]);
                    ev[u] = *reinterpret_cast<const float4*>(a.Ex + gi[u]);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (o[u] < 0) continue;
                    const float g4[4] = {gv[u].x, gv[u].y, gv[u].z, gv[u].w}, u4[4] = {uv[u].x, uv[u].y, uv[u].z, uv[u].w};
                    const float t4[4] = {tv[u].x, tv[u].y, tv[u].z, tv[u].w}, s4[4] = {sv[u].x, sv[u].y, sv[u].z, sv[u].w};
                    const float e4[4] = {ev[u].x, ev[u].y, ev[u].z, ev[u].w};
                    float r2[4], rs_[4], re[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float dy = g4[i];
                        if (a.gy.has_bn) {
                            const float y = (u4[i] - gmu) * grs;
                            dy = grs * (dy - gm1 - y * gm2);
                        }
                        r2[i] = t4[i] > 0.f ? dy : dy * sl2;
                        if (t4[i] <= 0.f) d2 += (double)dy * (double)t4[i];
                        if (SH(has_short)) {
                            rs_[i] = s4[i] > 0.f ? dy : dy * sls;
                            if (s4[i] <= 0.f) dss += (double)dy * (double)s4[i];
                        } else {
                            rs_[i] = dy;
                        }
                        re[i] = e4[i] > 0.f ? dy : dy * sle;
                        if (e4[i] <= 0.f) dse += (double)dy * (double)e4[i];
                    }
                    const float4 v2 = make_float4(r2[0], r2[1], r2[2], r2[3]), ve = make_float4(re[0], re[1], re[2], re[3]);
                    *reinterpret_cast<float4*>(a.dT2 + gi[u]) = v2;
                    *reinterpret_cast<float4*>(Gt + og[u]) = v2;
                    *reinterpret_cast<float4*>(a.dSh + gi[u]) = make_float4(rs_[0], rs_[1], rs_[2], rs_[3]);
                    *reinterpret_cast<float4*>(a.dEx + gi[u]) = ve;
                    if (SH(has_excit)) *reinterpret_cast<float4*>(Et + o[u]) = ve;
                }
            }
        } else if (mo.active) {
            const int n = nb * SH(Lout);
            for (int q = mo.j; q < n; q += mo.tpc) {
                int s, l;
                split(q, SH(Lout), sh_lout, &s, &l);
                const size_t idx = ((size_t)(b0 + s) * SH(Cout) + mo.c) * SH(Lout) + l;
                const int o = (s * SH(Cout) + mo.c) * SH(Lout) + l;
                float dy = a.gy.g[idx];
                if (a.gy.has_bn) {
                    const float y = (a.gy.u[idx] - gs.mean[mo.c]) * gs.rstd[mo.c];
                    dy = gs.rstd[mo.c] * (dy - gs.m1[mo.c] - y * gs.m2[mo.c]);
                }
                const float t2 = a.T2[idx];
                float v = t2 > 0.f ? dy : dy * sl2;
                if (t2 <= 0.f) d2 += (double)dy * (double)t2;
                a.dT2[idx] = v; Gt[(s * SH(Cout) + mo.c) * GP + GM + l] = v;
                if (SH(has_short)) {
                    const float sh = a.Sh[idx];
                    a.dSh[idx] = sh > 0.f ? dy : dy * sls;
                    if (sh <= 0.f) dss += (double)dy * (double)sh;
                } else {
                    a.dSh[idx] = dy;
                }
                const float ex = a.Ex[idx];               // E3 raw (has_excit) or E2 raw
                v = ex > 0.f ? dy : dy * sle;
                if (ex <= 0.f) dse += (double)dy * (double)ex;
                a.dEx[idx] = v;
                if (SH(has_excit)) Et[o] = v;
            }
        }
        __syncthreads();
        STAMP(2, 4);
        // conv2^T: dBn2[s][c1][l1]  (conv2 is Cout -> Cout)
        if constexpr (kStripB) {
            if (mo.active) {
                constexpr int K2 = kBlk[KIND < 0 ? 0 : KIND].cv2.K, CO = kBlk[KIND < 0 ? 0 : KIND].Cout;
                const int L4 = SH(L1) >> 2, n4 = nb * L4;
                const float tsl = a.vT1.slope ? a.vT1.slope[mo.c] : 1.f, tmu = vs1.mean[mo.c], trs = vs1.rstd[mo.c];
                for (int q = mo.j; q < n4; q += mo.tpc) {
                    const int sidx = q / L4, l0 = 4 * (q - sidx * L4);
                    const size_t idx = ((size_t)(b0 + sidx) * SH(Cout) + mo.c) * SH(L1) + l0;
                    float4 t1 = *reinterpret_cast<const float4*>(a.vT1.raw + idx);       // for y of the BatchNorm backward
                    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int co = 0; co < CO; ++co) {
                        float xw[Strip<K2>::NV4 * 4];
                        strip_window<K2>(Gt + (sidx * CO + co) * GP + GM, l0, xw);
                        strip_fma<K2, true>(W2 + (co * CO + mo.c) * K2, xw, acc);
                    }
                    *reinterpret_cast<float4*>(a.dBn2 + idx) = make_float4(acc[0], acc[1], acc[2], acc[3]);
                    if (a.vT1.slope) t1 = prelu4(t1, tsl);
                    const float y0 = (t1.x - tmu) * trs, y1 = (t1.y - tmu) * trs, y2 = (t1.z - tmu) * trs, y3 = (t1.w - tmu) * trs;
                    p2s += (double)((acc[0] + acc[1]) + (acc[2] + acc[3]));
                    p2q += (double)(acc[0] * y0 + acc[1] * y1) + (double)(acc[2] * y2 + acc[3] * y3);
                }
            }
        } else
        if (mo.active && vec1 && (SH(L1) & 3) == 0 && aligned16(a.vT1.raw) && aligned16(a.dBn2)) {
            // large batches: four consecutive positions per thread -- the global operand (T1, for y of the BatchNorm
            // backward) is one 16-byte load issued ahead of the four transposed-conv sums, the result one 16-byte store
            // (one dependent 4-byte round trip per output otherwise)
            const int L4 = SH(L1) >> 2, n4 = nb * L4;
            const float tsl = a.vT1.slope ? a.vT1.slope[mo.c] : 1.f, tmu = vs1.mean[mo.c], trs = vs1.rstd[mo.c];
            for (int q = mo.j; q < n4; q += mo.tpc) {
                const int sidx = q / L4, l0 = 4 * (q - sidx * L4);
                const size_t idx = ((size_t)(b0 + sidx) * SH(Cout) + mo.c) * SH(L1) + l0;
                float4 t1 = *reinterpret_cast<const float4*>(a.vT1.raw + idx);
                const float* gs = Gt + sidx * SH(Cout) * SH(Lout);
                const float a0 = conv_bwd_elem_fast(kind2, cv2, W2, gs, mo.c, l0);
                const float a1 = conv_bwd_elem_fast(kind2, cv2, W2, gs, mo.c, l0 + 1);
                const float a2 = conv_bwd_elem_fast(kind2, cv2, W2, gs, mo.c, l0 + 2);
                const float a3 = conv_bwd_elem_fast(kind2, cv2, W2, gs, mo.c, l0 + 3);
                *reinterpret_cast<float4*>(a.dBn2 + idx) = make_float4(a0, a1, a2, a3);
                if (a.vT1.slope) t1 = prelu4(t1, tsl);
                p2s += (double)((a0 + a1) + (a2 + a3));
                p2q += (double)(a0 * ((t1.x - tmu) * trs) + a1 * ((t1.y - tmu) * trs)) +
                       (double)(a2 * ((t1.z - tmu) * trs) + a3 * ((t1.w - tmu) * trs));
            }
        } else
        if (mo.active) {
            const int n = nb * SH(L1);
            for (int q = mo.j; q < n; q += mo.tpc) {
                int s, l;
                split(q, SH(L1), sh_l1, &s, &l);
                const float acc = conv_bwd_elem_fast(kind2, cv2, W2, Gt + s * SH(Cout) * SH(Lout), mo.c, l);
                const size_t idx = ((size_t)(b0 + s) * SH(Cout) + mo.c) * SH(L1) + l;
                a.dBn2[idx] = acc;
                const float y = view_y(a.vT1, &vs1, mo.c, idx);
                p2s += (double)acc; p2q += (double)acc * (double)y;
            }
        }
        // conv_excit^T (1x1 grouped): dBnE[s][ci][lo]
        if (SH(has_excit) && mi.active && vec1 && cve.K == 1 && cve.stride == 1 && !cve.transposed &&
            aligned16(a.vE2.raw) && aligned16(a.dBnE)) {
            // 1x1 grouped conv_excit, transposed: dBnE[ci][l] = sum_{co in ci's group} w[co][ci local] dE3[co][l]; quads
            const int L4 = SH(Lout) >> 2, n4 = nb * L4;
            const int cig = cve.Cin / cve.groups, cog = cve.Cout / cve.groups;
            const int gI = mi.c / cig, cil = mi.c - gI * cig;
            const float esl = a.vE2.slope ? a.vE2.slope[mi.c] : 1.f, emu = vse.mean[mi.c], ers = vse.rstd[mi.c];
            for (int q = mi.j; q < n4; q += mi.tpc) {
                const int sidx = q / L4, l0 = 4 * (q - sidx * L4);
                const size_t idx = ((size_t)(b0 + sidx) * SH(Cin) + mi.c) * SH(Lout) + l0;
                float4 e2 = *reinterpret_cast<const float4*>(a.vE2.raw + idx);
                float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
                for (int col = 0; col < cog; ++col) {
                    const int co = gI * cog + col;
                    const float w = We[co * cig + cil];
                    const float4 gq = *reinterpret_cast<const float4*>(Et + (sidx * SH(Cout) + co) * SH(Lout) + l0);
                    acc.x = fmaf(w, gq.x, acc.x); acc.y = fmaf(w, gq.y, acc.y); acc.z = fmaf(w, gq.z, acc.z); acc.w = fmaf(w, gq.w, acc.w);
                }
                *reinterpret_cast<float4*>(a.dBnE + idx) = acc;
                if (a.vE2.slope) e2 = prelu4(e2, esl);
                pes += (double)((acc.x + acc.y) + (acc.z + acc.w));
                peq += (double)(acc.x * ((e2.x - emu) * ers) + acc.y * ((e2.y - emu) * ers)) +
                       (double)(acc.z * ((e2.z - emu) * ers) + acc.w * ((e2.w - emu) * ers));
            }
        } else
        if (SH(has_excit) && mi.active) {
            const int n = nb * SH(Lout);
            for (int q = mi.j; q < n; q += mi.tpc) {
                int s, l;
                split(q, SH(Lout), sh_lout, &s, &l);
                const float acc = conv_bwd_elem(cve, We, Et + s * SH(Cout) * SH(Lout), mi.c, l);
                const size_t idx = ((size_t)(b0 + s) * SH(Cin) + mi.c) * SH(Lout) + l;
                a.dBnE[idx] = acc;
                const float y = view_y(a.vE2, &vse, mi.c, idx);
                pes += (double)acc; peq += (double)acc * (double)y;
            }
        }
    }
    STAMP(2, 5);
    if (SH(has_excit)) chan_reduce(pes, peq, SH(Cin), mi, a.pdBnE + (size_t)bx * SH(Cin) * 2, scr, scr2);
    const size_t slab = (size_t)bx * (size_t)a.slab_stride;
    // the five per-output-channel sums in one butterfly: {sum dBn2, sum dBn2*y, dslope2, dslope_short, dslope_e3}
    __shared__ double res8[8 * CT_MAXCH];
    double v8[8] = {p2s, p2q, d2, dss, dse, 0.0, 0.0, 0.0};
    chan_reduce_n<8>(v8, SH(Cout), mo, res8, scr, scr2);
    __syncthreads();
    STAMP(2, 6);
    if ((int)threadIdx.x < SH(Cout)) {
        const double* r = res8 + threadIdx.x * 8;
        double* pp = a.pdBn2 + ((size_t)bx * SH(Cout) + threadIdx.x) * 2;
        pp[0] = r[0]; pp[1] = r[1];
        a.dslope2[slab + threadIdx.x] = (float)r[2];
        if (SH(has_short)) a.dslope_s[slab + threadIdx.x] = (float)r[3];
        a.dslope_e[slab + threadIdx.x] = (float)r[4];
    }
}
#undef SH

template <int KIND, bool BIG = false>
__global__ __launch_bounds__(256) void block_bwd_b_kernel(BlockBwdBArgs ka) {
    extern __shared__ __attribute__((aligned(16))) float dyn[];
    __shared__ BlockBwdBArgs sa;
    const BlockBwdBArgs& a = raae::args_to_lds(&sa);
    block_bwd_b_body<KIND, BIG>(a, blockIdx.x, gridDim.x, dyn);
}
template <int KIND, bool BIG = false>
__global__ __launch_bounds__(256) void block_bwd_b_kernel_m(const BlockBwdBArgs* table) {
    extern __shared__ __attribute__((aligned(16))) float dyn[];
    __shared__ BlockBwdBArgs sa;
    const BlockBwdBArgs& a = raae::args_from_table(&sa, table);
    block_bwd_b_body<KIND, BIG>(a, blockIdx.x, gridDim.x, dyn);
}

typedef raae_block_bwd_a_t BlockBwdAArgs;

template <int KIND, bool BIG>        // see block_fwd_a_kernel
__device__ __forceinline__ void block_bwd_a_body(const BlockBwdAArgs& a, const int bx, const int gx, float* dyn) {
#define SH(f) (KIND >= 0 ? kBlk[KIND < 0 ? 0 : KIND].f : a.f)
    constexpr bool kHalo1 = KIND >= 0 && !kBlk[KIND < 0 ? 0 : KIND].cv1.transposed && kBlk[KIND < 0 ? 0 : KIND].cv1.pad_replicate &&
                            kBlk[KIND < 0 ? 0 : KIND].Lin % 8 == 0 && kBlk[KIND < 0 ? 0 : KIND].cv1.pad <= 7 &&
                            (256 / kBlk[KIND < 0 ? 0 : KIND].Cin) % 8 == 0;
    const raae_conv_t cv1 = SH(cv1), cvs = SH(cvs);
    const int sh_lin = KIND >= 0 ? clg2(SH(Lin)) : a.sh_lin;
    const int sh_l1 = KIND >= 0 ? clg2(SH(L1)) : a.sh_l1;
    const int sh_lout = KIND >= 0 ? clg2(SH(Lout)) : a.sh_lout;
    const int sh_e = KIND >= 0 ? clg2(SH(E)) : a.sh_e;
    __shared__ GradStats g1, ge;
    __shared__ ViewStats vs;
    __shared__ double scr[512], scr2[2 * CT_MAXCH * 8], res[2 * CT_MAXCH];
    STAMP(3, 0);
    const int nW1 = conv_nw_dev(cv1), nWs = SH(has_short) ? conv_nw_dev(cvs) : 0;
    const WeightRegs wregs = weights4_issue(a.w1, nW1, a.ws, nWs, a.wf1, SH(E) * SH(Lin), a.wf2, SH(Lout) * SH(E));
    {   // dBn2 through bn2 / PReLU1 -> dT1 ; dBnE through bn_excit / PReLU_e2 -> dE2 ; bn1 of the block input
        const raae::StatJob jobs[5] = {
            raae::stat_job_bn(a.g1.bn, SH(Cout), g1.mean, g1.rstd, false),
            raae::stat_job_bwd(a.g1.g_partials, a.g1.g_nparts, SH(Cout), a.g1.bn.count, g1.m1, g1.m2),
            SH(has_excit) ? raae::stat_job_bn(a.ge.bn, SH(Cin), ge.mean, ge.rstd, false) : raae::stat_job_none(),
            SH(has_excit) ? raae::stat_job_bwd(a.ge.g_partials, a.ge.g_nparts, SH(Cin), a.ge.bn.count, ge.m1, ge.m2)
                        : raae::stat_job_none(),
            a.in.has_bn ? raae::stat_job_bn(a.in.bn, SH(Cin), vs.mean, vs.rstd, false) : raae::stat_job_none()};
        raae::stat_jobs<5, CT_MAXCH>(jobs, false);
    }
    STAMP(3, 1);
    // strip-capable conv1 (and no conv_short): the dT1 tile rows carry an 8-float zero margin (strip_window)
    constexpr bool kStripA = KIND >= 0 && strip_conv_ok(kBlk[KIND < 0 ? 0 : KIND].cv1) && !kBlk[KIND < 0 ? 0 : KIND].has_short;
    constexpr int G1M = kStripA ? kStripMargin : 0;
    const int G1P = SH(L1) + 2 * G1M;
    float* G1 = dyn;                                      // dT1 [S][Cout][G1P]
    float* Gs = G1 + a.S * SH(Cout) * G1P;                    // dSh [S][Cout][Lout]
    float* Ge = Gs + a.S * SH(Cout) * SH(Lout);               // dE2 [S][Cin][Lout]
    float* De = Ge + a.S * SH(Cin) * SH(Lout);                // dE1 [S][Cin][E]
    float* W1 = De + a.S * SH(Cin) * SH(E);
    float* Wsh = W1 + nW1;
    float* Wf1 = Wsh + nWs;                               // [E][Lin]
    float* Wf2 = Wf1 + SH(E) * SH(Lin);                       // [Lout][E]
    weights4_commit(wregs, W1, a.w1, nW1, Wsh, a.ws, nWs, Wf1, a.wf1, SH(E) * SH(Lin), Wf2, a.wf2, SH(Lout) * SH(E));
    if (G1M > 0) for (int i = threadIdx.x; i < a.S * SH(Cout) * 2 * G1M; i += 256) {
        const int row = i / (2 * G1M), k = i - row * 2 * G1M;
        G1[row * G1P + (k < G1M ? k : SH(L1) + k)] = 0.f;
    }
    const ChanMap mo = chan_map(SH(Cout)), mi = chan_map(SH(Cin));
    const int kind1 = conv_kind(cv1), kinds = SH(has_short) ? conv_kind(cvs) : 0;
    const float sle1 = mi.active ? a.se1[mi.c] : 1.f;
    const int sub = (SH(Lout) >= 64 && (mi.tpc & 15) == 0) ? 16 : 1;
    const int jj = mi.j / sub, lane_sub = mi.j - jj * sub, tpo = mi.tpc / sub;
    double d1 = 0.0, de2 = 0.0, de1 = 0.0, prs = 0.0, prq = 0.0;
    // uniform: every staged row is whole quads, tensors 16-byte aligned, the group large enough for the wide path
    const bool vecA = BIG && ((SH(L1) | SH(Lout)) & 3) == 0 && a.S * SH(Lout) >= 256 && aligned16(a.g1.g) &&
                      aligned16(a.g1.raw) && aligned16(a.g1.u) && aligned16(a.dT1) && aligned16(a.dSh) &&
                      aligned16(a.dE2) && (!SH(has_excit) || (aligned16(a.ge.g) && aligned16(a.ge.raw) && aligned16(a.ge.u)));
    STAMP(3, 2);
    for (int grp = bx; grp < a.ngroups; grp += gx) {
        const int b0 = grp * a.S, nb = min(a.S, a.B - b0);
        __syncthreads();
        STAMP(3, 3);
        if (mo.active && vecA) {
            // 16-byte path (see block_bwd_b_body): dT1 quads through the BatchNorm / PReLU backward, dSh quads copied
            {
                const int L4 = SH(L1) >> 2, sh4 = sh_l1 >= 2 ? sh_l1 - 2 : -1, n4 = nb * L4;
                const size_t base = ((size_t)b0 * SH(Cout) + mo.c) * SH(L1);
                const bool hb = a.g1.has_bn != 0, hu = a.g1.u != nullptr, hr = a.g1.raw != nullptr;
                const float sl = a.g1.slope ? a.g1.slope[mo.c] : 1.f;
                const float mu = hb ? g1.mean[mo.c] : 0.f, rs = hb ? g1.rstd[mo.c] : 1.f;
                const float m1 = hb ? g1.m1[mo.c] : 0.f, m2 = hb ? g1.m2[mo.c] : 0.f;
                const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
                constexpr int U = 4;
                for (int q0 = mo.j; q0 < n4; q0 += U * mo.tpc) {
                    float4 gv[U], rv[U], uv[U];
                    size_t gi[U];
                    int o[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int q = q0 + u * mo.tpc;
                        int s, l;
                        split(q < n4 ? q : q0, L4, sh4, &s, &l);
                        gi[u] = base + (size_t)s * SH(Cout) * SH(L1) + 4 * l;
                        o[u] = q < n4 ? (s * SH(Cout) + mo.c) * G1P + G1M + 4 * l : -1;
                        gv[u] = *reinterpret_cast<const float4*>(a.g1.g + gi[u]);
                        rv[u] = hr ? *reinterpret_cast<const float4*>(a.g1.raw + gi[u]) : zero4;
                        uv[u] = (hu && hb) ? *reinterpret_cast<const float4*>(a.g1.u + gi[u]) : zero4;
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        if (o[u] < 0) continue;
                        const Grad4 r = grad_quad(a.g1, gv[u], rv[u], uv[u], hu, sl, mu, rs, m1, m2);
                        if (r.raw.x <= 0.f) d1 += (double)r.da.x * (double)r.raw.x;
                        if (r.raw.y <= 0.f) d1 += (double)r.da.y * (double)r.raw.y;
                        if (r.raw.z <= 0.f) d1 += (double)r.da.z * (double)r.raw.z;
                        if (r.raw.w <= 0.f) d1 += (double)r.da.w * (double)r.raw.w;
                        *reinterpret_cast<float4*>(G1 + o[u]) = r.dr;
                        *reinterpret_cast<float4*>(a.dT1 + gi[u]) = r.dr;
                    }
                }
            }
            {
                const int L4 = SH(Lout) >> 2, sh4 = sh_lout >= 2 ? sh_lout - 2 : -1, n4 = nb * L4;
                const size_t base = ((size_t)b0 * SH(Cout) + mo.c) * SH(Lout);
                // four quads per trip, the loads ahead of the stores (explicit temporaries: a private array here was
                // left in scratch memory by the compiler)
                const float* src = a.dSh + base;
                for (int q0 = mo.j; q0 < n4; q0 += 4 * mo.tpc) {
                    const int qa = q0, qb = q0 + mo.tpc, qc = q0 + 2 * mo.tpc, qd = q0 + 3 * mo.tpc;
                    int sa, la, sb, lb, sc, lc, sd, ld;
                    split(qa, L4, sh4, &sa, &la);
                    split(qb < n4 ? qb : qa, L4, sh4, &sb, &lb);
                    split(qc < n4 ? qc : qa, L4, sh4, &sc, &lc);
                    split(qd < n4 ? qd : qa, L4, sh4, &sd, &ld);
                    const float4 va = *reinterpret_cast<const float4*>(src + (size_t)sa * SH(Cout) * SH(Lout) + 4 * la);
                    const float4 vb = *reinterpret_cast<const float4*>(src + (size_t)sb * SH(Cout) * SH(Lout) + 4 * lb);
                    const float4 vc = *reinterpret_cast<const float4*>(src + (size_t)sc * SH(Cout) * SH(Lout) + 4 * lc);
                    const float4 vd = *reinterpret_cast<const float4*>(src + (size_t)sd * SH(Cout) * SH(Lout) + 4 * ld);
                    *reinterpret_cast<float4*>(Gs + (sa * SH(Cout) + mo.c) * SH(Lout) + 4 * la) = va;
                    if (qb < n4) *reinterpret_cast<float4*>(Gs + (sb * SH(Cout) + mo.c) * SH(Lout) + 4 * lb) = vb;
                    if (qc < n4) *reinterpret_cast<float4*>(Gs + (sc * SH(Cout) + mo.c) * SH(Lout) + 4 * lc) = vc;
                    if (qd < n4) *reinterpret_cast<float4*>(Gs + (sd * SH(Cout) + mo.c) * SH(Lout) + 4 * ld) = vd;
                }
            }
        } else if (mo.active) {
            const int n1 = nb * SH(L1);                     // dT1 (+ dslope1)
            for (int q = mo.j; q < n1; q += mo.tpc) {
                int s, l;
                split(q, SH(L1), sh_l1, &s, &l);
                const int o = (s * SH(Cout) + mo.c) * SH(L1) + l;
                float da, raw;
                const float v = grad_at(a.g1, &g1, mo.c, (size_t)b0 * SH(Cout) * SH(L1) + o, &da, &raw);
                if (raw <= 0.f) d1 += (double)da * (double)raw;
                G1[(s * SH(Cout) + mo.c) * G1P + G1M + l] = v; a.dT1[(size_t)b0 * SH(Cout) * SH(L1) + o] = v;
            }
            const int n2 = nb * SH(Lout);                   // dSh: plain copy
            for (int q = mo.j; q < n2; q += mo.tpc) {
                int s, l;
                split(q, SH(Lout), sh_lout, &s, &l);
                const int o = (s * SH(Cout) + mo.c) * SH(Lout) + l;
                Gs[o] = a.dSh[(size_t)b0 * SH(Cout) * SH(Lout) + o];
            }
        }
        STAMP(3, 4);
        if (mi.active && vecA) {                          // dE2, 16-byte path
            const int L4 = SH(Lout) >> 2, sh4 = sh_lout >= 2 ? sh_lout - 2 : -1, n4 = nb * L4;
            const size_t base = ((size_t)b0 * SH(Cin) + mi.c) * SH(Lout);
            const bool hb = SH(has_excit) && a.ge.has_bn != 0, hu = SH(has_excit) && a.ge.u != nullptr;
            const bool hr = SH(has_excit) && a.ge.raw != nullptr;
            const float sl = (SH(has_excit) && a.ge.slope) ? a.ge.slope[mi.c] : 1.f;
            const float mu = hb ? ge.mean[mi.c] : 0.f, rs = hb ? ge.rstd[mi.c] : 1.f;
            const float m1 = hb ? ge.m1[mi.c] : 0.f, m2 = hb ? ge.m2[mi.c] : 0.f;
            const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
            constexpr int U = 4;
            for (int q0 = mi.j; q0 < n4; q0 += U * mi.tpc) {
                float4 gv[U], rv[U], uv[U];
                size_t gi[U];
                int o[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int q = q0 + u * mi.tpc;
                    int s, l;
                    split(q < n4 ? q : q0, L4, sh4, &s, &l);
                    gi[u] = base + (size_t)s * SH(Cin) * SH(Lout) + 4 * l;
                    o[u] = q < n4 ? (s * SH(Cin) + mi.c) * SH(Lout) + 4 * l : -1;
                    if (SH(has_excit)) {
                        gv[u] = *reinterpret_cast<const float4*>(a.ge.g + gi[u]);
                        rv[u] = hr ? *reinterpret_cast<const float4*>(a.ge.raw + gi[u]) : zero4;
                        uv[u] = (hu && hb) ? *reinterpret_cast<const float4*>(a.ge.u + gi[u]) : zero4;
                    } else {
                        gv[u] = *reinterpret_cast<const float4*>(a.dE2 + gi[u]);       // materialised by phase B
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (o[u] < 0) continue;
                    float4 v = gv[u];
                    if (SH(has_excit)) {
                        const Grad4 r = grad_quad(a.ge, gv[u], rv[u], uv[u], hu, sl, mu, rs, m1, m2);
                        if (r.raw.x <= 0.f) de2 += (double)r.da.x * (double)r.raw.x;
                        if (r.raw.y <= 0.f) de2 += (double)r.da.y * (double)r.raw.y;
                        if (r.raw.z <= 0.f) de2 += (double)r.da.z * (double)r.raw.z;
                        if (r.raw.w <= 0.f) de2 += (double)r.da.w * (double)r.raw.w;
                        v = r.dr;
                        *reinterpret_cast<float4*>(a.dE2 + gi[u]) = v;
                    }
                    *reinterpret_cast<float4*>(Ge + o[u]) = v;
                }
            }
        } else if (mi.active) {                           // dE2
            const int n2 = nb * SH(Lout);
            for (int q = mi.j; q < n2; q += mi.tpc) {
                int s, l;
                split(q, SH(Lout), sh_lout, &s, &l);
                const int o = (s * SH(Cin) + mi.c) * SH(Lout) + l;
                const size_t idx = (size_t)b0 * SH(Cin) * SH(Lout) + o;
                float v;
                if (SH(has_excit)) {
                    float da, raw;
                    v = grad_at(a.ge, &ge, mi.c, idx, &da, &raw);
                    if (raw <= 0.f) de2 += (double)da * (double)raw;
                    a.dE2[idx] = v;
                } else {
                    v = a.dE2[idx];                       // materialised by phase B
                }
                Ge[o] = v;
            }
        }
        __syncthreads();
        STAMP(3, 5);
        // fc2^T: dE1a[s][ci][e] = sum_lo wf2[lo][e] dE2[s][ci][lo];  dE1 = dE1a * PReLUe1'(E1)
        if (mi.active) {
            const int n = nb * SH(E), nloop = (n + tpo - 1) / tpo;
            for (int it = 0; it < nloop; ++it) {
                const int q = jj + it * tpo;
                const bool ok = q < n && jj < tpo;
                int s = 0, e = 0;
                if (ok) split(q, SH(E), sh_e, &s, &e);
                const float* gr = Ge + (s * SH(Cin) + mi.c) * SH(Lout);
                // E1 is requested BEFORE the reduction it gates (behind it, it was one more dependent global round trip
                // per pass: 3-6 us per sample group at 4096 rows)
                const size_t idx = ((size_t)(b0 + s) * SH(Cin) + mi.c) * SH(E) + e;
                const float e1 = (ok && lane_sub == 0) ? a.E1[idx] : 0.f;
                float acc = 0.f;
                if (ok) for (int l = lane_sub; l < SH(Lout); l += sub) acc += Wf2[l * SH(E) + e] * gr[l];
                if (sub == 16) {
                    acc += __shfl_xor(acc, 1, 64); acc += __shfl_xor(acc, 2, 64);
                    acc += __shfl_xor(acc, 4, 64); acc += __shfl_xor(acc, 8, 64);
                }
                if (ok && lane_sub == 0) {
                    const float v = e1 > 0.f ? acc : acc * sle1;
                    if (e1 <= 0.f) de1 += (double)acc * (double)e1;
                    a.dE1[idx] = v;
                    De[(s * SH(Cin) + mi.c) * SH(E) + e] = v;
                }
            }
        }
        __syncthreads();
        STAMP(3, 6);
        // dR[s][ci][li] = conv1^T dT1 + short^T dSh | dSh + mask * sum_e wf1[e][li] dE1[s][ci][e]
        if constexpr (kStripA) {
            if (a.dR != nullptr && mi.active) {
                constexpr int K1 = kBlk[KIND < 0 ? 0 : KIND].cv1.K, CI = kBlk[KIND < 0 ? 0 : KIND].Cin, CO = kBlk[KIND < 0 ? 0 : KIND].Cout;
                constexpr int PAD1 = (K1 - 1) / 2, NE = kBlk[KIND < 0 ? 0 : KIND].E;
                const int L4 = SH(Lin) >> 2, n4 = nb * L4;
                const float xmu = a.in.has_bn ? vs.mean[mi.c] : 0.f, xrs = a.in.has_bn ? vs.rstd[mi.c] : 1.f;
                const float xsl = a.in.slope ? a.in.slope[mi.c] : 1.f;
                for (int q = mi.j; q < n4; q += mi.tpc) {
                    const int sidx = q / L4, l0 = 4 * (q - sidx * L4);
                    const size_t idx = ((size_t)(b0 + sidx) * SH(Cin) + mi.c) * SH(Lin) + l0;
                    // global operands first: dropout mask, and the block input for y of bn1's backward
                    float4 mk = make_float4(1.f, 1.f, 1.f, 1.f), xr = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (a.mask) mk = *reinterpret_cast<const float4*>(a.mask + idx);
                    if (a.pdR) xr = *reinterpret_cast<const float4*>(a.in.raw + idx);
                    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int co = 0; co < CO; ++co) {
                        float xw[Strip<K1>::NV4 * 4];
                        strip_window<K1>(G1 + (sidx * CO + co) * G1P + G1M, l0, xw);
                        strip_fma<K1, true>(W1 + (co * CI + mi.c) * K1, xw, acc);
                    }
                    if (cv1.pad_replicate && (l0 == 0 || l0 == SH(Lin) - 4)) {
                        // replicate padding: the gradient of the PAD halo positions on each side belongs to the edge
                        // element.  Summed over the halo, output l meets the first (left) / last (right) PAD - l' taps:
                        //   dR[0]   += sum_co sum_{n=1..PAD} g[co][PAD - n]     * (w[0] + ... + w[n-1])
                        //   dR[L-1] += sum_co sum_{n=1..PAD} g[co][L-1-PAD + n] * (w[K-n] + ... + w[K-1])
                        const bool left = l0 == 0;
                        float e = 0.f;
#pragma unroll
                        for (int co = 0; co < CO; ++co) {
                            const float* wv = W1 + (co * CI + mi.c) * K1;
                            const float* gr = G1 + (sidx * CO + co) * G1P + G1M;
                            float run = 0.f;
#pragma unroll
                            for (int n = 1; n <= PAD1; ++n) {
                                run += left ? wv[n - 1] : wv[K1 - n];
                                e = fmaf(left ? gr[PAD1 - n] : gr[SH(L1) - 1 - PAD1 + n], run, e);
                            }
                        }
                        if (left) acc[0] += e; else acc[3] += e;
                    }
                    const float4 gsq = *reinterpret_cast<const float4*>(Gs + (sidx * SH(Cout) + mi.c) * SH(Lout) + l0);
                    float fe[4] = {0.f, 0.f, 0.f, 0.f};
                    const float* dr = De + (sidx * SH(Cin) + mi.c) * SH(E);
#pragma unroll
                    for (int e = 0; e < NE; ++e) {
                        const float4 wq = *reinterpret_cast<const float4*>(Wf1 + e * SH(Lin) + l0);
                        const float de = dr[e];
                        fe[0] = fmaf(wq.x, de, fe[0]); fe[1] = fmaf(wq.y, de, fe[1]);
                        fe[2] = fmaf(wq.z, de, fe[2]); fe[3] = fmaf(wq.w, de, fe[3]);
                    }
                    const float o0 = acc[0] + gsq.x + fe[0] * mk.x, o1 = acc[1] + gsq.y + fe[1] * mk.y;
                    const float o2 = acc[2] + gsq.z + fe[2] * mk.z, o3 = acc[3] + gsq.w + fe[3] * mk.w;
                    *reinterpret_cast<float4*>(a.dR + idx) = make_float4(o0, o1, o2, o3);
                    if (a.pdR) {
                        if (a.in.slope) xr = prelu4(xr, xsl);
                        const float y0 = (xr.x - xmu) * xrs, y1 = (xr.y - xmu) * xrs, y2 = (xr.z - xmu) * xrs, y3 = (xr.w - xmu) * xrs;
                        prs += (double)((o0 + o1) + (o2 + o3));
                        prq += (double)(o0 * y0 + o1 * y1) + (double)(o2 * y2 + o3 * y3);
                    }
                }
            }
        } else
        if (!kHalo1 && vecA && (SH(Lin) & 3) == 0 && a.dR != nullptr && mi.active && aligned16(a.dR) && aligned16(a.mask) &&
            aligned16(a.in.raw)) {
            // large batches, four consecutive positions per thread: dropout mask and block input (y of bn1's backward)
            // arrive as 16-byte loads ahead of the sums, dR leaves as one 16-byte store
            const int L4 = SH(Lin) >> 2, n4 = nb * L4;
            const float xmu = a.in.has_bn ? vs.mean[mi.c] : 0.f, xrs = a.in.has_bn ? vs.rstd[mi.c] : 1.f;
            const float xsl = a.in.slope ? a.in.slope[mi.c] : 1.f;
            for (int q = mi.j; q < n4; q += mi.tpc) {
                const int sidx = q / L4, l0 = 4 * (q - sidx * L4);
                const size_t idx = ((size_t)(b0 + sidx) * SH(Cin) + mi.c) * SH(Lin) + l0;
                float4 mk = make_float4(1.f, 1.f, 1.f, 1.f), xr = make_float4(0.f, 0.f, 0.f, 0.f);
                if (a.mask) mk = *reinterpret_cast<const float4*>(a.mask + idx);
                if (a.pdR) xr = *reinterpret_cast<const float4*>(a.in.raw + idx);
                const float* g1p = G1 + sidx * SH(Cout) * G1P + G1M;      // (G1M == 0 here: plain [Cout][L1] rows)
                const float* gsp = Gs + sidx * SH(Cout) * SH(Lout);
                const float* dr = De + (sidx * SH(Cin) + mi.c) * SH(E);
                float o[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int l = l0 + r;
                    float acc = conv_bwd_elem_fast(kind1, cv1, W1, g1p, mi.c, l);
                    if (SH(has_short)) acc += conv_bwd_elem_fast(kinds, cvs, Wsh, gsp, mi.c, l);
                    else acc += gsp[mi.c * SH(Lout) + l];
                    float fe = 0.f;
                    for (int e = 0; e < SH(E); ++e) fe += Wf1[e * SH(Lin) + l] * dr[e];
                    o[r] = acc + fe * (r == 0 ? mk.x : r == 1 ? mk.y : r == 2 ? mk.z : mk.w);
                }
                *reinterpret_cast<float4*>(a.dR + idx) = make_float4(o[0], o[1], o[2], o[3]);
                if (a.pdR) {
                    if (a.in.slope) xr = prelu4(xr, xsl);
                    prs += (double)((o[0] + o[1]) + (o[2] + o[3]));
                    prq += (double)(o[0] * ((xr.x - xmu) * xrs) + o[1] * ((xr.y - xmu) * xrs)) +
                           (double)(o[2] * ((xr.z - xmu) * xrs) + o[3] * ((xr.w - xmu) * xrs));
                }
            }
        } else
        if (a.dR != nullptr && mi.active) {
            const int n = nb * SH(Lin);
            for (int q = mi.j; q < n; q += mi.tpc) {
                int s, l;
                split(q, SH(Lin), sh_lin, &s, &l);
                float acc;
                if constexpr (kHalo1) {
                    // own position through the unrolled taps; the replicate-halo positions are spread over the
                    // lanes next to each edge (conv_bwd_halo_t) instead of serialised on the edge lane
                    constexpr int K1 = kBlk[KIND < 0 ? 0 : KIND].cv1.K, S1 = kBlk[KIND < 0 ? 0 : KIND].cv1.stride;
                    const float* g1p = G1 + s * SH(Cout) * SH(L1);
                    acc = conv_bwd_elem_t<K1, S1, false, true>(cv1, W1, g1p, mi.c, l) +
                          conv_bwd_halo_t<K1, S1>(cv1, W1, g1p, mi.c, l);
                } else {
                    acc = conv_bwd_elem_fast(kind1, cv1, W1, G1 + s * SH(Cout) * SH(L1), mi.c, l);
                }
                if (SH(has_short)) acc += conv_bwd_elem_fast(kinds, cvs, Wsh, Gs + s * SH(Cout) * SH(Lout), mi.c, l);
                else acc += Gs[(s * SH(Cout) + mi.c) * SH(Lout) + l];
                float fe = 0.f;
                const float* dr = De + (s * SH(Cin) + mi.c) * SH(E);
                for (int e = 0; e < SH(E); ++e) fe += Wf1[e * SH(Lin) + l] * dr[e];
                const size_t idx = ((size_t)(b0 + s) * SH(Cin) + mi.c) * SH(Lin) + l;
                if (a.mask) fe *= a.mask[idx];
                acc += fe;
                a.dR[idx] = acc;
                if (a.pdR) {
                    const float y = view_y(a.in, &vs, mi.c, idx);
                    prs += (double)acc; prq += (double)acc * (double)y;
                }
            }
        }
    }
    STAMP(3, 7);
    const size_t slab = (size_t)bx * (size_t)a.slab_stride;
    STAMP(3, 8);
    chan_reduce(d1, 0.0, SH(Cout), mo, res, scr, scr2);
    __syncthreads();
    if (threadIdx.x < SH(Cout)) a.dslope1[slab + threadIdx.x] = (float)res[threadIdx.x * 2];
    // the four per-input-channel sums in one butterfly: {sum dR, sum dR*y, dslope_e2, dslope_e1}
    __shared__ double res4[4 * CT_MAXCH];
    double v4[4] = {prs, prq, de2, de1};
    chan_reduce_n<4>(v4, SH(Cin), mi, res4, scr, scr2);
    __syncthreads();
    STAMP(3, 9);
    if ((int)threadIdx.x < SH(Cin)) {
        const double* r = res4 + threadIdx.x * 4;
        if (a.dR != nullptr && a.pdR) {
            double* pp = a.pdR + ((size_t)bx * SH(Cin) + threadIdx.x) * 2;
            pp[0] = r[0]; pp[1] = r[1];
        }
        if (SH(has_excit)) a.dslope_e2[slab + threadIdx.x] = (float)r[2];
        a.dslope_e1[slab + threadIdx.x] = (float)r[3];
    }
}
#undef SH

template <int KIND, bool BIG = false>
__global__ __launch_bounds__(256) void block_bwd_a_kernel(BlockBwdAArgs ka) {
    extern __shared__ __attribute__((aligned(16))) float dyn[];
    __shared__ BlockBwdAArgs sa;
    const BlockBwdAArgs& a = raae::args_to_lds(&sa);
    block_bwd_a_body<KIND, BIG>(a, blockIdx.x, gridDim.x, dyn);
}
template <int KIND, bool BIG = false>
__global__ __launch_bounds__(256) void block_bwd_a_kernel_m(const BlockBwdAArgs* table) {
    extern __shared__ __attribute__((aligned(16))) float dyn[];
    __shared__ BlockBwdAArgs sa;
    const BlockBwdAArgs& a = raae::args_from_table(&sa, table);
    block_bwd_a_body<KIND, BIG>(a, blockIdx.x, gridDim.x, dyn);
}
