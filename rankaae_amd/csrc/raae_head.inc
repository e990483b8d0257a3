// The decoder's head (reference sc/clustering/model.py:461: BatchNorm1d(C, affine=False) -> Conv1d(C, 1, kernel_size=1)
// -> Softplus / ReLU on [B][C][L]) as two streaming kernels (included inside raae_conv.hip's anonymous namespace).
//
// A 1x1 convolution to ONE channel has no window to stage: out[b][l] = act(bias + sum_c w_c * bn(x)[b][c][l]).  The
// per-layer tiled kernels staged whole samples in LDS for it and, backward, ran twice over the same tensors (data
// gradient, then weight gradient): 17 + 49 + 59 us at 4096 rows for 20 + 41 MB.  Here a thread owns quads of four
// consecutive positions, issues every 16-byte load of its quads first, and the backward kernel produces in ONE pass
//   din[b][c][l] = w_c * go[b][l]                        (gradient w.r.t. the BatchNorm output)
//   dbias = sum go,  dw_c = sum go * y_c                 (one slab per workgroup)
//   din_partials[c] = {w_c * sum go, w_c * sum go * y_c} (what the BatchNorm backward of the consumer needs)
// from go = g * act'(out), y_c = (x_c - mean_c) * rstd_c.  Bytes per sample: forward 4(C + 1)L, backward 4(2C + 2)L.

struct HeadFwdArgs { raae_view_t in; int B, L; const float* w; const float* bias; float* out; int act; int nq; };
struct HeadBwdArgs {
    raae_grad_t go; raae_view_t in; int B, L; const float* w; float* din; double* din_partials; float* dw; float* dbias;
    long slab_stride; int nq;
};

constexpr int kHeadU = 4;          // quads per thread and trip of the forward kernel (all loads of a trip in flight together)

// `bx` / `gx`: the workgroup's index and the number of workgroups among those that run this body (co_kernel)
template <int C>
__device__ __forceinline__ void head_fwd_body(const HeadFwdArgs& a, const int bx, const int gx) {
    __shared__ ViewStats vs;
    view_prologue(a.in, C, &vs, bx == 0);
    float wc[C], mu[C], rs[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { wc[c] = a.w[c]; mu[c] = vs.mean[c]; rs[c] = vs.rstd[c]; }
    const float bias = a.bias[0];
    const int L4 = a.L >> 2;
    const int stride = gx * 256;
    constexpr int U = C <= 4 ? kHeadU : kHeadU / 2;
    for (int q0 = bx * 256 + threadIdx.x; q0 < a.nq; q0 += U * stride) {
        float4 x[U][C];
        size_t oi[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int q = q0 + u * stride;
            ok[u] = q < a.nq;
            const int qq = ok[u] ? q : q0;
            const int b = qq / L4, l = 4 * (qq - b * L4);
            oi[u] = (size_t)b * a.L + l;
            if (ok[u]) {
#pragma unroll
                for (int c = 0; c < C; ++c)
                    x[u][c] = *reinterpret_cast<const float4*>(a.in.raw + ((size_t)b * C + c) * a.L + l);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!ok[u]) continue;
            float acc[4] = {bias, bias, bias, bias};
#pragma unroll
            for (int c = 0; c < C; ++c) {
                acc[0] += wc[c] * ((x[u][c].x - mu[c]) * rs[c]);
                acc[1] += wc[c] * ((x[u][c].y - mu[c]) * rs[c]);
                acc[2] += wc[c] * ((x[u][c].z - mu[c]) * rs[c]);
                acc[3] += wc[c] * ((x[u][c].w - mu[c]) * rs[c]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (a.act == RAAE_OUT_SOFTPLUS) acc[i] = raae::softplus2(acc[i]);
                else if (a.act == RAAE_OUT_RELU) acc[i] = fmaxf(acc[i], 0.f);
            }
            *reinterpret_cast<float4*>(a.out + oi[u]) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        }
    }
}

template <int C>
__global__ __launch_bounds__(256) void head_fwd_kernel(HeadFwdArgs a) { head_fwd_body<C>(a, blockIdx.x, gridDim.x); }
template <int C>
__global__ __launch_bounds__(256) void head_fwd_kernel_m(const HeadFwdArgs* t) {      // one trial per grid plane
    const HeadFwdArgs a = t[blockIdx.z];
    head_fwd_body<C>(a, blockIdx.x, gridDim.x);
}

template <int C>
__device__ __forceinline__ void head_bwd_body(const HeadBwdArgs& a) {
    __shared__ ViewStats vs;
    __shared__ double red[4][C + 1];
    {
        const raae::StatJob jobs[1] = {view_job(a.in, C, &vs, false)};
        raae::stat_jobs<1, CV_MAXC>(jobs, false);
    }
    float wc[C], mu[C], rs[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { wc[c] = a.w[c]; mu[c] = vs.mean[c]; rs[c] = vs.rstd[c]; }
    const int L4 = a.L >> 2;
    const int stride = gridDim.x * 256;
    constexpr int U = 2;
    double s[C + 1];
#pragma unroll
    for (int c = 0; c <= C; ++c) s[c] = 0.0;
    for (int q0 = blockIdx.x * 256 + threadIdx.x; q0 < a.nq; q0 += U * stride) {
        float4 g[U], o[U], x[U][C];
        size_t gi[U], xi[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int q = q0 + u * stride;
            ok[u] = q < a.nq;
            const int qq = ok[u] ? q : q0;
            const int b = qq / L4, l = 4 * (qq - b * L4);
            gi[u] = (size_t)b * a.L + l;
            xi[u] = (size_t)b * C * a.L + l;
            if (ok[u]) {
                g[u] = *reinterpret_cast<const float4*>(a.go.g + gi[u]);
                if (a.go.act != RAAE_OUT_RAW) o[u] = *reinterpret_cast<const float4*>(a.go.raw + gi[u]);
#pragma unroll
                for (int c = 0; c < C; ++c) x[u][c] = *reinterpret_cast<const float4*>(a.in.raw + xi[u] + (size_t)c * a.L);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!ok[u]) continue;
            float go4[4] = {g[u].x, g[u].y, g[u].z, g[u].w};
            const float o4[4] = {o[u].x, o[u].y, o[u].z, o[u].w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (a.go.act == RAAE_OUT_SOFTPLUS) go4[i] = go4[i] * (1.f - expf(-2.f * o4[i]));
                else if (a.go.act == RAAE_OUT_RELU) go4[i] = o4[i] > 0.f ? go4[i] : 0.f;
            }
            s[C] += (double)((go4[0] + go4[1]) + (go4[2] + go4[3]));
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float y0 = (x[u][c].x - mu[c]) * rs[c], y1 = (x[u][c].y - mu[c]) * rs[c];
                const float y2 = (x[u][c].z - mu[c]) * rs[c], y3 = (x[u][c].w - mu[c]) * rs[c];
                s[c] += (double)(go4[0] * y0 + go4[1] * y1) + (double)(go4[2] * y2 + go4[3] * y3);
                *reinterpret_cast<float4*>(a.din + xi[u] + (size_t)c * a.L) =
                    make_float4(wc[c] * go4[0], wc[c] * go4[1], wc[c] * go4[2], wc[c] * go4[3]);
            }
        }
    }
    // fixed-order join: xor tree inside each wave, then the four waves in order
#pragma unroll
    for (int c = 0; c <= C; ++c) {
        double v = s[c];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][c] = v;
    }
    __syncthreads();
    if (threadIdx.x <= C) {
        const int c = threadIdx.x;
        const double tot = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
        red[0][c] = tot;
    }
    __syncthreads();
    const size_t slab = (size_t)blockIdx.x * (size_t)a.slab_stride;
    if (threadIdx.x < C) {
        const int c = threadIdx.x;
        a.dw[slab + c] = (float)red[0][c];
        double* p = a.din_partials + ((size_t)blockIdx.x * C + c) * 2;
        p[0] = (double)wc[c] * red[0][C];
        p[1] = (double)wc[c] * red[0][c];
    } else if (threadIdx.x == C) {
        a.dbias[slab] = (float)red[0][C];
    }
}
template <int C>
__global__ __launch_bounds__(256) void head_bwd_kernel(HeadBwdArgs a) { head_bwd_body<C>(a); }
template <int C>
__global__ __launch_bounds__(256) void head_bwd_kernel_m(const HeadBwdArgs* t) {
    const HeadBwdArgs a = t[blockIdx.z];
    head_bwd_body<C>(a);
}

// the head shape these kernels take: Conv1d(C, 1, kernel_size=1) over a plain BatchNorm view, rows of whole quads
static bool head_shape_ok(const raae_conv_t* cv, const raae_view_t* in) {
    return cv->K == 1 && cv->stride == 1 && cv->pad == 0 && cv->groups == 1 && !cv->transposed && cv->Cout == 1 &&
           (cv->Cin == 4 || cv->Cin == 8) && cv->Lin == cv->Lout && (cv->Lin & 3) == 0 && in->has_bn && !in->slope &&
           !in->mask && (reinterpret_cast<uintptr_t>(in->raw) & 15) == 0;
}
// workgroups: one quad per thread while that leaves CUs idle, then up to `unroll` quads per thread and trip; at most
// 256 workgroups (= partial rows / slabs the consumers have to add up)
static int head_grid(int nq, int unroll) {
    int per_trip = nq / (256 * 256);
    if (per_trip < 1) per_trip = 1;
    if (per_trip > unroll) per_trip = unroll;
    int g = (nq + 256 * per_trip - 1) / (256 * per_trip);
    if (g > 256) g = 256;
    return g < 1 ? 1 : g;
}
