// Fused multi-tensor Adam/AdamW, RAdam and AdaBound over the flat parameter arena, the per-step tick,
// the Philox random tape, and HIP stream/graph/event plumbing.
#include "raae_common.h"
#include "raae_philox.h"
#include <string.h>
#include <stdlib.h>

namespace {

#include "raae_adam_body.inc"


template <bool CHK, bool SC = false>
__device__ __forceinline__ void adam_body(float* p, float* m, float* v, const float* g_slabs, long slab_stride,
                                          const unsigned short* seg_nslab, long n, const double* hyper,
                                          const int* step, int decoupled, int* nan_step, const float* gscale = nullptr) {
    __shared__ float s_sc[8];
    if (threadIdx.x == 0) {
        const double lr = hyper[0], b1 = hyper[1], b2 = hyper[2], eps = hyper[3], wd = hyper[4];
        const double t = (double)step[0];
        const double bc1 = 1.0 - pow(b1, t), bc2 = 1.0 - pow(b2, t);
        s_sc[0] = (float)(1.0 - lr * wd);      // AdamW decay factor
        s_sc[1] = (float)(1.0 - b1);           // lerp weight
        s_sc[2] = (float)b2;
        s_sc[3] = (float)(1.0 - b2);
        s_sc[4] = (float)(-(lr / bc1));        // -step_size
        s_sc[5] = (float)sqrt(bc2);
        s_sc[6] = (float)eps;
        s_sc[7] = (float)wd;
    }
    __syncthreads();
    const float decay = s_sc[0], w1 = s_sc[1], b2f = s_sc[2], omb2 = s_sc[3], nstep = s_sc[4], bc2s = s_sc[5],
                epsf = s_sc[6], wdf = s_sc[7];
    bool seen = false;
    float gs = 1.f;
    if (SC) gs = gscale[0];                 // the clip scale raae_grad_norm left (scale_grad: raae_adam_body.inc)
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int ns = seg_nslab[i >> 6];
        if (ns == 0) continue;
        // fixed-order slab sum, 8 independent loads in flight at a time
        float g = 0.f;
        int s = 0;
        for (; s + 8 <= ns; s += 8) {
            float t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) t[u] = g_slabs[(size_t)(s + u) * slab_stride + i];
#pragma unroll
            for (int u = 0; u < 8; ++u) g += t[u];
        }
        for (; s < ns; ++s) g += g_slabs[(size_t)s * slab_stride + i];
        if (CHK) seen |= __builtin_isnan(g);
        if (SC) g = scale_grad(g, gs);
        float pv = p[i];
        if (decoupled) pv = pv * decay; else if (wdf != 0.f) g = g + wdf * pv;
        float mv = m[i], vv = v[i];
        mv = mv + w1 * (g - mv);
        vv = vv * b2f;
        vv = vv + (omb2 * g) * g;
        const float denom = sqrtf(vv) / bc2s + epsf;
        pv = pv + (nstep * mv) / denom;
        p[i] = pv; m[i] = mv; v[i] = vv;
    }
    if (CHK) nan_vote(seen, nan_step, step);
}

__global__ __launch_bounds__(256) void adam_kernel(AdamArgs a) {
    adam_body<false>(a.p, a.m, a.v, a.g_slabs, a.slab_stride, a.seg_nslab, a.n, a.hyper, a.step, a.decoupled, nullptr);
}
__global__ __launch_bounds__(256) void adam_kernel_m(const AdamArgs* t) {
    const AdamArgs a = t[blockIdx.z];
    adam_body<false>(a.p, a.m, a.v, a.g_slabs, a.slab_stride, a.seg_nslab, a.n, a.hyper, a.step, a.decoupled, nullptr);
}
// checked twins (AdamChkArgs: the argument block of the unchecked kernel + the flag word)
__global__ __launch_bounds__(256) void adam_chk_kernel(AdamChkArgs c) {
    const AdamArgs& a = c.a;
    adam_body<true>(a.p, a.m, a.v, a.g_slabs, a.slab_stride, a.seg_nslab, a.n, a.hyper, a.step, a.decoupled, c.nan_step);
}
__global__ __launch_bounds__(256) void adam_chk_kernel_m(const AdamChkArgs* t) {
    const AdamChkArgs c = t[blockIdx.z];
    const AdamArgs& a = c.a;
    adam_body<true>(a.p, a.m, a.v, a.g_slabs, a.slab_stride, a.seg_nslab, a.n, a.hyper, a.step, a.decoupled, c.nan_step);
}

// (adam_wide_body, the same update with the slabs of an element spread over 8 lanes: raae_adam_body.inc)
__global__ __launch_bounds__(256) void adam_wide_kernel(AdamArgs a) {
    adam_wide_body<false>(a.p, a.m, a.v, a.g_slabs, a.slab_stride, a.seg_nslab, a.n, a.hyper, a.step, a.decoupled, nullptr, blockIdx.x, gridDim.x);
}
__global__ __launch_bounds__(256) void adam_wide_kernel_m(const AdamArgs* t) {
    const AdamArgs a = t[blockIdx.z];
    adam_wide_body<false>(a.p, a.m, a.v, a.g_slabs, a.slab_stride, a.seg_nslab, a.n, a.hyper, a.step, a.decoupled, nullptr, blockIdx.x, gridDim.x);
}
__global__ __launch_bounds__(256) void adam_wide_chk_kernel(AdamChkArgs c) {
    const AdamArgs& a = c.a;
    adam_wide_body<true>(a.p, a.m, a.v, a.g_slabs, a.slab_stride, a.seg_nslab, a.n, a.hyper, a.step, a.decoupled,
                         c.nan_step, blockIdx.x, gridDim.x);
}
__global__ __launch_bounds__(256) void adam_wide_chk_kernel_m(const AdamChkArgs* t) {
    const AdamChkArgs c = t[blockIdx.z];
    const AdamArgs& a = c.a;
    adam_wide_body<true>(a.p, a.m, a.v, a.g_slabs, a.slab_stride, a.seg_nslab, a.n, a.hyper, a.step, a.decoupled,
                         c.nan_step, blockIdx.x, gridDim.x);
}

// clipped instances (raae_optim_step_clip with a scale): the bodies above with SC = true, checked or not, narrow or wide
template <bool CHK, bool WIDE>
__device__ __forceinline__ void adam_clip_run(const AdamChkArgs& c) {
    const AdamArgs& a = c.a;
    if (WIDE) adam_wide_body<CHK, true>(a.p, a.m, a.v, a.g_slabs, a.slab_stride, a.seg_nslab, a.n, a.hyper, a.step, a.decoupled,
                                        c.nan_step, blockIdx.x, gridDim.x, a.gscale);
    else adam_body<CHK, true>(a.p, a.m, a.v, a.g_slabs, a.slab_stride, a.seg_nslab, a.n, a.hyper, a.step, a.decoupled,
                              c.nan_step, a.gscale);
}
template <bool CHK, bool WIDE> __global__ __launch_bounds__(256) void adam_clip_kernel(AdamChkArgs c) { adam_clip_run<CHK, WIDE>(c); }
template <bool CHK, bool WIDE> __global__ __launch_bounds__(256) void adam_clip_kernel_m(const AdamChkArgs* t) {
    const AdamChkArgs c = t[blockIdx.z];
    adam_clip_run<CHK, WIDE>(c);
}

// ---- RAdam and AdaBound (torch_optimizer 0.1.0, the optimizer_name values the reference takes from that package) ----
// One kernel instance per rule: OptRule<R>::scalars forms the per-step scalars in double (Python floats) from the
// device hyper block and step count, in the operation order of the Python source (no contraction into fma there);
// OptRule<R>::update is the per-element fp32 update in the order of the torch ops.  Gradient reading as in Adam.
constexpr int OPT_NSC = 10;
struct OptimArgs { float* p; float* m; float* v; const float* g_slabs; long slab_stride; const unsigned short* seg_nslab;
                   long n; const double* hyper; const int* step;
                   const float* gscale; };  // NULL, or the clip scale (AdamArgs::gscale)
template <int RULE> struct OptRule;

// torch_optimizer.RAdam.step.  The class caches (t, N, step size) in a 10-entry buffer keyed on t % 10, filled by the
// first tensor stepped at a given t; every tensor of one optimizer here shares one step count, so the cache always
// holds what the formula gives at the current lr, and the formula is evaluated directly.  N is formed in double in
// this order: at t = 5 it misses 5 by only 4e-3 (beta2 = 0.999) or 4e-4 (0.9999); t = 6 is the first rectified step.
template <> struct OptRule<RAAE_OPT_RADAM> {
    __device__ static void scalars(const double* h, int step, float* s) {
#pragma clang fp contract(off)
        const double lr = h[0], b1 = h[1], b2 = h[2], eps = h[3], wd = h[4];
        const double t = (double)step;
        const double b2t = pow(b2, t);
        const double nmax = 2.0 / (1.0 - b2) - 1.0;
        const double nsma = nmax - 2.0 * t * b2t / (1.0 - b2t);
        const bool rect = nsma >= 5.0;
        const double ss = rect ? lr * sqrt((1.0 - b2t) * (nsma - 4.0) / (nmax - 4.0) * (nsma - 2.0) / nsma * nmax /
                                           (nmax - 2.0)) / (1.0 - pow(b1, t))
                               : lr / (1.0 - pow(b1, t));
        s[0] = (float)b1;
        s[1] = (float)(1.0 - b1);
        s[2] = (float)b2;
        s[3] = (float)(1.0 - b2);
        s[4] = (float)(-ss);
        s[5] = (float)eps;
        s[6] = (float)(-wd * lr);           // decoupled decay: p.add_(p, alpha=-wd*lr)
        s[7] = wd != 0.0 ? 1.f : 0.f;
        s[8] = rect ? 1.f : 0.f;
        s[9] = 0.f;
    }
    __device__ static void update(const float (&s)[OPT_NSC], float& p, float& m, float& v, float g) {
        v = v * s[2];
        v = v + (s[3] * g) * g;             // exp_avg_sq.mul_(b2).addcmul_(g, g, value=1-b2), before exp_avg
        m = m * s[0];
        m = m + s[1] * g;                   // exp_avg.mul_(b1).add_(g, alpha=1-b1)
        if (s[7] != 0.f) p = p + s[6] * p;
        if (s[8] != 0.f) p = p + (s[4] * m) / (sqrtf(v) + s[5]);   // addcdiv_(exp_avg, sqrt(v) + eps, value=-ss)
        else p = p + s[4] * m;                                     // the first steps: SGD with momentum
    }
};

// torch_optimizer.AdaBound.step (amsbound = False).  hyper[5] = base_lr (the lr at construction, self.base_lrs; a
// ReduceLROnPlateau cut of hyper[0] moves the bounds through final_lr * lr / base_lr).
template <> struct OptRule<RAAE_OPT_ADABOUND> {
    __device__ static void scalars(const double* h, int step, float* s) {
#pragma clang fp contract(off)
        const double lr = h[0], b1 = h[1], b2 = h[2], eps = h[3], wd = h[4], base_lr = h[5], final_lr = h[6],
                     gamma = h[7];
        const double t = (double)step;
        const double bc1 = 1.0 - pow(b1, t), bc2 = 1.0 - pow(b2, t);
        const double ss = lr * sqrt(bc2) / bc1;
        const double flr = final_lr * lr / base_lr;
        s[0] = (float)b1;
        s[1] = (float)(1.0 - b1);
        s[2] = (float)b2;
        s[3] = (float)(1.0 - b2);
        s[4] = (float)ss;                                       // torch.full_like(denom, step_size)
        s[5] = (float)(flr * (1.0 - 1.0 / (gamma * t + 1.0)));  // clamp_ bounds, as fp32 scalars
        s[6] = (float)(flr * (1.0 + 1.0 / (gamma * t)));
        s[7] = (float)eps;
        s[8] = (float)wd;
        s[9] = wd != 0.0 ? 1.f : 0.f;
    }
    __device__ static void update(const float (&s)[OPT_NSC], float& p, float& m, float& v, float g) {
        if (s[9] != 0.f) g = g + s[8] * p;                 // grad.add(p, alpha=wd): coupled L2
        m = m * s[0];
        m = m + s[1] * g;
        v = v * s[2];
        v = v + (s[3] * g) * g;
        float x = s[4] / (sqrtf(v) + s[7]);                // step_size.div_(denom).clamp_(lo, hi).mul_(exp_avg)
        x = x < s[5] ? s[5] : (x > s[6] ? s[6] : x);       // (NaN passes through, as in torch.clamp)
        x = x * m;
        p = p + (-x);
    }
};

template <int RULE>
__device__ __forceinline__ void optim_scalars(const OptimArgs& a, float (&sc)[OPT_NSC]) {
    __shared__ float s_sc[OPT_NSC];
    if (threadIdx.x == 0) OptRule<RULE>::scalars(a.hyper, a.step[0], s_sc);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < OPT_NSC; ++k) sc[k] = s_sc[k];
}

template <int RULE, bool CHK, bool SC = false>
__device__ __forceinline__ void optim_body(const OptimArgs& a, int* nan_step) {
    float sc[OPT_NSC];
    optim_scalars<RULE>(a, sc);
    bool seen = false;
    float gs = 1.f;
    if (SC) gs = a.gscale[0];
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (long)gridDim.x * 256) {
        const int ns = a.seg_nslab[i >> 6];
        if (ns == 0) continue;
        float g = 0.f;                                  // adam_body's fixed-order slab sum
        int s = 0;
        for (; s + 8 <= ns; s += 8) {
            float t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) t[u] = a.g_slabs[(size_t)(s + u) * a.slab_stride + i];
#pragma unroll
            for (int u = 0; u < 8; ++u) g += t[u];
        }
        for (; s < ns; ++s) g += a.g_slabs[(size_t)s * a.slab_stride + i];
        if (CHK) seen |= __builtin_isnan(g);
        if (SC) g = scale_grad(g, gs);
        float pv = a.p[i], mv = a.m[i], vv = a.v[i];
        OptRule<RULE>::update(sc, pv, mv, vv, g);
        a.p[i] = pv; a.m[i] = mv; a.v[i] = vv;
    }
    if (CHK) nan_vote(seen, nan_step, a.step);
}

template <int RULE, bool CHK, bool SC = false>
__device__ __forceinline__ void optim_wide_body(const OptimArgs& a, int* nan_step) {
    float sc[OPT_NSC];
    optim_scalars<RULE>(a, sc);
    float gs = 1.f;
    if (SC) gs = a.gscale[0];
    const int lane = threadIdx.x & 63, el = lane & 7, ch = lane >> 3;   // adam_wide_body's lane split and shuffle tree
    const long wave0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 8;
    bool seen = false;
    for (long base = wave0; base < a.n; base += (long)gridDim.x * 32) {
        const long i = base + el;                       // n is a multiple of 64: i < n whenever base < n
        const int ns = a.seg_nslab[i >> 6];
        if (ns == 0) continue;                          // uniform over the wave (8 elements share a segment)
        float g = 0.f;
        for (int s = ch; s < ns; s += 64) {
            float t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int r = s + 8 * u;
                t[u] = a.g_slabs[(size_t)(r < ns ? r : ch) * a.slab_stride + i];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) g += (s + 8 * u < ns) ? t[u] : 0.f;
        }
        g += __shfl_xor(g, 8, 64);
        g += __shfl_xor(g, 16, 64);
        g += __shfl_xor(g, 32, 64);
        if (ch != 0) continue;
        if (CHK) seen |= __builtin_isnan(g);
        if (SC) g = scale_grad(g, gs);
        float pv = a.p[i], mv = a.m[i], vv = a.v[i];
        OptRule<RULE>::update(sc, pv, mv, vv, g);
        a.p[i] = pv; a.m[i] = mv; a.v[i] = vv;
    }
    if (CHK) nan_vote(seen, nan_step, a.step);
}

template <int RULE> __global__ __launch_bounds__(256) void optim_kernel(OptimArgs a) { optim_body<RULE, false>(a, nullptr); }
template <int RULE> __global__ __launch_bounds__(256) void optim_kernel_m(const OptimArgs* t) {
    const OptimArgs a = t[blockIdx.z];
    optim_body<RULE, false>(a, nullptr);
}
template <int RULE> __global__ __launch_bounds__(256) void optim_wide_kernel(OptimArgs a) { optim_wide_body<RULE, false>(a, nullptr); }
template <int RULE> __global__ __launch_bounds__(256) void optim_wide_kernel_m(const OptimArgs* t) {
    const OptimArgs a = t[blockIdx.z];
    optim_wide_body<RULE, false>(a, nullptr);
}
// checked twins (raae_optim_step_chk)
struct OptimChkArgs { OptimArgs a; int* nan_step; };
template <int RULE> __global__ __launch_bounds__(256) void optim_chk_kernel(OptimChkArgs c) {
    optim_body<RULE, true>(c.a, c.nan_step);
}
template <int RULE> __global__ __launch_bounds__(256) void optim_chk_kernel_m(const OptimChkArgs* t) {
    const OptimChkArgs c = t[blockIdx.z];
    optim_body<RULE, true>(c.a, c.nan_step);
}
template <int RULE> __global__ __launch_bounds__(256) void optim_wide_chk_kernel(OptimChkArgs c) {
    optim_wide_body<RULE, true>(c.a, c.nan_step);
}
template <int RULE> __global__ __launch_bounds__(256) void optim_wide_chk_kernel_m(const OptimChkArgs* t) {
    const OptimChkArgs c = t[blockIdx.z];
    optim_wide_body<RULE, true>(c.a, c.nan_step);
}

// clipped instances (raae_optim_step_clip with a scale)
template <int RULE, bool CHK, bool WIDE> __global__ __launch_bounds__(256) void optim_clip_kernel(OptimChkArgs c) {
    if (WIDE) optim_wide_body<RULE, CHK, true>(c.a, c.nan_step); else optim_body<RULE, CHK, true>(c.a, c.nan_step);
}
template <int RULE, bool CHK, bool WIDE> __global__ __launch_bounds__(256) void optim_clip_kernel_m(const OptimChkArgs* t) {
    const OptimChkArgs c = t[blockIdx.z];
    if (WIDE) optim_wide_body<RULE, CHK, true>(c.a, c.nan_step); else optim_body<RULE, CHK, true>(c.a, c.nan_step);
}

// the grid of every update kernel: above 16 slabs 32 elements per workgroup (8 lanes per element), else one per thread
inline dim3 optim_grid(long n, int max_nslab) {
    long g = max_nslab > 16 ? (n + 31) / 32 : (n + 255) / 256;
    if (g > 4096) g = 4096;
    return dim3((int)g);
}

template <int RULE>
void launch_optim(const OptimArgs& a, int max_nslab, hipStream_t stream) {
    if (max_nslab > 16) {
        long g = (a.n + 31) / 32;               // raae_adam_step's geometry
        if (g > 4096) g = 4096;
        raae::launch(optim_wide_kernel<RULE>, optim_wide_kernel_m<RULE>, dim3((int)g), dim3(256), 0, stream, a);
    } else {
        long g = (a.n + 255) / 256;
        if (g > 4096) g = 4096;
        raae::launch(optim_kernel<RULE>, optim_kernel_m<RULE>, dim3((int)g), dim3(256), 0, stream, a);
    }
}

template <int RULE>
void launch_optim_chk(const OptimChkArgs& c, int max_nslab, hipStream_t stream) {
    if (max_nslab > 16)
        raae::launch(optim_wide_chk_kernel<RULE>, optim_wide_chk_kernel_m<RULE>, optim_grid(c.a.n, max_nslab), dim3(256), 0,
                     stream, c);
    else
        raae::launch(optim_chk_kernel<RULE>, optim_chk_kernel_m<RULE>, optim_grid(c.a.n, max_nslab), dim3(256), 0, stream, c);
}

template <int RULE>
void launch_optim_clip(const OptimChkArgs& c, int max_nslab, hipStream_t stream) {
    const dim3 grid = optim_grid(c.a.n, max_nslab), block(256);
    if (max_nslab > 16) {
        if (c.nan_step) raae::launch(optim_clip_kernel<RULE, true, true>, optim_clip_kernel_m<RULE, true, true>, grid, block, 0, stream, c);
        else raae::launch(optim_clip_kernel<RULE, false, true>, optim_clip_kernel_m<RULE, false, true>, grid, block, 0, stream, c);
    } else {
        if (c.nan_step) raae::launch(optim_clip_kernel<RULE, true, false>, optim_clip_kernel_m<RULE, true, false>, grid, block, 0, stream, c);
        else raae::launch(optim_clip_kernel<RULE, false, false>, optim_clip_kernel_m<RULE, false, false>, grid, block, 0, stream, c);
    }
}

// ---- gradient-norm clipping (config key `grad_clip_norm`): the L2 norm of an optimizer's slab-summed gradient ----
// Every lane sums the slabs of its elements in fp32 in the update kernels' order (one thread per element, or 8 lanes
// per element and their shuffle tree above 16 slabs) and accumulates the squares in double; the lanes meet in the
// xor-shuffle tree of a wave, the waves in LDS in wave order, and thread 0 stores the workgroup's partial.  The last
// workgroup to arrive (ticket, as the loss kernels' loss_fin_last_block) adds the partials -- thread t takes partials t,
// t + 256, ..., then the same tree -- and writes out = {norm, scale}, scale = min(1, max_norm / (norm + 1e-6)) (what
// torch.nn.utils.clip_grad_norm_ multiplies by; NaN for a NaN norm, as there), counts the step in *clipped when
// scale < 1 and resets the ticket for the next launch (graph replay).  No float atomics: the arrival order decides only
// WHO adds the partials, never the order in which they are added.
constexpr int GRAD_NORM_PARTS = RAAE_GRAD_NORM_PARTS;
struct GradNormArgs { const float* g_slabs; long slab_stride; const unsigned short* seg_nslab; long n; double max_norm;
                      double* partial; unsigned* ticket; float* out; int* clipped; };
template <bool WIDE>
__device__ __forceinline__ void grad_norm_body(const GradNormArgs& a) {
    __shared__ double s_red[16];
    __shared__ unsigned s_last;
    double acc = 0.0;
    if (!WIDE) {
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (long)gridDim.x * 256) {
            const int ns = a.seg_nslab[i >> 6];
            if (ns == 0) continue;
            float g = 0.f;                                  // adam_body's fixed-order slab sum
            int s = 0;
            for (; s + 8 <= ns; s += 8) {
                float t[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) t[u] = a.g_slabs[(size_t)(s + u) * a.slab_stride + i];
#pragma unroll
                for (int u = 0; u < 8; ++u) g += t[u];
            }
            for (; s < ns; ++s) g += a.g_slabs[(size_t)s * a.slab_stride + i];
            acc += (double)g * (double)g;
        }
    } else {
        const int lane = threadIdx.x & 63, el = lane & 7, ch = lane >> 3;   // adam_wide_body's lane split and shuffle tree
        const long wave0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 8;
        for (long base = wave0; base < a.n; base += (long)gridDim.x * 32) {
            const long i = base + el;                       // n is a multiple of 64: i < n whenever base < n
            const int ns = a.seg_nslab[i >> 6];
            if (ns == 0) continue;                          // uniform over the wave (8 elements share a segment)
            float g = 0.f;
            for (int s = ch; s < ns; s += 64) {
                float t[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int r = s + 8 * u;
                    t[u] = a.g_slabs[(size_t)(r < ns ? r : ch) * a.slab_stride + i];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) g += (s + 8 * u < ns) ? t[u] : 0.f;
            }
            g += __shfl_xor(g, 8, 64);
            g += __shfl_xor(g, 16, 64);
            g += __shfl_xor(g, 32, 64);
            if (ch == 0) acc += (double)g * (double)g;
        }
    }
    const double part = raae::block_sum(acc, s_red);
    if (threadIdx.x == 0) {
        a.partial[blockIdx.x] = part;
        __threadfence();
        s_last = atomicAdd(a.ticket, 1u) == gridDim.x - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!s_last) return;                     // uniform per workgroup
    __threadfence();
    double t = 0.0;
    for (unsigned i = threadIdx.x; i < gridDim.x; i += 256) t += ((volatile double*)a.partial)[i];
    t = raae::block_sum(t, s_red);
    if (threadIdx.x == 0) {
        const double norm = sqrt(t);
        const double r = a.max_norm / (norm + 1e-6);
        const float scale = (float)(r < 1.0 ? r : (r != r ? r : 1.0));
        a.out[0] = (float)norm;
        a.out[1] = scale;
        if (scale < 1.f) a.clipped[0] += 1;
        *a.ticket = 0u;
    }
}
__global__ __launch_bounds__(256) void grad_norm_kernel(GradNormArgs a) { grad_norm_body<false>(a); }
__global__ __launch_bounds__(256) void grad_norm_kernel_m(const GradNormArgs* t) {
    const GradNormArgs a = t[blockIdx.z];
    grad_norm_body<false>(a);
}
__global__ __launch_bounds__(256) void grad_norm_wide_kernel(GradNormArgs a) { grad_norm_body<true>(a); }
__global__ __launch_bounds__(256) void grad_norm_wide_kernel_m(const GradNormArgs* t) {
    const GradNormArgs a = t[blockIdx.z];
    grad_norm_body<true>(a);
}

// ---- moving average of the weights (config key `ema_decay`): ema[i] = fmaf(d, ema[i], omd * p[i]) ----
// One element-wise pass, plain fp32: the product omd * p[i] is rounded once and feeds the fused multiply-add (an fma
// argument cannot be contracted further), so the vector body, the scalar body and the tail give the same bits.  No
// atomics, no reduction: a replay is bitwise the eager call.  With both pointers 16-byte aligned a thread takes four
// elements per load (float4) and threads 0 .. n % 4 - 1 of workgroup 0 take the tail; otherwise one element per load.
// The choice is made HERE, from the pointers of the plane's own argument row, so every trial of a batch launches the
// same kernel instance with the same grid (raae_multi_build compares both).
struct EmaArgs { float* ema; const float* p; long n; float d; float omd; };
__device__ __forceinline__ void ema_body(const EmaArgs& a) {
    const long nthreads = (long)gridDim.x * 256, t0 = (long)blockIdx.x * 256 + threadIdx.x;
    const float d = a.d, omd = a.omd;
    if ((((uintptr_t)a.ema | (uintptr_t)a.p) & 15) == 0) {
        const long nq = a.n >> 2;
        float4* e4 = reinterpret_cast<float4*>(a.ema);
        const float4* p4 = reinterpret_cast<const float4*>(a.p);
        for (long q = t0; q < nq; q += nthreads) {
            float4 e = e4[q];
            const float4 w = p4[q];
            e.x = fmaf(d, e.x, omd * w.x); e.y = fmaf(d, e.y, omd * w.y);
            e.z = fmaf(d, e.z, omd * w.z); e.w = fmaf(d, e.w, omd * w.w);
            e4[q] = e;
        }
        const long i = (nq << 2) + t0;          // the tail: t0 < n % 4 <= 3, i.e. workgroup 0's first threads
        if (i < a.n) a.ema[i] = fmaf(d, a.ema[i], omd * a.p[i]);
    } else {
        for (long i = t0; i < a.n; i += nthreads) a.ema[i] = fmaf(d, a.ema[i], omd * a.p[i]);
    }
}
__global__ __launch_bounds__(256) void ema_kernel(EmaArgs a) { ema_body(a); }
__global__ __launch_bounds__(256) void ema_kernel_m(const EmaArgs* t) {
    const EmaArgs a = t[blockIdx.z];
    ema_body(a);
}

__global__ void tick_kernel(int* steps, int n, unsigned mask, unsigned long long* rng_counter, int* cursor,
                            int cursor_inc) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (int i = 0; i < n; ++i) if (mask & (1u << i)) steps[i] += 1;
        if (rng_counter) {
            rng_counter[0] += 1ull;
            raae::mask_keys_store(rng_counter, rng_counter[1], rng_counter[0]);       // {counter, seed, keys}
        }
        if (cursor) cursor[0] += cursor_inc;
    }
}

// floats [4 q, 4 q + 4) of the tape (segments start at multiples of 4 floats)
__device__ __forceinline__ void fill_quad(float* tape, const int* seg_desc, const float* seg_scale, int nseg, long total,
                                          unsigned long long seed, unsigned long long ctr, long q) {
    const long e0 = q * 4;
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {                       // last segment whose offset <= e0
        const int mid = (lo + hi + 1) >> 1;
        if ((long)seg_desc[mid * 4] <= e0) lo = mid; else hi = mid - 1;
    }
    const int kind = seg_desc[lo * 4 + 2];
    const long send = (long)seg_desc[lo * 4] + seg_desc[lo * 4 + 1];
    float o[4];
    if (kind == 0) {
        // Philox counter = (position of these four floats in the numbering of the step's Gaussian elements) / 4
        raae::normal4(((long)seg_desc[lo * 4 + 3] + (e0 - seg_desc[lo * 4])) >> 2, ctr, seed, o);
    } else if (kind == 1) {
        // dropout multipliers {0, 1/keep}: the counter-based hash of raae_common.h -- the function a kernel with a
        // raae_maskgen_t evaluates for a slot it generates itself (hash index = the slot's position in the numbering
        // of ALL dropout elements of the step, seg_desc[.][3], + the element's index in the slot: the same whether the
        // slot lives on the tape or in its consumer)
        const raae::MaskGen g = raae::mask_gen_make(seed, ctr, (uint32_t)seg_desc[lo * 4 + 3], seg_scale[lo]);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = raae::mask_val(g, (uint32_t)(e0 + j - seg_desc[lo * 4]));
    } else {
        // kind 2 (`precision: bf16`): keep flags {0, 1} stored as bf16 -- these four floats hold eight of them (bf16
        // element i of the slot is hashed at index i of the slot); the dense kernels multiply by the fp32 1/keep
        const raae::MaskGen g = raae::mask_gen_make(seed, ctr, (uint32_t)seg_desc[lo * 4 + 3], seg_scale[lo]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t e = 2u * (uint32_t)(e0 + j - seg_desc[lo * 4]);
            const uint32_t lo16 = raae::mask_keep(g, e) ? 0x3F80u : 0u, hi16 = raae::mask_keep(g, e + 1u) ? 0x3F80u : 0u;
            o[j] = __uint_as_float(lo16 | (hi16 << 16));
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) if (e0 + j < send && e0 + j < total) tape[e0 + j] = o[j];
}

struct RngFillArgs { float* tape; const int* seg_desc; const float* seg_scale; int nseg; long total; unsigned long long seed;
                     const unsigned long long* counter; };
__device__ __forceinline__ void rng_fill_body(const RngFillArgs& a) {
    const unsigned long long ctr = a.counter ? a.counter[0] : 0ull;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q * 4 < a.total; q += (long)gridDim.x * 256)
        fill_quad(a.tape, a.seg_desc, a.seg_scale, a.nseg, a.total, a.seed, ctr, q);
}
__global__ __launch_bounds__(256) void rng_fill_kernel(RngFillArgs a) { rng_fill_body(a); }
__global__ __launch_bounds__(256) void rng_fill_kernel_m(const RngFillArgs* t) {       // one trial per grid plane
    const RngFillArgs a = t[blockIdx.z];
    rng_fill_body(a);
}

// ---- the head of a training step in ONE launch (was: tick, tape fill, batch gather -- 19 us at 256 rows) ----
// Every workgroup reads the step counter and the row cursor AS THE PREVIOUS STEP LEFT THEM and works with counter + 1
// and cursor + stride; the last workgroup to finish (ticket) stores the advanced values, and the Adam step counts, for
// the kernels that follow.  Work: (a) gather the batch rows perm[cursor - B, cursor) (+ spectral noise: N(0, 1) from
// the Philox block of the element's position in the step's Gaussian numbering, or from the tape in parity mode),
// (b) fill the resident slots of the random tape.
struct StepBeginArgs {
    int* steps; int nsteps; unsigned step_mask; unsigned long long* rng_state; int* cursor; int stride; unsigned* ticket;
    const float* spec; const float* aux; const long* idx; int B; int L; int n_aux; float spec_noise;
    const float* noise_tape;      // parity mode: the noise slot on the (host-filled) tape; NULL: generated here
    long noise_goff;              // position of the noise slot in the Gaussian numbering (multiple of 4)
    float* spec_out; float* aux_out;
    float* tape; const int* seg_desc; const float* seg_scale; int nseg; long total;     // nseg == 0: no fill
};
__device__ __forceinline__ void step_begin_body(const StepBeginArgs& a) {
    // Thread 0 reads the old counters, hands them to the workgroup through LDS and only then takes the workgroup's
    // ticket -- at the START (the value comes back while the workgroup works): whoever draws the last one knows that
    // every workgroup has READ the counters (the LDS stores need the loaded values, and precede the ticket in program
    // order) and publishes the advanced ones at its end.  (Tickets of one address serialise at ~40 ns each: 2048
    // workgroups taking them at their END made this kernel 84 us long; the grid is now 64 ... 1024 workgroups.)
    __shared__ unsigned long long s_ctr, s_seed;
    __shared__ int s_cur;
    unsigned my_ticket = 0u;
    if (threadIdx.x == 0) {
        s_ctr = a.rng_state[0] + 1ull;
        s_seed = a.rng_state[1];
        s_cur = a.cursor[0] + a.stride;
        __threadfence();
        my_ticket = atomicAdd(a.ticket, 1u);
    }
    __syncthreads();
    const unsigned long long ctr = s_ctr, seed = s_seed;
    const int cur = s_cur;
    const long* idx = a.idx + (cur - a.B);
    const long nthreads = (long)gridDim.x * 256, t0 = (long)blockIdx.x * 256 + threadIdx.x;
    const long n = (long)a.B * a.L;
    if ((a.L & 3) == 0) {
        for (long i4 = t0; i4 * 4 < n; i4 += nthreads) {
            const long i = i4 * 4;
            const int b = (int)(i / a.L), l = (int)(i - (long)b * a.L);
            float4 v = *reinterpret_cast<const float4*>(a.spec + (size_t)idx[b] * a.L + l);
            if (a.spec_noise != 0.f) {
                float z[4];
                if (a.noise_tape != nullptr) { const float4 t = *reinterpret_cast<const float4*>(a.noise_tape + i); z[0] = t.x; z[1] = t.y; z[2] = t.z; z[3] = t.w; }
                else raae::normal4((a.noise_goff + i) >> 2, ctr, seed, z);
                v.x += z[0] * a.spec_noise; v.y += z[1] * a.spec_noise; v.z += z[2] * a.spec_noise; v.w += z[3] * a.spec_noise;
            }
            *reinterpret_cast<float4*>(a.spec_out + i) = v;
        }
    } else {
        for (long i = t0; i < n; i += nthreads) {
            const int b = (int)(i / a.L), l = (int)(i - (long)b * a.L);
            float v = a.spec[(size_t)idx[b] * a.L + l];
            if (a.spec_noise != 0.f) {
                if (a.noise_tape != nullptr) v += a.noise_tape[i] * a.spec_noise;
                else { float z[4]; raae::normal4((a.noise_goff + i) >> 2, ctr, seed, z); v += z[(a.noise_goff + i) & 3] * a.spec_noise; }
            }
            a.spec_out[i] = v;
        }
    }
    const long na = (long)a.B * a.n_aux;
    for (long i = t0; i < na; i += nthreads) {
        const int b = (int)(i / a.n_aux), k = (int)(i - (long)b * a.n_aux);
        a.aux_out[i] = a.aux[(size_t)idx[b] * a.n_aux + k];
    }
    if (a.nseg > 0) {
        // the segment table goes to LDS once per workgroup: the binary search of every quad is then six LDS reads, not
        // six dependent global round trips (a thread fills ~16 quads here, not one as in rng_fill_kernel)
        __shared__ int s_desc[4 * 256];
        __shared__ float s_scale[256];
        const int* desc = a.seg_desc;
        const float* scale = a.seg_scale;
        if (a.nseg <= 256) {
            for (int i = threadIdx.x; i < 4 * a.nseg; i += 256) s_desc[i] = a.seg_desc[i];
            for (int i = threadIdx.x; i < a.nseg; i += 256) s_scale[i] = a.seg_scale[i];
            __syncthreads();
            desc = s_desc; scale = s_scale;
        }
        for (long q = t0; q * 4 < a.total; q += nthreads)
            fill_quad(a.tape, desc, scale, a.nseg, a.total, seed, ctr, q);
    }
    // the workgroup that STARTED last publishes the advanced counters (nobody in this launch reads them again)
    if (threadIdx.x == 0 && my_ticket == gridDim.x - 1) {
        for (int i = 0; i < a.nsteps; ++i) if (a.step_mask & (1u << i)) a.steps[i] += 1;
        a.rng_state[0] = ctr;
        raae::mask_keys_store(a.rng_state, seed, ctr);
        a.cursor[0] = cur;
        *a.ticket = 0u;
    }
}
__global__ __launch_bounds__(256) void step_begin_kernel(StepBeginArgs a) { step_begin_body(a); }
__global__ __launch_bounds__(256) void step_begin_kernel_m(const StepBeginArgs* t) {
    const StepBeginArgs a = t[blockIdx.z];
    step_begin_body(a);
}

}  // namespace

extern "C" int raae_adam_step(float* p, float* m, float* v, const float* g_slabs, long slab_stride,
                              const unsigned short* seg_nslab, long n, const double* hyper, const int* step,
                              int decoupled, int max_nslab, void* stream) {
    RAAE_CHECK_ARG(p && m && v && g_slabs && seg_nslab && hyper && step && n > 0 && (n % 64) == 0 && max_nslab >= 0);
    const AdamArgs a = {p, m, v, g_slabs, slab_stride, seg_nslab, n, hyper, step, decoupled};
    if (max_nslab > 16) {
        long g = (n + 31) / 32;                 // 32 elements per workgroup (8 lanes per element)
        if (g > 4096) g = 4096;
        raae::launch(adam_wide_kernel, adam_wide_kernel_m, dim3((int)g), dim3(256), 0, (hipStream_t)stream, a);
    } else {
        long g = (n + 255) / 256;               // one element per thread
        if (g > 4096) g = 4096;
        raae::launch(adam_kernel, adam_kernel_m, dim3((int)g), dim3(256), 0, (hipStream_t)stream, a);
    }
    RAAE_LAUNCH_RET();
}

extern "C" int raae_optim_step(float* p, float* m, float* v, const float* g_slabs, long slab_stride,
                               const unsigned short* seg_nslab, long n, int rule, const double* hyper, const int* step,
                               int max_nslab, void* stream) {
    RAAE_CHECK_ARG(rule >= RAAE_OPT_ADAM && rule <= RAAE_OPT_ADABOUND);
    if (rule == RAAE_OPT_ADAM || rule == RAAE_OPT_ADAMW)
        return raae_adam_step(p, m, v, g_slabs, slab_stride, seg_nslab, n, hyper, step, rule == RAAE_OPT_ADAMW,
                              max_nslab, stream);
    RAAE_CHECK_ARG(p && m && v && g_slabs && seg_nslab && hyper && step && n > 0 && (n % 64) == 0 && max_nslab >= 0);
    const OptimArgs a = {p, m, v, g_slabs, slab_stride, seg_nslab, n, hyper, step};
    if (rule == RAAE_OPT_RADAM) launch_optim<RAAE_OPT_RADAM>(a, max_nslab, (hipStream_t)stream);
    else launch_optim<RAAE_OPT_ADABOUND>(a, max_nslab, (hipStream_t)stream);
    RAAE_LAUNCH_RET();
}

extern "C" int raae_optim_step_chk(float* p, float* m, float* v, const float* g_slabs, long slab_stride,
                                   const unsigned short* seg_nslab, long n, int rule, const double* hyper, const int* step,
                                   int max_nslab, int* nan_step, void* stream) {
    RAAE_CHECK_ARG(rule >= RAAE_OPT_ADAM && rule <= RAAE_OPT_ADABOUND && nan_step);
    RAAE_CHECK_ARG(p && m && v && g_slabs && seg_nslab && hyper && step && n > 0 && (n % 64) == 0 && max_nslab >= 0);
    const hipStream_t st = (hipStream_t)stream;
    if (rule == RAAE_OPT_ADAM || rule == RAAE_OPT_ADAMW) {
        const AdamChkArgs c = {{p, m, v, g_slabs, slab_stride, seg_nslab, n, hyper, step, rule == RAAE_OPT_ADAMW}, nan_step};
        if (max_nslab > 16) raae::launch(adam_wide_chk_kernel, adam_wide_chk_kernel_m, optim_grid(n, max_nslab), dim3(256), 0, st, c);
        else raae::launch(adam_chk_kernel, adam_chk_kernel_m, optim_grid(n, max_nslab), dim3(256), 0, st, c);
    } else {
        const OptimChkArgs c = {{p, m, v, g_slabs, slab_stride, seg_nslab, n, hyper, step}, nan_step};
        if (rule == RAAE_OPT_RADAM) launch_optim_chk<RAAE_OPT_RADAM>(c, max_nslab, st);
        else launch_optim_chk<RAAE_OPT_ADABOUND>(c, max_nslab, st);
    }
    RAAE_LAUNCH_RET();
}

extern "C" int raae_optim_step_clip(float* p, float* m, float* v, const float* g_slabs, long slab_stride,
                                    const unsigned short* seg_nslab, long n, int rule, const double* hyper, const int* step,
                                    int max_nslab, int* nan_step, const float* scale, void* stream) {
    if (scale == nullptr)               // no scale: the entries without one, launch for launch
        return nan_step ? raae_optim_step_chk(p, m, v, g_slabs, slab_stride, seg_nslab, n, rule, hyper, step, max_nslab, nan_step, stream)
                        : raae_optim_step(p, m, v, g_slabs, slab_stride, seg_nslab, n, rule, hyper, step, max_nslab, stream);
    RAAE_CHECK_ARG(rule >= RAAE_OPT_ADAM && rule <= RAAE_OPT_ADABOUND);
    RAAE_CHECK_ARG(p && m && v && g_slabs && seg_nslab && hyper && step && n > 0 && (n % 64) == 0 && max_nslab >= 0);
    const hipStream_t st = (hipStream_t)stream;
    if (rule == RAAE_OPT_ADAM || rule == RAAE_OPT_ADAMW) {
        const AdamChkArgs c = {{p, m, v, g_slabs, slab_stride, seg_nslab, n, hyper, step, rule == RAAE_OPT_ADAMW, scale}, nan_step};
        const dim3 grid = optim_grid(n, max_nslab), block(256);
        if (max_nslab > 16) {
            if (nan_step) raae::launch(adam_clip_kernel<true, true>, adam_clip_kernel_m<true, true>, grid, block, 0, st, c);
            else raae::launch(adam_clip_kernel<false, true>, adam_clip_kernel_m<false, true>, grid, block, 0, st, c);
        } else {
            if (nan_step) raae::launch(adam_clip_kernel<true, false>, adam_clip_kernel_m<true, false>, grid, block, 0, st, c);
            else raae::launch(adam_clip_kernel<false, false>, adam_clip_kernel_m<false, false>, grid, block, 0, st, c);
        }
    } else {
        const OptimChkArgs c = {{p, m, v, g_slabs, slab_stride, seg_nslab, n, hyper, step, scale}, nan_step};
        if (rule == RAAE_OPT_RADAM) launch_optim_clip<RAAE_OPT_RADAM>(c, max_nslab, st);
        else launch_optim_clip<RAAE_OPT_ADABOUND>(c, max_nslab, st);
    }
    RAAE_LAUNCH_RET();
}

extern "C" int raae_grad_norm(const float* g_slabs, long slab_stride, const unsigned short* seg_nslab, long n, int max_nslab,
                              double max_norm, double* partial, unsigned* ticket, float* out, int* clipped, void* stream) {
    RAAE_CHECK_ARG(g_slabs && seg_nslab && partial && ticket && out && clipped && n > 0 && (n % 64) == 0 && max_nslab >= 0);
    RAAE_CHECK_ARG(max_norm > 0.0 && max_norm <= 1.7976931348623157e308);      // finite, > 0 (false for NaN)
    const GradNormArgs a = {g_slabs, slab_stride, seg_nslab, n, max_norm, partial, ticket, out, clipped};
    long g = max_nslab > 16 ? (n + 31) / 32 : (n + 255) / 256;      // the update kernels' split of the elements ...
    if (g > GRAD_NORM_PARTS) g = GRAD_NORM_PARTS;                   // ... over at most as many workgroups as `partial` holds
    if (max_nslab > 16) raae::launch(grad_norm_wide_kernel, grad_norm_wide_kernel_m, dim3((int)g), dim3(256), 0, (hipStream_t)stream, a);
    else raae::launch(grad_norm_kernel, grad_norm_kernel_m, dim3((int)g), dim3(256), 0, (hipStream_t)stream, a);
    RAAE_LAUNCH_RET();
}

extern "C" int raae_ema_step(float* ema, const float* p, long n, double decay, void* stream) {
    RAAE_CHECK_ARG(ema && p && n >= 1 && decay >= 0.0 && decay < 1.0);      // (false for a NaN decay)
    const EmaArgs a = {ema, p, n, (float)decay, (float)(1.0 - decay)};
    // sized for four elements per thread whatever the alignment (one geometry per n: trials of a batch agree), at most
    // 64 workgroups -- the arena is a few tens of thousands of floats; above 65536 elements the kernel grid-strides
    long g = ((n + 3) / 4 + 255) / 256;
    if (g > 64) g = 64;
    raae::launch(ema_kernel, ema_kernel_m, dim3((int)g), dim3(256), 0, (hipStream_t)stream, a);
    RAAE_LAUNCH_RET();
}

extern "C" int raae_step_tick(int* steps, int n, unsigned mask, unsigned long long* rng_counter, int* cursor,
                              int cursor_inc, void* stream) {
    RAAE_CHECK_ARG(steps && n >= 0 && n <= 32);
    RAAE_PLAIN_LAUNCH(tick_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, steps, n, mask, rng_counter, cursor, cursor_inc);
    RAAE_LAUNCH_RET();
}

extern "C" int raae_rng_fill(float* tape, const int* seg_desc, const float* seg_scale, int nseg, long total,
                             unsigned long long seed, const unsigned long long* counter, void* stream) {
    RAAE_CHECK_ARG(tape && seg_desc && seg_scale && nseg > 0 && total > 0);
    long g = (total / 4 + 255) / 256;
    if (g > 4096) g = 4096;
    if (g < 1) g = 1;
    const RngFillArgs a = {tape, seg_desc, seg_scale, nseg, total, seed, counter};
    raae::launch(rng_fill_kernel, rng_fill_kernel_m, dim3((int)g), dim3(256), 0, (hipStream_t)stream, a);
    RAAE_LAUNCH_RET();
}

extern "C" int raae_step_begin(const raae_step_begin_t* p, void* stream) {
    RAAE_CHECK_ARG(p && p->steps && p->nsteps >= 0 && p->nsteps <= 32 && p->rng_state && p->cursor && p->ticket);
    RAAE_CHECK_ARG(p->spec && p->aux && p->idx && p->spec_out && p->aux_out && p->B > 0 && p->L > 0 && p->n_aux > 0);
    RAAE_CHECK_ARG(p->nseg == 0 || (p->tape && p->seg_desc && p->seg_scale && p->total > 0));
    RAAE_CHECK_ARG((p->noise_goff & 3) == 0 && p->noise_goff >= 0);
    StepBeginArgs a;
    a.steps = p->steps; a.nsteps = p->nsteps; a.step_mask = p->step_mask; a.rng_state = p->rng_state; a.cursor = p->cursor;
    a.stride = p->stride; a.ticket = p->ticket; a.spec = p->spec; a.aux = p->aux; a.idx = p->idx; a.B = p->B; a.L = p->L;
    a.n_aux = p->n_aux; a.spec_noise = p->spec_noise; a.noise_tape = p->noise_tape; a.noise_goff = p->noise_goff;
    a.spec_out = p->spec_out; a.aux_out = p->aux_out; a.tape = p->tape; a.seg_desc = p->seg_desc; a.seg_scale = p->seg_scale;
    a.nseg = p->nseg; a.total = p->nseg > 0 ? p->total : 0;
    long work = (long)p->B * p->L / 4;
    if (a.total / 4 > work) work = a.total / 4;
    long g = (work + 4095) / 4096;          // ~16 quads per thread ...
    if (g > 1024) g = 1024;                 // ... up to 1024 workgroups (their tickets, ~40 us, come back during ~45 us of fill at 4096 rows)
    if (g < 64) g = 64;
    raae::launch(step_begin_kernel, step_begin_kernel_m, dim3((int)g), dim3(256), 0, (hipStream_t)stream, a);
    RAAE_LAUNCH_RET();
}

// ---------------------------------------------------------------- runtime plumbing
extern "C" int raae_graph_begin(void* stream) {
    return (int)hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeThreadLocal);
}
extern "C" int raae_graph_end(void* stream, void** graph_exec) {
    RAAE_CHECK_ARG(graph_exec);
    hipGraph_t graph = nullptr;
    hipError_t e = hipStreamEndCapture((hipStream_t)stream, &graph);
    if (e != hipSuccess) return (int)e;
    if (const char* dot = getenv("RAAE_GRAPH_DOT")) (void)hipGraphDebugDotPrint(graph, dot, hipGraphDebugDotFlagsVerbose);
    hipGraphExec_t ex = nullptr;
    e = hipGraphInstantiate(&ex, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) return (int)e;
    *graph_exec = (void*)ex;
    return 0;
}
extern "C" int raae_graph_launch(void* graph_exec, void* stream) {
    return (int)hipGraphLaunch((hipGraphExec_t)graph_exec, (hipStream_t)stream);
}
extern "C" int raae_graph_destroy(void* graph_exec) { return (int)hipGraphExecDestroy((hipGraphExec_t)graph_exec); }
extern "C" int raae_event_create(void** ev) {
    RAAE_CHECK_ARG(ev);
    hipEvent_t e; hipError_t r = hipEventCreate(&e);
    *ev = (void*)e; return (int)r;
}
extern "C" int raae_event_record(void* ev, void* stream) { return (int)hipEventRecord((hipEvent_t)ev, (hipStream_t)stream); }
extern "C" int raae_event_elapsed_ms(void* start, void* stop, float* ms) {
    RAAE_CHECK_ARG(ms);
    hipError_t r = hipEventSynchronize((hipEvent_t)stop);
    if (r != hipSuccess) return (int)r;
    return (int)hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop);
}
extern "C" int raae_event_destroy(void* ev) { return (int)hipEventDestroy((hipEvent_t)ev); }
extern "C" int raae_stream_sync(void* stream) { return (int)hipStreamSynchronize((hipStream_t)stream); }
extern "C" const char* raae_error_string(int code) {
    if (code == RAAE_EINVAL) return "raae: invalid argument (host-side shape validation failed; nothing launched)";
    return hipGetErrorString((hipError_t)code);
}
extern "C" int raae_device_info(int* cu_count, int* lds_bytes, char* name, int name_len) {
    hipDeviceProp_t prop; int dev = 0;
    hipError_t r = hipGetDevice(&dev);
    if (r != hipSuccess) return (int)r;
    r = hipGetDeviceProperties(&prop, dev);
    if (r != hipSuccess) return (int)r;
    if (cu_count) *cu_count = prop.multiProcessorCount;
    if (lds_bytes) *lds_bytes = (int)prop.sharedMemPerBlock;
    if (name && name_len > 0) { strncpy(name, prop.gcnArchName, name_len - 1); name[name_len - 1] = 0; }
    return 0;
}
extern "C" int raae_abi_version(void) { return RAAE_ABI_VERSION; }
#ifndef RAAE_SOURCE_DIGEST
#define RAAE_SOURCE_DIGEST "unknown"
#endif
extern "C" const char* raae_source_digest(void) { return RAAE_SOURCE_DIGEST; }

// ---------------------------------------------------------------- data-parallel helper
namespace {
// (argument block + `_m` twins: with `grad_clip_norm` the flat gradient is part of a batched trial's step too)
struct SlabReduceArgs { const float* g_slabs; long slab_stride; const unsigned short* seg_nslab; long n; float* out; };
__device__ __forceinline__ void slab_reduce_body(const float* g_slabs, long slab_stride,
                                                 const unsigned short* seg_nslab, long n, float* out) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int ns = seg_nslab[i >> 6];
        float g = 0.f;
        int s = 0;
        for (; s + 8 <= ns; s += 8) {
            float t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) t[u] = g_slabs[(size_t)(s + u) * slab_stride + i];
#pragma unroll
            for (int u = 0; u < 8; ++u) g += t[u];
        }
        for (; s < ns; ++s) g += g_slabs[(size_t)s * slab_stride + i];
        out[i] = g;
    }
}
// the summation tree of adam_wide_kernel (8 lanes per element), so that the data-parallel path adds the
// slabs of a rank in exactly the order the single-GPU update does
__device__ __forceinline__ void slab_reduce_wide_body(const float* g_slabs, long slab_stride,
                                                      const unsigned short* seg_nslab, long n, float* out) {
    const int lane = threadIdx.x & 63, el = lane & 7, ch = lane >> 3;
    const long wave0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 8;
    for (long base = wave0; base < n; base += (long)gridDim.x * 32) {
        const long i = base + el;
        const int ns = seg_nslab[i >> 6];
        float g = 0.f;
        for (int s = ch; s < ns; s += 64) {
            float t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int r = s + 8 * u;
                t[u] = g_slabs[(size_t)(r < ns ? r : ch) * slab_stride + i];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) g += (s + 8 * u < ns) ? t[u] : 0.f;
        }
        g += __shfl_xor(g, 8, 64);
        g += __shfl_xor(g, 16, 64);
        g += __shfl_xor(g, 32, 64);
        if (ch == 0) out[i] = g;
    }
}
__global__ __launch_bounds__(256) void slab_reduce_kernel(SlabReduceArgs a) {
    slab_reduce_body(a.g_slabs, a.slab_stride, a.seg_nslab, a.n, a.out);
}
__global__ __launch_bounds__(256) void slab_reduce_kernel_m(const SlabReduceArgs* t) {
    const SlabReduceArgs a = t[blockIdx.z];
    slab_reduce_body(a.g_slabs, a.slab_stride, a.seg_nslab, a.n, a.out);
}
__global__ __launch_bounds__(256) void slab_reduce_wide_kernel(SlabReduceArgs a) {
    slab_reduce_wide_body(a.g_slabs, a.slab_stride, a.seg_nslab, a.n, a.out);
}
__global__ __launch_bounds__(256) void slab_reduce_wide_kernel_m(const SlabReduceArgs* t) {
    const SlabReduceArgs a = t[blockIdx.z];
    slab_reduce_wide_body(a.g_slabs, a.slab_stride, a.seg_nslab, a.n, a.out);
}
}  // namespace

extern "C" int raae_slab_reduce(const float* g_slabs, long slab_stride, const unsigned short* seg_nslab, long n,
                                float* out, int max_nslab, void* stream) {
    RAAE_CHECK_ARG(g_slabs && seg_nslab && out && n > 0 && (n % 64) == 0 && max_nslab >= 0);
    const SlabReduceArgs a = {g_slabs, slab_stride, seg_nslab, n, out};
    if (max_nslab > 16) {
        long g = (n + 31) / 32;
        if (g > 4096) g = 4096;
        raae::launch(slab_reduce_wide_kernel, slab_reduce_wide_kernel_m, dim3((int)g), dim3(256), 0, (hipStream_t)stream, a);
    } else {
        long g = (n + 255) / 256;
        if (g > 4096) g = 4096;
        raae::launch(slab_reduce_kernel, slab_reduce_kernel_m, dim3((int)g), dim3(256), 0, (hipStream_t)stream, a);
    }
    RAAE_LAUNCH_RET();
}


// ---------------------------------------------------------------- batched launches over trials (raae_common.h)
#include <cstdio>
#include <string>
#include <vector>
namespace {
struct LaunchRec { const void* fn; dim3 grid, block; unsigned lds, nbytes; unsigned char args[4096]; };
struct Recording { std::vector<LaunchRec> recs; bool bad = false; std::string refused; };
thread_local Recording* g_recording = nullptr;
thread_local std::string g_refusal;      // why this thread's last recording or program build was refused
struct MultiProgram { std::vector<LaunchRec> recs; std::vector<size_t> off; unsigned char* table = nullptr; int T = 0; };
void refuse(Recording* r, const std::string& why) {
    if (!r->bad) r->refused = why;       // the first offending launch
    r->bad = true;
}
}  // namespace
void raae::record_launch(const void* multi_fn, dim3 grid, dim3 block, size_t lds, const void* args, size_t nbytes) {
    Recording* r = g_recording;
    if (!r) return;
    LaunchRec rec;
    if (nbytes > sizeof(rec.args) || grid.z != 1) {
        refuse(r, "launch " + std::to_string(r->recs.size()) + ": " + std::to_string(nbytes) + "-byte argument block or a 3-D grid");
        return;
    }
    rec.fn = multi_fn; rec.grid = grid; rec.block = block; rec.lds = (unsigned)lds; rec.nbytes = (unsigned)nbytes;
    memcpy(rec.args, args, nbytes);
    r->recs.push_back(rec);
}
void raae::record_unsupported(const char* kernel) {
    if (g_recording) refuse(g_recording, kernel);
}
extern "C" int raae_record_begin(void) {
    if (g_recording) return RAAE_EINVAL;
    g_recording = new Recording();
    g_refusal.clear();
    return 0;
}
extern "C" int raae_record_end(void** handle, int* n_launches) {
    RAAE_CHECK_ARG(handle && g_recording);
    Recording* r = g_recording;
    g_recording = nullptr;
    if (r->bad) { g_refusal = r->refused; delete r; return RAAE_EINVAL; }
    if (n_launches) *n_launches = (int)r->recs.size();
    *handle = r;
    return 0;
}
extern "C" int raae_record_refusal(char* buf, int n) {
    RAAE_CHECK_ARG(buf && n > 0);
    snprintf(buf, (size_t)n, "%s", g_refusal.c_str());
    return (int)g_refusal.size();
}
extern "C" int raae_record_free(void* handle) { delete (Recording*)handle; return 0; }
extern "C" int raae_multi_build(void* const* handles, int T, void** program) {
    RAAE_CHECK_ARG(handles && program && T >= 1 && T <= 64);
    const Recording* r0 = (const Recording*)handles[0];
    RAAE_CHECK_ARG(r0 && !r0->recs.empty());
    MultiProgram* mp = new MultiProgram();
    mp->T = T; mp->recs = r0->recs;
    size_t total = 0;
    for (size_t i = 0; i < r0->recs.size(); ++i) {
        mp->off.push_back(total);
        total += ((size_t)T * r0->recs[i].nbytes + 255) & ~(size_t)255;
    }
    std::vector<unsigned char> host(total, 0);
    for (int t = 0; t < T; ++t) {
        const Recording* r = (const Recording*)handles[t];
        if (!r || r->recs.size() != r0->recs.size()) {
            g_refusal = "trial " + std::to_string(t) + " logged " + std::to_string(r ? r->recs.size() : 0) +
                        " launches, trial 0 " + std::to_string(r0->recs.size());
            delete mp;
            return RAAE_EINVAL;
        }
        for (size_t i = 0; i < r->recs.size(); ++i) {
            const LaunchRec &a = r0->recs[i], &b = r->recs[i];
            // the trials must be structurally identical: same kernel instance, geometry and LDS at every launch
            if (a.fn != b.fn || a.grid.x != b.grid.x || a.grid.y != b.grid.y || a.block.x != b.block.x || a.lds != b.lds ||
                a.nbytes != b.nbytes) {
                g_refusal = "launch " + std::to_string(i) + " of trial " + std::to_string(t) +
                            " differs from trial 0's in kernel instance, geometry or LDS";
                delete mp;
                return RAAE_EINVAL;
            }
            memcpy(host.data() + mp->off[i] + (size_t)t * a.nbytes, b.args, a.nbytes);
        }
    }
    hipError_t e = hipMalloc((void**)&mp->table, total);
    if (e != hipSuccess) { delete mp; return (int)e; }
    e = hipMemcpy(mp->table, host.data(), total, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(mp->table); delete mp; return (int)e; }
    *program = mp;
    return 0;
}
extern "C" int raae_multi_launch(void* program, void* stream) {
    RAAE_CHECK_ARG(program);
    MultiProgram* mp = (MultiProgram*)program;
    for (size_t i = 0; i < mp->recs.size(); ++i) {
        const LaunchRec& r = mp->recs[i];
        void* tptr = mp->table + mp->off[i];
        void* params[1] = {&tptr};
        const hipError_t e = hipLaunchKernel(r.fn, dim3(r.grid.x, r.grid.y, mp->T), r.block, params, r.lds, (hipStream_t)stream);
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}
extern "C" int raae_multi_count(void* program) { return program ? (int)((MultiProgram*)program)->recs.size() : 0; }
extern "C" int raae_multi_free(void* program) {
    if (!program) return 0;
    MultiProgram* mp = (MultiProgram*)program;
    if (mp->table) (void)hipFree(mp->table);
    delete mp;
    return 0;
}
