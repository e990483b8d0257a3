// The fused optimizer update, from the slab sum to the rule: included by raae_optim.hip (the update, norm and reduce
// kernels) and by raae_conv.hip, where the update of one network's slice of an optimizer's range rides in the launch
// of a block kernel (co_kernel).  `bx` / `gx`: the workgroup's index and the number of workgroups among those that run
// a body.
// Gradient of element i = fixed-order sum of seg_nslab[i/64] slabs; 0 slabs => parameter is
// skipped (the reference skips params whose .grad is None, trainer.py:318-321).

// ---- the slab sum: one thread per element, or the slabs of an element spread over 8 lanes ----
// Every kernel that reads a gradient -- update, norm, reduce -- sums through these two, so clipping, the data-parallel
// path and the clip scale of 1.0 see the same additions in the same order.
// One thread per element: 8 independent loads in flight at a time, then the tail.
__device__ __forceinline__ float slab_sum(const float* g_slabs, long slab_stride, int ns, long i) {
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
    return g;
}
// 8 lanes per element, lane = chunk*8 + element of the wave's 8: chunk c sums slabs c, c+8, ... eight loads deep (a row
// index past the count reads row c instead and adds 0), joined by a fixed xor-shuffle tree; every lane of the wave
// calls it and every lane holds the sum.  With one thread per element the 256 slabs of a conv weight were 32 dependent
// round trips (28 us per step phase).
__device__ __forceinline__ float slab_sum_wide(const float* g_slabs, long slab_stride, int ns, long i) {
    const int ch = (threadIdx.x & 63) >> 3;
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
    return g;
}

// The walk over a range's elements: act(i, g) once per element i, on the lane that owns it, g its slab sum.  A segment
// without slabs is skipped, or with EMPTY walked with g = 0.  Narrow: the thread grid-stride loop; WIDE: a wave owns 8
// consecutive elements per pass (32 per workgroup).
template <bool WIDE, bool EMPTY, class Act>
__device__ __forceinline__ void for_each_grad(const float* g_slabs, long slab_stride, const unsigned short* seg_nslab,
                                              long n, const int bx, const int gx, Act act) {
    if constexpr (WIDE) {
        const int lane = threadIdx.x & 63, el = lane & 7, ch = lane >> 3;
        for (long base = ((long)bx * 4 + (threadIdx.x >> 6)) * 8; base < n; base += (long)gx * 32) {
            const long i = base + el;                       // n is a multiple of 64: i < n whenever base < n
            const int ns = seg_nslab[i >> 6];
            if (!EMPTY && ns == 0) continue;                // uniform over the wave (8 elements share a segment)
            const float g = slab_sum_wide(g_slabs, slab_stride, ns, i);
            if (ch == 0) act(i, g);
        }
    } else {
        for (long i = (long)bx * 256 + threadIdx.x; i < n; i += (long)gx * 256) {
            const int ns = seg_nslab[i >> 6];
            if (!EMPTY && ns == 0) continue;
            act(i, slab_sum(g_slabs, slab_stride, ns, i));
        }
    }
}

// Gradient clipping (SC = true; raae_optim_step_clip): the slab-summed gradient times *gscale, the scale raae_grad_norm
// left, before weight decay and the moments; the NaN check looks at the gradient before the scale.  The product is
// handed on through an empty asm statement: the update that follows then compiles as it does on the slab sum itself
// (the product is never contracted into an add, never packed with another multiply), so that a scale of exactly 1.0f
// gives the bits of the instance without a scale.
__device__ __forceinline__ float scale_grad(float g, float gs) {
    float r = g * gs;
    asm volatile("" : "+v"(r));
    return r;
}

// NaN check of the checked instances (CHK = true; raae_optim_step_chk): every lane keeps whether a gradient it summed
// was NaN, the wave votes once after its loop, and one lane of a wave that saw one writes the optimizer's step count
// (1-based) into *nan_step if that still holds 0 -- the first step stays.  NaN only, as autograd's anomaly mode: an
// Inf gradient turns m / v / p into NaN and the next step's gradient is NaN.  Nothing else of the update changes.
__device__ __forceinline__ void nan_vote(bool seen, int* nan_step, const int* step) {
    if (__ballot(seen) != 0ull && (threadIdx.x & 63) == 0) atomicCAS(nan_step, 0, step[0]);
}

// ---- the rules ----
// One kernel family per rule: OptRule<R>::scalars forms the NSC per-step scalars in double (Python floats) from the
// device hyper block and step count, in the operation order of the Python source; OptRule<R>::update<WIDE> is the
// per-element fp32 update in the order of the torch ops.
// The argument block of every update kernel; the plain instances read neither gscale nor nan_step.
struct UpdateArgs { float* p; float* m; float* v; const float* g_slabs; long slab_stride; const unsigned short* seg_nslab;
                    long n; const double* hyper; const int* step;
                    int decoupled;              // the Adam family: AdamW's decay of p instead of Adam's of g
                    const float* gscale;        // NULL, or the clip scale of raae_grad_norm (SC = true instances only)
                    int* nan_step; };           // NULL, or the flag word of the checked instances (CHK = true)
template <int RULE> struct OptRule;

// torch.optim.Adam / AdamW single-tensor update (torch/optim/adam.py::_single_tensor_adam), one family for both
// (UpdateArgs::decoupled).
template <> struct OptRule<RAAE_OPT_ADAM> {
    static constexpr int NSC = 8;
    __device__ static void scalars(const double* h, int step, float* s) {
        const double lr = h[0], b1 = h[1], b2 = h[2], eps = h[3], wd = h[4];
        const double t = (double)step;
        const double bc1 = 1.0 - pow(b1, t), bc2 = 1.0 - pow(b2, t);
        s[0] = (float)(1.0 - lr * wd);      // AdamW decay factor
        s[1] = (float)(1.0 - b1);           // lerp weight
        s[2] = (float)b2;
        s[3] = (float)(1.0 - b2);
        s[4] = (float)(-(lr / bc1));        // -step_size
        s[5] = (float)sqrt(bc2);
        s[6] = (float)eps;
        s[7] = (float)wd;
    }
    // The two shapes round their multiply-adds differently, and both roundings are kept: one text, compiled twice.
    // WIDE: no contraction into fma -- as compiled into the wide kernel alone none of the multiply-adds is contracted
    // (the packed multiplies and adds come first), inlined into co_kernel some are -- pinned, so that the update rounds
    // the same wherever the body is instantiated.  One thread per element: the default, under which the compiler may
    // form fma (it does for the weight decay of g).
#define RAAE_ADAM_UPDATE                                                                                              \
    if (a.decoupled) p = p * s[0]; else if (s[7] != 0.f) g = g + s[7] * p;                                            \
    m = m + s[1] * (g - m);                                                                                           \
    v = v * s[2];                                                                                                     \
    v = v + (s[3] * g) * g;                                                                                           \
    const float denom = sqrtf(v) / s[5] + s[6];                                                                       \
    p = p + (s[4] * m) / denom;
    template <bool WIDE>
    __device__ static __forceinline__ void update(const UpdateArgs& a, const float (&s)[NSC], float& p, float& m, float& v,
                                                  float g) {
        if constexpr (WIDE) {
#pragma clang fp contract(off)
            RAAE_ADAM_UPDATE
        } else {
            RAAE_ADAM_UPDATE
        }
    }
#undef RAAE_ADAM_UPDATE
};

// ---- RAdam and AdaBound (torch_optimizer 0.1.0, the optimizer_name values the reference takes from that package) ----
// (no contraction into fma in their scalars; their updates compile under the default in both shapes)
// torch_optimizer.RAdam.step.  The class caches (t, N, step size) in a 10-entry buffer keyed on t % 10, filled by the
// first tensor stepped at a given t; every tensor of one optimizer here shares one step count, so the cache always
// holds what the formula gives at the current lr, and the formula is evaluated directly.  N is formed in double in
// this order: at t = 5 it misses 5 by only 4e-3 (beta2 = 0.999) or 4e-4 (0.9999); t = 6 is the first rectified step.
template <> struct OptRule<RAAE_OPT_RADAM> {
    static constexpr int NSC = 10;
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
    template <bool WIDE>
    __device__ static void update(const UpdateArgs&, const float (&s)[NSC], float& p, float& m, float& v, float g) {
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
    static constexpr int NSC = 10;
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
    template <bool WIDE>
    __device__ static void update(const UpdateArgs&, const float (&s)[NSC], float& p, float& m, float& v, float g) {
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

// ---- the update of every rule, shape and variant: update_kernel (raae_optim.hip), CoAdam (raae_conv.hip) ----
template <int RULE, bool WIDE, bool CHK, bool SC>
__device__ __forceinline__ void update_body(const UpdateArgs& a, const int bx, const int gx) {
    typedef OptRule<RULE> Rule;
    __shared__ float s_sc[Rule::NSC];
    if (threadIdx.x == 0) Rule::scalars(a.hyper, a.step[0], s_sc);
    __syncthreads();
    float sc[Rule::NSC];
#pragma unroll
    for (int k = 0; k < Rule::NSC; ++k) sc[k] = s_sc[k];
    bool seen = false;
    float gs = 1.f;
    if (SC) gs = a.gscale[0];
    for_each_grad<WIDE, false>(a.g_slabs, a.slab_stride, a.seg_nslab, a.n, bx, gx, [&](long i, float g) {
        if (CHK) seen |= __builtin_isnan(g);
        if (SC) g = scale_grad(g, gs);
        float pv = a.p[i], mv = a.m[i], vv = a.v[i];
        Rule::template update<WIDE>(a, sc, pv, mv, vv, g);
        a.p[i] = pv; a.m[i] = mv; a.v[i] = vv;
    });
    if (CHK) nan_vote(seen, a.nan_step, a.step);
}
