// The argument blocks and the wide (8 lanes per element) body of the fused Adam / AdamW update: included by
// raae_optim.hip (adam_wide_kernel and its checked twin) and by raae_conv.hip, where the update of one network's
// slice of an optimizer's range rides in the launch of a block kernel (co_kernel).  `bx` / `gx`: the workgroup's
// index and the number of workgroups among those that run this body.
// torch.optim.Adam / AdamW single-tensor update (torch/optim/adam.py::_single_tensor_adam),
// operation order mirrored in fp32; scalars formed in double like Python floats.
// Gradient of element i = fixed-order sum of seg_nslab[i/64] slabs; 0 slabs => parameter is
// skipped (the reference skips params whose .grad is None, trainer.py:318-321).
struct AdamArgs { float* p; float* m; float* v; const float* g_slabs; long slab_stride; const unsigned short* seg_nslab;
                  long n; const double* hyper; const int* step; int decoupled;
                  const float* gscale; };   // NULL, or the clip scale of raae_grad_norm (read by the SC = true instances only)

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

// checked twins: the argument block of the unchecked kernel + the flag word
struct AdamChkArgs { AdamArgs a; int* nan_step; };

// Same update with the slabs of an element spread over 8 lanes: for ranges whose tensors have many slabs.
template <bool CHK, bool SC = false>
__device__ __forceinline__ void adam_wide_body(float* p, float* m, float* v, const float* g_slabs, long slab_stride,
                                               const unsigned short* seg_nslab, long n, const double* hyper,
                                               const int* step, int decoupled, int* nan_step, const int bx, const int gx,
                                               const float* gscale = nullptr) {
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
    // A wave owns 8 consecutive elements; lane = chunk*8 + element: the slabs of an element are spread over
    // 8 lanes (chunk c sums slabs c, c+8, ... eight loads deep), joined by a fixed xor-shuffle tree.  With one
    // thread per element the 256 slabs of a conv weight were 32 dependent round trips (28 us per step phase).
    const int lane = threadIdx.x & 63, el = lane & 7, ch = lane >> 3;
    const long wave0 = ((long)bx * 4 + (threadIdx.x >> 6)) * 8;
    bool seen = false;
    float gs = 1.f;
    if (SC) gs = gscale[0];
    for (long base = wave0; base < n; base += (long)gx * 32) {
        // No contraction into fma: as compiled into adam_wide_kernel none of the multiply-adds below is contracted (the
        // packed multiplies and adds come first), inlined into another kernel some are -- pinned, so that the update
        // rounds the same wherever the body is instantiated.
#pragma clang fp contract(off)
        const long i = base + el;                       // n is a multiple of 64: i < n whenever base < n
        const int ns = seg_nslab[i >> 6];
        if (ns == 0) continue;                          // uniform over the wave (8 elements share a segment)
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
        if (ch != 0) continue;
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
