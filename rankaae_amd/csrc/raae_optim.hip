// Fused multi-tensor Adam/AdamW, RAdam and AdaBound over the flat parameter arena, the per-step tick,
// the Philox random tape, and HIP stream/graph/event plumbing.
#include "raae_common.h"
#include "raae_philox.h"
#include <string.h>
#include <stdlib.h>

namespace {

#include "raae_optim_body.inc"

// ---- the update kernels: every rule x {one thread per element, WIDE} x {plain, CHK} x {no scale, SC} ----
// (update_body: raae_optim_body.inc)
template <int RULE, bool WIDE, bool CHK, bool SC>
__global__ __launch_bounds__(256) void update_kernel(UpdateArgs a) { update_body<RULE, WIDE, CHK, SC>(a, blockIdx.x, gridDim.x); }
template <int RULE, bool WIDE, bool CHK, bool SC>
__global__ __launch_bounds__(256) void update_kernel_m(const UpdateArgs* t) {
    const UpdateArgs a = t[blockIdx.z];
    update_body<RULE, WIDE, CHK, SC>(a, blockIdx.x, gridDim.x);
}
// the instance of [rule][WIDE][CHK][SC]; Adam and AdamW share a family (UpdateArgs::decoupled)
struct UpdateInst { void (*single)(UpdateArgs); void (*multi)(const UpdateArgs*); };
#define RAAE_UPD(R, W, C, S) {update_kernel<R, W, C, S>, update_kernel_m<R, W, C, S>}
#define RAAE_UPD_SHAPE(R, W) {{RAAE_UPD(R, W, false, false), RAAE_UPD(R, W, false, true)},                            \
                              {RAAE_UPD(R, W, true, false), RAAE_UPD(R, W, true, true)}}
#define RAAE_UPD_RULE(R) {RAAE_UPD_SHAPE(R, false), RAAE_UPD_SHAPE(R, true)}
const UpdateInst kUpdate[4][2][2][2] = {RAAE_UPD_RULE(RAAE_OPT_ADAM), RAAE_UPD_RULE(RAAE_OPT_ADAM),
                                        RAAE_UPD_RULE(RAAE_OPT_RADAM), RAAE_UPD_RULE(RAAE_OPT_ADABOUND)};
#undef RAAE_UPD_RULE
#undef RAAE_UPD_SHAPE
#undef RAAE_UPD

// the shape and grid of every kernel that sums slabs (update, norm, reduce): above 16 slabs 8 lanes per element (32
// elements per workgroup), else one element per thread; at most `cap` workgroups
inline bool optim_wide(int max_nslab) { return max_nslab > 16; }
inline dim3 optim_grid(long n, int max_nslab, long cap = 4096) {
    long g = optim_wide(max_nslab) ? (n + 31) / 32 : (n + 255) / 256;
    if (g > cap) g = cap;
    return dim3((int)g);
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
    for_each_grad<WIDE, false>(a.g_slabs, a.slab_stride, a.seg_nslab, a.n, blockIdx.x, gridDim.x,
                               [&](long, float g) { acc += (double)g * (double)g; });
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
template <bool WIDE> __global__ __launch_bounds__(256) void grad_norm_kernel(GradNormArgs a) { grad_norm_body<WIDE>(a); }
template <bool WIDE> __global__ __launch_bounds__(256) void grad_norm_kernel_m(const GradNormArgs* t) {
    const GradNormArgs a = t[blockIdx.z];
    grad_norm_body<WIDE>(a);
}

// ---- the data-parallel helper: out[i] = the slab sum of element i, 0 for a segment without slabs ----
// Summed as the update sums, so that the data-parallel path adds the slabs of a rank in exactly the order the
// single-GPU update does.
// (argument block + `_m` twins: with `grad_clip_norm` the flat gradient is part of a batched trial's step too)
struct SlabReduceArgs { const float* g_slabs; long slab_stride; const unsigned short* seg_nslab; long n; float* out; };
template <bool WIDE>
__device__ __forceinline__ void slab_reduce_body(const SlabReduceArgs& a) {
    for_each_grad<WIDE, true>(a.g_slabs, a.slab_stride, a.seg_nslab, a.n, blockIdx.x, gridDim.x,
                              [&](long i, float g) { a.out[i] = g; });
}
template <bool WIDE> __global__ __launch_bounds__(256) void slab_reduce_kernel(SlabReduceArgs a) { slab_reduce_body<WIDE>(a); }
template <bool WIDE> __global__ __launch_bounds__(256) void slab_reduce_kernel_m(const SlabReduceArgs* t) {
    const SlabReduceArgs a = t[blockIdx.z];
    slab_reduce_body<WIDE>(a);
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

// The one launch path of the update, and the entry of a clipped one: the rule picks the family, max_nslab the shape and
// the grid, nan_step != NULL the checked and scale != NULL the clipped variant.  The entries without a flag word or a
// scale pass NULL: the same kernel, the same grid (raae_multi_build compares both across trials).
extern "C" int raae_optim_step_clip(float* p, float* m, float* v, const float* g_slabs, long slab_stride,
                                    const unsigned short* seg_nslab, long n, int rule, const double* hyper, const int* step,
                                    int max_nslab, int* nan_step, const float* scale, void* stream) {
    RAAE_CHECK_ARG(rule >= RAAE_OPT_ADAM && rule <= RAAE_OPT_ADABOUND);
    RAAE_CHECK_ARG(p && m && v && g_slabs && seg_nslab && hyper && step && n > 0 && (n % 64) == 0 && max_nslab >= 0);
    const UpdateArgs a = {p, m, v, g_slabs, slab_stride, seg_nslab, n, hyper, step, rule == RAAE_OPT_ADAMW, scale, nan_step};
    const UpdateInst& k = kUpdate[rule][optim_wide(max_nslab)][nan_step != nullptr][scale != nullptr];
    raae::launch(k.single, k.multi, optim_grid(n, max_nslab), dim3(256), 0, (hipStream_t)stream, a);
    RAAE_LAUNCH_RET();
}

extern "C" int raae_optim_step_chk(float* p, float* m, float* v, const float* g_slabs, long slab_stride,
                                   const unsigned short* seg_nslab, long n, int rule, const double* hyper, const int* step,
                                   int max_nslab, int* nan_step, void* stream) {
    RAAE_CHECK_ARG(nan_step);
    return raae_optim_step_clip(p, m, v, g_slabs, slab_stride, seg_nslab, n, rule, hyper, step, max_nslab, nan_step, nullptr, stream);
}

extern "C" int raae_optim_step(float* p, float* m, float* v, const float* g_slabs, long slab_stride,
                               const unsigned short* seg_nslab, long n, int rule, const double* hyper, const int* step,
                               int max_nslab, void* stream) {
    return raae_optim_step_clip(p, m, v, g_slabs, slab_stride, seg_nslab, n, rule, hyper, step, max_nslab, nullptr, nullptr, stream);
}

extern "C" int raae_adam_step(float* p, float* m, float* v, const float* g_slabs, long slab_stride,
                              const unsigned short* seg_nslab, long n, const double* hyper, const int* step,
                              int decoupled, int max_nslab, void* stream) {
    return raae_optim_step(p, m, v, g_slabs, slab_stride, seg_nslab, n, decoupled ? RAAE_OPT_ADAMW : RAAE_OPT_ADAM, hyper, step,
                           max_nslab, stream);
}

extern "C" int raae_grad_norm(const float* g_slabs, long slab_stride, const unsigned short* seg_nslab, long n, int max_nslab,
                              double max_norm, double* partial, unsigned* ticket, float* out, int* clipped, void* stream) {
    RAAE_CHECK_ARG(g_slabs && seg_nslab && partial && ticket && out && clipped && n > 0 && (n % 64) == 0 && max_nslab >= 0);
    RAAE_CHECK_ARG(max_norm > 0.0 && max_norm <= 1.7976931348623157e308);      // finite, > 0 (false for NaN)
    const GradNormArgs a = {g_slabs, slab_stride, seg_nslab, n, max_norm, partial, ticket, out, clipped};
    const dim3 grid = optim_grid(n, max_nslab, GRAD_NORM_PARTS);    // at most as many workgroups as `partial` holds
    if (optim_wide(max_nslab)) raae::launch(grad_norm_kernel<true>, grad_norm_kernel_m<true>, grid, dim3(256), 0, (hipStream_t)stream, a);
    else raae::launch(grad_norm_kernel<false>, grad_norm_kernel_m<false>, grid, dim3(256), 0, (hipStream_t)stream, a);
    RAAE_LAUNCH_RET();
}

extern "C" int raae_slab_reduce(const float* g_slabs, long slab_stride, const unsigned short* seg_nslab, long n,
                                float* out, int max_nslab, void* stream) {
    RAAE_CHECK_ARG(g_slabs && seg_nslab && out && n > 0 && (n % 64) == 0 && max_nslab >= 0);
    const SlabReduceArgs a = {g_slabs, slab_stride, seg_nslab, n, out};
    const dim3 grid = optim_grid(n, max_nslab);
    if (optim_wide(max_nslab)) raae::launch(slab_reduce_kernel<true>, slab_reduce_kernel_m<true>, grid, dim3(256), 0, (hipStream_t)stream, a);
    else raae::launch(slab_reduce_kernel<false>, slab_reduce_kernel_m<false>, grid, dim3(256), 0, (hipStream_t)stream, a);
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
