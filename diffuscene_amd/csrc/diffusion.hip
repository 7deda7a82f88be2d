// Elementwise DDPM steps (diffusion_ddpm.py:217-352,447-476).  HBM-bound: one read of each operand, one
// write of the result, coefficient gathers from device-resident tables.  Compiled with -ffp-contract=off:
// the reference evaluates  a*x + b*y  as two rounded products and a rounded sum; we do exactly that, so the
// results are bit-identical to the fp32 CPU path on the same inputs.
#define DSC_BAD_INDEX_COUNTER
#include "dsc_common.h"
#include <type_traits>

namespace {

// The step arithmetic, stated once.  Every product, sum and difference is a statement of its own (one rounding each, operands in the
// reference's order); the kernels below differ only in which elements they update, what they read and which indices they count.

// q_sample: a * v + s * n.  Also what a given element (completion, in-painting) gets for the next model call.
__device__ __forceinline__ float renoise(float v, float n, float a, float s) {
    const float p0 = a * v, p1 = s * n;
    return p0 + p1;
}

// x_start from the model output: m itself (mean type x0), else A * x - Bc * m (eps, v: ca / cb are the matching table pair).
__device__ __forceinline__ float predict_x0(float x, float m, float A, float Bc, int mean_type, bool clip) {
    float x0;
    if (mean_type == DSC_MEAN_X0) x0 = m;
    else { const float p0 = A * x, p1 = Bc * m; x0 = p0 - p1; }
    return clip ? fminf(fmaxf(x0, -1.0f), 1.0f) : x0;
}

// Per-scene coefficients of the posterior step at row tv.  sg is sigma[tv]; with zero_at_0 it is forced to 0 at tv == 0 (the caller
// still adds 0 * noise there), without it the caller does not read the noise at tv == 0.
struct PosteriorCoef { float A, Bc, k1, k2, sg; };

__device__ __forceinline__ PosteriorCoef posterior_coef(int64_t tv, const float* __restrict__ ca, const float* __restrict__ cb,
                                                        const float* __restrict__ c1, const float* __restrict__ c2,
                                                        const float* __restrict__ sigma, int mean_type, bool zero_at_0) {
    PosteriorCoef p;
    p.A = (mean_type == DSC_MEAN_X0) ? 0.f : ca[tv];
    p.Bc = (mean_type == DSC_MEAN_X0) ? 0.f : cb[tv];
    p.k1 = c1[tv], p.k2 = c2[tv];
    p.sg = (!zero_at_0 || tv != 0) ? sigma[tv] : 0.f;
    return p;
}

__device__ __forceinline__ float posterior_mean(float x0, float x, const PosteriorCoef& p) {
    const float m0 = p.k1 * x0, m1 = p.k2 * x;
    return m0 + m1;
}

// The last term of both updates: u + sigma * n.
__device__ __forceinline__ float add_noise(float u, float n, float sg) {
    const float nz = sg * n;
    return u + nz;
}

// Coefficients of one DDIM pair.  Every scene is at the same step: k comes from a device counter, the per-step scalars from device
// tables of S rows, so the launch can be captured once and replayed.  step[0] and times[k] are clamped and counted once per launch
// (``first``: one thread of the grid).  times_next[k] < 0 marks the last pair; a kernel that re-noises at t_next asks for it as a row
// (``want_tn``: clamped and counted like the others, 0 on the last pair), the others never index with it.
struct DdimCoef { int64_t tn; bool last; float A, Bc, R, M, an, cn, sg; };

__device__ __forceinline__ DdimCoef ddim_coef(const int64_t* __restrict__ step, const int64_t* __restrict__ times,
                                              const int64_t* __restrict__ times_next, const float* __restrict__ sqrt_an,
                                              const float* __restrict__ cnoise, const float* __restrict__ sigma,
                                              const float* __restrict__ ca, const float* __restrict__ cb, const float* __restrict__ ra,
                                              const float* __restrict__ rm, int mean_type, int S, int T, bool first, bool want_tn) {
    DdimCoef d;
    const int64_t k = dsc_checked_index(step[0], S, first);
    const int64_t tv = dsc_checked_index(times[k], T, first);
    const int64_t tn_raw = times_next[k];
    d.last = tn_raw < 0;
    d.tn = (d.last || !want_tn) ? 0 : dsc_checked_index(tn_raw, T, first);
    d.A = (mean_type == DSC_MEAN_X0) ? 0.f : ca[tv];
    d.Bc = (mean_type == DSC_MEAN_X0) ? 0.f : cb[tv];
    d.R = ra[tv], d.M = rm[tv];
    d.an = sqrt_an[k], d.cn = cnoise[k], d.sg = sigma[k];
    return d;
}

// x0 * sqrt(alpha_next) + c * pred_noise, pred_noise = m (eps) or (R * x - x0) / M; the division is IEEE.
__device__ __forceinline__ float ddim_mean(float x0, float x, float m, const DdimCoef& d, int mean_type) {
    float pn;
    if (mean_type == DSC_MEAN_EPS) pn = m;
    else { const float q0 = d.R * x; const float q1 = q0 - x0; pn = q1 / d.M; }
    const float u0 = x0 * d.an, u1 = d.cn * pn;
    return u0 + u1;
}

// The (a, s) of the re-noising that follows a step: row tv - 1 of the schedule, or times_next[k]; off after the last step.
struct Renoise { bool on; float a, s; };

__device__ __forceinline__ Renoise renoise_coef(bool on, int64_t row, const float* __restrict__ sa, const float* __restrict__ sb) {
    Renoise r;
    r.on = on;
    r.a = on ? sa[row] : 0.f, r.s = on ? sb[row] : 0.f;
    return r;
}

__global__ __launch_bounds__(256) void q_sample_kernel(const float* __restrict__ x0, const float* __restrict__ noise,
                                                      const int64_t* __restrict__ t, const float* __restrict__ sa,
                                                      const float* __restrict__ sb, float* __restrict__ xt,
                                                      float* __restrict__ vout, int64_t inner, int T) {
    const int b = blockIdx.y;
    const int64_t tv = dsc_checked_index(t[b], T, blockIdx.x == 0 && threadIdx.x == 0);      // one count per out-of-range scene
    const float a = sa[tv], s = sb[tv];
    const int64_t base = (int64_t)b * inner;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < inner; i += (int64_t)gridDim.x * blockDim.x) {
        const float x = x0[base + i], n = noise[base + i];
        xt[base + i] = renoise(x, n, a, s);
        if (vout) {
            const float q0 = a * n, q1 = s * x;
            vout[base + i] = q0 - q1;
        }
    }
}

__global__ __launch_bounds__(256) void p_sample_kernel(const float* xt, const float* __restrict__ mo,
                                                      const float* __restrict__ noise, const int64_t* __restrict__ t,
                                                      const float* __restrict__ ca, const float* __restrict__ cb,
                                                      const float* __restrict__ c1, const float* __restrict__ c2,
                                                      const float* __restrict__ sigma, float* out,   // out may alias xt (in-place step)
                                                      float* __restrict__ x0_out, int mean_type, int clip, int64_t inner, int T) {
    const int b = blockIdx.y;
    const int64_t tv = dsc_checked_index(t[b], T, blockIdx.x == 0 && threadIdx.x == 0);      // one count per out-of-range scene
    const PosteriorCoef p = posterior_coef(tv, ca, cb, c1, c2, sigma, mean_type, true);
    const int64_t base = (int64_t)b * inner;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < inner; i += (int64_t)gridDim.x * blockDim.x) {
        const float x = xt[base + i], m = mo[base + i];
        const float x0 = predict_x0(x, m, p.A, p.Bc, mean_type, clip);
        out[base + i] = add_noise(posterior_mean(x0, x, p), noise[base + i], p.sg);
        if (x0_out) x0_out[base + i] = x0;
    }
}

__global__ void add_scalar_i64_kernel(int64_t* t, int count, int64_t delta) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) t[i] += delta;
}

// One DDIM step (ddim_sample_loop, diffusion_ddpm.py:402-444, x_start / pred_noise as model_predictions(clip_x_start=True,
// rederive_pred_noise=False), :242-264).  Every scene is at the same step: the step index k comes from a device counter and the
// per-step scalars from device tables of S rows (t, t_next, sqrt(alpha_next), c, sigma), so the launch can be captured once and
// replayed.  x_start is always clamped to [-1, 1] (the reference ignores clip_denoised here).  t_next < 0 (the last pair): out = x_start
// and the noise is not read.  Each product and sum is rounded on its own, and the division is IEEE (no fast-math): bit-identical
// to the reference's fp32 expressions.
__global__ __launch_bounds__(256) void ddim_step_kernel(const float* xt, const float* __restrict__ mo, const float* __restrict__ noise,
                                                       const int64_t* __restrict__ step, const int64_t* __restrict__ times,
                                                       const int64_t* __restrict__ times_next, const float* __restrict__ sqrt_an,
                                                       const float* __restrict__ cnoise, const float* __restrict__ sigma,
                                                       const float* __restrict__ ca, const float* __restrict__ cb,
                                                       const float* __restrict__ ra, const float* __restrict__ rm,
                                                       float* out,   // out may alias xt (in-place step)
                                                       float* __restrict__ x0_out, int mean_type, int64_t inner, int S, int T) {
    const int b = blockIdx.y;
    const bool first = blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0;               // one count per launch
    const DdimCoef d = ddim_coef(step, times, times_next, sqrt_an, cnoise, sigma, ca, cb, ra, rm, mean_type, S, T, first, false);
    const int64_t base = (int64_t)b * inner;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < inner; i += (int64_t)gridDim.x * blockDim.x) {
        const float x = xt[base + i], m = mo[base + i];
        const float x0 = predict_x0(x, m, d.A, d.Bc, mean_type, true);
        if (x0_out) x0_out[base + i] = x0;
        if (d.last) { out[base + i] = x0; continue; }
        out[base + i] = add_noise(ddim_mean(x0, x, m, d, mean_type), noise[base + i], d.sg);
    }
}

// Advance of the captured DDIM loop: step += 1, then t[i] = times[step] for the next model call.  One block: every thread reads the
// counter before thread 0 stores it.
__global__ __launch_bounds__(256) void ddim_advance_kernel(int64_t* step, const int64_t* __restrict__ times, int64_t* __restrict__ t,
                                                          int count, int S) {
    const int64_t k = step[0] + 1;
    __syncthreads();
    if (threadIdx.x == 0) step[0] = k;
    const int64_t tv = times[dsc_checked_index(k, S, threadIdx.x == 0)];
    for (int i = threadIdx.x; i < count; i += blockDim.x) t[i] = tv;
}

__global__ __launch_bounds__(256) void complete_overwrite_kernel(float* __restrict__ x, const float* __restrict__ partial,
                                                                const float* __restrict__ noise,
                                                                const int64_t* __restrict__ t, const float* __restrict__ sa,
                                                                const float* __restrict__ sb, int n, int p, int c, int T) {
    const int b = blockIdx.y;
    const int64_t tv = dsc_checked_index(t[b], T, blockIdx.x == 0 && threadIdx.x == 0);      // one count per out-of-range scene
    const float a = sa[tv], s = sb[tv];
    const int64_t cnt = (int64_t)p * c;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * blockDim.x) {
        x[(int64_t)b * n * c + i] = renoise(partial[(int64_t)b * cnt + i], noise[(int64_t)b * cnt + i], a, s);   // rows [0,p) of scene b are the first p*c elements
    }
}

// complete_overwrite_kernel with a per-scene row count: scene b writes rows [0, counts[b]) of x (n rows), reading rows of partial /
// noise (pmax rows per scene; rows >= counts[b] are padding and never read).  counts[b] is clamped into [0, pmax] and an
// out-of-range value counted like a bad timestep.  The grid covers pmax rows; a scene with count 0 writes nothing.
__global__ __launch_bounds__(256) void complete_overwrite_ragged_kernel(float* __restrict__ x, const float* __restrict__ partial,
                                                                       const float* __restrict__ noise,
                                                                       const int64_t* __restrict__ counts,
                                                                       const int64_t* __restrict__ t, const float* __restrict__ sa,
                                                                       const float* __restrict__ sb, int n, int pmax, int c, int T) {
    const int b = blockIdx.y;
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    const int64_t tv = dsc_checked_index(t[b], T, first);
    const int64_t cnt = dsc_checked_index(counts[b], (int64_t)pmax + 1, first) * c;
    const float a = sa[tv], s = sb[tv];
    const int64_t pbase = (int64_t)b * pmax * c;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * blockDim.x) {
        x[(int64_t)b * n * c + i] = renoise(partial[pbase + i], noise[pbase + i], a, s);   // rows [0,count) of scene b are its first count*c elements
    }
}

// Fused step of the ragged completion loop: p_sample_kernel on rows >= counts[b]; rows < counts[b] (the given objects, whose
// posterior step the next overwrite would discard) get what the loop writes there next -- q_sample(partial, t - 1, noise_p) when
// t > 0 (the overwrite that precedes the next model call), partial itself when t == 0 (the final restore; noise_p is not read).
// Same expressions, same rounding as p_sample_kernel and complete_overwrite_kernel: bit-identical to their composition.
__global__ __launch_bounds__(256) void p_sample_inpaint_kernel(const float* xt, const float* __restrict__ mo,
                                                              const float* __restrict__ noise, const float* __restrict__ partial,
                                                              const float* __restrict__ noise_p,
                                                              const int64_t* __restrict__ counts, const int64_t* __restrict__ t,
                                                              const float* __restrict__ ca, const float* __restrict__ cb,
                                                              const float* __restrict__ c1, const float* __restrict__ c2,
                                                              const float* __restrict__ sigma, const float* __restrict__ sa,
                                                              const float* __restrict__ sb, float* out,   // out may alias xt
                                                              int mean_type, int clip, int n, int pmax, int c, int T) {
    const int b = blockIdx.y;
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    const int64_t tv = dsc_checked_index(t[b], T, first);
    const int64_t cnt = dsc_checked_index(counts[b], (int64_t)pmax + 1, first) * c;
    const PosteriorCoef p = posterior_coef(tv, ca, cb, c1, c2, sigma, mean_type, true);
    const Renoise r = renoise_coef(tv > 0, tv - 1, sa, sb);
    const int64_t inner = (int64_t)n * c;
    const int64_t base = (int64_t)b * inner, pbase = (int64_t)b * pmax * c;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < inner; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < cnt) {
            const float pv = partial[pbase + i];
            out[base + i] = r.on ? renoise(pv, noise_p[pbase + i], r.a, r.s) : pv;
            continue;
        }
        const float x = xt[base + i], m = mo[base + i];
        out[base + i] = add_noise(posterior_mean(predict_x0(x, m, p.A, p.Bc, mean_type, clip), x, p), noise[base + i], p.sg);
    }
}

// Fused step of the strided (DDIM) ragged completion loop: ddim_step_kernel on rows >= counts[b]; rows < counts[b] (the given
// objects, whose update the next overwrite would discard) get what the loop writes there next -- q_sample(partial, t_next, noise_p)
// when t_next >= 0 (the overwrite that precedes the next model call), partial itself on the last pair (the final restore; neither
// noise nor noise_p is read there).  Same expressions, same rounding as ddim_step_kernel and complete_overwrite_ragged_kernel:
// bit-identical to their composition.
__global__ __launch_bounds__(256) void ddim_inpaint_step_kernel(const float* xt, const float* __restrict__ mo,
                                                               const float* __restrict__ noise, const float* __restrict__ partial,
                                                               const float* __restrict__ noise_p,
                                                               const int64_t* __restrict__ counts, const int64_t* __restrict__ step,
                                                               const int64_t* __restrict__ times, const int64_t* __restrict__ times_next,
                                                               const float* __restrict__ sqrt_an, const float* __restrict__ cnoise,
                                                               const float* __restrict__ sigma, const float* __restrict__ ca,
                                                               const float* __restrict__ cb, const float* __restrict__ ra,
                                                               const float* __restrict__ rm, const float* __restrict__ sa,
                                                               const float* __restrict__ sb, float* out,   // out may alias xt
                                                               int mean_type, int n, int pmax, int c, int S, int T) {
    const int b = blockIdx.y;
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;                                  // one count per out-of-range scene
    const bool first_all = first && blockIdx.y == 0;                                         // one count per launch
    const DdimCoef d = ddim_coef(step, times, times_next, sqrt_an, cnoise, sigma, ca, cb, ra, rm, mean_type, S, T, first_all, true);
    const Renoise r = renoise_coef(!d.last, d.tn, sa, sb);
    const int64_t cnt = dsc_checked_index(counts[b], (int64_t)pmax + 1, first) * c;
    const int64_t inner = (int64_t)n * c;
    const int64_t base = (int64_t)b * inner, pbase = (int64_t)b * pmax * c;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < inner; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < cnt) {
            const float pv = partial[pbase + i];
            out[base + i] = r.on ? renoise(pv, noise_p[pbase + i], r.a, r.s) : pv;
            continue;
        }
        const float x = xt[base + i], m = mo[base + i];
        const float x0 = predict_x0(x, m, d.A, d.Bc, mean_type, true);
        if (d.last) { out[base + i] = x0; continue; }
        out[base + i] = add_noise(ddim_mean(x0, x, m, d, mean_type), noise[base + i], d.sg);
    }
}

// Element-wise in-painting (p_sample_loop_masked, ddim_masked_loop): the set of given elements is a (b, n, c) byte mask, any non-zero
// byte = given, instead of a row prefix.  known / noise / mask have x's shape.  Masked elements: x = sa[t] * known + sb[t] * noise;
// the others are neither read nor written.
__global__ __launch_bounds__(256) void masked_overwrite_kernel(float* __restrict__ x, const float* __restrict__ known,
                                                              const float* __restrict__ noise, const uint8_t* __restrict__ mask,
                                                              const int64_t* __restrict__ t, const float* __restrict__ sa,
                                                              const float* __restrict__ sb, int64_t inner, int T) {
    const int b = blockIdx.y;
    const int64_t tv = dsc_checked_index(t[b], T, blockIdx.x == 0 && threadIdx.x == 0);      // one count per out-of-range scene
    const float a = sa[tv], s = sb[tv];
    const int64_t base = (int64_t)b * inner;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < inner; i += (int64_t)gridDim.x * blockDim.x) {
        if (!mask[base + i]) continue;
        x[base + i] = renoise(known[base + i], noise[base + i], a, s);
    }
}

// Fused step of the masked loop: p_sample_kernel on the free elements; a given element (whose posterior step the next overwrite
// would discard) gets what the loop writes there next -- q_sample(known, t - 1, noise_k) when t > 0, known itself when t == 0 (the
// final select; noise_k is not read).  A given element reads mask, known and noise_k only; a free one mask, xt, mo and noise only:
// an all-free launch moves p_sample_kernel's bytes plus one byte per element.  Same expressions, same rounding as p_sample_kernel and
// masked_overwrite_kernel: bit-identical to their composition.
__global__ __launch_bounds__(256) void p_sample_masked_kernel(const float* xt, const float* __restrict__ mo,
                                                             const float* __restrict__ noise, const float* __restrict__ known,
                                                             const float* __restrict__ noise_k, const uint8_t* __restrict__ mask,
                                                             const int64_t* __restrict__ t,
                                                             const float* __restrict__ ca, const float* __restrict__ cb,
                                                             const float* __restrict__ c1, const float* __restrict__ c2,
                                                             const float* __restrict__ sigma, const float* __restrict__ sa,
                                                             const float* __restrict__ sb, float* out,   // out may alias xt
                                                             int mean_type, int clip, int64_t inner, int T) {
    const int b = blockIdx.y;
    const int64_t tv = dsc_checked_index(t[b], T, blockIdx.x == 0 && threadIdx.x == 0);      // one count per out-of-range scene
    const PosteriorCoef p = posterior_coef(tv, ca, cb, c1, c2, sigma, mean_type, true);
    const Renoise r = renoise_coef(tv > 0, tv - 1, sa, sb);
    const int64_t base = (int64_t)b * inner;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < inner; i += (int64_t)gridDim.x * blockDim.x) {
        if (mask[base + i]) {
            const float kv = known[base + i];
            out[base + i] = r.on ? renoise(kv, noise_k[base + i], r.a, r.s) : kv;
            continue;
        }
        const float x = xt[base + i], m = mo[base + i];
        out[base + i] = add_noise(posterior_mean(predict_x0(x, m, p.A, p.Bc, mean_type, clip), x, p), noise[base + i], p.sg);
    }
}

// Fused step of the strided (DDIM) masked loop: ddim_step_kernel on the free elements; a given element gets q_sample(known, t_next,
// noise_k) when t_next >= 0, known itself on the last pair (neither noise nor noise_k is read there).  Reads per element as
// p_sample_masked_kernel; index checks as ddim_inpaint_step_kernel.  Bit-identical to ddim_step_kernel followed by
// masked_overwrite_kernel at t_next (or by the final select).
__global__ __launch_bounds__(256) void ddim_masked_step_kernel(const float* xt, const float* __restrict__ mo,
                                                              const float* __restrict__ noise, const float* __restrict__ known,
                                                              const float* __restrict__ noise_k, const uint8_t* __restrict__ mask,
                                                              const int64_t* __restrict__ step,
                                                              const int64_t* __restrict__ times, const int64_t* __restrict__ times_next,
                                                              const float* __restrict__ sqrt_an, const float* __restrict__ cnoise,
                                                              const float* __restrict__ sigma, const float* __restrict__ ca,
                                                              const float* __restrict__ cb, const float* __restrict__ ra,
                                                              const float* __restrict__ rm, const float* __restrict__ sa,
                                                              const float* __restrict__ sb, float* out,   // out may alias xt
                                                              int mean_type, int64_t inner, int S, int T) {
    const int b = blockIdx.y;
    const bool first_all = blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0;           // one count per launch
    const DdimCoef d = ddim_coef(step, times, times_next, sqrt_an, cnoise, sigma, ca, cb, ra, rm, mean_type, S, T, first_all, true);
    const Renoise r = renoise_coef(!d.last, d.tn, sa, sb);
    const int64_t base = (int64_t)b * inner;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < inner; i += (int64_t)gridDim.x * blockDim.x) {
        if (mask[base + i]) {
            const float kv = known[base + i];
            out[base + i] = r.on ? renoise(kv, noise_k[base + i], r.a, r.s) : kv;
            continue;
        }
        const float x = xt[base + i], m = mo[base + i];
        const float x0 = predict_x0(x, m, d.A, d.Bc, mean_type, true);
        if (d.last) { out[base + i] = x0; continue; }
        out[base + i] = add_noise(ddim_mean(x0, x, m, d, mean_type), noise[base + i], d.sg);
    }
}

// Classifier-free guidance (p_sample_loop_guided / ddim_guided_loop).  model_out holds 2 b scenes: rows [0, b) are the denoiser on the
// text features (c), rows [b, 2 b) the denoiser on the null condition (u), both on the same x_t.  Scene i is guided with its own
// scale w = scale[i], read through a pointer:  m = u + w * (c - u), the difference, the product and the sum each rounded on its own.
// w == 0 gives u + 0 * (c - u) = u, w == 1 the conditional output up to rounding.
__device__ __forceinline__ float cfg_mix(float c, float u, float w) {
    const float d = c - u;
    const float p = w * d;
    return u + p;
}

// The unfused form: m (b, inner) from model_out (2 b, inner) and scale (b,).
__global__ __launch_bounds__(256) void cfg_combine_kernel(const float* __restrict__ mo, const float* __restrict__ scale,
                                                         float* __restrict__ out, int64_t inner) {
    const int b = blockIdx.y;
    const float w = scale[b];
    const int64_t base = (int64_t)b * inner, half = (int64_t)gridDim.y * inner;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < inner; i += (int64_t)gridDim.x * blockDim.x)
        out[base + i] = cfg_mix(mo[base + i], mo[half + base + i], w);
}

// p_sample_kernel with m computed in registers from the two halves of mo.  x_dup (may be NULL): a second copy of the new x, so that a
// captured loop can keep x as one (2 b, inner) buffer with both halves current.  At t == 0 the noise is not read (p_sample_kernel
// adds 0 * noise there).  Same expressions, same rounding as cfg_combine_kernel followed by p_sample_kernel: equal to their composition
// on finite noise (torch.equal; the sign of a zero result may differ at t == 0).
__global__ __launch_bounds__(256) void p_sample_cfg_kernel(const float* xt, const float* __restrict__ mo, const float* __restrict__ scale,
                                                          const float* __restrict__ noise, const int64_t* __restrict__ t,
                                                          const float* __restrict__ ca, const float* __restrict__ cb,
                                                          const float* __restrict__ c1, const float* __restrict__ c2,
                                                          const float* __restrict__ sigma, float* out,   // out may alias xt
                                                          float* __restrict__ x_dup, float* __restrict__ x0_out, int mean_type, int clip,
                                                          int64_t inner, int T) {
    const int b = blockIdx.y;
    const int64_t tv = dsc_checked_index(t[b], T, blockIdx.x == 0 && threadIdx.x == 0);      // one count per out-of-range scene
    const PosteriorCoef p = posterior_coef(tv, ca, cb, c1, c2, sigma, mean_type, false);
    const float w = scale[b];
    const int64_t base = (int64_t)b * inner, half = (int64_t)gridDim.y * inner;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < inner; i += (int64_t)gridDim.x * blockDim.x) {
        const float x = xt[base + i], m = cfg_mix(mo[base + i], mo[half + base + i], w);
        const float x0 = predict_x0(x, m, p.A, p.Bc, mean_type, clip);
        float y = posterior_mean(x0, x, p);       // t == 0: sigma is forced to 0 and the noise is not read
        if (tv != 0) y = add_noise(y, noise[base + i], p.sg);
        out[base + i] = y;
        if (x_dup) x_dup[base + i] = y;
        if (x0_out) x0_out[base + i] = x0;
    }
}

// ddim_step_kernel with m computed in registers from the two halves of mo; x_dup as in p_sample_cfg_kernel.  On the last pair the
// noise is not read.  Bit-identical to cfg_combine_kernel followed by ddim_step_kernel.
__global__ __launch_bounds__(256) void ddim_cfg_step_kernel(const float* xt, const float* __restrict__ mo, const float* __restrict__ scale,
                                                           const float* __restrict__ noise, const int64_t* __restrict__ step,
                                                           const int64_t* __restrict__ times, const int64_t* __restrict__ times_next,
                                                           const float* __restrict__ sqrt_an, const float* __restrict__ cnoise,
                                                           const float* __restrict__ sigma, const float* __restrict__ ca,
                                                           const float* __restrict__ cb, const float* __restrict__ ra,
                                                           const float* __restrict__ rm, float* out,   // out may alias xt
                                                           float* __restrict__ x_dup, float* __restrict__ x0_out, int mean_type,
                                                           int64_t inner, int S, int T) {
    const int b = blockIdx.y;
    const bool first = blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0;               // one count per launch
    const DdimCoef d = ddim_coef(step, times, times_next, sqrt_an, cnoise, sigma, ca, cb, ra, rm, mean_type, S, T, first, false);
    const float w = scale[b];
    const int64_t base = (int64_t)b * inner, half = (int64_t)gridDim.y * inner;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < inner; i += (int64_t)gridDim.x * blockDim.x) {
        const float x = xt[base + i], m = cfg_mix(mo[base + i], mo[half + base + i], w);
        const float x0 = predict_x0(x, m, d.A, d.Bc, mean_type, true);
        if (x0_out) x0_out[base + i] = x0;
        float y = x0;
        if (!d.last) y = add_noise(ddim_mean(x0, x, m, d, mean_type), noise[base + i], d.sg);
        out[base + i] = y;
        if (x_dup) x_dup[base + i] = y;
    }
}

// Guided in-painting (p_sample_loop_masked_guided): p_sample_masked_kernel with m computed in registers from the two halves of mo
// (2 b, inner); known / noise_k / mask stay (b, inner).  x_dup as in p_sample_cfg_kernel: every written element, given or free, goes
// there too.  A given element reads mask, known and noise_k only (no noise_k at t == 0); a free one mask, xt, both halves of mo and
// noise only.  Bit-identical to cfg_combine_kernel followed by p_sample_masked_kernel.
__global__ __launch_bounds__(256) void p_sample_masked_cfg_kernel(const float* xt, const float* __restrict__ mo,
                                                                 const float* __restrict__ scale, const float* __restrict__ noise,
                                                                 const float* __restrict__ known, const float* __restrict__ noise_k,
                                                                 const uint8_t* __restrict__ mask, const int64_t* __restrict__ t,
                                                                 const float* __restrict__ ca, const float* __restrict__ cb,
                                                                 const float* __restrict__ c1, const float* __restrict__ c2,
                                                                 const float* __restrict__ sigma, const float* __restrict__ sa,
                                                                 const float* __restrict__ sb, float* out,   // out may alias xt
                                                                 float* __restrict__ x_dup, int mean_type, int clip, int64_t inner,
                                                                 int T) {
    const int b = blockIdx.y;
    const int64_t tv = dsc_checked_index(t[b], T, blockIdx.x == 0 && threadIdx.x == 0);      // one count per out-of-range scene
    const PosteriorCoef p = posterior_coef(tv, ca, cb, c1, c2, sigma, mean_type, true);
    const Renoise r = renoise_coef(tv > 0, tv - 1, sa, sb);
    const float w = scale[b];
    const int64_t base = (int64_t)b * inner, half = (int64_t)gridDim.y * inner;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < inner; i += (int64_t)gridDim.x * blockDim.x) {
        float y;
        if (mask[base + i]) {
            const float kv = known[base + i];
            y = r.on ? renoise(kv, noise_k[base + i], r.a, r.s) : kv;
        } else {
            const float x = xt[base + i], m = cfg_mix(mo[base + i], mo[half + base + i], w);
            y = add_noise(posterior_mean(predict_x0(x, m, p.A, p.Bc, mean_type, clip), x, p), noise[base + i], p.sg);
        }
        out[base + i] = y;
        if (x_dup) x_dup[base + i] = y;
    }
}

// The strided twin (ddim_masked_guided_loop): ddim_masked_step_kernel with the same change and the same x_dup; index checks as there.
// On the last pair neither noise nor noise_k is read.  Bit-identical to cfg_combine_kernel followed by ddim_masked_step_kernel.
__global__ __launch_bounds__(256) void ddim_masked_cfg_step_kernel(const float* xt, const float* __restrict__ mo,
                                                                  const float* __restrict__ scale, const float* __restrict__ noise,
                                                                  const float* __restrict__ known, const float* __restrict__ noise_k,
                                                                  const uint8_t* __restrict__ mask, const int64_t* __restrict__ step,
                                                                  const int64_t* __restrict__ times,
                                                                  const int64_t* __restrict__ times_next,
                                                                  const float* __restrict__ sqrt_an, const float* __restrict__ cnoise,
                                                                  const float* __restrict__ sigma, const float* __restrict__ ca,
                                                                  const float* __restrict__ cb, const float* __restrict__ ra,
                                                                  const float* __restrict__ rm, const float* __restrict__ sa,
                                                                  const float* __restrict__ sb, float* out,   // out may alias xt
                                                                  float* __restrict__ x_dup, int mean_type, int64_t inner, int S,
                                                                  int T) {
    const int b = blockIdx.y;
    const bool first_all = blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0;           // one count per launch
    const DdimCoef d = ddim_coef(step, times, times_next, sqrt_an, cnoise, sigma, ca, cb, ra, rm, mean_type, S, T, first_all, true);
    const Renoise r = renoise_coef(!d.last, d.tn, sa, sb);
    const float w = scale[b];
    const int64_t base = (int64_t)b * inner, half = (int64_t)gridDim.y * inner;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < inner; i += (int64_t)gridDim.x * blockDim.x) {
        float y;
        if (mask[base + i]) {
            const float kv = known[base + i];
            y = r.on ? renoise(kv, noise_k[base + i], r.a, r.s) : kv;
        } else {
            const float x = xt[base + i], m = cfg_mix(mo[base + i], mo[half + base + i], w);
            y = predict_x0(x, m, d.A, d.Bc, mean_type, true);
            if (!d.last) y = add_noise(ddim_mean(y, x, m, d, mean_type), noise[base + i], d.sg);
        }
        out[base + i] = y;
        if (x_dup) x_dup[base + i] = y;
    }
}

// Per-scene gate of the text-condition dropout (text_drop_prob): y[b, :] = keep[b] ? x[b, :] : 0 -- a select, a dropped scene's x is
// not read.  Forward on the text features, backward on their incoming gradient.  y may alias x.
__global__ __launch_bounds__(256) void scene_gate_kernel(const float* x, const uint8_t* __restrict__ keep, float* y, int64_t inner) {
    const int b = blockIdx.y;
    const bool k = keep[b] != 0;
    const int64_t base = (int64_t)b * inner;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < inner; i += (int64_t)gridDim.x * blockDim.x)
        y[base + i] = k ? x[base + i] : 0.0f;
}

// Post-filter of generated scenes (reference delete_empty_from_network_samples, diffusion_scene_layout_ddpm.py:351-406): slot i
// of a scene is dropped when its 'empty' logit (column empty_col) is >= 0.  The reference takes that decision from BATCH ROW 0
// for every scene of the batch (:379, mode 0, kept as the drop-in default); mode 1 decides per scene, which is what batched
// generation needs.  One block per scene: keep flags -> exclusive prefix (ballot / popcount per wave, 3 waves cover N <= 192)
// -> kept rows move to the front in their original order, the tail is zero-filled, counts[b] = rows kept.
__global__ __launch_bounds__(192) void postfilter_compact_kernel(const float* __restrict__ x, int n, int c, int empty_col,
                                                                  int mode, int keep_empty, float* __restrict__ out,
                                                                  int* __restrict__ counts) {
    __shared__ int wave_cnt[3];
    __shared__ int dst[192];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* src_flags = x + (int64_t)(mode == 0 ? 0 : b) * n * c;
    const bool valid = tid < n;
    const bool keep = valid && (keep_empty || !(src_flags[(int64_t)tid * c + empty_col] >= 0.0f));
    const unsigned long long m = __ballot(keep);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += wave_cnt[w];
    const int total = wave_cnt[0] + wave_cnt[1] + wave_cnt[2];
    dst[tid] = keep ? base + before : -1;
    __syncthreads();
    const float* xs = x + (int64_t)b * n * c;
    float* os = out + (int64_t)b * n * c;
    for (int i = tid; i < n * c; i += 192) {
        const int r = i / c, col = i - r * c;
        const int d = dst[r];
        if (d >= 0) os[(int64_t)d * c + col] = xs[i];
    }
    for (int i = total * c + tid; i < n * c; i += 192) os[i] = 0.0f;
    if (tid == 0) counts[b] = total;
}

// Per-scene counter-based noise (include/diffuscene_hip.h, diffuscene_amd/scene_noise.py): Philox4x32-10 on the counter
// (q, stream, draw lo, draw hi) under the key (seed lo, seed hi), q the scene's own quad index -- nothing of the batch enters.
struct Quad { uint32_t r[4]; };

__device__ __forceinline__ Quad philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0, c1 = lo1, c2 = hi0 ^ c3 ^ k1, c3 = lo0;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    return Quad{{c0, c1, c2, c3}};
}

// u = (r >> 8) * 2^-24 + 2^-25: the product is exact, the sum is rounded to nearest even above 1/2 (there u needs 25 bits), so u lies
// in (0, 1] and u == 1 gives rho == 0, never an infinity.
__device__ __forceinline__ float unit_open(uint32_t r) {
    const float p = (float)(r >> 8) * 5.9604644775390625e-08f;
    return p + 2.98023223876953125e-08f;
}

// Box-Muller on one pair of words, full-precision logf / sinf / cosf; every product a statement of its own.
__device__ __forceinline__ void box_muller(uint32_t ra, uint32_t rb, float& z0, float& z1) {
    const float l = logf(unit_open(ra));
    const float m = -2.0f * l;
    const float rho = sqrtf(m);
    const float theta = 6.2831853071795864769f * unit_open(rb);
    const float c = cosf(theta), s = sinf(theta);
    z0 = rho * c;
    z1 = rho * s;
}

__device__ __forceinline__ void store_word(float* p, uint32_t r, float z) { *p = z; }
__device__ __forceinline__ void store_word(uint32_t* p, uint32_t r, float z) { *p = r; }

// One thread per Philox block = four consecutive elements of one scene; the grid is flat over B * quads (I: the index type, 32 bits
// where the count fits).  VEC4 (per_scene % 4 == 0 and a 16-byte-aligned out): every scene base is 16-byte aligned and a lane stores its
// quad as one dwordx4, lane i at base + 16 i -- the coalesced form.  Otherwise a scene's base is odd and a lane stores its live elements
// as dwords: the four stores of a wave interleave inside the same 1 KiB span, so every cache line they touch is completed by that wave.
// T = float: the normals; T = uint32_t: the raw words (the host-side probe).  *draw is read, never written.
template <typename T, typename I, bool VEC4>
__global__ __launch_bounds__(256) void scene_noise_kernel(T* __restrict__ out, const int64_t* __restrict__ seeds,
                                                          const int64_t* __restrict__ draw, uint32_t stream, I total, I quads,
                                                          int64_t per_scene) {
    const I idx = (I)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const I b = idx / quads, q = idx - b * quads;
    const uint64_t seed = (uint64_t)seeds[b], d = (uint64_t)draw[0];
    const Quad w = philox4x32_10((uint32_t)q, stream, (uint32_t)d, (uint32_t)(d >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (std::is_same<T, float>::value) {
        box_muller(w.r[0], w.r[1], z[0], z[1]);
        box_muller(w.r[2], w.r[3], z[2], z[3]);
    }
    const int64_t e = (int64_t)q * 4;
    T* o = out + (int64_t)b * per_scene + e;
    if constexpr (VEC4) {
        if constexpr (std::is_same<T, float>::value) *reinterpret_cast<float4*>(o) = make_float4(z[0], z[1], z[2], z[3]);
        else *reinterpret_cast<uint4*>(o) = make_uint4(w.r[0], w.r[1], w.r[2], w.r[3]);
    } else {
        const int64_t left = per_scene - e;
        const int live = left < 4 ? (int)left : 4;      // the last quad of a scene: per_scene & 3 live lanes
#pragma unroll
        for (int lane = 0; lane < 4; ++lane)
            if (lane < live) store_word(o + lane, w.r[lane], z[lane]);
    }
}

template <typename T>
int launch_scene_noise(T* out, const int64_t* seeds, const int64_t* draw, int64_t stream, int64_t B, int64_t per_scene,
                       dsc_stream_t hip_stream) {
    if (!out || !seeds || !draw || stream < 0 || stream > 0xffffffffll || B < 0 || per_scene < 0) return DSC_EINVAL;
    if (B == 0 || per_scene == 0) return 0;
    if (per_scene > (1ll << 32)) return DSC_ERANGE;
    const int64_t quads = (per_scene + 3) / 4;                          // <= 2^30
    if (B > (((1ll << 31) - 1) * 256) / quads) return DSC_ERANGE;       // the flat grid: fewer than 2^31 blocks of 256
    const int64_t total = B * quads;
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    const hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const bool vec4 = per_scene % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    const uint32_t st = (uint32_t)stream;
    DSC_CLEAR_STALE_ERROR();
    if (total <= 0xffffff00ll) {                                        // no 32-bit index of the last block wraps
        const uint32_t t32 = (uint32_t)total, q32 = (uint32_t)quads;
        if (vec4) hipLaunchKernelGGL((scene_noise_kernel<T, uint32_t, true>), grid, block, 0, s, out, seeds, draw, st, t32, q32, per_scene);
        else hipLaunchKernelGGL((scene_noise_kernel<T, uint32_t, false>), grid, block, 0, s, out, seeds, draw, st, t32, q32, per_scene);
    } else {
        if (vec4) hipLaunchKernelGGL((scene_noise_kernel<T, int64_t, true>), grid, block, 0, s, out, seeds, draw, st, total, quads, per_scene);
        else hipLaunchKernelGGL((scene_noise_kernel<T, int64_t, false>), grid, block, 0, s, out, seeds, draw, st, total, quads, per_scene);
    }
    DSC_LAUNCH_CHECK();
    return 0;
}

// ca / cb are read for every mean type but x0.
inline bool bad_mean_args(int32_t mean_type, const float* ca, const float* cb) {
    return mean_type < DSC_MEAN_EPS || mean_type > DSC_MEAN_V || (mean_type != DSC_MEAN_X0 && (!ca || !cb));
}

inline unsigned grid_x(int64_t inner) {
    int64_t g = (inner + 255) / 256;
    return (unsigned)(g > 64 ? 64 : g);
}

}  // namespace

extern "C" int dsc_q_sample_f32(const float* x0, const float* noise, const int64_t* t, const float* sqrt_ac,
                                const float* sqrt_1mac, float* x_t, float* v_out, int32_t b, int64_t inner,
                                int32_t num_timesteps, dsc_stream_t stream) {
    if (!x0 || !noise || !t || !sqrt_ac || !sqrt_1mac || !x_t || b < 1 || inner < 1 || num_timesteps < 1) return DSC_EINVAL;
    DSC_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL(q_sample_kernel, dim3(grid_x(inner), b), dim3(256), 0, static_cast<hipStream_t>(stream),
                       x0, noise, t, sqrt_ac, sqrt_1mac, x_t, v_out, inner, num_timesteps);
    DSC_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsc_p_sample_f32(const float* x_t, const float* model_out, const float* noise, const int64_t* t,
                                const float* ca, const float* cb, const float* coef1, const float* coef2,
                                const float* sigma, float* out, float* x0_out, int32_t mean_type, int32_t clip,
                                int32_t b, int64_t inner, int32_t num_timesteps, dsc_stream_t stream) {
    if (!x_t || !model_out || !noise || !t || !coef1 || !coef2 || !sigma || !out || b < 1 || inner < 1 || num_timesteps < 1)
        return DSC_EINVAL;
    if (bad_mean_args(mean_type, ca, cb)) return DSC_EINVAL;
    DSC_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL(p_sample_kernel, dim3(grid_x(inner), b), dim3(256), 0, static_cast<hipStream_t>(stream),
                       x_t, model_out, noise, t, ca, cb, coef1, coef2, sigma, out, x0_out, mean_type, clip, inner, num_timesteps);
    DSC_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsc_add_scalar_i64(int64_t* t, int32_t count, int64_t delta, dsc_stream_t stream) {
    if (!t || count < 1) return DSC_EINVAL;
    DSC_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL(add_scalar_i64_kernel, dim3((count + 255) / 256), dim3(256), 0,
                       static_cast<hipStream_t>(stream), t, count, delta);
    DSC_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsc_ddim_step_f32(const float* x_t, const float* model_out, const float* noise, const int64_t* step,
                                 const int64_t* times, const int64_t* times_next, const float* sqrt_alpha_next,
                                 const float* c_noise, const float* sigma, const float* ca, const float* cb,
                                 const float* sqrt_recip_ac, const float* sqrt_recipm1_ac, float* out, float* x0_out,
                                 int32_t mean_type, int32_t b, int64_t inner, int32_t num_steps, int32_t num_timesteps,
                                 dsc_stream_t stream) {
    if (!x_t || !model_out || !noise || !step || !times || !times_next || !sqrt_alpha_next || !c_noise || !sigma ||
        !sqrt_recip_ac || !sqrt_recipm1_ac || !out || b < 1 || inner < 1 || num_steps < 1 || num_timesteps < 1)
        return DSC_EINVAL;
    if (bad_mean_args(mean_type, ca, cb)) return DSC_EINVAL;
    if (b > 65535) return DSC_ERANGE;
    DSC_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL(ddim_step_kernel, dim3(grid_x(inner), b), dim3(256), 0, static_cast<hipStream_t>(stream),
                       x_t, model_out, noise, step, times, times_next, sqrt_alpha_next, c_noise, sigma, ca, cb,
                       sqrt_recip_ac, sqrt_recipm1_ac, out, x0_out, mean_type, inner, num_steps, num_timesteps);
    DSC_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsc_ddim_advance_i64(int64_t* step, const int64_t* times, int64_t* t, int32_t count, int32_t num_steps,
                                    dsc_stream_t stream) {
    if (!step || !times || !t || count < 1 || num_steps < 1) return DSC_EINVAL;
    DSC_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL(ddim_advance_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), step, times, t, count,
                       num_steps);
    DSC_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsc_postfilter_compact_f32(const float* samples, int32_t b, int32_t n, int32_t c, int32_t empty_col,
                                          int32_t mode, int32_t keep_empty, float* packed, int32_t* counts,
                                          dsc_stream_t stream) {
    if (!samples || !packed || !counts || b < 1 || n < 1 || c < 1 || empty_col < 0 || empty_col >= c) return DSC_EINVAL;
    if (mode < 0 || mode > 1 || samples == packed) return DSC_EINVAL;
    if (n > 192) return DSC_ERANGE;
    DSC_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL(postfilter_compact_kernel, dim3(b), dim3(192), 0, static_cast<hipStream_t>(stream), samples, n, c,
                       empty_col, mode, keep_empty, packed, counts);
    DSC_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsc_complete_overwrite_f32(float* x, const float* partial, const float* noise, const int64_t* t,
                                          const float* sqrt_ac, const float* sqrt_1mac, int32_t b, int32_t n,
                                          int32_t p, int32_t c, int32_t num_timesteps, dsc_stream_t stream) {
    if (!x || !partial || !noise || !t || !sqrt_ac || !sqrt_1mac || b < 1 || n < 1 || p < 1 || p > n || c < 1 || num_timesteps < 1)
        return DSC_EINVAL;
    DSC_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL(complete_overwrite_kernel, dim3(grid_x((int64_t)p * c), b), dim3(256), 0,
                       static_cast<hipStream_t>(stream), x, partial, noise, t, sqrt_ac, sqrt_1mac, n, p, c, num_timesteps);
    DSC_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsc_complete_overwrite_ragged_f32(float* x, const float* partial, const float* noise, const int64_t* counts,
                                                 const int64_t* t, const float* sqrt_ac, const float* sqrt_1mac, int32_t b,
                                                 int32_t n, int32_t pmax, int32_t c, int32_t num_timesteps, dsc_stream_t stream) {
    if (!x || !partial || !noise || !counts || !t || !sqrt_ac || !sqrt_1mac || b < 1 || n < 1 || pmax < 1 || pmax > n || c < 1 ||
        num_timesteps < 1)
        return DSC_EINVAL;
    if (b > 65535) return DSC_ERANGE;
    DSC_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL(complete_overwrite_ragged_kernel, dim3(grid_x((int64_t)pmax * c), b), dim3(256), 0,
                       static_cast<hipStream_t>(stream), x, partial, noise, counts, t, sqrt_ac, sqrt_1mac, n, pmax, c, num_timesteps);
    DSC_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsc_p_sample_inpaint_f32(const float* x_t, const float* model_out, const float* noise, const float* partial,
                                        const float* noise_p, const int64_t* counts, const int64_t* t, const float* ca,
                                        const float* cb, const float* coef1, const float* coef2, const float* sigma,
                                        const float* sqrt_ac, const float* sqrt_1mac, float* out, int32_t mean_type, int32_t clip,
                                        int32_t b, int32_t n, int32_t pmax, int32_t c, int32_t num_timesteps, dsc_stream_t stream) {
    if (!x_t || !model_out || !noise || !partial || !noise_p || !counts || !t || !coef1 || !coef2 || !sigma || !sqrt_ac || !sqrt_1mac ||
        !out || b < 1 || n < 1 || pmax < 1 || pmax > n || c < 1 || num_timesteps < 1)
        return DSC_EINVAL;
    if (bad_mean_args(mean_type, ca, cb)) return DSC_EINVAL;
    if (b > 65535) return DSC_ERANGE;
    DSC_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL(p_sample_inpaint_kernel, dim3(grid_x((int64_t)n * c), b), dim3(256), 0, static_cast<hipStream_t>(stream),
                       x_t, model_out, noise, partial, noise_p, counts, t, ca, cb, coef1, coef2, sigma, sqrt_ac, sqrt_1mac, out,
                       mean_type, clip, n, pmax, c, num_timesteps);
    DSC_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsc_ddim_inpaint_step_f32(const float* x_t, const float* model_out, const float* noise, const float* partial,
                                         const float* noise_p, const int64_t* counts, const int64_t* step, const int64_t* times,
                                         const int64_t* times_next, const float* sqrt_alpha_next, const float* c_noise,
                                         const float* sigma, const float* ca, const float* cb, const float* sqrt_recip_ac,
                                         const float* sqrt_recipm1_ac, const float* sqrt_ac, const float* sqrt_1mac, float* out,
                                         int32_t mean_type, int32_t b, int32_t n, int32_t pmax, int32_t c, int32_t num_steps,
                                         int32_t num_timesteps, dsc_stream_t stream) {
    if (!x_t || !model_out || !noise || !partial || !noise_p || !counts || !step || !times || !times_next || !sqrt_alpha_next ||
        !c_noise || !sigma || !sqrt_recip_ac || !sqrt_recipm1_ac || !sqrt_ac || !sqrt_1mac || !out || b < 1 || n < 1 || pmax < 1 ||
        pmax > n || c < 1 || num_steps < 1 || num_timesteps < 1)
        return DSC_EINVAL;
    if (bad_mean_args(mean_type, ca, cb)) return DSC_EINVAL;
    if (b > 65535) return DSC_ERANGE;
    DSC_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL(ddim_inpaint_step_kernel, dim3(grid_x((int64_t)n * c), b), dim3(256), 0, static_cast<hipStream_t>(stream),
                       x_t, model_out, noise, partial, noise_p, counts, step, times, times_next, sqrt_alpha_next, c_noise, sigma, ca,
                       cb, sqrt_recip_ac, sqrt_recipm1_ac, sqrt_ac, sqrt_1mac, out, mean_type, n, pmax, c, num_steps, num_timesteps);
    DSC_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsc_masked_overwrite_f32(float* x, const float* known, const float* noise, const uint8_t* mask, const int64_t* t,
                                        const float* sqrt_ac, const float* sqrt_1mac, int32_t b, int64_t inner,
                                        int32_t num_timesteps, dsc_stream_t stream) {
    if (!x || !known || !noise || !mask || !t || !sqrt_ac || !sqrt_1mac || b < 1 || inner < 1 || num_timesteps < 1) return DSC_EINVAL;
    if (b > 65535) return DSC_ERANGE;
    DSC_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL(masked_overwrite_kernel, dim3(grid_x(inner), b), dim3(256), 0, static_cast<hipStream_t>(stream),
                       x, known, noise, mask, t, sqrt_ac, sqrt_1mac, inner, num_timesteps);
    DSC_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsc_p_sample_masked_f32(const float* x_t, const float* model_out, const float* noise, const float* known,
                                       const float* noise_k, const uint8_t* mask, const int64_t* t, const float* ca, const float* cb,
                                       const float* coef1, const float* coef2, const float* sigma, const float* sqrt_ac,
                                       const float* sqrt_1mac, float* out, int32_t mean_type, int32_t clip, int32_t b, int64_t inner,
                                       int32_t num_timesteps, dsc_stream_t stream) {
    if (!x_t || !model_out || !noise || !known || !noise_k || !mask || !t || !coef1 || !coef2 || !sigma || !sqrt_ac || !sqrt_1mac ||
        !out || b < 1 || inner < 1 || num_timesteps < 1)
        return DSC_EINVAL;
    if (bad_mean_args(mean_type, ca, cb)) return DSC_EINVAL;
    if (b > 65535) return DSC_ERANGE;
    DSC_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL(p_sample_masked_kernel, dim3(grid_x(inner), b), dim3(256), 0, static_cast<hipStream_t>(stream),
                       x_t, model_out, noise, known, noise_k, mask, t, ca, cb, coef1, coef2, sigma, sqrt_ac, sqrt_1mac, out,
                       mean_type, clip, inner, num_timesteps);
    DSC_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsc_ddim_masked_step_f32(const float* x_t, const float* model_out, const float* noise, const float* known,
                                        const float* noise_k, const uint8_t* mask, const int64_t* step, const int64_t* times,
                                        const int64_t* times_next, const float* sqrt_alpha_next, const float* c_noise,
                                        const float* sigma, const float* ca, const float* cb, const float* sqrt_recip_ac,
                                        const float* sqrt_recipm1_ac, const float* sqrt_ac, const float* sqrt_1mac, float* out,
                                        int32_t mean_type, int32_t b, int64_t inner, int32_t num_steps, int32_t num_timesteps,
                                        dsc_stream_t stream) {
    if (!x_t || !model_out || !noise || !known || !noise_k || !mask || !step || !times || !times_next || !sqrt_alpha_next ||
        !c_noise || !sigma || !sqrt_recip_ac || !sqrt_recipm1_ac || !sqrt_ac || !sqrt_1mac || !out || b < 1 || inner < 1 ||
        num_steps < 1 || num_timesteps < 1)
        return DSC_EINVAL;
    if (bad_mean_args(mean_type, ca, cb)) return DSC_EINVAL;
    if (b > 65535) return DSC_ERANGE;
    DSC_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL(ddim_masked_step_kernel, dim3(grid_x(inner), b), dim3(256), 0, static_cast<hipStream_t>(stream),
                       x_t, model_out, noise, known, noise_k, mask, step, times, times_next, sqrt_alpha_next, c_noise, sigma, ca,
                       cb, sqrt_recip_ac, sqrt_recipm1_ac, sqrt_ac, sqrt_1mac, out, mean_type, inner, num_steps, num_timesteps);
    DSC_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsc_cfg_combine_f32(const float* model_out, const float* scale, float* out, int32_t b, int64_t inner,
                                   dsc_stream_t stream) {
    if (!model_out || !scale || !out || b < 1 || inner < 1) return DSC_EINVAL;
    if (b > 65535) return DSC_ERANGE;
    DSC_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL(cfg_combine_kernel, dim3(grid_x(inner), b), dim3(256), 0, static_cast<hipStream_t>(stream), model_out, scale,
                       out, inner);
    DSC_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsc_p_sample_cfg_f32(const float* x_t, const float* model_out, const float* scale, const float* noise, const int64_t* t,
                                    const float* ca, const float* cb, const float* coef1, const float* coef2, const float* sigma,
                                    float* out, float* x_dup, float* x0_out, int32_t mean_type, int32_t clip, int32_t b,
                                    int64_t inner, int32_t num_timesteps, dsc_stream_t stream) {
    if (!x_t || !model_out || !scale || !noise || !t || !coef1 || !coef2 || !sigma || !out || b < 1 || inner < 1 || num_timesteps < 1)
        return DSC_EINVAL;
    if (bad_mean_args(mean_type, ca, cb)) return DSC_EINVAL;
    if (b > 65535) return DSC_ERANGE;
    DSC_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL(p_sample_cfg_kernel, dim3(grid_x(inner), b), dim3(256), 0, static_cast<hipStream_t>(stream),
                       x_t, model_out, scale, noise, t, ca, cb, coef1, coef2, sigma, out, x_dup, x0_out, mean_type, clip, inner,
                       num_timesteps);
    DSC_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsc_ddim_cfg_step_f32(const float* x_t, const float* model_out, const float* scale, const float* noise,
                                     const int64_t* step, const int64_t* times, const int64_t* times_next,
                                     const float* sqrt_alpha_next, const float* c_noise, const float* sigma, const float* ca,
                                     const float* cb, const float* sqrt_recip_ac, const float* sqrt_recipm1_ac, float* out,
                                     float* x_dup, float* x0_out, int32_t mean_type, int32_t b, int64_t inner, int32_t num_steps,
                                     int32_t num_timesteps, dsc_stream_t stream) {
    if (!x_t || !model_out || !scale || !noise || !step || !times || !times_next || !sqrt_alpha_next || !c_noise || !sigma ||
        !sqrt_recip_ac || !sqrt_recipm1_ac || !out || b < 1 || inner < 1 || num_steps < 1 || num_timesteps < 1)
        return DSC_EINVAL;
    if (bad_mean_args(mean_type, ca, cb)) return DSC_EINVAL;
    if (b > 65535) return DSC_ERANGE;
    DSC_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL(ddim_cfg_step_kernel, dim3(grid_x(inner), b), dim3(256), 0, static_cast<hipStream_t>(stream),
                       x_t, model_out, scale, noise, step, times, times_next, sqrt_alpha_next, c_noise, sigma, ca, cb,
                       sqrt_recip_ac, sqrt_recipm1_ac, out, x_dup, x0_out, mean_type, inner, num_steps, num_timesteps);
    DSC_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsc_p_sample_masked_cfg_f32(const float* x_t, const float* model_out, const float* scale, const float* noise,
                                           const float* known, const float* noise_k, const uint8_t* mask, const int64_t* t,
                                           const float* ca, const float* cb, const float* coef1, const float* coef2, const float* sigma,
                                           const float* sqrt_ac, const float* sqrt_1mac, float* out, float* x_dup, int32_t mean_type,
                                           int32_t clip, int32_t b, int64_t inner, int32_t num_timesteps, dsc_stream_t stream) {
    if (!x_t || !model_out || !scale || !noise || !known || !noise_k || !mask || !t || !coef1 || !coef2 || !sigma || !sqrt_ac ||
        !sqrt_1mac || !out || b < 1 || inner < 1 || num_timesteps < 1)
        return DSC_EINVAL;
    if (bad_mean_args(mean_type, ca, cb)) return DSC_EINVAL;
    if (b > 65535) return DSC_ERANGE;
    DSC_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL(p_sample_masked_cfg_kernel, dim3(grid_x(inner), b), dim3(256), 0, static_cast<hipStream_t>(stream),
                       x_t, model_out, scale, noise, known, noise_k, mask, t, ca, cb, coef1, coef2, sigma, sqrt_ac, sqrt_1mac, out,
                       x_dup, mean_type, clip, inner, num_timesteps);
    DSC_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsc_ddim_masked_cfg_step_f32(const float* x_t, const float* model_out, const float* scale, const float* noise,
                                            const float* known, const float* noise_k, const uint8_t* mask, const int64_t* step,
                                            const int64_t* times, const int64_t* times_next, const float* sqrt_alpha_next,
                                            const float* c_noise, const float* sigma, const float* ca, const float* cb,
                                            const float* sqrt_recip_ac, const float* sqrt_recipm1_ac, const float* sqrt_ac,
                                            const float* sqrt_1mac, float* out, float* x_dup, int32_t mean_type, int32_t b,
                                            int64_t inner, int32_t num_steps, int32_t num_timesteps, dsc_stream_t stream) {
    if (!x_t || !model_out || !scale || !noise || !known || !noise_k || !mask || !step || !times || !times_next || !sqrt_alpha_next ||
        !c_noise || !sigma || !sqrt_recip_ac || !sqrt_recipm1_ac || !sqrt_ac || !sqrt_1mac || !out || b < 1 || inner < 1 ||
        num_steps < 1 || num_timesteps < 1)
        return DSC_EINVAL;
    if (bad_mean_args(mean_type, ca, cb)) return DSC_EINVAL;
    if (b > 65535) return DSC_ERANGE;
    DSC_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL(ddim_masked_cfg_step_kernel, dim3(grid_x(inner), b), dim3(256), 0, static_cast<hipStream_t>(stream),
                       x_t, model_out, scale, noise, known, noise_k, mask, step, times, times_next, sqrt_alpha_next, c_noise, sigma, ca,
                       cb, sqrt_recip_ac, sqrt_recipm1_ac, sqrt_ac, sqrt_1mac, out, x_dup, mean_type, inner, num_steps, num_timesteps);
    DSC_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsc_scene_gate_f32(const float* x, const uint8_t* keep, float* y, int32_t b, int64_t inner, dsc_stream_t stream) {
    if (!x || !keep || !y || b < 1 || inner < 1) return DSC_EINVAL;
    if (b > 65535) return DSC_ERANGE;
    DSC_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL(scene_gate_kernel, dim3(grid_x(inner), b), dim3(256), 0, static_cast<hipStream_t>(stream), x, keep, y, inner);
    DSC_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsc_scene_randn_f32(float* out, const int64_t* seeds, const int64_t* draw, int64_t stream, int64_t b,
                                   int64_t per_scene, dsc_stream_t hip_stream) {
    return launch_scene_noise(out, seeds, draw, stream, b, per_scene, hip_stream);
}

extern "C" int dsc_scene_philox_u32(uint32_t* out, const int64_t* seeds, const int64_t* draw, int64_t stream, int64_t b,
                                    int64_t per_scene, dsc_stream_t hip_stream) {
    return launch_scene_noise(out, seeds, draw, stream, b, per_scene, hip_stream);
}

unsigned dsc_bad_index_diffusion(bool reset) { return dsc_read_bad_index_count(reset); }

// Number of out-of-range device indices (timesteps outside [0, num_timesteps)) that kernels had to clamp since the
// last reset -- 0 in every correct run.  Synchronising (device-to-host reads of the per-unit counters): a test / debugging facility.
extern "C" int64_t dsc_device_error_count(int32_t reset) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    const unsigned a = dsc_bad_index_diffusion(reset != 0), b = dsc_bad_index_train(reset != 0), c = dsc_bad_index_retrieval(reset != 0);
    if (a == 0xffffffffu || b == 0xffffffffu || c == 0xffffffffu) return -1;
    return (int64_t)a + b + c;
}
