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

__global__ void add_scalar_i64_kernel(int64_t* t, int count, int64_t delta) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) t[i] += delta;
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

// Collision steering: one launch between the model call and the unchanged step.  One 256-thread block per scene,
// n <= 160, three phases:
//   1. thread i < n forms row i of the clamped x0 estimate -- the 8 box channels and the 'empty' logit; a given element (ragged rows or
//      mask) takes its given value, a free one clamp(predict_x0(x_t, m)), the float32 value the step will form, with m the guidance
//      mix where scale is set -- and from it the axis-aligned bounds of the box rotated about y (half extents hx = |c| sx + |s| sz,
//      hy = sy, hz = |s| sx + |c| sz, (c, s) the (cos, sin) channels over their hypot; a zero pair counts as angle 0), staged in LDS
//      with the validity flag (empty logit < 0);
//   2. a valid thread walks j = 0 .. n - 1 in index order over the other valid boxes: IoU(i, j) with union floor 1e-6 (the expressions
//      of networks/loss.py) where all three overlaps are positive -- boxes that only touch do not interact --, the energy terms j > i
//      and d IoU / d centre_i (sizes and angle carry no gradient; a face shared exactly by both boxes takes half the derivative);
//   3. the energy is summed in a fixed order (butterfly per wave, then the four partials: scene b's result does not depend on the
//      batch), the gradient goes to normalised units (* span / 2), and on an active step -- t < *t_below and weight[b] != 0 -- every
//      free translation element of a valid box whose weight * g is non-zero has its model output moved so that the step's
//      x0 = clamp(x0) - weight * g:  d = weight * g + (raw - clamp(raw));  mean type x0: m -= d;  eps / v: m += d / Bc (Bc == 0: no
//      change);  guided: the same delta goes to both halves of the 2 b output, which moves u + w (c - u) by it.
// From the float32 x0 on, the geometry is float64: an overlap is a small difference of box faces, so in float32 the sum over the pairs
// loses five to six digits and lands within a few ulp of the exact value only by the luck of its order; in float64 the energy and the
// gradient are the float32 numbers nearest to the exact ones, whatever the order, and the new model output is rounded once.  The
// work is n^2 pairs of ~40 operations per scene, far below a microsecond of the float64 rate: the launch is latency, not arithmetic.
// An inactive launch without optional outputs returns before it reads the scene and stores nothing.  Bad indices: t[b] / counts[b]
// once per scene by thread 0, step[0] and times[k] once per launch.
constexpr int STEER_MAXN = 160;

struct SteerArgs {
    const float* xt; float* mo;
    const int64_t *t, *step, *times;
    const float *ca, *cb, *partial;
    const int64_t* counts;
    const float* known;
    const uint8_t* mask;
    const float *scale, *weight;
    const int64_t* t_below;
    float *energy, *grad;
    int mean_type, b, n, pmax, c, empty_col, S, T;
    double c_lo[3], c_span[3], s_lo[3], s_span[3];
};

// Fixed-order block sum of four waves (the form of train.hip's block_sum_loss), in float64.
__device__ __forceinline__ double block_sum_steer(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// The frame both steering kernels stand on.  The scene: the checked time and given-row count, the weight, whether this launch moves the
// model output, the x0 coefficients, the guidance scale and the offsets of thread tid's row in either half of the model output.
struct SteerScene {
    int64_t cnt, row, half;
    float w, A, Bc, s;
    bool is_x0, active;
};

__device__ __forceinline__ SteerScene steer_scene(const SteerArgs& p, int b, int tid) {
    SteerScene f;
    const bool first = tid == 0;
    f.is_x0 = p.mean_type == DSC_MEAN_X0;
    int64_t tv;
    if (p.t) tv = dsc_checked_index(p.t[b], p.T, first);
    else tv = dsc_checked_index(p.times[dsc_checked_index(p.step[0], p.S, first && b == 0)], p.T, first && b == 0);
    f.cnt = 0;
    if (p.counts) f.cnt = dsc_checked_index(p.counts[b], (int64_t)p.pmax + 1, first);
    f.w = p.weight[b];
    f.active = f.w != 0.f && tv < p.t_below[0];
    f.A = f.is_x0 ? 0.f : p.ca[tv], f.Bc = f.is_x0 ? 0.f : p.cb[tv];
    f.s = p.scale ? p.scale[b] : 0.f;
    f.half = (int64_t)p.b * p.n * p.c;
    f.row = (int64_t)b * p.n * p.c + (int64_t)tid * p.c;
    return f;
}

// Row tid < n of the clamped x0 estimate: the 8 box channels and the 'empty' logit, and for the translation channels the unclamped and
// the clamped prediction and whether the element is free.
struct SteerRow {
    float v[9], raw[3], x0c[3];
    bool is_free[3];
};

__device__ __forceinline__ SteerRow steer_x0_row(const SteerArgs& p, const SteerScene& f, int b, int tid) {
    SteerRow r{};
    const int64_t row = f.row, half = f.half;
    const bool row_given = p.counts && tid < f.cnt;
    const int64_t grow = ((int64_t)b * p.pmax + tid) * p.c;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int ch = k < 8 ? k : p.empty_col;
        const bool given = row_given || (p.mask && p.mask[row + ch] != 0);
        if (given) {
            r.v[k] = row_given ? p.partial[grow + ch] : p.known[row + ch];
        } else {
            float m = p.mo[row + ch];
            if (p.scale) m = cfg_mix(m, p.mo[half + row + ch], f.s);
            const float x = predict_x0(f.is_x0 ? 0.f : p.xt[row + ch], m, f.A, f.Bc, p.mean_type, false);
            r.v[k] = fminf(fmaxf(x, -1.0f), 1.0f);
            if (k < 3) r.raw[k] = x, r.x0c[k] = r.v[k];
        }
        if (k < 3) r.is_free[k] = !given;
    }
    return r;
}

// Translation channel k of row tid < n, with g = dE / d centre_k: the gradient in normalised units goes to the optional output, and
// where `move` holds on an active step the free element's model output is moved (both halves of a guided one).
__device__ __forceinline__ void steer_store(const SteerArgs& p, const SteerScene& f, const SteerRow& r, int b, int tid, int k, double g,
                                            bool move) {
    const int64_t row = f.row, half = f.half;
    const double gn = g * p.c_span[k] * 0.5;                                                  // d centre / d x0 = span / 2
    if (p.grad) p.grad[((int64_t)b * p.n + tid) * 3 + k] = (float)gn;
    if (!move || !f.active || !r.is_free[k]) return;
    const double wg = (double)f.w * gn;
    if (wg == 0. || (!f.is_x0 && f.Bc == 0.f)) return;
    const double d = wg + ((double)r.raw[k] - (double)r.x0c[k]);
    const double delta = f.is_x0 ? -d : d / (double)f.Bc;
    if (p.scale) {
        const float c0 = p.mo[row + k], u0 = p.mo[half + row + k];
        p.mo[row + k] = (float)((double)c0 + delta);
        p.mo[half + row + k] = (float)((double)u0 + delta);
    } else {
        p.mo[row + k] = (float)((double)p.mo[row + k] + delta);
    }
}

__global__ __launch_bounds__(256) void steer_boxes_kernel(const SteerArgs p) {
    __shared__ double red[4];
    __shared__ double lo[STEER_MAXN][3], hi[STEER_MAXN][3];                                   // 7.5 KB
    __shared__ float valid[STEER_MAXN];
    const int b = blockIdx.x, tid = threadIdx.x, N = p.n;
    const SteerScene f = steer_scene(p, b, tid);
    if (!f.active && !p.energy && !p.grad) return;                                           // the whole block: nothing is stored
    double li[3] = {0., 0., 0.}, hi_i[3] = {0., 0., 0.};
    SteerRow r{};
    bool ok = false;
    if (tid < N) {
        r = steer_x0_row(p, f, b, tid);
        const float* v = r.v;
        double ctr[3], sz[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            ctr[k] = ((double)v[k] + 1.0) * 0.5 * p.c_span[k] + p.c_lo[k];
            sz[k] = ((double)v[3 + k] + 1.0) * 0.5 * p.s_span[k] + p.s_lo[k];
        }
        const double cs = (double)v[6], sn = (double)v[7];
        const double hyp = sqrt(cs * cs + sn * sn);
        double ac = 1.0, as = 0.0;
        if (hyp > 0.) ac = fabs(cs) / hyp, as = fabs(sn) / hyp;
        const double h[3] = {ac * sz[0] + as * sz[2], sz[1], as * sz[0] + ac * sz[2]};
        ok = v[8] < 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            li[k] = ctr[k] - h[k], hi_i[k] = ctr[k] + h[k];
            lo[tid][k] = li[k], hi[tid][k] = hi_i[k];
        }
        valid[tid] = ok ? 1.f : 0.f;
    }
    __syncthreads();
    double g[3] = {0., 0., 0.}, e = 0.;
    if (ok) {
        const double vi = (hi_i[0] - li[0]) * (hi_i[1] - li[1]) * (hi_i[2] - li[2]);
        for (int j = 0; j < N; ++j) {
            if (j == tid || valid[j] <= 0.f) continue;
            double wh[3], sgn[3], ej[3];
            bool hit = true;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double hj = hi[j][k], lj = lo[j][k];
                ej[k] = hj - lj;
                wh[k] = fmin(hi_i[k], hj) - fmax(li[k], lj);
                hit = hit && wh[k] > 0.;
                const double wr = hi_i[k] < hj ? 1. : (hi_i[k] == hj ? 0.5 : 0.);              // is the inner upper face box i's
                const double wl = li[k] > lj ? 1. : (li[k] == lj ? 0.5 : 0.);                  // the inner lower face
                sgn[k] = wr - wl;
            }
            if (!hit) continue;
            const double vj = ej[0] * ej[1] * ej[2];
            const double o = wh[0] * wh[1] * wh[2];
            const double uraw = (vi + vj) - o;
            const bool ucl = !(uraw > 1e-6);                                                  // the union at its floor
            const double u = ucl ? 1e-6 : uraw;
            const double iou = o / u;
            if (j > tid) e += iou;
            const double dio = ucl ? 1.0 / u : (1.0 + iou) / u;                               // d IoU / d overlap (d union / d overlap = -1)
#pragma unroll
            for (int k = 0; k < 3; ++k) g[k] += dio * (wh[(k + 1) % 3] * wh[(k + 2) % 3]) * sgn[k];
        }
    }
    const double E = block_sum_steer(e, red);
    if (p.energy && tid == 0) p.energy[b] = (float)E;
    if (tid >= N) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) steer_store(p, f, r, b, tid, k, g[k], ok);
}

// Floor-plan steering, the field: once per call, never inside the loop.  The mask image (h rows along z, w columns
// along x, inside iff > 0.5) covers [-s, s]^2, s = room_side; dx = 2 s / w, dz = 2 s / h.
//   F[i, j] = 1/2 min over inside (i', j') of ((i - i') dz)^2 + ((j - j') dx)^2,  0 where no pixel is inside,
// float64, rounded once.  The minimum is taken exactly in two passes: every float64 operation of the expression is monotone in
// |i - i'|, so for a column j' the nearest inside row decides.  One block per (scene, row i): thread j' < w walks column j' outwards
// from row i to its nearest inside pixel and stages ((i - i') dz)^2 in LDS (infinity: none); thread j < w then takes the minimum over
// j' of the staged term plus ((j - j') dx)^2 -- the very expressions of the definition, so the result is the float32 nearest to it.
constexpr int WALL_MAXHW = 256;

__global__ __launch_bounds__(256) void floor_field_kernel(const float* __restrict__ mask, float* __restrict__ field, int h, int w,
                                                          float room_side) {
    __shared__ double col[WALL_MAXHW];
    const int i = blockIdx.x, b = blockIdx.y, j = threadIdx.x;
    const double rs = (double)room_side;
    const double dx = 2.0 * rs / (double)w, dz = 2.0 * rs / (double)h;
    const float* m = mask + (int64_t)b * h * w;
    if (j < w) {
        int d = -1;
        for (int k = 0; k < h; ++k) {                                                        // |i - i'| = k, nearest first
            const bool up = i - k >= 0 && m[(int64_t)(i - k) * w + j] > 0.5f;
            const bool down = i + k < h && m[(int64_t)(i + k) * w + j] > 0.5f;
            if (up || down) {
                d = k;
                break;
            }
        }
        const double a = (double)d * dz;
        col[j] = d < 0 ? (double)INFINITY : a * a;
    }
    __syncthreads();
    if (j >= w) return;
    double best = (double)INFINITY;
    for (int k = 0; k < w; ++k) {
        const double c = (double)(j - k) * dx;
        const double cc = c * c;
        const double v = col[k] + cc;
        best = fmin(best, v);
    }
    const double f = 0.5 * best;
    field[((int64_t)b * h + i) * w + j] = best == (double)INFINITY ? 0.f : (float)f;
}

// Floor-plan steering, the launch inside the loop: after collision steering (if any), before the multistep launch and the guidance mix.
// One 256-thread block per scene, n <= 160, modelled on steer_boxes_kernel -- the same time sources, given parts, guidance operand and
// the same clamped x0 row per thread:
//   1. thread i < n forms row i of the clamped x0 estimate (steer_boxes_kernel, phase 1) and de-normalises the centre and half sizes;
//      (c, s) = the (cos, sin) channels over their hypot (a zero pair: angle 0); valid iff the empty logit < 0;
//   2. a valid thread visits its nine footprint points p_ab = centre_xz + R (a sx, b sz), a, b in {-1, 0, 1} in (a, b) order, R the
//      rotation about y (x' = c lx - s lz, z' = s lx + c lz), and at each: u = (x + s) / dx - 1/2, v = (z + s) / dz - 1/2, clamped to
//      the pixel centres, the cell j0 = min(floor(uc), w - 2), i0 likewise, and
//      e(p) = bilinear(F; i0, j0, fv, fu) + 1/2 ((u - uc) dx)^2 + 1/2 ((v - vc) dz)^2 with its derivative by the point: inside the
//      image the slope of the bilinear patch, outside the quadratic continuation; 36 float32 field reads per box, served by L2;
//   3. E = sum over valid boxes of (1/9) sum e(p) in the fixed order of block_sum_steer, `outside` = the number of valid boxes with a
//      point of e > 0, g = dE / d x0[:, {0, 2}] (* span / 2; y stays 0), and on an active step -- t < *t_below and weight[b] != 0 --
//      the store of steer_boxes_kernel on channels 0 and 2.
// float64 after the float32 x0 and the float32 field, one final rounding.  An inactive launch without optional outputs returns before
// it reads the scene.  field_b == 1: one field shared by every scene.  room_side is read through its pointer, as weight and t_below.
struct WallArgs {
    SteerArgs s;
    const float *field, *room_side;
    int32_t* outside;
    int field_b, h, w;
};

__global__ __launch_bounds__(256) void steer_walls_kernel(const WallArgs q) {
    __shared__ double red[4];
    const SteerArgs& p = q.s;
    const int b = blockIdx.x, tid = threadIdx.x, N = p.n, H = q.h, W = q.w;
    const SteerScene f = steer_scene(p, b, tid);
    if (!f.active && !p.energy && !p.grad && !q.outside) return;                             // the whole block: nothing is stored
    SteerRow r{};
    bool ok = false;
    double g[3] = {0., 0., 0.}, e = 0., out = 0.;
    if (tid < N) {
        r = steer_x0_row(p, f, b, tid);
        const float* v = r.v;
        ok = v[8] < 0.f;
        if (ok) {
            const double cx = ((double)v[0] + 1.0) * 0.5 * p.c_span[0] + p.c_lo[0];
            const double cz = ((double)v[2] + 1.0) * 0.5 * p.c_span[2] + p.c_lo[2];
            const double sx = ((double)v[3] + 1.0) * 0.5 * p.s_span[0] + p.s_lo[0];
            const double sz = ((double)v[5] + 1.0) * 0.5 * p.s_span[2] + p.s_lo[2];
            const double cs = (double)v[6], sn = (double)v[7];
            const double hyp = sqrt(cs * cs + sn * sn);
            double rc = 1.0, rsn = 0.0;
            if (hyp > 0.) rc = cs / hyp, rsn = sn / hyp;
            const double side = (double)q.room_side[0];
            const double dx = 2.0 * side / (double)W, dz = 2.0 * side / (double)H;
            const double rdx = 1.0 / dx, rdz = 1.0 / dz;                                      // a float64 division is a long serial chain: two per box
            const double umax = (double)(W - 1), vmax = (double)(H - 1);
            const float* F = q.field + (q.field_b == 1 ? 0 : (int64_t)b * H * W);
            double esum = 0., gx = 0., gz = 0.;
            bool any = false;
            for (int a = -1; a <= 1; ++a) {
                for (int bb = -1; bb <= 1; ++bb) {
                    const double lx = (double)a * sx, lz = (double)bb * sz;
                    const double xa = rc * lx, xb = rsn * lz, za = rsn * lx, zb = rc * lz;
                    const double px = cx + (xa - xb), pz = cz + (za + zb);
                    const double u = (px + side) * rdx - 0.5, vv = (pz + side) * rdz - 0.5;
                    const double uc = fmin(fmax(u, 0.), umax), vc = fmin(fmax(vv, 0.), vmax);  // fmax(NaN, 0) = 0: always a cell
                    const int j0 = min(max((int)floor(uc), 0), W - 2), i0 = min(max((int)floor(vc), 0), H - 2);
                    const double fu = uc - (double)j0, fv = vc - (double)i0;
                    const float* cell = F + (int64_t)i0 * W + j0;
                    const double f00 = (double)cell[0], f01 = (double)cell[1], f10 = (double)cell[W], f11 = (double)cell[W + 1];
                    const double top = f00 + (f01 - f00) * fu, bot = f10 + (f11 - f10) * fu;
                    const double bil = top + (bot - top) * fv;
                    const double ou = (u - uc) * dx, ov = (vv - vc) * dz;
                    const double ep = bil + 0.5 * (ou * ou) + 0.5 * (ov * ov);
                    esum += ep;
                    any = any || ep > 0.;
                    // d e / d u: the patch's slope where u is inside the image, the continuation's where it is clamped
                    const double su = (f01 - f00) + ((f11 - f10) - (f01 - f00)) * fv;
                    const double sv = bot - top;
                    gx += (u == uc ? su : ou * dx) * rdx;
                    gz += (vv == vc ? sv : ov * dz) * rdz;
                }
            }
            e = esum * (1.0 / 9.0);
            out = any ? 1. : 0.;
            g[0] = gx * (1.0 / 9.0), g[2] = gz * (1.0 / 9.0);
        }
    }
    const double E = block_sum_steer(e, red);
    const double O = block_sum_steer(out, red);
    if (p.energy && tid == 0) p.energy[b] = (float)E;
    if (q.outside && tid == 0) q.outside[b] = (int32_t)O;
    if (tid >= N) return;
    steer_store(p, f, r, b, tid, 0, g[0], ok);
    steer_store(p, f, r, b, tid, 1, g[1], false);                                            // y: the zero gradient is reported, never applied
    steer_store(p, f, r, b, tid, 2, g[2], ok);
}

// Which elements of a scene are given (completion, in-painting) instead of sampled: none, the first counts[b] rows, or a byte mask.
enum { GIVEN_NONE = 0, GIVEN_ROWS = 1, GIVEN_MASK = 2 };

// Multistep DPM-Solver++(2M): one launch between the model call (after collision steering, if any) and the unchanged
// strided step.  The solver is a data-prediction one: its first-order form is DDIM at eta = 0, its second-order form the same step on
// an extrapolated x0 estimate.  With the pairs (t_k, t'_k) of ddim_schedule(S, 0), lambda(t) = 1/2 ln(abar_t / (1 - abar_t)) and
// h_k = lambda(t'_k) - lambda(t_k), the history weights are e_0 = 0, e_k = h_k / (2 h_{k-1}) for 1 <= k <= S - 2 and e_{S-1} = 0 (the
// last pair takes x0: "lower order final"); the host computes them in float64 and hands over an (S,) float32 table.  At pair
// k = step[0], for every free element:
//   m     = mo, or cfg_mix(c, u, scale[b]) from the two halves of a 2 b output, in float32 exactly as the step forms it;
//   x0raw = predict_x0(x_t, m) in float32, the step's own expressions and rounding;  x0c = clamp(x0raw, -1, 1);
//   from here float64 with one final rounding:  D = x0c + e_k (x0c - hist);  d = x0raw - D;
//   mean type x0: m' = m - d;  eps / v: m' = m + d / Bc (Bc == 0: no change);  guided: the same delta goes to both halves;
//   hist  = x0c -- the float32 x0 of this pair, steered but not extrapolated.
// The step then runs on m': where D lies inside [-1, 1] its x0 is D, the DPM-Solver++(2M) update; outside, the step's clamp applies as
// it does to DDIM here.  What the kernel keeps:
// * e[k] == 0: hist is not read and mo is not written -- a stale or NaN history can never leak in, and S <= 2 is DDIM at eta = 0 bit
//   for bit.  hist is written on every pair except the last (k == S - 1), where the launch returns before it reads anything else.
// * A given element (ragged row prefix or mask) is neither read nor written: x_t, mo and hist alike.
// * Every scene is at the same pair; step[0] and times[k] are clamped and counted once per launch, counts[b] once per scene.
// * HBM traffic per free element: at most three reads (x_t, mo, hist; two of mo if guided) and two writes (mo, hist).  Every product,
//   sum and difference is a statement of its own (-ffp-contract=off).
template <int GIVEN, bool GUIDED>
__global__ __launch_bounds__(256) void multistep_x0_kernel(const float* __restrict__ xt, float* __restrict__ mo, float* __restrict__ hist,
                                                          const float* __restrict__ weights, const int64_t* __restrict__ step,
                                                          const int64_t* __restrict__ times, const float* __restrict__ ca,
                                                          const float* __restrict__ cb, const float* __restrict__ scale,
                                                          const int64_t* __restrict__ counts, const uint8_t* __restrict__ mask,
                                                          int mean_type, int64_t inner, int pmax, int c, int S, int T) {
    const int b = blockIdx.y;
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    const bool is_x0 = mean_type == DSC_MEAN_X0;
    const int64_t k = dsc_checked_index(step[0], S, first && b == 0);
    const int64_t tv = dsc_checked_index(times[k], T, first && b == 0);
    int64_t cnt = 0;
    if constexpr (GIVEN == GIVEN_ROWS) cnt = dsc_checked_index(counts[b], (int64_t)pmax + 1, first) * c;
    if (k == S - 1) return;                                                                  // the last pair: nothing is read or stored
    const float e = weights[k];
    const float A = is_x0 ? 0.f : ca[tv], Bc = is_x0 ? 0.f : cb[tv];
    const bool move = e != 0.f && (is_x0 || Bc != 0.f);
    float w = 0.f;
    if constexpr (GUIDED) w = scale[b];
    const int64_t base = (int64_t)b * inner, half = (int64_t)gridDim.y * inner;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < inner; i += (int64_t)gridDim.x * blockDim.x) {
        if constexpr (GIVEN == GIVEN_ROWS) {
            if (i < cnt) continue;
        }
        if constexpr (GIVEN == GIVEN_MASK) {
            if (mask[base + i] != 0) continue;
        }
        const float c0 = mo[base + i];
        float u0 = 0.f, m = c0;
        if constexpr (GUIDED) {
            u0 = mo[half + base + i];
            m = cfg_mix(c0, u0, w);
        }
        const float raw = predict_x0(is_x0 ? 0.f : xt[base + i], m, A, Bc, mean_type, false);
        const float x0c = fminf(fmaxf(raw, -1.0f), 1.0f);
        if (move) {
            const double x0d = (double)x0c;
            const double diff = x0d - (double)hist[base + i];
            const double ext = (double)e * diff;
            const double D = x0d + ext;
            const double d = (double)raw - D;
            const double delta = is_x0 ? -d : d / (double)Bc;
            mo[base + i] = (float)((double)c0 + delta);
            if constexpr (GUIDED) mo[half + base + i] = (float)((double)u0 + delta);
        }
        hist[base + i] = x0c;
    }
}

// The reverse step, one launch after the model call: every dsc_*p_sample*_f32 and dsc_ddim_*step_f32 is one instantiation.
//
//   STRIDED  false: the posterior step of p_sample (diffusion_ddpm.py:305-352) at the scene's own row tv = t[b]:
//                   out = k1 * x0 + k2 * x + sigma[tv] * noise, x0 clamped to [-1, 1] per ``clip``.
//            true:  one pair of ddim_sample_loop (:402-444; x_start / pred_noise as model_predictions(clip_x_start=True,
//                   rederive_pred_noise=False), :242-264).  Every scene is at the same pair k = step[0], a device counter, and the
//                   per-pair scalars come from device tables of S rows, so the launch can be captured once and replayed.  x0 is
//                   always clamped (the reference ignores clip_denoised here).  times_next[k] < 0 marks the last pair: out = x0.
//   GIVEN    none:  every element is free.
//            rows:  rows [0, counts[b]) of scene b are given; given / noise_g hold pmax rows per scene (rows >= counts[b] are padding,
//                   never read), so the given part is indexed at b * pmax * c + i, the rest at b * n * c + i.
//            mask:  element i is given where mask[i] != 0; mask / given / noise_g have x's shape.
//   GUIDED   mo holds 2 b scenes, [conditional; unconditional] on the same x, and m = cfg_mix(c, u, scale[b]) is formed in registers;
//            x_dup (may be NULL) receives a second copy of every written element, given or free, so that a captured loop keeps x
//            as one (2 b, inner) buffer with both halves current.
//
// A free element gets the step.  A given one, whose step the loop's next overwrite would discard, gets what the loop writes there
// next: q_sample(given, t - 1 or times_next[k], noise_g) -- the overwrite that precedes the next model call -- or, at t == 0 / on the
// last pair, given itself (the final restore).  What every instantiation keeps:
//
// * Rounding.  Every product, sum and difference is a statement of its own in the helpers above, operands in the reference's order,
//   the division IEEE: a fused instantiation is bit-identical to the composition of the unfused ones (cfg_combine, then the plain
//   step, then the overwrite at the next time or the restore), and the plain ones to the reference's fp32 expressions.
// * Noise at t == 0.  The posterior instantiations force sigma to 0 at tv == 0 and still add 0 * noise: infinite noise gives NaN on
//   a free element.  The exception is <posterior, none, guided> (SKIP_NOISE_AT_0): it loads sigma as tabulated and does not read the
//   noise at tv == 0 -- equal to the composition on finite noise, up to the sign of a zero.  tests/test_gpu_sampler_core.py pins both.
// * Last strided pair.  Neither noise nor noise_g is read.
// * Read sets.  A given element reads mask (nothing, for rows), given and noise_g only -- no noise_g at t == 0 or on the last pair;
//   a free one mask, xt, mo (both halves if guided) and noise only.  A pointer an instantiation has no use for is never loaded.
// * Bad indices (clamped, then counted by one thread each).  t[b] and counts[b] (into [0, pmax]): once per out-of-range scene, by
//   thread 0 of block x = 0.  step[0], times[k] and -- only where a given part exists and the pair is not the last -- times_next[k]:
//   once per launch.
// * Outputs.  out may alias xt (the in-place step), so neither is __restrict__, and an element is stored only after all of its loads.
//   x0_out (may be NULL) exists only without a given part.
template <bool STRIDED, int GIVEN, bool GUIDED>
__global__ __launch_bounds__(256) void step_kernel(
    const float* xt, const float* __restrict__ mo, const float* __restrict__ scale, const float* __restrict__ noise,
    const float* __restrict__ given, const float* __restrict__ noise_g, const uint8_t* __restrict__ mask,
    const int64_t* __restrict__ counts, const int64_t* __restrict__ t, const int64_t* __restrict__ step,
    const int64_t* __restrict__ times, const int64_t* __restrict__ times_next, const float* __restrict__ sqrt_an,
    const float* __restrict__ cnoise, const float* __restrict__ sigma, const float* __restrict__ ca, const float* __restrict__ cb,
    const float* __restrict__ c1, const float* __restrict__ c2, const float* __restrict__ ra, const float* __restrict__ rm,
    const float* __restrict__ sa, const float* __restrict__ sb, float* out, float* __restrict__ x_dup, float* __restrict__ x0_out,
    int mean_type, int clip, int64_t inner, int pmax, int c, int S, int T) {
    constexpr bool HAS_GIVEN = GIVEN != GIVEN_NONE;
    constexpr bool SKIP_NOISE_AT_0 = !STRIDED && !HAS_GIVEN && GUIDED;
    const int b = blockIdx.y;
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;                                  // one count per out-of-range scene
    PosteriorCoef p{};
    DdimCoef d{};
    Renoise r{};
    int64_t tv = 0;
    if constexpr (STRIDED) {
        d = ddim_coef(step, times, times_next, sqrt_an, cnoise, sigma, ca, cb, ra, rm, mean_type, S, T, first && b == 0, HAS_GIVEN);
        if constexpr (HAS_GIVEN) r = renoise_coef(!d.last, d.tn, sa, sb);
    } else {
        tv = dsc_checked_index(t[b], T, first);
        p = posterior_coef(tv, ca, cb, c1, c2, sigma, mean_type, !SKIP_NOISE_AT_0);
        if constexpr (HAS_GIVEN) r = renoise_coef(tv > 0, tv - 1, sa, sb);
    }
    const float A = STRIDED ? d.A : p.A, Bc = STRIDED ? d.Bc : p.Bc;
    int64_t cnt = 0;
    if constexpr (GIVEN == GIVEN_ROWS) cnt = dsc_checked_index(counts[b], (int64_t)pmax + 1, first) * c;
    float w = 0.f;
    if constexpr (GUIDED) w = scale[b];
    const int64_t base = (int64_t)b * inner, half = (int64_t)gridDim.y * inner;
    const int64_t gbase = GIVEN == GIVEN_ROWS ? (int64_t)b * pmax * c : base;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < inner; i += (int64_t)gridDim.x * blockDim.x) {
        bool is_given = false;
        if constexpr (GIVEN == GIVEN_ROWS) is_given = i < cnt;
        if constexpr (GIVEN == GIVEN_MASK) is_given = mask[base + i] != 0;
        float y, x0 = 0.f;
        if (is_given) {
            const float g = given[gbase + i];
            y = r.on ? renoise(g, noise_g[gbase + i], r.a, r.s) : g;
        } else {
            const float x = xt[base + i];
            float m = mo[base + i];
            if constexpr (GUIDED) m = cfg_mix(m, mo[half + base + i], w);
            x0 = predict_x0(x, m, A, Bc, mean_type, STRIDED || clip);
            if constexpr (STRIDED) {
                y = x0;
                if (!d.last) y = add_noise(ddim_mean(x0, x, m, d, mean_type), noise[base + i], d.sg);
            } else {
                y = posterior_mean(x0, x, p);
                if (!SKIP_NOISE_AT_0 || tv != 0) y = add_noise(y, noise[base + i], p.sg);
            }
        }
        out[base + i] = y;
        if constexpr (GUIDED) {
            if (x_dup) x_dup[base + i] = y;
        }
        if constexpr (!HAS_GIVEN) {
            if (x0_out) x0_out[base + i] = x0;
        }
    }
}

// The standalone overwrite of the completion and in-painting loops (p_sample_loop_complete, diffusion_ddpm.py:462-466, and its ragged
// and masked forms): the given branch of step_kernel at the scene's own t[b], x = sa[t] * given + sb[t] * noise_g, and no free
// branch -- an element that is not given is neither read nor written.  rows: the grid covers the pmax * c elements of a scene's given
// part; a scene with count 0 writes nothing; counts == NULL is the fixed form, every scene has pmax rows and nothing but t[b] is
// counted.  mask: the grid covers the scene.  Indices and their counting as in step_kernel.
template <int GIVEN>
__global__ __launch_bounds__(256) void overwrite_kernel(float* __restrict__ x, const float* __restrict__ given,
                                                       const float* __restrict__ noise_g, const uint8_t* __restrict__ mask,
                                                       const int64_t* __restrict__ counts, const int64_t* __restrict__ t,
                                                       const float* __restrict__ sa, const float* __restrict__ sb, int64_t inner,
                                                       int pmax, int c, int T) {
    static_assert(GIVEN == GIVEN_ROWS || GIVEN == GIVEN_MASK, "an overwrite needs a given part");
    const int b = blockIdx.y;
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;                                  // one count per out-of-range scene
    const int64_t tv = dsc_checked_index(t[b], T, first);
    const float a = sa[tv], s = sb[tv];
    int64_t cnt = inner;
    if constexpr (GIVEN == GIVEN_ROWS) cnt = (counts ? dsc_checked_index(counts[b], (int64_t)pmax + 1, first) : (int64_t)pmax) * c;
    const int64_t base = (int64_t)b * inner;
    const int64_t gbase = GIVEN == GIVEN_ROWS ? (int64_t)b * pmax * c : base;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * blockDim.x) {
        if constexpr (GIVEN == GIVEN_MASK) {
            if (!mask[base + i]) continue;
        }
        x[base + i] = renoise(given[gbase + i], noise_g[gbase + i], a, s);
    }
}

// The resampling jump of the completion and in-painting loops (RePaint): after the step that leaves the state at
// remaining index s, the whole state is diffused forward by j steps in one draw, x = ja[pos] * x + jb[pos] * noise, and the loop walks
// the stretch down again.  ja / jb are host tables (float64, rounded once) of sqrt(abar[time(s + j)] / abar[time(s)]) and its
// complement, indexed by the position the move of the step has left: the scene's own t[b] = s (T-step), or the step counter
// k = step[0] (strided; the target pair is k - j).  In place.
//   GIVEN none:  every element takes the jump -- dsc_q_sample_f32 on (ja, jb) at t = s.  The eager loops and the unfused graphs.
//         rows / mask:  a given element takes what the overwrite in front of the next model call would write,
//                q_sample(given, time(s + j), noise_g): the jump and that overwrite in one launch, bit-identical to their composition.
// Read sets as in step_kernel: a given element reads mask (nothing, for rows), given and noise_g only, a free one mask, x and noise
// only.  x_dup (may be NULL) receives a second copy of every written element (the null half of a guided loop's state).
// Bad indices: t[b], t[b] + j and counts[b] once per scene; step[0], step[0] - j and times[.] once per launch; the target is looked up
// only where a given part exists.
// Width: a scene's base is b * inner floats and inner is N * C -- 12 * 62, 21 * 65, 21 * 62: mostly off the 16-byte grid, as in
// scene_noise_kernel's per_scene % 4 != 0 case -- so every lane moves one dword and a wave covers 256 contiguous bytes per operand; the
// launch moves four floats per element and is latency at the loops' sizes, a dwordx4 form for the aligned shapes would buy nothing.
template <bool STRIDED, int GIVEN>
__global__ __launch_bounds__(256) void jump_kernel(float* x, const float* __restrict__ noise, const float* __restrict__ ja,
                                                  const float* __restrict__ jb, const int64_t* __restrict__ t,
                                                  const int64_t* __restrict__ step, const int64_t* __restrict__ times,
                                                  const float* __restrict__ given, const float* __restrict__ noise_g,
                                                  const uint8_t* __restrict__ mask, const int64_t* __restrict__ counts,
                                                  const float* __restrict__ sa, const float* __restrict__ sb, float* __restrict__ x_dup,
                                                  int jump, int64_t inner, int pmax, int c, int S, int T) {
    constexpr bool HAS_GIVEN = GIVEN != GIVEN_NONE;
    const int b = blockIdx.y;
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    int64_t pos, target = 0;
    if constexpr (STRIDED) {
        pos = dsc_checked_index(step[0], S, first && b == 0);
        if constexpr (HAS_GIVEN) target = dsc_checked_index(times[dsc_checked_index(pos - jump, S, first && b == 0)], T, first && b == 0);
    } else {
        pos = dsc_checked_index(t[b], T, first);
        if constexpr (HAS_GIVEN) target = dsc_checked_index(pos + jump, T, first);
    }
    const float a = ja[pos], s = jb[pos];
    Renoise r{};
    if constexpr (HAS_GIVEN) r = renoise_coef(true, target, sa, sb);
    int64_t cnt = 0;
    if constexpr (GIVEN == GIVEN_ROWS) cnt = dsc_checked_index(counts[b], (int64_t)pmax + 1, first) * c;
    const int64_t base = (int64_t)b * inner;
    const int64_t gbase = GIVEN == GIVEN_ROWS ? (int64_t)b * pmax * c : base;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < inner; i += (int64_t)gridDim.x * blockDim.x) {
        bool is_given = false;
        if constexpr (GIVEN == GIVEN_ROWS) is_given = i < cnt;
        if constexpr (GIVEN == GIVEN_MASK) is_given = mask[base + i] != 0;
        float y;
        if (is_given) y = renoise(given[gbase + i], noise_g[gbase + i], r.a, r.s);
        else y = renoise(x[base + i], noise[base + i], a, s);
        x[base + i] = y;
        if (x_dup) x_dup[base + i] = y;
    }
}

// The move after a jump in a strided loop, the seek form of ddim_advance_kernel: step += delta, then t[i] = times[step].  One block:
// every thread reads the counter before thread 0 stores it.
__global__ __launch_bounds__(256) void ddim_seek_kernel(int64_t* step, const int64_t* __restrict__ times, int64_t* __restrict__ t,
                                                       int count, int S, int64_t delta) {
    const int64_t k = dsc_checked_index(step[0] + delta, S, threadIdx.x == 0);
    __syncthreads();
    if (threadIdx.x == 0) step[0] = k;
    const int64_t tv = times[k];
    for (int i = threadIdx.x; i < count; i += blockDim.x) t[i] = tv;
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

// The operands of step_kernel under its parameter names; an entry point fills what its instantiation reads and leaves the rest null.
// rows: n, pmax, c describe the scene (inner = n * c); otherwise inner does.
struct StepArgs {
    const float *xt, *mo, *scale, *noise, *given, *noise_g;
    const uint8_t* mask;
    const int64_t *counts, *t, *step, *times, *times_next;
    const float *sqrt_an, *cnoise, *sigma, *ca, *cb, *c1, *c2, *ra, *rm, *sa, *sb;
    float *out, *x_dup, *x0_out;
    int32_t mean_type, clip, b;
    int64_t inner;
    int32_t n, pmax, c, S, T;
};

// The argument checks and the launch of every step.  Required: the operands of the free branch, the tables of the axis values and
// ca / cb as bad_mean_args says; x_dup and x0_out may be null.  blockIdx.y carries the scene: b <= 65535.
template <bool STRIDED, int GIVEN, bool GUIDED>
int launch_step(const StepArgs& a, dsc_stream_t stream) {
    static_assert(!(GIVEN == GIVEN_ROWS && GUIDED), "guided completion has no caller: not instantiated");
    constexpr bool HAS_GIVEN = GIVEN != GIVEN_NONE;
    if (!a.xt || !a.mo || !a.noise || !a.sigma || !a.out || a.b < 1 || a.T < 1) return DSC_EINVAL;
    if (STRIDED ? !a.step || !a.times || !a.times_next || !a.sqrt_an || !a.cnoise || !a.ra || !a.rm || a.S < 1 : !a.t || !a.c1 || !a.c2)
        return DSC_EINVAL;
    if (HAS_GIVEN && (!a.given || !a.noise_g || !a.sa || !a.sb)) return DSC_EINVAL;
    if (GIVEN == GIVEN_ROWS ? !a.counts || a.n < 1 || a.pmax < 1 || a.pmax > a.n || a.c < 1 : a.inner < 1) return DSC_EINVAL;
    if ((GIVEN == GIVEN_MASK && !a.mask) || (GUIDED && !a.scale)) return DSC_EINVAL;
    if (bad_mean_args(a.mean_type, a.ca, a.cb)) return DSC_EINVAL;
    if (a.b > 65535) return DSC_ERANGE;
    const int64_t inner = GIVEN == GIVEN_ROWS ? (int64_t)a.n * a.c : a.inner;
    DSC_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL((step_kernel<STRIDED, GIVEN, GUIDED>), dim3(grid_x(inner), a.b), dim3(256), 0, static_cast<hipStream_t>(stream),
                       a.xt, a.mo, a.scale, a.noise, a.given, a.noise_g, a.mask, a.counts, a.t, a.step, a.times, a.times_next, a.sqrt_an,
                       a.cnoise, a.sigma, a.ca, a.cb, a.c1, a.c2, a.ra, a.rm, a.sa, a.sb, a.out, a.x_dup, a.x0_out, a.mean_type, a.clip,
                       inner, a.pmax, a.c, a.S, a.T);
    DSC_LAUNCH_CHECK();
    return 0;
}

// The same for the three overwrites; counts is required by the ragged entry point alone, which checks it.
template <int GIVEN>
int launch_overwrite(float* x, const float* given, const float* noise_g, const uint8_t* mask, const int64_t* counts, const int64_t* t,
                     const float* sa, const float* sb, int32_t b, int64_t inner, int32_t n, int32_t pmax, int32_t c, int32_t T,
                     dsc_stream_t stream) {
    if (!x || !given || !noise_g || !t || !sa || !sb || b < 1 || T < 1) return DSC_EINVAL;
    if (GIVEN == GIVEN_ROWS ? n < 1 || pmax < 1 || pmax > n || c < 1 : !mask || inner < 1) return DSC_EINVAL;
    if (b > 65535) return DSC_ERANGE;
    if (GIVEN == GIVEN_ROWS) inner = (int64_t)n * c;
    const int64_t covered = GIVEN == GIVEN_ROWS ? (int64_t)pmax * c : inner;
    DSC_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL((overwrite_kernel<GIVEN>), dim3(grid_x(covered), b), dim3(256), 0, static_cast<hipStream_t>(stream),
                       x, given, noise_g, mask, counts, t, sa, sb, inner, pmax, c, T);
    DSC_LAUNCH_CHECK();
    return 0;
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
    StepArgs a{};
    a.xt = x_t, a.mo = model_out, a.noise = noise, a.out = out, a.x0_out = x0_out;
    a.t = t, a.ca = ca, a.cb = cb, a.c1 = coef1, a.c2 = coef2, a.sigma = sigma;
    a.mean_type = mean_type, a.clip = clip, a.b = b, a.inner = inner, a.T = num_timesteps;
    return launch_step<false, GIVEN_NONE, false>(a, stream);
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
    StepArgs a{};
    a.xt = x_t, a.mo = model_out, a.noise = noise, a.out = out, a.x0_out = x0_out;
    a.step = step, a.times = times, a.times_next = times_next, a.sqrt_an = sqrt_alpha_next, a.cnoise = c_noise, a.sigma = sigma;
    a.ca = ca, a.cb = cb, a.ra = sqrt_recip_ac, a.rm = sqrt_recipm1_ac;
    a.mean_type = mean_type, a.b = b, a.inner = inner, a.S = num_steps, a.T = num_timesteps;
    return launch_step<true, GIVEN_NONE, false>(a, stream);
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
    return launch_overwrite<GIVEN_ROWS>(x, partial, noise, nullptr, nullptr, t, sqrt_ac, sqrt_1mac, b, 0, n, p, c, num_timesteps, stream);
}

extern "C" int dsc_complete_overwrite_ragged_f32(float* x, const float* partial, const float* noise, const int64_t* counts,
                                                 const int64_t* t, const float* sqrt_ac, const float* sqrt_1mac, int32_t b,
                                                 int32_t n, int32_t pmax, int32_t c, int32_t num_timesteps, dsc_stream_t stream) {
    if (!counts) return DSC_EINVAL;
    return launch_overwrite<GIVEN_ROWS>(x, partial, noise, nullptr, counts, t, sqrt_ac, sqrt_1mac, b, 0, n, pmax, c, num_timesteps, stream);
}

extern "C" int dsc_masked_overwrite_f32(float* x, const float* known, const float* noise, const uint8_t* mask, const int64_t* t,
                                        const float* sqrt_ac, const float* sqrt_1mac, int32_t b, int64_t inner,
                                        int32_t num_timesteps, dsc_stream_t stream) {
    return launch_overwrite<GIVEN_MASK>(x, known, noise, mask, nullptr, t, sqrt_ac, sqrt_1mac, b, inner, 0, 0, 0, num_timesteps, stream);
}

extern "C" int dsc_p_sample_inpaint_f32(const float* x_t, const float* model_out, const float* noise, const float* partial,
                                        const float* noise_p, const int64_t* counts, const int64_t* t, const float* ca,
                                        const float* cb, const float* coef1, const float* coef2, const float* sigma,
                                        const float* sqrt_ac, const float* sqrt_1mac, float* out, int32_t mean_type, int32_t clip,
                                        int32_t b, int32_t n, int32_t pmax, int32_t c, int32_t num_timesteps, dsc_stream_t stream) {
    StepArgs a{};
    a.xt = x_t, a.mo = model_out, a.noise = noise, a.out = out;
    a.given = partial, a.noise_g = noise_p, a.counts = counts, a.sa = sqrt_ac, a.sb = sqrt_1mac;
    a.t = t, a.ca = ca, a.cb = cb, a.c1 = coef1, a.c2 = coef2, a.sigma = sigma;
    a.mean_type = mean_type, a.clip = clip, a.b = b, a.n = n, a.pmax = pmax, a.c = c, a.T = num_timesteps;
    return launch_step<false, GIVEN_ROWS, false>(a, stream);
}

extern "C" int dsc_ddim_inpaint_step_f32(const float* x_t, const float* model_out, const float* noise, const float* partial,
                                         const float* noise_p, const int64_t* counts, const int64_t* step, const int64_t* times,
                                         const int64_t* times_next, const float* sqrt_alpha_next, const float* c_noise,
                                         const float* sigma, const float* ca, const float* cb, const float* sqrt_recip_ac,
                                         const float* sqrt_recipm1_ac, const float* sqrt_ac, const float* sqrt_1mac, float* out,
                                         int32_t mean_type, int32_t b, int32_t n, int32_t pmax, int32_t c, int32_t num_steps,
                                         int32_t num_timesteps, dsc_stream_t stream) {
    StepArgs a{};
    a.xt = x_t, a.mo = model_out, a.noise = noise, a.out = out;
    a.given = partial, a.noise_g = noise_p, a.counts = counts, a.sa = sqrt_ac, a.sb = sqrt_1mac;
    a.step = step, a.times = times, a.times_next = times_next, a.sqrt_an = sqrt_alpha_next, a.cnoise = c_noise, a.sigma = sigma;
    a.ca = ca, a.cb = cb, a.ra = sqrt_recip_ac, a.rm = sqrt_recipm1_ac;
    a.mean_type = mean_type, a.b = b, a.n = n, a.pmax = pmax, a.c = c, a.S = num_steps, a.T = num_timesteps;
    return launch_step<true, GIVEN_ROWS, false>(a, stream);
}

extern "C" int dsc_p_sample_masked_f32(const float* x_t, const float* model_out, const float* noise, const float* known,
                                       const float* noise_k, const uint8_t* mask, const int64_t* t, const float* ca, const float* cb,
                                       const float* coef1, const float* coef2, const float* sigma, const float* sqrt_ac,
                                       const float* sqrt_1mac, float* out, int32_t mean_type, int32_t clip, int32_t b, int64_t inner,
                                       int32_t num_timesteps, dsc_stream_t stream) {
    StepArgs a{};
    a.xt = x_t, a.mo = model_out, a.noise = noise, a.out = out;
    a.given = known, a.noise_g = noise_k, a.mask = mask, a.sa = sqrt_ac, a.sb = sqrt_1mac;
    a.t = t, a.ca = ca, a.cb = cb, a.c1 = coef1, a.c2 = coef2, a.sigma = sigma;
    a.mean_type = mean_type, a.clip = clip, a.b = b, a.inner = inner, a.T = num_timesteps;
    return launch_step<false, GIVEN_MASK, false>(a, stream);
}

extern "C" int dsc_ddim_masked_step_f32(const float* x_t, const float* model_out, const float* noise, const float* known,
                                        const float* noise_k, const uint8_t* mask, const int64_t* step, const int64_t* times,
                                        const int64_t* times_next, const float* sqrt_alpha_next, const float* c_noise,
                                        const float* sigma, const float* ca, const float* cb, const float* sqrt_recip_ac,
                                        const float* sqrt_recipm1_ac, const float* sqrt_ac, const float* sqrt_1mac, float* out,
                                        int32_t mean_type, int32_t b, int64_t inner, int32_t num_steps, int32_t num_timesteps,
                                        dsc_stream_t stream) {
    StepArgs a{};
    a.xt = x_t, a.mo = model_out, a.noise = noise, a.out = out;
    a.given = known, a.noise_g = noise_k, a.mask = mask, a.sa = sqrt_ac, a.sb = sqrt_1mac;
    a.step = step, a.times = times, a.times_next = times_next, a.sqrt_an = sqrt_alpha_next, a.cnoise = c_noise, a.sigma = sigma;
    a.ca = ca, a.cb = cb, a.ra = sqrt_recip_ac, a.rm = sqrt_recipm1_ac;
    a.mean_type = mean_type, a.b = b, a.inner = inner, a.S = num_steps, a.T = num_timesteps;
    return launch_step<true, GIVEN_MASK, false>(a, stream);
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
    StepArgs a{};
    a.xt = x_t, a.mo = model_out, a.scale = scale, a.noise = noise, a.out = out, a.x_dup = x_dup, a.x0_out = x0_out;
    a.t = t, a.ca = ca, a.cb = cb, a.c1 = coef1, a.c2 = coef2, a.sigma = sigma;
    a.mean_type = mean_type, a.clip = clip, a.b = b, a.inner = inner, a.T = num_timesteps;
    return launch_step<false, GIVEN_NONE, true>(a, stream);
}

extern "C" int dsc_ddim_cfg_step_f32(const float* x_t, const float* model_out, const float* scale, const float* noise,
                                     const int64_t* step, const int64_t* times, const int64_t* times_next,
                                     const float* sqrt_alpha_next, const float* c_noise, const float* sigma, const float* ca,
                                     const float* cb, const float* sqrt_recip_ac, const float* sqrt_recipm1_ac, float* out,
                                     float* x_dup, float* x0_out, int32_t mean_type, int32_t b, int64_t inner, int32_t num_steps,
                                     int32_t num_timesteps, dsc_stream_t stream) {
    StepArgs a{};
    a.xt = x_t, a.mo = model_out, a.scale = scale, a.noise = noise, a.out = out, a.x_dup = x_dup, a.x0_out = x0_out;
    a.step = step, a.times = times, a.times_next = times_next, a.sqrt_an = sqrt_alpha_next, a.cnoise = c_noise, a.sigma = sigma;
    a.ca = ca, a.cb = cb, a.ra = sqrt_recip_ac, a.rm = sqrt_recipm1_ac;
    a.mean_type = mean_type, a.b = b, a.inner = inner, a.S = num_steps, a.T = num_timesteps;
    return launch_step<true, GIVEN_NONE, true>(a, stream);
}

extern "C" int dsc_p_sample_masked_cfg_f32(const float* x_t, const float* model_out, const float* scale, const float* noise,
                                           const float* known, const float* noise_k, const uint8_t* mask, const int64_t* t,
                                           const float* ca, const float* cb, const float* coef1, const float* coef2, const float* sigma,
                                           const float* sqrt_ac, const float* sqrt_1mac, float* out, float* x_dup, int32_t mean_type,
                                           int32_t clip, int32_t b, int64_t inner, int32_t num_timesteps, dsc_stream_t stream) {
    StepArgs a{};
    a.xt = x_t, a.mo = model_out, a.scale = scale, a.noise = noise, a.out = out, a.x_dup = x_dup;
    a.given = known, a.noise_g = noise_k, a.mask = mask, a.sa = sqrt_ac, a.sb = sqrt_1mac;
    a.t = t, a.ca = ca, a.cb = cb, a.c1 = coef1, a.c2 = coef2, a.sigma = sigma;
    a.mean_type = mean_type, a.clip = clip, a.b = b, a.inner = inner, a.T = num_timesteps;
    return launch_step<false, GIVEN_MASK, true>(a, stream);
}

extern "C" int dsc_ddim_masked_cfg_step_f32(const float* x_t, const float* model_out, const float* scale, const float* noise,
                                            const float* known, const float* noise_k, const uint8_t* mask, const int64_t* step,
                                            const int64_t* times, const int64_t* times_next, const float* sqrt_alpha_next,
                                            const float* c_noise, const float* sigma, const float* ca, const float* cb,
                                            const float* sqrt_recip_ac, const float* sqrt_recipm1_ac, const float* sqrt_ac,
                                            const float* sqrt_1mac, float* out, float* x_dup, int32_t mean_type, int32_t b,
                                            int64_t inner, int32_t num_steps, int32_t num_timesteps, dsc_stream_t stream) {
    StepArgs a{};
    a.xt = x_t, a.mo = model_out, a.scale = scale, a.noise = noise, a.out = out, a.x_dup = x_dup;
    a.given = known, a.noise_g = noise_k, a.mask = mask, a.sa = sqrt_ac, a.sb = sqrt_1mac;
    a.step = step, a.times = times, a.times_next = times_next, a.sqrt_an = sqrt_alpha_next, a.cnoise = c_noise, a.sigma = sigma;
    a.ca = ca, a.cb = cb, a.ra = sqrt_recip_ac, a.rm = sqrt_recipm1_ac;
    a.mean_type = mean_type, a.b = b, a.inner = inner, a.S = num_steps, a.T = num_timesteps;
    return launch_step<true, GIVEN_MASK, true>(a, stream);
}

// The checks and operands both steering launches share: DSC_EINVAL cases first, then DSC_ERANGE.
static int fill_steer_args(SteerArgs& p, const float* x_t, float* model_out, const int64_t* t, const int64_t* step, const int64_t* times,
                           const float* ca, const float* cb, const float* partial, const int64_t* counts, const float* known,
                           const uint8_t* mask, const float* cfg_scale, const float* weight, const int64_t* t_below, const float* bounds,
                           float* energy_out, float* grad_out, int32_t mean_type, int32_t b, int32_t n, int32_t pmax, int32_t c,
                           int32_t bbox_dim, int32_t class_dim, int32_t num_steps, int32_t num_timesteps) {
    if (!model_out || !weight || !t_below || !bounds || b < 1 || n < 1 || c < 1 || num_timesteps < 1) return DSC_EINVAL;
    if (t ? step || times : !step || !times || num_steps < 1) return DSC_EINVAL;            // one time source
    if (bad_mean_args(mean_type, ca, cb) || (mean_type != DSC_MEAN_X0 && !x_t)) return DSC_EINVAL;
    if ((partial != nullptr) != (counts != nullptr) || (known != nullptr) != (mask != nullptr) || (partial && known)) return DSC_EINVAL;
    if (partial && (pmax < 1 || pmax > n)) return DSC_EINVAL;
    if (class_dim < 1 || bbox_dim < 1 || bbox_dim + class_dim > c) return DSC_EINVAL;        // a re-arrangement sub-shape has no such layout
    if (bbox_dim != 8 || n > STEER_MAXN) return DSC_ERANGE;                                  // [translation 3 | size 3 | cos, sin]
    p.xt = x_t, p.mo = model_out, p.t = t, p.step = step, p.times = times, p.ca = ca, p.cb = cb;
    p.partial = partial, p.counts = counts, p.known = known, p.mask = mask, p.scale = cfg_scale, p.weight = weight, p.t_below = t_below;
    p.energy = energy_out, p.grad = grad_out;
    p.mean_type = mean_type, p.b = b, p.n = n, p.pmax = partial ? pmax : 0, p.c = c, p.empty_col = bbox_dim + class_dim - 1;
    p.S = t ? 0 : num_steps, p.T = num_timesteps;
    for (int k = 0; k < 3; ++k) {
        p.c_lo[k] = bounds[k], p.c_span[k] = (double)bounds[3 + k] - (double)bounds[k];
        p.s_lo[k] = bounds[6 + k], p.s_span[k] = (double)bounds[9 + k] - (double)bounds[6 + k];
    }
    return 0;
}

extern "C" int dsc_steer_boxes_f32(const float* x_t, float* model_out, const int64_t* t, const int64_t* step, const int64_t* times,
                                   const float* ca, const float* cb, const float* partial, const int64_t* counts, const float* known,
                                   const uint8_t* mask, const float* cfg_scale, const float* weight, const int64_t* t_below,
                                   const float* bounds, float* energy_out, float* grad_out, int32_t mean_type, int32_t b, int32_t n,
                                   int32_t pmax, int32_t c, int32_t bbox_dim, int32_t class_dim, int32_t num_steps,
                                   int32_t num_timesteps, dsc_stream_t stream) {
    SteerArgs p{};
    if (const int rc = fill_steer_args(p, x_t, model_out, t, step, times, ca, cb, partial, counts, known, mask, cfg_scale, weight, t_below,
                                       bounds, energy_out, grad_out, mean_type, b, n, pmax, c, bbox_dim, class_dim, num_steps,
                                       num_timesteps))
        return rc;
    DSC_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL(steer_boxes_kernel, dim3(b), dim3(256), 0, static_cast<hipStream_t>(stream), p);
    DSC_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsc_floor_field_f32(const float* mask, float* field, int32_t b, int32_t h, int32_t w, float room_side,
                                   dsc_stream_t stream) {
    if (!mask || !field || b < 1 || !(room_side > 0.f) || !(room_side < INFINITY)) return DSC_EINVAL;
    if (h < 2 || w < 2 || h > WALL_MAXHW || w > WALL_MAXHW || b > 65535) return DSC_ERANGE;
    DSC_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL(floor_field_kernel, dim3(h, b), dim3(256), 0, static_cast<hipStream_t>(stream), mask, field, h, w, room_side);
    DSC_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsc_steer_walls_f32(const float* x_t, float* model_out, const int64_t* t, const int64_t* step, const int64_t* times,
                                   const float* ca, const float* cb, const float* partial, const int64_t* counts, const float* known,
                                   const uint8_t* mask, const float* cfg_scale, const float* weight, const int64_t* t_below,
                                   const float* bounds, const float* field, const float* room_side, float* energy_out, float* grad_out,
                                   int32_t* outside_out, int32_t mean_type, int32_t b, int32_t n, int32_t pmax, int32_t c,
                                   int32_t bbox_dim, int32_t class_dim, int32_t num_steps, int32_t num_timesteps, int32_t field_b,
                                   int32_t h, int32_t w, dsc_stream_t stream) {
    // Its own DSC_EINVAL cases come before the shared DSC_ERANGE ones, its own DSC_ERANGE cases after.
    if (!field || !room_side || (field_b != 1 && field_b != b)) return DSC_EINVAL;
    WallArgs p{};
    if (const int rc = fill_steer_args(p.s, x_t, model_out, t, step, times, ca, cb, partial, counts, known, mask, cfg_scale, weight,
                                       t_below, bounds, energy_out, grad_out, mean_type, b, n, pmax, c, bbox_dim, class_dim, num_steps,
                                       num_timesteps))
        return rc;
    if (h < 2 || w < 2 || h > WALL_MAXHW || w > WALL_MAXHW) return DSC_ERANGE;
    p.field = field, p.room_side = room_side, p.outside = outside_out, p.field_b = field_b, p.h = h, p.w = w;
    DSC_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL(steer_walls_kernel, dim3(b), dim3(256), 0, static_cast<hipStream_t>(stream), p);
    DSC_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsc_multistep_x0_f32(const float* x_t, float* model_out, float* hist, const float* weights, const int64_t* step,
                                    const int64_t* times, const float* ca, const float* cb, const float* cfg_scale,
                                    const int64_t* counts, const uint8_t* mask, int32_t mean_type, int32_t b, int64_t inner,
                                    int32_t pmax, int32_t c, int32_t num_steps, int32_t num_timesteps, dsc_stream_t stream) {
    if (!model_out || !hist || !weights || !step || !times || b < 1 || inner < 1 || num_steps < 1 || num_timesteps < 1) return DSC_EINVAL;
    if (bad_mean_args(mean_type, ca, cb) || (mean_type != DSC_MEAN_X0 && !x_t)) return DSC_EINVAL;
    if (counts && mask) return DSC_EINVAL;                                                   // one given part
    if (counts && (c < 1 || pmax < 1 || inner % c != 0 || (int64_t)pmax * c > inner)) return DSC_EINVAL;
    if (b > 65535) return DSC_ERANGE;                                                        // blockIdx.y carries the scene
    const dim3 grid(grid_x(inner), b), block(256);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    DSC_CLEAR_STALE_ERROR();
#define DSC_MULTISTEP_LAUNCH(GIVEN, GUIDED)                                                                                       \
    hipLaunchKernelGGL((multistep_x0_kernel<GIVEN, GUIDED>), grid, block, 0, s, x_t, model_out, hist, weights, step, times, ca, cb, \
                       cfg_scale, counts, mask, mean_type, inner, pmax, c, num_steps, num_timesteps)
    if (counts) {
        if (cfg_scale) DSC_MULTISTEP_LAUNCH(GIVEN_ROWS, true); else DSC_MULTISTEP_LAUNCH(GIVEN_ROWS, false);
    } else if (mask) {
        if (cfg_scale) DSC_MULTISTEP_LAUNCH(GIVEN_MASK, true); else DSC_MULTISTEP_LAUNCH(GIVEN_MASK, false);
    } else {
        if (cfg_scale) DSC_MULTISTEP_LAUNCH(GIVEN_NONE, true); else DSC_MULTISTEP_LAUNCH(GIVEN_NONE, false);
    }
#undef DSC_MULTISTEP_LAUNCH
    DSC_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsc_resample_jump_f32(float* x, const float* noise, const float* ja, const float* jb, const int64_t* t,
                                     const int64_t* step, const int64_t* times, const float* given, const float* noise_g,
                                     const uint8_t* mask, const int64_t* counts, const float* sqrt_ac, const float* sqrt_1mac,
                                     float* x_dup, int32_t jump, int32_t b, int64_t inner, int32_t pmax, int32_t c, int32_t num_steps,
                                     int32_t num_timesteps, dsc_stream_t stream) {
    if (!x || !noise || !ja || !jb || jump < 1 || b < 1 || inner < 1 || num_timesteps < 1) return DSC_EINVAL;
    if (t ? step || times : !step || !times || num_steps < 1) return DSC_EINVAL;            // one time source
    if (counts && mask) return DSC_EINVAL;                                                   // one given part
    if (given ? !noise_g || !sqrt_ac || !sqrt_1mac || (!counts && !mask) : noise_g || counts || mask) return DSC_EINVAL;
    if (counts && (c < 1 || pmax < 1 || inner % c != 0 || (int64_t)pmax * c > inner)) return DSC_EINVAL;
    if (b > 65535) return DSC_ERANGE;                                                        // blockIdx.y carries the scene
    const dim3 grid(grid_x(inner), b), block(256);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    DSC_CLEAR_STALE_ERROR();
#define DSC_JUMP_LAUNCH(STRIDED, GIVEN)                                                                                            \
    hipLaunchKernelGGL((jump_kernel<STRIDED, GIVEN>), grid, block, 0, s, x, noise, ja, jb, t, step, times, given, noise_g, mask, counts, \
                       sqrt_ac, sqrt_1mac, x_dup, jump, inner, pmax, c, num_steps, num_timesteps)
    if (t) {
        if (counts) DSC_JUMP_LAUNCH(false, GIVEN_ROWS); else if (mask) DSC_JUMP_LAUNCH(false, GIVEN_MASK); else DSC_JUMP_LAUNCH(false, GIVEN_NONE);
    } else {
        if (counts) DSC_JUMP_LAUNCH(true, GIVEN_ROWS); else if (mask) DSC_JUMP_LAUNCH(true, GIVEN_MASK); else DSC_JUMP_LAUNCH(true, GIVEN_NONE);
    }
#undef DSC_JUMP_LAUNCH
    DSC_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsc_ddim_seek_i64(int64_t* step, const int64_t* times, int64_t* t, int32_t count, int32_t num_steps, int64_t delta,
                                 dsc_stream_t stream) {
    if (!step || !times || !t || count < 1 || num_steps < 1) return DSC_EINVAL;
    DSC_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL(ddim_seek_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), step, times, t, count, num_steps,
                       delta);
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
