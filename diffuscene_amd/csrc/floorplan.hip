// Floor-plan encoder (ResNet-18 on the room mask, networks/feature_extractors.py): the byte movers around its GEMMs.
//
// Activations are channel-last, token-major [b * h * w][c] -- the layout of every GEMM operand of this library; a (B, 1, H, W) mask
// already is in it.  A convolution is  patch gather -> dsc_gemm_f32 -> dsc_frozen_bn_act_f32, its backward  dsc_gemm_f32 on W^T ->
// dsc_conv_patches_bwd_f32  and  dsc_gemm_tn_f32 on the re-gathered patches.
//
// Every kernel here is a GATHER: one thread owns an output element (or four consecutive channels of it) and reads whatever feeds it, in
// a fixed order.  No atomics, no scatter: the results are deterministic for a shape.  All element offsets are int64 (rows x K reaches
// 3e8 at the largest accepted shape); row COUNTS fit int32 and are checked on the host, so the index decode inside a block is 32-bit.
//
// Vector width: lanes walk the channel dimension, which is contiguous.  With c % 4 == 0 and 16-byte aligned bases every access is one
// dwordx4 per lane (1 KiB per wave instruction); any other channel count or alignment (the 1- or 2-channel mask in front of conv1) runs
// the same kernel one dword per lane.
//
// Arithmetic: everything that is summed or scaled here is evaluated in float64 registers and rounded to float32 once, when it is
// stored -- these kernels wait for memory, the wider arithmetic is free, and the encoder's error is then that of its GEMMs alone.
// Compiled with -ffp-contract=off: the expressions below are the roundings the tests count.
#include "dsc_common.h"

namespace {

constexpr int kThreads = 256;

template <int V> struct vecf { float v[V]; };

template <int V> __device__ __forceinline__ vecf<V> ldv(const float* p) {
    vecf<V> r;
    if constexpr (V == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p);
        r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
    } else {
        r.v[0] = *p;
    }
    return r;
}
template <int V> __device__ __forceinline__ void stv(float* p, const vecf<V>& a) {
    if constexpr (V == 4) {
        f32x4 t; t.x = a.v[0]; t.y = a.v[1]; t.z = a.v[2]; t.w = a.v[3];
        *reinterpret_cast<f32x4*>(p) = t;
    } else {
        *p = a.v[0];
    }
}
template <int V> __device__ __forceinline__ vecf<V> zerov() {
    vecf<V> r;
#pragma unroll
    for (int q = 0; q < V; ++q) r.v[q] = 0.0f;
    return r;
}

struct conv_geom {
    int h, w, c, k, stride, pad, ho, wo, kk, kpad;     // kk = k * k * c, kpad = kk rounded up to 32
};

// patches[row][(ky * k + kx) * c + ch] = x[b][oy * stride - pad + ky][ox * stride - pad + kx][ch] (0 outside the image), columns
// [kk, kpad) = 0.  A block owns `rpb` consecutive patch rows, i.e. one contiguous piece of the output.
template <int V>
__global__ __launch_bounds__(kThreads) void conv_patches_kernel(const float* __restrict__ x, float* __restrict__ patches, conv_geom g,
                                                                int rows, int rpb) {
    const int kpv = g.kpad / V;
    const int row0 = (int)((int64_t)blockIdx.x * rpb);
    const int nrow = min(rpb, rows - row0);
    const int total = nrow * kpv;
    for (int e = threadIdx.x; e < total; e += kThreads) {
        const int r = e / kpv, col = (e - r * kpv) * V;
        const int row = row0 + r;
        vecf<V> out = zerov<V>();
        if (col < g.kk) {
            const int tap = col / g.c, ch = col - tap * g.c;
            const int ky = tap / g.k, kx = tap - ky * g.k;
            const int bo = row / g.wo, ox = row - bo * g.wo;
            const int b = bo / g.ho, oy = bo - b * g.ho;
            const int iy = oy * g.stride - g.pad + ky, ix = ox * g.stride - g.pad + kx;
            if (iy >= 0 && iy < g.h && ix >= 0 && ix < g.w)
                out = ldv<V>(x + (((int64_t)b * g.h + iy) * g.w + ix) * g.c + ch);
        }
        stv<V>(patches + (int64_t)row * g.kpad + col, out);
    }
}

// dx[b][iy][ix][ch] = sum over the taps (ky, kx), ky-major, of the patch entries that read this element: patch row (b, oy, ox) with
// oy * stride - pad + ky == iy (and the same in x), column (ky * k + kx) * c + ch.  At most k * k terms, added in that order in
// float64 and rounded once.
template <int V>
__global__ __launch_bounds__(kThreads) void conv_patches_bwd_kernel(const float* __restrict__ dp, float* __restrict__ dx, conv_geom g,
                                                                    int pixels, int ppb) {
    const int cv = g.c / V;
    const int pix0 = (int)((int64_t)blockIdx.x * ppb);
    const int npix = min(ppb, pixels - pix0);
    const int total = npix * cv;
    const int hw = g.h * g.w;
    for (int e = threadIdx.x; e < total; e += kThreads) {
        const int pl = e / cv, ch = (e - pl * cv) * V;
        const int pix = pix0 + pl;
        const int b = pix / hw, rem = pix - b * hw;
        const int iy = rem / g.w, ix = rem - iy * g.w;
        double acc[V];
#pragma unroll
        for (int q = 0; q < V; ++q) acc[q] = 0.0;
        for (int ky = 0; ky < g.k; ++ky) {
            const int ty = iy + g.pad - ky;
            if (ty < 0) break;
            const int oy = ty / g.stride;
            if (oy * g.stride != ty || oy >= g.ho) continue;
            for (int kx = 0; kx < g.k; ++kx) {
                const int tx = ix + g.pad - kx;
                if (tx < 0) break;
                const int ox = tx / g.stride;
                if (ox * g.stride != tx || ox >= g.wo) continue;
                const vecf<V> t = ldv<V>(dp + (((int64_t)b * g.ho + oy) * g.wo + ox) * g.kpad + (ky * g.k + kx) * g.c + ch);
#pragma unroll
                for (int q = 0; q < V; ++q) acc[q] = acc[q] + (double)t.v[q];
            }
        }
        vecf<V> out;
#pragma unroll
        for (int q = 0; q < V; ++q) out.v[q] = (float)acc[q];
        stv<V>(dx + (int64_t)pix * g.c + ch, out);
    }
}

// 3 x 3, stride 2, padding 1 max pooling.  The window is walked row-major over its in-image positions only (padding never wins); a
// later value replaces the running maximum only when it is greater (or NaN), so among equal maxima the first wins, and the slot
// ky * 3 + kx of the winner is stored -- torch.nn.functional.max_pool2d's choice.
template <int V>
__global__ __launch_bounds__(kThreads) void maxpool_kernel(const float* __restrict__ x, float* __restrict__ y, uint8_t* __restrict__ arg,
                                                           int h, int w, int c, int ho, int wo, int rows, int rpb) {
    const int cv = c / V;
    const int row0 = (int)((int64_t)blockIdx.x * rpb);
    const int nrow = min(rpb, rows - row0);
    const int total = nrow * cv;
    for (int e = threadIdx.x; e < total; e += kThreads) {
        const int r = e / cv, ch = (e - r * cv) * V;
        const int row = row0 + r;
        const int bo = row / wo, ox = row - bo * wo;
        const int b = bo / ho, oy = bo - b * ho;
        vecf<V> best;
        int slot[V];
        bool first = true;
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = oy * 2 - 1 + ky;
            if (iy < 0 || iy >= h) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = ox * 2 - 1 + kx;
                if (ix < 0 || ix >= w) continue;
                const vecf<V> t = ldv<V>(x + (((int64_t)b * h + iy) * w + ix) * c + ch);
#pragma unroll
                for (int q = 0; q < V; ++q) {
                    if (first) { best.v[q] = -INFINITY; slot[q] = ky * 3 + kx; }
                    if (t.v[q] > best.v[q] || t.v[q] != t.v[q]) { best.v[q] = t.v[q]; slot[q] = ky * 3 + kx; }
                }
                first = false;
            }
        }
        const int64_t o = (int64_t)row * c + ch;
        stv<V>(y + o, best);
        if constexpr (V == 4) {
            *reinterpret_cast<uchar4*>(arg + o) = make_uchar4((uint8_t)slot[0], (uint8_t)slot[1], (uint8_t)slot[2], (uint8_t)slot[3]);
        } else {
            arg[o] = (uint8_t)slot[0];
        }
    }
}

// dx[b][iy][ix][ch] = sum of dy over the at most four windows (oy, ox ascending) whose stored winner is this element.
template <int V>
__global__ __launch_bounds__(kThreads) void maxpool_bwd_kernel(const float* __restrict__ dy, const uint8_t* __restrict__ arg,
                                                               float* __restrict__ dx, int h, int w, int c, int ho, int wo, int pixels,
                                                               int ppb) {
    const int cv = c / V;
    const int pix0 = (int)((int64_t)blockIdx.x * ppb);
    const int npix = min(ppb, pixels - pix0);
    const int total = npix * cv;
    const int hw = h * w;
    for (int e = threadIdx.x; e < total; e += kThreads) {
        const int pl = e / cv, ch = (e - pl * cv) * V;
        const int pix = pix0 + pl;
        const int b = pix / hw, rem = pix - b * hw;
        const int iy = rem / w, ix = rem - iy * w;
        vecf<V> acc = zerov<V>();
        const int oy1 = min(ho - 1, (iy + 1) / 2), ox1 = min(wo - 1, (ix + 1) / 2);
        for (int oy = iy / 2; oy <= oy1; ++oy) {
            const int ky = iy + 1 - 2 * oy;
            for (int ox = ix / 2; ox <= ox1; ++ox) {
                const int s = ky * 3 + (ix + 1 - 2 * ox);
                const int64_t o = (((int64_t)b * ho + oy) * wo + ox) * c + ch;
                const vecf<V> t = ldv<V>(dy + o);
                uint8_t a[V];
                if constexpr (V == 4) {
                    const uchar4 u = *reinterpret_cast<const uchar4*>(arg + o);
                    a[0] = u.x; a[1] = u.y; a[2] = u.z; a[3] = u.w;
                } else {
                    a[0] = arg[o];
                }
#pragma unroll
                for (int q = 0; q < V; ++q)
                    if (a[q] == s) acc.v[q] = acc.v[q] + t.v[q];
            }
        }
        stv<V>(dx + (int64_t)pix * c + ch, acc);
    }
}

// FrozenBatchNorm2d.forward: scale = weight * rsqrt(running_var), shift = bias - running_mean * scale (eps is already inside running_var).
// A thread keeps its four channels for all its rows: 256 % (ch / 4) == 0, so the block's 256 lanes cover 256 / (ch / 4) whole rows -- one
// contiguous 4 KiB piece -- and the grid stride is a whole number of rows.
__device__ __forceinline__ void frozen_bn_affine(const float* weight, const float* bias, const float* mean, const float* var, int ch,
                                                 double* s, double* t, double* rs) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (weight != nullptr) {
            rs[q] = 1.0 / sqrt((double)var[ch + q]);
            s[q] = (double)weight[ch + q] * rs[q];
            t[q] = (double)bias[ch + q] - (double)mean[ch + q] * s[q];
        } else {
            rs[q] = 1.0; s[q] = 1.0; t[q] = 0.0;
        }
    }
}

__global__ __launch_bounds__(kThreads) void frozen_bn_act_kernel(const float* __restrict__ x, const float* __restrict__ weight,
                                                                 const float* __restrict__ bias, const float* __restrict__ mean,
                                                                 const float* __restrict__ var, const float* __restrict__ residual,
                                                                 float* __restrict__ y, int64_t rows, int c, int relu) {
    const int cv = c / 4, rpi = kThreads / cv;
    const int ch = (threadIdx.x % cv) * 4, r0 = threadIdx.x / cv;
    double s[4], t[4], rs[4];
    frozen_bn_affine(weight, bias, mean, var, ch, s, t, rs);
    const bool affine = weight != nullptr;
    for (int64_t row = (int64_t)blockIdx.x * rpi + r0; row < rows; row += (int64_t)gridDim.x * rpi) {
        const int64_t o = row * c + ch;
        vecf<4> v = ldv<4>(x + o);
        if (affine || residual != nullptr) {
            double a[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) a[q] = affine ? (double)v.v[q] * s[q] + t[q] : (double)v.v[q];
            if (residual != nullptr) {
                const vecf<4> rr = ldv<4>(residual + o);
#pragma unroll
                for (int q = 0; q < 4; ++q) a[q] = a[q] + (double)rr.v[q];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) v.v[q] = (float)a[q];
        }
        if (relu) {
#pragma unroll
            for (int q = 0; q < 4; ++q) v.v[q] = v.v[q] > 0.0f ? v.v[q] : 0.0f;
        }
        stv<4>(y + o, v);
    }
}

// g = dy * [y > 0] (relu) or dy; dx = g * scale; dresidual = g; per-block partial column sums of g * ((x - mean) * rsqrt(var)) and of g
// go to workspace[block][0 | 1][ch] as float64: a thread adds its rows in ascending order, the block adds its 256 / (ch / 4) row lanes in
// ascending order, the second kernel adds the blocks in ascending order and rounds to float32.
__global__ __launch_bounds__(kThreads) void frozen_bn_act_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                                     const float* __restrict__ x, const float* __restrict__ weight,
                                                                     const float* __restrict__ mean, const float* __restrict__ var,
                                                                     float* __restrict__ dx, float* __restrict__ dres,
                                                                     double* __restrict__ partial, int64_t rows, int c, int relu) {
    __shared__ double red[kThreads][8];
    const int cv = c / 4, rpi = kThreads / cv;
    const int ch = (threadIdx.x % cv) * 4, r0 = threadIdx.x / cv;
    double s[4], t[4], rs[4], m[4];
    frozen_bn_affine(weight, weight, mean, var, ch, s, t, rs);       // (t is not used by the backward)
    const bool affine = weight != nullptr;
#pragma unroll
    for (int q = 0; q < 4; ++q) m[q] = affine ? (double)mean[ch + q] : 0.0;
    double dw[4] = {0.0, 0.0, 0.0, 0.0}, db[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t row = (int64_t)blockIdx.x * rpi + r0; row < rows; row += (int64_t)gridDim.x * rpi) {
        const int64_t o = row * c + ch;
        vecf<4> g = ldv<4>(dy + o);
        if (relu) {
            const vecf<4> yy = ldv<4>(y + o);
#pragma unroll
            for (int q = 0; q < 4; ++q) g.v[q] = yy.v[q] > 0.0f ? g.v[q] : 0.0f;
        }
        if (dres != nullptr) stv<4>(dres + o, g);
        if (affine) {
            const vecf<4> xx = ldv<4>(x + o);
            vecf<4> d;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                d.v[q] = (float)((double)g.v[q] * s[q]);
                dw[q] = dw[q] + (double)g.v[q] * (((double)xx.v[q] - m[q]) * rs[q]);
                db[q] = db[q] + (double)g.v[q];
            }
            stv<4>(dx + o, d);
        } else {
            stv<4>(dx + o, g);
        }
    }
    if (!affine) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) { red[threadIdx.x][q] = dw[q]; red[threadIdx.x][4 + q] = db[q]; }
    __syncthreads();
    if (r0 == 0) {
        for (int r = 1; r < rpi; ++r) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                dw[q] = dw[q] + red[r * cv + threadIdx.x][q];
                db[q] = db[q] + red[r * cv + threadIdx.x][4 + q];
            }
        }
        double* p = partial + (int64_t)blockIdx.x * 2 * c;
#pragma unroll
        for (int q = 0; q < 4; ++q) { p[ch + q] = dw[q]; p[c + ch + q] = db[q]; }
    }
}

// Second stage of the column sums: a block owns `cpb` channels and cuts the partial rows into 256 / cpb interleaved parts; a thread adds
// the rows part, part + parts, ... in ascending order, then the first part's threads add the parts in ascending order and round to float32.
__global__ __launch_bounds__(kThreads) void frozen_bn_colsum_kernel(const double* __restrict__ partial, float* __restrict__ dweight,
                                                                    float* __restrict__ dbias, int blocks, int c, int cpb) {
    __shared__ double red[kThreads][2];
    const int parts = kThreads / cpb;
    const int cl = threadIdx.x % cpb, part = threadIdx.x / cpb;
    const int ch = blockIdx.x * cpb + cl;
    double a = 0.0, b = 0.0;
#pragma unroll 4
    for (int i = part; i < blocks; i += parts) {
        a = a + partial[(int64_t)i * 2 * c + ch];
        b = b + partial[(int64_t)i * 2 * c + c + ch];
    }
    red[threadIdx.x][0] = a;
    red[threadIdx.x][1] = b;
    __syncthreads();
    if (part == 0) {
        for (int r = 1; r < parts; ++r) {
            a = a + red[r * cpb + cl][0];
            b = b + red[r * cpb + cl][1];
        }
        dweight[ch] = (float)a;
        dbias[ch] = (float)b;
    }
}

// y[b][ch] = (sum over p ascending of x[b][p][ch]) / hw, in float64, rounded once
template <int V>
__global__ __launch_bounds__(kThreads) void avgpool_rows_kernel(const float* __restrict__ x, float* __restrict__ y, int b, int hw, int c) {
    const int cv = c / V;
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= (int64_t)b * cv) return;
    const int bi = (int)(e / cv), ch = (int)(e - (int64_t)bi * cv) * V;
    double acc[V];
#pragma unroll
    for (int q = 0; q < V; ++q) acc[q] = 0.0;
    const float* p = x + (int64_t)bi * hw * c + ch;
    for (int i = 0; i < hw; ++i) {
        const vecf<V> t = ldv<V>(p + (int64_t)i * c);
#pragma unroll
        for (int q = 0; q < V; ++q) acc[q] = acc[q] + (double)t.v[q];
    }
    vecf<V> out;
#pragma unroll
    for (int q = 0; q < V; ++q) out.v[q] = (float)(acc[q] / (double)hw);
    stv<V>(y + (int64_t)bi * c + ch, out);
}

// dx[b][p][ch] = dy[b][ch] / hw
template <int V>
__global__ __launch_bounds__(kThreads) void avgpool_rows_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int hw, int c,
                                                                    int rows, int rpb) {
    const int cv = c / V;
    const int row0 = (int)((int64_t)blockIdx.x * rpb);
    const int nrow = min(rpb, rows - row0);
    const int total = nrow * cv;
    const float n = (float)hw;
    for (int e = threadIdx.x; e < total; e += kThreads) {
        const int r = e / cv, ch = (e - r * cv) * V;
        const int row = row0 + r;
        vecf<V> t = ldv<V>(dy + (int64_t)(row / hw) * c + ch);
#pragma unroll
        for (int q = 0; q < V; ++q) t.v[q] = t.v[q] / n;
        stv<V>(dx + (int64_t)row * c + ch, t);
    }
}

constexpr int64_t kMaxRows = 0x7fffffff;

bool conv_geometry(int b, int h, int w, int c, int k, int stride, int pad, conv_geom* g, int* rc) {
    if (b < 1 || h < 1 || w < 1 || c < 1 || (k != 1 && k != 3 && k != 7) || (stride != 1 && stride != 2) || pad < 0 || pad >= k) {
        *rc = DSC_EINVAL;
        return false;
    }
    if (h > 4096 || w > 4096 || c > 4096 || h + 2 * pad < k || w + 2 * pad < k) {
        *rc = DSC_ERANGE;
        return false;
    }
    g->h = h; g->w = w; g->c = c; g->k = k; g->stride = stride; g->pad = pad;
    g->ho = (h + 2 * pad - k) / stride + 1;
    g->wo = (w + 2 * pad - k) / stride + 1;
    g->kk = k * k * c;
    g->kpad = (g->kk + 31) / 32 * 32;
    if ((int64_t)b * h * w > kMaxRows || (int64_t)b * g->ho * g->wo > kMaxRows) {
        *rc = DSC_ERANGE;
        return false;
    }
    return true;
}

inline bool vec4_ok(int c, const void* p0, const void* p1) { return (c & 3) == 0 && dsc_aligned16(p0) && dsc_aligned16(p1); }
inline int per_block(int lanes_per_row, int target) { return lanes_per_row >= target ? 1 : target / lanes_per_row; }
inline unsigned blocks_for(int64_t rows, int per) { return (unsigned)((rows + per - 1) / per); }

int frozen_bn_blocks(int64_t rows, int c) {
    const int rpi = kThreads / (c / 4);
    const int64_t want = (rows + (int64_t)rpi * 8 - 1) / ((int64_t)rpi * 8);
    return (int)(want < 1 ? 1 : (want > 1024 ? 1024 : want));
}
bool frozen_bn_shape(int64_t rows, int c, int* rc) {
    if (rows < 1 || c < 1) { *rc = DSC_EINVAL; return false; }
    if ((c & 3) || c > 1024 || (1024 % c) != 0 || rows > kMaxRows) { *rc = DSC_ERANGE; return false; }
    return true;
}

}  // namespace

extern "C" {

int dsc_conv_patches_f32(const float* x, float* patches, int32_t b, int32_t h, int32_t w, int32_t c, int32_t k, int32_t stride,
                         int32_t pad, dsc_stream_t stream) {
    conv_geom g;
    int rc = 0;
    if (x == nullptr || patches == nullptr) return DSC_EINVAL;
    if (!conv_geometry(b, h, w, c, k, stride, pad, &g, &rc)) return rc;
    const int rows = b * g.ho * g.wo;
    hipStream_t s = (hipStream_t)stream;
    DSC_CLEAR_STALE_ERROR();
    if (vec4_ok(c, x, patches)) {
        const int rpb = per_block(g.kpad / 4, 4096);
        hipLaunchKernelGGL(conv_patches_kernel<4>, dim3(blocks_for(rows, rpb)), dim3(kThreads), 0, s, x, patches, g, rows, rpb);
    } else {
        const int rpb = per_block(g.kpad, 4096);
        hipLaunchKernelGGL(conv_patches_kernel<1>, dim3(blocks_for(rows, rpb)), dim3(kThreads), 0, s, x, patches, g, rows, rpb);
    }
    DSC_LAUNCH_CHECK();
    return 0;
}

int dsc_conv_patches_bwd_f32(const float* dpatches, float* dx, int32_t b, int32_t h, int32_t w, int32_t c, int32_t k, int32_t stride,
                             int32_t pad, dsc_stream_t stream) {
    conv_geom g;
    int rc = 0;
    if (dpatches == nullptr || dx == nullptr) return DSC_EINVAL;
    if (!conv_geometry(b, h, w, c, k, stride, pad, &g, &rc)) return rc;
    const int pixels = b * h * w;
    hipStream_t s = (hipStream_t)stream;
    DSC_CLEAR_STALE_ERROR();
    if (vec4_ok(c, dpatches, dx)) {
        const int ppb = per_block(c / 4, 2048);
        hipLaunchKernelGGL(conv_patches_bwd_kernel<4>, dim3(blocks_for(pixels, ppb)), dim3(kThreads), 0, s, dpatches, dx, g, pixels, ppb);
    } else {
        const int ppb = per_block(c, 2048);
        hipLaunchKernelGGL(conv_patches_bwd_kernel<1>, dim3(blocks_for(pixels, ppb)), dim3(kThreads), 0, s, dpatches, dx, g, pixels, ppb);
    }
    DSC_LAUNCH_CHECK();
    return 0;
}

static int pool_shape(int32_t b, int32_t h, int32_t w, int32_t c, int* ho, int* wo) {
    if (b < 1 || h < 1 || w < 1 || c < 1) return DSC_EINVAL;
    if (h > 4096 || w > 4096 || c > 4096) return DSC_ERANGE;
    *ho = (h - 1) / 2 + 1;
    *wo = (w - 1) / 2 + 1;
    if ((int64_t)b * h * w > kMaxRows) return DSC_ERANGE;
    return 0;
}

int dsc_maxpool2d_f32(const float* x, float* y, uint8_t* arg, int32_t b, int32_t h, int32_t w, int32_t c, dsc_stream_t stream) {
    int ho, wo;
    if (x == nullptr || y == nullptr || arg == nullptr) return DSC_EINVAL;
    const int rc = pool_shape(b, h, w, c, &ho, &wo);
    if (rc) return rc;
    const int rows = b * ho * wo;
    hipStream_t s = (hipStream_t)stream;
    DSC_CLEAR_STALE_ERROR();
    if (vec4_ok(c, x, y) && (reinterpret_cast<uintptr_t>(arg) & 3u) == 0) {
        const int rpb = per_block(c / 4, 2048);
        hipLaunchKernelGGL(maxpool_kernel<4>, dim3(blocks_for(rows, rpb)), dim3(kThreads), 0, s, x, y, arg, h, w, c, ho, wo, rows, rpb);
    } else {
        const int rpb = per_block(c, 2048);
        hipLaunchKernelGGL(maxpool_kernel<1>, dim3(blocks_for(rows, rpb)), dim3(kThreads), 0, s, x, y, arg, h, w, c, ho, wo, rows, rpb);
    }
    DSC_LAUNCH_CHECK();
    return 0;
}

int dsc_maxpool2d_bwd_f32(const float* dy, const uint8_t* arg, float* dx, int32_t b, int32_t h, int32_t w, int32_t c,
                          dsc_stream_t stream) {
    int ho, wo;
    if (dy == nullptr || dx == nullptr || arg == nullptr) return DSC_EINVAL;
    const int rc = pool_shape(b, h, w, c, &ho, &wo);
    if (rc) return rc;
    const int pixels = b * h * w;
    hipStream_t s = (hipStream_t)stream;
    DSC_CLEAR_STALE_ERROR();
    if (vec4_ok(c, dy, dx) && (reinterpret_cast<uintptr_t>(arg) & 3u) == 0) {
        const int ppb = per_block(c / 4, 2048);
        hipLaunchKernelGGL(maxpool_bwd_kernel<4>, dim3(blocks_for(pixels, ppb)), dim3(kThreads), 0, s, dy, arg, dx, h, w, c, ho, wo,
                           pixels, ppb);
    } else {
        const int ppb = per_block(c, 2048);
        hipLaunchKernelGGL(maxpool_bwd_kernel<1>, dim3(blocks_for(pixels, ppb)), dim3(kThreads), 0, s, dy, arg, dx, h, w, c, ho, wo,
                           pixels, ppb);
    }
    DSC_LAUNCH_CHECK();
    return 0;
}

int dsc_frozen_bn_act_f32(const float* x, const float* weight, const float* bias, const float* running_mean, const float* running_var,
                          const float* residual, float* y, int64_t rows, int32_t ch, int32_t relu, dsc_stream_t stream) {
    int rc = 0;
    if (x == nullptr || y == nullptr) return DSC_EINVAL;
    const bool affine = weight != nullptr;
    if (affine != (bias != nullptr) || affine != (running_mean != nullptr) || affine != (running_var != nullptr)) return DSC_EINVAL;
    if (!frozen_bn_shape(rows, ch, &rc)) return rc;
    if (!dsc_aligned16(x) || !dsc_aligned16(y) || !dsc_aligned16(residual)) return DSC_EALIGN;
    const int rpi = kThreads / (ch / 4);
    int64_t blocks = (rows + rpi - 1) / rpi;
    if (blocks > 4096) blocks = 4096;
    DSC_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL(frozen_bn_act_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, x, weight, bias, running_mean,
                       running_var, residual, y, rows, ch, relu ? 1 : 0);
    DSC_LAUNCH_CHECK();
    return 0;
}

int64_t dsc_frozen_bn_workspace_floats(int64_t rows, int32_t ch) {
    int rc = 0;
    if (!frozen_bn_shape(rows, ch, &rc)) return rc;
    return (int64_t)frozen_bn_blocks(rows, ch) * 2 * ch * 2;      // float64 partial sums
}

int dsc_frozen_bn_act_bwd_f32(const float* dy, const float* y, const float* x, const float* weight, const float* running_mean,
                              const float* running_var, float* dx, float* dresidual, float* dweight, float* dbias, int64_t rows,
                              int32_t ch, int32_t relu, float* workspace, int64_t workspace_floats, dsc_stream_t stream) {
    int rc = 0;
    if (dy == nullptr || dx == nullptr || (relu && y == nullptr)) return DSC_EINVAL;
    const bool affine = weight != nullptr;
    if (affine != (running_mean != nullptr) || affine != (running_var != nullptr) || affine != (x != nullptr) ||
        affine != (dweight != nullptr) || affine != (dbias != nullptr))
        return DSC_EINVAL;
    if (!frozen_bn_shape(rows, ch, &rc)) return rc;
    if (!dsc_aligned16(dy) || !dsc_aligned16(y) || !dsc_aligned16(x) || !dsc_aligned16(dx) || !dsc_aligned16(dresidual)) return DSC_EALIGN;
    const int blocks = frozen_bn_blocks(rows, ch);
    if (affine && (workspace == nullptr || workspace_floats < (int64_t)blocks * 2 * ch * 2)) return DSC_EINVAL;
    if (affine && (reinterpret_cast<uintptr_t>(workspace) & 7u)) return DSC_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    DSC_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL(frozen_bn_act_bwd_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, dy, y, x, weight, running_mean, running_var,
                       dx, dresidual, reinterpret_cast<double*>(workspace), rows, ch, relu ? 1 : 0);
    DSC_LAUNCH_CHECK();
    if (affine) {
        const int cpb = ch < 16 ? ch : 16;                  // ch is a power of two: cpb divides both ch and the block
        hipLaunchKernelGGL(frozen_bn_colsum_kernel, dim3((unsigned)(ch / cpb)), dim3(kThreads), 0, s,
                           reinterpret_cast<const double*>(workspace), dweight, dbias, blocks, ch, cpb);
        DSC_LAUNCH_CHECK();
    }
    return 0;
}

int dsc_avgpool_rows_f32(const float* x, float* y, int32_t b, int32_t hw, int32_t ch, dsc_stream_t stream) {
    if (x == nullptr || y == nullptr || b < 1 || hw < 1 || ch < 1) return DSC_EINVAL;
    if (ch > 4096 || (int64_t)b * hw > kMaxRows) return DSC_ERANGE;
    hipStream_t s = (hipStream_t)stream;
    DSC_CLEAR_STALE_ERROR();
    if (vec4_ok(ch, x, y)) {
        hipLaunchKernelGGL(avgpool_rows_kernel<4>, dim3(blocks_for((int64_t)b * (ch / 4), kThreads)), dim3(kThreads), 0, s, x, y, b, hw, ch);
    } else {
        hipLaunchKernelGGL(avgpool_rows_kernel<1>, dim3(blocks_for((int64_t)b * ch, kThreads)), dim3(kThreads), 0, s, x, y, b, hw, ch);
    }
    DSC_LAUNCH_CHECK();
    return 0;
}

int dsc_avgpool_rows_bwd_f32(const float* dy, float* dx, int32_t b, int32_t hw, int32_t ch, dsc_stream_t stream) {
    if (dy == nullptr || dx == nullptr || b < 1 || hw < 1 || ch < 1) return DSC_EINVAL;
    if (ch > 4096 || (int64_t)b * hw > kMaxRows) return DSC_ERANGE;
    const int rows = b * hw;
    hipStream_t s = (hipStream_t)stream;
    DSC_CLEAR_STALE_ERROR();
    if (vec4_ok(ch, dy, dx)) {
        const int rpb = per_block(ch / 4, 2048);
        hipLaunchKernelGGL(avgpool_rows_bwd_kernel<4>, dim3(blocks_for(rows, rpb)), dim3(kThreads), 0, s, dy, dx, hw, ch, rows, rpb);
    } else {
        const int rpb = per_block(ch, 2048);
        hipLaunchKernelGGL(avgpool_rows_bwd_kernel<1>, dim3(blocks_for(rows, rpb)), dim3(kThreads), 0, s, dy, dx, hw, ch, rows, rpb);
    }
    DSC_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
