// Shape retrieval after sampling: for every generated object, the nearest 3D-FUTURE model of the
// predicted class in the 32-d latent shape-code space -- reference ThreedFutureDataset.get_closest_furniture_to_objfeats
// / ..._and_size (scene_synthesis/datasets/threed_future_dataset.py:49-77), called once per box from
// scene_synthesis/utils.py:80-110.  Brute-force scan, HBM/L2-bound: one wave per query, lanes stride over the
// database rows, argmin by wave shuffles.
//
// Bit-exact index parity with the numpy reference: squared differences are rounded products (this file is compiled with
// -ffp-contract=off) summed in numpy's pairwise order for a contiguous fp32 vector of 32 (8 strided partial sums,
// combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7))); size keys are float64 sums of 3 terms; ties go to the lowest
// database index (Python's stable sort / np.lexsort).
#define DSC_BAD_INDEX_COUNTER
#include "dsc_common.h"

namespace {

__device__ __forceinline__ float sqdist32_numpy_order(const float* __restrict__ a, const float* __restrict__ q) {
    float r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float d = a[j] - q[j]; r[j] = d * d; }
#pragma unroll
    for (int i = 8; i < 32; i += 8)
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float d = a[i + j] - q[i + j]; const float s = d * d; r[j] = r[j] + s; }
    return ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
}

__global__ __launch_bounds__(256) void retrieve_kernel(const float* __restrict__ qfeat, const int* __restrict__ qlabel,
                                                      const double* __restrict__ qsize, const float* __restrict__ db,
                                                      const int* __restrict__ dblabel, const double* __restrict__ dbsize,
                                                      int nq, int ndb, int* __restrict__ out_idx,
                                                      float* __restrict__ out_dist) {
    const int lane = threadIdx.x & 63;
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq) return;
    float q[32];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const f32x4 t4 = *reinterpret_cast<const f32x4*>(qfeat + (long)qi * 32 + c * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) q[c * 4 + e] = t4[e];
    }
    const int lab = qlabel[qi];
    double qs[3] = {0.0, 0.0, 0.0};
    if (qsize) { qs[0] = qsize[(long)qi * 3]; qs[1] = qsize[(long)qi * 3 + 1]; qs[2] = qsize[(long)qi * 3 + 2]; }
    double best_s = 1e300;
    float best_f = INFINITY;
    int best_i = 0x7fffffff;
    for (int j = lane; j < ndb; j += 64) {
        if (dblabel[j] != lab) continue;
        float row[32];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const f32x4 t4 = *reinterpret_cast<const f32x4*>(db + (long)j * 32 + c * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) row[c * 4 + e] = t4[e];
        }
        const float f = sqdist32_numpy_order(row, q);
        double sk = 0.0;
        if (qsize) {
            const double d0 = dbsize[(long)j * 3] - qs[0], d1 = dbsize[(long)j * 3 + 1] - qs[1], d2 = dbsize[(long)j * 3 + 2] - qs[2];
            const double p0 = d0 * d0, p1 = d1 * d1, p2 = d2 * d2;
            sk = (p0 + p1) + p2;
        }
        // lexicographic (size key, feature key, index); rows visited by a lane are in increasing index order
        if (sk < best_s || (sk == best_s && f < best_f)) { best_s = sk; best_f = f; best_i = j; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double os = __shfl_xor(best_s, o, 64);
        const float of = __shfl_xor(best_f, o, 64);
        const int oi = __shfl_xor(best_i, o, 64);
        const bool better = (os < best_s) || (os == best_s && (of < best_f || (of == best_f && oi < best_i)));
        if (better) { best_s = os; best_f = of; best_i = oi; }
    }
    if (lane == 0) {
        out_idx[qi] = (best_i == 0x7fffffff) ? -1 : best_i;
        if (out_dist) out_dist[qi] = best_f;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Scene statistics after sampling: the box-level quality numbers the reference appends to iou_states.txt for every scene
// (scripts/utils.py:559-747: axis_aligned_bbox_overlaps_3d, computer_intersection, judge_if_symmetry, computer_symmetry),
// for B scenes with their own object counts in two launches.
//
// box_bounds_kernel: one lane per box.  The eight corners (+-size).dot(R) + translation (scene_synthesis/utils.py:48-53,73)
// in float64, min / max, rounded once to float32.
//
// scene_stats_kernel: one workgroup per scene, bounds / class ids / model ids / volumes staged in LDS (160 objects: 5 KB).  The
// n x n cells of the scene's pair matrix are dealt to kStatsLanes = 256 VIRTUAL lanes (cell q -> lane q % 256, increasing q within a
// lane), whatever the block size: a 256-thread block owns one virtual lane per thread, a one-wave block owns four per lane.  Each
// group of 64 virtual lanes is summed by the xor butterfly, the four group totals as ((g0 + g1) + g2) + g3.  The order depends on n
// alone -- not on Nmax, not on the block size -- so the float64 sums of a scene are the same bits in every batch and under both
// launch shapes, and the integers are exact.  No atomics.
constexpr int kStatsMaxObjects = 160;
constexpr int kStatsLanes = 256;

__global__ __launch_bounds__(256) void box_bounds_kernel(const float* __restrict__ tr, const float* __restrict__ sz,
                                                        const float* __restrict__ ang, const int* __restrict__ counts, int batch,
                                                        int nmax, float* __restrict__ out) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)batch * nmax) return;
    const int b = (int)(idx / nmax), k = (int)(idx - (long)b * nmax);
    const int n = (int)dsc_checked_index(counts[b], (int64_t)nmax + 1, k == 0);
    float* o = out + idx * 6;
    if (k >= n) {                                    // padding rows are never read; their bounds are defined (zero)
#pragma unroll
        for (int e = 0; e < 6; ++e) o[e] = 0.0f;
        return;
    }
    const double sx = sz[idx * 3], sy = sz[idx * 3 + 1], s_z = sz[idx * 3 + 2];
    const double tx = tr[idx * 3], ty = tr[idx * 3 + 1], tz = tr[idx * 3 + 2];
    const double th = ang[idx];
    const double c = cos(th), s = sin(th);
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const double vx = (m & 1) ? sx : -sx, vy = (m & 2) ? sy : -sy, vz = (m & 4) ? s_z : -s_z;
        // v.dot(R), R = [[c, 0, -s], [0, 1, 0], [s, 0, c]]
        const double p[3] = {(vx * c + vz * s) + tx, vy + ty, (vz * c - vx * s) + tz};
#pragma unroll
        for (int e = 0; e < 3; ++e) { lo[e] = p[e] < lo[e] ? p[e] : lo[e]; hi[e] = p[e] > hi[e] ? p[e] : hi[e]; }
    }
#pragma unroll
    for (int e = 0; e < 3; ++e) { o[e] = (float)lo[e]; o[3 + e] = (float)hi[e]; }
}

template <class T>
__device__ __forceinline__ T stats_wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int NT>
__global__ __launch_bounds__(NT) void scene_stats_kernel(const float* __restrict__ bounds, const float* __restrict__ scores,
                                                        const int* __restrict__ model_ids, const int* __restrict__ counts,
                                                        int nmax, int num_classes, int* __restrict__ out_nint,
                                                        int* __restrict__ out_nsym, double* __restrict__ out_iou,
                                                        double* __restrict__ out_ovl, double* __restrict__ out_vol,
                                                        int* __restrict__ class_counts, float* __restrict__ pair_iou) {
    constexpr int G = kStatsLanes / NT;              // virtual lanes per thread
    constexpr int W = NT / 64;                       // waves per block
    __shared__ float s_box[kStatsMaxObjects * 6];
    __shared__ float s_vol[kStatsMaxObjects];
    __shared__ int s_cls[kStatsMaxObjects];
    __shared__ int s_mid[kStatsMaxObjects];
    __shared__ double s_red[3][4];
    __shared__ int s_redi[2][4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = (int)dsc_checked_index(counts[b], (int64_t)nmax + 1, tid == 0);
    const float* gb = bounds + (long)b * nmax * 6;
    for (int k = tid; k < n; k += NT) {
        float bx[6];
#pragma unroll
        for (int e = 0; e < 6; ++e) { bx[e] = gb[k * 6 + e]; s_box[k * 6 + e] = bx[e]; }
        s_vol[k] = (bx[3] - bx[0]) * (bx[4] - bx[1]) * (bx[5] - bx[2]);
        const float* sc = scores + ((long)b * nmax + k) * num_classes;
        float best = sc[0];
        int arg = 0;
        for (int c = 1; c < num_classes; ++c) {      // numpy.argmax: first maximum, a NaN counts as the maximum
            const float v = sc[c];
            if (v > best || (v != v && best == best)) { best = v; arg = c; }
        }
        s_cls[k] = arg;
        s_mid[k] = model_ids ? model_ids[(long)b * nmax + k] : 0;
    }
    __syncthreads();

    int nint[G], nsym[G];
    double siou[G], sovl[G], svol[G];
    const int cells = n * n;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int v = g * NT + tid;
        nint[g] = 0; nsym[g] = 0; siou[g] = 0.0; sovl[g] = 0.0;
        svol[g] = v < n ? (double)s_vol[v] : 0.0;
        for (int q = v; q < cells; q += kStatsLanes) {
            const int i = q / n, j = q - i * n;
            float iou = 0.0f;
            if (i < j) {
                const float* a = s_box + i * 6;
                const float* c = s_box + j * 6;
                float wh[3];
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    const float lt = a[e] > c[e] ? a[e] : c[e];
                    const float rb = a[3 + e] < c[3 + e] ? a[3 + e] : c[3 + e];
                    const float d = rb - lt;
                    wh[e] = d < 0.0f ? 0.0f : d;
                }
                const float overlap = wh[0] * wh[1] * wh[2];
                float uni = (s_vol[i] + s_vol[j]) - overlap;
                uni = uni < 1e-6f ? 1e-6f : uni;
                iou = overlap / uni;
                nint[g] += iou > 0.0f ? 1 : 0;
                siou[g] += (double)iou;
                sovl[g] += (double)overlap;
                if (s_cls[i] == s_cls[j] && s_mid[i] == s_mid[j]) {      // judge_if_symmetry, float64 on the float32 bounds
                    double dh = 0.0, dc[3];
#pragma unroll
                    for (int e = 0; e < 3; ++e) {
                        const double alo = a[e], ahi = a[3 + e], clo = c[e], chi = c[3 + e];
                        const double d = fabs((ahi - alo) / 2.0 - (chi - clo) / 2.0);
                        dh = d > dh ? d : dh;
                        dc[e] = fabs((ahi + alo) / 2.0 - (chi + clo) / 2.0);
                    }
                    nsym[g] += (dh < 0.1 && (dc[0] < 0.1 || dc[2] < 0.1)) ? 1 : 0;
                }
            }
            if (pair_iou) pair_iou[((long)b * nmax + i) * nmax + j] = iou;
        }
        nint[g] = stats_wave_sum(nint[g]);
        nsym[g] = stats_wave_sum(nsym[g]);
        siou[g] = stats_wave_sum(siou[g]);
        sovl[g] = stats_wave_sum(sovl[g]);
        svol[g] = stats_wave_sum(svol[g]);
    }
    if (W > 1) {                                     // one virtual group per wave: totals through LDS, summed in group order
        const int w = tid >> 6;
        if ((tid & 63) == 0) {
            s_redi[0][w] = nint[0]; s_redi[1][w] = nsym[0];
            s_red[0][w] = siou[0]; s_red[1][w] = sovl[0]; s_red[2][w] = svol[0];
        }
        __syncthreads();
    }
    if (tid == 0) {
        int ti[2];
        double td[3];
        if (W > 1) {
            for (int r = 0; r < 2; ++r) ti[r] = ((s_redi[r][0] + s_redi[r][1]) + s_redi[r][2]) + s_redi[r][3];
            for (int r = 0; r < 3; ++r) td[r] = ((s_red[r][0] + s_red[r][1]) + s_red[r][2]) + s_red[r][3];
        } else {
            ti[0] = ((nint[0] + nint[G > 1 ? 1 : 0]) + nint[G > 2 ? 2 : 0]) + nint[G > 3 ? 3 : 0];
            ti[1] = ((nsym[0] + nsym[G > 1 ? 1 : 0]) + nsym[G > 2 ? 2 : 0]) + nsym[G > 3 ? 3 : 0];
            td[0] = ((siou[0] + siou[G > 1 ? 1 : 0]) + siou[G > 2 ? 2 : 0]) + siou[G > 3 ? 3 : 0];
            td[1] = ((sovl[0] + sovl[G > 1 ? 1 : 0]) + sovl[G > 2 ? 2 : 0]) + sovl[G > 3 ? 3 : 0];
            td[2] = ((svol[0] + svol[G > 1 ? 1 : 0]) + svol[G > 2 ? 2 : 0]) + svol[G > 3 ? 3 : 0];
        }
        out_nint[b] = ti[0]; out_nsym[b] = ti[1];
        out_iou[b] = td[0]; out_ovl[b] = td[1]; out_vol[b] = td[2];
    }
    for (int c = tid; c < num_classes; c += NT) {
        int cnt = 0;
        for (int k = 0; k < n; ++k) cnt += s_cls[k] == c ? 1 : 0;
        class_counts[(long)b * num_classes + c] = cnt;
    }
    if (pair_iou && n < nmax)                        // cells outside the scene's n x n corner
        for (int q = tid; q < nmax * nmax; q += NT) {
            const int i = q / nmax, j = q - i * nmax;
            if (i >= n || j >= n) pair_iou[(long)b * nmax * nmax + q] = 0.0f;
        }
}

}  // namespace

unsigned dsc_bad_index_retrieval(bool reset) { return dsc_read_bad_index_count(reset); }

extern "C" int dsc_box_bounds_f32(const float* translations, const float* sizes, const float* angles, const int32_t* counts,
                                  int32_t batch, int32_t nmax, float* bounds, dsc_stream_t stream) {
    if (!translations || !sizes || !angles || !counts || !bounds || batch < 1 || nmax < 1) return DSC_EINVAL;
    DSC_CLEAR_STALE_ERROR();
    const long total = (long)batch * nmax;
    hipLaunchKernelGGL(box_bounds_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       translations, sizes, angles, counts, batch, nmax, bounds);
    DSC_LAUNCH_CHECK();
    return 0;
}

// block_threads: 0 = by Nmax (one wave up to DSC_STATS_ONE_WAVE_MAX objects, four waves above), or 64 / 256 (same bits either way)
extern "C" int dsc_scene_stats_f32(const float* bounds, const float* class_scores, const int32_t* model_ids, const int32_t* counts,
                                   int32_t batch, int32_t nmax, int32_t num_classes, int32_t block_threads,
                                   int32_t* num_intersecting, int32_t* num_symmetry, double* iou_sum, double* overlap_sum,
                                   double* volume_sum, int32_t* class_counts, float* pair_iou, dsc_stream_t stream) {
    if (!bounds || !class_scores || !counts || !num_intersecting || !num_symmetry || !iou_sum || !overlap_sum || !volume_sum ||
        !class_counts || batch < 1 || nmax < 1 || num_classes < 1)
        return DSC_EINVAL;
    if (nmax > kStatsMaxObjects) return DSC_ERANGE;
    if (block_threads != 0 && block_threads != 64 && block_threads != 256) return DSC_EINVAL;
    const int nt = block_threads ? block_threads : (nmax <= DSC_STATS_ONE_WAVE_MAX ? 64 : 256);
    DSC_CLEAR_STALE_ERROR();
    if (nt == 64)
        hipLaunchKernelGGL(scene_stats_kernel<64>, dim3(batch), dim3(64), 0, static_cast<hipStream_t>(stream), bounds, class_scores,
                           model_ids, counts, nmax, num_classes, num_intersecting, num_symmetry, iou_sum, overlap_sum, volume_sum,
                           class_counts, pair_iou);
    else
        hipLaunchKernelGGL(scene_stats_kernel<256>, dim3(batch), dim3(256), 0, static_cast<hipStream_t>(stream), bounds, class_scores,
                           model_ids, counts, nmax, num_classes, num_intersecting, num_symmetry, iou_sum, overlap_sum, volume_sum,
                           class_counts, pair_iou);
    DSC_LAUNCH_CHECK();
    return 0;
}

extern "C" int dsc_retrieve_nearest_f32(const float* query_feats, const int32_t* query_labels, const double* query_sizes,
                                        const float* db_feats, const int32_t* db_labels, const double* db_sizes,
                                        int32_t n_query, int32_t n_db, int32_t feat_dim, int32_t* out_index,
                                        float* out_dist, dsc_stream_t stream) {
    if (!query_feats || !query_labels || !db_feats || !db_labels || !out_index || n_query < 1 || n_db < 1) return DSC_EINVAL;
    if (feat_dim != 32) return DSC_ERANGE;
    if ((query_sizes != nullptr) != (db_sizes != nullptr)) return DSC_EINVAL;
    if (!dsc_aligned16(query_feats) || !dsc_aligned16(db_feats)) return DSC_EALIGN;
    DSC_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL(retrieve_kernel, dim3((n_query + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream),
                       query_feats, query_labels, query_sizes, db_feats, db_labels, db_sizes, n_query, n_db, out_index,
                       out_dist);
    DSC_LAUNCH_CHECK();
    return 0;
}
