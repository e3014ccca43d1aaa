// KITTI AP evaluation (mmdet3d/core/evaluation/kitti_utils): the rotated overlaps of rotate_iou.py + d3_box_overlap_kernel,
// and the greedy ground-truth <-> detection assignment of compute_statistics_jit / fused_compute_statistics, batched over
// frames, score thresholds and (class, difficulty, min-overlap) combinations.
//
// Arithmetic of the overlaps. The reference kernel is numba-CUDA on float32 arrays, so its typing decides the bits:
// float32 op float32 stays float32, but a float32 combined with a Python literal or an integer is float64. That makes
//   * `-x_d / 2`, `center /= num_of_inter` and `-2 - v[0]` float64 operations whose result goes straight back into a float32
//     slot - the same value as the float32 operation (halving is exact; a float64 quotient or difference of two float32
//     rounded to float32 is the correctly rounded float32 result), so they are written in float32 here;
//   * `trangle_area(...) / 2.0` float64, and with it the `area_val` accumulator of `area()`, the value `inter()` returns and
//     the final `area_inter / (area1 + area2 - area_inter)` (area1 + area2 itself is float32). These are carried in
//     double here, and the quotient is rounded to float32 on the store, as the float32 `dev_iou` does.
// No multiply-add of this file may be contracted into an fma: the pragma below holds for the whole translation unit
// (the Makefile passes -ffp-contract=off for it as well).
#include "gga_common.h"

#pragma clang fp contract(off)

#define KE_TILE 64            // boxes of either side staged per LDS tile of the overlap kernel
#define KE_SAMPLE_PTS 41      // N_SAMPLE_PTS of eval_class
#define KE_CHUNK 64           // frames per wave of the statistics kernel, one per lane

// ------------------------------------------------------------------------------------------------ rotated overlaps
// rbbox_to_corners: clockwise corners, rotated clockwise. rb = (cx, cy, x_d, y_d, angle).
__device__ __forceinline__ void ke_corners(const float* rb, float* c) {
    const float a_cos = cosf(rb[4]), a_sin = sinf(rb[4]);
    const float hx = rb[2] / 2.f, hy = rb[3] / 2.f;
    const float xs[4] = {-hx, -hx, hx, hx}, ys[4] = {-hy, hy, hy, -hy};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        c[2 * i] = a_cos * xs[i] + a_sin * ys[i] + rb[0];
        c[2 * i + 1] = -a_sin * xs[i] + a_cos * ys[i] + rb[1];
    }
}

__device__ __forceinline__ bool ke_point_in_quad(float px, float py, const float* q) {
    const float ab0 = q[2] - q[0], ab1 = q[3] - q[1];
    const float ad0 = q[6] - q[0], ad1 = q[7] - q[1];
    const float ap0 = px - q[0], ap1 = py - q[1];
    const float abab = ab0 * ab0 + ab1 * ab1;
    const float abap = ab0 * ap0 + ab1 * ap1;
    const float adad = ad0 * ad0 + ad1 * ad1;
    const float adap = ad0 * ap0 + ad1 * ap1;
    return abab >= abap && abap >= 0 && adad >= adap && adap >= 0;
}

__device__ __forceinline__ bool ke_segment_intersection(const float* p1, const float* p2, int i, int j, float* out) {
    const float A0 = p1[2 * i], A1 = p1[2 * i + 1];
    const float B0 = p1[2 * ((i + 1) & 3)], B1 = p1[2 * ((i + 1) & 3) + 1];
    const float C0 = p2[2 * j], C1 = p2[2 * j + 1];
    const float D0 = p2[2 * ((j + 1) & 3)], D1 = p2[2 * ((j + 1) & 3) + 1];
    const float BA0 = B0 - A0, BA1 = B1 - A1;
    const float DA0 = D0 - A0, CA0 = C0 - A0;
    const float DA1 = D1 - A1, CA1 = C1 - A1;
    const bool acd = DA1 * CA0 > CA1 * DA0;
    const bool bcd = (D1 - B1) * (C0 - B0) > (C1 - B1) * (D0 - B0);
    if (acd != bcd) {
        const bool abc = CA1 * BA0 > BA1 * CA0;
        const bool abd = DA1 * BA0 > BA1 * DA0;
        if (abc != abd) {
            const float DC0 = D0 - C0, DC1 = D1 - C1;
            const float ABBA = A0 * B1 - B0 * A1;
            const float CDDC = C0 * D1 - D0 * C1;
            const float DH = BA1 * DC0 - BA0 * DC1;
            const float Dx = ABBA * DC0 - BA0 * CDDC;
            const float Dy = ABBA * DC1 - BA1 * CDDC;
            out[0] = Dx / DH;
            out[1] = Dy / DH;
            return true;
        }
    }
    return false;
}

// inter(rbbox1, rbbox2) on prepared corners: quadrilateral_intersection, sort_vertex_in_convex_polygon, area. The
// reference's intersection_corners holds 8 points and is written without a bound; two convex quadrilaterals in general
// position give at most 8, and a ninth (degenerate input only) is dropped here instead of written past the array.
__device__ double ke_inter(const float* c1, const float* c2) {
    float pts[16];
    int n = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (ke_point_in_quad(c1[2 * i], c1[2 * i + 1], c2) && n < 8) { pts[2 * n] = c1[2 * i]; pts[2 * n + 1] = c1[2 * i + 1]; ++n; }
        if (ke_point_in_quad(c2[2 * i], c2[2 * i + 1], c1) && n < 8) { pts[2 * n] = c2[2 * i]; pts[2 * n + 1] = c2[2 * i + 1]; ++n; }
    }
    float t[2];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            if (ke_segment_intersection(c1, c2, i, j, t) && n < 8) { pts[2 * n] = t[0]; pts[2 * n + 1] = t[1]; ++n; }
    if (n > 0) {
        float cx = 0.f, cy = 0.f;
        for (int i = 0; i < n; ++i) { cx += pts[2 * i]; cy += pts[2 * i + 1]; }
        cx /= (float)n;
        cy /= (float)n;
        float vs[8];
        for (int i = 0; i < n; ++i) {
            float v0 = pts[2 * i] - cx, v1 = pts[2 * i + 1] - cy;
            const float d = sqrtf(v0 * v0 + v1 * v1);
            v0 = v0 / d;
            v1 = v1 / d;
            if (v1 < 0) v0 = -2.f - v0;
            vs[i] = v0;
        }
        for (int i = 1; i < n; ++i) {
            if (vs[i - 1] > vs[i]) {
                const float temp = vs[i], tx = pts[2 * i], ty = pts[2 * i + 1];
                int j = i;
                while (j > 0 && vs[j - 1] > temp) {
                    vs[j] = vs[j - 1];
                    pts[2 * j] = pts[2 * j - 2];
                    pts[2 * j + 1] = pts[2 * j - 1];
                    --j;
                }
                vs[j] = temp;
                pts[2 * j] = tx;
                pts[2 * j + 1] = ty;
            }
        }
    }
    double area_val = 0.0;
    for (int i = 0; i < n - 2; ++i) {
        const float* a = pts;
        const float* b = pts + 2 * i + 2;
        const float* c = pts + 2 * i + 4;
        const float cross = (a[0] - c[0]) * (b[1] - c[1]) - (a[1] - c[1]) * (b[0] - c[0]);
        area_val += fabs((double)cross / 2.0);
    }
    return area_val;
}

struct KeStaged {
    float corners[8];
    float area;          // x_d * y_d of the BEV rectangle, float32
};

// d3_box_overlap_kernel for one pair. The annotations keep their dtypes there: an operation between two values of a
// float32 side is float32 (the box's own lower face and volume), anything that mixes in a float64 side is float64, and
// with both sides float32 every operation is. A float32 +, -, * or / equals the float64 one rounded to float32 (53 >= 2 * 24
// + 2 bits), which is how the float32 steps are written.
__device__ __forceinline__ float ke_d3(const double* b, const double* q, float rinc, int dt_f32, int gt_f32) {
    if (!(rinc > 0)) return rinc;
    const int both = dt_f32 && gt_f32;
#define KE_RB(x) (dt_f32 ? (double)(float)(x) : (x))
#define KE_RQ(x) (gt_f32 ? (double)(float)(x) : (x))
#define KE_R(x) (both ? (double)(float)(x) : (x))
    const double lo_b = KE_RB(b[1] - b[4]), lo_q = KE_RQ(q[1] - q[4]);
    const double iw = KE_R(fmin(b[1], q[1]) - fmax(lo_b, lo_q));
    if (!(iw > 0)) return 0.f;
    double area1 = KE_RB(b[3] * b[4]);
    area1 = KE_RB(area1 * b[5]);
    double area2 = KE_RQ(q[3] * q[4]);
    area2 = KE_RQ(area2 * q[5]);
    const double inc = KE_R(iw * (double)rinc);
    double ua = KE_R(area1 + area2);
    ua = KE_R(ua - inc);
    return (float)(inc / ua);
#undef KE_RB
#undef KE_RQ
#undef KE_R
}

// One workgroup per frame; tiles of KE_TILE detections x KE_TILE ground truths, corners and sin / cos once per box and tile.
__global__ __launch_bounds__(256) void kitti_eval_overlaps_kernel(
    const double* __restrict__ dt, const int64_t* __restrict__ dt_off, int64_t n_dt, const double* __restrict__ gt,
    const int64_t* __restrict__ gt_off, int64_t n_gt, const int64_t* __restrict__ ov_off, int64_t n_ov, int metric, int dt_f32, int gt_f32,
    float* __restrict__ out) {
    __shared__ KeStaged s_dt[KE_TILE], s_gt[KE_TILE];
    const int f = blockIdx.x;
    const int64_t d0 = dt_off[f], g0 = gt_off[f], o0 = ov_off[f];
    const int64_t nd = dt_off[f + 1] - d0, ng = gt_off[f + 1] - g0;
    // offsets are the caller's device data: a frame that does not fit the arrays it indexes is left alone
    if (nd <= 0 || ng <= 0 || d0 < 0 || g0 < 0 || o0 < 0 || d0 + nd > n_dt || g0 + ng > n_gt || nd > (n_ov - o0) / ng) return;
    const int tid = threadIdx.x;
    for (int64_t td = 0; td < nd; td += KE_TILE) {
        const int cd = (int)(nd - td < KE_TILE ? nd - td : KE_TILE);
        for (int64_t tg = 0; tg < ng; tg += KE_TILE) {
            const int cg = (int)(ng - tg < KE_TILE ? ng - tg : KE_TILE);
            __syncthreads();
            if (tid < 2 * KE_TILE) {
                const bool is_gt = tid >= KE_TILE;
                const int k = is_gt ? tid - KE_TILE : tid;
                if (k < (is_gt ? cg : cd)) {
                    const double* src = is_gt ? gt + (g0 + tg + k) * 7 : dt + (d0 + td + k) * 7;
                    // BEV rectangle of a camera box: location x, z; dimensions 0, 2; rotation_y - cast to float32 first
                    const float rb[5] = {(float)src[0], (float)src[2], (float)src[3], (float)src[5], (float)src[6]};
                    KeStaged* dst = is_gt ? &s_gt[k] : &s_dt[k];
                    ke_corners(rb, dst->corners);
                    dst->area = rb[2] * rb[3];
                }
            }
            __syncthreads();
            for (int p = tid; p < cd * cg; p += 256) {
                const int j = p / cg, i = p - j * cg;          // detection j, ground truth i of the tile
                // the query box is the ground truth: inter(query, box)
                const double area_inter = ke_inter(s_gt[i].corners, s_dt[j].corners);
                float v;
                if (metric == 1) {
                    v = (float)(area_inter / ((double)(s_gt[i].area + s_dt[j].area) - area_inter));
                } else {
                    const double* b = dt + (d0 + td + j) * 7;
                    const double* q = gt + (g0 + tg + i) * 7;
                    v = ke_d3(b, q, (float)area_inter, dt_f32, gt_f32);
                }
                out[o0 + (td + j) * ng + (tg + i)] = v;
            }
        }
    }
}

extern "C" int gga_kitti_eval_overlaps(const double* dt_boxes, const int64_t* dt_offsets, int64_t n_dt, const double* gt_boxes,
                                       const int64_t* gt_offsets, int64_t n_gt, int n_frames, int metric, int dt_f32, int gt_f32,
                                       float* overlaps, const int64_t* overlap_offsets, int64_t n_overlaps, void* stream) {
    GGA_REQUIRE(n_frames >= 1 && n_dt >= 0 && n_gt >= 0 && n_overlaps >= 0, "gga_kitti_eval_overlaps: bad sizes");
    GGA_REQUIRE(metric == 1 || metric == 2, "gga_kitti_eval_overlaps: metric %d is not 1 (bev) or 2 (3d)", metric);
    if (n_overlaps == 0) return GGA_OK;
    GGA_REQUIRE(dt_boxes && dt_offsets && gt_boxes && gt_offsets && overlaps && overlap_offsets,
                "gga_kitti_eval_overlaps: null pointer argument");
    hipLaunchKernelGGL(kitti_eval_overlaps_kernel, dim3(n_frames), dim3(256), 0, (hipStream_t)stream, dt_boxes, dt_offsets, n_dt,
                       gt_boxes, gt_offsets, n_gt, overlap_offsets, n_overlaps, metric, dt_f32, gt_f32, overlaps);
    GGA_CHECK_LAUNCH("kitti_eval_overlaps_kernel");
    return GGA_OK;
}

// ------------------------------------------------------------------------------------------------ statistics
struct KeFrame {
    const void* ov;          // [nd, ng] overlaps of the frame
    const double* dt;        // [nd, 6] bbox (4), alpha, score
    const double* galpha;    // [ng]
    const int8_t* ig;        // [ng] ignored_gt of the combination's (class, difficulty)
    const int8_t* id;        // [nd] ignored_det
    const double* dc;        // [ndc, 4]
    int nd, ng, ndc;
};

// image_box_overlap(dt_bboxes, dc_bboxes, criterion=0) for one pair: intersection over the detection's own area. The
// DontCare boxes are float64; with float32 detections (dt_f32) their area is float32 arithmetic and the result is rounded
// to float32, as `np.zeros((N, K), dtype=boxes.dtype)` does.
__device__ __forceinline__ double ke_dc_overlap(const double* b, const double* q, int dt_f32) {
    const double iw = fmin(b[2], q[2]) - fmax(b[0], q[0]);
    if (!(iw > 0)) return 0.0;
    const double ih = fmin(b[3], q[3]) - fmax(b[1], q[1]);
    if (!(ih > 0)) return 0.0;
    double ua;
    if (dt_f32) ua = (double)(((float)b[2] - (float)b[0]) * ((float)b[3] - (float)b[1]));
    else ua = (b[2] - b[0]) * (b[3] - b[1]);
    const double v = iw * ih / ua;
    return dt_f32 ? (double)(float)v : v;
}

// compute_statistics_jit for one frame, one combination and one score threshold. `assigned` is this lane's bit set of
// assigned detections (word w at assigned[w * 64]). tp_det (first pass only): det index of every true positive, else -1.
template <typename OvT>
__device__ void ke_frame_stats(const KeFrame& fr, int metric, double min_overlap, double thresh, bool compute_fp,
                               bool compute_aos, int dt_f32, uint32_t* assigned, int& tp, int& fp, int& fn, double& sim,
                               int32_t* tp_det) {
    const OvT* ov = (const OvT*)fr.ov;
    const int nd = fr.nd, ng = fr.ng;
    const double NO_DETECTION = -10000000.0;
    for (int w = 0; w < (nd + 31) / 32; ++w) assigned[w * 64] = 0u;
#define KE_BIT(j) ((assigned[((j) >> 5) * 64] >> ((j) & 31)) & 1u)
#define KE_SET(j) (assigned[((j) >> 5) * 64] |= 1u << ((j) & 31))
#define KE_SCORE(j) (fr.dt[(j) * 6 + 5])
    for (int i = 0; i < ng; ++i) {
        if (tp_det) tp_det[i] = -1;
        if (fr.ig[i] == -1) continue;
        int det_idx = -1;
        double valid_detection = NO_DETECTION, max_overlap = 0.0;
        bool assigned_ignored_det = false;
        for (int j = 0; j < nd; ++j) {
            if (fr.id[j] == -1) continue;
            if (KE_BIT(j)) continue;
            if (compute_fp && KE_SCORE(j) < thresh) continue;
            const double overlap = (double)ov[(int64_t)j * ng + i];
            const double dt_score = KE_SCORE(j);
            if (!compute_fp && overlap > min_overlap && dt_score > valid_detection) {
                det_idx = j;
                valid_detection = dt_score;
            } else if (compute_fp && overlap > min_overlap && (overlap > max_overlap || assigned_ignored_det) && fr.id[j] == 0) {
                max_overlap = overlap;
                det_idx = j;
                valid_detection = 1;
                assigned_ignored_det = false;
            } else if (compute_fp && overlap > min_overlap && valid_detection == NO_DETECTION && fr.id[j] == 1) {
                det_idx = j;
                valid_detection = 1;
                assigned_ignored_det = true;
            }
        }
        if (valid_detection == NO_DETECTION && fr.ig[i] == 0) {
            ++fn;
        } else if (valid_detection != NO_DETECTION && (fr.ig[i] == 1 || fr.id[det_idx] == 1)) {
            KE_SET(det_idx);
        } else if (valid_detection != NO_DETECTION) {
            ++tp;
            if (tp_det) tp_det[i] = det_idx;
            if (compute_aos) sim += (1.0 + cos(fr.galpha[i] - fr.dt[det_idx * 6 + 4])) / 2.0;
            KE_SET(det_idx);
        }
    }
    if (compute_fp) {
        for (int j = 0; j < nd; ++j)
            if (!(KE_BIT(j) || fr.id[j] == -1 || fr.id[j] == 1 || KE_SCORE(j) < thresh)) ++fp;
        int nstuff = 0;
        if (metric == 0) {
            for (int i = 0; i < fr.ndc; ++i)
                for (int j = 0; j < nd; ++j) {
                    if (KE_BIT(j)) continue;
                    if (fr.id[j] == -1 || fr.id[j] == 1) continue;
                    if (KE_SCORE(j) < thresh) continue;
                    if (ke_dc_overlap(fr.dt + j * 6, fr.dc + i * 4, dt_f32) > min_overlap) {
                        KE_SET(j);
                        ++nstuff;
                    }
                }
        }
        fp -= nstuff;
    }
#undef KE_BIT
#undef KE_SET
#undef KE_SCORE
}

struct KeArgs {
    const void* overlaps;
    const int64_t *ov_off, *dt_off, *gt_off, *dc_off;
    const double *dt_data, *gt_alpha, *dc_boxes;
    const int8_t *ign_gt, *ign_dt;            // [n_cd, n_gt], [n_cd, n_dt]
    const int32_t* combo_cd;                  // [n_combos] row of ign_gt / ign_dt
    const double* combo_min_overlap;          // [n_combos]
    const double* thresholds;                 // [n_combos, 41]
    const int32_t* n_thresholds;              // [n_combos]
    int64_t n_dt, n_gt, n_dc, n_ov;
    int n_frames, n_combos, n_cd, max_dt, metric, compute_aos, dt_f32, ov_f64;
};

// frame f of the batch, or false when its offsets do not fit the arrays (never for offsets built by cumulative sums)
__device__ __forceinline__ bool ke_load_frame(const KeArgs& a, int f, int cd, KeFrame& fr) {
    const int64_t d0 = a.dt_off[f], g0 = a.gt_off[f], c0 = a.dc_off[f], o0 = a.ov_off[f];
    const int64_t nd = a.dt_off[f + 1] - d0, ng = a.gt_off[f + 1] - g0, ndc = a.dc_off[f + 1] - c0;
    if (nd < 0 || ng < 0 || ndc < 0 || d0 < 0 || g0 < 0 || c0 < 0 || o0 < 0 || nd > a.max_dt || d0 + nd > a.n_dt ||
        g0 + ng > a.n_gt || c0 + ndc > a.n_dc || (ng > 0 && nd > (a.n_ov - o0) / ng))
        return false;
    fr.ov = (const char*)a.overlaps + o0 * (a.ov_f64 ? 8 : 4);
    fr.dt = a.dt_data + d0 * 6;
    fr.galpha = a.gt_alpha + g0;
    fr.ig = a.ign_gt + (int64_t)cd * a.n_gt + g0;
    fr.id = a.ign_dt + (int64_t)cd * a.n_dt + d0;
    fr.dc = a.dc_boxes + c0 * 4;
    fr.nd = (int)nd; fr.ng = (int)ng; fr.ndc = (int)ndc;
    return true;
}

// One lane per (frame, combination), 64 frames per wave; every lane walks its own frame, so all loads are per-lane.
// First pass (compute_fp = 0, thresh = 0): the matched detection of every ground truth goes to tp_det [n_combos, n_gt] (the
// host gathers their scores for get_thresholds). Second pass (fused_compute_statistics): the lane repeats the assignment for
// each of the combination's thresholds; the 64 frames of the wave are summed by the fixed butterfly of wave_sum (integers, and
// the float64 similarity) into partial [wave, combination, (tp, fp, fn), threshold], and kitti_eval_reduce_kernel adds the
// waves in order - no atomics, the same bits every run.
__global__ __launch_bounds__(64) void kitti_eval_stats_kernel(KeArgs a, int compute_fp, uint32_t* __restrict__ assigned_ws,
                                                              int words, int32_t* __restrict__ tp_det,
                                                              int32_t* __restrict__ part_cnt, double* __restrict__ part_sim) {
    const int f = blockIdx.x * 64 + threadIdx.x, c = blockIdx.y, lane = threadIdx.x;
    const int64_t blk = (int64_t)blockIdx.x * a.n_combos + c;
    KeFrame fr;
    const bool live = f < a.n_frames && ke_load_frame(a, f, a.combo_cd[c], fr);
    uint32_t* assigned = assigned_ws + blk * words * 64 + lane;
    const double mo = a.combo_min_overlap[c];
    if (!compute_fp) {
        if (!live) return;
        int tp = 0, fp = 0, fn = 0;
        double sim = 0.0;
        int32_t* out = tp_det + (int64_t)c * a.n_gt + a.gt_off[f];
        if (a.ov_f64) ke_frame_stats<double>(fr, a.metric, mo, 0.0, false, false, a.dt_f32, assigned, tp, fp, fn, sim, out);
        else ke_frame_stats<float>(fr, a.metric, mo, 0.0, false, false, a.dt_f32, assigned, tp, fp, fn, sim, out);
        return;
    }
    int nt = a.n_thresholds[c];
    nt = nt < 0 ? 0 : (nt > KE_SAMPLE_PTS ? KE_SAMPLE_PTS : nt);
    for (int t = 0; t < KE_SAMPLE_PTS; ++t) {          // uniform over the wave: every lane reaches every wave_sum
        int tp = 0, fp = 0, fn = 0;
        double sim = 0.0;
        if (live && t < nt) {
            const double thresh = a.thresholds[c * KE_SAMPLE_PTS + t];
            if (a.ov_f64) ke_frame_stats<double>(fr, a.metric, mo, thresh, true, a.compute_aos != 0, a.dt_f32, assigned, tp, fp, fn, sim, nullptr);
            else ke_frame_stats<float>(fr, a.metric, mo, thresh, true, a.compute_aos != 0, a.dt_f32, assigned, tp, fp, fn, sim, nullptr);
        }
        tp = wave_sum(tp);
        fp = wave_sum(fp);
        fn = wave_sum(fn);
        sim = wave_sum(sim);
        if (lane == 0) {
            part_cnt[(blk * 3 + 0) * 64 + t] = tp;
            part_cnt[(blk * 3 + 1) * 64 + t] = fp;
            part_cnt[(blk * 3 + 2) * 64 + t] = fn;
            part_sim[blk * 64 + t] = sim;
        }
    }
}

__global__ __launch_bounds__(64) void kitti_eval_reduce_kernel(const int32_t* __restrict__ part_cnt,
                                                               const double* __restrict__ part_sim, int n_chunks, int n_combos,
                                                               int64_t* __restrict__ counts, double* __restrict__ similarity) {
    const int c = blockIdx.x, lane = threadIdx.x;
    if (lane >= KE_SAMPLE_PTS) return;
    int64_t tp = 0, fp = 0, fn = 0;
    double sim = 0.0;
    for (int chunk = 0; chunk < n_chunks; ++chunk) {
        const int64_t blk = (int64_t)chunk * n_combos + c;
        tp += part_cnt[(blk * 3 + 0) * 64 + lane];
        fp += part_cnt[(blk * 3 + 1) * 64 + lane];
        fn += part_cnt[(blk * 3 + 2) * 64 + lane];
        sim += part_sim[blk * 64 + lane];
    }
    int64_t* o = counts + ((int64_t)c * KE_SAMPLE_PTS + lane) * 3;
    o[0] = tp; o[1] = fp; o[2] = fn;
    similarity[c * KE_SAMPLE_PTS + lane] = sim;
}

static inline int64_t ke_chunks(int n_frames) { return ((int64_t)n_frames + KE_CHUNK - 1) / KE_CHUNK; }
static inline int ke_words(int max_dt) { return max_dt > 0 ? (max_dt + 31) / 32 : 1; }

extern "C" size_t gga_kitti_eval_stats_workspace_bytes(int n_frames, int n_combos, int max_dt) {
    if (n_frames < 1 || n_combos < 1 || max_dt < 0) return 0;
    const size_t blocks = (size_t)ke_chunks(n_frames) * n_combos;
    return gga_align_up(blocks * ke_words(max_dt) * 64 * 4, 256) + gga_align_up(blocks * 3 * 64 * 4, 256) + blocks * 64 * 8;
}

extern "C" int gga_kitti_eval_stats(const void* overlaps, int overlaps_f64, const int64_t* overlap_offsets, int64_t n_overlaps,
                                    const int64_t* dt_offsets, const int64_t* gt_offsets, const int64_t* dc_offsets,
                                    const double* dt_data, int64_t n_dt, const double* gt_alpha, int64_t n_gt,
                                    const double* dc_boxes, int64_t n_dc, const int8_t* ignored_gt, const int8_t* ignored_dt,
                                    int n_cd, const int32_t* combo_cd, const double* combo_min_overlap, int n_combos,
                                    int n_frames, int max_dt, int metric, int dt_f32, int compute_fp, int compute_aos,
                                    const double* thresholds, const int32_t* n_thresholds, int32_t* tp_det, int64_t* counts,
                                    double* similarity, void* workspace, size_t workspace_bytes, void* stream) {
    GGA_REQUIRE(n_frames >= 1 && n_combos >= 1 && n_cd >= 1 && n_dt >= 0 && n_gt >= 0 && n_dc >= 0 && n_overlaps >= 0 &&
                    max_dt >= 0 && n_combos <= 65535,
                "gga_kitti_eval_stats: bad sizes");
    GGA_REQUIRE(metric >= 0 && metric <= 2, "gga_kitti_eval_stats: metric %d not in 0..2", metric);
    GGA_REQUIRE(overlap_offsets && dt_offsets && gt_offsets && dc_offsets && combo_cd && combo_min_overlap && workspace &&
                    (n_overlaps == 0 || overlaps) && (n_dt == 0 || (dt_data && ignored_dt)) &&
                    (n_gt == 0 || (gt_alpha && ignored_gt)) && (n_dc == 0 || dc_boxes),
                "gga_kitti_eval_stats: null pointer argument");
    if (compute_fp) GGA_REQUIRE(thresholds && n_thresholds && counts && similarity,
                                "gga_kitti_eval_stats: null pointer argument (compute_fp needs thresholds, counts, similarity)");
    else GGA_REQUIRE(n_gt == 0 || tp_det, "gga_kitti_eval_stats: null pointer argument (tp_det)");
    const size_t need = gga_kitti_eval_stats_workspace_bytes(n_frames, n_combos, max_dt);
    if (workspace_bytes < need) {
        gga_set_error("gga_kitti_eval_stats: workspace %zu B < required %zu B", workspace_bytes, need);
        return GGA_ERR_WORKSPACE;
    }
    KeArgs a;
    a.overlaps = overlaps; a.ov_off = overlap_offsets; a.dt_off = dt_offsets; a.gt_off = gt_offsets; a.dc_off = dc_offsets;
    a.dt_data = dt_data; a.gt_alpha = gt_alpha; a.dc_boxes = dc_boxes; a.ign_gt = ignored_gt; a.ign_dt = ignored_dt;
    a.combo_cd = combo_cd; a.combo_min_overlap = combo_min_overlap; a.thresholds = thresholds; a.n_thresholds = n_thresholds;
    a.n_dt = n_dt; a.n_gt = n_gt; a.n_dc = n_dc; a.n_ov = n_overlaps; a.n_frames = n_frames; a.n_combos = n_combos; a.n_cd = n_cd;
    a.max_dt = max_dt; a.metric = metric; a.compute_aos = compute_aos; a.dt_f32 = dt_f32; a.ov_f64 = overlaps_f64;
    const int words = ke_words(max_dt);
    const int64_t chunks = ke_chunks(n_frames);
    const size_t blocks = (size_t)chunks * n_combos;
    uint32_t* assigned = (uint32_t*)workspace;
    int32_t* part_cnt = (int32_t*)((char*)workspace + gga_align_up(blocks * words * 64 * 4, 256));
    double* part_sim = (double*)((char*)part_cnt + gga_align_up(blocks * 3 * 64 * 4, 256));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(kitti_eval_stats_kernel, dim3((unsigned)chunks, n_combos), dim3(64), 0, s, a, compute_fp, assigned, words, tp_det,
                       part_cnt, part_sim);
    GGA_CHECK_LAUNCH("kitti_eval_stats_kernel");
    if (!compute_fp) return GGA_OK;
    hipLaunchKernelGGL(kitti_eval_reduce_kernel, dim3(n_combos), dim3(64), 0, s, part_cnt, part_sim, (int)chunks, n_combos, counts,
                       similarity);
    GGA_CHECK_LAUNCH("kitti_eval_reduce_kernel");
    return GGA_OK;
}
