// Indoor mAP / mAR evaluation (mmdet3d/core/evaluation/indoor_eval.py `eval_det_cls`) for all classes and frames at once.
//
// The host sorts detections and ground truths into (class, frame) segments, segment s = class * n_frames + frame, each side
// with one offsets array [n_segments + 1]; a segment may be empty on either side. Boxes are float32 rows (x, y, z_bottom, dx,
// dy, dz, yaw): the DepthInstance3DBoxes tensor with origin (0.5, 0.5, 0).
//
//   indoor_match_kernel   per detection the largest 3D IoU over the ground truths of its segment and that ground truth's index
//                         within the segment (`if iou > iou_max`: the first one that reaches the maximum; -inf / -1 without any)
//   indoor_claim_kernel   per (threshold, ground truth) the smallest output position among the detections that pick it with
//                         iou_max > threshold (atomicMin on int32)
//   indoor_flag_kernel    TP = the detection holds that minimum, everything else FP
//
// The reference marks ground truths while it walks the detections of a class in descending score order; a detection whose best
// ground truth is taken is a false positive, it does not look for a second best. So the detection that gets a ground truth at a
// threshold is the first, in that order, among those that pick it and pass the threshold - a minimum, which does not depend on the
// order the atomics arrive in. The output position (class start + rank within the class) is unique per detection.
//
// 3D IoU: BaseInstance3DBoxes.overlaps(mode='iou') in float32 - BEV IoU of (x, y, dx, dy, yaw) by rotated_iou, the BEV overlap
// recovered as iou2d * (a1 + a2) / (1 + iou2d), times the height overlap, over max(v1 + v2 - overlap, 1e-8).
#include "gga_common.h"
#include "rotated_iou.h"

#define IE_MAX_THR 8          // GGA_INDOOR_EVAL_MAX_THRESHOLDS
#define IE_BLOCK 256

struct IeThresholds { float v[IE_MAX_THR]; };

__device__ __forceinline__ float indoor_iou3d(const float* d, const float* g) {
    const float bd[5] = { d[0], d[1], d[3], d[4], d[6] }, bg[5] = { g[0], g[1], g[3], g[4], g[6] };
    const float top = fminf(d[2] + d[5], g[2] + g[5]), bottom = fmaxf(d[2], g[2]);
    const float ov_h = fmaxf(top - bottom, 0.0f);
    const float iou2d = rotated_iou(bd, bg, 0);
    const float a1 = bd[2] * bd[3], a2 = bg[2] * bg[3];
    const float ov_bev = iou2d * (a1 + a2) / (1.0f + iou2d);
    const float ov3d = ov_bev * ov_h;
    const float v1 = a1 * d[5], v2 = a2 * g[5];
    return ov3d / fmaxf(v1 + v2 - ov3d, 1e-8f);
}

// segment s with off[s] <= i < off[s + 1] (the last one that starts at or before i: empty segments are stepped over)
__device__ __forceinline__ int indoor_segment_of(const int64_t* __restrict__ off, int n_segments, int64_t i) {
    int lo = 0, hi = n_segments;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (off[mid] <= i) lo = mid; else hi = mid; }
    return lo;
}

// one thread per detection: the lanes of a wave are neighbours in segment order and read the same few ground-truth rows. (A wave
// per detection with a butterfly over the lanes was measured too: segments hold 0 to about 10 ground truths, 60 lanes idle, and
// it took 571 us where this takes 92 us at SUN RGB-D val size - EXPERIMENTS.md 6j.)
__global__ __launch_bounds__(IE_BLOCK) void indoor_match_kernel(const float* __restrict__ det, const int64_t* __restrict__ det_off,
                                                                int64_t n_det, const float* __restrict__ gt,
                                                                const int64_t* __restrict__ gt_off, int64_t n_gt, int n_segments,
                                                                float* __restrict__ iou_max, int32_t* __restrict__ jmax) {
    const int64_t i = (int64_t)blockIdx.x * IE_BLOCK + threadIdx.x;
    if (i >= n_det) return;
    const int s = indoor_segment_of(det_off, n_segments, i);
    int64_t g0 = gt_off[s], g1 = gt_off[s + 1];
    if (g0 < 0 || g1 < g0 || g1 > n_gt) g1 = g0 = 0;              // offsets that do not fit the totals: no ground truth
    float d[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) d[k] = det[i * 7 + k];
    float best = -INFINITY;
    int32_t arg = -1;
    for (int64_t g = g0; g < g1; ++g) {
        const float v = indoor_iou3d(d, gt + g * 7);
        if (v > best) { best = v; arg = (int32_t)(g - g0); }
    }
    iou_max[i] = best;
    jmax[i] = arg;
}

__global__ __launch_bounds__(IE_BLOCK) void indoor_claim_kernel(const float* __restrict__ iou_max, const int32_t* __restrict__ jmax,
                                                                const int32_t* __restrict__ det_pos, const int64_t* __restrict__ det_off,
                                                                int64_t n_det, const int64_t* __restrict__ gt_off, int64_t n_gt,
                                                                int n_segments, IeThresholds thr, int n_thr, int32_t* __restrict__ claim) {
    const int64_t i = (int64_t)blockIdx.x * IE_BLOCK + threadIdx.x;
    if (i >= n_det) return;
    const int32_t j = jmax[i];
    if (j < 0) return;
    const int s = indoor_segment_of(det_off, n_segments, i);
    const int64_t g = gt_off[s] + j;
    if (g < 0 || g >= n_gt || g >= gt_off[s + 1]) return;
    const float v = iou_max[i];
    const int32_t pos = det_pos[i];
    for (int t = 0; t < n_thr; ++t)
        if (v > thr.v[t]) atomicMin(&claim[(int64_t)t * n_gt + g], pos);
}

__global__ __launch_bounds__(IE_BLOCK) void indoor_flag_kernel(const float* __restrict__ iou_max, const int32_t* __restrict__ jmax,
                                                               const int32_t* __restrict__ det_pos, const int64_t* __restrict__ det_off,
                                                               int64_t n_det, const int64_t* __restrict__ gt_off, int64_t n_gt,
                                                               int n_segments, IeThresholds thr, int n_thr,
                                                               const int32_t* __restrict__ claim, uint8_t* __restrict__ tp) {
    const int64_t i = (int64_t)blockIdx.x * IE_BLOCK + threadIdx.x;
    if (i >= n_det) return;
    const int32_t pos = det_pos[i];
    if (pos < 0 || pos >= n_det) return;                           // a position outside the output: nothing written
    const int32_t j = jmax[i];
    int64_t g = -1;
    if (j >= 0) {
        const int s = indoor_segment_of(det_off, n_segments, i);
        g = gt_off[s] + j;
        if (g < 0 || g >= n_gt || g >= gt_off[s + 1]) g = -1;
    }
    const float v = iou_max[i];
    for (int t = 0; t < n_thr; ++t)
        tp[(int64_t)t * n_det + pos] = (g >= 0 && v > thr.v[t] && claim[(int64_t)t * n_gt + g] == pos) ? 1 : 0;
}

extern "C" int gga_indoor_eval_match(const float* det_boxes, const int64_t* det_offsets, int64_t n_det, const float* gt_boxes,
                                     const int64_t* gt_offsets, int64_t n_gt, int n_segments, float* iou_max, int32_t* jmax,
                                     void* stream) {
    GGA_REQUIRE(n_det >= 0 && n_gt >= 0 && n_segments >= 0, "gga_indoor_eval_match: negative size (n_det %lld, n_gt %lld, n_segments %d)",
                (long long)n_det, (long long)n_gt, n_segments);
    if (n_det == 0) return GGA_OK;
    GGA_REQUIRE(n_segments >= 1, "gga_indoor_eval_match: detections without a segment");
    GGA_REQUIRE(det_boxes && det_offsets && gt_offsets && iou_max && jmax && (n_gt == 0 || gt_boxes),
                "gga_indoor_eval_match: null pointer argument");
    hipLaunchKernelGGL(indoor_match_kernel, dim3((unsigned)((n_det + IE_BLOCK - 1) / IE_BLOCK)), dim3(IE_BLOCK), 0, (hipStream_t)stream,
                       det_boxes, det_offsets, n_det, gt_boxes, gt_offsets, n_gt, n_segments, iou_max, jmax);
    GGA_CHECK_LAUNCH("indoor_match_kernel");
    return GGA_OK;
}

extern "C" size_t gga_indoor_eval_workspace_bytes(int64_t n_gt, int n_thresholds) {
    return (size_t)(n_gt > 0 ? n_gt : 0) * (size_t)(n_thresholds > 0 ? n_thresholds : 0) * 4 + 16;
}

extern "C" int gga_indoor_eval_assign(const float* iou_max, const int32_t* jmax, const int32_t* det_pos, const int64_t* det_offsets,
                                      int64_t n_det, const int64_t* gt_offsets, int64_t n_gt, int n_segments,
                                      const float* thresholds_host, int n_thresholds, uint8_t* tp, void* workspace,
                                      size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GGA_REQUIRE(n_det >= 0 && n_gt >= 0 && n_segments >= 0, "gga_indoor_eval_assign: negative size");
    GGA_REQUIRE(n_det < 0x7f7f7f7f, "gga_indoor_eval_assign: %lld detections do not fit the int32 positions", (long long)n_det);
    GGA_REQUIRE(n_thresholds >= 1 && n_thresholds <= IE_MAX_THR && thresholds_host,
                "gga_indoor_eval_assign: n_thresholds=%d not in [1, %d] (or null thresholds)", n_thresholds, IE_MAX_THR);
    if (n_det == 0) return GGA_OK;
    GGA_REQUIRE(n_segments >= 1, "gga_indoor_eval_assign: detections without a segment");
    GGA_REQUIRE(iou_max && jmax && det_pos && det_offsets && gt_offsets && tp && workspace, "gga_indoor_eval_assign: null pointer argument");
    if (workspace_bytes < gga_indoor_eval_workspace_bytes(n_gt, n_thresholds)) {
        gga_set_error("gga_indoor_eval_assign: workspace %zu B < required %zu B", workspace_bytes,
                      gga_indoor_eval_workspace_bytes(n_gt, n_thresholds));
        return GGA_ERR_WORKSPACE;
    }
    IeThresholds thr;
    for (int t = 0; t < IE_MAX_THR; ++t) thr.v[t] = t < n_thresholds ? thresholds_host[t] : INFINITY;
    int32_t* claim = (int32_t*)workspace;
    const unsigned blocks = (unsigned)((n_det + IE_BLOCK - 1) / IE_BLOCK);
    if (n_gt > 0) {
        // 0x7f7f7f7f: above every position
        GGA_CHECK_HIP(hipMemsetAsync(claim, 0x7f, (size_t)n_gt * n_thresholds * 4, stream), "indoor_eval memset");
        hipLaunchKernelGGL(indoor_claim_kernel, dim3(blocks), dim3(IE_BLOCK), 0, stream, iou_max, jmax, det_pos, det_offsets, n_det,
                           gt_offsets, n_gt, n_segments, thr, n_thresholds, claim);
        GGA_CHECK_LAUNCH("indoor_claim_kernel");
    }
    hipLaunchKernelGGL(indoor_flag_kernel, dim3(blocks), dim3(IE_BLOCK), 0, stream, iou_max, jmax, det_pos, det_offsets, n_det, gt_offsets,
                       n_gt, n_segments, thr, n_thresholds, claim, tp);
    GGA_CHECK_LAUNCH("indoor_flag_kernel");
    return GGA_OK;
}
