// KITTI result formatting of a whole test run (mmdet3d/datasets/kitti_dataset_GGA_train.py `convert_valid_bboxes` +
// `bbox2result_kitti`): LiDAR detections -> the annotation columns kitti_eval and the submission writer read, the invalid
// ones dropped, in one launch for all frames.
//
// Arithmetic. Every step is the float32 operation the host path (torch CPU on float32 tensors) performs, in its order:
// limit_yaw, Box3DMode LIDAR -> CAM, CameraInstance3DBoxes.corners, points_cam2img, min / max, the two validity tests, the
// clip to the image, alpha. Python scalars that meet a float32 tensor are cast to float32 first (2 pi, pi / 2, 0.5), the
// matrix products are sums of float32 products from left to right, and no multiply-add is contracted into an fma (pragma
// below, -ffp-contract=off in the Makefile). sin / cos / atan2 are evaluated in double and rounded: the correctly rounded
// float32 value of the float32 operation, whatever math library the host side was built with.
//
// Compaction. One wave per frame walks the frame's detections 64 at a time: a ballot of the validity flags, the rank of a
// lane among the valid lanes below it, a running base - the valid detections of frame f land at rows
// frame_offsets[f] .. frame_offsets[f] + valid_counts[f] in their original order, for any count per frame.
#include "gga_common.h"

#pragma clang fp contract(off)

#define KF_COLS 20            // GGA_KITTI_FORMAT_COLS
#define KF_WAVES 4            // frames per block

struct KfRange { float v[6]; };

__device__ __forceinline__ float kf_limit_period(float val, float offset, float period) {
    return val - floorf(val / period + offset) * period;
}

__global__ __launch_bounds__(KF_WAVES * GGA_WAVE) void kitti_format_kernel(
    const float* __restrict__ boxes, const float* __restrict__ scores, const int64_t* __restrict__ labels, int64_t n_dets,
    const int64_t* __restrict__ frame_offsets, int n_frames, const float* __restrict__ lidar2cam, const float* __restrict__ p2,
    const int32_t* __restrict__ image_hw, KfRange range, float* __restrict__ out_cols, int64_t* __restrict__ out_labels,
    float* __restrict__ out_yaw, int32_t* __restrict__ valid_counts) {
    const int lane = threadIdx.x & (GGA_WAVE - 1);
    const int frame = blockIdx.x * KF_WAVES + (threadIdx.x >> 6);        // wave-uniform
    if (frame >= n_frames) return;
    const int64_t begin = frame_offsets[frame], end = frame_offsets[frame + 1];
    if (begin < 0 || end < begin || end > n_dets) {                      // offsets that do not fit the totals: nothing written
        if (lane == 0) valid_counts[frame] = 0;
        return;
    }
    const float* rt = lidar2cam + (int64_t)frame * 16;
    const float* pm = p2 + (int64_t)frame * 16;
    const float img_h = (float)image_hw[2 * frame], img_w = (float)image_hw[2 * frame + 1];
    const float two_pi = (float)(2.0 * M_PI), half_pi = (float)(M_PI / 2.0);
    int base = 0;
    for (int64_t chunk = begin; chunk < end; chunk += GGA_WAVE) {        // trip count is the same for all lanes of the wave
        const int64_t i = chunk + lane;
        const bool live = i < end;
        bool valid = false;
        float col[KF_COLS];
        int64_t label = 0;
        if (live) {
            const float* b = boxes + i * 7;
            const float x = b[0], y = b[1], z = b[2], dx = b[3], dy = b[4], dz = b[5];
            const float yaw = kf_limit_period(b[6], 0.5f, two_pi);       // box_preds.limit_yaw(offset=0.5, period=2 pi)
            out_yaw[i] = yaw;
            // lidar_boxes_to_camera: sizes (x, y, z) -> (x, z, y), yaw -> limit_period(-yaw - pi/2, 2 pi), centre through rt
            const float sx = dx, sy = dz, sz = dy;
            const float ry = kf_limit_period(-yaw - half_pi, 0.5f, two_pi);
            float c[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) c[r] = x * rt[4 * r] + y * rt[4 * r + 1] + z * rt[4 * r + 2] + rt[4 * r + 3];
            // corners: dims * (a - 0.5, b - 1, c - 0.5), rotated about the camera's y axis, moved to the centre; projected by P2
            const float cs = (float)cos((double)ry), sn = (float)sin((double)ry);
            float minx = INFINITY, miny = INFINITY, maxx = -INFINITY, maxy = -INFINITY;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float px = sx * ((k & 4) ? 0.5f : -0.5f);
                const float py = sy * ((k & 2) ? 0.f : -1.f);
                const float pz = sz * ((k & 1) ? 0.5f : -0.5f);
                const float qx = px * cs + pz * sn + c[0];
                const float qy = py + c[1];
                const float qz = px * -sn + pz * cs + c[2];
                const float u = qx * pm[0] + qy * pm[1] + qz * pm[2] + pm[3];
                const float v = qx * pm[4] + qy * pm[5] + qz * pm[6] + pm[7];
                const float w = qx * pm[8] + qy * pm[9] + qz * pm[10] + pm[11];
                const float iu = u / w, iv = v / w;
                minx = fminf(minx, iu);
                maxx = fmaxf(maxx, iu);
                miny = fminf(miny, iv);
                maxy = fmaxf(maxy, iv);
            }
            const bool in_image = minx < img_w && miny < img_h && maxx > 0.f && maxy > 0.f;
            const bool in_range = x > range.v[0] && y > range.v[1] && z > range.v[2] && x < range.v[3] && y < range.v[4] && z < range.v[5];
            valid = in_image && in_range;
            // bbox2result_kitti: the 2D box clipped to the image, alpha = -atan2(-y, x) + rotation_y
            col[0] = fmaxf(minx, 0.f);
            col[1] = fmaxf(miny, 0.f);
            col[2] = fminf(maxx, img_w);
            col[3] = fminf(maxy, img_h);
            col[4] = sx; col[5] = sy; col[6] = sz;
            col[7] = c[0]; col[8] = c[1]; col[9] = c[2];
            col[10] = ry;
            col[11] = -(float)atan2((double)-y, (double)x) + ry;
            col[12] = scores[i];
            col[13] = x; col[14] = y; col[15] = z; col[16] = dx; col[17] = dy; col[18] = dz; col[19] = yaw;
            label = labels[i];
        }
        const unsigned long long mask = __ballot(valid);
        if (valid) {
            const int64_t row = begin + base + __popcll(mask & ((1ull << lane) - 1ull));     // < end <= n_dets
            float* o = out_cols + row * KF_COLS;
#pragma unroll
            for (int k = 0; k < KF_COLS; ++k) o[k] = col[k];
            out_labels[row] = label;
        }
        base += __popcll(mask);
    }
    if (lane == 0) valid_counts[frame] = base;
}

extern "C" int gga_kitti_format_dets(const float* boxes, const float* scores, const int64_t* labels, int64_t n_dets,
                                     const int64_t* frame_offsets, int n_frames, const float* lidar2cam, const float* p2,
                                     const int32_t* image_hw, const float* limit_range_host, float* out_cols,
                                     int64_t* out_labels, float* out_yaw, int32_t* valid_counts, void* stream) {
    GGA_REQUIRE(n_dets >= 0 && n_frames >= 0, "gga_kitti_format_dets: negative size (n_dets %lld, n_frames %d)", (long long)n_dets, n_frames);
    GGA_REQUIRE(limit_range_host, "gga_kitti_format_dets: null pointer (limit_range_host)");
    if (n_frames == 0) return GGA_OK;
    GGA_REQUIRE(frame_offsets && lidar2cam && p2 && image_hw && valid_counts, "gga_kitti_format_dets: null pointer (per-frame arrays)");
    GGA_REQUIRE(n_dets == 0 || (boxes && scores && labels && out_cols && out_labels && out_yaw),
                "gga_kitti_format_dets: null pointer (per-detection arrays)");
    KfRange range;
    for (int k = 0; k < 6; ++k) range.v[k] = limit_range_host[k];
    const int blocks = (n_frames + KF_WAVES - 1) / KF_WAVES;
    hipLaunchKernelGGL(kitti_format_kernel, dim3(blocks), dim3(KF_WAVES * GGA_WAVE), 0, (hipStream_t)stream, boxes, scores, labels,
                       n_dets, frame_offsets, n_frames, lidar2cam, p2, image_hw, range, out_cols, out_labels, out_yaw, valid_counts);
    GGA_CHECK_LAUNCH("gga_kitti_format_dets");
    return GGA_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The camera-box variant (mmdet3d/datasets/kitti_mono_dataset.py `convert_valid_bboxes` :497-561 + `bbox2result_kitti`
// :302-334): the detections of the image branch are camera boxes already, so there is no yaw limit, no change of frame and no
// LiDAR range test - corners, projection by P2, min / max, valid = the 2D box meets the image, the clip, and
// alpha = -atan2(x, z) + rotation_y. The reference also converts the boxes to the LiDAR frame and never reads the result;
// that is left out. Same compaction and the same arithmetic rules as above.
#define KFC_COLS 13           // GGA_KITTI_FORMAT_CAM_COLS

__global__ __launch_bounds__(KF_WAVES * GGA_WAVE) void kitti_format_cam_kernel(
    const float* __restrict__ boxes, const float* __restrict__ scores, const int64_t* __restrict__ labels, int64_t n_dets,
    const int64_t* __restrict__ frame_offsets, int n_frames, const float* __restrict__ p2, const int32_t* __restrict__ image_hw,
    float* __restrict__ out_cols, int64_t* __restrict__ out_labels, int32_t* __restrict__ valid_counts) {
    const int lane = threadIdx.x & (GGA_WAVE - 1);
    const int frame = blockIdx.x * KF_WAVES + (threadIdx.x >> 6);        // wave-uniform
    if (frame >= n_frames) return;
    const int64_t begin = frame_offsets[frame], end = frame_offsets[frame + 1];
    if (begin < 0 || end < begin || end > n_dets) {                      // offsets that do not fit the totals: nothing written
        if (lane == 0) valid_counts[frame] = 0;
        return;
    }
    const float* pm = p2 + (int64_t)frame * 16;
    const float img_h = (float)image_hw[2 * frame], img_w = (float)image_hw[2 * frame + 1];
    int base = 0;
    for (int64_t chunk = begin; chunk < end; chunk += GGA_WAVE) {        // trip count is the same for all lanes of the wave
        const int64_t i = chunk + lane;
        const bool live = i < end;
        bool valid = false;
        float col[KFC_COLS];
        int64_t label = 0;
        if (live) {
            const float* b = boxes + i * 7;
            const float x = b[0], y = b[1], z = b[2], sx = b[3], sy = b[4], sz = b[5], ry = b[6];
            // corners: dims * (a - 0.5, b - 1, c - 0.5), rotated about the camera's y axis, moved to the centre; projected by P2
            const float cs = (float)cos((double)ry), sn = (float)sin((double)ry);
            float minx = INFINITY, miny = INFINITY, maxx = -INFINITY, maxy = -INFINITY;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float px = sx * ((k & 4) ? 0.5f : -0.5f);
                const float py = sy * ((k & 2) ? 0.f : -1.f);
                const float pz = sz * ((k & 1) ? 0.5f : -0.5f);
                const float qx = px * cs + pz * sn + x;
                const float qy = py + y;
                const float qz = px * -sn + pz * cs + z;
                const float u = qx * pm[0] + qy * pm[1] + qz * pm[2] + pm[3];
                const float v = qx * pm[4] + qy * pm[5] + qz * pm[6] + pm[7];
                const float w = qx * pm[8] + qy * pm[9] + qz * pm[10] + pm[11];
                const float iu = u / w, iv = v / w;
                minx = fminf(minx, iu);
                maxx = fmaxf(maxx, iu);
                miny = fminf(miny, iv);
                maxy = fmaxf(maxy, iv);
            }
            valid = minx < img_w && miny < img_h && maxx > 0.f && maxy > 0.f;
            col[0] = fmaxf(minx, 0.f);
            col[1] = fmaxf(miny, 0.f);
            col[2] = fminf(maxx, img_w);
            col[3] = fminf(maxy, img_h);
            col[4] = sx; col[5] = sy; col[6] = sz;
            col[7] = x; col[8] = y; col[9] = z;
            col[10] = ry;
            col[11] = -(float)atan2((double)x, (double)z) + ry;
            col[12] = scores[i];
            label = labels[i];
        }
        const unsigned long long mask = __ballot(valid);
        if (valid) {
            const int64_t row = begin + base + __popcll(mask & ((1ull << lane) - 1ull));     // < end <= n_dets
            float* o = out_cols + row * KFC_COLS;
#pragma unroll
            for (int k = 0; k < KFC_COLS; ++k) o[k] = col[k];
            out_labels[row] = label;
        }
        base += __popcll(mask);
    }
    if (lane == 0) valid_counts[frame] = base;
}

extern "C" int gga_kitti_format_dets_cam(const float* boxes, const float* scores, const int64_t* labels, int64_t n_dets,
                                         const int64_t* frame_offsets, int n_frames, const float* p2, const int32_t* image_hw,
                                         float* out_cols, int64_t* out_labels, int32_t* valid_counts, void* stream) {
    GGA_REQUIRE(n_dets >= 0 && n_frames >= 0, "gga_kitti_format_dets_cam: negative size (n_dets %lld, n_frames %d)", (long long)n_dets, n_frames);
    if (n_frames == 0) return GGA_OK;
    GGA_REQUIRE(frame_offsets && p2 && image_hw && valid_counts, "gga_kitti_format_dets_cam: null pointer (per-frame arrays)");
    GGA_REQUIRE(n_dets == 0 || (boxes && scores && labels && out_cols && out_labels),
                "gga_kitti_format_dets_cam: null pointer (per-detection arrays)");
    const int blocks = (n_frames + KF_WAVES - 1) / KF_WAVES;
    hipLaunchKernelGGL(kitti_format_cam_kernel, dim3(blocks), dim3(KF_WAVES * GGA_WAVE), 0, (hipStream_t)stream, boxes, scores, labels,
                       n_dets, frame_offsets, n_frames, p2, image_hw, out_cols, out_labels, valid_counts);
    GGA_CHECK_LAUNCH("gga_kitti_format_dets_cam");
    return GGA_OK;
}
