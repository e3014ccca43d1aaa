// Rotated BEV IoU of two rectangles (x, y, w, h, angle): the exact polygon overlap mmcv.ops.box_iou_rotated computes.
// Shared by postproc.hip (pairwise IoU, rotated NMS) and indoor_eval.hip (the 3D IoU of BaseInstance3DBoxes.overlaps).
#pragma once
#include "gga_common.h"

struct P2 { float x, y; };

__device__ __forceinline__ float cross2(P2 a, P2 b) { return a.x * b.y - a.y * b.x; }

// Every routine comes in two forms: the `_rot` one takes the boxes' cos / sin (a caller that meets a box in many pairs computes
// them once per box), the plain one computes them at the call. One body serves both: the same float operations on the same
// values, so the overlap is bit-identical whichever form is called.
__device__ __forceinline__ void rect_corners_rot(const float* b, float c, float s, float sx, float sy, P2 out[4]) {
    const float hw = b[2] * 0.5f, hh = b[3] * 0.5f;
    const float cx = b[0] - sx, cy = b[1] - sy;
    const float dx[4] = { -hw, hw, hw, -hw }, dy[4] = { -hh, -hh, hh, hh };
#pragma unroll
    for (int i = 0; i < 4; ++i) { out[i].x = cx + dx[i] * c - dy[i] * s; out[i].y = cy + dx[i] * s + dy[i] * c; }
}

__device__ __forceinline__ void rect_corners(const float* b, float sx, float sy, P2 out[4]) {
    rect_corners_rot(b, cosf(b[4]), sinf(b[4]), sx, sy, out);
}

// exact overlap area of two rotated rectangles (x, y, w, h, angle): Sutherland-Hodgman clip of
// rectangle 1 by the four half planes of rectangle 2 (both convex, counter-clockwise)
__device__ float rotated_inter_area_rot(const float* b1, float c1, float s1, const float* b2, float c2, float s2) {
    // shift both to their mid point for precision, as mmcv's box_iou_rotated_utils does
    const float sx = (b1[0] + b2[0]) * 0.5f, sy = (b1[1] + b2[1]) * 0.5f;
    P2 poly[10], tmp[10], q[4];
    rect_corners_rot(b1, c1, s1, sx, sy, poly);
    rect_corners_rot(b2, c2, s2, sx, sy, q);
    int n = 4;
    for (int e = 0; e < 4 && n > 0; ++e) {
        const P2 a = q[e], bq = q[(e + 1) & 3];
        const P2 ed = { bq.x - a.x, bq.y - a.y };
        int m = 0;
        for (int i = 0; i < n; ++i) {
            const P2 p = poly[i], r = poly[(i + 1) % n];
            const float dp = cross2(ed, P2{ p.x - a.x, p.y - a.y });
            const float dr = cross2(ed, P2{ r.x - a.x, r.y - a.y });
            if (dp >= 0.0f) tmp[m++] = p;
            if ((dp >= 0.0f) != (dr >= 0.0f)) {
                const float t = dp / (dp - dr);
                tmp[m++] = P2{ p.x + t * (r.x - p.x), p.y + t * (r.y - p.y) };
            }
        }
        n = m;
        for (int i = 0; i < n; ++i) poly[i] = tmp[i];
    }
    if (n < 3) return 0.0f;
    float area = 0.0f;
    for (int i = 0; i < n; ++i) area += cross2(poly[i], poly[(i + 1) % n]);
    return fabsf(area) * 0.5f;
}

__device__ __forceinline__ float rotated_inter_area(const float* b1, const float* b2) {
    return rotated_inter_area_rot(b1, cosf(b1[4]), sinf(b1[4]), b2, cosf(b2[4]), sinf(b2[4]));
}

__device__ __forceinline__ float rotated_iou_rot(const float* b1, float c1, float s1, const float* b2, float c2, float s2, int mode_iof) {
    const float a1 = b1[2] * b1[3], a2 = b2[2] * b2[3];
    if (a1 < 1e-14f || a2 < 1e-14f) return 0.0f;
    const float inter = rotated_inter_area_rot(b1, c1, s1, b2, c2, s2);
    const float base = mode_iof ? a1 : (a1 + a2 - inter);
    return inter / base;
}

__device__ __forceinline__ float rotated_iou(const float* b1, const float* b2, int mode_iof) {
    return rotated_iou_rot(b1, cosf(b1[4]), sinf(b1[4]), b2, cosf(b2[4]), sinf(b2[4]), mode_iof);
}
