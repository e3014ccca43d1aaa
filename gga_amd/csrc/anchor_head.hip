// Anchor3DHead on the device (gfx950): the targets of a whole batch, the three losses of a whole batch, and the gather + decode
// of the kept anchors of a whole batch.
//
// Reference: mmdet3d/models/dense_heads/train_mixins.py:63-80,126-183 (a Python loop over frames and, inside a frame, over the
// class groups: per group an IoU matrix, a few `max` calls, a loop over the ground truths and several `nonzero` calls),
// core/bbox/iou_calculators/iou3d_calculator.py:99-145 with structures/base_box3d.py:144-162 (nearest-BEV IoU),
// core/bbox/coders/delta_xyzwhlr_bbox_coder.py:20-91, train_mixins.py:319-349 (direction target) and
// dense_heads/anchor3d_head.py:194-278 (loss_single), :427-516 (get_bboxes_single). mmdet's MaxIoUAssigner is restated from its
// published behaviour (gga_amd/anchor_head.py::MaxIoUAssigner states the rule).
//
// Targets: two launches ordered by the stream. Pass 1 finds, per (frame, group, ground truth), the largest IoU over the group's
// anchors - an integer atomicMax on the bit pattern (IoU >= 0, so the order is the float order), reduced per wave first, and
// only by waves that overlap the ground truth at all. Pass 2 recomputes the same IoUs through the same function, applies the
// assigner's rule, encodes the positives and writes every output element.
//
// The file is compiled with -ffp-contract=off (Makefile): where the reference does separate f32 operations, so does this.
#include <float.h>
#include <math.h>

#include "gga_common.h"

#define AH_THREADS 256
#define AH_CHUNK 64

#define AH_PI ((float)M_PI)
#define AH_TWO_PI ((float)(2.0 * M_PI))
#define AH_QUARTER_PI ((float)(M_PI / 4.0))

struct ah_bev {
    float x1, y1, x2, y2, area;
};

// core/bbox/structures/utils.py:11-25, one rounded f32 operation per tensor operation
__device__ __forceinline__ float ah_limit_period(float val, float offset, float period) {
    return __fsub_rn(val, __fmul_rn(floorf(__fadd_rn(__fdiv_rn(val, period), offset)), period));
}

// base_box3d.py:144-162 and the area of mmdet's bbox_overlaps: box = (x, y, z, dx, dy, dz, yaw)
__device__ __forceinline__ ah_bev ah_nearest_bev(const float* __restrict__ b) {
    const float normed = fabsf(ah_limit_period(b[6], 0.5f, AH_PI));
    const bool swap = normed > AH_QUARTER_PI;
    const float w = swap ? b[4] : b[3], h = swap ? b[3] : b[4];
    const float hw = __fmul_rn(w, 0.5f), hh = __fmul_rn(h, 0.5f);        // dims / 2
    ah_bev r;
    r.x1 = __fsub_rn(b[0], hw);
    r.y1 = __fsub_rn(b[1], hh);
    r.x2 = __fadd_rn(b[0], hw);
    r.y2 = __fadd_rn(b[1], hh);
    r.area = __fmul_rn(__fsub_rn(r.x2, r.x1), __fsub_rn(r.y2, r.y1));
    return r;
}

// bbox_overlaps(gt, anchor) with eps = 1e-6 on the union. Both passes call this one function: the same bits. A pair that fails
// the interval test has overlap clamp(.., 0) = 0 and IoU 0 / max(union, eps) = 0.
__device__ __forceinline__ float ah_iou(const ah_bev& g, const ah_bev& a) {
    const float w = __fsub_rn(fminf(g.x2, a.x2), fmaxf(g.x1, a.x1));
    const float h = __fsub_rn(fminf(g.y2, a.y2), fmaxf(g.y1, a.y1));
    if (!(w > 0.0f && h > 0.0f)) return 0.0f;
    const float overlap = __fmul_rn(w, h);
    const float uni = fmaxf(__fsub_rn(__fadd_rn(g.area, a.area), overlap), 1e-6f);
    return __fdiv_rn(overlap, uni);
}

__device__ __forceinline__ bool ah_visible(int64_t label, int group, const gga_anchor_params& P) {
    return label >= 0 && label < P.num_classes && (!P.assign_per_class || label == group);
}

// ----------------------------------------------------------------------------- targets, pass 1
// grid (ceil(A / n_groups / 256), n_groups, B): a workgroup holds anchors of ONE group, so a wave's maximum belongs to one
// (group, ground truth) cell of gt_max [n_groups, N].
__global__ __launch_bounds__(AH_THREADS) void anchor_gt_max_kernel(
    const float* __restrict__ anchors, int A, gga_anchor_params P, const float* __restrict__ boxes,
    const int64_t* __restrict__ labels, int N, const int32_t* __restrict__ frame_offsets, uint32_t* __restrict__ gt_max) {
    const int b = blockIdx.z, g = blockIdx.y, tid = threadIdx.x;
    const int per_group = A / P.n_groups;
    const int j = blockIdx.x * AH_THREADS + tid;
    const bool valid = j < per_group;
    __shared__ ah_bev s_gt[AH_CHUNK];
    __shared__ int s_vis[AH_CHUNK];
    ah_bev mine = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (valid) {
        const int a = ((j / P.n_rot) * P.n_groups + g) * P.n_rot + j % P.n_rot;
        mine = ah_nearest_bev(anchors + (int64_t)a * 7);
    }
    const int o0 = frame_offsets[b];
    const int n = frame_offsets[b + 1] - o0;
    for (int c0 = 0; c0 < n; c0 += AH_CHUNK) {
        __syncthreads();
        if (tid < AH_CHUNK) {
            const int i = c0 + tid;
            int vis = 0;
            if (i < n) {
                vis = ah_visible(labels[o0 + i], g, P) ? 1 : 0;
                s_gt[tid] = ah_nearest_bev(boxes + (int64_t)(o0 + i) * 7);
            }
            s_vis[tid] = vis;
        }
        __syncthreads();
        const int m = min(AH_CHUNK, n - c0);
        for (int jj = 0; jj < m; ++jj) {
            if (!s_vis[jj]) continue;
            float v = valid ? ah_iou(s_gt[jj], mine) : 0.0f;
            if (__ballot(v > 0.0f) == 0) continue;                 // most waves overlap nothing: they issue nothing
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
            if ((tid & 63) == 0) {
                uint32_t* cell = gt_max + (int64_t)g * N + (o0 + c0 + jj);
                const uint32_t bits = __float_as_uint(v);
                if (bits > __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(cell, bits);
            }
        }
    }
}

// ----------------------------------------------------------------------------- targets, pass 2
// grid (ceil(A / 256), B): thread = anchor, in head order, so that the outputs are written in rows.
__global__ __launch_bounds__(AH_THREADS) void anchor_assign_kernel(
    const float* __restrict__ anchors, int A, gga_anchor_params P, const float* __restrict__ boxes,
    const int64_t* __restrict__ labels, int N, const int32_t* __restrict__ frame_offsets, const uint32_t* __restrict__ gt_max,
    int64_t* __restrict__ out_labels, float* __restrict__ label_weights, float* __restrict__ bbox_targets,
    uint8_t* __restrict__ pos_flag, int64_t* __restrict__ dir_targets, float* __restrict__ dir_weights,
    int32_t* __restrict__ pos_count) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const int a = blockIdx.x * AH_THREADS + tid;
    const bool valid = a < A;
    __shared__ ah_bev s_gt[AH_CHUNK];
    __shared__ int s_lab[AH_CHUNK];
    __shared__ float s_gmax[GGA_ANCHOR_MAX_GROUPS * AH_CHUNK];
    __shared__ float s_thr[3 * GGA_ANCHOR_MAX_GROUPS];
    if (tid < P.n_groups) {
        s_thr[tid] = P.pos_iou_thr[tid];
        s_thr[GGA_ANCHOR_MAX_GROUPS + tid] = P.neg_iou_thr[tid];
        s_thr[2 * GGA_ANCHOR_MAX_GROUPS + tid] = P.min_pos_iou[tid];
    }
    float av[7] = {0.0f, 0.0f, 0.0f, 1.0f, 1.0f, 1.0f, 0.0f};
    if (valid)
        for (int k = 0; k < 7; ++k) av[k] = anchors[(int64_t)a * 7 + k];
    const ah_bev mine = ah_nearest_bev(av);
    const int g = valid ? (a / P.n_rot) % P.n_groups : 0;
    const int o0 = frame_offsets[b];
    const int n = frame_offsets[b + 1] - o0;
    float best = -1.0f;
    int arg = -1, low = -1;
    for (int c0 = 0; c0 < n; c0 += AH_CHUNK) {
        __syncthreads();                                            // (also orders the thresholds before their first read)
        const int m = min(AH_CHUNK, n - c0);
        if (tid < AH_CHUNK) {
            int lab = -1;
            if (tid < m) {
                const int64_t l = labels[o0 + c0 + tid];
                lab = (l >= 0 && l < P.num_classes) ? (int)l : -1;
                s_gt[tid] = ah_nearest_bev(boxes + (int64_t)(o0 + c0 + tid) * 7);
            }
            s_lab[tid] = lab;
        }
        for (int t = tid; t < P.n_groups * AH_CHUNK; t += AH_THREADS) {
            const int gg = t / AH_CHUNK, jj = t - gg * AH_CHUNK;
            s_gmax[t] = jj < m ? __uint_as_float(gt_max[(int64_t)gg * N + (o0 + c0 + jj)]) : 0.0f;
        }
        __syncthreads();
        if (!valid) continue;
        const float min_pos = s_thr[2 * GGA_ANCHOR_MAX_GROUPS + g];
        for (int jj = 0; jj < m; ++jj) {
            const int lab = s_lab[jj];
            if (lab < 0 || (P.assign_per_class && lab != g)) continue;
            const float v = ah_iou(s_gt[jj], mine);
            if (v > best) { best = v; arg = c0 + jj; }              // argmax: the lowest index among equal values
            const float gm = s_gmax[g * AH_CHUNK + jj];
            if (v == gm && gm >= min_pos) low = c0 + jj;            // ascending order: a later ground truth overwrites
        }
    }
    __syncthreads();
    int assigned = 0;                                               // no ground truth in sight: every anchor is negative
    if (arg >= 0) {
        assigned = -1;
        if (best >= 0.0f && best < s_thr[GGA_ANCHOR_MAX_GROUPS + g]) assigned = 0;
        if (best >= s_thr[g]) assigned = arg + 1;
        if (low >= 0) assigned = low + 1;
    }
    const bool pos = valid && assigned > 0;
    const uint64_t pos_lanes = __ballot(pos);
    if ((tid & 63) == 0 && pos_lanes) atomicAdd(pos_count + b, __popcll(pos_lanes));
    if (!valid) return;
    const int64_t row = (int64_t)b * A + a;
    float t[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    int64_t dir = 0;
    int64_t label = P.num_classes;
    if (pos) {
        const float* __restrict__ gt = boxes + (int64_t)(o0 + assigned - 1) * 7;
        label = labels[o0 + assigned - 1];
        float gv[7];
        for (int k = 0; k < 7; ++k) gv[k] = gt[k];
        // DeltaXYZWLHRBBoxCoder.encode(anchor, gt)
        const float za = __fadd_rn(av[2], __fmul_rn(av[5], 0.5f));
        const float zg = __fadd_rn(gv[2], __fmul_rn(gv[5], 0.5f));
        const float diagonal = __fsqrt_rn(__fadd_rn(__fmul_rn(av[4], av[4]), __fmul_rn(av[3], av[3])));
        t[0] = __fdiv_rn(__fsub_rn(gv[0], av[0]), diagonal);
        t[1] = __fdiv_rn(__fsub_rn(gv[1], av[1]), diagonal);
        t[2] = __fdiv_rn(__fsub_rn(zg, za), av[5]);
        t[3] = logf(__fdiv_rn(gv[3], av[3]));
        t[4] = logf(__fdiv_rn(gv[4], av[4]));
        t[5] = logf(__fdiv_rn(gv[5], av[5]));
        t[6] = __fsub_rn(gv[6], av[6]);
        // get_direction_target, num_bins = 2
        const float rot_gt = __fadd_rn(t[6], av[6]);
        const float offset_rot = ah_limit_period(__fsub_rn(rot_gt, P.dir_offset), P.dir_limit_offset, AH_TWO_PI);
        dir = floorf(__fdiv_rn(offset_rot, AH_PI)) >= 1.0f ? 1 : 0;          // floor, then clamp to [0, 1]
    }
    out_labels[row] = label;
    label_weights[row] = pos ? (P.pos_weight > 0.0f ? P.pos_weight : 1.0f) : (assigned == 0 ? 1.0f : 0.0f);
    for (int k = 0; k < 7; ++k) bbox_targets[row * 7 + k] = t[k];
    pos_flag[row] = pos ? 1 : 0;
    dir_targets[row] = dir;
    dir_weights[row] = pos ? 1.0f : 0.0f;
}

extern "C" size_t gga_anchor_targets_workspace_bytes(int64_t N, int n_groups) {
    if (N < 0 || n_groups < 1 || n_groups > GGA_ANCHOR_MAX_GROUPS) return 0;
    return gga_align_up((size_t)(N > 0 ? N : 1) * n_groups * sizeof(uint32_t), 256);
}

extern "C" int gga_anchor_targets(const float* anchors, int A, const gga_anchor_params* prm, const float* boxes,
                                  const int64_t* labels, int N, const int32_t* frame_offsets,
                                  const int32_t* frame_offsets_host, int B, int64_t* out_labels, float* label_weights,
                                  float* bbox_targets, uint8_t* pos_flag, int64_t* dir_targets, float* dir_weights,
                                  int32_t* pos_count, void* workspace, size_t workspace_bytes, void* stream_) {
    const char* fn = "gga_anchor_targets";
    hipStream_t stream = (hipStream_t)stream_;
    GGA_REQUIRE(prm, "%s: null params", fn);
    GGA_REQUIRE(B >= 1 && B <= 65535, "%s: B %d not in 1..65535", fn, B);
    GGA_REQUIRE(prm->n_groups >= 1 && prm->n_groups <= GGA_ANCHOR_MAX_GROUPS, "%s: n_groups %d not in 1..%d", fn, prm->n_groups,
                GGA_ANCHOR_MAX_GROUPS);
    GGA_REQUIRE(prm->n_rot >= 1 && prm->n_rot <= 1024, "%s: n_rot %d not in 1..1024", fn, prm->n_rot);
    GGA_REQUIRE(prm->num_classes >= 1 && prm->num_classes <= 1024, "%s: num_classes %d not in 1..1024", fn, prm->num_classes);
    GGA_REQUIRE(A >= 1 && (int64_t)A * B < (1ll << 31) / 8, "%s: A %d (B %d): A * B must be in 1..2^28", fn, A, B);
    GGA_REQUIRE(A % (prm->n_groups * prm->n_rot) == 0, "%s: A %d is not a multiple of n_groups * n_rot = %d", fn, A,
                prm->n_groups * prm->n_rot);
    GGA_REQUIRE(N >= 0, "%s: N %d < 0", fn, N);
    GGA_REQUIRE(frame_offsets_host, "%s: null frame_offsets_host", fn);
    GGA_REQUIRE(frame_offsets_host[0] >= 0, "%s: frame_offsets[0] = %d < 0", fn, frame_offsets_host[0]);
    for (int f = 0; f < B; ++f)
        GGA_REQUIRE(frame_offsets_host[f + 1] >= frame_offsets_host[f], "%s: frame_offsets not monotone at frame %d (%d after %d)",
                    fn, f, frame_offsets_host[f + 1], frame_offsets_host[f]);
    GGA_REQUIRE(frame_offsets_host[B] <= N, "%s: frame_offsets end at %d, past the %d boxes", fn, frame_offsets_host[B], N);
    GGA_REQUIRE(anchors && frame_offsets && out_labels && label_weights && bbox_targets && pos_flag && dir_targets &&
                    dir_weights && pos_count && workspace,
                "%s: null pointer argument", fn);
    GGA_REQUIRE(N == 0 || (boxes && labels), "%s: null boxes / labels with N %d", fn, N);
    GGA_REQUIRE(workspace_bytes >= gga_anchor_targets_workspace_bytes(N, prm->n_groups), "%s: workspace of %zu bytes, %zu needed", fn,
                workspace_bytes, gga_anchor_targets_workspace_bytes(N, prm->n_groups));
    uint32_t* gt_max = (uint32_t*)workspace;
    GGA_CHECK_HIP(hipMemsetAsync(pos_count, 0, (size_t)B * sizeof(int32_t), stream), "anchor pos_count memset");
    if (frame_offsets_host[B] > frame_offsets_host[0]) {
        GGA_CHECK_HIP(hipMemsetAsync(gt_max, 0, (size_t)N * prm->n_groups * sizeof(uint32_t), stream), "anchor gt_max memset");
        const int per_group = A / prm->n_groups;
        hipLaunchKernelGGL(anchor_gt_max_kernel, dim3((per_group + AH_THREADS - 1) / AH_THREADS, prm->n_groups, B),
                           dim3(AH_THREADS), 0, stream, anchors, A, *prm, boxes, labels, N, frame_offsets, gt_max);
        GGA_CHECK_LAUNCH("anchor_gt_max_kernel");
    }
    hipLaunchKernelGGL(anchor_assign_kernel, dim3((A + AH_THREADS - 1) / AH_THREADS, B), dim3(AH_THREADS), 0, stream, anchors, A,
                       *prm, boxes, labels, N, frame_offsets, gt_max, out_labels, label_weights, bbox_targets, pos_flag, dir_targets,
                       dir_weights, pos_count);
    GGA_CHECK_LAUNCH("anchor_assign_kernel");
    return GGA_OK;
}

// ----------------------------------------------------------------------------- losses
// The anchor `i` = pixel * n_anchors + a of frame b reads channel a * C + c of cls_score, a * 7 + k of bbox_pred and a * 2 + d
// of dir_cls_pred at element b * stride[0] + channel * stride[1] + pixel * stride[2]: the reference's
// permute(0, 2, 3, 1).reshape(-1, C) without a copy, for NCHW and channels-last memory alike.
__device__ __forceinline__ int64_t ah_at(const int64_t* s, int b, int channel, int pixel) {
    return (int64_t)b * s[0] + (int64_t)channel * s[1] + (int64_t)pixel * s[2];
}

// p = sigmoid(x), q = 1 - p, log p and log q, each without cancellation
__device__ __forceinline__ void ah_log_sigmoid(float x, float& log_p, float& log_q, float& p, float& q) {
    const float e = log1pf(expf(-fabsf(x)));
    log_p = -(fmaxf(-x, 0.0f) + e);
    log_q = -(fmaxf(x, 0.0f) + e);
    p = 1.0f / (1.0f + expf(-x));
    q = 1.0f / (1.0f + expf(x));
}

// pred - target of code entry k; with diff_rad_by_sin entry 6 is sin p cos t - cos p sin t (add_sin_difference,
// anchor3d_head.py:280-302), formed in f64: the two products nearly cancel where the yaw is right, and only positives come here
__device__ __forceinline__ float ah_reg_diff(const gga_anchor_loss_params& P, int k, float p, float t) {
    if (k == 6 && P.diff_rad_by_sin) return (float)(sin((double)p) * cos((double)t) - cos((double)p) * sin((double)t));
    return p - t;
}

// partial sums [block][3] (f64) of the focal, smooth-L1 and direction terms; a thread walks its anchors in ascending order, the
// wave and then the four waves are added in a fixed order
__global__ __launch_bounds__(AH_THREADS) void anchor_loss_partial_kernel(
    gga_anchor_loss_params P, const float* __restrict__ cls, const float* __restrict__ reg, const float* __restrict__ dir,
    const int64_t* __restrict__ labels, const float* __restrict__ label_weights, const uint8_t* __restrict__ pos_flag,
    const float* __restrict__ bbox_targets, const int64_t* __restrict__ dir_targets, const float* __restrict__ dir_weights,
    double* __restrict__ partials) {
    const int A = P.HW * P.n_anchors, C = P.num_classes;
    const int64_t total = (int64_t)P.B * A;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t idx = (int64_t)blockIdx.x * AH_THREADS + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * AH_THREADS) {
        const int b = (int)(idx / A), i = (int)(idx - (int64_t)b * A);
        const int pixel = i / P.n_anchors, a = i - pixel * P.n_anchors;
        const float lw = label_weights[idx];
        if (lw != 0.0f) {
            const int64_t label = labels[idx];
            float s = 0.0f;
            for (int c = 0; c < C; ++c) {
                const float x = cls[ah_at(P.cls_stride, b, a * C + c, pixel)];
                float log_p, log_q, p, q;
                ah_log_sigmoid(x, log_p, log_q, p, q);
                s += label == c ? -P.alpha * powf(q, P.gamma) * log_p : -(1.0f - P.alpha) * powf(p, P.gamma) * log_q;
            }
            acc[0] += (double)(s * lw);
        }
        if (!pos_flag[idx]) continue;
        float s = 0.0f;
        for (int k = 0; k < 7; ++k) {
            const float d = fabsf(ah_reg_diff(P, k, reg[ah_at(P.reg_stride, b, a * 7 + k, pixel)], bbox_targets[idx * 7 + k]));
            s += P.code_weight[k] * (d < P.beta ? 0.5f * d * d / P.beta : d - 0.5f * P.beta);
        }
        acc[1] += (double)s;
        if (dir) {
            const float d0 = dir[ah_at(P.dir_stride, b, a * 2, pixel)], d1 = dir[ah_at(P.dir_stride, b, a * 2 + 1, pixel)];
            const float mx = fmaxf(d0, d1);
            const float lse = mx + logf(expf(d0 - mx) + expf(d1 - mx));
            acc[2] += (double)((lse - (dir_targets[idx] ? d1 : d0)) * dir_weights[idx]);
        }
    }
    __shared__ double s_acc[3][AH_THREADS / 64];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double w = wave_sum(acc[k]);
        if ((threadIdx.x & 63) == 0) s_acc[k][threadIdx.x >> 6] = w;
    }
    __syncthreads();
    if (threadIdx.x < 3)
        partials[(int64_t)blockIdx.x * 3 + threadIdx.x] =
            (s_acc[threadIdx.x][0] + s_acc[threadIdx.x][1]) + (s_acc[threadIdx.x][2] + s_acc[threadIdx.x][3]);
}

// out[k] = loss_weight[k] * sum_k / (avg_factor + eps_f32), out[3] = avg_factor = sum_b max(pos_count[b], 1)
__global__ __launch_bounds__(AH_THREADS) void anchor_loss_final_kernel(gga_anchor_loss_params P, const double* __restrict__ partials,
                                                                      int n_blocks, const int32_t* __restrict__ pos_count,
                                                                      float* __restrict__ out) {
    double acc[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < n_blocks; i += AH_THREADS)
        for (int k = 0; k < 3; ++k) acc[k] += partials[(int64_t)i * 3 + k];
    int cnt = 0;
    for (int b = threadIdx.x; b < P.B; b += AH_THREADS) cnt += max(pos_count[b], 1);
    __shared__ double s_acc[3][AH_THREADS / 64];
    __shared__ int s_cnt[AH_THREADS / 64];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double w = wave_sum(acc[k]);
        if ((threadIdx.x & 63) == 0) s_acc[k][threadIdx.x >> 6] = w;
    }
    cnt = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int avg = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        const double den = (double)avg + (double)FLT_EPSILON;
        for (int k = 0; k < 3; ++k)
            out[k] = P.loss_weight[k] * (float)(((s_acc[k][0] + s_acc[k][1]) + (s_acc[k][2] + s_acc[k][3])) / den);
        out[3] = (float)avg;
    }
}

// one thread per anchor: every channel of the anchor in the three gradient tensors is written
__global__ __launch_bounds__(AH_THREADS) void anchor_loss_bwd_kernel(
    gga_anchor_loss_params P, const float* __restrict__ cls, const float* __restrict__ reg, const float* __restrict__ dir,
    const int64_t* __restrict__ labels, const float* __restrict__ label_weights, const uint8_t* __restrict__ pos_flag,
    const float* __restrict__ bbox_targets, const int64_t* __restrict__ dir_targets, const float* __restrict__ dir_weights,
    const float* __restrict__ fwd_out, const float* __restrict__ grad_out, float* __restrict__ g_cls, float* __restrict__ g_reg,
    float* __restrict__ g_dir) {
    const int A = P.HW * P.n_anchors, C = P.num_classes;
    const int64_t idx = (int64_t)blockIdx.x * AH_THREADS + threadIdx.x;
    if (idx >= (int64_t)P.B * A) return;
    const int b = (int)(idx / A), i = (int)(idx - (int64_t)b * A);
    const int pixel = i / P.n_anchors, a = i - pixel * P.n_anchors;
    const double den = (double)fwd_out[3] + (double)FLT_EPSILON;
    const float lw = label_weights[idx];
    const bool pos = pos_flag[idx] != 0;
    {
        const float scale = (float)((double)(grad_out[0] * P.loss_weight[0]) / den) * lw;
        const int64_t label = labels[idx];
        for (int c = 0; c < C; ++c) {
            const int64_t at = ah_at(P.cls_stride, b, a * C + c, pixel);
            float g = 0.0f;
            if (lw != 0.0f) {
                float log_p, log_q, p, q;
                ah_log_sigmoid(cls[at], log_p, log_q, p, q);
                // d/dx of -alpha q^gamma log p   and of   -(1-alpha) p^gamma log q,   q = 1 - p, dp/dx = p q
                g = label == c ? P.alpha * powf(q, P.gamma) * (P.gamma * p * log_p - q)
                               : (1.0f - P.alpha) * powf(p, P.gamma) * (p - P.gamma * q * log_q);
                g *= scale;
            }
            g_cls[at] = g;
        }
    }
    {
        const float scale = (float)((double)(grad_out[1] * P.loss_weight[1]) / den);
        for (int k = 0; k < 7; ++k) {
            const int64_t at = ah_at(P.reg_stride, b, a * 7 + k, pixel);
            float g = 0.0f;
            if (pos) {
                const float p = reg[at], t = bbox_targets[idx * 7 + k];
                const float d = ah_reg_diff(P, k, p, t);
                g = fabsf(d) < P.beta ? d / P.beta : (d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f));
                if (k == 6 && P.diff_rad_by_sin) g *= (float)cos((double)p - (double)t);      // d (sin p cos t - cos p sin t) / dp
                g *= P.code_weight[k] * scale;
            }
            g_reg[at] = g;
        }
    }
    if (dir) {
        const int64_t at0 = ah_at(P.dir_stride, b, a * 2, pixel), at1 = ah_at(P.dir_stride, b, a * 2 + 1, pixel);
        float g0 = 0.0f, g1 = 0.0f;
        if (pos) {
            const float scale = (float)((double)(grad_out[2] * P.loss_weight[2]) / den) * dir_weights[idx];
            const float d0 = dir[at0], d1 = dir[at1];
            const float mx = fmaxf(d0, d1);
            const float e0 = expf(d0 - mx), e1 = expf(d1 - mx);
            const float p1 = e1 / (e0 + e1), p0 = e0 / (e0 + e1);
            const bool one = dir_targets[idx] != 0;
            g0 = (one ? p0 : -p1) * scale;                                   // softmax - one-hot, p0 - 1 = -p1
            g1 = (one ? -p0 : p1) * scale;
        }
        g_dir[at0] = g0;
        g_dir[at1] = g1;
    }
}

static int anchor_loss_check(const char* fn, const gga_anchor_loss_params* P, const void* cls, const void* reg, const void* dir,
                             const void* labels, const void* label_weights, const void* pos_flag, const void* bbox_targets,
                             const void* dir_targets, const void* dir_weights) {
    GGA_REQUIRE(P, "%s: null params", fn);
    GGA_REQUIRE(P->B >= 1 && P->B <= 65535, "%s: B %d not in 1..65535", fn, P->B);
    GGA_REQUIRE(P->HW >= 1 && P->n_anchors >= 1 && P->n_anchors <= 4096, "%s: HW %d, n_anchors %d", fn, P->HW, P->n_anchors);
    GGA_REQUIRE((int64_t)P->HW * P->n_anchors * P->B < (1ll << 31) / 8, "%s: B * HW * n_anchors must be < 2^28", fn);
    GGA_REQUIRE(P->num_classes >= 1 && P->num_classes <= 1024, "%s: num_classes %d not in 1..1024", fn, P->num_classes);
    GGA_REQUIRE(P->beta > 0.0f, "%s: beta %g must be > 0", fn, (double)P->beta);
    for (int k = 0; k < 3; ++k) {
        GGA_REQUIRE(P->cls_stride[k] > 0 && P->reg_stride[k] > 0, "%s: stride %d of cls_score / bbox_pred is %lld / %lld, must be > 0",
                    fn, k, (long long)P->cls_stride[k], (long long)P->reg_stride[k]);
        GGA_REQUIRE(!dir || P->dir_stride[k] > 0, "%s: stride %d of dir_cls_pred is %lld, must be > 0", fn, k,
                    (long long)P->dir_stride[k]);
    }
    GGA_REQUIRE(cls && reg && labels && label_weights && pos_flag && bbox_targets, "%s: null pointer argument", fn);
    GGA_REQUIRE(!dir || (dir_targets && dir_weights), "%s: dir_cls_pred without dir_targets / dir_weights", fn);
    return GGA_OK;
}

extern "C" int gga_anchor_loss_fwd(const gga_anchor_loss_params* prm, const float* cls_score, const float* bbox_pred,
                                   const float* dir_cls_pred, const int64_t* labels, const float* label_weights,
                                   const uint8_t* pos_flag, const float* bbox_targets, const int64_t* dir_targets,
                                   const float* dir_weights, const int32_t* pos_count, float* out, void* workspace,
                                   size_t workspace_bytes, void* stream_) {
    const char* fn = "gga_anchor_loss_fwd";
    if (int rc = anchor_loss_check(fn, prm, cls_score, bbox_pred, dir_cls_pred, labels, label_weights, pos_flag, bbox_targets,
                                   dir_targets, dir_weights))
        return rc;
    GGA_REQUIRE(pos_count && out && workspace, "%s: null pointer argument", fn);
    GGA_REQUIRE(workspace_bytes >= GGA_ANCHOR_LOSS_WORKSPACE_BYTES, "%s: workspace of %zu bytes, %d needed", fn, workspace_bytes,
                GGA_ANCHOR_LOSS_WORKSPACE_BYTES);
    const int64_t total = (int64_t)prm->B * prm->HW * prm->n_anchors;
    const int max_blocks = GGA_ANCHOR_LOSS_WORKSPACE_BYTES / (3 * (int)sizeof(double));
    const int n_blocks = (int)((total + AH_THREADS - 1) / AH_THREADS < max_blocks ? (total + AH_THREADS - 1) / AH_THREADS : max_blocks);
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(anchor_loss_partial_kernel, dim3(n_blocks), dim3(AH_THREADS), 0, stream, *prm, cls_score, bbox_pred,
                       dir_cls_pred, labels, label_weights, pos_flag, bbox_targets, dir_targets, dir_weights, (double*)workspace);
    GGA_CHECK_LAUNCH("anchor_loss_partial_kernel");
    hipLaunchKernelGGL(anchor_loss_final_kernel, dim3(1), dim3(AH_THREADS), 0, stream, *prm, (const double*)workspace, n_blocks,
                       pos_count, out);
    GGA_CHECK_LAUNCH("anchor_loss_final_kernel");
    return GGA_OK;
}

extern "C" int gga_anchor_loss_bwd(const gga_anchor_loss_params* prm, const float* cls_score, const float* bbox_pred,
                                   const float* dir_cls_pred, const int64_t* labels, const float* label_weights,
                                   const uint8_t* pos_flag, const float* bbox_targets, const int64_t* dir_targets,
                                   const float* dir_weights, const float* fwd_out, const float* grad_out, float* grad_cls,
                                   float* grad_bbox, float* grad_dir, void* stream_) {
    const char* fn = "gga_anchor_loss_bwd";
    if (int rc = anchor_loss_check(fn, prm, cls_score, bbox_pred, dir_cls_pred, labels, label_weights, pos_flag, bbox_targets,
                                   dir_targets, dir_weights))
        return rc;
    GGA_REQUIRE(fwd_out && grad_out && grad_cls && grad_bbox && (!dir_cls_pred || grad_dir), "%s: null pointer argument", fn);
    const int64_t total = (int64_t)prm->B * prm->HW * prm->n_anchors;
    hipLaunchKernelGGL(anchor_loss_bwd_kernel, dim3((unsigned)((total + AH_THREADS - 1) / AH_THREADS)), dim3(AH_THREADS), 0,
                       (hipStream_t)stream_, *prm, cls_score, bbox_pred, dir_cls_pred, labels, label_weights, pos_flag, bbox_targets,
                       dir_targets, dir_weights, fwd_out, grad_out, grad_cls, grad_bbox, grad_dir);
    GGA_CHECK_LAUNCH("anchor_loss_bwd_kernel");
    return GGA_OK;
}

// ----------------------------------------------------------------------------- gather + decode of the kept anchors
struct ah_strides {
    int64_t reg[3], dir[3];
};

// one thread per kept anchor (frame b, slot s): the anchor inds[b, s] of the frame. DeltaXYZWLHRBBoxCoder.decode in the coder's
// order of operations; scores are gathered from the sigmoid scores the top-k was taken on (the same bits); direction bit =
// argmax of the two direction logits (the first on a tie).
__global__ __launch_bounds__(AH_THREADS) void anchor_decode_kernel(
    const int64_t* __restrict__ inds, int B, int K, const float* __restrict__ anchors, int A, int n_anchors, int C,
    const float* __restrict__ scores, const float* __restrict__ reg, const float* __restrict__ dir, ah_strides S,
    float* __restrict__ out_boxes, float* __restrict__ out_scores, int64_t* __restrict__ out_dir) {
    const int row = blockIdx.x * AH_THREADS + threadIdx.x;
    if (row >= B * K) return;
    const int b = row / K;
    const int64_t i = inds[row];
    float box[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    int64_t bit = 0;
    const bool ok = i >= 0 && i < A;                                     // an index off the map: a row of zeros
    if (ok) {
        const int pixel = (int)(i / n_anchors), a = (int)(i - (int64_t)pixel * n_anchors);
        float an[7], t[7];
        for (int k = 0; k < 7; ++k) {
            an[k] = anchors[i * 7 + k];
            t[k] = reg[ah_at(S.reg, b, a * 7 + k, pixel)];
        }
        const float za = __fadd_rn(an[2], __fmul_rn(an[5], 0.5f));
        const float diagonal = __fsqrt_rn(__fadd_rn(__fmul_rn(an[4], an[4]), __fmul_rn(an[3], an[3])));
        box[0] = __fadd_rn(__fmul_rn(t[0], diagonal), an[0]);
        box[1] = __fadd_rn(__fmul_rn(t[1], diagonal), an[1]);
        const float zg = __fadd_rn(__fmul_rn(t[2], an[5]), za);
        box[3] = __fmul_rn(expf(t[3]), an[3]);
        box[4] = __fmul_rn(expf(t[4]), an[4]);
        box[5] = __fmul_rn(expf(t[5]), an[5]);
        box[6] = __fadd_rn(t[6], an[6]);
        box[2] = __fsub_rn(zg, __fmul_rn(box[5], 0.5f));
        if (dir) bit = dir[ah_at(S.dir, b, a * 2 + 1, pixel)] > dir[ah_at(S.dir, b, a * 2, pixel)] ? 1 : 0;
    }
    for (int k = 0; k < 7; ++k) out_boxes[(int64_t)row * 7 + k] = box[k];
    for (int c = 0; c < C; ++c) out_scores[(int64_t)row * C + c] = ok ? scores[((int64_t)b * A + i) * C + c] : 0.0f;
    out_dir[row] = bit;
}

extern "C" int gga_anchor_decode(const int64_t* inds, int B, int K, const float* anchors, int A, int n_anchors, int num_classes,
                                 const float* scores, const float* bbox_pred, const int64_t* bbox_stride,
                                 const float* dir_cls_pred, const int64_t* dir_stride, float* out_boxes, float* out_scores,
                                 int64_t* out_dir, void* stream_) {
    const char* fn = "gga_anchor_decode";
    GGA_REQUIRE(B >= 1 && B <= 65535, "%s: B %d not in 1..65535", fn, B);
    GGA_REQUIRE(K >= 1 && (int64_t)B * K < (1 << 24), "%s: K %d (B %d): B * K must be in 1..2^24", fn, K, B);
    GGA_REQUIRE(n_anchors >= 1 && A >= 1 && A % n_anchors == 0 && (int64_t)A * B < (1ll << 31) / 8,
                "%s: A %d, n_anchors %d (B %d): A a multiple of n_anchors, A * B < 2^28", fn, A, n_anchors, B);
    GGA_REQUIRE(num_classes >= 1 && num_classes <= 1024, "%s: num_classes %d not in 1..1024", fn, num_classes);
    GGA_REQUIRE(inds && anchors && scores && bbox_pred && bbox_stride && out_boxes && out_scores && out_dir,
                "%s: null pointer argument", fn);
    GGA_REQUIRE(!dir_cls_pred || dir_stride, "%s: dir_cls_pred without its strides", fn);
    ah_strides S;
    for (int k = 0; k < 3; ++k) {
        GGA_REQUIRE(bbox_stride[k] > 0 && (!dir_cls_pred || dir_stride[k] > 0), "%s: stride %d must be > 0", fn, k);
        S.reg[k] = bbox_stride[k];
        S.dir[k] = dir_cls_pred ? dir_stride[k] : 0;
    }
    hipLaunchKernelGGL(anchor_decode_kernel, dim3((B * K + AH_THREADS - 1) / AH_THREADS), dim3(AH_THREADS), 0, (hipStream_t)stream_,
                       inds, B, K, anchors, A, n_anchors, num_classes, scores, bbox_pred, dir_cls_pred, S, out_boxes, out_scores,
                       out_dir);
    GGA_CHECK_LAUNCH("anchor_decode_kernel");
    return GGA_OK;
}
