// Supervised CenterPoint targets and regression loss (gfx950).
//
// Reference: mmdet3d/models/dense_heads/centerpoint_head.py:435-583 (get_targets_single: a Python loop per object with several
// tiny host-to-device copies each) and :623-638 (the masked, code-weighted L1 over the gathered predictions). Here the targets
// of a whole batch are ONE launch: a workgroup per (frame, task) ranks the frame's objects of its task (class-major, then
// object index), fills the K slots, and max-splats the gaussian patches into its own heat maps. The loss is one launch each
// way for all tasks, reduced in a fixed order.
//
// The file is compiled with -ffp-contract=off (Makefile): where the reference does separate f32 operations, so does this.
#include <float.h>

#include "gga_common.h"

#define CT_THREADS 256

// mmdet3d/core/utils/gaussian.py:57-86 in f64, operation by operation.
__device__ static double center_gaussian_radius(double height, double width, double min_overlap) {
    const double b1 = height + width;
    const double c1 = width * height * (1 - min_overlap) / (1 + min_overlap);
    const double r1 = (b1 + sqrt(b1 * b1 - 4 * c1)) / 2;
    const double b2 = 2 * (height + width);
    const double c2 = (1 - min_overlap) * width * height;
    const double r2 = (b2 + sqrt(b2 * b2 - 16 * c2)) / 2;
    const double a3 = 4 * min_overlap;
    const double b3 = -2 * min_overlap * (height + width);
    const double c3 = (min_overlap - 1) * width * height;
    const double r3 = (b3 + sqrt(b3 * b3 - 4 * a3 * c3)) / 2;
    return fmin(fmin(r1, r2), r3);
}

// The rank key of object i of the frame for task `task`: its class index inside the task, or -1 when the object belongs to
// another task, carries label -1 or a label outside the table.
__device__ __forceinline__ int center_key(const int64_t* __restrict__ labels, int i, const gga_center_params& P, int task) {
    const int64_t l = labels[i];
    if (l < 0 || l >= P.n_classes) return -1;
    return P.class_task[l] == task ? P.class_index[l] : -1;
}

__global__ __launch_bounds__(CT_THREADS) void center_targets_kernel(
    const float* __restrict__ boxes, const int64_t* __restrict__ labels, const int32_t* __restrict__ frame_offsets, int B,
    gga_center_params P, int64_t* __restrict__ ind, uint8_t* __restrict__ mask, float* __restrict__ anno_box,
    float* __restrict__ heatmaps, const float* __restrict__ patch_table, const int32_t* __restrict__ patch_offsets,
    int max_radius) {
    const int b = blockIdx.x, task = blockIdx.y, tid = threadIdx.x;
    const int K = P.K, H = P.H, W = P.W;
    __shared__ int s_key[CT_THREADS];
    __shared__ int4 s_obj[GGA_CENTER_MAX_K];           // (class in task, cx, cy, radius); radius < 0: the slot is empty
    __shared__ float s_anno[GGA_CENTER_MAX_K * 8];
    for (int s = tid; s < K; s += CT_THREADS) s_obj[s] = make_int4(0, 0, 0, -1);
    for (int s = tid; s < K * 8; s += CT_THREADS) s_anno[s] = 0.0f;

    const int o0 = frame_offsets[b];
    const int n = frame_offsets[b + 1] - o0;
    const int64_t* __restrict__ lab = labels + o0;
    for (int i0 = 0; i0 < n; i0 += CT_THREADS) {
        const int i = i0 + tid;
        const int key = i < n ? center_key(lab, i, P, task) : -1;
        int rank = 0;
        for (int j0 = 0; j0 < n; j0 += CT_THREADS) {
            __syncthreads();                            // (also orders the clearing of the slots before the first write)
            s_key[tid] = j0 + tid < n ? center_key(lab, j0 + tid, P, task) : -1;
            __syncthreads();
            const int m = min(CT_THREADS, n - j0);
            if (key >= 0)
                for (int jj = 0; jj < m; ++jj) {
                    const int kj = s_key[jj];
                    rank += (kj >= 0 && (kj < key || (kj == key && j0 + jj < i))) ? 1 : 0;
                }
        }
        if (key < 0 || rank >= K) continue;             // another task's object, or past the last slot: dropped, not splatted
        const float* __restrict__ bx = boxes + (int64_t)(o0 + i) * 7;
        const float x = bx[0], y = bx[1], z = bx[2], dx = bx[3], dy = bx[4], dz = bx[5], yaw = bx[6];
        const float width = __fdiv_rn(__fdiv_rn(dx, P.voxel_size[0]), P.out_size_factor);
        const float length = __fdiv_rn(__fdiv_rn(dy, P.voxel_size[1]), P.out_size_factor);
        if (!(width > 0.0f && length > 0.0f)) continue;                 // the slot is used up and stays empty
        const double rd = center_gaussian_radius((double)length, (double)width, (double)P.gaussian_overlap);
        // int(radius): truncation; a radius beyond any table (a box of kilometres) is clamped so that the cast is defined
        const int radius = max(P.min_radius, (int)fmin(rd, 1.0e9));
        const float cxf = __fdiv_rn(__fdiv_rn(__fsub_rn(x, P.pc_range[0]), P.voxel_size[0]), P.out_size_factor);
        const float cyf = __fdiv_rn(__fdiv_rn(__fsub_rn(y, P.pc_range[1]), P.voxel_size[1]), P.out_size_factor);
        // trunc(c) in [0, size)  <=>  -1 < c < size; NaN and +-inf fail the test
        if (!(cxf > -1.0f && cxf < (float)W && cyf > -1.0f && cyf < (float)H)) continue;
        const int cx = (int)cxf, cy = (int)cyf;
        s_obj[rank] = make_int4(key, cx, cy, radius);
        float* a = s_anno + rank * 8;
        a[0] = __fsub_rn(cxf, (float)cx);
        a[1] = __fsub_rn(cyf, (float)cy);
        a[2] = __fadd_rn(z, __fmul_rn(dz, 0.5f));                        // gravity centre
        a[3] = logf(dx);
        a[4] = logf(dy);
        a[5] = logf(dz);                                                 // NaN for dz < 0: the loss masks it
        a[6] = sinf(yaw);
        a[7] = cosf(yaw);
    }
    __syncthreads();

    const int64_t slot0 = ((int64_t)task * B + b) * K;
    for (int s = tid; s < K; s += CT_THREADS) {
        const int4 o = s_obj[s];
        ind[slot0 + s] = o.w >= 0 ? (int64_t)o.z * W + o.y : 0;
        mask[slot0 + s] = o.w >= 0 ? 1 : 0;
    }
    for (int s = tid; s < K * 8; s += CT_THREADS) anno_box[slot0 * 8 + s] = s_anno[s];

    // the splat of the slots' patches into this (frame, task)'s maps: values are >= 0, so float order == int order, and the
    // maximum does not depend on the order (two threads may hold overlapping patches of two objects: hence the atomic)
    const int n_cls = P.task_classes[task];
    float* __restrict__ maps = heatmaps + ((int64_t)B * P.task_class_base[task] + (int64_t)b * n_cls) * H * W;
    for (int s = 0; s < K; ++s) {
        const int4 o = s_obj[s];
        const int r = o.w;
        if (r < 0 || r > max_radius) continue;
        const int d = 2 * r + 1;
        const int left = min(o.y, r), right = min(W - o.y, r + 1);       // clipped to the map like gaussian.py:42-50
        const int top = min(o.z, r), bottom = min(H - o.z, r + 1);
        const int pw = left + right, ph = top + bottom;
        const float* __restrict__ patch = patch_table + patch_offsets[r];
        int* hm = reinterpret_cast<int*>(maps + (int64_t)o.x * H * W);
        for (int t = tid; t < pw * ph; t += CT_THREADS) {
            const int yy = t / pw - top, xx = t - (t / pw) * pw - left;
            atomicMax(&hm[(int64_t)(o.z + yy) * W + (o.y + xx)], __float_as_int(patch[(r + yy) * d + (r + xx)]));
        }
    }
}

extern "C" int gga_center_targets(const float* boxes, const int64_t* labels, const int32_t* frame_offsets, int B,
                                  const gga_center_params* prm, int64_t* ind, uint8_t* mask, float* anno_box, float* heatmaps,
                                  const float* patch_table, const int32_t* patch_offsets, int max_radius, void* stream_) {
    const char* fn = "gga_center_targets";
    hipStream_t stream = (hipStream_t)stream_;
    GGA_REQUIRE(prm, "%s: null params", fn);
    GGA_REQUIRE(B >= 1 && B <= 65535, "%s: B %d not in 1..65535", fn, B);
    GGA_REQUIRE(prm->n_tasks >= 1 && prm->n_tasks <= GGA_MAX_TASKS, "%s: n_tasks %d not in 1..%d", fn, prm->n_tasks, GGA_MAX_TASKS);
    GGA_REQUIRE(prm->n_classes >= 1 && prm->n_classes <= GGA_CENTER_MAX_CLASSES, "%s: n_classes %d not in 1..%d", fn,
                prm->n_classes, GGA_CENTER_MAX_CLASSES);
    GGA_REQUIRE(prm->K >= 1 && prm->K <= GGA_CENTER_MAX_K, "%s: K %d not in 1..%d", fn, prm->K, GGA_CENTER_MAX_K);
    GGA_REQUIRE(prm->H >= 1 && prm->W >= 1 && (int64_t)prm->H * prm->W < (1 << 30), "%s: bad map size %d x %d", fn, prm->H, prm->W);
    GGA_REQUIRE(prm->voxel_size[0] > 0 && prm->voxel_size[1] > 0 && prm->out_size_factor > 0, "%s: voxel_size and out_size_factor must be > 0", fn);
    GGA_REQUIRE(prm->min_radius >= 0 && max_radius >= prm->min_radius, "%s: min_radius %d, max_radius %d", fn, prm->min_radius, max_radius);
    int base = 0;
    for (int t = 0; t < prm->n_tasks; ++t) {
        GGA_REQUIRE(prm->task_classes[t] >= 1 && prm->task_class_base[t] == base, "%s: task %d: classes %d at base %d (expected %d)",
                    fn, t, prm->task_classes[t], prm->task_class_base[t], base);
        base += prm->task_classes[t];
    }
    GGA_REQUIRE(base == prm->n_classes, "%s: the tasks hold %d classes, n_classes is %d", fn, base, prm->n_classes);
    for (int c = 0; c < prm->n_classes; ++c) {
        const int t = prm->class_task[c];
        GGA_REQUIRE(t >= 0 && t < prm->n_tasks && prm->class_index[c] >= 0 && prm->class_index[c] < prm->task_classes[t],
                    "%s: class %d -> task %d, index %d: outside the table", fn, c, t, prm->class_index[c]);
    }
    GGA_REQUIRE(boxes && labels && frame_offsets && ind && mask && anno_box && heatmaps && patch_table && patch_offsets,
                "%s: null pointer argument", fn);
    GGA_CHECK_HIP(hipMemsetAsync(heatmaps, 0, (size_t)B * prm->n_classes * prm->H * prm->W * sizeof(float), stream), "center heatmap memset");
    hipLaunchKernelGGL(center_targets_kernel, dim3(B, prm->n_tasks), dim3(CT_THREADS), 0, stream, boxes, labels, frame_offsets, B,
                       *prm, ind, mask, anno_box, heatmaps, patch_table, patch_offsets, max_radius);
    GGA_CHECK_LAUNCH("center_targets_kernel");
    return GGA_OK;
}

// ----------------------------------------------------------------------------- regression loss
// loss[t] = loss_weight * sum_{slot, c} mask * [anno not NaN] * code_weights[c] * |pred - anno| / ((sum mask + 1e-4) + eps_f32)
// One workgroup per task: a thread walks its slots in ascending order (f64 running sum), the wave and then the four waves are
// added in a fixed order. No atomics: the same inputs give the same bits, whichever tasks share the launch.
__global__ __launch_bounds__(CT_THREADS) void center_reg_loss_fwd_kernel(gga_center_loss_table tb, int n_slots,
                                                                        gga_center_loss_weights w) {
    const gga_center_loss_task& T = tb.task[blockIdx.x];
    const float* __restrict__ pred = T.pred;
    const float* __restrict__ anno = T.anno_box;
    const uint8_t* __restrict__ mask = T.mask;
    double acc = 0.0;
    int cnt = 0;
    for (int s = threadIdx.x; s < n_slots; s += CT_THREADS) {
        if (!mask[s]) continue;
        ++cnt;
        const float4 p0 = reinterpret_cast<const float4*>(pred)[2 * s], p1 = reinterpret_cast<const float4*>(pred)[2 * s + 1];
        const float4 a0 = reinterpret_cast<const float4*>(anno)[2 * s], a1 = reinterpret_cast<const float4*>(anno)[2 * s + 1];
        const float p[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
        const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
        for (int c = 0; c < 8; ++c)
            if (a[c] == a[c]) acc += (double)(w.code_weights[c] * fabsf(p[c] - a[c]));
    }
    acc = wave_sum(acc);
    cnt = wave_sum(cnt);
    __shared__ double s_acc[CT_THREADS / 64];
    __shared__ int s_cnt[CT_THREADS / 64];
    if ((threadIdx.x & 63) == 0) { s_acc[threadIdx.x >> 6] = acc; s_cnt[threadIdx.x >> 6] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double tot = (s_acc[0] + s_acc[1]) + (s_acc[2] + s_acc[3]);
        const float num = (float)(s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3]);
        const float avg = (num + 1e-4f) + FLT_EPSILON;
        T.loss[0] = w.loss_weight * ((float)tot / avg);
        T.loss[1] = num;
    }
}

// grad_pred[s, c] = (*grad_loss) * loss_weight * mask * [anno not NaN] * code_weights[c] * sign(pred - anno) / avg
__global__ __launch_bounds__(CT_THREADS) void center_reg_loss_bwd_kernel(gga_center_loss_table tb, int n_slots,
                                                                        gga_center_loss_weights w) {
    const gga_center_loss_task& T = tb.task[blockIdx.y];
    const int e = blockIdx.x * CT_THREADS + threadIdx.x;
    if (e >= n_slots * 8) return;
    const int s = e >> 3, c = e & 7;
    float g = 0.0f;
    if (T.mask[s]) {
        const float a = T.anno_box[e], d = T.pred[e] - a;
        if (a == a) {
            const float avg = (T.loss[1] + 1e-4f) + FLT_EPSILON;
            const float sgn = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
            g = (*T.grad_loss) * w.loss_weight * w.code_weights[c] * sgn / avg;
        }
    }
    T.grad_pred[e] = g;
}

static int center_loss_check(const char* fn, const gga_center_loss_table* tb, int B, int K, const gga_center_loss_weights* w, bool bwd) {
    GGA_REQUIRE(tb, "%s: null task table", fn);
    GGA_REQUIRE(tb->n_tasks >= 1 && tb->n_tasks <= GGA_MAX_TASKS, "%s: n_tasks %d not in 1..%d", fn, tb->n_tasks, GGA_MAX_TASKS);
    GGA_REQUIRE(w, "%s: null weights", fn);
    GGA_REQUIRE(B >= 1 && K >= 1 && (int64_t)B * K * 8 < (1ll << 31), "%s: bad B %d, K %d", fn, B, K);
    for (int t = 0; t < tb->n_tasks; ++t) {
        const gga_center_loss_task& T = tb->task[t];
        GGA_REQUIRE(T.pred && T.anno_box && T.mask && T.loss && (!bwd || (T.grad_loss && T.grad_pred)), "%s: null pointer (task %d)", fn, t);
        GGA_REQUIRE(((uintptr_t)T.pred & 15) == 0 && ((uintptr_t)T.anno_box & 15) == 0, "%s: pred/anno_box must be 16-byte aligned (task %d)", fn, t);
    }
    return GGA_OK;
}

extern "C" int gga_center_reg_loss_fwd(const gga_center_loss_table* tb, int B, int K, const gga_center_loss_weights* w, void* stream_) {
    if (int rc = center_loss_check("gga_center_reg_loss_fwd", tb, B, K, w, false)) return rc;
    hipLaunchKernelGGL(center_reg_loss_fwd_kernel, dim3(tb->n_tasks), dim3(CT_THREADS), 0, (hipStream_t)stream_, *tb, B * K, *w);
    GGA_CHECK_LAUNCH("center_reg_loss_fwd_kernel");
    return GGA_OK;
}

extern "C" int gga_center_reg_loss_bwd(const gga_center_loss_table* tb, int B, int K, const gga_center_loss_weights* w, void* stream_) {
    if (int rc = center_loss_check("gga_center_reg_loss_bwd", tb, B, K, w, true)) return rc;
    hipLaunchKernelGGL(center_reg_loss_bwd_kernel, dim3((B * K * 8 + CT_THREADS - 1) / CT_THREADS, tb->n_tasks), dim3(CT_THREADS), 0,
                       (hipStream_t)stream_, *tb, B * K, *w);
    GGA_CHECK_LAUNCH("center_reg_loss_bwd_kernel");
    return GGA_OK;
}
