// The mono3d test run on the device, for gfx950: the flip test-time augmentation's map merge and the tail of a whole-batch
// `get_bboxes`.
//
// gga_mono3d_tta_merge. Reference: mmdet3d/models/detectors/single_stage_mono3d.py:136-181 (aug_test). For the flipped view it
// runs, per output group and FPN level, torch.flip(dims=[3]), then `1 - x` on channel 0 of the regression maps, then
// torch.mean(torch.cat([view 0, view 1]), dim=0) and a slice assignment that puts view 0 back into the regression channels
// >= 6 - about ten launches per (group, level), on maps of a few hundred KB. Here one thread owns one output element (or four
// neighbours of a row) of one (group, level) map of one frame: a = view 0 at (h, w), b = view 1 at (h, W - 1 - w),
//     MEAN:  (a + b) * 0.5                       REG:  channel 0      (a + (1 - b)) * 0.5
//                                                      channels 1..5  (a + b) * 0.5
//                                                      channels >= 6  a
// With two views the reference's mean is one rounded float32 addition and an exact halving, and `1 - x` is one float32
// operation, so the result has the reference's bits (the file is compiled without contraction). All maps of all levels go
// in ONE launch: blockIdx.y is the table entry, and an entry whose W is a multiple of 4 and whose pointers are 16-byte aligned
// is read and written in 16-byte pieces (a W-reversed read of four neighbours is still one contiguous segment), the others
// element by element - the choice is uniform over a block. Memory-bound: every source element read once (the REG channels
// >= 6 of view 1 not at all), every output element written once.
//
// gga_mono3d_collect. Reference: the tail of box3d_multiclass_nms (mmdet3d/core/post_processing/box3d_nms.py:93-127) per image:
// the kept detections of all classes concatenated class by class, cut to the max_num highest scores when there are more, and
// every per-candidate array gathered at the kept rows. Input: the packed (row, class) lists and per-image counts that
// gga_multiclass_nms3d writes. One workgroup per image: its list's scores go to the workspace; when the list is longer than
// max_per_img, an entry's output slot is its rank (the number of entries with a higher score, or the same score earlier in the
// list), else its list position; entries whose slot is < max_per_img gather their rows into the fixed-shape outputs. The rank
// is a walk over the list per entry - lists are a few hundred entries, the candidates of one image after NMS.
#include "gga_common.h"

#define M3T_THREADS 256

__device__ __forceinline__ float m3t_pair(float a, float b, bool one_minus) {
    const float v = one_minus ? __fsub_rn(1.0f, b) : b;
    return __fmul_rn(__fadd_rn(a, v), 0.5f);
}

__global__ __launch_bounds__(M3T_THREADS) void mono3d_tta_merge_kernel(const gga_mono3d_tta_table tb) {
    const gga_mono3d_tta_map& M = tb.map[blockIdx.y];
    const int C = M.channels, H = M.H, W = M.W, F = tb.n_frames;
    const bool vec = (W % 4 == 0) && (((uintptr_t)M.src | (uintptr_t)M.dst) % 16 == 0);
    const int Wq = vec ? W / 4 : W;
    const int64_t idx = (int64_t)blockIdx.x * M3T_THREADS + threadIdx.x;
    if (idx >= (int64_t)F * C * H * Wq) return;
    const int q = (int)(idx % Wq);
    const int64_t row = idx / Wq;                           // (f * C + c) * H + h
    const int c = (int)((row / H) % C);
    const bool keep = M.kind == GGA_MONO3D_TTA_REG && c >= 6;
    const bool one_minus = M.kind == GGA_MONO3D_TTA_REG && c == 0;
    const float* a = M.src + row * W;                        // view 0 of frame f is row f of the [2 F, C, H, W] map
    const float* b = a + (int64_t)F * C * H * W;             // view 1
    float* out = M.dst + row * W;
    if (vec) {
        float4 y = *reinterpret_cast<const float4*>(a + 4 * q);
        if (!keep) {
            const float4 x = *reinterpret_cast<const float4*>(b + (W - 4 - 4 * q));
            y.x = m3t_pair(y.x, x.w, one_minus);
            y.y = m3t_pair(y.y, x.z, one_minus);
            y.z = m3t_pair(y.z, x.y, one_minus);
            y.w = m3t_pair(y.w, x.x, one_minus);
        }
        *reinterpret_cast<float4*>(out + 4 * q) = y;
    } else {
        out[q] = keep ? a[q] : m3t_pair(a[q], b[W - 1 - q], one_minus);
    }
}

extern "C" int gga_mono3d_tta_merge(const gga_mono3d_tta_table* tb, void* stream) {
    const char* fn = "gga_mono3d_tta_merge";
    GGA_REQUIRE(tb != nullptr, "%s: null table", fn);
    GGA_REQUIRE(tb->n_maps >= 1 && tb->n_maps <= GGA_MONO3D_TTA_MAX_MAPS, "%s: n_maps %d not in 1..%d", fn, tb->n_maps,
                GGA_MONO3D_TTA_MAX_MAPS);
    GGA_REQUIRE(tb->n_frames > 0, "%s: n_frames %d must be positive", fn, tb->n_frames);
    int64_t max_items = 0;
    for (int m = 0; m < tb->n_maps; ++m) {
        const gga_mono3d_tta_map& M = tb->map[m];
        GGA_REQUIRE(M.src != nullptr && M.dst != nullptr, "%s: null pointer in map %d", fn, m);
        GGA_REQUIRE(M.H > 0 && M.W > 0 && M.channels > 0, "%s: map %d: H %d, W %d and channels %d must be positive", fn, m, M.H,
                    M.W, M.channels);
        GGA_REQUIRE(M.kind == GGA_MONO3D_TTA_MEAN || M.kind == GGA_MONO3D_TTA_REG, "%s: unknown kind %d of map %d", fn, M.kind, m);
        GGA_REQUIRE(M.kind != GGA_MONO3D_TTA_REG || M.channels >= 7, "%s: REG map %d has %d channels, fewer than 7", fn, m,
                    M.channels);
        const int64_t items = (int64_t)tb->n_frames * M.channels * M.H * M.W;
        GGA_REQUIRE(2 * items < ((int64_t)1 << 40), "%s: map %d too large", fn, m);
        max_items = items > max_items ? items : max_items;  // (a 16-byte entry uses a quarter of its blocks; the rest return)
    }
    const int64_t blocks = (max_items + M3T_THREADS - 1) / M3T_THREADS;
    GGA_REQUIRE(blocks < ((int64_t)1 << 31), "%s: %lld blocks exceed the grid", fn, (long long)blocks);
    hipLaunchKernelGGL(mono3d_tta_merge_kernel, dim3((unsigned)blocks, (unsigned)tb->n_maps), dim3(M3T_THREADS), 0,
                       (hipStream_t)stream, *tb);
    GGA_CHECK_LAUNCH(fn);
    return GGA_OK;
}

// ---------------------------------------------------------------------------------------------------------------- collect
struct M3CArgs {
    const int32_t *rows, *classes, *counts;
    const float *scores, *boxes, *boxes2d;
    const int64_t *dir, *attr;
    int64_t n_rows, n_pairs;
    int n_images, n_classes, score_stride, code, max_per_img;
    float *out_boxes, *out_scores, *out_boxes2d;
    int32_t *out_labels, *out_dir, *out_attr, *out_count;
    float* list_scores;
};

__global__ __launch_bounds__(M3T_THREADS) void mono3d_collect_kernel(const M3CArgs A) {
    const int img = blockIdx.x, tid = threadIdx.x, M = A.max_per_img;
    int64_t start = 0;
    for (int i = 0; i < img; ++i) start += max(A.counts[i], 0);
    int64_t k64 = max(A.counts[img], 0);
    if (start > A.n_pairs) start = A.n_pairs;               // (counts that do not fit the lists: nothing beyond them is read)
    if (start + k64 > A.n_pairs) k64 = A.n_pairs - start;
    const int k = (int)k64;
    const int32_t* rows = A.rows + start;
    const int32_t* classes = A.classes + start;
    float* ls = A.list_scores + start;
    const bool cap = k > M;
    if (cap) {
        for (int i = tid; i < k; i += M3T_THREADS) {
            const int64_t r = rows[i];
            const int c = classes[i];
            const bool ok = r >= 0 && r < A.n_rows && c >= 0 && c < A.n_classes;
            ls[i] = ok ? A.scores[r * A.score_stride + c] : -INFINITY;
        }
        __syncthreads();
    }
    const int n_out = min(k, M);
    for (int i = tid; i < k; i += M3T_THREADS) {
        const int64_t r = rows[i];
        const int c = classes[i];
        if (!(r >= 0 && r < A.n_rows && c >= 0 && c < A.n_classes)) continue;
        int slot = i;
        if (cap) {
            const float s = ls[i];
            slot = 0;
            for (int j = 0; j < k; ++j) {
                const float t = ls[j];
                slot += (t > s || (t == s && j < i)) ? 1 : 0;
            }
            if (slot >= M) continue;
        }
        const int64_t o = (int64_t)img * M + slot;
        for (int d = 0; d < A.code; ++d) A.out_boxes[o * A.code + d] = A.boxes[r * A.code + d];
        A.out_scores[o] = A.scores[r * A.score_stride + c];
        A.out_labels[o] = c;
        A.out_dir[o] = A.dir ? (int32_t)A.dir[r] : 0;
        A.out_attr[o] = A.attr ? (int32_t)A.attr[r] : 0;
        if (A.out_boxes2d)
            for (int d = 0; d < 4; ++d) A.out_boxes2d[o * 4 + d] = A.boxes2d[r * 4 + d];
    }
    // the slots behind the last detection read as zero (the buffer is downloaded whole)
    for (int i = n_out + tid; i < M; i += M3T_THREADS) {
        const int64_t o = (int64_t)img * M + i;
        for (int d = 0; d < A.code; ++d) A.out_boxes[o * A.code + d] = 0.0f;
        A.out_scores[o] = 0.0f;
        A.out_labels[o] = 0;
        A.out_dir[o] = 0;
        A.out_attr[o] = 0;
        if (A.out_boxes2d)
            for (int d = 0; d < 4; ++d) A.out_boxes2d[o * 4 + d] = 0.0f;
    }
    if (tid == 0) A.out_count[img] = n_out;
}

static bool m3c_sizes_ok(int64_t n_rows, int n_classes, int n_images) {
    return n_rows >= 0 && n_classes >= 1 && n_classes <= GGA_MULTICLASS_NMS_MAX_CLASSES && n_images >= 1 &&
           n_images <= GGA_MONO3D_COLLECT_MAX_IMAGES && n_rows * n_classes < ((int64_t)1 << 31);
}

// the scores of the kept lists, one float per (row, class) pair
extern "C" size_t gga_mono3d_collect_workspace_bytes(int64_t n_rows, int n_classes, int n_images) {
    if (!m3c_sizes_ok(n_rows, n_classes, n_images)) return 0;
    return gga_align_up((size_t)(n_rows * n_classes) * 4 + 4, 256);
}

extern "C" int gga_mono3d_collect(const int32_t* rows, const int32_t* classes, const int32_t* counts, int n_images, int64_t n_rows,
                                  int n_classes, const float* scores, int score_stride, const float* boxes, int code,
                                  const int64_t* dir, const int64_t* attr, const float* boxes2d, int max_per_img, float* out_boxes,
                                  float* out_scores, int32_t* out_labels, int32_t* out_dir, int32_t* out_attr, float* out_boxes2d,
                                  int32_t* out_count, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "gga_mono3d_collect";
    GGA_REQUIRE(m3c_sizes_ok(n_rows, n_classes, n_images),
                "%s: bad sizes (n_rows=%lld classes=%d images=%d; classes in 1..%d, images in 1..%d, n_rows * classes < 2^31)", fn,
                (long long)n_rows, n_classes, n_images, GGA_MULTICLASS_NMS_MAX_CLASSES, GGA_MONO3D_COLLECT_MAX_IMAGES);
    GGA_REQUIRE(code >= 1 && code <= 64, "%s: code size %d not in 1..64", fn, code);
    GGA_REQUIRE(max_per_img >= 1 && (int64_t)max_per_img * n_images < ((int64_t)1 << 24), "%s: max_per_img %d not in 1..2^24 / images",
                fn, max_per_img);
    GGA_REQUIRE(score_stride >= n_classes, "%s: score_stride %d below the %d classes", fn, score_stride, n_classes);
    GGA_REQUIRE(counts && out_count && out_boxes && out_scores && out_labels && out_dir && out_attr, "%s: null output or count pointer",
                fn);
    GGA_REQUIRE((boxes2d == nullptr) == (out_boxes2d == nullptr), "%s: boxes2d and out_boxes2d must both be given or both be null", fn);
    GGA_REQUIRE(n_rows == 0 || (rows && classes && scores && boxes && workspace), "%s: null pointer argument", fn);
    const size_t need = gga_mono3d_collect_workspace_bytes(n_rows, n_classes, n_images);
    if (n_rows > 0 && workspace_bytes < need) {
        gga_set_error("%s: workspace %zu B < required %zu B", fn, workspace_bytes, need);
        return GGA_ERR_INVALID_ARG;
    }
    M3CArgs A;
    A.rows = rows; A.classes = classes; A.counts = counts;
    A.scores = scores; A.boxes = boxes; A.boxes2d = boxes2d;
    A.dir = dir; A.attr = attr;
    A.n_rows = n_rows; A.n_pairs = n_rows * n_classes;
    A.n_images = n_images; A.n_classes = n_classes; A.score_stride = score_stride; A.code = code; A.max_per_img = max_per_img;
    A.out_boxes = out_boxes; A.out_scores = out_scores; A.out_boxes2d = out_boxes2d;
    A.out_labels = out_labels; A.out_dir = out_dir; A.out_attr = out_attr; A.out_count = out_count;
    A.list_scores = static_cast<float*>(workspace);
    hipLaunchKernelGGL(mono3d_collect_kernel, dim3((unsigned)n_images), dim3(M3T_THREADS), 0, (hipStream_t)stream, A);
    GGA_CHECK_LAUNCH(fn);
    return GGA_OK;
}
