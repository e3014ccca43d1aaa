// Per-class 3D NMS of a whole batch in a fixed number of launches: FCAF3DHead._nms (mmdet3d/models/dense_heads/fcaf3d_head.py,
// the per-class loop around mmcv's nms3d / nms3d_normal) for every (scene, class) pair at once.
//
// The python loop this replaces runs, per scene and class, one nonzero (a host synchronisation), a stable sort, the two
// launches of gga_nms_rotated_sorted and one count read-back: 8 x 18 = 144 rounds at the ScanNet shape. Here:
//   mcn_key_kernel      one 64-bit key per (row, class) pair: scene | class | score bits made to sort descending; a pair that
//                       is no candidate (score <= score_thr, NaN, scene out of range) gets a key above every real one
//   rocPRIM radix sort  stable, of (key, pair index): the pairs of a (scene, class) segment become contiguous, in descending
//                       score order, ties in input order - the order `torch.sort(descending=True, stable=True)` gives the loop
//   mcn_segment_kernel  where each segment begins and ends in the sorted order
//   mcn_nms_kernel      greedy NMS, one workgroup per segment, matrix-free (below)
//   mcn_pack_kernel     the kept pairs of all segments packed scene by scene, class-ascending, and the per-scene counts
// Nothing is read back: segment sizes stay on the device, and the n^2 / 8-byte overlap mask of gga_nms_rotated_sorted (whose
// size the host would have to know per segment) is never formed.
//
// mcn_nms_kernel walks its segment in blocks of 64 candidates. A block is first tested against the boxes kept so far: lane =
// candidate, the 16 waves share the kept list, which passes through LDS in chunks of MCN_CHUNK boxes with their cos / sin (the
// chunk that is resident is only extended, so a segment that keeps <= MCN_CHUNK boxes gathers each kept box once). The block's
// survivors then resolve among themselves on a 64 x 64 bit mask as nms_scan_kernel does, and are appended to the kept list.
// The overlap is rotated_iou_rot(kept, candidate) of rotated_iou.h for oriented and axis-aligned boxes alike (heading 0 for
// the latter, as nms3d_normal calls the rotated routine): the earlier box first, the float operations of nms_mask_kernel.
#include "gga_index.h"
#include "rotated_iou.h"

#define MCN_THREADS 1024
#define MCN_WAVES (MCN_THREADS / 64)
#define MCN_CHUNK 256
#define MCN_CLASS_BITS 7                                   // GGA_MULTICLASS_NMS_MAX_CLASSES = 128
#define MCN_SCENE_SHIFT (32 + MCN_CLASS_BITS)
#define MCN_MAX_SCENES (1 << 20)

static int mcn_scene_bits(int n_scenes) {
    int b = 1;
    while ((1 << b) < n_scenes) ++b;
    return b;
}

// key of a candidate: scene << 39 | class << 32 | ~(order-preserving bits of the score); -0.0 counts as +0.0 (they tie)
__global__ __launch_bounds__(256) void mcn_key_kernel(const float* __restrict__ scores, const int64_t* __restrict__ scene,
                                                     int64_t n_pairs, int C, int n_scenes, float score_thr, uint64_t sentinel,
                                                     uint64_t* __restrict__ keys) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pairs) return;
    const int64_t row = p / C;
    const int c = (int)(p - row * C);
    const float s = scores[p];
    const int64_t sc = scene[row];
    uint64_t key = sentinel;
    if (s > score_thr && sc >= 0 && sc < n_scenes) {       // (false for a NaN score)
        uint32_t u = __float_as_uint(s == 0.0f ? 0.0f : s);
        u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);    // ascending with the float
        key = ((uint64_t)sc << MCN_SCENE_SHIFT) | ((uint64_t)c << 32) | (uint64_t)(~u);
    }
    keys[p] = key;
}

__global__ __launch_bounds__(256) void mcn_segment_kernel(const uint64_t* __restrict__ keys, int64_t n_pairs, int C,
                                                         uint64_t sentinel, int32_t* __restrict__ seg_begin,
                                                         int32_t* __restrict__ seg_end) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pairs) return;
    const uint64_t k = keys[i];
    if (k & sentinel) return;
    const uint64_t id = k >> 32;                           // scene << 7 | class
    const int64_t seg = (int64_t)(id >> MCN_CLASS_BITS) * C + (int64_t)(id & ((1u << MCN_CLASS_BITS) - 1));
    if (i == 0 || (keys[i - 1] >> 32) != id) seg_begin[seg] = (int32_t)i;
    if (i + 1 == n_pairs || (keys[i + 1] >> 32) != id) seg_end[seg] = (int32_t)(i + 1);
}

// (x, y, dx, dy, heading, cos, sin) of the box of pair p
__device__ __forceinline__ void mcn_load_box(const float* __restrict__ boxes, int p, int C, float* d) {
    const float* b = boxes + (int64_t)(p / C) * 7;
    d[0] = b[0]; d[1] = b[1]; d[2] = b[3]; d[3] = b[4]; d[4] = b[6];
    d[5] = cosf(b[6]); d[6] = sinf(b[6]);
}

__global__ __launch_bounds__(MCN_THREADS) void mcn_nms_kernel(const float* __restrict__ boxes, int C,
                                                             const int32_t* __restrict__ order,
                                                             const int32_t* __restrict__ seg_begin,
                                                             const int32_t* __restrict__ seg_end, float thr, int32_t* kept,
                                                             int32_t* __restrict__ seg_kept) {
    __shared__ float kb[MCN_CHUNK][7];
    __shared__ float cb[64][7];
    __shared__ int cpair[64];
    __shared__ unsigned long long supp, bmask[64];
    __shared__ int nk_s;
    const int seg = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b0 = seg_begin[seg], m = seg_end[seg] - b0;
    if (m <= 0) {
        if (tid == 0) seg_kept[seg] = 0;
        return;
    }
    int nk = 0, res_chunk = -1, res_cnt = 0;               // kept so far; the chunk of the kept list that sits in kb
    for (int blk = 0; blk < m; blk += 64) {
        const int cnt = min(64, m - blk);
        if (tid < 64) {
            if (tid < cnt) {
                const int p = order[b0 + blk + tid];
                cpair[tid] = p;
                mcn_load_box(boxes, p, C, cb[tid]);
            }
            bmask[tid] = 0;
        }
        if (tid == 0) supp = 0;
        __syncthreads();
        float me[5], mc = 1.0f, ms = 0.0f;
#pragma unroll
        for (int k = 0; k < 5; ++k) me[k] = lane < cnt ? cb[lane][k] : 0.0f;
        if (lane < cnt) { mc = cb[lane][5]; ms = cb[lane][6]; }
        // 1. against the kept list: lane = candidate, the waves take the kept boxes of the chunk in turn
        for (int q = 0; q * MCN_CHUNK < nk; ++q) {
            const int qcnt = min(MCN_CHUNK, nk - q * MCN_CHUNK);
            const int lo = res_chunk == q ? res_cnt : 0;
            __syncthreads();                               // (the chunk's readers of the round before)
            for (int e = lo + tid; e < qcnt; e += MCN_THREADS) mcn_load_box(boxes, kept[b0 + q * MCN_CHUNK + e], C, kb[e]);
            res_chunk = q; res_cnt = qcnt;
            __syncthreads();
            bool s = lane >= cnt || ((supp >> lane) & 1ull);
            for (int k = wave; k < qcnt; k += MCN_WAVES) {
                if (__ballot(!s) == 0ull) break;
                if (!s && rotated_iou_rot(kb[k], kb[k][5], kb[k][6], me, mc, ms, 0) > thr) s = true;
            }
            const unsigned long long bal = __ballot(s && lane < cnt);
            if (lane == 0 && bal) atomicOr(&supp, bal);
        }
        __syncthreads();
        // 2. the block among itself: bit j of bmask[i] = the earlier candidate i overlaps the later candidate j
        const unsigned long long sv = supp;
        {
            const int i = lane, j0 = max(i + 1, wave * (64 / MCN_WAVES)), j1 = min(cnt, (wave + 1) * (64 / MCN_WAVES));
            unsigned long long bits = 0;
            if (i < cnt && !((sv >> i) & 1ull))
                for (int j = j0; j < j1; ++j)
                    if (!((sv >> j) & 1ull) && rotated_iou_rot(me, mc, ms, cb[j], cb[j][5], cb[j][6], 0) > thr) bits |= 1ull << j;
            if (bits) atomicOr(&bmask[i], bits);
        }
        __syncthreads();
        // 3. greedy scan of the block in score order (every lane of wave 0 walks the same words), survivors appended
        if (wave == 0) {
            unsigned long long removed = sv, keep = 0;
            for (int c = 0; c < cnt; ++c) {
                if ((removed >> c) & 1ull) continue;
                keep |= 1ull << c;
                removed |= bmask[c];
            }
            if ((keep >> lane) & 1ull) kept[b0 + nk + __popcll(keep & ((1ull << lane) - 1ull))] = cpair[lane];
            if (lane == 0) nk_s = nk + __popcll(keep);
        }
        __threadfence_block();
        __syncthreads();
        nk = nk_s;
    }
    if (tid == 0) seg_kept[seg] = nk;
}

// segment (scene, class) -> its kept pairs at out_*[sum of the kept of every segment before it ...]; out_count[scene]
__global__ __launch_bounds__(256) void mcn_pack_kernel(const int32_t* __restrict__ kept, const int32_t* __restrict__ seg_begin,
                                                      const int32_t* __restrict__ seg_kept, int C, int32_t* __restrict__ out_row,
                                                      int32_t* __restrict__ out_class, int32_t* __restrict__ out_count) {
    __shared__ int part[4];
    const int seg = blockIdx.x, tid = threadIdx.x;
    int before = 0;
    for (int s = tid; s < seg; s += 256) before += seg_kept[s];
    before = wave_sum(before);
    if ((tid & 63) == 0) part[tid >> 6] = before;
    __syncthreads();
    before = part[0] + part[1] + part[2] + part[3];
    const int nk = seg_kept[seg], b0 = seg_begin[seg], c = seg % C;
    for (int k = tid; k < nk; k += 256) {
        out_row[before + k] = kept[b0 + k] / C;
        out_class[before + k] = c;
    }
    if (c == 0 && tid == 0) {
        int total = 0;
        for (int k = 0; k < C; ++k) total += seg_kept[seg + k];
        out_count[seg / C] = total;
    }
}

static bool mcn_sizes_ok(int64_t n, int C, int n_scenes) {
    return n >= 0 && C >= 1 && C <= GGA_MULTICLASS_NMS_MAX_CLASSES && n_scenes >= 1 && n_scenes <= MCN_MAX_SCENES &&
           n * C < ((int64_t)1 << 31) && (int64_t)n_scenes * C < ((int64_t)1 << 31);
}

// temporaries of the sort | keys | sorted keys | sorted pair indices | kept pairs | segment begin, end, kept
extern "C" size_t gga_multiclass_nms3d_workspace_bytes(int64_t n, int n_classes, int n_scenes) {
    if (!mcn_sizes_ok(n, n_classes, n_scenes)) return 0;
    const size_t np = (size_t)n * n_classes, ns = (size_t)n_scenes * n_classes;
    return (np ? gga_argsort_temp_bytes<uint64_t>((int64_t)np, 64) : 0) + 2 * gga_align_up(np * 8, 256) + 2 * gga_align_up(np * 4, 256) +
           gga_align_up(3 * ns * 4, 256);
}

extern "C" int gga_multiclass_nms3d(const float* boxes, const float* scores, const int64_t* scene, int64_t n, int n_classes,
                                    int n_scenes, float score_thr, float iou_thr, int32_t* out_row, int32_t* out_class,
                                    int32_t* out_count, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int C = n_classes;
    GGA_REQUIRE(mcn_sizes_ok(n, C, n_scenes),
                "gga_multiclass_nms3d: bad sizes (n=%lld classes=%d scenes=%d; classes in 1..%d, scenes in 1..%d, n * classes < 2^31)",
                (long long)n, C, n_scenes, GGA_MULTICLASS_NMS_MAX_CLASSES, MCN_MAX_SCENES);
    GGA_REQUIRE(out_count, "gga_multiclass_nms3d: null out_count");
    GGA_REQUIRE(n == 0 || (boxes && scores && scene && out_row && out_class && workspace),
                "gga_multiclass_nms3d: null pointer argument");
    const size_t need = gga_multiclass_nms3d_workspace_bytes(n, C, n_scenes);
    if (n > 0 && workspace_bytes < need) {
        gga_set_error("gga_multiclass_nms3d: workspace %zu B < required %zu B", workspace_bytes, need);
        return GGA_ERR_INVALID_ARG;
    }
    if (n == 0) {
        GGA_CHECK_HIP(hipMemsetAsync(out_count, 0, (size_t)n_scenes * 4, stream), "multiclass nms memset");
        return GGA_OK;
    }
    const int64_t np = n * C;
    const int ns = n_scenes * C;
    unsigned char* w = static_cast<unsigned char*>(workspace);
    const size_t tb_max = gga_argsort_temp_bytes<uint64_t>(np, 64);
    uint64_t* keys = reinterpret_cast<uint64_t*>(w + tb_max);
    uint64_t* keys_sorted = reinterpret_cast<uint64_t*>(w + tb_max + gga_align_up((size_t)np * 8, 256));
    int32_t* order = reinterpret_cast<int32_t*>(w + tb_max + 2 * gga_align_up((size_t)np * 8, 256));
    int32_t* kept = reinterpret_cast<int32_t*>(w + tb_max + 2 * gga_align_up((size_t)np * 8, 256) + gga_align_up((size_t)np * 4, 256));
    int32_t* seg_begin = reinterpret_cast<int32_t*>(w + tb_max + 2 * gga_align_up((size_t)np * 8, 256) + 2 * gga_align_up((size_t)np * 4, 256));
    int32_t *seg_end = seg_begin + ns, *seg_kept = seg_end + ns;
    const int sbits = mcn_scene_bits(n_scenes);
    const uint64_t sentinel = 1ull << (MCN_SCENE_SHIFT + sbits);       // above every real key; the sort covers this bit too
    GGA_CHECK_HIP(hipMemsetAsync(seg_begin, 0, (size_t)2 * ns * 4, stream), "multiclass nms memset");
    const unsigned pair_blocks = (unsigned)((np + 255) / 256);
    hipLaunchKernelGGL(mcn_key_kernel, dim3(pair_blocks), dim3(256), 0, stream, scores, scene, np, C, n_scenes, score_thr, sentinel,
                       keys);
    GGA_CHECK_LAUNCH("mcn_key_kernel");
    if (int rc = gga_argsort("gga_multiclass_nms3d", w, (const uint64_t*)keys, keys_sorted, order, np, MCN_SCENE_SHIFT + sbits + 1, stream))
        return rc;
    hipLaunchKernelGGL(mcn_segment_kernel, dim3(pair_blocks), dim3(256), 0, stream, keys_sorted, np, C, sentinel, seg_begin, seg_end);
    GGA_CHECK_LAUNCH("mcn_segment_kernel");
    hipLaunchKernelGGL(mcn_nms_kernel, dim3((unsigned)ns), dim3(MCN_THREADS), 0, stream, boxes, C, order, seg_begin, seg_end, iou_thr,
                       kept, seg_kept);
    GGA_CHECK_LAUNCH("mcn_nms_kernel");
    hipLaunchKernelGGL(mcn_pack_kernel, dim3((unsigned)ns), dim3(256), 0, stream, kept, seg_begin, seg_kept, C, out_row, out_class,
                       out_count);
    GGA_CHECK_LAUNCH("mcn_pack_kernel");
    return GGA_OK;
}
