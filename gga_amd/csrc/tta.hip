// Test-time augmentation: the head maps of all views of a batch merged per scale group in ONE launch, for gfx950.
//
// Reference: mmdet3d/models/detectors/centerpoint_gga.py:123-182 (aug_test_pts). Per view, task and key it runs torch.flip,
// a slice assignment for the channel whose sign or offset a flip changes, `+=` into the first view of the scale group and a
// final `/=` - a few hundred launches over maps of a few MB. Here one thread owns one output element (or four neighbours of a
// row) of one map and walks the group's views in view order:
//     acc = value(first view); acc = acc + value(next view) ...; out = acc / n
// with value() = the mirrored read, negated or taken from 1 where the table of include/gga_hip.h says so. The additions and the
// IEEE division are those of the reference's sequence, so the result has its bits (the file is compiled without contraction).
//
// Memory-bound: every source element is read once and every output element written once, rows coalesced. A W-reversed read of
// four neighbours is still one contiguous 16-byte segment; the 16-byte form runs when W is a multiple of 4 and every base
// pointer is 16-byte aligned (then every row start is), else the same body runs one element per thread.
#include "gga_common.h"

__device__ __forceinline__ float tta_value(float x, int op) {
    return op == 0 ? x : (op == 1 ? -x : __fsub_rn(1.0f, x));
}

// what a flipped view does to channel c of a map of `kind`: 0 nothing, 1 negate, 2 one minus
__device__ __forceinline__ int tta_op(int kind, int c, int hflip, int vflip) {
    if (kind == GGA_TTA_PLAIN || c > 1) return 0;
    // reg: h -> channel 1, v -> channel 0; rot: h -> 0, v -> 1; vel: h -> 1, v -> 0
    const int h_ch = kind == GGA_TTA_ROT ? 0 : 1;
    const bool hit = (hflip && c == h_ch) || (vflip && c == 1 - h_ch);
    if (!hit) return 0;
    return kind == GGA_TTA_REG ? 2 : 1;
}

template <bool VEC>
__global__ __launch_bounds__(256) void tta_merge_kernel(gga_tta_table tb, int F, int H, int W) {
    const gga_tta_map& M = tb.map[blockIdx.y];
    const int C = M.channels;
    const int Wq = VEC ? W / 4 : W;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)tb.n_groups * F * C * H * Wq) return;
    const int q = (int)(idx % Wq);
    int64_t r = idx / Wq;
    const int h = (int)(r % H);
    r /= H;
    const int c = (int)(r % C);
    r /= C;
    const int f = (int)(r % F);
    const int s = (int)(r / F);
    const int64_t plane = (int64_t)H * W;

    float acc[VEC ? 4 : 1] = {};
    int n = 0;
    for (int v = 0; v < tb.n_views; ++v) {
        if (tb.group[v] != s) continue;                     // uniform over the grid's s: no divergence inside a row
        const int hf = tb.hflip[v], vf = tb.vflip[v];
        const int op = tta_op(M.kind, c, hf, vf);
        const float* row = M.src + (((int64_t)v * F + f) * C + c) * plane + (int64_t)(hf ? H - 1 - h : h) * W;
        if (VEC) {
            const float4 x = *reinterpret_cast<const float4*>(row + (vf ? W - 4 - 4 * q : 4 * q));
            const float e[4] = {vf ? x.w : x.x, vf ? x.z : x.y, vf ? x.y : x.z, vf ? x.x : x.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float val = tta_value(e[j], op);
                acc[j] = n == 0 ? val : __fadd_rn(acc[j], val);
            }
        } else {
            const float val = tta_value(row[vf ? W - 1 - q : q], op);
            acc[0] = n == 0 ? val : __fadd_rn(acc[0], val);
        }
        ++n;
    }
    if (n == 0) return;                                     // (the entry point refuses a group without a view)
    const float div = (float)n;
    float* out = M.dst + (((int64_t)s * F + f) * C + c) * plane + (int64_t)h * W;
    if (VEC) {
        float4 y;
        y.x = __fdiv_rn(acc[0], div);
        y.y = __fdiv_rn(acc[1], div);
        y.z = __fdiv_rn(acc[2], div);
        y.w = __fdiv_rn(acc[3], div);
        *reinterpret_cast<float4*>(out + 4 * q) = y;
    } else {
        out[q] = __fdiv_rn(acc[0], div);
    }
}

extern "C" int gga_tta_merge_maps(const gga_tta_table* tb, int n_frames, int H, int W, void* stream) {
    const char* fn = "gga_tta_merge_maps";
    GGA_REQUIRE(tb != nullptr, "%s: null table", fn);
    GGA_REQUIRE(tb->n_maps >= 1 && tb->n_maps <= GGA_TTA_MAX_MAPS, "%s: n_maps %d not in 1..%d", fn, tb->n_maps, GGA_TTA_MAX_MAPS);
    GGA_REQUIRE(tb->n_views >= 1 && tb->n_views <= GGA_TTA_MAX_VIEWS, "%s: n_views %d not in 1..%d", fn, tb->n_views,
                GGA_TTA_MAX_VIEWS);
    GGA_REQUIRE(tb->n_groups >= 1 && tb->n_groups <= tb->n_views, "%s: n_groups %d not in 1..n_views (%d)", fn, tb->n_groups,
                tb->n_views);
    GGA_REQUIRE(H > 0 && W > 0 && n_frames > 0, "%s: H %d, W %d and n_frames %d must be positive", fn, H, W, n_frames);
    bool seen[GGA_TTA_MAX_VIEWS] = {};
    for (int v = 0; v < tb->n_views; ++v) {
        GGA_REQUIRE(tb->group[v] >= 0 && tb->group[v] < tb->n_groups, "%s: group %d of view %d not in 0..%d", fn, tb->group[v], v,
                    tb->n_groups - 1);
        seen[tb->group[v]] = true;
    }
    for (int s = 0; s < tb->n_groups; ++s) GGA_REQUIRE(seen[s], "%s: group %d has no view", fn, s);
    bool vec = W % 4 == 0;
    int64_t max_items = 0;
    for (int m = 0; m < tb->n_maps; ++m) {
        const gga_tta_map& M = tb->map[m];
        GGA_REQUIRE(M.kind >= GGA_TTA_PLAIN && M.kind <= GGA_TTA_VEL, "%s: unknown kind %d of map %d", fn, M.kind, m);
        GGA_REQUIRE(M.channels >= (M.kind == GGA_TTA_PLAIN ? 1 : 2), "%s: map %d of kind %d has %d channels", fn, m, M.kind,
                    M.channels);
        GGA_REQUIRE(M.src != nullptr && M.dst != nullptr, "%s: null pointer in map %d", fn, m);
        vec = vec && ((uintptr_t)M.src % 16 == 0) && ((uintptr_t)M.dst % 16 == 0);
        const int64_t items = (int64_t)tb->n_groups * n_frames * M.channels * H * W;
        GGA_REQUIRE((int64_t)tb->n_views * n_frames * M.channels * H * W < ((int64_t)1 << 40), "%s: map %d too large", fn, m);
        max_items = items > max_items ? items : max_items;
    }
    if (vec) max_items /= 4;
    const int64_t blocks = (max_items + 255) / 256;
    GGA_REQUIRE(blocks < ((int64_t)1 << 31), "%s: %lld blocks exceed the grid", fn, (long long)blocks);
    const dim3 grid((unsigned)blocks, (unsigned)tb->n_maps);
    if (vec)
        hipLaunchKernelGGL(tta_merge_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, *tb, n_frames, H, W);
    else
        hipLaunchKernelGGL(tta_merge_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, *tb, n_frames, H, W);
    GGA_CHECK_LAUNCH(fn);
    return GGA_OK;
}
