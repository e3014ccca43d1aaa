// What the two fused PillarFeatureNet fronts share: pfn.hip (hard voxels, padded [M,P,4]) and the fused
// DynamicPillarFeatureNet section of dynamic_voxel.hip (points + voxel map). Per-thread and per-block device code lives
// here once; the two single-block kernels both fronts launch (statistics, backward close) are defined in pfn.hip and
// reached through pfn_launch_stats / pfn_launch_bwd_final. The decorations, the moments accumulation, the dot product
// and the arg-max stay in their own files: they differ in arithmetic (DESIGN.md, a2').
#pragma once
#include "gga_common.h"

#define PFN_C 64
#define PFN_F 10
#define PFN_NM 65            // 10 first moments + 55 second moments
#define PFN_BW 12            // per-channel accumulators of the backward: A, Bx, G[10]
// saved (doubles): S1[F] S2[F][F] mean[C] invstd[C], then the number of rows normalised over
#define PFN_SAVED_S1 0
#define PFN_SAVED_S2 (PFN_SAVED_S1 + PFN_F)
#define PFN_SAVED_MEAN (PFN_SAVED_S2 + PFN_F * PFN_F)
#define PFN_SAVED_INVSTD (PFN_SAVED_MEAN + PFN_C)
#define PFN_SAVED_ROWS (PFN_SAVED_INVSTD + PFN_C)

struct PfnGeom {
    float vx, vy, vz, xo, yo, zo;
};
static inline PfnGeom pfn_geom(const gga_pfn_params* prm) {
    return {prm->voxel_size[0], prm->voxel_size[1], prm->voxel_size[2], prm->offsets[0], prm->offsets[1], prm->offsets[2]};
}

// Pillar centre of the cell co = (batch, z, y, x): coors * voxel_size + offset as TWO rounded f32 ops like the reference
// (pillar_encoder.py:141-150). A 1-ulp difference of the ~70 m centre is amplified by gamma*invstd ~ 30-60 downstream.
// HIP's __fmul_rn/__fadd_rn are plain * and + and hipcc fuses them under its default -ffp-contract=fast, so the product
// is passed through an empty asm to keep it a separately rounded value.
__device__ __forceinline__ void pfn_centre(const int4 co, const PfnGeom g, float cen[3]) {
    float tx = (float)co.w * g.vx, ty = (float)co.z * g.vy, tz = (float)co.y * g.vz;
    asm volatile("" : "+v"(tx), "+v"(ty), "+v"(tz));
    cen[0] = tx + g.xo; cen[1] = ty + g.yo; cen[2] = tz + g.zo;
}

// lane = output channel: its row of the [C][F] weight, kept in registers
__device__ __forceinline__ void pfn_load_weights(const float* __restrict__ weight, int lane, float w[PFN_F]) {
#pragma unroll
    for (int a = 0; a < PFN_F; ++a) w[a] = weight[lane * PFN_F + a];
}

// a device-side count clamped to [0, cap]; cap itself when there is no count (exact-sized buffers)
__device__ __forceinline__ int64_t pfn_clamped(const int32_t* __restrict__ count, int64_t cap) {
    if (!count) return cap;
    const int64_t v = *count;
    return v < cap ? (v < 0 ? 0 : v) : cap;
}

// Tail of a moments kernel (256 threads): the block's sum of every moment in a fixed order -> partials[block][NM]
__device__ __forceinline__ void pfn_moments_commit(const double acc[PFN_NM], double* __restrict__ partials) {
    __shared__ double sh[4][PFN_NM];
#pragma unroll
    for (int i = 0; i < PFN_NM; ++i) {
        const double s = wave_sum(acc[i]);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][i] = s;
    }
    __syncthreads();
    if (threadIdx.x < PFN_NM)
        partials[(int64_t)blockIdx.x * PFN_NM + threadIdx.x] =
            (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]);
}

// Tail of a backward kernel (4 waves, lane = channel): the four waves' accumulators -> partials[block][BW][C]
__device__ __forceinline__ void pfn_bwd_commit(const float acc[PFN_BW], float* __restrict__ partials) {
    __shared__ float sh[4][PFN_BW][PFN_C];
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < PFN_BW; ++i) sh[threadIdx.x >> 6][i][lane] = acc[i];
    __syncthreads();
    for (int t = threadIdx.x; t < PFN_BW * PFN_C; t += 256) {
        const int i = t / PFN_C, c = t - i * PFN_C;
        partials[(int64_t)blockIdx.x * PFN_BW * PFN_C + t] = (sh[0][i][c] + sh[1][i][c]) + (sh[2][i][c] + sh[3][i][c]);
    }
}

// grids: one thread per item (moments), one wave per item (apply, backward)
static inline int pfn_blocks(int64_t m) {
    int64_t b = (m + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 256 ? 256 : b));
}
static inline int pfn_wave_blocks(int64_t m) {
    int64_t b = (m + 3) / 4;
    return (int)(b < 1 ? 1 : (b > 512 ? 512 : b));
}

static inline int pfn_check_params(const char* fn, const gga_pfn_params* prm) {
    GGA_REQUIRE(prm, "%s: null params", fn);
    GGA_REQUIRE(prm->channels == PFN_C && prm->in_features == 4,
                "%s: the fused kernel is specialised for 4 point features -> %d channels (got %d -> %d)", fn, PFN_C,
                prm->in_features, prm->channels);
    return GGA_OK;
}

// pfn.hip. Statistics over min(cap, *count) * rows_per_item rows (cap items when count is null) from the moments
// partials, or the running statistics in eval mode -> saved, scale_shift[2][C]; update_when_empty: whether zero rows
// still move the running statistics (the hard front does, the dynamic one does not).
int pfn_launch_stats(const double* partials, int nblocks, const int32_t* count, int64_t cap, int rows_per_item,
                     int update_when_empty, const float* weight, const float* gamma, const float* beta,
                     const gga_pfn_params* prm, float* running_mean, float* running_var, double* saved, float* scale_shift,
                     hipStream_t stream);
// pfn.hip. Closes the BatchNorm backward from the backward partials [nblocks][BW][C] and the saved moments.
int pfn_launch_bwd_final(const float* partials, int nblocks, const float* weight, const float* gamma, const double* saved,
                         float* grad_weight, float* grad_gamma, float* grad_beta, hipStream_t stream);
