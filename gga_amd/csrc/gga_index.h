// Index-building helpers shared by the voxelizers and compactors (voxelize.hip, dynamic_voxel.hip, points_prep.hip,
// frame_points.hip, sparse_index.hip, multiclass_nms.hip): the argsort, the workgroup scans, the 64-bit hash and the frame
// table / voxel grid of the point ops. Helpers only - every kernel stays in its file.
#pragma once
#include "gga_common.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

// ---- argsort ---------------------------------------------------------------------------------------------------------
// order[i] = index of the i-th smallest key over the key bits [0, bits): a stable LSD radix sort of (key, counting iterator).
// rocPRIM's default hands anything up to 2^20 items to its merge sort (dozens of merge-path launches); with the limit at 4096
// a call goes through Onesweep: one histogram and one pass per 8 key bits.
typedef rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config, rocprim::default_config, 4096> gga_argsort_config;

template <typename Key>
static size_t gga_argsort_temp_bytes(int64_t n, int bits) {
    size_t tb = 0;
    (void)rocprim::radix_sort_pairs<gga_argsort_config>(nullptr, tb, (const Key*)nullptr, (Key*)nullptr,
                                                        rocprim::counting_iterator<int32_t>(0), (int32_t*)nullptr, (size_t)n, 0,
                                                        (unsigned)bits, (hipStream_t)0);
    return gga_align_up(tb, 256);
}

// `temp`: gga_argsort_temp_bytes<Key>(n, bits) bytes (a caller that lays its workspace out for more bits passes the same pointer)
template <typename Key>
static int gga_argsort(const char* who, void* temp, const Key* keys_in, Key* keys_out, int32_t* order, int64_t n, int bits,
                       hipStream_t stream) {
    size_t tb = gga_argsort_temp_bytes<Key>(n, bits);
    const hipError_t e = rocprim::radix_sort_pairs<gga_argsort_config>(temp, tb, keys_in, keys_out, rocprim::counting_iterator<int32_t>(0),
                                                                       order, (size_t)n, 0, (unsigned)bits, stream);
    if (e != hipSuccess) {
        gga_set_error("%s: rocprim::radix_sort_pairs: %s", who, hipGetErrorString(e));
        return GGA_ERR_LAUNCH;
    }
    return GGA_OK;
}

// ---- workgroup scans -------------------------------------------------------------------------------------------------
// Every thread of a workgroup of NT threads (a multiple of 64, x only) calls these together. Two barriers each, so a kernel
// may call them again right away (a loop over chunks) and values written to LDS before the call are visible after it.

// sum of the earlier waves' totals -> return, sum of all -> total; `wave_total` is read from the wave's `writer` lane
template <int NT>
__device__ __forceinline__ int gga_block_wave_offset(int wave_total, bool writer, int& total) {
    __shared__ int gga_wave_tot[NT / 64];
    const int wave = threadIdx.x >> 6;
    if (writer) gga_wave_tot[wave] = wave_total;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        const int t = gga_wave_tot[w];
        base += (w < wave) ? t : 0;
        tot += t;
    }
    __syncthreads();
    total = tot;
    return base;
}

// exclusive prefix of one value per thread, in thread order (wave __shfl_up, then the per-wave totals through LDS)
template <int NT>
__device__ __forceinline__ int gga_block_scan(int v, int& total) {
    const int lane = threadIdx.x & 63;
    int s = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(s, o, 64); if (lane >= o) s += t; }
    return gga_block_wave_offset<NT>(s, lane == 63, total) + s - v;
}

// the same for a flag (compaction: the rank of a kept thread among the kept ones): wave ballot + popcount
template <int NT>
__device__ __forceinline__ int gga_block_scan_flag(bool flag, int& total) {
    const int lane = threadIdx.x & 63;
    const unsigned long long bal = __ballot(flag);
    return gga_block_wave_offset<NT>(__popcll(bal), lane == 0, total) + __popcll(bal & ((1ull << lane) - 1ull));
}

// ---- 64-bit open-addressing hash ---------------------------------------------------------------------------------------
#define GGA_HASH_EMPTY 0xFFFFFFFFFFFFFFFFull       // a table is emptied by a 0xFF fill

// slots for n keys: a power of two >= 2 n + 2 (load <= 1/2, linear probing always ends)
static inline uint64_t gga_hash_capacity(int64_t n) {
    uint64_t cap = 1024;
    while (cap < (uint64_t)(2 * n + 2)) cap <<= 1;
    return cap;
}

__device__ __forceinline__ uint32_t gga_hash64(unsigned long long k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return (uint32_t)k;
}

// slot of `key`, claimed by a 64-bit CAS if the key is new; mask = capacity - 1
__device__ __forceinline__ uint32_t gga_hash_insert(unsigned long long* keys, uint32_t mask, unsigned long long key) {
    uint32_t h = gga_hash64(key) & mask;
    while (true) {
        const unsigned long long prev = atomicCAS(&keys[h], GGA_HASH_EMPTY, key);
        if (prev == GGA_HASH_EMPTY || prev == key) return h;
        h = (h + 1) & mask;
    }
}

// ---- frames of points and their voxel grid ---------------------------------------------------------------------------
// Frames concatenated in one array (kernel argument, by value): frame b is rows [off[b], off[b + 1]), of which the first
// n(b) hold points.
struct GgaFrames {
    int32_t off[GGA_MAX_BATCH + 1];
    const int32_t* cnt;     // optional device-side point counts (frames stored at capacity offsets), clamped to the capacity
    __device__ __forceinline__ int n(int b) const {
        const int cap = off[b + 1] - off[b];
        if (!cnt) return cap;
        const int c = cnt[b];
        return c < 0 ? 0 : (c < cap ? c : cap);
    }
};

// offsets_host [batch + 1] (batch already checked against GGA_MAX_BATCH) -> frames; *max_n = rows of the largest frame
static int gga_frames_from_host(const char* who, const int64_t* offsets_host, const int32_t* counts_dev, int batch,
                                GgaFrames* frames, int* max_n) {
    const int64_t total = offsets_host[batch];
    GGA_REQUIRE(offsets_host[0] == 0 && total >= 0 && total < (1ll << 30), "%s: offsets must start at 0 and total points < 2^30", who);
    frames->cnt = counts_dev;
    frames->off[0] = 0;
    *max_n = 0;
    for (int b = 1; b <= batch; ++b) {
        GGA_REQUIRE(offsets_host[b] >= offsets_host[b - 1], "%s: offsets not monotone", who);
        frames->off[b] = (int32_t)offsets_host[b];
        const int nb = (int)(offsets_host[b] - offsets_host[b - 1]);
        *max_n = nb > *max_n ? nb : *max_n;
    }
    return GGA_OK;
}

struct GgaVoxGeom {
    float vs[3];
    float lo[3];
    int32_t grid[3];  // x, y, z
};

static inline GgaVoxGeom gga_vox_geom(const gga_voxel_params* prm) {
    GgaVoxGeom g;
    for (int j = 0; j < 3; ++j) { g.vs[j] = prm->voxel_size[j]; g.lo[j] = prm->pc_range[j]; }
    gga_voxel_grid_size(prm, g.grid);
    return g;
}

// Cell (x, y, z) of a point: floor((p - lo) / vs) per axis in f32 with a true division (voxel_generator.py:189). The hard and
// the dynamic voxelizer both go through this one function, so they cannot disagree on a point's cell. False = outside the
// grid: NaN and +-inf come out of the division as NaN / +-inf and fail the `0 <= cell < grid` test.
__device__ __forceinline__ bool gga_point_cell(const float* __restrict__ p, const GgaVoxGeom& g, int32_t c[3]) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float cf = floorf(__fdiv_rn(__fsub_rn(p[j], g.lo[j]), g.vs[j]));
        ok = ok && (cf >= 0.0f) && (cf < (float)g.grid[j]);
        c[j] = (int32_t)cf;
    }
    return ok;
}
