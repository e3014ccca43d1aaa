// Dynamic voxelization for gfx950: every point keeps its cell, nothing is capped (mmcv.ops.Voxelization with
// max_num_points = -1 / max_voxels = -1, and mmcv.ops.DynamicScatter).
//
//   coors     one thread per point: cell (b, z, y, x) through gga_point_cell (the hard voxelizer's function) and a u32 key
//             ((b Z + z) Y + y) X + x; a point outside the grid, past its frame's device-side count or with a non-finite
//             coordinate gets (b, -1, -1, -1) and the key 0xFFFFFFFF ("dropped").
//   map       stable LSD radix sort of (key, point index) over the significant key bits (rocPRIM), segment heads, an
//             inclusive scan of the heads = voxel id. Ascending keys are lexicographic (b, z, y, x): the order of
//             torch.unique(dim=0) and of mmcv. The sort is stable, so a voxel's points stay in ascending original index.
//             The number of significant bits is the bit length of B Z Y X, so a dropped key's low bits (all ones) sort
//             strictly after every valid key.
//   scatter   segmented mean / max over `order`: no float atomics, a fixed summation order per voxel (two runs give the same
//             bits). Pillar populations are skewed (median a few points, hundreds to thousands next to the sensor), hence
//             the split rule: a segment of more than DV_CHUNK points is not walked by one lane group. The sorted point
//             array is cut into fixed tiles of DV_CHUNK positions; a segment longer than a tile cannot lie inside one, so at
//             most two long segments meet a tile (the one holding its first position, slot 0, and the one holding its last,
//             slot 1). One wave per tile reduces the two intersections; the voxel pass then combines a long segment's
//             partials in tile order. Max keeps the arg-max point; on ties the lowest original point index (mmcv's
//             atomicMin traceback).
//
// All writes are plain vector stores. Every buffer is sized by the caller from the point count before launch; every index
// read from `order` / `point2voxel` / arg-max is bounded by construction (order is a permutation of [0, n), voxel ids are
// < the device-side voxel count <= n) and the voxel count is clamped to the rows the caller allocated.
#include "gga_index.h"
#include "pfn_common.h"

#include <rocprim/device/device_scan.hpp>

#define DV_DROPPED 0xFFFFFFFFu
#define DV_CHUNK 256           // split rule: longest segment one lane group walks alone = positions per tile
#define DV_NO_POINT 0x7FFFFFFF

__global__ __launch_bounds__(256) void dv_coors_kernel(const float* __restrict__ points, int ndim, GgaFrames fo, GgaVoxGeom g,
                                                      int4* __restrict__ coors, uint32_t* __restrict__ keys) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= fo.off[b + 1] - fo.off[b]) return;          // every row of the frame's capacity is written
    const int64_t gi = (int64_t)fo.off[b] + i;
    int32_t c[3];                                           // x, y, z
    if (i >= fo.n(b) || !gga_point_cell(points + gi * ndim, g, c)) {
        coors[gi] = make_int4(b, -1, -1, -1);
        keys[gi] = DV_DROPPED;
        return;
    }
    coors[gi] = make_int4(b, c[2], c[1], c[0]);
    keys[gi] = (((uint32_t)b * (uint32_t)g.grid[2] + (uint32_t)c[2]) * (uint32_t)g.grid[1] + (uint32_t)c[1]) * (uint32_t)g.grid[0] +
               (uint32_t)c[0];
}

// keys of caller-supplied coordinates ([n, 3] (z, y, x) or [n, 4] (b, z, y, x)): any entry outside the grid / batch drops the row
__global__ __launch_bounds__(256) void dv_keys_kernel(const int32_t* __restrict__ coors, int cols, int64_t n, int batch, int gx,
                                                     int gy, int gz, uint32_t* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t* c = coors + i * cols;
    const int b = cols == 4 ? c[0] : 0;
    const int z = c[cols - 3], y = c[cols - 2], x = c[cols - 1];
    const bool ok = b >= 0 && b < batch && z >= 0 && z < gz && y >= 0 && y < gy && x >= 0 && x < gx;
    keys[i] = ok ? (((uint32_t)b * (uint32_t)gz + (uint32_t)z) * (uint32_t)gy + (uint32_t)y) * (uint32_t)gx + (uint32_t)x : DV_DROPPED;
}

__global__ __launch_bounds__(256) void dv_heads_kernel(const uint32_t* __restrict__ sk, int64_t n, int32_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = sk[i];
    flags[i] = (k != DV_DROPPED && (i == 0 || sk[i - 1] != k)) ? 1 : 0;
}

__global__ __launch_bounds__(256) void dv_finalize_kernel(const uint32_t* __restrict__ sk, const int32_t* __restrict__ incl,
                                                         const int32_t* __restrict__ order, int64_t n, int gx, int gy, int gz,
                                                         int4* __restrict__ voxel_coors, int32_t* __restrict__ voxel_start,
                                                         int32_t* __restrict__ point2voxel, int32_t* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = sk[i];
    const int32_t p = order[i];
    if (k == DV_DROPPED) {
        point2voxel[p] = -1;
        if (i == 0) {          // every point dropped
            counts[0] = 0;
            counts[1] = 0;
        }
        return;
    }
    const int32_t v = incl[i] - 1;
    point2voxel[p] = v;
    if (i == 0 || sk[i - 1] != k) {
        voxel_start[v] = (int32_t)i;
        uint32_t r = k;
        const int cx = (int)(r % (uint32_t)gx); r /= (uint32_t)gx;
        const int cy = (int)(r % (uint32_t)gy); r /= (uint32_t)gy;
        const int cz = (int)(r % (uint32_t)gz); r /= (uint32_t)gz;
        voxel_coors[v] = make_int4((int)r, cz, cy, cx);
    }
    if (i == n - 1 || sk[i + 1] == DV_DROPPED) {      // last valid position
        counts[0] = v + 1;
        counts[1] = (int32_t)(i + 1);
        voxel_start[v + 1] = (int32_t)(i + 1);
    }
}

static size_t dv_scan_temp_bytes(int64_t n) {
    size_t tb = 0;
    (void)rocprim::inclusive_scan(nullptr, tb, (const int32_t*)nullptr, (int32_t*)nullptr, (size_t)n, rocprim::plus<int32_t>(),
                                  (hipStream_t)0);
    return gga_align_up(tb, 256);
}
static inline size_t dv_rows_bytes(int64_t n) { return gga_align_up((size_t)n * 4, 256); }

// number of key bits the sort has to look at: the bit length of the cell count (see the header comment)
static int dv_key_bits(uint64_t cells) {
    int bits = 1;
    while (bits < 32 && (cells >> bits) != 0) ++bits;
    return bits;
}

static int dv_cells(const char* who, int batch, int gx, int gy, int gz, uint64_t* cells) {
    GGA_REQUIRE(batch >= 1 && batch <= GGA_MAX_BATCH, "%s: batch %d not in [1, %d]", who, batch, GGA_MAX_BATCH);
    GGA_REQUIRE(gx > 0 && gy > 0 && gz > 0, "%s: empty grid", who);
    // (each factor < 2^31 and the running product is checked after every step: no overflow of the u64)
    uint64_t c = (uint64_t)batch * (uint64_t)gz;
    GGA_REQUIRE(c < 0xFFFFFFFFull, "%s: batch x grid does not fit the 32-bit voxel key", who);
    c *= (uint64_t)gy;
    GGA_REQUIRE(c < 0xFFFFFFFFull, "%s: batch x grid does not fit the 32-bit voxel key", who);
    c *= (uint64_t)gx;
    GGA_REQUIRE(c < 0xFFFFFFFFull, "%s: batch %d x grid %d x %d x %d = %llu cells does not fit the 32-bit voxel key", who, batch,
                gz, gy, gx, (unsigned long long)c);
    *cells = c;
    return GGA_OK;
}

extern "C" int gga_dynamic_voxelize(const float* points, int ndim, const int64_t* offsets_host, const int32_t* counts_dev,
                                    int batch, const gga_voxel_params* prm, int32_t* coors, uint32_t* keys, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GGA_REQUIRE(points && offsets_host && prm && coors && keys, "gga_dynamic_voxelize: null pointer argument");
    GGA_REQUIRE(batch >= 1 && batch <= GGA_MAX_BATCH, "gga_dynamic_voxelize: batch %d not in [1, %d]", batch, GGA_MAX_BATCH);
    GGA_REQUIRE(ndim >= 3 && ndim <= 16, "gga_dynamic_voxelize: ndim %d not in [3, 16]", ndim);
    GgaFrames fo;
    int max_n;
    if (int rc = gga_frames_from_host("gga_dynamic_voxelize", offsets_host, counts_dev, batch, &fo, &max_n)) return rc;
    const GgaVoxGeom g = gga_vox_geom(prm);
    uint64_t cells;
    if (int rc = dv_cells("gga_dynamic_voxelize", batch, g.grid[0], g.grid[1], g.grid[2], &cells)) return rc;
    if (max_n == 0) return GGA_OK;
    hipLaunchKernelGGL(dv_coors_kernel, dim3((max_n + 255) / 256, batch), dim3(256), 0, stream, points, ndim, fo, g,
                       reinterpret_cast<int4*>(coors), keys);
    GGA_CHECK_LAUNCH("dv_coors_kernel");
    return GGA_OK;
}

extern "C" size_t gga_dynamic_voxel_map_workspace_bytes(int64_t n_points) {
    if (n_points < 1) return 0;
    // sort temp | scan temp | keys (built from coors) | sorted keys | head flags | scanned flags
    return gga_argsort_temp_bytes<uint32_t>(n_points, 32) + dv_scan_temp_bytes(n_points) + 4 * dv_rows_bytes(n_points);
}

extern "C" int gga_dynamic_voxel_map(const uint32_t* keys, const int32_t* coors, int coor_cols, int64_t n_points, int batch,
                                     int grid_x, int grid_y, int grid_z, int32_t* voxel_coors, int32_t* voxel_start,
                                     int32_t* order, int32_t* point2voxel, int32_t* counts, void* workspace,
                                     size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GGA_REQUIRE((keys || coors) && voxel_coors && voxel_start && order && point2voxel && counts,
                "gga_dynamic_voxel_map: null pointer argument");
    GGA_REQUIRE(keys || coor_cols == 3 || coor_cols == 4, "gga_dynamic_voxel_map: coors must have 3 or 4 columns, got %d",
                coor_cols);
    GGA_REQUIRE(n_points >= 0 && n_points < (1ll << 30), "gga_dynamic_voxel_map: n_points %lld not in [0, 2^30)",
                (long long)n_points);
    uint64_t cells;
    const int rc = dv_cells("gga_dynamic_voxel_map", batch, grid_x, grid_y, grid_z, &cells);
    if (rc != GGA_OK) return rc;
    GGA_REQUIRE(keys || coor_cols == 4 || batch == 1, "gga_dynamic_voxel_map: 3-column coors are one sample (batch 1)");
    GGA_CHECK_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int32_t), stream), "dynamic map memset(counts)");
    GGA_CHECK_HIP(hipMemsetAsync(voxel_start, 0, ((size_t)n_points + 1) * sizeof(int32_t), stream), "dynamic map memset(start)");
    if (n_points == 0) return GGA_OK;
    GGA_REQUIRE(workspace, "gga_dynamic_voxel_map: null pointer argument");
    if (gga_dynamic_voxel_map_workspace_bytes(n_points) > workspace_bytes) {
        gga_set_error("gga_dynamic_voxel_map: workspace %zu B < required %zu B", workspace_bytes,
                      gga_dynamic_voxel_map_workspace_bytes(n_points));
        return GGA_ERR_WORKSPACE;
    }
    GGA_CHECK_HIP(hipMemsetAsync(voxel_coors, 0, (size_t)n_points * 4 * sizeof(int32_t), stream), "dynamic map memset(coors)");
    const int bits = dv_key_bits(cells);
    char* w = (char*)workspace;
    void* sort_tmp = w;      w += gga_argsort_temp_bytes<uint32_t>(n_points, 32);
    void* scan_tmp = w;      w += dv_scan_temp_bytes(n_points);
    uint32_t* own_keys = (uint32_t*)w; w += dv_rows_bytes(n_points);
    uint32_t* sk = (uint32_t*)w;       w += dv_rows_bytes(n_points);
    int32_t* flags = (int32_t*)w;      w += dv_rows_bytes(n_points);
    int32_t* incl = (int32_t*)w;
    const dim3 grid((unsigned)((n_points + 255) / 256));
    if (!keys) {
        hipLaunchKernelGGL(dv_keys_kernel, grid, dim3(256), 0, stream, coors, coor_cols, n_points, batch, grid_x, grid_y, grid_z,
                           own_keys);
        GGA_CHECK_LAUNCH("dv_keys_kernel");
        keys = own_keys;
    }
    if (int rc = gga_argsort("gga_dynamic_voxel_map", sort_tmp, keys, sk, order, n_points, bits, stream)) return rc;
    hipLaunchKernelGGL(dv_heads_kernel, grid, dim3(256), 0, stream, sk, n_points, flags);
    GGA_CHECK_LAUNCH("dv_heads_kernel");
    size_t tb = dv_scan_temp_bytes(n_points);
    const hipError_t e = rocprim::inclusive_scan(scan_tmp, tb, (const int32_t*)flags, incl, (size_t)n_points, rocprim::plus<int32_t>(), stream);
    if (e != hipSuccess) {
        gga_set_error("gga_dynamic_voxel_map: rocprim::inclusive_scan: %s", hipGetErrorString(e));
        return GGA_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(dv_finalize_kernel, grid, dim3(256), 0, stream, sk, incl, order, n_points, grid_x, grid_y, grid_z,
                       reinterpret_cast<int4*>(voxel_coors), voxel_start, point2voxel, counts);
    GGA_CHECK_LAUNCH("dv_finalize_kernel");
    return GGA_OK;
}

// ---- DynamicScatter -------------------------------------------------------------------------------------------------
// A partial result of one lane: running sum, or running max with the point that holds it.
struct DvAcc {
    float v;
    int32_t idx;
};
template <bool MAX>
__device__ __forceinline__ void dv_take(DvAcc& a, float x, int32_t p) {
    if (MAX) {
        if (a.idx == DV_NO_POINT || x > a.v) { a.v = x; a.idx = p; }      // strict >: the first (lowest) index keeps a tie
    } else {
        a.v += x;
    }
}
template <bool MAX>
__device__ __forceinline__ void dv_merge(DvAcc& a, float v, int32_t idx) {
    if (MAX) {
        if (idx != DV_NO_POINT && (a.idx == DV_NO_POINT || v > a.v || (v == a.v && idx < a.idx))) { a.v = v; a.idx = idx; }
    } else {
        a.v += v;
    }
}

// lanes per row: the power of two >= channels, at most the wave
static inline int dv_group(int channels) {
    int g = 1;
    while (g < channels && g < 64) g <<= 1;
    return g;
}

// One wave per tile of DV_CHUNK sorted positions: partials of the (at most two) long segments that meet the tile. A row is
// read by G lanes; the 64 / G lane groups take positions lo + r, lo + r + R, ... and are merged by a fixed shuffle tree.
template <bool MAX>
__global__ __launch_bounds__(256) void dv_tile_kernel(const float* __restrict__ feats, int C, int G, int64_t n, int64_t ntiles,
                                                     const int32_t* __restrict__ order, const int32_t* __restrict__ p2v,
                                                     const int32_t* __restrict__ voxel_start, const int32_t* __restrict__ counts,
                                                     float* __restrict__ part_v, int32_t* __restrict__ part_i) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= ntiles) return;
    int64_t nv = counts[1];
    nv = nv < 0 ? 0 : (nv < n ? nv : n);
    const int64_t t0 = t * DV_CHUNK;
    if (t0 >= nv) return;
    const int64_t t1 = (t0 + DV_CHUNK < nv) ? t0 + DV_CHUNK : nv;
    const int32_t va = p2v[order[t0]], vb = p2v[order[t1 - 1]];
    const int R = 64 / G, r = lane / G, c0 = lane % G;
    for (int slot = 0; slot < 2; ++slot) {
        const int32_t v = slot == 0 ? va : vb;
        if (v < 0 || (slot == 1 && vb == va)) continue;
        const int64_t s = voxel_start[v], e = voxel_start[v + 1];
        if (e - s <= DV_CHUNK) continue;                  // short segment: the voxel pass walks it
        const int64_t lo = s > t0 ? s : t0, hi = e < t1 ? e : t1;
        for (int c = c0; c < C; c += G) {
            DvAcc a = {0.0f, DV_NO_POINT};
            for (int64_t j = lo + r; j < hi; j += R) {
                const int32_t p = order[j];
                dv_take<MAX>(a, feats[(int64_t)p * C + c], p);
            }
            for (int o = G; o < 64; o <<= 1) {
                const float ov = __shfl_xor(a.v, o, 64);
                const int32_t oi = __shfl_xor(a.idx, o, 64);
                dv_merge<MAX>(a, ov, oi);
            }
            if (r == 0) {
                part_v[(t * 2 + slot) * C + c] = a.v;
                if (MAX) part_i[(t * 2 + slot) * C + c] = a.idx;
            }
        }
    }
}

// G lanes per voxel: a short segment is walked in order, a long one combines its tiles' partials in tile order.
template <bool MAX>
__global__ __launch_bounds__(256) void dv_voxel_kernel(const float* __restrict__ feats, int C, int G, int64_t rows,
                                                      const int32_t* __restrict__ order, const int32_t* __restrict__ voxel_start,
                                                      const int32_t* __restrict__ counts, const float* __restrict__ part_v,
                                                      const int32_t* __restrict__ part_i, float* __restrict__ out,
                                                      int32_t* __restrict__ argmax) {
    const int64_t gt = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t v = gt / G;
    const int c0 = (int)(gt % G);
    int64_t m = counts[0];
    m = m < rows ? m : rows;
    if (v >= m) return;
    const int64_t s = voxel_start[v], e = voxel_start[v + 1];
    const int64_t len = e - s;
    for (int c = c0; c < C; c += G) {
        DvAcc a = {0.0f, DV_NO_POINT};
        if (len <= DV_CHUNK) {
            for (int64_t j = s; j < e; ++j) {
                const int32_t p = order[j];
                dv_take<MAX>(a, feats[(int64_t)p * C + c], p);
            }
        } else {
            const int64_t ta = s / DV_CHUNK, tb = (e - 1) / DV_CHUNK;
            for (int64_t t = ta; t <= tb; ++t) {
                const int slot = (s <= t * DV_CHUNK) ? 0 : 1;
                const int64_t q = (t * 2 + slot) * C + c;
                dv_merge<MAX>(a, part_v[q], MAX ? part_i[q] : 0);
            }
        }
        if (MAX) {
            out[v * C + c] = a.v;
            argmax[v * C + c] = a.idx;
        } else {
            out[v * C + c] = __fdiv_rn(a.v, (float)len);
        }
    }
}

template <bool MAX>
__global__ __launch_bounds__(256) void dv_scatter_bwd_kernel(const float* __restrict__ gout, int C, int64_t n, int64_t rows,
                                                            const int32_t* __restrict__ p2v, const int32_t* __restrict__ voxel_start,
                                                            const int32_t* __restrict__ argmax, float* __restrict__ gin) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n * C) return;
    const int64_t i = t / C;
    const int c = (int)(t - i * C);
    const int32_t v = p2v[i];
    float g = 0.0f;
    if (v >= 0 && v < rows) {
        if (MAX) {
            g = argmax[(int64_t)v * C + c] == (int32_t)i ? gout[(int64_t)v * C + c] : 0.0f;
        } else {
            g = __fdiv_rn(gout[(int64_t)v * C + c], (float)(voxel_start[v + 1] - voxel_start[v]));
        }
    }
    gin[t] = g;
}

static inline int64_t dv_tiles(int64_t n) { return (n + DV_CHUNK - 1) / DV_CHUNK; }

extern "C" int gga_dynamic_scatter_chunk(void) { return DV_CHUNK; }

extern "C" size_t gga_dynamic_scatter_workspace_bytes(int64_t n_points, int channels) {
    if (n_points < 1 || channels < 1) return 0;
    return 2 * gga_align_up((size_t)dv_tiles(n_points) * 2 * (size_t)channels * 4, 256);
}

extern "C" int gga_dynamic_scatter_fwd(const float* feats, int channels, int64_t n_points, const int32_t* order,
                                       const int32_t* point2voxel, const int32_t* voxel_start, const int32_t* counts,
                                       int64_t out_rows, int mode, float* out, int32_t* argmax, void* workspace,
                                       size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GGA_REQUIRE(mode == GGA_DYNAMIC_MEAN || mode == GGA_DYNAMIC_MAX, "gga_dynamic_scatter_fwd: mode %d is neither mean nor max", mode);
    GGA_REQUIRE(channels >= 1 && channels <= 128, "gga_dynamic_scatter_fwd: channels %d not in [1, 128]", channels);
    GGA_REQUIRE(n_points >= 0 && n_points < (1ll << 30) && out_rows >= 0 && out_rows <= n_points,
                "gga_dynamic_scatter_fwd: bad sizes (n_points=%lld out_rows=%lld)", (long long)n_points, (long long)out_rows);
    if (n_points == 0 || out_rows == 0) return GGA_OK;
    GGA_REQUIRE(feats && order && point2voxel && voxel_start && counts && out && workspace && (mode == GGA_DYNAMIC_MEAN || argmax),
                "gga_dynamic_scatter_fwd: null pointer argument");
    if (gga_dynamic_scatter_workspace_bytes(n_points, channels) > workspace_bytes) {
        gga_set_error("gga_dynamic_scatter_fwd: workspace %zu B < required %zu B", workspace_bytes,
                      gga_dynamic_scatter_workspace_bytes(n_points, channels));
        return GGA_ERR_WORKSPACE;
    }
    const int G = dv_group(channels);
    const int64_t ntiles = dv_tiles(n_points);
    float* part_v = (float*)workspace;
    int32_t* part_i = (int32_t*)((char*)workspace + gga_align_up((size_t)ntiles * 2 * (size_t)channels * 4, 256));
    const dim3 tgrid((unsigned)((ntiles + 3) / 4)), vgrid((unsigned)((out_rows * G + 255) / 256));
    if (mode == GGA_DYNAMIC_MAX) {
        hipLaunchKernelGGL(dv_tile_kernel<true>, tgrid, dim3(256), 0, stream, feats, channels, G, n_points, ntiles, order,
                           point2voxel, voxel_start, counts, part_v, part_i);
        GGA_CHECK_LAUNCH("dv_tile_kernel");
        hipLaunchKernelGGL(dv_voxel_kernel<true>, vgrid, dim3(256), 0, stream, feats, channels, G, out_rows, order, voxel_start,
                           counts, part_v, part_i, out, argmax);
    } else {
        hipLaunchKernelGGL(dv_tile_kernel<false>, tgrid, dim3(256), 0, stream, feats, channels, G, n_points, ntiles, order,
                           point2voxel, voxel_start, counts, part_v, part_i);
        GGA_CHECK_LAUNCH("dv_tile_kernel");
        hipLaunchKernelGGL(dv_voxel_kernel<false>, vgrid, dim3(256), 0, stream, feats, channels, G, out_rows, order, voxel_start,
                           counts, part_v, part_i, out, argmax);
    }
    GGA_CHECK_LAUNCH("dv_voxel_kernel");
    return GGA_OK;
}

extern "C" int gga_dynamic_scatter_bwd(const float* grad_out, int channels, int64_t n_points, const int32_t* point2voxel,
                                       const int32_t* voxel_start, const int32_t* argmax, int64_t out_rows, int mode,
                                       float* grad_in, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GGA_REQUIRE(mode == GGA_DYNAMIC_MEAN || mode == GGA_DYNAMIC_MAX, "gga_dynamic_scatter_bwd: mode %d is neither mean nor max", mode);
    GGA_REQUIRE(channels >= 1 && channels <= 128, "gga_dynamic_scatter_bwd: channels %d not in [1, 128]", channels);
    GGA_REQUIRE(n_points >= 0 && n_points < (1ll << 30) && out_rows >= 0 && out_rows <= n_points,
                "gga_dynamic_scatter_bwd: bad sizes (n_points=%lld out_rows=%lld)", (long long)n_points, (long long)out_rows);
    if (n_points == 0) return GGA_OK;
    GGA_REQUIRE(point2voxel && voxel_start && grad_in && (out_rows == 0 || grad_out) &&
                    (mode == GGA_DYNAMIC_MEAN || out_rows == 0 || argmax),
                "gga_dynamic_scatter_bwd: null pointer argument");
    const int64_t total = n_points * channels;
    if (mode == GGA_DYNAMIC_MAX)
        hipLaunchKernelGGL(dv_scatter_bwd_kernel<true>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, grad_out,
                           channels, n_points, out_rows, point2voxel, voxel_start, argmax, grad_in);
    else
        hipLaunchKernelGGL(dv_scatter_bwd_kernel<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, grad_out,
                           channels, n_points, out_rows, point2voxel, voxel_start, argmax, grad_in);
    GGA_CHECK_LAUNCH("dv_scatter_bwd_kernel");
    return GGA_OK;
}

// ---- fused DynamicPillarFeatureNet ----------------------------------------------------------------------------------
// The shipped form only: one layer, 4 point features -> 64 channels, mode = 'max', cluster and voxel centre, no distance,
// affine BatchNorm1d with running statistics, fp32 (pillar_encoder.py:276-323). The structure of pfn.hip without the padding;
// constants, the layout of `saved`, the voxel centre, the weight load, the count clamps and the two block-reduction tails
// are pfn_common.h's, and the statistics and backward-close kernels are pfn.hip's own (one definition for both fronts):
//
//   pass 0  per-voxel mean of the points: the mean scatter above on the 4 point features (x, y, z used).
//   pass 1  dpfn_moments_kernel  first (10) and second (55) moments of the decorated features over the kept points, f64, in a
//                                fixed order (grid-stride over the sorted positions, shuffle tree, block partials).
//           pfn_launch_stats     z = W f is linear, so the BatchNorm batch statistics over the R = kept points follow from
//                                the moments; scale / shift per channel; running statistics updated unless R = 0.
//   pass 2  dpfn_tile_kernel     long segments (more than DV_CHUNK points): one wave per tile of sorted positions, lane =
//                                channel, partial max + arg-max of the (at most two) long segments that meet the tile.
//           dpfn_voxel_kernel    one wave per voxel, lane = channel, the 10 weights in registers: relu(z scale + shift),
//                                running max with its arg-max point (i32; strict >, so the lowest point index keeps a tie),
//                                or the tile partials combined in tile order; one 256 B store per voxel.
//   backward dpfn_bwd_kernel     per channel A = sum g, Bx = sum g xhat, G[10] = sum g f(arg-max point);
//           pfn_launch_bwd_final closes the BatchNorm backward analytically from the moments.
// Decoration: (x, y, z, r, x-mx, y-my, z-mz, x-cx, y-cy, z-cz) - no legacy in-place quirk in the dynamic class.
// counts = {voxels, kept points} of the map on the device: pfn_clamped(counts, rows) voxels, pfn_clamped(counts + 1, n) points.
__device__ __forceinline__ void dpfn_decorate(const float4 p, const int4 co, const float4 mu, const PfnGeom g, float f[PFN_F]) {
    float cen[3];
    pfn_centre(co, g, cen);
    f[0] = p.x; f[1] = p.y; f[2] = p.z; f[3] = p.w;
    f[4] = p.x - mu.x; f[5] = p.y - mu.y; f[6] = p.z - mu.z;
    f[7] = p.x - cen[0]; f[8] = p.y - cen[1]; f[9] = p.z - cen[2];
}

__device__ __forceinline__ float dpfn_z(const float f[PFN_F], const float w[PFN_F]) {
    float z = 0.0f;
#pragma unroll
    for (int a = 0; a < PFN_F; ++a) z = fmaf(f[a], w[a], z);       // explicit: the same bits wherever a point is evaluated
    return z;
}

__global__ __launch_bounds__(256) void dpfn_moments_kernel(const float4* __restrict__ points, const int4* __restrict__ coors,
                                                          int64_t n, int64_t rows, const int32_t* __restrict__ order,
                                                          const int32_t* __restrict__ p2v, const int32_t* __restrict__ counts,
                                                          const float4* __restrict__ mean, PfnGeom g,
                                                          double* __restrict__ partials) {
    const int64_t nv = pfn_clamped(counts + 1, n);
    double acc[PFN_NM];
#pragma unroll
    for (int i = 0; i < PFN_NM; ++i) acc[i] = 0.0;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < nv; j += (int64_t)gridDim.x * 256) {
        const int32_t p = order[j];
        const int32_t v = p2v[p];
        if (v < 0 || v >= rows) continue;
        float f[PFN_F];
        dpfn_decorate(points[p], coors[p], mean[v], g, f);
        int k = PFN_F;
#pragma unroll
        for (int a = 0; a < PFN_F; ++a) {
            acc[a] += (double)f[a];
#pragma unroll
            for (int b = a; b < PFN_F; ++b) acc[k++] += (double)f[a] * (double)f[b];
        }
    }
    pfn_moments_commit(acc, partials);
}

// running max of relu(z scale + shift) over the sorted positions [lo, hi) of voxel v; lane = channel
__device__ __forceinline__ void dpfn_walk(const float4* __restrict__ points, const int4* __restrict__ coors,
                                          const int32_t* __restrict__ order, int64_t lo, int64_t hi, const float4 mu,
                                          const PfnGeom g, const float w[PFN_F], float sc, float sh, DvAcc& a) {
    for (int64_t j = lo; j < hi; ++j) {
        const int32_t p = order[j];                      // wave-uniform
        float f[PFN_F];
        dpfn_decorate(points[p], coors[p], mu, g, f);
        const float y = fmaxf(fmaf(dpfn_z(f, w), sc, sh), 0.0f);
        dv_take<true>(a, y, p);
    }
}

__global__ __launch_bounds__(256) void dpfn_tile_kernel(const float4* __restrict__ points, const int4* __restrict__ coors,
                                                       int64_t n, int64_t rows, int64_t ntiles, const int32_t* __restrict__ order,
                                                       const int32_t* __restrict__ p2v, const int32_t* __restrict__ voxel_start,
                                                       const int32_t* __restrict__ counts, const float4* __restrict__ mean,
                                                       PfnGeom g, const float* __restrict__ weight,
                                                       const float* __restrict__ scale_shift, float* __restrict__ part_v,
                                                       int32_t* __restrict__ part_i) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= ntiles) return;
    const int64_t nv = pfn_clamped(counts + 1, n);
    const int64_t t0 = t * DV_CHUNK;
    if (t0 >= nv) return;
    const int64_t t1 = (t0 + DV_CHUNK < nv) ? t0 + DV_CHUNK : nv;
    const int32_t va = p2v[order[t0]], vb = p2v[order[t1 - 1]];
    float w[PFN_F];
    pfn_load_weights(weight, lane, w);
    const float sc = scale_shift[lane], sh = scale_shift[PFN_C + lane];
    for (int slot = 0; slot < 2; ++slot) {
        const int32_t v = slot == 0 ? va : vb;
        if (v < 0 || v >= rows || (slot == 1 && vb == va)) continue;
        const int64_t s = voxel_start[v], e = voxel_start[v + 1];
        if (e - s <= DV_CHUNK) continue;
        DvAcc a = {0.0f, DV_NO_POINT};
        dpfn_walk(points, coors, order, s > t0 ? s : t0, e < t1 ? e : t1, mean[v], g, w, sc, sh, a);
        part_v[(t * 2 + slot) * PFN_C + lane] = a.v;
        part_i[(t * 2 + slot) * PFN_C + lane] = a.idx;
    }
}

__global__ __launch_bounds__(256) void dpfn_voxel_kernel(const float4* __restrict__ points, const int4* __restrict__ coors,
                                                        int64_t rows, const int32_t* __restrict__ order,
                                                        const int32_t* __restrict__ voxel_start, const int32_t* __restrict__ counts,
                                                        const float4* __restrict__ mean, PfnGeom g,
                                                        const float* __restrict__ weight, const float* __restrict__ scale_shift,
                                                        const float* __restrict__ part_v, const int32_t* __restrict__ part_i,
                                                        float* __restrict__ out, int32_t* __restrict__ argmax) {
    const int lane = threadIdx.x & 63;
    const int64_t m = pfn_clamped(counts, rows);
    float w[PFN_F];
    pfn_load_weights(weight, lane, w);
    const float sc = scale_shift[lane], sh = scale_shift[PFN_C + lane];
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t v = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); v < m; v += nwaves) {
        const int64_t s = voxel_start[v], e = voxel_start[v + 1];
        DvAcc a = {0.0f, DV_NO_POINT};
        if (e - s <= DV_CHUNK) {
            dpfn_walk(points, coors, order, s, e, mean[v], g, w, sc, sh, a);
        } else {
            const int64_t ta = s / DV_CHUNK, tb = (e - 1) / DV_CHUNK;
            for (int64_t t = ta; t <= tb; ++t) {
                const int64_t q = (t * 2 + ((s <= t * DV_CHUNK) ? 0 : 1)) * PFN_C + lane;
                dv_merge<true>(a, part_v[q], part_i[q]);
            }
        }
        out[v * PFN_C + lane] = a.v;
        argmax[v * PFN_C + lane] = a.idx;
    }
}

__global__ __launch_bounds__(256) void dpfn_bwd_kernel(const float4* __restrict__ points, const int4* __restrict__ coors, int64_t n,
                                                      int64_t rows, const int32_t* __restrict__ counts,
                                                      const float4* __restrict__ mean, PfnGeom g, const float* __restrict__ weight,
                                                      const double* __restrict__ saved, const float* __restrict__ out,
                                                      const int32_t* __restrict__ argmax, const float* __restrict__ grad_out,
                                                      float* __restrict__ partials) {
    const int lane = threadIdx.x & 63;
    float w[PFN_F];
    pfn_load_weights(weight, lane, w);
    const float mean_c = (float)saved[PFN_SAVED_MEAN + lane], invstd_c = (float)saved[PFN_SAVED_INVSTD + lane];
    float acc[PFN_BW];
#pragma unroll
    for (int i = 0; i < PFN_BW; ++i) acc[i] = 0.0f;
    const int64_t m = pfn_clamped(counts, rows);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t v = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); v < m; v += nwaves) {
        const float y = out[v * PFN_C + lane];
        const float gy = y > 0.0f ? grad_out[v * PFN_C + lane] : 0.0f;    // ReLU gate
        const int32_t bi = argmax[v * PFN_C + lane];
        if (bi < 0 || bi >= n) continue;                                     // (never: every voxel has a point)
        float f[PFN_F];
        dpfn_decorate(points[bi], coors[bi], mean[v], g, f);
        const float xhat = (dpfn_z(f, w) - mean_c) * invstd_c;
        acc[0] += gy;
        acc[1] += gy * xhat;
#pragma unroll
        for (int a = 0; a < PFN_F; ++a) acc[2 + a] += gy * f[a];
    }
    pfn_bwd_commit(acc, partials);
}

// workspace: mean scatter | block partials (moments f64 / backward f32) | tile partials (value, point) | scale, shift
static size_t dpfn_ws_scatter(int64_t n) { return gga_align_up(gga_dynamic_scatter_workspace_bytes(n, 4), 256); }
static size_t dpfn_ws_partials(int64_t n) {
    const size_t a = (size_t)pfn_blocks(n) * PFN_NM * sizeof(double);
    const size_t b = (size_t)pfn_wave_blocks(n) * PFN_BW * PFN_C * sizeof(float);
    return gga_align_up(a > b ? a : b, 256);
}
static size_t dpfn_ws_tiles(int64_t n) { return gga_align_up((size_t)dv_tiles(n) * 2 * PFN_C * 4, 256); }

extern "C" size_t gga_dynamic_pfn_workspace_bytes(int64_t n_points) {
    if (n_points < 1) return 0;
    return dpfn_ws_scatter(n_points) + dpfn_ws_partials(n_points) + 2 * dpfn_ws_tiles(n_points) + 2 * PFN_C * sizeof(float);
}

static int dpfn_check(const char* fn, const gga_pfn_params* prm, int64_t n, int64_t rows) {
    if (int rc = pfn_check_params(fn, prm)) return rc;
    GGA_REQUIRE(n >= 1 && n < (1ll << 30) && rows >= 1 && rows <= n, "%s: bad sizes (n_points=%lld out_rows=%lld)", fn,
                (long long)n, (long long)rows);
    return GGA_OK;
}

extern "C" int gga_dynamic_pfn_fwd(const float* points, const int32_t* coors, int64_t n_points, const int32_t* order,
                                   const int32_t* point2voxel, const int32_t* voxel_start, const int32_t* counts,
                                   int64_t out_rows, const gga_pfn_params* prm, const float* weight, const float* gamma,
                                   const float* beta, float* running_mean, float* running_var, float* out, int32_t* argmax,
                                   float* mean, double* saved, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = dpfn_check("gga_dynamic_pfn_fwd", prm, n_points, out_rows)) return rc;
    GGA_REQUIRE(points && coors && order && point2voxel && voxel_start && counts && weight && gamma && beta && running_mean &&
                    running_var && out && argmax && mean && saved && workspace,
                "gga_dynamic_pfn_fwd: null pointer argument");
    GGA_REQUIRE_WORKSPACE("gga_dynamic_pfn_fwd", workspace_bytes, gga_dynamic_pfn_workspace_bytes(n_points));
    const PfnGeom g = pfn_geom(prm);
    char* w = (char*)workspace;
    void* ws_scatter = w;               w += dpfn_ws_scatter(n_points);
    double* partials = (double*)w;      w += dpfn_ws_partials(n_points);
    float* part_v = (float*)w;          w += dpfn_ws_tiles(n_points);
    int32_t* part_i = (int32_t*)w;      w += dpfn_ws_tiles(n_points);
    float* scale_shift = (float*)w;
    if (int rc = gga_dynamic_scatter_fwd(points, 4, n_points, order, point2voxel, voxel_start, counts, out_rows, GGA_DYNAMIC_MEAN,
                                         mean, nullptr, ws_scatter, dpfn_ws_scatter(n_points), stream_))
        return rc;
    const int nb = pfn_blocks(n_points);
    if (prm->training) {
        hipLaunchKernelGGL(dpfn_moments_kernel, dim3(nb), dim3(256), 0, stream, (const float4*)points, (const int4*)coors, n_points,
                           out_rows, order, point2voxel, counts, (const float4*)mean, g, partials);
        GGA_CHECK_LAUNCH("dpfn_moments_kernel");
    }
    if (int rc = pfn_launch_stats(partials, nb, counts + 1, n_points, 1, 0, weight, gamma, beta, prm, running_mean, running_var, saved,
                                  scale_shift, stream))
        return rc;
    const int64_t ntiles = dv_tiles(n_points);
    hipLaunchKernelGGL(dpfn_tile_kernel, dim3((unsigned)((ntiles + 3) / 4)), dim3(256), 0, stream, (const float4*)points,
                       (const int4*)coors, n_points, out_rows, ntiles, order, point2voxel, voxel_start, counts, (const float4*)mean, g,
                       weight, scale_shift, part_v, part_i);
    GGA_CHECK_LAUNCH("dpfn_tile_kernel");
    hipLaunchKernelGGL(dpfn_voxel_kernel, dim3(pfn_wave_blocks(out_rows)), dim3(256), 0, stream, (const float4*)points,
                       (const int4*)coors, out_rows, order, voxel_start, counts, (const float4*)mean, g, weight, scale_shift, part_v,
                       part_i, out, argmax);
    GGA_CHECK_LAUNCH("dpfn_voxel_kernel");
    return GGA_OK;
}

extern "C" int gga_dynamic_pfn_bwd(const float* points, const int32_t* coors, int64_t n_points, const int32_t* counts,
                                   int64_t out_rows, const gga_pfn_params* prm, const float* weight, const float* gamma,
                                   const float* out, const int32_t* argmax, const float* mean, const double* saved,
                                   const float* grad_out, float* grad_weight, float* grad_gamma, float* grad_beta,
                                   void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = dpfn_check("gga_dynamic_pfn_bwd", prm, n_points, out_rows)) return rc;
    GGA_REQUIRE(points && coors && counts && weight && gamma && out && argmax && mean && saved && grad_out && grad_weight &&
                    grad_gamma && grad_beta && workspace,
                "gga_dynamic_pfn_bwd: null pointer argument");
    GGA_REQUIRE(prm->training, "gga_dynamic_pfn_bwd: backward is defined for training-mode batch statistics");
    GGA_REQUIRE_WORKSPACE("gga_dynamic_pfn_bwd", workspace_bytes, gga_dynamic_pfn_workspace_bytes(n_points));
    const PfnGeom g = pfn_geom(prm);
    float* partials = (float*)((char*)workspace + dpfn_ws_scatter(n_points));
    const int nb = pfn_wave_blocks(out_rows);
    hipLaunchKernelGGL(dpfn_bwd_kernel, dim3(nb), dim3(256), 0, stream, (const float4*)points, (const int4*)coors, n_points, out_rows,
                       counts, (const float4*)mean, g, weight, saved, out, argmax, grad_out, partials);
    GGA_CHECK_LAUNCH("dpfn_bwd_kernel");
    return pfn_launch_bwd_final(partials, nb, weight, gamma, saved, grad_weight, grad_gamma, grad_beta, stream);
}
