/*
 * gga_hip.h — C ABI of libgga_hip.so: the MI355X (gfx950) kernels of the GGA
 * training hot path.
 *
 * Boundary rules
 *   - plain C: device pointers, sizes, POD structs. No torch / ATen types.
 *   - every pointer is a DEVICE pointer unless its name ends in `_host`.
 *   - `stream` is a hipStream_t passed as void*. Every entry point only
 *     ENQUEUES work on it: no allocation, no synchronisation, no host read-back,
 *     so a caller may capture any sequence of calls into a hipGraph.
 *   - memory is owned by the caller (the PyTorch caching allocator in gga_amd/);
 *     scratch is passed in as `workspace` and sized by the *_workspace_bytes()
 *     helper next to each entry point.
 *   - return 0 on success, a negative gga_status otherwise; gga_last_error()
 *     returns a thread-local message for the last failure.
 *   - no global mutable state, re-entrant across processes (one rank per GPU).
 *
 * What each entry point replaces in the reference (paths under /root/reference,
 * a pure-Python mmdet3d fork whose native ops come from the un-vendored
 * mmcv-full / mmdet wheels — see SURVEY.md §2.2): cited per function below.
 * INTEGRATION.md shows the ctypes binding a reference maintainer would add.
 */
#ifndef GGA_HIP_H_
#define GGA_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    GGA_OK = 0,
    GGA_ERR_INVALID_ARG = -1,   /* null pointer, bad size, unsupported shape */
    GGA_ERR_WORKSPACE = -2,     /* workspace too small */
    GGA_ERR_LAUNCH = -3         /* hipGetLastError() != hipSuccess after a launch */
} gga_status;

const char* gga_last_error(void);
/* ABI version of this header; bumped on any signature change. */
int gga_abi_version(void);

/* Measurement only (bench.py's `roofline` objects): kernel timing sessions. After
 * gga_timing_begin(site, n, key) the next n calls of that site's entry point bracket their
 * launches with a pair of HIP events on the caller's stream (no synchronisation, so the step
 * being timed is not disturbed); gga_timing_collect waits for those events and writes the
 * durations in milliseconds, returning how many were taken (negative status on error) and
 * disarming the site. `key` = 0 times every call; otherwise only calls whose shape key matches
 * (see the site list). Thread-safe; one session per site at a time. */
enum {
    GGA_TIME_SCATTER_FWD = 0,   /* gga_pillar_scatter_fwd: NHWC fill [+ map] + rows, NCHW canvas kernel */
    GGA_TIME_DENSE_CONV = 1,    /* gga_dense_conv3x3_bn_bwd: key = GGA_TIMING_CONV_KEY(cin, cout, H*W) */
    GGA_TIME_SPARSE_CONV = 2,   /* gga_sparse_conv_apply_bn_bwd: key = GGA_TIMING_CONV_KEY(cin, cout, 0); gga_sparse_conv_apply_halo: (cin, cout, kvol) */
    GGA_TIME_SPARSE_WGRAD = 3,  /* gga_sparse_conv_wgrad_planes: key = GGA_TIMING_CONV_KEY(cin, cout, 0) */
    GGA_TIME_DENSE_WGRAD = 4,   /* gga_dense_wgrad3x3_block_amax: key as GGA_TIME_DENSE_CONV */
    GGA_TIME_SITES = 5
};
#define GGA_TIMING_CONV_KEY(cin, cout, hw) \
    (((int64_t)(cin) << 48) | ((int64_t)(cout) << 32) | ((int64_t)(hw) & 0xffffffffll))
int gga_timing_begin(int site, int max_samples, int64_t key);
int gga_timing_collect(int site, float* ms_host, int cap);

/* ------------------------------------------------------------------------- */
/* a1. Hard voxelization, whole batch in one call.                            */
/* Replaces: mmcv.ops.Voxelization(deterministic=True) called once per frame  */
/* in a Python loop + torch.cat + F.pad —                                     */
/*   mmdet3d/models/detectors/mvx_two_stage_gga.py:211-236 (voxelize),        */
/*   semantics restated in mmdet3d/core/voxel/voxel_generator.py:137-208.     */
/* First-come semantics, bit-exact: voxel id = order of first point, slot =   */
/* order of the point inside its voxel, voxels beyond max_voxels and points   */
/* beyond max_points dropped.                                                 */
/* ------------------------------------------------------------------------- */
typedef struct {
    float voxel_size[3];     /* x, y, z */
    float pc_range[6];       /* xmin, ymin, zmin, xmax, ymax, zmax */
    int32_t max_points;      /* per voxel */
    int32_t max_voxels;      /* per frame */
} gga_voxel_params;

/* grid = round((max - min) / voxel_size) in f32, as mmcv / the numpy voxelizer do. */
void gga_voxel_grid_size(const gga_voxel_params* prm, int32_t grid_xyz[3]);

size_t gga_hard_voxelize_workspace_bytes(int batch, int64_t total_points);

/*
 * points         [total_points, ndim] f32, frames concatenated
 * offsets_host   [batch + 1] i64 row offsets of each frame in `points`
 * counts_dev     null, or [batch] i32 on the device: frame b's points are the first min(counts_dev[b], capacity) rows of
 *                its range (frames at capacity offsets with their real counts on the device, the output of
 *                gga_points_prepare_batch): no host synchronisation
 * voxels         [batch * max_voxels, max_points, ndim] f32  (zero-filled here)
 * coors          [batch * max_voxels, 4] i32  (b, z, y, x)
 * num_points     [batch * max_voxels] i32
 * voxel_num      [batch + 1] i32: voxels per frame, [batch] = total M.
 * Frames are compacted: frame b occupies rows [sum_{b'<b} M_b', +M_b); rows >= M
 * are left zero.
 */
int gga_hard_voxelize_batch(const float* points, int ndim, const int64_t* offsets_host, const int32_t* counts_dev,
                            int batch, const gga_voxel_params* prm, float* voxels, int32_t* coors,
                            int32_t* num_points, int32_t* voxel_num, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- */
/* a0. Point-level tail of the train data pipeline,    */
/*     batched over frames, between loading and voxelization.                  */
/* ------------------------------------------------------------------------- */
/* Per frame, over the row list [pasted objects' points, scene points]:
 *  - ObjectSample_GGA.remove_points_in_boxes_v2 (mmdet3d/datasets/pipelines/gga_processing.py:
 *    58-68): scene rows whose BEV distance (f64, sqrt(dx*dx + dy*dy) like scipy cdist) to any
 *    pasted object's centre is < min_distance are dropped;
 *  - points.cat([sampled_points, points]) (gga_processing.py:176);
 *  - PointsRangeFilter / BasePoints.in_range_3d (transforms_3d.py:942-977,
 *    core/points/base_points.py:203-225): strict f32 inequalities against pc_range_dev[6];
 *  - PointShuffle (transforms_3d.py:858-883): rows permuted by a bijection seeded with
 *    shuffle_seeds_host[f] (0 = keep the order; the reference draws torch.randperm).
 * Kept rows are compacted in order (stable). scene / sampled: [rows, ndim] f32 with host row
 * offsets [n_frames+1] (sampled*, center* may be NULL = nothing pasted); centers_xy [n,2] f64.
 * Output: frame f's rows start at capacity offset (pasted + scene rows of the frames before it)
 * in out_points; out_counts[f] (device i32) = kept rows. */
size_t gga_points_prepare_workspace_bytes(int n_frames, int64_t total_rows, int64_t max_frame_rows);
int gga_points_prepare_batch(const float* scene, const int64_t* scene_offsets_host, const float* sampled,
                             const int64_t* sampled_offsets_host, const double* centers_xy,
                             const int64_t* center_offsets_host, int n_frames, int ndim, double min_distance,
                             const float* pc_range_dev, const uint64_t* shuffle_seeds_host, float* out_points,
                             int32_t* out_counts, void* workspace, size_t workspace_bytes, void* stream);

/* a2. HardSimpleVFE: mean of the valid points of each voxel.
 * Replaces mmdet3d/models/voxel_encoders/voxel_encoder.py:43-45.
 * out [m, num_features] = sum_p voxels[m, p, :num_features] / num_points[m]. */
int gga_voxel_mean(const float* voxels, const int32_t* num_points, int64_t m, int max_points,
                   int ndim, int num_features, float* out, void* stream);

/* ------------------------------------------------------------------------- */
/* a1d. Dynamic voxelization: every point keeps its cell, no cap on points per  */
/* voxel or voxels per frame. Replaces mmcv.ops.Voxelization(max_num_points=-1, */
/* max_voxels=-1) (mmdet3d/models/detectors/dynamic_voxelnet.py:52-72: per-frame */
/* loop + F.pad + cat) and mmcv.ops.DynamicScatter (voxel_encoders/             */
/* voxel_encoder.py:64,155-174, pillar_encoder.py:231-234).                      */
/* ------------------------------------------------------------------------- */
/*
 * points [total, ndim] f32, frames at offsets_host [batch + 1]; counts_dev: optional device i32 [batch] point counts of
 * frames stored at capacity offsets (NULL = every row is a point).
 * coors [total, 4] i32 (b, z, y, x): the cell of the hard voxelizer (same device function); (b, -1, -1, -1) for a point
 * outside the grid, at or past its frame's count, or with a non-finite coordinate.
 * keys [total] u32: ((b Z + z) Y + y) X + x, 0xFFFFFFFF for such a dropped point. batch x grid must stay below 2^32 - 1.
 */
int gga_dynamic_voxelize(const float* points, int ndim, const int64_t* offsets_host, const int32_t* counts_dev, int batch,
                         const gga_voxel_params* prm, int32_t* coors, uint32_t* keys, void* stream);

/*
 * Sorted point-to-voxel map of n_points keys (or, keys == NULL, of coors [n_points, coor_cols] with 3 (z, y, x) or
 * 4 (b, z, y, x) columns; a row with an entry outside the batch / grid is dropped). Capacity of every output is n_points:
 * voxel_coors [n_points, 4] ascending (b, z, y, x) (rows >= M zero), voxel_start [n_points + 1] (segment v of `order` is
 * [voxel_start[v], voxel_start[v + 1])), order [n_points] point indices grouped by voxel, ascending inside a voxel, dropped
 * points last; point2voxel [n_points] (-1 = dropped); counts [2] = (voxels M, points kept). No host read-back.
 */
size_t gga_dynamic_voxel_map_workspace_bytes(int64_t n_points);
int gga_dynamic_voxel_map(const uint32_t* keys, const int32_t* coors, int coor_cols, int64_t n_points, int batch, int grid_x,
                          int grid_y, int grid_z, int32_t* voxel_coors, int32_t* voxel_start, int32_t* order,
                          int32_t* point2voxel, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);

/*
 * DynamicScatter over such a map: out [out_rows, channels] = mean or max of feats [n_points, channels] over each voxel's
 * points, channels in [1, 128]. Only voxels < min(counts[0], out_rows) are written. No float atomics: the order of the
 * additions is fixed, two calls give the same bits. A voxel of more than gga_dynamic_scatter_chunk() points is reduced tile
 * by tile and its partials are combined in tile order. Max also writes argmax [out_rows, channels] i32, the point holding
 * the maximum (the lowest index on ties). Backward: grad_in [n_points, channels] = grad_out[voxel] / n (mean) or grad_out
 * at the arg-max point (max); dropped points get zero; every element of grad_in is written.
 */
enum { GGA_DYNAMIC_MEAN = 0, GGA_DYNAMIC_MAX = 1 };
int gga_dynamic_scatter_chunk(void);
size_t gga_dynamic_scatter_workspace_bytes(int64_t n_points, int channels);
int gga_dynamic_scatter_fwd(const float* feats, int channels, int64_t n_points, const int32_t* order,
                            const int32_t* point2voxel, const int32_t* voxel_start, const int32_t* counts, int64_t out_rows,
                            int mode, float* out, int32_t* argmax, void* workspace, size_t workspace_bytes, void* stream);
int gga_dynamic_scatter_bwd(const float* grad_out, int channels, int64_t n_points, const int32_t* point2voxel,
                            const int32_t* voxel_start, const int32_t* argmax, int64_t out_rows, int mode, float* grad_in,
                            void* stream);

/* ------------------------------------------------------------------------- */
/* a2'. Fused PillarFeatureNet (one PFNLayer, legacy=True, mode='max'):       */
/* decorate (cluster-mean / pillar-centre offsets) + Linear(10->64, no bias)  */
/* + BatchNorm1d (batch statistics over all m*P rows, padding included) +     */
/* ReLU + max over the P points, and its backward w.r.t. the parameters.      */
/* Replaces mmdet3d/models/voxel_encoders/pillar_encoder.py:93-159 and        */
/* voxel_encoders/utils.py:145-182 (PFNLayer.forward).                        */
/* ------------------------------------------------------------------------- */
typedef struct {
    float voxel_size[3];   /* vx, vy, vz */
    float offsets[3];      /* x_offset = vx/2 + pc_range[0], ... (pillar_encoder.py:87-90) */
    float eps, momentum;   /* BatchNorm1d(eps=1e-3, momentum=0.01) */
    int32_t training;      /* 1: batch statistics + running-stat update, 0: running statistics */
    int32_t in_features;   /* point features (x, y, z, r) = 4 */
    int32_t channels;      /* output channels = 64 */
} gga_pfn_params;

size_t gga_pfn_workspace_bytes(int64_t m);
/*
 * voxels [m,P,4] f32, num_points [m] i32, coors [m,4] i32 (b,z,y,x)
 * weight [64,10], gamma/beta [64], running_mean/var [64] (updated in place when training)
 * out [m,64] f32; argmax [m,64] u8 (index of the winning point, 255 = a padding row)
 * saved [239] f64: first/second moments of the decorated features, per-channel mean / invstd,
 *   and the row count the statistics were taken over
 * num_valid: optional device i32 scalar; only pillars < *num_valid exist (capacity-sized buffers of
 *   gga_hard_voxelize_batch read without a host sync): the BatchNorm statistics run over
 *   min(m, *num_valid) * max_points rows and the out rows past it are zero.
 */
int gga_pfn_fwd(const float* voxels, const int32_t* num_points, const int32_t* coors, int64_t m,
                const int32_t* num_valid, int max_points, const gga_pfn_params* prm, const float* weight, const float* gamma,
                const float* beta, float* running_mean, float* running_var, float* out,
                uint8_t* argmax, double* saved, void* workspace, size_t workspace_bytes,
                void* stream);
/* grad_weight [64,10], grad_gamma [64], grad_beta [64] from grad_out [m,64] (points carry no grad). */
int gga_pfn_bwd(const float* voxels, const int32_t* num_points, const int32_t* coors, int64_t m,
                const int32_t* num_valid, int max_points, const gga_pfn_params* prm, const float* weight, const float* gamma,
                const float* out, const uint8_t* argmax, const double* saved, const float* grad_out,
                float* grad_weight, float* grad_gamma, float* grad_beta, void* workspace,
                size_t workspace_bytes, void* stream);

/*
 * Fused DynamicPillarFeatureNet (pillar_encoder.py:162-323) in its shipped form: one layer, 4 point features -> 64
 * channels, mode = 'max', cluster and voxel centre, no distance, affine BatchNorm1d with running statistics, fp32.
 * Decoration (x, y, z, r, x-mx, y-my, z-mz, x-cx, y-cy, z-cz); the BatchNorm statistics run over the kept points
 * (counts[1]) only - a dropped point takes part in nothing.
 * points [n_points, 4] f32, coors [n_points, 4] i32 (b, z, y, x) per point, order / point2voxel / voxel_start / counts: the
 * map of gga_dynamic_voxel_map. weight [64, 10], gamma / beta [64], running_mean / var [64] (updated in place when
 * prm->training; gga_pfn_params as for gga_pfn_fwd). out [out_rows, 64] f32 and argmax [out_rows, 64] i32 (the point holding
 * the maximum, the lowest index on ties): only voxels < min(counts[0], out_rows) are written. mean [out_rows, 4] f32: the
 * voxels' point means (kept for the backward). saved [239] f64: moments, per-channel mean / invstd, row count.
 * Backward w.r.t. weight, gamma, beta (training mode); the points need no gradient.
 */
size_t gga_dynamic_pfn_workspace_bytes(int64_t n_points);
int gga_dynamic_pfn_fwd(const float* points, const int32_t* coors, int64_t n_points, const int32_t* order,
                        const int32_t* point2voxel, const int32_t* voxel_start, const int32_t* counts, int64_t out_rows,
                        const gga_pfn_params* prm, const float* weight, const float* gamma, const float* beta,
                        float* running_mean, float* running_var, float* out, int32_t* argmax, float* mean, double* saved,
                        void* workspace, size_t workspace_bytes, void* stream);
int gga_dynamic_pfn_bwd(const float* points, const int32_t* coors, int64_t n_points, const int32_t* counts, int64_t out_rows,
                        const gga_pfn_params* prm, const float* weight, const float* gamma, const float* out,
                        const int32_t* argmax, const float* mean, const double* saved, const float* grad_out,
                        float* grad_weight, float* grad_gamma, float* grad_beta, void* workspace, size_t workspace_bytes,
                        void* stream);

/* ------------------------------------------------------------------------- */
/* a3. PointPillars scatter (the kernel the "HBM GB/s on voxel scatter"       */
/* metric measures) and its backward.                                         */
/* Replaces mmdet3d/models/middle_encoders/pillar_scatter.py:62-102           */
/* (per-frame zeros + boolean mask + index_put + stack).                      */
/* ------------------------------------------------------------------------- */
enum { GGA_LAYOUT_NCHW = 0, GGA_LAYOUT_NHWC = 1 };

/* cell_map: [batch * ny * nx] i32 scratch that MUST hold -1 everywhere on entry
 * and holds -1 everywhere again on return (the canvas pass resets the entries it
 * consumes), so one hipMemset at allocation time serves every later call. */
size_t gga_pillar_scatter_map_bytes(int batch, int ny, int nx);

/*
 * feats      [m, channels] f32;  coors [m, 4] i32 (b, z, y, x)
 * num_valid  optional device i32 scalar: only rows < *num_valid are scattered
 *            (lets the caller keep a capacity-sized buffer without a host sync)
 * canvas     dense output, written in full (zero where no pillar):
 *            NCHW: [batch, channels, ny, nx]   NHWC: [batch, ny, nx, channels]
 * channels must be a multiple of 4. Duplicate (b, y, x): the highest row wins
 * (= the sequential index_put of the reference's CPU path).
 * unique_coors != 0: the caller guarantees that no (b, y, x) repeats (true for the output of
 * gga_hard_voxelize_batch and for the sites of a sparse tensor); the NHWC path then needs no
 * winner map (cell_map may be NULL) - with duplicates any one of the rows wins, as in the
 * reference's CUDA index_put. NHWC = zero fill + one 16 B copy per thread of the occupied rows.
 */
int gga_pillar_scatter_fwd(const float* feats, const int32_t* coors, int64_t m,
                           const int32_t* num_valid, int batch, int channels, int ny, int nx,
                           int layout, int unique_coors, int32_t* cell_map, float* canvas, void* stream);

/* grad_feats [m, channels] = grad_canvas gathered at each pillar's cell
 * (rows >= *num_valid get zeros). */
int gga_pillar_scatter_bwd(const float* grad_canvas, const int32_t* coors, int64_t m,
                           const int32_t* num_valid, int batch, int channels, int ny, int nx,
                           int layout, float* grad_feats, void* stream);

/* SparseEncoder's handover to the 2D backbone (middle_encoders/sparse_encoder.py:134-138: spatial_features =
 * out.dense().view(N, C * D, H, W)) in channels-last memory: out [batch, height, width, channels * depth] f32 with
 * out[b][y][x][c * depth + z] = feats[row][c] for the site coors[row] = (b, z, y, x), zeros elsewhere (the call zeroes out);
 * distinct sites. _bwd: grad_feats [n, channels] gathered from the map's gradient in the same layout. channels % 4 == 0. */
int gga_sparse_bev_nhwc_fwd(const float* feats, const int32_t* coors, int64_t n, int batch, int channels, int depth, int height,
                            int width, float* out, void* stream);
int gga_sparse_bev_nhwc_bwd(const float* grad_out, const int32_t* coors, int64_t n, int batch, int channels, int depth,
                            int height, int width, float* grad_feats, void* stream);

/* Gather map of a dense 2D convolution (kernel kh x kw, given stride / zero padding, dilation 1)
 * over the canvas, restricted to its occupied cells: map[k = ky*kw + kx][r] = row of the NHWC
 * convolution output [batch*oh*ow, C] that read pillar r through tap (ky, kx), or -1
 * (oh = (ny + 2*pad_h - kh)/stride_h + 1, likewise ow; rows >= *num_valid get -1). With it the
 * backward of the first SECOND convolution (second.py:49-57 applied to the canvas of
 * pillar_scatter.py:58-102) runs on the pillars only: its input gradient is needed just at the
 * occupied cells (all the scatter's backward reads) and its weight gradient only sees non-zero
 * input there - gga_sparse_conv_apply_bn_bwd / gga_sparse_conv_wgrad_planes with this map, the
 * output gradient as `x` (rows = output cells) and the pillar features as the other operand. */
int gga_pillar_conv_map(const int32_t* coors, int64_t m, const int32_t* num_valid, int batch, int ny, int nx,
                        int kh, int kw, int stride_h, int stride_w, int pad_h, int pad_w, int32_t* map,
                        void* stream);


/* ------------------------------------------------------------------------- */
/* a3'. Sparse 3D convolution (SubMConv3d / SparseConv3d) for SparseEncoder.  */
/* Replaces the mmcv / spconv natives behind                                  */
/*   mmdet3d/models/middle_encoders/sparse_encoder.py:107-214 and             */
/*   mmdet3d/ops/sparse_block.py:82-199 (SparseConvTensor, rule-book build,   */
/*   per-offset gather-GEMM-scatter). Coordinates are [n,4] i32 (b,z,y,x);    */
/*   weights are [kz,ky,kx,Cin,Cout] (the mmcv layout, write_spconv2.py:47).  */
/* ------------------------------------------------------------------------- */
/* Hash index of one resolution level (cell -> row). `index` is caller memory of
 * gga_sparse_index_bytes(n) bytes; remember n: later calls need it as *_index_n. */
size_t gga_sparse_index_bytes(int64_t n);
int gga_sparse_build_index(const int32_t* coors, int64_t n, int B, int D, int H, int W, void* index,
                           size_t index_bytes, void* stream);

/* Output sites of a strided SparseConv3d: every cell reached by some (input site, offset).
 * out_dhw is computed here ((in + 2p - k)/s + 1). out_coors [cap_out,4]; *n_out (device i32)
 * = number of sites, ordered by the first (input row, offset) that reaches them. out_index
 * becomes the hash index of the OUTPUT level, sized for n_in*kvol
 * (gga_sparse_out_index_bytes); pass that product as its *_index_n later. */
size_t gga_sparse_out_index_bytes(int64_t n_in, int kvol);
size_t gga_sparse_out_sites_workspace_bytes(int64_t n_in, int kvol);
int gga_sparse_conv_out_sites(const int32_t* in_coors, int64_t n_in, int B, const int32_t in_dhw[3],
                              const int32_t kernel[3], const int32_t stride[3], const int32_t pad[3],
                              int32_t out_dhw[3], int32_t* out_coors, int64_t cap_out, int32_t* n_out,
                              void* out_index, size_t out_index_bytes, void* workspace,
                              size_t workspace_bytes, void* stream);

/* Rule books in gather form. nbr [kvol, n_out]: input row under offset k of each output row
 * (-1: none). nbr_t [kvol, n_in] (optional): output row fed by each input row through offset k
 * (backward-data). Submanifold conv: out == in coords, stride 1, pad k/2, nbr_t = NULL
 * (it is nbr[kvol-1-k]). */
int gga_sparse_rulebook(const int32_t* out_coors, int64_t n_out, const int32_t* in_coors, int64_t n_in,
                        int B, const int32_t in_dhw[3], const int32_t out_dhw[3], const int32_t kernel[3],
                        const int32_t stride[3], const int32_t pad[3], const void* in_index,
                        int64_t in_index_n, const void* out_index, int64_t out_index_n, int32_t* nbr,
                        int32_t* nbr_t, void* stream);

/* Bit k of mask[r] is set when map[k][r] >= 0 (kvol <= 32). Sorting rows by this mask gives
 * tiles whose rows use the same kernel offsets; the conv kernel skips the others. */
int gga_sparse_rowmask(const int32_t* map, int64_t n_rows, int kvol, uint32_t* mask, void* stream);
/* order[i] = the row with the i-th smallest mask, rows with equal masks in row order (a stable sort of the int32 masks: the
 * processing order gga_sparse_conv_apply_bn_bwd takes as `perm`; replaces the framework's stable sort, gather_gemm.py). kvol <= 32
 * mask bits take part; masks are compared as signed 32-bit values when kvol == 32. workspace: device memory of
 * gga_sparse_mask_order_workspace_bytes(n_rows) bytes. */
/* order[i] = the row with the i-th smallest Z-order key (sample, then the bit-interleaved (z, y, x)) of coors [n_rows][4] =
 * (sample, z, y, x): consecutive rows are close in space - the tiles of the halo form (gga_sparse_halo_build). Coordinates must be
 * distinct, 0 <= coordinate < max_extent <= 65536, 0 <= sample < batch_size. */
size_t gga_sparse_morton_order_workspace_bytes(int64_t n_rows);
int gga_sparse_morton_order(const int32_t* coors, int64_t n_rows, int batch_size, int max_extent, int32_t* order,
                            void* workspace, size_t workspace_bytes, void* stream);
size_t gga_sparse_mask_order_workspace_bytes(int64_t n_rows);
int gga_sparse_mask_order(const uint32_t* mask, int64_t n_rows, int kvol, int32_t* order, void* workspace,
                          size_t workspace_bytes, void* stream);

/* The gather-GEMM y[r,:] = sum_k x[map[kk][r],:] @ W[k], kk = flip ? kvol-1-k : k, runs on the 16-bit matrix
 * instructions with fp32 carried by operand planes. Three bfloat16 planes (planes = 3): a fp32 number is
 * the exact sum of three bf16 numbers, so every product is the sum of nine bf16 products, each
 * exact in fp32, accumulated in fp32 by v_mfma_f32_32x32x16_bf16 (1.7x the fp32 MFMA rate on
 * gfx950; error vs float64 not larger than the fp32 MFMA's). The kernels issue six of the nine: the
 * three products of the low planes are together below 2^-23 of the product (one fp32 ulp) and the
 * measured error of a convolution does not change; build with -DX9_NINE for all nine. Two fp16 planes (planes = 2):
 * see gga_absmax_bits below. The entry points (gga_sparse_pack_weight_planes, gga_sparse_conv_apply_bn_bwd,
 * gga_sparse_conv_wgrad_planes) are declared there, next to the dense kernels that share the arithmetic.
 * gga_sparse_split_weight_bytes: size of a packed weight operand, packed[k][chunk][plane][col][32 ch] 16-bit elements,
 * zero beyond cin / cout (sized for three planes whatever `planes` the packing call is given; cout <= 128, else 0).
 * Replaces the weight handling inside mmcv's indice_conv (sparse_block.py:9-20 call sites). */
size_t gga_sparse_split_weight_bytes(int kvol, int cin, int cout);

/* Dense 3x3 / stride 1 / zero-pad 1 convolution of a channels-last image on the same plane arithmetic
 * (gga_dense_conv3x3_bn_bwd, gga_dense_conv3x3_levels below): x [B,H,W,cin] (cin a multiple of 32), y [B,H,W,cout]
 * (cout 64 or 128), split_weight from gga_dense_conv3x3_pack_planes. The SECOND
 * block convolutions and the first convolution of every head branch (backbones/second.py:58-63,
 * dense_heads/centerpoint_head.py:58-68); backward-data is the same call on grad_y with the
 * taps reversed and the channel roles swapped. Each workgroup fetches its input halo once per
 * 32-channel chunk, splits it into the operand planes on the way into LDS and reuses it for
 * all nine taps.
 * The convolution can also leave the batch statistics of its output for the BatchNorm
 * that follows: stats [gga_dense_conv3x3_stat_rows(B,H,W,cout,planes,1)][2][cout] f64 = partial sums and sums of
 * squares per channel - the `partials` of gga_bn_relu_fwd / gga_bn_stats, so
 * the BatchNorm does not read y a second time for its reduction.
 * Rows of `stats` (per slice) for a launch of this arithmetic over n_slices 128-channel output slices: the two-plane launches
 * run the producer / consumer form (dense_conv_ws.hip: tiles of 8 x 32 pixels at 128 output channels, 16 x 32 at 64, one row
 * per workgroup, <= 256; GGA_DC_WS=0 puts them back on the lock-step kernel), the three-plane launches the lock-step kernel
 * (tiles of 8 or 16 rows by shape, one row per tile). H, W are those of the tile space (swapped for a transposed launch). */
int64_t gga_dense_conv3x3_stat_rows(int B, int H, int W, int cout, int planes, int n_slices);
int gga_dense_conv3x3_tile_rows(int B, int H, int W, int cout, int planes);      /* 8 or 16: the tile_rows to hand gga_dense_conv3x3_levels for slices of this shape */

/* Two-fp16-plane arithmetic for the dense kernels (the default of gga_amd/dense_conv.py): each operand is scaled by
 * the power of two that puts its largest finite magnitude into [2^14, 2^15) and split into two round-to-nearest fp16
 * planes (22 significand bits), so a product needs THREE matrix products instead of the six of the three-bf16-plane
 * form; the result is scaled back exactly. Absolute accuracy per element: 2^-39 of the tensor's largest magnitude
 * (fp16 has no fp32 exponent range) - see DESIGN.md 5. `planes` = 3 selects the bf16 form (no absmax needed).
 * gga_absmax_bits: bits of the largest finite |x| of a [rows, width] f32 matrix into *out_bits (device). */
int gga_absmax_bits(const float* x, int64_t rows, int width, int64_t row_stride, uint32_t* out_bits, void* stream);
/* Operands for MANY convolution weights in two launches (gga_amd/weight_bank.py keeps the tables; weights change once per step, all
 * together): gga_absmax_table zeroes `slots[0 .. n_slots)` and leaves in every entry's slot the bits of the largest finite |x| of
 * its block of `n` floats (several entries may share a slot: the absmax of their union); gga_pack_weights_table writes, per entry,
 * kvol x n_c x n_col elements W[tap][c0 + c][col0 + col] = src[k0 * s_k0 + k1 * s_k1 + c * s_c + col * s_col] (tap = k0 * kw + k1,
 * taken in reverse order when `reverse`) into a packed operand of n_in input channels and `co` (padded, 32 * ceil(n_out / 32) for
 * n_out <= 128) columns in the stage layout of gga_sparse_pack_weight_planes (layout 0) or gga_dense_conv3x3_pack_planes (layout
 * 1); padding is never written (the caller zeroes operands once). `first`: running sum of the entries' element counts; `total`:
 * the sum; `first_block`: running sum of gga_absmax_table_blocks(n). Tables live in device memory. */
typedef struct {
    const float* src;
    uint16_t* dst;
    const uint32_t* amax;     /* absmax bits of the operand's weights (planes == 2), or NULL */
    int64_t s_k0, s_k1, s_c, s_col;
    int64_t first;
    int32_t kw, kvol, n_c, n_col, c0, col0, n_in, co, layout, reverse;
} GgaPackEntry;
typedef struct {
    const float* src;
    uint32_t* slot;
    int64_t n;
    int64_t first_block;
} GgaAmaxEntry;
int64_t gga_absmax_table_blocks(int64_t n);
int gga_absmax_table(const GgaAmaxEntry* table_device, int n_entries, int64_t n_blocks, uint32_t* slots, int n_slots, void* stream);
int gga_pack_weights_table(const GgaPackEntry* table_device, int n_entries, int64_t total, int planes, void* stream);
/* The gather-GEMM kernels (sparse, strided and transposed convolutions) in the same two forms.
 * gga_sparse_pack_weight_planes splits the weights into planes and lays them out as the kernel stages them:
 * `weight` is [kvol,cin,cout] (transpose 0) or [kvol,cout,cin] (transpose 1: the forward weight of a cout->cin conv, for
 * its backward-data pass); `packed`: gga_sparse_split_weight_bytes(kvol, cin, cout) bytes; amax_weight: the weight's absmax
 * bits (planes == 2; NULL with planes == 3). cout <= 128. */
int gga_sparse_pack_weight_planes(const float* weight, int kvol, int cin, int cout, int transpose, int planes,
                                  const uint32_t* amax_weight, void* packed, void* stream);
/* y[r,:] = sum_k x[map[kk][r],:] @ W[k], kk = flip ? kvol-1-k : k, W given as
 * gga_sparse_pack_weight_planes(.., cin, cout, .., planes, ..); y is a column block of a [n_rows, y_row_stride] matrix
 * (y_row_stride = cout: a plain [n_rows, cout] result).
 *   forward        : map = nbr,   flip 0
 *   backward-data  : x = grad_out, map = nbr_t (or nbr with flip 1 for SubM), W packed with
 *                    transpose 1, cin/cout swapped
 * perm (optional, [n_rows]): processing order of the rows (e.g. gga_sparse_mask_order of the row masks);
 * rowmask (optional, [n_rows]): gga_sparse_rowmask of `map`. Output rows are not permuted. amax_x, amax_weight: the operands'
 * absmax bits (planes == 2; NULL with planes == 3). cout <= 128; any cin (a multiple of 4 gathers 16 bytes per load).
 * With an arithmetic rule book over the pixels of a channels-last image this gather-GEMM is also the stride-2 3x3 convolution
 * of a SECOND stage (mmdet3d/models/backbones/second.py:49-57) and the kernel = stride transposed convolution of SECONDFPN
 * (necks/second_fpn.py:52-69), forward and backward-data (gga_amd/strided_conv.py).
 * stats (NULL: none) receives the per-channel sums of the output for the BatchNorm that follows
 * (ops/sparse_block.py:117-134, backbones/second.py:49-57, necks/second_fpn.py:52-69: conv -> BN -> ReLU): stats
 * [gga_sparse_conv_apply_tiles(n_rows)][2][cout] f64 = per workgroup of 128 rows the sum and the sum of squares - the
 * partials gga_bn_relu_fwd takes. */
int64_t gga_sparse_conv_apply_tiles(int64_t n_rows);
/* With bn_x (NULL: none of this, the other bn_* arguments are ignored) the launch is the backward-data pass that produces the
 * gradient of z = relu(bn(bn_x)) (the conv -> BatchNorm1d -> ReLU -> conv chains of middle_encoders/sparse_encoder.py:107-214):
 * rows are masked by the ReLU (recomputed from bn_x [n_rows, row stride bn_x_row_stride] and gamma, beta, mean, invstd exactly
 * as the forward decided) before they are stored, and stats (required) holds the sums of g and g * xhat for
 * gga_bn_relu_bwd_partials. */
int gga_sparse_conv_apply_bn_bwd(const float* x, const int32_t* map, const void* split_weight, const int32_t* perm,
                                 const uint32_t* rowmask, int64_t n_rows, int kvol, int cin, int cout, int flip, float* y,
                                 int64_t y_row_stride, int planes, const uint32_t* amax_x, const uint32_t* amax_weight,
                                 double* stats, const float* bn_x, int64_t bn_x_row_stride, const float* bn_gamma,
                                 const float* bn_beta, const float* bn_mean, const float* bn_invstd, void* stream);
/* Halo form of gga_sparse_conv_apply_bn_bwd for SUBMANIFOLD convolutions (same reference path: SubMConv3d of
 * middle_encoders/sparse_encoder.py:107-214 / ops/sparse_block.py:117-199; same arithmetic and epilogues). The rows are
 * processed in tiles of gga_sparse_halo_tile_rows() (256) rows that lie close together in space; the distinct input rows a
 * tile's kvol x 256 rule-book entries name (its halo) are staged once per 32-channel chunk in LDS and every offset reads
 * them there. gga_sparse_halo_build makes the tiling from the rule book and a spatial order of its rows (gga_amd/gather_gemm.py::
 * _Halo: Z-order of the level's coordinates):
 *   tile_rows    int32 [n_tiles * 256]         output row (= row of the rule book) of each tile slot, -1 = empty slot
 *   halo_rows    int32 [n_tiles][capacity]     tile t's halo: its first halo_counts[t] entries, distinct input rows
 *   halo_counts  int32 [n_tiles]
 *   local_map    uint16 [n_tiles][kvol][256]   position of the neighbour in the tile's halo, 0xFFFF = none; offset k of a
 *                                              flipped (backward-data) launch reads entry kvol-1-k
 * n_tiles = ceil(n_rows / 256); capacity >= kvol * 256 (no tile can overflow); apply: 8 <= kvol <= 27; cin % 32 == 0; cout 64
 * or 128; two fp16 planes only (planes == 2). stats (may be NULL) is sized as for gga_sparse_conv_apply_bn_bwd
 * ([gga_sparse_conv_apply_tiles(n_rows)][2][cout]); the rows no tile writes are zeroed. */
int64_t gga_sparse_halo_tile_rows(void);
int gga_sparse_halo_build(const int32_t* nbr, const int32_t* tile_rows, int64_t n_rows, int64_t n_tiles, int kvol,
                          int halo_capacity, int32_t* halo_rows, int32_t* halo_counts, uint16_t* local_map, void* stream);
int gga_sparse_conv_apply_halo(const float* x, const void* split_weight, const int32_t* tile_rows,
                               const int32_t* halo_counts, int halo_capacity, const int32_t* halo_rows,
                               const uint16_t* local_map, int64_t n_rows, int64_t n_tiles, int kvol, int cin, int cout, int flip,
                               float* y, int64_t y_row_stride, int planes, const uint32_t* amax_x, const uint32_t* amax_weight,
                               double* stats, const float* bn_x, int64_t bn_x_row_stride, const float* bn_gamma,
                               const float* bn_beta, const float* bn_mean, const float* bn_invstd, void* stream);
/* grad_weight [kvol,cin,cout] = sum_r x[nbr[k][r]]^T grad_out[r] on the operand planes (overwritten, not accumulated),
 * DETERMINISTIC: pairs are compacted in row order, every workgroup writes its partial sum to
 * workspace [chunks][kvol][CI][CO] (gga_sparse_conv_wgrad_workspace_bytes) and a second kernel adds the chunks in a fixed
 * order in f64. No atomics. cin, cout <= 128. x / grad_out may be column blocks of wider matrices: row strides in floats
 * (>= cin / cout). amax_x, amax_grad_out: the operands' absmax bits (planes == 2; NULL with planes == 3).
 * Every x row a rule-book entry names must start below byte 4 GiB of x (32-bit pair offsets; the kernel TRAPS - the stream
 * reports a fault - on a row beyond it: 8 M rows of 128 floats).
 * Non-finite inputs: absent neighbours, tail pairs and (dense weight gradient) pixels outside the image are not selected to zero
 * but read a real element - row 0 / the clamped pixel - and multiply it by a scale of 0 (one instruction less per fragment beside
 * the matrix instructions). With finite tensors that is 0; an Inf / NaN in the substituted element turns that padded contribution
 * into NaN, i.e. a non-finite value in x or grad_out can reach weight-gradient entries it would not reach through a select. The
 * train Runner's range guard reports non-finite operands on its guarded iterations. */
size_t gga_sparse_conv_wgrad_workspace_bytes(int64_t n_rows, int kvol, int cin, int cout);
int gga_sparse_conv_wgrad_planes(const float* x, int64_t x_row_stride, const float* grad_out, int64_t grad_out_row_stride,
                                 const int32_t* nbr, int64_t n_rows, int kvol, int cin, int cout, float* grad_weight,
                                 int planes, const uint32_t* amax_x, const uint32_t* amax_grad_out, void* workspace,
                                 size_t workspace_bytes, void* stream);
/* The kernel = stride transposed convolution of SECONDFPN (necks/second_fpn.py:52-69; s = 1: the 1x1 product) as a streaming
 * GEMM over the coarse pixels - no rule book, mask or permutation: every address is arithmetic on the pixel index
 * (csrc/deconv_stream.hip). Two fp16 planes only, fp32 in and out; y and gx are bit for bit what the gather-GEMM over the
 * arithmetic rule book gives (gga_sparse_conv_apply_bn_bwd, gga_amd/strided_conv.py).
 *   forward        x [B*h*w, cin] -> y [B, s*h, s*w, cout] channels-last (every element written exactly once);
 *                  stats (NULL: none) [gga_deconv_stream_tiles(B*h*w, cin, s)][2][cout] f64: sum and sum of squares per
 *                  (tap, pixel tile) - the partials gga_bn_relu_fwd takes; fp32 inside a 32-pixel block, as the gather kernel.
 *   backward-data  gy [B, s*h, s*w, cout] -> gx [B*h*w, cin]; all cin columns from one pass over gy.
 * weight_blocks: HOST array of device pointers to the packed operands (gga_pack_weights_table, gather layout) of the
 * 128-column blocks - forward: W[ky][kx][cin][cout block], cout / 128 of them; backward-data: W[ky][kx][cout][cin block],
 * one of min(cin, 128) columns per 128 input channels. amax_*: the operands' absmax bits. cin 64, 128 or 256; cout a
 * multiple of 128 (backward-data: 128, 256 or 512); 1 <= s <= 4; B * h * w * s * s < 2^31. */
int64_t gga_deconv_stream_tiles(int64_t n_pixels, int cin, int s);
int gga_deconv_stream_fwd(const float* x, const void* const* weight_blocks, const uint32_t* amax_x,
                          const uint32_t* amax_weight, int B, int h, int w, int cin, int cout, int s, float* y, double* stats,
                          void* stream);
int gga_deconv_stream_bwd(const float* gy, const void* const* weight_blocks, const uint32_t* amax_gy,
                          const uint32_t* amax_weight, int B, int h, int w, int cin, int cout, int s, float* gx, void* stream);
/* split_weight of the dense 3x3 kernels straight from the framework's [cout, cin, 3, 3] parameter with
 * arbitrary element strides (channels-last parameters included): size
 * gga_sparse_split_weight_bytes(9, cin, cout); backward != 0 packs the operand of the
 * backward-data convolution (a cout -> cin convolution: size ..._bytes(9, cout, cin)). amax_weight: the weight's absmax bits
 * (planes == 2; NULL with planes == 3). */
int gga_dense_conv3x3_pack_planes(const float* weight, int64_t stride_co, int64_t stride_ci, int64_t stride_ky,
                                  int64_t stride_kx, int cin, int cout, int backward, int planes,
                                  const uint32_t* amax_weight, void* packed, void* stream);
/* The dense 3x3 convolution (described above): x [B,H,W,cin], split_weight from gga_dense_conv3x3_pack_planes with the same
 * `planes`, amax_x / amax_weight the operands' absmax bits (planes == 2; NULL with planes == 3), stats NULL or
 * [gga_dense_conv3x3_stat_rows(..)][2][cout] f64.
 * y may be a 64- or 128-channel slice of a wider channels-last tensor: pixel p of the
 * result starts at y + p * y_pixel_stride (floats; cout: a dense result). A convolution with more output channels runs as
 * one call per slice (each with the weights of its slice): the backward-data of the 384 -> 64
 * shared convolution of the head (centerpoint_head.py:255-262) is three 64 -> 128 calls.
 * transposed != 0: the tiles run 32 pixels along H instead of W (maps whose width is a
 * poor multiple of 32, e.g. 124 x 108 or 62 x 54); split_weight must then be packed with the ky / kx
 * strides swapped, and stats holds gga_dense_conv3x3_stat_rows(B, W, H, ..) rows. Results are identical.
 * bn_x != NULL: the call is the backward-data convolution that produces the gradient of z = relu(bn(bn_x)) (the
 * conv -> BatchNorm -> ReLU -> conv chains of backbones/second.py:46-63): the epilogue masks the tile with the ReLU
 * (recomputed from bn_x and gamma, beta, mean, invstd of the `cout` channels of this launch, exactly as the forward
 * pass decided it) before it is stored, and `stats` (required) receives the partial sums of
 * g and g * xhat instead - the reduce pass of that BatchNorm's backward, which gga_bn_relu_bwd_partials then skips.
 * gga_dense_conv3x3_bn_bwd_pays_planes: 1 when that epilogue costs less than the reduce pass it replaces for a launch of this
 * shape (H, W of the tile space) and arithmetic (two planes: always). */
int gga_dense_conv3x3_bn_bwd_pays_planes(int B, int H, int W, int cout, int planes);
int gga_dense_conv3x3_bn_bwd_pays(int B, int H, int W, int cout);   /* = ..._pays_planes(.., 3) */
int gga_dense_conv3x3_bn_bwd(const float* x, const void* split_weight, int B, int H, int W, int cin, int cout, float* y,
                             int64_t y_pixel_stride, int transposed, double* stats, int planes, const uint32_t* amax_x,
                             const uint32_t* amax_weight, const float* bn_x, int64_t bn_x_pixel_stride, const float* bn_gamma,
                             const float* bn_beta, const float* bn_mean, const float* bn_invstd, void* stream);
/* The same convolution (no BatchNorm epilogue) over several images of different sizes in ONE launch (the tower convolutions of
 * an FPN head,
 * anchor_free_mono3d_head.py:160-250, share their weights over the levels, and the small levels alone leave most of the
 * chip idle): entry e convolves x[e] [B, heights[e], widths[e], cin] with split_weight[e] (entries that are output slices of
 * one convolution bring their own operand) into y[e] (pixel stride y_pixel_stride floats). bias (NULL: none): per entry the
 * `cout` bias values of its output channels (NULL entries: none), added in the epilogue - this is also how a single map with
 * a bias is run. tile_rows: 8, or 16 (cout 128 only: the form gga_dense_conv3x3_bn_bwd picks for maps with at least 384
 * 16-row tiles - large and small maps go into separate launches); transposed: every entry walks its map transposed (as
 * in gga_dense_conv3x3_bn_bwd; split_weight packed accordingly); stats (NULL: none): per entry the f64 [tiles][2][cout]
 * BatchNorm sums of its output (tiles of the entry = B * ceil(w / 32) * ceil(h / tile_rows) in its
 * tile space). At most 16 entries. */
int gga_dense_conv3x3_levels(int n_entries, const float* const* x, const int32_t* heights, const int32_t* widths,
                             const void* const* split_weight, int B, int cin, int cout, float* const* y, int64_t y_pixel_stride,
                             int planes, const uint32_t* const* amax_x, const uint32_t* amax_weight, const float* const* bias,
                             int tile_rows, int transposed, double* const* stats, void* stream);
/* Weight gradient of the dense 3x3 convolution on the operand planes, with the pixel index as the GEMM's K (transposed
 * LDS reads): x [B,H,W,cin], grad_y [B,H,W,cout] channels-last, cin and cout multiples of 64;
 * grad_weight is written as a [cout, cin, 3, 3] tensor with the given element strides
 * (overwritten, not accumulated); transposed != 0 walks the maps transposed, as the forward kernel does (the same
 * gradient up to the order of summation).
 * Replaces the convolution-backward-weights call behind autograd
 * for backbones/second.py:58-63 and dense_heads/centerpoint_head.py:58-68,120-121.
 * amax_x, amax_grad_y: the operands' absmax bits (planes == 2; NULL with planes == 3) - one value per tensor, or, when the
 * operand's *_per_block flag is set, one per 64-channel block (amax_x[ci / 64], amax_grad_y[co / 64]): dW[ci][co] only sees
 * channel ci of x and channel co of grad_y, so on two fp16 planes a block whose
 * values lie far below the tensor's largest magnitude keeps its own 22 significant bits (the 960-channel gradient of the 15 head
 * branches: regression branches with a few object cells beside the heat-map branches).
 * One image of an operand (H * W * max(cin, cout) floats) must stay below 2 GiB: the kernel addresses a staged piece by a 32-bit
 * offset inside its image row beside a scalar row base (GGA_ERR_* otherwise). */
size_t gga_dense_wgrad3x3_workspace_bytes(int B, int H, int W, int cin, int cout);
int gga_dense_wgrad3x3_block_amax(const float* x, const float* grad_y, int B, int H, int W, int cin, int cout,
                                  float* grad_weight, int64_t stride_co, int64_t stride_ci, int64_t stride_ky,
                                  int64_t stride_kx, int transposed, int planes, const uint32_t* amax_x, int amax_x_per_block,
                                  const uint32_t* amax_grad_y, int amax_grad_y_per_block, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- */
/* a4/a5 (elementwise part). Fused training-mode BatchNorm (+ residual add)   */
/* (+ ReLU) over a [rows, channels] row-major tensor = the sparse [N,C]        */
/* features and the memory of a channels-last [B,C,H,W] activation.           */
/* Replaces the separate BN / ReLU / add kernels of                            */
/*   mmdet3d/models/backbones/second.py:46-63, necks/second_fpn.py:66-69,      */
/*   dense_heads/centerpoint_head.py (ConvModule), ops/sparse_block.py:117-134 */
/* y = relu(bn(x) + residual); channels % 4 == 0 and channels/4 must divide 256. */
/* ------------------------------------------------------------------------- */
size_t gga_bn_relu_workspace_bytes(int64_t rows, int channels);
size_t gga_bn_relu_mask_bytes(int64_t rows, int channels);   /* 1 bit / element ReLU sign */
/* Statistics only (no normalised output): saved [2*channels] = mean / invstd, scale_shift
 * [2*channels] = gamma*invstd, beta - mean*gamma*invstd; running stats updated when training. For
 * consumers that apply the affine + ReLU themselves while loading (gga_head_conv3x3_* with
 * in_scale_shift), so the normalised activation is never written. Its backward is
 * gga_bn_relu_bwd with relu = 2 and mask_bits = scale_shift: the ReLU mask is
 * recomputed as fma(x, scale, shift) > 0 instead of read from stored bits.
 * partials != NULL: batch statistics (whatever `training` says) from per-channel sums already reduced by the producer of x:
 * n_partials >= 1 rows [2][partials_width] f64 (sum, sum of squares over disjoint row sets that together cover all `rows`), of
 * which this BatchNorm's channels are columns column_offset .. column_offset + channels (partials_width = channels,
 * column_offset = 0: rows of its own; wider: a convolution launch that computed the inputs of several BatchNorms side by
 * side, the head's paired first convolutions). x and workspace may then be NULL.
 * partials == NULL: a reduce pass over x (training) or the running statistics; x and workspace required, partials_width and
 * column_offset ignored. */
int gga_bn_stats(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                 int64_t rows, int channels, float eps, float momentum, int training, float* saved,
                 float* scale_shift, const double* partials, int n_partials, int partials_width, int column_offset,
                 void* workspace, size_t workspace_bytes, void* stream);
/* Forward: saved [2*channels] f32 receives mean / invstd; running stats are updated when training. relu != 0 also writes
 * mask_bits (gga_bn_relu_mask_bytes). y may be a column block of a wider row-major matrix:
 * row r starts at y + r * y_row_stride (floats; a multiple of 4, >= channels; the
 * pointer 16 B aligned; channels: a dense result). The three SECONDFPN branches write their BN+ReLU output straight into
 * their channel slice of the concatenated map and read their slice of its gradient in place
 * (necks/second_fpn.py:85-91: torch.cat of the deblock outputs) - no concat copy, no split copy.
 * partials != NULL: training-mode statistics from per-channel sums already reduced by the producer of x: partials
 * [n_partials][2][channels] f64 (sum, sum of squares over disjoint row sets that together cover all `rows`), e.g. the `stats`
 * of gga_dense_conv3x3_bn_bwd or gga_sparse_conv_apply_bn_bwd; the reduce pass over x is skipped.
 * Backward (batch statistics): grad_x, optional grad_residual (= masked grad_y), grad_gamma/beta; grad_y strided like y.
 * relu: 0 none, 1 mask_bits = the bits written by the forward, 2 mask_bits = scale_shift of
 * gga_bn_stats (mask recomputed from x). training = 0 is the backward of an evaluation-mode forward (running statistics,
 * e.g. a frozen backbone with norm_eval): grad_x = gamma * invstd * g, grad_gamma / grad_beta as in training mode.
 * amax_y / amax_grad_x (NULL: none): the bits of the largest finite magnitude written (y /
 * grad_x), max-combined into *amax (the caller zeroes it; several calls may share it) - what the two-fp16-plane
 * convolution kernels that consume the tensor derive their scale from, without a pass of their own. */
int gga_bn_relu_fwd(const float* x, const float* residual, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, int64_t rows, int channels, float eps, float momentum,
                    int training, int relu, float* y, int64_t y_row_stride, void* mask_bits, float* saved,
                    const double* partials, int n_partials, uint32_t* amax_y, void* workspace, size_t workspace_bytes,
                    void* stream);
int gga_bn_relu_bwd(const float* grad_y, int64_t grad_y_row_stride, const float* x, const void* mask_bits,
                    const float* gamma, const float* saved, int64_t rows, int channels, int relu, int training, float* grad_x,
                    float* grad_residual, float* grad_gamma, float* grad_beta, uint32_t* amax_grad_x, void* workspace,
                    size_t workspace_bytes, void* stream);
/* sums[c] = sum over the rows of x [rows, channels] (row major; channels / 4 must divide 256) - the bias gradient of a
 * convolution from its output gradient in channels-last memory. Workspace: gga_bn_relu_workspace_bytes(rows, channels). */
int gga_column_sums(const float* x, int64_t rows, int channels, float* sums, void* workspace, size_t workspace_bytes,
                    void* stream);
/* The backward pass whose reduce pass was done by the producer of the gradient (gga_dense_conv3x3_bn_bwd): grad_masked
 * is already multiplied by the ReLU mask, partials [n_partials][2][channels] f64 hold the sums of g and g * xhat. */
int gga_bn_relu_bwd_partials(const float* grad_masked, int64_t grad_row_stride, const float* x, const float* gamma,
                             const float* saved, int64_t rows, int channels, int training, const double* partials,
                             int n_partials, float* grad_x, float* grad_gamma, float* grad_beta, uint32_t* amax_grad_x,
                             void* workspace, size_t workspace_bytes, void* stream);

/* Fused GroupNorm (+ ReLU) over a channels-last [B, rows_per_sample, channels] activation (statistics per sample and
 * group of channels / groups channels): replaces the GN + ReLU of the ConvModules in the PGD / FCOS3D head
 * (mmdet3d/models/dense_heads/anchor_free_mono3d_head.py:160-250, norm_cfg type 'GN'), whose framework kernels need NCHW
 * memory. stat [B][groups][2] = mean, rstd; scale_shift [B][2][channels]; both are kept for the backward, which
 * recomputes the ReLU mask from x. channels/4 must divide 256, channels per group % 4 == 0. amax_* as in gga_bn_relu_fwd / _bwd. */
size_t gga_gn_relu_workspace_bytes(int B, int channels);
int gga_gn_relu_fwd(const float* x, const float* gamma, const float* beta, int B, int64_t rows_per_sample, int channels,
                    int groups, float eps, int relu, float* y, float* stat, float* scale_shift, uint32_t* amax_y,
                    void* workspace, size_t workspace_bytes, void* stream);
int gga_gn_relu_bwd(const float* grad_y, const float* x, const float* gamma, const float* stat, const float* scale_shift,
                    int B, int64_t rows_per_sample, int channels, int groups, int relu, float* grad_x, float* grad_gamma,
                    float* grad_beta, uint32_t* amax_grad_x, void* workspace, size_t workspace_bytes, void* stream);

/* a5 (output convs of the head branches): 3x3 conv, 64 input channels -> 1..4 output channels,
 * stride 1, pad 1, + bias. Replaces the last layer of each SeparateHead branch,
 * mmdet3d/models/dense_heads/centerpoint_head.py:70-79 (HBM-bound; N = 9 taps x cout on the
 * matrix cores). x: channels-last memory [B,H,W,64] of a [B,64,H,W] tensor, or a 64-channel column block of
 * a wider one (x_pixel_stride floats between pixels, 64 when dense); weight [cout,64,3,3];
 * y [B,cout,H,W] NCHW-contiguous. in_scale_shift (optional, [2*64]): the convolution input is
 * relu(x * scale + shift) per channel, applied while loading - the BatchNorm + ReLU of the
 * branch's ConvModule (centerpoint_head.py:58-68) fused into its consumer.
 * Map size: H and W below 16384 and 16 * W * x_pixel_stride below 2^31 elements (the kernel keeps 16-bit halo
 * coordinates and 32-bit element offsets within a tile); a larger map returns GGA_ERR_INVALID_ARG before anything is
 * launched. */
int gga_head_conv3x3_fwd(const float* x, int64_t x_pixel_stride, const float* in_scale_shift, const float* weight,
                         const float* bias, int B, int H, int W, int cin, int cout, float* y, void* stream);
/* The same convolution on the 13 x 32 tiles that tile_active calls active, one byte per tile in the layout
 * [B][ceil(H / 13)][ceil(W / 32)] (non-zero = active): those tiles of y receive exactly the values gga_head_conv3x3_fwd
 * writes there, bit for bit, and every other element of y is left untouched. For a map that is read at a few cells only:
 * a regression map of a CenterHead in training, which F.gather_pred reads at the object cells (gga_head_cell_tiles). */
int gga_head_conv3x3_fwd_tiles(const float* x, int64_t x_pixel_stride, const float* in_scale_shift, const float* weight,
                               const float* bias, int B, int H, int W, int cin, int cout, const uint8_t* tile_active, float* y,
                               void* stream);
/* The tile maps of gga_head_conv3x3_fwd_tiles from gather indices: ind [n_maps, K] int64, a cell index y * W + x per slot.
 * Stores 1 into tile_active [n_maps][ceil(H / 13)][ceil(W / 32)], which the caller has zeroed, for the tile that holds
 * each index - all K slots of a map, whatever their mask says: the gather reads the dead slots' cell (0) too. An index
 * outside [0, H * W) marks nothing. One launch for all maps (every task of a head: n_maps = tasks x B).
 * gga_head_cell_tiles_count: the number of tiles (= bytes) of B maps, 0 for a size below 1. */
int64_t gga_head_cell_tiles_count(int B, int H, int W);
int gga_head_cell_tiles(const int64_t* ind, int n_maps, int K, int H, int W, uint8_t* tile_active, void* stream);
/* grad_weight [cout,64,3,3] and grad_bias [cout] (optional) from grad_y [B,cout,H,W]. Map size: H and W below 16384
 * (the forward's bound, kept on this side so that both directions accept the same maps) and 8 * W * x_pixel_stride
 * below 2^31 elements, else GGA_ERR_INVALID_ARG before anything is launched. workspace:
 * gga_head_conv3x3_workspace_bytes(cout), the partial sums of the at most 512 workgroups of the launch. */
size_t gga_head_conv3x3_workspace_bytes(int cout);
int gga_head_conv3x3_wgrad(const float* x, int64_t x_pixel_stride, const float* in_scale_shift, const float* grad_y,
                           int B, int H, int W, int cin, int cout, float* grad_weight, float* grad_bias,
                           void* workspace, size_t workspace_bytes, void* stream);

/* Backward of the whole branch tail BatchNorm(training) -> ReLU -> this conv w.r.t. the BatchNorm input x
 * (centerpoint_head.py:58-79 under autograd): grad_x [B,H,W,64], grad_gamma / grad_beta [64] (optional) from
 * grad_y [B,cout,H,W], the conv weight and the statistics gga_bn_stats left (saved = mean / invstd,
 * scale_shift). The conv's input gradient is rebuilt from grad_y inside the two BatchNorm-backward passes and
 * never stored. x / grad_x may be 64-channel column blocks of wider tensors (pixel strides in floats).
 * amax_grad_x (optional): atomicMax target for the bits of the largest finite |grad_x| written (not reset here).
 * workspace: gga_bn_relu_workspace_bytes(B*H*W, 64). */
int gga_head_tail_bwd(const float* grad_y, const float* x, int64_t x_pixel_stride, const float* scale_shift,
                      const float* gamma, const float* saved, const float* weight, int B, int H, int W, int cin, int cout,
                      float* grad_x, int64_t grad_x_pixel_stride, float* grad_gamma, float* grad_beta, uint32_t* amax_grad_x,
                      void* workspace, size_t workspace_bytes, void* stream);

/* Which 8 x 32 tiles of a branch's output gradient hold anything: tile_active[(b * tiles_y + ty) * tiles_x + tx]
 * (tiles_x = ceil(W / 32), tiles_y = ceil(H / 8), one byte each) is 1 when any bit of any value of any of the cout
 * channels of grad_y [B,cout,H,W] is set inside the tile or within one pixel around it (clipped to the image; -0.0, NaN
 * and Inf count as set), else 0. The regression branches of a CenterHead receive a gradient only at the cells of live
 * objects (F.gather_pred), so nearly all of their tiles are inactive. */
int gga_head_tile_activity(const float* grad_y, int B, int H, int W, int cout, uint8_t* tile_active, void* stream);

/* Backward of one head branch = gga_head_conv3x3_wgrad (with in_scale_shift = scale_shift) followed by
 * gga_head_tail_bwd, same arguments and bit-identical results for finite x, on the active tiles of grad_y: the
 * weight gradient and the BatchNorm-backward sums visit only those (an inactive tile contributes exactly +0 to every
 * sum), and the pass that writes grad_x skips the rebuild of the conv's input gradient on the others.
 * sparse_grad_y: a hint, never a change of the result - 0 for a gradient known to be dense (a heat-map branch's): no map
 * is built and every tile is visited, exactly the two calls above; non-zero otherwise (a dense gradient then costs the
 * map on top: measured +15-20 us per branch at 16 x 248 x 216).
 * workspace: gga_head_branch_bwd_workspace_bytes(B, H, W, cout), used by this stream alone until the call's work is done. */
size_t gga_head_branch_bwd_workspace_bytes(int B, int H, int W, int cout);
int gga_head_branch_bwd(const float* grad_y, const float* x, int64_t x_pixel_stride, const float* scale_shift,
                        const float* gamma, const float* saved, const float* weight, int B, int H, int W, int cin, int cout,
                        float* grad_weight, float* grad_bias, float* grad_x, int64_t grad_x_pixel_stride, float* grad_gamma,
                        float* grad_beta, uint32_t* amax_grad_x, int sparse_grad_y, void* workspace, size_t workspace_bytes,
                        void* stream);

/* ------------------------------------------------------------------------- */
/* a6/a7. Heat-map target splat on the device.                                */
/* Replaces the per-object numpy gaussian + H2D copy + torch.max(out=) of     */
/* mmdet3d/core/utils/gaussian.py:25-54 called from                           */
/* mmdet3d/models/dense_heads/centerpoint_head_gga.py:576.                    */
/* ------------------------------------------------------------------------- */
/*
 * heatmap       [n_maps, H, W] f32, zero-filled here, then max-splatted
 * objs          [n_obj, 4] i32: (map index, cx, cy, radius)
 * patch_table   f32 gaussian patches for radius 0..max_radius, concatenated;
 *               patch r is (2r+1)^2 values at patch_offsets[r] (built on the host
 *               with the reference's f64 formula so the values are bit-identical)
 */
int gga_heatmap_splat(float* heatmap, int n_maps, int H, int W, const int32_t* objs, int n_obj,
                      const float* patch_table, const int32_t* patch_offsets, int max_radius,
                      void* stream);

/* ------------------------------------------------------------------------- */
/* The tasks of a head in one launch (a8 - a13).                              */
/* A CenterHead computes the same losses for every task (class group), on     */
/* maps of one size. Each loss kernel takes this table BY VALUE and picks its */
/* task from blockIdx.y, so a stage costs one launch whatever the number of   */
/* tasks, and every task's result is bit for bit what a table holding that    */
/* task alone gives. An entry carries one task's device pointers (shapes at   */
/* the fields, semantics at the stage that uses them) and the two sizes that  */
/* differ between tasks; a stage reads only its own fields, the others may    */
/* stay null. B, K, H, W are common to the tasks of a table.                  */
/* ------------------------------------------------------------------------- */
#define GGA_MAX_TASKS 8
typedef struct {
    /* focal loss: logits, target [n_heat] (n_heat = B * classes of the task * H * W); focal_out [2] = (loss, num_pos),
     * written by the forward and read by the backward; focal_grad [1] = d / d loss; grad_logits [n_heat] */
    const float* logits;
    const float* target;
    int64_t n_heat;
    float* focal_out;
    const float* focal_grad;
    float* grad_logits;
    /* gather: reg [B,2,H,W], height [B,1,H,W], dim [B,3,H,W], rot [B,2,H,W] and their gradients (same shapes) */
    const float *reg, *height, *dim, *rot;
    float *g_reg, *g_height, *g_dim, *g_rot;
    /* gather and box losses: ind [B,K] i64, mask [B,K] u8; pred [B,K,8] = (dx, dy, z, log l, log w, log h, sin, cos)
     * (written by the gather, read by the losses); grad_pred [B,K,8] (written by the losses' backward, read by the gather's) */
    const int64_t* ind;
    const uint8_t* mask;
    float* pred;
    float* grad_pred;
    /* box losses, inputs: anno_box [B,K,5] (x1, y1, x2, y2, srl); lidar2img [B,K,4,4]; bound_mask [B,K,4];
     * ibp_xy [n_pts,2] in-box points of every object (xy, packed); ibp_offsets [n_ibp_obj + 1] point ranges;
     * ibp_slot [n_ibp_obj] = b * K + k (the three may be null when n_ibp_obj == 0) */
    const float* anno_box;
    const float* lidar2img;
    const uint8_t* bound_mask;
    const float* ibp_xy;
    const int32_t* ibp_offsets;
    const int32_t* ibp_slot;
    int32_t n_ibp_obj;
    /* box losses, outputs of the forward: losses [GGA_L_NUM], box_out [B,K,12], term_grads [GGA_L_NUM,B,K,8] = d losses[t] /
     * d pred per term (see gga_box_losses_fwd); the backward reads term_grads and grad_losses [GGA_L_NUM] = d / d losses */
    float* losses;
    float* box_out;
    float* term_grads;
    const float* grad_losses;
} gga_task;

typedef struct {
    int32_t n_tasks;                      /* 1 .. GGA_MAX_TASKS, else GGA_ERR_INVALID_ARG */
    gga_task task[GGA_MAX_TASKS];
} gga_task_table;

/* ------------------------------------------------------------------------- */
/* a8. clip_sigmoid + GaussianFocalLoss (mean over max(num_pos,1)), fused.    */
/* Replaces mmdet3d/models/utils/clip_sigmoid.py:16 + mmdet GaussianFocalLoss */
/* + the host-syncing num_pos.item() of centerpoint_head_gga.py:650-655.      */
/* ------------------------------------------------------------------------- */
/* Every task of the table in one launch per kernel. Workspace: n_max = the largest n_heat of the table.
 * forward:  focal_out[0] = scale * sum(loss) / (max(num_pos,1) + eps_f32); focal_out[1] = num_pos.
 * backward: grad_logits[i] = (*focal_grad) * scale * dloss_i/dlogit_i / (max(num_pos,1)+eps); focal_out is what the
 *           forward call wrote (num_pos is read from focal_out[1]).
 * logits, target and grad_logits must be 16-byte aligned. */
size_t gga_focal_loss_workspace_bytes(int64_t n_max, int n_tasks);
int gga_focal_loss_fwd(const gga_task_table* tasks, float alpha, float gamma, float scale, void* workspace,
                       size_t workspace_bytes, void* stream);
int gga_focal_loss_bwd(const gga_task_table* tasks, float alpha, float gamma, float scale, void* stream);

/* ------------------------------------------------------------------------- */
/* a9. Gather the 8 regression channels at the object cells, and its backward */
/* (scatter-add into the dense head-map gradients).                           */
/* Replaces cat + permute + contiguous + gather of                            */
/* centerpoint_head_gga.py:141-164,657-676.                                   */
/* ------------------------------------------------------------------------- */
/* All tasks of the table in one launch (B, K, H, W are the tasks' common sizes).
 * forward:  reg, height, dim, rot gathered at ind -> pred [B,K,8].
 * backward: the four gradient maps are zero-filled here, then grad_pred is scatter-added; slots with mask == 0 are skipped
 *           (their weight is zero in every loss term). It keeps a frame's K slots in LDS: K <= 512, else
 *           GGA_ERR_INVALID_ARG. It clears every gradient map with ONE memset when each task's four maps lie one behind the
 *           other (reg, height, dim, rot) and the tasks one behind the other, else with one memset per task or map. */
int gga_gather_pred_fwd(const gga_task_table* tasks, int B, int K, int H, int W, void* stream);
int gga_gather_pred_bwd(const gga_task_table* tasks, int B, int K, int H, int W, void* stream);

/* ------------------------------------------------------------------------- */
/* a10-a13. The GGA geometry-aware losses of a task, forward + analytic       */
/* gradient in one pass: rotation, decode, 8 corners, lidar2img projection,   */
/* 2D box (BPL), semantic ratio (SRL), point-to-box alignment (PAL).          */
/* Replaces centerpoint_head_gga.py:167-341 (GGA_calculate_rotation,          */
/* get_distance_single/bev, get_prediction_single) and the loss assembly      */
/* :678-721 with mmdet L1Loss(reduction='mean', loss_weight).                 */
/* ------------------------------------------------------------------------- */
typedef struct {
    int32_t B, K;                 /* frames, object slots per frame (max_objs) */
    int32_t fm_w;                 /* feature-map width (ind = y * fm_w + x) */
    float voxel_size[2];          /* train_cfg.voxel_size[:2] */
    float out_size_factor;
    float pc_range[2];            /* train_cfg.point_cloud_range[:2] */
    float code_weights[5];        /* train_cfg.code_weights */
    float l1_loss_weight;         /* L1Loss.loss_weight (0.25) */
    float w_bpl, w_srl, w_pal;    /* head:697-721 multipliers (0.3, 0.1, 0.1) */
} gga_loss_params;

/* indices into losses[] */
enum { GGA_L_BPL = 0, GGA_L_SRL = 1, GGA_L_PAL_MIN = 2, GGA_L_PAL_X = 3, GGA_L_PAL_Y = 4,
       GGA_L_NUM = 5 };

/* All tasks of the table in one launch per kernel (box_slot_kernel excepted: one launch per task, see head_loss.hip); prm
 * (B, K included) is common to the tasks. Inputs: the task's pred, ind, mask, anno_box, lidar2img, bound_mask and in-box
 * points (shapes at gga_task). Outputs per task:
 *   losses      [5] f32, final dict values (weights and 1/(num+1e-4+eps) applied)
 *   box_out     [B,K,12] f32: rot, l, w, u_min, v_min, u_max, v_max, X, Y, p2c_min, p2c_x, p2c_y
 *               (intermediates, for parity tests / logging)
 *   term_grads  [5,B,K,8] f32: d losses[t] / d pred, per term
 * term_grads and box_out are cleared with ONE memset when each task's box_out lies behind its term_grads and the tasks one
 * behind the other (else with one memset per task or buffer); a second one clears the workspace. */
size_t gga_box_losses_workspace_bytes(int B, int K, int n_tasks);
int gga_box_losses_fwd(const gga_task_table* tasks, const gga_loss_params* prm, void* workspace, size_t workspace_bytes,
                       void* stream);
/* task.grad_pred [B,K,8] = sum_t task.grad_losses[t] * task.term_grads[t] (grad_losses [5] on the device). */
int gga_box_losses_bwd(const gga_task_table* tasks, int B, int K, void* stream);

/* ------------------------------------------------------------------------- */
/* Supervised CenterPoint: the targets of a batch in one launch, and the      */
/* code-weighted masked L1 of all tasks in one launch each way.               */
/* Replaces the per-object Python loop of                                     */
/* mmdet3d/models/dense_heads/centerpoint_head.py:435-583 (several tiny       */
/* host-to-device copies per object) and the loss assembly of :623-638.       */
/* ------------------------------------------------------------------------- */
#define GGA_CENTER_MAX_CLASSES 64
#define GGA_CENTER_MAX_K 512
typedef struct {
    float pc_range[2];            /* train_cfg.point_cloud_range[:2] */
    float voxel_size[2];          /* train_cfg.voxel_size[:2] */
    float out_size_factor;
    float gaussian_overlap;
    int32_t min_radius;
    int32_t K;                    /* max_objs * dense_reg slots per (frame, task), 1 .. GGA_CENTER_MAX_K */
    int32_t H, W;                 /* feature-map size */
    int32_t n_tasks;              /* 1 .. GGA_MAX_TASKS */
    int32_t n_classes;            /* 1 .. GGA_CENTER_MAX_CLASSES, the sum of task_classes */
    int32_t task_classes[GGA_MAX_TASKS];        /* classes of task t */
    int32_t task_class_base[GGA_MAX_TASKS];     /* classes of the tasks before t */
    int32_t class_task[GGA_CENTER_MAX_CLASSES]; /* label -> task */
    int32_t class_index[GGA_CENTER_MAX_CLASSES];/* label -> index inside its task */
} gga_center_params;

/* boxes [N,7] f32 (x, y, z bottom centre, dx, dy, dz, yaw) and labels [N] i64 of the whole batch, frame f being rows
 * frame_offsets[f] .. frame_offsets[f+1] (frame_offsets [B+1] i32, on the device like the rest). One workgroup per (frame,
 * task). An object goes to the task of its label (label < 0 or >= n_classes: dropped); its slot inside the (frame, task) is
 * its rank class-major, then by object index; ranks >= K are dropped. An object whose scaled width or length is <= 0 or whose
 * integer cell lies off the map keeps its slot, which stays empty. Outputs, every element written (zero where empty):
 *   ind       [n_tasks, B, K] i64   cy * W + cx
 *   mask      [n_tasks, B, K] u8
 *   anno_box  [n_tasks, B, K, 8] f32  (cx_f - cx, cy_f - cy, z + dz / 2, log dx, log dy, log dz, sin yaw, cos yaw)
 *   heatmaps  [B * n_classes * H * W] f32: task t is the [B, task_classes[t], H, W] block at B * task_class_base[t] * H * W;
 *             cleared here, then max-splatted from patch_table / patch_offsets (as gga_heatmap_splat takes them) with
 *             radius = max(min_radius, int(gaussian_radius((length, width), gaussian_overlap))). The table must reach the
 *             largest radius of the batch: an object with radius > max_radius is not splatted. */
int gga_center_targets(const float* boxes, const int64_t* labels, const int32_t* frame_offsets, int B,
                       const gga_center_params* prm, int64_t* ind, uint8_t* mask, float* anno_box, float* heatmaps,
                       const float* patch_table, const int32_t* patch_offsets, int max_radius, void* stream);

typedef struct {
    const float* pred;            /* [B,K,8] from gga_gather_pred_fwd */
    const float* anno_box;        /* [B,K,8]; a NaN element has weight 0 in the loss and in the gradient */
    const uint8_t* mask;          /* [B,K] */
    float* loss;                  /* [2] = (loss, sum(mask)), written by the forward and read by the backward */
    const float* grad_loss;       /* [1] d / d loss */
    float* grad_pred;             /* [B,K,8], every element written */
} gga_center_loss_task;

typedef struct {
    int32_t n_tasks;              /* 1 .. GGA_MAX_TASKS */
    gga_center_loss_task task[GGA_MAX_TASKS];
} gga_center_loss_table;

typedef struct {
    float code_weights[8];        /* train_cfg.code_weights */
    float loss_weight;            /* L1Loss.loss_weight */
} gga_center_loss_weights;

/* loss[0] = loss_weight * sum(mask * [anno_box not NaN] * code_weights[c] * |pred - anno_box|) / ((sum(mask) + 1e-4) + eps_f32)
 * per task, reduced in a fixed order without floating-point atomics: the same inputs give the same bits, and a task's value
 * does not depend on the other tasks of the table. pred and anno_box must be 16-byte aligned. */
int gga_center_reg_loss_fwd(const gga_center_loss_table* tasks, int B, int K, const gga_center_loss_weights* weights,
                            void* stream);
int gga_center_reg_loss_bwd(const gga_center_loss_table* tasks, int B, int K, const gga_center_loss_weights* weights,
                            void* stream);

/* ------------------------------------------------------------------------- */
/* Anchor3DHead (SECOND / PointPillars): the targets of a batch without a     */
/* read-back, the three losses of a batch, the decode of the kept anchors.    */
/* Replaces the per-frame, per-class assignment loop of                       */
/* mmdet3d/models/dense_heads/train_mixins.py:63-80,126-183, the gathers and   */
/* eager losses of anchor3d_head.py:194-278 and the per-frame decode of        */
/* :427-516.                                                                  */
/* ------------------------------------------------------------------------- */
#define GGA_ANCHOR_MAX_GROUPS 16
typedef struct {
    int32_t n_groups;             /* assigners: 1, or one per anchor size (1 .. GGA_ANCHOR_MAX_GROUPS) */
    int32_t n_rot;                /* rotations per size; the group of anchor a is (a / n_rot) % n_groups */
    int32_t num_classes;          /* background label; a ground truth with a label outside [0, num_classes) takes no part */
    int32_t assign_per_class;     /* != 0: group g sees only the ground truths with label g */
    float pos_iou_thr[GGA_ANCHOR_MAX_GROUPS];
    float neg_iou_thr[GGA_ANCHOR_MAX_GROUPS];
    float min_pos_iou[GGA_ANCHOR_MAX_GROUPS];
    float pos_weight;             /* train_cfg.pos_weight: > 0 is the label weight of a positive, otherwise that is 1 */
    float dir_offset, dir_limit_offset;
} gga_anchor_params;

/* anchors [A,7] f32 in head order (h, w, size, rot); boxes [N,7] f32 / labels [N] i64 of the whole batch, frame f being rows
 * frame_offsets[f] .. frame_offsets[f+1] (frame_offsets [B+1] i32 on the device; frame_offsets_host is the same array in host
 * memory, checked here before anything is launched: non-negative, monotone, ending at or before N).
 * IoU = mmdet's bbox_overlaps of the nearest-BEV boxes with eps 1e-6 on the union, in f32 with one rounded operation per tensor
 * operation of the reference. Per (frame, group), over the ground truths the group sees, MaxIoUAssigner with
 * match_low_quality and gt_max_assign_all: an anchor starts ignored (-1); 0 <= max IoU < neg_iou_thr makes it negative;
 * max IoU >= pos_iou_thr assigns the argmax (the lowest index among equal values); then for every ground truth i in ascending
 * order whose best IoU over the group's anchors is >= min_pos_iou, every anchor that reaches that best IoU goes to i. A group
 * that sees no ground truth has only negatives. Outputs, every element written:
 *   labels [B,A] i64 (num_classes for negatives and ignored anchors), label_weights [B,A] f32 (positive: pos_weight if > 0
 *   else 1; negative 1; ignored 0), bbox_targets [B,A,7] f32 (DeltaXYZWLHRBBoxCoder.encode(anchor, gt) for positives, else 0),
 *   pos_flag [B,A] u8, dir_targets [B,A] i64 (get_direction_target, two bins), dir_weights [B,A] f32, pos_count [B] i32.
 * workspace: gga_anchor_targets_workspace_bytes(N, n_groups) bytes (0 for sizes it refuses). Launches: two memsets and two
 * kernels, ordered by the stream; integer atomics only, so the same inputs give the same bits. */
size_t gga_anchor_targets_workspace_bytes(int64_t N, int n_groups);
int gga_anchor_targets(const float* anchors, int A, const gga_anchor_params* prm, const float* boxes, const int64_t* labels, int N,
                       const int32_t* frame_offsets, const int32_t* frame_offsets_host, int B, int64_t* out_labels,
                       float* label_weights, float* bbox_targets, uint8_t* pos_flag, int64_t* dir_targets, float* dir_weights,
                       int32_t* pos_count, void* workspace, size_t workspace_bytes, void* stream);

typedef struct {
    int32_t B, HW, n_anchors, num_classes;  /* A = HW * n_anchors anchors per frame, anchor i = pixel * n_anchors + a */
    int32_t diff_rad_by_sin;
    int32_t reserved;
    int64_t cls_stride[3];        /* (batch, channel, pixel) strides in elements of cls_score [B, n_anchors * C, H, W] */
    int64_t reg_stride[3];        /* of bbox_pred [B, n_anchors * 7, H, W] */
    int64_t dir_stride[3];        /* of dir_cls_pred [B, n_anchors * 2, H, W] */
    float gamma, alpha;           /* sigmoid focal loss */
    float beta;                   /* smooth L1 */
    float code_weight[7];
    float loss_weight[3];         /* loss_cls, loss_bbox, loss_dir */
} gga_anchor_loss_params;

/* Anchor i of frame b reads channel a * C + c of cls_score, a * 7 + k of bbox_pred and a * 2 + d of dir_cls_pred at pixel i /
 * n_anchors: the reference's permute(0, 2, 3, 1).reshape, through the strides, for NCHW and channels-last memory alike.
 *   out[0] = loss_weight[0] * sum over anchors and classes of label_weights * sigmoid focal loss        / (avg + eps_f32)
 *   out[1] = loss_weight[1] * sum over positives and k of code_weight[k] * smooth_l1(pred, target; beta) / (avg + eps_f32)
 *            (diff_rad_by_sin: column 6 compares sin p * cos t with cos p * sin t)
 *   out[2] = loss_weight[2] * sum over positives of dir_weights * two-way softmax cross entropy          / (avg + eps_f32)
 *   out[3] = avg = sum_b max(pos_count[b], 1), read on the device
 * dir_cls_pred may be null (no direction classifier): out[2] = 0. Reduced in a fixed order without floating-point atomics: the
 * same inputs give the same bits (forward: a kernel of per-workgroup f64 partial sums, then one workgroup that adds them;
 * backward: one kernel). workspace: GGA_ANCHOR_LOSS_WORKSPACE_BYTES. The backward reads out[3] and grad_out [3] f32
 * (d / d out[0..2]) from the device and writes every element of the three gradient tensors, which have the strides of their
 * inputs. */
#define GGA_ANCHOR_LOSS_WORKSPACE_BYTES 24576
int gga_anchor_loss_fwd(const gga_anchor_loss_params* prm, const float* cls_score, const float* bbox_pred, const float* dir_cls_pred,
                        const int64_t* labels, const float* label_weights, const uint8_t* pos_flag, const float* bbox_targets,
                        const int64_t* dir_targets, const float* dir_weights, const int32_t* pos_count, float* out,
                        void* workspace, size_t workspace_bytes, void* stream);
int gga_anchor_loss_bwd(const gga_anchor_loss_params* prm, const float* cls_score, const float* bbox_pred, const float* dir_cls_pred,
                        const int64_t* labels, const float* label_weights, const uint8_t* pos_flag, const float* bbox_targets,
                        const int64_t* dir_targets, const float* dir_weights, const float* fwd_out, const float* grad_out,
                        float* grad_cls, float* grad_bbox, float* grad_dir, void* stream);

/* The kept anchors of a batch: inds [B,K] i64 (anchor index inside the frame; an index outside [0, A) gives a row of zeros),
 * scores [B,A,C] f32 contiguous (the sigmoid scores the top-k was taken on). Row b * K + s of the outputs: out_boxes [.,7] =
 * DeltaXYZWLHRBBoxCoder.decode(anchor, bbox_pred at the anchor) in the coder's order of f32 operations, out_scores [.,C] the
 * gathered scores, out_dir i64 = 1 where the second direction logit is the larger (0 without dir_cls_pred). bbox_stride /
 * dir_stride: host arrays of the (batch, channel, pixel) strides in elements. */
int gga_anchor_decode(const int64_t* inds, int B, int K, const float* anchors, int A, int n_anchors, int num_classes,
                      const float* scores, const float* bbox_pred, const int64_t* bbox_stride, const float* dir_cls_pred,
                      const int64_t* dir_stride, float* out_boxes, float* out_scores, int64_t* out_dir, void* stream);

/* ------------------------------------------------------------------------- */
/* SURVEY.md §8(f) rank 1 — inference / pseudo-label post-processing.        */
/* ------------------------------------------------------------------------- */
/* Rotated BEV IoU. Replaces mmcv.ops.box_iou_rotated as called by
 * mmdet3d/core/bbox/structures/base_box3d.py:469 (BaseInstance3DBoxes.overlaps).
 * boxes [n,5] / [m,5] = (x, y, w, h, angle[rad]); out [n,m] (or [n] when aligned);
 * mode_iof: intersection over the area of box1 instead of the union. */
int gga_box_iou_rotated(const float* boxes1, int n, const float* boxes2, int m, int mode_iof,
                        int aligned, float* out, void* stream);

/* Rotated NMS on score-sorted boxes. Replaces mmcv.ops.nms_rotated's native half as called by
 * mmdet3d/core/post_processing/box3d_nms.py:264 (nms_bev) <- centerpoint_head_gga.py:885-890;
 * like mmcv, the caller sorts by descending score. keep [n] i64 receives the positions (in the
 * sorted order) of the surviving boxes, *num_keep (device) their count (<= max_keep if > 0). */
size_t gga_nms_rotated_workspace_bytes(int n);
int gga_nms_rotated_sorted(const float* boxes_sorted, int n, float iou_threshold, int max_keep,
                           int64_t* keep, int32_t* num_keep, void* workspace,
                           size_t workspace_bytes, void* stream);
/* Circular NMS of CenterPoint (mmdet3d/core/post_processing/box3d_nms.py:181-225, test_cfg
 * nms_type='circle'): xy_sorted [n,2] f32 centres by descending score; a kept centre suppresses the
 * later ones with (dx*dx + dy*dy) <= thresh, the distance in the reference's float32 arithmetic.
 * keep / num_keep / workspace as for gga_nms_rotated_sorted (same workspace size). */
int gga_circle_nms_sorted(const float* xy_sorted, int n, double thresh, int max_keep, int64_t* keep,
                          int32_t* num_keep, void* workspace, size_t workspace_bytes, void* stream);


/* Points in rotated 3D boxes. Replaces mmcv.ops.points_in_boxes_part / points_in_boxes_all as
 * called by base_box3d.py:534,566. points [B,M,3]; boxes [B,T,7] = (x, y, z_bottom, dx, dy, dz,
 * yaw). all = 0: out [B,M] i32 index of the first box containing the point or -1;
 * all = 1: out [B,M,T] i32 flags. */
int gga_points_in_boxes(const float* points, const float* boxes, int B, int M, int T, int all,
                        int32_t* out, void* stream);

/* Detections of a whole batch in one launch: the per-(frame, task) post-processing of CenterHead_GGA.get_bboxes /
 * get_task_detections (mmdet3d/models/dense_heads/centerpoint_head_gga.py:725-934) behind CenterPointBBoxCoder.decode's
 * top-k (mmdet3d/core/bbox/coders/centerpoint_bbox_coders.py:117-229), with nms_bev -> mmcv.ops.nms_rotated
 * (mmdet3d/core/post_processing/box3d_nms.py:231-268) inside. boxes [n_tasks, n_frames, k, box_dim] = the decoded boxes
 * (x, y, z gravity centre, dx, dy, dz, yaw [, vx, vy]) of every task's k top-scored cells in descending score order, scores /
 * labels [n_tasks, n_frames, k] (labels as the coder's float class index within the task). Per frame and task: coder mask
 * (centre inside coder_range [6] inclusive, score > coder_score_threshold when has_coder_score_threshold), head threshold
 * (score >= score_threshold when > 0), rotated BEV NMS over the first pre_max_size survivors on the boxes as nms_bev sees them
 * (centre -/+ extent / 2 and back), IoU > nms_threshold suppresses, at most post_max_size kept (<= 0: no cap), range filter
 * (limit_range [6] inclusive; NULL: none); tasks concatenated in order, z moved to the bottom centre, label + class_offset[task]
 * (0 + offset when single_class[task]). out_boxes [n_frames, n_tasks * k, box_dim], out_scores / out_labels [n_frames,
 * n_tasks * k], out_count [n_frames]: frame b's detections are rows 0 .. out_count[b]. k <= 128. workspace:
 * gga_centerpoint_detect_workspace_bytes (the per-task counts between the two launches). */
size_t gga_centerpoint_detect_workspace_bytes(int n_tasks, int n_frames);
int gga_centerpoint_detect(const float* boxes, const float* scores, const float* labels, int n_tasks, int n_frames, int k,
                           int box_dim, const float* coder_range, float coder_score_threshold, int has_coder_score_threshold,
                           float score_threshold, const float* limit_range, float nms_threshold, int pre_max_size,
                           int post_max_size, const int32_t* class_offset, const int32_t* single_class, float* out_boxes,
                           float* out_scores, int32_t* out_labels, int32_t* out_count, void* workspace, size_t workspace_bytes,
                           void* stream);

/* Per-class 3D NMS of a whole batch in a fixed number of launches: the loop of FCAF3DHead._nms
 * (mmdet3d/models/dense_heads/fcaf3d_head.py: per scene, per class, mmcv's nms3d / nms3d_normal) for every (scene, class)
 * pair at once, with nothing read back in between. boxes [n,7] f32 = (x, y, z, dx, dy, dz, heading), heading 0 for an
 * axis-aligned head; scores [n, n_classes] f32; scene [n] i64, rows in any order (the rows of a scene need not be contiguous).
 * Per scene, for each class c in ascending order: the candidates are the scene's rows with scores[., c] > score_thr (strict;
 * a NaN score is no candidate), taken by descending score with ties in input order (a stable sort); greedy NMS on the BEV
 * rectangle (x, y, dx, dy, heading): a kept box suppresses every later one whose rotated IoU with it (the exact polygon overlap
 * of gga_box_iou_rotated, the same float operations as gga_nms_rotated_sorted, the earlier box first) is > iou_thr. No cap on
 * the number kept. out_row / out_class [n * n_classes] i32: the input row and the class of every kept detection, packed scene
 * by scene, within a scene class-ascending, within a class by descending score; out_count [n_scenes] i32: the detections of
 * each scene (scene s begins at the sum of the counts before it). Entries behind the last detection are not written. A row
 * whose scene lies outside [0, n_scenes) is never kept. n == 0 writes zero counts.
 * GGA_ERR_INVALID_ARG before any launch for: n < 0; n_classes outside 1..GGA_MULTICLASS_NMS_MAX_CLASSES; n_scenes outside
 * 1..2^20; n * n_classes >= 2^31; a null out_count; any other null pointer while n > 0; a workspace smaller than
 * gga_multiclass_nms3d_workspace_bytes (0 for sizes it refuses). Launches: one memset, the key kernel, rocPRIM's radix sort,
 * the segment, NMS and pack kernels - their number does not depend on n_scenes or n_classes. */
#define GGA_MULTICLASS_NMS_MAX_CLASSES 128
size_t gga_multiclass_nms3d_workspace_bytes(int64_t n, int n_classes, int n_scenes);
int gga_multiclass_nms3d(const float* boxes, const float* scores, const int64_t* scene, int64_t n, int n_classes, int n_scenes,
                         float score_thr, float iou_thr, int32_t* out_row, int32_t* out_class, int32_t* out_count,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Test-time augmentation: the head maps of all views of a batch merged per scale group in one launch. Restates the per-view
 * torch.flip / slice-assign / `+=` / `/=` sequence of mmdet3d/models/detectors/centerpoint_gga.py:123-182 (aug_test_pts).
 * A map is a contiguous f32 [n_views * n_frames, channels, H, W] tensor, view-major (view v of frame f is row v * n_frames + f);
 * dst is [n_groups * n_frames, channels, H, W]. dst[s * n_frames + f] = acc / n with acc = value(first view of group s) and
 * acc = acc + value(next view) in view order, n = the number of views of the group, a true f32 division: the bits of the
 * reference's sequence. value() undoes the view's flips: hflip reads row H-1-h, vflip reads column W-1-w (both may apply),
 * and by kind
 *     GGA_TTA_REG: hflip channel 1 <- 1 - x, vflip channel 0 <- 1 - x
 *     GGA_TTA_ROT: hflip channel 0 <- -x,    vflip channel 1 <- -x
 *     GGA_TTA_VEL: hflip channel 1 <- -x,    vflip channel 0 <- -x
 *     GGA_TTA_PLAIN (heatmap logits, height, dim, ...): mirrored only.
 * GGA_ERR_INVALID_ARG before any HIP call for: a null table; n_maps outside 1..GGA_TTA_MAX_MAPS; n_views outside
 * 1..GGA_TTA_MAX_VIEWS; n_groups outside 1..n_views; H, W or n_frames <= 0; a group index outside 0..n_groups-1; a group
 * without a view; an unknown kind; a REG / ROT / VEL map with fewer than 2 channels; a null map pointer. Rows are read and
 * written with 16-byte accesses when W is a multiple of 4 and every pointer is 16-byte aligned, else element by element. */
#define GGA_TTA_MAX_VIEWS 16
#define GGA_TTA_MAX_MAPS (GGA_MAX_TASKS * 6)
enum { GGA_TTA_PLAIN = 0, GGA_TTA_REG = 1, GGA_TTA_ROT = 2, GGA_TTA_VEL = 3 };
typedef struct {
    const float* src;
    float* dst;
    int32_t channels;
    int32_t kind;
} gga_tta_map;
typedef struct {
    int32_t n_maps, n_views, n_groups;
    int32_t group[GGA_TTA_MAX_VIEWS];     /* scale group of a view */
    int32_t hflip[GGA_TTA_MAX_VIEWS];     /* pcd_horizontal_flip (y -> -y: the map's H index) */
    int32_t vflip[GGA_TTA_MAX_VIEWS];     /* pcd_vertical_flip (x -> -x: the map's W index) */
    gga_tta_map map[GGA_TTA_MAX_MAPS];
} gga_tta_table;
int gga_tta_merge_maps(const gga_tta_table* table, int n_frames, int H, int W, void* stream);

/* Flip test-time augmentation of the mono3d detectors: the head maps of the two views of a batch merged in one launch.
 * Restates mmdet3d/models/detectors/single_stage_mono3d.py:141-181 (aug_test: torch.flip(dims=[3]) of the flipped view,
 * `1 - x` on its regression channel 0, torch.mean over the two views, the regression channels >= 6 taken from view 0) for
 * every frame of a batch. One table entry per (output group, FPN level): src is a contiguous f32 [2 * n_frames, channels, H, W]
 * map, view-major (view 0 = the unflipped image of frame f at row f, view 1 = its horizontal mirror at row n_frames + f); dst is
 * [n_frames, channels, H, W]. With a = view 0 at (h, w) and b = view 1 at (h, W - 1 - w) - the whole padded map is mirrored, as
 * torch.flip does -
 *     GGA_MONO3D_TTA_MEAN: (a + b) * 0.5 in every channel
 *     GGA_MONO3D_TTA_REG:  channel 0: (a + (1 - b)) * 0.5; channels 1..5: (a + b) * 0.5; channels >= 6: a
 * each a single rounded f32 operation per step: the bits of the reference's sequence (its mean of two values is one addition and
 * an exact halving). Entries may differ in channels, H and W; an entry is read and written with 16-byte accesses when its W is a
 * multiple of 4 and its two pointers are 16-byte aligned, else element by element. (The direction-classifier group is view 0's
 * own output and needs no entry.)
 * GGA_ERR_INVALID_ARG before any HIP call for: a null table; n_maps outside 1..GGA_MONO3D_TTA_MAX_MAPS; n_frames <= 0; a null
 * map pointer; H, W or channels <= 0; an unknown kind; a REG map with fewer than 7 channels. */
#define GGA_MONO3D_TTA_MAX_MAPS 48
enum { GGA_MONO3D_TTA_MEAN = 0, GGA_MONO3D_TTA_REG = 1 };
typedef struct {
    const float* src;
    float* dst;
    int32_t channels, H, W, kind;
} gga_mono3d_tta_map;
typedef struct {
    int32_t n_maps, n_frames;
    gga_mono3d_tta_map map[GGA_MONO3D_TTA_MAX_MAPS];
} gga_mono3d_tta_table;
int gga_mono3d_tta_merge(const gga_mono3d_tta_table* table, void* stream);

/* The tail of a whole-batch mono3d `get_bboxes`: what box3d_multiclass_nms (mmdet3d/core/post_processing/box3d_nms.py:93-127)
 * does after its per-class NMS, for every image of a batch in one launch and without a read-back. rows / classes
 * [n_rows * n_classes] i32 and counts [n_images] i32 are the packed output of gga_multiclass_nms3d (scene = image): image i's kept
 * (candidate row, class) pairs begin at the sum of the counts before it, class-ascending, by descending score within a class.
 * Per-candidate arrays: scores f32 with score_stride >= n_classes floats per row, boxes f32 [n_rows, code], dir / attr i64
 * [n_rows] (optional: null gives zeros), boxes2d f32 [n_rows, 4] (optional, together with out_boxes2d).
 * Per image: a list of at most max_per_img pairs is taken in list order; a longer one is cut to its max_per_img highest
 * scores in descending order, equal scores in list order (the reference's unstable sort leaves that order open). Outputs, fixed
 * shape: out_boxes f32 [n_images, max_per_img, code], out_scores f32, out_labels / out_dir / out_attr i32 [n_images,
 * max_per_img], out_boxes2d f32 [n_images, max_per_img, 4], out_count i32 [n_images] = min(count, max_per_img); the slots
 * behind an image's last detection are zero. A pair whose row or class lies outside its range is not gathered.
 * GGA_ERR_INVALID_ARG before any launch for: n_rows < 0; n_classes outside 1..GGA_MULTICLASS_NMS_MAX_CLASSES; n_images outside
 * 1..GGA_MONO3D_COLLECT_MAX_IMAGES; n_rows * n_classes >= 2^31; code outside 1..64; max_per_img < 1 or max_per_img * n_images >=
 * 2^24; score_stride < n_classes; a null counts or output pointer; boxes2d without out_boxes2d or the reverse; any other null
 * pointer while n_rows > 0; a workspace smaller than gga_mono3d_collect_workspace_bytes (0 for sizes it refuses). */
#define GGA_MONO3D_COLLECT_MAX_IMAGES 4096
size_t gga_mono3d_collect_workspace_bytes(int64_t n_rows, int n_classes, int n_images);
int gga_mono3d_collect(const int32_t* rows, const int32_t* classes, const int32_t* counts, int n_images, int64_t n_rows,
                       int n_classes, const float* scores, int score_stride, const float* boxes, int code, const int64_t* dir,
                       const int64_t* attr, const float* boxes2d, int max_per_img, float* out_boxes, float* out_scores,
                       int32_t* out_labels, int32_t* out_dir, int32_t* out_attr, float* out_boxes2d, int32_t* out_count,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Pseudo-label matching: image-plane IoU of every detection with the ground truths of its own
 * frame and the argmax, i.e. `calculate_iou_partly(dt_annos, gt_annos, metric=0)` followed by
 * `np.argmax(c_overlap, axis=-1)` in tools/utils_pseudo_labels_gga.py:44-59 (IoU arithmetic:
 * image_box_overlap, mmdet3d/core/evaluation/kitti_utils/eval.py:86-114, criterion -1).
 * dt_boxes [n_dt,4], gt_boxes [n_gt,4] = (x1,y1,x2,y2) f64, both concatenated over frames with
 * device offsets dt_offsets / gt_offsets [n_frames+1]. round_f32: the detections were float32
 * (the usual case: float32 predictions, float64 KITTI labels) - their own area is then float32
 * arithmetic and each overlap is rounded to float32, as the reference's typing gives. match [n_dt]: index of the first
 * maximum within the frame's ground truths (-1 if it has none); best_iou [n_dt] optional;
 * overlaps optional: frame f's [n_dt_f, n_gt_f] matrix at overlap_offsets[f]. */
int gga_image_box_match(const double* dt_boxes, const int64_t* dt_offsets, const double* gt_boxes,
                        const int64_t* gt_offsets, int n_frames, int64_t n_dt, int round_f32, int64_t* match,
                        double* best_iou, double* overlaps, const int64_t* overlap_offsets, void* stream);

/* ------------------------------------------------------------------------- */
/* KITTI AP evaluation (mmdet3d/core/evaluation/kitti_utils/eval.py,         */
/* rotate_iou.py): bbox / BEV / 3D / AOS.                                    */
/* ------------------------------------------------------------------------- */
/* Rotated overlaps of every detection with the ground truths of its own frame: `rotate_iou_gpu_eval` (rotate_iou.py:19-379)
 * and, for metric 2, `d3_box_overlap_kernel` (eval.py:123-160), as `calculate_iou_partly(dt_annos, gt_annos, metric)` calls
 * them from eval_class - only the per-frame blocks, not the part-wise (sum dt) x (sum gt) matrices. dt_boxes [n_dt,7],
 * gt_boxes [n_gt,7] f64 = location (3), dimensions (3), rotation_y in camera coordinates as the annos hold them, concatenated
 * over frames with device offsets dt_offsets / gt_offsets [n_frames+1]. metric 1: BEV IoU of columns (0, 2 / 3, 5 / 6), criterion
 * -1. metric 2: BEV intersection area x height overlap over the union volume, criterion -1. The query box is the ground truth.
 * The BEV part is float32 arithmetic on the boxes cast to float32 (the reference's kernel signature), with the operations
 * numba types float64 carried in double (kitti_eval.hip lists them). dt_f32 / gt_f32: the annos of that side were float32,
 * which decides the dtype of every operation of the height part as numpy / numba would. overlaps f32: frame f's
 * [n_dt_f, n_gt_f] matrix at overlap_offsets[f] (the layout gga_image_box_match writes for metric 0); n_overlaps = its
 * length. A frame whose offsets do not fit n_dt / n_gt / n_overlaps is not written. */
int gga_kitti_eval_overlaps(const double* dt_boxes, const int64_t* dt_offsets, int64_t n_dt, const double* gt_boxes,
                            const int64_t* gt_offsets, int64_t n_gt, int n_frames, int metric, int dt_f32, int gt_f32,
                            float* overlaps, const int64_t* overlap_offsets, int64_t n_overlaps, void* stream);

/* `compute_statistics_jit` (eval.py:163-281) for all frames and all combinations of one metric at once. A combination c
 * is a (class, difficulty) pair - row combo_cd[c] of ignored_gt [n_cd, n_gt] / ignored_dt [n_cd, n_dt] (int8: 0 counted,
 * 1 ignored, -1 other class; clean_data) - with the min overlap combo_min_overlap[c]. overlaps: the per-frame matrices
 * at overlap_offsets (f64 when overlaps_f64, as gga_image_box_match writes them, else f32), compared in float64.
 * dt_data [n_dt,6] f64 = bbox (4), alpha, score; gt_alpha [n_gt]; dc_boxes [n_dc,4] the DontCare boxes (used by metric 0
 * only) with offsets dc_offsets [n_frames+1]; dt_f32: the detections' columns were float32 (decides the rounding of the
 * detection-vs-DontCare overlap). max_dt >= the largest number of detections of one frame.
 * compute_fp = 0: the first pass of eval_class (thresh 0): tp_det [n_combos, n_gt] i32 = for every ground truth the
 *   index within its frame of the detection it was matched to as a true positive, else -1 (fill with -1 beforehand; the scores
 *   of these detections are what get_thresholds sorts).
 * compute_fp = 1: `fused_compute_statistics` (eval.py:293-340): thresholds [n_combos, 41] f64 with n_thresholds [n_combos]
 *   valid entries each; counts [n_combos, 41, 3] i64 = tp, fp, fn and similarity [n_combos, 41] f64 (the AOS sum, when
 *   compute_aos) summed over the frames. One lane per (frame, combination) walks the thresholds; the 64 frames of a wave are
 *   summed by a fixed butterfly and the waves in order by a second launch, so the result has the same bits on every run.
 * workspace: gga_kitti_eval_stats_workspace_bytes. A frame whose offsets do not fit the totals is skipped. */
size_t gga_kitti_eval_stats_workspace_bytes(int n_frames, int n_combos, int max_dt);
int gga_kitti_eval_stats(const void* overlaps, int overlaps_f64, const int64_t* overlap_offsets, int64_t n_overlaps,
                         const int64_t* dt_offsets, const int64_t* gt_offsets, const int64_t* dc_offsets,
                         const double* dt_data, int64_t n_dt, const double* gt_alpha, int64_t n_gt, const double* dc_boxes,
                         int64_t n_dc, const int8_t* ignored_gt, const int8_t* ignored_dt, int n_cd, const int32_t* combo_cd,
                         const double* combo_min_overlap, int n_combos, int n_frames, int max_dt, int metric, int dt_f32,
                         int compute_fp, int compute_aos, const double* thresholds, const int32_t* n_thresholds,
                         int32_t* tp_det, int64_t* counts, double* similarity, void* workspace, size_t workspace_bytes,
                         void* stream);

/* KITTI result formatting of a whole test run in one launch: `convert_valid_bboxes` + `bbox2result_kitti`
 * (mmdet3d/datasets/kitti_dataset_GGA_train.py:453-566,680-761) for LiDAR detections. boxes [n_dets,7] f32 (x, y, z_bottom,
 * dx, dy, dz, yaw), scores [n_dets] f32, labels [n_dets] i64, concatenated over frames with frame_offsets [n_frames+1]. Per
 * frame: lidar2cam [n_frames,4,4] f32 = R0_rect @ Tr_velo_to_cam (formed by the caller in float32), p2 [n_frames,4,4] f32,
 * image_hw [n_frames,2] i32 = (height, width). limit_range_host: the six floats of pcd_limit_range (HOST pointer).
 * Per detection, float32 in the host path's operation order: yaw limited (offset 0.5, period 2 pi), the camera box, its eight
 * corners projected by p2, the unclipped 2D box, valid = (2D box meets the image) and (bottom centre strictly inside the
 * range), the 2D box clipped to the image, alpha = -atan2(-y, x) + rotation_y.
 * out_yaw [n_dets]: the limited yaw of EVERY detection in input order (the in-place side effect of limit_yaw).
 * The valid detections of frame f are written, in their original order, to rows frame_offsets[f] ..
 * frame_offsets[f] + valid_counts[f] of out_cols [n_dets, GGA_KITTI_FORMAT_COLS] f32 = bbox (4), dimensions (3), location (3),
 * rotation_y, alpha, score, limited-yaw LiDAR box (7) and out_labels [n_dets] i64; the other rows are not written.
 * valid_counts [n_frames] i32. Any number of detections per frame, 0 included; a frame whose offsets do not fit n_dets gets
 * count 0 and nothing written. */
#define GGA_KITTI_FORMAT_COLS 20
int gga_kitti_format_dets(const float* boxes, const float* scores, const int64_t* labels, int64_t n_dets,
                          const int64_t* frame_offsets, int n_frames, const float* lidar2cam, const float* p2,
                          const int32_t* image_hw, const float* limit_range_host, float* out_cols, int64_t* out_labels,
                          float* out_yaw, int32_t* valid_counts, void* stream);

/* The camera-box variant for the image branch (mmdet3d/datasets/kitti_mono_dataset.py:302-334,497-561): boxes [n_dets,7] f32 are
 * CameraInstance3DBoxes rows (x, y_bottom, z, x_size, y_size, z_size, rotation_y). No yaw limit, no change of frame, no range
 * test: the eight corners projected by p2, valid = the unclipped 2D box meets the image (x1 < w, y1 < h, x2 > 0, y2 > 0), the
 * clip, alpha = -atan2(x, z) + rotation_y. out_cols [n_dets, GGA_KITTI_FORMAT_CAM_COLS] f32 = bbox (4), dimensions (3),
 * location (3), rotation_y, alpha, score; rows, out_labels, valid_counts and the frame_offsets rule as above. */
#define GGA_KITTI_FORMAT_CAM_COLS 13
int gga_kitti_format_dets_cam(const float* boxes, const float* scores, const int64_t* labels, int64_t n_dets,
                              const int64_t* frame_offsets, int n_frames, const float* p2, const int32_t* image_hw,
                              float* out_cols, int64_t* out_labels, int32_t* valid_counts, void* stream);

/* ------------------------------------------------------------------------- */
/* Image batch of the mono3d branch (gga_amd/image_pipelines.py).              */
/* ------------------------------------------------------------------------- */
/* One launch builds the detector's input from the uint8 sources of a whole batch. src: DEVICE buffer of src_bytes bytes that
 * holds every image as H x W x 3 uint8 at its src_offset. images_host: HOST array of n_images <= GGA_IMAGE_BATCH_MAX records
 * (checked here, then passed to the kernel by value). table: DEVICE [3,256] f32, table[c][v] = the normalised value of byte v
 * in output channel c. out: DEVICE f32, [n_images,3,out_h,out_w] (GGA_LAYOUT_NCHW) or [n_images,out_h,out_w,3]
 * (GGA_LAYOUT_NHWC), 16-byte aligned, out_w a multiple of 4; EVERY element is written (torch.empty is enough).
 * Output pixel (b, c, y, x): 0 outside dst_h x dst_w; otherwise table[c][p], p = the fixed-point bilinear sample (weights
 * of 1/2048, half-pixel centres, integers only; DESIGN.md "Image batch") of source channel c (2 - c with reverse_channels)
 * of the src_h x src_w source resized to dst_h x dst_w, at (y, x') with x' = dst_w - 1 - x when flip. dst == src reads the
 * source pixel itself. Bit-identical to image_pipelines.materialize on the host.
 * Refused before any launch: null pointers, n_images < 0 or above the maximum, an unknown layout, sizes < 1, dst larger than
 * out, an offset or extent that leaves the source buffer. n_images == 0 is a no-op. */
#define GGA_IMAGE_BATCH_MAX 64
typedef struct {
    int64_t src_offset;
    int32_t src_h, src_w, dst_h, dst_w, flip, reserved;
} gga_image_desc;
int gga_image_batch(const uint8_t* src, int64_t src_bytes, const gga_image_desc* images_host, int n_images, const float* table,
                    int reverse_channels, int out_h, int out_w, int layout, float* out, void* stream);

/* ------------------------------------------------------------------------- */
/* Indoor mAP / mAR evaluation (mmdet3d/core/evaluation/indoor_eval.py).       */
/* ------------------------------------------------------------------------- */
/* Detections and ground truths are sorted by the caller into (class, frame) segments, segment = class * n_frames + frame,
 * with device offsets det_offsets / gt_offsets [n_segments+1]; a segment may be empty on either side. Boxes [n,7] f32 =
 * (x, y, z_bottom, dx, dy, dz, yaw), the DepthInstance3DBoxes tensor with origin (0.5, 0.5, 0).
 * gga_indoor_eval_match: for every detection iou_max [n_det] f32 = the largest 3D IoU (BaseInstance3DBoxes.overlaps, mode
 * 'iou', float32: rotated BEV IoU -> BEV overlap iou2d * (a1 + a2) / (1 + iou2d), times the height overlap, over
 * max(v1 + v2 - overlap, 1e-8)) over the ground truths of its segment and jmax [n_det] i32 = the index of that ground truth
 * within the segment: the first one that reaches the maximum (eval_det_cls, `if iou > iou_max`). A segment without ground
 * truths gives -inf and -1. One thread per detection. */
int gga_indoor_eval_match(const float* det_boxes, const int64_t* det_offsets, int64_t n_det, const float* gt_boxes,
                          const int64_t* gt_offsets, int64_t n_gt, int n_segments, float* iou_max, int32_t* jmax, void* stream);

/* The TP / FP marking of eval_det_cls for n_thresholds <= GGA_INDOOR_EVAL_MAX_THRESHOLDS IoU thresholds (thresholds_host:
 * HOST pointer to 8 floats) at once. det_pos [n_det] i32: the position of each detection in the output order - class-major,
 * within a class by descending score (its class's first position + its rank in the class); positions are distinct. A
 * detection is a true positive at threshold t when iou_max > t and it has the smallest position among the detections of
 * its segment with the same jmax and iou_max > t; it is a false positive otherwise (a detection whose best ground truth is
 * taken does not fall back to another). tp [n_thresholds, n_det] u8, indexed by det_pos: 1 = TP, 0 = FP. One atomicMin per
 * (threshold, detection) and a compare pass: the result does not depend on scheduling.
 * workspace: gga_indoor_eval_workspace_bytes. */
#define GGA_INDOOR_EVAL_MAX_THRESHOLDS 8
size_t gga_indoor_eval_workspace_bytes(int64_t n_gt, int n_thresholds);
int gga_indoor_eval_assign(const float* iou_max, const int32_t* jmax, const int32_t* det_pos, const int64_t* det_offsets,
                           int64_t n_det, const int64_t* gt_offsets, int64_t n_gt, int n_segments,
                           const float* thresholds_host, int n_thresholds, uint8_t* tp, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- */
/* Offline GGA label generation primitives,             */
/* tools/data_converter/utils_gga.py. float64, reference operation order.       */
/* ------------------------------------------------------------------------- */
/* region_grow (utils_gga.py:6-38) for n_thresholds distance thresholds at once (the reference
 * calls it for thresh = 0.1 .. 0.7 with the same masks, kitti_converter_gga.py:373-381).
 * pc [n_points, dim] f64 (dim <= 4; the reference passes homogeneous camera coordinates),
 * mask_search / mask_origin [n_points] u8 (origin must be a subset of search),
 * ratio: the early-exit in-box ratio (use_ratio 0 = the reference's ratio=None).
 * out_masks [n_thresholds, n_points] u8 = mask_best * mask_origin (or mask_best for ratio None). */
size_t gga_region_grow_workspace_bytes(int64_t n_points, int n_thresholds);
int gga_region_grow(const double* pc, int64_t n_points, int dim, const uint8_t* mask_search,
                    const uint8_t* mask_origin, const double* thresholds, int n_thresholds, double ratio,
                    int use_ratio, uint8_t* out_masks, void* workspace, size_t workspace_bytes, void* stream);

/* points_in_convex_polygon_3d_jit (mmdet3d/core/bbox/box_np_ops.py:641-705) as used by
 * points_in_frustm_indices (utils_gga.py:87-100): out[i, j] = 1 iff for every surface k of
 * polyhedron j: p_i . normal_vec[j,k] + d[j,k] < 0. points [n, point_stride >= 3] f64,
 * normal_vec [n_polyhedra, n_surfaces, 3], d [n_polyhedra, n_surfaces] (surface_equ_3d). */
int gga_points_in_convex_polyhedra(const double* points, int64_t n_points, int point_stride, const double* normal_vec,
                                   const double* d, int n_polyhedra, int n_surfaces, uint8_t* out, void* stream);

/* Every point-in-polyhedron question of one frame in one pass over its raw cloud (the data preparation's per-frame point
 * stage: image frustum, ground-truth boxes, object frusta, reduced cloud).
 * points [n_points, point_stride] f32 as the velodyne file holds them (columns 0..2 = x, y, z; widened to f64 on the device,
 * which is exact), normal_vec [n_polyhedra, n_surfaces, 3] f64 and d [n_polyhedra, n_surfaces] f64 (surface_equ_3d).
 * Inside is gga_points_in_convex_polyhedra's test in its arithmetic, so every bit equals what that entry returns for the
 * same points given as f64.
 *   member         [ceil(n_polyhedra / 32), n_points] u32: bit p % 32 of word [p / 32, i] = point i inside polyhedron p;
 *                  the bits above the last polyhedron are zero
 *   counts         [n_polyhedra] i32: points inside p
 *   counts_reduced [n_polyhedra] i32: points inside p and inside reduce_poly (= counts when reduce_poly is -1)
 *   reduced        [n_points, point_stride] f32: the rows inside reduce_poly, whole and in input order (a stable compaction;
 *                  rows behind the last one are not written); not touched and may be null when reduce_poly is -1
 *   n_reduced      i32: the number of those rows (0 when reduce_poly is -1)
 * n_points == 0 returns GGA_OK and writes nothing. GGA_ERR_INVALID_ARG before any HIP call for n_points outside 0..2^21,
 * point_stride outside 3..64, n_polyhedra outside 1..256, n_surfaces < 1 or n_polyhedra * n_surfaces > 1920 (the table is
 * kept in LDS), reduce_poly outside -1..n_polyhedra-1, a null pointer while n_points > 0; GGA_ERR_WORKSPACE for a workspace
 * below gga_frame_point_tests_workspace_bytes(n_points) (0 for a refused n_points). Rows are moved with 16-byte accesses
 * when point_stride is 4 and points / reduced lie on 16-byte addresses. Launches: one memset when counts, counts_reduced
 * and n_reduced lie one behind the other (else three), the test kernel, and with a reduce_poly one single-workgroup scan
 * and the scatter. */
size_t gga_frame_point_tests_workspace_bytes(int64_t n_points);
int gga_frame_point_tests(const float* points, int64_t n_points, int point_stride, const double* normal_vec, const double* d,
                          int n_polyhedra, int n_surfaces, int reduce_poly, uint32_t* member, int32_t* counts,
                          int32_t* counts_reduced, float* reduced, int32_t* n_reduced, void* workspace,
                          size_t workspace_bytes, void* stream);

/* RANSAC scoring of calculate_ground (utils_gga.py:121-125): for every candidate plane a.p = 1,
 * counts[c] = #{ i : |p_i . plane_c - 1| / ||plane_c|| < threshold }; masks (optional)
 * [n_planes, n_points] u8 the inlier masks. */
int gga_plane_inliers(const double* points, int64_t n_points, int point_stride, const double* planes, int n_planes,
                      double threshold, int32_t* counts, uint8_t* masks, void* stream);

/* ------------------------------------------------------------------------- */
/* §8(f)4. Modulated deformable convolution (DCNv2), sampling half.           */
/* Replaces the un-vendored mmcv ModulatedDeformConv2dPack natives behind     */
/* `dcn_on_last_conv=True` of the PGD / FCOS3D heads                          */
/* (mmdet3d/models/dense_heads/anchor_free_mono3d_head.py:187-211,            */
/* configs/_base_/models/pgd.py:47). deform_groups = groups = 1.              */
/* ------------------------------------------------------------------------- */
/* x [B,H,W,C] f32 channels-last (C a multiple of 256, <= 1024); offset [B, 2*kh*kw, Ho, Wo] f32 NCHW with
 * channel 2k = vertical, 2k+1 = horizontal offset of tap k = i*kw + j (mmcv's layout); mask [B, kh*kw, Ho, Wo]
 * (already through the sigmoid). col [B*Ho*Wo, kh*kw*C] f32:
 * col[p, k, c] = mask[p,k] * bilinear(x[..,c], p*stride - pad + tap*dil + offset[p,k]); samples outside
 * (-1, H) x (-1, W) are 0, corners outside the image contribute 0. The convolution is then
 * y = col @ W[Cout, kh, kw, C]^T + bias (a library GEMM on the caller's side). */
int gga_dcn_im2col(const float* x, const float* offset, const float* mask, int B, int H, int W, int C, int kh, int kw,
                   int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, float* col, void* stream);
/* the same with one more output: the bits of the largest finite |col| written, max-combined into *amax_col (zeroed by the
 * caller; NULL: not wanted) - the scale of the two-fp16-plane matrix kernels that multiply col by the weight */
int gga_dcn_im2col_amax(const float* x, const float* offset, const float* mask, int B, int H, int W, int C, int kh, int kw,
                        int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, float* col, uint32_t* amax_col,
                        void* stream);
/* Backward of the sampling: grad_col [B*Ho*Wo, kh*kw*C] -> grad_x [B,H,W,C] (zero-filled here, float atomic
 * adds: the scatter targets are data dependent; NULL to skip), grad_offset / grad_mask in the layouts above. */
int gga_dcn_col2im(const float* x, const float* offset, const float* mask, const float* grad_col, int B, int H, int W,
                   int C, int kh, int kw, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w,
                   float* grad_x, float* grad_offset, float* grad_mask, void* stream);

/* FCOS3D / PGD target assignment (FCOSMono3DHead._get_target_single, fcos_mono3d_head.py:773-956, for the
 * whole batch in one launch). points [P,2] f32: all levels concatenated, level l = rows
 * level_begin_host[l] .. level_begin_host[l+1] (host int32 [n_levels]; the last level ends at P) with stride
 * strides_host[l] and regress range regress_ranges_host[2l], [2l+1]. Ground truths of all images concatenated,
 * image b = rows gt_offsets[b] .. gt_offsets[b+1] (device int64 [batch+1]): gt_bboxes [G,4], centers2d [G,2],
 * depths [G], gt_bboxes_3d [G,code] (yaw already made local), labels int64. Outputs [batch, P(, .)]:
 * labels, bbox_targets (l, t, r, b), labels_3d, bbox_targets_3d (dx, dy, depth, gt[3:]), centerness
 * exp(-alpha * |d| / (1.414 * stride * radius)), attr. Points with no admissible ground truth get the
 * background labels and (like the reference) the regression targets of the image's first box. */
int gga_fcos3d_targets(const float* points, int n_points, int n_levels, const int32_t* level_begin_host,
                       const float* strides_host, const float* regress_ranges_host, float center_sample_radius,
                       const int64_t* gt_offsets, int batch, const float* gt_bboxes, const float* centers2d,
                       const float* depths, const float* gt_bboxes_3d, int code_size, const int64_t* gt_labels,
                       const int64_t* gt_labels_3d, const int64_t* attr_labels, int64_t background_label,
                       int64_t attr_background_label, float centerness_alpha, int64_t* labels, float* bbox_targets,
                       int64_t* labels_3d, float* bbox_targets_3d, float* centerness_targets, int64_t* attr_targets,
                       void* stream);

/* ------------------------------------------------------------------------- */
/* Point operators of the PointNet++ family (mmcv.ops furthest_point_sample,  */
/* ball_query, grouping_operation, gather_points, three_nn, three_interpolate */
/* and QueryAndGroup, as mmdet3d/ops/pointnet_modules/point_sa_module.py and  */
/* point_fp_module.py call them). mmcv's sources are not part of the          */
/* reference tree: the definitions below ARE the contract (DESIGN.md "Point   */
/* operators"). All tensors f32 / i32, contiguous. Every squared distance is  */
/* d2 = (dx*dx + dy*dy) + dz*dz in float32, one rounding per operation, no    */
/* fused multiply-add.                                                        */
/* ------------------------------------------------------------------------- */
#define GGA_FPS_REGISTER_MAX_N 20480    /* largest N of the register path of gga_furthest_point_sample */
#define GGA_GROUP_MAX_SAMPLES 256       /* largest sample_num of gga_query_and_group, largest K of gga_group_max_* */
/* Furthest point sampling. xyz [B,N,3] -> out [B,num_points] i32; 1 <= num_points <= N. The first sample is index 0; every
 * point's running minimum starts at 1e10; each round takes min(minimum, d2 to the last sample) and picks the largest minimum,
 * the LOWEST index among equal maxima. N <= GGA_FPS_REGISTER_MAX_N keeps coordinates and minima in registers; a larger N, or
 * general != 0, takes the general path, which needs temp [B,N] f32 (any content). Both paths give the same indices. */
int gga_furthest_point_sample(const float* xyz, int B, int N, int num_points, int general, float* temp, int32_t* out,
                              void* stream);
/* Ball query. xyz [B,N,3], center_xyz [B,M,3] -> idx [B,M,sample_num] i32. Candidates in ascending index; a hit has
 * d2 < max_radius^2 and (d2 == 0 or d2 >= min_radius^2), the squares taken in float32. Slot j holds the j-th hit, every slot no
 * hit reached holds the first hit, and a centre without any hit holds index 0 everywhere (mmcv's behaviour: point 0 is then
 * grouped although it lies outside). */
int gga_ball_query(const float* xyz, const float* center_xyz, int B, int N, int M, float min_radius, float max_radius,
                   int sample_num, int32_t* idx, void* stream);
/* out[b,c,j] = features[b,c,idx[b,j]]: features [B,C,N], idx [B,J] -> out [B,C,J]. gather_points is J = M,
 * grouping_operation J = M * sample_num. The backward adds grad_out into grad_features (zeroed by the caller) with float
 * atomics. An index outside [0,N) reads as 0 and receives nothing. */
int gga_group_points_fwd(const float* features, const int32_t* idx, int B, int C, int N, int64_t J, float* out, void* stream);
int gga_group_points_bwd(const float* grad_out, const int32_t* idx, int B, int C, int N, int64_t J, float* grad_features,
                         void* stream);
/* The three nearest source points of every target point: target [B,n,3], source [B,m,3], m >= 3 -> dist [B,n,3] =
 * sqrtf(d2) ascending, idx [B,n,3]. Found with strict '<' in ascending index: the earlier index wins on ties. */
int gga_three_nn(const float* target, const float* source, int B, int n, int m, float* dist, int32_t* idx, void* stream);
/* out[b,c,i] = (w0*f[i0] + w1*f[i1]) + w2*f[i2]: features [B,C,m], idx / weight [B,n,3] -> out [B,C,n]. The backward adds
 * grad_out * w into grad_features (zeroed by the caller) with float atomics. */
int gga_three_interpolate_fwd(const float* features, const int32_t* idx, const float* weight, int B, int C, int m, int n,
                              float* out, void* stream);
int gga_three_interpolate_bwd(const float* grad_out, const int32_t* idx, const float* weight, int B, int C, int m, int n,
                              float* grad_features, void* stream);
/* QueryAndGroup in one launch: the ball query above (query != 0; idx is written) or a given idx (query == 0), then
 * out [B, (use_xyz ? 3 : 0) + C, M, sample_num] = cat((xyz[idx] - centre) [/ max_radius when normalize_xyz: a true float32
 * division], features[:, idx]). features [B,C,N] may be NULL with C = 0. sample_num <= GGA_GROUP_MAX_SAMPLES. */
int gga_query_and_group(const float* xyz, const float* center_xyz, const float* features, int B, int N, int M, int C,
                        float min_radius, float max_radius, int sample_num, int use_xyz, int normalize_xyz, int query,
                        int32_t* idx, float* out, void* stream);
/* Its backward: grad_out in the layout of out -> grad_xyz [B,N,3] and grad_features [B,C,N] (both zeroed by the caller,
 * float atomics), grad_center [B,M,3] (written). Any of the three may be NULL. */
int gga_query_and_group_bwd(const float* grad_out, const int32_t* idx, int B, int N, int M, int C, float max_radius,
                            int sample_num, int use_xyz, int normalize_xyz, float* grad_xyz, float* grad_center,
                            float* grad_features, void* stream);
/* Max pool over the samples of a group (the tail of a set abstraction level): x [B,C,M,K] f32, read through the element strides
 * (sb, sc, sm, sk) of its four dimensions (contiguous NCHW and channels-last memory alike, no copy) -> y [B,C,M] f32 and
 * arg [B,C,M] u8, both contiguous; 1 <= K <= GGA_GROUP_MAX_SAMPLES, so a position fits a byte. The definition is the scan
 * k = 0 .. K-1 from best = x[0], arg = 0 that takes x[k] when x[k] > best, or when x[k] is NaN and best is not: the lowest k
 * among equal maxima (+0 and -0 are equal), NaN at the first NaN's position for a group with a NaN, -inf at 0 for a group of
 * -inf. Strides must be non-negative. */
int gga_group_max_fwd(const float* x, int B, int C, int M, int K, int64_t sb, int64_t sc, int64_t sm, int64_t sk, float* y,
                      uint8_t* arg, void* stream);
/* Its backward: grad_x [B,C,M,K] through the same four strides, every element written exactly once (grad_y[b,c,m] at
 * k == arg[b,c,m], zero elsewhere): no memset before it, no atomics, the same bits on every run. */
int gga_group_max_bwd(const float* grad_y, const uint8_t* arg, int B, int C, int M, int K, int64_t sb, int64_t sc, int64_t sm,
                      int64_t sk, float* grad_x, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GGA_HIP_H_ */
