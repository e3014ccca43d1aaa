// All point-in-polyhedron questions of one KITTI frame in one pass over its raw float32 cloud (data preparation:
// tools/create_data_gga.py). The per-call form (label_gen.hip: points_in_polyhedra_kernel) is asked once per question - the
// image frustum, the ground-truth boxes, every object's 2D-box frustum, the reduced cloud - each time on a float64 copy of
// the cloud made and uploaded by the host. Here the file's float32 rows are read once:
//   frame_points_test_kernel     one thread per point; the P*S face equations (nx, ny, nz, d) sit in LDS; the point's
//                                membership bits are built in a register and leave as one coalesced word per 32 polyhedra;
//                                the per-polyhedron counts are summed per wavefront (ballot + popcount), per workgroup in
//                                LDS, and reach global memory as one atomic per workgroup and polyhedron;
//   frame_points_scan_kernel     exclusive scan of the workgroups' counts of points inside `reduce_poly` (one workgroup:
//                                at most 8192 counts);
//   frame_points_scatter_kernel  the rows inside `reduce_poly`, in input order, to `reduced` (a stable compaction).
// Arithmetic: a float32 coordinate widens to float64 exactly, so the face test is points_in_polyhedra_kernel's to the bit:
// s = ((x*n0 + y*n1) + z*n2) + d with every product rounded on its own (no fma), inside iff s < 0 for every face.
#include "gga_index.h"

#pragma clang fp contract(off)

#define FP_THREADS 256
#define FP_MAX_POINTS (1ll << 21)
#define FP_MAX_POLY 256
#define FP_MAX_FACES 1920          // P * S: 60 KiB of LDS for the table, 2 KiB for the counts
#define FP_MAX_STRIDE 64
#define FP_SCAN_THREADS 1024

static inline int64_t fp_blocks(int64_t n) { return (n + FP_THREADS - 1) / FP_THREADS; }

// NS: the number of faces when it is known at compile time (6: boxes and frusta - the face loop is then unrolled, so that a
// polyhedron's twelve LDS reads are in flight together; the kernel is bound by that latency), 0 = read n_surf.
template <bool ROW4, int NS>
__global__ __launch_bounds__(FP_THREADS) void frame_points_test_kernel(const float* __restrict__ pts, int n, int stride,
                                                                      const double* __restrict__ normal,
                                                                      const double* __restrict__ dconst, int n_poly, int n_surf_,
                                                                      int reduce_poly, uint32_t* __restrict__ member,
                                                                      int32_t* __restrict__ counts,
                                                                      int32_t* __restrict__ counts_reduced,
                                                                      int32_t* __restrict__ block_counts) {
    const int n_surf = NS ? NS : n_surf_;
    extern __shared__ __attribute__((aligned(32))) char fp_smem[];
    double4* table = (double4*)fp_smem;                                         // [n_poly * n_surf] (nx, ny, nz, d)
    int* cnt = (int*)(fp_smem + (size_t)n_poly * n_surf * sizeof(double4));     // [2 * n_poly]
    const int tid = threadIdx.x, lane = tid & 63;
    const int faces = n_poly * n_surf;
    for (int f = tid; f < faces; f += FP_THREADS)
        table[f] = make_double4(normal[3 * f], normal[3 * f + 1], normal[3 * f + 2], dconst[f]);
    for (int p = tid; p < 2 * n_poly; p += FP_THREADS) cnt[p] = 0;
    __syncthreads();

    const int i = blockIdx.x * FP_THREADS + tid;
    const bool valid = i < n;
    double x = 0.0, y = 0.0, z = 0.0;
    if (valid) {
        if (ROW4) {
            const float4 r = ((const float4*)pts)[i];
            x = r.x; y = r.y; z = r.z;
        } else {
            const float* r = pts + (size_t)i * stride;
            x = r[0]; y = r[1]; z = r[2];
        }
    }
    // the reduce polyhedron first: every other count is also wanted restricted to it
    bool in_red = valid;
    if (reduce_poly >= 0) {
#pragma unroll
        for (int k = 0; k < n_surf; ++k) {
            const double4 e = table[reduce_poly * n_surf + k];
            const double a = x * e.x, b = y * e.y, c = z * e.z;
            double s = a + b; s = s + c; s = s + e.w;
            in_red = in_red && !(s >= 0);
        }
    }
    uint32_t word = 0;
    for (int p = 0; p < n_poly; ++p) {
        bool in = valid;
#pragma unroll
        for (int k = 0; k < n_surf; ++k) {
            const double4 e = table[p * n_surf + k];
            const double a = x * e.x, b = y * e.y, c = z * e.z;
            double s = a + b; s = s + c; s = s + e.w;
            in = in && !(s >= 0);
        }
        word |= (in ? 1u : 0u) << (p & 31);
        const unsigned long long m = __ballot(in), mr = __ballot(in && in_red);
        if (lane == 0) {
            if (m) atomicAdd(&cnt[p], __popcll(m));
            if (mr) atomicAdd(&cnt[n_poly + p], __popcll(mr));
        }
        if ((p & 31) == 31 || p == n_poly - 1) {
            if (valid) member[(size_t)(p >> 5) * n + i] = word;
            word = 0;
        }
    }
    __syncthreads();
    for (int p = tid; p < n_poly; p += FP_THREADS) {
        if (cnt[p]) atomicAdd(&counts[p], cnt[p]);
        if (cnt[n_poly + p]) atomicAdd(&counts_reduced[p], cnt[n_poly + p]);
    }
    if (tid == 0 && reduce_poly >= 0) block_counts[blockIdx.x] = cnt[reduce_poly];
}

// block_counts [n_blocks] -> its exclusive prefix sums in place, the total to *n_reduced. One workgroup; thread t owns
// `chunk` consecutive entries.
__global__ __launch_bounds__(FP_SCAN_THREADS) void frame_points_scan_kernel(int32_t* __restrict__ block_counts, int n_blocks,
                                                                           int32_t* __restrict__ n_reduced) {
    const int tid = threadIdx.x;
    const int chunk = (n_blocks + FP_SCAN_THREADS - 1) / FP_SCAN_THREADS;
    const int b0 = min(n_blocks, tid * chunk), b1 = min(n_blocks, b0 + chunk);
    int own = 0;
    for (int b = b0; b < b1; ++b) own += block_counts[b];
    int total;
    int run = gga_block_scan<FP_SCAN_THREADS>(own, total);
    for (int b = b0; b < b1; ++b) { const int c = block_counts[b]; block_counts[b] = run; run += c; }
    if (tid == 0) *n_reduced = total;
}

template <bool ROW4>
__global__ __launch_bounds__(FP_THREADS) void frame_points_scatter_kernel(const float* __restrict__ pts, int n, int stride,
                                                                         const uint32_t* __restrict__ member_word, int bit,
                                                                         const int32_t* __restrict__ block_offsets,
                                                                         float* __restrict__ reduced) {
    const int i = blockIdx.x * FP_THREADS + threadIdx.x;
    const bool keep = i < n && ((member_word[i] >> bit) & 1u);
    int kept;
    const int dst = block_offsets[blockIdx.x] + gga_block_scan_flag<FP_THREADS>(keep, kept);
    if (!keep) return;
    if (ROW4) {
        ((float4*)reduced)[dst] = ((const float4*)pts)[i];
    } else {
        const float* src = pts + (size_t)i * stride;
        float* out = reduced + (size_t)dst * stride;
        for (int j = 0; j < stride; ++j) out[j] = src[j];
    }
}

extern "C" size_t gga_frame_point_tests_workspace_bytes(int64_t n_points) {
    if (n_points < 0 || n_points > FP_MAX_POINTS) return 0;
    return gga_align_up((size_t)fp_blocks(n_points) * sizeof(int32_t), 256);
}

extern "C" int gga_frame_point_tests(const float* points, int64_t n_points, int point_stride, const double* normal_vec,
                                     const double* d, int n_polyhedra, int n_surfaces, int reduce_poly, uint32_t* member,
                                     int32_t* counts, int32_t* counts_reduced, float* reduced, int32_t* n_reduced,
                                     void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GGA_REQUIRE(n_points >= 0 && n_points <= FP_MAX_POINTS && point_stride >= 3 && point_stride <= FP_MAX_STRIDE &&
                    n_polyhedra >= 1 && n_polyhedra <= FP_MAX_POLY && n_surfaces >= 1 &&
                    (int64_t)n_polyhedra * n_surfaces <= FP_MAX_FACES && reduce_poly >= -1 && reduce_poly < n_polyhedra,
                "gga_frame_point_tests: bad sizes (n=%lld <= 2^21, stride=%d in 3..%d, polyhedra=%d in 1..%d, surfaces=%d with "
                "polyhedra*surfaces <= %d, reduce_poly=%d in -1..polyhedra-1)",
                (long long)n_points, point_stride, FP_MAX_STRIDE, n_polyhedra, FP_MAX_POLY, n_surfaces, FP_MAX_FACES, reduce_poly);
    if (n_points == 0) return GGA_OK;          // nothing is written: the caller knows every count is zero
    GGA_REQUIRE(points && normal_vec && d && member && counts && counts_reduced && n_reduced && workspace &&
                    (reduce_poly < 0 || reduced),
                "gga_frame_point_tests: null pointer argument");
    const size_t need = gga_frame_point_tests_workspace_bytes(n_points);
    if (workspace_bytes < need) {
        gga_set_error("gga_frame_point_tests: workspace %zu B < required %zu B", workspace_bytes, need);
        return GGA_ERR_WORKSPACE;
    }
    const int n = (int)n_points, blocks = (int)fp_blocks(n_points);
    int32_t* block_counts = (int32_t*)workspace;
    if (counts_reduced == counts + n_polyhedra && n_reduced == counts_reduced + n_polyhedra) {      // one behind the other: one memset
        GGA_CHECK_HIP(hipMemsetAsync(counts, 0, ((size_t)2 * n_polyhedra + 1) * 4, stream), "frame_point_tests memset");
    } else {
        GGA_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)n_polyhedra * 4, stream), "frame_point_tests memset");
        GGA_CHECK_HIP(hipMemsetAsync(counts_reduced, 0, (size_t)n_polyhedra * 4, stream), "frame_point_tests memset");
        GGA_CHECK_HIP(hipMemsetAsync(n_reduced, 0, 4, stream), "frame_point_tests memset");
    }
    const size_t lds = (size_t)n_polyhedra * n_surfaces * sizeof(double4) + (size_t)2 * n_polyhedra * sizeof(int);
    // a whole row in one 16-byte load where the rows are 16 bytes and lie on 16-byte addresses
    const bool row4 = point_stride == 4 && ((uintptr_t)points & 15) == 0 && (reduce_poly < 0 || ((uintptr_t)reduced & 15) == 0);
#define FP_LAUNCH_TEST(ROW4_, NS_)                                                                                              \
    hipLaunchKernelGGL((frame_points_test_kernel<ROW4_, NS_>), dim3(blocks), dim3(FP_THREADS), lds, stream, points, n, point_stride, \
                       normal_vec, d, n_polyhedra, n_surfaces, reduce_poly, member, counts, counts_reduced, block_counts)
    if (n_surfaces == 6) { if (row4) FP_LAUNCH_TEST(true, 6); else FP_LAUNCH_TEST(false, 6); }
    else                 { if (row4) FP_LAUNCH_TEST(true, 0); else FP_LAUNCH_TEST(false, 0); }
#undef FP_LAUNCH_TEST
    GGA_CHECK_LAUNCH("frame_points_test_kernel");
    if (reduce_poly < 0) return GGA_OK;        // no reduced cloud: counts_reduced == counts, n_reduced == 0
    hipLaunchKernelGGL(frame_points_scan_kernel, dim3(1), dim3(FP_SCAN_THREADS), 0, stream, block_counts, blocks, n_reduced);
    GGA_CHECK_LAUNCH("frame_points_scan_kernel");
    const uint32_t* word = member + (size_t)(reduce_poly >> 5) * n;
    if (row4)
        hipLaunchKernelGGL(frame_points_scatter_kernel<true>, dim3(blocks), dim3(FP_THREADS), 0, stream, points, n, point_stride,
                           word, reduce_poly & 31, block_counts, reduced);
    else
        hipLaunchKernelGGL(frame_points_scatter_kernel<false>, dim3(blocks), dim3(FP_THREADS), 0, stream, points, n, point_stride,
                           word, reduce_poly & 31, block_counts, reduced);
    GGA_CHECK_LAUNCH("frame_points_scatter_kernel");
    return GGA_OK;
}
