// The PointNet++ point operators (mmcv.ops furthest_point_sample, ball_query, grouping_operation, gather_points, three_nn,
// three_interpolate, and QueryAndGroup as one launch) for gfx950. Contracts: include/gga_hip.h "Point operators"; the
// definitions and tie rules are restated in DESIGN.md "Point operators". Compiled with -ffp-contract=off: every squared
// distance is (dx*dx + dy*dy) + dz*dz with one rounding per operation, so indices can be compared bit for bit.
#include "gga_common.h"

__device__ __forceinline__ float pn2_d2(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// ------------------------------------------------------------------------------ furthest point sampling
// One 1024-thread workgroup per cloud: the rounds are one dependent chain. A candidate is the 64-bit key
// (bits of its running minimum) << 32 | ~index: minima are >= +0, so keys order like (minimum, then lower index), and the keys
// of a cloud are distinct. Per round: every thread folds the last sample into its points' minima and keeps its best key with
// that point's coordinates; a wave64 butterfly finds the wave's best key, whose owner lane publishes key and coordinates in
// LDS; after ONE barrier every thread reads the 16 wave entries and knows the new sample. Two alternating slot sets make the
// single barrier enough: a wave can be at most one round ahead of the slowest, so it never writes a set still being read.
#define FPS_THREADS 1024
#define FPS_WAVES (FPS_THREADS / GGA_WAVE)
struct FpsSlot {
    unsigned long long key;
    float x, y, z, pad;
};

__device__ __forceinline__ unsigned long long fps_key(float minimum, int index) {
    return ((unsigned long long)__float_as_uint(minimum) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)index);
}

// -> the new sample's index, its coordinates in (lx, ly, lz)
__device__ __forceinline__ int fps_pick(unsigned long long key, float bx, float by, float bz, FpsSlot* slots, float& lx,
                                        float& ly, float& lz) {
    unsigned long long best = key;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_xor(best, o, 64);
        best = t > best ? t : best;
    }
    if (key == best) {
        FpsSlot s;
        s.key = key; s.x = bx; s.y = by; s.z = bz; s.pad = 0.f;
        slots[threadIdx.x >> 6] = s;
    }
    __syncthreads();
    int w = 0;
    best = slots[0].key;
#pragma unroll 2
    for (int i = 1; i < FPS_WAVES; ++i) {
        const unsigned long long t = slots[i].key;
        if (t > best) { best = t; w = i; }
    }
    lx = slots[w].x; ly = slots[w].y; lz = slots[w].z;
    return (int)(0xFFFFFFFFu - (uint32_t)(best & 0xFFFFFFFFull));
}

// Register path: thread t owns points t, t + 1024, ... (PPT of them) with coordinates and running minima in registers for
// the whole call. A slot past N holds minimum +0 and a higher index than any real point, so it never wins.
template <int PPT>
__global__ __launch_bounds__(FPS_THREADS) void fps_reg_kernel(const float* __restrict__ xyz, int N, int num_points,
                                                              int32_t* __restrict__ out) {
    __shared__ FpsSlot slots[2][FPS_WAVES];
    const int t = threadIdx.x;
    const float* p = xyz + (int64_t)blockIdx.x * N * 3;
    int32_t* o = out + (int64_t)blockIdx.x * num_points;
    float px[PPT], py[PPT], pz[PPT], mn[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int i = t + k * FPS_THREADS;
        const bool in = i < N;
        px[k] = in ? p[(int64_t)i * 3] : 0.f;
        py[k] = in ? p[(int64_t)i * 3 + 1] : 0.f;
        pz[k] = in ? p[(int64_t)i * 3 + 2] : 0.f;
        mn[k] = in ? 1e10f : 0.f;
    }
    float lx = p[0], ly = p[1], lz = p[2];
    if (t == 0) o[0] = 0;
    for (int j = 1; j < num_points; ++j) {
        // strict '>' in ascending k keeps the thread's lowest index among equal minima; the key is built once, for the best
        float bm = -1.f, bx = 0.f, by = 0.f, bz = 0.f;
        int bk = 0;
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const float d = pn2_d2(px[k], py[k], pz[k], lx, ly, lz);
            const float m = d < mn[k] ? d : mn[k];
            mn[k] = m;
            if (m > bm) { bm = m; bk = k; bx = px[k]; by = py[k]; bz = pz[k]; }
        }
        const int last = fps_pick(fps_key(bm, t + bk * FPS_THREADS), bx, by, bz, slots[j & 1], lx, ly, lz);
        if (t == 0) o[j] = last;
    }
}

// General path, any N: the running minima live in `temp` [B, N] and the coordinates are read again every round. A thread
// without a point (t >= N) offers the key of a slot past N with minimum +0, as the register path does.
__global__ __launch_bounds__(FPS_THREADS) void fps_general_kernel(const float* __restrict__ xyz, int N, int num_points,
                                                                  float* __restrict__ temp, int32_t* __restrict__ out) {
    __shared__ FpsSlot slots[2][FPS_WAVES];
    const int t = threadIdx.x;
    const float* p = xyz + (int64_t)blockIdx.x * N * 3;
    float* mins = temp + (int64_t)blockIdx.x * N;
    int32_t* o = out + (int64_t)blockIdx.x * num_points;
    float lx = p[0], ly = p[1], lz = p[2];
    if (t == 0) o[0] = 0;
    for (int j = 1; j < num_points; ++j) {
        unsigned long long key = fps_key(0.f, 0x7FFFFFFF);
        float bx = 0.f, by = 0.f, bz = 0.f;
        for (int i = t; i < N; i += FPS_THREADS) {
            const float x = p[(int64_t)i * 3], y = p[(int64_t)i * 3 + 1], z = p[(int64_t)i * 3 + 2];
            const float before = j == 1 ? 1e10f : mins[i];
            const float d = pn2_d2(x, y, z, lx, ly, lz);
            const float m = d < before ? d : before;
            mins[i] = m;
            const unsigned long long kk = fps_key(m, i);
            if (kk > key) { key = kk; bx = x; by = y; bz = z; }
        }
        // every thread offers a distinct key: the placeholder of a thread without a better point is made unique by its lane
        if (key == fps_key(0.f, 0x7FFFFFFF)) key -= (unsigned)t;
        const int last = fps_pick(key, bx, by, bz, slots[j & 1], lx, ly, lz);
        if (t == 0) o[j] = last;
    }
}

extern "C" int gga_furthest_point_sample(const float* xyz, int B, int N, int num_points, int general, float* temp,
                                         int32_t* out, void* stream) {
    GGA_REQUIRE(B >= 1 && N >= 1 && num_points >= 1, "gga_furthest_point_sample: bad sizes (B %d, N %d, num_points %d)", B, N,
                num_points);
    GGA_REQUIRE(num_points <= N, "gga_furthest_point_sample: num_points %d > N %d", num_points, N);
    GGA_REQUIRE(N <= 0x3FFFFFFF, "gga_furthest_point_sample: N %d too large", N);
    GGA_REQUIRE(xyz && out, "gga_furthest_point_sample: null pointer argument");
    const bool gen = general || N > GGA_FPS_REGISTER_MAX_N;
    GGA_REQUIRE(!gen || temp, "gga_furthest_point_sample: the general path (N > %d, or forced) needs temp [B, N]",
                GGA_FPS_REGISTER_MAX_N);
    hipStream_t s = (hipStream_t)stream;
    if (gen)
        hipLaunchKernelGGL(fps_general_kernel, dim3(B), dim3(FPS_THREADS), 0, s, xyz, N, num_points, temp, out);
    else if (N <= FPS_THREADS)
        hipLaunchKernelGGL(fps_reg_kernel<1>, dim3(B), dim3(FPS_THREADS), 0, s, xyz, N, num_points, out);
    else if (N <= 4 * FPS_THREADS)
        hipLaunchKernelGGL(fps_reg_kernel<4>, dim3(B), dim3(FPS_THREADS), 0, s, xyz, N, num_points, out);
    else
        hipLaunchKernelGGL(fps_reg_kernel<GGA_FPS_REGISTER_MAX_N / FPS_THREADS>, dim3(B), dim3(FPS_THREADS), 0, s, xyz, N,
                           num_points, out);
    GGA_CHECK_LAUNCH("fps_kernel");
    return GGA_OK;
}

// ------------------------------------------------------------------------------ ball query
// One wave per centre keeps the index order: 64 candidates per step, a ballot of the hits, the slot of a hit = hits so far +
// the hits on lower lanes, and the scan ends once sample_num hits are in. Slots no hit reached take the first hit (index 0
// when there is none, as mmcv leaves them). `slots` may be global or LDS memory.
#define PN2_CENTRES 4       // centres (waves) per 256-thread workgroup

__device__ __forceinline__ void ball_query_wave(const float* __restrict__ p, int N, float cx, float cy, float cz, float r2min,
                                                float r2max, int K, int* slots, int lane) {
    int cnt = 0, first = 0;
    for (int c0 = 0; c0 < N && cnt < K; c0 += GGA_WAVE) {
        const int i = c0 + lane;
        bool hit = false;
        if (i < N) {
            const float d = pn2_d2(cx, cy, cz, p[(int64_t)i * 3], p[(int64_t)i * 3 + 1], p[(int64_t)i * 3 + 2]);
            hit = d < r2max && (d == 0.f || d >= r2min);
        }
        const unsigned long long mask = __ballot(hit);
        if (mask) {
            if (cnt == 0) first = c0 + __ffsll((long long)mask) - 1;
            const int slot = cnt + __popcll(mask & ((1ull << lane) - 1ull));
            if (hit && slot < K) slots[slot] = i;
            cnt += __popcll(mask);
        }
    }
    cnt = cnt < K ? cnt : K;
    for (int l = cnt + lane; l < K; l += GGA_WAVE) slots[l] = first;
}

__global__ __launch_bounds__(256) void ball_query_kernel(const float* __restrict__ xyz, const float* __restrict__ centre, int N,
                                                         int M, float r2min, float r2max, int K, int32_t* __restrict__ idx) {
    const int lane = threadIdx.x & 63, b = blockIdx.y, m = blockIdx.x * PN2_CENTRES + (threadIdx.x >> 6);
    if (m >= M) return;
    const float* c = centre + ((int64_t)b * M + m) * 3;
    ball_query_wave(xyz + (int64_t)b * N * 3, N, c[0], c[1], c[2], r2min, r2max, K, idx + ((int64_t)b * M + m) * K, lane);
}

static int pn2_radii(const char* name, float min_radius, float max_radius, float* r2min, float* r2max) {
    GGA_REQUIRE(min_radius >= 0.f && max_radius >= 0.f, "%s: negative radius", name);
    *r2min = min_radius * min_radius;
    *r2max = max_radius * max_radius;
    return GGA_OK;
}

extern "C" int gga_ball_query(const float* xyz, const float* center_xyz, int B, int N, int M, float min_radius,
                              float max_radius, int sample_num, int32_t* idx, void* stream) {
    GGA_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && M >= 0, "gga_ball_query: bad sizes (B %d, N %d, M %d)", B, N, M);
    GGA_REQUIRE(sample_num >= 1, "gga_ball_query: sample_num %d < 1", sample_num);
    GGA_REQUIRE(N <= 0x3FFFFFFF, "gga_ball_query: N %d too large", N);
    float r2min, r2max;
    if (int rc = pn2_radii("gga_ball_query", min_radius, max_radius, &r2min, &r2max)) return rc;
    if (M == 0) return GGA_OK;
    GGA_REQUIRE(xyz && center_xyz && idx, "gga_ball_query: null pointer argument");
    hipLaunchKernelGGL(ball_query_kernel, dim3((M + PN2_CENTRES - 1) / PN2_CENTRES, B), dim3(256), 0, (hipStream_t)stream, xyz,
                       center_xyz, N, M, r2min, r2max, sample_num, idx);
    GGA_CHECK_LAUNCH("ball_query_kernel");
    return GGA_OK;
}

// ------------------------------------------------------------------------------ gather / grouping
// out[b, c, j] = features[b, c, idx[b, j]]: gather_points with J = M, grouping_operation with J = M * K. An index outside
// [0, N) reads as zero and receives no gradient (no access leaves the buffers).
__global__ __launch_bounds__(256) void gather_fwd_kernel(const float* __restrict__ feat, const int32_t* __restrict__ idx,
                                                         int C, int N, int64_t J, int64_t total, float* __restrict__ out) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t bc = e / J, j = e - bc * J;
        const int i = idx[(bc / C) * J + j];
        out[e] = (unsigned)i < (unsigned)N ? feat[bc * N + i] : 0.f;
    }
}

// `gout` may be a channel range of a wider tensor: [B, c_total, J] with this call's C channels starting at c_off.
__global__ __launch_bounds__(256) void gather_bwd_kernel(const float* __restrict__ gout, const int32_t* __restrict__ idx, int C,
                                                         int c_total, int c_off, int N, int64_t J, int64_t total,
                                                         float* __restrict__ gfeat) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t bc = e / J, j = e - bc * J, b = bc / C;
        const int i = idx[b * J + j];
        if ((unsigned)i < (unsigned)N) atomicAdd(gfeat + bc * N + i, gout[((b * c_total + c_off) + (bc - b * C)) * J + j]);
    }
}

static inline int pn2_blocks(int64_t total) {
    const int64_t b = (total + 255) / 256;
    return (int)(b < 16384 ? b : 16384);
}

static int pn2_gather(const char* name, const float* src, const int32_t* idx, int B, int C, int N, int64_t J, float* dst,
                      int backward, void* stream) {
    GGA_REQUIRE(B >= 1 && C >= 0 && N >= 1 && J >= 0, "%s: bad sizes (B %d, C %d, N %d, J %lld)", name, B, C, N, (long long)J);
    const int64_t total = (int64_t)B * C * J;
    if (total == 0) return GGA_OK;
    GGA_REQUIRE(src && idx && dst, "%s: null pointer argument", name);
    if (backward)
        hipLaunchKernelGGL(gather_bwd_kernel, dim3(pn2_blocks(total)), dim3(256), 0, (hipStream_t)stream, src, idx, C, C, 0, N,
                           J, total, dst);
    else
        hipLaunchKernelGGL(gather_fwd_kernel, dim3(pn2_blocks(total)), dim3(256), 0, (hipStream_t)stream, src, idx, C, N, J,
                           total, dst);
    GGA_CHECK_LAUNCH(name);
    return GGA_OK;
}

extern "C" int gga_group_points_fwd(const float* features, const int32_t* idx, int B, int C, int N, int64_t J, float* out,
                                    void* stream) {
    return pn2_gather("gga_group_points_fwd", features, idx, B, C, N, J, out, 0, stream);
}

extern "C" int gga_group_points_bwd(const float* grad_out, const int32_t* idx, int B, int C, int N, int64_t J,
                                    float* grad_features, void* stream) {
    return pn2_gather("gga_group_points_bwd", grad_out, idx, B, C, N, J, grad_features, 1, stream);
}

// ------------------------------------------------------------------------------ three nearest neighbours
// One thread per target point; the source points pass through LDS 256 at a time. Strict '<' in ascending index: of equal
// distances the earlier index stays in front.
__global__ __launch_bounds__(256) void three_nn_kernel(const float* __restrict__ target, const float* __restrict__ source, int n,
                                                       int m, float* __restrict__ dist, int32_t* __restrict__ idx) {
    __shared__ float s[256 * 3];
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const float* src = source + (int64_t)b * m * 3;
    float tx = 0.f, ty = 0.f, tz = 0.f;
    if (i < n) {
        const float* t = target + ((int64_t)b * n + i) * 3;
        tx = t[0]; ty = t[1]; tz = t[2];
    }
    float d0 = INFINITY, d1 = INFINITY, d2 = INFINITY;
    int i0 = 0, i1 = 0, i2 = 0;
    for (int k0 = 0; k0 < m; k0 += 256) {
        const int cnt = min(256, m - k0);
        __syncthreads();
        for (int e = threadIdx.x; e < cnt * 3; e += 256) s[e] = src[(int64_t)k0 * 3 + e];
        __syncthreads();
        for (int k = 0; k < cnt; ++k) {
            const float d = pn2_d2(tx, ty, tz, s[k * 3], s[k * 3 + 1], s[k * 3 + 2]);
            if (d < d0) { d2 = d1; i2 = i1; d1 = d0; i1 = i0; d0 = d; i0 = k0 + k; }
            else if (d < d1) { d2 = d1; i2 = i1; d1 = d; i1 = k0 + k; }
            else if (d < d2) { d2 = d; i2 = k0 + k; }
        }
    }
    if (i < n) {
        float* dd = dist + ((int64_t)b * n + i) * 3;
        int32_t* ii = idx + ((int64_t)b * n + i) * 3;
        // sqrtf correctly rounded: the float64 root rounded to float32 is (53 >= 2 * 24 + 2 bits), whatever the build makes
        // of the float32 one (__fsqrt_rn is the hardware's approximate root here)
        dd[0] = (float)sqrt((double)d0); dd[1] = (float)sqrt((double)d1); dd[2] = (float)sqrt((double)d2);
        ii[0] = i0; ii[1] = i1; ii[2] = i2;
    }
}

extern "C" int gga_three_nn(const float* target, const float* source, int B, int n, int m, float* dist, int32_t* idx,
                            void* stream) {
    GGA_REQUIRE(B >= 1 && B <= 65535 && n >= 0 && m >= 0, "gga_three_nn: bad sizes (B %d, n %d, m %d)", B, n, m);
    GGA_REQUIRE(m >= 3, "gga_three_nn: m %d < 3 source points", m);
    if (n == 0) return GGA_OK;
    GGA_REQUIRE(target && source && dist && idx, "gga_three_nn: null pointer argument");
    hipLaunchKernelGGL(three_nn_kernel, dim3((n + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, target, source, n, m, dist,
                       idx);
    GGA_CHECK_LAUNCH("three_nn_kernel");
    return GGA_OK;
}

// ------------------------------------------------------------------------------ three_interpolate
__global__ __launch_bounds__(256) void three_interpolate_fwd_kernel(const float* __restrict__ feat, const int32_t* __restrict__ idx,
                                                                    const float* __restrict__ weight, int C, int m, int n,
                                                                    int64_t total, float* __restrict__ out) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t bc = e / n, i = e - bc * n, q = ((bc / C) * n + i) * 3;
        const float* f = feat + bc * m;
        float v[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int s = idx[q + k];
            v[k] = (unsigned)s < (unsigned)m ? weight[q + k] * f[s] : 0.f;
        }
        out[e] = (v[0] + v[1]) + v[2];
    }
}

__global__ __launch_bounds__(256) void three_interpolate_bwd_kernel(const float* __restrict__ gout, const int32_t* __restrict__ idx,
                                                                    const float* __restrict__ weight, int C, int m, int n,
                                                                    int64_t total, float* __restrict__ gfeat) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t bc = e / n, i = e - bc * n, q = ((bc / C) * n + i) * 3;
        const float g = gout[e];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int s = idx[q + k];
            if ((unsigned)s < (unsigned)m) atomicAdd(gfeat + bc * m + s, g * weight[q + k]);
        }
    }
}

static int pn2_interpolate(const char* name, const float* src, const int32_t* idx, const float* weight, int B, int C, int m, int n,
                           float* dst, int backward, void* stream) {
    GGA_REQUIRE(B >= 1 && C >= 0 && m >= 1 && n >= 0, "%s: bad sizes (B %d, C %d, m %d, n %d)", name, B, C, m, n);
    const int64_t total = (int64_t)B * C * n;
    if (total == 0) return GGA_OK;
    GGA_REQUIRE(src && idx && weight && dst, "%s: null pointer argument", name);
    if (backward)
        hipLaunchKernelGGL(three_interpolate_bwd_kernel, dim3(pn2_blocks(total)), dim3(256), 0, (hipStream_t)stream, src, idx,
                           weight, C, m, n, total, dst);
    else
        hipLaunchKernelGGL(three_interpolate_fwd_kernel, dim3(pn2_blocks(total)), dim3(256), 0, (hipStream_t)stream, src, idx,
                           weight, C, m, n, total, dst);
    GGA_CHECK_LAUNCH(name);
    return GGA_OK;
}

extern "C" int gga_three_interpolate_fwd(const float* features, const int32_t* idx, const float* weight, int B, int C, int m,
                                         int n, float* out, void* stream) {
    return pn2_interpolate("gga_three_interpolate_fwd", features, idx, weight, B, C, m, n, out, 0, stream);
}

extern "C" int gga_three_interpolate_bwd(const float* grad_out, const int32_t* idx, const float* weight, int B, int C, int m,
                                         int n, float* grad_features, void* stream) {
    return pn2_interpolate("gga_three_interpolate_bwd", grad_out, idx, weight, B, C, m, n, grad_features, 1, stream);
}

// ------------------------------------------------------------------------------ QueryAndGroup in one launch
// One wave per centre: the ball query leaves the group's indices in LDS (and in `idx`), then the wave writes the group's
// (channel, sample) plane: (xyz[i] - centre) [/ norm_radius, a true division] for the three coordinate channels when use_xyz,
// features[c][i] for the rest. query = 0 takes `idx` as given instead.
__global__ __launch_bounds__(256) void query_and_group_kernel(const float* __restrict__ xyz, const float* __restrict__ centre,
                                                              const float* __restrict__ feat, int N, int M, int C, int K,
                                                              float r2min, float r2max, float norm_radius, int use_xyz, int query,
                                                              int32_t* __restrict__ idx, float* __restrict__ out) {
    __shared__ int sidx[PN2_CENTRES][GGA_GROUP_MAX_SAMPLES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.y, m = blockIdx.x * PN2_CENTRES + w;
    const bool live = m < M;
    const float* p = xyz + (int64_t)b * N * 3;
    int32_t* gi = idx + ((int64_t)b * M + (live ? m : 0)) * K;
    float c[3] = {0.f, 0.f, 0.f};
    if (live) {
        const float* q = centre + ((int64_t)b * M + m) * 3;
        c[0] = q[0]; c[1] = q[1]; c[2] = q[2];
        if (query)
            ball_query_wave(p, N, c[0], c[1], c[2], r2min, r2max, K, sidx[w], lane);
        else
            for (int l = lane; l < K; l += GGA_WAVE) sidx[w][l] = gi[l];
    }
    __syncthreads();
    if (!live) return;
    if (query)
        for (int l = lane; l < K; l += GGA_WAVE) gi[l] = sidx[w][l];
    const int X = use_xyz ? 3 : 0, CH = X + C;
    for (int e = lane; e < CH * K; e += GGA_WAVE) {
        const int ch = e / K, l = e - ch * K, i = sidx[w][l];
        float v = 0.f;
        if ((unsigned)i < (unsigned)N) {
            if (ch < X) {
                v = p[(int64_t)i * 3 + ch] - (ch == 0 ? c[0] : ch == 1 ? c[1] : c[2]);
                if (norm_radius > 0.f) v = __fdiv_rn(v, norm_radius);
            } else {
                v = feat[((int64_t)b * C + (ch - X)) * N + i];
            }
        }
        out[(((int64_t)b * CH + ch) * M + m) * K + l] = v;
    }
}

// Backward of the above, coordinate channels: points take their group entries back by float atomics (a point sits in many
// groups); a centre's gradient is minus the sum over its own group, summed in the wave. The feature channels go through
// gather_bwd_kernel, whose lanes run along one channel's (centre, sample) entries: atomics of a wave land in one feature row.
__global__ __launch_bounds__(256) void query_and_group_bwd_kernel(const float* __restrict__ gout, const int32_t* __restrict__ idx,
                                                                  int N, int M, int C, int K, float norm_radius,
                                                                  float* __restrict__ gxyz, float* __restrict__ gcentre) {
    const int lane = threadIdx.x & 63, b = blockIdx.y, m = blockIdx.x * PN2_CENTRES + (threadIdx.x >> 6);
    if (m >= M) return;
    const int32_t* gi = idx + ((int64_t)b * M + m) * K;
    const int CH = 3 + C;
    for (int ch = 0; ch < 3; ++ch) {
        float acc = 0.f;
        for (int l = lane; l < K; l += GGA_WAVE) {
            const int i = gi[l];
            if ((unsigned)i >= (unsigned)N) continue;
            float t = gout[(((int64_t)b * CH + ch) * M + m) * K + l];
            if (norm_radius > 0.f) t = __fdiv_rn(t, norm_radius);
            if (gxyz) atomicAdd(gxyz + ((int64_t)b * N + i) * 3 + ch, t);
            acc += t;
        }
        acc = wave_sum(acc);
        if (gcentre && lane == 0) gcentre[((int64_t)b * M + m) * 3 + ch] = -acc;
    }
}

extern "C" int gga_query_and_group(const float* xyz, const float* center_xyz, const float* features, int B, int N, int M, int C,
                                   float min_radius, float max_radius, int sample_num, int use_xyz, int normalize_xyz, int query,
                                   int32_t* idx, float* out, void* stream) {
    GGA_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && M >= 0 && C >= 0, "gga_query_and_group: bad sizes (B %d, N %d, M %d, C %d)", B,
                N, M, C);
    GGA_REQUIRE(sample_num >= 1 && sample_num <= GGA_GROUP_MAX_SAMPLES, "gga_query_and_group: sample_num %d not in 1..%d",
                sample_num, GGA_GROUP_MAX_SAMPLES);
    GGA_REQUIRE(N <= 0x3FFFFFFF, "gga_query_and_group: N %d too large", N);
    GGA_REQUIRE(use_xyz || C > 0, "gga_query_and_group: neither coordinates nor features to group");
    GGA_REQUIRE((int64_t)(C + 3) * sample_num <= 0x7FFFFFFF, "gga_query_and_group: C * sample_num too large");
    float r2min, r2max;
    if (int rc = pn2_radii("gga_query_and_group", min_radius, max_radius, &r2min, &r2max)) return rc;
    GGA_REQUIRE(!normalize_xyz || max_radius > 0.f, "gga_query_and_group: normalize_xyz needs max_radius > 0");
    if (M == 0) return GGA_OK;
    GGA_REQUIRE(xyz && center_xyz && idx && out && (C == 0 || features), "gga_query_and_group: null pointer argument");
    hipLaunchKernelGGL(query_and_group_kernel, dim3((M + PN2_CENTRES - 1) / PN2_CENTRES, B), dim3(256), 0, (hipStream_t)stream,
                       xyz, center_xyz, features, N, M, C, sample_num, r2min, r2max, normalize_xyz ? max_radius : 0.f, use_xyz,
                       query, idx, out);
    GGA_CHECK_LAUNCH("query_and_group_kernel");
    return GGA_OK;
}

extern "C" int gga_query_and_group_bwd(const float* grad_out, const int32_t* idx, int B, int N, int M, int C, float max_radius,
                                       int sample_num, int use_xyz, int normalize_xyz, float* grad_xyz, float* grad_center,
                                       float* grad_features, void* stream) {
    GGA_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && M >= 0 && C >= 0, "gga_query_and_group_bwd: bad sizes (B %d, N %d, M %d, C %d)",
                B, N, M, C);
    GGA_REQUIRE(sample_num >= 1, "gga_query_and_group_bwd: sample_num %d < 1", sample_num);
    GGA_REQUIRE((int64_t)(C + 3) * sample_num <= 0x7FFFFFFF, "gga_query_and_group_bwd: C * sample_num too large");
    GGA_REQUIRE(!normalize_xyz || max_radius > 0.f, "gga_query_and_group_bwd: normalize_xyz needs max_radius > 0");
    GGA_REQUIRE(grad_xyz || grad_center || grad_features, "gga_query_and_group_bwd: no gradient asked for");
    GGA_REQUIRE(use_xyz || !(grad_xyz || grad_center), "gga_query_and_group_bwd: coordinate gradients without use_xyz");
    GGA_REQUIRE(C > 0 || !grad_features, "gga_query_and_group_bwd: feature gradient with C = 0");
    if (M == 0) return GGA_OK;
    GGA_REQUIRE(grad_out && idx, "gga_query_and_group_bwd: null pointer argument");
    if (grad_xyz || grad_center) {
        hipLaunchKernelGGL(query_and_group_bwd_kernel, dim3((M + PN2_CENTRES - 1) / PN2_CENTRES, B), dim3(256), 0,
                           (hipStream_t)stream, grad_out, idx, N, M, C, sample_num, normalize_xyz ? max_radius : 0.f, grad_xyz,
                           grad_center);
        GGA_CHECK_LAUNCH("query_and_group_bwd_kernel");
    }
    if (grad_features) {
        const int X = use_xyz ? 3 : 0;
        const int64_t J = (int64_t)M * sample_num, total = (int64_t)B * C * J;
        hipLaunchKernelGGL(gather_bwd_kernel, dim3(pn2_blocks(total)), dim3(256), 0, (hipStream_t)stream, grad_out, idx, C, X + C, X,
                           N, J, total, grad_features);
        GGA_CHECK_LAUNCH("gather_bwd_kernel");
    }
    return GGA_OK;
}

// ------------------------------------------------------------------------------ group max pool
// y[b,c,m] = max over k of x[b,c,m,k], arg = its position, by the scan of include/gga_hip.h: from (x[0], 0), x[k] replaces the
// best when x[k] > best, or when x[k] is NaN and the best is not. gmax_better orders (value, position) pairs so that any
// reduction tree gives that scan's answer: a NaN beats every number, of two NaNs or two equal values (+0 == -0) the lower
// position wins. Positions of a group are distinct, so the order is total; the filler (-inf, K) of a lane without an element
// loses to every element. x and gx are addressed through the caller's element strides, in 64-bit arithmetic.
// Two lane layouts, both correct for any strides, each coalesced for one memory format:
//   _k_: L = min(64, the power of two >= K) lanes scan one group along k (contiguous k: NCHW). A wave takes 64 consecutive
//        groups, 64 / L of them per step, and hands every result to the lane of its group, so y and arg leave as one store.
//        The forward has a form with four samples per lane (one 16 B load, L from K / 4) for 16 B aligned groups: the
//        one-sample form is bound by its compare and shuffle instructions, not by memory (1.4 TB/s at K = 64).
//   _c_: lanes along 64 channels (contiguous channels: channels-last), a workgroup pools a 64 channel x 16 centre tile and
//        turns it through LDS (rows padded by a word: the column writes and the row reads are conflict-free), so the
//        [B, C, M] store runs along m.
#define GMAX_TILE 64         // channels of a tile of the _c_ kernels
#define GMAX_TILE_M 16       // centres of a tile: four per wave. Small on purpose: the pool shapes of a VoteNet step give 512 to
                             // 8192 workgroups, several rounds over the chip, where 64-centre tiles left 128 to 2048

__device__ __forceinline__ bool gmax_better(float v, int k, float bv, int bk) {
    const bool vn = v != v, bn = bv != bv;
    if (vn || bn) return vn && (!bn || k < bk);
    return v > bv || (v == bv && k < bk);
}

// element offset of group g = (b * C + c) * M + m, or -1 past the end
__device__ __forceinline__ int64_t gmax_base(int64_t g, int64_t groups, int C, int M, int64_t sb, int64_t sc, int64_t sm) {
    if (g >= groups) return -1;
    const int64_t bc = g / M, m = g - bc * M, b = bc / C, c = bc - b * C;
    return b * sb + c * sc + m * sm;
}

template <int L, int V>
__global__ __launch_bounds__(256) void group_max_fwd_k_kernel(const float* __restrict__ x, int C, int M, int K, int64_t sb,
                                                              int64_t sc, int64_t sm, int64_t sk, int64_t groups,
                                                              float* __restrict__ y, uint8_t* __restrict__ arg) {
    constexpr int G = GGA_WAVE / L, U = L >= 4 ? 4 : L;
    const int lane = threadIdx.x & 63, sub = lane / L, l = lane % L;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), step = (int64_t)gridDim.x * 4 * GGA_WAVE;
    for (int64_t g0 = wave * GGA_WAVE; g0 < groups; g0 += step) {
        const int64_t g = g0 + lane;
        const long long base = gmax_base(g, groups, C, M, sb, sc, sm);
        float rv = 0.f;
        int rk = 0;
#pragma unroll U
        for (int j = 0; j < L; ++j) {
            const long long gb = __shfl(base, j * G + sub, 64);      // the group this sub-wave scans in step j
            float bv = -INFINITY;
            int bk = K;
            if (gb >= 0) {
                if (V == 4) {                                        // sk == 1, K % 4 == 0, every group 16 B aligned
                    for (int k = l * 4; k < K; k += L * 4) {
                        const float4 q = *reinterpret_cast<const float4*>(x + gb + k);
                        const float v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (gmax_better(v[i], k + i, bv, bk)) { bv = v[i]; bk = k + i; }
                    }
                } else {
                    for (int k = l; k < K; k += L) {
                        const float v = x[gb + (int64_t)k * sk];
                        if (gmax_better(v, k, bv, bk)) { bv = v; bk = k; }
                    }
                }
            }
#pragma unroll
            for (int o = L / 2; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o, 64);
                const int ok = __shfl_xor(bk, o, 64);
                if (gmax_better(ov, ok, bv, bk)) { bv = ov; bk = ok; }
            }
            // lane t owns group g0 + t: scanned in step t / G by sub-wave t % G
            const float tv = __shfl(bv, (lane % G) * L, 64);
            const int tk = __shfl(bk, (lane % G) * L, 64);
            if (lane / G == j) { rv = tv; rk = tk; }
        }
        if (g < groups) {
            y[g] = rv;
            arg[g] = (uint8_t)rk;
        }
    }
}

template <int L>
__global__ __launch_bounds__(256) void group_max_bwd_k_kernel(const float* __restrict__ gy, const uint8_t* __restrict__ arg, int C,
                                                              int M, int K, int64_t sb, int64_t sc, int64_t sm, int64_t sk,
                                                              int64_t groups, float* __restrict__ gx) {
    constexpr int G = GGA_WAVE / L, U = L >= 4 ? 4 : L;
    const int lane = threadIdx.x & 63, sub = lane / L, l = lane % L;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), step = (int64_t)gridDim.x * 4 * GGA_WAVE;
    for (int64_t g0 = wave * GGA_WAVE; g0 < groups; g0 += step) {
        const int64_t g = g0 + lane;
        const long long base = gmax_base(g, groups, C, M, sb, sc, sm);
        const float mine = g < groups ? gy[g] : 0.f;
        const int mine_k = g < groups ? (int)arg[g] : 0;
#pragma unroll U
        for (int j = 0; j < L; ++j) {
            const int src = j * G + sub;
            const long long gb = __shfl(base, src, 64);
            const float v = __shfl(mine, src, 64);
            const int a = __shfl(mine_k, src, 64);
            if (gb >= 0)
                for (int k = l; k < K; k += L) gx[gb + (int64_t)k * sk] = k == a ? v : 0.f;
        }
    }
}

// blockIdx.x = (b * mtiles + mt) * ctiles + ct: the workgroups that share a centre's rows are neighbours
__global__ __launch_bounds__(256) void group_max_fwd_c_kernel(const float* __restrict__ x, int C, int M, int K, int64_t sb,
                                                              int64_t sc, int64_t sm, int64_t sk, int mtiles, int ctiles,
                                                              float* __restrict__ y, uint8_t* __restrict__ arg) {
    __shared__ float sv[GMAX_TILE][GMAX_TILE_M + 1];
    __shared__ uint8_t sa[GMAX_TILE][GMAX_TILE_M + 4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int64_t t = blockIdx.x;
    const int ct = (int)(t % ctiles);
    t /= ctiles;
    const int mt = (int)(t % mtiles);
    const int64_t b = t / mtiles;
    const int c = ct * GMAX_TILE + lane, m0 = mt * GMAX_TILE_M;
    for (int i = 0; i < GMAX_TILE_M / 4; ++i) {
        const int ml = w * (GMAX_TILE_M / 4) + i, m = m0 + ml;
        if (m >= M) break;                                           // the same for the whole wave
        float bv = -INFINITY;
        int bk = K;
        if (c < C) {
            const float* p = x + (b * sb + (int64_t)c * sc + (int64_t)m * sm);
#pragma unroll 8
            for (int k = 0; k < K; ++k) {
                const float v = p[(int64_t)k * sk];
                if (gmax_better(v, k, bv, bk)) { bv = v; bk = k; }
            }
        }
        sv[lane][ml] = bv;
        sa[lane][ml] = (uint8_t)bk;
    }
    __syncthreads();
    // the turned tile: 16 consecutive threads along m
    const int ml = threadIdx.x % GMAX_TILE_M, m = m0 + ml;
    for (int cl = threadIdx.x / GMAX_TILE_M; cl < GMAX_TILE; cl += 256 / GMAX_TILE_M) {
        const int cc = ct * GMAX_TILE + cl;
        if (cc < C && m < M) {
            const int64_t o = (b * C + cc) * M + m;
            y[o] = sv[cl][ml];
            arg[o] = sa[cl][ml];
        }
    }
}

__global__ __launch_bounds__(256) void group_max_bwd_c_kernel(const float* __restrict__ gy, const uint8_t* __restrict__ arg, int C,
                                                              int M, int K, int64_t sb, int64_t sc, int64_t sm, int64_t sk,
                                                              int mtiles, int ctiles, float* __restrict__ gx) {
    __shared__ float sv[GMAX_TILE][GMAX_TILE_M + 1];
    __shared__ uint8_t sa[GMAX_TILE][GMAX_TILE_M + 4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int64_t t = blockIdx.x;
    const int ct = (int)(t % ctiles);
    t /= ctiles;
    const int mt = (int)(t % mtiles);
    const int64_t b = t / mtiles;
    const int m0 = mt * GMAX_TILE_M;
    for (int cl = threadIdx.x / GMAX_TILE_M; cl < GMAX_TILE; cl += 256 / GMAX_TILE_M) {
        const int cc = ct * GMAX_TILE + cl, ml = threadIdx.x % GMAX_TILE_M, m = m0 + ml;
        const bool in = cc < C && m < M;
        const int64_t o = in ? (b * C + cc) * M + m : 0;
        sv[cl][ml] = in ? gy[o] : 0.f;
        sa[cl][ml] = in ? arg[o] : (uint8_t)0;
    }
    __syncthreads();
    const int c = ct * GMAX_TILE + lane;
    if (c >= C) return;
    for (int i = 0; i < GMAX_TILE_M / 4; ++i) {
        const int ml = w * (GMAX_TILE_M / 4) + i, m = m0 + ml;
        if (m >= M) break;
        const float v = sv[lane][ml];
        const int a = sa[lane][ml];
        float* p = gx + (b * sb + (int64_t)c * sc + (int64_t)m * sm);
#pragma unroll 8
        for (int k = 0; k < K; ++k) p[(int64_t)k * sk] = k == a ? v : 0.f;
    }
}

struct GmaxPlan {
    int channels_on_lanes, lanes, mtiles, ctiles;
    int64_t groups;
    unsigned blocks;
};

static int gmax_plan(const char* name, const void* p0, const void* p1, const void* p2, int B, int C, int M, int K, int64_t sb,
                     int64_t sc, int64_t sm, int64_t sk, GmaxPlan* plan) {
    GGA_REQUIRE(p0 && p1 && p2, "%s: null pointer argument", name);
    GGA_REQUIRE(B >= 1 && C >= 1 && M >= 1, "%s: bad sizes (B %d, C %d, M %d)", name, B, C, M);
    GGA_REQUIRE(K >= 1 && K <= GGA_GROUP_MAX_SAMPLES, "%s: K %d not in 1..%d", name, K, GGA_GROUP_MAX_SAMPLES);
    GGA_REQUIRE(sb >= 0 && sc >= 0 && sm >= 0 && sk >= 0, "%s: negative stride (%lld, %lld, %lld, %lld)", name, (long long)sb,
                (long long)sc, (long long)sm, (long long)sk);
    plan->groups = (int64_t)B * C * M;
    plan->channels_on_lanes = sc == 1 && C > 1 && !(sk == 1 && K > 1);
    plan->lanes = 1;
    while (plan->lanes < K && plan->lanes < GGA_WAVE) plan->lanes *= 2;
    plan->mtiles = (M + GMAX_TILE_M - 1) / GMAX_TILE_M;
    plan->ctiles = (C + GMAX_TILE - 1) / GMAX_TILE;
    if (plan->channels_on_lanes) {
        const int64_t blocks = (int64_t)B * plan->mtiles * plan->ctiles;
        GGA_REQUIRE(blocks <= 0x7FFFFFFF, "%s: B * C * M too large for one launch (%lld workgroups)", name, (long long)blocks);
        plan->blocks = (unsigned)blocks;
    } else {
        const int64_t blocks = (plan->groups + 255) / 256;
        plan->blocks = (unsigned)(blocks < 65536 ? blocks : 65536);
    }
    return GGA_OK;
}

#define GMAX_COMMA ,
#define GMAX_LAUNCH_K(kernel, lanes, TAIL, ...)                                                                                           \
    switch (lanes) {                                                                                                          \
        case 1: hipLaunchKernelGGL((kernel<1 TAIL>), dim3(plan.blocks), dim3(256), 0, s, __VA_ARGS__); break;                        \
        case 2: hipLaunchKernelGGL((kernel<2 TAIL>), dim3(plan.blocks), dim3(256), 0, s, __VA_ARGS__); break;                        \
        case 4: hipLaunchKernelGGL((kernel<4 TAIL>), dim3(plan.blocks), dim3(256), 0, s, __VA_ARGS__); break;                        \
        case 8: hipLaunchKernelGGL((kernel<8 TAIL>), dim3(plan.blocks), dim3(256), 0, s, __VA_ARGS__); break;                        \
        case 16: hipLaunchKernelGGL((kernel<16 TAIL>), dim3(plan.blocks), dim3(256), 0, s, __VA_ARGS__); break;                      \
        case 32: hipLaunchKernelGGL((kernel<32 TAIL>), dim3(plan.blocks), dim3(256), 0, s, __VA_ARGS__); break;                      \
        default: hipLaunchKernelGGL((kernel<64 TAIL>), dim3(plan.blocks), dim3(256), 0, s, __VA_ARGS__); break;                      \
    }

extern "C" int gga_group_max_fwd(const float* x, int B, int C, int M, int K, int64_t sb, int64_t sc, int64_t sm, int64_t sk,
                                 float* y, uint8_t* arg, void* stream) {
    GmaxPlan plan;
    if (int rc = gmax_plan("gga_group_max_fwd", x, y, arg, B, C, M, K, sb, sc, sm, sk, &plan)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (plan.channels_on_lanes) {
        hipLaunchKernelGGL(group_max_fwd_c_kernel, dim3(plan.blocks), dim3(256), 0, s, x, C, M, K, sb, sc, sm, sk, plan.mtiles,
                           plan.ctiles, y, arg);
    } else {
        // four consecutive samples per lane as one 16 B load where every group starts on a 16 B boundary: a quarter of the
        // lanes per group, and of the cross-lane steps per byte
        const bool wide = sk == 1 && K % 4 == 0 && sb % 4 == 0 && sc % 4 == 0 && sm % 4 == 0 && ((uintptr_t)x & 15) == 0;
        if (wide) {
            int lanes = 1;
            while (lanes * 4 < K) lanes *= 2;
            GMAX_LAUNCH_K(group_max_fwd_k_kernel, lanes, GMAX_COMMA 4, x, C, M, K, sb, sc, sm, sk, plan.groups, y, arg)
        } else {
            GMAX_LAUNCH_K(group_max_fwd_k_kernel, plan.lanes, GMAX_COMMA 1, x, C, M, K, sb, sc, sm, sk, plan.groups, y, arg)
        }
    }
    GGA_CHECK_LAUNCH("gga_group_max_fwd");
    return GGA_OK;
}

extern "C" int gga_group_max_bwd(const float* grad_y, const uint8_t* arg, int B, int C, int M, int K, int64_t sb, int64_t sc,
                                 int64_t sm, int64_t sk, float* grad_x, void* stream) {
    GmaxPlan plan;
    if (int rc = gmax_plan("gga_group_max_bwd", grad_y, arg, grad_x, B, C, M, K, sb, sc, sm, sk, &plan)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (plan.channels_on_lanes) {
        hipLaunchKernelGGL(group_max_bwd_c_kernel, dim3(plan.blocks), dim3(256), 0, s, grad_y, arg, C, M, K, sb, sc, sm, sk,
                           plan.mtiles, plan.ctiles, grad_x);
    } else {
        GMAX_LAUNCH_K(group_max_bwd_k_kernel, plan.lanes, , grad_y, arg, C, M, K, sb, sc, sm, sk, plan.groups, grad_x)
    }
    GGA_CHECK_LAUNCH("gga_group_max_bwd");
    return GGA_OK;
}
