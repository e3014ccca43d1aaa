// The kernel = stride transposed convolutions of SECONDFPN (necks/second_fpn.py:52-69; stride 1 = a 1x1 product) as
// STREAMING GEMMs over the coarse pixels, forward and backward-data, on two fp16 operand planes (conv_planes.h).
//
// sp_conv_x9_kernel runs these layers as a gather-GEMM over the FINE pixels with an arithmetic rule book: 4 bytes of
// index per (tap, fine row), every coarse row of x fetched and split s*s times, and a backward-data launch per 128 input
// channels that each reads the whole gradient. None of that is needed: with kernel = stride every fine pixel belongs to
// exactly one (coarse pixel, tap), so
//   forward        y[b, s*iy + ky, s*ix + kx, :] = x[b, iy, ix, :] . W[ky][kx]            (cin -> cout, one chain)
//   backward-data  gx[b, iy, ix, :] = sum over (ky, kx) of gy[b, s*iy + ky, s*ix + kx, :] . W[ky][kx]^T
// and a workgroup that owns a run of consecutive coarse pixels finds every address by arithmetic on the pixel index.
//
// Workgroup: 256 threads, a tile of TP consecutive coarse pixels (rows of the GEMM).
//   A   the tile's rows are fetched once (forward: for all s*s taps; backward: the tap's fine rows), split once into the
//       two fp16 planes (h2_split2s, the gather kernel's split) and kept in LDS: row L at L * (4 * K + 16) bytes =
//       [plane 0: K fp16 | plane 1: K fp16 | 16 pad] - 16 consecutive lanes reading the same 16-byte segment of 16 rows
//       cover all 64 banks (ds_read_b128 conflict-free);
//   B   a wave owns 32-column tiles of the output and ALL its pixel blocks, so no two waves share a weight fragment:
//       the fragments go from the packed operand (weight bank, LAYOUT_GATHER: [tap][32-channel chunk][plane][column]
//       [32 ch], quarters swizzled) straight to registers, one stage ahead - no LDS image, no barrier in the k loop;
//   D   32x32x16 with A = pixels, B = weight columns, as in sp_conv_x9_kernel: register v of lane l = row (v / 4) * 8 +
//       (l / 32) * 4 + v % 4, column l % 32. A store instruction writes 128 contiguous bytes per half wave.
// Arithmetic = the gather kernel's, bit for bit: per (row, tap) ONE accumulator chain from zero over the k-steps of 16
// channels in ascending order with the three plane products in its order (a0 b1, a1 b0, a0 b0); backward-data adds each
// finished tap to the running total in tap order; the result is rescaled by the two operand scales in its order.
// The forward's BatchNorm sums are fp32 over the gather kernel's 32-row blocks (16 rows per lane in register order, then
// the other half wave), added in float64 (deconv_stream_stats_kernel: the sizes at which the blocks do not line up).
#include "gga_common.h"
#include "conv_planes.h"

#define DS_THREADS 256
#define DS_BWD_TP 64

static inline int ds_fwd_tp(int cin) { return cin <= 128 ? 128 : 64; }      // 65-66 KB of planes either way: two workgroups per CU

// pixel -> element offset of its first fine pixel (tap 0, channel 0) in the [B, s*h, s*w, C] image, or -1 past the end
__device__ __forceinline__ int64_t ds_fine_base(int64_t p, int64_t n_pix, int h, int w, int s, int C) {
    if (p >= n_pix) return -1;
    const int64_t hw = (int64_t)h * w;
    const int64_t b = p / hw;
    const int rem = (int)(p - b * hw);
    const int iy = rem / w, ix = rem - iy * w;
    return (((b * s * h + (int64_t)s * iy) * s * w) + (int64_t)s * ix) * C;
}

// TP rows of K floats, row L at src + base(L) (base < 0: a row of zeros) -> the two-plane LDS image. K % 32 == 0.
template <int TP, typename BaseFn>
__device__ __forceinline__ void ds_stage_rows(const float* __restrict__ src, BaseFn base, unsigned char* img, const int K,
                                              const int rowb, const float scale, const int tid) {
    const int c4s = K == 64 ? 4 : (K == 128 ? 5 : (K == 256 ? 6 : 7));       // log2 of float4s per row (K = 64 .. 512)
    const int total4 = TP << c4s;                         // a multiple of 8 float4s per thread (TP >= 64, K >= 128, or 128 x 64)
    for (int f0 = 0; f0 < total4; f0 += DS_THREADS * 8) {
        float4 v[8];
        bool ok[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {                     // unconditional loads: a row past the end reads row 0 and is zeroed
            const int f = f0 + tid + DS_THREADS * j;
            const int64_t b = base(f >> c4s);
            ok[j] = b >= 0;
            v[j] = *reinterpret_cast<const float4*>(src + (ok[j] ? b : 0) + 4 * (f & ((1 << c4s) - 1)));
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int f = f0 + tid + DS_THREADS * j;
            if (!ok[j]) v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            uint2 p0, p1;
            h2_split2s(v[j].x, v[j].y, scale, p0.x, p1.x);
            h2_split2s(v[j].z, v[j].w, scale, p0.y, p1.y);
            unsigned char* dst = img + (f >> c4s) * rowb + 8 * (f & ((1 << c4s) - 1));
            *reinterpret_cast<uint2*>(dst) = p0;
            *reinterpret_cast<uint2*>(dst + 2 * K) = p1;
        }
    }
}

typedef uint32_t ds_u4 __attribute__((ext_vector_type(4)));
union DsFrag { ds_u4 q; mf_v8h v; };

// ------------------------------------------------------------------------------------------------------------ forward
// RB: 32-pixel blocks of the tile (TP = 32 * RB); wave w computes columns col0 + 32 w .. + 31 of every block.
template <int RB>
__global__ __launch_bounds__(DS_THREADS, 2) void deconv_stream_fwd_kernel(const float* __restrict__ X, const uint16_t* __restrict__ Wp,
                                                                        float* __restrict__ Y, double* __restrict__ stats,
                                                                        const uint32_t* __restrict__ amax_x,
                                                                        const uint32_t* __restrict__ amax_w, int64_t n_pix, int h,
                                                                        int w, int s, int cin, int cout, int col0, int64_t n_tiles) {
    constexpr int TP = 32 * RB;
    extern __shared__ __attribute__((aligned(16))) unsigned char ds_smem[];
    const int rowb = 4 * cin + 16;
    unsigned char* const Xs = ds_smem;
    int64_t* const obase = reinterpret_cast<int64_t*>(ds_smem + TP * rowb);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int sbx = h2_scale_exp(*amax_x), sbw = h2_scale_exp(*amax_w);
    const int64_t tile = blockIdx.x;
    const int64_t p0 = tile * TP;
    if (tid < TP) obase[tid] = ds_fine_base(p0 + tid, n_pix, h, w, s, cout);
    ds_stage_rows<TP>(X, [&](int L) { return p0 + L < n_pix ? (p0 + L) * cin : (int64_t)-1; }, Xs, cin, rowb, h2_scale(sbx), tid);
    __syncthreads();

    const int nchunks = cin >> 5, taps = s * s, nstages = taps * nchunks;
    const int col = wave * 32 + r;
    const int qsw = (col >> 2) & 3;
    // fragment (k-step ks, plane p) of stage st: 8 channels 16 ks + 8 hh .. of column `col`
    const uint16_t* const wl = Wp + col * 32;
    auto load_b = [&](int st, DsFrag (&b)[2][2]) {
        const uint16_t* src = wl + (int64_t)st * (2 * 128 * 32);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int p = 0; p < 2; ++p)
                b[ks][p].q = *reinterpret_cast<const ds_u4*>(src + p * (128 * 32) + (((2 * ks + hh) ^ qsw) << 3));
    };
    const unsigned char* const arow = Xs + r * rowb + hh * 16;
    const float dx = h2_descale(sbx), dw = h2_descale(sbw);
    DsFrag b0[2][2], b1[2][2];                            // the stage's weight fragments and the next stage's, in turns
    load_b(0, b0);
    int st = 0;
    for (int k = 0; k < taps; ++k) {
        mf_v16 acc[RB];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[rb][i] = 0.0f;
        // one stage = 32 channels: request the next stage's fragments first (the scheduler must not sink the loads behind
        // the matrix instructions: they are waited for a whole stage later), then two k-steps from the LDS planes
        auto stage = [&](int ch, DsFrag (&bc)[2][2], DsFrag (&bnx)[2][2]) {
            load_b(st + 1 < nstages ? st + 1 : st, bnx);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                DsFrag a[RB][2];
#pragma unroll
                for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                    for (int p = 0; p < 2; ++p)
                        a[rb][p].q = *reinterpret_cast<const ds_u4*>(arow + rb * 32 * rowb + p * 2 * cin + ch * 64 + ks * 32);
#define DS_MH(PA, PB) _Pragma("unroll") for (int rb = 0; rb < RB; ++rb) acc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[rb][PA].v, bc[ks][PB].v, acc[rb], 0, 0, 0);
                DS_MH(0, 1) DS_MH(1, 0) DS_MH(0, 0)
#undef DS_MH
            }
            ++st;
        };
        for (int ch = 0; ch < nchunks; ch += 2) {         // (cin / 32 is even)
            stage(ch, b0, b1);
            stage(ch + 1, b1, b0);
        }
        // the tap's chain is complete: its rows of the output image and their BatchNorm sums
        const int ky = k / s, kx = k - ky * s;
        const int64_t tapoff = ((int64_t)ky * s * w + kx) * cout + col0 + col;
        float s1[RB], s2[RB];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            s1[rb] = 0.0f; s2[rb] = 0.0f;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const float val = (acc[rb][v] + 0.0f) * dx * dw;
                const int64_t ob = obase[rb * 32 + (v >> 2) * 8 + hh * 4 + (v & 3)];
                if (ob >= 0) Y[ob + tapoff] = val;
                s1[rb] += val; s2[rb] = fmaf(val, val, s2[rb]);      // (fused, as the gather kernel's sums compile)
            }
        }
        if (stats) {
            double a1 = 0.0, a2 = 0.0;
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                s1[rb] += __shfl_xor(s1[rb], 32);
                s2[rb] += __shfl_xor(s2[rb], 32);
                a1 += (double)s1[rb]; a2 += (double)s2[rb];
            }
            if (hh == 0) {
                double* dst = stats + ((int64_t)k * n_tiles + tile) * 2 * cout + col0 + col;
                dst[0] = a1; dst[cout] = a2;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------ backward-data
// Tile: 64 coarse pixels. The N = cin output columns are NCT = cin / 32 tiles; a wave owns CT of them and RBW of the two
// 32-pixel blocks: (CT, RBW) = (2, 2) for cin 256 (both 128-column operands from ONE pass over gy), (1, 2) for 128,
// (1, 1) for 64 (wave = column tile x pixel block). CO: columns of a packed operand (64 or 128).
template <int CT, int RBW, int CO>
__global__ __launch_bounds__(DS_THREADS, 2) void deconv_stream_bwd_kernel(const float* __restrict__ G, const uint16_t* __restrict__ Wp0,
                                                                        const uint16_t* __restrict__ Wp1, float* __restrict__ GX,
                                                                        const uint32_t* __restrict__ amax_g,
                                                                        const uint32_t* __restrict__ amax_w, int64_t n_pix, int h,
                                                                        int w, int s, int cin, int cout) {
    constexpr int TP = DS_BWD_TP;
    constexpr int WC = RBW == 2 ? 4 : 2;                  // waves across the columns
    extern __shared__ __attribute__((aligned(16))) unsigned char ds_smem[];
    const int rowb = 4 * cout + 16;
    unsigned char* const Gs = ds_smem;
    int64_t* const gbase = reinterpret_cast<int64_t*>(ds_smem + TP * rowb);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int sbg = h2_scale_exp(*amax_g), sbw = h2_scale_exp(*amax_w);
    const float gscale = h2_scale(sbg);
    const int64_t p0 = (int64_t)blockIdx.x * TP;
    if (tid < TP) gbase[tid] = ds_fine_base(p0 + tid, n_pix, h, w, s, cout);

    const int nchunks = cout >> 5, taps = s * s, nstages = taps * nchunks;
    const int ct0 = (wave % WC) * CT, rb0 = (wave / WC) * RBW;
    const uint16_t* wl[CT];
    int qsw[CT];
#pragma unroll
    for (int j = 0; j < CT; ++j) {
        const int gcol = (ct0 + j) * 32 + r;              // column of gx
        const int c = gcol % CO;
        wl[j] = (gcol / CO ? Wp1 : Wp0) + c * 32;
        qsw[j] = (c >> 2) & 3;
    }
    auto load_b = [&](int st, DsFrag (&b)[CT][2][2]) {
#pragma unroll
        for (int j = 0; j < CT; ++j) {
            const uint16_t* src = wl[j] + (int64_t)st * (2 * CO * 32);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int p = 0; p < 2; ++p)
                    b[j][ks][p].q = *reinterpret_cast<const ds_u4*>(src + p * (CO * 32) + (((2 * ks + hh) ^ qsw[j]) << 3));
        }
    };
    const unsigned char* const arow = Gs + (rb0 * 32 + r) * rowb + hh * 16;
    mf_v16 acc[CT][RBW], total[CT][RBW];
#pragma unroll
    for (int j = 0; j < CT; ++j)
#pragma unroll
        for (int rb = 0; rb < RBW; ++rb)
#pragma unroll
            for (int i = 0; i < 16; ++i) { acc[j][rb][i] = 0.0f; total[j][rb][i] = 0.0f; }
    DsFrag b0[CT][2][2], b1[CT][2][2];
    load_b(0, b0);
    int st = 0;
    for (int k = 0; k < taps; ++k) {
        const int ky = k / s, kx = k - ky * s;
        const int64_t tapoff = ((int64_t)ky * s * w + kx) * cout;
        __syncthreads();                                  // the previous tap's image has been read (first tap: gbase is written)
        ds_stage_rows<TP>(G, [&](int L) { const int64_t b = gbase[L]; return b >= 0 ? b + tapoff : b; }, Gs, cout, rowb, gscale, tid);
        __syncthreads();
        auto stage = [&](int ch, DsFrag (&bc)[CT][2][2], DsFrag (&bnx)[CT][2][2]) {       // as in the forward kernel
            load_b(st + 1 < nstages ? st + 1 : st, bnx);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                DsFrag a[RBW][2];
#pragma unroll
                for (int rb = 0; rb < RBW; ++rb)
#pragma unroll
                    for (int p = 0; p < 2; ++p)
                        a[rb][p].q = *reinterpret_cast<const ds_u4*>(arow + rb * 32 * rowb + p * 2 * cout + ch * 64 + ks * 32);
#define DS_MH(PA, PB) _Pragma("unroll") for (int j = 0; j < CT; ++j) _Pragma("unroll") for (int rb = 0; rb < RBW; ++rb) acc[j][rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[rb][PA].v, bc[j][ks][PB].v, acc[j][rb], 0, 0, 0);
                DS_MH(0, 1) DS_MH(1, 0) DS_MH(0, 0)
#undef DS_MH
            }
            ++st;
        };
        for (int ch = 0; ch < nchunks; ch += 2) {         // (cout / 32 is even)
            stage(ch, b0, b1);
            stage(ch + 1, b1, b0);
        }
        // the tap's chain is complete: one addition per element, a fresh chain (offset_sums of sp_conv_x9_kernel)
#pragma unroll
        for (int j = 0; j < CT; ++j)
#pragma unroll
            for (int rb = 0; rb < RBW; ++rb) {
                total[j][rb] += acc[j][rb];
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[j][rb][i] = 0.0f;
            }
    }
    const float dg = h2_descale(sbg), dw = h2_descale(sbw);
#pragma unroll
    for (int j = 0; j < CT; ++j)
#pragma unroll
        for (int rb = 0; rb < RBW; ++rb)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int64_t p = p0 + (rb0 + rb) * 32 + (v >> 2) * 8 + hh * 4 + (v & 3);
                if (p < n_pix) GX[p * cin + (ct0 + j) * 32 + r] = (total[j][rb][v] + 0.0f) * dg * dw;
            }
}

// ------------------------------------------------------------------------------------------------------- entry points
static int ds_check(const char* who, const void* a, const void* b, const void* c, const void* d, const void* e, int B, int h, int w,
                    int cin, int cout, int s) {
    GGA_REQUIRE(a && b && c && d && e, "%s: null pointer argument", who);
    GGA_REQUIRE(s >= 1 && s <= 4, "%s: stride %d outside 1..4", who, s);
    GGA_REQUIRE(cin == 64 || cin == 128 || cin == 256, "%s: cin %d is not 64, 128 or 256", who, cin);
    GGA_REQUIRE(cout >= 128 && cout % 128 == 0, "%s: cout %d is not a multiple of 128", who, cout);
    GGA_REQUIRE(B >= 1 && h >= 1 && w >= 1, "%s: bad sizes (B=%d h=%d w=%d)", who, B, h, w);
    GGA_REQUIRE((int64_t)B * h * w * s * s < ((int64_t)1 << 31), "%s: %lld output rows (B * h * w * s * s must stay below 2^31)", who,
                (long long)B * h * w * s * s);
    return GGA_OK;
}

// The forward kernel's fp32 block sums are the gather kernel's only when every tap's rows start at a multiple of 32 in the
// gather kernel's processing order (the fine rows sorted by tap, then by pixel: position = tap * n_pix + pixel): s == 1 or
// n_pix % 32 == 0. Other sizes take the sums from the finished image in exactly that order - 128 positions per workgroup,
// wave = a 32-position block, lane (r, hh) the rows (v / 4) * 8 + hh * 4 + v % 4 of its block in register order, then the
// other half wave, then the four blocks in float64 (x9_epilogue_rb) - so the BatchNorm statistics, and with them every
// array of a training step, do not depend on which of the two kernels ran. One more read of y, at sizes where it is small.
static inline bool ds_blocks_align(int64_t n_pix, int s) { return s == 1 || n_pix % 32 == 0; }

__global__ __launch_bounds__(DS_THREADS) void deconv_stream_stats_kernel(const float* __restrict__ Y, double* __restrict__ stats,
                                                                         int64_t n_pix, int h, int w, int s, int cout) {
    __shared__ int64_t base[128];
    extern __shared__ __attribute__((aligned(16))) unsigned char ds_smem[];
    float* const red = reinterpret_cast<float*>(ds_smem);                  // [4 waves][2][cout]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int64_t total = n_pix * s * s, q0 = (int64_t)blockIdx.x * 128;
    if (tid < 128) {
        const int64_t q = q0 + tid;
        int64_t b = -1;
        if (q < total) {
            const int k = (int)(q / n_pix);
            const int ky = k / s, kx = k - ky * s;
            b = ds_fine_base(q - (int64_t)k * n_pix, n_pix, h, w, s, cout) + ((int64_t)ky * s * w + kx) * cout;
        }
        base[tid] = b;
    }
    __syncthreads();
    for (int c = r; c < cout; c += 32) {
        float val[16];
#pragma unroll
        for (int v = 0; v < 16; ++v) {                    // (a row past the end reads row 0 and counts as zero: x + 0 = x)
            const int64_t b = base[wave * 32 + (v >> 2) * 8 + hh * 4 + (v & 3)];
            val[v] = Y[(b >= 0 ? b : 0) + c];
            if (b < 0) val[v] = 0.0f;
        }
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int v = 0; v < 16; ++v) { s1 += val[v]; s2 = fmaf(val[v], val[v], s2); }      // the fused form the gather kernel's sums compile to
        s1 += __shfl_xor(s1, 32);
        s2 += __shfl_xor(s2, 32);
        if (hh == 0) { red[(wave * 2 + 0) * cout + c] = s1; red[(wave * 2 + 1) * cout + c] = s2; }
    }
    __syncthreads();
    for (int i = tid; i < 2 * cout; i += DS_THREADS) {
        const int which = i / cout, c = i - which * cout;
        double a = 0.0;
#pragma unroll
        for (int w_ = 0; w_ < 4; ++w_) a += (double)red[(w_ * 2 + which) * cout + c];
        stats[((int64_t)blockIdx.x * 2 + which) * cout + c] = a;
    }
}

extern "C" int64_t gga_deconv_stream_tiles(int64_t n_pixels, int cin, int s) {
    if (n_pixels < 1 || s < 1 || s > 4 || !(cin == 64 || cin == 128 || cin == 256)) return 0;
    if (!ds_blocks_align(n_pixels, s)) return (n_pixels * s * s + 127) / 128;
    const int tp = ds_fwd_tp(cin);
    return (n_pixels + tp - 1) / tp * s * s;
}

extern "C" int gga_deconv_stream_fwd(const float* x, const void* const* weight_blocks, const uint32_t* amax_x,
                                     const uint32_t* amax_weight, int B, int h, int w, int cin, int cout, int s, float* y,
                                     double* stats, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = ds_check("gga_deconv_stream_fwd", x, weight_blocks, amax_x, amax_weight, y, B, h, w, cin, cout, s)) return rc;
    for (int c = 0; c < cout / 128; ++c) GGA_REQUIRE(weight_blocks[c], "gga_deconv_stream_fwd: null pointer argument (weight block %d)", c);
    const int64_t n_pix = (int64_t)B * h * w;
    const int tp = ds_fwd_tp(cin);
    const int64_t n_tiles = (n_pix + tp - 1) / tp;
    const size_t lds = (size_t)tp * (4 * cin + 16) + (size_t)tp * sizeof(int64_t);
    const bool aligned = ds_blocks_align(n_pix, s);
    GGA_REQUIRE(!stats || aligned || cout <= 1024, "gga_deconv_stream_fwd: cout %d above 1024 with sums (the block sums are kept in LDS)", cout);
    static bool once = false;
    if (!once) {
        GGA_CHECK_HIP(hipFuncSetAttribute((const void*)deconv_stream_fwd_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024), "deconv_stream_fwd_kernel: LDS size");
        GGA_CHECK_HIP(hipFuncSetAttribute((const void*)deconv_stream_fwd_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024), "deconv_stream_fwd_kernel: LDS size");
        once = true;
    }
    double* const kstats = aligned ? stats : nullptr;
    for (int c = 0; c < cout / 128; ++c) {
        const uint16_t* wp = (const uint16_t*)weight_blocks[c];
        if (tp == 128) hipLaunchKernelGGL((deconv_stream_fwd_kernel<4>), dim3((unsigned)n_tiles), dim3(DS_THREADS), lds, stream, x, wp, y, kstats, amax_x, amax_weight, n_pix, h, w, s, cin, cout, c * 128, n_tiles);
        else hipLaunchKernelGGL((deconv_stream_fwd_kernel<2>), dim3((unsigned)n_tiles), dim3(DS_THREADS), lds, stream, x, wp, y, kstats, amax_x, amax_weight, n_pix, h, w, s, cin, cout, c * 128, n_tiles);
        GGA_CHECK_LAUNCH("deconv_stream_fwd_kernel");
    }
    if (stats && !aligned) {
        hipLaunchKernelGGL(deconv_stream_stats_kernel, dim3((unsigned)gga_deconv_stream_tiles(n_pix, cin, s)), dim3(DS_THREADS),
                           (size_t)8 * cout * sizeof(float), stream, y, stats, n_pix, h, w, s, cout);
        GGA_CHECK_LAUNCH("deconv_stream_stats_kernel");
    }
    return GGA_OK;
}

extern "C" int gga_deconv_stream_bwd(const float* gy, const void* const* weight_blocks, const uint32_t* amax_gy,
                                     const uint32_t* amax_weight, int B, int h, int w, int cin, int cout, int s, float* gx,
                                     void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = ds_check("gga_deconv_stream_bwd", gy, weight_blocks, amax_gy, amax_weight, gx, B, h, w, cin, cout, s)) return rc;
    GGA_REQUIRE(cout <= 512 && (cout & (cout - 1)) == 0, "gga_deconv_stream_bwd: cout %d is not 128, 256 or 512 (the gradient tile is kept in LDS)", cout);
    const int nblocks = cin == 256 ? 2 : 1;
    for (int c = 0; c < nblocks; ++c) GGA_REQUIRE(weight_blocks[c], "gga_deconv_stream_bwd: null pointer argument (weight block %d)", c);
    const int64_t n_pix = (int64_t)B * h * w;
    const int64_t n_tiles = (n_pix + DS_BWD_TP - 1) / DS_BWD_TP;
    const size_t lds = (size_t)DS_BWD_TP * (4 * cout + 16) + (size_t)DS_BWD_TP * sizeof(int64_t);
    static bool once = false;
    if (!once) {
        GGA_CHECK_HIP(hipFuncSetAttribute((const void*)deconv_stream_bwd_kernel<2, 2, 128>, hipFuncAttributeMaxDynamicSharedMemorySize, 136 * 1024), "deconv_stream_bwd_kernel: LDS size");
        GGA_CHECK_HIP(hipFuncSetAttribute((const void*)deconv_stream_bwd_kernel<1, 2, 128>, hipFuncAttributeMaxDynamicSharedMemorySize, 136 * 1024), "deconv_stream_bwd_kernel: LDS size");
        GGA_CHECK_HIP(hipFuncSetAttribute((const void*)deconv_stream_bwd_kernel<1, 1, 64>, hipFuncAttributeMaxDynamicSharedMemorySize, 136 * 1024), "deconv_stream_bwd_kernel: LDS size");
        once = true;
    }
    const uint16_t* w0 = (const uint16_t*)weight_blocks[0];
    const uint16_t* w1 = nblocks == 2 ? (const uint16_t*)weight_blocks[1] : w0;
    const dim3 grid((unsigned)n_tiles), block(DS_THREADS);
    if (cin == 256) hipLaunchKernelGGL((deconv_stream_bwd_kernel<2, 2, 128>), grid, block, lds, stream, gy, w0, w1, gx, amax_gy, amax_weight, n_pix, h, w, s, cin, cout);
    else if (cin == 128) hipLaunchKernelGGL((deconv_stream_bwd_kernel<1, 2, 128>), grid, block, lds, stream, gy, w0, w1, gx, amax_gy, amax_weight, n_pix, h, w, s, cin, cout);
    else hipLaunchKernelGGL((deconv_stream_bwd_kernel<1, 1, 64>), grid, block, lds, stream, gy, w0, w1, gx, amax_gy, amax_weight, n_pix, h, w, s, cin, cout);
    GGA_CHECK_LAUNCH("deconv_stream_bwd_kernel");
    return GGA_OK;
}
