// The image batch of the mono3d branch, built on the device in one launch: the uint8 sources of a whole batch (decoded files,
// H x W x 3 each, at their offsets in one buffer) -> the [B, 3, Hp, Wp] float32 tensor the detector takes, resized, flipped,
// channel-reversed, normalised and zero-padded (gga_amd/image_pipelines.py: Resize, RandomFlip3D, Normalize, Pad).
//
// Arithmetic. Integers and one table lookup, so the host path (image_pipelines.resize_bilinear / materialize) gives the same
// bits for every input. The sample at output column x of a dst_w wide image taken from a src_w wide one:
//   q = ((2 x + 1) src_w 2048 + dst_w) / (2 dst_w) - 1024        (floor; = round(fx 2048), fx = (x + 0.5) src_w / dst_w - 0.5)
//   x0 = q >> 11, w1 = q & 2047, w0 = 2048 - w1; x0 < 0: x0 = 0, w1 = 0; x0 >= src_w - 1: both taps src_w - 1
// rows likewise; pixel = (sum wy wx p + 2^21) >> 22 <= 255, at most 255 * 2^22 + 2^21 < 2^31. dst == src is the identity and is
// read with one byte load per element instead of four. The value written is table[c][pixel]: the [3, 256] float32 table is
// the whole normalisation of a uint8 input.
//
// Shape. A "row" is (b, c, y) of out_w floats in NCHW memory and (b, y) of 3 out_w floats in NHWC memory; a lane produces four
// consecutive floats of a row as one 16-byte store, a block IB_ROWS consecutive rows of a 1024-float chunk, so the column
// taps of a lane (one 64-bit division each) serve eight rows. Every element of `out` is written, the padding with zeros.
#include "gga_common.h"

#define IB_THREADS 256
#define IB_VEC 4
#define IB_ROWS 8
#define IB_MAX_DIM (1 << 20)

struct IbTable {
    int n;
    gga_image_desc d[GGA_IMAGE_BATCH_MAX];
};

// taps of output index i: the two source indices and the weight (of 2048) of the second
__device__ __forceinline__ void ib_taps(int i, int src, int dst, int& i0, int& i1, int& w1) {
    const unsigned long long num = (unsigned long long)(2 * i + 1) * (unsigned long long)src * 2048ull + (unsigned long long)dst;
    const long long q = (long long)(num / (2ull * (unsigned long long)dst)) - 1024;
    i0 = (int)(q >> 11);
    w1 = (int)(q & 2047);
    if (i0 < 0) { i0 = 0; w1 = 0; }
    if (i0 >= src - 1) { i0 = src - 1; i1 = src - 1; } else { i1 = i0 + 1; }
}

template <bool NHWC>
__global__ __launch_bounds__(IB_THREADS) void image_batch_kernel(const uint8_t* __restrict__ src, const IbTable tab,
                                                                 const float* __restrict__ table, int reverse, int out_h,
                                                                 int out_w, int64_t n_rows, float* __restrict__ out) {
    __shared__ float lut[3 * 256];
    for (int k = threadIdx.x; k < 3 * 256; k += IB_THREADS) lut[k] = table[k];
    __syncthreads();
    const int row_len = NHWC ? 3 * out_w : out_w;                       // a multiple of 4 (checked by the entry point)
    const int e0 = (blockIdx.y * IB_THREADS + threadIdx.x) * IB_VEC;
    if (e0 >= row_len) return;
    int xs[IB_VEC], ch[IB_VEC];                                         // output column and channel of the lane's four floats
#pragma unroll
    for (int j = 0; j < IB_VEC; ++j) {
        xs[j] = NHWC ? (e0 + j) / 3 : e0 + j;
        ch[j] = NHWC ? (e0 + j) % 3 : 0;
    }
    const int rows_per_image = NHWC ? out_h : 3 * out_h;
    int cur_b = -1, x0[IB_VEC], x1[IB_VEC], wx[IB_VEC];
    const int64_t r_begin = (int64_t)blockIdx.x * IB_ROWS;
    for (int k = 0; k < IB_ROWS; ++k) {
        const int64_t r = r_begin + k;                                  // block-uniform
        if (r >= n_rows) break;
        const int b = (int)(r / rows_per_image), rem = (int)(r % rows_per_image);
        const int c_row = NHWC ? 0 : rem / out_h, y = NHWC ? rem : rem % out_h;
        const gga_image_desc d = tab.d[b];
        const bool same = d.dst_h == d.src_h && d.dst_w == d.src_w;
        float v[IB_VEC] = {0.f, 0.f, 0.f, 0.f};
        if (y < d.dst_h) {
            const uint8_t* img = src + d.src_offset;
            if (same) {
                const uint8_t* line = img + (int64_t)y * d.src_w * 3;
                // (byte loads: reading a lane's four pixels of an NCHW row as one unaligned 12-byte load was measured and is
                // slower, 38 against 26 us at the config's batch - EXPERIMENTS.md)
#pragma unroll
                for (int j = 0; j < IB_VEC; ++j) {
                    if (xs[j] < d.dst_w) {
                        const int c = NHWC ? ch[j] : c_row;
                        const int x = d.flip ? d.dst_w - 1 - xs[j] : xs[j];
                        v[j] = lut[c * 256 + line[x * 3 + (reverse ? 2 - c : c)]];
                    }
                }
            } else {
                if (b != cur_b) {                                       // the lane's column taps: once per image
                    cur_b = b;
#pragma unroll
                    for (int j = 0; j < IB_VEC; ++j)
                        if (xs[j] < d.dst_w) ib_taps(d.flip ? d.dst_w - 1 - xs[j] : xs[j], d.src_w, d.dst_w, x0[j], x1[j], wx[j]);
                }
                int y0, y1, wy;
                ib_taps(y, d.src_h, d.dst_h, y0, y1, wy);
                const uint8_t* top = img + (int64_t)y0 * d.src_w * 3;
                const uint8_t* bot = img + (int64_t)y1 * d.src_w * 3;
#pragma unroll
                for (int j = 0; j < IB_VEC; ++j) {
                    if (xs[j] < d.dst_w) {
                        const int c = NHWC ? ch[j] : c_row;
                        const int cs = reverse ? 2 - c : c;
                        const unsigned a0 = (unsigned)(2048 - wx[j]), a1 = (unsigned)wx[j];
                        const unsigned t = a0 * top[x0[j] * 3 + cs] + a1 * top[x1[j] * 3 + cs];
                        const unsigned u = a0 * bot[x0[j] * 3 + cs] + a1 * bot[x1[j] * 3 + cs];
                        const unsigned p = ((unsigned)(2048 - wy) * t + (unsigned)wy * u + (1u << 21)) >> 22;
                        v[j] = lut[c * 256 + p];
                    }
                }
            }
        }
        *reinterpret_cast<float4*>(out + r * row_len + e0) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

extern "C" int gga_image_batch(const uint8_t* src, int64_t src_bytes, const gga_image_desc* images_host, int n_images,
                               const float* table, int reverse_channels, int out_h, int out_w, int layout, float* out,
                               void* stream) {
    GGA_REQUIRE(n_images >= 0, "gga_image_batch: negative size (n_images %d)", n_images);
    GGA_REQUIRE(n_images <= GGA_IMAGE_BATCH_MAX, "gga_image_batch: n_images %d above GGA_IMAGE_BATCH_MAX %d", n_images, GGA_IMAGE_BATCH_MAX);
    GGA_REQUIRE(layout == GGA_LAYOUT_NCHW || layout == GGA_LAYOUT_NHWC, "gga_image_batch: unknown layout %d", layout);
    if (n_images == 0) return GGA_OK;
    GGA_REQUIRE(src && images_host && table && out, "gga_image_batch: null pointer");
    GGA_REQUIRE(((uintptr_t)out & 15) == 0, "gga_image_batch: out is not 16-byte aligned");
    GGA_REQUIRE(src_bytes >= 0 && out_h >= 1 && out_w >= 1 && out_h <= IB_MAX_DIM && out_w <= IB_MAX_DIM,
                "gga_image_batch: bad sizes (src_bytes %lld, out %d x %d)", (long long)src_bytes, out_h, out_w);
    GGA_REQUIRE(out_w % 4 == 0, "gga_image_batch: out_w %d is not a multiple of 4 (16-byte stores)", out_w);
    IbTable tab;
    tab.n = n_images;
    for (int i = 0; i < n_images; ++i) {
        const gga_image_desc& d = images_host[i];
        GGA_REQUIRE(d.src_h >= 1 && d.src_w >= 1 && d.dst_h >= 1 && d.dst_w >= 1 && d.src_h <= IB_MAX_DIM && d.src_w <= IB_MAX_DIM,
                    "gga_image_batch: image %d: bad sizes (src %d x %d, dst %d x %d)", i, d.src_h, d.src_w, d.dst_h, d.dst_w);
        GGA_REQUIRE(d.dst_h <= out_h && d.dst_w <= out_w, "gga_image_batch: image %d: dst %d x %d larger than out %d x %d", i,
                    d.dst_h, d.dst_w, out_h, out_w);
        GGA_REQUIRE(d.src_offset >= 0 && d.src_offset <= src_bytes && (int64_t)d.src_h * d.src_w * 3 <= src_bytes - d.src_offset,
                    "gga_image_batch: image %d: offset %lld + %d x %d x 3 bytes leaves the source buffer of %lld bytes", i,
                    (long long)d.src_offset, d.src_h, d.src_w, (long long)src_bytes);
        tab.d[i] = d;
        tab.d[i].flip = d.flip != 0;
    }
    const int64_t n_rows = (int64_t)n_images * out_h * (layout == GGA_LAYOUT_NHWC ? 1 : 3);
    const int row_len = layout == GGA_LAYOUT_NHWC ? 3 * out_w : out_w;
    const int64_t blocks_x = (n_rows + IB_ROWS - 1) / IB_ROWS;
    GGA_REQUIRE(blocks_x < (1ll << 31), "gga_image_batch: %lld rows: 2^31 blocks and more", (long long)n_rows);
    const dim3 grid((unsigned)blocks_x, (unsigned)((row_len + IB_THREADS * IB_VEC - 1) / (IB_THREADS * IB_VEC)));
    if (layout == GGA_LAYOUT_NHWC)
        hipLaunchKernelGGL(image_batch_kernel<true>, grid, dim3(IB_THREADS), 0, (hipStream_t)stream, src, tab, table,
                           reverse_channels != 0, out_h, out_w, n_rows, out);
    else
        hipLaunchKernelGGL(image_batch_kernel<false>, grid, dim3(IB_THREADS), 0, (hipStream_t)stream, src, tab, table,
                           reverse_channels != 0, out_h, out_w, n_rows, out);
    GGA_CHECK_LAUNCH("gga_image_batch");
    return GGA_OK;
}
