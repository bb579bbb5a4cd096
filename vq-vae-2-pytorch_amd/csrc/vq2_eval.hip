// Held-out evaluation and 8-bit export: none of these kernels is launched by the train step.
//   nhwc_to_u8       normalised fp32 NHWC -> 8-bit pixels in a canvas (inverse of u8_to_nhwc4_kernel, vq2_elem.hip)
//   sse_per_image    one sum of squared differences per image, fixed reduction tree
//   index_hist       code-usage histogram of a quantizer's indices (integer atomics only)
//   eval_accumulate  folds a batch into a device accumulator of doubles, so that an evaluation loop never syncs
//   image_metrics    per image: integer squared error and Gaussian-window SSIM of the two 8-bit images nhwc_to_u8 writes
//   prior_eval_rows        per logits row of the stage-2 prior: cross-entropy term, predictive entropy, rank of the target
//   prior_eval_accumulate  folds those rows into per-position running totals, one thread per position, in batch order
#include <math.h>
#include "vq2_common.h"

namespace vq2 {

// ------------------------------------------------------------------ normalised NHWC -> 8-bit canvas
// invTrans (train_vqvae.py:22-25) + the quantisation inside torchvision's save_image, per element and in fp32 with
// every operation rounded on its own (the library is built with -ffp-contract=off):
//     u = x / inv_s[c] + m[c];   v = u * 255 + 0.5;   byte = trunc(clamp(v, 0, 255));   NaN -> 0
// A workgroup converts tiles of TOU8_TILE consecutive pixels of the (n, y, x) pixel stream; thread t loads pixels
// t, t + 256, ... (one 16-byte load each when the pixel stride is 4).  DWORD: the bytes are staged in LDS in
// destination order and leave as aligned dwords, consecutive lanes consecutive dwords -- HWC as the C * TOU8_TILE / 4
// dwords of the tile's byte stream (rows of W * C bytes), CHW as one dword of 4 pixels per channel plane; the launcher
// checks that every row segment of every grid cell starts and ends on a 4-byte boundary.  Otherwise single byte stores.
constexpr int TOU8_TILE = 1024;

struct ToU8Params {
    const float *src; uint8_t *dst;
    int64_t total;            // N * H * W pixels
    int64_t ntiles;
    int64_t pitch, plane;     // bytes per canvas row; bytes per canvas channel plane (CHW)
    int64_t istride;          // batch form: bytes from one image to the next (every image in cell 0 of its own canvas), else 0
    int C, ld, H, W, cols, pad, vec;
    float inv_s[4], m[4];
};

// canvas byte offset of channel 0 of the pixel (row grow = n * H + y, column x): image n sits in grid cell
// (n / cols, n % cols) whose origin is (cell_row * (H + pad) + pad, cell_col * (W + pad) + pad), torchvision's make_grid.
// Rows, cells and canvas coordinates fit 32 bits (the launcher checks N * H < 2^31 and the cells against the int32
// canvas), so the divisions are 32-bit ones; only the final byte offset is 64-bit.
template <int LAYOUT>
__device__ __forceinline__ int64_t u8_dst_offset(const ToU8Params &P, uint32_t grow, uint32_t x) {
    const uint32_t n = grow / (uint32_t)P.H, y = grow - n * (uint32_t)P.H;
    const uint32_t k = P.istride ? 0u : n;
    const uint32_t cr = k / (uint32_t)P.cols, cc = k - cr * (uint32_t)P.cols;
    const uint32_t Y = cr * (uint32_t)(P.H + P.pad) + P.pad + y, X = cc * (uint32_t)(P.W + P.pad) + P.pad + x;
    return (int64_t)n * P.istride + (int64_t)Y * P.pitch + (LAYOUT == VQ2_U8_HWC ? (int64_t)X * P.C : (int64_t)X);
}

// a = q * b + r for a tile's first element (the same for every lane): one 32-bit division unless a needs 64 bits
__device__ __forceinline__ void tile_row(int64_t a, uint32_t b, uint32_t &q, uint32_t &r) {
    if ((a >> 32) == 0) {
        q = (uint32_t)a / b;
        r = (uint32_t)a - q * b;
    } else {
        const int64_t q64 = a / b;
        q = (uint32_t)q64;
        r = (uint32_t)(a - q64 * b);
    }
}

__device__ __forceinline__ uint32_t to_byte(float x, float inv_s, float m) {
    const float u = x / inv_s + m;
    float v = u * 255.f + 0.5f;
    v = fminf(fmaxf(v, 0.f), 255.f);   // fmaxf returns the operand that is a number: NaN -> 0
    return (uint32_t)v;
}

template <int LAYOUT, bool DWORD>
__global__ __launch_bounds__(256) void nhwc_to_u8_kernel(const ToU8Params P) {
    __shared__ uint32_t stage[DWORD ? TOU8_TILE : 1];   // TOU8_TILE pixels x <= 4 bytes
    uint8_t *sb = reinterpret_cast<uint8_t *>(stage);
    const int t = threadIdx.x, C = P.C;
    for (int64_t tile = blockIdx.x; tile < P.ntiles; tile += gridDim.x) {
        const int64_t tile0 = tile * TOU8_TILE;
        // all of the thread's 16-byte loads of the tile are issued before the first one is waited for
        float4 pix[TOU8_TILE / 256];
#pragma unroll
        for (int j = 0; j < TOU8_TILE / 256; ++j) {
            const int64_t g = tile0 + j * 256 + t;
            pix[j] = (P.vec && g < P.total) ? reinterpret_cast<const float4 *>(P.src)[g] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        // image row and column of the tile's first pixel; a lane's own row is 32-bit arithmetic from there
        uint32_t prow0 = 0, pcol0 = 0;
        if (!DWORD || LAYOUT == VQ2_U8_CHW) tile_row(tile0, (uint32_t)P.W, prow0, pcol0);
#pragma unroll
        for (int j = 0; j < TOU8_TILE / 256; ++j) {
            const int q = j * 256 + t;
            const int64_t g = tile0 + q;
            if (g < P.total) {
                float x[4] = {0.f, 0.f, 0.f, 0.f};
                if (P.vec) {
                    x[0] = pix[j].x; x[1] = pix[j].y; x[2] = pix[j].z; x[3] = pix[j].w;
                } else {
                    for (int c = 0; c < C; ++c) x[c] = P.src[g * P.ld + c];
                }
                uint32_t b[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) b[c] = to_byte(x[c], P.inv_s[c], P.m[c]);
                if (DWORD) {
                    for (int c = 0; c < C; ++c) sb[LAYOUT == VQ2_U8_HWC ? q * C + c : c * TOU8_TILE + q] = (uint8_t)b[c];
                } else {
                    const uint32_t u = pcol0 + q, r = u / (uint32_t)P.W;
                    const int64_t o = u8_dst_offset<LAYOUT>(P, prow0 + r, u - r * (uint32_t)P.W);
                    for (int c = 0; c < C; ++c) P.dst[o + (LAYOUT == VQ2_U8_HWC ? c : c * P.plane)] = (uint8_t)b[c];
                }
            }
        }
        if (DWORD) {
            __syncthreads();
            if (LAYOUT == VQ2_U8_HWC) {
                // byte stream of the tile: rows of W * C bytes (a multiple of 4, as is every row's start in the canvas)
                const uint32_t rowb = (uint32_t)P.W * C;
                const int64_t s0 = tile0 * C;
                uint32_t row0, off0;
                tile_row(s0, rowb, row0, off0);
                for (int k = 0; k < C; ++k) {
                    const uint32_t d = t + 256 * k;
                    if (s0 + 4 * (int64_t)d < P.total * C) {
                        const uint32_t u = off0 + 4 * d, r = u / rowb;
                        const int64_t o = u8_dst_offset<LAYOUT>(P, row0 + r, 0) + (u - r * rowb);
                        *reinterpret_cast<uint32_t *>(P.dst + o) = stage[d];
                    }
                }
            } else if (tile0 + 4 * t < P.total) {
                // 4 consecutive pixels of one row (W and pad are multiples of 4): one dword per channel plane
                const uint32_t u = pcol0 + 4 * t, r = u / (uint32_t)P.W;
                const int64_t o = u8_dst_offset<LAYOUT>(P, prow0 + r, u - r * (uint32_t)P.W);
                for (int c = 0; c < C; ++c)
                    *reinterpret_cast<uint32_t *>(P.dst + o + c * P.plane) = stage[c * (TOU8_TILE / 4) + t];
            }
            __syncthreads();   // the staging area is refilled by the next tile
        }
    }
}

// ------------------------------------------------------------------ per-image sum of squared differences
// Image n is per4 float4s; split s of S sums the float4s [s * chunk, (s + 1) * chunk): thread t takes t, t + 256, ...
// in order, then the butterfly of wave_sum, then the four waves.  S and chunk depend on per4 alone, so the tree of an
// image does not know how many images the launch holds.
constexpr int SSE_SPLIT4 = 2048, SSE_MAX_SPLITS = 64;

static inline int sse_splits(int64_t per4) {
    const int64_t s = (per4 + SSE_SPLIT4 - 1) / SSE_SPLIT4;
    return (int)(s < 1 ? 1 : (s > SSE_MAX_SPLITS ? SSE_MAX_SPLITS : s));
}

__global__ __launch_bounds__(256) void sse_partial_kernel(const float4 *__restrict__ a, const float4 *__restrict__ b,
                                                          int64_t per4, int64_t chunk, float *__restrict__ part) {
    __shared__ float wsum[4];
    const int64_t n = blockIdx.y, lo = blockIdx.x * chunk;
    const int64_t hi = lo + chunk < per4 ? lo + chunk : per4;
    const float4 *pa = a + n * per4, *pb = b + n * per4;
    float s = 0.f;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        const float4 x = pa[i], y = pb[i];
        const float d0 = x.x - y.x, d1 = x.y - y.y, d2 = x.z - y.z, d3 = x.w - y.w;
        s += d0 * d0; s += d1 * d1; s += d2 * d2; s += d3 * d3;
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[n * gridDim.x + blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

__global__ __launch_bounds__(64) void sse_final_kernel(const float *__restrict__ part, int S, float *__restrict__ sse) {
    const int n = blockIdx.x, t = threadIdx.x;
    const float v = wave_sum(t < S ? part[(int64_t)n * S + t] : 0.f);
    if (t == 0) sse[n] = v;
}

// ------------------------------------------------------------------ code-usage histogram
// int32 histogram of the workgroup's share in LDS, flushed with 64-bit integer atomics (integer addition commutes:
// the result does not depend on the order).  An index outside [0, K) is counted nowhere and raises the flag.
__global__ __launch_bounds__(256) void index_hist_kernel(const int64_t *__restrict__ idx, int64_t M, int K,
                                                         unsigned long long *__restrict__ counts, int *__restrict__ flag) {
    extern __shared__ int hist[];
    for (int k = threadIdx.x; k < K; k += 256) hist[k] = 0;
    __syncthreads();
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < M; i += (int64_t)gridDim.x * 256) {
        const int64_t v = idx[i];
        if ((uint64_t)v < (uint64_t)K) atomicAdd(&hist[(int)v], 1);
        else bad = true;
    }
    if (bad) atomicOr(flag, 1);
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += 256) {
        const int h = hist[k];
        if (h) atomicAdd(&counts[k], (unsigned long long)h);
    }
}

// ------------------------------------------------------------------ batch -> running totals (one workgroup)
// acc[0] += sse[0], then sse[1], ... one image after the other in double: the total of a set of images does not depend
// on how the set was cut into batches.  acc[1] += N * elems, acc[2] += diff * N, acc[3] += N.
__global__ __launch_bounds__(256) void eval_accumulate_kernel(const float *__restrict__ sse, int N, double elems,
                                                              const float *__restrict__ diff, double *__restrict__ acc) {
    __shared__ float buf[256];
    double s = threadIdx.x == 0 ? acc[0] : 0.0;
    for (int base = 0; base < N; base += 256) {
        if (base + (int)threadIdx.x < N) buf[threadIdx.x] = sse[base + threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = N - base < 256 ? N - base : 256;
            for (int i = 0; i < m; ++i) s += (double)buf[i];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        acc[0] = s;
        acc[1] += (double)N * elems;
        acc[2] += (double)diff[0] * (double)N;
        acc[3] += (double)N;
    }
}

// ------------------------------------------------------------------ 8-bit squared error and SSIM per image
// Both tensors become bytes through to_byte (the bytes nhwc_to_u8 writes); everything after that is integer (the
// squared error) or fp64 (SSIM, Wang et al. 2004: 11x11 Gaussian window of sigma 1.5, valid region, data range 255).
// One workgroup per tile of IM_T x IM_T window positions of one image:
//   1. the IM_P x IM_P pixel patch of both tensors -> one dword of <= 4 bytes per pixel in LDS.  A lane whose pixel is
//      outside the image loads nothing and stores 0.  A pixel's squared error is counted by the tile that owns it: the
//      tile of its own window position, the last tile of a row / column taking the 10 trailing pixels as well.
//   2. per channel: horizontal 11-tap pass of a, b, a^2, b^2, ab into an fp64 LDS tile (IM_P rows x IM_T columns),
//      vertical pass with consecutive lanes on consecutive columns, then the SSIM map value; positions outside the
//      valid region add nothing.
//   3. fixed tree: a thread adds its positions channel after channel, wave butterfly, the four waves in order; the
//      tile's partials go to the workspace and image_metrics_final_kernel folds them in tile order.  The tree depends on
//      (C, H, W) alone.
// In fp64 with separately rounded operations a == b gives mu_a == mu_b and var_a == var_b == cov bit for bit, so that
// numerator and denominator below are the same number and S == 1.0 exactly.
constexpr int IM_T = 32, IM_WIN = 11, IM_P = IM_T + IM_WIN - 1, IM_PIX = IM_P * IM_P;
constexpr int IM_LOADS = (IM_PIX + 255) / 256;

struct ImParams {
    const float *a, *b;
    int64_t lda, ldb;
    int C, H, W, tiles_x, tiles_y, veca, vecb;
    float inv_s[4], m[4];
    double g[IM_WIN];
    double *part_s;                 // [N * tiles] SSIM map sums
    unsigned long long *part_e;     // [N * tiles] squared errors
};

__device__ __forceinline__ uint32_t pack_bytes(const float x[4], const ImParams &P) {
    uint32_t w = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) w |= (c < P.C ? to_byte(x[c], P.inv_s[c], P.m[c]) : 0u) << (8 * c);
    return w;
}

__device__ __forceinline__ uint32_t sq_diff_bytes(uint32_t wa, uint32_t wb) {
    uint32_t e = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int d = (int)((wa >> (8 * c)) & 255u) - (int)((wb >> (8 * c)) & 255u);
        e += (uint32_t)(d * d);
    }
    return e;
}

__global__ __launch_bounds__(256) void image_metrics_kernel(const ImParams P) {
    __shared__ uint32_t pa[IM_PIX], pb[IM_PIX];
    __shared__ double hd[5][IM_P][IM_T];
    __shared__ double wsum[4];
    __shared__ uint32_t wsum_e[4];
    const int t = threadIdx.x, n = blockIdx.y, H = P.H, W = P.W;
    const int tyi = blockIdx.x / P.tiles_x, txi = blockIdx.x - tyi * P.tiles_x;
    const int ty0 = tyi * IM_T, tx0 = txi * IM_T;
    const bool last_y = tyi == P.tiles_y - 1, last_x = txi == P.tiles_x - 1;
    const int64_t img0 = (int64_t)n * H * W;

    // ---- 1. patch -> bytes.  All of the thread's 16-byte loads are issued before the first one is waited for.
    float4 va[IM_LOADS], vb[IM_LOADS];
#pragma unroll
    for (int j = 0; j < IM_LOADS; ++j) {
        const int p = j * 256 + t, py = p / IM_P, px = p - py * IM_P;
        const int gy = ty0 + py, gx = tx0 + px;
        const bool in = p < IM_PIX && gy < H && gx < W;
        const int64_t g = img0 + (int64_t)gy * W + gx;
        va[j] = (in && P.veca) ? reinterpret_cast<const float4 *>(P.a)[g] : make_float4(0.f, 0.f, 0.f, 0.f);
        vb[j] = (in && P.vecb) ? reinterpret_cast<const float4 *>(P.b)[g] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    uint32_t err = 0;
#pragma unroll
    for (int j = 0; j < IM_LOADS; ++j) {
        const int p = j * 256 + t, py = p / IM_P, px = p - py * IM_P;
        const int gy = ty0 + py, gx = tx0 + px;
        if (p < IM_PIX) {
            uint32_t wa = 0, wb = 0;
            if (gy < H && gx < W) {
                const int64_t g = img0 + (int64_t)gy * W + gx;
                float xa[4] = {va[j].x, va[j].y, va[j].z, va[j].w}, xb[4] = {vb[j].x, vb[j].y, vb[j].z, vb[j].w};
                if (!P.veca) for (int c = 0; c < P.C; ++c) xa[c] = P.a[g * P.lda + c];
                if (!P.vecb) for (int c = 0; c < P.C; ++c) xb[c] = P.b[g * P.ldb + c];
                wa = pack_bytes(xa, P);
                wb = pack_bytes(xb, P);
                if ((py < IM_T || last_y) && (px < IM_T || last_x)) err += sq_diff_bytes(wa, wb);
            }
            pa[p] = wa;
            pb[p] = wb;
        }
    }
    // a tile's squared error is at most 42 * 42 * 4 * 255^2 < 2^29: 32 bits hold every partial sum
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) err += (uint32_t)__shfl_xor((int)err, o, 64);
    if ((t & 63) == 0) wsum_e[t >> 6] = err;
    __syncthreads();

    // ---- 2. per channel: horizontal pass, vertical pass, map value
    const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
    const int vy = H - (IM_WIN - 1) - ty0, vx = W - (IM_WIN - 1) - tx0;   // valid positions of this tile: oy < vy, ox < vx
    double acc = 0.0;
    for (int c = 0; c < P.C; ++c) {
        const int sh = 8 * c;
        for (int i = t; i < IM_P * IM_T; i += 256) {
            const int row = i >> 5, col = i & 31;
            const uint32_t *ra = pa + row * IM_P + col, *rb = pb + row * IM_P + col;
            double sa = 0.0, sb = 0.0, saa = 0.0, sbb = 0.0, sab = 0.0;
#pragma unroll
            for (int k = 0; k < IM_WIN; ++k) {
                const double da = (double)((ra[k] >> sh) & 255u), db = (double)((rb[k] >> sh) & 255u);
                sa += P.g[k] * da;
                sb += P.g[k] * db;
                saa += P.g[k] * (da * da);
                sbb += P.g[k] * (db * db);
                sab += P.g[k] * (da * db);
            }
            hd[0][row][col] = sa; hd[1][row][col] = sb; hd[2][row][col] = saa; hd[3][row][col] = sbb; hd[4][row][col] = sab;
        }
        __syncthreads();
        for (int i = t; i < IM_T * IM_T; i += 256) {
            const int oy = i >> 5, ox = i & 31;
            double mua = 0.0, mub = 0.0, eaa = 0.0, ebb = 0.0, eab = 0.0;
#pragma unroll
            for (int k = 0; k < IM_WIN; ++k) {
                mua += P.g[k] * hd[0][oy + k][ox];
                mub += P.g[k] * hd[1][oy + k][ox];
                eaa += P.g[k] * hd[2][oy + k][ox];
                ebb += P.g[k] * hd[3][oy + k][ox];
                eab += P.g[k] * hd[4][oy + k][ox];
            }
            const double maa = mua * mua, mbb = mub * mub, mab = mua * mub;
            const double va2 = eaa - maa, vb2 = ebb - mbb, cov = eab - mab;
            const double s = ((2.0 * mab + C1) * (2.0 * cov + C2)) / ((maa + mbb + C1) * (va2 + vb2 + C2));
            acc += (oy < vy && ox < vx) ? s : 0.0;
        }
        __syncthreads();   // the fp64 tile is refilled by the next channel
    }
    // ---- 3. fixed tree
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((t & 63) == 0) wsum[t >> 6] = acc;
    __syncthreads();
    if (t == 0) {
        const int64_t slot = (int64_t)n * gridDim.x + blockIdx.x;
        P.part_s[slot] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        P.part_e[slot] = ((unsigned long long)wsum_e[0] + wsum_e[1]) + ((unsigned long long)wsum_e[2] + wsum_e[3]);
    }
}

// image n: thread t adds the tiles t, t + 64, ... in order, then the butterfly; ssim = sum / count
__global__ __launch_bounds__(64) void image_metrics_final_kernel(const double *__restrict__ part_s,
                                                                 const unsigned long long *__restrict__ part_e, int tiles,
                                                                 double count, long long *__restrict__ sse_u8,
                                                                 double *__restrict__ ssim) {
    const int n = blockIdx.x, t = threadIdx.x;
    double s = 0.0;
    unsigned long long e = 0;
    for (int i = t; i < tiles; i += 64) {
        s += part_s[(int64_t)n * tiles + i];
        e += part_e[(int64_t)n * tiles + i];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, 64);
        e += __shfl_xor(e, o, 64);
    }
    if (t == 0) {
        ssim[n] = s / count;
        sse_u8[n] = (long long)e;
    }
}

// acc_d[0] += ssim[0], then ssim[1], ... in image order (as eval_accumulate_kernel does); acc_i[0] += sum of sse_u8
__global__ __launch_bounds__(256) void image_metrics_accumulate_kernel(const long long *__restrict__ sse_u8,
                                                                       const double *__restrict__ ssim, int N,
                                                                       long long *__restrict__ acc_i, double *__restrict__ acc_d) {
    __shared__ double buf[256];
    __shared__ long long ebuf[256];
    double s = threadIdx.x == 0 ? acc_d[0] : 0.0;
    long long e = threadIdx.x == 0 ? acc_i[0] : 0;
    for (int base = 0; base < N; base += 256) {
        if (base + (int)threadIdx.x < N) {
            buf[threadIdx.x] = ssim[base + threadIdx.x];
            ebuf[threadIdx.x] = sse_u8[base + threadIdx.x];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = N - base < 256 ? N - base : 256;
            for (int i = 0; i < m; ++i) { s += buf[i]; e += ebuf[i]; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        acc_d[0] = s;
        acc_i[0] = e;
    }
}

// ------------------------------------------------------------------ stage-2 prior: per-row likelihood terms
// One wave per row, as xent_rows_kernel (vq2_prior.hip): lane c takes the float4 groups c, c + 64, ... of the row; the
// guards keep the pad lanes of the last group out of every result.  Pass 1: the row maximum.  Pass 2: with d = l - m and
// e = expf(d) in fp32, the sums of e and of e * d in fp64 (a 16,384-class row is 64 groups per lane: the row is looped
// over, never held), and the integer count of the classes that beat the target -- a larger logit, or an equal one at a
// lower index, which is the tie rule of xent_rows_kernel's arg-max: rank 0 there is a hit here.  An out-of-range target
// is compared with nothing and read through nowhere.
struct RowSums { double s, u; int above; };

__device__ __forceinline__ void row_term(RowSums &a, float v, float m, float lt, int c, int t) {
    const float d = v - m, e = expf(d);
    a.s += (double)e;
    a.u += (double)e * (double)d;
    a.above += (v > lt || (v == lt && c < t)) ? 1 : 0;
}

__global__ __launch_bounds__(256) void prior_eval_rows_kernel(const float *__restrict__ logits, int ld,
                                                              const int64_t *__restrict__ target, int64_t M, int ncls,
                                                              float *__restrict__ nll, float *__restrict__ entropy,
                                                              int32_t *__restrict__ rank) {
    const int lane = threadIdx.x & 63;
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < M; row += (int64_t)gridDim.x * 4) {
        const float *x = logits + row * ld;
        const int64_t t64 = target[row];
        const bool valid = (uint64_t)t64 < (uint64_t)ncls;
        const int t = valid ? (int)t64 : 0;
        const float lt = valid ? x[t] : INFINITY;      // out of range: the count below is not used
        float m = -INFINITY;
        for (int c = lane * 4; c < ncls; c += 256) {
            const float4 v = *reinterpret_cast<const float4 *>(x + c);
            m = fmaxf(m, v.x);
            if (c + 1 < ncls) m = fmaxf(m, v.y);
            if (c + 2 < ncls) m = fmaxf(m, v.z);
            if (c + 3 < ncls) m = fmaxf(m, v.w);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        RowSums a = {0.0, 0.0, 0};
        for (int c = lane * 4; c < ncls; c += 256) {
            const float4 v = *reinterpret_cast<const float4 *>(x + c);
            row_term(a, v.x, m, lt, c, t);
            if (c + 1 < ncls) row_term(a, v.y, m, lt, c + 1, t);
            if (c + 2 < ncls) row_term(a, v.z, m, lt, c + 2, t);
            if (c + 3 < ncls) row_term(a, v.w, m, lt, c + 3, t);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            a.s += __shfl_xor(a.s, o, 64);
            a.u += __shfl_xor(a.u, o, 64);
            a.above += __shfl_xor(a.above, o, 64);
        }
        if (lane == 0) {
            const double ls = log(a.s);                // s >= 1: the maximum's own term is exp(0)
            nll[row] = valid ? (float)(ls - (double)(lt - m)) : 0.f;
            entropy[row] = (float)(ls - a.u / a.s);
            rank[row] = valid ? a.above : -1;
        }
    }
}

// ------------------------------------------------------------------ stage-2 prior: rows -> running totals
// Rows are [N, L].  Three kinds of workgroup in one launch, none of which shares an output with another:
//   blockIdx.x <  PB            positions: thread p owns pos_*[p] and adds the batch's N rows to it in image order
//   blockIdx.x == PB            counters: images += N; bad += rows of rank -1 (integers: any order gives the same sum)
//   blockIdx.x >  PB            image blockIdx.x - PB - 1: its L rows through LDS, thread 0 adds them in position order
__global__ __launch_bounds__(256) void prior_eval_accumulate_kernel(const float *__restrict__ row_nll,
                                                                    const float *__restrict__ row_entropy,
                                                                    const int32_t *__restrict__ row_rank, int N, int L, int top_k,
                                                                    int PB, double *__restrict__ pos_nll,
                                                                    double *__restrict__ pos_entropy,
                                                                    long long *__restrict__ pos_hit1,
                                                                    long long *__restrict__ pos_hitk,
                                                                    long long *__restrict__ counters, float *__restrict__ image_nll) {
    __shared__ float buf[256];
    __shared__ int bad_of[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b < PB) {
        const int p = b * 256 + tid;
        if (p >= L) return;
        double sn = pos_nll[p], se = pos_entropy[p];
        int h1 = 0, hk = 0;
        for (int n = 0; n < N; ++n) {
            const int64_t r = (int64_t)n * L + p;
            const int rk = row_rank[r];
            sn += (double)row_nll[r];
            se += (double)row_entropy[r];
            h1 += rk == 0;
            hk += rk >= 0 && rk < top_k;
        }
        pos_nll[p] = sn;
        pos_entropy[p] = se;
        pos_hit1[p] += h1;
        pos_hitk[p] += hk;
    } else if (b == PB) {
        const int64_t rows = (int64_t)N * L;
        int bad = 0;
        for (int64_t r = tid; r < rows; r += 256) bad += row_rank[r] == -1;
        bad_of[tid] = bad;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) bad_of[tid] += bad_of[tid + o];
            __syncthreads();
        }
        if (tid == 0) {
            counters[0] += N;
            counters[1] += bad_of[0];
        }
    } else {
        const int n = b - PB - 1;
        const float *src = row_nll + (int64_t)n * L;
        double s = 0.0;
        for (int base = 0; base < L; base += 256) {
            if (base + tid < L) buf[tid] = src[base + tid];
            __syncthreads();
            if (tid == 0) {
                const int m = L - base < 256 ? L - base : 256;
                for (int i = 0; i < m; ++i) s += (double)buf[i];
            }
            __syncthreads();
        }
        if (tid == 0) image_nll[n] = (float)s;
    }
}

}  // namespace vq2

using namespace vq2;

extern "C" int vq2_nhwc_to_u8(const float *src, int32_t ld, int32_t N, int32_t C, int32_t H, int32_t W,
                              const float *inv_s, const float *mean, uint8_t *dst, int layout, int32_t Hc, int32_t Wc,
                              int64_t pitch, int32_t cols, int32_t pad, int64_t image_pitch, vq2_stream_t stream) {
    VQ2_REQUIRE(src && dst && inv_s && mean, "nhwc_to_u8: null pointer");
    VQ2_REQUIRE(layout == VQ2_U8_HWC || layout == VQ2_U8_CHW, "nhwc_to_u8: layout %d is neither VQ2_U8_HWC nor VQ2_U8_CHW", layout);
    VQ2_REQUIRE(C >= 1 && C <= 4, "nhwc_to_u8: %d channels (1..4)", C);
    VQ2_REQUIRE(N > 0 && H > 0 && W > 0 && Hc > 0 && Wc > 0 && ld >= C, "nhwc_to_u8: non-positive dimension or ld < C");
    VQ2_REQUIRE(cols >= 1 && pad >= 0, "nhwc_to_u8: the grid needs cols >= 1 and pad >= 0");
    const bool hwc = layout == VQ2_U8_HWC;
    // every image cell, its padding included, lies inside the canvas
    const int64_t placed = image_pitch ? 1 : N;   // batch form: one image per canvas
    const int64_t cell_rows = (placed + cols - 1) / cols, cell_cols = placed < cols ? placed : cols;
    VQ2_REQUIRE(cell_rows * ((int64_t)H + pad) + pad <= Hc && cell_cols * ((int64_t)W + pad) + pad <= Wc,
                "nhwc_to_u8: %d images of %dx%d in %d columns with padding %d do not fit the %dx%d canvas", N, H, W, cols,
                pad, Hc, Wc);
    VQ2_REQUIRE(pitch >= (int64_t)Wc * (hwc ? C : 1), "nhwc_to_u8: pitch %lld is shorter than a canvas row", (long long)pitch);
    VQ2_REQUIRE(image_pitch == 0 || image_pitch >= pitch * Hc * (hwc ? 1 : C),
                "nhwc_to_u8: image_pitch %lld is shorter than one image's canvas", (long long)image_pitch);
    VQ2_REQUIRE((int64_t)W * C < (1 << 30), "nhwc_to_u8: rows of 2^30 bytes and more are not supported");
    VQ2_REQUIRE((int64_t)N * H < ((int64_t)1 << 31), "nhwc_to_u8: 2^31 image rows and more are not supported");
    for (int c = 0; c < C; ++c) VQ2_REQUIRE(inv_s[c] != 0.f, "nhwc_to_u8: inv_s[%d] is zero", c);
    ToU8Params P;
    P.src = src; P.dst = dst;
    P.total = (int64_t)N * H * W;
    P.ntiles = (P.total + TOU8_TILE - 1) / TOU8_TILE;
    P.pitch = pitch; P.plane = pitch * Hc; P.istride = image_pitch;
    P.C = C; P.ld = ld; P.H = H; P.W = W; P.cols = cols; P.pad = pad;
    P.vec = ld == 4 && aligned16(src);
    for (int c = 0; c < 4; ++c) { P.inv_s[c] = c < C ? inv_s[c] : 1.f; P.m[c] = c < C ? mean[c] : 0.f; }
    // dword stores need every row segment of every cell to start and end on a 4-byte boundary of the canvas
    const int unit = hwc ? C : 1;   // bytes per pixel within one row segment
    const bool dword = (reinterpret_cast<uintptr_t>(dst) & 3u) == 0 && pitch % 4 == 0 && image_pitch % 4 == 0 && ((int64_t)W * unit) % 4 == 0 &&
                       ((int64_t)pad * unit) % 4 == 0;
    hipStream_t s = to_stream(stream);
    const dim3 grid((unsigned)(P.ntiles < 2048 ? P.ntiles : 2048)), block(256);
    if (hwc && dword) hipLaunchKernelGGL((nhwc_to_u8_kernel<VQ2_U8_HWC, true>), grid, block, 0, s, P);
    else if (hwc) hipLaunchKernelGGL((nhwc_to_u8_kernel<VQ2_U8_HWC, false>), grid, block, 0, s, P);
    else if (dword) hipLaunchKernelGGL((nhwc_to_u8_kernel<VQ2_U8_CHW, true>), grid, block, 0, s, P);
    else hipLaunchKernelGGL((nhwc_to_u8_kernel<VQ2_U8_CHW, false>), grid, block, 0, s, P);
    return check_launch("nhwc_to_u8_kernel");
}

extern "C" size_t vq2_sse_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t ld) {
    if (N <= 0 || H <= 0 || W <= 0 || ld <= 0 || ld % 4) return 0;
    return (size_t)N * sse_splits((int64_t)H * W * (ld / 4)) * sizeof(float);
}

extern "C" int vq2_sse_per_image(const float *a, const float *b, int32_t N, int32_t H, int32_t W, int32_t ld, float *sse,
                                 void *ws, size_t ws_bytes, vq2_stream_t stream) {
    VQ2_REQUIRE(a && b && sse && ws, "sse_per_image: null pointer");
    VQ2_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0 && ld > 0 && ld % 4 == 0,
                "sse_per_image: need 1..65535 images and a pixel stride that is a multiple of 4");
    VQ2_REQUIRE(aligned16(a) && aligned16(b), "sse_per_image: pointers must be 16-byte aligned");
    const int64_t per4 = (int64_t)H * W * (ld / 4);
    const int S = sse_splits(per4);
    if (ws_bytes < (size_t)N * S * sizeof(float)) return set_error(VQ2_ERR_WORKSPACE, "sse_per_image: workspace too small");
    hipStream_t s = to_stream(stream);
    hipLaunchKernelGGL(sse_partial_kernel, dim3(S, N), dim3(256), 0, s, reinterpret_cast<const float4 *>(a),
                       reinterpret_cast<const float4 *>(b), per4, (per4 + S - 1) / S, static_cast<float *>(ws));
    if (int e = check_launch("sse_partial_kernel")) return e;
    hipLaunchKernelGGL(sse_final_kernel, dim3(N), dim3(64), 0, s, static_cast<const float *>(ws), S, sse);
    return check_launch("sse_final_kernel");
}

extern "C" int vq2_index_hist(const int64_t *idx, int64_t M, int32_t K, int64_t *counts, int32_t *flag,
                              vq2_stream_t stream) {
    VQ2_REQUIRE(idx && counts && flag, "index_hist: null pointer");
    VQ2_REQUIRE(M > 0 && M < ((int64_t)1 << 31) && K >= 1 && K <= 16384, "index_hist: need 1 <= M < 2^31 and 1 <= K <= 16384");
    const size_t lds = (size_t)K * sizeof(int);
    allow_big_lds(index_hist_kernel, lds);
    int64_t blocks = (M + 4095) / 4096;
    blocks = blocks > 256 ? 256 : blocks;
    hipLaunchKernelGGL(index_hist_kernel, dim3((unsigned)blocks), dim3(256), lds, to_stream(stream), idx, M, K,
                       reinterpret_cast<unsigned long long *>(counts), flag);
    return check_launch("index_hist_kernel");
}

extern "C" int vq2_eval_accumulate(const float *sse, int32_t N, int64_t elems_per_image, const float *diff, double *acc,
                                   vq2_stream_t stream) {
    VQ2_REQUIRE(sse && diff && acc && N > 0 && elems_per_image > 0, "eval_accumulate: bad arguments");
    hipLaunchKernelGGL(eval_accumulate_kernel, dim3(1), dim3(256), 0, to_stream(stream), sse, N, (double)elems_per_image,
                       diff, acc);
    return check_launch("eval_accumulate_kernel");
}

static inline int64_t im_tiles(int32_t H, int32_t W, int *tx, int *ty) {
    const int x = (W - (IM_WIN - 1) + IM_T - 1) / IM_T, y = (H - (IM_WIN - 1) + IM_T - 1) / IM_T;
    if (tx) *tx = x;
    if (ty) *ty = y;
    return (int64_t)x * y;
}

extern "C" size_t vq2_image_metrics_workspace_bytes(int32_t N, int32_t C, int32_t H, int32_t W) {
    if (N <= 0 || N > 65535 || C < 1 || C > 4 || H < IM_WIN || W < IM_WIN) return 0;
    return (size_t)N * (size_t)im_tiles(H, W, nullptr, nullptr) * (sizeof(double) + sizeof(unsigned long long));
}

extern "C" int vq2_image_metrics(const float *a, int32_t lda, const float *b, int32_t ldb, int32_t N, int32_t C, int32_t H,
                                 int32_t W, const float *inv_s, const float *mean, int64_t *sse_u8, double *ssim, void *ws,
                                 size_t ws_bytes, vq2_stream_t stream) {
    VQ2_REQUIRE(a && b && inv_s && mean && sse_u8 && ssim && ws, "image_metrics: null pointer");
    VQ2_REQUIRE(C >= 1 && C <= 4, "image_metrics: %d channels (1..4)", C);
    VQ2_REQUIRE(N >= 1 && N <= 65535, "image_metrics: %d images (1..65535)", N);
    VQ2_REQUIRE(lda >= C && ldb >= C, "image_metrics: pixel strides %d and %d are shorter than %d channels", lda, ldb, C);
    VQ2_REQUIRE(H >= IM_WIN && W >= IM_WIN, "image_metrics: a %dx%d image is smaller than the %dx%d window", H, W, IM_WIN, IM_WIN);
    for (int c = 0; c < C; ++c) VQ2_REQUIRE(inv_s[c] != 0.f, "image_metrics: inv_s[%d] is zero", c);
    ImParams P;
    const int64_t tiles = im_tiles(H, W, &P.tiles_x, &P.tiles_y);
    VQ2_REQUIRE(tiles < ((int64_t)1 << 31), "image_metrics: a %dx%d image has 2^31 tiles or more", H, W);
    const size_t slots = (size_t)N * (size_t)tiles;
    if (ws_bytes < slots * (sizeof(double) + sizeof(unsigned long long)))
        return set_error(VQ2_ERR_WORKSPACE, "image_metrics: workspace too small");
    VQ2_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7u) == 0, "image_metrics: the workspace must be 8-byte aligned");
    P.a = a; P.b = b; P.lda = lda; P.ldb = ldb;
    P.C = C; P.H = H; P.W = W;
    P.veca = lda == 4 && aligned16(a);
    P.vecb = ldb == 4 && aligned16(b);
    for (int c = 0; c < 4; ++c) { P.inv_s[c] = c < C ? inv_s[c] : 1.f; P.m[c] = c < C ? mean[c] : 0.f; }
    double gsum = 0.0;
    for (int k = 0; k < IM_WIN; ++k) {
        const double d = k - IM_WIN / 2;
        P.g[k] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
        gsum += P.g[k];
    }
    for (int k = 0; k < IM_WIN; ++k) P.g[k] /= gsum;
    P.part_s = static_cast<double *>(ws);
    P.part_e = reinterpret_cast<unsigned long long *>(P.part_s + slots);
    hipStream_t s = to_stream(stream);
    hipLaunchKernelGGL(image_metrics_kernel, dim3((unsigned)tiles, (unsigned)N), dim3(256), 0, s, P);
    if (int e = check_launch("image_metrics_kernel")) return e;
    hipLaunchKernelGGL(image_metrics_final_kernel, dim3((unsigned)N), dim3(64), 0, s, P.part_s, P.part_e, (int)tiles,
                       (double)(H - (IM_WIN - 1)) * (double)(W - (IM_WIN - 1)) * (double)C,
                       reinterpret_cast<long long *>(sse_u8), ssim);
    return check_launch("image_metrics_final_kernel");
}

extern "C" int vq2_image_metrics_accumulate(const int64_t *sse_u8, const double *ssim, int32_t N, int64_t *acc_i,
                                            double *acc_d, vq2_stream_t stream) {
    VQ2_REQUIRE(sse_u8 && ssim && acc_i && acc_d && N > 0, "image_metrics_accumulate: bad arguments");
    hipLaunchKernelGGL(image_metrics_accumulate_kernel, dim3(1), dim3(256), 0, to_stream(stream),
                       reinterpret_cast<const long long *>(sse_u8), ssim, N, reinterpret_cast<long long *>(acc_i), acc_d);
    return check_launch("image_metrics_accumulate_kernel");
}

extern "C" int vq2_prior_eval_rows(const float *logits, int32_t ld, const int64_t *target, int64_t M, int32_t n_class,
                                   float *row_nll, float *row_entropy, int32_t *row_rank, vq2_stream_t stream) {
    VQ2_REQUIRE(logits && target && row_nll && row_entropy && row_rank, "prior_eval_rows: null pointer");
    VQ2_REQUIRE(M >= 1 && M < ((int64_t)1 << 31), "prior_eval_rows: need 1 <= M < 2^31 rows");
    VQ2_REQUIRE(n_class >= 1 && n_class <= 16384, "prior_eval_rows: n_class must be in 1..16384, got %d", n_class);
    VQ2_REQUIRE(ld % 4 == 0 && ld >= (n_class + 3) / 4 * 4, "prior_eval_rows: row stride %d must be a multiple of 4 and >= ceil4(%d)",
                ld, n_class);
    VQ2_REQUIRE(aligned16(logits), "prior_eval_rows: the logits must be 16-byte aligned");
    const int64_t blocks = (M + 3) / 4;
    hipLaunchKernelGGL(prior_eval_rows_kernel, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(256), 0, to_stream(stream),
                       logits, ld, target, M, n_class, row_nll, row_entropy, row_rank);
    return check_launch("prior_eval_rows_kernel");
}

extern "C" int vq2_prior_eval_accumulate(const float *row_nll, const float *row_entropy, const int32_t *row_rank, int32_t N,
                                         int32_t L, int32_t top_k, double *pos_nll, double *pos_entropy, int64_t *pos_hit1,
                                         int64_t *pos_hitk, int64_t *counters, float *image_nll, vq2_stream_t stream) {
    VQ2_REQUIRE(row_nll && row_entropy && row_rank && pos_nll && pos_entropy && pos_hit1 && pos_hitk && counters,
                "prior_eval_accumulate: null pointer");
    VQ2_REQUIRE(N >= 1 && L >= 1 && top_k >= 1, "prior_eval_accumulate: need N >= 1, L >= 1 and top_k >= 1");
    VQ2_REQUIRE((int64_t)N * L < ((int64_t)1 << 31), "prior_eval_accumulate: 2^31 rows and more are not supported");
    VQ2_REQUIRE(((reinterpret_cast<uintptr_t>(pos_nll) | reinterpret_cast<uintptr_t>(pos_entropy) | reinterpret_cast<uintptr_t>(pos_hit1) |
                  reinterpret_cast<uintptr_t>(pos_hitk) | reinterpret_cast<uintptr_t>(counters)) & 7u) == 0,
                "prior_eval_accumulate: the state must be 8-byte aligned");
    const int PB = (L + 255) / 256;
    hipLaunchKernelGGL(prior_eval_accumulate_kernel, dim3((unsigned)(PB + 1 + (image_nll ? N : 0))), dim3(256), 0, to_stream(stream),
                       row_nll, row_entropy, row_rank, N, L, top_k, PB, pos_nll, pos_entropy, reinterpret_cast<long long *>(pos_hit1),
                       reinterpret_cast<long long *>(pos_hitk), reinterpret_cast<long long *>(counters), image_nll);
    return check_launch("prior_eval_accumulate_kernel");
}
