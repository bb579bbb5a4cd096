// HBM-bound helpers of the stage-1 step: layout conversion at the NCHW module boundary,
// fused ReLU backward, channel-slice copy/accumulate, MSE loss + gradient (train_vqvae.py:31,83),
// Adam (train_vqvae.py:185).  All 16-byte vectorised, grid-stride, deterministic reductions.
#include "vq2_common.h"

namespace vq2 {

static inline int grid_for(int64_t work_items, int cap = 4096) {
    int64_t b = (work_items + 255) / 256;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

// [N][C][HW] -> [N][HW][ld] through a 32x33 LDS tile; channels >= C are written as zeros
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const float *__restrict__ src, float *__restrict__ dst, int C,
                                                           int HW, int ld) {
    __shared__ float tile[32][33];
    const int n = blockIdx.z, p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    for (int j = ty; j < 32; j += 8) {
        const int c = c0 + j, p = p0 + tx;
        tile[j][tx] = (c < C && p < HW) ? src[((size_t)n * C + c) * HW + p] : 0.f;
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
        const int p = p0 + j, c = c0 + tx;
        if (p < HW && c < ld) dst[((size_t)n * HW + p) * ld + c] = tile[tx][j];
    }
}

__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(const float *__restrict__ src, float *__restrict__ dst, int C,
                                                           int HW, int ld) {
    __shared__ float tile[32][33];
    const int n = blockIdx.z, p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int j = ty; j < 32; j += 8) {
        const int p = p0 + j, c = c0 + tx;
        tile[j][tx] = (p < HW && c < C) ? src[((size_t)n * HW + p) * ld + c] : 0.f;
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
        const int c = c0 + j, p = p0 + tx;
        if (c < C && p < HW) dst[((size_t)n * C + c) * HW + p] = tile[tx][j];
    }
}

// C <= 4 with pixel stride 4 (the image / reconstruction): one thread per pixel, plane reads coalesce
// across threads, one 16-byte store (resp. load) per pixel
__global__ void nchw_to_nhwc4_kernel(const float *__restrict__ src, float4 *__restrict__ dst, int C, int64_t HW,
                                     int64_t total) {
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t n = g / HW, p = g - n * HW;
        const float *s = src + n * C * HW + p;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        v.x = s[0];
        if (C > 1) v.y = s[HW];
        if (C > 2) v.z = s[2 * HW];
        if (C > 3) v.w = s[3 * HW];
        dst[g] = v;
    }
}

__global__ void nhwc4_to_nchw_kernel(const float4 *__restrict__ src, float *__restrict__ dst, int C, int64_t HW,
                                     int64_t total) {
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t n = g / HW, p = g - n * HW;
        const float4 v = src[g];
        float *d = dst + n * C * HW + p;
        d[0] = v.x;
        if (C > 1) d[HW] = v.y;
        if (C > 2) d[2 * HW] = v.z;
        if (C > 3) d[3 * HW] = v.w;
    }
}

__global__ void relu_bwd_kernel(const float *__restrict__ dy, int lddy, const float *__restrict__ y, int ldy,
                                float *__restrict__ g, int ldg, int64_t pixels, int C4) {
    const int64_t total = pixels * C4;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = t / C4;
        const int c = (int)(t - p * C4) * 4;
        const float4 a = *reinterpret_cast<const float4 *>(dy + p * lddy + c);
        const float4 b = *reinterpret_cast<const float4 *>(y + p * ldy + c);
        float4 o;
        o.x = b.x > 0.f ? a.x : 0.f; o.y = b.y > 0.f ? a.y : 0.f; o.z = b.z > 0.f ? a.z : 0.f; o.w = b.w > 0.f ? a.w : 0.f;
        *reinterpret_cast<float4 *>(g + p * ldg + c) = o;
    }
}

__global__ void slice_copy_kernel(const float *__restrict__ src, int lds_, float *__restrict__ dst, int ldd,
                                  int64_t pixels, int C4, int accumulate) {
    const int64_t total = pixels * C4;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = t / C4;
        const int c = (int)(t - p * C4) * 4;
        float4 v = *reinterpret_cast<const float4 *>(src + p * lds_ + c);
        float4 *o = reinterpret_cast<float4 *>(dst + p * ldd + c);
        if (accumulate) { const float4 w = *o; v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w; }
        *o = v;
    }
}

constexpr int MSE_BLOCKS = 1024;

__global__ __launch_bounds__(256) void mse_partial_kernel(const float *__restrict__ a, const float *__restrict__ b,
                                                          int64_t n, float coef, const float *__restrict__ gscale,
                                                          float *__restrict__ grad, float *__restrict__ part) {
    __shared__ float wsum[4];
    const float gs = coef * (gscale ? gscale[0] : 1.f);
    float s = 0.f;
    const int64_t n4 = n / 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 x = reinterpret_cast<const float4 *>(a)[i], y = reinterpret_cast<const float4 *>(b)[i];
        const float d0 = x.x - y.x, d1 = x.y - y.y, d2 = x.z - y.z, d3 = x.w - y.w;
        s += d0 * d0; s += d1 * d1; s += d2 * d2; s += d3 * d3;
        if (grad) reinterpret_cast<float4 *>(grad)[i] = make_float4(gs * d0, gs * d1, gs * d2, gs * d3);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {  // ragged tail
        const int64_t i = n4 * 4 + threadIdx.x;
        const float d = a[i] - b[i];
        s += d * d;
        if (grad) grad[i] = gs * d;
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// latent != null: also total[0] = loss + weight * latent[0], the `recon_loss + 0.25 * latent_loss` of train_vqvae.py:85
// (same two fp32 operations as the stand-alone axpby launch it replaces)
__global__ void mse_final_kernel(const float *__restrict__ part, int nparts, float denom, float *__restrict__ loss,
                                 const float *__restrict__ latent, float weight, float *__restrict__ total) {
    __shared__ float red[256];
    float s = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 256) s += part[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float l = red[0] / denom;
        loss[0] = l;
        if (latent) total[0] = l + weight * latent[0];
    }
}

// torch.optim.Adam single-tensor math (lerp / addcmul / addcdiv), one pass over a flat arena
__global__ void adam_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                            float *__restrict__ v, int64_t n, float w1, float b2, float w2, float bc2_sqrt, float eps,
                            float neg_step, float gscale) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float gi = g[i] * gscale;
        float mi = m[i], vi = v[i];
        mi = mi + w1 * (gi - mi);                 // exp_avg.lerp_(grad, 1-beta1)
        vi = vi * b2 + (w2 * gi) * gi;            // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1-beta2)
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        p[i] = p[i] + neg_step * (mi / denom);    // param.addcdiv_(exp_avg, denom, value=-step_size)
        m[i] = mi;
        v[i] = vi;
    }
}

// ------------------------------------------------------------------ global gradient norm, clipped / averaged Adam
// The second path of the step tail, taken only on request (FusedAdam(clip_grad_norm=, ema_decay=)); adam_kernel above
// stays the default.  ctl (device, 4 floats) = [norm, coef, skip, skipped_total].
//   grad_norm_partial_kernel  part[b] = sum over block b's float4s of (g[i] * gscale)^2: the product in fp32 exactly as
//                             adam_kernel forms gi, squares and sums in fp64.  GN_BLOCKS caps the grid, so the block count
//                             is a function of n alone; a thread adds its elements in index order, a wave folds by xor
//                             shuffles, the four waves in wave order: no atomics, one order.
//   grad_norm_final_kernel    one wave: lane l adds its contiguous run of partials in index order, lane 0 adds the 64 lane
//                             sums in lane order; the same lane writes all of ctl.
//   adam_ex_kernel            adam_kernel's operations on gi = (g[i] * gscale) * coef, four elements per 16-byte access;
//                             AVG: p_avg += wavg * (p_new - p_avg) in the same pass.  ctl[2] != 0: every thread returns
//                             before its first store.
constexpr int GN_BLOCKS = 1024;
constexpr int ADAM_EX_BLOCKS = 2048;     // 8 waves on every SIMD of 256 CUs: one resident round

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const float4 *__restrict__ g, int64_t n4, float gscale,
                                                                double *__restrict__ part) {
    __shared__ double wsum[4];
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 x = g[i];
        const float a = x.x * gscale, b = x.y * gscale, c = x.z * gscale, d = x.w * gscale;
        s += (double)a * (double)a; s += (double)b * (double)b; s += (double)c * (double)c; s += (double)d * (double)d;
    }
    s = wave_sum_f64(s);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

__global__ __launch_bounds__(64) void grad_norm_final_kernel(const double *__restrict__ part, int nparts, double max_norm,
                                                             float *__restrict__ ctl) {
    __shared__ double lane_sum[64];
    const int run = (nparts + 63) / 64, lo = threadIdx.x * run, hi = min(lo + run, nparts);
    double s = 0.0;
    for (int i = lo; i < hi; ++i) s += part[i];
    lane_sum[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double total = 0.0;
    for (int l = 0; l < 64; ++l) total += lane_sum[l];
    const double norm = sqrt(total);
    const bool finite = norm - norm == 0.0;             // false for inf and NaN
    // torch.nn.utils.clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped to 1
    const double coef = finite ? fmin(1.0, max_norm / (norm + 1e-6)) : 0.0;
    ctl[0] = (float)norm;
    ctl[1] = (float)coef;
    ctl[2] = finite ? 0.f : 1.f;
    if (!finite) ctl[3] = ctl[3] + 1.f;
}

template <bool AVG>
__global__ __launch_bounds__(256) void adam_ex_kernel(float4 *__restrict__ p, const float4 *__restrict__ g,
                                                      float4 *__restrict__ m, float4 *__restrict__ v,
                                                      float4 *__restrict__ p_avg, int64_t n4, float w1, float b2, float w2,
                                                      float bc2_sqrt, float eps, float neg_step, float gscale,
                                                      const float *__restrict__ ctl, float wavg) {
    float coef = 1.f;
    if (ctl) {
        if (ctl[2] != 0.f) return;                      // a non-finite gradient norm: the step is skipped whole
        coef = ctl[1];
    }
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 g4 = g[i];
        float4 p4 = p[i], m4 = m[i], v4 = v[i], a4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (AVG) a4 = p_avg[i];
        const float gs[4] = {g4.x, g4.y, g4.z, g4.w};
        float *ps = &p4.x, *ms = &m4.x, *vs = &v4.x, *as = &a4.x;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float gi = (gs[k] * gscale) * coef;
            float mi = ms[k], vi = vs[k];
            mi = mi + w1 * (gi - mi);
            vi = vi * b2 + (w2 * gi) * gi;
            const float denom = sqrtf(vi) / bc2_sqrt + eps;
            const float pi = ps[k] + neg_step * (mi / denom);
            ps[k] = pi; ms[k] = mi; vs[k] = vi;
            if (AVG) as[k] = as[k] + wavg * (pi - as[k]);
        }
        p[i] = p4; m[i] = m4; v[i] = v4;
        if (AVG) p_avg[i] = a4;
    }
}

__global__ void axpby_kernel(const float *__restrict__ a, const float *__restrict__ b, float alpha,
                             float *__restrict__ dst, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = a[i] + alpha * b[i];
}

__global__ void scale_kernel(const float *__restrict__ src, const float *__restrict__ scalar, float alpha,
                             float *__restrict__ dst, int64_t n) {
    const float s = scalar[0] * alpha;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = src[i] * s;
}

// ------------------------------------------------------------------ 8-bit image -> normalised NHWC4
// ToTensor + Normalize (+ crop) + layout change of the reference's loader (train_vqvae.py:149-155,
// extract_code.py:47-53) in one pass: dst[n][y][x][c] = lut[c][src byte], pad lanes 0.  The table (built on the host
// with the reference's own fp32 operations, so the result does not depend on how a division is lowered here) sits in
// LDS.  A workgroup converts tiles of U8_TILE consecutive output pixels; thread t stores pixels t, t + 256, ... of the
// tile as one float4 each (consecutive lanes, consecutive 16-byte pixels).  DWORD: the tile's source bytes come in as
// aligned dwords, consecutive lanes consecutive dwords, through an LDS staging area -- HWC as the C * U8_TILE / 4
// dwords of the cropped byte stream (a lane's dword k: 4 pixels = 12 bytes in three loads at C = 3), CHW as one dword
// of 4 pixels per channel plane; the launcher checks that no dword straddles a row.  Otherwise single byte loads.
constexpr int U8_TILE = 1024;

struct U8Params {
    const uint8_t *src; const float *lut; float4 *dst;
    int64_t total;            // N * H * W output pixels
    int64_t ntiles;
    int C, H, W, Hs, Ws, y0, x0;
};

// source element offset of channel 0 of output pixel (row grow = n * H + y, column x)
template <int LAYOUT>
__device__ __forceinline__ int64_t u8_src_offset(const U8Params &P, int64_t grow, int x) {
    const int64_t n = grow / P.H;
    const int y = (int)(grow - n * P.H) + P.y0;
    if (LAYOUT == VQ2_U8_HWC) return ((n * P.Hs + y) * P.Ws + P.x0 + x) * P.C;
    return (n * P.C * P.Hs + y) * P.Ws + P.x0 + x;
}

template <int LAYOUT, bool DWORD>
__global__ __launch_bounds__(256) void u8_to_nhwc4_kernel(const U8Params P) {
    __shared__ float lut[4 * 256];
    __shared__ uint32_t stage[DWORD ? U8_TILE : 1];   // U8_TILE pixels x <= 4 bytes
    const int t = threadIdx.x, C = P.C;
    for (int i = t; i < C * 256; i += 256) lut[i] = P.lut[i];
    __syncthreads();
    const int64_t plane = (int64_t)P.Hs * P.Ws;
    for (int64_t tile = blockIdx.x; tile < P.ntiles; tile += gridDim.x) {
        const int64_t tile0 = tile * U8_TILE;
        if (DWORD) {
            if (LAYOUT == VQ2_U8_HWC) {
                // byte stream of the cropped image: rows of W * C bytes (a multiple of 4, as is every row's start)
                const uint32_t rowb = (uint32_t)P.W * C;
                const int64_t s0 = tile0 * C, row0 = s0 / rowb;
                const uint32_t off0 = (uint32_t)(s0 - row0 * rowb);
                for (int k = 0; k < C; ++k) {
                    const uint32_t d = t + 256 * k;
                    if (s0 + 4 * (int64_t)d < P.total * C) {
                        const uint32_t u = off0 + 4 * d, r = u / rowb;
                        const int64_t o = u8_src_offset<LAYOUT>(P, row0 + r, 0) + (u - r * rowb);
                        stage[d] = *reinterpret_cast<const uint32_t *>(P.src + o);
                    }
                }
            } else if (tile0 + 4 * t < P.total) {
                // 4 consecutive pixels of one row (W, x0 and Ws are multiples of 4): one dword per channel plane
                const int64_t row0 = tile0 / P.W;
                const uint32_t u = (uint32_t)(tile0 - row0 * P.W) + 4 * t, r = u / (uint32_t)P.W;
                const int64_t o = u8_src_offset<LAYOUT>(P, row0 + r, (int)(u - r * (uint32_t)P.W));
                for (int c = 0; c < C; ++c)
                    stage[c * (U8_TILE / 4) + t] = *reinterpret_cast<const uint32_t *>(P.src + o + c * plane);
            }
            __syncthreads();
        }
        const uint8_t *sb = reinterpret_cast<const uint8_t *>(stage);
#pragma unroll
        for (int j = 0; j < U8_TILE / 256; ++j) {
            const int q = j * 256 + t;
            const int64_t g = tile0 + q;
            if (g >= P.total) break;
            uint32_t b[4] = {0, 0, 0, 0};
            if (DWORD) {
                for (int c = 0; c < C; ++c) b[c] = LAYOUT == VQ2_U8_HWC ? sb[q * C + c] : sb[c * U8_TILE + q];
            } else {
                const int64_t grow = g / P.W;
                const int64_t o = u8_src_offset<LAYOUT>(P, grow, (int)(g - grow * P.W));
                for (int c = 0; c < C; ++c) b[c] = P.src[o + (LAYOUT == VQ2_U8_HWC ? c : c * plane)];
            }
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            v.x = lut[b[0]];
            if (C > 1) v.y = lut[256 + b[1]];
            if (C > 2) v.z = lut[512 + b[2]];
            if (C > 3) v.w = lut[768 + b[3]];
            P.dst[g] = v;
        }
        if (DWORD) __syncthreads();   // the staging area is refilled by the next tile
    }
}

}  // namespace vq2

using namespace vq2;

// (format strings by name: tests/test_host_cpu.py's census of conv label families reads the literal ones)
static const char NCHW4_LABEL[] = "nchw_to_nhwc4|N=%d,H=%d,W=%d,C=%d";
static const char U8_LABEL[] = "u8_to_nhwc4|N=%d,H=%d,W=%d,C=%d,%s,%s";

extern "C" int vq2_nchw_to_nhwc(const float *src, float *dst, int32_t N, int32_t C, int32_t H, int32_t W, int32_t ld,
                                vq2_stream_t stream) {
    VQ2_REQUIRE(src && dst && N > 0 && C > 0 && H > 0 && W > 0 && ld >= C, "nchw_to_nhwc: bad arguments");
    if (ld == 4 && aligned16(dst)) {
        const int64_t HW4 = (int64_t)H * W, total = HW4 * N;
        ProfScope prof(prof_level() ? prof_label(NCHW4_LABEL, N, H, W, C) : "", 0.0, (double)total * (4 * C + 16),
                       to_stream(stream));
        hipLaunchKernelGGL(nchw_to_nhwc4_kernel, dim3(grid_for(total)), dim3(256), 0, to_stream(stream), src,
                           reinterpret_cast<float4 *>(dst), C, HW4, total);
        return check_launch("nchw_to_nhwc4_kernel");
    }
    VQ2_REQUIRE(N <= 65535, "nchw_to_nhwc: batch > 65535");
    const int HW = H * W;
    dim3 grid((HW + 31) / 32, (ld + 31) / 32, N);
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, grid, dim3(256), 0, to_stream(stream), src, dst, C, HW, ld);
    return check_launch("nchw_to_nhwc_kernel");
}

extern "C" int vq2_u8_to_nhwc4(const uint8_t *src, int layout, int32_t N, int32_t C, int32_t Hs, int32_t Ws, int32_t y0,
                               int32_t x0, int32_t H, int32_t W, const float *lut, float *dst, vq2_stream_t stream) {
    VQ2_REQUIRE(src && lut && dst, "u8_to_nhwc4: null pointer");
    VQ2_REQUIRE(layout == VQ2_U8_HWC || layout == VQ2_U8_CHW, "u8_to_nhwc4: layout %d is neither VQ2_U8_HWC nor VQ2_U8_CHW", layout);
    VQ2_REQUIRE(C >= 1 && C <= 4, "u8_to_nhwc4: %d channels (1..4 fit the 4-float pixel)", C);
    VQ2_REQUIRE(N > 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0, "u8_to_nhwc4: non-positive dimension");
    VQ2_REQUIRE(y0 >= 0 && x0 >= 0 && (int64_t)y0 + H <= Hs && (int64_t)x0 + W <= Ws,
                "u8_to_nhwc4: crop %dx%d at (%d, %d) leaves the %dx%d source", H, W, y0, x0, Hs, Ws);
    VQ2_REQUIRE(aligned16(dst), "u8_to_nhwc4: dst must be 16-byte aligned");
    VQ2_REQUIRE((int64_t)Ws * C < (1 << 30), "u8_to_nhwc4: source rows of 2^30 bytes and more are not supported");
    U8Params P;
    P.src = src; P.lut = lut; P.dst = reinterpret_cast<float4 *>(dst);
    P.total = (int64_t)N * H * W;
    P.ntiles = (P.total + U8_TILE - 1) / U8_TILE;
    P.C = C; P.H = H; P.W = W; P.Hs = Hs; P.Ws = Ws; P.y0 = y0; P.x0 = x0;
    // dword loads need every row segment to start and end on a 4-byte boundary of the source
    const bool hwc = layout == VQ2_U8_HWC;
    const int unit = hwc ? C : 1;   // bytes per pixel within one row segment
    const bool dword = (reinterpret_cast<uintptr_t>(src) & 3u) == 0 && ((int64_t)W * unit) % 4 == 0 &&
                       ((int64_t)x0 * unit) % 4 == 0 && ((int64_t)Ws * unit) % 4 == 0;
    hipStream_t s = to_stream(stream);
    ProfScope prof(prof_level() ? prof_label(U8_LABEL, N, H, W, C, hwc ? "hwc" : "chw", dword ? "dword" : "byte") : "",
                   0.0, (double)P.total * (C + 16), s);
    const dim3 grid((unsigned)(P.ntiles < 2048 ? P.ntiles : 2048)), block(256);
    if (hwc && dword) hipLaunchKernelGGL((u8_to_nhwc4_kernel<VQ2_U8_HWC, true>), grid, block, 0, s, P);
    else if (hwc) hipLaunchKernelGGL((u8_to_nhwc4_kernel<VQ2_U8_HWC, false>), grid, block, 0, s, P);
    else if (dword) hipLaunchKernelGGL((u8_to_nhwc4_kernel<VQ2_U8_CHW, true>), grid, block, 0, s, P);
    else hipLaunchKernelGGL((u8_to_nhwc4_kernel<VQ2_U8_CHW, false>), grid, block, 0, s, P);
    return check_launch("u8_to_nhwc4_kernel");
}

extern "C" int vq2_nhwc_to_nchw(const float *src, float *dst, int32_t N, int32_t C, int32_t H, int32_t W, int32_t ld,
                                vq2_stream_t stream) {
    VQ2_REQUIRE(src && dst && N > 0 && C > 0 && H > 0 && W > 0 && ld >= C, "nhwc_to_nchw: bad arguments");
    if (ld == 4 && aligned16(src)) {
        const int64_t HW4 = (int64_t)H * W, total = HW4 * N;
        hipLaunchKernelGGL(nhwc4_to_nchw_kernel, dim3(grid_for(total)), dim3(256), 0, to_stream(stream),
                           reinterpret_cast<const float4 *>(src), dst, C, HW4, total);
        return check_launch("nhwc4_to_nchw_kernel");
    }
    VQ2_REQUIRE(N <= 65535, "nhwc_to_nchw: batch > 65535");
    const int HW = H * W;
    dim3 grid((HW + 31) / 32, (C + 31) / 32, N);
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, grid, dim3(256), 0, to_stream(stream), src, dst, C, HW, ld);
    return check_launch("nhwc_to_nchw_kernel");
}

extern "C" int vq2_relu_bwd(const float *dy, int32_t lddy, const float *y, int32_t ldy, float *g, int32_t ldg,
                            int64_t pixels, int32_t C, vq2_stream_t stream) {
    VQ2_REQUIRE(dy && y && g && pixels > 0 && C > 0 && C % 4 == 0, "relu_bwd: need C %% 4 == 0");
    VQ2_REQUIRE(lddy >= C && ldy >= C && ldg >= C && lddy % 4 == 0 && ldy % 4 == 0 && ldg % 4 == 0,
                "relu_bwd: bad pixel strides");
    VQ2_REQUIRE(aligned16(dy) && aligned16(y) && aligned16(g), "relu_bwd: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(relu_bwd_kernel, dim3(grid_for(pixels * (C / 4))), dim3(256), 0, to_stream(stream), dy, lddy, y,
                       ldy, g, ldg, pixels, C / 4);
    return check_launch("relu_bwd_kernel");
}

extern "C" int vq2_slice_copy(const float *src, int32_t lds_, float *dst, int32_t ldd, int64_t pixels, int32_t C,
                              int accumulate, vq2_stream_t stream) {
    VQ2_REQUIRE(src && dst && pixels > 0 && C > 0 && C % 4 == 0 && lds_ >= C && ldd >= C && lds_ % 4 == 0 && ldd % 4 == 0,
                "slice_copy: bad arguments");
    VQ2_REQUIRE(aligned16(src) && aligned16(dst), "slice_copy: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(slice_copy_kernel, dim3(grid_for(pixels * (C / 4))), dim3(256), 0, to_stream(stream), src, lds_,
                       dst, ldd, pixels, C / 4, accumulate);
    return check_launch("slice_copy_kernel");
}

extern "C" size_t vq2_mse_workspace_bytes(int64_t numel) { return numel > 0 ? MSE_BLOCKS * sizeof(float) : 0; }

static int mse_impl(const float *a, const float *b, int64_t numel, int64_t denom, const float *gscale, float *loss,
                    float *grad, const float *latent, float weight, float *total, void *ws, size_t ws_bytes,
                    vq2_stream_t stream);

extern "C" int vq2_mse_fwd_bwd(const float *a, const float *b, int64_t numel, int64_t denom, const float *gscale,
                               float *loss, float *grad, void *ws, size_t ws_bytes, vq2_stream_t stream) {
    return mse_impl(a, b, numel, denom, gscale, loss, grad, nullptr, 0.f, nullptr, ws, ws_bytes, stream);
}

extern "C" int vq2_stage1_loss(const float *a, const float *b, int64_t numel, int64_t denom, const float *latent,
                               float weight, float *recon, float *total, float *grad, void *ws, size_t ws_bytes,
                               vq2_stream_t stream) {
    VQ2_REQUIRE(latent && total, "stage1_loss: null pointer");
    return mse_impl(a, b, numel, denom, nullptr, recon, grad, latent, weight, total, ws, ws_bytes, stream);
}

static int mse_impl(const float *a, const float *b, int64_t numel, int64_t denom, const float *gscale, float *loss,
                    float *grad, const float *latent, float weight, float *total, void *ws, size_t ws_bytes,
                    vq2_stream_t stream) {
    VQ2_REQUIRE(a && b && loss && ws && numel > 0 && denom > 0, "mse: bad arguments");
    VQ2_REQUIRE(aligned16(a) && aligned16(b) && (!grad || aligned16(grad)), "mse: pointers must be 16-byte aligned");
    VQ2_REQUIRE(ws_bytes >= MSE_BLOCKS * sizeof(float), "mse: workspace too small");
    const int blocks = grid_for(numel / 4 + 1, MSE_BLOCKS);
    hipStream_t s = to_stream(stream);
    hipLaunchKernelGGL(mse_partial_kernel, dim3(blocks), dim3(256), 0, s, a, b, numel, (float)(2.0 / (double)denom),
                       gscale, grad, static_cast<float *>(ws));
    if (int e = check_launch("mse_partial_kernel")) return e;
    hipLaunchKernelGGL(mse_final_kernel, dim3(1), dim3(256), 0, s, static_cast<const float *>(ws), blocks,
                       (float)denom, loss, latent, weight, total);
    return check_launch("mse_final_kernel");
}

extern "C" int vq2_adam_step(float *p, const float *g, float *m, float *v, int64_t n, double lr, double beta1,
                             double beta2, double eps, int32_t step, double grad_scale, vq2_stream_t stream) {
    VQ2_REQUIRE(p && g && m && v && n > 0 && step >= 1, "adam: bad arguments");
    // scalar prep in double exactly as torch/optim/adam.py does on the host
    const double bc1 = 1.0 - pow(beta1, (double)step);
    const double bc2 = 1.0 - pow(beta2, (double)step);
    const double step_size = lr / bc1;
    const double bc2_sqrt = sqrt(bc2);
    hipLaunchKernelGGL(adam_kernel, dim3(grid_for(n)), dim3(256), 0, to_stream(stream), p, g, m, v, n,
                       (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)bc2_sqrt, (float)eps,
                       (float)(-step_size), (float)grad_scale);
    return check_launch("adam_kernel");
}

extern "C" size_t vq2_grad_norm_workspace_bytes(int64_t n) { return n > 0 ? GN_BLOCKS * sizeof(double) : 0; }

extern "C" int vq2_grad_norm(const float *g, int64_t n, double grad_scale, double max_norm, float *ctl, void *ws,
                             size_t ws_bytes, vq2_stream_t stream) {
    VQ2_REQUIRE(g && ctl && ws, "grad_norm: null pointer");
    VQ2_REQUIRE(n > 0 && n % 4 == 0, "grad_norm: n = %lld must be a positive multiple of 4", (long long)n);
    VQ2_REQUIRE(aligned16(g) && aligned16(ctl) && aligned16(ws), "grad_norm: pointers must be 16-byte aligned");
    VQ2_REQUIRE(max_norm > 0.0, "grad_norm: max_norm must be positive (+inf: measure only), got %g", max_norm);  // NaN fails too
    VQ2_REQUIRE(ws_bytes >= GN_BLOCKS * sizeof(double), "grad_norm: workspace too small");
    const int blocks = grid_for(n / 4, GN_BLOCKS);
    hipStream_t s = to_stream(stream);
    hipLaunchKernelGGL(grad_norm_partial_kernel, dim3(blocks), dim3(256), 0, s, reinterpret_cast<const float4 *>(g), n / 4,
                       (float)grad_scale, static_cast<double *>(ws));
    if (int e = check_launch("grad_norm_partial_kernel")) return e;
    hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(64), 0, s, static_cast<const double *>(ws), blocks, max_norm, ctl);
    return check_launch("grad_norm_final_kernel");
}

extern "C" int vq2_adam_step_ex(float *p, const float *g, float *m, float *v, float *p_avg, int64_t n, double lr,
                                double beta1, double beta2, double eps, int32_t step, double grad_scale, const float *ctl,
                                double avg_decay, vq2_stream_t stream) {
    VQ2_REQUIRE(p && g && m && v && step >= 1, "adam_ex: bad arguments");
    VQ2_REQUIRE(n > 0 && n % 4 == 0, "adam_ex: n = %lld must be a positive multiple of 4", (long long)n);
    VQ2_REQUIRE(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && aligned16(p_avg),
                "adam_ex: pointers must be 16-byte aligned");
    VQ2_REQUIRE(avg_decay >= 0.0 && avg_decay < 1.0, "adam_ex: avg_decay must lie in [0, 1), got %g", avg_decay);  // NaN fails too
    // scalar prep as in vq2_adam_step
    const double bc1 = 1.0 - pow(beta1, (double)step);
    const double bc2 = 1.0 - pow(beta2, (double)step);
    const double step_size = lr / bc1;
    const double bc2_sqrt = sqrt(bc2);
    hipStream_t s = to_stream(stream);
    const dim3 grid(grid_for(n / 4, ADAM_EX_BLOCKS)), block(256);
#define VQ2_ADAM_EX(AVG)                                                                                                  \
    hipLaunchKernelGGL(adam_ex_kernel<AVG>, grid, block, 0, s, reinterpret_cast<float4 *>(p),                             \
                       reinterpret_cast<const float4 *>(g), reinterpret_cast<float4 *>(m), reinterpret_cast<float4 *>(v), \
                       reinterpret_cast<float4 *>(p_avg), n / 4, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2),  \
                       (float)bc2_sqrt, (float)eps, (float)(-step_size), (float)grad_scale, ctl, (float)(1.0 - avg_decay))
    if (p_avg) VQ2_ADAM_EX(true);
    else VQ2_ADAM_EX(false);
#undef VQ2_ADAM_EX
    return check_launch("adam_ex_kernel");
}

extern "C" int vq2_axpby(const float *a, const float *b, float alpha, float *dst, int64_t n, vq2_stream_t stream) {
    VQ2_REQUIRE(a && b && dst && n > 0, "axpby: bad arguments");
    hipLaunchKernelGGL(axpby_kernel, dim3(grid_for(n)), dim3(256), 0, to_stream(stream), a, b, alpha, dst, n);
    return check_launch("axpby_kernel");
}

extern "C" int vq2_scale(const float *src, const float *scalar, float alpha, float *dst, int64_t n,
                         vq2_stream_t stream) {
    VQ2_REQUIRE(src && scalar && dst && n > 0, "scale: bad arguments");
    hipLaunchKernelGGL(scale_kernel, dim3(grid_for(n)), dim3(256), 0, to_stream(stream), src, scalar, alpha, dst, n);
    return check_launch("scale_kernel");
}

// ------------------------------------------------------------------ calibration (not on the product path)
// Register-resident v_mfma_f32_32x32x2_f32 loop: what the chip sustains for this instruction at the
// clock it holds under load -- the practical ceiling the conv kernels are measured against in DESIGN.md.
__global__ __launch_bounds__(256) void mfma_peak_kernel(float *out, int iters, float seed) {
    f32x16 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    float a = seed + threadIdx.x * 1e-3f, b = seed - threadIdx.x * 2e-3f;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[i], 0, 0, 0);
            a += 1e-6f;
        }
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) s += acc[i][r];
    if (s == 123.456f) out[0] = s;  // keep the loop alive
}

// the same arithmetic rate through v_mfma_f32_16x16x4_f32 (32 cycles per instruction, half the FLOPs): does the chip
// hold a different clock for this shape (MI355X_MICROARCH.md, DVFS note 7)?
typedef float f32x4v __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void mfma_peak16_kernel(float *out, int iters, float seed) {
    f32x4v acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = f32x4v{0.f, 0.f, 0.f, 0.f};
    float a = seed + threadIdx.x * 1e-3f, b = seed - threadIdx.x * 2e-3f;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[i], 0, 0, 0);
            a += 1e-6f;
        }
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    if (s == 123.456f) out[0] = s;
}

extern "C" int vq2_debug_mfma_peak16(float *scratch, int32_t blocks, int32_t iters, vq2_stream_t stream) {
    VQ2_REQUIRE(scratch && blocks > 0 && iters > 0, "mfma_peak16: bad arguments");
    hipLaunchKernelGGL(mfma_peak16_kernel, dim3(blocks), dim3(256), 0, to_stream(stream), scratch, iters, 0.5f);
    return check_launch("mfma_peak16_kernel");
}

extern "C" int vq2_debug_mfma_peak(float *scratch, int32_t blocks, int32_t iters, vq2_stream_t stream) {
    VQ2_REQUIRE(scratch && blocks > 0 && iters > 0, "mfma_peak: bad arguments");
    hipLaunchKernelGGL(mfma_peak_kernel, dim3(blocks), dim3(256), 0, to_stream(stream), scratch, iters, 0.5f);
    return check_launch("mfma_peak_kernel");
}
