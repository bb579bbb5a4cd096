// The two ends of the stage-2 prior (PixelSNAIL, pixelsnail.py:397-431 and train_pixelsnail.py:39-48) and the x2 upsample
// between them.
//
//   one-hot convolution   conv(one_hot(idx), w) is a row lookup: per output pixel and tap one row of Co floats of the weight,
//                         chosen by the class the tap lands on.  The weight is repacked per forward to [tap][class][ceil4(Co)]
//                         so that the row is contiguous and a lane reads 16 bytes of it; the row / column shift of
//                         shift_down / shift_right and the `horizontal + vertical` add are part of the same launch.  The weight
//                         gradient is the scatter by class, done without atomics: one workgroup per (class, 256 output
//                         channels, 8 taps) scans the index map in raster order, finds its pixels with a ballot, and adds their dy rows
//                         tap by tap in that order, in double.  The bias gradient is a two-stage column sum in a fixed order.
//   cross-entropy head    one wave per row of logits: maximum and arg-max (lowest index wins a tie), sum of exponentials,
//                         NLL term and hit; one workgroup then sums rows in a fixed order.  The backward writes
//                         (exp((l - max) - log_sum) - [c == target]) * g / M from the logits and the two saved row values.
//   nearest x2 upsample   forward a copy to four places, backward ((g00 + g01) + g10) + g11.
//
// Every index that comes from data (a class, a target) is range-checked before it forms an address.  64-bit addressing
// throughout; pad lanes C .. ceil4(C) - 1 of every NHWC output are written as 0.  No floating-point atomics anywhere: two runs
// give the same bits.
#include "vq2_common.h"

namespace vq2 {

static inline int prior_grid(int64_t work_items) {
    const int64_t b = (work_items + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}
static inline int up4(int c) { return (c + 3) / 4 * 4; }

__device__ __forceinline__ float4 real_lanes(float4 v, int c, int C) {
    if (c + 1 >= C) v.y = 0.f;
    if (c + 2 >= C) v.z = 0.f;
    if (c + 3 >= C) v.w = 0.f;
    return v;
}

// (pixel, first channel of the group) of work item t; see split_item of vq2_gated.hip
__device__ __forceinline__ void split_item(int64_t t, int groups, bool small, int64_t &p, int &c) {
    if (small) {
        const uint32_t q = (uint32_t)t / (uint32_t)groups;
        p = q;
        c = (int)((uint32_t)t - q * (uint32_t)groups) * 4;
    } else {
        p = t / groups;
        c = (int)(t - p * groups) * 4;
    }
}

struct OneHot {
    int N, H, W, Co, Cop, ncls, KH, KW, pt, pl, sd, sr;
};

// ----------------------------------------------------------------------------- one-hot conv: weight repack
// w [Co][ncls][T] (OIHW with T = KH * KW) -> wp [T][ncls][Cop], lanes Co .. Cop - 1 zero.  One workgroup per (class, 64 output
// channels): the 64 runs of T contiguous floats go through LDS so that both sides are read / written in runs.
__global__ __launch_bounds__(256) void onehot_pack_kernel(const float *__restrict__ w, float *__restrict__ wp, int Co, int Cop,
                                                          int ncls, int T) {
    __shared__ float tile[64 * 33];
    const int cls = blockIdx.x, co0 = blockIdx.y * 64;
    for (int i = threadIdx.x; i < 64 * T; i += 256) {
        const int c = i / T, t = i - c * T;
        tile[c * 33 + t] = (co0 + c < Co) ? w[((int64_t)(co0 + c) * ncls + cls) * T + t] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * T; i += 256) {
        const int t = i >> 6, c = i & 63;
        if (co0 + c < Cop) wp[((int64_t)t * ncls + cls) * Cop + co0 + c] = tile[c * 33 + t];
    }
}

// ----------------------------------------------------------------------------- one-hot conv: forward
// y[n,h,w,:] = [acc[n,h,w,:] +] (h >= sd && w >= sr ? bias + sum_taps wp[tap][idx[n, h - sd - pt + kh, w - sr - pl + kw]] : 0)
__global__ __launch_bounds__(256) void onehot_conv_fwd_kernel(const int64_t *__restrict__ idx, const float *__restrict__ wp,
                                                              const float *__restrict__ bias, const float *__restrict__ acc,
                                                              int ldacc, float *__restrict__ y, int ldy, const OneHot g) {
    const int G = g.Cop / 4;
    const int64_t total = (int64_t)g.N * g.H * g.W * G;
    const bool small = total < ((int64_t)1 << 31);
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        int64_t p;
        int c;
        split_item(t, G, small, p, c);
        const int wq = (int)(p % g.W);
        const int64_t nh = p / g.W;
        const int hq = (int)(nh % g.H);
        const int64_t n = nh / g.H;
        const int hs = hq - g.sd, ws = wq - g.sr;          // the pixel of the unshifted conv output that lands here
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (hs >= 0 && ws >= 0) {
            if (bias) {
                o.x = bias[c];
                if (c + 1 < g.Co) o.y = bias[c + 1];
                if (c + 2 < g.Co) o.z = bias[c + 2];
                if (c + 3 < g.Co) o.w = bias[c + 3];
            }
            for (int kh = 0; kh < g.KH; ++kh) {
                const int hi = hs - g.pt + kh;
                if (hi < 0 || hi >= g.H) continue;
                for (int kw = 0; kw < g.KW; ++kw) {
                    const int wi = ws - g.pl + kw;
                    if (wi < 0 || wi >= g.W) continue;
                    const int64_t cls = idx[(n * g.H + hi) * g.W + wi];
                    if ((uint64_t)cls >= (uint64_t)g.ncls) continue;          // out of range: contributes nothing, reads nothing
                    const float4 r = *reinterpret_cast<const float4 *>(wp + ((int64_t)(kh * g.KW + kw) * g.ncls + cls) * g.Cop + c);
                    o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w;
                }
            }
        }
        if (acc) {
            const float4 a = *reinterpret_cast<const float4 *>(acc + p * ldacc + c);
            o.x += a.x; o.y += a.y; o.z += a.z; o.w += a.w;
        }
        *reinterpret_cast<float4 *>(y + p * ldy + c) = real_lanes(o, c, g.Co);
    }
}

// ----------------------------------------------------------------------------- one-hot conv: weight gradient
// Workgroup (class, chunk of 256 output channels, group of 8 taps), thread = output channel.  The index map is scanned 256
// pixels at a time; the pixels that hold the class are found with one ballot per wave and visited in raster order by every
// thread, so each sum has one fixed order.  An input pixel (hq, wq) is read by tap (kh, kw) of the conv output at
// (hq + pt - kh, wq + pl - kw), which the shift moves to (+ sd, + sr); pixels the shift pushes off the image have no gradient.
#define OH_TAPS 8
__global__ __launch_bounds__(256) void onehot_wgrad_kernel(const int64_t *__restrict__ idx, const float *__restrict__ dy,
                                                           int lddy, float *__restrict__ dw, const OneHot g) {
    __shared__ unsigned long long hits[4];
    const int T = g.KH * g.KW;
    const int cls = blockIdx.x;
    const int co = blockIdx.y * 256 + threadIdx.x;
    const int t0 = blockIdx.z * OH_TAPS;                 // this workgroup's taps: t0 .. min(t0 + 8, T) - 1
    const int nt = min(OH_TAPS, T - t0);
    const int kh0 = t0 / g.KW, kw0 = t0 - kh0 * g.KW;
    const bool active = co < g.Co;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc[OH_TAPS];
#pragma unroll
    for (int t = 0; t < OH_TAPS; ++t) acc[t] = 0.0;
    const int M = g.N * g.H * g.W;                       // < 2^31, checked by the host
    for (int base = 0; base < M; base += 256) {
        const int q = base + threadIdx.x;
        const bool match = q < M && idx[q] == (int64_t)cls;
        const unsigned long long b = __ballot(match);
        __syncthreads();                                 // the previous round's readers are done
        if (lane == 0) hits[wave] = b;
        __syncthreads();
        if (!active) continue;
        for (int wv = 0; wv < 4; ++wv) {
            unsigned long long bits = hits[wv];
            while (bits) {
                const int j = __ffsll((long long)bits) - 1;
                bits &= bits - 1;
                const int qq = base + wv * 64 + j;
                const int wq = qq % g.W;
                const int nh = qq / g.W;
                const int hq = nh % g.H;
                const int64_t row0 = (int64_t)(nh - hq) * g.W;      // first pixel of image n
                // tap t = kh * KW + kw lands on (hq + pt + sd - kh, wq + pl + sr - kw): walk the taps in order
                const int wf0 = wq + g.pl + g.sr;
                int hf = hq + g.pt + g.sd - kh0, wf = wf0 - kw0, kw = kw0;
#pragma unroll
                for (int t = 0; t < OH_TAPS; ++t) {
                    if (t < nt) {
                        if (hf >= g.sd && hf < g.H && wf >= g.sr && wf < g.W)
                            acc[t] += (double)dy[(row0 + (int64_t)hf * g.W + wf) * lddy + co];
                        --wf;
                        if (++kw == g.KW) { kw = 0; wf = wf0; --hf; }
                    }
                }
            }
        }
    }
    if (active) {
        float *out = dw + ((int64_t)co * g.ncls + cls) * T + t0;
#pragma unroll
        for (int t = 0; t < OH_TAPS; ++t)
            if (t < nt) out[t] = (float)acc[t];
    }
}

// bias gradient, stage 1: slab s = rows [s * 64, s * 64 + 64) of dy, thread = output channel, shifted-in pixels skipped
__global__ __launch_bounds__(256) void onehot_bgrad_partial_kernel(const float *__restrict__ dy, int lddy, double *__restrict__ part,
                                                                   const OneHot g) {
    const int co = blockIdx.y * 256 + threadIdx.x;
    if (co >= g.Co) return;
    const int M = g.N * g.H * g.W;
    const int r0 = blockIdx.x * 64, r1 = min(r0 + 64, M);
    double s = 0.0;
    for (int r = r0; r < r1; ++r) {
        const int wq = r % g.W, hq = (r / g.W) % g.H;
        if (hq >= g.sd && wq >= g.sr) s += (double)dy[(int64_t)r * lddy + co];
    }
    part[(int64_t)blockIdx.x * g.Co + co] = s;
}

// stage 2: slabs in ascending order
__global__ __launch_bounds__(256) void onehot_bgrad_final_kernel(const double *__restrict__ part, int slabs, int Co,
                                                                 float *__restrict__ db) {
    const int co = blockIdx.x * 256 + threadIdx.x;
    if (co >= Co) return;
    double s = 0.0;
    for (int i = 0; i < slabs; ++i) s += part[(int64_t)i * Co + co];
    db[co] = (float)s;
}

// ----------------------------------------------------------------------------- cross-entropy
__device__ __forceinline__ void take_max(float &m, int &am, float v, int c) {
    if (v > m) { m = v; am = c; }
}

// one wave per row.  stat[row] = (max, log of the sum of exp(l - max)); nll[row]; ok[row] = arg-max == target
__global__ __launch_bounds__(256) void xent_rows_kernel(const float *__restrict__ logits, int ld, const int64_t *__restrict__ target,
                                                        int64_t M, int ncls, float *__restrict__ stat, float *__restrict__ nll,
                                                        int32_t *__restrict__ ok) {
    const int lane = threadIdx.x & 63;
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < M; row += (int64_t)gridDim.x * 4) {
        const float *x = logits + row * ld;
        float m = -INFINITY;
        int am = 0x7fffffff;
        for (int c = lane * 4; c < ncls; c += 256) {        // ascending c with a strict compare: the lowest index of a lane's maximum
            const float4 v = *reinterpret_cast<const float4 *>(x + c);
            take_max(m, am, v.x, c);
            if (c + 1 < ncls) take_max(m, am, v.y, c + 1);
            if (c + 2 < ncls) take_max(m, am, v.z, c + 2);
            if (c + 3 < ncls) take_max(m, am, v.w, c + 3);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float om = __shfl_xor(m, o, 64);
            const int oa = __shfl_xor(am, o, 64);
            if (om > m || (om == m && oa < am)) { m = om; am = oa; }
        }
        float s = 0.f;
        for (int c = lane * 4; c < ncls; c += 256) {
            const float4 v = *reinterpret_cast<const float4 *>(x + c);
            s += expf(v.x - m);
            if (c + 1 < ncls) s += expf(v.y - m);
            if (c + 2 < ncls) s += expf(v.z - m);
            if (c + 3 < ncls) s += expf(v.w - m);
        }
        s = wave_sum(s);
        if (lane == 0) {
            const float ls = logf(s);
            const int64_t t = target[row];
            const bool valid = (uint64_t)t < (uint64_t)ncls;          // out of range: no loss term, no hit, no gradient
            stat[row * 2] = m;
            stat[row * 2 + 1] = ls;
            nll[row] = valid ? ls - (x[t] - m) : 0.f;
            ok[row] = (valid && (int64_t)am == t) ? 1 : 0;
        }
    }
}

// one workgroup: thread i sums rows i, i + 256, ... in double, then a tree over LDS; loss = mean, accuracy = hits / M, count = hits
__global__ __launch_bounds__(256) void xent_reduce_kernel(const float *__restrict__ nll, const int32_t *__restrict__ ok, int64_t M,
                                                          float *__restrict__ loss, float *__restrict__ accuracy,
                                                          int32_t *__restrict__ count) {
    __shared__ double ssum[256];
    __shared__ int scnt[256];
    double s = 0.0;
    int n = 0;
    for (int64_t r = threadIdx.x; r < M; r += 256) {
        s += (double)nll[r];
        n += ok[r];
    }
    ssum[threadIdx.x] = s;
    scnt[threadIdx.x] = n;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            ssum[threadIdx.x] += ssum[threadIdx.x + o];
            scnt[threadIdx.x] += scnt[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        loss[0] = (float)(ssum[0] / (double)M);
        accuracy[0] = (float)scnt[0] / (float)M;
        count[0] = scnt[0];
    }
}

__global__ __launch_bounds__(256) void xent_bwd_kernel(const float *__restrict__ logits, int ld, const int64_t *__restrict__ target,
                                                       const float *__restrict__ stat, const float *__restrict__ gout, int64_t M,
                                                       int ncls, float *__restrict__ dl, int lddl) {
    const int G = (ncls + 3) / 4;
    const int64_t total = M * G;
    const bool small = total < ((int64_t)1 << 31);
    const float scale = gout[0] / (float)M;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        int64_t row;
        int c;
        split_item(i, G, small, row, c);
        const int64_t t = target[row];
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((uint64_t)t < (uint64_t)ncls) {
            const float m = stat[row * 2], ls = stat[row * 2 + 1];
            const float4 v = *reinterpret_cast<const float4 *>(logits + row * ld + c);
            const int tc = (int)t - c;
            o.x = (expf((v.x - m) - ls) - (tc == 0 ? 1.f : 0.f)) * scale;
            o.y = (expf((v.y - m) - ls) - (tc == 1 ? 1.f : 0.f)) * scale;
            o.z = (expf((v.z - m) - ls) - (tc == 2 ? 1.f : 0.f)) * scale;
            o.w = (expf((v.w - m) - ls) - (tc == 3 ? 1.f : 0.f)) * scale;
        }
        *reinterpret_cast<float4 *>(dl + row * lddl + c) = real_lanes(o, c, ncls);
    }
}

// ----------------------------------------------------------------------------- nearest x2 upsample
// y [N, 2H, 2W, C]: y[n, ho, wo] = x[n, ho / 2, wo / 2]
__global__ __launch_bounds__(256) void upsample2_fwd_kernel(const float *__restrict__ x, int ldx, float *__restrict__ y, int ldy,
                                                            int64_t N, int H, int W, int C) {
    const int G = (C + 3) / 4;
    const int64_t total = N * (2 * H) * (2 * W) * G;
    const bool small = total < ((int64_t)1 << 31);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        int64_t p;
        int c;
        split_item(i, G, small, p, c);
        const int wo = (int)(p % (2 * W));
        const int64_t nh = p / (2 * W);
        const int ho = (int)(nh % (2 * H));
        const int64_t n = nh / (2 * H);
        const float4 v = *reinterpret_cast<const float4 *>(x + ((n * H + ho / 2) * W + wo / 2) * ldx + c);
        *reinterpret_cast<float4 *>(y + p * ldy + c) = real_lanes(v, c, C);
    }
}

// dx [N, H, W, C] = ((dy[2h, 2w] + dy[2h, 2w + 1]) + dy[2h + 1, 2w]) + dy[2h + 1, 2w + 1]
__global__ __launch_bounds__(256) void upsample2_bwd_kernel(const float *__restrict__ dy, int lddy, float *__restrict__ dx, int lddx,
                                                            int64_t N, int H, int W, int C) {
    const int G = (C + 3) / 4;
    const int64_t total = N * H * W * G;
    const bool small = total < ((int64_t)1 << 31);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        int64_t p;
        int c;
        split_item(i, G, small, p, c);
        const int w = (int)(p % W);
        const int64_t nh = p / W;
        const int h = (int)(nh % H);
        const int64_t n = nh / H;
        const float *r0 = dy + ((n * 2 * H + 2 * h) * (2 * W) + 2 * w) * lddy + c;
        const float *r1 = r0 + (int64_t)(2 * W) * lddy;
        const float4 a = *reinterpret_cast<const float4 *>(r0), b = *reinterpret_cast<const float4 *>(r0 + lddy);
        const float4 d = *reinterpret_cast<const float4 *>(r1), e = *reinterpret_cast<const float4 *>(r1 + lddy);
        float4 o;
        o.x = ((a.x + b.x) + d.x) + e.x; o.y = ((a.y + b.y) + d.y) + e.y;
        o.z = ((a.z + b.z) + d.z) + e.z; o.w = ((a.w + b.w) + d.w) + e.w;
        *reinterpret_cast<float4 *>(dx + p * lddx + c) = real_lanes(o, c, C);
    }
}

// ----------------------------------------------------------------------------- host side
static int rows_ok(const char *what, const void *ptr, int ld, int C) {
    VQ2_REQUIRE(ld % 4 == 0 && ld >= up4(C), "%s: pixel stride %d must be a multiple of 4 and >= ceil4(%d)", what, ld, C);
    VQ2_REQUIRE(ptr != nullptr, "%s: null pointer", what);
    VQ2_REQUIRE(aligned16(ptr), "%s: pointers must be 16-byte aligned", what);
    return VQ2_OK;
}

static int onehot_ok(const char *what, const vq2_onehot_desc *d, OneHot &g) {
    VQ2_REQUIRE(d != nullptr, "%s: null descriptor", what);
    VQ2_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->Co > 0 && d->Co <= (1 << 24), "%s: bad shape", what);
    VQ2_REQUIRE((int64_t)d->N * d->H * d->W < ((int64_t)1 << 31), "%s: N * H * W must be below 2^31", what);
    VQ2_REQUIRE(d->n_class >= 1 && d->n_class <= 16384, "%s: n_class must be in 1..16384, got %d", what, d->n_class);
    VQ2_REQUIRE(d->KH >= 1 && d->KH <= 7 && d->KW >= 1 && d->KW <= 7 && d->KH * d->KW <= 32,
                "%s: kernel sides in 1..7 with at most 32 taps, got %d x %d", what, d->KH, d->KW);
    VQ2_REQUIRE(d->pad_top >= 0 && d->pad_top < d->KH && d->pad_left >= 0 && d->pad_left < d->KW, "%s: bad padding", what);
    VQ2_REQUIRE((d->shift_down == 0 || d->shift_down == 1) && (d->shift_right == 0 || d->shift_right == 1),
                "%s: shifts must be 0 or 1", what);
    g.N = d->N; g.H = d->H; g.W = d->W; g.Co = d->Co; g.Cop = up4(d->Co); g.ncls = d->n_class;
    g.KH = d->KH; g.KW = d->KW; g.pt = d->pad_top; g.pl = d->pad_left; g.sd = d->shift_down; g.sr = d->shift_right;
    return VQ2_OK;
}

}  // namespace vq2

using namespace vq2;

extern "C" int vq2_onehot_pack_weight(const float *w, float *wp, int32_t Co, int32_t n_class, int32_t KH, int32_t KW,
                                      vq2_stream_t stream) {
    vq2_onehot_desc d{1, 1, 1, Co, n_class, KH, KW, 0, 0, 0, 0, up4(Co)};
    OneHot g;
    if (int e = onehot_ok("onehot_pack_weight", &d, g)) return e;
    VQ2_REQUIRE(w != nullptr && wp != nullptr && aligned16(wp), "onehot_pack_weight: null or misaligned pointer");
    hipLaunchKernelGGL(onehot_pack_kernel, dim3(n_class, (g.Cop + 63) / 64), dim3(256), 0, to_stream(stream), w, wp, Co, g.Cop,
                       n_class, KH * KW);
    return check_launch("onehot_pack_kernel");
}

extern "C" int vq2_onehot_conv_fwd(const vq2_onehot_desc *d, const int64_t *idx, const float *wp, const float *bias,
                                   const float *acc, int32_t ldacc, float *y, vq2_stream_t stream) {
    OneHot g;
    if (int e = onehot_ok("onehot_conv_fwd", d, g)) return e;
    VQ2_REQUIRE(idx != nullptr && wp != nullptr && aligned16(wp), "onehot_conv_fwd: null or misaligned pointer");
    if (int e = rows_ok("onehot_conv_fwd y", y, d->ldy, d->Co)) return e;
    if (acc)
        if (int e = rows_ok("onehot_conv_fwd acc", acc, ldacc, d->Co)) return e;
    const int64_t items = (int64_t)g.N * g.H * g.W * (g.Cop / 4);
    hipLaunchKernelGGL(onehot_conv_fwd_kernel, dim3(prior_grid(items)), dim3(256), 0, to_stream(stream), idx, wp, bias, acc, ldacc,
                       y, d->ldy, g);
    return check_launch("onehot_conv_fwd_kernel");
}

extern "C" size_t vq2_onehot_conv_wgrad_workspace_bytes(const vq2_onehot_desc *d) {
    if (!d || d->N <= 0 || d->H <= 0 || d->W <= 0 || d->Co <= 0) return 0;
    const int64_t M = (int64_t)d->N * d->H * d->W;
    return (size_t)((M + 63) / 64) * (size_t)d->Co * sizeof(double);
}

extern "C" int vq2_onehot_conv_wgrad(const vq2_onehot_desc *d, const int64_t *idx, const float *dy, float *dw, float *db,
                                     void *ws, size_t ws_bytes, vq2_stream_t stream) {
    OneHot g;
    if (int e = onehot_ok("onehot_conv_wgrad", d, g)) return e;
    VQ2_REQUIRE(idx != nullptr && dw != nullptr, "onehot_conv_wgrad: null pointer");
    if (int e = rows_ok("onehot_conv_wgrad dy", dy, d->ldy, d->Co)) return e;
    hipLaunchKernelGGL(onehot_wgrad_kernel, dim3(g.ncls, (g.Co + 255) / 256, (g.KH * g.KW + OH_TAPS - 1) / OH_TAPS), dim3(256), 0, to_stream(stream), idx, dy, d->ldy, dw, g);
    if (int e = check_launch("onehot_wgrad_kernel")) return e;
    if (db) {
        const int slabs = (int)(((int64_t)g.N * g.H * g.W + 63) / 64);
        if (ws == nullptr || ws_bytes < vq2_onehot_conv_wgrad_workspace_bytes(d) || (reinterpret_cast<uintptr_t>(ws) & 7u))
            return set_error(VQ2_ERR_WORKSPACE, "onehot_conv_wgrad: workspace too small or misaligned");
        hipLaunchKernelGGL(onehot_bgrad_partial_kernel, dim3(slabs, (g.Co + 255) / 256), dim3(256), 0, to_stream(stream), dy, d->ldy,
                           static_cast<double *>(ws), g);
        if (int e = check_launch("onehot_bgrad_partial_kernel")) return e;
        hipLaunchKernelGGL(onehot_bgrad_final_kernel, dim3((g.Co + 255) / 256), dim3(256), 0, to_stream(stream),
                           static_cast<const double *>(ws), slabs, g.Co, db);
        return check_launch("onehot_bgrad_final_kernel");
    }
    return VQ2_OK;
}

static int xent_ok(const char *what, int64_t M, int32_t n_class) {
    VQ2_REQUIRE(M > 0 && M < ((int64_t)1 << 36), "%s: bad row count", what);
    VQ2_REQUIRE(n_class >= 1 && n_class <= 16384, "%s: n_class must be in 1..16384, got %d", what, n_class);
    return VQ2_OK;
}

extern "C" int vq2_xent_fwd(const float *logits, int32_t ld, const int64_t *target, int64_t M, int32_t n_class, float *stat,
                            float *row_nll, int32_t *row_ok, float *loss, float *accuracy, int32_t *correct, vq2_stream_t stream) {
    if (int e = xent_ok("xent_fwd", M, n_class)) return e;
    if (int e = rows_ok("xent_fwd", logits, ld, n_class)) return e;
    VQ2_REQUIRE(target && stat && row_nll && row_ok && loss && accuracy && correct, "xent_fwd: null pointer");
    hipLaunchKernelGGL(xent_rows_kernel, dim3(prior_grid(M * 64)), dim3(256), 0, to_stream(stream), logits, ld, target, M, n_class,
                       stat, row_nll, row_ok);
    if (int e = check_launch("xent_rows_kernel")) return e;
    hipLaunchKernelGGL(xent_reduce_kernel, dim3(1), dim3(256), 0, to_stream(stream), row_nll, row_ok, M, loss, accuracy, correct);
    return check_launch("xent_reduce_kernel");
}

extern "C" int vq2_xent_bwd(const float *logits, int32_t ld, const int64_t *target, const float *stat, const float *gout,
                            int64_t M, int32_t n_class, float *dlogits, int32_t lddl, vq2_stream_t stream) {
    if (int e = xent_ok("xent_bwd", M, n_class)) return e;
    if (int e = rows_ok("xent_bwd logits", logits, ld, n_class)) return e;
    if (int e = rows_ok("xent_bwd dlogits", dlogits, lddl, n_class)) return e;
    VQ2_REQUIRE(target && stat && gout, "xent_bwd: null pointer");
    hipLaunchKernelGGL(xent_bwd_kernel, dim3(prior_grid(M * (up4(n_class) / 4))), dim3(256), 0, to_stream(stream), logits, ld, target,
                       stat, gout, M, n_class, dlogits, lddl);
    return check_launch("xent_bwd_kernel");
}

static int upsample_ok(const char *what, int32_t N, int32_t H, int32_t W, int32_t C) {
    VQ2_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C <= (1 << 24) && H < (1 << 30) && W < (1 << 30) &&
                    (int64_t)N * H * W < ((int64_t)1 << 34), "%s: bad shape", what);
    return VQ2_OK;
}

extern "C" int vq2_upsample2_fwd(const float *x, int32_t ldx, float *y, int32_t ldy, int32_t N, int32_t H, int32_t W, int32_t C,
                                 vq2_stream_t stream) {
    if (int e = upsample_ok("upsample2_fwd", N, H, W, C)) return e;
    if (int e = rows_ok("upsample2_fwd x", x, ldx, C)) return e;
    if (int e = rows_ok("upsample2_fwd y", y, ldy, C)) return e;
    hipLaunchKernelGGL(upsample2_fwd_kernel, dim3(prior_grid((int64_t)N * H * W * 4 * (up4(C) / 4))), dim3(256), 0, to_stream(stream),
                       x, ldx, y, ldy, (int64_t)N, H, W, C);
    return check_launch("upsample2_fwd_kernel");
}

extern "C" int vq2_upsample2_bwd(const float *dy, int32_t lddy, float *dx, int32_t lddx, int32_t N, int32_t H, int32_t W,
                                 int32_t C, vq2_stream_t stream) {
    if (int e = upsample_ok("upsample2_bwd", N, H, W, C)) return e;
    if (int e = rows_ok("upsample2_bwd dy", dy, lddy, C)) return e;
    if (int e = rows_ok("upsample2_bwd dx", dx, lddx, C)) return e;
    hipLaunchKernelGGL(upsample2_bwd_kernel, dim3(prior_grid((int64_t)N * H * W * (up4(C) / 4))), dim3(256), 0, to_stream(stream), dy,
                       lddy, dx, lddx, (int64_t)N, H, W, C);
    return check_launch("upsample2_bwd_kernel");
}
