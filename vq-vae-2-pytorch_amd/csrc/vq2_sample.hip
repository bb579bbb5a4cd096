// Sampling from the stage-2 prior one image row at a time (the reference's sample.py:17-29 evaluates the whole model on
// rows 0..i for every pixel; every layer is causal in raster order, so only row i is new).
//
//   row convolution    output row `row` of a causal conv (pad_top == KH - 1) from input rows kept in a history with its own
//                      image and row strides.  The GEMM is small in M (N * W pixels) and long in K (KH * KW * Ci), so K is
//                      split over taps: convg_row_partial_kernel writes one [M][Co] slab per split, convg_row_reduce_kernel
//                      adds the slabs in ascending order and applies the epilogue of vq2_conv_fwd.  No atomics: two runs
//                      give the same bits.  v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation) with the
//                      weight panel rows on the A side and the pixels on the B side: a lane then holds 4 consecutive output
//                      channels of one pixel and stores 16 bytes.  Both operands come straight from global memory as float4
//                      reads of 4 consecutive input channels (k step s of an MFMA quadruple takes channel 4 * g + s from
//                      both sides, as in vq2_attn.hip); the four waves of a workgroup share the panel rows through the
//                      vector cache and differ in their 32 pixels.  It reads the VQ2_PACK_FWD panel [Co][tap][Ci].
//   column convolution  output pixel (row, col) of the same conv for all N images: M = N, so the weight panel is the traffic.
//                      Work is cut into steps of (one computed tap, 64 input channels); a workgroup owns 32 output channels
//                      and one contiguous range of steps, its four waves take 16 channels of a step each (a float4 per lane
//                      from either side, every panel element read once per 64 images) and add their accumulators through
//                      LDS in wave order.  convg_col_partial_kernel writes one [N][Co] slab per range,
//                      convg_row_reduce_kernel (M = N) adds the slabs in ascending order with the epilogue.  The same
//                      v_mfma_f32_16x16x4_f32 with the images on the 16-wide B side; taps outside the image are skipped for
//                      the whole grid (row and col are launch constants).  No atomics.
//   categorical draw   one wave per row of logits: maximum, sum of exponentials over lane-contiguous chunks, a fixed-order
//                      scan over the lanes, then every lane walks its chunk for the first class whose running sum passes
//                      u * sum; the lowest such lane wins.  u comes from Philox4x32-7 keyed by (seed, position, row).
//   filtered draw      the same draw over a top-k / nucleus truncated support (semantics: include/vq2.h).  Both cuts are
//                      thresholds on z, found by bisection over the order-preserving 32-bit key of z: a pass counts, or sums
//                      in the draw's own order, the classes at or above a candidate key.  A removed class adds 0.f, so with
//                      the filters off the sums, and the code, are the plain draw's bit for bit.
#include "vq2_conv.h"
#include "vq2_philox.h"

namespace {

using vq2::philox4x32_7;

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

constexpr int RC_BM = 128;   // pixels per workgroup: 4 waves x 32
constexpr int RC_BN = 64;    // output channels per workgroup (every wave computes all of them)

struct RowConv {
    const float *x, *w;
    float *ws;
    long long x_image_stride, x_row_stride;
    int W, Ci, Co, KH, KW, pad_left, ldx, row, M, K;
    int relu_in;
    unsigned tap_mask;   // bit t: tap t = kh * KW + kw is computed
    int tps;             // active taps per split
};

// the computed taps kh * KW + kw, ascending, and their number (VQ2_ROW_CAUSAL_TAPS: the last kernel row ends before its centre)
static int computed_taps(const vq2_conv_desc *d, int flags, unsigned char *taps) {
    int n = 0;
    for (int kh = 0; kh < d->KH; ++kh)
        for (int kw = 0; kw < d->KW; ++kw) {
            if ((flags & VQ2_ROW_CAUSAL_TAPS) && kh == d->KH - 1 && kw >= d->KW / 2) continue;
            taps[n++] = (unsigned char)(kh * d->KW + kw);
        }
    return n;
}

// which taps are computed and how they are cut into splits: a function of the shape and the flags alone
struct RowPlan { unsigned mask; int ntaps, tps, splits; };
static RowPlan row_plan(const vq2_conv_desc *d, int flags) {
    RowPlan p{0u, 0, 1, 1};
    unsigned char taps[32];
    p.ntaps = computed_taps(d, flags, taps);
    for (int t = 0; t < p.ntaps; ++t) p.mask |= 1u << taps[t];
    if (p.ntaps == 0) return p;   // a 1 x 1 'causal' kernel: nothing but the bias
    const long tiles = (((long)d->N * d->W + RC_BM - 1) / RC_BM) * ((d->Co + RC_BN - 1) / RC_BN);
    long want = (512 + tiles - 1) / tiles;          // about two workgroups per compute unit
    if (want > p.ntaps) want = p.ntaps;
    p.tps = (int)((p.ntaps + want - 1) / want);
    p.splits = (p.ntaps + p.tps - 1) / p.tps;
    return p;
}

__global__ __launch_bounds__(256) void convg_row_partial_kernel(const RowConv P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
    const int m0 = blockIdx.x * RC_BM + wave * 32, co0 = blockIdx.y * RC_BN, split = blockIdx.z;
    int pn[2], pw[2], pp[2];
    bool pv[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        pp[mt] = m0 + 16 * mt + col;
        pv[mt] = pp[mt] < P.M;
        pn[mt] = pp[mt] / P.W;
        pw[mt] = pp[mt] - pn[mt] * P.W;
    }
    const float *wrow[4];
    bool wv[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int co = co0 + 16 * nt + col;
        wv[nt] = co < P.Co;
        wrow[nt] = P.w + (size_t)(wv[nt] ? co : 0) * P.K;
    }
    f32x4 acc[4][2];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) acc[nt][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int t0 = split * P.tps, t1 = t0 + P.tps;
    const int T = P.KH * P.KW;
    int active = 0;
    for (int tap = 0; tap < T; ++tap) {
        if (!((P.tap_mask >> tap) & 1u)) continue;
        const int ai = active++;
        if (ai < t0 || ai >= t1) continue;
        const int kh = tap / P.KW, kw = tap - kh * P.KW;
        const int r = P.row - (P.KH - 1) + kh;
        if (r < 0) continue;                                   // above the image: zeros (workgroup-uniform)
        const float *xp[2];
        bool xv[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int wi = pw[mt] - P.pad_left + kw;
            xv[mt] = pv[mt] && wi >= 0 && wi < P.W;
            xp[mt] = P.x + (xv[mt] ? (long long)pn[mt] * P.x_image_stride + (long long)r * P.x_row_stride + (long long)wi * P.ldx : 0ll);
        }
        const int koff = tap * P.Ci;
        for (int c0 = 0; c0 < P.Ci; c0 += 16) {
            const int c = c0 + 4 * g;
            const bool cv = c < P.Ci;
            float4 a[4], b[2];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
                a[nt] = (wv[nt] && cv) ? *reinterpret_cast<const float4 *>(wrow[nt] + koff + c) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                b[mt] = (xv[mt] && cv) ? *reinterpret_cast<const float4 *>(xp[mt] + c) : make_float4(0.f, 0.f, 0.f, 0.f);
                if (P.relu_in) b[mt] = vq2::relu4(b[mt]);
            }
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    acc[nt][mt] = mfma4(a[nt].x, b[mt].x, acc[nt][mt]);
                    acc[nt][mt] = mfma4(a[nt].y, b[mt].y, acc[nt][mt]);
                    acc[nt][mt] = mfma4(a[nt].z, b[mt].z, acc[nt][mt]);
                    acc[nt][mt] = mfma4(a[nt].w, b[mt].w, acc[nt][mt]);
                }
        }
    }
    // accumulator register r of lane (col, g) is output channel 16 * nt + 4 * g + r of pixel col
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        if (!pv[mt]) continue;
        float *dst = P.ws + ((size_t)split * P.M + pp[mt]) * P.Co;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const int co = co0 + 16 * nt + 4 * g;
            if (co < P.Co)
                *reinterpret_cast<float4 *>(dst + co) = make_float4(acc[nt][mt][0], acc[nt][mt][1], acc[nt][mt][2], acc[nt][mt][3]);
        }
    }
}

// y = [relu](((slab 0 + slab 1) + ...) + bias [+ residual]), pad lanes Cor .. Co - 1 written as 0
__global__ __launch_bounds__(256) void convg_row_reduce_kernel(const float *__restrict__ ws, int splits, int M, int Co, int Cor,
                                                               const float *__restrict__ bias, const float *__restrict__ res,
                                                               int ldres, float *__restrict__ y, int ldy, int relu_out) {
    const int G = Co / 4;
    const long total = (long)M * G;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int p = (int)(t / G), c = (int)(t - (long)p * G) * 4;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < splits; ++k) {
        const float4 v = *reinterpret_cast<const float4 *>(ws + ((size_t)k * M + p) * Co + c);
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    float o[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (c + k >= Cor) { o[k] = 0.f; continue; }
        if (bias) o[k] += bias[c + k];
        if (res) o[k] += res[(size_t)p * ldres + c + k];
        if (relu_out) o[k] = fmaxf(o[k], 0.f);
    }
    *reinterpret_cast<float4 *>(y + (size_t)p * ldy + c) = make_float4(o[0], o[1], o[2], o[3]);
}

// ----------------------------------------------------------------------------- column convolution
constexpr int CC_BN = 32;    // output channels per workgroup: 2 MFMA tiles, every wave computes both
constexpr int CC_BK = 64;    // input channels per step: 16 per wave

struct ColConv {
    const float *x, *w;
    float *ws;
    long long x_image_stride, x_row_stride;
    int N, W, Ci, Co, KH, KW, pad_left, ldx, row, col, K;
    int relu_in;
    int cb;              // channel blocks per tap: ceil(Ci / CC_BK)
    int steps, sps;      // steps = computed taps * cb; steps per split
    unsigned char taps[32];   // the computed taps (kh * KW + kw), ascending
};

// which taps are computed and how the steps are cut into splits: a function of the shape and the flags alone
struct ColPlan { unsigned char taps[32]; int ntaps, cb, steps, sps, splits, mt; };
static ColPlan col_plan(const vq2_conv_desc *d, int flags) {
    ColPlan p{};
    p.ntaps = computed_taps(d, flags, p.taps);
    p.cb = (d->Ci + CC_BK - 1) / CC_BK;
    p.steps = p.ntaps * p.cb;
    p.mt = d->N <= 16 ? 1 : 4;                       // image tiles of 16 per workgroup
    p.sps = 1;
    p.splits = 1;
    if (p.steps == 0) return p;                      // a 1 x 1 'causal' kernel: nothing but the bias
    const long tiles = (long)((d->Co + CC_BN - 1) / CC_BN) * ((d->N + 16 * p.mt - 1) / (16 * p.mt));
    long want = (512 + tiles - 1) / tiles;           // about two workgroups per compute unit
    // a slab is written and read once: keep that at or below half the panel's bytes (splits * N <= K / 4)
    const long cap = (long)p.ntaps * d->Ci / (4l * d->N);
    if (want > cap) want = cap;
    if (want > p.steps) want = p.steps;
    if (want < 1) want = 1;
    p.sps = (int)((p.steps + want - 1) / want);
    p.splits = (p.steps + p.sps - 1) / p.sps;
    return p;
}

template <int MT>
__global__ __launch_bounds__(256) void convg_col_partial_kernel(const ColConv P) {
    __shared__ float4 red[4][2 * MT][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
    const int co0 = blockIdx.x * CC_BN, split = blockIdx.y, n0 = blockIdx.z * (16 * MT);
    const float *wrow[2];
    bool wv[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int co = co0 + 16 * nt + col;
        wv[nt] = co < P.Co;
        wrow[nt] = P.w + (size_t)(wv[nt] ? co : 0) * P.K;
    }
    const float *ximg[MT];
    bool pv[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int n = n0 + 16 * mt + col;
        pv[mt] = n < P.N;
        ximg[mt] = P.x + (pv[mt] ? (long long)n * P.x_image_stride : 0ll);
    }
    f32x4 acc[2][MT];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int s0 = split * P.sps, s1 = min(s0 + P.sps, P.steps);
    for (int step = s0; step < s1; ++step) {
        const int ai = step / P.cb, c = (step - ai * P.cb) * CC_BK + wave * 16 + 4 * g;
        const int tap = P.taps[ai];
        const int kh = tap / P.KW, kw = tap - kh * P.KW;
        const int r = P.row - (P.KH - 1) + kh, wi = P.col - P.pad_left + kw;
        if (r < 0 || wi < 0 || wi >= P.W) continue;            // outside the image: zeros (the same for the whole grid)
        const bool cv = c < P.Ci;
        const long long xoff = (long long)r * P.x_row_stride + (long long)wi * P.ldx + c;
        const int koff = tap * P.Ci + c;
        float4 a[2], b[MT];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
            a[nt] = (wv[nt] && cv) ? *reinterpret_cast<const float4 *>(wrow[nt] + koff) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            b[mt] = (pv[mt] && cv) ? *reinterpret_cast<const float4 *>(ximg[mt] + xoff) : make_float4(0.f, 0.f, 0.f, 0.f);
            if (P.relu_in) b[mt] = vq2::relu4(b[mt]);
        }
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                acc[nt][mt] = mfma4(a[nt].x, b[mt].x, acc[nt][mt]);
                acc[nt][mt] = mfma4(a[nt].y, b[mt].y, acc[nt][mt]);
                acc[nt][mt] = mfma4(a[nt].z, b[mt].z, acc[nt][mt]);
                acc[nt][mt] = mfma4(a[nt].w, b[mt].w, acc[nt][mt]);
            }
    }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
            red[wave][nt * MT + mt][lane] = make_float4(acc[nt][mt][0], acc[nt][mt][1], acc[nt][mt][2], acc[nt][mt][3]);
    __syncthreads();
    // the four waves' sums in wave order; accumulator register r of lane (col, g) is output channel 16 * nt + 4 * g + r of
    // image col of its tile
    for (int e = threadIdx.x; e < 2 * MT * 64; e += 256) {
        const int t = e >> 6, l = e & 63, nt = t / MT, mt = t - nt * MT;
        const int n = n0 + 16 * mt + (l & 15), co = co0 + 16 * nt + 4 * (l >> 4);
        if (n >= P.N || co >= P.Co) continue;
        float4 s = red[0][t][l];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const float4 v = red[w][t][l];
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        *reinterpret_cast<float4 *>(P.ws + ((size_t)split * P.N + n) * P.Co + co) = s;
    }
}

// ----------------------------------------------------------------------------- categorical draw
__device__ __forceinline__ float uniform_of(uint32_t seed_lo, uint32_t seed_hi, uint32_t pos_lo, uint32_t pos_hi, uint32_t row) {
    const uint4 w = philox4x32_7(pos_lo, pos_hi, row, 0u, seed_lo, seed_hi);
    return (float)(w.x >> 8) * 5.9604644775390625e-08f;   // 2^-24: u in [0, 1), exact
}

// -- the pieces both draw kernels are made of (one wave per row; lane `lane` owns classes c0 .. c1 - 1)
__device__ __forceinline__ float wave_max(float mx) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    return mx;
}

// inclusive scan of the lanes' chunk sums in one fixed tree; excl is the sum of the lanes below, the return value the total
__device__ __forceinline__ float lane_scan(float s, int lane, float &excl) {
    float incl = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = 0.f;
    return __shfl(incl, 63, 64);
}

// the class of the lowest lane that found one, else `fallback`
__device__ __forceinline__ int lowest_hit(int found, int fallback, int &winner) {
    const unsigned long long hit = __ballot(found >= 0);
    winner = hit ? __ffsll((long long)hit) - 1 : 0;
    return hit ? __shfl(found, winner, 64) : fallback;
}

__global__ __launch_bounds__(256) void sample_categorical_kernel(const float *__restrict__ logits, long long row_stride, int M,
                                                                 int n_class, float temperature, uint32_t seed_lo,
                                                                 uint32_t seed_hi, uint32_t pos_lo, uint32_t pos_hi,
                                                                 long long *__restrict__ out, long long out_stride) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;                                      // whole waves leave: no shuffle crosses a wave
    const float *l = logits + (long long)row * row_stride;
    const int chunk = (n_class + 63) / 64;
    const int c0 = min(lane * chunk, n_class), c1 = min(c0 + chunk, n_class);
    float mx = -INFINITY;
    for (int c = c0; c < c1; ++c) mx = fmaxf(mx, l[c] / temperature);
    mx = wave_max(mx);
    float s = 0.f;
    for (int c = c0; c < c1; ++c) s += expf(l[c] / temperature - mx);
    float excl;
    const float total = lane_scan(s, lane, excl);
    const float thr = uniform_of(seed_lo, seed_hi, pos_lo, pos_hi, (uint32_t)row) * total;
    // running sum at class c of this lane: excl + (own exponentials up to c, in order); first class that passes thr
    int found = -1;
    float run = 0.f;
    for (int c = c0; c < c1; ++c) {
        run += expf(l[c] / temperature - mx);
        if (excl + run > thr) { found = c; break; }
    }
    int winner;
    const int cls = lowest_hit(found, n_class - 1, winner);    // rounding left no class above thr: the last one
    if (lane == 0) out[(long long)row * out_stride] = (long long)cls;
}

// -- the draw from a truncated support (top-k, then nucleus)
// z in an unsigned key of the same order (z >= v  <=>  key(z) >= key(v) for non-NaN values; -0 counts as +0)
__device__ __forceinline__ uint32_t order_key(float z) {
    const uint32_t b = z == 0.f ? 0u : __float_as_uint(z);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

constexpr int SF_REG = 8;            // a lane's chunk for n_class <= 512: z and e stay in registers
constexpr int SF_LDS_FLOATS = 16384; // larger rows: z staged in LDS, 64 KB at the most

// a lane's chunk of z = l / temperature and e = exp(z - max).  REG: both in registers, every loop unrolled over SF_REG
// guarded slots.  Otherwise z sits in the wave's LDS slab at [k][lane] (a lane reads back only what it wrote: no barrier,
// no bank conflict) and e is formed again where it is needed -- expf of the same arguments, so the same bits.
template <bool REG> struct Chunk {
    float z[REG ? SF_REG : 1], e[REG ? SF_REG : 1];
    float *slab;
    float mx;
    int cnt;
    template <class F> __device__ __forceinline__ void each(F f) const {
        if constexpr (REG) {
#pragma unroll
            for (int k = 0; k < SF_REG; ++k)
                if (k < cnt) f(k, z[k], e[k]);
        } else {
            for (int k = 0; k < cnt; ++k) {
                const float zk = slab[k * 64];
                f(k, zk, expf(zk - mx));
            }
        }
    }
    template <class F> __device__ __forceinline__ void each_z(F f) const {
        if constexpr (REG) {
#pragma unroll
            for (int k = 0; k < SF_REG; ++k)
                if (k < cnt) f(z[k]);
        } else {
            for (int k = 0; k < cnt; ++k) f(slab[k * 64]);
        }
    }
};

template <bool REG>
__global__ __launch_bounds__(256) void sample_filtered_kernel(const float *__restrict__ logits, long long row_stride, int M,
                                                              int n_class, float temperature, int top_k, float top_p,
                                                              uint32_t seed_lo, uint32_t seed_hi, uint32_t pos_lo, uint32_t pos_hi,
                                                              long long *__restrict__ out, long long out_stride,
                                                              float *__restrict__ logp, int *__restrict__ kept) {
    extern __shared__ float sf_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = blockIdx.x * (blockDim.x >> 6) + wave;
    if (row >= M) return;                                      // whole waves leave; the kernel has no barrier
    const float *l = logits + (long long)row * row_stride;
    const int chunk = (n_class + 63) / 64;
    const int c0 = min(lane * chunk, n_class), c1 = min(c0 + chunk, n_class);
    Chunk<REG> ch;
    ch.cnt = c1 - c0;
    ch.slab = sf_lds + (size_t)wave * chunk * 64 + lane;
    float mx = -INFINITY;
    if constexpr (REG) {
#pragma unroll
        for (int k = 0; k < SF_REG; ++k) {
            ch.z[k] = k < ch.cnt ? l[c0 + k] / temperature : -INFINITY;
            mx = fmaxf(mx, ch.z[k]);
        }
    } else {
        for (int k = 0; k < ch.cnt; ++k) {
            const float zk = l[c0 + k] / temperature;
            ch.slab[k * 64] = zk;
            mx = fmaxf(mx, zk);
        }
    }
    ch.mx = mx = wave_max(mx);
    if constexpr (REG) {
#pragma unroll
        for (int k = 0; k < SF_REG; ++k) ch.e[k] = expf(ch.z[k] - mx);
    }
    // Both cuts are the largest 32-bit key t for which a predicate that is true at t = 0 and monotone in t still holds, built
    // bit by bit from the top: 32 passes each, the same for every lane (the predicate is a wave-wide reduction).
    uint32_t cut = 0u;                                         // kept: order_key(z) >= cut
    if (top_k > 0 && top_k < n_class) {                        // v_k: the largest t with |{z >= t}| >= k
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t t = cut | (1u << bit);
            int n = 0;
            ch.each_z([&](float zk) { n += order_key(zk) >= t ? 1 : 0; });
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
            if (n >= top_k) cut = t;
        }
    }
    float excl;
    if (top_p < 1.f) {                                         // t*: the largest t >= v_k with mass(t) >= top_p * S_K
        float s = 0.f;
        ch.each([&](int, float zk, float ek) { s += order_key(zk) >= cut ? ek : 0.f; });
        const float target = top_p * lane_scan(s, lane, excl);
        const uint32_t floor_key = cut;
        cut = 0u;
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t t = cut | (1u << bit);
            const uint32_t both = t > floor_key ? t : floor_key;
            float m = 0.f;
            ch.each([&](int, float zk, float ek) { m += order_key(zk) >= both ? ek : 0.f; });
            const float mass = lane_scan(m, lane, excl);
            if (mass >= target && mass > 0.f) cut = t;         // mass > 0: the arg-max stays whatever top_p * S_K rounds to
        }
        if (cut < floor_key) cut = floor_key;
    }
    // the draw over the kept classes: the sums of sample_categorical_kernel with 0.f in place of a removed class
    float s = 0.f;
    int n = 0;
    ch.each([&](int, float zk, float ek) {
        const bool keep = order_key(zk) >= cut;
        s += keep ? ek : 0.f;
        n += keep ? 1 : 0;
    });
    const float total = lane_scan(s, lane, excl);
    const float thr = uniform_of(seed_lo, seed_hi, pos_lo, pos_hi, (uint32_t)row) * total;
    int found = -1, last = -1;
    float zfound = 0.f, zlast = 0.f, run = 0.f;
    ch.each([&](int k, float zk, float ek) {
        const bool keep = order_key(zk) >= cut;
        run += keep ? ek : 0.f;
        if (keep) { last = c0 + k; zlast = zk; }
        if (keep && found < 0 && excl + run > thr) { found = c0 + k; zfound = zk; }
    });
    // rounding left no kept class above thr: the last kept one (the highest lane that kept any)
    const unsigned long long any = __ballot(last >= 0);
    const int top_lane = any ? 63 - __clzll((long long)any) : 0;
    const int fallback = any ? __shfl(last, top_lane, 64) : n_class - 1;
    const float zfallback = __shfl(zlast, top_lane, 64);
    int winner;
    const int cls = lowest_hit(found, fallback, winner);
    const float zw = __shfl(zfound, winner, 64);
    const float zcls = __ballot(found >= 0) ? zw : zfallback;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0) {
        out[(long long)row * out_stride] = (long long)cls;
        if (logp) logp[row] = (zcls - mx) - logf(total);
        if (kept) kept[row] = n;
    }
}

__global__ __launch_bounds__(256) void sample_uniforms_kernel(float *__restrict__ u, int M, uint32_t seed_lo, uint32_t seed_hi,
                                                              uint32_t pos_lo, uint32_t pos_hi) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row < M) u[row] = uniform_of(seed_lo, seed_hi, pos_lo, pos_hi, (uint32_t)row);
}

// what both forms ask beyond vq2::check_conv_desc; a workspace below the form's own `need` is answered with its `short_ws`
int check_row(const vq2_conv_desc *d, int32_t row, int64_t x_image_stride, int64_t x_row_stride, int flags, const float *x,
              const float *wp, const float *residual, int32_t ldres, const float *y, const void *ws, size_t ws_bytes, size_t need,
              int short_ws, const char *who) {
    if (int e = vq2::check_conv_desc(d, who)) return e;
    VQ2_REQUIRE(d->same_size == 1 && d->pad_top == d->KH - 1,
                "%s: same_size and pad_top == KH - 1 required (the kernel must end at the output row)", who);
    VQ2_REQUIRE(row >= 0 && row < d->H, "%s: row %d outside the %d rows", who, row, d->H);
    VQ2_REQUIRE(x_image_stride >= 0 && x_row_stride >= 0 && x_image_stride % 4 == 0 && x_row_stride % 4 == 0,
                "%s: input strides must be non-negative multiples of 4", who);
    VQ2_REQUIRE((flags & ~(VQ2_RELU_IN | VQ2_RELU_OUT | VQ2_ROW_CAUSAL_TAPS)) == 0, "%s: unknown flag", who);
    VQ2_REQUIRE((int64_t)d->Co * d->KH * d->KW * d->Ci < ((int64_t)1 << 31), "%s: tensor exceeds 2^31 elements", who);
    VQ2_REQUIRE(x && wp && y && ws, "%s: null pointer", who);
    VQ2_REQUIRE(vq2::aligned16(x) && vq2::aligned16(wp) && vq2::aligned16(y) && vq2::aligned16(ws) &&
                    (!residual || vq2::aligned16(residual)), "%s: pointers must be 16-byte aligned", who);
    VQ2_REQUIRE(!residual || (ldres >= d->Co && ldres % 4 == 0), "%s: ldres must be >= Co and a multiple of 4", who);
    if (ws_bytes < need) return vq2::set_error(short_ws, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, need);
    return VQ2_OK;
}

// the second kernel of both forms: the slabs [splits][M][Co] of ws summed in ascending order, then the epilogue
int launch_reduce(const vq2_conv_desc *d, int flags, const float *ws, int splits, int M, const float *bias, const float *residual,
                  int32_t ldres, float *y, hipStream_t s) {
    const dim3 grid((unsigned)(((long)M * (d->Co / 4) + 255) / 256));      // a thread per 4 output channels of a pixel
    hipLaunchKernelGGL(convg_row_reduce_kernel, grid, dim3(256), 0, s, ws, splits, M, d->Co, d->Cor ? d->Cor : d->Co, bias,
                       residual, ldres, y, d->ldy, (flags & VQ2_RELU_OUT) != 0);
    return vq2::check_launch("convg_row_reduce_kernel");
}

}  // namespace

extern "C" size_t vq2_conv_fwd_row_workspace_bytes(const vq2_conv_desc *d, int flags) {
    if (!d || d->N <= 0 || d->W <= 0 || d->Co <= 0 || d->KH < 1 || d->KW < 1 || d->KH * d->KW > 32) return 0;
    const RowPlan p = row_plan(d, flags);
    return (size_t)p.splits * d->N * d->W * d->Co * sizeof(float);
}

extern "C" int vq2_conv_fwd_row(const vq2_conv_desc *d, int32_t row, int64_t x_image_stride, int64_t x_row_stride, int flags,
                                const float *x, const float *wp, const float *bias, const float *residual, int32_t ldres,
                                float *y, void *ws, size_t ws_bytes, vq2_stream_t stream) {
    if (int e = check_row(d, row, x_image_stride, x_row_stride, flags, x, wp, residual, ldres, y, ws, ws_bytes,
                          vq2_conv_fwd_row_workspace_bytes(d, flags), VQ2_ERR_WORKSPACE, "conv_fwd_row")) return e;
    const RowPlan pl = row_plan(d, flags);
    hipStream_t s = vq2::to_stream(stream);
    RowConv P{};
    P.x = x; P.w = wp; P.ws = static_cast<float *>(ws);
    P.x_image_stride = x_image_stride; P.x_row_stride = x_row_stride;
    P.W = d->W; P.Ci = d->Ci; P.Co = d->Co; P.KH = d->KH; P.KW = d->KW; P.pad_left = d->pad_left; P.ldx = d->ldx;
    P.row = row; P.M = d->N * d->W; P.K = d->KH * d->KW * d->Ci;
    P.relu_in = (flags & VQ2_RELU_IN) != 0;
    P.tap_mask = pl.mask; P.tps = pl.tps;
    const dim3 grid((P.M + RC_BM - 1) / RC_BM, (P.Co + RC_BN - 1) / RC_BN, pl.splits);
    hipLaunchKernelGGL(convg_row_partial_kernel, grid, dim3(256), 0, s, P);
    if (int e = vq2::check_launch("convg_row_partial_kernel")) return e;
    return launch_reduce(d, flags, P.ws, pl.splits, P.M, bias, residual, ldres, y, s);
}

extern "C" size_t vq2_conv_fwd_col_workspace_bytes(const vq2_conv_desc *d, int flags) {
    if (!d || d->N <= 0 || d->Ci <= 0 || d->Co <= 0 || d->KH < 1 || d->KW < 1 || d->KH * d->KW > 32) return 0;
    const ColPlan p = col_plan(d, flags);
    return (size_t)p.splits * d->N * d->Co * sizeof(float);
}

extern "C" int vq2_conv_fwd_col(const vq2_conv_desc *d, int32_t row, int32_t col, int64_t x_image_stride, int64_t x_row_stride,
                                int flags, const float *x, const float *wp, const float *bias, const float *residual,
                                int32_t ldres, float *y, void *ws, size_t ws_bytes, vq2_stream_t stream) {
    if (int e = check_row(d, row, x_image_stride, x_row_stride, flags, x, wp, residual, ldres, y, ws, ws_bytes,
                          vq2_conv_fwd_col_workspace_bytes(d, flags), VQ2_ERR_INVALID, "conv_fwd_col")) return e;
    VQ2_REQUIRE(col >= 0 && col < d->W, "conv_fwd_col: col %d outside the %d columns", col, d->W);
    const ColPlan pl = col_plan(d, flags);
    const int chunks = (d->N + 16 * pl.mt - 1) / (16 * pl.mt);
    VQ2_REQUIRE(chunks <= 65535, "conv_fwd_col: %d images exceed the grid", d->N);
    hipStream_t s = vq2::to_stream(stream);
    ColConv P{};
    P.x = x; P.w = wp; P.ws = static_cast<float *>(ws);
    P.x_image_stride = x_image_stride; P.x_row_stride = x_row_stride;
    P.N = d->N; P.W = d->W; P.Ci = d->Ci; P.Co = d->Co; P.KH = d->KH; P.KW = d->KW; P.pad_left = d->pad_left; P.ldx = d->ldx;
    P.row = row; P.col = col; P.K = d->KH * d->KW * d->Ci;
    P.relu_in = (flags & VQ2_RELU_IN) != 0;
    P.cb = pl.cb; P.steps = pl.steps; P.sps = pl.sps;
    for (int t = 0; t < 32; ++t) P.taps[t] = pl.taps[t];
    const dim3 grid((P.Co + CC_BN - 1) / CC_BN, pl.splits, chunks);
    if (pl.mt == 1)
        hipLaunchKernelGGL(convg_col_partial_kernel<1>, grid, dim3(256), 0, s, P);
    else
        hipLaunchKernelGGL(convg_col_partial_kernel<4>, grid, dim3(256), 0, s, P);
    if (int e = vq2::check_launch("convg_col_partial_kernel")) return e;
    return launch_reduce(d, flags, P.ws, pl.splits, P.N, bias, residual, ldres, y, s);
}

extern "C" int vq2_sample_categorical(const float *logits, int64_t row_stride, int32_t M, int32_t n_class, float temperature,
                                      uint64_t seed, uint64_t position, int64_t *out, int64_t out_stride, vq2_stream_t stream) {
    VQ2_REQUIRE(logits && out, "sample_categorical: null pointer");
    VQ2_REQUIRE(M >= 1 && row_stride >= n_class && out_stride >= 1, "sample_categorical: M >= 1, row_stride >= n_class and out_stride >= 1 required");
    VQ2_REQUIRE(temperature > 0.f, "sample_categorical: temperature must be positive");
    VQ2_REQUIRE(n_class >= 1 && n_class <= 16384, "sample_categorical: n_class must be in 1..16384 (got %d)", n_class);
    hipLaunchKernelGGL(sample_categorical_kernel, dim3((M + 3) / 4), dim3(256), 0, vq2::to_stream(stream), logits,
                       (long long)row_stride, M, n_class, temperature, (uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32),
                       (uint32_t)(position & 0xFFFFFFFFu), (uint32_t)(position >> 32), reinterpret_cast<long long *>(out),
                       (long long)out_stride);
    return vq2::check_launch("sample_categorical_kernel");
}

extern "C" int vq2_sample_filtered(const float *logits, int64_t row_stride, int32_t M, int32_t n_class, float temperature,
                                   int32_t top_k, float top_p, uint64_t seed, uint64_t position, int64_t *out, int64_t out_stride,
                                   float *logp, int32_t *kept, vq2_stream_t stream) {
    VQ2_REQUIRE(logits && out, "sample_filtered: null pointer");
    VQ2_REQUIRE(M >= 1 && row_stride >= n_class && out_stride >= 1, "sample_filtered: M >= 1, row_stride >= n_class and out_stride >= 1 required");
    VQ2_REQUIRE(temperature > 0.f, "sample_filtered: temperature must be positive");
    VQ2_REQUIRE(n_class >= 1 && n_class <= 16384, "sample_filtered: n_class must be in 1..16384 (got %d)", n_class);
    VQ2_REQUIRE(top_k >= 0 && top_k <= n_class, "sample_filtered: top_k must be 0 (off) or in 1..n_class (got %d)", top_k);
    VQ2_REQUIRE(top_p > 0.f && top_p <= 1.f, "sample_filtered: top_p must be in (0, 1]");      // false for NaN
    hipStream_t s = vq2::to_stream(stream);
    const uint32_t seed_lo = (uint32_t)(seed & 0xFFFFFFFFu), seed_hi = (uint32_t)(seed >> 32);
    const uint32_t pos_lo = (uint32_t)(position & 0xFFFFFFFFu), pos_hi = (uint32_t)(position >> 32);
    const int chunk = (n_class + 63) / 64;
    if (chunk <= SF_REG) {
        hipLaunchKernelGGL(sample_filtered_kernel<true>, dim3((M + 3) / 4), dim3(256), 0, s, logits, (long long)row_stride, M, n_class,
                           temperature, top_k, top_p, seed_lo, seed_hi, pos_lo, pos_hi, reinterpret_cast<long long *>(out),
                           (long long)out_stride, logp, kept);
        return vq2::check_launch("sample_filtered_kernel<registers>");
    }
    // one LDS slab of chunk * 64 floats per wave: as many waves per workgroup, up to 4, as 64 KB hold
    const int slab = chunk * 64;
    const int waves = SF_LDS_FLOATS / slab >= 4 ? 4 : SF_LDS_FLOATS / slab;
    hipLaunchKernelGGL(sample_filtered_kernel<false>, dim3((M + waves - 1) / waves), dim3(64 * waves),
                       (size_t)waves * slab * sizeof(float), s, logits, (long long)row_stride, M, n_class, temperature, top_k, top_p,
                       seed_lo, seed_hi, pos_lo, pos_hi, reinterpret_cast<long long *>(out), (long long)out_stride, logp, kept);
    return vq2::check_launch("sample_filtered_kernel<lds>");
}

extern "C" int vq2_sample_uniforms(float *u, int32_t M, uint64_t seed, uint64_t position, vq2_stream_t stream) {
    VQ2_REQUIRE(u && M >= 1, "sample_uniforms: null pointer or M < 1");
    hipLaunchKernelGGL(sample_uniforms_kernel, dim3((M + 255) / 256), dim3(256), 0, vq2::to_stream(stream), u, M,
                       (uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32), (uint32_t)(position & 0xFFFFFFFFu),
                       (uint32_t)(position >> 32));
    return vq2::check_launch("sample_uniforms_kernel");
}
