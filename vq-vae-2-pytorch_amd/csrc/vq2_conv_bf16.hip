// bf16-operand implicit-GEMM conv forward / data gradient for gfx950 (MI355X): the stage-2 layers (same_size == 1).
//
//   y = sum_k bf16(a_k) * bf16(w_k), accumulated in fp32 by v_mfma_f32_32x32x16_bf16, then the one fp32 conv
//   epilogue (vq2_conv_epilogue.h: bias, mask, residual, ReLU-out).  bf16() is round-to-nearest-even of the fp32 value.
//
//   GEMM rows  m = (n, h, w) output pixels        GEMM cols  co        GEMM depth  k = (kh, kw, ci), ci fastest
//
// Every tensor in memory stays fp32 NHWC.  The activation is read as 16-byte fp32 runs, rounded while it is staged
// (the compiler's fp32 -> bf16 conversion: v_cvt_pk_bf16_f32) and written to LDS as bf16.  The weight panel is bf16
// already: pack_bf16_kernel writes it as [Co][K] rows with K = taps * Ci, so that the 8 consecutive k a lane feeds to one
// MFMA (k = 8 * (lane >> 5) + j of a 16-deep step) are one 16-byte run, in global memory and in LDS alike.
// The depth-side channel count is a multiple of 16: a 16-deep MFMA step, and the 8-element run of a staging thread, never
// straddle two taps, so one bounds test covers a run.  Pixels outside the image stage as 0.
//
// LDS rows are BK + 8 bf16 = 80 bytes: the 16-byte slot of row r is 5 r (+ lane >> 5) mod 16, a permutation over 16
// consecutive rows -- the ds_read_b128 fragment reads are conflict-free (the byte image of the fp32 tiles' BK = 16 rows).
// The 16-byte staging STORES are not: four threads fill the four slots of a row, so within 16 lanes row r + 3 (slots 15, 0,
// 1, 2) meets row r (slots 0, 1, 2) -- a two-way conflict on three of sixteen slots, once per chunk; not swizzled away.
// No atomics, no split-K: one fixed summation order per output element, which depends on neither the launch's batch size
// nor its other images.
#include "vq2_conv.h"

namespace vq2 {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x8 __attribute__((ext_vector_type(8)));

namespace b16 {
constexpr int BK = 32;          // depth of a staged chunk: two MFMA steps
constexpr int LDK = BK + 8;     // bf16 per LDS row (80 bytes)
}  // namespace b16

__device__ __forceinline__ bf16x8 round8(float4 lo, float4 hi, bool relu) {
    if (relu) { lo = relu4(lo); hi = relu4(hi); }
    const f32x8 v = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    return __builtin_convertvector(v, bf16x8);
}

// 4 waves as 2 x 2, each MT x NT 32x32 accumulators: BM = 64 MT pixels x BN = 64 NT channels.
template <int MT, int NT>
__global__ __launch_bounds__(256, 2) void conv_gemm_bf16_kernel(const ConvGemmParams P) {
    using namespace b16;
    constexpr int BM = 64 * MT, BN = 64 * NT;
    constexpr int RPP = 256 / (BK / 8);   // 64 rows staged per pass: 4 threads of 8 k each per row
    constexpr int A_LD = BM / RPP, B_LD = BN / RPP;
    extern __shared__ __attribute__((aligned(16))) __bf16 smem_h[];
    __bf16 *As = smem_h;                   // [2][BM][LDK]
    __bf16 *Bs = smem_h + 2 * BM * LDK;    // [2][BN][LDK]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int ntiles = (P.Co + BN - 1) / BN;
    const int vid = xcd_remap(blockIdx.x, gridDim.x);
    const int n0 = (vid % ntiles) * BN;
    const int m0 = (vid / ntiles) * BM;
    const __bf16 *__restrict__ wp = reinterpret_cast<const __bf16 *>(P.w);
    const float *__restrict__ xp = P.x;

    // ---- per-thread staging coordinates (fixed over the K loop)
    const int lrow = tid >> 2;          // 0..63
    const int lk = (tid & 3) * 8;       // first of this thread's 8 k inside a chunk
    const GatherRows<A_LD> rows(P, m0 + lrow, RPP, P.H, P.W, 1, P.pad_h, P.pad_w);   // same_size: the output grid is the input's
    KWalker kk(P, lk);

    float4 ra[A_LD][2];
    uint4 rb[B_LD];
    auto load_chunk = [&]() {
        const bool kv = kk.k < P.K;
#pragma unroll
        for (int j = 0; j < A_LD; ++j) {
            ra[j][0] = ra[j][1] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (kv && rows.inside(P, j, kk.kh, kk.kw)) {
                const float4 *src = reinterpret_cast<const float4 *>(xp + rows.at(P, j, kk.kh, kk.kw, kk.ci));
                ra[j][0] = src[0];
                ra[j][1] = src[1];
            }
        }
#pragma unroll
        for (int j = 0; j < B_LD; ++j) {
            const int co = n0 + lrow + RPP * j;
            rb[j] = make_uint4(0u, 0u, 0u, 0u);
            if (kv && co < P.Co) rb[j] = *reinterpret_cast<const uint4 *>(wp + (size_t)co * P.K + kk.k);
        }
    };
    auto store_chunk = [&](int buf) {
        __bf16 *a = As + buf * BM * LDK + lrow * LDK + lk;
        __bf16 *b = Bs + buf * BN * LDK + lrow * LDK + lk;
#pragma unroll
        for (int j = 0; j < A_LD; ++j)
            *reinterpret_cast<bf16x8 *>(a + RPP * j * LDK) = round8(ra[j][0], ra[j][1], P.relu_in != 0);
#pragma unroll
        for (int j = 0; j < B_LD; ++j) *reinterpret_cast<uint4 *>(b + RPP * j * LDK) = rb[j];
    };

    f32x16 acc[MT][NT];
    zero_acc(acc);

    // operand maps of v_mfma_f32_32x32x16_bf16: lane l holds A[row l & 31][k = 8 (l >> 5) + j] and B[k][col l & 31], j < 8
    const int frag_row = lane & 31, frag_k = 8 * (lane >> 5);
    auto compute = [&](int buf) {
        const __bf16 *a = As + buf * BM * LDK + (wm * MT * 32 + frag_row) * LDK + frag_k;
        const __bf16 *b = Bs + buf * BN * LDK + (wn * NT * 32 + frag_row) * LDK + frag_k;
        bf16x8 fa[BK / 16][MT], fb[BK / 16][NT];
#pragma unroll
        for (int s = 0; s < BK / 16; ++s) {
#pragma unroll
            for (int i = 0; i < MT; ++i) fa[s][i] = *reinterpret_cast<const bf16x8 *>(a + i * 32 * LDK + s * 16);
#pragma unroll
            for (int j = 0; j < NT; ++j) fb[s][j] = *reinterpret_cast<const bf16x8 *>(b + j * 32 * LDK + s * 16);
        }
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int s = 0; s < BK / 16; ++s)
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[s][i], fb[s][j], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
    };

    const int nchunks = (P.K + BK - 1) / BK;
    load_chunk();
    store_chunk(0);
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const int buf = c & 1;
        if (c + 1 < nchunks) {
            kk.advance(P, BK);
            load_chunk();   // global loads in flight while the matrix pipe works on chunk c
        }
        compute(buf);
        if (c + 1 < nchunks) store_chunk(buf ^ 1);
        __syncthreads();
    }

    // ---- epilogue: the pointer form of the one conv epilogue (vq2_conv_epilogue.h), one output pixel per GEMM row
    conv_epilogue_pointers<MT, NT>(P, acc, m0, n0, wm, wn, lane, 1, 0, 0);
}

template <int MT, int NT>
static int launch_conv_gemm_bf16(const ConvPlan &, const ConvGemmParams &P, const char *name, hipStream_t s) {
    constexpr int BM = 64 * MT, BN = 64 * NT;
    const size_t lds = (size_t)2 * (BM + BN) * b16::LDK * sizeof(__bf16);
    auto kern = conv_gemm_bf16_kernel<MT, NT>;
    allow_big_lds(kern, lds);
    const unsigned nwg = (unsigned)(((P.M + BM - 1) / BM) * ((P.Co + BN - 1) / BN));
    ProfScope prof(name, P.flops, P.bytes, s, true);
    hipLaunchKernelGGL(kern, dim3(nwg), dim3(256), lds, s, P);
    return check_launch("conv_gemm_bf16_kernel");
}

static const ConvTile BF16_TILES[] = {
    {{128, 128, b16::BK}, launch_conv_gemm_bf16<2, 2>},
    {{128, 64, b16::BK}, launch_conv_gemm_bf16<2, 1>},
};
ConvTiles bf16_tiles() { return {BF16_TILES, sizeof(BF16_TILES) / sizeof(ConvTile)}; }

// ---------------------------------------------------------------------------------------------- the bf16 weight panel
// [rows][taps][depth] bf16, rows = the GEMM's columns: forward (flip 0) rows = co, depth = ci, tap (kh, kw); data gradient
// (flip 1) rows = ci, depth = co, tap flipped.  w is the reference [Cor][Cir][KH][KW]; padded channels pack as 0.
__global__ __launch_bounds__(256) void pack_bf16_kernel(const float *__restrict__ w, __bf16 *__restrict__ p, int Or, int Ir,
                                                        int Op, int Ip, int KH, int KW, int flip, int total) {
    const int taps = KH * KW;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < total; t += gridDim.x * 256) {
        int o, i, kh, kw;
        if (!flip) {
            i = t % Ip; const int tap = (t / Ip) % taps; o = t / (Ip * taps);
            kh = tap / KW; kw = tap % KW;
        } else {
            o = t % Op; const int tapf = (t / Op) % taps; i = t / (Op * taps);
            kh = KH - 1 - tapf / KW; kw = KW - 1 - tapf % KW;
        }
        const float v = (o < Or && i < Ir) ? w[((o * Ir + i) * KH + kh) * KW + kw] : 0.f;
        p[t] = (__bf16)v;
    }
}

int pack_weight_bf16(const vq2_conv_desc *d, int flip, const float *w, float *packed, hipStream_t s) {
    const int total = d->Co * d->Ci * d->KH * d->KW;
    const int blocks = (total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024;
    hipLaunchKernelGGL(pack_bf16_kernel, dim3(blocks), dim3(256), 0, s, w, reinterpret_cast<__bf16 *>(packed), real_co(d),
                       real_ci(d), d->Co, d->Ci, d->KH, d->KW, flip, total);
    return check_launch("pack_bf16_kernel");
}

}  // namespace vq2
