// Launch parameters, kernel plan, host helpers and the device-side GEMM skeleton shared by the conv kernels of libvq2
// (vq2_conv.hip, vq2_conv_bf16.hip, vq2_wino.hip, vq2_wgrad.hip, vq2_wgrad_bf16.hip); the epilogue contract is vq2_conv_epilogue.h, included below.
#pragma once
#include "vq2_common.h"

namespace vq2 {

struct ConvGemmParams {
    const float *x;   // [N,H,W,ldx]
    const float *w;   // [phases][Co][K]   (K = KH*KW*Ci, ci fastest)
    const float *bias;  // [Co] or null
    const float *mask;  // shape of y (pixel stride ldm) or null: y *= (mask > 0)
    const float *res;   // shape of y (pixel stride ldr) or null: y += res
    float *y;           // [N,Hy,Wy,ldy]
    int N, H, W, Ci, ldx;
    int Ho, Wo, Co, ldy;  // virtual output grid (rows of the GEMM) and channels
    int KH, KW, stride, pad_h, pad_w;
    int K, M;             // K = KH*KW*Ci, M = N*Ho*Wo
    int phases;           // 1, or 4 for the sub-pixel transposed conv
    int Hy, Wy;           // real output image size
    int ldm, ldr;
    int relu_in, relu_out;
    int mask_after;       // apply the mask to (acc + residual) instead of to acc alone
    int nbias;            // bias has nbias entries (real output channels)
    int c4_tpw;           // conv_k4s2_c4_kernel: tiles per workgroup
    int ci_real;          // real input channels (<= Ci; the rest are zero padding), 0 = Ci
    int allow_bf16;       // the caller set VQ2_ALLOW_BF16 on a same_size layer: P.w is the bf16 panel if conv_bf16_shape(Ci)
    double flops, bytes;  // algorithmic work of this launch (for the profiler only)
};

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
constexpr int OOB = 0x7FFFFFF0;  // >= num_records of every descriptor: loads return 0, stores are dropped
constexpr unsigned RSRC_FLAGS = 0x00020000;

// How many ELEMENTS a tensor may have for a kernel's 32-bit byte offsets, one constant per out-of-range sentinel (the other
// three, sp::REACH / c4::REACH / ctm::REACH, sit next to their sentinels in vq2_conv.hip):
//   FAST_REACH     kernels that send lanes out of range with OOB: every tensor below 2 GiB
//   PENALTY_REACH  kernels that send lanes out of range by ADDING 2^31 to a valid offset (conv_gemm_fast_kernel's uniform
//                  chunks, the Winograd kernels): as an unsigned buffer offset anything >= 2^31 - (tensor bytes) is out of
//                  range, so every tensor stays below 1 GiB
constexpr long FAST_REACH = (1L << 31) / 4;
constexpr long PENALTY_REACH = (1L << 30) / 4;

__device__ __forceinline__ float4 as_f4(u32x4 v) {
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
__device__ __forceinline__ float f4_at(const float4 &v, int c) { return c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w; }

// ---------------------------------------------------------------------------------------------- descriptor helpers
static inline int real_ci(const vq2_conv_desc *d) { return d->Cir ? d->Cir : d->Ci; }
static inline int real_co(const vq2_conv_desc *d) { return d->Cor ? d->Cor : d->Co; }

struct ConvHW { int h, w; };
static inline ConvHW out_hw(const vq2_conv_desc *d) {
    if (d->transposed) return {2 * d->H, 2 * d->W};
    if (d->same_size) return {d->H, d->W};
    return {(d->H + 2 * d->pad_top - d->KH) / d->stride + 1, (d->W + 2 * d->pad_left - d->KW) / d->stride + 1};
}

// The contract of vq2_conv_desc (include/vq2.h), checked by every conv entry point before anything is planned: the one copy
// of it.  `who` names the entry point in the null-pointer message.  DESC_PLAN_ONLY: the two entry points that plan a weight
// gradient without launching it (workspace size, reduction job) leave out the 2^31-element check, the one check that a
// recorded plan of tests/golden/wgrad_plans.json fails; the launch itself is checked in full.
enum { DESC_PLAN_ONLY = 1 };
static inline int check_conv_desc(const vq2_conv_desc *d, const char *who, int how = 0) {
    VQ2_REQUIRE(d != nullptr, "%s: the conv descriptor is null", who);
    if (int e = check_forms()) return e;
    VQ2_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->Ci > 0 && d->Co > 0, "conv desc: non-positive dims");
    VQ2_REQUIRE(d->Ci % 4 == 0 && d->Co % 4 == 0, "conv desc: Ci=%d, Co=%d must be multiples of 4", d->Ci, d->Co);
    VQ2_REQUIRE(d->ldx >= d->Ci && d->ldx % 4 == 0, "conv desc: ldx=%d must be >= Ci and a multiple of 4", d->ldx);
    VQ2_REQUIRE(d->ldy >= d->Co && d->ldy % 4 == 0, "conv desc: ldy=%d must be >= Co and a multiple of 4", d->ldy);
    VQ2_REQUIRE(d->Cir >= 0 && d->Cir <= d->Ci && d->Cor >= 0 && d->Cor <= d->Co, "conv desc: Cir/Cor out of range");
    VQ2_REQUIRE((d->same_size == 0 || d->same_size == 1) && (d->transposed == 0 || d->transposed == 1),
                "conv desc: same_size=%d and transposed=%d must be 0 or 1", d->same_size, d->transposed);
    VQ2_REQUIRE(d->KH >= 1 && d->KH <= 7 && d->KW >= 1 && d->KW <= 7, "conv desc: KH=%d, KW=%d must lie in 1..7", d->KH, d->KW);
    VQ2_REQUIRE(d->pad_top >= 0 && d->pad_top < d->KH && d->pad_left >= 0 && d->pad_left < d->KW,
                "conv desc: 0 <= pad_top < KH and 0 <= pad_left < KW required (got %d, %d)", d->pad_top, d->pad_left);
    if (d->same_size) {
        VQ2_REQUIRE(d->stride == 1 && !d->transposed, "conv desc: same_size needs stride 1 and no transposition");
        if (d->KH * d->KW > 32) return set_error(VQ2_ERR_UNSUPPORTED, "conv desc: %d x %d has more than 32 taps", d->KH, d->KW);
    } else {
        VQ2_REQUIRE(d->KW == d->KH && d->pad_left == d->pad_top,
                    "conv desc: a square kernel and pad_top == pad_left required without same_size");
        if (d->transposed) {
            VQ2_REQUIRE(d->KH == 4 && d->stride == 2 && d->pad_top == 1,
                        "conv-transpose supports k4 s2 p1 only (vqvae.py:150-160,191-193)");
        } else {
            VQ2_REQUIRE(d->stride == 1 || d->stride == 2, "conv: stride 1 or 2");
            VQ2_REQUIRE(d->H + 2 * d->pad_top >= d->KH && d->W + 2 * d->pad_left >= d->KW, "conv: kernel larger than padded input");
            if (d->stride == 2) VQ2_REQUIRE(d->KH == 4 && d->pad_top == 1 && d->H % 2 == 0 && d->W % 2 == 0,
                                            "stride-2 conv supports k4 p1 on even sizes (vqvae.py:105,107,114)");
        }
    }
    const ConvHW o = out_hw(d);
    const int64_t lim = (int64_t)1 << 31;
    VQ2_REQUIRE((how & DESC_PLAN_ONLY) || ((int64_t)d->N * d->H * d->W * d->ldx < lim && (int64_t)d->N * o.h * o.w * d->ldy < lim),
                "conv: tensor exceeds 2^31 elements (int32 indexing)");
    return VQ2_OK;
}

// Algorithmic work of a layer, the same for its forward, data-gradient and weight-gradient launches (for the profiler only):
// real channels, every tap once; the input-sized and the output-sized tensor cross memory once each, plus `more_in` /
// `more_out` further tensors of those sizes (residual, mask), plus the weights.
struct ConvWork { double flops, bytes; };
static inline ConvWork conv_work(const vq2_conv_desc *d, int more_in, int more_out) {
    const double cir = real_ci(d), cor = real_co(d);
    const ConvHW o = out_hw(d);
    const double pix_in = (double)d->N * d->H * d->W, pix_out = (double)d->N * o.h * o.w;
    const double macs = d->transposed ? pix_in * 16.0 * cir * cor : pix_out * d->KH * d->KW * cir * cor;
    return {2.0 * macs, 4.0 * (pix_in * cir * (1.0 + more_in) + pix_out * cor * (1.0 + more_out) + cir * cor * d->KH * d->KW)};
}

// ---------------------------------------------------------------------------------------------- extents of a launch
// Element counts of the tensors of a forward / data-gradient launch, computed once; every "does this tensor fit the 32-bit
// offsets of that kernel" test compares them with the kernel's reach.
struct ConvExtents {
    long x, y, mask, res, w;   // mask / res: output pixels times ldm / ldr, whether or not the pointer is set
    long aux() const { return mask > res ? mask : res; }
    bool acts_fit(long reach) const { return x < reach && y < reach && aux() < reach; }
    bool all_fit(long reach) const { return acts_fit(reach) && w < reach; }
};
static inline ConvExtents conv_extents(const ConvGemmParams &P) {
    const long ypix = (long)P.N * P.Hy * P.Wy;
    return {(long)P.N * P.H * P.W * P.ldx, ypix * P.ldy, ypix * P.ldm, ypix * P.ldr, (long)P.Co * P.K * P.phases};
}

// ---------------------------------------------------------------------------------------------- the plan of a launch
// plan_conv() (vq2_conv.hip) chooses the kernel of a forward / data-gradient launch from the shape and strides alone;
// launch_conv() launches what the plan says.
enum ConvFamily {
    CONV_GEMM_GEN, CONV_GEMM_FAST, CONV_K4S2_C4, CONV_1X1_K64, CONV_SUBPIXEL, CONV_WINO3, CONV_WINO_K4S2, CONV_WINO_SUBPIXEL,
    CONV_GEMM_BF16,
    CONV_FAMILIES
};

struct ConvPlan {
    int family;        // ConvFamily
    int tile;          // index into the family's tile table (conv_tiles)
    // instantiation flags (each read by its own family only)
    bool occ4;         // fast GEMM: four workgroups per CU (a property of the 128x128x16 tile)
    bool uni;          // fast GEMM: every chunk lies in one tap (scalar k tracking)
    bool tap_inner;    // fast GEMM: uniform chunks with the taps innermost
    bool rows64;       // Winograd: rows of whole 64-pixel segments (else 32-pixel segments)
    bool wide;         // Winograd: 128-channel tiles (else 64)
    bool c4;           // conv_k4s2_c4: the fourth input channel is real
    int tpw;           // conv_k4s2_c4: tiles per workgroup
    int nb;            // conv1x1_k64: Co / 32 column blocks
};

// A tile of a family: what the label prints of it and the launcher of its instantiations.
//   GEMM families: dim = BM x BN x BK;   Winograd families: dim = image rows x pixels per row, NT;   conv1x1_k64: dim[0] = NB
struct ConvTile {
    int dim[3];
    int (*launch)(const ConvPlan &, const ConvGemmParams &, const char *name, hipStream_t);
};
struct ConvTiles { const ConvTile *tile; int n; };
ConvTiles conv_tiles(int family);                 // vq2_conv.hip; the Winograd families from wino_tiles
ConvTiles wino_tiles(int family);                 // vq2_wino.hip
ConvTiles bf16_tiles();                           // vq2_conv_bf16.hip

// The eligibility rule of the bf16-operand kernel (vq2_conv_bf16.hip), the one copy of it: a same_size layer whose
// depth-side channel count (Ci for the forward, Co for the data gradient) is a multiple of 16, so that a 16-deep MFMA step
// stays inside one tap.  vq2_conv_bf16_eligible() exports it; the host packs the bf16 panel exactly when it holds.
static inline bool conv_bf16_shape(int same_size, int depth_channels) { return same_size == 1 && depth_channels % 16 == 0; }
int pack_weight_bf16(const vq2_conv_desc *d, int flip, const float *w, float *packed, hipStream_t s);   // vq2_conv_bf16.hip

// The eligibility rule of the bf16-operand WEIGHT GRADIENT (vq2_wgrad_bf16.hip), the one copy of it: a same_size layer with
// both channel counts multiples of 16 (both operands are staged in 16-byte fp32 runs of whole channel groups, and a K tile
// column run never straddles two taps).  vq2_conv_wgrad_bf16_eligible() exports it.
static inline bool conv_wgrad_bf16_shape(const vq2_conv_desc *d) { return d->same_size == 1 && d->Ci % 16 == 0 && d->Co % 16 == 0; }

// The plan of a bf16-operand weight gradient: the GEMM [O x M] * [M x K] in plain roles (O = Co, K = taps * Ci, M = pixels),
// its own tile and split.  plan_wgrad_bf16 / launch_wgrad_bf16: vq2_wgrad_bf16.hip; vq2_wgrad.hip turns the plan into the
// slab layout [S][O][K] + bias partials [S][O] that the unchanged reduction kernels read.
struct WgradBf16Plan { int tile, bmo, bnk, O, I, K, M, S, rows_per_split; };
WgradBf16Plan plan_wgrad_bf16(const vq2_conv_desc *d);
int launch_wgrad_bf16(const WgradBf16Plan &p, const vq2_conv_desc *d, int relu_in, const float *x, const float *dy, float *ws,
                      float *bias_ws, hipStream_t s);

namespace wino {
constexpr int BK = 8;   // input channels per staged block of the Winograd kernels (vq2_wino.hip)
}

ConvPlan plan_conv(const ConvGemmParams &P);
int launch_conv(const ConvPlan &plan, const ConvGemmParams &P, hipStream_t s);

// ---------------------------------------------------------------------------------------------- device: GEMM skeleton
template <int A, int B>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[A][B]) {
#pragma unroll
    for (int i = 0; i < A; ++i)
#pragma unroll
        for (int j = 0; j < B; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}
template <int A>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[A]) {
#pragma unroll
    for (int i = 0; i < A; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
}

// The pixels a staging thread of the pointer GEMM kernels (conv_gemm_kernel, conv_gemm_bf16_kernel) gathers for: GEMM rows
// m_first + m_step * j of the Ho x Wo output grid, as the input pixel of tap (0, 0) and its coordinates.
template <int A_LD>
struct GatherRows {
    int pix[A_LD], h[A_LD], w[A_LD];
    __device__ __forceinline__ GatherRows(const ConvGemmParams &P, int m_first, int m_step, int Ho, int Wo, int stride, int pad_h,
                                          int pad_w) {
        const int HoWo = Ho * Wo;
#pragma unroll
        for (int j = 0; j < A_LD; ++j) {
            const int m = m_first + m_step * j;
            if (m < P.M) {
                const int n = m / HoWo;
                const int r = m - n * HoWo;
                const int ho = r / Wo;
                const int wo = r - ho * Wo;
                h[j] = ho * stride - pad_h;
                w[j] = wo * stride - pad_w;
                pix[j] = (n * P.H + h[j]) * P.W + w[j];
            } else {
                h[j] = -(1 << 24); w[j] = 0; pix[j] = 0;  // every bounds test fails
            }
        }
    }
    // is tap (kh, kw) of row j inside the image, and where (in elements of x, 64-bit)
    __device__ __forceinline__ bool inside(const ConvGemmParams &P, int j, int kh, int kw) const {
        return (unsigned)(h[j] + kh) < (unsigned)P.H && (unsigned)(w[j] + kw) < (unsigned)P.W;
    }
    __device__ __forceinline__ size_t at(const ConvGemmParams &P, int j, int kh, int kw, int ci) const {
        return (size_t)(pix[j] + kh * P.W + kw) * P.ldx + ci;
    }
};

// k -> (kh, kw, ci) of a staging thread's run of consecutive k (4 floats, or 8 in the bf16 kernel), advanced by one chunk
struct KWalker {
    int k, ci, kh, kw;
    __device__ __forceinline__ KWalker(const ConvGemmParams &P, int k0) : k(k0) {
        const int tap = k0 / P.Ci;
        ci = k0 - tap * P.Ci;
        kh = tap / P.KW;
        kw = tap - kh * P.KW;
    }
    __device__ __forceinline__ void advance(const ConvGemmParams &P, int bk) {
        k += bk;
        ci += bk;
        while (ci >= P.Ci) {
            ci -= P.Ci;
            if (++kw == P.KW) { kw = 0; ++kh; }
        }
    }
};

// One staged chunk of the fp32 GEMM kernels: a / b = this lane's fragment rows in the LDS tiles (rows LDK floats apart, 32
// rows per MFMA tile).  The fragment registers are double-buffered: the ds_reads of k-group g+1 are issued before the MFMAs
// of group g, so LDS latency never sits between two MFMA groups; the MT * NT independent accumulators take turns, so
// consecutive MFMAs never depend on each other.  PRIO raises the wave's priority around the MFMAs; after_group0() runs
// behind the MFMAs of k-group 0.
template <int MT, int NT, int BK, int LDK, bool PRIO, class F>
__device__ __forceinline__ void mfma_chunk_f32(f32x16 (&acc)[MT][NT], const float *a, const float *b, F after_group0) {
    float4 fa[2][MT], fb[2][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i) fa[0][i] = *reinterpret_cast<const float4 *>(a + i * 32 * LDK);
#pragma unroll
    for (int j = 0; j < NT; ++j) fb[0][j] = *reinterpret_cast<const float4 *>(b + j * 32 * LDK);
#pragma unroll
    for (int k8 = 0; k8 < BK / 8; ++k8) {
        const int cur = k8 & 1, nxt = cur ^ 1;
        if (k8 + 1 < BK / 8) {
#pragma unroll
            for (int i = 0; i < MT; ++i) fa[nxt][i] = *reinterpret_cast<const float4 *>(a + i * 32 * LDK + (k8 + 1) * 8);
#pragma unroll
            for (int j = 0; j < NT; ++j) fb[nxt][j] = *reinterpret_cast<const float4 *>(b + j * 32 * LDK + (k8 + 1) * 8);
        }
        if (PRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int c = 0; c < 4; ++c)   // x, y, z, w
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(f4_at(fa[cur][i], c), f4_at(fb[cur][j], c), acc[i][j], 0, 0, 0);
        if (PRIO) __builtin_amdgcn_s_setprio(0);
        if (k8 == 0) after_group0();
    }
}

}  // namespace vq2

#include "vq2_conv_epilogue.h"
