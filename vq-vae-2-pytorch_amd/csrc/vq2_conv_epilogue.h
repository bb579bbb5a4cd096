// The epilogue of every forward / data-gradient conv kernel of libvq2, stated once (included by vq2_conv.h).
//
//   v = acc + bias[co]                       (co < nbias)
//   if mask and not mask_after:  v = mask > 0 ? v : 0
//   if res:                      v += res
//   if mask and mask_after:      v = mask > 0 ? v : 0
//   v = relu_floor(v, relu_out ? 0 : 0x80000000)
//   store; out-of-range lanes are dropped
//
// conv_epilogue_value() is that rule on one element, in fp32 and in that order (the build keeps -ffp-contract=off: nothing is
// reassociated).  ConvEpilogue carries what the rule needs from ConvGemmParams for the kernels that address y / mask / res
// through buffer descriptors, and its store8() is their common 8-element step; conv_epilogue_pointers() is the 64-bit
// pointer form of the two general GEMM kernels.  vq2_conv.hip, vq2_conv_bf16.hip and vq2_wino.hip apply a mask or a residual
// nowhere else.  (convT_small_mfma_kernel, vq2_rbwino.hip, vq2_resblock.hip and vq2_sample.hip have other contracts.)
#pragma once

namespace vq2 {

// (mk / rs by reference: a caller without a mask / residual leaves them unset, and they are read only under their flags)
__device__ __forceinline__ float conv_epilogue_value(float acc, float bias, const float &mk, const float &rs, bool mask_first,
                                                     bool has_res, bool mask_last, int relu_bits) {
    float v = acc + bias;
    if (mask_first) v = (mk > 0.f) ? v : 0.f;
    if (has_res) v += rs;
    if (mask_last) v = (mk > 0.f) ? v : 0.f;
    return relu_floor(v, relu_bits);
}

__device__ __forceinline__ float conv_bias_value(const ConvGemmParams &P, int co) {
    return (P.bias && co < P.nbias) ? P.bias[co] : 0.f;
}

constexpr int ALL_VALID = 0;   // store8's sentinel of a caller that passes pixels inside the tensor only: no range test

struct ConvEpilogue {
    __amdgpu_buffer_rsrc_t ry, rmk, rrs;   // a null mask / residual gets a zero-record descriptor on y: its loads return 0
    bool has_mask, has_res, mask_first, mask_last;
    int ldy4, ldm4, ldr4;                  // pixel strides in bytes
    int relu_bits;

    __device__ __forceinline__ explicit ConvEpilogue(const ConvGemmParams &P) {
        const int ybytes = P.N * P.Hy * P.Wy * 4;   // per unit of pixel stride
        ry = __builtin_amdgcn_make_buffer_rsrc(P.y, 0, ybytes * P.ldy, RSRC_FLAGS);
        rmk = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(P.mask ? P.mask : P.y), 0, P.mask ? ybytes * P.ldm : 0, RSRC_FLAGS);
        rrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(P.res ? P.res : P.y), 0, P.res ? ybytes * P.ldr : 0, RSRC_FLAGS);
        has_mask = P.mask != nullptr; has_res = P.res != nullptr;
        mask_first = has_mask && !P.mask_after; mask_last = has_mask && P.mask_after;
        ldy4 = P.ldy * 4; ldm4 = P.ldm * 4; ldr4 = P.ldr * 4;
        relu_bits = P.relu_out ? 0 : (int)0x80000000;
    }

    // Eight accumulator values of channel co (co4 = 4 * co, bv = its bias) to the pixels pix[] + poff; a negative pix[q] is
    // dropped by sending its offsets to SENT, beyond every descriptor's range.  All mask loads, then all residual loads, then
    // the stores: y may alias neither, but the compiler cannot know that, and a load -> store -> load chain would serialise on
    // HBM latency.
    template <int SENT>
    __device__ __forceinline__ void store8(const float (&val)[8], const int (&pix)[8], int co4, float bv, int poff = 0) const {
        auto at = [&](int q, int ld4) {
            const int off = (pix[q] + poff) * ld4 + co4;
            if constexpr (SENT == ALL_VALID) return off;
            else return pix[q] >= 0 ? off : SENT;
        };
        float mk[8], rs[8];
        if (has_mask) {
#pragma unroll
            for (int q = 0; q < 8; ++q) mk[q] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rmk, at(q, ldm4), 0, 0));
        }
        if (has_res) {
#pragma unroll
            for (int q = 0; q < 8; ++q) rs[q] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rrs, at(q, ldr4), 0, 0));
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float v = conv_epilogue_value(val[q], bv, mk[q], rs[q], mask_first, has_res, mask_last, relu_bits);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), ry, at(q, ldy4), 0, 0);
        }
    }
};

// GEMM row of accumulator register r of a 32x32 MFMA tile, for a lane of the upper (rowq = 0) or lower (rowq = 4) half
__device__ __forceinline__ int acc_row(int rowq, int r) { return rowq + (r & 3) + 8 * (r >> 2); }

// The pointer form (conv_gemm_kernel, conv_gemm_bf16_kernel): 64-bit indexing, for the tensors the 32-bit kernels refuse.
// Wave (wm, wn) of a workgroup at (m0, n0) owns MT x NT tiles; a lane holds column (lane & 31) of 16 rows per tile.  os = 2:
// GEMM row m is pixel (ho, wo) of sub-pixel phase (oh, ow), stored at (2 ho + oh, 2 wo + ow); os = 1: row m is pixel m.
// Eight rows at a time keep the register footprint small.
template <int MT, int NT>
__device__ __forceinline__ void conv_epilogue_pointers(const ConvGemmParams &P, const f32x16 (&acc)[MT][NT], int m0, int n0,
                                                       int wm, int wn, int lane, int os, int oh, int ow) {
    const float *__restrict__ maskp = P.mask;
    const float *__restrict__ resp = P.res;
    float *__restrict__ yp = P.y;
    const bool mask_first = maskp && !P.mask_after, mask_last = maskp && P.mask_after;
    const int relu_bits = P.relu_out ? 0 : (int)0x80000000;
    const int colq = lane & 31, rowq = 4 * (lane >> 5);
    const int HoWo = P.Ho * P.Wo;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int co = n0 + (wn * NT + j) * 32 + colq;
        const bool cv = co < P.Co;
        const float bv = conv_bias_value(P, co);
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int mb = m0 + (wm * MT + i) * 32;
#pragma unroll
            for (int rb = 0; rb < 16; rb += 8) {
                size_t pix[8];
                bool ok[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int m = mb + acc_row(rowq, rb + q);
                    ok[q] = cv && m < P.M;
                    if (os == 1) {
                        pix[q] = (size_t)m;
                    } else {
                        const int n = m / HoWo;
                        const int rr = m - n * HoWo;
                        const int ho = rr / P.Wo;
                        const int wo = rr - ho * P.Wo;
                        pix[q] = (size_t)((n * P.Hy + (ho * os + oh)) * P.Wy + (wo * os + ow));
                    }
                }
                float mk[8], rs[8];
                if (maskp) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) mk[q] = ok[q] ? maskp[pix[q] * P.ldm + co] : 0.f;
                }
                if (resp) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) rs[q] = ok[q] ? resp[pix[q] * P.ldr + co] : 0.f;
                }
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const float v = conv_epilogue_value(acc[i][j][rb + q], bv, mk[q], rs[q], mask_first, resp != nullptr, mask_last, relu_bits);
                    if (ok[q]) yp[pix[q] * P.ldy + co] = v;
                }
            }
        }
    }
}

}  // namespace vq2
