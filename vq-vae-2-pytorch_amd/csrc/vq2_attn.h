// What the fp32 attention kernels (vq2_attn.hip) and the bf16-operand ones (vq2_attn_bf16.hip) share: the tile lengths, the
// launch parameters and their validation, the dropout decision, the base-2 exponential and the half-wave exchanges.
// Everything is in an unnamed namespace, as it was inside vq2_attn.hip: each of the two files gets its own internal copy,
// and the fp32 kernels keep their symbol names and their device code ("bf16 attention").
#pragma once
#include "vq2_common.h"
#include "vq2_philox.h"

namespace {

constexpr int AT_BQ = 64;   // queries per workgroup (4 waves x 16)
constexpr int AT_BK = 64;   // keys per staged block
// attn_dkv_kernel starts its query-tile loop at its own key-block index and runs on the grid of query tiles
static_assert(AT_BQ == AT_BK, "the dK/dV kernel and the backward launch grid assume equal query and key tile lengths");

struct AttnParams {
    int B, L, nh, dh;
    int ldq, ldk, ldv, ldo;
    float scale;      // 1 / sqrt(dim_head)
    float scale2;     // scale * log2(e): scores are kept in the base-2 domain (v_exp_f32 is 2^x).  Every kernel forms
                      // s * scale2 as ONE rounded multiply of the same MFMA sum, so the backward pass sees the forward's
                      // scores bit for bit (a row with a single visible key has P = 1 exactly in all three)
    float inv_keep;   // 1 / (1 - p)
    uint32_t thr;     // keep iff word >= thr
    uint32_t seed_lo, seed_hi;
    int dropout;
};

using vq2::philox4x32_7;
// the four keep words of keys 4 * jq .. 4 * jq + 3 for query i
__device__ __forceinline__ uint4 keep_words(const AttnParams &P, int b, int h, int i, int jq) {
    return philox4x32_7((uint32_t)jq, (uint32_t)i, (uint32_t)b, (uint32_t)h, P.seed_lo, P.seed_hi);
}
__device__ __forceinline__ uint32_t word_of(uint4 w, int k) { return k == 0 ? w.x : k == 1 ? w.y : k == 2 ? w.z : w.w; }

__device__ __forceinline__ float exp2_fast(float x) { return __builtin_amdgcn_exp2f(x); }

__device__ __forceinline__ float group_max(float v) {   // over the four lane groups that share a column
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float group_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

// number of key blocks a query tile can see: keys 0 .. min(L - 1, last query of the tile) - 1
__device__ __forceinline__ int visible_key_blocks(int qt, int L) {
    const int imax = min(L - 1, qt * AT_BQ + AT_BQ - 1);
    return imax >= 1 ? (imax - 1) / AT_BK + 1 : 0;
}

int fill_params(const vq2_attn_desc *d, AttnParams &P, const char *what) {
    VQ2_REQUIRE(d, "%s: null descriptor", what);
    VQ2_REQUIRE(d->B >= 1 && d->L >= 1 && d->n_head >= 1, "%s: non-positive size", what);
    VQ2_REQUIRE(d->dim_head >= 4 && d->dim_head <= 64 && d->dim_head % 4 == 0,
                "%s: dim_head must be a multiple of 4 in 4..64 (got %d)", what, d->dim_head);
    VQ2_REQUIRE(d->B <= 65535 && d->n_head <= 65535, "%s: at most 65535 batch items and heads", what);
    const int64_t ch = (int64_t)d->n_head * d->dim_head;
    VQ2_REQUIRE(d->ldq >= ch && d->ldk >= ch && d->ldv >= ch && d->ldo >= ch, "%s: pixel stride below n_head * dim_head", what);
    VQ2_REQUIRE(d->ldq % 4 == 0 && d->ldk % 4 == 0 && d->ldv % 4 == 0 && d->ldo % 4 == 0, "%s: pixel strides must be multiples of 4", what);
    VQ2_REQUIRE((double)d->B * d->L * d->n_head < 2147483648.0, "%s: B * L * n_head exceeds 2^31", what);
    VQ2_REQUIRE(d->p_drop >= 0.f && d->p_drop < 1.f, "%s: dropout probability must be in [0, 1)", what);
    P.B = d->B; P.L = d->L; P.nh = d->n_head; P.dh = d->dim_head;
    P.ldq = d->ldq; P.ldk = d->ldk; P.ldv = d->ldv; P.ldo = d->ldo;
    const double sc = 1.0 / sqrt((double)d->dim_head);
    P.scale = (float)sc;
    P.scale2 = (float)(sc * 1.4426950408889634);
    P.dropout = d->p_drop > 0.f;
    P.inv_keep = (float)(1.0 / (1.0 - (double)d->p_drop));
    P.thr = (uint32_t)((double)d->p_drop * 4294967296.0);
    P.seed_lo = (uint32_t)(d->seed & 0xFFFFFFFFu);
    P.seed_hi = (uint32_t)(d->seed >> 32);
    return VQ2_OK;
}

}  // namespace

#define ATTN_BY_DT(dh, ...)                   \
    switch (((dh) + 15) / 16) {               \
    case 1: { constexpr int DT = 1; __VA_ARGS__; } break; \
    case 2: { constexpr int DT = 2; __VA_ARGS__; } break; \
    case 3: { constexpr int DT = 3; __VA_ARGS__; } break; \
    default: { constexpr int DT = 4; __VA_ARGS__; } break; \
    }
