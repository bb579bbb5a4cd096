// bf16-operand fused strictly causal self-attention for gfx950 (MI355X): the kernels of vq2_attn.hip with the four matrix
// products on v_mfma_f32_16x16x16_bf16 (vq2.h, vq2_causal_attn_fwd_ex / vq2_causal_attn_bwd_ex with VQ2_ALLOW_BF16).
//
// Contract.  r() is round-to-nearest-even of an fp32 value to bf16 (the compiler's conversion, v_cvt_pk_bf16_f32, as in
// vq2_conv_bf16.hip).  Every tensor in memory stays fp32.
//     forward    S = sum_d r(q) r(k) in fp32, then ONE rounded multiply by scale2; mask, running max / sum, exp2 and lse in
//                fp32 exactly as attn_fwd_kernel; the row sum adds the unrounded p; O = sum_j r(p~) r(v), p~ = p after the
//                dropout keep / inv_keep scaling; o = O / lsum.
//     backward   S again from r(q), r(k) by the same operations (the forward's bits: a row with one visible key has P = 1);
//                dP = sum_d r(dO) r(v); D = sum_j P dP and dS = P (dP - D) in fp32; dV = sum_i r(p~) r(dO);
//                dQ = scale sum_j r(dS) r(k); dK = scale sum_i r(dS) r(q).
// Mask, exact-zero row 0, dropout decision, tiling, grids and accumulation orders are those of vq2_attn.hip.
//
// Matrix shapes.  dim_head = 16 * DT exactly (eligibility), so a head has no pad channels.  As in the fp32 kernels a wave
// keeps its 16 queries (forward, delta, dQ) or 16 keys (dK / dV) on the MFMA columns.  v_mfma_f32_16x16x16_bf16 takes
// A[row = lane & 15][k = 4 g + j] and B[k = 4 g + j][col = lane & 15] (g = lane >> 4, j < 4) and leaves
// C[row = 4 g + r][col = lane & 15] in accumulator register r.  So
//     S^T[key][query] = sum_d K[key][d] Q[query][d]      A = 4 consecutive channels of a K row (LDS), B = the wave's Q
// is ONE instruction per 16 keys and 16 channels (four fp32 ones before), its result has keys 4 g + r of the lane's query
// in the 4 accumulator registers, and those, converted 4-wide, ARE the B operand of
//     O^T[d][query]   = sum_key V^T[d][key] P^T[key][query]     A = V^T[d][4 consecutive keys] (LDS, transposed tile)
// No lane movement and no LDS round trip for P, as before.
//
// LDS holds bf16, rounded while staged from 16-byte fp32 global runs.  An operand read by rows is a tile [64][DP + 8], one
// read as its transpose a tile [DP][64 + 8]; the dQ and dK / dV kernels need K, Q and dO both ways and stage both images
// from one global read.  Either way a lane's A operand is one 8-byte ds_read_b64.
// Bank conflicts by the rule bank = (byte / 4) mod 64 per 32-lane half for ds_read_b64: the row pitch is (DP + 8) / 2 =
// 4 (2 DT + 1) dwords, the transposed pitch 36 = 4 * 9 dwords, both 4 * odd, so the 16 rows of a half start 4 banks apart
// (a permutation of 0, 4, .., 60) and its two lane groups take dwords 0-1 and 2-3 of each: every operand read is
// conflict-free.  The staging stores are not: the 8-byte row stores of a 16-lane group land 2-way (pitch * 4 rows = 0 mod
// 32 banks every 8 rows at most), and the 2-byte transposed stores put the 4-channel runs of one row 16 m banks apart,
// 2 DT distinct dwords on a bank (2-way at dim_head 16, 8-way at 64), two lanes sharing each dword.  One staging pass
// per 64-key block against 16 DT operand reads per wave; not swizzled away, and not measured.
// No atomics, fixed summation orders: bit-reproducible, an image's result does not depend on its batch.
#include "vq2_attn.h"

namespace {

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

constexpr int AT_LDT = AT_BK + 8;   // bf16 per row of a transposed tile

__device__ __forceinline__ bf16x4 round4(f32x4 v) { return __builtin_convertvector(v, bf16x4); }

__device__ __forceinline__ f32x4 mfma16(bf16x4 a, bf16x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
}

// rows [r0, r0 + 64) of one head's [L, DP] fp32 matrix, rounded: as rows[64][DP + 8] (ROWS) and / or as tr[DP][64 + 8]
// (TRANS); rows >= L stage as 0
template <int DP, bool ROWS, bool TRANS>
__device__ __forceinline__ void stage_tile(__bf16 *rows, __bf16 *tr, const float *base, int ld, int r0, int L) {
    constexpr int LDR = DP + 8, V4 = DP / 4;
    for (int idx = threadIdx.x; idx < 64 * V4; idx += 256) {
        const int r = idx / V4, c = (idx - r * V4) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (r0 + r < L) {
            const float4 x = *reinterpret_cast<const float4 *>(base + (size_t)(r0 + r) * ld + c);
            v = f32x4{x.x, x.y, x.z, x.w};
        }
        const bf16x4 h = round4(v);
        if (ROWS) *reinterpret_cast<bf16x4 *>(rows + r * LDR + c) = h;
        if (TRANS) {
#pragma unroll
            for (int k = 0; k < 4; ++k) tr[(c + k) * AT_LDT + r] = h[k];
        }
    }
}

// one lane's fragment of row `row`, rounded (d = 16 * t + 4 * g ..), zero for rows outside the matrix
template <int DT>
__device__ __forceinline__ void load_frag(bf16x4 (&f)[DT], const float *base, int ld, int row, int L, int g) {
#pragma unroll
    for (int t = 0; t < DT; ++t) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row < L) {
            const float4 x = *reinterpret_cast<const float4 *>(base + (size_t)row * ld + 16 * t + 4 * g);
            v = f32x4{x.x, x.y, x.z, x.w};
        }
        f[t] = round4(v);
    }
}

template <int DT>
__device__ __forceinline__ void store_frag(const f32x4 (&acc)[DT], float mul, float *base, int ld, int row, int L, int g) {
#pragma unroll
    for (int t = 0; t < DT; ++t)
        if (row < L)
            *reinterpret_cast<float4 *>(base + (size_t)row * ld + 16 * t + 4 * g) =
                make_float4(acc[t][0] * mul, acc[t][1] * mul, acc[t][2] * mul, acc[t][3] * mul);
}

// acc[row = tile row 16 * sub + 4 g + r][col = lane's own row] = sum_d rows[16 * sub + ..][d] * frag[d]
template <int DT>
__device__ __forceinline__ f32x4 dot_tile(const __bf16 *rows, int sub, const bf16x4 (&frag)[DT], int col, int g) {
    constexpr int LDR = 16 * DT + 8;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < DT; ++t)
        acc = mfma16(*reinterpret_cast<const bf16x4 *>(rows + (16 * sub + col) * LDR + 16 * t + 4 * g), frag[t], acc);
    return acc;
}

// out[t][d = 16 t + 4 g + r][lane's own row] += sum over the 16 tile rows of sub-tile `sub` of tile[row][d] * w[row],
// the tile given transposed; w is the lane's 4 rows 4 g + j, already rounded
template <int DT>
__device__ __forceinline__ void accum_tile(f32x4 (&out)[DT], const __bf16 *tr, int sub, bf16x4 w, int col, int g) {
#pragma unroll
    for (int t = 0; t < DT; ++t)
        out[t] = mfma16(*reinterpret_cast<const bf16x4 *>(tr + (16 * t + col) * AT_LDT + 16 * sub + 4 * g), w, out[t]);
}

template <int DT>
__global__ __launch_bounds__(256) void attn_fwd_bf16_kernel(AttnParams P, const float *__restrict__ q, const float *__restrict__ k,
                                                            const float *__restrict__ v, float *__restrict__ o,
                                                            float *__restrict__ lse) {
    constexpr int DP = 16 * DT, LDR = DP + 8;
    __shared__ __attribute__((aligned(16))) __bf16 Ks[AT_BK * LDR];
    __shared__ __attribute__((aligned(16))) __bf16 Vt[DP * AT_LDT];
    const int qt = gridDim.x - 1 - blockIdx.x, h = blockIdx.y, b = blockIdx.z;   // longest tiles first
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
    const int L = P.L;
    const int iw0 = qt * AT_BQ + wave * 16, i = iw0 + col;
    const float *kb_ = k + (size_t)b * L * P.ldk + h * DP;
    const float *vb = v + (size_t)b * L * P.ldv + h * DP;
    bf16x4 qf[DT];
    load_frag<DT>(qf, q + (size_t)b * L * P.ldq + h * DP, P.ldq, i, L, g);
    f32x4 oacc[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t) oacc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, lsum = 0.f;   // lsum: this lane's share (its 4 keys of every tile); all four groups share m
    const int nkb = visible_key_blocks(qt, L);
    for (int kb = 0; kb < nkb; ++kb) {
        __syncthreads();
        stage_tile<DP, true, false>(Ks, nullptr, kb_, P.ldk, kb * AT_BK, L);
        stage_tile<DP, false, true>(nullptr, Vt, vb, P.ldv, kb * AT_BK, L);
        __syncthreads();
        const int j0 = kb * AT_BK;
        if (j0 >= iw0 + 15) continue;   // wave-uniform: none of this wave's queries sees this block
        f32x4 s[4];
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            if (j0 + 16 * kt >= iw0 + 15) { s[kt] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY}; continue; }
            s[kt] = dot_tile<DT>(Ks, kt, qf, col, g);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = j0 + 16 * kt + 4 * g + r;
                s[kt][r] = j < i ? s[kt][r] * P.scale2 : -INFINITY;
                mx = fmaxf(mx, s[kt][r]);
            }
        }
        mx = group_max(mx);
        const float m_new = fmaxf(m, mx);
        const float m_use = m_new == -INFINITY ? 0.f : m_new;
        const float alpha = exp2_fast(m - m_use);
        m = m_new;
        lsum *= alpha;
#pragma unroll
        for (int t = 0; t < DT; ++t) oacc[t] *= alpha;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            if (j0 + 16 * kt >= iw0 + 15) continue;
            f32x4 p;
#pragma unroll
            for (int r = 0; r < 4; ++r) { p[r] = exp2_fast(s[kt][r] - m_use); lsum += p[r]; }
            if (P.dropout) {
                const uint4 w = keep_words(P, b, h, i, (j0 + 16 * kt + 4 * g) >> 2);
#pragma unroll
                for (int r = 0; r < 4; ++r) p[r] = word_of(w, r) >= P.thr ? p[r] * P.inv_keep : 0.f;
            }
            accum_tile<DT>(oacc, Vt, kt, round4(p), col, g);
        }
    }
    lsum = group_sum(lsum);
    float *ob = o + (size_t)b * L * P.ldo + h * DP;
#pragma unroll
    for (int t = 0; t < DT; ++t) {
        if (i < L)
            *reinterpret_cast<float4 *>(ob + (size_t)i * P.ldo + 16 * t + 4 * g) =
                lsum > 0.f ? make_float4(oacc[t][0] / lsum, oacc[t][1] / lsum, oacc[t][2] / lsum, oacc[t][3] / lsum)
                           : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (g == 0 && i < L) lse[((size_t)b * P.nh + h) * L + i] = lsum > 0.f ? m + log2f(lsum) : 0.f;   // base-2 log-sum-exp
}

// delta[b][h][i] = sum_j P_ij dP_ij from the recomputed values (attn_delta_kernel says why it is not dO . O): the S and dP
// products of attn_dq_bf16_kernel by the same operations, each lane summing its keys in increasing order, then the four
// lane groups in a fixed order
template <int DT>
__global__ __launch_bounds__(256) void attn_delta_bf16_kernel(AttnParams P, const float *__restrict__ q, const float *__restrict__ k,
                                                              const float *__restrict__ v, const float *__restrict__ dO, int lddo,
                                                              const float *__restrict__ lse, float *__restrict__ delta) {
    constexpr int DP = 16 * DT, LDR = DP + 8;
    __shared__ __attribute__((aligned(16))) __bf16 Ks[AT_BK * LDR];
    __shared__ __attribute__((aligned(16))) __bf16 Vs[AT_BK * LDR];
    const int qt = gridDim.x - 1 - blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
    const int L = P.L;
    const int iw0 = qt * AT_BQ + wave * 16, i = iw0 + col;
    const float *kb_ = k + (size_t)b * L * P.ldk + h * DP;
    const float *vb = v + (size_t)b * L * P.ldv + h * DP;
    bf16x4 qf[DT], gf[DT];
    load_frag<DT>(qf, q + (size_t)b * L * P.ldq + h * DP, P.ldq, i, L, g);
    load_frag<DT>(gf, dO + (size_t)b * L * lddo + h * DP, lddo, i, L, g);
    const float lse_i = i < L ? lse[((size_t)b * P.nh + h) * L + i] : 0.f;
    float dsum = 0.f;
    const int nkb = visible_key_blocks(qt, L);
    for (int kb = 0; kb < nkb; ++kb) {
        __syncthreads();
        stage_tile<DP, true, false>(Ks, nullptr, kb_, P.ldk, kb * AT_BK, L);
        stage_tile<DP, true, false>(Vs, nullptr, vb, P.ldv, kb * AT_BK, L);
        __syncthreads();
        const int j0 = kb * AT_BK;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            if (j0 + 16 * kt >= iw0 + 15) continue;   // wave-uniform
            const f32x4 s = dot_tile<DT>(Ks, kt, qf, col, g);
            const f32x4 dp = dot_tile<DT>(Vs, kt, gf, col, g);
            uint4 w = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
            if (P.dropout) w = keep_words(P, b, h, i, (j0 + 16 * kt + 4 * g) >> 2);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = j0 + 16 * kt + 4 * g + r;
                const float p = (j < i && i < L) ? exp2_fast(s[r] * P.scale2 - lse_i) : 0.f;
                const float dpe = P.dropout ? (word_of(w, r) >= P.thr ? dp[r] * P.inv_keep : 0.f) : dp[r];
                dsum += p * dpe;
            }
        }
    }
    dsum = group_sum(dsum);
    if (g == 0 && i < L) delta[((size_t)b * P.nh + h) * L + i] = dsum;
}

// dQ: the forward loop again, with P recomputed from the saved log-sum-exp; K is staged both ways (rows for S, transposed
// for the dS K product)
template <int DT>
__global__ __launch_bounds__(256) void attn_dq_bf16_kernel(AttnParams P, const float *__restrict__ q, const float *__restrict__ k,
                                                           const float *__restrict__ v, const float *__restrict__ dO, int lddo,
                                                           const float *__restrict__ lse, const float *__restrict__ delta,
                                                           float *__restrict__ dq, int lddq) {
    constexpr int DP = 16 * DT, LDR = DP + 8;
    __shared__ __attribute__((aligned(16))) __bf16 Ks[AT_BK * LDR];
    __shared__ __attribute__((aligned(16))) __bf16 Kt[DP * AT_LDT];
    __shared__ __attribute__((aligned(16))) __bf16 Vs[AT_BK * LDR];
    const int qt = gridDim.x - 1 - blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
    const int L = P.L;
    const int iw0 = qt * AT_BQ + wave * 16, i = iw0 + col;
    const float *kb_ = k + (size_t)b * L * P.ldk + h * DP;
    const float *vb = v + (size_t)b * L * P.ldv + h * DP;
    bf16x4 qf[DT], gf[DT];
    load_frag<DT>(qf, q + (size_t)b * L * P.ldq + h * DP, P.ldq, i, L, g);
    load_frag<DT>(gf, dO + (size_t)b * L * lddo + h * DP, lddo, i, L, g);
    const float lse_i = i < L ? lse[((size_t)b * P.nh + h) * L + i] : 0.f;
    const float del_i = i < L ? delta[((size_t)b * P.nh + h) * L + i] : 0.f;
    f32x4 acc[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nkb = visible_key_blocks(qt, L);
    for (int kb = 0; kb < nkb; ++kb) {
        __syncthreads();
        stage_tile<DP, true, true>(Ks, Kt, kb_, P.ldk, kb * AT_BK, L);
        stage_tile<DP, true, false>(Vs, nullptr, vb, P.ldv, kb * AT_BK, L);
        __syncthreads();
        const int j0 = kb * AT_BK;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            if (j0 + 16 * kt >= iw0 + 15) continue;   // wave-uniform
            const f32x4 s = dot_tile<DT>(Ks, kt, qf, col, g);
            const f32x4 dp = dot_tile<DT>(Vs, kt, gf, col, g);
            uint4 w = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
            if (P.dropout) w = keep_words(P, b, h, i, (j0 + 16 * kt + 4 * g) >> 2);
            f32x4 ds;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = j0 + 16 * kt + 4 * g + r;
                const float p = (j < i && i < L) ? exp2_fast(s[r] * P.scale2 - lse_i) : 0.f;
                const float dpe = P.dropout ? (word_of(w, r) >= P.thr ? dp[r] * P.inv_keep : 0.f) : dp[r];
                ds[r] = p * (dpe - del_i);
            }
            accum_tile<DT>(acc, Kt, kt, round4(ds), col, g);
        }
    }
    store_frag<DT>(acc, P.scale, dq + (size_t)b * L * lddq + h * DP, lddq, i, L, g);
}

// dK, dV: one workgroup per key block, query tiles in increasing order; Q and dO are staged both ways
template <int DT>
__global__ __launch_bounds__(256) void attn_dkv_bf16_kernel(AttnParams P, const float *__restrict__ q, const float *__restrict__ k,
                                                            const float *__restrict__ v, const float *__restrict__ dO, int lddo,
                                                            const float *__restrict__ lse, const float *__restrict__ delta,
                                                            float *__restrict__ dk, int lddk, float *__restrict__ dv, int lddv) {
    constexpr int DP = 16 * DT, LDR = DP + 8;
    __shared__ __attribute__((aligned(16))) __bf16 Qs[AT_BQ * LDR];
    __shared__ __attribute__((aligned(16))) __bf16 Qt[DP * AT_LDT];
    __shared__ __attribute__((aligned(16))) __bf16 Gs[AT_BQ * LDR];
    __shared__ __attribute__((aligned(16))) __bf16 Gt[DP * AT_LDT];
    __shared__ __attribute__((aligned(16))) float lses[AT_BQ];
    __shared__ __attribute__((aligned(16))) float dels[AT_BQ];
    const int jb = blockIdx.x, h = blockIdx.y, b = blockIdx.z;   // key block 0 is the longest: natural order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
    const int L = P.L;
    const int jw0 = jb * AT_BK + wave * 16, j = jw0 + col;
    const float *qb = q + (size_t)b * L * P.ldq + h * DP;
    const float *gb = dO + (size_t)b * L * lddo + h * DP;
    const float *lb = lse + ((size_t)b * P.nh + h) * L;
    const float *db = delta + ((size_t)b * P.nh + h) * L;
    bf16x4 kf[DT], vf[DT];
    load_frag<DT>(kf, k + (size_t)b * L * P.ldk + h * DP, P.ldk, j, L, g);
    load_frag<DT>(vf, v + (size_t)b * L * P.ldv + h * DP, P.ldv, j, L, g);
    f32x4 dka[DT], dva[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t) { dka[t] = f32x4{0.f, 0.f, 0.f, 0.f}; dva[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    const int nqt = (L + AT_BQ - 1) / AT_BQ;
    for (int it = jb; it < nqt; ++it) {   // queries > the block's first key start in tile jb (AT_BQ == AT_BK)
        __syncthreads();
        stage_tile<DP, true, true>(Qs, Qt, qb, P.ldq, it * AT_BQ, L);
        stage_tile<DP, true, true>(Gs, Gt, gb, lddo, it * AT_BQ, L);
        if (threadIdx.x < AT_BQ) {
            const int i = it * AT_BQ + threadIdx.x;
            lses[threadIdx.x] = i < L ? lb[i] : 0.f;
            dels[threadIdx.x] = i < L ? db[i] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int qs = 0; qs < 4; ++qs) {
            const int ib = it * AT_BQ + 16 * qs;
            if (ib + 15 <= jw0 || ib >= L) continue;   // wave-uniform: no query of the sub-tile is past this wave's first key
            const f32x4 s = dot_tile<DT>(Qs, qs, kf, col, g);
            const f32x4 dp = dot_tile<DT>(Gs, qs, vf, col, g);
            const float4 l4 = *reinterpret_cast<const float4 *>(lses + 16 * qs + 4 * g);
            const float4 d4 = *reinterpret_cast<const float4 *>(dels + 16 * qs + 4 * g);
            const float lr[4] = {l4.x, l4.y, l4.z, l4.w}, dr[4] = {d4.x, d4.y, d4.z, d4.w};
            f32x4 pd, ds;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = ib + 4 * g + r;
                const float p = (j < i && i < L) ? exp2_fast(s[r] * P.scale2 - lr[r]) : 0.f;
                float pk = p, dpe = dp[r];
                if (P.dropout) {
                    const bool keep = word_of(keep_words(P, b, h, i, j >> 2), j & 3) >= P.thr;
                    pk = keep ? p * P.inv_keep : 0.f;
                    dpe = keep ? dp[r] * P.inv_keep : 0.f;
                }
                pd[r] = pk;
                ds[r] = p * (dpe - dr[r]);
            }
            accum_tile<DT>(dva, Gt, qs, round4(pd), col, g);
            accum_tile<DT>(dka, Qt, qs, round4(ds), col, g);
        }
    }
    store_frag<DT>(dka, P.scale, dk + (size_t)b * L * lddk + h * DP, lddk, j, L, g);
    store_frag<DT>(dva, 1.f, dv + (size_t)b * L * lddv + h * DP, lddv, j, L, g);
}

int check_flags(int flags, const char *what) {
    VQ2_REQUIRE((flags & ~VQ2_ALLOW_BF16) == 0, "%s: flags may hold VQ2_ALLOW_BF16 only (got %d)", what, flags);
    return VQ2_OK;
}

// profile label of a launch: kernel<DT>|shape,bf16 (a non-conv family, so the format is a constant as in vq2_elem.hip)
const char ATTN_LABEL[] = "%s<%d>|B=%d,L=%d,nh=%d,dh=%d,bf16";
const char *attn_label(const char *kernel, const AttnParams &P) {
    return vq2::prof_enabled() ? vq2::prof_label(ATTN_LABEL, kernel, P.dh / 16, P.B, P.L, P.nh, P.dh) : kernel;
}
// counted work of one pass over the visible (i, j) pairs: `products` matrix products of 2 * dim_head flops each
double attn_flops(const AttnParams &P, int products) {
    return (double)products * P.B * P.nh * P.dh * (double)P.L * (P.L - 1);
}
double attn_bytes(const AttnParams &P, int tensors) { return 4.0 * tensors * P.B * P.L * (double)P.nh * P.dh; }

}  // namespace

extern "C" int vq2_causal_attn_bf16_eligible(const vq2_attn_desc *d) {
    return d && d->dim_head >= 16 && d->dim_head <= 64 && d->dim_head % 16 == 0;
}

extern "C" int vq2_causal_attn_fwd_ex(const vq2_attn_desc *d, int flags, const float *q, const float *k, const float *v, float *o,
                                      float *lse, vq2_stream_t stream) {
    if (int e = check_flags(flags, "causal_attn_fwd_ex")) return e;
    if (!(flags & VQ2_ALLOW_BF16) || !vq2_causal_attn_bf16_eligible(d)) return vq2_causal_attn_fwd(d, q, k, v, o, lse, stream);
    AttnParams P;
    if (int e = fill_params(d, P, "causal_attn_fwd_ex")) return e;
    VQ2_REQUIRE(q && k && v && o && lse, "causal_attn_fwd_ex: null pointer");
    VQ2_REQUIRE(vq2::aligned16(q) && vq2::aligned16(k) && vq2::aligned16(v) && vq2::aligned16(o),
                "causal_attn_fwd_ex: pointers must be 16-byte aligned");
    hipStream_t s = vq2::to_stream(stream);
    const dim3 grid((P.L + AT_BQ - 1) / AT_BQ, P.nh, P.B);
    vq2::ProfScope prof(attn_label("attn_fwd", P), attn_flops(P, 2), attn_bytes(P, 4), s);
    ATTN_BY_DT(P.dh, hipLaunchKernelGGL((attn_fwd_bf16_kernel<DT>), grid, dim3(256), 0, s, P, q, k, v, o, lse));
    return vq2::check_launch("attn_fwd_bf16_kernel");
}

extern "C" int vq2_causal_attn_bwd_ex(const vq2_attn_desc *d, int flags, const float *q, const float *k, const float *v,
                                      const float *lse, const float *dO, int32_t lddo, float *dq, int32_t lddq, float *dk,
                                      int32_t lddk, float *dv, int32_t lddv, float *delta_ws, vq2_stream_t stream) {
    if (int e = check_flags(flags, "causal_attn_bwd_ex")) return e;
    if (!(flags & VQ2_ALLOW_BF16) || !vq2_causal_attn_bf16_eligible(d))
        return vq2_causal_attn_bwd(d, q, k, v, lse, dO, lddo, dq, lddq, dk, lddk, dv, lddv, delta_ws, stream);
    AttnParams P;
    if (int e = fill_params(d, P, "causal_attn_bwd_ex")) return e;
    VQ2_REQUIRE(q && k && v && lse && dO && dq && dk && dv && delta_ws, "causal_attn_bwd_ex: null pointer");
    VQ2_REQUIRE(vq2::aligned16(q) && vq2::aligned16(k) && vq2::aligned16(v) && vq2::aligned16(dO) &&
                    vq2::aligned16(dq) && vq2::aligned16(dk) && vq2::aligned16(dv),
                "causal_attn_bwd_ex: pointers must be 16-byte aligned");
    const int ch = P.nh * P.dh;
    VQ2_REQUIRE(lddo >= ch && lddq >= ch && lddk >= ch && lddv >= ch && lddo % 4 == 0 && lddq % 4 == 0 && lddk % 4 == 0 && lddv % 4 == 0,
                "causal_attn_bwd_ex: gradient pixel strides must be multiples of 4, at least n_head * dim_head");
    hipStream_t s = vq2::to_stream(stream);
    const dim3 grid((P.L + AT_BQ - 1) / AT_BQ, P.nh, P.B);
    {
        vq2::ProfScope prof(attn_label("attn_delta", P), attn_flops(P, 2), attn_bytes(P, 4), s);
        ATTN_BY_DT(P.dh, hipLaunchKernelGGL((attn_delta_bf16_kernel<DT>), grid, dim3(256), 0, s, P, q, k, v, dO, lddo, lse, delta_ws));
        if (int e = vq2::check_launch("attn_delta_bf16_kernel")) return e;
    }
    {
        vq2::ProfScope prof(attn_label("attn_dkv", P), attn_flops(P, 4), attn_bytes(P, 6), s);
        ATTN_BY_DT(P.dh, hipLaunchKernelGGL((attn_dkv_bf16_kernel<DT>), grid, dim3(256), 0, s, P, q, k, v, dO, lddo, lse, delta_ws, dk, lddk, dv, lddv));
        if (int e = vq2::check_launch("attn_dkv_bf16_kernel")) return e;
    }
    vq2::ProfScope prof(attn_label("attn_dq", P), attn_flops(P, 3), attn_bytes(P, 5), s);
    ATTN_BY_DT(P.dh, hipLaunchKernelGGL((attn_dq_bf16_kernel<DT>), grid, dim3(256), 0, s, P, q, k, v, dO, lddo, lse, delta_ws, dq, lddq));
    return vq2::check_launch("attn_dq_bf16_kernel");
}
