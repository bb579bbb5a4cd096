// Fused strictly causal self-attention (PixelSNAIL CausalAttention, reference pixelsnail.py:195-234) and the
// weight-norm reparametrisation of its three projections (pixelsnail.py:17-18), fp32 in and out.
//
// Query i attends to keys j < i (the diagonal is masked; row 0 sees nothing and is exactly 0).  Scores and
// probabilities exist only in registers: the forward pass keeps a running max / sum per query (online softmax) and
// leaves one log-sum-exp per (b, h, i); the backward pass recomputes P from Q, K and that value.
//
// Matrix shapes.  Everything runs on v_mfma_f32_16x16x4_f32 (exact fp32).  Its k step of 4 is what makes every
// dim_head % 4 == 0 a whole number of steps; heads are zero-padded to DP = 16 * DT floats (DT = 1..4 is the template
// argument), which only costs for widths that are no multiple of 16.  One wave owns 16 queries (forward, dQ) or 16
// keys (dK / dV) and keeps them on the MFMA *columns* (lane & 15): then
//     S^T[key][query]  = sum_d K[key][d] Q[query][d]          A = K rows from LDS, B = the wave's Q in registers
// comes out with the query on the lane and 4 consecutive keys in the 4 accumulator registers of lane group g = lane >> 4
// (key = 16 * tile + 4 * g + r), and the second product
//     O^T[d][query]    = sum_key V^T[d][key] P^T[key][query]
// takes accumulator register r as the B operand of k step r directly: the MFMA sums over (g, r) in some order, and the A
// operand V^T[d][16 * tile + 4 * g + r] is read from LDS in that same order.  No lane movement, no LDS round trip for
// P.  The same argument picks d = 16 * t + 4 * g + s for k step s of the first product, so both operands of it are
// float4 reads of 4 consecutive head channels.  Softmax statistics are per lane plus two half-wave exchanges.
//
// Bit-reproducible: no atomics.  dK / dV are accumulated per key block over the query tiles in increasing order
// (attn_dkv_kernel), dQ per query tile over the key blocks in increasing order (attn_dq_kernel).
//
// Dropout: keep(seed, b, h, i, j) = word (j & 3) of Philox4x32-7 with counter (j >> 2, i, b, h) and key = the 64-bit
// seed, >= floor(p * 2^32).  Nothing else enters (no tile size, no launch geometry, same in forward and backward);
// attn_keep_mask_kernel writes it out as bytes for tests.
#include "vq2_attn.h"

namespace {

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// rows [r0, r0 + 64) of one head's [L, dh] matrix -> LDS tile [64][DP + 4]; rows >= L and channels >= dh read as 0
template <int DP>
__device__ __forceinline__ void stage_tile(float *tile, const float *base, int ld, int r0, int L, int dh) {
    constexpr int LDR = DP + 4, V4 = DP / 4;
    for (int idx = threadIdx.x; idx < 64 * V4; idx += 256) {
        const int r = idx / V4, c = (idx - r * V4) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r0 + r < L && c < dh) v = *reinterpret_cast<const float4 *>(base + (size_t)(r0 + r) * ld + c);
        *reinterpret_cast<float4 *>(tile + r * LDR + c) = v;
    }
}

// one lane's 4 * DT-float fragment of row `row` (d = 16 * t + 4 * g ..), zero outside the matrix
template <int DT>
__device__ __forceinline__ void load_frag(float4 (&f)[DT], const float *base, int ld, int row, int L, int dh, int g) {
#pragma unroll
    for (int t = 0; t < DT; ++t) {
        const int d = 16 * t + 4 * g;
        f[t] = (row < L && d < dh) ? *reinterpret_cast<const float4 *>(base + (size_t)row * ld + d) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

template <int DT>
__device__ __forceinline__ void store_frag(const f32x4 (&acc)[DT], float mul, float *base, int ld, int row, int L, int dh, int g) {
#pragma unroll
    for (int t = 0; t < DT; ++t) {
        const int d = 16 * t + 4 * g;
        if (row < L && d < dh)
            *reinterpret_cast<float4 *>(base + (size_t)row * ld + d) = make_float4(acc[t][0] * mul, acc[t][1] * mul, acc[t][2] * mul, acc[t][3] * mul);
    }
}

// acc[row = LDS row][col = lane's own row] = sum_d tile[16 * sub + (lane & 15)][d] * frag[d]
template <int DT>
__device__ __forceinline__ f32x4 dot_tile(const float *tile, int sub, const float4 (&frag)[DT], int col, int g) {
    constexpr int LDR = 16 * DT + 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < DT; ++t) {
        const float4 a = *reinterpret_cast<const float4 *>(tile + (16 * sub + col) * LDR + 16 * t + 4 * g);
        acc = mfma4(a.x, frag[t].x, acc);
        acc = mfma4(a.y, frag[t].y, acc);
        acc = mfma4(a.z, frag[t].z, acc);
        acc = mfma4(a.w, frag[t].w, acc);
    }
    return acc;
}

// out[t][d][lane's own row] += sum over the 16 LDS rows of sub-tile `sub` of tile[row][d] * w[row]
template <int DT>
__device__ __forceinline__ void accum_tile(f32x4 (&out)[DT], const float *tile, int sub, f32x4 w, int col, int g) {
    constexpr int LDR = 16 * DT + 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float *row = tile + (16 * sub + 4 * g + r) * LDR + col;
#pragma unroll
        for (int t = 0; t < DT; ++t) out[t] = mfma4(row[16 * t], w[r], out[t]);
    }
}

template <int DT>
__global__ __launch_bounds__(256) void attn_fwd_kernel(AttnParams P, const float *__restrict__ q, const float *__restrict__ k,
                                                       const float *__restrict__ v, float *__restrict__ o, float *__restrict__ lse) {
    constexpr int DP = 16 * DT, LDR = DP + 4;
    __shared__ __attribute__((aligned(16))) float Ks[AT_BK * LDR];
    __shared__ __attribute__((aligned(16))) float Vs[AT_BK * LDR];
    const int qt = gridDim.x - 1 - blockIdx.x, h = blockIdx.y, b = blockIdx.z;   // longest tiles first
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
    const int L = P.L, dh = P.dh;
    const int iw0 = qt * AT_BQ + wave * 16, i = iw0 + col;
    const float *qb = q + (size_t)b * L * P.ldq + h * dh;
    const float *kb_ = k + (size_t)b * L * P.ldk + h * dh;
    const float *vb = v + (size_t)b * L * P.ldv + h * dh;
    float4 qf[DT];
    load_frag<DT>(qf, qb, P.ldq, i, L, dh, g);
    f32x4 oacc[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t) oacc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, lsum = 0.f;   // lsum: this lane's share (its 4 keys of every tile); all four groups share m
    const int nkb = visible_key_blocks(qt, L);
    for (int kb = 0; kb < nkb; ++kb) {
        __syncthreads();
        stage_tile<DP>(Ks, kb_, P.ldk, kb * AT_BK, L, dh);
        stage_tile<DP>(Vs, vb, P.ldv, kb * AT_BK, L, dh);
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
            accum_tile<DT>(oacc, Vs, kt, p, col, g);
        }
    }
    lsum = group_sum(lsum);
    float *ob = o + (size_t)b * L * P.ldo + h * dh;
#pragma unroll
    for (int t = 0; t < DT; ++t) {
        const int d = 16 * t + 4 * g;
        if (i < L && d < dh)
            *reinterpret_cast<float4 *>(ob + (size_t)i * P.ldo + d) =
                lsum > 0.f ? make_float4(oacc[t][0] / lsum, oacc[t][1] / lsum, oacc[t][2] / lsum, oacc[t][3] / lsum)
                           : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (g == 0 && i < L) lse[((size_t)b * P.nh + h) * L + i] = lsum > 0.f ? m + log2f(lsum) : 0.f;   // base-2 log-sum-exp
}

// ---------------------------------------------------------------- a window of queries over keys kept by image row
// The forward loop for the queries at raster positions q0 .. q0 + nq - 1 only (the sampler's current row, vq2.h
// vq2_causal_attn_fwd_rows): q and o are dense [B, nq, ld], the key / value at position p lives at image row p / W of a
// buffer with its own image and row strides, so that a history of rows in any layout is read in place.  Key blocks start
// at multiples of AT_BK from position 0 as in attn_fwd_kernel and each query's statistics are its own lane's, so a query
// gets bit for bit what the full-sequence kernel gives it.  No dropout, no log-sum-exp.
struct AttnRows {
    int q0, nq, W;
    long long kv_image_stride, kv_row_stride;
};

// positions [r0, r0 + 64) of one head -> LDS tile [64][DP + 4]; positions >= Lk and channels >= dh read as 0
template <int DP>
__device__ __forceinline__ void stage_tile_rows(float *tile, const float *base, int ld, int r0, int Lk, int dh, int W,
                                                long long row_stride) {
    constexpr int LDR = DP + 4, V4 = DP / 4;
    for (int idx = threadIdx.x; idx < 64 * V4; idx += 256) {
        const int r = idx / V4, c = (idx - r * V4) * 4;
        const int p = r0 + r;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p < Lk && c < dh) {
            const int pr = p / W, pc = p - pr * W;
            v = *reinterpret_cast<const float4 *>(base + (long long)pr * row_stride + (long long)pc * ld + c);
        }
        *reinterpret_cast<float4 *>(tile + r * LDR + c) = v;
    }
}

template <int DT>
__global__ __launch_bounds__(256) void attn_fwd_rows_kernel(AttnParams P, AttnRows R, const float *__restrict__ q,
                                                            const float *__restrict__ k, const float *__restrict__ v,
                                                            float *__restrict__ o) {
    constexpr int DP = 16 * DT, LDR = DP + 4;
    __shared__ __attribute__((aligned(16))) float Ks[AT_BK * LDR];
    __shared__ __attribute__((aligned(16))) float Vs[AT_BK * LDR];
    const int qt = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
    const int dh = P.dh, nq = R.nq;
    const int lq = qt * AT_BQ + wave * 16 + col;        // index inside the window
    const int iw0 = R.q0 + qt * AT_BQ + wave * 16, i = iw0 + col;   // raster positions
    const int Lk = R.q0 + nq - 1;                       // the last query's own position and everything past it is visible to no query: never read
    const float *kb_ = k + (long long)b * R.kv_image_stride + h * dh;
    const float *vb = v + (long long)b * R.kv_image_stride + h * dh;
    float4 qf[DT];
    load_frag<DT>(qf, q + (size_t)b * nq * P.ldq + h * dh, P.ldq, lq, nq, dh, g);
    f32x4 oacc[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t) oacc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, lsum = 0.f;
    const int imax = R.q0 + min(nq - 1, qt * AT_BQ + AT_BQ - 1);
    const int nkb = imax >= 1 ? (imax - 1) / AT_BK + 1 : 0;
    for (int kb = 0; kb < nkb; ++kb) {
        __syncthreads();
        stage_tile_rows<DP>(Ks, kb_, P.ldk, kb * AT_BK, Lk, dh, R.W, R.kv_row_stride);
        stage_tile_rows<DP>(Vs, vb, P.ldv, kb * AT_BK, Lk, dh, R.W, R.kv_row_stride);
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
            accum_tile<DT>(oacc, Vs, kt, p, col, g);
        }
    }
    lsum = group_sum(lsum);
    float *ob = o + (size_t)b * nq * P.ldo + h * dh;
#pragma unroll
    for (int t = 0; t < DT; ++t) {
        const int d = 16 * t + 4 * g;
        if (lq < nq && d < dh)
            *reinterpret_cast<float4 *>(ob + (size_t)lq * P.ldo + d) =
                lsum > 0.f ? make_float4(oacc[t][0] / lsum, oacc[t][1] / lsum, oacc[t][2] / lsum, oacc[t][3] / lsum)
                           : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// delta[b][h][i] = sum_j P_ij dP_ij (with dropout: of the kept, rescaled dP), the row term D_i of the softmax backward
// dS = P (dP - D).  In exact arithmetic D_i = sum_d dO_id O_id, and that form needs no pass over the keys; but it is
// rounded independently of dP, and where a row sees only a few keys dP - D cancels: at L = 3 the dK error came out at 5.4 x
// that of a plain fp32 evaluation, whose softmax backward forms D from the very dP values it is subtracted from, so
// that their errors cancel with it.  This kernel forms D that way: the forward loop again (the S and dP products of
// attn_dq_kernel, by the same operations, so a row with one visible key has D = dP and dS = 0 exactly), each lane
// summing its keys in increasing order, then the four lane groups in a fixed order.
template <int DT>
__global__ __launch_bounds__(256) void attn_delta_kernel(AttnParams P, const float *__restrict__ q, const float *__restrict__ k,
                                                         const float *__restrict__ v, const float *__restrict__ dO, int lddo,
                                                         const float *__restrict__ lse, float *__restrict__ delta) {
    constexpr int DP = 16 * DT, LDR = DP + 4;
    __shared__ __attribute__((aligned(16))) float Ks[AT_BK * LDR];
    __shared__ __attribute__((aligned(16))) float Vs[AT_BK * LDR];
    const int qt = gridDim.x - 1 - blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
    const int L = P.L, dh = P.dh;
    const int iw0 = qt * AT_BQ + wave * 16, i = iw0 + col;
    const float *kb_ = k + (size_t)b * L * P.ldk + h * dh;
    const float *vb = v + (size_t)b * L * P.ldv + h * dh;
    float4 qf[DT], gf[DT];
    load_frag<DT>(qf, q + (size_t)b * L * P.ldq + h * dh, P.ldq, i, L, dh, g);
    load_frag<DT>(gf, dO + (size_t)b * L * lddo + h * dh, lddo, i, L, dh, g);
    const float lse_i = i < L ? lse[((size_t)b * P.nh + h) * L + i] : 0.f;
    float dsum = 0.f;
    const int nkb = visible_key_blocks(qt, L);
    for (int kb = 0; kb < nkb; ++kb) {
        __syncthreads();
        stage_tile<DP>(Ks, kb_, P.ldk, kb * AT_BK, L, dh);
        stage_tile<DP>(Vs, vb, P.ldv, kb * AT_BK, L, dh);
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

// dQ: the forward loop again, with P recomputed from the saved log-sum-exp
template <int DT>
__global__ __launch_bounds__(256) void attn_dq_kernel(AttnParams P, const float *__restrict__ q, const float *__restrict__ k,
                                                      const float *__restrict__ v, const float *__restrict__ dO, int lddo,
                                                      const float *__restrict__ lse, const float *__restrict__ delta,
                                                      float *__restrict__ dq, int lddq) {
    constexpr int DP = 16 * DT, LDR = DP + 4;
    __shared__ __attribute__((aligned(16))) float Ks[AT_BK * LDR];
    __shared__ __attribute__((aligned(16))) float Vs[AT_BK * LDR];
    const int qt = gridDim.x - 1 - blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
    const int L = P.L, dh = P.dh;
    const int iw0 = qt * AT_BQ + wave * 16, i = iw0 + col;
    const float *kb_ = k + (size_t)b * L * P.ldk + h * dh;
    const float *vb = v + (size_t)b * L * P.ldv + h * dh;
    float4 qf[DT], gf[DT];
    load_frag<DT>(qf, q + (size_t)b * L * P.ldq + h * dh, P.ldq, i, L, dh, g);
    load_frag<DT>(gf, dO + (size_t)b * L * lddo + h * dh, lddo, i, L, dh, g);
    const float lse_i = i < L ? lse[((size_t)b * P.nh + h) * L + i] : 0.f;
    const float del_i = i < L ? delta[((size_t)b * P.nh + h) * L + i] : 0.f;
    f32x4 acc[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nkb = visible_key_blocks(qt, L);
    for (int kb = 0; kb < nkb; ++kb) {
        __syncthreads();
        stage_tile<DP>(Ks, kb_, P.ldk, kb * AT_BK, L, dh);
        stage_tile<DP>(Vs, vb, P.ldv, kb * AT_BK, L, dh);
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
            accum_tile<DT>(acc, Ks, kt, ds, col, g);
        }
    }
    store_frag<DT>(acc, P.scale, dq + (size_t)b * L * lddq + h * dh, lddq, i, L, dh, g);
}

// dK, dV: one workgroup per key block, query tiles in increasing order
template <int DT>
__global__ __launch_bounds__(256) void attn_dkv_kernel(AttnParams P, const float *__restrict__ q, const float *__restrict__ k,
                                                       const float *__restrict__ v, const float *__restrict__ dO, int lddo,
                                                       const float *__restrict__ lse, const float *__restrict__ delta,
                                                       float *__restrict__ dk, int lddk, float *__restrict__ dv, int lddv) {
    constexpr int DP = 16 * DT, LDR = DP + 4;
    __shared__ __attribute__((aligned(16))) float Qs[AT_BQ * LDR];
    __shared__ __attribute__((aligned(16))) float Gs[AT_BQ * LDR];
    __shared__ __attribute__((aligned(16))) float lses[AT_BQ];
    __shared__ __attribute__((aligned(16))) float dels[AT_BQ];
    const int jb = blockIdx.x, h = blockIdx.y, b = blockIdx.z;   // key block 0 is the longest: natural order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
    const int L = P.L, dh = P.dh;
    const int jw0 = jb * AT_BK + wave * 16, j = jw0 + col;
    const float *qb = q + (size_t)b * L * P.ldq + h * dh;
    const float *gb = dO + (size_t)b * L * lddo + h * dh;
    const float *lb = lse + ((size_t)b * P.nh + h) * L;
    const float *db = delta + ((size_t)b * P.nh + h) * L;
    float4 kf[DT], vf[DT];
    load_frag<DT>(kf, k + (size_t)b * L * P.ldk + h * dh, P.ldk, j, L, dh, g);
    load_frag<DT>(vf, v + (size_t)b * L * P.ldv + h * dh, P.ldv, j, L, dh, g);
    f32x4 dka[DT], dva[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t) { dka[t] = f32x4{0.f, 0.f, 0.f, 0.f}; dva[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    const int nqt = (L + AT_BQ - 1) / AT_BQ;
    for (int it = jb; it < nqt; ++it) {   // queries > the block's first key start in tile jb (AT_BQ == AT_BK)
        __syncthreads();
        stage_tile<DP>(Qs, qb, P.ldq, it * AT_BQ, L, dh);
        stage_tile<DP>(Gs, gb, lddo, it * AT_BQ, L, dh);
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
            accum_tile<DT>(dva, Gs, qs, pd, col, g);
            accum_tile<DT>(dka, Qs, qs, ds, col, g);
        }
    }
    store_frag<DT>(dka, P.scale, dk + (size_t)b * L * lddk + h * dh, lddk, j, L, dh, g);
    store_frag<DT>(dva, 1.f, dv + (size_t)b * L * lddv + h * dh, lddv, j, L, dh, g);
}

// keep decisions as bytes [B][nh][L][L] (every (i, j), the causal mask is not applied)
__global__ __launch_bounds__(256) void attn_keep_mask_kernel(AttnParams P, uint8_t *__restrict__ mask) {
    const int Lq = (P.L + 3) / 4;
    const size_t total = (size_t)P.B * P.nh * P.L * Lq;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int jq = (int)(idx % Lq);
    const int i = (int)((idx / Lq) % P.L);
    const int h = (int)((idx / ((size_t)Lq * P.L)) % P.nh);
    const int b = (int)(idx / ((size_t)Lq * P.L * P.nh));
    const uint4 w = keep_words(P, b, h, i, jq);
    uint8_t *row = mask + (((size_t)b * P.nh + h) * P.L + i) * P.L;
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (4 * jq + r < P.L) row[4 * jq + r] = word_of(w, r) >= P.thr ? 1 : 0;
}

// ---------------------------------------------------------------- weight norm (one wave per output row)
// The row routines: lane c takes columns c, c + 64, ... in order, then the butterfly of wave_sum.  The per-layer kernels
// and the table-driven ones both run exactly these, so a row has one set of bits whichever launch formed it.
__device__ __forceinline__ void wn_row_fwd(const float *vr, const float *g, float *wr, int cols, int lane) {
    float ss = 0.f;
    for (int c = lane; c < cols; c += 64) ss += vr[c] * vr[c];
    ss = vq2::wave_sum(ss);
    const float f = g[0] / sqrtf(ss);
    for (int c = lane; c < cols; c += 64) wr[c] = vr[c] * f;
}

__device__ __forceinline__ void wn_row_bwd(const float *wr, const float *vr, const float *g, float *dvr, float *dg, int cols,
                                           int lane) {
    float ss = 0.f, dot = 0.f;
    for (int c = lane; c < cols; c += 64) { ss += vr[c] * vr[c]; dot += wr[c] * vr[c]; }
    ss = vq2::wave_sum(ss);
    dot = vq2::wave_sum(dot);
    const float n = sqrtf(ss);
    const float f = g[0] / n, e = dot / ss;   // dv = (g / n) * (dw - v * (dw . v) / n^2)
    for (int c = lane; c < cols; c += 64) dvr[c] = f * (wr[c] - vr[c] * e);
    if (lane == 0) dg[0] = dot / n;
}

__global__ __launch_bounds__(64) void weight_norm_fwd_kernel(const float *__restrict__ v, const float *__restrict__ g,
                                                             float *__restrict__ w, int cols) {
    const int row = blockIdx.x;
    wn_row_fwd(v + (size_t)row * cols, g + row, w + (size_t)row * cols, cols, threadIdx.x);
}

__global__ __launch_bounds__(64) void weight_norm_bwd_kernel(const float *__restrict__ dw, const float *__restrict__ v,
                                                             const float *__restrict__ g, float *__restrict__ dv,
                                                             float *__restrict__ dg, int cols) {
    const int row = blockIdx.x;
    wn_row_bwd(dw + (size_t)row * cols, v + (size_t)row * cols, g + row, dv + (size_t)row * cols, dg + row, cols, threadIdx.x);
}

// Table-driven forms: every weight-normed tensor of a model in one launch.  A workgroup is four waves, a wave takes one row
// at a time; the rows [tab[first].row_start, tab[last].row_start) are dealt to the waves of a fixed grid, and each wave finds
// the entry of its row by bisection over row_start (a handful of cached loads against one read of the row itself).
constexpr int WN_WAVES = 4;
constexpr int WN_GRID = 2048;      // 256 CUs x 8 workgroups: enough rows in flight for a kernel bound by one read of v

__device__ __forceinline__ int wn_find(const vq2_wn_entry *tab, int first, int last, int r) {
    int lo = first, hi = last - 1;            // the largest index whose row_start is <= r
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].row_start <= r) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(64 * WN_WAVES) void wn_table_fwd_kernel(const vq2_wn_entry *tab, int first, int last,
                                                                     float *params, float *w) {
    const int lane = threadIdx.x & 63;
    const int r1 = tab[last].row_start;
    for (int r = tab[first].row_start + blockIdx.x * WN_WAVES + (threadIdx.x >> 6); r < r1; r += gridDim.x * WN_WAVES) {
        const vq2_wn_entry e = tab[wn_find(tab, first, last, r)];
        const int row = r - e.row_start;
        float *vr = params + e.v_off + (int64_t)row * e.cols;
        if (e.mask_from < e.kw) {
            // the 'causal' edit of the parameter itself: last kernel row, columns from mask_from on.  The lane that zeroes
            // column c is the lane that reads it below
            for (int c = lane; c < e.cols; c += 64)
                if ((c / e.kw) % e.kh == e.kh - 1 && c % e.kw >= e.mask_from) vr[c] = 0.f;
        }
        wn_row_fwd(vr, params + e.g_off + row, w + e.w_off + (int64_t)row * e.cols, e.cols, lane);
    }
}

__global__ __launch_bounds__(64 * WN_WAVES) void wn_table_bwd_kernel(const vq2_wn_entry *tab, int first, int last,
                                                                     const float *params, const float *dw, float *grads) {
    const int lane = threadIdx.x & 63;
    const int r1 = tab[last].row_start;
    for (int r = tab[first].row_start + blockIdx.x * WN_WAVES + (threadIdx.x >> 6); r < r1; r += gridDim.x * WN_WAVES) {
        const vq2_wn_entry e = tab[wn_find(tab, first, last, r)];
        const int row = r - e.row_start;
        const int64_t o = (int64_t)row * e.cols;
        wn_row_bwd(dw + e.w_off + o, params + e.v_off + o, params + e.g_off + row, grads + e.v_off + o, grads + e.g_off + row,
                   e.cols, lane);
    }
}

}  // namespace

extern "C" int vq2_causal_attn_fwd(const vq2_attn_desc *d, const float *q, const float *k, const float *v, float *o, float *lse,
                                   vq2_stream_t stream) {
    AttnParams P;
    if (int e = fill_params(d, P, "causal_attn_fwd")) return e;
    VQ2_REQUIRE(q && k && v && o && lse, "causal_attn_fwd: null pointer");
    VQ2_REQUIRE(vq2::aligned16(q) && vq2::aligned16(k) && vq2::aligned16(v) && vq2::aligned16(o),
                "causal_attn_fwd: pointers must be 16-byte aligned");
    const dim3 grid((P.L + AT_BQ - 1) / AT_BQ, P.nh, P.B);
    ATTN_BY_DT(P.dh, hipLaunchKernelGGL((attn_fwd_kernel<DT>), grid, dim3(256), 0, vq2::to_stream(stream), P, q, k, v, o, lse));
    return vq2::check_launch("attn_fwd_kernel");
}

extern "C" int vq2_causal_attn_fwd_rows(const vq2_attn_desc *d, int32_t q0, int32_t nq, int32_t W, int64_t kv_image_stride,
                                        int64_t kv_row_stride, const float *q, const float *k, const float *v, float *o,
                                        vq2_stream_t stream) {
    AttnParams P;
    if (int e = fill_params(d, P, "causal_attn_fwd_rows")) return e;
    VQ2_REQUIRE(!P.dropout, "causal_attn_fwd_rows: p_drop must be 0");
    VQ2_REQUIRE(q && k && v && o, "causal_attn_fwd_rows: null pointer");
    VQ2_REQUIRE(vq2::aligned16(q) && vq2::aligned16(k) && vq2::aligned16(v) && vq2::aligned16(o),
                "causal_attn_fwd_rows: pointers must be 16-byte aligned");
    VQ2_REQUIRE(q0 >= 0 && nq >= 1 && W >= 1 && (int64_t)q0 + nq <= (int64_t)d->L,
                "causal_attn_fwd_rows: the window q0=%d, nq=%d must lie inside the L=%d positions", q0, nq, d->L);
    VQ2_REQUIRE(kv_image_stride % 4 == 0 && kv_row_stride % 4 == 0 && kv_image_stride >= 0 && kv_row_stride >= 0,
                "causal_attn_fwd_rows: key / value strides must be non-negative multiples of 4");
    const AttnRows R{q0, nq, W, (long long)kv_image_stride, (long long)kv_row_stride};
    const dim3 grid((nq + AT_BQ - 1) / AT_BQ, P.nh, P.B);
    ATTN_BY_DT(P.dh, hipLaunchKernelGGL((attn_fwd_rows_kernel<DT>), grid, dim3(256), 0, vq2::to_stream(stream), P, R, q, k, v, o));
    return vq2::check_launch("attn_fwd_rows_kernel");
}

extern "C" int vq2_causal_attn_bwd(const vq2_attn_desc *d, const float *q, const float *k, const float *v,
                                   const float *lse, const float *dO, int32_t lddo, float *dq, int32_t lddq, float *dk,
                                   int32_t lddk, float *dv, int32_t lddv, float *delta_ws, vq2_stream_t stream) {
    AttnParams P;
    if (int e = fill_params(d, P, "causal_attn_bwd")) return e;
    VQ2_REQUIRE(q && k && v && lse && dO && dq && dk && dv && delta_ws, "causal_attn_bwd: null pointer");
    VQ2_REQUIRE(vq2::aligned16(q) && vq2::aligned16(k) && vq2::aligned16(v) && vq2::aligned16(dO) &&
                    vq2::aligned16(dq) && vq2::aligned16(dk) && vq2::aligned16(dv),
                "causal_attn_bwd: pointers must be 16-byte aligned");
    const int ch = P.nh * P.dh;
    VQ2_REQUIRE(lddo >= ch && lddq >= ch && lddk >= ch && lddv >= ch && lddo % 4 == 0 && lddq % 4 == 0 && lddk % 4 == 0 && lddv % 4 == 0,
                "causal_attn_bwd: gradient pixel strides must be multiples of 4, at least n_head * dim_head");
    hipStream_t s = vq2::to_stream(stream);
    const dim3 grid((P.L + AT_BQ - 1) / AT_BQ, P.nh, P.B);
    ATTN_BY_DT(P.dh, hipLaunchKernelGGL((attn_delta_kernel<DT>), grid, dim3(256), 0, s, P, q, k, v, dO, lddo, lse, delta_ws));
    if (int e = vq2::check_launch("attn_delta_kernel")) return e;
    ATTN_BY_DT(P.dh, hipLaunchKernelGGL((attn_dkv_kernel<DT>), grid, dim3(256), 0, s, P, q, k, v, dO, lddo, lse, delta_ws, dk, lddk, dv, lddv));
    if (int e = vq2::check_launch("attn_dkv_kernel")) return e;
    ATTN_BY_DT(P.dh, hipLaunchKernelGGL((attn_dq_kernel<DT>), grid, dim3(256), 0, s, P, q, k, v, dO, lddo, lse, delta_ws, dq, lddq));
    return vq2::check_launch("attn_dq_kernel");
}

extern "C" int vq2_causal_attn_keep_mask(const vq2_attn_desc *d, uint8_t *mask, vq2_stream_t stream) {
    AttnParams P;
    if (int e = fill_params(d, P, "causal_attn_keep_mask")) return e;
    VQ2_REQUIRE(mask, "causal_attn_keep_mask: null pointer");
    const double total = (double)P.B * P.nh * P.L * ((P.L + 3) / 4);
    VQ2_REQUIRE(total < 2147483648.0 * 256.0, "causal_attn_keep_mask: mask too large");
    hipLaunchKernelGGL(attn_keep_mask_kernel, dim3((unsigned)(((size_t)total + 255) / 256)), dim3(256), 0, vq2::to_stream(stream), P, mask);
    return vq2::check_launch("attn_keep_mask_kernel");
}

extern "C" int vq2_weight_norm_fwd(const float *v, const float *g, float *w, int32_t rows, int32_t cols, vq2_stream_t stream) {
    VQ2_REQUIRE(v && g && w, "weight_norm_fwd: null pointer");
    VQ2_REQUIRE(rows >= 1 && cols >= 1, "weight_norm_fwd: non-positive size");
    hipLaunchKernelGGL(weight_norm_fwd_kernel, dim3(rows), dim3(64), 0, vq2::to_stream(stream), v, g, w, cols);
    return vq2::check_launch("weight_norm_fwd_kernel");
}

extern "C" int vq2_weight_norm_bwd(const float *dw, const float *v, const float *g, float *dv, float *dg, int32_t rows,
                                   int32_t cols, vq2_stream_t stream) {
    VQ2_REQUIRE(dw && v && g && dv && dg, "weight_norm_bwd: null pointer");
    VQ2_REQUIRE(rows >= 1 && cols >= 1, "weight_norm_bwd: non-positive size");
    hipLaunchKernelGGL(weight_norm_bwd_kernel, dim3(rows), dim3(64), 0, vq2::to_stream(stream), dw, v, g, dv, dg, cols);
    return vq2::check_launch("weight_norm_bwd_kernel");
}

extern "C" int vq2_wn_table_fwd(const vq2_wn_entry *table, int32_t n_entries, float *params, float *w, vq2_stream_t stream) {
    VQ2_REQUIRE(table && params && w, "wn_table_fwd: null pointer");
    VQ2_REQUIRE(n_entries >= 1, "wn_table_fwd: the table needs at least one entry");
    VQ2_REQUIRE(vq2::aligned16(table), "wn_table_fwd: the table must be 16-byte aligned");
    hipLaunchKernelGGL(wn_table_fwd_kernel, dim3(WN_GRID), dim3(64 * WN_WAVES), 0, vq2::to_stream(stream), table, 0, n_entries,
                       params, w);
    return vq2::check_launch("wn_table_fwd_kernel");
}

extern "C" int vq2_wn_table_bwd(const vq2_wn_entry *table, int32_t first, int32_t last, const float *params, const float *dw,
                                float *grads, vq2_stream_t stream) {
    VQ2_REQUIRE(table && params && dw && grads, "wn_table_bwd: null pointer");
    VQ2_REQUIRE(first >= 0 && first <= last, "wn_table_bwd: the entry range [%d, %d) is not a range", first, last);
    VQ2_REQUIRE(vq2::aligned16(table), "wn_table_bwd: the table must be 16-byte aligned");
    if (first == last) return VQ2_OK;
    hipLaunchKernelGGL(wn_table_bwd_kernel, dim3(WN_GRID), dim3(64 * WN_WAVES), 0, vq2::to_stream(stream), table, first, last,
                       params, dw, grads);
    return vq2::check_launch("wn_table_bwd_kernel");
}
