// Weight gradient of conv2d / conv-transpose2d (NHWC activations, reference-layout output).
//
//   dw[o][i][kh][kw] = sum_{n,ho,wo} G[n,ho,wo,o] * X[n, ho*s+kh-p, wo*s+kw-p, i]
//
//   conv  : X = (relu) input x,  G = dy                  -> dw in OIHW  (o = Co, i = Ci)
//   convT : X = dy (the 2H x 2W tensor), G = (relu) x    -> dw in IOHW  (o = Ci, i = Co)
//
// This is a GEMM [O x M] * [M x K] (K = KH*KW*I) whose reduction dimension M = N*Ho*Wo is
// huge and whose output is tiny, so the reduction is split over `S` workgroups per output
// tile; every split writes its partial tile to a slab in the caller's workspace and a second
// launch sums the slabs in a fixed order (bit-reproducible, no float atomics) and scatters
// into the reference weight layout.  Both operands are consumed "reduction-major" straight
// from NHWC memory: v_mfma_f32_32x32x2_f32 wants A[i][k] / B[k][j] with lanes along i / j,
// and consecutive lanes read consecutive channels -> conflict-free ds_read_b32, no transposes.
#include "vq2_conv.h"

namespace vq2 {

struct WgradParams {
    const float *x;  // image operand [N,H,W,ldx], I channels
    const float *g;  // grad  operand [N,Ho,Wo,ldg], O channels
    float *ws;       // [S][O][K] partial slabs
    float *bias_ws;  // [S][O] partial column sums of g (bias gradient) or null
    int bias_taps;   // bias gradient from the GATHERED operand (it is dy: exchanged roles, conv-transpose): bit t set =
                     // tap t visits every dy pixel exactly once over the taps of this mask; the column sums of those
                     // k-blocks of the staged X tile are the bias gradient.  0 = bias from the G tile (plain conv)
    int bias_nslots; // popcount(bias_taps): bias_ws is [S][nslots][I]
    int N, H, W, I, ldx;
    int Ho, Wo, O, ldg;
    int KH, KW, stride, pad_h, pad_w;
    int K, M;
    int rows_per_split;  // multiple of 32
    int relu_x, relu_g;
};

constexpr int WG_BKR = 32;  // reduction rows (pixels) per staged chunk

// rows staged per pass by the 256 threads when a row has c4 float4: the largest power of two <= 256 / c4
// (a 96-wide tile has 24 float4 per row -> 8 rows per pass, 64 threads sit the X staging out)
constexpr int rows_per_pass(int c4) {
    int r = 32;
    while (r * c4 > 256) r >>= 1;
    return r;
}

template <int WAVES_M, int WAVES_N, int MT, int NT>
__global__ __launch_bounds__(256) void wgrad_kernel(const WgradParams P) {
    constexpr int BMO = WAVES_M * MT * 32;  // tile rows  (o)
    constexpr int BNK = WAVES_N * NT * 32;  // tile cols  (k)
    constexpr int G_C4 = BMO / 4, X_C4 = BNK / 4;
    constexpr int G_RSTEP = rows_per_pass(G_C4), X_RSTEP = rows_per_pass(X_C4);
    constexpr int G_LD = WG_BKR / G_RSTEP, X_LD = WG_BKR / X_RSTEP;
    static_assert(G_C4 * G_RSTEP == 256, "every thread stages G");
    static_assert(WAVES_M * WAVES_N == 4, "4 waves");
    static_assert(G_C4 <= 256 && X_C4 <= 256 && G_LD >= 1 && X_LD >= 1, "tile/thread mapping");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *Gs = smem;                       // [2][32][BMO]
    float *Xs = smem + 2 * WG_BKR * BMO;    // [2][32][BNK]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    // 1-D grid, XCD-aware: the k-tiles and o-tiles of one split share its G/X pixels -> same L2
    const int ktiles = (P.K + BNK - 1) / BNK;
    const int otiles = (P.O + BMO - 1) / BMO;
    const int vid = xcd_remap(blockIdx.x, gridDim.x);
    const int k0 = (vid % ktiles) * BNK;
    const int o0 = ((vid / ktiles) % otiles) * BMO;
    const int split = vid / (ktiles * otiles);
    const int m_begin = split * P.rows_per_split;
    const int m_end = min(P.M, m_begin + P.rows_per_split);

    // fixed per-thread column coordinates
    const int g_c = o0 + (tid % G_C4) * 4;
    const int g_r = tid / G_C4;
    const int x_k = k0 + (tid % X_C4) * 4;
    const int x_r = tid / X_C4;
    const bool g_cv = g_c < P.O;
    const bool x_act = tid < X_C4 * X_RSTEP;       // threads beyond the last full staging row sit X out
    const bool x_kv = x_act && x_k < P.K;
    int kh = 0, kw = 0, ci = 0;
    if (x_kv) {
        const int tap = x_k / P.I;
        ci = x_k - tap * P.I;
        kh = tap / P.KW;
        kw = tap - kh * P.KW;
    }
    const int HoWo = P.Ho * P.Wo;

    // (n, ho, wo) of this thread's X rows, advanced by 32 rows per chunk without divisions
    int xn[X_LD], xho[X_LD], xwo[X_LD];
#pragma unroll
    for (int j = 0; j < X_LD; ++j) {
        const int m = m_begin + x_r + j * X_RSTEP;
        xn[j] = m / HoWo;
        const int r = m - xn[j] * HoWo;
        xho[j] = r / P.Wo;
        xwo[j] = r - xho[j] * P.Wo;
    }
    float4 rg[G_LD], rx[X_LD];
    auto load_chunk = [&](int mbase) {
#pragma unroll
        for (int j = 0; j < G_LD; ++j) {
            const int m = mbase + g_r + j * G_RSTEP;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (g_cv && m < m_end) v = *reinterpret_cast<const float4 *>(P.g + (size_t)m * P.ldg + g_c);
            rg[j] = v;
        }
#pragma unroll
        for (int j = 0; j < X_LD; ++j) {
            const int m = mbase + x_r + j * X_RSTEP;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (x_kv && m < m_end) {
                const int ih = xho[j] * P.stride - P.pad_h + kh;
                const int iw = xwo[j] * P.stride - P.pad_w + kw;
                if ((unsigned)ih < (unsigned)P.H && (unsigned)iw < (unsigned)P.W)
                    v = *reinterpret_cast<const float4 *>(P.x + ((size_t)(xn[j] * P.H + ih) * P.W + iw) * P.ldx + ci);
            }
            rx[j] = v;  // ReLU applied at the LDS write, so the load is not waited for here
            // next chunk: 32 rows further in (n, ho, wo) order
            xwo[j] += WG_BKR;
            while (xwo[j] >= P.Wo) {
                xwo[j] -= P.Wo;
                if (++xho[j] == P.Ho) { xho[j] = 0; ++xn[j]; }
            }
        }
    };
    auto store_chunk = [&](int buf) {
        float *gs = Gs + buf * WG_BKR * BMO;
        float *xs = Xs + buf * WG_BKR * BNK;
#pragma unroll
        for (int j = 0; j < G_LD; ++j)
            *reinterpret_cast<float4 *>(gs + (g_r + j * G_RSTEP) * BMO + (tid % G_C4) * 4) = P.relu_g ? relu4(rg[j]) : rg[j];
#pragma unroll
        for (int j = 0; j < X_LD; ++j)
            if (X_C4 * X_RSTEP == 256 || x_act)
                *reinterpret_cast<float4 *>(xs + (x_r + j * X_RSTEP) * BNK + (tid % X_C4) * 4) = P.relu_x ? relu4(rx[j]) : rx[j];
    };

    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nchunks = (m_end - m_begin + WG_BKR - 1) / WG_BKR;
    if (nchunks > 0) {
        load_chunk(m_begin);
        store_chunk(0);
    }
    __syncthreads();
    const int fr = lane & 31, fk = lane >> 5;
    const bool do_bias = P.bias_ws != nullptr && !P.bias_taps && k0 == 0 && tid < BMO;
    int bx_col = -1;   // this thread's slot in a bias_ws row when its k column belongs to a bias tap
    if (P.bias_ws != nullptr && P.bias_taps && o0 == 0 && tid < BNK && k0 + tid < P.K) {
        const int tap = (k0 + tid) / P.I;
        if ((P.bias_taps >> tap) & 1) bx_col = __popc(P.bias_taps & ((1u << tap) - 1u)) * P.I + (k0 + tid - tap * P.I);
    }
    const bool do_bias_x = bx_col >= 0;
    float bsum = 0.f;
    for (int c = 0; c < nchunks; ++c) {
        const int buf = c & 1;
        if (c + 1 < nchunks) load_chunk(m_begin + (c + 1) * WG_BKR);
        if (do_bias) {  // bias gradient rides along: column sums of the staged grad tile
            const float *gcol = Gs + buf * WG_BKR * BMO + tid;
            float s0 = 0.f, s1 = 0.f;
#pragma unroll
            for (int r = 0; r < WG_BKR; r += 2) { s0 += gcol[r * BMO]; s1 += gcol[(r + 1) * BMO]; }
            bsum += s0 + s1;
        }
        if (do_bias_x) {
            const float *xcol = Xs + buf * WG_BKR * BNK + tid;
            float s0 = 0.f, s1 = 0.f;
#pragma unroll
            for (int r = 0; r < WG_BKR; r += 2) { s0 += xcol[r * BNK]; s1 += xcol[(r + 1) * BNK]; }
            bsum += s0 + s1;
        }
        // a wave's 32-wide blocks are INTERLEAVED with the other waves' (block i of wave wm = i*WAVES_M + wm): the two
        // fragments of a k-step are then 256 bytes apart and k-steps 1 KiB apart -- one ds_read2st64_b32 with immediate
        // offsets per operand and step, no vector add to rebuild a base (vector instructions cost matrix time)
        const float *gs = Gs + buf * WG_BKR * BMO + fk * BMO + wm * 32 + fr;
        const float *xs = Xs + buf * WG_BKR * BNK + fk * BNK + wn * 32 + fr;
        // fragments double-buffered: the ds_reads of k-step kk+1 are in flight during the MFMAs of step kk
        float fa[2][MT], fb[2][NT];
#pragma unroll
        for (int i = 0; i < MT; ++i) fa[0][i] = gs[i * WAVES_M * 32];
#pragma unroll
        for (int j = 0; j < NT; ++j) fb[0][j] = xs[j * WAVES_N * 32];
#pragma unroll
        for (int kk = 0; kk < WG_BKR / 2; ++kk) {
            const int cur = kk & 1, nxt = cur ^ 1;
            if (kk + 1 < WG_BKR / 2) {
#pragma unroll
                for (int i = 0; i < MT; ++i) fa[nxt][i] = gs[(kk + 1) * 2 * BMO + i * WAVES_M * 32];
#pragma unroll
                for (int j = 0; j < NT; ++j) fb[nxt][j] = xs[(kk + 1) * 2 * BNK + j * WAVES_N * 32];
            }
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[cur][i], fb[cur][j], acc[i][j], 0, 0, 0);
            // pin the order: next step's LDS reads first, then this step's MFMAs (hipcc otherwise sinks the
            // reads to just before their use and waits lgkmcnt(0) in front of every MFMA group)
            __builtin_amdgcn_sched_group_barrier(0x100, MT + NT, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, MT * NT, 0);
        }
        if (c + 1 < nchunks) store_chunk(buf ^ 1);
        __syncthreads();
    }

    if (do_bias && o0 + tid < P.O) P.bias_ws[(size_t)split * P.O + o0 + tid] = bsum;
    if (do_bias_x) P.bias_ws[(size_t)split * P.bias_nslots * P.I + bx_col] = bsum;

    // partial tile -> slab [split][o][k]
    float *slab = P.ws + (size_t)split * P.O * P.K;
    const int colq = lane & 31, rowq = 4 * (lane >> 5);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int k = k0 + (j * WAVES_N + wn) * 32 + colq;
        if (k >= P.K) continue;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int ob = o0 + (i * WAVES_M + wm) * 32 + rowq;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = ob + (r & 3) + 8 * (r >> 2);
                if (o < P.O) slab[(size_t)o * P.K + k] = acc[i][j][r];
            }
        }
    }
}

// ====================================================================== low-VALU variant
// Same math as wgrad_kernel for the common case Wo % 32 == 0: a 32-row chunk then lies inside ONE output
// row, so (n, ho, wo0) of the chunk is wave-uniform and tracked on the scalar unit; every gather offset
// is "uniform chunk base + per-thread constant" -- one vector add per load, fetched with raw buffer loads
// whose range check supplies the zeros (no exec branches, no 64-bit address math).  With two waves per
// SIMD the partner's fp32 MFMAs starve the vector ALU, so the address work is what was limiting.
// (u32x4, OOB, RSRC_FLAGS, as_f4: vq2_conv.h)
// WINO (3x3 stride-1 pad-1, 128 x 128 tiles, I % 128 == 0, Wo % 64 == 0): the same sum as F(2,3) Winograd along the image
// rows (csrc/vq2_wino.hip has the forward form).  The reduction runs over column PAIRS (P.M, P.rows_per_split, P.Wo are
// in pairs... P.Wo stays in pixels), the K axis is (kernel row kh, Winograd index v, channel): for pair t of a row with
// input columns d0..d3 = 2t-1 .. 2t+2 and gradients g0, g1 of its two pixels
//     S_v[kh] += E_v^T V_v,   E = (g0, g0 + g1, g0 - g1, g1),   V = (d0 - d2, d1 + d2, d2 - d1, d3 - d1)
// and the reduction kernels finish with  dw[kh][0] = S0 + (S1 + S2)/2, dw[kh][1] = (S1 - S2)/2, dw[kh][2] = (S1 + S2)/2 + S3:
// 12 products per pair instead of 18 -- 2/3 of the matrix instructions.  A workgroup owns ONE (kh, v, 128-channel block):
// v is workgroup-uniform, so the transform is one fused multiply-add by +-1 per staged element (exact).
// WINO == 2 (4x4 stride-2 pad-1 conv and conv-transpose, I == 64 or I % 128 == 0): the four taps of a kernel row split by
// column parity into two 2-tap filters (csrc/vq2_wino.hip, wino_k4s2_kernel), each as F(2,2) over output column pairs:
//     S1 += g0^T (d0 - d1),  S2 += (g0 + g1)^T d1,  S3 += g1^T (d1 - d2);   dw[first tap] = S1 + S2, dw[second] = S2 - S3
// with d0..d2 = input columns 4t+pc, 4t+pc+2, 4t+pc+4 (pc = -1: taps 0, 2; pc = 0: taps 1, 3): 3/4 of the matrix
// instructions.  K axis = (v, parity, kh, channel), kh fastest: a 128-wide tile holds two kernel rows of ONE (v, parity).
// WINO == 3 (the exchanged-roles form of a 3x3 conv with 32 output channels -- the ResBlock 3x3 -- on 128 x 96 tiles): the
// STREAMED operand is x and carries V_v (two pixels of the row, with column checks), the gathered operand is dy and carries
// E_v at the three row shifts 1 - kh: S_v[kh] += V_v[r]^T E_v[r - kh + 1].  K axis = (v, kh, co); a tile is one v.
template <int WAVES_M, int WAVES_N, int MT, int NT, bool RELU_X, bool RELU_G, int WINO = 0>
__global__ __launch_bounds__(256) void wgrad_fast_kernel(const WgradParams P) {
    constexpr int BMO = WAVES_M * MT * 32;
    constexpr int BNK = WAVES_N * NT * 32;
    constexpr int G_C4 = BMO / 4, X_C4 = BNK / 4;
    constexpr int G_RSTEP = rows_per_pass(G_C4), X_RSTEP = rows_per_pass(X_C4);
    constexpr int G_LD = WG_BKR / G_RSTEP, X_LD = WG_BKR / X_RSTEP;
    static_assert(G_C4 * G_RSTEP == 256, "every thread stages G");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *Gs = smem;
    float *Xs = smem + 2 * WG_BKR * BMO;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int ktiles = (P.K + BNK - 1) / BNK;
    const int otiles = (P.O + BMO - 1) / BMO;
    const int vid = xcd_remap(blockIdx.x, gridDim.x);
    const int k0 = (vid % ktiles) * BNK;
    const int o0 = ((vid / ktiles) % otiles) * BMO;
    const int split = vid / (ktiles * otiles);
    const int m_begin = split * P.rows_per_split;
    const int m_end = min(P.M, m_begin + P.rows_per_split);

    const __amdgpu_buffer_rsrc_t rg =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(P.g), 0, (WINO ? 2 : 1) * P.M * P.ldg * 4, RSRC_FLAGS);
    const __amdgpu_buffer_rsrc_t rx =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(P.x), 0, P.N * P.H * P.W * P.ldx * 4, RSRC_FLAGS);

    // per-thread constants
    const int g_c = o0 + (tid % G_C4) * 4;
    const int g_r = tid / G_C4;
    const int x_k = k0 + (tid % X_C4) * 4;
    const int x_r = tid / X_C4;
    const bool g_cv = g_c < P.O;
    const bool x_act = tid < X_C4 * X_RSTEP;       // threads beyond the last full staging row sit X out
    const bool x_kv = x_act && x_k < P.K;
    int kh = 0, kw = 0, ci = 0;
    if (x_kv) {
        const int tap = x_k / P.I;
        ci = x_k - tap * P.I;
        kh = tap / P.KW;
        kw = tap - kh * P.KW;
    }
    // WINO: the K tile is one (kh, v) of all threads (I % BNK == 0); column offsets of the two input pixels of V_v and of
    // the gradient pixel(s) of E_v, relative to the pair's first pixel
    int nu = 0, xo_a = 0, xo_b = 0, go_a = 0;
    bool g_two = false;
    float sv = -1.f, sg = 1.f;
    bool x_two = true, bias2 = false, bias2u = false;                                  // WINO == 2: V of the middle product is one pixel
    int par = 0;
    if constexpr (WINO == 1) {
        const int vt = k0 / P.I;
        kh = vt >> 2; nu = vt & 3; kw = 0;
        ci = x_k - vt * P.I;
        xo_a = (nu == 0) ? -1 : (nu == 1) ? 0 : (nu == 2) ? 1 : 2;     // V = x[a] + sv * x[b]
        xo_b = (nu == 0) ? 1 : (nu == 1) ? 1 : 0;
        sv = (nu == 1) ? 1.f : -1.f;
        go_a = (nu == 3) ? 1 : 0;                                       // E = g[a] (+ sg * g[1])
        g_two = (nu == 1 || nu == 2);
        sg = (nu == 2) ? -1.f : 1.f;
    }
    if constexpr (WINO == 2) {
        const int vt = x_k / P.I;                                       // per thread: the tile may hold two kernel rows
        const int vt0 = k0 / P.I;
        kh = vt & 3; par = (vt0 >> 2) & 1; nu = vt0 >> 3; kw = 0;       // nu, par: workgroup-uniform
        ci = x_k - vt * P.I;
        const int pc = par ? 0 : -1;
        xo_a = (nu == 0) ? pc : pc + 2;
        xo_b = (nu == 0) ? pc + 2 : pc + 4;
        x_two = nu != 1;
        sv = -1.f;
        go_a = (nu == 2) ? 1 : 0;
        g_two = nu == 1;
        sg = 1.f;
        // conv-transpose: the bias gradient is the column sum of the GATHERED operand (dy).  The middle-product tiles read
        // d1 = columns 4t+1 (odd parity) / 4t+2 (even) of rows 2ho (kh 1) / 2ho+1 (kh 2); with the spare second load on
        // columns 4t+3 / 4t they visit every dy pixel exactly once.
        bias2u = P.bias_ws != nullptr && P.bias_taps != 0 && nu == 1 && o0 == 0;   // workgroup-uniform: every thread of
        bias2 = bias2u && (kh == 1 || kh == 2) && x_kv;                            // such a tile loads and adds, two kernel
        if (nu == 1) xo_b = par ? 0 : 3;                                           // rows' threads keep their sums
    }
    int go_b = 1;                                                      // WINO == 3: second pixel of V on the streamed side
    if constexpr (WINO == 3) {
        nu = k0 / BNK;                                                  // workgroup-uniform (one v per 96-wide tile)
        const int kl = x_k - k0;
        kh = kl / P.I; kw = 0; ci = kl - kh * P.I;                      // kh: per thread (three kernel rows per tile)
        go_a = (nu == 0) ? -1 : (nu == 1) ? 0 : (nu == 2) ? 1 : 2;     // V = x[a] + sg * x[b]
        go_b = (nu == 0) ? 1 : (nu == 1) ? 1 : 0;
        g_two = true;
        sg = (nu == 1) ? 1.f : -1.f;
        xo_a = (nu == 3) ? 1 : 0;                                       // E = dy[a] (+ sv * dy[1])
        xo_b = 1;
        x_two = (nu == 1 || nu == 2);
        sv = (nu == 2) ? -1.f : 1.f;
    }
    // WINO on rows of 32 pixels (16 pairs): a 32-pair chunk is TWO image rows.  Staging rows 0..15 are the first, 16..31 the
    // second (G_RSTEP = X_RSTEP = 8, so load j belongs to row j >> 1: a compile-time property of the load).
    const bool two_row = WINO != 0 && P.Wo == 32;
    int g_const[G_LD], x_const[X_LD], x_iw[X_LD];
#pragma unroll
    for (int j = 0; j < G_LD; ++j) {
        const int rj = g_r + j * G_RSTEP, r2 = two_row ? rj >> 4 : 0, tj = rj - 16 * r2;
        g_const[j] = (WINO ? (r2 * P.Wo + 2 * tj) * P.ldg + g_c : rj * P.ldg + g_c) * 4;
    }
#pragma unroll
    for (int j = 0; j < X_LD; ++j) {
        const int rj = x_r + j * X_RSTEP;                    // row inside the 32-row chunk
        if constexpr (WINO) {
            constexpr int CS = WINO == 2 ? 4 : 2;            // input columns per pair
            constexpr int RS = WINO == 2 ? 2 : 1;            // input rows per row of the G grid
            const int r2 = two_row ? rj >> 4 : 0, tj = rj - 16 * r2;
            x_iw[j] = CS * tj;                               // + CS * pair0 + xo = input column
            x_const[j] = (((WINO == 3 ? -kh : kh) + RS * r2) * P.W + CS * tj) * P.ldx * 4 + ci * 4;
        } else {
        x_iw[j] = rj * P.stride - P.pad_w + kw;               // + wo0*stride = input column
        x_const[j] = ((kh * P.W + kw + rj * P.stride) * P.ldx + ci) * 4;
        }
    }
    // wave-uniform chunk position (scalar registers)
    int un, uho, uwo;
    const int row_len = WINO ? P.Wo / 2 : P.Wo;              // reduction positions per image row (WINO: column pairs)
    {
        const int HoWo = P.Ho * row_len;
        un = m_begin / HoWo;
        const int r = m_begin - un * HoWo;
        uho = r / row_len;
        uwo = r - uho * row_len;
    }

    u32x4 rgv[G_LD], rxv[X_LD];
    u32x4 rgw[WINO ? G_LD : 1], rxw[WINO ? X_LD : 1];       // WINO: the second pixel of every staged element
    float4 bsum4 = make_float4(0.f, 0.f, 0.f, 0.f);          // WINO == 2, conv-transpose: bias partial of this thread's 4 channels
    auto load_chunk_wino = [&](int mbase) {
        const int rows_left = m_end - mbase;                  // uniform (pairs)
        const int gbase = ((un * P.Ho + uho) * P.Wo + 2 * uwo + go_a) * P.ldg * 4;   // uniform
#pragma unroll
        for (int j = 0; j < G_LD; ++j) {
            const bool v = g_cv && (g_r + j * G_RSTEP) < rows_left;
            if constexpr (WINO == 3) {                         // (gbase carries go_a; the second pixel is go_b - go_a further)
                const int col = 2 * (uwo + ((g_r + j * G_RSTEP) & (two_row ? 15 : 31)));
                const bool va = v && (unsigned)(col + go_a) < (unsigned)P.Wo;
                const bool vb = v && (unsigned)(col + go_b) < (unsigned)P.Wo;
                rgv[j] = __builtin_amdgcn_raw_buffer_load_b128(rg, va ? gbase + g_const[j] : OOB, 0, 0);
                rgw[j] = __builtin_amdgcn_raw_buffer_load_b128(rg, vb ? gbase + g_const[j] + (go_b - go_a) * P.ldg * 4 : OOB, 0, 0);
            } else {
            rgv[j] = __builtin_amdgcn_raw_buffer_load_b128(rg, v ? gbase + g_const[j] : OOB, 0, 0);
            rgw[j] = __builtin_amdgcn_raw_buffer_load_b128(rg, (v && g_two) ? gbase + g_const[j] + P.ldg * 4 : OOB, 0, 0);
            }
        }
        constexpr int CS = WINO == 2 ? 4 : 2;
        const int ihu = WINO == 3 ? uho + 1 : (WINO == 2 ? 2 * uho : uho) - 1;   // pad 1 (WINO 3: row shift 1 - kh)
        const int xbase = ((un * P.H + ihu) * P.W + CS * uwo) * P.ldx * 4;            // uniform
        constexpr int RS = WINO == 2 ? 2 : 1;
        const int ihk = ihu + (WINO == 3 ? -kh : kh);
        const bool hv0 = x_kv && (unsigned)ihk < (unsigned)P.H;                       // first row of the chunk
        const bool hv1 = two_row ? x_kv && (unsigned)(ihk + RS) < (unsigned)P.H : hv0;  // second row (two-row chunks)
        const int iwu = CS * uwo;
        const int xa = xo_a * P.ldx * 4, xb = xo_b * P.ldx * 4;
        const bool want_b = x_two || bias2u;
#pragma unroll
        for (int j = 0; j < X_LD; ++j) {
            const bool v = ((x_r + j * X_RSTEP) >= 16 ? hv1 : hv0) && (x_r + j * X_RSTEP) < rows_left;
            const bool va = v && (unsigned)(iwu + x_iw[j] + xo_a) < (unsigned)P.W;
            const bool vb = v && want_b && (unsigned)(iwu + x_iw[j] + xo_b) < (unsigned)P.W;
            rxv[j] = __builtin_amdgcn_raw_buffer_load_b128(rx, va ? xbase + x_const[j] + xa : OOB, 0, 0);
            rxw[j] = __builtin_amdgcn_raw_buffer_load_b128(rx, vb ? xbase + x_const[j] + xb : OOB, 0, 0);
        }
        uwo += WG_BKR;
        if (uwo >= row_len) {
            uwo = 0;
            uho += two_row ? 2 : 1;
            if (uho >= P.Ho) { uho = 0; ++un; }
        }
    };
    auto load_chunk = [&](int mbase) {
        if constexpr (WINO) { load_chunk_wino(mbase); return; }
        const int rows_left = m_end - mbase;                  // uniform
        const int gbase = mbase * P.ldg * 4;                  // uniform
#pragma unroll
        for (int j = 0; j < G_LD; ++j) {
            const bool v = g_cv && (g_r + j * G_RSTEP) < rows_left;
            rgv[j] = __builtin_amdgcn_raw_buffer_load_b128(rg, v ? gbase + g_const[j] : OOB, 0, 0);
        }
        const int ihu = uho * P.stride - P.pad_h;             // uniform
        const int xbase = ((un * P.H + ihu) * P.W + uwo * P.stride - P.pad_w) * P.ldx * 4;  // uniform
        const bool hv = x_kv && (unsigned)(ihu + kh) < (unsigned)P.H;
        const int iwu = uwo * P.stride;
#pragma unroll
        for (int j = 0; j < X_LD; ++j) {
            const bool v = hv && (x_r + j * X_RSTEP) < rows_left && (unsigned)(iwu + x_iw[j]) < (unsigned)P.W;
            rxv[j] = __builtin_amdgcn_raw_buffer_load_b128(rx, v ? xbase + x_const[j] : OOB, 0, 0);
        }
        // next chunk: 32 rows further along the same output row, or the start of the next one
        uwo += WG_BKR;
        if (uwo >= P.Wo) {
            uwo = 0;
            if (++uho == P.Ho) { uho = 0; ++un; }
        }
    };
    auto store_chunk = [&](int buf) {
        float *gs = Gs + buf * WG_BKR * BMO;
        float *xs = Xs + buf * WG_BKR * BNK;
#pragma unroll
        for (int j = 0; j < G_LD; ++j) {
            float4 v = as_f4(rgv[j]);
            if (RELU_G) v = relu4(v);
            if constexpr (WINO) {
                if (g_two) {                                   // workgroup-uniform
                    float4 w = as_f4(rgw[j]);
                    if (RELU_G) w = relu4(w);
                    v = make_float4(fmaf(sg, w.x, v.x), fmaf(sg, w.y, v.y), fmaf(sg, w.z, v.z), fmaf(sg, w.w, v.w));
                }
            }
            *reinterpret_cast<float4 *>(gs + (g_r + j * G_RSTEP) * BMO + (tid % G_C4) * 4) = v;
        }
#pragma unroll
        for (int j = 0; j < X_LD; ++j) {
            float4 v = as_f4(rxv[j]);
            if constexpr (WINO) {
                float4 w = as_f4(rxw[j]);
                if (RELU_X) { v = relu4(v); w = relu4(w); }
                if (WINO == 2 && bias2u) {                     // (rows past the split and out-of-range pixels were read as 0)
                    bsum4.x += v.x + w.x; bsum4.y += v.y + w.y; bsum4.z += v.z + w.z; bsum4.w += v.w + w.w;
                }
                if (WINO == 1 || x_two)                        // x_two: workgroup-uniform
                    v = make_float4(fmaf(sv, w.x, v.x), fmaf(sv, w.y, v.y), fmaf(sv, w.z, v.z), fmaf(sv, w.w, v.w));
                if (X_C4 * X_RSTEP == 256 || x_act)
                    *reinterpret_cast<float4 *>(xs + (x_r + j * X_RSTEP) * BNK + (tid % X_C4) * 4) = v;
            } else {
            if (X_C4 * X_RSTEP == 256 || x_act)
                *reinterpret_cast<float4 *>(xs + (x_r + j * X_RSTEP) * BNK + (tid % X_C4) * 4) = RELU_X ? relu4(v) : v;
            }
        }
    };

    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nchunks = (m_end - m_begin + WG_BKR - 1) / WG_BKR;
    if (nchunks > 0) {
        load_chunk(m_begin);
        store_chunk(0);
    }
    __syncthreads();
    const int fr = lane & 31, fk = lane >> 5;
    // (WINO: the tile (kh 0, v 1) stages E = g0 + g1 -- its column sums over the pairs are the sums over the pixels)
    // (WINO == 2: the tile (v 1, parity 0, kh 0..1) likewise)
    const bool do_bias = P.bias_ws != nullptr && !P.bias_taps && k0 == (WINO == 2 ? 8 * P.I : WINO == 1 ? P.I : 0) && tid < BMO;
    // exchanged roles: dy is the gathered operand; its centre tap visits every pixel exactly once, so the
    // column sums of that k-block of the staged X tile are the bias gradient (tile width == one tap)
    int bx_col = -1;   // this thread's slot in a bias_ws row when its k column belongs to a bias tap
    if (WINO == 3 && P.bias_ws != nullptr && P.bias_taps && o0 == 0 && k0 == BNK && tid >= P.I && tid < 2 * P.I)
        bx_col = tid - P.I;        // tile v = 1 stages E = dy0 + dy1; its kh = 1 columns (row shift 0) see every dy row once
    if (WINO == 0 && P.bias_ws != nullptr && P.bias_taps && o0 == 0 && tid < BNK && k0 + tid < P.K) {
        const int tap = (k0 + tid) / P.I;
        if ((P.bias_taps >> tap) & 1) bx_col = __popc(P.bias_taps & ((1u << tap) - 1u)) * P.I + (k0 + tid - tap * P.I);
    }
    const bool do_bias_x = bx_col >= 0;
    float bsum = 0.f;
    for (int c = 0; c < nchunks; ++c) {
        const int buf = c & 1;
        if (c + 1 < nchunks) load_chunk(m_begin + (c + 1) * WG_BKR);
        if (do_bias) {
            const float *gcol = Gs + buf * WG_BKR * BMO + tid;
            float s0 = 0.f, s1 = 0.f;
#pragma unroll
            for (int r = 0; r < WG_BKR; r += 2) { s0 += gcol[r * BMO]; s1 += gcol[(r + 1) * BMO]; }
            bsum += s0 + s1;
        }
        if (do_bias_x) {
            const float *xcol = Xs + buf * WG_BKR * BNK + tid;
            float s0 = 0.f, s1 = 0.f;
#pragma unroll
            for (int r = 0; r < WG_BKR; r += 2) { s0 += xcol[r * BNK]; s1 += xcol[(r + 1) * BNK]; }
            bsum += s0 + s1;
        }
        // a wave's 32-wide blocks are INTERLEAVED with the other waves' (block i of wave wm = i*WAVES_M + wm): the two
        // fragments of a k-step are then 256 bytes apart and k-steps 1 KiB apart -- one ds_read2st64_b32 with immediate
        // offsets per operand and step, no vector add to rebuild a base (vector instructions cost matrix time)
        const float *gs = Gs + buf * WG_BKR * BMO + fk * BMO + wm * 32 + fr;
        const float *xs = Xs + buf * WG_BKR * BNK + fk * BNK + wn * 32 + fr;
        // fragments double-buffered: the ds_reads of k-step kk+1 are in flight during the MFMAs of step kk
        float fa[2][MT], fb[2][NT];
#pragma unroll
        for (int i = 0; i < MT; ++i) fa[0][i] = gs[i * WAVES_M * 32];
#pragma unroll
        for (int j = 0; j < NT; ++j) fb[0][j] = xs[j * WAVES_N * 32];
#pragma unroll
        for (int kk = 0; kk < WG_BKR / 2; ++kk) {
            const int cur = kk & 1, nxt = cur ^ 1;
            if (kk + 1 < WG_BKR / 2) {
#pragma unroll
                for (int i = 0; i < MT; ++i) fa[nxt][i] = gs[(kk + 1) * 2 * BMO + i * WAVES_M * 32];
#pragma unroll
                for (int j = 0; j < NT; ++j) fb[nxt][j] = xs[(kk + 1) * 2 * BNK + j * WAVES_N * 32];
            }
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[cur][i], fb[cur][j], acc[i][j], 0, 0, 0);
            // pin the order: next step's LDS reads first, then this step's MFMAs (hipcc otherwise sinks the
            // reads to just before their use and waits lgkmcnt(0) in front of every MFMA group)
            __builtin_amdgcn_sched_group_barrier(0x100, MT + NT, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, MT * NT, 0);
        }
        if (c + 1 < nchunks) store_chunk(buf ^ 1);
        __syncthreads();
    }
    if (do_bias && o0 + tid < P.O) P.bias_ws[(size_t)split * P.O + o0 + tid] = bsum;
    if (do_bias_x) P.bias_ws[(size_t)split * P.bias_nslots * P.I + bx_col] = bsum;
    if constexpr (WINO == 2) {
        // the eight staging row groups meet in LDS (fixed order); 4 slots per split: (parity, kernel row 1 | 2) -- the
        // reduction kernel adds all S * 4 of them (a long slot list is a long chain of dependent loads there)
        if (bias2u) {                                      // workgroup-uniform
            float4 *red = reinterpret_cast<float4 *>(Xs);  // (the main loop ended with a barrier: the tiles are free)
            red[tid] = bsum4;
            __syncthreads();
            if (bias2 && x_r == 0) {
                float4 t = red[tid];
#pragma unroll
                for (int r = 1; r < 8; ++r) {
                    const float4 u = red[r * X_C4 + tid];
                    t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
                }
                const int slot = par * 2 + (kh - 1);
                *reinterpret_cast<float4 *>(P.bias_ws + ((size_t)split * 4 + slot) * P.I + ci) = t;
            }
        }
    }

    float *slab = P.ws + (size_t)split * P.O * P.K;
    const int colq = lane & 31, rowq = 4 * (lane >> 5);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int k = k0 + (j * WAVES_N + wn) * 32 + colq;
        if (k >= P.K) continue;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int ob = o0 + (i * WAVES_M + wm) * 32 + rowq;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = ob + (r & 3) + 8 * (r >> 2);
                if (o < P.O) slab[(size_t)o * P.K + k] = acc[i][j][r];
            }
        }
    }
}

// Winograd slabs (wgrad_fast_kernel<..., WINO>) -> reference layout.  mode 1: [S][O][(kh 3, v 4, i)], one thread column per
// (o, kh, i), three taps out; mode 2: [S][O][(v 3, parity 2, kh 4, i)], one column per (o, parity, kh, i), two taps out;
// mode 3: [S][O = ci][(v 4, kh 3, i = co)], as mode 1 into the transposed destination.
// Same fixed order as the plain reduction: split lane g adds splits g, g+8, ...; the 8 partials are added in lane order.
__device__ __forceinline__ void wino_reduce_unit(int mode, int t, int lane, int g, const float *__restrict__ ws,
                                                 float *__restrict__ dw, int O, int I, int Or, int Ir, int S,
                                                 float (*part4)[8][33]) {
    const int nv = mode == 2 ? 3 : 4, ntap = mode == 2 ? 16 : 9;
    const int KW_ = (mode == 2 ? 24 : 12) * I, stride = O * KW_;
    const int per_o = (mode == 2 ? 8 : 3) * I, cols = O * per_o;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    int o = 0, q = 0, i = 0;     // q = kh (mode 1) or parity * 4 + kh (mode 2)
    if (t < cols) {
        o = t / per_o;
        const int r = t - o * per_o;
        q = r / I; i = r - q * I;
        // column of v: mode 1 (kh * 4 + v) * I + i; mode 2 ((v * 2 + parity) * 4 + kh) * I + i = (v * 8 + q) * I + i
        // mode 3 (exchanged roles, slab rows = input channels): (v * 3 + kh) * I + i
        const float *src = ws + (size_t)o * KW_ + (mode == 1 ? q * 4 * I : q * I) + i;
        const int vstep = mode == 1 ? I : (mode == 2 ? 8 : 3) * I;
        for (int z = g; z < S; z += 8) {
#pragma unroll
            for (int v = 0; v < 4; ++v)
                if (v < nv) s[v] += src[(size_t)z * stride + v * vstep];
        }
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) part4[v][g][lane] = s[v];
    __syncthreads();
    if (g == 0 && t < cols && o < Or && i < Ir) {
        float r4[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            float a = part4[v][0][lane];
#pragma unroll
            for (int qq = 1; qq < 8; ++qq) a += part4[v][qq][lane];
            r4[v] = a;
        }
        float *dst = dw + (mode == 3 ? (size_t)i * Or + o : (size_t)o * Ir + i) * ntap;
        if (mode != 2) {
            const float h = 0.5f * (r4[1] + r4[2]);
            dst[q * 3 + 0] = r4[0] + h;
            dst[q * 3 + 1] = 0.5f * (r4[1] - r4[2]);
            dst[q * 3 + 2] = h + r4[3];
        } else {
            const int par = q >> 2, kh = q & 3;
            dst[kh * 4 + par] = r4[0] + r4[1];          // taps 0 / 1
            dst[kh * 4 + par + 2] = r4[1] - r4[2];      // taps 2 / 3
        }
    }
    __syncthreads();
}

// Sum the slabs and scatter [o][tap][i] (padded O x I) -> reference layout [Or][Ir][tap].
// 256 threads = 32 outputs x 8 split-lanes: lane g adds splits g, g+8, ... (4 loads in flight), the 8
// partial sums are combined through LDS in a fixed order -> bit-reproducible, and latency is paid
// S/32 times instead of S times.  The last workgroup also folds the bias partials.
// (This kernel and wgrad_reduce_batched_kernel take the same job -- wgrad_job_init_impl fills it for both -- and give the
// same dw, but they are NOT one kernel: with more than 32 bias partials this one adds them into one accumulator per lane,
// the batched one into four (its bias units run through the slab loop), so the db bits differ.  Merging them changes bits.)
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float *__restrict__ ws, float *__restrict__ dw, int O,
                                                           int I, int Or, int Ir, int taps, int S,
                                                           const float *__restrict__ bias_ws, float *__restrict__ db,
                                                           int swapped, int bias_splits) {
    __shared__ float part[8][33];
    const int lane = threadIdx.x & 31, g = threadIdx.x >> 5;
    __shared__ float part4[4][8][33];
    const int wmode = (swapped >> 1) & 3;     // 0 plain, 1 F(2,3) rows, 2 F(2,2) by parity
    if (wmode) {
        const int cols = O * (wmode == 2 ? 8 : 3) * I;
        for (int base = blockIdx.x * 32; base < cols; base += gridDim.x * 32)
            wino_reduce_unit(wmode, base + lane, lane, g, ws, dw, O, I, Or, Ir, S, part4);
    }
    const int K = taps * I;
    const int total = wmode ? 0 : O * K;
    swapped = wmode ? 0 : (swapped & 1);
    for (int base = blockIdx.x * 32; base < total; base += gridDim.x * 32) {
        const int t = base + lane;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        if (t < total) {
            int z = g;
            for (; z + 24 < S; z += 32) {
                s0 += ws[(size_t)z * total + t];
                s1 += ws[(size_t)(z + 8) * total + t];
                s2 += ws[(size_t)(z + 16) * total + t];
                s3 += ws[(size_t)(z + 24) * total + t];
            }
            for (; z < S; z += 8) s0 += ws[(size_t)z * total + t];
        }
        part[g][lane] = (s0 + s1) + (s2 + s3);
        __syncthreads();
        if (g == 0 && t < total) {
            float s = part[0][lane];
#pragma unroll
            for (int q = 1; q < 8; ++q) s += part[q][lane];
            const int o = t / K, k = t - o * K;
            const int tap = k / I, i = k - tap * I;
            if (o < Or && i < Ir) {
                if (swapped) dw[((size_t)i * Or + o) * taps + (taps - 1 - tap)] = s;   // slab is [ci][flipped tap][co]
                else dw[((size_t)o * Ir + i) * taps + tap] = s;
            }
        }
        __syncthreads();
    }
    if (db && bias_ws && blockIdx.x == gridDim.x - 1) {
        // bias_splits > 0: partials came from the gathered operand, [bias_splits][I]; else from the G tile, [S][O]
        const int bstride = bias_splits ? I : O, blimit = bias_splits ? Ir : Or, bcount = bias_splits ? bias_splits : S;
        for (int base = 0; base < blimit; base += 32) {
            const int o = base + lane;
            float s0 = 0.f;
            if (o < blimit)
                for (int z = g; z < bcount; z += 8) s0 += bias_ws[(size_t)z * bstride + o];
            part[g][lane] = s0;
            __syncthreads();
            if (g == 0 && o < blimit) {
                float s = part[0][lane];
#pragma unroll
                for (int q = 1; q < 8; ++q) s += part[q][lane];
                db[o] = s;
            }
            __syncthreads();
        }
    }
}

static int colsum_impl(const float *dy, int64_t rows, int C, int ld, float *db, int nout, float *ws, hipStream_t s);

// All layers' slab reductions in ONE launch (the per-layer reductions are latency-bound and tiny).
// Index space = "units" of 32 consecutive outputs; a job owns [unit_offset, unit_offset + n_units_w +
// n_units_b): first the weight units, then the bias units.  Same 32 x 8 fixed-order scheme as above.
// (Bias units share the four-accumulator loop of the weight units: see the note at wgrad_reduce_kernel before merging.)
__global__ __launch_bounds__(256) void wgrad_reduce_batched_kernel(const vq2_wgrad_job *__restrict__ jobs, int njobs,
                                                                   int64_t total_units) {
    __shared__ float part[8][33];
    __shared__ float part4[4][8][33];
    const int lane = threadIdx.x & 31, g = threadIdx.x >> 5;
    for (int64_t u = blockIdx.x; u < total_units; u += gridDim.x) {
        int lo = 0, hi = njobs - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (jobs[mid].unit_offset <= u) lo = mid; else hi = mid - 1;
        }
        const vq2_wgrad_job j = jobs[lo];
        const int lu = (int)(u - j.unit_offset);
        const bool is_bias = lu >= j.n_units_w;
        if ((j.swapped & 6) && !is_bias) {   // Winograd slabs: unit = 32 thread columns (wino_reduce_unit)
            wino_reduce_unit((j.swapped >> 1) & 3, lu * 32 + lane, lane, g, j.ws, j.dw, j.O, j.I, j.Or, j.Ir, j.S, part4);
            continue;
        }
        const int K = j.taps * j.I;
        const int total = is_bias ? (j.bias_splits ? j.I : j.O) : j.O * K;      // stride between splits
        const int limit = is_bias ? (j.bias_splits ? j.Ir : j.Or) : j.O * K;
        const int nsplit = (is_bias && j.bias_splits) ? j.bias_splits : j.S;
        const float *src = is_bias ? j.bias_ws : j.ws;
        const int t = (is_bias ? lu - j.n_units_w : lu) * 32 + lane;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        if (t < limit) {
            int z = g;
            for (; z + 24 < nsplit; z += 32) {
                s0 += src[(size_t)z * total + t];
                s1 += src[(size_t)(z + 8) * total + t];
                s2 += src[(size_t)(z + 16) * total + t];
                s3 += src[(size_t)(z + 24) * total + t];
            }
            for (; z < nsplit; z += 8) s0 += src[(size_t)z * total + t];
        }
        part[g][lane] = (s0 + s1) + (s2 + s3);
        __syncthreads();
        if (g == 0 && t < limit) {
            float s = part[0][lane];
#pragma unroll
            for (int q = 1; q < 8; ++q) s += part[q][lane];
            if (is_bias) {
                j.db[t] = s;
            } else {
                const int o = t / K, k = t - o * K;
                const int tap = k / j.I, i = k - tap * j.I;
                if (o < j.Or && i < j.Ir) {
                    if (j.swapped & 1) j.dw[((size_t)i * j.Or + o) * j.taps + (j.taps - 1 - tap)] = s;
                    else j.dw[((size_t)o * j.Ir + i) * j.taps + tap] = s;
                }
            }
        }
        __syncthreads();
    }
}

// ====================================================================== the plan: roles, kernel, tile, splits
// plan_wgrad() decides everything about a launch from the layer (vq2_conv_desc) alone; wgrad_params() and wgrad_job_init_impl()
// fill the kernels' arguments from it, the tile's launcher launches what it says, wgrad_label() prints it (as on the
// forward side: plan_conv / conv_tiles / conv_label / launch_conv).
// Roles (see the head of this file): plain conv, the same conv with x and dy exchanged (plan_wgrad says when), conv-transpose
enum WgradRole { WGRAD_PLAIN, WGRAD_EXCHANGED, WGRAD_CONVT };
// wgrad_kernel, wgrad_fast_kernel direct, wgrad_fast_kernel<..., WINO = wino>, wgrad_bf16_kernel (vq2_wgrad_bf16.hip)
enum WgradFamily { WGRAD_GEN, WGRAD_FAST, WGRAD_WINO, WGRAD_BF16 };

struct WgradPlan {
    int role, family;   // WgradRole, WgradFamily
    int wino;           // WGRAD_WINO: the mode, 1 F(2,3) along the rows, 2 F(2,2) by column parity, 3 F(2,3) with exchanged
                        // roles (K and M are then the Winograd ones, M in column pairs: see wgrad_fast_kernel)
    int tile;           // position in WGRAD_TILES
    int O, I, K, M, S, rows_per_split;   // the GEMM [O x M] * [M x K] and its split
    int Or, Ir;         // real channels of the rows and columns of a slab: the reduction writes dw for those only
    int bias_taps, bias_nslots, bias_splits;   // see WgradParams; vq2_wgrad_job.bias_splits (S * nslots, or 0 for [S][O])
    size_t bias_floats; // bias partials behind the S slabs: [S][nslots][I] from the gathered operand, or [S][O]
    int mode;           // the reduction kernels' mode word (vq2_wgrad_job.swapped): bit 0 exchanged roles, bits 1-2 wino
    long ext_x, ext_g;  // element counts of the two operands as the kernels index them
    WgradBf16Plan b16;  // WGRAD_BF16: the tile and split of the bf16-operand kernel (`tile` is then not a WGRAD_TILES position)
};

// The two operands as the kernels see them -- the exchange of x and dy, written once: X is gathered through the taps (an
// H x W grid) and is dy unless the role is plain, G is streamed row by row (an Ho x Wo grid, M = N * Ho * Wo rows).
static WgradParams wgrad_operands(const vq2_conv_desc *d, int role) {
    WgradParams P{};
    P.N = d->N; P.KH = d->KH; P.KW = d->KW; P.stride = d->stride; P.pad_h = d->pad_top; P.pad_w = d->pad_left;
    P.H = d->H; P.W = d->W; P.Ho = d->H; P.Wo = d->W;
    P.ldx = role == WGRAD_PLAIN ? d->ldx : d->ldy;
    P.ldg = role == WGRAD_PLAIN ? d->ldy : d->ldx;
    if (role == WGRAD_PLAIN) { P.Ho = out_hw(d).h; P.Wo = out_hw(d).w; }
    else if (role == WGRAD_CONVT) { P.H = 2 * d->H; P.W = 2 * d->W; }      // dy is the 2H x 2W tensor
    else { P.stride = 1; P.pad_h = P.pad_w = d->KH - 1 - d->pad_top; }       // dy the size of x; flipped taps, pad' = K - 1 - p
    return P;
}

// The launcher of a tile picks the instantiation the plan names: the family, and the operand the ReLU sits on (compile-time
// in the fast kernel: every vector instruction competes with the MFMAs).  The Winograd modes exist on one tile each -- 1 and
// 2 on 128 x 128, 3 on 128 x 96 -- and without a ReLU on the operand that is never x (mode 1: G, mode 3: X).
template <int WM, int WN, int MT, int NT>
static int launch_wgrad(const WgradPlan &pl, const WgradParams &P, hipStream_t s) {
    constexpr int BMO = WM * MT * 32, BNK = WN * NT * 32;
    const bool rx = P.relu_x, rg = P.relu_g;
    void (*kern)(const WgradParams) = nullptr;
    if (pl.family == WGRAD_GEN) kern = wgrad_kernel<WM, WN, MT, NT>;
    else if (pl.family == WGRAD_FAST)
        kern = rx ? wgrad_fast_kernel<WM, WN, MT, NT, true, false>
                  : rg ? wgrad_fast_kernel<WM, WN, MT, NT, false, true> : wgrad_fast_kernel<WM, WN, MT, NT, false, false>;
    else if constexpr (BMO == 128 && BNK == 128) {
        if (pl.wino == 1) kern = rx ? wgrad_fast_kernel<WM, WN, MT, NT, true, false, 1> : wgrad_fast_kernel<WM, WN, MT, NT, false, false, 1>;
        if (pl.wino == 2)
            kern = rx ? wgrad_fast_kernel<WM, WN, MT, NT, true, false, 2>
                      : rg ? wgrad_fast_kernel<WM, WN, MT, NT, false, true, 2> : wgrad_fast_kernel<WM, WN, MT, NT, false, false, 2>;
    } else if constexpr (BMO == 128 && BNK == 96) {
        if (pl.wino == 3) kern = rg ? wgrad_fast_kernel<WM, WN, MT, NT, false, true, 3> : wgrad_fast_kernel<WM, WN, MT, NT, false, false, 3>;
    }
    if (!kern) return set_error(VQ2_ERR_INVALID, "conv_wgrad: the %d x %d tile has no Winograd mode %d", BMO, BNK, pl.wino);
    const size_t lds = (size_t)2 * WG_BKR * (BMO + BNK) * sizeof(float);
    allow_big_lds(kern, lds);
    // (Winograd modes: K is a whole number of tiles -- mode 3 has four, one per v -- and O a multiple of 128)
    hipLaunchKernelGGL(kern, dim3(((P.K + BNK - 1) / BNK) * ((P.O + BMO - 1) / BMO) * pl.S), dim3(256), lds, s, P);
    return check_launch(pl.wino == 3 ? "wgrad_fast_kernel<wino sw>" : pl.wino ? "wgrad_fast_kernel<wino>" : "wgrad_kernel");
}

// Every tile (o x k) once, with its launcher, in the order plan_wgrad tries them (a plan's `tile` is the position).
struct WgradTile { int bmo, bnk; int (*launch)(const WgradPlan &, const WgradParams &, hipStream_t); };
template <int WM, int WN, int MT, int NT>
static constexpr WgradTile wgrad_tile() { return {WM * MT * 32, WN * NT * 32, launch_wgrad<WM, WN, MT, NT>}; }
static constexpr WgradTile WGRAD_TILES[] = {
    wgrad_tile<2, 2, 2, 2>(),     // 128 x 128
    wgrad_tile<1, 4, 2, 1>(),     // 64 x 128
    wgrad_tile<1, 4, 1, 2>(),     // 32 x 256
    // 128 x 96 = one kernel row of a 3x3 conv with 32 gathered channels (the ResBlock weight gradient with
    // exchanged roles, K = 288): 48 MFMAs per wave and chunk instead of 16 for the same staging
    wgrad_tile<4, 1, 1, 3>(),
    wgrad_tile<4, 1, 1, 1>(),     // 128 x 32 (1x1 convs with few inputs)
    wgrad_tile<2, 2, 1, 1>(),     // 64 x 64
};
constexpr int WGRAD_NTILES = sizeof(WGRAD_TILES) / sizeof(WgradTile);

// position of the tile with these dimensions (the two that plan_wgrad names exist: checked when this file is compiled)
static constexpr int wgrad_tile_of(int bmo, int bnk) {
    for (int i = 0; i < WGRAD_NTILES; ++i)
        if (WGRAD_TILES[i].bmo == bmo && WGRAD_TILES[i].bnk == bnk) return i;
    return -1;
}
static_assert(wgrad_tile_of(128, 128) >= 0 && wgrad_tile_of(128, 96) >= 0, "plan_wgrad names a tile that WGRAD_TILES lacks");

static WgradPlan plan_wgrad(const vq2_conv_desc *d) {
    WgradPlan p{};
    // A stride-1 "same" conv with few output channels (the ResBlock 3x3, 128 -> 32): gathering the im2col
    // of the WIDE tensor x re-reads it KH*KW times through L2.  The same sum with the roles exchanged,
    //   dw[co][ci][kh][kw] = sum_q relu(x)[q][ci] * dy[q - (kh-p, kw-p)][co],
    // gathers the NARROW tensor dy instead (flipped taps, pad' = K-1-p) and streams x once.  Square kernels with the
    // same centred padding on both axes only.
    // (Exchanged roles and the Winograd modes below are fast-kernel forms: VQ2_FORMS=general plans neither, =direct no
    // Winograd mode.)
    const bool fast = forms() > FORMS_GENERAL;
    // Winograd modes: tensors that the 32-bit byte offsets of wgrad_fast_kernel reach (x and dy counted over the INPUT grid)
    const long pix = (long)d->N * d->H * d->W;
    const bool wino = forms() == FORMS_ALL && pix * d->ldx < FAST_REACH && pix * d->ldy * (d->transposed ? 4 : 1) < FAST_REACH;
    if (fast && !d->transposed && d->stride == 1 && d->KH == d->KW && d->pad_top == d->pad_left && 2 * d->pad_top == d->KH - 1 &&
        d->KH > 1 && d->Co <= 32 && d->Ci >= 64)
        p.role = WGRAD_EXCHANGED;
    else
        p.role = d->transposed ? WGRAD_CONVT : WGRAD_PLAIN;
    const WgradParams v = wgrad_operands(d, p.role);
    const bool plain = p.role == WGRAD_PLAIN;
    p.O = plain ? d->Co : d->Ci;
    p.I = plain ? d->Ci : d->Co;
    p.Or = plain ? real_co(d) : real_ci(d);
    p.Ir = plain ? real_ci(d) : real_co(d);
    p.M = d->N * v.Ho * v.Wo;
    p.K = d->KH * d->KW * p.I;
    if (wino && plain && d->KH == 3 && d->KW == 3 && d->stride == 1 && d->pad_top == 1 && d->pad_left == 1 &&
        p.O % 128 == 0 && p.I % 128 == 0 && (d->W % 64 == 0 || (d->W == 32 && d->H % 2 == 0))) {
        p.wino = 1;
        p.K = 12 * p.I;
        p.M = p.M / 2;
    }
    {   // 4x4 stride-2 conv / conv-transpose: F(2,2) by column parity over output column pairs
        const int wo = d->transposed ? d->W : d->W / 2;       // width of the G operand's grid
        if (wino && p.role != WGRAD_EXCHANGED && d->KH == 4 && d->KW == 4 && d->stride == 2 && d->pad_top == 1 && d->H % 2 == 0 &&
            d->W % 2 == 0 && p.O % 128 == 0 && (p.I == 64 || p.I % 128 == 0) &&
            (wo % 64 == 0 || (wo == 32 && (d->transposed ? d->H : d->H / 2) % 2 == 0))) {
            p.wino = 2;
            p.K = 24 * p.I;
            p.M = p.M / 2;
        }
    }
    // output tile (o x k): the one that wastes the least padded work, the earlier (larger) tile on ties; modes 1 and 2
    // have the 128 x 128 tile only
    if (p.wino) {
        p.tile = wgrad_tile_of(128, 128);
    } else {
        long best = -1;
        for (int c = 0; c < WGRAD_NTILES; ++c) {
            const WgradTile &t = WGRAD_TILES[c];
            if (t.bnk == 96 && p.M < 65536) continue;   // measured: +6 % at 131072 rows, -9 % at 32768
            const long po = (p.O + t.bmo - 1) / t.bmo * t.bmo;
            const long pk = (p.K + t.bnk - 1) / t.bnk * t.bnk;
            const long work = po * pk;
            if (best < 0 || work < best) { best = work; p.tile = c; }
        }
    }
    if (wino && p.role == WGRAD_EXCHANGED && d->KH == 3 && d->pad_top == 1 && p.I == 32 && p.O % 128 == 0 &&
        (d->W % 64 == 0 || (d->W == 32 && d->H % 2 == 0))) {
        p.wino = 3;                 // exchanged roles + F(2,3): four 128 x 96 tiles (v) of three kernel rows each
        p.K = 4 * 96;
        p.M = p.M / 2;
        p.tile = wgrad_tile_of(128, 96);   // whatever the tile search said
    }
    const int bmo = WGRAD_TILES[p.tile].bmo, bnk = WGRAD_TILES[p.tile].bnk;
    const int tiles = ((p.K + bnk - 1) / bnk) * ((p.O + bmo - 1) / bmo);
    const int lds = 2 * WG_BKR * (bmo + bnk) * 4;
    int per_cu = (160 * 1024) / lds;                 // resident workgroups per CU (LDS-bound), at most 4
    if (per_cu > 4) per_cu = 4;
    int S = (256 * per_cu) / tiles;                  // fill the resident slots without a tail round
    const int max_s = (p.M + 255) / 256;             // at least 8 chunks of 32 rows per split
    if (S > max_s) S = max_s;
    if (S < 1) S = 1;
    int rps = (p.M + S - 1) / S;
    rps = (rps + 31) / 32 * 32;
    p.S = (p.M + rps - 1) / rps;
    p.rows_per_split = rps;
    // The kernel.  wgrad_fast_kernel in its direct forms: rows of whole 32-pixel chunks, tensors that 32-bit byte offsets
    // reach.  This reach test is NOT the one of the Winograd modes above: it counts the operands as the kernels index them
    // (X over its own grid, 2H x 2W for a conv-transpose; G over the M reduction rows), that one counts x and dy over the
    // input grid.  (rows_per_split % 32 cannot fail after the rounding above: it is the kernel's own precondition, kept.)
    p.ext_x = (long)d->N * v.H * v.W * v.ldx;
    p.ext_g = (long)p.M * v.ldg;
    const bool fast_ok = fast && v.Wo % WG_BKR == 0 && p.rows_per_split % WG_BKR == 0 && p.ext_x < FAST_REACH && p.ext_g < FAST_REACH;
    p.family = p.wino ? WGRAD_WINO : fast_ok ? WGRAD_FAST : WGRAD_GEN;
    // Bias partials.  Which taps of the gathered operand cover every dy pixel exactly once (bias gradient = their column
    // sums): exchanged roles -> the centre tap (its own flip); conv-transpose k4 s2 p1 -> taps (1,1),(1,2),(2,1),(2,2), one
    // per output phase, never out of bounds.  Plain conv: none, the bias gradient is the column sums of the G tile.
    if (p.wino == 2 && d->transposed) { p.bias_taps = 1; p.bias_nslots = 4; }    // flag only: see wgrad_fast_kernel<..., 2>
    else if (p.role == WGRAD_EXCHANGED) { p.bias_taps = 1 << ((d->KH / 2) * d->KW + d->KW / 2); p.bias_nslots = 1; }
    else if (d->transposed) { p.bias_taps = (1 << 5) | (1 << 6) | (1 << 9) | (1 << 10); p.bias_nslots = 4; }
    p.bias_floats = p.bias_taps ? (size_t)p.S * p.bias_nslots * p.I : (size_t)p.S * p.O;
    p.bias_splits = p.bias_taps ? p.S * p.bias_nslots : 0;
    p.mode = (p.role == WGRAD_EXCHANGED) | (p.wino << 1);
    return p;
}

// The plan of a launch with its flags: VQ2_ALLOW_BF16 on an eligible layer (conv_wgrad_bf16_shape) takes the bf16-operand
// kernel with a plan of its own -- plain roles, no Winograd mode, its own tile and split, whatever the fp32 plan of the layer
// says; slabs [S][O][K] and bias partials [S][O] in the plain layout (mode word 0).  Every other launch, flag or not, is
// plan_wgrad(d) unchanged.
static WgradPlan plan_wgrad(const vq2_conv_desc *d, int flags) {
    if (!((flags & VQ2_ALLOW_BF16) && conv_wgrad_bf16_shape(d))) return plan_wgrad(d);
    WgradPlan p{};
    p.b16 = plan_wgrad_bf16(d);
    p.role = WGRAD_PLAIN; p.family = WGRAD_BF16;
    p.O = p.b16.O; p.I = p.b16.I; p.K = p.b16.K; p.M = p.b16.M; p.S = p.b16.S; p.rows_per_split = p.b16.rows_per_split;
    p.Or = real_co(d); p.Ir = real_ci(d);
    p.bias_floats = (size_t)p.S * p.O;
    p.ext_x = (long)p.M * d->ldx; p.ext_g = (long)p.M * d->ldy;
    return p;
}

static size_t wgrad_ws_bytes(const WgradPlan &p) { return ((size_t)p.S * p.O * p.K + p.bias_floats) * sizeof(float); }

// The kernels' arguments of a planned launch; the slabs [S][O][K] come first in ws, the bias partials behind them.
static int wgrad_params(const vq2_conv_desc *d, const WgradPlan &p, int flags, const float *x, const float *dy, float *db, void *ws,
                        WgradParams &P) {
    VQ2_REQUIRE(p.ext_x < (1L << 31) && p.ext_g < (1L << 31), "conv_wgrad: tensor exceeds 2^31 elements");
    const bool plain = p.role == WGRAD_PLAIN;
    const int relu = (flags & VQ2_RELU_IN) != 0;       // of x, whichever operand that is
    P = wgrad_operands(d, p.role);
    P.x = plain ? x : dy; P.relu_x = plain ? relu : 0;
    P.g = plain ? dy : x; P.relu_g = plain ? 0 : relu;
    P.ws = static_cast<float *>(ws);
    P.bias_ws = db ? P.ws + (size_t)p.S * p.O * p.K : nullptr;
    P.bias_taps = p.bias_taps; P.bias_nslots = p.bias_nslots;
    P.O = p.O; P.I = p.I; P.K = p.K; P.M = p.M; P.rows_per_split = p.rows_per_split;
    return VQ2_OK;
}

// The profiler label of a planned launch, "wgrad<tile><form>|<shape>,fast|gen" (wgrad_fast_kernel or wgrad_kernel):
// formatted here and nowhere else.
static const char *wgrad_label(const WgradPlan &p, int bmo, int bnk, const vq2_conv_desc *d) {
    const char *form = p.wino == 3 ? "swwino" : p.role == WGRAD_EXCHANGED ? "sw" : p.wino == 1 ? "wino" : p.wino == 2 ? "wino4" : "";
    return prof_label("wgrad<%dx%d>%s|O=%d,K=%d,M=%d,S=%d,k%d,%s", bmo, bnk, form, p.O, p.K, p.M, p.S, d->KH,
                      p.family == WGRAD_BF16 ? "bf16" : p.family == WGRAD_GEN ? "gen" : "fast");
}

// ------------------------------------------------------------------ column sums (bias gradient)
constexpr int CS_MAX_BLOCKS = 512;

static inline int64_t cs_rows_per_block(int64_t rows) {
    int64_t rpb = (rows + CS_MAX_BLOCKS - 1) / CS_MAX_BLOCKS;
    return rpb < 256 ? 256 : rpb;
}

__global__ __launch_bounds__(256) void colsum_partial_kernel(const float *__restrict__ x, int64_t rows, int C, int ld,
                                                             int64_t rpb, float *__restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float red[];  // [nrg][C]
    const int C4 = C / 4;
    const int nrg = 256 / C4 > 0 ? 256 / C4 : 1;
    const int64_t r0 = (int64_t)blockIdx.x * rpb;
    const int64_t r1 = r0 + rpb < rows ? r0 + rpb : rows;
    for (int cbase = 0; cbase < C4; cbase += 256) {
        const int c4 = cbase + (int)(threadIdx.x % (C4 < 256 ? C4 : 256));
        const int rg = threadIdx.x / (C4 < 256 ? C4 : 256);
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        if (rg < nrg && c4 < C4) {
            for (int64_t r = r0 + rg; r < r1; r += nrg) {
                const float4 v = *reinterpret_cast<const float4 *>(x + r * ld + c4 * 4);
                a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
            }
            *reinterpret_cast<float4 *>(red + (size_t)rg * C + c4 * 4) = a;
        }
        __syncthreads();
        for (int c = threadIdx.x; c < C; c += 256) {
            if (c / 4 >= cbase && c / 4 < cbase + 256) {
                float s = 0.f;
                for (int g = 0; g < nrg; ++g) s += red[(size_t)g * C + c];
                part[(size_t)blockIdx.x * C + c] = s;
            }
        }
        __syncthreads();
    }
}

// 256 threads = 32 columns x 8 lanes over the partial blocks; fixed combine order (reproducible)
__global__ __launch_bounds__(256) void colsum_final_kernel(const float *__restrict__ part, int nblocks, int C, int nout,
                                                           float *__restrict__ out) {
    __shared__ float red[8][33];
    const int lane = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + lane;
    float s0 = 0.f, s1 = 0.f;
    if (c < nout) {
        int b = g;
        for (; b + 8 < nblocks; b += 16) { s0 += part[(size_t)b * C + c]; s1 += part[(size_t)(b + 8) * C + c]; }
        for (; b < nblocks; b += 8) s0 += part[(size_t)b * C + c];
    }
    red[g][lane] = s0 + s1;
    __syncthreads();
    if (g == 0 && c < nout) {
        float s = red[0][lane];
#pragma unroll
        for (int q = 1; q < 8; ++q) s += red[q][lane];
        out[c] = s;
    }
}

static int colsum_impl(const float *dy, int64_t rows, int C, int ld, float *db, int nout, float *ws, hipStream_t s) {
    const int64_t rpb = cs_rows_per_block(rows);
    const int64_t nb = (rows + rpb - 1) / rpb;
    const int C4 = C / 4;
    const int nrg = 256 / C4 > 0 ? 256 / C4 : 1;
    hipLaunchKernelGGL(colsum_partial_kernel, dim3((unsigned)nb), dim3(256), (size_t)nrg * C * sizeof(float), s, dy, rows,
                       C, ld, rpb, ws);
    if (int e = check_launch("colsum_partial_kernel")) return e;
    hipLaunchKernelGGL(colsum_final_kernel, dim3((nout + 31) / 32), dim3(256), 0, s, ws, (int)nb, C, nout, db);
    return check_launch("colsum_final_kernel");
}

}  // namespace vq2

using namespace vq2;

extern "C" int vq2_conv_wgrad_bf16_eligible(const vq2_conv_desc *d) { return d != nullptr && conv_wgrad_bf16_shape(d); }

// 0 for anything check_conv_desc refuses.  flags: those of the launch the workspace is for (VQ2_ALLOW_BF16 changes the plan)
extern "C" size_t vq2_conv_wgrad_workspace_bytes_ex(const vq2_conv_desc *d, int flags) {
    if (!d || check_conv_desc(d, "conv_wgrad_workspace_bytes", DESC_PLAN_ONLY)) return 0;   // (null: no message)
    return wgrad_ws_bytes(plan_wgrad(d, flags));
}
extern "C" size_t vq2_conv_wgrad_workspace_bytes(const vq2_conv_desc *d) { return vq2_conv_wgrad_workspace_bytes_ex(d, 0); }

// The reduction job of a planned layer: what wgrad_reduce_batched_kernel reads, and the arguments of wgrad_reduce_kernel.
static void wgrad_job_init_impl(const vq2_conv_desc *d, const WgradPlan &p, const void *ws, float *dw, float *db, vq2_wgrad_job *job) {
    const float *w = static_cast<const float *>(ws);
    job->ws = w; job->dw = dw;
    job->O = p.O; job->I = p.I; job->Or = p.Or; job->Ir = p.Ir;
    job->swapped = p.mode;
    job->taps = d->KH * d->KW; job->S = p.S;
    job->n_units_w = p.wino ? (p.O * (p.wino == 2 ? 8 : 3) * p.I + 31) / 32 : (p.O * p.K + 31) / 32;
    // without db no bias partials were asked for: nothing of the bias is described
    job->db = db; job->bias_ws = db ? w + (size_t)p.S * p.O * p.K : nullptr;
    job->bias_splits = db ? p.bias_splits : 0;
    job->n_units_b = db ? ((p.bias_taps ? p.Ir : p.Or) + 31) / 32 : 0;
    job->unit_offset = 0;
}

// slabs (+ bias partials); reduce == true also runs the per-layer reduction into dw/db
static int wgrad_impl(const vq2_conv_desc *d, int flags, const float *x, const float *dy, float *dw, float *db, void *ws,
                      size_t ws_bytes, vq2_stream_t stream, bool reduce) {
    if (int e = check_conv_desc(d, "conv_wgrad")) return e;
    VQ2_REQUIRE(x && dy && ws && (dw || !reduce), "conv_wgrad: null pointer");
    VQ2_REQUIRE(aligned16(x) && aligned16(dy) && aligned16(ws), "conv_wgrad: pointers must be 16-byte aligned");
    const WgradPlan p = plan_wgrad(d, flags);
    VQ2_REQUIRE(ws_bytes >= wgrad_ws_bytes(p), "conv_wgrad: workspace too small");
    hipStream_t s = to_stream(stream);
    const ConvWork work = conv_work(d, 0, 0);
    if (p.family == WGRAD_BF16) {
        float *slabs = static_cast<float *>(ws);
        ProfScope prof(prof_enabled() ? wgrad_label(p, p.b16.bmo, p.b16.bnk, d) : "wgrad", work.flops, work.bytes, s);
        if (int e = launch_wgrad_bf16(p.b16, d, (flags & VQ2_RELU_IN) != 0, x, dy, slabs,
                                      db ? slabs + (size_t)p.S * p.O * p.K : nullptr, s)) return e;
    } else {
        WgradParams P;
        if (int e = wgrad_params(d, p, flags, x, dy, db, ws, P)) return e;
        const WgradTile &tile = WGRAD_TILES[p.tile];
        ProfScope prof(prof_enabled() ? wgrad_label(p, tile.bmo, tile.bnk, d) : "wgrad", work.flops, work.bytes, s);
        if (int e = tile.launch(p, P, s)) return e;
    }
    if (!reduce) return VQ2_OK;
    vq2_wgrad_job j;   // what the deferred path hands to wgrad_reduce_batched_kernel, reduced at once
    wgrad_job_init_impl(d, p, ws, dw, db, &j);
    const int total = p.O * p.K;
    const int blocks = (total + 31) / 32 < 4096 ? (total + 31) / 32 : 4096;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(blocks), dim3(256), 0, s, j.ws, j.dw, j.O, j.I, j.Or, j.Ir, j.taps, j.S,
                       j.bias_ws, j.db, j.swapped, j.bias_splits);
    return check_launch("wgrad_reduce_kernel");
}

extern "C" int vq2_conv_wgrad(const vq2_conv_desc *d, int flags, const float *x, const float *dy, float *dw, float *db,
                              void *ws, size_t ws_bytes, vq2_stream_t stream) {
    return wgrad_impl(d, flags, x, dy, dw, db, ws, ws_bytes, stream, true);
}
extern "C" int vq2_conv_wgrad_partial(const vq2_conv_desc *d, int flags, const float *x, const float *dy, float *db,
                                      void *ws, size_t ws_bytes, vq2_stream_t stream) {
    return wgrad_impl(d, flags, x, dy, nullptr, db, ws, ws_bytes, stream, false);
}

extern "C" int vq2_wgrad_job_init_ex(const vq2_conv_desc *d, int flags, const void *ws, float *dw, float *db, vq2_wgrad_job *job) {
    if (int e = check_conv_desc(d, "wgrad_job_init", DESC_PLAN_ONLY)) return e;
    VQ2_REQUIRE(ws && dw && job, "wgrad_job_init: null pointer");
    wgrad_job_init_impl(d, plan_wgrad(d, flags), ws, dw, db, job);
    return VQ2_OK;
}
extern "C" int vq2_wgrad_job_init(const vq2_conv_desc *d, const void *ws, float *dw, float *db, vq2_wgrad_job *job) {
    return vq2_wgrad_job_init_ex(d, 0, ws, dw, db, job);
}

extern "C" int vq2_wgrad_reduce_batched(const vq2_wgrad_job *jobs_dev, int32_t njobs, int64_t total_units,
                                        vq2_stream_t stream) {
    VQ2_REQUIRE(jobs_dev && njobs > 0 && total_units > 0, "wgrad_reduce_batched: bad arguments");
    const unsigned blocks = (unsigned)(total_units < 8192 ? total_units : 8192);
    hipLaunchKernelGGL(wgrad_reduce_batched_kernel, dim3(blocks), dim3(256), 0, to_stream(stream), jobs_dev, njobs,
                       total_units);
    return check_launch("wgrad_reduce_batched_kernel");
}

extern "C" size_t vq2_colsum_workspace_bytes(int64_t rows, int32_t C) {
    if (rows <= 0 || C <= 0) return 0;
    const int64_t rpb = cs_rows_per_block(rows);
    return (size_t)((rows + rpb - 1) / rpb) * C * sizeof(float);
}

extern "C" int vq2_colsum(const float *dy, int64_t rows, int32_t C, int32_t ld, float *db, void *ws, size_t ws_bytes,
                          vq2_stream_t stream) {
    VQ2_REQUIRE(dy && db && ws, "colsum: null pointer");
    VQ2_REQUIRE(rows > 0 && C > 0 && C % 4 == 0 && ld >= C && ld % 4 == 0 && C <= 4096, "colsum: bad shape");
    VQ2_REQUIRE(aligned16(dy), "colsum: dy must be 16-byte aligned");
    VQ2_REQUIRE(ws_bytes >= vq2_colsum_workspace_bytes(rows, C), "colsum: workspace too small");
    return colsum_impl(dy, rows, C, ld, db, C, static_cast<float *>(ws), to_stream(stream));
}
