// bf16-operand weight gradient of the stage-2 convs (same_size == 1) for gfx950 (MI355X).
//
//   dw[o][i][kh][kw] = sum over (n,h,w) of  bf16(dy[n,h,w,o]) * bf16(a[n, h-pad_top+kh, w-pad_left+kw, i])
//
// a = x or relu(x) (the ReLU first, then the rounding); bf16() is round-to-nearest-even, the compiler's conversion
// (v_cvt_pk_bf16_f32); the sum is accumulated in fp32 by v_mfma_f32_32x32x16_bf16.  The bias gradient stays the fp32 sum of
// the UNROUNDED dy: the staging threads hold the fp32 values before they round them.
//
//   GEMM [O x M] * [M x K]:  rows o = co,  columns k = (kh, kw, ci) with ci fastest,  depth m = (n, h, w) pixels
//
// Plain roles only (dy streamed, x gathered through the taps), no Winograd mode.  The reduction over M is split over S
// workgroups per output tile; every split writes its partial tile to the slab [split][o][k] of the caller's workspace and
// its bias partial to [split][o] behind the slabs: the layout that wgrad_reduce_kernel / wgrad_reduce_batched_kernel
// (vq2_wgrad.hip) sum in a fixed order.  No atomics; two runs give the same bits.
//
// Both operands are pixel-major in memory (NHWC) and the matrix instruction wants 8 consecutive depth elements -- 8 pixels
// of ONE channel -- per lane, so the tiles are transposed in registers while they are staged: a staging thread loads 8
// pixels x 4 channels (eight 16-byte fp32 loads), rounds, and writes four 16-byte runs of 8 pixels into [channel][pixel]
// rows of 32 pixels = 64 bytes, which ds_read_b128 consumes as the forward kernel's fragments (vq2_conv_bf16.hip).
//
// LDS image: row r (a channel) holds its four 16-byte slots t (8 pixels each) at 64 r + 16 (t ^ ((r >> 2) & 3)).
//   ds_read_b128 (banks of 256 bytes, four groups of 16 lanes {0-3,12-15,20-27}, {4-11,16-19,28-31} and those + 32): a group
//   reads slot t of 16 rows; two rows collide only if r & 3 and (r >> 2) & 3 both agree, and inside either group the four
//   rows of every r & 3 class have four different (r >> 2) & 3 -- no conflict.
//   ds_write_b128 (banks of 128 bytes, groups of 8 consecutive lanes = 8 consecutive channel groups c4): a thread writes rows
//   4 c4 + q, q = 0..3; address mod 128 = 64 (q & 1) + 16 (pg ^ (c4 & 3)).  The threads with c4 & 4 write q ^ 1 where the
//   others write q, so the eight lanes of a group hit eight different slots -- no conflict.
// 64-bit addressing throughout: no reach limit beyond the descriptor's own 2^31 elements.
#include "vq2_conv.h"

namespace vq2 {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x8 __attribute__((ext_vector_type(8)));

namespace wb16 {
constexpr int BP = 32;          // pixels per staged chunk: two 16-deep MFMA steps
constexpr int ROWB = BP * 2;    // bytes per LDS row (32 bf16)
}  // namespace wb16

struct WgradBf16Params {
    const float *x;   // [N,H,W,ldx], I channels: gathered through the taps
    const float *g;   // dy [N,H,W,ldg], O channels: streamed
    float *ws;        // [S][O][K] partial slabs
    float *bias_ws;   // [S][O] partial column sums of the unrounded dy, or null
    int N, H, W, I, ldx, O, ldg;
    int KH, KW, pad_h, pad_w;
    int K, M;
    int rows_per_split;   // multiple of 32
    int relu_x;
};

// 4 waves as 2 x 2, each MT x NT 32x32 accumulators: BMO = 64 MT output channels x BNK = 64 NT columns of k.
// Threads 0 .. BMO-1 stage the dy tile, BMO .. BMO+BNK-1 the x tile (whole waves either way), one 8-pixel x 4-channel
// unit each: unit u = (channel group c4 = u % (channels / 4), pixel group pg = u / (channels / 4)).
template <int MT, int NT>
__global__ __launch_bounds__(256, 2) void wgrad_bf16_kernel(const WgradBf16Params P) {
    using namespace wb16;
    constexpr int BMO = 64 * MT, BNK = 64 * NT;
    static_assert(BMO + BNK <= 256, "one staging unit per thread");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_wb[];
    unsigned char *Gs = smem_wb;                        // [2][BMO] rows of 64 bytes
    unsigned char *Xs = smem_wb + 2 * BMO * ROWB;       // [2][BNK] rows

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int ktiles = (P.K + BNK - 1) / BNK;
    const int otiles = (P.O + BMO - 1) / BMO;
    const int vid = xcd_remap(blockIdx.x, gridDim.x);
    const int k0 = (vid % ktiles) * BNK;
    const int o0 = ((vid / ktiles) % otiles) * BMO;
    const int split = vid / (ktiles * otiles);
    const int m_begin = split * P.rows_per_split;
    const int m_end = min(P.M, m_begin + P.rows_per_split);

    // ---- per-thread staging coordinates (fixed over the loop)
    const bool is_g = tid < BMO;                         // wave-uniform (BMO is a multiple of 64)
    const bool is_x = !is_g && tid < BMO + BNK;
    const int u = is_g ? tid : tid - BMO;
    const int nc4 = is_g ? BMO / 4 : BNK / 4;
    const int c4 = u % nc4, pg = u / nc4;                // pg = 0..3 for a staging thread
    const int col = (is_g ? o0 : k0) + 4 * c4;           // first of this thread's 4 channels (o) / columns (k)
    const bool col_ok = is_g ? col < P.O : (is_x && col < P.K);   // O, K are multiples of 4: all four or none
    int kh = 0, kw = 0, ci = 0;
    if (is_x && col_ok) {
        const int tap = col / P.I;                       // I % 4 == 0: the four columns share the tap
        ci = col - tap * P.I;
        kh = tap / P.KW;
        kw = tap - kh * P.KW;
    }
    // (n, h, w) of the first of this thread's 8 pixels in the coming chunk (x staging only)
    int pn, ph, pw;
    {
        const int m = m_begin + pg * 8, HW = P.H * P.W;
        pn = m / HW;
        const int r = m - pn * HW;
        ph = r / P.W;
        pw = r - ph * P.W;
    }
    const bool do_bias = P.bias_ws != nullptr && k0 == 0;   // workgroup-uniform

    // The eight loads of a chunk are UNCONDITIONAL (a branch around each load makes the compiler wait for every one before
    // it issues the next: eight dependent round trips per chunk): an element that contributes 0 -- a row past the split, a
    // tap outside the image, a column past O or K -- loads the first four floats of its tensor instead (always there) and
    // is zeroed by its bit of `live` when the chunk is staged.
    float4 rv[8];
    unsigned live = 0;
    auto load_chunk = [&](int mbase) {
        const int m0 = mbase + pg * 8;
        live = 0;
        if (is_g) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool v = col_ok && m0 + j < m_end;
                const size_t off = v ? (size_t)(m0 + j) * P.ldg + col : (size_t)0;
                rv[j] = *reinterpret_cast<const float4 *>(P.g + off);
                live |= (unsigned)v << j;
            }
        } else if (is_x) {
            int n = pn, h = ph, w = pw;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int ih = h - P.pad_h + kh, iw = w - P.pad_w + kw;
                const bool v = col_ok && m0 + j < m_end && (unsigned)ih < (unsigned)P.H && (unsigned)iw < (unsigned)P.W;
                const size_t off = v ? ((size_t)(n * P.H + ih) * P.W + iw) * P.ldx + ci : (size_t)0;
                rv[j] = *reinterpret_cast<const float4 *>(P.x + off);
                live |= (unsigned)v << j;
                if (++w == P.W) { w = 0; if (++h == P.H) { h = 0; ++n; } }
            }
            // next chunk: 32 pixels further in (n, h, w) order
            pw += BP;
            while (pw >= P.W) {
                pw -= P.W;
                if (++ph == P.H) { ph = 0; ++pn; }
            }
        }
    };
    float4 bsum = make_float4(0.f, 0.f, 0.f, 0.f);       // dy staging: fp32 sums of this thread's 4 channels, unrounded
    auto store_chunk = [&](int buf) {
        if (!is_g && !is_x) return;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (!((live >> j) & 1u)) rv[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (is_g && do_bias) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { bsum.x += rv[j].x; bsum.y += rv[j].y; bsum.z += rv[j].z; bsum.w += rv[j].w; }
        }
        if (is_x && P.relu_x) {
#pragma unroll
            for (int j = 0; j < 8; ++j) rv[j] = relu4(rv[j]);
        }
        // transpose in registers: channel q of the 8 pixels -> one 16-byte run
        uint4 t[4];                                      // (as four dwords each: the row swap below is then 16 dword selects;
#pragma unroll                                           //  a select between two bf16x8 compiles to a per-element search)
        for (int q = 0; q < 4; ++q) {
            const f32x8 v = {f4_at(rv[0], q), f4_at(rv[1], q), f4_at(rv[2], q), f4_at(rv[3], q),
                             f4_at(rv[4], q), f4_at(rv[5], q), f4_at(rv[6], q), f4_at(rv[7], q)};
            t[q] = __builtin_bit_cast(uint4, __builtin_convertvector(v, bf16x8));
        }
        unsigned char *tile = is_g ? Gs + buf * BMO * ROWB : Xs + buf * BNK * ROWB;
        unsigned char *dst = tile + 4 * c4 * ROWB + 16 * (pg ^ (c4 & 3));   // rows 4 c4 + q: (row >> 2) & 3 = c4 & 3
        const bool sw = (c4 & 4) != 0;                   // these threads write rows q ^ 1 first (bank spread, see the head)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = sw ? (q ^ 1) : q;
            const uint4 a = t[q], b = t[q ^ 1];
            *reinterpret_cast<uint4 *>(dst + row * ROWB) = make_uint4(sw ? b.x : a.x, sw ? b.y : a.y, sw ? b.z : a.z, sw ? b.w : a.w);
        }
    };

    f32x16 acc[MT][NT];
    zero_acc(acc);

    // operand maps of v_mfma_f32_32x32x16_bf16: lane l holds A[row l & 31][depth 8 (l >> 5) + j] and B[depth][col l & 31], j < 8
    const int fr = lane & 31, fh = lane >> 5, fx = (fr >> 2) & 3;
    auto compute = [&](int buf) {
        const unsigned char *a = Gs + buf * BMO * ROWB + (wm * MT * 32 + fr) * ROWB;
        const unsigned char *b = Xs + buf * BNK * ROWB + (wn * NT * 32 + fr) * ROWB;
        bf16x8 fa[BP / 16][MT], fb[BP / 16][NT];
#pragma unroll
        for (int s = 0; s < BP / 16; ++s) {
            const int off = 16 * ((2 * s + fh) ^ fx);    // rows 32 apart share (row >> 2) & 3
#pragma unroll
            for (int i = 0; i < MT; ++i) fa[s][i] = *reinterpret_cast<const bf16x8 *>(a + i * 32 * ROWB + off);
#pragma unroll
            for (int j = 0; j < NT; ++j) fb[s][j] = *reinterpret_cast<const bf16x8 *>(b + j * 32 * ROWB + off);
        }
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int s = 0; s < BP / 16; ++s)
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[s][i], fb[s][j], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
    };

    const int nchunks = (m_end - m_begin + BP - 1) / BP;   // a split that ends with no rows writes a zero slab
    if (nchunks > 0) {
        load_chunk(m_begin);
        store_chunk(0);
    }
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const int buf = c & 1;
        if (c + 1 < nchunks) load_chunk(m_begin + (c + 1) * BP);   // global loads in flight while the matrix pipe works
        compute(buf);
        if (c + 1 < nchunks) store_chunk(buf ^ 1);
        __syncthreads();
    }

    // ---- bias partial [split][o]: the four pixel groups of a channel group meet in LDS, added in a fixed order
    if (do_bias) {                                       // (the loop ended with a barrier: the tiles are free)
        float4 *red = reinterpret_cast<float4 *>(smem_wb);
        if (is_g) red[tid] = bsum;
        __syncthreads();
        if (tid < BMO / 4 && o0 + 4 * tid < P.O) {
            float4 s = red[tid];
#pragma unroll
            for (int q = 1; q < 4; ++q) {
                const float4 v = red[q * (BMO / 4) + tid];
                s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
            }
            *reinterpret_cast<float4 *>(P.bias_ws + (size_t)split * P.O + o0 + 4 * tid) = s;
        }
    }

    // ---- partial tile -> slab [split][o][k]  (C/D map: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5))
    float *slab = P.ws + (size_t)split * P.O * P.K;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int k = k0 + (wn * NT + j) * 32 + fr;
        if (k >= P.K) continue;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int ob = o0 + (wm * MT + i) * 32 + 4 * fh;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = ob + (r & 3) + 8 * (r >> 2);
                if (o < P.O) slab[(size_t)o * P.K + k] = acc[i][j][r];
            }
        }
    }
}

template <int MT, int NT>
static int launch_wgrad_bf16_tile(const WgradBf16Params &P, int S, hipStream_t s) {
    constexpr int BMO = 64 * MT, BNK = 64 * NT;
    const size_t lds = (size_t)2 * (BMO + BNK) * wb16::ROWB;
    const unsigned nwg = (unsigned)(((P.K + BNK - 1) / BNK) * ((P.O + BMO - 1) / BMO) * S);
    hipLaunchKernelGGL((wgrad_bf16_kernel<MT, NT>), dim3(nwg), dim3(256), lds, s, P);
    return check_launch("wgrad_bf16_kernel");
}

// Every tile (o x k) once, in the order plan_wgrad_bf16 tries them
struct WgradBf16Tile { int bmo, bnk; int (*launch)(const WgradBf16Params &, int S, hipStream_t); };
static const WgradBf16Tile WGRAD_BF16_TILES[] = {
    {128, 128, launch_wgrad_bf16_tile<2, 2>},
    {64, 128, launch_wgrad_bf16_tile<1, 2>},
    {64, 64, launch_wgrad_bf16_tile<1, 1>},
};
constexpr int WGRAD_BF16_NTILES = sizeof(WGRAD_BF16_TILES) / sizeof(WgradBf16Tile);

WgradBf16Plan plan_wgrad_bf16(const vq2_conv_desc *d) {
    WgradBf16Plan p{};
    p.O = d->Co; p.I = d->Ci;
    p.K = d->KH * d->KW * d->Ci;
    p.M = d->N * d->H * d->W;
    // the tile that wastes the least padded work, the earlier (larger) one on ties
    long best = -1;
    for (int c = 0; c < WGRAD_BF16_NTILES; ++c) {
        const WgradBf16Tile &t = WGRAD_BF16_TILES[c];
        const long po = (p.O + t.bmo - 1) / t.bmo * t.bmo;
        const long pk = (p.K + t.bnk - 1) / t.bnk * t.bnk;
        if (best < 0 || po * pk < best) { best = po * pk; p.tile = c; }
    }
    p.bmo = WGRAD_BF16_TILES[p.tile].bmo; p.bnk = WGRAD_BF16_TILES[p.tile].bnk;
    // the split: two workgroups per CU are resident (__launch_bounds__(256, 2)); fill those 512 slots without a tail round,
    // with at least 8 chunks of 32 pixels per split
    const int tiles = ((p.K + p.bnk - 1) / p.bnk) * ((p.O + p.bmo - 1) / p.bmo);
    int S = 512 / tiles;
    const int max_s = (p.M + 255) / 256;
    if (S > max_s) S = max_s;
    if (S < 1) S = 1;
    int rps = (p.M + S - 1) / S;
    rps = (rps + wb16::BP - 1) / wb16::BP * wb16::BP;
    p.S = (p.M + rps - 1) / rps;
    p.rows_per_split = rps;
    return p;
}

int launch_wgrad_bf16(const WgradBf16Plan &p, const vq2_conv_desc *d, int relu_in, const float *x, const float *dy, float *ws,
                      float *bias_ws, hipStream_t s) {
    WgradBf16Params P{};
    P.x = x; P.g = dy; P.ws = ws; P.bias_ws = bias_ws;
    P.N = d->N; P.H = d->H; P.W = d->W; P.I = p.I; P.ldx = d->ldx; P.O = p.O; P.ldg = d->ldy;
    P.KH = d->KH; P.KW = d->KW; P.pad_h = d->pad_top; P.pad_w = d->pad_left;
    P.K = p.K; P.M = p.M; P.rows_per_split = p.rows_per_split; P.relu_x = relu_in;
    return WGRAD_BF16_TILES[p.tile].launch(P, p.S, s);
}

}  // namespace vq2
