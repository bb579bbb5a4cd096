// Elementwise kernels of the stage-2 GatedResBlock (pixelsnail.py:122-179): ELU, ELU followed by dropout in one pass,
// and the gate with its skip connection, GLU(t) + input, each with its backward.  Meant to be HBM-bound (their rates have
// not been measured on their own): every tensor crosses memory once, 16 bytes per lane (the second half of a GLU operand whose half width is no multiple of 4 goes dword by dword).
// Rows are NHWC pixels [pixels, C] with pixel strides; 64-bit indexing throughout; the pad lanes C .. ceil4(C) - 1 of every
// output are written as 0 whatever the input holds there.  No reductions and no atomics: results are bit-reproducible.
#include "vq2_common.h"
#include "vq2_philox.h"

namespace vq2 {

static inline int gated_grid(int64_t work_items) {
    const int64_t b = (work_items + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}
static inline int up4(int c) { return (c + 3) / 4 * 4; }

__device__ __forceinline__ float elu1(float x) { return x > 0.f ? x : expm1f(x); }
__device__ __forceinline__ float sigmoid1(float x) { return 1.f / (1.f + expf(-x)); }
// lanes c + i >= C become 0
__device__ __forceinline__ float4 real_lanes(float4 v, int c, int C) {
    if (c + 1 >= C) v.y = 0.f;
    if (c + 2 >= C) v.z = 0.f;
    if (c + 3 >= C) v.w = 0.f;
    return v;
}

// (pixel, first channel of the group) of work item t when a row has `groups` groups of 4 channels.  A 64-bit division is a long
// instruction sequence on this chip; launches of fewer than 2^31 items (every real one) divide in 32 bits.  `small` is uniform.
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

struct DropParams {
    uint32_t thr;               // keep iff word >= thr
    uint32_t seed_lo, seed_hi;
    float inv_keep;             // 1 / (1 - p)
    int on;                     // 0: no dropout (p == 0)
};

// keep decisions of the four elements e .. e + 3 (flat indices of the unpadded tensor): word (e' & 3) of the Philox block
// e' >> 2.  e % 4 == 0 (every row of a tensor with C % 4 == 0) needs one block, anything else two.
__device__ __forceinline__ void keep4(const DropParams &D, int64_t e, bool keep[4]) {
    const uint64_t q = (uint64_t)e >> 2;
    const int r = (int)(e & 3);
    const uint4 a = philox4x32_7((uint32_t)q, (uint32_t)(q >> 32), 0u, 0u, D.seed_lo, D.seed_hi);
    uint32_t w[8] = {a.x, a.y, a.z, a.w, 0u, 0u, 0u, 0u};
    if (r) {
        const uint4 b = philox4x32_7((uint32_t)(q + 1), (uint32_t)((q + 1) >> 32), 0u, 0u, D.seed_lo, D.seed_hi);
        w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t v = w[i];                    // w[r + i] without a dynamically indexed register array
        if (r == 1) v = w[i + 1];
        if (r == 2) v = w[i + 2];
        if (r == 3) v = w[i + 3];
        keep[i] = v >= D.thr;
    }
}

// y = [keep / (1 - p) *] ELU(x)
__global__ __launch_bounds__(256) void elu_fwd_kernel(const float *__restrict__ x, int ldx, float *__restrict__ y, int ldy,
                                                      int64_t pixels, int C, const DropParams D) {
    const int C4 = (C + 3) / 4;
    const int64_t total = pixels * C4;
    const bool small = total < ((int64_t)1 << 31);
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        int64_t p;
        int c;
        split_item(t, C4, small, p, c);
        const float4 v = *reinterpret_cast<const float4 *>(x + p * ldx + c);
        float4 o = make_float4(elu1(v.x), elu1(v.y), elu1(v.z), elu1(v.w));
        if (D.on) {
            bool k[4];
            keep4(D, p * C + c, k);
            o.x = k[0] ? o.x * D.inv_keep : 0.f; o.y = k[1] ? o.y * D.inv_keep : 0.f;
            o.z = k[2] ? o.z * D.inv_keep : 0.f; o.w = k[3] ? o.w * D.inv_keep : 0.f;
        }
        *reinterpret_cast<float4 *>(y + p * ldy + c) = real_lanes(o, c, C);
    }
}

// FROM_Y: dx = dy * (y > 0 ? 1 : y + 1), `src` is the forward output (plain ELU)
// else:   dx = dy * keep / (1 - p) * (x > 0 ? 1 : exp(x)), `src` is the forward input (ELU + dropout)
template <bool FROM_Y>
__global__ __launch_bounds__(256) void elu_bwd_kernel(const float *__restrict__ dy, int lddy, const float *__restrict__ src,
                                                      int lds, float *__restrict__ dx, int lddx, int64_t pixels, int C,
                                                      const DropParams D) {
    const int C4 = (C + 3) / 4;
    const int64_t total = pixels * C4;
    const bool small = total < ((int64_t)1 << 31);
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        int64_t p;
        int c;
        split_item(t, C4, small, p, c);
        const float4 g = *reinterpret_cast<const float4 *>(dy + p * lddy + c);
        const float4 s = *reinterpret_cast<const float4 *>(src + p * lds + c);
        float4 o;
        if (FROM_Y) {
            o.x = g.x * (s.x > 0.f ? 1.f : s.x + 1.f); o.y = g.y * (s.y > 0.f ? 1.f : s.y + 1.f);
            o.z = g.z * (s.z > 0.f ? 1.f : s.z + 1.f); o.w = g.w * (s.w > 0.f ? 1.f : s.w + 1.f);
        } else {
            o.x = g.x * (s.x > 0.f ? 1.f : expf(s.x)); o.y = g.y * (s.y > 0.f ? 1.f : expf(s.y));
            o.z = g.z * (s.z > 0.f ? 1.f : expf(s.z)); o.w = g.w * (s.w > 0.f ? 1.f : expf(s.w));
            if (D.on) {
                bool k[4];
                keep4(D, p * C + c, k);
                o.x = k[0] ? o.x * D.inv_keep : 0.f; o.y = k[1] ? o.y * D.inv_keep : 0.f;
                o.z = k[2] ? o.z * D.inv_keep : 0.f; o.w = k[3] ? o.w * D.inv_keep : 0.f;
            }
        }
        *reinterpret_cast<float4 *>(dx + p * lddx + c) = real_lanes(o, c, C);
    }
}

__global__ __launch_bounds__(256) void dropout_keep_mask_kernel(uint8_t *__restrict__ mask, int64_t total, const DropParams D) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const uint64_t q = (uint64_t)e >> 2;
        const uint4 a = philox4x32_7((uint32_t)q, (uint32_t)(q >> 32), 0u, 0u, D.seed_lo, D.seed_hi);
        const int r = (int)(e & 3);
        const uint32_t w = r == 0 ? a.x : r == 1 ? a.y : r == 2 ? a.z : a.w;
        mask[e] = w >= D.thr ? 1 : 0;
    }
}

// out[c] = a[c] * sigmoid(b[c]) + res[c];  a = t[c], b = t[Ch + c].  ALIGNED: Ch % 4 == 0, b is read as float4.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void glu_res_fwd_kernel(const float *__restrict__ t, int ldt, const float *__restrict__ res,
                                                          int ldres, float *__restrict__ out, int ldo, int64_t pixels, int Ch) {
    const int G = (Ch + 3) / 4;
    const int64_t total = pixels * G;
    const bool small = total < ((int64_t)1 << 31);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        int64_t p;
        int c;
        split_item(i, G, small, p, c);
        const float *row = t + p * ldt;
        const float4 a = *reinterpret_cast<const float4 *>(row + c);
        float4 b;
        if (ALIGNED) {
            b = *reinterpret_cast<const float4 *>(row + Ch + c);
        } else {
            b.x = row[Ch + c];
            b.y = c + 1 < Ch ? row[Ch + c + 1] : 0.f;
            b.z = c + 2 < Ch ? row[Ch + c + 2] : 0.f;
            b.w = c + 3 < Ch ? row[Ch + c + 3] : 0.f;
        }
        const float4 r = *reinterpret_cast<const float4 *>(res + p * ldres + c);
        float4 o;
        o.x = a.x * sigmoid1(b.x) + r.x; o.y = a.y * sigmoid1(b.y) + r.y;
        o.z = a.z * sigmoid1(b.z) + r.z; o.w = a.w * sigmoid1(b.w) + r.w;
        *reinterpret_cast<float4 *>(out + p * ldo + c) = real_lanes(o, c, Ch);
    }
}

// dt[c] = dout[c] * s, dt[Ch + c] = dout[c] * a * s * (1 - s), s = sigmoid(b); lanes 2 Ch .. ceil4(2 Ch) - 1 of dt = 0
template <bool ALIGNED>
__global__ __launch_bounds__(256) void glu_res_bwd_kernel(const float *__restrict__ dout, int lddo, const float *__restrict__ t,
                                                          int ldt, float *__restrict__ dt, int lddt, int64_t pixels, int Ch) {
    const int G = (Ch + 3) / 4;
    const int64_t total = pixels * G;
    const bool small = total < ((int64_t)1 << 31);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        int64_t p;
        int c;
        split_item(i, G, small, p, c);
        const float *row = t + p * ldt;
        float *drow = dt + p * lddt;
        const float4 g = *reinterpret_cast<const float4 *>(dout + p * lddo + c);
        const float4 a = *reinterpret_cast<const float4 *>(row + c);
        if (ALIGNED) {
            const float4 b = *reinterpret_cast<const float4 *>(row + Ch + c);
            const float4 s = make_float4(sigmoid1(b.x), sigmoid1(b.y), sigmoid1(b.z), sigmoid1(b.w));
            *reinterpret_cast<float4 *>(drow + c) = make_float4(g.x * s.x, g.y * s.y, g.z * s.z, g.w * s.w);
            *reinterpret_cast<float4 *>(drow + Ch + c) =
                make_float4(g.x * a.x * s.x * (1.f - s.x), g.y * a.y * s.y * (1.f - s.y), g.z * a.z * s.z * (1.f - s.z),
                            g.w * a.w * s.w * (1.f - s.w));
        } else {
            const float gv[4] = {g.x, g.y, g.z, g.w}, av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (c + k < Ch) {
                    const float s = sigmoid1(row[Ch + c + k]);
                    drow[c + k] = gv[k] * s;
                    drow[Ch + c + k] = gv[k] * av[k] * s * (1.f - s);
                }
            if (c == 0)
                for (int k = 2 * Ch; k < (2 * Ch + 3) / 4 * 4; ++k) drow[k] = 0.f;
        }
    }
}

// ------------------------------------------------------------------ the class label in the gate: [a | b] = t + E[label[image]]
// The row of E that pixel p adds to its t, or nullptr: image p / ppi's label is looked at before any address is formed from
// it, and one outside [0, n_label) adds nothing.  `small` (uniform): p and ppi fit 32 bits, as in split_item.
__device__ __forceinline__ const float *label_row(const float *__restrict__ embed, int lde, const int64_t *__restrict__ label,
                                                  int64_t p, int64_t ppi, bool small, int n_label) {
    const int64_t img = small ? (int64_t)((uint32_t)p / (uint32_t)ppi) : p / ppi;
    const int64_t l = label[img];
    return l >= 0 && l < (int64_t)n_label ? embed + l * lde : nullptr;
}

// a and b of group c with the label's row added in registers (t in memory stays the conv output).  ALIGNED: Ch % 4 == 0, the
// second half of t and both halves of the row are read as float4; else they go dword by dword, lanes >= Ch left 0.
template <bool ALIGNED>
__device__ __forceinline__ void gate_operands(const float *__restrict__ row, const float *__restrict__ e, int c, int Ch, float4 &a,
                                              float4 &b) {
    a = *reinterpret_cast<const float4 *>(row + c);
    if (ALIGNED) {
        b = *reinterpret_cast<const float4 *>(row + Ch + c);
        if (e) {
            const float4 ea = *reinterpret_cast<const float4 *>(e + c), eb = *reinterpret_cast<const float4 *>(e + Ch + c);
            a.x += ea.x; a.y += ea.y; a.z += ea.z; a.w += ea.w;
            b.x += eb.x; b.y += eb.y; b.z += eb.z; b.w += eb.w;
        }
    } else {
        b.x = row[Ch + c];
        b.y = c + 1 < Ch ? row[Ch + c + 1] : 0.f;
        b.z = c + 2 < Ch ? row[Ch + c + 2] : 0.f;
        b.w = c + 3 < Ch ? row[Ch + c + 3] : 0.f;
        if (e) {
            a.x += e[c]; b.x += e[Ch + c];
            if (c + 1 < Ch) { a.y += e[c + 1]; b.y += e[Ch + c + 1]; }
            if (c + 2 < Ch) { a.z += e[c + 2]; b.z += e[Ch + c + 2]; }
            if (c + 3 < Ch) { a.w += e[c + 3]; b.w += e[Ch + c + 3]; }
        }
    }
}

// glu_res_fwd_kernel with the label's row added to t in registers
template <bool ALIGNED>
__global__ __launch_bounds__(256) void glu_res_label_fwd_kernel(const float *__restrict__ t, int ldt, const float *__restrict__ res,
                                                                int ldres, const float *__restrict__ embed, int lde,
                                                                const int64_t *__restrict__ label, int64_t ppi,
                                                                float *__restrict__ out, int ldo, int64_t pixels, int Ch,
                                                                int n_label) {
    const int G = (Ch + 3) / 4;
    const int64_t total = pixels * G;
    const bool small = total < ((int64_t)1 << 31);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        int64_t p;
        int c;
        split_item(i, G, small, p, c);
        float4 a, b;
        gate_operands<ALIGNED>(t + p * ldt, label_row(embed, lde, label, p, ppi, small, n_label), c, Ch, a, b);
        const float4 r = *reinterpret_cast<const float4 *>(res + p * ldres + c);
        float4 o;
        o.x = a.x * sigmoid1(b.x) + r.x; o.y = a.y * sigmoid1(b.y) + r.y;
        o.z = a.z * sigmoid1(b.z) + r.z; o.w = a.w * sigmoid1(b.w) + r.w;
        *reinterpret_cast<float4 *>(out + p * ldo + c) = real_lanes(o, c, Ch);
    }
}

// glu_res_bwd_kernel with the label's row added to a and b before the sigmoid; dt as there
template <bool ALIGNED>
__global__ __launch_bounds__(256) void glu_res_label_bwd_kernel(const float *__restrict__ dout, int lddo, const float *__restrict__ t,
                                                                int ldt, const float *__restrict__ embed, int lde,
                                                                const int64_t *__restrict__ label, int64_t ppi,
                                                                float *__restrict__ dt, int lddt, int64_t pixels, int Ch,
                                                                int n_label) {
    const int G = (Ch + 3) / 4;
    const int64_t total = pixels * G;
    const bool small = total < ((int64_t)1 << 31);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        int64_t p;
        int c;
        split_item(i, G, small, p, c);
        float *drow = dt + p * lddt;
        const float4 g = *reinterpret_cast<const float4 *>(dout + p * lddo + c);
        float4 a, b;
        gate_operands<ALIGNED>(t + p * ldt, label_row(embed, lde, label, p, ppi, small, n_label), c, Ch, a, b);
        const float4 s = make_float4(sigmoid1(b.x), sigmoid1(b.y), sigmoid1(b.z), sigmoid1(b.w));
        const float4 da = make_float4(g.x * s.x, g.y * s.y, g.z * s.z, g.w * s.w);
        const float4 db = make_float4(g.x * a.x * s.x * (1.f - s.x), g.y * a.y * s.y * (1.f - s.y), g.z * a.z * s.z * (1.f - s.z),
                                      g.w * a.w * s.w * (1.f - s.w));
        if (ALIGNED) {
            *reinterpret_cast<float4 *>(drow + c) = da;
            *reinterpret_cast<float4 *>(drow + Ch + c) = db;
        } else {
            const float dav[4] = {da.x, da.y, da.z, da.w}, dbv[4] = {db.x, db.y, db.z, db.w};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (c + k < Ch) {
                    drow[c + k] = dav[k];
                    drow[Ch + c + k] = dbv[k];
                }
            if (c == 0)
                for (int k = 2 * Ch; k < (2 * Ch + 3) / 4 * 4; ++k) drow[k] = 0.f;
        }
    }
}

// dE, first pass: the column sums of one image's pixels r0 .. r1 - 1 of dt, the split of colsum_partial_kernel (vq2_wgrad.hip)
// per image: thread (rg, c4) adds rows r0 + rg, r0 + rg + nrg, ... of one 16-byte group, the row groups are then added in
// ascending order through LDS.  part [images][nsplit][4 * C4].  Lanes C2 .. 4 * C4 - 1 of dt are read and their sums never used.
constexpr int LG_MAX_SPLIT = 32;
constexpr int LG_MIN_ROWS = 64;

static inline int64_t lg_rows_per_block(int64_t ppi) {
    const int64_t rpb = (ppi + LG_MAX_SPLIT - 1) / LG_MAX_SPLIT;
    return rpb < LG_MIN_ROWS ? LG_MIN_ROWS : rpb;
}
static inline int lg_row_groups(int C4) { return 256 / C4 > 0 ? 256 / C4 : 1; }

__global__ __launch_bounds__(256) void label_grad_partial_kernel(const float *__restrict__ dt, int lddt, int64_t ppi, int64_t rpb,
                                                                 int nsplit, int C4, float *__restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float red[];  // [nrg][4 * C4]
    const int Cp = 4 * C4;
    const int tc = C4 < 256 ? C4 : 256;                          // threads along the channel groups
    const int nrg = 256 / C4 > 0 ? 256 / C4 : 1;
    const int64_t img = blockIdx.x / nsplit;
    const int64_t r0 = (int64_t)(blockIdx.x % nsplit) * rpb;
    const int64_t r1 = r0 + rpb < ppi ? r0 + rpb : ppi;
    const float *x = dt + img * ppi * lddt;
    for (int cbase = 0; cbase < C4; cbase += 256) {
        const int c4 = cbase + (int)(threadIdx.x % tc);
        const int rg = threadIdx.x / tc;
        if (rg < nrg && c4 < C4) {
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int64_t r = r0 + rg; r < r1; r += nrg) {
                const float4 v = *reinterpret_cast<const float4 *>(x + r * lddt + c4 * 4);
                a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
            }
            *reinterpret_cast<float4 *>(red + (size_t)rg * Cp + c4 * 4) = a;
        }
        __syncthreads();
        const int c1 = (cbase + 256 < C4 ? cbase + 256 : C4) * 4;
        for (int c = cbase * 4 + threadIdx.x; c < c1; c += 256) {
            float s = 0.f;
            for (int g = 0; g < nrg; ++g) s += red[(size_t)g * Cp + c];
            part[(size_t)blockIdx.x * Cp + c] = s;
        }
        __syncthreads();
    }
}

// dE, second pass: one workgroup per (label row, 256 columns).  Images ascending; an image's splits are added first, then the
// image to the row.  A row no image names is written 0; a label outside [0, n_label) matches no row.
__global__ __launch_bounds__(256) void label_grad_rows_kernel(const float *__restrict__ part, const int64_t *__restrict__ label,
                                                              int images, int nsplit, int Cp, int C2, float *__restrict__ dE) {
    const int64_t l = blockIdx.x;
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= C2) return;
    float acc = 0.f;
    for (int b = 0; b < images; ++b) {
        if (label[b] != l) continue;
        const float *src = part + (size_t)b * nsplit * Cp + c;
        float s = src[0];
        for (int k = 1; k < nsplit; ++k) s += src[(size_t)k * Cp];
        acc += s;
    }
    dE[(size_t)l * C2 + c] = acc;
}

static int rows_ok(const char *what, const void *ptr, int ld, int C) {
    VQ2_REQUIRE(ld % 4 == 0 && ld >= up4(C), "%s: pixel stride %d must be a multiple of 4 and >= ceil4(%d)", what, ld, C);
    VQ2_REQUIRE(ptr != nullptr, "%s: null pointer", what);
    VQ2_REQUIRE(aligned16(ptr), "%s: pointers must be 16-byte aligned", what);
    return VQ2_OK;
}

static int drop_params(const char *what, float p, uint64_t seed, DropParams &D) {
    VQ2_REQUIRE(p >= 0.f && p < 1.f, "%s: dropout probability must be in [0, 1)", what);
    D.on = p > 0.f;
    D.thr = (uint32_t)((double)p * 4294967296.0);
    D.inv_keep = (float)(1.0 / (1.0 - (double)p));
    D.seed_lo = (uint32_t)seed; D.seed_hi = (uint32_t)(seed >> 32);
    return VQ2_OK;
}

static int shape_ok(const char *what, int64_t pixels, int C) {
    VQ2_REQUIRE(pixels > 0 && C > 0 && C <= (1 << 24) && pixels < ((int64_t)1 << 36), "%s: bad shape", what);
    return VQ2_OK;
}

// the label operands of the two gate kernels: pixels = images * pixels_per_image, E [n_label, 2 * Ch] with rows lde apart
static int labels_ok(const char *what, const void *embed, int lde, const void *label, int64_t images, int64_t ppi, int64_t pixels,
                     int Ch, int n_label) {
    VQ2_REQUIRE(embed != nullptr && label != nullptr, "%s: null pointer", what);
    VQ2_REQUIRE(images > 0 && ppi > 0 && images <= pixels && ppi <= pixels && images * ppi == pixels,
                "%s: pixels must be images * pixels_per_image", what);
    VQ2_REQUIRE(n_label > 0 && lde >= 2 * Ch, "%s: the label table needs n_label > 0 and a row stride >= 2 * Ch", what);
    VQ2_REQUIRE(((uintptr_t)label & 7) == 0, "%s: label must be 8-byte aligned", what);
    if (Ch % 4 == 0)
        VQ2_REQUIRE(lde % 4 == 0 && aligned16(embed), "%s: with Ch %% 4 == 0 the label table is read 16 bytes at a time", what);
    return VQ2_OK;
}

}  // namespace vq2

using namespace vq2;

extern "C" int vq2_elu_dropout_fwd(const float *x, int32_t ldx, float *y, int32_t ldy, int64_t pixels, int32_t C, float p,
                                   uint64_t seed, vq2_stream_t stream) {
    if (int e = shape_ok("elu_fwd", pixels, C)) return e;
    DropParams D;
    if (int e = drop_params("elu_fwd", p, seed, D)) return e;
    if (int e = rows_ok("elu_fwd", x, ldx, C)) return e;
    if (int e = rows_ok("elu_fwd", y, ldy, C)) return e;
    hipLaunchKernelGGL(elu_fwd_kernel, dim3(gated_grid(pixels * (up4(C) / 4))), dim3(256), 0, to_stream(stream), x, ldx, y,
                       ldy, pixels, C, D);
    return check_launch("elu_fwd_kernel");
}

extern "C" int vq2_elu_fwd(const float *x, int32_t ldx, float *y, int32_t ldy, int64_t pixels, int32_t C,
                           vq2_stream_t stream) {
    return vq2_elu_dropout_fwd(x, ldx, y, ldy, pixels, C, 0.f, 0, stream);
}

extern "C" int vq2_elu_bwd(const float *dy, int32_t lddy, const float *y, int32_t ldy, float *dx, int32_t lddx,
                           int64_t pixels, int32_t C, vq2_stream_t stream) {
    if (int e = shape_ok("elu_bwd", pixels, C)) return e;
    if (int e = rows_ok("elu_bwd", dy, lddy, C)) return e;
    if (int e = rows_ok("elu_bwd", y, ldy, C)) return e;
    if (int e = rows_ok("elu_bwd", dx, lddx, C)) return e;
    DropParams D{};
    hipLaunchKernelGGL(elu_bwd_kernel<true>, dim3(gated_grid(pixels * (up4(C) / 4))), dim3(256), 0, to_stream(stream), dy,
                       lddy, y, ldy, dx, lddx, pixels, C, D);
    return check_launch("elu_bwd_kernel");
}

extern "C" int vq2_elu_dropout_bwd(const float *dy, int32_t lddy, const float *x, int32_t ldx, float *dx, int32_t lddx,
                                   int64_t pixels, int32_t C, float p, uint64_t seed, vq2_stream_t stream) {
    if (int e = shape_ok("elu_dropout_bwd", pixels, C)) return e;
    DropParams D;
    if (int e = drop_params("elu_dropout_bwd", p, seed, D)) return e;
    if (int e = rows_ok("elu_dropout_bwd", dy, lddy, C)) return e;
    if (int e = rows_ok("elu_dropout_bwd", x, ldx, C)) return e;
    if (int e = rows_ok("elu_dropout_bwd", dx, lddx, C)) return e;
    hipLaunchKernelGGL(elu_bwd_kernel<false>, dim3(gated_grid(pixels * (up4(C) / 4))), dim3(256), 0, to_stream(stream), dy,
                       lddy, x, ldx, dx, lddx, pixels, C, D);
    return check_launch("elu_dropout_bwd_kernel");
}

extern "C" int vq2_dropout_keep_mask(uint8_t *mask, int64_t pixels, int32_t C, float p, uint64_t seed, vq2_stream_t stream) {
    if (int e = shape_ok("dropout_keep_mask", pixels, C)) return e;
    VQ2_REQUIRE(mask != nullptr, "dropout_keep_mask: null pointer");
    DropParams D;
    if (int e = drop_params("dropout_keep_mask", p, seed, D)) return e;
    const int64_t total = pixels * C;
    hipLaunchKernelGGL(dropout_keep_mask_kernel, dim3(gated_grid(total)), dim3(256), 0, to_stream(stream), mask, total, D);
    return check_launch("dropout_keep_mask_kernel");
}

extern "C" int vq2_glu_res_fwd(const float *t, int32_t ldt, const float *res, int32_t ldres, float *out, int32_t ldo,
                               int64_t pixels, int32_t Ch, vq2_stream_t stream) {
    if (int e = shape_ok("glu_res_fwd", pixels, Ch)) return e;
    if (int e = rows_ok("glu_res_fwd", t, ldt, 2 * Ch)) return e;
    if (int e = rows_ok("glu_res_fwd", res, ldres, Ch)) return e;
    if (int e = rows_ok("glu_res_fwd", out, ldo, Ch)) return e;
    const dim3 grid(gated_grid(pixels * (up4(Ch) / 4)));
    if (Ch % 4 == 0)
        hipLaunchKernelGGL(glu_res_fwd_kernel<true>, grid, dim3(256), 0, to_stream(stream), t, ldt, res, ldres, out, ldo, pixels, Ch);
    else
        hipLaunchKernelGGL(glu_res_fwd_kernel<false>, grid, dim3(256), 0, to_stream(stream), t, ldt, res, ldres, out, ldo, pixels, Ch);
    return check_launch("glu_res_fwd_kernel");
}

extern "C" int vq2_glu_res_bwd(const float *dout, int32_t lddo, const float *t, int32_t ldt, float *dt, int32_t lddt,
                               int64_t pixels, int32_t Ch, vq2_stream_t stream) {
    if (int e = shape_ok("glu_res_bwd", pixels, Ch)) return e;
    if (int e = rows_ok("glu_res_bwd", dout, lddo, Ch)) return e;
    if (int e = rows_ok("glu_res_bwd", t, ldt, 2 * Ch)) return e;
    if (int e = rows_ok("glu_res_bwd", dt, lddt, 2 * Ch)) return e;
    const dim3 grid(gated_grid(pixels * (up4(Ch) / 4)));
    if (Ch % 4 == 0)
        hipLaunchKernelGGL(glu_res_bwd_kernel<true>, grid, dim3(256), 0, to_stream(stream), dout, lddo, t, ldt, dt, lddt, pixels, Ch);
    else
        hipLaunchKernelGGL(glu_res_bwd_kernel<false>, grid, dim3(256), 0, to_stream(stream), dout, lddo, t, ldt, dt, lddt, pixels, Ch);
    return check_launch("glu_res_bwd_kernel");
}

extern "C" int vq2_glu_res_label_fwd(const float *t, int32_t ldt, const float *res, int32_t ldres, const float *embed, int32_t lde,
                                     const int64_t *label, int64_t images, int64_t pixels_per_image, float *out, int32_t ldo,
                                     int64_t pixels, int32_t Ch, int32_t n_label, vq2_stream_t stream) {
    if (int e = shape_ok("glu_res_label_fwd", pixels, Ch)) return e;
    if (int e = rows_ok("glu_res_label_fwd", t, ldt, 2 * Ch)) return e;
    if (int e = rows_ok("glu_res_label_fwd", res, ldres, Ch)) return e;
    if (int e = rows_ok("glu_res_label_fwd", out, ldo, Ch)) return e;
    if (int e = labels_ok("glu_res_label_fwd", embed, lde, label, images, pixels_per_image, pixels, Ch, n_label)) return e;
    const dim3 grid(gated_grid(pixels * (up4(Ch) / 4)));
    if (Ch % 4 == 0)
        hipLaunchKernelGGL(glu_res_label_fwd_kernel<true>, grid, dim3(256), 0, to_stream(stream), t, ldt, res, ldres, embed, lde,
                           label, pixels_per_image, out, ldo, pixels, Ch, n_label);
    else
        hipLaunchKernelGGL(glu_res_label_fwd_kernel<false>, grid, dim3(256), 0, to_stream(stream), t, ldt, res, ldres, embed, lde,
                           label, pixels_per_image, out, ldo, pixels, Ch, n_label);
    return check_launch("glu_res_label_fwd_kernel");
}

extern "C" int vq2_glu_res_label_bwd(const float *dout, int32_t lddo, const float *t, int32_t ldt, const float *embed, int32_t lde,
                                     const int64_t *label, int64_t images, int64_t pixels_per_image, float *dt, int32_t lddt,
                                     int64_t pixels, int32_t Ch, int32_t n_label, vq2_stream_t stream) {
    if (int e = shape_ok("glu_res_label_bwd", pixels, Ch)) return e;
    if (int e = rows_ok("glu_res_label_bwd", dout, lddo, Ch)) return e;
    if (int e = rows_ok("glu_res_label_bwd", t, ldt, 2 * Ch)) return e;
    if (int e = rows_ok("glu_res_label_bwd", dt, lddt, 2 * Ch)) return e;
    if (int e = labels_ok("glu_res_label_bwd", embed, lde, label, images, pixels_per_image, pixels, Ch, n_label)) return e;
    const dim3 grid(gated_grid(pixels * (up4(Ch) / 4)));
    if (Ch % 4 == 0)
        hipLaunchKernelGGL(glu_res_label_bwd_kernel<true>, grid, dim3(256), 0, to_stream(stream), dout, lddo, t, ldt, embed, lde,
                           label, pixels_per_image, dt, lddt, pixels, Ch, n_label);
    else
        hipLaunchKernelGGL(glu_res_label_bwd_kernel<false>, grid, dim3(256), 0, to_stream(stream), dout, lddo, t, ldt, embed, lde,
                           label, pixels_per_image, dt, lddt, pixels, Ch, n_label);
    return check_launch("glu_res_label_bwd_kernel");
}

// images <= 2^16, C2 <= 8192 (one row of partial sums per row group fits the LDS of a launch), n_label <= 2^24
static bool label_grad_shape(int64_t images, int64_t ppi, int32_t C2, int32_t n_label) {
    return images > 0 && images <= (1 << 16) && ppi > 0 && ppi < ((int64_t)1 << 36) / images && C2 > 0 && C2 <= 8192 &&
           n_label > 0 && n_label <= (1 << 24);
}

extern "C" size_t vq2_label_embed_grad_workspace_bytes(int64_t images, int64_t pixels_per_image, int32_t C2) {
    if (!label_grad_shape(images, pixels_per_image, C2, 1)) return 0;
    const int64_t rpb = lg_rows_per_block(pixels_per_image);
    return (size_t)(images * ((pixels_per_image + rpb - 1) / rpb)) * up4(C2) * sizeof(float);
}

extern "C" int vq2_label_embed_grad(const float *dt, int32_t lddt, const int64_t *label, int64_t images, int64_t pixels_per_image,
                                    int32_t C2, int32_t n_label, float *dE, void *ws, size_t ws_bytes, vq2_stream_t stream) {
    VQ2_REQUIRE(label_grad_shape(images, pixels_per_image, C2, n_label), "label_embed_grad: bad shape");
    if (int e = rows_ok("label_embed_grad", dt, lddt, C2)) return e;
    VQ2_REQUIRE(label && dE && ws, "label_embed_grad: null pointer");
    VQ2_REQUIRE(((uintptr_t)label & 7) == 0 && aligned16(ws), "label_embed_grad: label must be 8-byte, ws 16-byte aligned");
    VQ2_REQUIRE(ws_bytes >= vq2_label_embed_grad_workspace_bytes(images, pixels_per_image, C2),
                "label_embed_grad: workspace too small");
    const int64_t rpb = lg_rows_per_block(pixels_per_image);
    const int nsplit = (int)((pixels_per_image + rpb - 1) / rpb);
    const int C4 = up4(C2) / 4;
    float *part = static_cast<float *>(ws);
    hipStream_t s = to_stream(stream);
    hipLaunchKernelGGL(label_grad_partial_kernel, dim3((unsigned)(images * nsplit)), dim3(256),
                       (size_t)lg_row_groups(C4) * 4 * C4 * sizeof(float), s, dt, lddt, pixels_per_image, rpb, nsplit, C4, part);
    if (int e = check_launch("label_grad_partial_kernel")) return e;
    hipLaunchKernelGGL(label_grad_rows_kernel, dim3((unsigned)n_label, (unsigned)((C2 + 255) / 256)), dim3(256), 0, s, part, label,
                       (int)images, nsplit, 4 * C4, C2, dE);
    return check_launch("label_grad_rows_kernel");
}
