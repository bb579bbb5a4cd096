"""CPU statement of the dead-code restart rule: Philox4x32-7 in plain Python integers, the draw of a
candidate row per code, and the whole EMA update with restarts in numpy -- every fp32 step an np.float32 operation in
the kernels' own order, so codebooks can be compared bit for bit; the normalisation also in float64 for tolerance
checks.  Shared by tests/test_code_restart_cpu.py and the GPU tests."""
import numpy as np

M32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85


def philox4x32_7(counter, key):
    """counter: four 32-bit words, key: two -> four 32-bit words (Salmon et al. 2011, seven rounds)."""
    c0, c1, c2, c3 = (int(c) & M32 for c in counter)
    k0, k1 = (int(k) & M32 for k in key)
    for _ in range(7):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def draw(seed, step, slot, k, m_total):
    """Global row r in [0, m_total) of code k's candidate: word 0 of Philox at counter (k, lo32(step), hi32(step), slot),
    key = the 64-bit seed, scaled by a 32 x 32 -> high-32 multiply."""
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_7((k, step & M32, step >> 32, slot), (seed & M32, seed >> 32))[0]
    return (w * int(m_total)) >> 32


def picks(seed, step, slot, n_codes, m_total):
    return np.array([draw(seed, step, slot, k, m_total) for k in range(n_codes)], dtype=np.int64)


def candidates(x, pk, rank=0, world=1):
    """cand [K, D] as rank `rank` of `world` writes it from its own rows x [M, D]: the picked row where it owns it, else
    zeros."""
    m = x.shape[0]
    cand = np.zeros((len(pk), x.shape[1]), dtype=np.float32)
    mine = (pk // m) == rank
    cand[mine] = x[pk[mine] % m]
    return cand


def fma32(a, b, c):
    """fl32(a * b + c) for fp32 a, b, c: the product is exact in float64, the sum is formed there and rounded once."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def kernel_sum(cs):
    """sum_k cs[k] in the order of the one-workgroup counts kernel: thread t adds k = t, t + 1024, ... in turn, then a
    halving tree over the 1024 partial sums."""
    part = np.zeros(1024, dtype=np.float32)
    for j in range(0, len(cs), 1024):
        chunk = cs[j:j + 1024]
        part[:len(chunk)] = part[:len(chunk)] + chunk
    o = 512
    while o:
        part[:o] = part[:o] + part[o:2 * o]
        o //= 2
    return part[0]


def ema_update_restart(embed, cluster_size, embed_avg, counts, sums_t, cand, decay, eps, threshold):
    """The rule, steps 1-6, on numpy fp32 arrays: embed / embed_avg [D, K], cluster_size / counts [K], sums_t / cand
    [K, D].  `threshold` is the effective one (0 before `start`).  Returns a dict of the new embed, cluster_size,
    embed_avg, the dead mask, n, and embed64: the normalisation of the fp32 embed_avg / cluster_size in float64."""
    f32 = np.float32
    d, k = embed.shape
    dec, alpha, eps32, thr = f32(decay), f32(1.0 - decay), f32(eps), f32(threshold)
    keps = f32(float(k) * eps)
    cs = fma32(alpha, counts, cluster_size * dec)
    dead = (cs < thr) & np.isfinite(cand).all(axis=1)
    ea = fma32(alpha, sums_t.T, embed_avg * dec)
    cs = np.where(dead, thr, cs).astype(f32)
    ea[:, dead] = (thr * cand[dead]).T
    n = kernel_sum(cs)
    denom = f32(n + keps)
    size = ((cs + eps32) / denom * n).astype(f32)
    new_embed = (ea / size[None, :]).astype(f32)
    n64 = cs.astype(np.float64).sum()
    size64 = (cs.astype(np.float64) + float(eps)) / (n64 + k * float(eps)) * n64
    return {"embed": new_embed, "cluster_size": cs, "embed_avg": ea.astype(f32), "dead": dead, "n": n,
            "embed64": ea.astype(np.float64) / size64[None, :]}


def plain_ema_update(embed, cluster_size, embed_avg, counts, sums_t, decay, eps):
    """The update without restarts, written on its own (not as threshold = 0 of the function above)."""
    f32 = np.float32
    d, k = embed.shape
    dec, alpha, eps32 = f32(decay), f32(1.0 - decay), f32(eps)
    cs = fma32(alpha, counts, cluster_size * dec)
    ea = fma32(alpha, sums_t.T, embed_avg * dec)
    n = kernel_sum(cs)
    size = ((cs + eps32) / f32(n + f32(float(k) * eps)) * n).astype(f32)
    return {"embed": (ea / size[None, :]).astype(f32), "cluster_size": cs, "embed_avg": ea}


def prepared(embed):
    """(embedT, enorm) in vq_prepare_kernel's order: four chains over d = g, g + 4, ..., then (p0 + p1) + (p2 + p3)."""
    d, k = embed.shape
    sq = (embed * embed).astype(np.float32)
    part = np.zeros((4, k), dtype=np.float32)
    for dd in range(d):
        part[dd % 4] = part[dd % 4] + sq[dd]
    return np.ascontiguousarray(embed.T), (part[0] + part[1]) + (part[2] + part[3])
