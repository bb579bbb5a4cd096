"""The truncated draw of vq2_sample_filtered stated in numpy, for z = l / temperature in float64 or float32.

    top-k   v_k is the k-th largest z counting multiplicity, K = {c : z_c >= v_k} (ties at the k-th value kept); 0: off
    top-p   on K, with e_c = exp(z_c - max z): t* is the largest value among {z_c : c in K} whose upper set
            {c in K : z_c >= t*} holds at least top_p of the mass of K; that upper set is kept; 1: off
    draw    the smallest kept class, in ascending class order, whose running sum of kept probabilities exceeds u; the
            last kept class if rounding leaves none

kept_mask() works on thresholds (no sort of the row); kept_mask_by_sorting() is the plain definition -- sort descending, take
the shortest prefix that satisfies the rule, close it over ties -- and the CPU test holds one against the other."""
import numpy as np


def _mass_at_or_above(z, inside, v):
    e = np.exp(z - z[inside].max())
    return e[inside & (z >= v)].sum()


def kept_mask(z, top_k=0, top_p=1.0):
    """Boolean mask of the kept classes of one row z (1-D)."""
    z = np.asarray(z)
    n = z.shape[0]
    inside = np.ones(n, dtype=bool)
    if 0 < top_k < n:
        v_k = np.partition(z, n - top_k)[n - top_k]         # the k-th largest, counting multiplicity
        inside = z >= v_k
    if top_p < 1.0:
        total = _mass_at_or_above(z, inside, -np.inf)
        values = np.unique(z[inside])                       # ascending; the mass above a value falls as the value rises,
        lo, hi = 0, len(values) - 1                         # so the last value that still holds the mass is found by bisection
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if _mass_at_or_above(z, inside, values[mid]) >= top_p * total:
                lo = mid
            else:
                hi = mid - 1
        inside = inside & (z >= values[lo])
    return inside


def kept_mask_by_sorting(z, top_k=0, top_p=1.0):
    """The same set from a descending sort: the shortest prefix that has top_k members (top-k), then the shortest prefix
    of those whose tie-closed extension holds top_p of their mass (top-p), each closed over ties at its last value."""
    z = np.asarray(z)
    n = z.shape[0]
    order = np.argsort(-z, kind="stable")
    zs = z[order]
    m = n
    if 0 < top_k < n:
        m = top_k
        while m < n and zs[m] == zs[m - 1]:
            m += 1
    if top_p < 1.0:
        e = np.exp(zs[:m] - zs[0])
        total = e.sum()
        q = 1
        while True:
            while q < m and zs[q] == zs[q - 1]:
                q += 1
            if e[:q].sum() >= top_p * total or q == m:
                break
            q += 1
        m = q
    mask = np.zeros(n, dtype=bool)
    mask[order[:m]] = True
    return mask


def kept_count(z, top_k=0, top_p=1.0):
    return int(kept_mask(z, top_k, top_p).sum())


def kept_counts(z, top_k=0, top_p=1.0):
    """kept_count of every row of z [M, n] at once, in float64: one descending sort and one cumulative sum per row.  The
    kept set of a row is its `count` largest values (a threshold set), so the count determines it."""
    z = np.asarray(z, dtype=np.float64)
    m, n = z.shape
    zs = -np.sort(-z, axis=1)
    col = np.arange(n)[None, :]
    size = np.full(m, n)
    if 0 < top_k < n:
        size = (zs >= zs[:, top_k - 1:top_k]).sum(1)
    if top_p >= 1.0:
        return size
    e = np.where(col < size[:, None], np.exp(zs - zs[:, :1]), 0.0)
    cum = np.cumsum(e, 1)
    run_ends = np.ones((m, n), dtype=bool)                  # a prefix may end only where the next value differs
    run_ends[:, :-1] = zs[:, :-1] != zs[:, 1:]
    ok = run_ends & (cum >= top_p * cum[:, -1:]) | (col == size[:, None] - 1)
    return np.argmax(ok, 1) + 1


def probabilities(z, mask):
    """The renormalised distribution over the kept classes (0 elsewhere), in z's dtype."""
    e = np.where(mask, np.exp(z - z[mask].max()), 0)
    return e / e.sum()


def draw(z, u, top_k=0, top_p=1.0):
    """(class, log-probability) of the restricted draw at uniform u."""
    z = np.asarray(z)
    mask = kept_mask(z, top_k, top_p)
    p = probabilities(z, mask)
    hit = np.nonzero(mask & (np.cumsum(p) > u))[0]
    c = int(hit[0]) if hit.size else int(np.nonzero(mask)[0][-1])
    return c, float(np.log(p[c]))
