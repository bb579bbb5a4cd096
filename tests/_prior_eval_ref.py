"""The yardsticks of the prior's held-out evaluation, stated from the formulas of include/vq2.h and shared by
tests/test_prior_eval_cpu.py and tests/test_gpu_prior_eval.py:

    row_quantities   per logits row, in any dtype: cross-entropy term, predictive entropy, rank of the target
    accumulate       the running state of vq2_prior_eval_accumulate as a numpy loop, double precision, same order
    bound            the rule of tests/test_gpu_prior_kernels.py: err <= 4 x the error of the same formula in float32 torch
    model_rows       logits of tests/_pixelsnail_model_ref.pixelsnail in a dtype -> the row quantities, [B, H*W] each
"""
import numpy as np
import torch


def row_quantities(logits, target, dtype=torch.float64):
    """logits [M, C] (any float dtype), target [M] int64 -> (nll [M], entropy [M]) in `dtype` and rank [M] int64.
    With m the row maximum and s = sum exp(l - m): nll = log s - (l[t] - m), entropy = log s - sum(exp(l - m) (l - m)) / s,
    rank = #{c: l[c] > l[t]} + #{c < t: l[c] == l[t]}.  A target outside [0, C): nll 0, rank -1."""
    l = logits.to(dtype)
    n_class = l.shape[1]
    m = l.max(1, keepdim=True)[0]
    d = l - m
    e = d.exp()
    s = e.sum(1)
    ls = s.log()
    valid = (target >= 0) & (target < n_class)
    t = target.clamp(0, n_class - 1).view(-1, 1)
    lt = l.gather(1, t)
    nll = torch.where(valid, ls - (lt - m).view(-1), torch.zeros_like(ls))
    entropy = ls - (e * d).sum(1) / s
    classes = torch.arange(n_class).view(1, -1)
    above = (l > lt) | ((l == lt) & (classes < t))
    rank = torch.where(valid, above.sum(1), torch.full_like(target, -1))
    return nll, entropy, rank


def brute_rank(logits, target):
    """The rank by two Python loops: classes with a larger logit, and lower classes with an equal one."""
    out = []
    for row, t in zip(logits.tolist(), target.tolist()):
        if not 0 <= t < len(row):
            out.append(-1)
            continue
        out.append(sum(1 for v in row if v > row[t]) + sum(1 for c in range(t) if row[c] == row[t]))
    return torch.tensor(out, dtype=torch.int64)


def new_state(length):
    return {"pos_nll": np.zeros(length, np.float64), "pos_entropy": np.zeros(length, np.float64),
            "pos_hit1": np.zeros(length, np.int64), "pos_hitk": np.zeros(length, np.int64), "counters": np.zeros(2, np.int64)}


def accumulate(state, nll, entropy, rank, n, length, top_k):
    """One batch of [n, length] rows (float32 nll / entropy, int32 rank as numpy) into `state`, in place: per position the
    images in order, in double.  Returns image_nll float32 [n]: per image the positions in order, in double, rounded once."""
    nll, entropy, rank = (a.reshape(n, length) for a in (nll, entropy, rank))
    for p in range(length):
        sn, se = state["pos_nll"][p], state["pos_entropy"][p]
        for i in range(n):
            sn = sn + np.float64(nll[i, p])
            se = se + np.float64(entropy[i, p])
        state["pos_nll"][p], state["pos_entropy"][p] = sn, se
        state["pos_hit1"][p] += int((rank[:, p] == 0).sum())
        state["pos_hitk"][p] += int(((rank[:, p] >= 0) & (rank[:, p] < top_k)).sum())
    state["counters"][0] += n
    state["counters"][1] += int((rank == -1).sum())
    image = np.zeros(n, np.float32)
    for i in range(n):
        s = np.float64(0.0)
        for p in range(length):
            s = s + np.float64(nll[i, p])
        image[i] = np.float32(s)
    return image


def bound(name, got, ref64, ref32, failed=None):
    """err <= 4 x the float32 formula's error, both against float64; returns that error (0: the formula is exact there and
    so must the result be).  failed: a list that collects the names that miss the bound instead of raising at the first,
    so that a test can print every figure before it asserts."""
    got, ref64, ref32 = (a.double() if torch.is_tensor(a) else torch.tensor(a, dtype=torch.float64) for a in (got, ref64, ref32))
    err = float((got - ref64).abs().max())
    err32 = float((ref32 - ref64).abs().max())
    print("%s: err %.3e, fp32 torch %.3e, ratio %.2f" % (name, err, err32, err / err32 if err32 else float("inf") if err else 0.0))
    if failed is not None and err > 4 * err32:
        failed.append(name)
    else:
        assert err <= 4 * err32, name
    return err32


def model_rows(M, sd, codes, n_class, attention, condition, dtype):
    """The row quantities of the plain-torch PixelSNAIL (M = _pixelsnail_model_ref) computed in `dtype` from the float32
    state_dict `sd`: (nll, entropy, rank), each [B, H*W]."""
    sdt = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    with torch.no_grad():
        logits = M.pixelsnail(codes, sdt, n_class, attention, condition)
    b, c, h, w = logits.shape
    rows = logits.permute(0, 2, 3, 1).reshape(b * h * w, c)
    return tuple(a.reshape(b, h * w) for a in row_quantities(rows, codes.reshape(-1), dtype))


def totals(nll, entropy, rank, top_k):
    """What PriorEvaluator.result() reports, from the [B, L] rows of ONE run, every sum and division in that run's own
    dtype: the float64 run is float64 throughout and the float32 run float32 throughout (sums and means as torch forms
    them), as the float32 run of _pixelsnail_model_ref.run_case is -- its loss is F.cross_entropy's float32 mean.  A
    float32 run whose rows were summed in float64 would be a third, more accurate thing: its mean can land within 1e-10
    of the float64 run's by cancellation, far below what any float32 result can resolve (half an ulp of a mean of 1.8 is
    6e-08), and a bound taken from it would measure that accident."""
    b, length = nll.shape
    return {"nll": nll.sum() / (b * length), "entropy": entropy.sum() / (b * length),
            "nll_map": nll.sum(0) / b, "image_nll": nll.sum(1),
            "accuracy": int((rank == 0).sum()) / (b * length),
            "top_k_accuracy": int(((rank >= 0) & (rank < top_k)).sum()) / (b * length)}
