"""CPU checks of the causal-attention yardstick (tests/_attention_ref.py) against the goldens captured from the
reference's CausalAttention (scripts/make_golden_attention.py), and of the module's host side."""
import numpy as np
import pytest
import torch

import _attention_ref as R


def _cases(g):
    return [tuple(int(v) for v in row) for row in g["cases"]]


def _load(g, ci, dtype):
    t = f"c{ci}."
    sd = {n: torch.from_numpy(g[t + "sd." + n]).to(dtype).requires_grad_(True) for n in R.PARAM_NAMES}
    query = torch.from_numpy(g[t + "in.query"]).to(dtype).requires_grad_(True)
    key = torch.from_numpy(g[t + "in.key"]).to(dtype).requires_grad_(True)
    return query, key, torch.from_numpy(g[t + "in.gout"]).to(dtype), sd


def _run(g, ci, dtype, fill=None, taps=None):
    query, key, gout, sd = _load(g, ci, dtype)
    out = R.causal_attention(query, key, sd, _cases(g)[ci][6], fill=fill, taps=taps)
    (out * gout).sum().backward()
    grads = {"query": query.grad, "key": key.grad}
    grads.update({n: sd[n].grad for n in R.PARAM_NAMES})
    return out.detach(), grads


def test_reference_formula_reproduces_the_goldens(golden):
    g = golden("pixelsnail_attention")
    assert len(_cases(g)) >= 3
    for ci in range(len(_cases(g))):
        taps = {}
        out64, g64 = _run(g, ci, torch.float64, taps=taps)
        want = {"out": g[f"c{ci}.out.f64"], **{k: g[f"c{ci}.grad.f64.{k}"] for k in g64}}
        have = {"out": out64.numpy(), **{k: v.numpy() for k, v in g64.items()}}
        assert len(have) == 12                                # the output and eleven gradients
        for k in want:
            scale = np.abs(want[k]).max()
            if k == "key.bias":
                # a constant added to every key shifts each row of scores as a whole, which the softmax ignores: this
                # gradient is exactly 0 and what the golden holds is the rounding of its summands, the per-pixel
                # gradients of K -- they are the scale
                scale = float(taps["k"].grad.abs().sum((0, 1)).max())
            assert np.abs(have[k] - want[k]).max() <= 1e-12 * scale, (ci, k)
        # float32: within the float32-vs-float64 gap the golden itself records.  The yardstick states the formula with
        # torch's own operations in the order the layer is written (linear, matmul, softmax), so its float32 run carries
        # the same roundings as the golden's and no allowance beyond the gap is needed
        out32, g32 = _run(g, ci, torch.float32)
        have = {"out": out32.numpy(), **{k: v.numpy() for k, v in g32.items()}}
        for k in want:
            ref32 = g[f"c{ci}.out.f32"] if k == "out" else g[f"c{ci}.grad.f32.{k}"]
            gap = np.abs(ref32.astype(np.float64) - want[k]).max()
            assert np.abs(have[k].astype(np.float64) - want[k]).max() <= gap, (ci, k, gap)


def test_row_zero_is_exactly_zero(golden):
    g = golden("pixelsnail_attention")
    for ci in range(len(_cases(g))):
        for dtype in (torch.float32, torch.float64):
            out, _ = _run(g, ci, dtype)
            assert torch.count_nonzero(out[:, :, 0, 0]) == 0
        assert np.count_nonzero(g[f"c{ci}.out.f32"][:, :, 0, 0]) == 0 and np.count_nonzero(g[f"c{ci}.out.f64"][:, :, 0, 0]) == 0


def test_masked_fill_equivalence_on_the_golden_cases(golden):
    """Excluding the masked scores and filling them with -1e4 give the same float32 result while every unmasked score
    of a row is above about -9,896: the filled entries' exponentials are exactly 0."""
    g = golden("pixelsnail_attention")
    for ci in range(len(_cases(g))):
        a, ga = _run(g, ci, torch.float32)
        b, gb = _run(g, ci, torch.float32, fill=-1e4)
        assert torch.equal(a, b), ci
        for k in ga:
            assert torch.allclose(ga[k], gb[k], rtol=0, atol=1e-6 * float(ga[k].abs().max()) + 1e-30), (ci, k)
    assert float(torch.exp(torch.tensor(-103.98, dtype=torch.float32))) == 0.0
    assert float(torch.exp(torch.tensor(-1e4 + 9896.0, dtype=torch.float32))) == 0.0


def test_state_dict_table_matches_the_golden(golden):
    import vqvae2_amd
    g = golden("pixelsnail_attention")
    for ci, (b, h, w, cq, ck, ch, nh) in enumerate(_cases(g)):
        m = vqvae2_amd.CausalAttention(cq, ck, ch, n_head=nh)
        sd = m.state_dict()
        names = [k[len(f"c{ci}.sd."):] for k in g.files if k.startswith(f"c{ci}.sd.")]
        assert sorted(sd.keys()) == sorted(names) == sorted(R.PARAM_NAMES)
        for n in names:
            assert tuple(sd[n].shape) == g[f"c{ci}.sd.{n}"].shape, n
        m.load_state_dict({n: torch.from_numpy(g[f"c{ci}.sd.{n}"]) for n in names}, strict=True)
        # weight_norm initialisation: g is the row norm of v, so the effective weight starts as v itself
        f = vqvae2_amd.CausalAttention(cq, ck, ch, n_head=nh)
        assert torch.allclose(f.query.weight_g, f.query.weight_v.norm(2, dim=1, keepdim=True))


def test_refusals_without_gpu():
    import vqvae2_amd
    with pytest.raises(NotImplementedError):
        vqvae2_amd.CausalAttention(8, 8, 12, n_head=2)        # dim_head 6
    with pytest.raises(NotImplementedError):
        vqvae2_amd.CausalAttention(8, 8, 136, n_head=2)       # dim_head 68
    with pytest.raises(NotImplementedError):
        vqvae2_amd.CausalAttention(8, 8, 30, n_head=4)        # channel not divisible by n_head
    m = vqvae2_amd.CausalAttention(8, 8, 16, n_head=2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(1, 8, 3, 3), torch.zeros(1, 8, 3, 3))
    d = vqvae2_amd._lib.AttnDesc()
    d.B, d.L, d.n_head, d.dim_head, d.ldq, d.ldk, d.ldv, d.ldo = 1, 4, 2, 6, 12, 12, 12, 12
    assert vqvae2_amd._lib.lib.vq2_causal_attn_fwd(d, None, None, None, None, None, None) == 1     # VQ2_ERR_INVALID
    assert b"dim_head" in vqvae2_amd._lib.lib.vq2_last_error()
