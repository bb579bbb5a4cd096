"""CPU: Quantize / VQVAE / VQVAE_Deep at any embed_dim % 4 == 0 in 4..256 and any n_embed in 1..16384 -- the
constructor space, the statistics-buffer layout, and the fixture tests/golden/quantize_shapes.npz (captured from the
reference by scripts/capture_quantize_shapes.py) against its own margin claim and against the oracle."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import vqvae_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_capture():
    spec = importlib.util.spec_from_file_location(
        "capture_quantize_shapes", os.path.join(ROOT, "scripts", "capture_quantize_shapes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


CAP = load_capture()
TOL = dict(rtol=1e-5, atol=1e-6)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def close(a, b, **kw):
    np.testing.assert_allclose(np.asarray(a), np.asarray(b), **{**TOL, **kw})


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


def layout_of(sd):
    return [str(k) for k in sd.keys()], [list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()]


def test_constructor_space(amd, golden):
    g = golden("quantize_shapes")
    for tag, D, K, _, _ in CAP.CASES:
        q = amd.Quantize(D, K)
        sd = q.state_dict()
        assert list(sd.keys()) == ["embed", "cluster_size", "embed_avg"], tag
        assert [tuple(v.shape) for v in sd.values()] == [(D, K), (K,), (D, K)], tag
    for tag, cls, kwargs in CAP.MODEL_CASES:
        keys, shapes = layout_of(getattr(amd, cls)(**kwargs).state_dict())
        assert keys == [str(k) for k in g[f"{tag}.keys"]], tag
        assert shapes == g[f"{tag}.shapes"].tolist(), tag


def test_refusals(amd):
    for dim, n_embed in [(6, 512), (260, 512), (64, 16385), (0, 512), (64, 0)]:
        with pytest.raises(NotImplementedError, match="multiple of 4 in 4..256 and n_embed in 1..16384"):
            amd.Quantize(dim, n_embed)
    with pytest.raises(NotImplementedError):
        amd.VQVAE(embed_dim=6)
    with pytest.raises(NotImplementedError):
        amd.VQVAE(n_embed=16385)
    amd.Quantize(4, 1)
    amd.Quantize(256, 16384)
    amd.Quantize(64, 510)


def test_stats_layout_helper(amd):
    ops = amd.ops
    D = 48
    for K in (5, 510, 512, 2050):
        n = ops.vq_stats_numel(K, D)
        assert n % 4 == 0 and n == (K + 3) // 4 * 4 + K * D
        stats = ops.vq_stats_alloc(K, D, torch.device("cpu"))
        assert stats.numel() == n and stats.data_ptr() % 16 == 0
        counts, sums_t = ops.vq_stats_views(stats, K, D)
        assert counts.numel() == K and sums_t.numel() == K * D
        assert counts.data_ptr() == stats.data_ptr()
        assert sums_t.data_ptr() % 16 == 0                                    # a float4 boundary for every K
        off = (sums_t.data_ptr() - stats.data_ptr()) // 4
        assert off == (K + 3) // 4 * 4
        # the kernels write the two views and nothing else: whatever lies between them must already be zero
        counts.fill_(7.0)
        sums_t.fill_(7.0)
        assert int((stats != 7.0).sum()) == off - K and float(stats[K:off].abs().sum()) == 0.0
        if K % 4 == 0:                                                        # today's [counts | sumsT], byte for byte
            assert off == K and n == K + K * D
        with pytest.raises(RuntimeError):
            ops.vq_stats_views(torch.zeros(K + K * D + 1), K, D)


def test_fixture_margins(golden):
    """Bit-exact indices on the GPU are a property of the kernel, not of luck: every non-tie row of every case keeps an
    fp64 gap of at least 1e-5 of (||x||^2 + 1) between its two best codes."""
    g = golden("quantize_shapes")
    assert CAP.MARGIN == 1e-5
    want = {("s48_510", 48, 510, False), ("s64_510", 64, 510, False), ("s48_512", 48, 512, False),
            ("s96_1000", 96, 1000, False), ("s192_512", 192, 512, False), ("s12_5", 12, 5, False),
            ("s20_2050", 20, 2050, False), ("s48_510_tie", 48, 510, True)}
    assert {(tag, D, K, tie) for tag, D, K, _, tie in CAP.CASES} == want
    for tag, D, K, xs, tie in CAP.CASES:
        assert xs == (2, 8, 8, D)
        seed = int(g[f"{tag}.seed"])
        x, embed, _, _ = CAP.shape_inputs(tag, D, K, xs, tie, seed)
        rel = CAP.relative_margins(x, embed, tie)
        assert rel.size == 128 - (len(CAP.TIE_ROWS) if tie else 0)
        assert float(rel.min()) >= 1e-5, (tag, float(rel.min()))


def test_oracle_agrees_with_fixture(golden):
    g = golden("quantize_shapes")
    step, rstep = CAP.EMBED_COL_STEP, CAP.OUT_ROW_STEP
    for tag, D, K, xs, tie in CAP.CASES:
        x, embed, cs0, gw = CAP.shape_inputs(tag, D, K, xs, tie, int(g[f"{tag}.seed"]))
        for training in (True, False):
            e, cs, ea = t(embed).clone(), t(cs0).clone(), (t(embed) * t(cs0)[None, :]).clone()
            xt = t(x).clone().requires_grad_(True)
            out, diff, idx = O.quantize_forward(xt, e, cs, ea, training)
            ((out * t(gw)).sum() + 0.25 * diff).backward()
            if not training:
                assert np.array_equal(idx.numpy().astype(np.int32), g[f"{tag}.eval_idx"]), tag
                close(diff.detach(), g[f"{tag}.eval_diff"])
                assert torch.equal(e, t(embed)) and torch.equal(cs, t(cs0))
                continue
            assert np.array_equal(idx.numpy().astype(np.int32), g[f"{tag}.idx"]), tag
            close(out.detach().reshape(-1, D)[::rstep], g[f"{tag}.out_rows"])
            close(diff.detach(), g[f"{tag}.diff"])
            close(xt.grad, g[f"{tag}.xgrad"])
            close(cs, g[f"{tag}.cluster_size_after"])
            close(ea[:, ::step], g[f"{tag}.embed_avg_after_cols"])
            close(e[:, ::step], g[f"{tag}.embed_after_cols"])
    gi = g["s48_510_tie.idx"].reshape(-1)
    assert gi[0] == 5 and gi[1] == 64 and gi[2] == 5      # first index wins on exact ties
