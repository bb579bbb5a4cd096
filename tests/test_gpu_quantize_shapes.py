"""GPU: Quantize / VQVAE / VQVAE_Deep at embed_dim % 4 == 0 and any n_embed (through the C ABI, via vqvae2_amd) against
tests/golden/quantize_shapes.npz -- the reference's own outputs on seeded inputs whose fp64 margins make bit-exact
indices a fair demand (tests/test_quantize_shapes_cpu.py::test_fixture_margins) -- and against the CPU oracle."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import rng
from oracle import vqvae_deep_oracle as OD
from oracle import vqvae_oracle as O
from test_quantize_shapes_cpu import CAP

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def close(a, b, rtol, atol, what=""):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, err_msg=what)


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


def launched(amd, fn):
    lib = amd._lib.lib
    lib.vq2_prof_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        lib.vq2_prof_enable(0)
    buf = ctypes.create_string_buffer(1 << 16)
    lib.vq2_prof_report(buf, len(buf))
    return out, [ln.split()[0] for ln in buf.value.decode().splitlines()]


def make_quantize(amd, D, K, embed, cs0, training):
    q = amd.Quantize(D, K)
    q.load_state_dict({"embed": t(embed), "cluster_size": t(cs0), "embed_avg": t(embed) * t(cs0)[None, :]})
    return q.to(dev()).train(training)


@pytest.mark.parametrize("case", CAP.CASES, ids=[c[0] for c in CAP.CASES])
def test_fixture_case(amd, golden, case):
    """Indices bit-exact against the reference; output rows, diff, input gradient and the buffers after one update at
    the tolerances of test_gpu_parity.test_quantize_golden; counts exact; eval mode leaves the buffers alone."""
    g = golden("quantize_shapes")
    tag, D, K, xs, tie = case
    x, embed, cs0, gw = CAP.shape_inputs(tag, D, K, xs, tie, int(g[f"{tag}.seed"]))
    want_idx = g[f"{tag}.idx"]
    # statistics of the pre-update codebook straight from the op: counts exact, pad zero, sums against the oracle's scatter
    xd = t(x).to(dev())
    _, _, idx0, stats = amd.ops.QuantizeFn.apply(xd, t(embed).to(dev()), True, None, None)
    assert np.array_equal(idx0.cpu().numpy().astype(np.int32), want_idx), f"{tag}: indices differ (stats pass)"
    counts, sums_t = amd.ops.vq_stats_views(stats, K, D)
    rc, rs = O.quantize_stats(t(x), t(want_idx.astype(np.int64)), K)
    assert torch.equal(counts.cpu(), rc) and float(counts.sum()) == 128, tag
    assert float(stats[K:(K + 3) // 4 * 4].abs().sum()) == 0.0, tag
    close(sums_t.reshape(K, D).t(), rs, rtol=1e-5, atol=1e-5, what=f"{tag}.sums")
    # train mode, as the fixture was captured
    q = make_quantize(amd, D, K, embed, cs0, True)
    xt = t(x).to(dev()).requires_grad_(True)
    out, diff, idx = q(xt)
    ((out * t(gw).to(dev())).sum() + 0.25 * diff).backward()
    assert idx.dtype == torch.int64 and tuple(idx.shape) == xs[:-1]
    assert np.array_equal(idx.cpu().numpy().astype(np.int32), want_idx), f"{tag}: indices differ"
    close(out.reshape(-1, D)[::CAP.OUT_ROW_STEP], g[f"{tag}.out_rows"], rtol=1e-6, atol=1e-6, what=tag)
    close(diff, g[f"{tag}.diff"], rtol=1e-5, atol=1e-7, what=tag)
    close(xt.grad, g[f"{tag}.xgrad"], rtol=1e-5, atol=1e-7, what=tag)
    close(q.cluster_size, g[f"{tag}.cluster_size_after"], rtol=1e-5, atol=1e-6, what=tag)
    step = CAP.EMBED_COL_STEP
    close(q.embed_avg[:, ::step], g[f"{tag}.embed_avg_after_cols"], rtol=1e-5, atol=1e-5, what=tag)
    close(q.embed[:, ::step], g[f"{tag}.embed_after_cols"], rtol=1e-4, atol=1e-5, what=tag)
    # the whole updated codebook against the oracle's update of the same statistics
    e, cs, ea = t(embed).clone(), t(cs0).clone(), t(embed) * t(cs0)[None, :]
    O.ema_update_(e, cs, ea, rc, rs)
    close(q.embed_avg, ea, rtol=1e-5, atol=1e-5, what=tag)
    close(q.embed, e, rtol=1e-4, atol=1e-5, what=tag)
    if tie:
        flat = idx.reshape(-1)
        assert int(flat[0]) == 5 and int(flat[1]) == 64 and int(flat[2]) == 5     # the first index wins
    # eval mode
    qe = make_quantize(amd, D, K, embed, cs0, False)
    with torch.no_grad():
        _, diff_e, idx_e = qe(t(x).to(dev()))
    assert np.array_equal(idx_e.cpu().numpy().astype(np.int32), g[f"{tag}.eval_idx"]), tag
    close(diff_e, g[f"{tag}.eval_diff"], rtol=1e-5, atol=1e-7, what=tag)
    assert torch.equal(qe.embed.cpu(), t(embed)) and torch.equal(qe.cluster_size.cpu(), t(cs0))
    code = qe.embed_code(idx_e)
    close(code, F.embedding(idx_e.cpu(), t(embed).t()), rtol=0, atol=0)


@pytest.mark.parametrize("D,K", [(48, 510), (96, 1000), (192, 512), (12, 5)])
def test_prepared_codebook_is_bitwise_a_separate_prepare(amd, D, K):
    """What vq2_vq_ema_update_prepare leaves for the next forward (embedT, ||e||^2) equals vq2_vq_prepare of the updated
    codebook bit for bit, also where a block owns floor(256 / D) codes and some threads own nothing."""
    x = t(rng.normal(5, f"prep.x{D}", (2, 16, 16, D))).to(dev())
    e = t(rng.normal(5, f"prep.e{D}", (D, K)))
    q = amd.Quantize(D, K)
    q.load_state_dict({"embed": e, "cluster_size": torch.ones(K), "embed_avg": e.clone()})
    q.to(dev()).train()
    q(x)
    prep = q._prepared()
    assert prep is not None, "the EMA update did not leave a prepared codebook"
    embed_t, enorm = amd.ops.vq_prepare(q.embed)
    torch.cuda.synchronize()
    assert torch.equal(prep[0], embed_t) and torch.equal(prep[1], enorm)
    assert torch.equal(prep[0], q.embed.t())


def test_full_size_launch_ragged_both_ways(amd):
    """D = 48, K = 510 at M = 32*64*64 (+ a ragged tail): the 512-vector workgroups with dword staging, against the
    fp64 argmin in row blocks (at most max(2, M/2000) flips, each below 2e-6 of the distance scale), the oracle's
    scatter statistics and count conservation."""
    D, K = 48, 510
    x = t(rng.normal(23, "fs.x", (32, 64, 64, D)))
    x = torch.cat([x.reshape(-1, D), x.reshape(-1, D)[:77] * 0.25], 0).contiguous()      # M = 131,149: not a multiple of 128
    M = x.shape[0]
    assert M >= 512 * 256 and M % 128
    e = t(rng.normal(23, "fs.e", (D, K)))
    q = amd.Quantize(D, K)
    q.load_state_dict({"embed": e, "cluster_size": torch.zeros(K), "embed_avg": e.clone()})
    q.to(dev()).train()
    (out, diff, idx), labels = launched(amd, lambda: q(x.to(dev()).reshape(M, 1, 1, D)))
    assert f"vq_fwd|M={M},D={D},K={K},ragged" in labels, labels
    idx = idx.cpu().reshape(-1)
    margin, ref_idx = O.quantize_margin_chunked(x, e)
    bad = idx != ref_idx
    scale = x.double().pow(2).sum(-1) + 1.0
    print("full size: %d flips of %d, worst relative margin %.3e" %
          (int(bad.sum()), M, float((margin / scale)[bad].max()) if bool(bad.any()) else 0.0))
    assert int(bad.sum()) <= max(2, M // 2000), f"{int(bad.sum())} index mismatches vs the fp64 argmin"
    assert not bool(bad.any()) or float((margin / scale)[bad].max()) < 2e-6
    code = F.embedding(idx, e.t())
    close(out.reshape(M, D), x + (code - x), rtol=1e-6, atol=1e-6)
    close(diff, (code - x).pow(2).mean(), rtol=1e-4, atol=0)
    # the statistics buffer itself, straight from the op on the same input: GPU counts exact and summing to M, GPU sumsT
    # against the oracle's scatter.  The vectors of one code share a direction, so a code's running sum grows like i * mean
    # with |mean| <= 1 per component on these unit-variance inputs; the oracle adds the n rows one after the other in fp32,
    # each addition rounding by at most u = 2^-24 of the running sum, and the roundings add in quadrature:
    # u * sqrt(sum_i i^2) = u * n^1.5 / sqrt(3).  The GPU's fixed tree does better; u * n^1.5 bounds the two together.
    _, _, idx_s, stats = amd.ops.QuantizeFn.apply(x.to(dev()).reshape(M, 1, 1, D), e.to(dev()), True, None, None)
    assert torch.equal(idx_s.cpu().reshape(-1), idx)
    g_counts, g_sums_t = amd.ops.vq_stats_views(stats, K, D)
    counts, sums = O.quantize_stats(x, idx, K)
    assert torch.equal(g_counts.cpu(), counts) and float(g_counts.sum()) == M
    assert float(stats[K:(K + 3) // 4 * 4].abs().sum()) == 0.0
    n_max = float(counts.max())
    print("full size: max rows per code %d, sumsT max abs error %.3e, bound %.3e" %
          (n_max, float((g_sums_t.cpu().reshape(K, D).t() - sums).abs().max()), 2.0 ** -24 * n_max ** 1.5))
    close(g_sums_t.reshape(K, D).t(), sums, rtol=1e-5, atol=2.0 ** -24 * n_max ** 1.5, what="sumsT")
    close(q.cluster_size, 0.01 * counts, rtol=1e-6, atol=0)
    cs, ea, emb = torch.zeros(K), e.clone(), e.clone()
    O.ema_update_(emb, cs, ea, counts, sums)
    close(q.embed_avg, ea, rtol=5e-5, atol=1e-5)
    close(q.embed, emb, rtol=1e-4, atol=1e-5)


def _vqvae_48_510_step(amd, seed, hooks=None):
    cfg = O.VQVAEConfig(embed_dim=48, n_embed=510)
    st = O.make_state(cfg, seed)
    m = amd.VQVAE(embed_dim=48, n_embed=510)
    m.load_state_dict(st)
    m.to(dev())
    if hooks is not None:
        for key in ("t", "b"):
            getattr(m, f"quantize_{key}").register_forward_hook(
                lambda mod, i, o, key=key: hooks.__setitem__(key, (i[0].detach().cpu(), o[2].cpu())))
    tr = amd.Stage1Trainer(m, lr=3e-4)
    img = O.make_images(2, 64, seed)
    out = tr.step(img.to(dev()), return_dec=True)
    torch.cuda.synchronize()
    return cfg, st, m, tr, img, out


def test_vqvae_48_510_one_step_vs_oracle(amd):
    """VQVAE(embed_dim=48, n_embed=510) on 2x3x64x64: one Stage1Trainer.step against the CPU oracle -- codes under the
    near-tie rule, loss / reconstruction / EVERY parameter gradient at the tolerances of test_gpu_parity._step_vs_oracle
    (its all_elementwise form).  The widths this creates: 1x1 convs to 48 channels, a 48 -> 48 transposed conv, a
    96-channel decoder input and the 176-channel quantize_conv_b."""
    seen = {}
    cfg, st, m, tr, img, out = _vqvae_48_510_step(amd, 53, seen)
    embed0 = {k: st[f"quantize_{k}.embed"].clone() for k in ("t", "b")}
    pads = []
    for qz in tr.quantizers:                     # the pad floats of the statistics slices stay zero through a step
        k = qz.n_embed
        pads.append(float(qz.deferred_stats[k:(k + 3) // 4 * 4].abs().sum()))
    assert pads == [0.0, 0.0]
    adam = O.AdamState({k: v for k, v in st.items() if not O.is_buffer(k)})
    ref = O.train_step(st, cfg, img, adam)
    exact, flips = True, 0
    for n, key in enumerate(("t", "b")):
        x, got = seen[key]
        bad = (got != ref["ids"][n]).reshape(-1)
        if bool(bad.any()):
            exact = False
            flips += int(bad.sum())
            margin, _ = O.quantize_margin(x, embed0[key])
            scale = x.double().pow(2).sum(-1).reshape(-1) + 1.0
            assert int(bad.sum()) <= max(2, bad.numel() // 2000), f"{key}: {int(bad.sum())} index mismatches"
            assert float((margin / scale)[bad].max()) < 2e-6, f"{key}: mismatch away from a near-tie"
    close(out["loss"], ref["loss"], rtol=1e-4, atol=0)
    if exact:
        close(out["dec"], ref["dec"], rtol=1e-3, atol=1e-4)
    else:
        # a flipped near-tie moves ONE latent vector to the neighbouring code, which changes the reconstruction inside that
        # vector's footprint by at most its own magnitude: of the 128 top-level vectors (the coarsest footprint) `flips`
        # are affected, so the relative L2 error is at most sqrt(flips / 128)
        rel = float((out["dec"].cpu() - ref["dec"]).norm() / ref["dec"].norm())
        assert rel < (flips / 128.0) ** 0.5, f"reconstruction off by {rel:.3e} with {flips} near-tie flips"
    n_grads = 0
    for k, p in m.named_parameters():
        if p.grad is None:
            assert k.startswith("dec_ir."), k
            continue
        gref = ref["grads"][k]
        close(p.grad.norm(), gref.norm(), rtol=2e-3 if exact else 2e-2, atol=0, what=k)
        close(p.grad, gref, rtol=2e-3, atol=(5e-4 if exact else 2e-3) * float(gref.abs().max()) + 1e-9,
              what=k + " (element-wise)")
        n_grads += 1
    assert n_grads == len(m.live_parameters())
    sd = m.state_dict()
    for k in ("quantize_t.cluster_size", "quantize_b.cluster_size", "quantize_t.embed_avg", "quantize_b.embed_avg",
              "quantize_t.embed", "quantize_b.embed"):
        close(sd[k], st[k], rtol=1e-3 if exact else 5e-2, atol=2e-5 if exact else 2e-2, what=k)


def test_vqvae_48_510_step_is_bit_reproducible(amd):
    a = _vqvae_48_510_step(amd, 54)[2].state_dict()
    b = _vqvae_48_510_step(amd, 54)[2].state_dict()
    assert list(a.keys()) == list(b.keys())
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k} differs between two identical steps"


def test_deep_192_forward_backward_vs_oracle(amd):
    """VQVAE_Deep(embed_dim=192) on 2x3x32x32 with an explicit style=: forward + backward against
    oracle/vqvae_deep_oracle.py, checked the way test_gpu_deep.test_default_deep_model_step_vs_oracle checks 256.
    Not through Stage1Trainer.step: the trainer calls model(img) and has no style input, and the fork's
    VQVAE_Deep.forward raises TypeError without one (mirrored, see test_gpu_deep.py).  The step of this model is the
    drop-in module's -- forward with the EMA update inside it, backward -- so that is what is checked: every parameter
    gradient, the style gradient and the EMA buffers against the oracle.  The trainer's statistics slices and the
    bit-reproducibility of a step at these widths are covered by the two VQVAE(48, 510) tests above."""
    cfg = OD.DeepConfig(embed_dim=192)
    st = OD.make_deep_state(cfg, 9, 0.3, 1.5)
    m = amd.VQVAE_Deep(embed_dim=192)
    m.load_state_dict(st)
    m.to(dev()).train()
    img = O.make_images(2, 32, 9)
    style = OD.make_style(2, cfg, 9)
    seen = {}
    for key in ("t", "b"):
        getattr(m, f"quantize_{key}").register_forward_hook(
            lambda mod, i, o, key=key: seen.__setitem__(key, (i[0].detach().cpu(), o[2].cpu())))
    sg = style.to(dev()).requires_grad_(True)
    dec, diff, quant = m(img.to(dev()), style=sg)
    assert tuple(dec.shape) == (2, 3, 32, 32) and tuple(quant.shape) == (2, 384, 4, 4)
    loss = F.mse_loss(dec, img.to(dev())) + 0.25 * diff.mean()
    loss.backward()
    for key in ("t", "b"):
        x, ids = seen[key]
        margin, want = O.quantize_margin_chunked(x, st[f"quantize_{key}.embed"])
        bad = ids.reshape(-1) != want
        if bool(bad.any()):
            scale = x.reshape(bad.numel(), -1).double().pow(2).sum(-1) + 1.0
            assert int(bad.sum()) <= 2 and float((margin / scale)[bad].max()) < 2e-6, f"{key}: index away from a near-tie"
    ref_st = {k: (v.clone().requires_grad_(True) if not (O.is_buffer(k) or OD.is_dead_key(k)) else v.clone())
              for k, v in st.items()}
    sr = style.clone().requires_grad_(True)
    rdec, rdiff, rquant, rid_t, rid_b = OD.deep_forward(ref_st, cfg, img, sr, training=True)
    (F.mse_loss(rdec, img) + 0.25 * rdiff.mean()).backward()
    assert torch.equal(seen["t"][1], rid_t) and torch.equal(seen["b"][1], rid_b), \
        "GPU and CPU chose different codes on this seed (40 latent vectors): not a near-tie matter"
    close(dec, rdec, rtol=1e-3, atol=1e-4, what="dec")
    close(quant, rquant, rtol=1e-4, atol=1e-5, what="quant")

    def grad_close(got, want, what):
        want = want.detach()
        close(got, want, rtol=2e-3, atol=2e-4 * float(want.abs().max()) + 1e-10, what=what)
    grad_close(sg.grad, sr.grad, "style gradient")
    n = 0
    for k, p in m.named_parameters():
        if OD.is_dead_key(k):
            assert p.grad is None, k
            continue
        if k.startswith("dec.blocks.") and k.endswith(".conv1.bias"):      # analytically zero: see test_gpu_deep.py
            wmax = float(ref_st[k[:-4] + "weight"].grad.abs().max())
            assert float(p.grad.abs().max()) < 1e-4 * wmax and float(ref_st[k].grad.abs().max()) < 1e-4 * wmax, k
        else:
            grad_close(p.grad, ref_st[k].grad, k)
        n += 1
    assert n > 150
    for k in ("quantize_t.cluster_size", "quantize_b.cluster_size", "quantize_t.embed_avg", "quantize_b.embed"):
        close(m.state_dict()[k], ref_st[k], rtol=1e-4, atol=1e-5, what=k)


def test_profiler_labels_of_aligned_and_ragged_shapes(amd, golden):
    """K % 4 == 0 keeps the label it had, whatever D; K % 4 != 0 says so in its label.  (Labels are the library's own
    launch brackets, not kernel symbols: that the aligned kernels themselves are unchanged is shown by their gfx950
    assembly and by the kernel trace recorded in profiles/quantize_shapes.json.)"""
    shapes = [(D, K) for _, D, K, _, _ in CAP.CASES] + [(64, 512), (16, 64), (256, 512), (64, 8192)]
    for D, K in shapes:
        q = amd.Quantize(D, K).to(dev()).train()
        x = torch.randn(2, 8, 8, D, device=dev())
        _, labels = launched(amd, lambda: q(x))
        vq = sorted(l for l in labels if l.startswith("vq_"))
        tail = ",ragged" if K % 4 else ""
        assert vq == sorted([f"vq_fwd|M=128,D={D},K={K}{tail}", f"vq_stats|M=128,D={D},K={K}"]), (D, K, vq)
