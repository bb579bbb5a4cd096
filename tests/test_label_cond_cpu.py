"""The class-conditional prior's rule in plain float64 torch (_label_cond_ref.py), checked against itself without a GPU: zero
tables give the unlabelled reference, the logits are causal in the codes and depend on the label, the stated table gradient
is autograd's, and the host side of the new entry points (binding, refusals before a launch, constructor arguments)."""
import inspect

import pytest
import torch

import _label_cond_ref as LR
import _pixelsnail_model_ref as M

N_LABEL = 3
LABEL = torch.tensor([2, 0, 2])


@pytest.fixture(scope="module")
def g():
    return M.load()


def _case(g, ci, batch=3):
    """(case, float64 state_dict with seeded tables, codes [batch,H,W], condition or None)"""
    c = M.cases(g)[ci]
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in LR.add_tables(M.state_dict(g, ci), N_LABEL, 11).items()}
    gen = torch.Generator().manual_seed(40 + ci)
    h, w = c["shape"]
    codes = torch.randint(0, c["n_class"], (batch, h, w), generator=gen)
    cond = torch.randint(0, c["n_class"], (batch, h // 2, w // 2), generator=gen) if "cond" in c else None
    return c, sd, codes, cond


@pytest.mark.parametrize("ci", [0, 1], ids=["attention", "conditioned"])
def test_zero_tables_give_the_unlabelled_reference(g, ci):
    c, sd, codes, cond = _case(g, ci)
    plain = {k: v for k, v in sd.items() if not k.endswith("label_embed")}
    zero = {k: (torch.zeros_like(v) if k.endswith("label_embed") else v) for k, v in sd.items()}
    assert len(LR.table_names(sd)) == c["args"][3] * c["args"][2]          # one table per 'causal' block
    with torch.no_grad():
        want = M.pixelsnail(codes, plain, c["n_class"], c["attention"], cond)
        assert torch.equal(LR.pixelsnail(codes, zero, c["n_class"], c["attention"], cond, LABEL), want)
        assert torch.equal(LR.pixelsnail(codes, plain, c["n_class"], c["attention"], cond, None), want)
        # a label outside the table adds nothing either
        assert torch.equal(LR.pixelsnail(codes, sd, c["n_class"], c["attention"], cond, torch.tensor([-1, N_LABEL, -7])), want)
        assert not torch.equal(LR.pixelsnail(codes, sd, c["n_class"], c["attention"], cond, LABEL), want)


@pytest.mark.parametrize("ci", [0, 1], ids=["attention", "conditioned"])
def test_logits_are_causal_in_the_codes_and_depend_on_the_label(g, ci):
    c, sd, codes, cond = _case(g, ci)
    _, h, w = codes.shape
    with torch.no_grad():
        y0 = LR.pixelsnail(codes, sd, c["n_class"], c["attention"], cond, LABEL)
        raster = torch.arange(h * w).view(h, w)
        for p in ((h // 2) * w + w // 2, 1 * w + 0, h * w - 2):
            changed = codes.clone()
            changed[:, p // w, p % w] = (changed[:, p // w, p % w] + 1) % c["n_class"]
            y1 = LR.pixelsnail(changed, sd, c["n_class"], c["attention"], cond, LABEL)
            before = raster <= p                # logits at (i, j) see codes before (i, j) only
            assert torch.equal(y0[:, :, before], y1[:, :, before]), p
            assert not torch.equal(y0[:, :, ~before], y1[:, :, ~before]), p
        other = LR.pixelsnail(codes, sd, c["n_class"], c["attention"], cond, torch.tensor([2, 1, 2]))
        assert torch.equal(other[0], y0[0]) and torch.equal(other[2], y0[2])         # an image sees its own label only
        assert not torch.equal(other[1, :, 0, 0], y0[1, :, 0, 0])                     # ... already at the first pixel


def test_stated_table_gradient_is_autograds():
    gen = torch.Generator().manual_seed(3)
    images, ppi, ch, n_label = 5, 7, 3, 4
    label = torch.tensor([1, 3, 1, -1, 4])                                            # repeats, 0 and 2 unused, two out of range
    t = torch.randn(images * ppi, 2 * ch, generator=gen, dtype=torch.float64)
    res = torch.randn(images * ppi, ch, generator=gen, dtype=torch.float64)
    dout = torch.randn(images * ppi, ch, generator=gen, dtype=torch.float64)
    embed = torch.randn(n_label, 2 * ch, generator=gen, dtype=torch.float64).requires_grad_(True)
    tt = t.clone().requires_grad_(True)
    (LR.glu_label_fwd(tt, res, embed, label, ppi) * dout).sum().backward()
    dt = LR.glu_label_bwd(dout, t, embed.detach(), label, ppi)
    assert torch.allclose(dt, tt.grad, rtol=1e-13, atol=1e-15)
    dE = LR.label_embed_grad(dt, label, ppi, n_label)
    assert torch.allclose(dE, embed.grad, rtol=1e-13, atol=1e-15)
    assert float(dE[0].abs().sum()) == 0 and float(dE[2].abs().sum()) == 0 and float(dE[1].abs().sum()) > 0


def test_model_reference_table_gradient_is_a_sum_of_dt(g):
    """In the whole model: the gradient autograd gives a table equals the stated sum over the gradient of the block's t."""
    c, sd, codes, cond = _case(g, 1)
    res = LR.run(sd, codes, c["n_class"], c["attention"], cond, LABEL, torch.float64)
    for name in LR.table_names(sd):
        dE = res["grad." + name]
        assert dE.shape == (N_LABEL, 2 * c["args"][0]) and float(dE[1].abs().sum()) == 0      # label 1 is unused
        assert float(dE[0].abs().sum()) > 0 and float(dE[2].abs().sum()) > 0


# ----------------------------------------------------------------------------- host side, no device
@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


def test_entry_points_are_bound(amd):
    L = amd._lib
    assert L.API_VERSION >= 22 and L.lib.vq2_version() == L.API_VERSION
    for name in ("vq2_glu_res_label_fwd", "vq2_glu_res_label_bwd", "vq2_label_embed_grad", "vq2_label_embed_grad_workspace_bytes"):
        assert name in L.EXPORTS
    # two runs of 64 pixels per image, ceil4(6) lanes; 1024 pixels: 16 runs; a refused shape: 0
    assert L.lib.vq2_label_embed_grad_workspace_bytes(3, 100, 6) == 3 * 2 * 8 * 4
    assert L.lib.vq2_label_embed_grad_workspace_bytes(32, 1024, 512) == 32 * 16 * 512 * 4
    assert L.lib.vq2_label_embed_grad_workspace_bytes(0, 4, 8) == 0 and L.lib.vq2_label_embed_grad_workspace_bytes(1, 4, 8200) == 0


def test_refusals_before_a_launch(amd):
    lib = amd._lib.lib
    import ctypes
    p = ctypes.c_void_p(64)        # never dereferenced: every call below is refused on the host
    assert lib.vq2_glu_res_label_fwd(p, 8, p, 4, p, 8, p, 2, 3, p, 4, 7, 4, 3, None) == 1
    assert b"images * pixels_per_image" in lib.vq2_last_error()
    assert lib.vq2_glu_res_label_bwd(p, 4, p, 8, p, 8, p, 2, 3, p, 8, 5, 4, 3, None) == 1
    assert lib.vq2_glu_res_label_fwd(p, 8, p, 4, p, 8, p, 2, 3, p, 4, 6, 4, 0, None) == 1          # n_label 0
    assert lib.vq2_glu_res_label_fwd(p, 8, p, 4, p, 6, p, 2, 3, p, 4, 6, 4, 3, None) == 1          # lde < 2 Ch
    assert lib.vq2_glu_res_label_fwd(p, 8, p, 4, None, 8, p, 2, 3, p, 4, 6, 4, 3, None) == 1
    assert lib.vq2_glu_res_label_fwd(p, 8, p, 4, p, 8, ctypes.c_void_p(68), 2, 3, p, 4, 6, 4, 3, None) == 1     # label alignment
    assert lib.vq2_label_embed_grad(p, 8, p, 2, 3, 8, 3, p, p, 0, None) == 1 and b"workspace" in lib.vq2_last_error()
    assert lib.vq2_label_embed_grad(p, 4, p, 2, 3, 8, 3, p, p, 1 << 20, None) == 1                 # lddt < ceil4(C2)


def test_constructor_arguments_and_parameters(amd):
    for cls in (amd.PixelSNAIL, amd.PixelBlock, amd.GatedResBlock):
        params = inspect.signature(cls.__init__).parameters
        assert list(params)[-1] == "n_label" and params["n_label"].default == 0
    assert list(inspect.signature(amd.PixelSNAIL.forward).parameters) == ["self", "input", "condition", "cache", "label"]
    for fn in (amd.Stage2Trainer.step, amd.PriorSampler.sample, amd.PriorSampler.logits_given, amd.sample_model,
               amd.score_codes_labelled, amd.PriorEvaluator.update_labelled):
        assert "label" in inspect.signature(fn).parameters
    torch.manual_seed(0)
    plain = amd.PixelSNAIL([4, 6], 6, 8, 3, 2, 2, 8, attention=False)
    torch.manual_seed(0)
    m = amd.PixelSNAIL([4, 6], 6, 8, 3, 2, 2, 8, attention=False, n_label=5)
    tables = [k for k in m.state_dict() if k.endswith("label_embed")]
    assert tables == [f"blocks.{i}.resblocks.{k}.label_embed" for i in range(2) for k in range(2)]
    assert sorted(set(m.state_dict()) - set(tables)) == sorted(plain.state_dict())
    for k in tables:
        t = m.state_dict()[k]
        assert t.shape == (5, 16) and t.dtype == torch.float32 and 0.02 < float(t.std()) < 0.08
    assert all(isinstance(p, torch.nn.Parameter) and p.requires_grad for n, p in m.named_parameters() if n.endswith("label_embed"))
    assert not any("label" in k for k in plain.state_dict())
    with pytest.raises(ValueError):
        amd.PixelSNAIL([4, 6], 6, 8, 3, 2, 2, 8, attention=False, n_label=-1)


def test_class_names_from_file_names(amd):
    from vqvae2_amd import codes
    assert codes.class_name("n01/a.png") == "n01" and codes.class_name("a.png") == "" and codes.class_name("x/y/a.png") == "x/y"
    names = sorted({"dog", "cat", "bird"})
    lab = codes.labels_of(["dog/1.png", "bird/2.png", "fish/3.png", "cat/4.png"], names)
    assert lab.dtype == torch.int64 and lab.tolist() == [2, 0, -1, 1]
