"""GPU checks of the class-conditional prior (PixelSNAIL(..., n_label=3)) against the float64 statement of its rule
(_label_cond_ref.py): logits and every gradient, the sampler in both steppings, exact resume of a labelled Stage2Trainer,
PriorEvaluator with labels, the error paths, and the unlabelled model left as it was.

Models: the constructor arguments and weights of the small golden cases of tests/golden/pixelsnail_model.npz (0: attention,
1: conditioned bottom prior) plus n_label=3 and seeded tables, batch 3 with labels [2, 0, 2].  The bar is the model parity
test's (test_gpu_pixelsnail_model.py): per tensor, 4 x the gap between the float32 and the float64 run of the reference;
ratios are printed.

Two interfaces differ from the issue's wording because tests/test_prior_eval_cpu.py pins the parameter lists of
PriorEvaluator.update and score_codes: the label goes through PriorEvaluator.update_labelled(label, ...) and
score_codes_labelled(model, codes, label, condition=None)."""
import numpy as np
import pytest
import torch

import _label_cond_ref as LR
import _pixelsnail_model_ref as M

pytestmark = pytest.mark.gpu

N_LABEL = 3
LABEL = [2, 0, 2]
CASES = {0: "attention", 1: "conditioned"}


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


@pytest.fixture(scope="module")
def g():
    return M.load()


@pytest.fixture(scope="module")
def ref(g):
    """Per case: the inputs and the reference's float64 and float32 runs, computed once."""
    out = {}
    for ci in CASES:
        c = M.cases(g)[ci]
        sd = LR.add_tables(M.state_dict(g, ci), N_LABEL, 11)
        gen = torch.Generator().manual_seed(40 + ci)
        h, w = c["shape"]
        codes = torch.randint(0, c["n_class"], (3, h, w), generator=gen)
        cond = torch.randint(0, c["n_class"], (3, h // 2, w // 2), generator=gen) if "cond" in c else None
        label = torch.tensor(LABEL)
        runs = {dt: LR.run(sd, codes, c["n_class"], c["attention"], cond, label, dt) for dt in (torch.float64, torch.float32)}
        out[ci] = dict(c=c, sd=sd, codes=codes, cond=cond, label=label, f64=runs[torch.float64], f32=runs[torch.float32])
    return out


def _model(amd, r, train=False):
    c = r["c"]
    m = amd.PixelSNAIL(c["shape"], c["n_class"], *c["args"], **c["kw"], n_label=N_LABEL)
    m.load_state_dict(r["sd"], strict=True)
    assert sorted(m.state_dict()) == sorted(r["sd"])
    m = m.cuda()
    return m.train() if train else m.eval()


def _dev(r):
    return r["codes"].cuda(), (r["cond"].cuda() if r["cond"] is not None else None), r["label"].cuda()


def _compare(tag, have, r):
    bad = []
    for k, v in have.items():
        f64 = r["f64"][k].numpy()
        gap = float(np.abs(r["f32"][k].double().numpy() - f64).max())
        err = float(np.abs(v.detach().double().cpu().numpy() - f64).max())
        print("%s %s: err %.3e, reference gap %.3e, ratio %.2f" % (tag, k, err, gap, err / gap if gap else float("inf")))
        if not (gap > 0 and err <= 4 * gap):
            bad.append((k, err, gap))
    assert not bad, bad


@pytest.mark.parametrize("ci", CASES, ids=CASES.values())
def test_logits_and_every_gradient_against_fp64(amd, ref, ci):
    r = ref[ci]
    m = _model(amd, r)
    codes, cond, label = _dev(r)
    out, _ = m(codes, condition=cond, label=label)
    loss, _ = amd.prior_loss(out, codes)
    loss.backward()
    torch.cuda.synchronize()
    have = {"logits": out}
    have.update({"grad." + k: p.grad for k, p in m.named_parameters()})
    tables = ["grad." + k for k in LR.table_names(r["sd"])]
    assert tables and all(k in have for k in tables)
    assert sorted(k for k in have if k.startswith("grad.")) == sorted(k for k in r["f64"] if k.startswith("grad."))
    for k in tables:
        assert float(have[k][1].abs().sum()) == 0 and float(have[k][0].abs().sum()) > 0        # label 1: no image, exactly 0
    _compare(f"case {ci}", have, r)
    # The loss is ONE float32 number: the reference's float32 run can land anywhere inside half an ulp of the float64 one,
    # so its own gap says nothing about a scalar.  The bound is reasoned instead: the mean of -log_softmax(logits)[target]
    # moves by at most twice the largest logit error (log-softmax is 2-Lipschitz in the max norm), for which the bar above
    # allows 4 x the logits' gap, plus two ulps of the float32 result (2^-22 |loss|).
    want = float(r["f64"]["loss"])
    gap = float((r["f32"]["logits"].double() - r["f64"]["logits"]).abs().max())
    err = abs(float(loss) - want)
    print("case %d loss: err %.3e, bound %.3e" % (ci, err, 8 * gap + 2.0 ** -22 * abs(want)))
    assert err <= 8 * gap + 2.0 ** -22 * abs(want)
    # a label outside the table: the unlabelled model's logits, bit for bit, and no gradient into any table
    c = r["c"]
    plain = amd.PixelSNAIL(c["shape"], c["n_class"], *c["args"], **c["kw"])
    plain.load_state_dict({k: v for k, v in r["sd"].items() if not k.endswith("label_embed")})
    with torch.no_grad():
        want, _ = plain.cuda().eval()(codes, condition=cond)
    m.zero_grad(set_to_none=True)
    out, _ = m(codes, condition=cond, label=torch.tensor([-1, N_LABEL, -1], device="cuda"))
    assert torch.equal(out, want)
    amd.prior_loss(out, codes)[0].backward()
    assert all(float(p.grad.abs().sum()) == 0 for k, p in m.named_parameters() if k.endswith("label_embed"))


@pytest.mark.parametrize("ci", CASES, ids=CASES.values())
def test_unlabelled_model_is_what_it_was(amd, g, ref, ci):
    r = ref[ci]
    c = r["c"]
    codes, cond, label = _dev(r)
    want = M.state_dict(g, ci)
    outs = []
    for kw in ({}, {"n_label": 0}):
        m = amd.PixelSNAIL(c["shape"], c["n_class"], *c["args"], **c["kw"], **kw)
        m.load_state_dict(want, strict=True)
        assert sorted(m.state_dict()) == sorted(want)
        with torch.no_grad():
            outs.append(m.cuda().eval()(codes, condition=cond)[0].clone())
    assert torch.equal(outs[0], outs[1])
    with pytest.raises(RuntimeError, match="n_label=0"):
        m(codes, condition=cond, label=label)


@pytest.mark.parametrize("stepping", ["row", "pixel"])
@pytest.mark.parametrize("ci", CASES, ids=CASES.values())
def test_sampler_with_labels(amd, ref, ci, stepping):
    r = ref[ci]
    m = _model(amd, r)
    codes, cond, label = _dev(r)
    sampler = amd.PriorSampler(m, stepping=stepping)
    have = sampler.logits_given(codes, cond, label=label)
    f64 = r["f64"]["logits"].numpy()
    gap = float(np.abs(r["f32"]["logits"].double().numpy() - f64).max())
    err = float(np.abs(have.double().cpu().numpy() - f64).max())
    print("case %d %s stepping: err %.3e, reference gap %.3e, ratio %.2f" % (ci, stepping, err, gap, err / gap))
    assert gap > 0 and err <= 4 * gap
    # two labels: different logits already at step 0; an int is every image's label
    zero = sampler.logits_given(codes, cond, label=0)
    two = sampler.logits_given(codes, cond, label=torch.full((3,), 2, device="cuda"))
    assert not torch.equal(zero[:, :, 0, 0], two[:, :, 0, 0])
    assert torch.equal(two[0], have[0]) and torch.equal(zero[1], have[1])
    # a free run repeats bit for bit per seed, and the label buffer is refilled by every call
    a = sampler.sample(3, 1.0, cond, seed=5, label=label)
    b = sampler.sample(3, 1.0, cond, seed=5, label=1)
    assert torch.equal(a, sampler.sample(3, 1.0, cond, seed=5, label=label))
    assert torch.equal(b, sampler.sample(3, 1.0, cond, seed=5, label=torch.tensor([1, 1, 1], device="cuda")))
    assert a.shape == codes.shape and a.dtype == torch.int64 and int(a.min()) >= 0 and int(a.max()) < r["c"]["n_class"]
    via = []
    for _ in range(2):                                  # sample_model draws its seed from torch's generator
        torch.manual_seed(9)
        via.append(amd.sample_model(m, "cuda", 3, r["c"]["shape"], 1.0, cond, stepping=stepping, label=label))
    assert torch.equal(via[0], via[1]) and via[0].shape == codes.shape
    with pytest.raises(RuntimeError, match="needs `label`"):
        sampler.sample(3, 1.0, cond, seed=5)
    with pytest.raises(RuntimeError, match="label"):
        sampler.logits_given(codes, cond, label=torch.tensor([0, 1], device="cuda"))


def test_sampler_refuses_a_label_for_an_unlabelled_model(amd, g):
    c = M.cases(g)[2]
    m = amd.PixelSNAIL(c["shape"], c["n_class"], *c["args"], **c["kw"])
    m.load_state_dict(M.state_dict(g, 2))
    with pytest.raises(RuntimeError, match="n_label=0"):
        amd.PriorSampler(m.cuda().eval()).sample(1, 1.0, label=0)


@pytest.mark.parametrize("ci", CASES, ids=CASES.values())
def test_labelled_trainer_resumes_exactly(amd, ref, ci):
    r = ref[ci]
    codes, cond, label = _dev(r)
    hier = "bottom" if cond is not None else "top"
    args = (cond, codes) if cond is not None else (codes,)

    def trainer():
        return amd.Stage2Trainer(_model(amd, r, train=True), hier, lr=1e-3, sched="cycle", n_iter=8)

    def steps(tr, n, seed):
        torch.manual_seed(seed)
        return [float(tr.step(*args, label=label)["loss"]) for _ in range(n)]

    def numpy_sd(m):
        return {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}

    whole = trainer()
    l_whole = steps(whole, 2, 21) + steps(whole, 2, 22)
    first = trainer()
    l_first = steps(first, 2, 21)
    ck = first.state_dict()
    assert ck["adam_m"].numel() == sum(p.numel() for p in first.model.parameters())
    ck = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in ck.items()}
    ck["model"] = {k: v.cpu() for k, v in ck["model"].items()}
    tables = LR.table_names(ck["model"])
    assert tables == LR.table_names(r["sd"])
    for k in tables:                                    # the tables move: rows 0 and 2 (used), not row 1
        moved = (ck["model"][k] != r["sd"][k]).any(1)
        assert moved.tolist() == [True, False, True], k
    second = trainer()
    with torch.no_grad():
        for p in second.model.parameters():
            p.add_(0.25)
    second.load_state_dict(ck)
    l_second = steps(second, 2, 22)
    torch.cuda.synchronize()
    assert l_first + l_second == l_whole
    a, b = numpy_sd(second.model), numpy_sd(whole.model)
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert whole.arena.grads_ready()
    with pytest.raises(RuntimeError, match="needs `label`"):
        whole.step(*args)


@pytest.mark.parametrize("ci", CASES, ids=CASES.values())
def test_evaluator_with_labels_does_not_depend_on_the_batching(amd, ref, ci):
    r = ref[ci]
    m = _model(amd, r)
    codes, cond, label = _dev(r)
    hier = "bottom" if cond is not None else "top"

    def update(ev, sl):
        if hier == "bottom":
            return ev.update_labelled(label[sl], cond[sl], codes[sl], return_image_nll=True)
        return ev.update_labelled(label[sl], codes[sl], return_image_nll=True)

    one, cut = amd.PriorEvaluator(m, hier), amd.PriorEvaluator(m, hier)
    nll = update(one, slice(0, 3))
    parts = torch.cat([update(cut, slice(0, 2)), update(cut, slice(2, 3))])
    assert torch.equal(one._state, cut._state) and torch.equal(nll, parts)
    res = one.result()
    want = float(r["f64"]["loss"])
    assert res["images"] == 3 and abs(res["nll"] - want) <= 1e-4 * abs(want)
    score = amd.score_codes_labelled(m, codes, label, cond)
    assert torch.equal(score, -nll)
    # Stage2Trainer.evaluate takes the label as a batch's third element
    m.train()
    tr = amd.Stage2Trainer(m, hier)
    top = cond if hier == "bottom" else codes
    held = tr.evaluate([(top[:2].cpu(), codes[:2].cpu(), label[:2].cpu()), (top[2:].cpu(), codes[2:].cpu(), label[2:].cpu())])
    assert held["nll"] == res["nll"] and m.training
    with pytest.raises(RuntimeError, match="needs `label`"):
        amd.PriorEvaluator(m, hier).update(top, codes if hier == "bottom" else None)
    with pytest.raises(RuntimeError, match="needs `label`"):
        amd.score_codes(m, codes, cond)


def test_error_paths(amd, ref):
    r = ref[1]
    m = _model(amd, r)
    codes, cond, label = _dev(r)
    with pytest.raises(RuntimeError, match="needs `label`"):
        m(codes, condition=cond)
    for bad in (label.cpu(), label.int(), label[:2], label.view(3, 1), [2, 0, 2]):
        with pytest.raises(RuntimeError, match="label must be an int64 tensor"):
            m(codes, condition=cond, label=bad)
    block = m.blocks[0].resblocks[0]
    x = torch.zeros(3, r["c"]["args"][0], 4, 6, device="cuda")
    with pytest.raises(RuntimeError, match="needs `label`"):
        block(x)
    with pytest.raises(RuntimeError, match="n_label=0"):
        amd.GatedResBlock(8, 8, 3, conv="causal").cuda()(x, label=label)
