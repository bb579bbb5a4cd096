"""Host side of the prior's held-out evaluation, no GPU: the two C entry points and their refusals, the fp64 finish of
PriorEvaluator.result() on a hand-made state buffer, the command lines of the two example scripts, and the float64 row
reference of tests/_prior_eval_ref.py against torch's own cross-entropy and a brute-force rank."""
import ctypes
import importlib.util
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _prior_eval_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


def _example(name):
    spec = importlib.util.spec_from_file_location(name + "_example", os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_entry_points_are_declared_bound_and_refuse_bad_arguments(amd):
    hdr = open(os.path.join(ROOT, "include", "vq2.h")).read()
    P, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    want = {"vq2_prior_eval_rows": (ctypes.c_int, [P, I32, P, I64, I32, P, P, P, P]),
            "vq2_prior_eval_accumulate": (ctypes.c_int, [P, P, P, I32, I32, I32, P, P, P, P, P, P, P])}
    raw = ctypes.CDLL(amd._lib.LIB_PATH)
    for name, (res, args) in want.items():
        assert hasattr(raw, name) and name in amd._lib.EXPORTS, name
        fn = getattr(amd._lib.lib, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
        decl = hdr[hdr.index("int " + name + "("):]
        decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)
        assert decl.count(",") + 1 == len(args), f"{name}: vq2.h declares {decl.count(',') + 1} arguments"
    assert amd._lib.API_VERSION >= 15
    L = amd._lib.lib
    backing = ctypes.create_string_buffer(4096 + 16)
    d = ctypes.c_void_p((ctypes.addressof(backing) + 15) & ~15)
    off4 = ctypes.c_void_p(d.value + 4)
    # refusals come before any launch (no GPU here)
    assert L.vq2_prior_eval_rows(None, 8, d, 1, 6, d, d, d, None) == 1 and b"null pointer" in L.vq2_last_error()
    assert L.vq2_prior_eval_rows(d, 8, d, 1, 6, d, None, d, None) == 1
    assert L.vq2_prior_eval_rows(d, 8, d, 0, 6, d, d, d, None) == 1
    assert L.vq2_prior_eval_rows(d, 8, d, 1, 0, d, d, d, None) == 1
    assert L.vq2_prior_eval_rows(d, 16388, d, 1, 16385, d, d, d, None) == 1 and b"16384" in L.vq2_last_error()
    assert L.vq2_prior_eval_rows(d, 4, d, 1, 6, d, d, d, None) == 1 and b"stride" in L.vq2_last_error()     # ld < ceil4(6)
    assert L.vq2_prior_eval_rows(d, 10, d, 1, 6, d, d, d, None) == 1 and b"stride" in L.vq2_last_error()    # ld % 4
    assert L.vq2_prior_eval_rows(off4, 8, d, 1, 6, d, d, d, None) == 1 and b"aligned" in L.vq2_last_error()
    acc = L.vq2_prior_eval_accumulate
    assert acc(None, d, d, 1, 1, 1, d, d, d, d, d, None, None) == 1 and b"null pointer" in L.vq2_last_error()
    assert acc(d, d, d, 1, 1, 1, d, d, d, d, None, None, None) == 1
    assert acc(d, d, d, 0, 1, 1, d, d, d, d, d, None, None) == 1
    assert acc(d, d, d, 1, 0, 1, d, d, d, d, d, None, None) == 1
    assert acc(d, d, d, 1, 1, 0, d, d, d, d, d, None, None) == 1
    assert acc(d, d, d, 1 << 16, 1 << 15, 1, d, d, d, d, d, None, None) == 1
    assert acc(d, d, d, 1, 1, 1, off4, d, d, d, d, None, None) == 1 and b"aligned" in L.vq2_last_error()


def test_python_surface(amd):
    assert amd.PriorEvaluator is amd.evaluate.PriorEvaluator and amd.score_codes is amd.evaluate.score_codes
    assert list(inspect.signature(amd.PriorEvaluator.__init__).parameters) == ["self", "model", "hier", "top_k"]
    assert list(inspect.signature(amd.PriorEvaluator.update).parameters) == ["self", "top", "bottom", "return_image_nll"]
    assert list(inspect.signature(amd.score_codes).parameters) == ["model", "codes", "condition"]
    assert list(inspect.signature(amd.Stage2Trainer.evaluate).parameters) == ["self", "batches", "top_k"]
    assert inspect.signature(amd.Stage2Trainer.evaluate).parameters["top_k"].default == 5
    for fn in (amd.ops.prior_eval_rows, amd.ops.prior_eval_accumulate):
        assert inspect.isfunction(fn)                      # plain functions, not autograd Functions
    with pytest.raises(RuntimeError):
        amd.ops.prior_eval_rows(torch.zeros(1, 2, 2, 8), torch.zeros(1, 2, 2, dtype=torch.int64), 6)     # no CPU path
    with pytest.raises(ValueError):
        amd.PriorEvaluator(torch.nn.Linear(1, 1), "middle")


def _hand_state(amd, h, w, n_class, pos_nll, pos_entropy, hit1, hitk, images, bad, counts, flag=0):
    n = h * w
    s = torch.zeros(amd.PriorEvaluator.state_len(n, n_class), dtype=torch.int64)
    assert s.numel() == 4 * n + 2 + n_class + 1
    s[:n] = torch.tensor(pos_nll, dtype=torch.float64).view(torch.int64)
    s[n:2 * n] = torch.tensor(pos_entropy, dtype=torch.float64).view(torch.int64)
    s[2 * n:3 * n] = torch.tensor(hit1)
    s[3 * n:4 * n] = torch.tensor(hitk)
    s[4 * n], s[4 * n + 1] = images, bad
    s[4 * n + 2:4 * n + 2 + n_class] = torch.tensor(counts)
    s[-1] = flag
    return s


def test_host_finish_on_a_hand_made_state(amd):
    finish = amd.PriorEvaluator.finish
    h, w, k, images = 2, 3, 4, 8
    pos_nll = [8.0, 4.0, 2.0, 16.0, 1.0, 1.0]                   # the sum over 8 images at each of the 6 positions
    pos_entropy = [4.0, 4.0, 4.0, 2.0, 1.0, 1.0]
    hit1, hitk = [8, 4, 0, 2, 1, 1], [8, 8, 0, 4, 2, 2]
    counts = [24, 12, 12, 0]                                    # 48 codes: p = 1/2, 1/4, 1/4
    r = finish(_hand_state(amd, h, w, k, pos_nll, pos_entropy, hit1, hitk, images, 0, counts), (h, w), k, 3)
    assert r["images"] == 8 and r["codes"] == 48 and r["top_k"] == 3
    assert r["nll"] == 32.0 / 48 and r["bits_per_code"] == (32.0 / 48) / math.log(2.0)
    assert r["perplexity"] == math.exp(32.0 / 48)
    assert r["entropy"] == 16.0 / 48
    assert r["accuracy"] == 16 / 48 and r["top_k_accuracy"] == 24 / 48
    assert abs(r["unigram_nll"] - 1.5 * math.log(2.0)) <= 1e-15                # 1/2 ln 2 + 2 * 1/4 ln 4
    assert r["nll_map"].dtype == torch.float64 and tuple(r["nll_map"].shape) == (2, 3)
    assert r["nll_map"].tolist() == [[1.0, 0.5, 0.25], [2.0, 0.125, 0.125]]
    assert r["nll_rows"] == [(1.0 + 0.5 + 0.25) / 3, (2.0 + 0.125 + 0.125) / 3]
    assert r["counts"].tolist() == counts and r["counts"].dtype == torch.int64
    # top_k is clamped to n_class
    assert finish(_hand_state(amd, h, w, k, pos_nll, pos_entropy, hit1, hitk, images, 0, counts), (h, w), k, 600)["top_k"] == 4
    assert amd.PriorEvaluator(type("M", (), {"n_class": 6})(), "top", top_k=600).top_k == 6
    # a target outside the classes, seen by either kernel, is an error
    with pytest.raises(RuntimeError, match="outside"):
        finish(_hand_state(amd, h, w, k, pos_nll, pos_entropy, hit1, hitk, images, 2, counts), (h, w), k, 3)
    with pytest.raises(RuntimeError, match="outside"):
        finish(_hand_state(amd, h, w, k, pos_nll, pos_entropy, hit1, hitk, images, 0, counts, flag=1), (h, w), k, 3)
    with pytest.raises(ValueError):
        finish(torch.zeros(5, dtype=torch.int64), (h, w), k, 3)
    # no batch seen: NaNs and zeros
    e = finish(torch.zeros(amd.PriorEvaluator.state_len(6, k), dtype=torch.int64), (h, w), k, 3)
    assert e["images"] == 0 and e["codes"] == 0 and e["counts"].tolist() == [0, 0, 0, 0]
    for key in ("nll", "bits_per_code", "perplexity", "accuracy", "top_k_accuracy", "entropy", "unigram_nll"):
        assert math.isnan(e[key]), key
    assert bool(torch.isnan(e["nll_map"]).all()) and all(math.isnan(v) for v in e["nll_rows"]) and len(e["nll_rows"]) == 2
    line = amd.PriorEvaluator.summary(r)
    assert "\n" not in line and "bits/code" in line and "top3" in line


def test_position_sums_are_taken_in_ascending_order(amd):
    # 1e16 + 1 + 1 ... : only the ascending order loses every 1.0
    h, w = 1, 5
    r = amd.PriorEvaluator.finish(_hand_state(amd, h, w, 2, [1e16, 1.0, 1.0, 1.0, -1e16], [0.0] * 5, [0] * 5, [0] * 5, 1, 0,
                                              [5, 0]), (h, w), 2, 1)
    assert r["nll"] == 0.0


def test_example_command_lines(amd):
    train = _example("train_pixelsnail")
    old = train.parse_args(["codes.db"])
    assert (old.val_path, old.eval_every) == (None, 0)                         # off: the old command line runs as before
    assert (old.batch, old.epoch, old.hier, old.lr, old.max_steps, old.path) == (32, 420, "top", 3e-4, 0, "codes.db")
    new = train.parse_args(["--val_path", "val.db", "--eval_every", "50", "--hier", "bottom", "codes.db"])
    assert (new.val_path, new.eval_every, new.hier, new.path) == ("val.db", 50, "bottom", "codes.db")
    ev = _example("eval_pixelsnail")
    a = ev.parse_args(["--ckpt", "pixelsnail_top_001.pt", "codes.db"])
    assert (a.ckpt, a.hier, a.batch, a.top_k, a.dump_map, a.path) == ("pixelsnail_top_001.pt", "top", 32, 5, None, "codes.db")
    b = ev.parse_args(["--ckpt", "x.pt", "--hier", "bottom", "--batch", "8", "--top_k", "3", "--dump_map", "m.npy", "c.db"])
    assert (b.hier, b.batch, b.top_k, b.dump_map, b.path) == ("bottom", 8, 3, "m.npy", "c.db")
    with pytest.raises(SystemExit):
        ev.parse_args(["codes.db"])                                            # --ckpt is required


@pytest.mark.parametrize("n_class", [1, 6, 513])
def test_row_reference_against_torch_and_brute_force(n_class):
    g = torch.Generator().manual_seed(n_class)
    m = 37
    logits = (torch.randn(m, n_class, generator=g) * 3).float()
    logits[3] = logits[3].round()                                              # a row with many ties
    target = torch.randint(0, n_class, (m,), generator=g)
    nll, entropy, rank = E.row_quantities(logits, target)
    want = F.cross_entropy(logits.double(), target, reduction="none")
    assert float((nll - want).abs().max()) <= 1e-13 * max(1.0, float(want.abs().max()))
    p = F.softmax(logits.double(), 1)
    h = -(p * F.log_softmax(logits.double(), 1)).sum(1)
    assert float((entropy - h).abs().max()) <= 1e-13 * max(1.0, float(h.max()))
    assert torch.equal(rank, E.brute_rank(logits, target))
    lowest_max = (logits == logits.max(1, keepdim=True)[0]).to(torch.uint8).argmax(1)     # the first index of the maximum
    assert torch.equal(rank == 0, lowest_max == target)
    if n_class == 1:
        assert float(nll.abs().max()) == 0 and float(entropy.abs().max()) == 0 and int(rank.abs().max()) == 0
    # ties: 2, 5 and 9 share the target's value -> one class beats target 5; an all-equal row gives rank t
    if n_class >= 10:
        row = torch.full((1, n_class), -1.0)
        row[0, [2, 5, 9]] = 4.0
        assert E.row_quantities(row, torch.tensor([5]))[2].tolist() == [1]
        flat = torch.zeros(3, n_class)
        assert E.row_quantities(flat, torch.tensor([0, 7, n_class - 1]))[2].tolist() == [0, 7, n_class - 1]
    # out of range: nll 0, rank -1, entropy as computed
    o = E.row_quantities(logits[:2], torch.tensor([-1, n_class]))
    assert o[0].tolist() == [0.0, 0.0] and o[2].tolist() == [-1, -1] and torch.equal(o[1], entropy[:2])
    # the float32 statement of the same formula stays close to it
    n32, h32, r32 = E.row_quantities(logits, target, torch.float32)
    assert n32.dtype == torch.float32 and torch.equal(r32, rank)
    assert float((n32.double() - nll).abs().max()) <= 1e-5 and float((h32.double() - entropy).abs().max()) <= 1e-5


def test_accumulate_reference_does_not_depend_on_the_batching():
    rng = np.random.default_rng(3)
    n, length = 9, 7
    nll = rng.random((n, length), dtype=np.float32) * 9
    ent = rng.random((n, length), dtype=np.float32) * 5
    rank = rng.integers(-1, 6, (n, length)).astype(np.int32)
    whole = E.new_state(length)
    image = E.accumulate(whole, nll, ent, rank, n, length, 3)
    parts, images, lo = E.new_state(length), [], 0
    for b in (5, 3, 1):
        images.append(E.accumulate(parts, nll[lo:lo + b], ent[lo:lo + b], rank[lo:lo + b], b, length, 3))
        lo += b
    for k in whole:
        assert whole[k].tobytes() == parts[k].tobytes(), k
    assert np.concatenate(images).tobytes() == image.tobytes()
    assert whole["counters"].tolist() == [9, int((rank == -1).sum())]
    assert int(whole["pos_hit1"].sum()) == int((rank == 0).sum())
    assert int(whole["pos_hitk"].sum()) == int(((rank >= 0) & (rank < 3)).sum())
