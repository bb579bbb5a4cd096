"""CPU checks of the truncated draw's reference (tests/_sample_filter_ref.py): the threshold form of the kept set against the
plain sort-based definition on random rows and on crafted ties at the cut, a worked nucleus case, the restricted draw, and the
library's declaration of vq2_sample_filtered with the refusals that reach no kernel."""
import ctypes
import math

import numpy as np
import pytest

import _sample_filter_ref as F

SETTINGS = [(0, 1.0), (1, 1.0), (3, 1.0), (7, 1.0), (0, 0.05), (0, 0.5), (0, 0.9), (0, 0.999), (5, 0.5), (12, 0.9), (1, 0.5)]


def halves(n):
    """l_c = -c ln 2: masses 1/2, 1/4, ... (of a total 1 - 2^-n)."""
    return -np.arange(n) * math.log(2.0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_threshold_form_equals_the_sort_based_definition_on_random_rows(dtype):
    rng = np.random.default_rng(11)
    for n in (1, 2, 5, 37, 200):
        for _ in range(6):
            z = (rng.standard_normal(n) * 3).astype(dtype)
            for top_k, top_p in SETTINGS:
                k = min(top_k, n)
                a, b = F.kept_mask(z, k, top_p), F.kept_mask_by_sorting(z, k, top_p)
                assert np.array_equal(a, b), (n, k, top_p)
                assert a[np.argmax(z)]                                      # the arg-max is always kept
                assert not a.any() or z[a].min() >= z[~a].max(initial=-np.inf)  # an upper set of z
                if top_p == 1.0 and k:
                    assert a.sum() == k                                     # no ties in a random row


def test_ties_at_the_cut_are_kept():
    #            0    1    2    3    4    5    6    7
    z = np.array([1.0, 3.0, 2.0, 3.0, 2.0, 0.0, 2.0, -np.inf])
    assert F.kept_mask(z, 1).tolist() == [False, True, False, True, False, False, False, False]      # both 3s
    assert F.kept_mask(z, 2).sum() == 2
    for k in (3, 4, 5):                                                     # the k-th value is one of the three 2s
        assert F.kept_mask(z, k).tolist() == [False, True, True, True, True, False, True, False], k
    assert F.kept_mask(z, 6).sum() == 6 and F.kept_mask(z, 7).sum() == 7 and F.kept_mask(z, 8).all() and F.kept_mask(z, 0).all()
    for k in range(9):
        for p in (0.3, 0.6, 0.8, 0.95, 1.0):
            assert np.array_equal(F.kept_mask(z, k, p), F.kept_mask_by_sorting(z, k, p)), (k, p)
    # nucleus ties: two classes of mass 0.4 each and one of 0.2; any p < 0.8 keeps the tied pair, never one of them
    z = np.log(np.array([0.4, 0.2, 0.4]))
    for p in (0.1, 0.4, 0.41, 0.79):
        assert F.kept_mask(z, 0, p).tolist() == [True, False, True], p
    assert F.kept_mask(z, 0, 0.81).all()
    # top-p acts on the distribution over K: with top_k = 2 of masses 1/2, 1/4, 1/8, ... the first holds 2/3 of K
    z = halves(12)
    assert F.kept_count(z, 2, 0.66) == 1 and F.kept_count(z, 2, 0.67) == 2


def test_row_batched_counts_equal_the_row_form():
    rng = np.random.default_rng(5)
    for n in (1, 5, 64, 130):
        z = rng.standard_normal((9, n)) * 3
        z[1:4] = np.round(z[1:4])                                           # rows full of ties
        z[4, 3::3] = -np.inf
        for top_k, top_p in SETTINGS:
            k = min(top_k, n)
            want = [F.kept_count(row, k, top_p) for row in z]
            assert F.kept_counts(z, k, top_p).tolist() == want, (n, k, top_p)
            assert [int(F.kept_mask_by_sorting(row, k, top_p).sum()) for row in z] == want, (n, k, top_p)


@pytest.mark.parametrize("n", [8, 12, 512, 1000])
def test_worked_nucleus_case(n):
    z = halves(n)                                 # n >= 8: the total 1 - 2^-n is close enough to 1 for the cuts below
    assert F.kept_count(z, 0, 0.7) == 2           # 1/2 < 0.7 <= 3/4
    assert F.kept_count(z, 0, 0.5) == 1           # 1/2 of a total just below 1
    assert F.kept_count(z, 0, 0.76) == 3          # 3/4 < 0.76 <= 7/8
    assert F.kept_count(z, 0, 1.0) == n
    assert F.kept_mask(z, 0, 0.7).tolist() == [True, True] + [False] * (n - 2)
    assert F.kept_count(z.astype(np.float32), 0, 0.7) == 2


def test_restricted_draw():
    z = np.log(np.array([0.1, 0.4, 0.05, 0.3, 0.15]))
    # top_k = 2 keeps classes 1 and 3 with probabilities 4/7 and 3/7
    assert F.draw(z, 0.0, 2) == (1, pytest.approx(math.log(4 / 7)))
    assert F.draw(z, 0.57, 2)[0] == 1 and F.draw(z, 0.58, 2)[0] == 3
    assert F.draw(z, np.nextafter(1.0, 0.0), 2) == (3, pytest.approx(math.log(3 / 7)))
    assert F.draw(z, 0.999, 1) == (1, 0.0)                                  # greedy: probability 1
    # filters off: the plain rule cumsum(p) > u
    p = np.exp(z) / np.exp(z).sum()
    for u in np.linspace(0, 1, 101, endpoint=False):
        c, lp = F.draw(z, u)
        assert c == int(np.nonzero(np.cumsum(p) > u)[0][0]) and lp == pytest.approx(math.log(p[c]))
    # never a removed class, whatever u
    for u in np.linspace(0, 1, 101, endpoint=False):
        assert F.draw(z, u, 0, 0.6)[0] in (1, 3)
    assert F.draw(np.array([0.0, -np.inf, 0.0]), 0.75)[0] == 2              # -inf carries no mass


def test_library_declares_the_filtered_draw():
    import vqvae2_amd as amd
    L = amd._lib
    P, I32, I64, Fl, U64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_uint64
    assert "vq2_sample_filtered" in L.EXPORTS
    fn = L.lib.vq2_sample_filtered
    assert fn.restype == ctypes.c_int and list(fn.argtypes) == [P, I64, I32, I32, Fl, I32, Fl, U64, U64, P, I64, P, P, P]
    assert L.API_VERSION >= 14
    one = ctypes.c_void_p(16)
    # refused before any launch
    for top_k, top_p in ((-1, 1.0), (9, 1.0), (0, 0.0), (0, -0.1), (0, 1.5), (0, float("nan"))):
        assert fn(one, 8, 1, 8, 1.0, top_k, top_p, 1, 0, one, 1, None, None, None) == 1, (top_k, top_p)
        assert b"top_" in L.lib.vq2_last_error()
    assert fn(one, 8, 1, 8, 0.0, 0, 1.0, 1, 0, one, 1, None, None, None) == 1            # what the plain draw refuses
    assert fn(one, 16385, 1, 16385, 1.0, 0, 1.0, 1, 0, one, 1, None, None, None) == 1
    assert fn(None, 8, 1, 8, 1.0, 0, 1.0, 1, 0, one, 1, None, None, None) == 1
