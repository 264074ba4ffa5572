"""CPU model of the pool bound in the select of the screened conv3 (points2surf_amd/csrc/p2s_chain_screen.inl): from the second
tile of an item on, (p, c) is a candidate iff t[p][c] >= max(R_c - mu_c, E_c - mu_c / 2), E_c the exact fp32 maximum of the rows
confirmed in the EARLIER tiles.  The bound dismisses no pool winner, only narrows the R rule, and narrows it enough.

The model is the one of tests/test_conv3_screen_margin_cpu.py (its inputs, its screen values t, its fp32 values, kappa read
from p2s_chain.hip) with the second term: per 64-point tile the threshold is formed in fp32 as the kernel forms it (mu = mu_c *
Heff, max(R - mu, E - 0.5 mu); E = -inf before the first confirm leaves the R rule), the rows the rule keeps are "confirmed" and
E is raised by THEIR fp32 values after the tile.  The fp32 values are one fp32 matrix product: any order of 128 rounded products
and additions lies within the margin's k_fp32, so the rule must keep the winner of this evaluation too.

Each item also runs with its points reversed: the record holder then tends to come last and E is as low as it gets."""
import numpy as np
import pytest
import torch

from points2surf_amd import synth
from test_conv3_screen_margin_cpu import NQ, _kappa, _no_winner_dismissed, _passes


def _screen_item_pool(h, w, kappa):
    """h [P][128], w [1024][128] fp32 -> (R-rule mask, R-and-E-rule mask, fp32 values), each [P][1024]; None when the kernel would
    not screen the item (an activation beyond the half range)"""
    f32 = np.float32
    if not (np.abs(h) <= 65504.0).all():
        return None
    h16 = h.astype(np.float16).astype(np.float64)
    w16 = w.astype(np.float16).astype(np.float64)
    t = np.zeros((h.shape[0], 1024), np.float32)
    for kb in range(8):                                   # one MFMA per k-block: 16 exact products into the fp32 accumulator
        k = slice(16 * kb, 16 * kb + 16)
        t = (t.astype(np.float64) + h16[:, k] @ w16[:, k].T).astype(np.float32)
    v32 = (torch.from_numpy(np.ascontiguousarray(h)) @ torch.from_numpy(w).t()).numpy()
    norm = f32(np.sqrt((w.astype(np.float64) ** 2).sum(1)) * (1.0 + 2.0 ** -20)).astype(np.float32)
    mu_c = (f32(2.0) * kappa * (norm * f32(1.0 + 2.0 ** -10) + f32(2.0 ** -10))).astype(np.float32)
    hsq = (h.astype(np.float32) ** 2).sum(1, dtype=np.float32)
    cand_r = np.zeros(t.shape, bool)
    cand_e = np.zeros(t.shape, bool)
    R = np.full(1024, -np.inf, np.float32)
    E = np.full(1024, -np.inf, np.float32)
    Hsq = f32(0.0)
    for p0 in range(0, h.shape[0], 64):
        rows = slice(p0, min(p0 + 64, h.shape[0]))
        Hsq = max(Hsq, hsq[rows].max())
        Heff = f32(np.sqrt(Hsq)) * f32(1.0 + 2.0 ** -10) + f32(2.0 ** -10)
        R = np.maximum(R, t[rows].max(0))
        mu = (mu_c * f32(Heff)).astype(np.float32)
        thr_r = (R - mu).astype(np.float32)
        thr_e = (E - f32(0.5) * mu).astype(np.float32)    # E of the earlier tiles only
        assert thr_r.dtype == np.float32 and thr_e.dtype == np.float32
        cand_r[rows] = t[rows] >= thr_r[None, :]
        cand_e[rows] = t[rows] >= np.maximum(thr_r, thr_e)[None, :]
        E = np.maximum(E, np.where(cand_e[rows], v32[rows], -np.inf).max(0).astype(np.float32))
    return cand_r, cand_e, v32


def _orders(h):
    return (('in order', h), ('reversed', np.ascontiguousarray(h[::-1])))


def _check_item(h, w, kappa, what):
    """-> (candidates of the R rule, of the pool bound) or None for an item the kernel does not screen"""
    r = _screen_item_pool(h, w, kappa)
    if r is None:
        return None
    cand_r, cand_e, v32 = r
    assert not (cand_e & ~cand_r).any(), '%s: the pool bound keeps a product the R rule dismisses' % what
    _no_winner_dismissed(cand_e, v32, what)
    return int(cand_r.sum()), int(cand_e.sum())


@pytest.mark.parametrize('model', ['p2s_max'] + list(synth.STRESS_MODELS))
def test_no_winner_is_dismissed_and_the_bound_only_narrows(model, golden_dir, fixture_cloud):
    kappa = _kappa()
    screened = 0
    for name, h, w in _passes(model, golden_dir, fixture_cloud):
        for i in range(h.shape[0]):
            for order, hi in _orders(h[i]):
                if _check_item(hi, w, kappa, '%s %s item %d %s' % (model, name, i, order)) is not None:
                    screened += 1
    print('%s: %d of %d item runs screened' % (model, screened, 2 * 4 * NQ))
    assert screened > 0


@pytest.mark.parametrize('scale', [2.0 ** -16, 2.0 ** -20])
def test_rows_in_the_subnormal_range_of_fp16(scale, golden_dir, fixture_cloud):
    """conv2 rows times 2^-16 / 2^-20: the absolute terms of mu / 2 pay for the subnormal roundings against an exact E"""
    kappa = _kappa()
    for name, h, w in _passes('p2s_max', golden_dir, fixture_cloud):
        for i in range(h.shape[0]):
            for order, hi in _orders((h[i] * np.float32(scale)).astype(np.float32)):
                assert _check_item(hi, w, kappa, '%s item %d x %g %s' % (name, i, scale, order)) is not None


def test_the_bound_removes_a_quarter_of_the_candidates_of_the_long_passes(golden_dir, fixture_cloud):
    """a condition: on the default weights each of the two 1000-point passes keeps at most 0.75 of the R rule's candidates
    (measured when the rule was derived: 0.63 and 0.60; the 300-point passes, five tiles, gain little and carry no condition)"""
    kappa = _kappa()
    long_passes = 0
    for name, h, w in _passes('p2s_max', golden_dir, fixture_cloud):
        n_r = n_e = n_e_rev = 0
        for i in range(h.shape[0]):
            (_, hi), (_, hr) = _orders(h[i])
            a = _check_item(hi, w, kappa, '%s item %d' % (name, i))
            b = _check_item(hr, w, kappa, '%s item %d reversed' % (name, i))
            assert a is not None and b is not None
            n_r, n_e, n_e_rev = n_r + a[0], n_e + a[1], n_e_rev + b[1]
        per = 1.0 / (1024.0 * h.shape[0])
        print('%s (P = %d): %.2f candidates per channel by the R rule, %.2f with the pool bound (%.3f of them; reversed: %.2f)' % (
            name, h.shape[1], n_r * per, n_e * per, n_e / n_r, n_e_rev * per))
        if h.shape[1] == 1000:
            long_passes += 1
            assert n_e <= 0.75 * n_r, name
    assert long_passes == 2
