"""CPU model of the one-piece screen of conv3 (points2surf_amd/csrc/p2s_chain_screen.inl): the select with the kernel's kappa
dismisses no pool winner, and does not keep too many candidates.

The model follows the kernel's select: per item the points in order in 64-point tiles, t[p][c] = the sum over k of
fp16(h_pk) * fp16(w_ck) (products exact, eight 16-wide blocks added into an fp32 accumulator), R_c the running maximum of
t[.][c], H the running maximum of the row norms, both over the tiles so far with the current one, and (p, c) a candidate iff
t[p][c] >= R_c - mu_c * Heff with mu_c and Heff built in fp32 as p2s_screen_mu_kernel and the kernel build them.  kappa is
read from p2s_chain.hip (P2S_SCR_KAPPA), so the test follows the constant the kernel is compiled with.  The conv2 activations
come from oracle.torch_port (8 queries of the fixture cloud, the kNN patches and sub-samples of the reference golden; STN and
main pass of both encoders), conv3 has its BatchNorm folded as the engine folds it.  The fp32 values are an fp32 matrix
product (any order of at most 128 rounded products and additions is inside the margin's k_fp32).

An item with an activation beyond the half range is not screened by the kernel (it runs densely) and is left out here."""
import os
import re

import numpy as np
import pytest
import torch

from points2surf_amd import synth
from oracle import p2s_oracle as O
from oracle.torch_port import TorchPort

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NQ = 8
_CACHE = {}


def _kappa():
    with open(os.path.join(REPO, 'points2surf_amd', 'csrc', 'p2s_chain.hip')) as f:
        m = re.search(r'P2S_SCR_KAPPA\s*=\s*(0x[0-9a-fA-F.]+p[-+]?\d+)f\s*;', f.read())
    assert m, 'P2S_SCR_KAPPA not found in p2s_chain.hip'
    return np.float32(float.fromhex(m.group(1)))


def _folded_conv3(w, pre):
    """conv3 of a trunk with its bn3 folded: [1024][128] fp32"""
    W = w[pre + '.conv3.weight'][:, :, 0].astype(np.float64)
    s = w[pre + '.bn3.weight'].astype(np.float64) / np.sqrt(w[pre + '.bn3.running_var'].astype(np.float64) + 1e-5)
    return (W * s[:, None]).astype(np.float32)


@torch.no_grad()
def _passes(model, golden_dir, cloud):
    """[(name, h [NQ][P][128] fp32, w [1024][128] fp32)] of the four screened passes of ``model``"""
    if model in _CACHE:
        return _CACHE[model]
    g = np.load(os.path.join(golden_dir, 'ref_p2s_max_grid32.npz'))
    q, _ = O.query_grid(cloud, 32, 3)
    q = q[:NQ]
    _, ps = O.patch_radius_and_ps(cloud, g['knn_ids'][:NQ], q)
    sub = cloud[g['sub_ids'][:NQ]]
    w, cfg = synth.make_weights(model)
    port = TorchPort(w, cfg)
    patch = torch.as_tensor(ps).transpose(1, 2)
    shape = (torch.as_tensor(sub) - torch.as_tensor(q).unsqueeze(1)).transpose(1, 2)
    assert not cfg.get('single_transformer')
    if cfg.get('use_point_stn') and cfg.get('shared_transformer'):       # the preamble of TorchPort.forward
        r = port._qstn(torch.cat((patch, shape), dim=2), 'point_stn')
        shape, patch = torch.bmm(r, shape), torch.bmm(r, patch)
    elif cfg.get('use_point_stn'):
        r = port._qstn(shape, 'feat_global.stn1')
        shape, patch = torch.bmm(r, shape), torch.bmm(r, patch)
    out = []
    for pre, x in (('feat_global', shape.contiguous()), ('feat_local', patch.contiguous())):
        x = port._conv_bn(x, pre + '.conv0a', pre + '.bn0a')
        x = port._conv_bn(x, pre + '.conv0b', pre + '.bn0b')
        hs = port._conv_bn(port._conv_bn(x, pre + '.stn2.conv1', pre + '.stn2.bn1'), pre + '.stn2.conv2', pre + '.stn2.bn2')
        out.append((pre + '.stn2', hs.transpose(1, 2).contiguous().numpy(), _folded_conv3(w, pre + '.stn2')))
        t = port._trunk(x, pre + '.stn2')
        t = (t + torch.eye(64).view(1, 4096)).view(-1, 64, 64)
        x = torch.bmm(t, x)
        hm = port._conv_bn(port._conv_bn(x, pre + '.conv1', pre + '.bn1'), pre + '.conv2', pre + '.bn2')
        out.append((pre, hm.transpose(1, 2).contiguous().numpy(), _folded_conv3(w, pre)))
    _CACHE[model] = out
    return out


def _screen_item(h, w, kappa):
    """h [P][128], w [1024][128] fp32 -> (candidate mask [P][1024], fp32 values [P][1024]); None when the kernel would not
    screen the item (an activation beyond the half range)"""
    f32 = np.float32
    if not (np.abs(h) <= 65504.0).all():
        return None
    h16 = h.astype(np.float16).astype(np.float64)
    w16 = w.astype(np.float16).astype(np.float64)
    t = np.zeros((h.shape[0], 1024), np.float32)
    for kb in range(8):                                   # one MFMA per k-block: 16 exact products into the fp32 accumulator
        k = slice(16 * kb, 16 * kb + 16)
        t = (t.astype(np.float64) + h16[:, k] @ w16[:, k].T).astype(np.float32)
    v32 = (torch.from_numpy(h) @ torch.from_numpy(w).t()).numpy()
    # margin coefficient and H as the device builds them
    norm = f32(np.sqrt((w.astype(np.float64) ** 2).sum(1)) * (1.0 + 2.0 ** -20)).astype(np.float32)
    mu_c = (f32(2.0) * kappa * (norm * f32(1.0 + 2.0 ** -10) + f32(2.0 ** -10))).astype(np.float32)
    hsq = (h.astype(np.float32) ** 2).sum(1, dtype=np.float32)
    cand = np.zeros(t.shape, bool)
    R = np.full(1024, -np.inf, np.float32)
    Hsq = f32(0.0)
    for p0 in range(0, h.shape[0], 64):
        rows = slice(p0, min(p0 + 64, h.shape[0]))
        Hsq = max(Hsq, hsq[rows].max())
        Heff = f32(np.sqrt(Hsq)) * f32(1.0 + 2.0 ** -10) + f32(2.0 ** -10)
        R = np.maximum(R, t[rows].max(0))
        thr = (R - mu_c * f32(Heff)).astype(np.float32)
        cand[rows] = t[rows] >= thr[None, :]
    return cand, v32


def _no_winner_dismissed(cand, v32, what):
    """the largest fp32 value of a column is the value of a candidate row -- of ANY of the rows that hold it, ties included.  The
    comparison is exact on purpose: v32 is one fp32 evaluation of every product (torch's order, not the device's fmaf chain),
    and the margin must keep the winner of every such evaluation, since each lies within k_fp32 of the real-number product;
    which row wins a near tie may differ from the device, that some holder of the maximum is kept may not"""
    best = v32.max(0)
    kept = np.where(cand, v32, -np.inf).max(0)
    bad = np.nonzero(kept != best)[0]
    assert bad.size == 0, '%s: the fp32 maximum of channels %s is not among the candidates' % (what, bad[:8].tolist())


@pytest.mark.parametrize('model', ['p2s_max'] + list(synth.STRESS_MODELS))
def test_no_winner_is_dismissed(model, golden_dir, fixture_cloud):
    kappa = _kappa()
    screened = 0
    for name, h, w in _passes(model, golden_dir, fixture_cloud):
        for i in range(h.shape[0]):
            r = _screen_item(h[i], w, kappa)
            if r is None:
                continue
            screened += 1
            _no_winner_dismissed(r[0], r[1], '%s %s item %d' % (model, name, i))
    print('%s: %d of %d items screened' % (model, screened, 4 * NQ))
    assert screened > 0


def test_candidates_per_channel_on_default_weights(golden_dir, fixture_cloud):
    """a condition, not a measurement: at most 16 candidates per pooled channel, mean over the four passes"""
    kappa = _kappa()
    n = items = 0
    for name, h, w in _passes('p2s_max', golden_dir, fixture_cloud):
        per = []
        for i in range(h.shape[0]):
            r = _screen_item(h[i], w, kappa)
            assert r is not None
            per.append(r[0].sum() / 1024.0)
        print('%s (P = %d): %.2f candidates per channel' % (name, h.shape[1], float(np.mean(per))))
        n += float(np.sum(per))
        items += len(per)
    mean = n / items
    print('kappa = %g * 2^-10: %.2f candidates per channel over the four passes' % (float(kappa) * 1024.0, mean))
    assert mean <= 16.0


@pytest.mark.parametrize('scale', [2.0 ** -16, 2.0 ** -20])
def test_rows_in_the_subnormal_range_of_fp16(scale, golden_dir, fixture_cloud):
    """conv2 rows times 2^-16 / 2^-20: their fp16 roundings are subnormal or zero, the margin's absolute terms pay for it"""
    kappa = _kappa()
    for name, h, w in _passes('p2s_max', golden_dir, fixture_cloud):
        for i in range(h.shape[0]):
            hs = (h[i] * np.float32(scale)).astype(np.float32)
            cand, v32 = _screen_item(hs, w, kappa)
            _no_winner_dismissed(cand, v32, '%s item %d x %g' % (name, i, scale))
