"""Recorded outputs of the chain kernels' small layers (conv0a .. conv2) for tests/test_gpu_chain_small_layers.py.

The bit-equality tests of the chain kernels compare the screened, the dense and the stem-reusing paths with each other, and all
of them share layer_k64 and the epilogues around it: a change of those is pinned against values recorded from the commit
BEFORE it.  Run on a GPU from a checkout of that commit (or with P2S_LIB_PATH naming its library):

    python tools/make_chain_small_layers_golden.py [FILE]     # default: tests/golden/chain_small_layers_parent.npz

Chunks of 3 queries with seeded inputs (numpy's legacy generator: the same on every machine); per case both pooled STN features
(p2s_debug_stn_pool), both pooled main features and the logits.  Sizes (patch / sub-sample points) cover every row-tile and tail
form of the small layers: a single point, a tile of at most 32 rows, a full tile, a 16-row tail, several tiles.  p2s_max runs
with its default and its adversarial weights as three handles -- stem reuse on, off, and P2S_CONV3_DENSE=1; the three must
agree to the bit at the recording commit (asserted here), so the file keeps one set of arrays per (weights, size) and the test
compares each handle with it.  The test imports the case list and the runner from this file."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'chain_small_layers_parent.npz')
SEED = 20261020
NQ = 3
SIZES = ((1, 40), (33, 64), (64, 65), (65, 129), (113, 200))
KEYS = ('stn_pool', 'feat_local', 'feat_global', 'logits')
HANDLES = (('reuse', {}), ('recompute', {'stem_reuse': False}), ('dense', {'dense': True}))


def cases():
    """(case id, model, patch points, sub-sample points, handles, NaN coordinate)"""
    out = []
    for model in ('p2s_max', 'p2s_max_stress'):
        for k, n in SIZES:
            out.append(('%s_%d_%d' % (model, k, n), model, k, n, HANDLES, False))
    out.append(('p2s_max_sum_65_129', 'p2s_max_sum', 65, 129, HANDLES[:1], False))
    out.append(('p2s_vanilla_33_64', 'p2s_vanilla', 33, 64, HANDLES[:1], False))
    out.append(('p2s_max_65_129_nan', 'p2s_max', 65, 129, HANDLES[:1], True))
    return out


def inputs(k, n, nan):
    """the chunk of a case as numpy arrays: patch [3, k, 3] in the unit ball's cube, sub-sample [3, n, 3], queries, radii"""
    rs = np.random.RandomState(SEED + 1000 * k + n)
    patch = (rs.random_sample((NQ, k, 3)) * 2 - 1).astype(np.float32)
    sub = (rs.random_sample((NQ, n, 3)) - 0.5).astype(np.float32)
    q = (rs.random_sample((NQ, 3)) * 0.2).astype(np.float32)
    rad = (rs.random_sample((NQ,)) * 0.1 + 0.05).astype(np.float32)
    if nan:
        patch[1, k - 1, 2] = np.nan          # the single point of the patch's second tile
    return patch, sub, q, rad


def model(engine, w, cfg, dense=False, **stem):
    """a handle with the given stem setting (configuration) and conv3 (P2S_CONV3_DENSE: read at creation)"""
    old = os.environ.get('P2S_CONV3_DENSE')
    os.environ['P2S_CONV3_DENSE'] = '1' if dense else '0'
    try:
        return engine.Model(w, dict(cfg, **stem))
    finally:
        if old is None:
            del os.environ['P2S_CONV3_DENSE']
        else:
            os.environ['P2S_CONV3_DENSE'] = old


def run_case(engine, synth, case, weights_cache=None):
    """{handle name: {key: array}} of one case"""
    import torch
    _, name, k, n, handles, nan = case
    weights_cache = weights_cache if weights_cache is not None else {}
    if name not in weights_cache:
        weights_cache[name] = synth.make_weights(name)
    w, cfg = weights_cache[name]
    cfg = dict(cfg, points_per_patch=k, sub_sample_size=n)
    patch, sub, q, rad = (torch.from_numpy(a).cuda() for a in inputs(k, n, nan))
    out = {}
    for hname, env in handles:
        m = model(engine, w, cfg, **env)
        lg = m.forward(patch, sub, q, rad, want_sdf=False)
        lg = lg[0] if isinstance(lg, (tuple, list)) else lg
        stn = m.debug_stn_pool(NQ)
        torch.cuda.synchronize()
        fl, fg = m.features(patch, sub, q)
        torch.cuda.synchronize()
        out[hname] = {'stn_pool': stn.cpu().numpy(), 'feat_local': fl.cpu().numpy(), 'feat_global': fg.cpu().numpy(),
                      'logits': lg.cpu().numpy()}
        m.close()
    return out


def main():
    sys.path.insert(0, ROOT)
    from points2surf_amd import engine, synth
    arrays, cache = {}, {}
    for case in cases():
        res = run_case(engine, synth, case, cache)
        first = res[case[4][0][0]]
        for hname, r in res.items():
            for key in KEYS:
                assert np.array_equal(first[key], r[key], equal_nan=True), (case[0], hname, key)
        for key in KEYS:
            arrays['%s/%s' % (case[0], key)] = first[key]
        print(case[0], {key: first[key].shape for key in KEYS}, 'NaN values: %d' % sum(int(np.isnan(first[key]).sum()) for key in KEYS))
    dst = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    np.savez_compressed(dst, **arrays)
    print(dst, os.path.getsize(dst), 'bytes')


if __name__ == '__main__':
    main()
