"""Recorded outputs of whole chunks for tests/test_gpu_chunk_small_kernels.py: what the kernels AROUND the chain launches compute.

The FC layers of the STN head and of the decoder (p2s_gemm.hip) were re-pipelined in r17 under the rule that every output
element keeps its one accumulation chain over k; the test pins that against values recorded from the commit BEFORE the change.
Run on a GPU from a checkout of that commit (or with P2S_LIB_PATH naming its library):

    python tools/make_chunk_small_kernels_golden.py [FILE]     # default: tests/golden/chunk_small_kernels_parent.npz

Inputs: grid queries of the fixture cloud with their 300-point kNN patches and 1000-point uniform sub-samples (seeded), as chunks
of 130 queries (four 32-row tiles and a ragged fifth of 2 rows), of 3, of 1 (one row) and of 2050 (where the widest layer runs
on 64-row tiles: 32 full ones and a ragged one of 2 rows).
Weight sets: p2s_max default and adversarial (both with stem reuse on and off), p2s_vanilla (QSTN), a sym_op='sum' model, the two
single_transformer models (the A2 operand of the FC kernel as max and as sum), p2s_max with the fp16-pair encoder (the 16-bit
head layers, which r17 leaves alone), and one chunk with a NaN coordinate.

Per case the file keeps logits and SDF in full and, of the pooled STN features and the two pooled main features, the full arrays
for the chunks of 1 and 3 and a SHA-256 for the larger chunks (the arrays would not fit a committed file).  The digest is taken
of the float32 bytes with every NaN replaced by the canonical one and -0 by +0: equal digests <=> array_equal(equal_nan=True).
The test imports the case list and the runner from this file."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'chunk_small_kernels_parent.npz')
CLOUD = os.path.join(ROOT, 'tests', 'golden', 'cloud_abc_00994122.npy')
SEED = 20261020
NQ = 130
NBIG = 2050          # SF3 runs on 64-row tiles from 1985 queries on: 32 full tiles and a ragged one of 2 rows
KEYS = ('stn_pool', 'feat_local', 'feat_global', 'logits', 'sdf')
WIDE = ('stn_pool', 'feat_local', 'feat_global')       # kept as digests for the chunks of more than 3 queries
BOTH = (('reuse', {}), ('recompute', {'stem_reuse': False}))
ONE = BOTH[:1]


def cases():
    """(case id, model, configuration extras, queries, handles, NaN coordinate)"""
    out = []
    for nq in (1, 3, NQ):
        out.append(('p2s_max_%d' % nq, 'p2s_max', {}, nq, BOTH, False))
    for nq in (3, NQ):
        out.append(('p2s_max_stress_%d' % nq, 'p2s_max_stress', {}, nq, BOTH, False))
        out.append(('p2s_vanilla_%d' % nq, 'p2s_vanilla', {}, nq, ONE, False))
        out.append(('p2s_shared_encoder_%d' % nq, 'p2s_shared_encoder', {}, nq, ONE, False))
    out.append(('p2s_max_sum_%d' % NQ, 'p2s_max_sum', {}, NQ, ONE, False))
    out.append(('p2s_shared_encoder_sum_%d' % NQ, 'p2s_shared_encoder_sum', {}, NQ, ONE, False))
    out.append(('p2s_max_fp16x2_%d' % NQ, 'p2s_max', {'encoder_bf16': 4}, NQ, ONE, False))
    out.append(('p2s_max_%d_nan' % NQ, 'p2s_max', {}, NQ, ONE, True))
    out.append(('p2s_max_%d' % NBIG, 'p2s_max', {}, NBIG, ONE, False))
    return out


def digest(a):
    a = np.ascontiguousarray(a, dtype=np.float32) + np.float32(0)
    a = np.where(np.isnan(a), np.float32(np.nan), a)
    return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)


def inputs(engine, cache):
    """NBIG grid queries of the fixture cloud, their patches, sub-samples and radii (a case takes the first of them); computed
    once, never written to"""
    if 'in' not in cache:
        cloud = engine.Cloud(np.load(CLOUD))
        q = cloud.query_grid(32, 3)
        q = q[:: max(1, q.shape[0] // NBIG)][:NBIG].contiguous()
        assert q.shape[0] == NBIG
        _, sub = engine.Rng(SEED).subsample_uniform(cloud, NBIG, 1000)
        _, patch, rad = cloud.knn_patch(q, 300, want_ids=False)
        cache['in'] = (patch.contiguous(), sub.contiguous(), q, rad.contiguous())
    return cache['in']


def run_case(engine, synth, case, cache):
    """{handle name: {key: array}} of one case"""
    import torch
    _, name, extra, nq, handles, nan = case
    weights = cache.setdefault('weights', {})
    if name not in weights:
        weights[name] = synth.make_weights(name)
    w, cfg = weights[name]
    cfg = dict(cfg, points_per_patch=300, sub_sample_size=1000, **extra)
    patch, sub, q, rad = (t[:nq].contiguous() for t in inputs(engine, cache))
    if nan:
        patch = patch.clone()
        patch[77, 5, 1] = float('nan')
    out = {}
    for hname, stem in handles:
        m = engine.Model(w, dict(cfg, **stem))
        lg, sdf = m.forward(patch, sub, q, rad, want_sdf=True)
        stn = m.debug_stn_pool(nq)
        torch.cuda.synchronize()
        fl, fg = m.features(patch, sub, q)
        torch.cuda.synchronize()
        out[hname] = {'stn_pool': stn.cpu().numpy(), 'feat_local': fl.cpu().numpy(), 'feat_global': fg.cpu().numpy(),
                      'logits': lg.cpu().numpy(), 'sdf': sdf.cpu().numpy()}
        m.close()
    return out


def recorded(case, key, value):
    """what the file keeps of one array"""
    return digest(value) if case[3] > 3 and key in WIDE else value


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
            arrays['%s/%s' % (case[0], key)] = recorded(case, key, first[key])
        print(case[0], {key: first[key].shape for key in KEYS}, 'NaN values: %d' % sum(int(np.isnan(first[key]).sum()) for key in KEYS))
    for i, t in enumerate(inputs(engine, cache)):
        arrays['inputs/%d' % i] = digest(t.cpu().numpy())
    dst = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    np.savez_compressed(dst, **arrays)
    print(dst, os.path.getsize(dst), 'bytes')


if __name__ == '__main__':
    main()
