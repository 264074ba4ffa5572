"""Workers mode on the GPU: the reference's sub-sample streams under --workers W --batchSize B (p2s_stream_order,
p2s_subsample_workers, p2s_infer_shape_workers / p2s_infer_queries_workers, engine.WorkerStreams, the drop-in's
P2S_RNG_MODE=workers) against points2surf_amd/streams.py and the goldens of the unmodified reference
(tests/golden/ref_workers_*.npz, tools/make_golden_workers.py)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, 'tests', 'golden')
ABC = os.path.join(GOLDEN, 'abc_minimal')
DROPIN = os.path.join(REPO, 'points2surf_amd', 'dropin')
SEED = 40938661
PARAMS = [(0, 1000, 7, 501), (0, 50, 3, 1), (0, 100, 4, 1000), (10, 100, 4, 100), (37 * 5 + 11, 2000, 3, 37),
          (0, 1, 1, 1), (1234, 777, 1, 50), (501 * 7 * 3 + 250, 4000, 7, 501), (2 ** 40 + 3, 300, 5, 17)]


def golden(case):
    with open(os.path.join(GOLDEN, 'meta_workers.json')) as f:
        meta = json.load(f)['ref_workers_' + case]
    return np.load(os.path.join(GOLDEN, 'ref_workers_%s.npz' % case)), meta


def shape_names():
    with open(os.path.join(ABC, 'abc3.txt')) as f:
        return [x.strip() for x in f if x.strip()]


def load_cloud(name):
    return np.ascontiguousarray(np.load(os.path.join(ABC, '04_pts', name + '.xyz.npy'))[:, :3], dtype=np.float32)


def make_model(name, **extra):
    from points2surf_amd import engine, synth
    w, cfg = synth.make_weights(name, seed=1234)
    cfg.update(extra)
    return engine.Model(w, cfg), cfg


def sdf_check(sdf, ref, tol):
    """max |dSDF| below ``tol`` and no sign flip (none of these goldens has a tie: the same shapes pass with 0 flips in
    dataset mode, tests/test_gpu_fulleval.py)"""
    d = float(np.abs(sdf - ref).max())
    flips = int((np.sign(sdf) != np.sign(ref)).sum())
    return d, flips


def tol_of(model):
    # the fixed-radius models' patches in patch space are scaled by the radius: the same limit as their dataset-mode
    # golden tests (tests/test_gpu_fulleval.py)
    return 1e-4 if model.endswith('_radius') else 1e-5


# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('g0,n,W,B', PARAMS)
def test_stream_order_kernel_matches_host_model(g0, n, W, B):
    import ctypes
    import torch
    from points2surf_amd import _lib, streams
    lib = _lib.load()
    dev = torch.device('cuda', torch.cuda.current_device())
    q = torch.arange(3 * n, dtype=torch.float32, device=dev).reshape(n, 3) * 0.5
    qo = torch.full((n, 3), -1.0, dtype=torch.float32, device=dev)
    src = torch.full((n,), -1, dtype=torch.int64, device=dev)
    counts = np.zeros(W, np.int64)
    _lib.check(lib.p2s_stream_order(g0, n, W, B, ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(qo.data_ptr()),
                                    ctypes.c_void_p(src.data_ptr()), counts.ctypes.data_as(ctypes.c_void_p),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    order, c_ref = streams.stream_order(g0, n, W, B)
    assert np.array_equal(src.cpu().numpy(), order)
    assert np.array_equal(counts, c_ref)
    assert torch.equal(qo, q[torch.from_numpy(order).to(dev)])


def test_stream_order_refuses_bad_arguments():
    import ctypes
    from points2surf_amd import _lib
    lib = _lib.load()
    for args in [(0, 10, 0, 5), (0, 10, 3, 0), (-1, 10, 3, 5), (0, -1, 3, 5), (0, 10, 5000, 5)]:
        assert lib.p2s_stream_order(*args, None, None, None, None, None) == -1
    counts = np.zeros(3, np.int64)
    assert lib.p2s_stream_order(5, 100, 3, 7, None, None, None, counts.ctypes.data_as(ctypes.c_void_p), None) == 0
    assert counts.sum() == 100


# --------------------------------------------------------------------------------------------------------------------
def _batch_digests(pts, sizes):
    starts = np.concatenate([[0], np.cumsum(sizes)])
    return [hashlib.sha256(np.ascontiguousarray(pts[starts[b]:starts[b + 1]]).tobytes()).digest() for b in range(len(sizes))]


@pytest.mark.parametrize('case', ['p2s_max_w7_b501', 'p2s_max_w3_b37', 'p2s_vanilla_w7_b501', 'p2s_vanilla_w3_b37'])
def test_subsample_workers_reproduces_reference_batches(case):
    """the sub-sample points of every query, in query order across the three shapes, cut into the reference's batches:
    every batch digest equals the one the reference's DataLoader workers delivered"""
    import torch
    from points2surf_amd import engine
    g, meta = golden(case)
    weighted = meta['model'] == 'p2s_vanilla'
    ws = engine.WorkerStreams(SEED, meta['workers'], meta['batchSize'])
    parts = []
    for name in shape_names():
        cloud = engine.Cloud(load_cloud(name))
        q = cloud.query_grid(32, 3)
        if weighted:
            _, pts = ws.subsample(cloud, 1000, query_ms=q)
        else:
            _, pts = ws.subsample(cloud, 1000, n_queries=int(q.shape[0]))
        torch.cuda.synchronize()
        parts.append(pts.cpu().numpy())
        cloud.close()
    pts = np.concatenate(parts)
    assert ws.position == pts.shape[0] == int(g['batch_sizes'].sum())
    got = _batch_digests(pts, g['batch_sizes'])
    bad = [b for b in range(len(got)) if got[b] != g['sub_sha'][b].tobytes()]
    assert not bad, 'batches %s of %d differ from the reference' % (bad[:8], len(got))
    ws.close()


# --------------------------------------------------------------------------------------------------------------------
def run_rec(model_name, W, B, chunk=0, want_logits=False, ws=None, model=None, **extra):
    """engine.infer_shape with one WorkerStreams carried across the three abc3 shapes -> list of sdf arrays"""
    from points2surf_amd import engine
    if model is None:
        model, cfg = make_model(model_name, **extra)
    if ws is None:
        ws = engine.WorkerStreams(SEED, W, B, first=model.cfg.get('patch_radius', 0.0) > 0.0)
    out = []
    for name in shape_names():
        cloud = engine.Cloud(load_cloud(name))
        r = engine.infer_shape(model, cloud, ws, 32, 3, chunk=chunk, want_logits=want_logits)
        out.append(tuple(x.cpu().numpy() for x in r if x is not None))
        cloud.close()
    return out, ws, model


@pytest.mark.parametrize('case', ['p2s_max_w7_b501', 'p2s_vanilla_w7_b501', 'p2s_max_w3_b37', 'p2s_vanilla_w3_b37',
                                  'p2s_medium_radius_w7_b501'])
@pytest.mark.parametrize('chunk', [0, 1000])
def test_infer_shape_workers_matches_reference(case, chunk):
    g, meta = golden(case)
    out, ws, model = run_rec(meta['model'], meta['workers'], meta['batchSize'], chunk=chunk)
    total = 0
    for i, (sdf, q) in enumerate(out):
        ref = g['sdf_%d' % i]
        d, flips = sdf_check(sdf, ref, tol_of(meta['model']))
        print('%s chunk %d shape %d: max|dSDF| %.3g, sign flips %d/%d' % (case, chunk, i, d, flips, ref.size))
        assert sdf.shape == ref.shape and d < tol_of(meta['model']) and flips == 0
        assert hashlib.sha256(np.ascontiguousarray(q).tobytes()).hexdigest() == meta['shapes'][i]['query_sha256']
        total += ref.size
    assert ws.position == total
    model.close()
    ws.close()


def test_gt_query_pass_workers_matches_reference():
    """the GT-query pass (05_query_pts, one rotation per query from the worker's twin of the first generator)"""
    from points2surf_amd import engine
    g, meta = golden('p2s_max_w7_b501_gt')
    model, _ = make_model('p2s_max')
    ws = engine.WorkerStreams(SEED, meta['workers'], meta['batchSize'], first=True)
    for i, name in enumerate(shape_names()):
        cloud = engine.Cloud(load_cloud(name))
        q = np.load(os.path.join(ABC, '05_query_pts', name + '.ply.npy')).astype(np.float32)
        sdf = engine.infer_queries(model, cloud, ws, True, engine.upload(q, model.device)).cpu().numpy()
        ref = g['sdf_%d' % i]
        d, flips = sdf_check(sdf, ref, 1e-5)
        print('GT-query pass workers shape %d: max|dSDF| %.3g, sign flips %d/%d' % (i, d, flips, ref.size))
        assert d < 1e-5 and flips == 0
        cloud.close()
    assert ws.position == 6000
    model.close()
    ws.close()


# --------------------------------------------------------------------------------------------------------------------
def test_workers_mode_equals_dataset_mode_when_one_stream_serves_all():
    """W = 1 with any B, and W = 4 with B at least the whole dataset: one stream takes every query, bit-identical SDF
    to the --workers 0 path"""
    from points2surf_amd import engine
    for model_name in ('p2s_max', 'p2s_vanilla'):
        model, _ = make_model(model_name)
        rng = engine.Rng(SEED)
        base = []
        for name in shape_names():
            cloud = engine.Cloud(load_cloud(name))
            base.append(engine.infer_shape(model, cloud, rng, 32, 3)[0].cpu().numpy())
            cloud.close()
        for W, B in ((1, 37), (4, 10 ** 6)):
            out, ws, _ = run_rec(model_name, W, B, model=model)
            for a, (b, _) in zip(base, out):
                assert np.array_equal(a, b), (model_name, W, B)
            ws.close()
        model.close()


def test_logits_capture_follows_query_order():
    """the captured logits are scattered back like the SDF: sign of the last logit = sign of the SDF"""
    out, ws, model = run_rec('p2s_max', 3, 37, want_logits=True)
    g, _ = golden('p2s_max_w3_b37')
    for i, (sdf, q, logits) in enumerate(out):
        assert logits.shape == (sdf.shape[0], 2)
        assert np.array_equal(logits[:, 1] >= 0, sdf > 0)
        assert np.abs(sdf - g['sdf_%d' % i]).max() < 1e-5
    model.close()
    ws.close()


def test_fp16_pair_fallback_in_workers_mode():
    """fp16 pair encoder with a checkpoint whose first-layer activations overflow the half range for some queries (the
    construction of tests/test_gpu_fp16_fallback.py: a BatchNorm channel scaled up, the next layer's input column scaled
    down -- the same function): the flagged queries are re-run in fp32 at their stream-order slot, so after the scatter
    they equal fp32 workers mode bit for bit, and every query stays at the golden (the fp16 pair's own limit, 1e-4)"""
    from points2surf_amd import engine, synth
    w, cfg = synth.make_weights('p2s_max', seed=1234)
    w2 = {k: v.copy() for k, v in w.items()}
    for c in range(2):
        w2['feat_local.bn0a.weight'][c] *= 2.0 ** 22
        w2['feat_local.bn0a.bias'][c] *= 2.0 ** 22
        w2['feat_local.conv0b.weight'][:, c, :] /= 2.0 ** 22
    g, meta = golden('p2s_max_w3_b37')
    res, fallback = {}, 0
    for enc in (0, 4):
        model = engine.Model(w2, dict(cfg, encoder_bf16=enc))
        sdf, n = [], 0
        ws = engine.WorkerStreams(SEED, 3, 37)
        for name in shape_names():
            cloud = engine.Cloud(load_cloud(name))
            sdf.append(engine.infer_shape(model, cloud, ws, 32, 3, chunk=1000)[0].cpu().numpy())
            n += int(model.counters()['fallback_queries'])
            cloud.close()
        res[enc] = sdf
        if enc == 4:
            fallback = n
        model.close()
        ws.close()
    assert fallback > 0
    same = sum(int((a == b).sum()) for a, b in zip(res[0], res[4]))
    print('fp16 pair workers mode: %d queries re-run in fp32, %d bit-identical to fp32 workers mode' % (fallback, same))
    assert same >= fallback
    for i, a in enumerate(res[4]):
        assert np.abs(a - g['sdf_%d' % i]).max() < 1e-4
        assert int((np.sign(a) != np.sign(g['sdf_%d' % i])).sum()) == 0


# --------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_generator_untouched():
    """W > 1 with a cloud smaller than the sub-sample, and a partial query range: P2S_EINVAL before any draw -- the
    following valid run over the three shapes still gives the golden result"""
    from points2surf_amd import engine, _lib
    g, meta = golden('p2s_max_w3_b37')
    model, _ = make_model('p2s_max')
    ws = engine.WorkerStreams(SEED, 3, 37)
    small = engine.Cloud(load_cloud(shape_names()[0])[:800])
    with pytest.raises(_lib.P2SError) as e:
        engine.infer_shape(model, small, ws, 32, 3)
    assert e.value.code == -1 and 'fewer than the sub-sample' in str(e.value)
    first = engine.Cloud(load_cloud(shape_names()[0]))
    with pytest.raises(_lib.P2SError) as e:
        engine.infer_shape(model, first, ws, 32, 3, q_begin=10)
    assert e.value.code == -1 and 'whole shapes' in str(e.value)
    with pytest.raises(_lib.P2SError):
        engine.infer_shape(model, first, ws, 32, 3, q_end=100)
    assert ws.position == 0
    small.close()
    first.close()
    out, ws, _ = run_rec('p2s_max', 3, 37, model=model, ws=ws)
    for i, (sdf, _) in enumerate(out):
        assert np.abs(sdf - g['sdf_%d' % i]).max() < 1e-5
        assert int((np.sign(sdf) != np.sign(g['sdf_%d' % i])).sum()) == 0
    model.close()
    ws.close()


def test_skip_shape_and_state_round_trip():
    """skip_shape of the first shape + inference of the other two == the full run's last two shapes; get_state /
    set_state carry all 2 W generators and the cursor"""
    from points2surf_amd import engine
    g, meta = golden('p2s_medium_radius_w7_b501')
    model, cfg = make_model('p2s_medium_radius')
    ws = engine.WorkerStreams(SEED, 7, 501, first=True)
    names = shape_names()
    c0 = engine.Cloud(load_cloud(names[0]))
    n0 = ws.skip_shape(c0, cfg, c0.query_grid(32, 3), model.sub_sample_size)
    c0.close()
    assert ws.position == n0 == meta['shapes'][0]['queries']
    st = ws.get_state()
    ws2 = engine.WorkerStreams(SEED, 7, 501, first=True)
    ws2.set_state(st)
    for i in (1, 2):
        c = engine.Cloud(load_cloud(names[i]))
        sdf = engine.infer_shape(model, c, ws2, 32, 3)[0].cpu().numpy()
        assert np.abs(sdf - g['sdf_%d' % i]).max() < 1e-4
        assert int((np.sign(sdf) != np.sign(g['sdf_%d' % i])).sum()) == 0
        c.close()
    model.close()
    ws.close()
    ws2.close()


# --------------------------------------------------------------------------------------------------------------------
def _write_model_files(modeldir, name):
    import torch
    from points2surf_amd import synth
    from oracle.make_golden import train_namespace
    w, cfg = synth.make_weights(name, seed=1234)
    os.makedirs(modeldir, exist_ok=True)
    torch.save(synth.to_torch_state_dict(w), os.path.join(modeldir, name + '_model.pth'))
    torch.save(train_namespace(cfg, batch=500), os.path.join(modeldir, name + '_params.pth'))


def _dropin_args(tmp_path, model, extra=()):
    modeldir = str(tmp_path / 'models')
    _write_model_files(modeldir, model)
    return ['--indir', ABC, '--outdir', str(tmp_path / 'out'), '--dataset', 'abc3.txt', '--modeldir', modeldir,
            '--models', model, '--query_grid_resolution', '32', '--epsilon', '3', '--certainty_threshold', '13',
            '--sigma', '5', '--workers', '7', '--batchSize', '501', '--cache_capacity', '5'] + list(extra)


def _run_dropin(args, env_extra, reconstruction=True, timeout=600):
    code = ('import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n'
            'import source.points_to_surf_eval as ev\n'
            'opt = ev.parse_arguments(sys.argv[1:]); opt.reconstruction = %r\n'
            'ev.points_to_surf_eval(opt)\n') % (REPO, DROPIN, reconstruction)
    env = dict(os.environ)
    env.pop('P2S_RNG_MODE', None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, '-c', code] + list(args), env=env, cwd=REPO, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r


def test_dropin_workers_mode_writes_reference_results(tmp_path):
    """P2S_RNG_MODE=workers with --workers 7 --batchSize 501: the reference's dist_ms of that command line; without the
    variable the same command line still writes the --workers 0 results"""
    args = _dropin_args(tmp_path, 'p2s_max')
    _run_dropin(args, {'P2S_RNG_MODE': 'workers'})
    g, _ = golden('p2s_max_w7_b501')
    for i, name in enumerate(shape_names()):
        sdf = np.load(str(tmp_path / 'out' / 'rec' / 'dist_ms' / (name + '.xyz.npy')))
        assert np.abs(sdf - g['sdf_%d' % i]).max() < 1e-5
        assert int((np.sign(sdf) != np.sign(g['sdf_%d' % i])).sum()) == 0
    out0 = tmp_path / 'default'
    args0 = [a if a != str(tmp_path / 'out') else str(out0) for a in args]
    _run_dropin(args0, {})
    from points2surf_amd import engine
    model, _ = make_model('p2s_max')
    rng = engine.Rng(SEED)
    for i, name in enumerate(shape_names()):
        cloud = engine.Cloud(load_cloud(name))
        ref = engine.infer_shape(model, cloud, rng, 32, 3)[0].cpu().numpy()
        cloud.close()
        assert np.array_equal(np.load(str(out0 / 'rec' / 'dist_ms' / (name + '.xyz.npy'))), ref)
    model.close()


def test_dropin_workers_gt_pass_and_random_patches(tmp_path):
    """the GT-query pass golden and the sequential_shapes_random_patches golden through the drop-in in workers mode"""
    g, meta = golden('p2s_max_w7_b501_gt')
    _run_dropin(_dropin_args(tmp_path, 'p2s_max'), {'P2S_RNG_MODE': 'workers'}, reconstruction=False)
    for i, name in enumerate(shape_names()):
        sdf = np.load(str(tmp_path / 'out' / 'eval' / 'eval' / (name + '.xyz.npy')))
        assert np.abs(sdf - g['sdf_%d' % i]).max() < 1e-5
        assert int((np.sign(sdf) != np.sign(g['sdf_%d' % i])).sum()) == 0
    g, meta = golden('p2s_max_w3_b37_recsample')
    rs = tmp_path / 'rs'
    rs.mkdir()
    args = _dropin_args(rs, 'p2s_max', ['--sampling', 'sequential_shapes_random_patches', '--patches_per_shape',
                                        str(meta['patches_per_shape'])])
    args[args.index('--workers') + 1] = '3'
    args[args.index('--batchSize') + 1] = '37'
    _run_dropin(args, {'P2S_RNG_MODE': 'workers'})
    for i, name in enumerate(shape_names()):
        sdf = np.load(str(rs / 'out' / 'rec' / 'dist_ms' / (name + '.xyz.npy')))
        idx = np.loadtxt(str(rs / 'out' / 'rec' / (name + '.idx')), dtype=np.int64)
        assert np.array_equal(idx, g['idx_%d' % i])
        assert np.abs(sdf - g['sdf_%d' % i]).max() < 1e-5
        assert int((np.sign(sdf) != np.sign(g['sdf_%d' % i])).sum()) == 0


def test_dropin_workers_mode_two_ranks_one_gpu(tmp_path):
    """two ranks on one GPU over gloo (stream hand-off of the 2 W generator states + the cursor) write files
    bit-identical to one process; P2S_SHARD=queries with workers mode is refused"""
    import socket
    args = _dropin_args(tmp_path, 'p2s_vanilla')
    _run_dropin(args, {'P2S_RNG_MODE': 'workers'})
    single = {n: np.load(str(tmp_path / 'out' / 'rec' / 'dist_ms' / (n + '.xyz.npy'))) for n in shape_names()}
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    out2 = str(tmp_path / 'two')
    args2 = [a if a != str(tmp_path / 'out') else out2 for a in args]
    procs = []
    for rank in range(2):
        env = dict(os.environ, P2S_RNG_MODE='workers', WORLD_SIZE='2', RANK=str(rank), LOCAL_RANK=str(rank),
                   LOCAL_WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), P2S_DIST_BACKEND='gloo',
                   HIP_VISIBLE_DEVICES=os.environ.get('HIP_VISIBLE_DEVICES', '0').split(',')[0])
        code = ('import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n'
                'import source.points_to_surf_eval as ev\n'
                'opt = ev.parse_arguments(sys.argv[1:]); opt.reconstruction = True\n'
                'ev.points_to_surf_eval(opt)\n') % (REPO, DROPIN)
        procs.append(subprocess.Popen([sys.executable, '-c', code] + args2, env=env, cwd=REPO, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), '\n'.join(o[-3000:] for o in outs)
    for n, ref in single.items():
        assert np.array_equal(np.load(os.path.join(out2, 'rec', 'dist_ms', n + '.xyz.npy')), ref)
