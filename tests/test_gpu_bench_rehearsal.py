"""GPU: rehearsal of bench.py's N > 1 control flow on a one-GPU box -- two ranks share the GPU, collectives over gloo
(``P2S_BENCH_SHARE_GPU=1 --backend gloo``; RCCL refuses two ranks on one device).  Exercises everything the driver's
multi-GPU run executes except the RCCL transport itself: self-spawn through torch.distributed.run, process-group
set-up, one shape per rank per step with the other rank's draws skipped (exact dataset stream) or per-shape seeds,
sharding.gather_variable, the max-over-ranks timing and the single JSON line of rank 0."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('mode', ['dataset', 'per_shape'])
def test_two_ranks_on_one_gpu(mode, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT', 'MASTER_ADDR')}
    env['P2S_BENCH_SHARE_GPU'] = '1'
    dump = str(tmp_path / 'dump')
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '2', '--backend', 'gloo', '--steps', '2',
                        '--warmup', '1', '--res', '32', '--rng-mode', mode, '--cpu-seconds', '3', '--dump-outputs', dump],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    lines = [l for l in r.stdout.split('\n') if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-1500:]                      # rank 0 alone prints
    d = json.loads(lines[0])
    assert d['config']['rng_mode'] == mode and 'REHEARSAL' in d['config']['parallelism'] and d['n_gpus'] == 1
    assert d['config']['queries_per_shape'] == {'00994122': 2976} and d['value'] > 0 and d['steps'] == 2
    assert d['roofline']['launches'] > 0
    # also at N > 1 rank 0 times the CPU baseline (after the timed region) and relates shapes/hour to it
    cb = d['cpu_baseline']
    assert cb['kind'] in ('port', 'reference') and cb['value'] > 0 and cb['cores'] >= 1 and len(cb['thread_probe_queries_per_s']) >= 1
    assert d['config']['shapes_per_hour_vs_cpu'] > 1.0 and cb['shapes_per_hour_cpu'] > 0
    assert d['self_check']['vs_cpu_' + cb['kind']]['sign_flips'] == 0
    assert d['stage_ms_rank0']['ms_cloud'] > 0 and d['stage_ms_rank0']['ms_grid'] > 0      # fresh handle per step
    g = d['self_check']['vs_reference_golden']
    assert g['queries'] == 2976 and g['sign_flips'] == 0 and g['max_abs_dsdf'] < 1e-4
    assert d['config']['assignment'].startswith('sharding.assign_shapes') and d['config']['collective'].startswith('gloo (world 2)')
    if mode == 'dataset':
        # the exact dataset-wide stream by hand-off through the rendezvous store: rank 0 re-derives the last shape of rank 1
        # from a fresh single stream and finds it bit-identical
        assert d['config']['stream_mode'] == 'dataset/handoff'
        h = d['self_check']['stream_handoff']
        assert h['bit_identical_to_single_stream'] is True and h['shapes'] == 6 and not h['state_mismatches']
        assert h['sdf_replayed'] == [{'shape': 5, 'owner': 1, 'queries': 2976, 'bit_identical': True}]
    else:
        # per-shape seeds: nothing crosses shapes, the replay still re-derives rank 1's last shape bit for bit
        h = d['self_check']['stream_handoff']
        assert d['config']['stream_mode'] == 'per_shape' and h['mode'] == 'per_shape' and h['bit_identical_to_single_stream'] is True
    # --dump-outputs: the last timed step is shapes 4 and 5 (one per rank), cut out of rank 0's gather.  Both must equal,
    # bit for bit, the same shapes inferred here in one process from one stream (dataset: shapes 0-3 skipped, shape 0
    # checked against the reference's golden on the way; per_shape: seeded with seed + 4 / + 5)
    assert d['outputs_dumped']['files'] == {'sdf_0.npy': [2976], 'sdf_1.npy': [2976]}
    _check_dump_against_one_process(dump, mode, [4, 5])


def _check_dump_against_one_process(dump, mode, last_step):
    import importlib.util
    import numpy as np
    spec = importlib.util.spec_from_file_location('p2s_bench', os.path.join(REPO, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from points2surf_amd import engine, parity, sharding, synth
    w, cfg = synth.make_weights('p2s_max')
    model = engine.Model(w, cfg)
    pts = np.ascontiguousarray(np.load(bench.cloud_path(bench.FIXTURE_SHAPE))[:, :3], dtype=np.float32)
    rng = engine.Rng(bench.SEED_DATA)
    want = []
    for g in range(last_step[-1] + 1):
        if mode == 'per_shape':
            bench.reseed(rng, bench.SEED_DATA + g)
        if g in last_step:
            want.append(bench.complete_shape(engine, model, pts, rng, 32, 0)[0].numpy())
        elif mode == 'dataset' and g == 0:
            sdf0 = bench.complete_shape(engine, model, pts, rng, 32, 0)[0].numpy()
            c = parity.compare_sdf(sdf0, np.load(os.path.join(bench.GOLDEN, 'ref_p2s_max_grid32.npz'))['sdf_full'])
            assert c['max_abs_dsdf'] < 1e-4 and c['flipped'].size == 0
        elif mode == 'dataset':
            c = engine.Cloud(pts)
            sharding.skip_shape_stream(c, rng, cfg, 32, bench.EPSILON, model.sub_sample_size)
            c.close()
    rng.close()
    for k, ref in enumerate(want):
        got = np.load(os.path.join(dump, 'sdf_%d.npy' % k))
        assert got.dtype == np.float32 and got.shape == ref.shape and np.array_equal(got, ref), k


def test_eight_ranks_three_clouds_at_the_real_world_size():
    """the control flow SCALE will run -- 8 ranks, the three abc_minimal clouds round-robin as one
    dataset with the exact dataset-wide stream (7 skipped shapes per rank and step), gather to rank 0 -- over gloo, one
    rank per GPU; rank 0's self-check compares all three clouds with the reference's golden.  Eight ranks on ONE GPU
    (plus this process and the torchrun launcher, which both hold the device) are ten processes with the GPU open, more
    than a GPU shared between jobs admits at once: this needs eight devices."""
    import torch
    have = torch.cuda.device_count()
    if have < 8:
        pytest.skip('needs 8 GPUs (one rank per GPU), found %d' % have)
    env = {k: v for k, v in os.environ.items()
           if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT', 'MASTER_ADDR', 'P2S_BENCH_SHARE_GPU')}
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '8', '--backend', 'gloo', '--steps', '3',
                        '--warmup', '1', '--res', '64', '--dataset', 'abc3', '--cpu-seconds', '3'], env=env, capture_output=True, text=True,
                       timeout=1200)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    lines = [l for l in r.stdout.split('\n') if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-1500:]
    d = json.loads(lines[0])
    assert 'x8' in d['config']['parallelism'] and len(d['config']['queries_per_shape']) == 3
    assert 'REHEARSAL' not in d['config']['parallelism'] and d['n_gpus'] == 8
    g = d['self_check']['vs_reference_golden']
    assert g['file'].endswith('ref_rec_p2s_max_abc3_grid64.npz') and len(g['shapes']) == 3
    assert g['sign_flips'] == 0 and g['max_abs_dsdf'] < 1e-4 and g['queries'] == sum(d['config']['queries_per_shape'].values())
    # rank 0 replays the whole stream -- the generator state at both ends of ALL 32 shapes equals what
    # their owners saw -- and re-infers the last shape of EVERY other rank bit for bit
    h = d['self_check']['stream_handoff']
    assert d['config']['stream_mode'] == 'dataset/handoff' and h['bit_identical_to_single_stream'] is True
    assert h['shapes'] == 32 and not h['state_mismatches']
    assert sorted(r['owner'] for r in h['sdf_replayed']) == list(range(1, 8)) and all(r['bit_identical'] for r in h['sdf_replayed'])
    assert d['cpu_baseline']['same_box'] == (d['cpu_baseline']['kind'] == 'reference')
    # the keys a SCALE run is read by: the CPU baseline and the ratio at the real world size
    assert d['cpu_baseline']['value'] > 0 and d['config']['shapes_per_hour_vs_cpu'] > 1.0 and d['config']['shapes_per_hour'] > 0


def test_a_rank_that_raises_takes_the_run_down_within_seconds():
    """VERDICT r5 item 4 / ADVICE r5: a rank that raises mid-run (injected: rank 2 at its third shape, i.e. inside the timed
    block, while ranks that are already through sit in ``StreamHandoff.finish()``) must end the WHOLE run promptly with a
    non-zero exit code -- not leave its peers in the closing gather until the process group's time-out (30 min).
    Three ranks: with this process and the launcher they are five processes with the GPU open, within what a shared
    GPU machine admits."""
    import time
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT', 'MASTER_ADDR')}
    env['P2S_BENCH_SHARE_GPU'] = '1'
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '3', '--backend', 'gloo', '--steps', '3',
                        '--warmup', '1', '--res', '32', '--cpu-seconds', '0', '--fault', '2:2'], env=env, capture_output=True,
                       text=True, timeout=600)
    dt = time.time() - t0
    assert r.returncode != 0 and 'injected fault' in r.stderr, (r.returncode, r.stderr[-1500:])
    assert not [l for l in r.stdout.split('\n') if l.startswith('{')]            # no JSON line from a broken run
    assert dt < 180, dt
    # a peer that was waiting names the failed rank (hand-off record), it does not time out
    assert 'TimeoutError' not in r.stderr


def test_replicate_mode_still_gives_the_exact_stream():
    """P2S_STREAM_HANDOFF=replicate (the r03 behaviour: every rank consumes every foreign shape's draws itself)"""
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT', 'MASTER_ADDR')}
    env.update(P2S_BENCH_SHARE_GPU='1', P2S_STREAM_HANDOFF='replicate')
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '2', '--backend', 'gloo', '--steps', '2',
                        '--warmup', '1', '--res', '32', '--cpu-seconds', '0'], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    d = json.loads([l for l in r.stdout.split('\n') if l.startswith('{')][0])
    assert d['config']['stream_mode'] == 'dataset/replicate' and d['value'] > 0


def test_golden_check_classifies_a_flipped_sign_with_device_and_cpu_logits(fixture_cloud):
    """the self-check's flip analysis: a doctored golden with ONE sign reversed must come back as one flip
    that is NOT an fp32 tie (both the device's and the CPU port's sign logit are far from zero), with the unmasked
    difference = 2 |sdf| -- and the same machinery positions the stream at a query of the SECOND shape of a dataset"""
    import importlib.util
    import numpy as np
    import torch
    spec = importlib.util.spec_from_file_location('p2s_bench', os.path.join(REPO, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from points2surf_amd import engine, parity, synth
    w, cfg = synth.make_weights('p2s_max')
    model = engine.Model(w, cfg)
    a = np.ascontiguousarray(fixture_cloud[:20000], dtype=np.float32)
    b = np.ascontiguousarray(fixture_cloud[5000:30000], dtype=np.float32)
    rng = engine.Rng(bench.SEED_DATA)
    sdfs = [bench.complete_shape(engine, model, p, rng, 24, 0)[0].numpy() for p in (a, b)]
    refs = [s.copy() for s in sdfs]
    j = int(np.argmax(np.abs(refs[1])))                      # a query whose sign logit is certainly not a tie
    refs[1][j] = -refs[1][j]
    shapes = [('shape_a', a, refs[0]), ('shape_b', b, refs[1])]
    rec, ok = bench.golden_check(engine, parity, model, w, cfg, shapes, 24, sdfs, 1e-4, 0)
    assert not ok and rec['sign_flips'] == 1 and rec['sign_flips_not_ties'] == 1
    f = rec['flipped'][0]
    assert f['shape'] == 'shape_b' and f['query'] == j and not f['tie'] and rec['tie_logit'] == parity.TIE_LOGIT_FP32
    assert abs(f['sign_logit_device'] - f['sign_logit_cpu_port']) < 1e-3 and abs(f['sign_logit_device']) > 1e-3
    assert abs(rec['max_abs_diff_unmasked'] - 2 * abs(sdfs[1][j])) < 1e-6 and rec['max_abs_dsdf'] < 1e-6
    # the logit the analysis computed belongs to THAT query: its sign is the sign of the device's SDF there
    assert (f['sign_logit_device'] >= 0) == (sdfs[1][j] > 0)


@pytest.mark.parametrize('encoder', ['fp32', 'fp16x2'])
def test_dropin_leg_of_the_bench(encoder, golden_dir, capsys):
    """bench.py's ``secondary.dropin_*`` leg (the hot path measured through boundary B1: the drop-in's
    points_to_surf_eval + implicit_surface_to_mesh_directory, files in / files out) at grid 32 on the three clouds: every
    file of the contract is written, the SDF equals the reference's golden, the environment is left as it was, and what the
    drop-in prints (the reference's progress lines) stays off stdout, which carries the bench's one JSON line"""
    import importlib.util
    import numpy as np
    spec = importlib.util.spec_from_file_location('p2s_bench', os.path.join(REPO, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from points2surf_amd import parity
    g = np.load(os.path.join(golden_dir, 'ref_fulleval_p2s_max_abc3_grid32.npz'))
    shapes = [(n, np.ascontiguousarray(np.load(bench.cloud_path(n))[:, :3], dtype=np.float32), g['rec_%d' % i])
              for i, n in enumerate(bench.ABC3)]
    before = os.environ.get('P2S_ENCODER')
    mods = [m for m in sys.modules if m == 'source' or m.startswith('source.')]
    try:
        rec, sdfs = bench.dropin_leg(shapes, 32, encoder)
    finally:
        for m in [m for m in sys.modules if (m == 'source' or m.startswith('source.')) and m not in mods]:
            del sys.modules[m]
        dropin = os.path.join(REPO, 'points2surf_amd', 'dropin')
        while dropin in sys.path:
            sys.path.remove(dropin)
    assert os.environ.get('P2S_ENCODER') == before
    cap = capsys.readouterr()
    assert cap.out == '' and 'evaluated' in cap.err
    assert rec['files_written'] == 7 * 3 and rec['shapes'] == 3 and rec['queries'] == sum(s[2].shape[0] for s in shapes)
    for sdf, (_, _, ref) in zip(sdfs, shapes):           # what the drop-in wrote, against the reference's golden
        c = parity.compare_sdf(sdf, ref)
        assert c['max_abs_dsdf'] < 1e-5 and c['flipped'].size == 0
    assert rec['value'] > 0 and rec['value_shape_loop'] >= rec['value'] and rec['seconds_mesh_directory'] > 0


def test_bench_model_flag_measures_configs3():
    """``bench.py --model p2s_vanilla --bf16 4`` = BASELINE configs[3] (p2s_vanilla with QSTN, fp16-pair
    encoder + fp32 decoder) through the same line: metric / workload name the model, the QSTN trunk launch is counted (3
    chain launches per chunk), the golden check runs against the model's own golden with the split-precision tie threshold"""
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT', 'MASTER_ADDR')}
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--model', 'p2s_vanilla', '--bf16', '4', '--steps', '2',
                        '--warmup', '1', '--res', '32', '--cpu-seconds', '0'], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    d = json.loads([l for l in r.stdout.split('\n') if l.startswith('{')][0])
    assert 'p2s_vanilla' in d['metric'] and 'fp16-pair' in d['metric'] and d['dtype'] == 'fp16x2'
    assert 'configs[3]' in d['config']['workload'] and 'p2s_vanilla' in d['config']['workload']
    assert d['roofline']['launches'] % 3 == 0 and d['roofline']['mfma_passes_per_product'] == 3
    assert d['stage_ms_rank0']['ms_chain_qstn'] > 0
    g = d['self_check']['vs_reference_golden']
    assert g['file'].endswith('ref_p2s_vanilla_grid32.npz') and g['queries'] == 2976 and g['max_abs_dsdf'] < 1e-4
    assert g['sign_flips_not_ties'] == 0 and g['tie_logit'] == 2e-5 and 'secondary' not in d
