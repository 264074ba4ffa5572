"""GPU: the device memory the model, generator, cloud-set and trainer handles own (csrc/p2s_devmem.h).  Buffers that grew
give the answers of buffers reserved at the right size from the start, a failed call leaves a handle that still does, and
create / use / destroy cycles give back what they took.  Small synthetic model (32-point patches and sub-samples), a cloud
of about 2000 points."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = 40938661
K = 32                 # points per patch and per sub-sample
CHUNK = 1000           # queries per chunk: the 32^3 grid of the cloud (2174 queries) needs three, the 16^3 grid (653) less than one
RADIUS = 0.1


def same(a, b):
    import torch
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def shape_call(world, model, rng, res):
    """one per-shape pipeline call from the generator's first draw -> [sdf, queries]"""
    import torch
    from points2surf_amd import engine
    rng.set_state(*world['start'])
    out = [t.clone() for t in engine.infer_shape(model, world['cloud'], rng, res, 3, chunk=CHUNK)]
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope='module')
def world(fixture_cloud):
    """clouds, weights, queries and -- computed once, on a handle that never regrows -- the outputs of the pipeline calls"""
    import torch
    from points2surf_amd import engine, synth
    torch.cuda.set_device(0)
    w, cfg = synth.make_weights('p2s_max')
    cfg = dict(cfg, points_per_patch=K, sub_sample_size=K)
    cloud = engine.Cloud(fixture_cloud[::17])              # 2041 points
    other = engine.Cloud(fixture_cloud[5::29])             # 1196 points
    n16, n32 = cloud.count_queries(16, 3), cloud.count_queries(32, 3)
    assert 0 < n16 < CHUNK and n32 > 2 * CHUNK, (n16, n32)
    g = np.random.default_rng(7)                           # queries near the surface: balls of RADIUS hold 0 .. some tens of points
    near = fixture_cloud[::17][g.integers(0, 2041, 5000)] + g.normal(0, 0.03, (5000, 3))
    queries = torch.from_numpy(near.astype(np.float32)).cuda()
    rng = engine.Rng(SEED)
    world = dict(w=w, cfg=cfg, cloud=cloud, other=other, queries=queries, start=rng.get_state())
    model = engine.Model(w, cfg)
    world['fresh'] = {res: shape_call(world, model, rng, res) for res in (32, 16)}      # the larger grid first
    model.close()
    rng.close()
    return world


def test_pipeline_regrow_gives_the_same_answers(world):
    from points2surf_amd import engine
    model, rng = engine.Model(world['w'], world['cfg']), engine.Rng(SEED)
    first = shape_call(world, model, rng, 16)           # reserves one short chunk
    grown = shape_call(world, model, rng, 32)           # several chunks: the chunk buffers and the workspace regrow
    again = shape_call(world, model, rng, 16)           # served by the buffers of the 32^3 call
    model.close()
    rng.close()
    assert same(grown, world['fresh'][32])
    assert same(again, world['fresh'][16])
    assert same(first, again)


def test_failed_call_leaves_a_usable_handle(world):
    from points2surf_amd import engine, _lib
    model, rng = engine.Model(world['w'], world['cfg']), engine.Rng(SEED)
    model.debug_fault_chunk(1)                          # the second of the 32^3 call's chunks
    with pytest.raises(_lib.P2SError) as err:
        shape_call(world, model, rng, 32)
    assert err.value.code == -2 and 'injected fault' in str(err.value)
    clean = [shape_call(world, model, rng, res) for res in (32, 16)]
    model.close()
    rng.close()
    assert same(clean[0], world['fresh'][32]) and same(clean[1], world['fresh'][16])


def regrow_case(make, call, sizes):
    """call(handles, size) at sizes (small, large, small) on one make(), and at (large, small) on a fresh one: the outputs
    at equal sizes are bit-identical"""
    import torch
    handles = make()
    small, grown, again = [call(handles, size) for size in sizes]
    fresh = make()
    fresh_grown, fresh_small = call(fresh, sizes[1]), call(fresh, sizes[2])
    torch.cuda.synchronize()
    for h in handles + fresh:
        h.close()
    assert same(grown, fresh_grown) and same(again, fresh_small) and same(small, again)


def test_workers_regrow_gives_the_same_answers(world):
    from points2surf_amd import engine

    def make():
        ws = engine.WorkerStreams(SEED, 2, 16)
        ws.start = ws.get_state()
        return [engine.Model(world['w'], world['cfg']), ws]

    def call(handles, n):
        model, ws = handles
        ws.set_state(ws.start)
        return [engine.infer_queries(model, world['cloud'], ws, None, world['queries'][:n], chunk=CHUNK).clone()]

    regrow_case(make, call, (100, 5000, 100))           # 100 -> room for 1149 queries; 5000 regrows


def test_weighted_subsample_regrow_gives_the_same_answers(world):
    from points2surf_amd import engine

    def call(handles, nq):
        handles[0].set_state(*world['start'])
        return [t.clone() for t in handles[0].subsample_weighted(world['cloud'], world['queries'][:nq], 16)]

    regrow_case(lambda: [engine.Rng(SEED)], call, (8, 64, 8))


def test_ball_regrow_gives_the_same_answers(world):
    from points2surf_amd import engine

    def call(handles, nq):
        handles[0].set_state(*world['start'])
        q = world['queries'][:nq]
        counts = engine.ball_count(world['cloud'], q, RADIUS).clone()
        return [counts] + [t.clone() for t in engine.ball_patch(world['cloud'], handles[0], q, RADIUS, 16, with_rotation=True)]

    regrow_case(lambda: [engine.Rng(SEED)], call, (10, 3000, 10))


def test_cloudset_regrow_gives_the_same_answers(world):
    from points2surf_amd import engine

    def call(handles, items):
        cset, rng = handles
        rng.set_state(*world['start'])
        cloud_of = (np.arange(items) * 7 // 3) % 2
        return [t.clone() for t in cset.subsample_uniform(rng, cloud_of, 8)]

    regrow_case(lambda: [engine.CloudSet([world['cloud'], world['other']]), engine.Rng(SEED)], call, (4, 4096, 4))


# Free device memory lost over 8 create / use / destroy cycles on the commit before the handles moved onto the owners of
# p2s_devmem.h: the largest of three runs of this test there (0, 0 and 0 bytes: profiles/r18/handle_memory.txt).
PARENT_LOSS = 0
# The smallest block per cycle the test is meant to catch: the cloud set's device copy of the generator segments
# (p2s_cloudset_s::Items::seg_dev), 16 bytes for each of SET_ITEMS items = 4 MB.  The other blocks of the cycle that a
# free-memory reading resolves are larger (the fp16-pair model's fallback copies of patch and sub-sample: 6 MB each; weights,
# workspace, generator streams, trainer parameters and arena: tens of MB and more).
SET_ITEMS = 1 << 18
SMALLEST_BLOCK = SET_ITEMS * 16


def test_create_use_destroy_gives_the_memory_back(world):
    import torch
    from points2surf_amd import engine, train
    cfg4 = dict(world['cfg'], encoder_bf16=4)           # the fp16 pair model owns the most buffers (fallback side buffers)
    cfg_t = dict(world['cfg'], points_per_patch=8, sub_sample_size=8)
    g = np.random.default_rng(1)
    batch = [torch.from_numpy(a.astype(np.float32)).cuda() for a in
             (g.uniform(-0.5, 0.5, (4, 8, 3)), g.uniform(-0.5, 0.5, (4, 8, 3)), g.uniform(-0.4, 0.4, (4, 3)),
              g.uniform(0.0, 0.1, 4), g.integers(0, 2, 4), g.uniform(0.05, 0.2, 4))]
    cloud_of = np.zeros(SET_ITEMS, dtype=np.int32)

    def cycle():
        model, rng = engine.Model(world['w'], cfg4), engine.Rng(SEED)          # (the generator: with its jump tables)
        engine.infer_shape(model, world['cloud'], rng, 16, 3, chunk=CHUNK)
        rng.subsample_weighted(world['cloud'], world['queries'][:8], 16)
        cset = engine.CloudSet([world['cloud'], world['other']])
        cset.subsample_uniform(rng, cloud_of, 1, want_pts=False)
        trainer = train.Trainer(cfg_t, world['w'])
        trainer.forward_backward(*batch)
        torch.cuda.synchronize()
        for h in (trainer, cset, rng, model):
            h.close()
        engine.release_scratch()

    def free_bytes():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        return torch.cuda.mem_get_info()[0]

    cycle()
    before = free_bytes()
    for _ in range(8):
        cycle()
    loss = before - free_bytes()
    print('handle memory: %d bytes of free device memory lost over 8 cycles' % loss)
    assert loss <= PARENT_LOSS + SMALLEST_BLOCK, (loss, PARENT_LOSS, SMALLEST_BLOCK)
