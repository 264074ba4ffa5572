"""The mesh-metric kernels (points2surf_amd/csrc/p2s_metrics.hip) where they can go wrong unseen by one mesh and 6000
uniform points: the scan's carry across chunks of 1024 faces, searchsorted-left over zero-area faces, the fold at
l1 + l2 = 1, the 256-point tiles of remove_close with partial last tiles, pairs exactly at the radius, degree ties and
degrees in the hundreds, the `limit` of the compaction, the per-query nearest-neighbour distances with outliers far
outside the target's box, the reduction at its stride boundaries, and the generator's session renewal under
random_sample.  Expected values: tests/metrics_model.py (pinned to oracle/metrics_oracle.py and scipy by
tests/test_metrics_model.py, which also pins what each input is for) and the oracle itself.

Every comparison is one of: bit equality; an exact known answer; (n - 1) * 2^-53 relative for a sum of n non-negative
terms (the bound of any summation order); nf * 2^-53 relative for the area of nf faces (the same bound)."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest

import metrics_model as M

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESHES = os.path.join(REPO, 'tests', 'golden', 'abc_minimal', '03_meshes')
NAMES = ['00011084_fddd53ce45f640f3ab922328_trimesh_019', '00016513_3d6966cd42eb44ab8f4224f2_trimesh_053',
         '00994122_57d9d4755722f9d2d7436f0a_trimesh_000']
P2S_EINVAL = -1
CANARY = -12345                          # n_out before a call that must leave it alone
PAD = 8                                  # rows behind every output that must still hold the sentinel


def _env():
    import torch
    from points2surf_amd import _lib, engine
    return torch, _lib, engine, _lib.load()


@functools.lru_cache(maxsize=None)
def _fixture_mesh(i):
    from points2surf_amd import ply
    v, f = ply.read_ply(os.path.join(MESHES, NAMES[i] + '.ply'))
    return v.astype(np.float32), f.astype(np.int32)


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- a. sampling -------------------------------------------------------------------------------------------------------

EXACT_NF = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 5000)
COUNTS = (1, 255, 256, 257, 3000)


@pytest.mark.parametrize('nf,degenerate', [(nf, False) for nf in EXACT_NF] + [(nf, True) for nf in EXACT_NF if nf > 1])
def test_exact_meshes_every_face_id_and_every_bit(nf, degenerate):
    """lattice_mesh: areas and all their partial sums are exact, so the scan's association cannot change a bit -- every
    face id equals the model's and the oracle's, no share left out; the points are the same float64 expression rounded
    once; counts around the 256-sample blocks, one generator continuing like numpy's"""
    torch, _lib, engine, lib = _env()
    from points2surf_amd import metrics
    from oracle import metrics_oracle as MO
    deg = M.degenerate_positions(nf) if degenerate else {}
    v, f = M.lattice_mesh(nf, deg)
    areas = M.face_areas(v, f)
    exact_area = math.fsum(areas.tolist())
    vt, ft = _cuda(v), _cuda(f)
    seed = 1000 + nf
    rng, rs, twin = engine.Rng(seed), np.random.RandomState(seed), np.random.RandomState(seed)
    for count in COUNTS:
        pts, area, fid = metrics.sample_surface(vt, ft, count, rng, want_faces=True)
        torch.cuda.synchronize()
        pts, fid = pts.cpu().numpy(), fid.cpu().numpy()
        want_pts, want_face, want_area, _ = M.sample_model(v, f, twin.random_sample(3 * count))
        ref_pts, ref_area, ref_face = MO.sample_surface(v, f, count, rs)
        assert area == exact_area == want_area == ref_area, (nf, count, area, exact_area)
        assert np.array_equal(fid, want_face), (nf, count, np.nonzero(fid != want_face)[0][:8])
        assert np.array_equal(fid, ref_face)
        assert np.all(areas[fid] > 0.0)                        # no zero-area face is ever picked
        assert np.array_equal(pts, want_pts), (nf, count, np.nonzero(np.any(pts != want_pts, axis=1))[0][:8])
        assert np.array_equal(pts, ref_pts)
    mt, pos = rng.get_state()
    st = rs.get_state()
    assert np.array_equal(mt, st[1]) and pos == st[2]
    rng.check()
    rng.close()


@pytest.mark.parametrize('i', [0, 1, 2])
def test_fixture_meshes_every_decided_face_id(i):
    """inexact areas: the device's scan and np.cumsum associate differently, each within nf * 2^-53 relative of the exact
    sums.  Face ids are compared for every sample whose pick lies further than nf * 2^-53 * total from every cumulative
    value (tests/test_metrics_model.py: that leaves out less than 0.1 % for this seed); points bit for bit wherever the
    faces agree."""
    torch, _lib, engine, lib = _env()
    from points2surf_amd import metrics
    from oracle import metrics_oracle as MO
    v, f = _fixture_mesh(i)
    nf, count = len(f), 5000
    rng = engine.Rng(M.FIXTURE_SEED)
    pts, area, fid = metrics.sample_surface(_cuda(v), _cuda(f), count, rng, want_faces=True)
    torch.cuda.synchronize()
    pts, fid = pts.cpu().numpy(), fid.cpu().numpy()
    u = np.random.RandomState(M.FIXTURE_SEED).random_sample(3 * count)
    want_pts, want_face, want_area, cum = M.sample_model(v, f, u)
    ref_pts, ref_area, ref_face = MO.sample_surface(v, f, count, np.random.RandomState(M.FIXTURE_SEED))
    exact = math.fsum(M.face_areas(v, f).tolist())
    print('mesh %d: nf %d, area device %.17g, cumsum %.17g, fsum %.17g' % (i, nf, area, want_area, exact))
    assert abs(area - exact) <= nf * 2.0 ** -53 * area         # any order of summing nf non-negative areas
    decided = M.boundary_margin(cum, u[:count]) > nf * 2.0 ** -53 * cum[-1]
    print('left out %d of %d, faces differing %d' % (count - decided.sum(), count, np.count_nonzero(fid != want_face)))
    assert 1.0 - decided.mean() < 0.001
    assert np.array_equal(fid[decided], want_face[decided]) and np.array_equal(fid[decided], ref_face[decided])
    same = fid == want_face
    assert np.array_equal(pts[same], want_pts[same]) and np.array_equal(pts[same], ref_pts[same])
    mt, pos = rng.get_state()
    st = np.random.RandomState(M.FIXTURE_SEED)
    st.random_sample(3 * count)
    assert np.array_equal(mt, st.get_state()[1]) and pos == st.get_state()[2]
    rng.close()


@pytest.mark.parametrize('want_faces', [True, False])
def test_fed_deviates_at_the_edges_of_the_rule(want_faces):
    """p2s_mesh_sample_surface with hand-written deviates (M.fed_deviates): picks of 0.0, of exactly a cumulative value
    (searchsorted-left takes the face that ends there, also where zero-area faces repeat the value), the largest double
    below 1 with zero-area faces last; l1 + l2 exactly 1.0 and 1 + 2^-53 (not folded), one ulp above 1 (folded)"""
    torch, _lib, engine, lib = _env()
    nf = 1025
    v, f = M.lattice_mesh(nf, M.degenerate_positions(nf))
    cum = np.cumsum(M.face_areas(v, f))
    u, exact_k, n = M.fed_deviates(cum)
    want_pts, want_face, want_area, _ = M.sample_model(v, f, u)
    vt, ft, ut = _cuda(v), _cuda(f), _cuda(u)
    pts = torch.full((n + PAD, 3), float(M.SENTINEL), dtype=torch.float32, device='cuda')
    fid = torch.full((n + PAD,), -7, dtype=torch.int32, device='cuda') if want_faces else None
    area = ctypes.c_double(-1.0)
    _lib.check(lib.p2s_mesh_sample_surface(engine._ptr(vt), engine._ptr(ft), nf, engine._ptr(ut), n, engine._ptr(pts),
                                           engine._ptr(fid), ctypes.byref(area), 0, engine._stream_ptr(vt.device)))
    torch.cuda.synchronize()
    pts = pts.cpu().numpy()
    assert area.value == want_area
    assert np.all(pts[n:] == M.SENTINEL)
    if want_faces:
        fid = fid.cpu().numpy()
        assert np.all(fid[n:] == -7)
        assert np.array_equal(fid[:n], want_face), np.nonzero(fid[:n] != want_face)[0][:8]
    assert np.array_equal(pts[:n], want_pts), np.nonzero(np.any(pts[:n] != want_pts, axis=1))[0][:8]


# ---- b. remove_close through the C entry point, sentinel-filled output --------------------------------------------------

def _remove_close(pts, radius, limit, m=None, src_null=False, out_null=False, n_null=False):
    """-> (return code, n_out, output rows [m + PAD, 3]); the output starts as the sentinel, n_out as CANARY"""
    torch, _lib, engine, lib = _env()
    rows = len(pts)
    m = rows if m is None else m
    src = _cuda(pts if rows else np.zeros((1, 3), np.float32))
    out = torch.full((rows + PAD, 3), float(M.SENTINEL), dtype=torch.float32, device='cuda')
    n = ctypes.c_int64(CANARY)
    rc = lib.p2s_points_remove_close(None if src_null else engine._ptr(src), m, ctypes.c_double(radius), limit,
                                     None if out_null else engine._ptr(out), None if n_null else ctypes.byref(n), 0,
                                     engine._stream_ptr(src.device))
    torch.cuda.synchronize()
    return rc, n.value, out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _remove_close_case(name, m):
    from oracle import metrics_oracle as MO
    pts, radius = M.remove_close_input(name, m)
    keep, degree = M.remove_close_model(pts, radius)
    kept_ref, _ = MO.remove_close(pts, radius)
    assert np.array_equal(pts[keep], kept_ref)                  # the model is the oracle here
    return pts, radius, keep, degree


@pytest.mark.parametrize('m', M.M_LIST)
@pytest.mark.parametrize('name', M.REMOVE_CLOSE_INPUTS)
def test_remove_close_tiles_ties_and_exact_radius(name, m):
    """m around every multiple of the 256-point tile; uniform points, a cluster with degrees in the hundreds and stacks
    of duplicates, a lattice with pairs exactly at the radius and equal degrees, pairs straddling the tile borders, and
    radius 0.  The kept points are the model's and the oracle's, as arrays in order; nothing is written behind them."""
    pts, radius, keep, degree = _remove_close_case(name, m)
    rc, n, out = _remove_close(pts, radius, m)
    assert rc == 0
    assert n == keep.sum(), (name, m, n, int(keep.sum()), int(degree.max()))
    assert np.array_equal(out[:n], pts[keep]), (name, m, np.nonzero(np.any(out[:n] != pts[keep], axis=1))[0][:8])
    assert np.all(out[n:] == M.SENTINEL)


def test_remove_close_limit_cuts_to_the_first_kept_points():
    """the cut to `count` of sample_surface_even: the first min(limit, kept) kept points, n_out = min(limit, kept), no
    row written beyond that"""
    pts, radius, keep, _ = _remove_close_case('clustered', 3000)
    kept = int(keep.sum())
    assert 2 < kept < 2999
    for limit in (0, 1, kept - 1, kept, kept + 1, 3000):
        rc, n, out = _remove_close(pts, radius, limit)
        want = min(limit, kept)
        assert rc == 0 and n == want, (limit, n, want)
        assert np.array_equal(out[:want], pts[keep][:want]), limit
        assert np.all(out[want:] == M.SENTINEL), limit


def test_remove_close_refusals_write_nothing():
    """P2S_EINVAL, the output and n_out untouched: more than 2,000,000 points, a negative limit, NULL pointers, and a
    radius that is negative (r * r would make it |r|), infinite or NaN (NaN would remove nothing)"""
    pts, radius, keep, _ = _remove_close_case('clustered', 257)
    assert keep.sum() < 257
    refused = [dict(radius=radius, limit=257, m=2000001), dict(radius=radius, limit=-1), dict(radius=radius, limit=257, src_null=True),
               dict(radius=radius, limit=257, out_null=True), dict(radius=radius, limit=257, n_null=True)]
    refused += [dict(radius=r, limit=257) for r in (-radius, -2.0 ** -1074, -np.inf, np.inf, np.nan)]
    for kw in refused:
        rc, n, out = _remove_close(pts, **kw)
        assert rc == P2S_EINVAL, kw
        assert n == CANARY and np.all(out == M.SENTINEL), kw
    # the same call with nothing wrong is served; -0.0 is zero
    rc, n, out = _remove_close(pts, radius, 257)
    assert rc == 0 and n == keep.sum() and np.array_equal(out[:n], pts[keep])
    keep0, _ = M.remove_close_model(pts, 0.0)
    rc, n, out = _remove_close(pts, -0.0, 257)
    assert rc == 0 and n == keep0.sum() and np.array_equal(out[:n], pts[keep0])
    rc, n, out = _remove_close(np.zeros((0, 3), np.float32), radius, 0)      # m = 0: served, nothing to keep
    assert rc == 0 and n == 0 and np.all(out == M.SENTINEL)


# ---- c. nearest-neighbour statistics through the C entry point, per-query distances requested -----------------------------

def _nn_stats(cloud, q, want_dist=True, want_stats=True):
    """-> (dist [n] float64 or None, max, sum); the distance buffer is padded and the padding checked"""
    torch, _lib, engine, lib = _env()
    n = len(q)
    qt = _cuda(q)
    dist = torch.full((n + PAD,), -3.0, dtype=torch.float64, device='cuda') if want_dist else None
    mx, sm = ctypes.c_double(-1.0), ctypes.c_double(-1.0)
    _lib.check(lib.p2s_nn_distance_stats(cloud.handle, engine._ptr(qt), n, engine._ptr(dist),
                                         ctypes.byref(mx) if want_stats else None, ctypes.byref(sm) if want_stats else None,
                                         engine._stream_ptr(cloud.device)))
    torch.cuda.synchronize()
    if want_dist:
        dist = dist.cpu().numpy()
        assert np.all(dist[n:] == -3.0)
        dist = dist[:n]
    return dist, mx.value, sm.value


def _check_nn(target, q, what):
    torch, _lib, engine, lib = _env()
    n = len(q)
    want, want_max, want_sum = M.nn_model(q, target)
    cloud = engine.Cloud(target)
    try:
        dist, mx, sm = _nn_stats(cloud, q)
        again, mx2, sm2 = _nn_stats(cloud, q)
    finally:
        cloud.close()
    bad = np.nonzero(dist != want)[0]
    assert len(bad) == 0, (what, bad[:8], dist[bad[:8]], want[bad[:8]])     # a nearest-id tie changes the id, not the distance
    assert mx == want_max, (what, mx, want_max)
    # any order of summing n non-negative terms stays within (n - 1) * 2^-53 relative of the exact sum
    assert abs(sm - want_sum) <= (n - 1) * 2.0 ** -53 * want_sum, (what, sm, want_sum)
    assert np.array_equal(dist.view(np.uint64), again.view(np.uint64)) and (mx, sm) == (mx2, sm2)
    return dist


NN_SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2049)


@pytest.mark.parametrize('n', NN_SIZES)
@pytest.mark.parametrize('name', ['one', 'two', 'five', 'copies', 'coplanar', 'clustered', 'lattice'])
def test_nn_distances_per_query_max_and_sum(name, n):
    """targets: the smallest clouds, 3000 copies of one point, a flat cloud, a cluster with duplicates, a lattice; queries:
    the target's own points, points up to 10 box sizes outside, box corners, -0.0; n around the wave, the 1024-stride of the
    reduction and beyond"""
    target = M.nn_targets()[name]
    dist = _check_nn(target, M.nn_queries(target, n), '%s n %d' % (name, n))
    assert np.all(dist[1::4] == 0.0) and dist[0] > 0.0


def test_nn_distances_at_70001_queries():
    target = M.uniform_points(2000, seed=8)
    _check_nn(target, M.nn_queries(target, 70001), 'uniform 2000, n 70001')


@pytest.mark.parametrize('at', [0, 1023, 1024, 2048])
def test_nn_single_largest_distance_at_the_stride_boundaries(at):
    """n = 2049: element `at` alone is 40 box sizes away; the reduction walks the array in strides of 1024, so 0, 1023, 1024
    and n - 1 are the first and last lane of the first stride, the first lane of the second and the lone element of the third"""
    target = M.nn_targets()['coplanar']
    dist = _check_nn(target, M.nn_queries(target, 2049, far_at=at), 'far query at %d' % at)
    assert int(np.argmax(dist)) == at


def test_outlier_sets_known_answers_through_directed_stats():
    """no model involved: both directed maxima and both sums are exact numbers (M.outlier_sets)"""
    torch, _lib, engine, lib = _env()
    from points2surf_amd import metrics
    for name, a, b, (h_ab, s_ab, h_ba, s_ba) in M.outlier_sets():
        at, bt = _cuda(a), _cuda(b)
        assert metrics.directed_stats(at, bt) == (h_ab, s_ab), name
        assert metrics.directed_stats(bt, at) == (h_ba, s_ba), name


def test_nn_optional_outputs():
    """dist_out_dev NULL (what metrics.directed_stats passes) and max_host / sum_host NULL: the rest is unchanged"""
    torch, _lib, engine, lib = _env()
    target = M.nn_targets()['clustered']
    q = M.nn_queries(target, 1025)
    want, want_max, want_sum = M.nn_model(q, target)
    cloud = engine.Cloud(target)
    try:
        full = _nn_stats(cloud, q)
        none, mx, sm = _nn_stats(cloud, q, want_dist=False)
        dist, mx0, sm0 = _nn_stats(cloud, q, want_stats=False)
        assert lib.p2s_nn_distance_stats(cloud.handle, engine._ptr(_cuda(q)), 0, None, None, None, None) == P2S_EINVAL
    finally:
        cloud.close()
    assert none is None and (mx, sm) == (full[1], full[2]) and mx == want_max
    assert (mx0, sm0) == (-1.0, -1.0) and np.array_equal(dist, want) and np.array_equal(full[0], want)


# ---- d. generator renewal under random_sample ---------------------------------------------------------------------------

SESSION_WORDS = (2 * 64 - 1) * 624       # levels = 1, blocks_per_stream = 64: 79,248 words; per = (79,248 - 1024) / 2 = 39,112 doubles


def _small_session_rng(seed):
    """a generator whose sessions hold 79,248 words instead of ~327 M: jump_0 of the shipped tables alone"""
    torch, _lib, engine, lib = _env()
    rng = engine.Rng(seed, parallel=False)
    t = np.load(engine._JUMP_TABLES)
    assert int(t['blocks_per_stream']) == 64
    sup = np.ascontiguousarray(t['jump_0'], dtype=np.uint16)
    counts = np.array([sup.size], dtype=np.int32)
    _lib.check(lib.p2s_rng_set_jump_tables(rng.handle, sup.ctypes.data_as(ctypes.c_void_p), counts.ctypes.data_as(ctypes.c_void_p), 1, 64))
    return rng


def _random_sample(rng, n):
    torch, _lib, engine, lib = _env()
    out = torch.full((n + PAD,), -1.0, dtype=torch.float64, device='cuda')
    with torch.cuda.device(rng.device):
        _lib.check(lib.p2s_rng_random_sample(rng.handle, n, engine._ptr(out), engine._stream_ptr(rng.device)))
    torch.cuda.synchronize()
    a = out.cpu().numpy()
    assert np.all(a[n:] == -1.0)
    return a[:n]


@pytest.mark.parametrize('calls', [(100003,), (30000, 30000, 30000, 1, 50000)])
def test_random_sample_across_session_renewals(calls):
    """one call that takes three sessions (39,112 + 39,112 + 21,779 doubles: the output offset of every part), and calls
    between which the session runs out (60,000 + 60,000 words fit no session of 79,248): every call is numpy's
    random_sample bit for bit, and the state afterwards is numpy's"""
    assert SESSION_WORDS == 79248 and (SESSION_WORDS - 1024) // 2 == 39112
    seed = 4242
    rng, ref = _small_session_rng(seed), np.random.RandomState(seed)
    for k, n in enumerate(calls):
        got, want = _random_sample(rng, n), ref.random_sample(n)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (k, n, bad[:4], len(bad))
    mt, pos = rng.get_state()
    st = ref.get_state()
    assert np.array_equal(mt, st[1]) and pos == st[2]
    rng.check()
    rng.close()


def test_random_sample_between_uniform_subsamples_on_the_shipped_tables():
    """randint, random_sample, randint from one generator: the mode switch closes the masked-rejection session, opens a raw
    one and closes that again; the stream stays numpy's"""
    torch, _lib, engine, lib = _env()
    seed = 77
    pts = M.uniform_points(1000, seed=2)
    cloud, rng, ref = engine.Cloud(pts), engine.Rng(seed), np.random.RandomState(seed)
    try:
        a = rng.subsample_uniform(cloud, 300, 50, want_pts=False)[0].cpu().numpy().reshape(-1)
        assert np.array_equal(a, ref.randint(0, 1000, 300 * 50))
        assert np.array_equal(_random_sample(rng, 1000), ref.random_sample(1000))
        b = rng.subsample_uniform(cloud, 7, 333, want_pts=False)[0].cpu().numpy().reshape(-1)
        assert np.array_equal(b, ref.randint(0, 1000, 7 * 333))
        assert np.array_equal(_random_sample(rng, 1), ref.random_sample(1))
        mt, pos = rng.get_state()
        st = ref.get_state()
        assert np.array_equal(mt, st[1]) and pos == st[2]
        rng.check()
    finally:
        rng.close()
        cloud.close()


# ---- e. sample_surface_even end to end ----------------------------------------------------------------------------------

@pytest.mark.parametrize('which', ['lattice', 'fixture'])
def test_sample_surface_even_is_the_oracle_row_for_row(which):
    """count = 300: 900 candidates, remove_close at sqrt(area / 900), the cut to 300.  tests/test_metrics_model.py shows
    for this seed that every face pick is decided, that no candidate pair lies at the radius, and that more than 300
    survive (the cut is taken): the rows are the oracle's"""
    torch, _lib, engine, lib = _env()
    from points2surf_amd import metrics
    from oracle import metrics_oracle as MO
    count = 300
    v, f = M.even_lattice_mesh() if which == 'lattice' else _fixture_mesh(2)
    vt, ft = _cuda(v), _cuda(f)
    rng, twin = engine.Rng(M.EVEN_SEED), engine.Rng(M.EVEN_SEED)
    out = metrics.sample_surface_even(vt, ft, count, rng)
    cand, area, fid = metrics.sample_surface(vt, ft, 3 * count, twin, want_faces=True)     # the candidates it drew
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    ref_cand, ref_area, ref_face = MO.sample_surface(v, f, 3 * count, np.random.RandomState(M.EVEN_SEED))
    assert np.array_equal(fid.cpu().numpy(), ref_face) and np.array_equal(cand.cpu().numpy(), ref_cand)
    want = MO.sample_surface_even(v, f, count, np.random.RandomState(M.EVEN_SEED))
    assert out.shape[0] <= count
    assert np.array_equal(out, want)
    radius = float(np.sqrt(area / (3 * count)))                 # the radius the device used
    assert M.remove_close_model(out, radius)[0].all()           # no two rows within it
    mt, pos = rng.get_state()
    mt2, pos2 = twin.get_state()
    assert np.array_equal(mt, mt2) and pos == pos2
    rng.close()
    twin.close()
