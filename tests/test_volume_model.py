"""tests/volume_model.py against the oracle (oracle/p2s_oracle.py::propagate_sign), and the statements about the inputs of
tests/test_gpu_volume_edges.py that make those inputs worth running: a recipe that stops exercising the path it is aimed at
fails here, on the CPU."""
import numpy as np
import pytest

import volume_model as M
from oracle import p2s_oracle as O


def _smooth_random_field(res, seed, keep):
    """sign of a low-pass filtered noise field, a fraction ``keep`` of it known: several accepted sweeps, then a tie"""
    rng = np.random.default_rng(seed)
    g = O._box_sum_nearest(O._box_sum_nearest(rng.standard_normal((res, res, res)), 5), 5)
    s = np.sign(g).astype(np.int8)
    s[rng.random(s.shape) > keep] = 0
    return s


@pytest.mark.parametrize('keep', [0.05, 0.3, 0.7])
@pytest.mark.parametrize('res,sigma,thr', [(16, 1, 1), (20, 2, 3), (24, 3, 5), (31, 4, 9.5), (32, 5, 13), (17, 6, 40.5),
                                           (27, 5, 12.5), (32, 3, 4.5), (21, 6, 41)])
def test_model_is_the_oracle(res, sigma, thr, keep):
    s0 = _smooth_random_field(res, res * 7 + sigma, keep)
    mag = np.random.default_rng(1).uniform(0.1, 2.0, size=s0.shape).astype(np.float32)      # some above 1: the clamp
    s, sweeps, why, left = M.propagate(s0, sigma, thr)
    got = M.compose(s0 * mag, s, clamp=True)
    ref, it_ref = O.propagate_sign((s0 * mag).astype(np.float64), sigma, thr, return_iters=True)
    assert sweeps == it_ref
    assert np.array_equal(got.astype(np.float64), np.clip(ref, -1.0, 1.0)), M.first_difference(got, np.clip(ref, -1, 1))
    assert left == np.count_nonzero(s == 0) and why == ('known' if left == 0 else 'tie')


def test_model_runs_more_than_one_sweep_somewhere():
    """the comparison above is not one of single discarded sweeps"""
    counts = [M.propagate(_smooth_random_field(res, res * 7 + sigma, 0.3), sigma, thr)[1]
              for res, sigma, thr in [(20, 2, 3), (24, 3, 5), (32, 5, 13), (21, 6, 41)]]
    assert min(counts) >= 3, counts


def test_model_through_the_sample_helper_is_the_oracles_sdf_volume():
    s0 = M.sparse_random_field(32)
    q, d = M.samples_from_signs(s0, 0.5)
    assert q.dtype == np.float32 and d.dtype == np.float32 and len(d) == np.count_nonzero(s0)
    assert np.array_equal(O.model_space_to_volume_space(q, 32), np.argwhere(s0 != 0))       # sorted, one per voxel
    got, sweeps, _, _ = M.expected_volume(s0, 5, 13.0)
    assert sweeps >= 2
    assert np.array_equal(got.astype(np.float64), O.sdf_volume(q, d, 32, 5, 13.0))


@pytest.mark.parametrize('res', [32, 64, 128, 208, 256])
def test_voxel_centres_fall_into_their_voxels_in_float32(res):
    s = np.zeros((res, res, res), np.int8)
    idx = np.arange(res)
    s[idx, idx, idx[::-1]] = 1
    q, d = M.samples_from_signs(s)                          # asserts floor((q + 1) / 2 * res) == i for every i
    assert np.array_equal(O.model_space_to_volume_space(q, res), np.stack([idx, idx, idx[::-1]], axis=1))


def test_tile_activity_is_the_widened_box_rule():
    """tile_activity against the definition, voxel by voxel, at a tile size small enough to enumerate"""
    s0 = _smooth_random_field(24, 3, 0.15)
    tile, halo = (4, 8, 16), 2
    act, slab = M.tile_activity(s0, 3, 5, tile=tile, halo=halo)
    fields = [s0]
    M.propagate(s0, 3, 5, on_accept=lambda k, a, b: fields.append(b))
    nt = [6, 3, 2]
    assert slab == -(-36 // 8) and len(act) >= 3 and act[0].sum() == 36
    for k in range(1, len(act)):
        changed = np.argwhere(fields[k - 1] != fields[k])
        want = np.zeros(8, np.int64)
        for t in range(36):
            tx, ty, tz = t // 6, (t // 2) % 3, t % 2
            lo = np.array([tx * 4, ty * 8, tz * 16]) - halo
            hi = np.array([tx * 4 + 4, ty * 8 + 8, tz * 16 + 16]) + halo
            want[t // slab] += bool(np.any(np.all((changed >= lo) & (changed < hi), axis=1)))
        assert np.array_equal(act[k], want), k
    assert nt[0] * nt[1] * nt[2] == 36


# ---- a. steered sweep counts ----------------------------------------------------------------------------------------

@pytest.mark.parametrize('axis', [0, 1, 2])
@pytest.mark.parametrize('res,p,sweeps', M.SLAB_CASES)
def test_slab_inputs_end_known_after_the_steered_count(res, p, sweeps, axis):
    s, n, why, left = M.propagate(M.slab_field(res, p, axis), 3, 5)
    assert (n, why, left) == (sweeps, 'known', 0)
    assert np.all(s == -1)


def test_slab_counts_sit_on_the_batch_seams():
    assert sorted(c[2] for c in M.SLAB_CASES) == [15, 16, 17, 31, 32, 33]


def test_all_known_and_unreachable_threshold():
    s0 = np.where(M.sparse_random_field(32) == 1, 1, -1).astype(np.int8)
    assert M.propagate(s0, 3, 5)[1:] == (0, 'known', 0)
    s0 = M.sparse_random_field(32)
    s, n, why, left = M.propagate(s0, 3, 28.0)               # thr > sigma^3: one sweep, discarded
    assert (n, why) == (1, 'tie') and np.array_equal(s, s0) and left == np.count_nonzero(s0 == 0)


# ---- b. sparse fronts, ties, long runs -------------------------------------------------------------------------------

SEED_CASES = [(64, 3, 5.0, ()), (64, 5, 13.0, ()), (128, 5, 13.0, tuple(M.SEED_CENTRES_128))]


@pytest.mark.parametrize('res,sigma,thr,centres', SEED_CASES)
def test_seed_block_inputs_run_long_and_end_in_a_tie(res, sigma, thr, centres):
    s0 = M.seed_blocks_field(res, 7, centres)
    assert np.count_nonzero(s0 == 1) == 3 * 125 and np.count_nonzero(s0 == -1) == 3 * 125     # six whole, disjoint blocks
    s, sweeps, why, left = M.propagate(s0, sigma, thr)
    assert why == 'tie' and left > 0 and sweeps >= 32, (sweeps, why, left)
    assert np.count_nonzero(s == 1) > 1000 and np.count_nonzero(s == -1) > 1000               # both signs grew: fronts met


def test_seed_centres_at_128_sit_on_tile_corners_and_inside_a_tile():
    on_corner = [c for c in M.SEED_CENTRES_128 if c[0] % 8 == 0 and c[1] % 16 == 0 and c[2] == 64]
    assert len(on_corner) >= 2
    x, y, z = M.SEED_CENTRES_128[2]
    assert x // 8 == (x - 2) // 8 == (x + 2) // 8 and y // 16 == (y - 2) // 16 == (y + 2) // 16 and z // 64 == (z - 2) // 64 == (z + 2) // 64


# ---- c. more than one tile per workgroup ----------------------------------------------------------------------------

def test_holes_input_keeps_a_slab_above_its_workgroups_after_sweep_0():
    """208^3: 4 x 13 x 26 = 1352 tiles of 8 x 16 x 64 > 1024 workgroups = 128 per slab of 169 tiles.  Sweep 0 evaluates every
    tile; the input must give some slab more than 128 ACTIVE tiles in at least two later sweeps, so workgroups walk two
    tiles of a compact list that earlier sweeps built."""
    s0 = M.holes_field()
    assert s0.shape == (208, 208, 208) and 208 % 16 == 0
    frac = np.count_nonzero(s0 == 0) / s0.size
    assert 0.1 < frac < 0.25, frac
    faces = [s0[0], s0[-1], s0[:, 0], s0[:, -1], s0[:, :, 0], s0[:, :, -1]]
    assert sum(bool(np.any(f == 0)) for f in faces) >= 3 and np.count_nonzero(s0 == 1) > 0          # holes touch faces
    assert np.any(s0[:, :, 192:] == 0) and np.any(s0[:, :, -1] == 0)                                # ... and the partial z tile
    act, slab = M.tile_activity(s0, 5, 13.0)
    assert slab == 169 and act[0].sum() == 1352
    _, sweeps, why, left = M.propagate(s0, 5, 13.0)
    assert sweeps == len(act) and sweeps >= 8, sweeps
    assert why == 'tie' and left > 0
    busiest = act[1:].max(axis=1)
    assert np.count_nonzero(busiest > 128) >= 2, busiest
    assert busiest[-1] < 128                                   # ... and the lists shrink below one tile per workgroup again


# ---- d. thresholds ---------------------------------------------------------------------------------------------------

def test_threshold_list_separates_outputs():
    s0 = M.sparse_random_field(32)
    frac_m, frac_p = np.mean(s0 == -1), np.mean(s0 == 1)
    assert 0.17 < frac_m < 0.23 and 0.08 < frac_p < 0.12 and not np.any(s0[16:, :, :][:, :4] == 1)
    q, d = M.samples_from_signs(s0)
    outs = {}
    for sigma, thr in M.THRESHOLDS:
        outs[(sigma, thr)] = O.sdf_volume(q, d, 32, sigma, thr)
        assert np.array_equal(M.expected_volume(s0, sigma, thr)[0].astype(np.float64), outs[(sigma, thr)])
    five = [outs[k] for k in M.THRESHOLDS if k[0] == 5]
    assert len(five) == 9
    distinct = {v.tobytes() for v in five}
    assert len(distinct) >= 4, len(distinct)                 # 0.5 | 1.5 | 12.5, 13 | 13.5 | >= 124.5 at least


def test_pinhole_inputs_decide_at_the_top_of_the_threshold_range():
    s0 = M.pinhole_field(32)
    n = np.count_nonzero(s0 == 0)
    assert n == 125 and np.abs(M.box_sum(s0, 5))[s0 == 0].max() == 124 and np.abs(M.box_sum(s0, 3))[s0 == 0].max() == 26
    want = {(5, 124.0): (1, 'known', 0), (5, 124.5): (1, 'tie', n), (5, 125.0): (1, 'tie', n),
            (3, 26.0): (1, 'known', 0), (3, 26.5): (1, 'tie', n), (3, 27.0): (1, 'tie', n)}
    assert sorted(want) == sorted(M.PINHOLE_THRESHOLDS)
    q, d = M.samples_from_signs(s0)
    for (sigma, thr), w in want.items():
        v, sweeps, why, left = M.expected_volume(s0, sigma, thr)
        assert (sweeps, why, left) == w, (sigma, thr)
        assert np.array_equal(v.astype(np.float64), O.sdf_volume(q, d, 32, sigma, thr))
        assert np.count_nonzero(v == 0) == left


# ---- e. / f. ----------------------------------------------------------------------------------------------------------

def test_generic_cases_are_sizes_the_fused_path_does_not_serve():
    for res, sigma, thr in M.GENERIC_CASES:
        assert res % 16 != 0 or sigma > 5
    assert any(res % 16 != 0 and res % 2 == 1 for res, _, _ in M.GENERIC_CASES)


def test_values_case_holds_what_it_is_for():
    q, d = M.values_case(32)
    v = O.model_space_to_volume_space(q, 32)
    assert len(np.unique(v, axis=0)) == len(v)                                   # one sample per voxel
    assert np.any(np.abs(d) > 1) and np.any((d == 0) & np.signbit(d))
    assert np.any((v == 0).any(axis=1) | (v == 31).any(axis=1))                  # samples on border voxels
    a, b = O.sdf_volume(q, d, 32, 5, 13.0, clamp=True), O.sdf_volume(q, d, 32, 5, 13.0, clamp=False)
    assert np.abs(a).max() == 1.0 and np.abs(b).max() == 3.5 and not np.array_equal(a, b)
