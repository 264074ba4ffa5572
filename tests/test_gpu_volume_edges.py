"""Sign propagation on the GPU where the fused sweep kernel (vol_sweep_kernel, p2s_volume.hip) can go wrong unseen by
noisy spheres: steered sweep counts on the seams of the host protocols, sparse fronts that meet in ties over dozens of
sweeps, more active tiles than workgroups, every threshold regime of the byte compare, the three-pass path at sizes it
alone serves, and the values the drop-in passes.  Expected values: tests/volume_model.py (pinned to the oracle by
tests/test_volume_model.py, which also pins what each input is for) and, up to 64^3, the oracle itself.  Everything is
bit-exact: np.array_equal on the float32 volume, == on the sweep count."""
import functools

import numpy as np
import pytest

import volume_model as M

pytestmark = pytest.mark.gpu

PROTOCOLS = ['mailbox', 'copy_per_batch']


def _protocol(monkeypatch, protocol, generic=False):
    monkeypatch.delenv('P2S_VOLUME_NO_MAILBOX', raising=False)
    monkeypatch.delenv('P2S_VOLUME_GENERIC', raising=False)
    if protocol == 'copy_per_batch':
        monkeypatch.setenv('P2S_VOLUME_NO_MAILBOX', '1')
    if generic:
        monkeypatch.setenv('P2S_VOLUME_GENERIC', '1')


def _run(q, d, res, sigma, thr, clamp=True):
    from points2surf_amd import engine
    vol, iters = engine.sdf_volume(q, d, res, sigma, thr, clamp=clamp)
    v = vol.cpu().numpy()
    assert v.dtype == np.float32 and v.shape == (res, res, res)
    return v, iters


def _same(got, want, what, iters=None, sweeps=None):
    """the volume first: its message names the first differing voxel and its tile; then the sweep count"""
    assert np.array_equal(got, want), '%s: %s; sweeps %s, expected %s' % (what, M.first_difference(got, want), iters, sweeps)
    assert iters == sweeps, '%s: %s sweeps, expected %s' % (what, iters, sweeps)


def _oracle(q, d, res, sigma, thr, clamp=True):
    from oracle import p2s_oracle as O
    vol = np.zeros((res, res, res))
    vol = O.add_samples_to_volume(vol, q, d)
    vol, iters = O.propagate_sign(vol, sigma, thr, return_iters=True)
    if clamp:
        vol = np.clip(vol, -1.0, 1.0)
    assert np.array_equal(vol, O.sdf_volume(q, d, res, sigma, thr, clamp=clamp))
    return vol, iters


@functools.lru_cache(maxsize=None)
def _field_case(kind, res, sigma, thr, *args):
    """-> (q, d, model volume, model sweeps, oracle volume or None): computed once per module"""
    if kind == 'slab':
        s0 = M.slab_field(res, *args)
    elif kind == 'seeds':
        s0 = M.seed_blocks_field(res, 7, M.SEED_CENTRES_128 if res == 128 else ())
    elif kind == 'holes':
        s0 = M.holes_field(res)
    elif kind == 'sparse':
        s0 = M.sparse_random_field(res)
    elif kind == 'pinhole':
        s0 = M.pinhole_field(res)
    elif kind == 'known':
        s0 = np.where(M.sparse_random_field(res) == 1, 1, -1).astype(np.int8)
    else:
        raise ValueError(kind)
    q, d = M.samples_from_signs(s0, 0.5)
    want, sweeps, why, left = M.expected_volume(s0, sigma, thr, 0.5)
    ref = None
    if res <= 64:
        ref, it_ref = _oracle(q, d, res, sigma, thr)
        assert it_ref == sweeps and np.array_equal(want.astype(np.float64), ref)       # the model is the oracle here
    return q, d, want, sweeps, ref


def _check_field_case(case, res, sigma, thr, what):
    q, d, want, sweeps, ref = case
    got, iters = _run(q, d, res, sigma, thr)
    _same(got, want, what, iters, sweeps)
    if ref is not None:
        _same(got.astype(np.float64), ref, what + ' (oracle)', iters, sweeps)
    return got


# ---- a. steered sweep counts, under both host protocols --------------------------------------------------------------

SLAB_RUNS = [(res, p, n, 2) for res, p, n in M.SLAB_CASES] + \
            [(res, p, n, axis) for res, p, n in M.SLAB_CASES if n in (16, 32) for axis in (0, 1)]


@pytest.mark.parametrize('protocol', PROTOCOLS)
@pytest.mark.parametrize('res,p,sweeps,axis', SLAB_RUNS)
def test_steered_sweep_counts(res, p, sweeps, axis, protocol, monkeypatch):
    """a one-voxel slab of -1 at index p along one axis (2 = z, the byte-packed one), the rest unknown, sigma 3, thr 5:
    the verdict 'everything known' falls at launch 15, 16, 17, 31, 32, 33 -- on and around the seams of the batches of 16
    whose verdict the copy-per-batch protocol reads one batch late, and past the mailbox protocol's four launches ahead"""
    case = _field_case('slab', res, 3, 5.0, p, axis)
    assert case[3] == sweeps
    _protocol(monkeypatch, protocol)
    got = _check_field_case(case, res, 3, 5.0, 'slab res %d p %d axis %d, %s' % (res, p, axis, protocol))
    assert np.all(got[1:-1, 1:-1, 1:-1] < 0)


@pytest.mark.parametrize('protocol', PROTOCOLS)
def test_all_known_volume_takes_no_sweep(protocol, monkeypatch):
    case = _field_case('known', 32, 3, 5.0)
    assert case[3] == 0
    _protocol(monkeypatch, protocol)
    _check_field_case(case, 32, 3, 5.0, 'all known, ' + protocol)


@pytest.mark.parametrize('protocol', PROTOCOLS)
def test_threshold_above_the_full_box_takes_one_sweep_and_fills_nothing(protocol, monkeypatch):
    case = _field_case('sparse', 32, 3, 28.0)
    assert case[3] == 1
    _protocol(monkeypatch, protocol)
    got = _check_field_case(case, 32, 3, 28.0, 'thr 28 > 27, ' + protocol)
    assert np.count_nonzero(got == 0) == np.count_nonzero(M.sparse_random_field(32)[1:-1, 1:-1, 1:-1] == 0)


# ---- b. sparse fronts, ties and long runs ----------------------------------------------------------------------------

@pytest.mark.parametrize('res,sigma,thr', [(64, 3, 5.0), (64, 5, 13.0), (128, 5, 13.0)])
def test_seed_blocks_sparse_fronts_meeting_in_ties(res, sigma, thr, monkeypatch):
    """six 5^3 blocks of alternating sign in an unknown volume: thin fronts cross quiet tiles (the activation masks and the
    compact lists carry them), meet in ties, and the run ends by 'no progress' with unknowns left after dozens of sweeps:
    the speculative buffer is discarded, and the totals the verdict reads have been carried as deltas all the way"""
    case = _field_case('seeds', res, sigma, thr)
    assert case[3] >= 32
    for protocol in PROTOCOLS:
        _protocol(monkeypatch, protocol)
        got = _check_field_case(case, res, sigma, thr, 'seed blocks res %d sigma %d, %s' % (res, sigma, protocol))
        assert np.count_nonzero(got == 0) > 0


# ---- c. more active tiles than workgroups ----------------------------------------------------------------------------

def test_more_than_one_tile_per_workgroup_at_208(monkeypatch):
    """208^3 = 1352 tiles on 1024 workgroups; the holes input keeps a slab above 128 active tiles for sweeps after the
    first (tests/test_volume_model.py), so workgroups walk two tiles of a list that earlier sweeps built: the prefetch of
    the next tile, the s_changed ping-pong and the per-tile count deltas run with n_act > 1.  The last z tile is three
    quarters outside the volume."""
    res, sigma, thr = 208, 5, 13.0
    case = _field_case('holes', res, sigma, thr)
    q, d, want, sweeps, _ = case
    assert sweeps >= 8
    import torch
    qd, dd = torch.from_numpy(q).cuda(), torch.from_numpy(d).cuda()
    _protocol(monkeypatch, 'mailbox')
    first, it_first = _run(qd, dd, res, sigma, thr)
    _same(first, want, 'holes 208, fused', it_first, sweeps)
    # scratch, lists and flags are reused: a call at another size in between must leave nothing behind
    small = _field_case('sparse', 32, 5, 13.0)
    _check_field_case(small, 32, 5, 13.0, 'sparse 32 between the two calls at 208')
    again, it_again = _run(qd, dd, res, sigma, thr)
    _same(again, want, 'holes 208, fused, repeated after a call at 32', it_again, sweeps)
    _protocol(monkeypatch, 'copy_per_batch')
    batch, it_batch = _run(qd, dd, res, sigma, thr)
    _same(batch, want, 'holes 208, fused, copy per batch', it_batch, sweeps)
    _protocol(monkeypatch, 'mailbox', generic=True)
    generic, it_generic = _run(qd, dd, res, sigma, thr)
    _same(generic, want, 'holes 208, three-pass path', it_generic, sweeps)


# ---- d. thresholds on the device ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('sigma,thr', M.THRESHOLDS)
def test_thresholds_on_a_sparse_field(sigma, thr, monkeypatch):
    """about 20 % -1 everywhere, about 20 % +1 in one half: sums of every size and both signs against the byte compare's
    constants from 'always' (thr <= 1) to 'never' (thr above the full box)"""
    _protocol(monkeypatch, 'mailbox')
    _check_field_case(_field_case('sparse', 32, sigma, thr), 32, sigma, thr, 'sparse sigma %d thr %g' % (sigma, thr))


@pytest.mark.parametrize('sigma,thr', M.PINHOLE_THRESHOLDS)
def test_thresholds_at_the_top_of_the_range(sigma, thr, monkeypatch):
    """single unknown voxels in a solid volume: box sums one short of full, so the compare at full - 1, full - 0.5 and full
    decides between 'all filled' and 'sweep discarded'"""
    _protocol(monkeypatch, 'mailbox')
    case = _field_case('pinhole', 32, sigma, thr)
    got = _check_field_case(case, 32, sigma, thr, 'pinholes sigma %d thr %g' % (sigma, thr))
    assert np.count_nonzero(got == 0) == (0 if thr < sigma ** 3 - 0.75 else 125)


# ---- e. the three-pass path at sizes it alone serves -------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _generic_case(kind, res, sigma, thr):
    if kind == 'sphere':
        q, d = M.noisy_sphere_samples(res)
    else:
        q, d = M.samples_from_signs(M.seed_blocks_field(res, 7), 0.5)
    ref, it_ref = _oracle(q, d, res, sigma, thr)
    return q, d, ref, it_ref


@pytest.mark.parametrize('kind', ['sphere', 'seeds'])
@pytest.mark.parametrize('res,sigma,thr', M.GENERIC_CASES)
def test_three_pass_path_against_the_oracle(res, sigma, thr, kind, monkeypatch):
    """res % 16 != 0 or sigma > 5: only the separable three-pass path with a host decision per sweep runs"""
    _protocol(monkeypatch, 'mailbox')
    q, d, ref, it_ref = _generic_case(kind, res, sigma, thr)
    assert it_ref >= 2
    got, iters = _run(q, d, res, sigma, thr)
    _same(got.astype(np.float64), ref, '%s res %d sigma %d' % (kind, res, sigma), iters, it_ref)


# ---- f. values ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('generic', [False, True])
@pytest.mark.parametrize('clamp', [True, False])
def test_sample_values_outside_the_unit_range_with_and_without_clamp(clamp, generic, monkeypatch):
    """magnitudes above 1, a -0.0 sample (no sign: unknown, filled), samples on border voxels (they seed the propagation
    and are then overwritten by -1); clamp=False is the call of the drop-in's propagate_sign"""
    q, d = M.values_case(32)
    ref, it_ref = _oracle(q, d, 32, 5, 13.0, clamp=clamp)
    _protocol(monkeypatch, 'mailbox', generic=generic)
    got, iters = _run(q, d, 32, 5, 13.0, clamp=clamp)
    _same(got.astype(np.float64), ref, 'values clamp=%s generic=%s' % (clamp, generic), iters, it_ref)
    assert np.abs(got).max() == (1.0 if clamp else 3.5)
