"""Integer restatement of the sign propagation (oracle/p2s_oracle.py::propagate_sign, reference source/sdf.py:114-178) for
the sizes at which the float64 oracle is too slow (128^3, 208^3), the way the other tests/*_model.py files restate their
device algorithms -- plus the inputs of tests/test_gpu_volume_edges.py and the statements about those inputs that
tests/test_volume_model.py pins on the CPU.

    state      int8 sign field s and the mask unknown_initially = (s == 0) of the initial field
    box sum    int16, separable, scipy's taps  out[i] = sum_j in[i + sigma // 2 - j], j = 0 .. sigma - 1, edges replicated
    decision   |sum| < float32(thr) -> 0, else sign(sum)
    loop       stop ('known') when no voxel is unknown; evaluate a sweep; stop ('tie') when the zeros of the new field are
               no fewer than the unknowns before it (the sweep is discarded); else s[unknown_initially] = new[...]

Nothing here reads anything from the kernel: the tile activity below is a statement about the INPUT (which tiles of a
given size see a change inside their box widened by the halo), derived from the rule above alone."""
import numpy as np


def box_sum(s, sigma):
    """sigma^3 box sum of an int8 / int16 field, int16, scipy.ndimage.convolve(ones, mode='nearest', origin 0)"""
    sigma = int(sigma)
    assert 1 <= sigma <= 31                                  # 31^3 = 29791 fits int16
    hi, lo = sigma // 2, sigma - 1 - sigma // 2              # offsets hi, hi - 1, ..., -lo
    out = s.astype(np.int16)
    for axis in range(3):
        n = out.shape[axis]
        pad = [(0, 0)] * 3
        pad[axis] = (lo, hi)
        p = np.pad(out, pad, mode='edge')
        acc = np.zeros_like(out)
        for o in range(-lo, hi + 1):
            sl = [slice(None)] * 3
            sl[axis] = slice(lo + o, lo + o + n)
            acc += p[tuple(sl)]
        out = acc
    return out


def new_signs(s, sigma, thr):
    a = box_sum(s, sigma)
    return np.where(np.abs(a).astype(np.float32) < np.float32(thr), 0, np.sign(a)).astype(np.int8)


def propagate(sign0, sigma, thr, on_accept=None):
    """-> (final int8 sign field, sweeps, 'known' | 'tie', unknowns left).  ``sweeps`` counts every evaluated sweep, the
    discarded last one of a 'tie' included (the reference's ``iters``).  ``on_accept(k, before, after)`` is called for
    every accepted sweep k with the sign fields around it."""
    s = np.array(sign0, dtype=np.int8)
    assert s.ndim == 3 and s.shape[0] == s.shape[1] == s.shape[2] and np.all(np.abs(s) <= 1)
    unk0 = s == 0
    sweeps = 0
    while True:
        before = int(np.count_nonzero(s == 0))
        if before == 0:
            why = 'known'
            break
        new = new_signs(s, sigma, thr)
        sweeps += 1
        if int(np.count_nonzero(new == 0)) >= before:
            why = 'tie'
            break
        nxt = np.where(unk0, new, s)
        if on_accept is not None:
            on_accept(sweeps - 1, s, nxt)
        s = nxt
    return s, sweeps, why, int(np.count_nonzero(s == 0))


def compose(vol0, s_final, clamp=True):
    """the volume handed to the iso-surface: the samples, the six faces -1, every remaining zero the propagated sign,
    optionally clamped to [-1, 1] (reference source/sdf.py:128-133, 177, 199-201)"""
    v = np.array(vol0, dtype=np.float32)
    for a in range(3):
        sl = [slice(None)] * 3
        for i in (0, -1):
            sl[a] = i
            v[tuple(sl)] = -1.0
    zero = v == 0
    v[zero] = s_final[zero].astype(np.float32)
    if clamp:
        v = np.clip(v, -1.0, 1.0)
    return v


def expected_volume(sign0, sigma, thr, magnitude=0.5, clamp=True):
    """-> (float32 volume, sweeps, why, unknowns left) for the samples ``samples_from_signs(sign0, magnitude)``"""
    s, sweeps, why, left = propagate(sign0, sigma, thr)
    vol0 = np.asarray(sign0, dtype=np.float32) * np.float32(magnitude)
    return compose(vol0, s, clamp), sweeps, why, left


def samples_from_signs(sign0, magnitude=0.5):
    """a sign field as inputs of sdf_volume: one sample sign * magnitude at the centre of every known voxel, in voxel order
    (sorted, one per voxel: the contract of add_samples_to_volume); unknown voxels get none.  ``magnitude``: scalar or
    per-voxel array."""
    s = np.asarray(sign0)
    res = s.shape[0]
    c = ((np.arange(res, dtype=np.float32) + np.float32(0.5)) / np.float32(res) * np.float32(2.0) - np.float32(1.0)).astype(np.float32)
    back = np.floor((c + np.float32(1.0)) / np.float32(2.0) * np.float32(res))           # source/sdf.py:73-75 in float32
    assert back.dtype == np.float32 and np.array_equal(back, np.arange(res)), res
    ix, iy, iz = np.nonzero(s)
    q = np.stack([c[ix], c[iy], c[iz]], axis=1).astype(np.float32)
    mag = np.broadcast_to(np.asarray(magnitude, dtype=np.float32), s.shape)
    d = (s[ix, iy, iz].astype(np.float32) * mag[ix, iy, iz]).astype(np.float32)
    return q, d


def tile_activity(sign0, sigma, thr, tile=(8, 16, 64), halo=2):
    """-> (int array [sweeps, 8], tiles per slab): how many tiles of each of the 8 contiguous slabs of the tile order
    (x slowest, z fastest; slab = ceil(n_tiles / 8)) have to be evaluated in each sweep.  Sweep 0 evaluates every tile;
    sweep k >= 1 those tiles in whose box, widened by ``halo`` and clipped to the volume, a state byte was changed by
    sweep k - 1 (every other tile would reproduce its previous output)."""
    res = np.asarray(sign0).shape[0]
    nt = [-(-res // t) for t in tile]
    n_tiles = nt[0] * nt[1] * nt[2]
    slab = -(-n_tiles // 8)
    slab_of = np.arange(n_tiles) // slab
    rows = [np.bincount(slab_of, minlength=8)]

    def on_accept(k, before, after):
        m = before != after
        for a in range(3):
            parts = []
            for t in range(nt[a]):
                sl = [slice(None)] * 3
                sl[a] = slice(max(t * tile[a] - halo, 0), min((t + 1) * tile[a] + halo, res))
                parts.append(m[tuple(sl)].any(axis=a))
            m = np.stack(parts, axis=a)
        rows.append(np.bincount(slab_of[m.reshape(-1)], minlength=8))

    _, sweeps, why, _ = propagate(sign0, sigma, thr, on_accept)
    # one row per evaluated sweep: the discarded last sweep of a 'tie' has one, the stop after a 'known' run has none
    return np.array(rows[:sweeps], dtype=np.int64).reshape(-1, 8), slab


# ---------------------------------------------------------------------------------------------------------------------
# the inputs of tests/test_gpu_volume_edges.py
# ---------------------------------------------------------------------------------------------------------------------

# (res, p, sweeps): a one-voxel slab of -1 at index p along one axis, the rest unknown, sigma 3, thr 5: the front moves one
# voxel per sweep, the run ends 'known' after max(p, res - 1 - p) sweeps -- on and around the seams of the batches of 16
SLAB_CASES = [(16, 0, 15), (32, 15, 16), (32, 14, 17), (32, 0, 31), (48, 15, 32), (48, 14, 33)]


def slab_field(res, p, axis):
    s = np.zeros((res, res, res), np.int8)
    sl = [slice(None)] * 3
    sl[axis] = p
    s[tuple(sl)] = -1
    return s


def _put(s, centre, side, value):
    lo = [int(c) - side // 2 for c in centre]
    s[tuple(slice(max(l, 0), max(l + side, 0)) for l in lo)] = value


def seed_blocks_field(res, seed=7, centres=()):
    """six 5^3 blocks of alternating sign in an unknown volume: ``centres`` first, the rest placed by default_rng(seed)"""
    rng = np.random.default_rng(seed)
    s = np.zeros((res, res, res), np.int8)
    cs = [tuple(c) for c in centres]
    while len(cs) < 6:
        cs.append(tuple(int(v) for v in rng.integers(4, res - 4, size=3)))
    for i, c in enumerate(cs):
        _put(s, c, 5, 1 if i % 2 == 0 else -1)
    return s


# at 128: two blocks centred on tile corners (x a multiple of 8, y of 16, z = 64), one well inside a tile
SEED_CENTRES_128 = [(40, 48, 64), (88, 80, 64), (20, 24, 32)]


def holes_field(res=208, seed=3, boxes=140, blocks=12):
    """known -1 everywhere; ``boxes`` random boxes of unknown (sides 6 .. 43, free to overlap and to touch the faces);
    ``blocks`` 5^3 blocks of +1"""
    rng = np.random.default_rng(seed)
    s = np.full((res, res, res), -1, np.int8)
    for _ in range(boxes):
        side = rng.integers(6, 44, size=3)
        lo = [int(rng.integers(0, res - int(d) + 1)) for d in side]
        s[tuple(slice(l, l + int(d)) for l, d in zip(lo, side))] = 0
    s[:20, :20, res - 20:] = 0          # one hole in the corner of the last z tile (208 = 3 x 64 + 16), on three faces
    for _ in range(blocks):
        _put(s, rng.integers(2, res - 2, size=3), 5, 1)
    return s


def sparse_random_field(res=32, seed=5):
    """about 20 % -1 everywhere, about 20 % +1 in one half only, the rest unknown"""
    rng = np.random.default_rng(seed)
    u = rng.random((res, res, res))
    s = np.zeros((res, res, res), np.int8)
    s[u < 0.2] = -1
    plus = (u >= 0.2) & (u < 0.4)
    plus[res // 2:] = False
    s[plus] = 1
    return s


def pinhole_field(res=32):
    """known -1 everywhere but single unknown voxels on a lattice of spacing 6: every box that holds one sums to one short
    of full (-124 at sigma 5, -26 at sigma 3).  At thr = full - 1 the sweep is accepted and fills them all; from
    full - 0.5 on every such box is a zero of the new field, more than there were unknowns, and the sweep is discarded:
    the only inputs on which the decision at the top of the threshold range changes the output."""
    s = np.full((res, res, res), -1, np.int8)
    s[3::6, 3::6, 3::6] = 0
    return s


THRESHOLDS = [(5, t) for t in (0.5, 1.0, 1.5, 12.5, 13.0, 13.5, 124.5, 125.0, 126.0)] + \
             [(3, 26.5), (3, 27.0), (3, 28.0), (2, 8.0), (1, 1.0)]
PINHOLE_THRESHOLDS = [(5, 124.0), (5, 124.5), (5, 125.0), (3, 26.0), (3, 26.5), (3, 27.0)]

# sizes only the three-pass path serves (res % 16 != 0 or sigma > 5)
GENERIC_CASES = [(20, 5, 13.0), (33, 5, 13.0), (50, 5, 13.0), (33, 4, 9.5), (32, 7, 40.0)]


def noisy_sphere_samples(res, seed=0):
    """the recipe of test_gpu_volume.py's oracle test: a band of samples around a sphere of radius 0.5, one per voxel"""
    from oracle import p2s_oracle as O
    from points2surf_amd import synth
    pts = synth.make_cloud(20000, seed=3, kind='sphere')
    q, _ = O.query_grid(pts, res, 3)
    d = (0.5 - np.linalg.norm(q, axis=1)).astype(np.float32)
    d += (0.002 * np.random.default_rng(seed).standard_normal(d.shape)).astype(np.float32)
    return np.ascontiguousarray(q, dtype=np.float32), d


def values_case(res=32, seed=9):
    """-> (q, d): samples with magnitudes above 1, an exact -0.0 and samples on border voxels (the drop-in calls with
    clamp=False; nothing clamps the samples before the call)"""
    rng = np.random.default_rng(seed)
    s = sparse_random_field(res, seed)
    mag = rng.uniform(0.05, 0.9, size=s.shape).astype(np.float32)
    mag[rng.random(s.shape) < 0.1] = 3.5
    s[0, 5, 5], s[res - 1, 6, 7], s[9, 0, 3], s[4, 4, res - 1] = 1, -1, 1, 1       # on the faces
    mag[0, 5, 5], mag[res - 1, 6, 7] = 3.5, 0.25
    s[10, 11, 12] = -1
    mag[10, 11, 12] = 0.0                                                          # -1 * 0.0 = -0.0: a sample that is no sign
    q, d = samples_from_signs(s, mag)
    assert np.any(np.abs(d) > 1) and np.any((d == 0) & np.signbit(d))
    return q, d


def first_difference(a, b, tile=(8, 16, 64)):
    """message for a failed volume comparison: the first differing voxel and the tile it lies in"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return 'shapes %s %s' % (a.shape, b.shape)
    diff = np.argwhere(a != b)
    if len(diff) == 0:
        return 'equal'
    v = tuple(int(c) for c in diff[0])
    t = tuple(c // n for c, n in zip(v, tile))
    nt = [-(-a.shape[i] // tile[i]) for i in range(3)]
    return '%d voxels differ; first at %s (got %r, want %r) in tile (tx, ty, tz) = %s, tile index %d' % (
        len(diff), v, a[v].item(), b[v].item(), t, (t[0] * nt[1] + t[1]) * nt[2] + t[2])
