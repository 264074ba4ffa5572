"""The numpy model of the renderer (tests/figure_model.py) against closed forms, and the host parts of points2surf_amd/figure.py
(normalisation target, colour index, colour map, PNG writer, camera fit, direction table) against short restatements.  No
device."""
import math

import numpy as np
import pytest

import figure_model as FM
from points2surf_amd import figure


def byte_of(x):
    return int(math.floor(255.0 * math.sqrt(x) + 0.5))


def test_icosphere_head_on_depth_within_the_sagitta():
    v, f = FM.icosphere(2)
    distance = 3.0
    p = FM.params(width=9, height=9, eye=(0.0, 0.0, distance), tan_half_w=0.4, tan_half_h=0.4)
    m = FM.render(v, f, p)
    tri = v.astype(np.float64)[f]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    plane = np.abs((n * tri[:, 0]).sum(1)) / np.sqrt((n * n).sum(1))           # the faces' distances from the centre
    sagitta = 1.0 - plane.min()
    assert 0.0 < sagitta < 0.03
    centre = m['depth'][4, 4]                                                  # sx = sy = 0: the ray through the centre, |d| = 1
    assert distance - 1.0 - 1e-7 <= centre <= distance - 1.0 + sagitta
    assert m['face'][4, 4] >= 0 and m['stats'][0] == 81 and m['stats'][1] == (m['face'] >= 0).sum()
    assert m['face'][0, 0] == -1 and np.isinf(m['depth'][0, 0])               # the corner ray passes the unit sphere at 1.35
    assert tuple(m['rgb'][0, 0]) == (255, 255, 255)
    # seen head-on: the cosine between a face's normal and the direction of a point p of it is (plane distance) / |p| >= 1 - sagitta
    assert m['lambert'].reshape(9, 9)[4, 4] >= 1.0 - sagitta - 1e-9


@pytest.mark.parametrize('tilt', [0.0, 0.5, 1.1])
def test_single_triangle_gives_the_byte_of_the_formula(tilt):
    c, s = math.cos(tilt), math.sin(tilt)
    v = np.array([(-4.0, -4.0 * c, -4.0 * s), (4.0, -4.0 * c, -4.0 * s), (0.0, 4.0 * c, 4.0 * s)], np.float32)       # normal (0, -s, c)
    f = np.array([(0, 1, 2)], np.int32)
    base = (0.8, 0.5, 0.25)
    p = FM.params(width=1, height=1, projection=1, eye=(0.0, 0.0, 9.0), base_rgb=base, ambient=0.55, diffuse=0.45)
    m = FM.render(v, f, p)
    want = [byte_of(b * (0.55 * 1.0 + 0.45 * c)) for b in base]
    assert m['rgb'].shape == (1, 1, 3) and m['rgb'][0, 0].tolist() == want
    assert abs(m['lambert'][0] - c) < 1e-6 and m['ao'][0] == 1.0
    back = FM.render(v, f[:, [0, 2, 1]], p)                                    # the other side: the two-sided headlight sees the same
    assert back['rgb'][0, 0].tolist() == want
    vivid = FM.render(v, f, p, vertex_rgb=np.array([(1, 0, 0), (1, 0, 0), (1, 0, 0)], np.float32))
    assert vivid['rgb'][0, 0].tolist() == [byte_of(0.55 + 0.45 * c), 0, 0]


def test_supersampling_averages_before_the_gamma():
    v, f = FM.sheet(1, 1.0)                                                    # covers x in [-1, 1]: the left half of a 1 x 1 picture of [-1, 3]
    p = FM.params(width=1, height=1, samples=2, projection=1, eye=(1.0, 0.0, 5.0), half_w=2.0, half_h=0.5, base_rgb=(0.25, 0.25, 0.25),
                  background_rgb=(1.0, 1.0, 1.0), ambient=0.5, diffuse=0.5)
    m = FM.render(v, f, p)
    assert (m['face'] >= 0).sum() == 2 and m['rgb'][0, 0].tolist() == [byte_of((0.25 + 0.25 + 1.0 + 1.0) / 4.0)] * 3


def test_plate_over_floor_occludes_the_counted_share():
    gap, plate, bias, radius, K = 0.25, 0.5, 1.0 / 1024.0, 0.75, 64
    v, f = FM.floor_and_plate(gap, plate)
    table = figure.ao_directions(K)
    px = 0.9
    p = FM.params(width=1, height=1, projection=1, eye=(px, 0.0, 5.0), half_w=0.01, half_h=0.01, ao_rays=K, ao_radius=radius, ao_bias=bias)
    m = FM.render(v, f, p, ao_dirs=table)
    assert m['face'][0, 0] >= 0 and abs(m['depth'][0, 0] - 5.0) < 1e-12          # the floor, not the plate
    # by hand: the basis of n = (0, 0, 1) is the world's, so a direction h reaches the plate's plane at t = (gap - bias) / hz
    t = (gap - bias) / np.maximum(table[:, 2], 1e-300)
    x, y = px + t * table[:, 0], t * table[:, 1]
    share = int(((t <= radius) & (np.abs(x) <= plate) & (np.abs(y) <= plate)).sum())
    assert 0 < share < K
    assert m['stats'][2] == K and m['stats'][3] == share and m['ao'][0] == (K - share) / K
    assert m['rgb'][0, 0].tolist() == [byte_of(0.8 * (0.6 * (K - share) / K + 0.4))] * 3
    short = FM.render(v, f, dict(p, ao_radius=gap / 2.0), ao_dirs=table)       # too short to reach the plate
    assert short['stats'][3] == 0 and short['ao'][0] == 1.0


def test_the_walks_count_fewer_tests_than_every_pair():
    v, f = FM.icosphere(3)
    p = FM.params(width=5, height=4, samples=2, ao_rays=3, ao_radius=0.4, tan_half_w=0.3, tan_half_h=0.25)
    m = FM.render(v, f, p, ao_dirs=figure.ao_directions(3))                    # asserts walk == exhaustive for every ray
    rays = m['stats'][0] + m['stats'][2]
    assert 0 < m['stats'][4] < rays * len(f) // 8
    assert np.array_equal(FM.render(v, f, p, ao_dirs=figure.ao_directions(3), count_tests=False)['rgb'], m['rgb'])


def test_normalization_target_and_colour_index():
    a, b = np.array([0.5, 0.1, 0.3]), np.array([0.2, 0.4, 0.9, 0.7, 0.6, 0.8, 1.0])
    both = np.sort(np.concatenate([a, b]))
    assert figure.normalization_target([a, b], 0.9) == both[int(10 * 0.9)] == 1.0
    assert figure.normalization_target([a, b], 0.5) == both[5] and figure.normalization_target([a, b], 0.0) == 0.1
    assert figure.normalization_target([a, b], 1.0) == both[-1] and figure.normalization_target([a], 2.0) == 0.5
    assert figure.normalization_target([a, b], None) == 1.0
    assert figure.normalization_target([], 0.9) == 0.0 and figure.normalization_target([np.zeros(0), np.zeros(0)], 1.0) == 0.0
    target = 0.4
    d = np.array([0.0, 0.1, 0.2, 0.39999, target, 0.5, 40.0, np.inf])
    want = np.minimum((d[:-1] / target * 255).astype(np.int32), 255).tolist() + [255]
    assert figure.distance_indices(d, target).tolist() == want and want[0] == 0 and want[4] == 255 and want[5] == 255
    assert figure.distance_indices(d, target).dtype == np.int32
    cm = figure.colormap()
    assert figure.distance_colors(d, target).tolist() == cm[want].tolist()
    assert figure.distance_indices([0.0, 1e-9], 0.0).tolist() == [0, 255]       # an empty group or all distances 0
    assert figure.distance_colors(np.zeros(0), 1.0).shape == (0, 3)


def test_colour_map_runs_blue_green_yellow():
    cm = figure.colormap()
    assert cm.shape == (256, 3) and cm.dtype == np.uint8
    assert cm[0, 2] > 200 and cm[0, 0] < 40                                    # blue
    assert cm[128, 1] > max(cm[128, 0], cm[128, 2]) + 80                       # green
    assert cm[255, 0] > 230 and cm[255, 1] > 230 and cm[255, 2] < 40           # yellow
    cp = np.asarray(figure.CONTROL_POINTS)
    for k in range(3):                                                         # linear between the control points
        want = np.floor(np.interp(np.arange(256) / 255.0, cp[:, 0], cp[:, 1 + k]) * 255.0 + 0.5)
        assert cm[:, k].tolist() == want.tolist()


decode_png = FM.decode_png          # the 20-line decoder: 8-bit RGB, filter 0 on every row, every CRC checked


@pytest.mark.parametrize('shape', [(1, 1), (11, 13), (40, 9)])
def test_write_png_round_trip_and_same_bytes(tmp_path, shape):
    img = np.random.RandomState(shape[0]).randint(0, 256, shape + (3,)).astype(np.uint8)
    a, b = str(tmp_path / 'a.png'), str(tmp_path / 'b.png')
    figure.write_png(a, img)
    figure.write_png(b, img.copy())
    da, db = open(a, 'rb').read(), open(b, 'rb').read()
    assert da == db == figure.png_bytes(img)
    assert np.array_equal(decode_png(da), img)
    for bad in (img.astype(np.float32), img[:, :, :2], img[0], np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            figure.write_png(a, bad)


@pytest.mark.parametrize('projection', figure.PROJECTIONS)
@pytest.mark.parametrize('view', [(30.0, 20.0, 30.0, 4.0 / 3.0), (0.0, 0.0, 60.0, 1.0), (200.0, -75.0, 20.0, 0.5), (45.0, 90.0, 30.0, 2.0),
                                  (10.0, -90.0, 45.0, 1.0)])
def test_fit_camera_is_orthonormal_and_contains_the_sphere(projection, view):
    az, el, fov, aspect = view
    lo, hi = np.array([-1.0, 0.5, 2.0]), np.array([3.0, 1.5, 2.5])
    cam = figure.fit_camera((lo, hi), az, el, fov, aspect, projection=projection)
    r, u, f = (np.asarray(cam[k]) for k in ('right', 'up', 'forward'))
    for a, b, want in ((r, r, 1), (u, u, 1), (f, f, 1), (r, u, 0), (r, f, 0), (u, f, 0)):
        assert abs(float(a @ b) - want) <= 2.0 ** -40
    assert np.allclose(np.cross(r, u), -f)                                     # right-handed with the camera looking along forward
    centre, radius = (lo + hi) / 2.0, float(np.linalg.norm(hi - lo)) / 2.0
    assert np.allclose(cam['centre'], centre) and abs(cam['radius'] - radius) < 1e-12
    c = centre - np.asarray(cam['eye'])
    assert abs(float(c @ r)) < 1e-9 and abs(float(c @ u)) < 1e-9 and float(c @ f) > radius      # looks at the centre from outside
    if projection == 'pinhole':
        assert abs(cam['tan_half_h'] - math.tan(math.radians(fov) / 2.0)) < 1e-12 and abs(cam['tan_half_w'] - aspect * cam['tan_half_h']) < 1e-12
        for axis, tan in ((r, cam['tan_half_w']), (u, cam['tan_half_h'])):
            for sign in (1.0, -1.0):                                           # the four side planes, normals pointing inward
                n = (tan * f - sign * axis) / math.sqrt(tan * tan + 1.0)
                assert float(n @ c) >= radius
    else:
        assert cam['half_w'] >= radius and cam['half_h'] >= radius and abs(cam['half_w'] - aspect * cam['half_h']) < 1e-12
    with pytest.raises(ValueError):
        figure.fit_camera((lo, hi), projection='fisheye')
    with pytest.raises(ValueError):
        figure.fit_camera((lo, hi), fov=180.0)


def test_ao_directions_are_unit_upper_and_cosine_weighted():
    assert figure.ao_directions(0).shape == (0, 3)
    for K in (1, 5, 16, 64):
        h = figure.ao_directions(K)
        assert h.shape == (K, 3) and h.dtype == np.float64
        assert np.allclose((h * h).sum(1), 1.0, atol=1e-15) and (h[:, 2] >= 0.0).all()
        k = np.arange(K)
        assert np.allclose(np.hypot(h[:, 0], h[:, 1]), np.sqrt((k + 0.5) / K))
        assert np.allclose(np.arctan2(h[:, 1], h[:, 0]), np.angle(np.exp(1j * k * math.pi * (3.0 - math.sqrt(5.0)))))
    assert abs(figure.ao_directions(64)[:, 2].mean() - 2.0 / 3.0) < 0.01       # E[cos] of a cosine-weighted set


def test_the_wrappers_check_before_the_device():
    v, f = FM.cube()
    for kw in (dict(width=0), dict(height=0), dict(samples=0), dict(samples=5), dict(ao_rays=-1), dict(ao_rays=65), dict(shading='phong'),
               dict(width=2.5), dict(samples=True), dict(width=1 << 15, height=1 << 14, samples=1)):
        with pytest.raises(ValueError):
            figure.render((v, f), **kw)
        with pytest.raises(ValueError):
            figure.figure_dirs(['nowhere'], None, 'nowhere', **{k: x for k, x in kw.items()})
    assert 'min 0.0, max 0.0, mean 0.0' in figure.stats_text(np.zeros(0), 0.0, 0.9)
    text = figure.stats_text(np.array([0.25, 0.75]), 0.5, 0.9)
    assert 'min 0.25, max 0.75, mean 0.5' in text and 'normalised to 0.5 (cut 0.9)' in text
    assert figure.linear_albedo(np.array([[255, 0, 51]], np.uint8)).tolist() == [[1.0, 0.0, np.float32(0.04)]]
