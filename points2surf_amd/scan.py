"""Scan meshes into point clouds and draw the GT query points on the device: the stages of the reference's
``make_dataset.py`` that start one BlenSor process per mesh (:242-380, ``04_pts``) and call trimesh
(source/sdf.py:288-315, ``05_query_pts``), through libp2s_hip.so (p2s_mesh_raycast, p2s_mesh_tof_scan,
p2s_mesh_query_points).  Torch tensors are containers only; no CPU fallback.

Unpinned: BlenSor absent.  BlenSor's ray grid and its noise source (Python's ``random.gauss`` inside Blender) cannot be
executed here, so the sensor is the project's own definition: camera at the origin looking along +y, x
right, z up, the object at ``R(q) p + location``, pixel (i, j) looking along
``normalise(((i + 1/2 - W/2) 2 tan(a_w / 2) / W, 1, (j + 1/2 - H/2) 2 tan(a_h / 2) / H))``, noise along the ray.  What IS
restated from the reference is the seeded draw sequence of the poses (make_dataset.py:303-315) and the construction of
the query points.  The one deviation of the query points: the reference's ``mesh.sample`` draws from numpy's unseeded
global generator, so its files are not reproducible even by itself; here every deviate comes from the one
``RandomState(filename_to_hash(mesh_file))`` -- surface samples, then offsets, then far points.

``python -m points2surf_amd.scan --indir DATASET [--stage pts|query_pts|all]`` writes ``04_pts`` (and its companions)
and ``05_query_pts`` from ``03_meshes``; ``python -m points2surf_amd.gt_sdf --indir DATASET`` then writes
``05_query_dist``.
"""
import argparse
import configparser
import ctypes
import hashlib
import math
import os

import numpy as np
import torch

from . import _lib
from . import engine as _engine
from . import gt_sdf as _gt_sdf
from . import ply as _ply
from .file_utils import call_necessary as _call_necessary

METHODS = _gt_sdf.METHODS
# the reference's blensor_script_template.py: a 176 x 144 time-of-flight sensor, 43.6 x 34.6 degrees, max_distance 10
DEFAULT_SENSOR = dict(width=176, height=144, angle_w=43.6, angle_h=34.6, max_distance=10.0)
DEFAULT_SETTINGS = dict(num_scans_per_mesh_min=5, num_scans_per_mesh_max=30, scanner_noise_sigma_min=0.0,
                        scanner_noise_sigma_max=0.05, grid_resolution=256, epsilon=3)


def filename_to_hash(file_path):
    """md5 of the basename before its first dot, mod 2^32 - 1 (the reference's seed of everything per mesh)"""
    stem = os.path.basename(file_path).split('.')[0]
    return int(hashlib.md5(stem.encode()).hexdigest(), 16) % (2 ** 32 - 1)


def random_quaternion(u):
    """uniform random unit quaternion (w, x, y, z) from three uniform deviates (Shoemake, Graphics Gems III, 1992, in
    the arrangement of Gohlke's transformations.py)"""
    r1, r2 = math.sqrt(1.0 - u[0]), math.sqrt(u[0])
    t1, t2 = 2.0 * math.pi * u[1], 2.0 * math.pi * u[2]
    return np.array([math.cos(t2) * r2, math.sin(t1) * r1, math.cos(t1) * r1, math.sin(t2) * r2])


def scan_poses(mesh_file, n_min=5, n_max=30, sigma_min=0.0, sigma_max=0.05, rays_per_scan=176 * 144):
    """The scanner poses of one mesh, a function of the file's basename only: the draw sequence of make_dataset.py:303-315
    from ``RandomState(filename_to_hash(mesh_file))`` -- ``randint`` (number of scans), ``rand`` (sigma), then per scan
    ``rand(3)`` (location) and ``rand(3)`` (quaternion) -- continued with ``standard_normal(S * rays_per_scan)`` for the
    noise (``rays_per_scan=0``: none).  dict: n_scans, sigma, locations [S, 3], rotations [S, 4] (w, x, y, z), noise."""
    rnd = np.random.RandomState(filename_to_hash(mesh_file))
    n_scans = int(rnd.randint(n_min, n_max + 1))
    sigma = float(rnd.rand() * (sigma_max - sigma_min) + sigma_min)
    locations, rotations = np.empty((n_scans, 3)), np.empty((n_scans, 4))
    for s in range(n_scans):
        loc = (rnd.rand(3) * 2.0 - 1.0) * np.array([0.1, 1.0, 0.1])
        loc[1] += 4.0                                     # in front of the camera, along its view direction
        locations[s] = loc
        rotations[s] = random_quaternion(rnd.rand(3))
    noise = rnd.standard_normal(n_scans * int(rays_per_scan))
    return dict(n_scans=n_scans, sigma=sigma, locations=locations, rotations=rotations, noise=noise)


def _sensor(sensor):
    s = dict(DEFAULT_SENSOR)
    s.update(sensor or {})
    return s


def sensor_struct(sensor=None):
    """``p2s_tof_sensor`` of a sensor dict (DEFAULT_SENSOR keys); the two tangents are computed here, on the host"""
    s = _sensor(sensor)
    return _lib.TofSensor(int(s['width']), int(s['height']), math.tan(math.radians(s['angle_w']) / 2.0),
                          math.tan(math.radians(s['angle_h']) / 2.0), float(s['max_distance']))


class TriMesh(_gt_sdf.TriMesh):
    """``gt_sdf.TriMesh`` that also casts rays; keeps its vertices and faces on the device for the surface samples"""

    def __init__(self, verts, faces, device=None):
        if isinstance(verts, np.ndarray):
            verts = torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float32))
        if isinstance(faces, np.ndarray):
            faces = torch.from_numpy(np.ascontiguousarray(faces).astype(np.int32))
        super().__init__(verts, faces, device=device)
        self.verts = verts.to(self.device, torch.float32).contiguous()
        self.faces = faces.to(self.device, torch.int32).contiguous()
        self.ray_tests = 0

    def raycast(self, rays, t_max=float('inf'), method='index'):
        """rays [n, 6] float64 (origin, direction) -> (t [n] float64, face [n] int32) device tensors: the first hit in
        (0, t_max], ties to the smallest face id; a miss is (inf, -1).  ``self.ray_tests`` = ray-triangle tests."""
        if self.handle is None:
            raise RuntimeError('TriMesh is closed')
        if isinstance(rays, np.ndarray):
            rays = torch.from_numpy(np.ascontiguousarray(rays, dtype=np.float64))
        r = rays.to(self.device, torch.float64).contiguous()
        if r.ndim != 2 or r.shape[1] != 6:
            raise ValueError('rays must be [n, 6] (got %s)' % (tuple(r.shape),))
        n = int(r.shape[0])
        t = torch.empty((n,), dtype=torch.float64, device=self.device)
        face = torch.empty((n,), dtype=torch.int32, device=self.device)
        tests = ctypes.c_int64(0)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.p2s_mesh_raycast(self.handle, _engine._ptr(r), n, float(t_max), METHODS[method], _engine._ptr(t),
                                                 _engine._ptr(face), ctypes.byref(tests), _engine._stream_ptr(self.device)))
        self.ray_tests = int(tests.value)
        return t, face


def load_mesh(path, device=None):
    v, f = _ply.read_ply(path)
    return TriMesh(np.asarray(v, dtype=np.float32), np.asarray(f), device=device)


def tof_scan(mesh, poses, sensor=None, method='index'):
    """Scan ``mesh`` from the poses of ``scan_poses`` (keys locations, rotations, sigma, noise).  dict of device tensors
    points / points_noisefree / normals [N, 3] float64 and face [N] int32 in the order (scan, row, column), plus
    hits_per_scan (numpy int32 [S]) and tests (ray-triangle tests)."""
    if mesh.handle is None:
        raise RuntimeError('TriMesh is closed')
    st = sensor_struct(sensor)
    loc = np.asarray(poses['locations'], np.float64).reshape(-1, 3)
    rot = np.asarray(poses['rotations'], np.float64).reshape(-1, 4)
    if len(loc) != len(rot):
        raise ValueError('%d locations, %d rotations' % (len(loc), len(rot)))
    S, n = len(loc), len(loc) * st.width * st.height
    noise = poses['noise']
    if isinstance(noise, np.ndarray):
        noise = torch.from_numpy(np.ascontiguousarray(noise, dtype=np.float64))
    noise = noise.to(mesh.device, torch.float64).contiguous().reshape(-1)
    if noise.shape[0] != n:
        raise ValueError('noise must hold one deviate per ray: %d, got %d' % (n, noise.shape[0]))
    pose = np.ascontiguousarray(np.concatenate([loc, rot], axis=1))
    dev = mesh.device
    noisy = torch.empty((n, 3), dtype=torch.float64, device=dev)
    clean = torch.empty((n, 3), dtype=torch.float64, device=dev)
    normal = torch.empty((n, 3), dtype=torch.float64, device=dev)
    face = torch.empty((n,), dtype=torch.int32, device=dev)
    hits = np.zeros((S,), np.int32)
    n_hits, tests = ctypes.c_int64(0), ctypes.c_int64(0)
    with torch.cuda.device(dev):
        _lib.check(mesh.lib.p2s_mesh_tof_scan(mesh.handle, pose.ctypes.data_as(ctypes.c_void_p), S, ctypes.byref(st),
                                              float(poses['sigma']), _engine._ptr(noise), METHODS[method], _engine._ptr(noisy),
                                              _engine._ptr(clean), _engine._ptr(face), _engine._ptr(normal),
                                              hits.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n_hits), ctypes.byref(tests),
                                              _engine._stream_ptr(dev)))
    N = int(n_hits.value)
    return dict(points=noisy[:N], points_noisefree=clean[:N], normals=normal[:N], face=face[:N], hits_per_scan=hits,
                tests=int(tests.value))


def query_points(mesh, seed, num_query_pts=2000, patch_radius=4.0 / 256, far_ratio=0.1, want_parts=False):
    """get_query_pts_for_mesh (source/sdf.py:288-315): float32 device tensor [num, 3] -- ``int(num * far_ratio)`` uniform
    points of [-0.5, 0.5)^3, then area-weighted surface samples moved along their face normal by
    ``(u - 0.5) * 2 * patch_radius``.  All deviates from ``RandomState(seed)``: samples, offsets, far points."""
    from . import metrics as _metrics
    n_far = int(num_query_pts * far_ratio)
    n_close = num_query_pts - n_far
    dev = mesh.device
    rng = _engine.Rng(seed, device=dev)
    lib = mesh.lib
    u = torch.empty((n_close + 3 * n_far,), dtype=torch.float64, device=dev)
    out = torch.empty((num_query_pts, 3), dtype=torch.float32, device=dev)
    try:
        samples, _, fid = _metrics.sample_surface(mesh.verts, mesh.faces, n_close, rng, want_faces=True)
        with torch.cuda.device(dev):
            s = _engine._stream_ptr(dev)
            _lib.check(lib.p2s_rng_random_sample(rng.handle, n_close + 3 * n_far, _engine._ptr(u), s))
            _lib.check(lib.p2s_mesh_query_points(mesh.handle, _engine._ptr(samples), _engine._ptr(fid), _engine._ptr(u),
                                                 ctypes.c_void_p(u.data_ptr() + 8 * n_close), n_close, n_far,
                                                 float(patch_radius), _engine._ptr(out), s))
        torch.cuda.synchronize(dev)
    finally:
        rng.close()
    return (out, samples, fid) if want_parts else out


def _refuse_open(mesh, f_mesh):
    if not mesh.closed:
        raise ValueError('%s is not closed (%d open or non-manifold edges): no data set from it'
                         % (f_mesh, mesh.info()['bad_edges']))


def _mesh_files(indir):
    mesh_dir = os.path.join(indir, '03_meshes')
    return [(n, os.path.join(mesh_dir, n)) for n in sorted(os.listdir(mesh_dir))
            if n.endswith('.ply') and os.path.isfile(os.path.join(mesh_dir, n))]


def write_pts_dir(indir, n_min=5, n_max=30, sigma_min=0.0, sigma_max=0.05, sensor=None, device=None):
    """For every ``indir/03_meshes/<stem>.ply``: 04_pts/<stem>.xyz.npy (noisy points, float32 [N, 3]),
    04_pts_noisefree/<stem>.xyz.npy, 06_normals/pts/<stem>.xyz.npy (the hit faces' normals), 04_locations/<stem>.npz,
    04_rotations/<stem>.npz and 04_hits_per_scan/<stem>.xyz.npz with the reference's keys; up-to-date files are skipped.
    Returns the list of 04_pts files written."""
    s = _sensor(sensor)
    written = []
    for name, f_mesh in _mesh_files(indir):
        stem = name[:-4]
        outs = dict(pts=os.path.join(indir, '04_pts', stem + '.xyz.npy'),
                    clean=os.path.join(indir, '04_pts_noisefree', stem + '.xyz.npy'),
                    normals=os.path.join(indir, '06_normals', 'pts', stem + '.xyz.npy'),
                    loc=os.path.join(indir, '04_locations', stem + '.npz'),
                    rot=os.path.join(indir, '04_rotations', stem + '.npz'),
                    hits=os.path.join(indir, '04_hits_per_scan', stem + '.xyz.npz'))
        if not _call_necessary([f_mesh], list(outs.values())):
            continue
        mesh = load_mesh(f_mesh, device=device)
        try:
            _refuse_open(mesh, f_mesh)
            poses = scan_poses(f_mesh, n_min, n_max, sigma_min, sigma_max, rays_per_scan=int(s['width']) * int(s['height']))
            res = tof_scan(mesh, poses, sensor=s)
            if res['points'].shape[0] == 0:
                print('WARNING: no scanner hits for {} in {} scans'.format(name, poses['n_scans']))
            for f in outs.values():
                os.makedirs(os.path.dirname(f), exist_ok=True)
            np.savez_compressed(outs['loc'], locations=poses['locations'])
            np.savez_compressed(outs['rot'], rotations=poses['rotations'])
            np.savez_compressed(outs['hits'], hits_per_scan=res['hits_per_scan'])
            np.save(outs['clean'], res['points_noisefree'].to(torch.float32).cpu().numpy())
            np.save(outs['normals'], res['normals'].to(torch.float32).cpu().numpy())
            np.save(outs['pts'], res['points'].to(torch.float32).cpu().numpy())
        finally:
            mesh.close()
        written.append(outs['pts'])
    return written


def write_query_pts_dir(indir, patch_radius, num_query_pts=2000, device=None):
    """``indir/05_query_pts/<mesh>.npy`` (float32 [num_query_pts, 3]) for every ``indir/03_meshes/<mesh>``; up-to-date
    files are skipped.  Returns the list of files written."""
    written = []
    for name, f_mesh in _mesh_files(indir):
        f_out = os.path.join(indir, '05_query_pts', name + '.npy')
        if not _call_necessary([f_mesh], [f_out]):
            continue
        mesh = load_mesh(f_mesh, device=device)
        try:
            _refuse_open(mesh, f_mesh)
            q = query_points(mesh, filename_to_hash(f_mesh), num_query_pts, patch_radius)
            os.makedirs(os.path.dirname(f_out), exist_ok=True)
            np.save(f_out, q.cpu().numpy())
        finally:
            mesh.close()
        written.append(f_out)
    return written


def read_settings(indir):
    """the [general] values of ``indir/settings.ini`` this module uses, over DEFAULT_SETTINGS (the file may be absent)"""
    out = dict(DEFAULT_SETTINGS)
    cfg = configparser.ConfigParser()
    f = os.path.join(indir, 'settings.ini')
    if os.path.isfile(f):
        cfg.read(f)
        if cfg.has_section('general'):
            g = cfg['general']
            for key, default in DEFAULT_SETTINGS.items():
                if key in g:
                    out[key] = type(default)(g[key])
            if 'scanner_noise_sigma' in g:                # the single-value form of the reference's own error message
                for key in ('scanner_noise_sigma_min', 'scanner_noise_sigma_max'):
                    if key not in g:
                        out[key] = float(g['scanner_noise_sigma'])
    out['patch_radius'] = (1.0 + out['epsilon']) / out['grid_resolution']
    return out


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='write DATASET/04_pts (scan) and DATASET/05_query_pts from 03_meshes')
    ap.add_argument('--indir', required=True)
    ap.add_argument('--stage', choices=('pts', 'query_pts', 'all'), default='all')
    ap.add_argument('--num_query_pts', type=int, default=2000)
    return ap.parse_args(argv)


def main(argv=None):
    opt = parse_args(argv)
    cfg = read_settings(opt.indir)
    files = []
    if opt.stage in ('pts', 'all'):
        files += write_pts_dir(opt.indir, cfg['num_scans_per_mesh_min'], cfg['num_scans_per_mesh_max'],
                               cfg['scanner_noise_sigma_min'], cfg['scanner_noise_sigma_max'])
    if opt.stage in ('query_pts', 'all'):
        files += write_query_pts_dir(opt.indir, cfg['patch_radius'], opt.num_query_pts)
    for f in files:
        print(f)


if __name__ == '__main__':
    main()
