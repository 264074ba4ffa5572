"""Pictures of meshes, rendered on the device: what the reference's ``source/figure/distance_vis.py`` prepares
for an external viewer -- every vertex of a reconstruction coloured by its distance to the GT surface, all methods of one
shape normalised to a common percentile -- and the picture itself: ``render`` casts the camera's rays over the octree of a
``TriMesh`` (p2s_mesh_render in libp2s_hip.so; the definition is in include/p2s_hip.h), shades the hits with a two-sided
headlight and an ambient-occlusion term, and returns 8-bit RGB.  Torch tensors are containers only; no CPU fallback.  The
colour map is the project's own (piecewise linear through CONTROL_POINTS: 0 blue, 1/2 green, 1 yellow), ``write_png`` needs
``zlib`` and ``struct`` only.

The defaults (16 occlusion rays, ao_radius 5 % of the bounding sphere's diameter, ao_bias 2^-10 of its radius, ambient 0.6,
diffuse 0.4, a 30 degree lens, azimuth 30, elevation 20, y up) are choices.  Nobody has tuned them.  One headlight, no shadow
but the occlusion term, no texture, no transparency, a regular sample grid, one picture per mesh (no contact sheet).

``python -m points2surf_amd.figure --rec DIR [DIR ...] [--gt DIR] --outdir OUT [--cut 0.9] [--azimuth 30 --elevation 20]
[--width 1024 --height 768] [--samples 2] [--ao_rays 16] [--shading flat|smooth] [--dataset FILE] [--gpu_idx I]``
pairs the meshes of every ``--rec`` directory with those of ``--gt`` by the rules of ``metrics`` (same name up to the first
dot, the first in sorted order; with ``--dataset`` only the shapes it names, without it every GT mesh).  The reconstructions
of one GT mesh form a group: one normalisation target (``normalization_target`` over all their vertex distances) and one
camera, fitted to the GT mesh, so the pictures can be put side by side.  Per reconstruction:
``OUT/<rec dir name>/<name>_vis.ply`` (vertex colours), ``<name>.png`` (rendered with those colours) and ``<name>_stats.txt``;
per GT mesh ``OUT/gt/<name>.png`` (plain); ``OUT/figure_report.csv`` with one row per picture.  Without ``--gt`` the meshes of
``--rec`` are rendered plainly, each with its own camera.
"""
import argparse
import csv
import ctypes
import math
import os
import struct
import sys
import zlib

import numpy as np

from . import _lib

PROJECTIONS = ('pinhole', 'orthographic')
SHADINGS = ('flat', 'smooth')
MAX_SAMPLES, MAX_AO_RAYS, MAX_SAMPLE_COUNT = 4, 64, 1 << 28
# the colour map: (position, red, green, blue), linear in between
CONTROL_POINTS = ((0.0, 0.05, 0.20, 0.85), (0.25, 0.00, 0.55, 0.85), (0.5, 0.10, 0.75, 0.35), (0.75, 0.70, 0.80, 0.15),
                  (1.0, 0.98, 0.95, 0.10))
REPORT_FILE = 'figure_report.csv'
REPORT_COLUMNS = ('picture', 'mesh', 'source', 'verts', 'faces', 'min_distance', 'max_distance', 'mean_distance', 'target', 'cut',
                  'width', 'height', 'samples', 'ao_rays', 'shading', 'primary_hits', 'occluded_share', 'verdict')
STATS_KEYS = ('primary_rays', 'primary_hits', 'ao_rays', 'ao_occluded', 'tests', 'stack_overflows')


def colormap():
    """uint8 [256, 3]: entry i is the map at i / 255"""
    x = np.arange(256, dtype=np.float64) / 255.0
    cp = np.asarray(CONTROL_POINTS, np.float64)
    rgb = np.stack([np.interp(x, cp[:, 0], cp[:, 1 + k]) for k in range(3)], 1)
    return np.floor(rgb * 255.0 + 0.5).astype(np.uint8)


def normalization_target(list_of_distance_arrays, cut=0.9):
    """the reference's rule (distance_vis.get_normalization_target): all distances of a group concatenated and sorted; the
    element at index int(n * cut) when cut < 1, else the last.  An empty group has the target 0.0 (the reference fails)."""
    parts = [np.asarray(d, np.float64).reshape(-1) for d in list_of_distance_arrays]
    d = np.sort(np.concatenate(parts)) if parts else np.zeros(0)
    if len(d) == 0:
        return 0.0
    if cut is not None and cut < 1.0:
        return float(d[int(len(d) * cut)])
    return float(d[-1])


def distance_indices(d, target):
    """int32 [n]: int32(d / target * 255) clamped to 0 .. 255 (a distance that is not finite: 255).  A target that is not
    positive (all distances 0, or an empty group) maps 0 to 0 and everything else to 255."""
    d = np.asarray(d, np.float64).reshape(-1)
    if not target > 0.0:
        return np.where(d > 0.0, 255, 0).astype(np.int32)
    with np.errstate(all='ignore'):
        x = d / target * 255.0
    x = np.where(np.isfinite(x), np.minimum(np.maximum(x, 0.0), 255.0), 255.0)
    return x.astype(np.int32)


def distance_colors(d, target):
    """uint8 [n, 3]: the colour of every distance, 0 blue, target / 2 green, target and beyond yellow"""
    return colormap()[distance_indices(d, target)]


def _as_mesh(mesh, device=None):
    """a ``scan.TriMesh`` of ``mesh``: one as it is, or built from (verts, faces); (mesh, built here)"""
    from . import scan as _scan
    if isinstance(mesh, (tuple, list)):
        return _scan.TriMesh(np.asarray(mesh[0], np.float32), np.asarray(mesh[1]), device=device), True
    return mesh, False


def vertex_distances(rec_mesh, gt_mesh):
    """float64 numpy [V]: the unsigned exact distance of every vertex of the reconstruction to the GT surface
    (``TriMesh.distance(signed=False)``).  ``rec_mesh``: (verts, faces), a [V, 3] array, or a mesh with ``.verts``;
    ``gt_mesh``: a TriMesh or (verts, faces)."""
    import torch
    gt, own = _as_mesh(gt_mesh)
    try:
        v = rec_mesh[0] if isinstance(rec_mesh, (tuple, list)) else getattr(rec_mesh, 'verts', rec_mesh)
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        v = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
        if len(v) == 0:
            return np.zeros(0)
        return gt.distance(v, signed=False).cpu().numpy()
    finally:
        if own:
            gt.close()


def ao_directions(count):
    """float64 [count, 3]: a cosine-weighted set of unit directions of the hemisphere z >= 0 in closed form -- direction k
    has the radius sqrt((k + 1/2) / count) in the disc and the azimuth k times the golden angle"""
    k = np.arange(int(count), dtype=np.float64)
    r = np.sqrt((k + 0.5) / max(int(count), 1))
    phi = k * (math.pi * (3.0 - math.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(np.maximum(0.0, 1.0 - r * r))], 1).reshape(-1, 3)


def _unit(v):
    return v / math.sqrt(float(v @ v))


def fit_camera(bounds, azimuth=30.0, elevation=20.0, fov=30.0, aspect=4.0 / 3.0, projection='pinhole', margin=1.05):
    """A camera that sees the whole bounding sphere of ``bounds`` = (lo [3], hi [3]): a dict with projection, eye and the
    orthonormal frame right / up / forward, tan_half_w / tan_half_h (pinhole) and half_w / half_h (orthographic).  The
    camera looks at the centre from ``azimuth`` (degrees around +y, 0 = from +z) and ``elevation`` (degrees above the
    x-z plane); ``fov`` is the vertical opening angle of the pinhole; ``aspect`` = width / height; ``margin`` > 1 leaves
    a rim around the sphere."""
    if projection not in PROJECTIONS:
        raise ValueError('projection must be one of %s (got %r)' % (', '.join(PROJECTIONS), projection))
    lo, hi = np.asarray(bounds[0], np.float64).reshape(3), np.asarray(bounds[1], np.float64).reshape(3)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and 0.0 < fov < 180.0 and aspect > 0.0 and margin >= 1.0):
        raise ValueError('fit_camera: finite bounds, 0 < fov < 180, aspect > 0 and margin >= 1 are needed')
    centre = (lo + hi) / 2.0
    radius = max(math.sqrt(float((hi - lo) @ (hi - lo))) / 2.0, 1e-12)
    az, el = math.radians(azimuth), math.radians(elevation)
    back = np.array([math.cos(el) * math.sin(az), math.sin(el), math.cos(el) * math.cos(az)])
    forward = _unit(-back)
    world_up = np.array([0.0, 1.0, 0.0]) if abs(forward[1]) < 0.999 else np.array([0.0, 0.0, -1.0])
    right = _unit(np.cross(forward, world_up))
    up = _unit(np.cross(right, forward))
    right = _unit(np.cross(forward, up))
    th = math.tan(math.radians(fov) / 2.0)
    tw = th * aspect
    distance = radius * margin / math.sin(math.atan(min(th, tw)))
    half_h = radius * margin * (1.0 if aspect >= 1.0 else 1.0 / aspect)
    return dict(projection=projection, eye=centre - distance * forward, right=right, up=up, forward=forward, tan_half_w=tw,
                tan_half_h=th, half_w=half_h * aspect, half_h=half_h, centre=centre, radius=radius)


def mesh_bounds(mesh):
    """(lo [3], hi [3]) float64 of the vertices of a ``scan.TriMesh``"""
    v = getattr(mesh, 'verts', None)
    if v is None or v.shape[0] == 0:
        raise ValueError('the bounds need a mesh that keeps its vertices (scan.TriMesh); pass camera, ao_radius and ao_bias instead')
    return v.min(0).values.double().cpu().numpy(), v.max(0).values.double().cpu().numpy()


def _check_render(width, height, samples, ao_rays, shading):
    for name, x, lo, hi in (('width', width, 1, MAX_SAMPLE_COUNT), ('height', height, 1, MAX_SAMPLE_COUNT), ('samples', samples, 1, MAX_SAMPLES),
                            ('ao_rays', ao_rays, 0, MAX_AO_RAYS)):
        if isinstance(x, bool) or int(x) != x or not lo <= int(x) <= hi:
            raise ValueError('%s must be an integer in %d .. %d (got %r)' % (name, lo, hi, x))
    if int(width) * int(height) * int(samples) ** 2 > MAX_SAMPLE_COUNT:
        raise ValueError('width * height * samples^2 must be at most 2^28')
    if shading not in SHADINGS:
        raise ValueError('shading must be one of %s (got %r)' % (', '.join(SHADINGS), shading))


def render_params(camera, width, height, samples, ao_rays, shading, ao_radius, ao_bias, ambient, diffuse, base_rgb, background_rgb):
    """the ``_lib.RenderParams`` of a camera dict (``fit_camera``) and the settings"""
    p = _lib.RenderParams()
    p.width, p.height, p.samples, p.ao_rays = int(width), int(height), int(samples), int(ao_rays)
    p.projection, p.shading = PROJECTIONS.index(camera['projection']), SHADINGS.index(shading)
    for name in ('eye', 'right', 'up', 'forward'):
        setattr(p, name, (ctypes.c_double * 3)(*[float(x) for x in np.asarray(camera[name], np.float64).reshape(3)]))
    for name in ('tan_half_w', 'tan_half_h', 'half_w', 'half_h'):
        setattr(p, name, float(camera.get(name, 0.0)))
    p.ao_radius, p.ao_bias, p.ambient, p.diffuse = float(ao_radius), float(ao_bias), float(ambient), float(diffuse)
    p.base_rgb = (ctypes.c_double * 3)(*[float(x) for x in base_rgb])
    p.background_rgb = (ctypes.c_double * 3)(*[float(x) for x in background_rgb])
    return p


def render(mesh, vertex_rgb=None, camera=None, width=1024, height=768, samples=2, ao_rays=16, shading='flat', azimuth=30.0,
           elevation=20.0, fov=30.0, projection='pinhole', ao_radius=None, ao_bias=None, ambient=0.6, diffuse=0.4,
           base_rgb=(0.8, 0.8, 0.8), background_rgb=(1.0, 1.0, 1.0), ao_dirs=None, want_depth=False, want_face=False, want_stats=False):
    """``mesh`` (a ``scan.TriMesh``, or (verts, faces)) -> uint8 numpy [height, width, 3]; with ``want_depth`` / ``want_face``
    also the first hit of every sample, float64 t and int32 face id [height * samples, width * samples] (a miss: inf, -1),
    with ``want_stats`` a dict (STATS_KEYS).  ``vertex_rgb`` [V, 3]: linear albedo per vertex in [0, 1] (the picture is
    encoded with gamma 2), else ``base_rgb``.  ``camera``: a dict as ``fit_camera`` returns; None fits one to the mesh's
    bounding sphere from ``azimuth``, ``elevation``, ``fov`` and ``projection``.  ``ao_radius`` / ``ao_bias`` None: 5 % of
    the bounding sphere's diameter / 2^-10 of its radius.  ``ao_dirs`` [ao_rays, 3]: the table of ``ao_directions`` unless
    given."""
    import torch
    from . import engine as _engine
    _check_render(width, height, samples, ao_rays, shading)
    mesh, own = _as_mesh(mesh)
    try:
        if mesh.handle is None:
            raise RuntimeError('TriMesh is closed')
        dev = mesh.device
        if camera is None or ao_radius is None or ao_bias is None:
            lo, hi = mesh_bounds(mesh)
            radius = max(math.sqrt(float((hi - lo) @ (hi - lo))) / 2.0, 1e-12)
            if camera is None:
                camera = fit_camera((lo, hi), azimuth, elevation, fov, float(width) / float(height), projection)
            ao_radius = 0.1 * radius if ao_radius is None else ao_radius
            ao_bias = radius / 1024.0 if ao_bias is None else ao_bias
        prm = render_params(camera, width, height, samples, ao_rays, shading, ao_radius, ao_bias, ambient, diffuse, base_rgb, background_rgb)
        W, H, ss, K = int(width), int(height), int(samples), int(ao_rays)
        rgb_in = None
        if vertex_rgb is not None:
            c = vertex_rgb.detach() if isinstance(vertex_rgb, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(vertex_rgb, np.float32))
            rgb_in = c.to(dev, torch.float32).contiguous()
            if rgb_in.ndim != 2 or tuple(rgb_in.shape) != (mesh.n_verts, 3):
                raise ValueError('vertex_rgb must be [%d, 3] (got %s)' % (mesh.n_verts, tuple(rgb_in.shape)))
        table = None
        if K > 0:
            t = ao_directions(K) if ao_dirs is None else np.ascontiguousarray(ao_dirs, np.float64)
            if t.shape != (K, 3):
                raise ValueError('ao_dirs must be [%d, 3] (got %s)' % (K, t.shape))
            table = torch.from_numpy(t).to(dev)
        st = (ctypes.c_int64 * 8)()
        with torch.cuda.device(dev):
            rgb = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
            depth = torch.empty((H * ss, W * ss), dtype=torch.float64, device=dev) if want_depth else None
            face = torch.empty((H * ss, W * ss), dtype=torch.int32, device=dev) if want_face else None
            _lib.check(mesh.lib.p2s_mesh_render(mesh.handle, ctypes.byref(prm), _engine._ptr(rgb_in), _engine._ptr(table), _engine._ptr(rgb),
                                                _engine._ptr(depth), _engine._ptr(face), st, _engine._stream_ptr(dev)))
        out = (rgb.cpu().numpy(),) + ((depth.cpu().numpy(),) if want_depth else ()) + ((face.cpu().numpy(),) if want_face else ()) + \
            ((dict(zip(STATS_KEYS, (int(x) for x in st))),) if want_stats else ())
        return out[0] if len(out) == 1 else out
    finally:
        if own:
            mesh.close()


def _chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xffffffff)


def png_bytes(rgb):
    """the PNG file of uint8 [H, W, 3]: 8-bit RGB, no filter, one IDAT chunk at zlib level 9; the same image gives the same
    bytes"""
    a = np.asarray(rgb)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError('write_png takes uint8 [H, W, 3] with H, W >= 1 (got %s %s)' % (a.dtype, a.shape))
    h, w = a.shape[:2]
    raw = np.concatenate([np.zeros((h, 1), np.uint8), np.ascontiguousarray(a).reshape(h, w * 3)], 1).tobytes()
    return b'\x89PNG\r\n\x1a\n' + _chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0)) + \
        _chunk(b'IDAT', zlib.compress(raw, 9)) + _chunk(b'IEND', b'')


def write_png(path, rgb):
    data = png_bytes(rgb)
    with open(path, 'wb') as fh:
        fh.write(data)


def linear_albedo(colors_u8):
    """float32 [n, 3]: (c / 255)^2 -- the albedo that a fully lit surface shows as the colour c after the gamma-2 encoding"""
    c = np.asarray(colors_u8, np.float64) / 255.0
    return (c * c).astype(np.float32)


def stats_text(d, target, cut):
    d = np.asarray(d, np.float64)
    lo, hi, mean = (float(d.min()), float(d.max()), float(d.mean())) if len(d) else (0.0, 0.0, 0.0)
    return ('unsigned distance of the vertices of the reconstruction to the GT surface: min %r, max %r, mean %r; '
            'colours normalised to %r (cut %r)\n' % (lo, hi, mean, float(target), cut))


def _stem(name):
    return os.path.basename(name).split('.')[0]


def _load(path, device):
    from . import mesh_formats as _formats
    from . import scan as _scan
    v, f = _formats.read_mesh(path)
    v, f = np.ascontiguousarray(v, np.float32).reshape(-1, 3), np.ascontiguousarray(f).astype(np.int32).reshape(-1, 3)
    return _scan.TriMesh(v, f, device=device), v, f


def _groups(rec_dirs, labels, gt_dir, dataset):
    """GT file -> [(label, reconstruction file)]: the pairing of ``metrics`` -- two files belong together when their names agree
    up to the first dot, the first in sorted order wins, and a data set file (one shape name per line) restricts the GT meshes
    to its shapes.  Without a data set file every GT mesh counts (``metrics`` keeps the reference's rule there, which needs
    GT files without an extension)."""
    from .simplify import _names
    wanted = None
    if dataset:
        if not os.path.isfile(dataset):
            raise ValueError('File does not exist: {}'.format(dataset))
        with open(dataset) as fh:
            wanted = set((line.replace('\n', '') + '.ply').split('.')[0] for line in fh.readlines())
    groups = {}
    refs = {}
    for name in _names(gt_dir, None):
        if wanted is None or _stem(name) in wanted:
            refs.setdefault(_stem(name), os.path.join(gt_dir, name))
    for rec_dir, label in zip(rec_dirs, labels):
        taken = set()
        for name in _names(rec_dir, None):
            if _stem(name) in refs and _stem(name) not in taken:
                taken.add(_stem(name))
                groups.setdefault(refs[_stem(name)], []).append((label, os.path.join(rec_dir, name)))
    return groups


def _row(picture, path, source, v, f, d, target, cut, opt, stats, verdict='rendered'):
    has = d is not None and len(d) > 0
    return dict(picture=picture, mesh=os.path.basename(path), source=source, verts=len(v), faces=len(f),
                min_distance=repr(float(d.min())) if has else '', max_distance=repr(float(d.max())) if has else '',
                mean_distance=repr(float(d.mean())) if has else '', target=repr(float(target)) if d is not None else '',
                cut=repr(cut) if d is not None else '', width=opt['width'], height=opt['height'], samples=opt['samples'],
                ao_rays=opt['ao_rays'], shading=opt['shading'], primary_hits=stats['primary_hits'] if stats else '',
                occluded_share=repr(stats['ao_occluded'] / stats['ao_rays']) if stats and stats['ao_rays'] else '', verdict=verdict)


def _failed(picture, path, source, opt, e):
    row = dict.fromkeys(REPORT_COLUMNS, '')
    row.update(picture=picture, mesh=os.path.basename(path), source=source, width=opt['width'], height=opt['height'], samples=opt['samples'],
               ao_rays=opt['ao_rays'], shading=opt['shading'], verdict='failed: %s' % ' '.join(str(e).split()))
    return row


def figure_dirs(rec_dirs, gt_dir, outdir, cut=0.9, azimuth=30.0, elevation=20.0, width=1024, height=768, samples=2, ao_rays=16,
                shading='flat', dataset=None, device=None):
    """the command line as a function; returns the rows of figure_report.csv (dicts of REPORT_COLUMNS).  A mesh that fails
    is named in the report with the reason; the run goes on."""
    from . import ply as _ply
    from .simplify import _names
    _check_render(width, height, samples, ao_rays, shading)
    opt = dict(width=int(width), height=int(height), samples=int(samples), ao_rays=int(ao_rays), shading=shading)
    view = dict(azimuth=azimuth, elevation=elevation)
    labels = [os.path.basename(os.path.normpath(d)) for d in rec_dirs]
    if len(set(labels)) != len(labels) or 'gt' in labels and gt_dir:
        raise ValueError('the --rec directories need distinct names, none of them "gt" (got %s)' % ', '.join(labels))
    os.makedirs(outdir, exist_ok=True)
    rows = []
    if not gt_dir:
        for rec_dir, label in zip(rec_dirs, labels):
            os.makedirs(os.path.join(outdir, label), exist_ok=True)
            for name in _names(rec_dir, dataset):
                path, pic = os.path.join(rec_dir, name), os.path.join(label, _stem(name) + '.png')
                try:
                    mesh, v, f = _load(path, device)
                    try:
                        rgb, st = render(mesh, want_stats=True, **opt, **view)
                    finally:
                        mesh.close()
                    write_png(os.path.join(outdir, pic), rgb)
                    rows.append(_row(pic, path, label, v, f, None, 0.0, cut, opt, st))
                except Exception as e:
                    rows.append(_failed(pic, path, label, opt, e))
    else:
        groups = _groups(rec_dirs, labels, gt_dir, dataset)
        if not groups:
            raise ValueError('no reconstruction of %s has a GT mesh of the same name in %s' % (', '.join(rec_dirs), gt_dir))
        os.makedirs(os.path.join(outdir, 'gt'), exist_ok=True)
        for ref in sorted(groups):
            pic = os.path.join('gt', _stem(ref) + '.png')
            try:
                gt, gv, gf = _load(ref, device)
            except Exception as e:
                rows.append(_failed(pic, ref, 'gt', opt, e))
                continue
            try:
                camera = fit_camera(mesh_bounds(gt), aspect=float(width) / float(height), **view)
                ao = dict(ao_radius=0.1 * camera['radius'], ao_bias=camera['radius'] / 1024.0)
                rgb, st = render(gt, camera=camera, want_stats=True, **opt, **ao)
                write_png(os.path.join(outdir, pic), rgb)
                rows.append(_row(pic, ref, 'gt', gv, gf, None, 0.0, cut, opt, st))
                members = []
                for label, new in groups[ref]:
                    try:
                        mesh, v, f = _load(new, device)
                        members.append((label, new, mesh, v, f, vertex_distances(v, gt)))
                    except Exception as e:
                        rows.append(_failed(os.path.join(label, _stem(new) + '.png'), new, label, opt, e))
                target = normalization_target([m[5] for m in members], cut)
                for label, new, mesh, v, f, d in members:
                    base = os.path.join(label, _stem(new))
                    try:
                        os.makedirs(os.path.join(outdir, label), exist_ok=True)
                        colors = distance_colors(d, target)
                        rgba = np.concatenate([colors, np.full((len(colors), 1), 255, np.uint8)], 1)
                        _ply.write_ply(os.path.join(outdir, base + '_vis.ply'), v, f, vertex_colors=rgba)
                        with open(os.path.join(outdir, base + '_stats.txt'), 'w') as fh:
                            fh.write(stats_text(d, target, cut))
                        rgb, st = render(mesh, vertex_rgb=linear_albedo(colors), camera=camera, want_stats=True, **opt, **ao)
                        write_png(os.path.join(outdir, base + '.png'), rgb)
                        rows.append(_row(base + '.png', new, label, v, f, d, target, cut, opt, st))
                    except Exception as e:
                        rows.append(_failed(base + '.png', new, label, opt, e))
                    finally:
                        mesh.close()
            except Exception as e:
                rows.append(_failed(pic, ref, 'gt', opt, e))
            finally:
                gt.close()
    with open(os.path.join(outdir, REPORT_FILE), 'w', newline='') as fh:
        w = csv.DictWriter(fh, fieldnames=REPORT_COLUMNS)
        w.writeheader()
        w.writerows(rows)
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m points2surf_amd.figure',
                                 description='render the meshes of the --rec directories, coloured by their distance to the --gt meshes')
    ap.add_argument('--rec', nargs='+', required=True, help='directories of reconstructions (one per method)')
    ap.add_argument('--gt', default=None, help='directory of GT meshes; without it the reconstructions are rendered plainly')
    ap.add_argument('--outdir', required=True)
    ap.add_argument('--cut', type=float, default=0.9, help='the share of all distances of a group that the colour map spans')
    ap.add_argument('--azimuth', type=float, default=30.0)
    ap.add_argument('--elevation', type=float, default=20.0)
    ap.add_argument('--width', type=int, default=1024)
    ap.add_argument('--height', type=int, default=768)
    ap.add_argument('--samples', type=int, default=2, help='samples per pixel and axis (1 .. 4)')
    ap.add_argument('--ao_rays', type=int, default=16, help='occlusion rays per sample (0 .. 64)')
    ap.add_argument('--shading', choices=SHADINGS, default='flat')
    ap.add_argument('--dataset', default=None, help='a list of shape names: only these meshes')
    ap.add_argument('--gpu_idx', type=int, default=0)
    opt = ap.parse_args(argv)
    try:
        _check_render(opt.width, opt.height, opt.samples, opt.ao_rays, opt.shading)
    except ValueError as e:
        ap.error(str(e))
    from . import engine as _engine
    device = _engine.select_device(opt.gpu_idx)
    rows = figure_dirs(opt.rec, opt.gt, opt.outdir, cut=opt.cut, azimuth=opt.azimuth, elevation=opt.elevation, width=opt.width,
                       height=opt.height, samples=opt.samples, ao_rays=opt.ao_rays, shading=opt.shading, dataset=opt.dataset, device=device)
    for r in rows:
        print('%s: %s' % (r['picture'], r['verdict']))
    print(os.path.join(opt.outdir, REPORT_FILE))
    return 0 if all(r['verdict'] == 'rendered' for r in rows) else 1


if __name__ == '__main__':
    sys.exit(main())
