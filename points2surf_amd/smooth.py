"""Triangle meshes smoothed on the device: rounds of the umbrella operator with uniform weights, a half-step
with lambda and one with mu (Taubin 1995, "lambda | mu"; mu = 0 is plain Laplacian smoothing) -- the remedy for the one-voxel
terraces of an iso-surface, and the "Taubin Smooth" step of the usual iso-surface -> clean -> smooth -> simplify sequence.  It
runs in libp2s_hip.so (p2s_mesh_smooth); the definition is in include/p2s_hip.h.  This is the project's own definition -- not
vcglib's and not MeshLab's filter.  Faces are not touched and vertices are connected by INDEX: run ``clean.repair`` first.
The smoothed mesh is not tested for self-intersections (``gt_sdf.TriMesh.check`` finds them).  The umbrella operator rounds
every crease: the filter that keeps sharp edges is ``denoise``.  Nothing else in the package calls this.
Torch tensors are containers only; no CPU fallback.

The defaults (10 iterations, lambda 0.5, mu -0.53) are MeshLab's Taubin defaults.  Nobody has measured them on reconstructions
of this project: they are a starting point, not a recommendation.

``python -m points2surf_amd.smooth --indir DIR --outdir DIR2 [--iterations 10] [--lambda 0.5] [--mu -0.53]
[--boundary fixed|curve|free] [--dataset FILE] [--gpu_idx I]`` reads every mesh of ``DIR`` that mesh_formats can read (with
``--dataset``: the shapes that the list names), writes ``DIR2/<stem>.ply`` and ``DIR2/smooth_report.csv`` with one row per mesh:
the report of the call, and area and signed volume before and after (``components.components`` of input and output, summed on
the host), which is where shrinkage shows.  A mesh whose output is newer than its input keeps its file and its row.  A mesh
that fails is named in the report with the reason; the run goes on.
"""
import argparse
import csv
import ctypes
import math
import os
import struct
import sys

import numpy as np
import torch

from . import _lib
from . import components as _components
from . import engine as _engine
from . import file_utils
from . import mesh_formats as _formats
from . import ply as _ply
from .simplify import _device, _names

MAX_ITERATIONS = 10000
BOUNDARY_MODES = ('fixed', 'curve', 'free')
CLASSES = ('free', 'boundary curve', 'boundary fixed', 'non-manifold fixed', 'masked', 'unreferenced')
REPORT_KEYS = ('verts_in', 'faces_in', 'free', 'boundary_curve', 'boundary_fixed', 'nonmanifold_fixed', 'masked', 'unreferenced', 'edges',
               'max_neighbours', 'half_steps', 'max_displacement', 'nonfinite')
REPORT_FILE = 'smooth_report.csv'
REPORT_COLUMNS = ('mesh', 'iterations', 'lambda', 'mu', 'boundary') + REPORT_KEYS + ('area_in', 'area_out', 'volume_in', 'volume_out',
                                                                                       'verdict')


def report_dict(a):
    """the int64[16] report of p2s_mesh_smooth as a dict (REPORT_KEYS); ``max_displacement`` is the square root of [10]"""
    a = [int(x) for x in a]
    m = (1 << 32) - 1
    return dict(verts_in=a[0] & m, faces_in=a[0] >> 32, free=a[1], boundary_curve=a[2], boundary_fixed=a[3], nonmanifold_fixed=a[4],
                masked=a[5], unreferenced=a[6], edges=a[7], max_neighbours=a[8], half_steps=a[9],
                max_displacement=math.sqrt(struct.unpack('<d', struct.pack('<q', a[10]))[0]), nonfinite=a[11])


def _check_params(iterations, lam, mu, boundary):
    if isinstance(iterations, bool) or int(iterations) != iterations or not 0 <= int(iterations) <= MAX_ITERATIONS:
        raise ValueError('iterations must be an integer in 0 .. %d (got %r)' % (MAX_ITERATIONS, iterations))
    if not 0.0 < float(lam) <= 1.0:                                     # false for NaN
        raise ValueError('lam must satisfy 0 < lam <= 1 (got %r)' % (lam,))
    if not -2.0 <= float(mu) <= 0.0:
        raise ValueError('mu must lie in -2 .. 0 (got %r)' % (mu,))
    if boundary not in BOUNDARY_MODES:
        raise ValueError('boundary must be one of %s (got %r)' % (', '.join(BOUNDARY_MODES), boundary))


def _ptr(t):
    return _engine._ptr(t) if t is not None and t.numel() else None


def _fixed_mask(fixed, V, dev):
    """``fixed`` [V] (bool or integer, numpy array or tensor, may be None) as a uint8 device tensor of zeros and ones"""
    if fixed is None:
        return None
    if isinstance(fixed, np.ndarray):
        fixed = torch.from_numpy(np.ascontiguousarray(fixed != 0))
    fx = (fixed.to(dev) != 0).to(torch.uint8).contiguous()
    if tuple(fx.shape) != (V,):
        raise ValueError('fixed must be [%d] (got %s)' % (V, tuple(fx.shape)))
    return fx


def smooth(verts, faces, iterations=10, lam=0.5, mu=-0.53, boundary='fixed', fixed=None, device=None, want_class=False):
    """``verts`` [V, 3] float32, ``faces`` [F, 3] int32 (numpy arrays or tensors) -> (verts_out, faces, report): the moved
    vertices as a new float32 device tensor, the faces as an int32 device tensor (untouched) and the report dict (REPORT_KEYS).
    ``boundary``: 'fixed' keeps every vertex on an edge of one face, 'curve' moves those with exactly two such edges along
    their boundary curve, 'free' treats every vertex alike.  ``fixed`` [V] (bool or integer, may be None): nonzero entries
    keep their vertex where it is.  With ``want_class`` the report also holds 'class' [V] uint8 (index of CLASSES)."""
    _check_params(iterations, lam, mu, boundary)
    dev = _device(device)
    lib = _lib.load()
    v, f = _components._mesh(verts, faces, dev)
    V, F = int(v.shape[0]), int(f.shape[0])
    fx = _fixed_mask(fixed, V, dev)
    rep = (ctypes.c_int64 * 16)()
    with torch.cuda.device(dev):
        vo = torch.empty((V, 3), dtype=torch.float32, device=dev)
        cls = torch.empty((V,), dtype=torch.uint8, device=dev) if want_class else None
        _lib.check(lib.p2s_mesh_smooth(_ptr(v), V, _ptr(f), F, int(iterations), float(lam), float(mu), BOUNDARY_MODES.index(boundary),
                                       _ptr(fx), _ptr(vo), _ptr(cls), rep, dev.index, _engine._stream_ptr(dev)))
    r = report_dict(rep)
    if want_class:
        r['class'] = cls
    return vo, f, r


def _measures(v, f, device):
    """area and signed volume of a mesh: the components' float64 measures, summed on the host"""
    if int(f.shape[0]) == 0:
        return 0.0, 0.0
    stats = _components.components(v, f, device=device)[1]
    return float(stats['area'].sum()), float(stats['volume'].sum())


def smooth_file(file_in, file_out, iterations=10, lam=0.5, mu=-0.53, boundary='fixed', device=None):
    """``file_in`` (any type of mesh_formats) smoothed into the PLY ``file_out``; the report of ``smooth`` with 'area_in',
    'area_out', 'volume_in' and 'volume_out' added"""
    _check_params(iterations, lam, mu, boundary)
    v, f = _formats.read_mesh(file_in)
    v, f = np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f).astype(np.int32).reshape(-1, 3)
    vo, fo, rep = smooth(v, f, iterations=iterations, lam=lam, mu=mu, boundary=boundary, device=device)
    rep['area_in'], rep['volume_in'] = _measures(v, fo, device)
    rep['area_out'], rep['volume_out'] = _measures(vo, fo, device)
    os.makedirs(os.path.dirname(os.path.abspath(file_out)), exist_ok=True)
    _ply.write_ply(file_out, vo.cpu().numpy(), fo.cpu().numpy())
    return rep


def _settings(iterations, lam, mu, boundary):
    return {'iterations': str(int(iterations)), 'lambda': repr(float(lam)), 'mu': repr(float(mu)), 'boundary': boundary}


def smooth_dir(indir, outdir, iterations=10, lam=0.5, mu=-0.53, boundary='fixed', dataset=None, device=None):
    """every mesh of ``indir`` as ``outdir/<stem>.ply`` and ``outdir/smooth_report.csv``; a mesh whose output is newer than its
    input, written with the same settings, keeps its file and its row of the earlier report.  Returns the files written by
    this run."""
    _check_params(iterations, lam, mu, boundary)
    os.makedirs(outdir, exist_ok=True)
    report_path = os.path.join(outdir, REPORT_FILE)
    settings = _settings(iterations, lam, mu, boundary)
    old = {}
    if os.path.isfile(report_path):
        with open(report_path, newline='') as fh:
            old = {r['mesh']: r for r in csv.DictReader(fh)}
    written, rows = [], []
    for name in _names(indir, dataset):
        f_in, f_out = os.path.join(indir, name), os.path.join(outdir, os.path.splitext(name)[0] + '.ply')
        prev = old.get(name, {})
        if prev.get('verdict') == 'smoothed' and all(prev.get(k) == x for k, x in settings.items()) and \
                not file_utils.call_necessary([f_in], [f_out]):
            print('up to date: %s' % name)
            rows.append(prev)
            continue
        try:
            rep = smooth_file(f_in, f_out, iterations=iterations, lam=lam, mu=mu, boundary=boundary, device=device)
            row = {k: rep[k] for k in REPORT_KEYS + ('area_in', 'area_out', 'volume_in', 'volume_out')}
            row.update(settings, mesh=name, verdict='smoothed')
            rows.append(row)
            written.append(f_out)
        except Exception as e:                          # named in the report; the run goes on
            if os.path.isfile(f_out):
                os.remove(f_out)                        # a mesh that fails now is not left over from an earlier run
            row = dict.fromkeys(REPORT_COLUMNS, '')
            row.update(settings, mesh=name, verdict='failed: %s' % ' '.join(str(e).split()))
            rows.append(row)
    with open(report_path, 'w', newline='') as fh:
        w = csv.DictWriter(fh, fieldnames=REPORT_COLUMNS)
        w.writeheader()
        w.writerows(rows)
    return written


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m points2surf_amd.smooth',
                                 description='smooth every mesh of INDIR into OUTDIR (Taubin lambda | mu; --mu 0: Laplacian)')
    ap.add_argument('--indir', required=True)
    ap.add_argument('--outdir', required=True)
    ap.add_argument('--iterations', type=int, default=10, help='rounds of a lambda and a mu half-step (0 .. 10000)')
    ap.add_argument('--lambda', dest='lam', type=float, default=0.5, help='0 < lambda <= 1')
    ap.add_argument('--mu', type=float, default=-0.53, help='-2 <= mu <= 0; 0 is plain Laplacian smoothing')
    ap.add_argument('--boundary', choices=BOUNDARY_MODES, default='fixed')
    ap.add_argument('--dataset', default=None, help='a list of shape names: only these meshes')
    ap.add_argument('--gpu_idx', type=int, default=0)
    opt = ap.parse_args(argv)
    try:
        _check_params(opt.iterations, opt.lam, opt.mu, opt.boundary)
    except ValueError as e:
        ap.error(str(e))
    device = _engine.select_device(opt.gpu_idx)
    for f in smooth_dir(opt.indir, opt.outdir, iterations=opt.iterations, lam=opt.lam, mu=opt.mu, boundary=opt.boundary,
                        dataset=opt.dataset, device=device):
        print(f)
    print(os.path.join(opt.outdir, REPORT_FILE))
    return 0


if __name__ == '__main__':
    sys.exit(main())
