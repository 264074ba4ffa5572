"""Triangle meshes denoised on the device with their sharp edges kept: the face normals are filtered with
the weight max(0, ni . nj - T)^2 over the faces that share a vertex, then the vertices are moved toward the filtered normals
(Sun, Rosin, Martin and Langbein, "Fast and effective feature-preserving mesh denoising", TVCG 2007) -- where ``smooth``, the
umbrella operator, rounds every crease, this keeps the flat faces and sharp edges of CAD parts and prints.  It runs in
libp2s_hip.so (p2s_mesh_denoise); the definition is in include/p2s_hip.h.  This is the project's own definition.  Faces are not
touched and are connected by vertex INDEX; faces of opposite orientation do not see each other: run ``clean.repair`` first.
The face weights are uniform (no area weight), nothing chooses T, a fan of d faces at one vertex costs O(d^2) per normal
iteration, and the result is not tested for self-intersections (``gt_sdf.TriMesh.check`` finds them).  Nothing else in the
package calls this.  Torch tensors are containers only; no CPU fallback.

The defaults (T = 0.5, 10 normal and 10 vertex iterations) are the middle of the paper's ranges and of the one table this was
tried on, a noisy cube.  Nobody has measured them on reconstructions of this project: they are a starting point, not a
recommendation.

``python -m points2surf_amd.denoise --indir DIR --outdir DIR2 [--threshold 0.5] [--normal_iterations 10]
[--vertex_iterations 10] [--boundary fixed|free] [--dataset FILE] [--gpu_idx I]`` reads every mesh of ``DIR`` that mesh_formats
can read (with ``--dataset``: the shapes that the list names), writes ``DIR2/<stem>.ply`` and ``DIR2/denoise_report.csv`` with
one row per mesh: the report of the call, and area and signed volume before and after (``components.components`` of input and
output, summed on the host).  A mesh whose output is newer than its input keeps its file and its row.  A mesh that fails is
named in the report with the reason; the run goes on.
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
from .smooth import _fixed_mask, _measures, _ptr

MAX_ITERATIONS = 10000
BOUNDARY_MODES = ('fixed', 'free')
CLASSES = ('free', 'boundary fixed', 'masked', 'unreferenced', 'no live face')
REPORT_KEYS = ('verts_in', 'faces_in', 'free', 'boundary_fixed', 'masked', 'unreferenced', 'no_live_face', 'dead_faces', 'max_neighbours',
               'normal_iterations_run', 'vertex_iterations_run', 'max_displacement', 'nonfinite')
REPORT_FILE = 'denoise_report.csv'
REPORT_COLUMNS = ('mesh', 'threshold', 'normal_iterations', 'vertex_iterations', 'boundary') + REPORT_KEYS + (
    'area_in', 'area_out', 'volume_in', 'volume_out', 'verdict')


def report_dict(a):
    """the int64[16] report of p2s_mesh_denoise as a dict (REPORT_KEYS); ``max_displacement`` is the square root of [10]"""
    a = [int(x) for x in a]
    m = (1 << 32) - 1
    return dict(verts_in=a[0] & m, faces_in=a[0] >> 32, free=a[1], boundary_fixed=a[2], masked=a[3], unreferenced=a[4], no_live_face=a[5],
                dead_faces=a[6], max_neighbours=a[7], normal_iterations_run=a[8], vertex_iterations_run=a[9],
                max_displacement=math.sqrt(struct.unpack('<d', struct.pack('<q', a[10]))[0]), nonfinite=a[11])


def _check_params(threshold, normal_iterations, vertex_iterations, boundary):
    if not 0.0 <= float(threshold) < 1.0:                               # false for NaN
        raise ValueError('threshold must satisfy 0 <= threshold < 1 (got %r)' % (threshold,))
    for name, it in (('normal_iterations', normal_iterations), ('vertex_iterations', vertex_iterations)):
        if isinstance(it, bool) or int(it) != it or not 0 <= int(it) <= MAX_ITERATIONS:
            raise ValueError('%s must be an integer in 0 .. %d (got %r)' % (name, MAX_ITERATIONS, it))
    if boundary not in BOUNDARY_MODES:
        raise ValueError('boundary must be one of %s (got %r)' % (', '.join(BOUNDARY_MODES), boundary))


def denoise(verts, faces, threshold=0.5, normal_iterations=10, vertex_iterations=10, boundary='fixed', fixed=None, device=None,
            want_class=False, want_normals=False):
    """``verts`` [V, 3] float32, ``faces`` [F, 3] int32 (numpy arrays or tensors) -> (verts_out, faces, report): the moved
    vertices as a new float32 device tensor, the faces as an int32 device tensor (untouched) and the report dict (REPORT_KEYS).
    ``threshold`` is T: a neighbour whose normal has a cosine of at most T with a face's own does not count.  ``boundary``:
    'fixed' keeps every vertex on an edge of one face, 'free' treats every vertex alike.  ``fixed`` [V] (bool or integer, may
    be None): nonzero entries keep their vertex where it is.  With ``want_class`` the report also holds 'class' [V] uint8
    (index of CLASSES), with ``want_normals`` 'normals' [F, 3] float32, the filtered normals that the vertices were moved
    toward."""
    _check_params(threshold, normal_iterations, vertex_iterations, boundary)
    dev = _device(device)
    lib = _lib.load()
    v, f = _components._mesh(verts, faces, dev)
    V, F = int(v.shape[0]), int(f.shape[0])
    fx = _fixed_mask(fixed, V, dev)
    rep = (ctypes.c_int64 * 16)()
    with torch.cuda.device(dev):
        vo = torch.empty((V, 3), dtype=torch.float32, device=dev)
        cls = torch.empty((V,), dtype=torch.uint8, device=dev) if want_class else None
        nrm = torch.empty((F, 3), dtype=torch.float32, device=dev) if want_normals else None
        _lib.check(lib.p2s_mesh_denoise(_ptr(v), V, _ptr(f), F, float(threshold), int(normal_iterations), int(vertex_iterations),
                                        BOUNDARY_MODES.index(boundary), _ptr(fx), _ptr(vo), _ptr(nrm), _ptr(cls), rep, dev.index,
                                        _engine._stream_ptr(dev)))
    r = report_dict(rep)
    if want_class:
        r['class'] = cls
    if want_normals:
        r['normals'] = nrm
    return vo, f, r


def denoise_file(file_in, file_out, threshold=0.5, normal_iterations=10, vertex_iterations=10, boundary='fixed', device=None):
    """``file_in`` (any type of mesh_formats) denoised into the PLY ``file_out``; the report of ``denoise`` with 'area_in',
    'area_out', 'volume_in' and 'volume_out' added"""
    _check_params(threshold, normal_iterations, vertex_iterations, boundary)
    v, f = _formats.read_mesh(file_in)
    v, f = np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f).astype(np.int32).reshape(-1, 3)
    vo, fo, rep = denoise(v, f, threshold=threshold, normal_iterations=normal_iterations, vertex_iterations=vertex_iterations,
                          boundary=boundary, device=device)
    rep['area_in'], rep['volume_in'] = _measures(v, fo, device)
    rep['area_out'], rep['volume_out'] = _measures(vo, fo, device)
    os.makedirs(os.path.dirname(os.path.abspath(file_out)), exist_ok=True)
    _ply.write_ply(file_out, vo.cpu().numpy(), fo.cpu().numpy())
    return rep


def _settings(threshold, normal_iterations, vertex_iterations, boundary):
    return {'threshold': repr(float(threshold)), 'normal_iterations': str(int(normal_iterations)),
            'vertex_iterations': str(int(vertex_iterations)), 'boundary': boundary}


def denoise_dir(indir, outdir, threshold=0.5, normal_iterations=10, vertex_iterations=10, boundary='fixed', dataset=None, device=None):
    """every mesh of ``indir`` as ``outdir/<stem>.ply`` and ``outdir/denoise_report.csv``; a mesh whose output is newer than its
    input, written with the same settings, keeps its file and its row of the earlier report.  Returns the files written by
    this run."""
    _check_params(threshold, normal_iterations, vertex_iterations, boundary)
    os.makedirs(outdir, exist_ok=True)
    report_path = os.path.join(outdir, REPORT_FILE)
    settings = _settings(threshold, normal_iterations, vertex_iterations, boundary)
    old = {}
    if os.path.isfile(report_path):
        with open(report_path, newline='') as fh:
            old = {r['mesh']: r for r in csv.DictReader(fh)}
    written, rows = [], []
    for name in _names(indir, dataset):
        f_in, f_out = os.path.join(indir, name), os.path.join(outdir, os.path.splitext(name)[0] + '.ply')
        prev = old.get(name, {})
        if prev.get('verdict') == 'denoised' and all(prev.get(k) == x for k, x in settings.items()) and \
                not file_utils.call_necessary([f_in], [f_out]):
            print('up to date: %s' % name)
            rows.append(prev)
            continue
        try:
            rep = denoise_file(f_in, f_out, threshold=threshold, normal_iterations=normal_iterations, vertex_iterations=vertex_iterations,
                               boundary=boundary, device=device)
            row = {k: rep[k] for k in REPORT_KEYS + ('area_in', 'area_out', 'volume_in', 'volume_out')}
            row.update(settings, mesh=name, verdict='denoised')
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
    ap = argparse.ArgumentParser(prog='python -m points2surf_amd.denoise',
                                 description='denoise every mesh of INDIR into OUTDIR, keeping sharp edges (normal filtering)')
    ap.add_argument('--indir', required=True)
    ap.add_argument('--outdir', required=True)
    ap.add_argument('--threshold', type=float, default=0.5, help='0 <= T < 1: neighbours with a cosine of at most T do not count')
    ap.add_argument('--normal_iterations', type=int, default=10, help='rounds of the normal filter (0 .. 10000)')
    ap.add_argument('--vertex_iterations', type=int, default=10, help='rounds of the vertex update (0 .. 10000)')
    ap.add_argument('--boundary', choices=BOUNDARY_MODES, default='fixed')
    ap.add_argument('--dataset', default=None, help='a list of shape names: only these meshes')
    ap.add_argument('--gpu_idx', type=int, default=0)
    opt = ap.parse_args(argv)
    try:
        _check_params(opt.threshold, opt.normal_iterations, opt.vertex_iterations, opt.boundary)
    except ValueError as e:
        ap.error(str(e))
    device = _engine.select_device(opt.gpu_idx)
    for f in denoise_dir(opt.indir, opt.outdir, threshold=opt.threshold, normal_iterations=opt.normal_iterations,
                         vertex_iterations=opt.vertex_iterations, boundary=opt.boundary, dataset=opt.dataset, device=device):
        print(f)
    print(os.path.join(opt.outdir, REPORT_FILE))
    return 0


if __name__ == '__main__':
    sys.exit(main())
