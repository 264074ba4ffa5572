"""Simplification of triangle meshes on the device by quadric vertex clustering (Lindstrom 2000,
"Out-of-core simplification of large polygonal models"): one grid over the mesh, one vertex per occupied cell, placed by
the accumulated plane quadrics of the faces that touch the cell.  It runs in libp2s_hip.so (p2s_mesh_simplify); the
definition is in include/p2s_hip.h.  This is the project's own definition -- it does NOT reproduce MeshLab's "Quadric Edge
Collapse Decimation" of the reference's ``hole_filling_mesh_simp.mlx``.  Clustering does not preserve topology: the report
counts the boundary edges and the edges of more than two faces of the input and of the output.  Torch tensors are
containers only; no CPU fallback.

``python -m points2surf_amd.simplify --indir DIR --outdir DIR2 [--max_faces 100000] [--resolution R]
[--placement quadric|mean] [--epsilon E] [--dataset FILE]`` reads every mesh of ``DIR`` that mesh_formats can read (with
``--dataset``: the shapes that the list names), writes ``DIR2/<stem>.ply`` and ``DIR2/simplify_report.csv`` with one row per
mesh: the report, the milliseconds and the verdict.  A mesh that fails is named there with the reason; the run goes on.
"""
import argparse
import csv
import ctypes
import os
import time

import numpy as np
import torch

from . import _lib
from . import engine as _engine
from . import mesh_formats as _formats
from . import ply as _ply

PLACEMENTS = {'mean': 0, 'quadric': 1}
REPORT_KEYS = ('verts_in', 'faces_in', 'verts_out', 'faces_out', 'resolution', 'cells_occupied', 'faces_collapsed',
               'faces_duplicate', 'faces_degenerate', 'cells_quadric', 'cells_trace_zero', 'cells_fallback', 'probes',
               'boundary_edges_out', 'nonmanifold_edges_out', 'boundary_edges_in', 'nonmanifold_edges_in')
REPORT_FILE = 'simplify_report.csv'


def report_dict(a):
    """the int64[16] report of p2s_mesh_simplify as a dict (REPORT_KEYS)"""
    a = [int(x) for x in a]
    m = (1 << 32) - 1
    return dict(verts_in=a[0] & m, faces_in=a[0] >> 32, verts_out=a[1], faces_out=a[2], resolution=a[3], cells_occupied=a[4],
                faces_collapsed=a[5], faces_duplicate=a[6], faces_degenerate=a[7], cells_quadric=a[8], cells_trace_zero=a[9],
                cells_fallback=a[10], probes=a[11], boundary_edges_out=a[12] & m, nonmanifold_edges_out=a[12] >> 32,
                boundary_edges_in=a[13] & m, nonmanifold_edges_in=a[13] >> 32)


def _device(device):
    if not torch.cuda.is_available():
        raise RuntimeError('points2surf_amd needs a ROCm GPU (gfx950); no CPU fallback exists')
    d = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    return torch.device('cuda', torch.cuda.current_device()) if d.index is None else d


def _check_args(max_faces, resolution, placement, epsilon):
    if placement not in PLACEMENTS:
        raise ValueError('placement must be one of %s (got %r)' % (', '.join(sorted(PLACEMENTS)), placement))
    resolution = int(resolution or 0)
    if not 0 <= resolution <= 1024:
        raise ValueError('resolution must be 0 (searched for max_faces) or 1 .. 1024 (got %d)' % resolution)
    if resolution == 0 and (max_faces is None or int(max_faces) < 0):
        raise ValueError('max_faces >= 0 is needed when no resolution is given (got %r)' % (max_faces,))
    epsilon = float(epsilon)
    if not 1e-6 <= epsilon <= 1.0:
        raise ValueError('epsilon must lie in [1e-6, 1] (got %r)' % epsilon)
    return int(max_faces if max_faces is not None else 0), resolution, PLACEMENTS[placement], epsilon


def simplify(verts, faces, max_faces=100000, resolution=0, placement='quadric', epsilon=1e-3, device=None, want_map=False):
    """``verts`` [V, 3] float32, ``faces`` [F, 3] int32 (numpy arrays or tensors) -> (verts, faces, report): device tensors
    [V', 3] float32 and [F', 3] int32 and the report dict (REPORT_KEYS).  ``resolution`` 1 .. 1024 is the grid; 0 searches
    the finest grid that leaves at most ``max_faces`` faces (a mesh that has no more is returned as it is).  With
    ``want_map`` the report also holds 'vert_map' [V] int32 (the output vertex of every input vertex, -1: none) and
    'face_src' [F'] int32 (the input face of every output face)."""
    max_faces, resolution, placement, epsilon = _check_args(max_faces, resolution, placement, epsilon)
    dev = _device(device)
    lib = _lib.load()
    if isinstance(verts, np.ndarray):
        verts = torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float32))
    v = verts.to(dev, torch.float32).contiguous()
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError('verts must be [V, 3] (got %s)' % (tuple(v.shape),))
    if isinstance(faces, np.ndarray):
        faces = torch.from_numpy(np.ascontiguousarray(faces).astype(np.int32))
    f = faces.to(dev, torch.int32).contiguous()
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError('faces must be [F, 3] (got %s)' % (tuple(f.shape),))
    V, F = int(v.shape[0]), int(f.shape[0])
    vo = torch.empty((V, 3), dtype=torch.float32, device=dev)
    fo = torch.empty((F, 3), dtype=torch.int32, device=dev)
    so = torch.empty((F,), dtype=torch.int32, device=dev) if want_map else None
    mo = torch.empty((V,), dtype=torch.int32, device=dev) if want_map else None
    rep = (ctypes.c_int64 * 16)()

    def ptr(t):
        return _engine._ptr(t) if t is not None and t.numel() else None

    with torch.cuda.device(dev):
        _lib.check(lib.p2s_mesh_simplify(ptr(v), V, ptr(f), F, resolution, max_faces, placement, ctypes.c_double(epsilon), ptr(vo), V,
                                         ptr(fo), ptr(so), F, ptr(mo), rep, dev.index, _engine._stream_ptr(dev)))
    r = report_dict(rep)
    if want_map:
        r['vert_map'] = mo
        r['face_src'] = so[:r['faces_out']]
    return vo[:r['verts_out']], fo[:r['faces_out']], r


def simplify_file(file_in, file_out, device=None, **kw):
    """``file_in`` (any type of mesh_formats) simplified into the PLY ``file_out``; (report dict, milliseconds of the call
    with the mesh on the device)"""
    v, f = _formats.read_mesh(file_in)
    dev = _device(device)
    vt = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev)
    ft = torch.from_numpy(np.ascontiguousarray(f).astype(np.int32)).to(dev)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    vo, fo, rep = simplify(vt, ft, device=dev, **kw)          # the call synchronises its stream
    ms = (time.perf_counter() - t0) * 1e3
    os.makedirs(os.path.dirname(os.path.abspath(file_out)), exist_ok=True)
    _ply.write_ply(file_out, vo.cpu().numpy(), fo.cpu().numpy())
    return rep, ms


def _names(indir, dataset):
    names = [n for n in sorted(os.listdir(indir))
             if os.path.isfile(os.path.join(indir, n)) and os.path.splitext(n)[1].lower() in _formats.READERS]
    if dataset:
        with open(dataset) as fh:
            wanted = {line.strip() for line in fh if line.strip()}
        names = [n for n in names if os.path.splitext(n)[0] in wanted or n in wanted]
    return names


def simplify_dir(indir, outdir, dataset=None, device=None, **kw):
    """every mesh of ``indir`` as ``outdir/<stem>.ply`` and ``outdir/simplify_report.csv``; returns the files written"""
    os.makedirs(outdir, exist_ok=True)
    written, rows = [], []
    for name in _names(indir, dataset):
        f_out = os.path.join(outdir, os.path.splitext(name)[0] + '.ply')
        try:
            rep, ms = simplify_file(os.path.join(indir, name), f_out, device=device, **kw)
            rows.append([name] + [rep[k] for k in REPORT_KEYS] + ['%.3f' % ms, 'written'])
            written.append(f_out)
        except Exception as e:                          # named in the report; the run goes on
            if os.path.isfile(f_out):
                os.remove(f_out)                        # a mesh that fails now is not left over from an earlier run
            rows.append([name] + [''] * len(REPORT_KEYS) + ['', 'failed: %s' % ' '.join(str(e).split())])
    with open(os.path.join(outdir, REPORT_FILE), 'w', newline='') as fh:
        w = csv.writer(fh)
        w.writerow(['mesh'] + list(REPORT_KEYS) + ['milliseconds', 'verdict'])
        w.writerows(rows)
    return written


def main(argv=None):
    ap = argparse.ArgumentParser(description='simplify every mesh of INDIR into OUTDIR by quadric vertex clustering')
    ap.add_argument('--indir', required=True)
    ap.add_argument('--outdir', required=True)
    ap.add_argument('--max_faces', type=int, default=100000, help='the finest grid that leaves at most this many faces')
    ap.add_argument('--resolution', type=int, default=0, help='the grid 1 .. 1024 itself; 0: searched for --max_faces')
    ap.add_argument('--placement', choices=sorted(PLACEMENTS), default='quadric')
    ap.add_argument('--epsilon', type=float, default=1e-3, help='Tikhonov weight of the quadric solve, in [1e-6, 1]')
    ap.add_argument('--dataset', default=None, help='a list of shape names: only these meshes')
    opt = ap.parse_args(argv)
    _check_args(opt.max_faces, opt.resolution, opt.placement, opt.epsilon)
    for f in simplify_dir(opt.indir, opt.outdir, dataset=opt.dataset, max_faces=opt.max_faces, resolution=opt.resolution,
                          placement=opt.placement, epsilon=opt.epsilon):
        print(f)
    print(os.path.join(opt.outdir, REPORT_FILE))


if __name__ == '__main__':
    main()
