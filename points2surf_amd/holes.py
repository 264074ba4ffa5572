"""The holes of triangle meshes closed on the device: every simple boundary loop of at most ``max_hole_edges``
edges gets the minimum-area triangulation of its vertices (Barequet & Sharir 1995; the first stage of Liepa 2003) -- the place
of "Close Holes" in the reference's post-processing script for reconstructions, hole_filling_mesh_simp.mlx (MaxHoleSize 30).
It runs in libp2s_hip.so (p2s_mesh_fill_holes); the definition is in include/p2s_hip.h.  This is the project's own definition
-- not vcglib's ear cutting and not MeshLab's filter.  No vertex is added or moved, and a chord that is an edge of the mesh
already is never used, so no edge gets a third face.  The call neither welds nor orients: run ``clean.repair`` first, and
``manifold.manifold`` where boundary vertices are not simple.  Torch tensors are containers only; no CPU fallback.

``python -m points2surf_amd.holes --indir DIR --outdir DIR2 [--max_hole_edges 30] [--dataset FILE] [--gpu_idx I]`` reads every
mesh of ``DIR`` that mesh_formats can read (with ``--dataset``: the shapes that the list names), writes ``DIR2/<stem>.ply`` and
``DIR2/holes_report.csv`` with one row per mesh.  A mesh whose output is newer than its input keeps its file and its row.  A
mesh that fails is named in the report with the reason; the run goes on.
"""
import argparse
import csv
import ctypes
import os
import sys

import numpy as np
import torch

from . import _lib
from . import engine as _engine
from . import file_utils
from . import mesh_formats as _formats
from . import ply as _ply
from .simplify import _device, _names

P2S_EINVAL = -1
MAX_HOLE_EDGES = 128
REASONS = ('filled', 'too long', 'blocked')
REPORT_KEYS = ('verts_in', 'faces_in', 'faces_out', 'loops_found', 'holes_filled', 'faces_added', 'loops_too_long', 'loops_blocked',
               'boundary_edges_in', 'boundary_edges_out', 'boundary_groups_out', 'longest_filled', 'nonmanifold_edges')
REPORT_FILE = 'holes_report.csv'
REPORT_COLUMNS = ('mesh', 'max_hole_edges') + REPORT_KEYS + ('verdict',)


def report_dict(a):
    """the int64[16] report of p2s_mesh_fill_holes as a dict (REPORT_KEYS)"""
    a = [int(x) for x in a]
    m = (1 << 32) - 1
    return dict(verts_in=a[0] & m, faces_in=a[0] >> 32, faces_out=a[1], loops_found=a[2], holes_filled=a[3], faces_added=a[4],
                loops_too_long=a[5], loops_blocked=a[6], boundary_edges_in=a[7], boundary_edges_out=a[8], boundary_groups_out=a[9],
                longest_filled=a[10], nonmanifold_edges=a[11])


def _check_args(verts, faces, max_hole_edges):
    if len(verts.shape) != 2 or verts.shape[1] != 3:
        raise ValueError('verts must be [V, 3] (got %s)' % (tuple(verts.shape),))
    if len(faces.shape) != 2 or faces.shape[1] != 3:
        raise ValueError('faces must be [F, 3] (got %s)' % (tuple(faces.shape),))
    _check_edges(max_hole_edges)


def _check_edges(max_hole_edges):
    if isinstance(max_hole_edges, bool) or int(max_hole_edges) != max_hole_edges or not 0 <= int(max_hole_edges) <= MAX_HOLE_EDGES:
        raise ValueError('max_hole_edges must be an integer in 0 .. %d (got %r)' % (MAX_HOLE_EDGES, max_hole_edges))


def _ptr(t):
    return _engine._ptr(t) if t is not None and t.numel() else None


def fill(verts, faces, max_hole_edges=30, device=None, want_map=False, want_holes=False):
    """``verts`` [V, 3] float32, ``faces`` [F, 3] int32 (numpy arrays or tensors) -> (verts, faces, report): the input vertices
    (as a float32 device tensor, untouched), the faces [F', 3] int32 with the added ones behind the input's, and the report dict
    (REPORT_KEYS).  With ``want_map`` the report also holds 'face_src' [F'] int32 (the input face, -1 for an added one); with
    ``want_holes`` 'holes' [H, 4] int32 (v0, edges, first added face or -1, reason: index of REASONS) and 'hole_area' [H]
    float64, one row per loop in ascending v0."""
    _check_args(verts, faces, max_hole_edges)
    dev = _device(device)
    lib = _lib.load()
    if isinstance(verts, np.ndarray):
        verts = torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float32))
    if isinstance(faces, np.ndarray):
        faces = torch.from_numpy(np.ascontiguousarray(faces).astype(np.int32))
    v, f = verts.to(dev, torch.float32).contiguous(), faces.to(dev, torch.int32).contiguous()
    V, F = int(v.shape[0]), int(f.shape[0])
    rep = (ctypes.c_int64 * 16)()
    cap_f, cap_h = F + F // 16 + 1024, 256                               # F + boundary edges always suffices; few meshes need it
    with torch.cuda.device(dev):
        while True:
            fo = torch.empty((cap_f, 3), dtype=torch.int32, device=dev)
            fs = torch.empty((cap_f,), dtype=torch.int32, device=dev) if want_map else None
            ho = torch.empty((cap_h, 4), dtype=torch.int32, device=dev) if want_holes else None
            ha = torch.empty((cap_h,), dtype=torch.float64, device=dev) if want_holes else None
            rc = lib.p2s_mesh_fill_holes(_ptr(v), V, _ptr(f), F, int(max_hole_edges), _ptr(fo), cap_f, _ptr(fs), _ptr(ho), _ptr(ha), cap_h,
                                         rep, dev.index, _engine._stream_ptr(dev))
            if rc == P2S_EINVAL and (int(rep[1]) > cap_f or (want_holes and int(rep[2]) > cap_h)):      # the capacity refusal: exact counts
                cap_f, cap_h = max(cap_f, int(rep[1])), max(cap_h, int(rep[2]))
                continue
            _lib.check(rc)
            break
    r = report_dict(rep)
    if want_map:
        r['face_src'] = fs[:r['faces_out']]
    if want_holes:
        r['holes'] = ho[:r['loops_found']]
        r['hole_area'] = ha[:r['loops_found']]
    return v, fo[:r['faces_out']], r


def fill_file(file_in, file_out, max_hole_edges=30, device=None):
    """``file_in`` (any type of mesh_formats) with its holes closed into the PLY ``file_out``; the report of ``fill``"""
    _check_edges(max_hole_edges)
    v, f = _formats.read_mesh(file_in)
    v, f = np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f).astype(np.int32).reshape(-1, 3)
    vo, fo, rep = fill(v, f, max_hole_edges=max_hole_edges, device=device)
    os.makedirs(os.path.dirname(os.path.abspath(file_out)), exist_ok=True)
    _ply.write_ply(file_out, vo.cpu().numpy(), fo.cpu().numpy())
    return rep


def _row(name, max_hole_edges, rep):
    row = {k: rep[k] for k in REPORT_KEYS}
    row.update(mesh=name, max_hole_edges=max_hole_edges, verdict='closed' if rep['boundary_edges_out'] == 0 else 'open')
    return row


def fill_dir(indir, outdir, max_hole_edges=30, dataset=None, device=None):
    """every mesh of ``indir`` as ``outdir/<stem>.ply`` and ``outdir/holes_report.csv``; a mesh whose output is newer than its
    input keeps its file and its row of the earlier report.  Returns the files written by this run."""
    _check_edges(max_hole_edges)
    os.makedirs(outdir, exist_ok=True)
    report_path = os.path.join(outdir, REPORT_FILE)
    old = {}
    if os.path.isfile(report_path):
        with open(report_path, newline='') as fh:
            old = {r['mesh']: r for r in csv.DictReader(fh)}
    written, rows = [], []
    for name in _names(indir, dataset):
        f_in, f_out = os.path.join(indir, name), os.path.join(outdir, os.path.splitext(name)[0] + '.ply')
        prev = old.get(name, {})
        if prev.get('verdict') in ('closed', 'open') and prev.get('max_hole_edges') == str(max_hole_edges) and \
                not file_utils.call_necessary([f_in], [f_out]):
            print('up to date: %s' % name)
            rows.append(prev)
            continue
        try:
            rows.append(_row(name, max_hole_edges, fill_file(f_in, f_out, max_hole_edges=max_hole_edges, device=device)))
            written.append(f_out)
        except Exception as e:                          # named in the report; the run goes on
            if os.path.isfile(f_out):
                os.remove(f_out)                        # a mesh that fails now is not left over from an earlier run
            row = dict.fromkeys(REPORT_COLUMNS, '')
            row.update(mesh=name, max_hole_edges=max_hole_edges, verdict='failed: %s' % ' '.join(str(e).split()))
            rows.append(row)
    with open(report_path, 'w', newline='') as fh:
        w = csv.DictWriter(fh, fieldnames=REPORT_COLUMNS)
        w.writeheader()
        w.writerows(rows)
    return written


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m points2surf_amd.holes',
                                 description='close the holes of every mesh of INDIR into OUTDIR by minimum-area triangulation')
    ap.add_argument('--indir', required=True)
    ap.add_argument('--outdir', required=True)
    ap.add_argument('--max_hole_edges', type=int, default=30, help='close loops of up to this many edges (0 .. 128)')
    ap.add_argument('--dataset', default=None, help='a list of shape names: only these meshes')
    ap.add_argument('--gpu_idx', type=int, default=0)
    opt = ap.parse_args(argv)
    if not 0 <= opt.max_hole_edges <= MAX_HOLE_EDGES:
        ap.error('--max_hole_edges must lie in 0 .. %d' % MAX_HOLE_EDGES)
    device = _engine.select_device(opt.gpu_idx)
    for f in fill_dir(opt.indir, opt.outdir, max_hole_edges=opt.max_hole_edges, dataset=opt.dataset, device=device):
        print(f)
    print(os.path.join(opt.outdir, REPORT_FILE))
    return 0


if __name__ == '__main__':
    sys.exit(main())
