"""Triangle meshes made 2-manifold on the device: faces removed at the edges of more than two faces, vertices
split where their faces do not form one fan -- steps 1 to 3 of the reference's post-processing script for reconstructions,
hole_filling_mesh_simp.mlx.  It runs in libp2s_hip.so (p2s_mesh_manifold); the definition is in include/p2s_hip.h.  This is
the project's own definition -- not vcglib's and not MeshLab's filters.  Vertices are connected by INDEX, coordinates are never
compared: the split leaves vertices of equal coordinates, which a later weld (``clean.repair``) merges again.  Torch tensors
are containers only; no CPU fallback.

``python -m points2surf_amd.manifold --indir DIR --outdir DIR2 [--edges split|remove] [--max_hole_edges 30] [--fill fan|area]
[--dataset FILE] [--gpu_idx I]`` reads every mesh of ``DIR`` that mesh_formats can read (with ``--dataset``: the shapes that the list names),
writes ``DIR2/<stem>.ply`` and ``DIR2/manifold_report.csv`` with one row per mesh.  A mesh whose output is newer than its input
keeps its file and its row.  A mesh that fails is named in the report with the reason; the run goes on.

``--edges split`` (the default) loses no face: one call with mode 2.  ``--edges remove`` is the reference script's sequence,
three calls: mode 1 (faces removed at edges of more than two faces), ``clean.repair(max_hole_edges)``, mode 2.  What that
sequence implies: the repair call fills holes of up to ``--max_hole_edges`` edges (30 is the script's value) by fans, and it
also welds equal coordinates, orients the components and flips inverted ones; a fan fill may itself create an edge of three
faces; so it is the last call, in mode 2, that guarantees the result.  The watertight / winding_consistent / is_volume bits of
the report are the repair's, taken BEFORE that last call.  How many faces ``remove`` costs on real reconstructions nobody has
measured.  Nothing chooses between the two automatically.  ``--fill area`` (opt-in; ``fan`` is the default and changes nothing)
replaces the fans: the repair call fills nothing, and BEHIND the last call ``holes.fill`` closes loops of up to ``--max_hole_edges``
edges (0 .. 128) by their minimum-area triangulation, which never adds an edge of more than two faces.
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
EDGES = ('split', 'remove')
FILLS = ('fan', 'area')
REPORT_KEYS = ('verts_in', 'faces_in', 'verts_out', 'faces_out', 'nonmanifold_edges_in', 'faces_removed', 'vertices_split', 'vertices_added',
               'vertices_dropped', 'boundary_edges_in', 'boundary_edges_out', 'rejoined_edges', 'hook_rounds')
REPORT_FILE = 'manifold_report.csv'
REPORT_COLUMNS = ('mesh', 'edges', 'verts_in', 'faces_in', 'verts_out', 'faces_out', 'nonmanifold_edges_in', 'faces_removed', 'holes_filled',
                  'faces_added', 'vertices_split', 'vertices_added', 'boundary_edges_in', 'boundary_edges_out', 'rejoined_edges', 'watertight',
                  'winding_consistent', 'is_volume', 'verdict')


def report_dict(a):
    """the int64[16] report of p2s_mesh_manifold as a dict (REPORT_KEYS)"""
    a = [int(x) for x in a]
    m = (1 << 32) - 1
    return dict(verts_in=a[0] & m, faces_in=a[0] >> 32, verts_out=a[1], faces_out=a[2], nonmanifold_edges_in=a[3], faces_removed=a[4],
                vertices_split=a[5], vertices_added=a[6], vertices_dropped=a[7], boundary_edges_in=a[8], boundary_edges_out=a[9],
                rejoined_edges=a[10], hook_rounds=a[11])


def _mode(edges, split):
    if edges not in EDGES:
        raise ValueError('edges must be one of %s (got %r)' % (', '.join(EDGES), edges))
    mode = (1 if edges == 'remove' else 0) | (2 if split else 0)
    if mode == 0:
        raise ValueError("edges='split' with split=False leaves nothing to do")
    return mode


def _shapes(verts, faces):
    if len(verts.shape) != 2 or verts.shape[1] != 3:
        raise ValueError('verts must be [V, 3] (got %s)' % (tuple(verts.shape),))
    if len(faces.shape) != 2 or faces.shape[1] != 3:
        raise ValueError('faces must be [F, 3] (got %s)' % (tuple(faces.shape),))


def _ptr(t):
    return _engine._ptr(t) if t is not None and t.numel() else None


def manifold(verts, faces, edges='split', split=True, device=None, want_map=False):
    """``verts`` [V, 3] float32, ``faces`` [F, 3] int32 (numpy arrays or tensors) -> (verts, faces, report): device tensors
    [V', 3] float32 and [F', 3] int32 and the report dict (REPORT_KEYS).  One call of p2s_mesh_manifold: ``edges='split'`` is
    mode 2; ``edges='remove'`` is mode 3, or mode 1 with ``split=False``.  With ``want_map`` the report also holds 'vert_src'
    [V'] and 'face_src' [F'] int32 device tensors: the input ids."""
    mode = _mode(edges, split)
    _shapes(verts, faces)
    dev = _device(device)
    lib = _lib.load()
    if isinstance(verts, np.ndarray):
        verts = torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float32))
    if isinstance(faces, np.ndarray):
        faces = torch.from_numpy(np.ascontiguousarray(faces).astype(np.int32))
    v, f = verts.to(dev, torch.float32).contiguous(), faces.to(dev, torch.int32).contiguous()
    V, F = int(v.shape[0]), int(f.shape[0])
    fo = torch.empty((F, 3), dtype=torch.int32, device=dev)
    fs = torch.empty((F,), dtype=torch.int32, device=dev) if want_map else None
    rep = (ctypes.c_int64 * 16)()
    cap = min(3 * F, V + V // 8 + 1024)                                  # 3 F always suffices; few meshes need it
    with torch.cuda.device(dev):
        while True:
            vo = torch.empty((cap, 3), dtype=torch.float32, device=dev)
            vs = torch.empty((cap,), dtype=torch.int32, device=dev) if want_map else None
            rc = lib.p2s_mesh_manifold(_ptr(v), V, _ptr(f), F, mode, _ptr(vo), cap, _ptr(fo), F, _ptr(vs), _ptr(fs), rep, dev.index,
                                       _engine._stream_ptr(dev))
            if rc == P2S_EINVAL and int(rep[1]) > cap:              # the capacity refusal: the report holds the exact count
                cap = int(rep[1])
                continue
            _lib.check(rc)
            break
    r = report_dict(rep)
    if want_map:
        r['vert_src'] = vs[:r['verts_out']]
        r['face_src'] = fs[:r['faces_out']]
    return vo[:r['verts_out']], fo[:r['faces_out']], r


def _fill(fill, max_hole_edges):
    if fill not in FILLS:
        raise ValueError('fill must be one of %s (got %r)' % (', '.join(FILLS), fill))
    most = 64 if fill == 'fan' else 128
    if not 0 <= int(max_hole_edges) <= most:
        raise ValueError('max_hole_edges must lie in 0 .. %d (got %r)' % (most, max_hole_edges))


def remove_fill_split(verts, faces, max_hole_edges=30, device=None, fill='fan'):
    """the reference script's sequence (see the head of this file): mode 1, ``clean.repair(max_hole_edges)``, mode 2 ->
    (verts, faces, report): the report of the last call with 'verts_in', 'faces_in', 'nonmanifold_edges_in', 'faces_removed' and
    'boundary_edges_in' of the first, and 'repair': the report of the repair call.  ``fill='area'``: the repair fills nothing
    (``max_hole_edges=0``: weld, orient, flip), and behind mode 2 ``holes.fill(max_hole_edges)`` (0 .. 128) closes the loops by
    their minimum-area triangulation, which adds no edge of more than two faces; the report then holds 'fill', the report of
    that call, and its 'faces_out' and 'boundary_edges_out'"""
    from . import clean
    _fill(fill, max_hole_edges)
    if fill == 'area':
        from . import holes
        v1, f1, first = manifold(verts, faces, edges='remove', split=False, device=device)
        v2, f2, _, mid = clean.repair(v1, f1, max_hole_edges=0, device=device)
        v3, f3, last = manifold(v2, f2, edges='split', device=device)
        v4, f4, filled = holes.fill(v3, f3, max_hole_edges=int(max_hole_edges), device=device)
        for k in ('verts_in', 'faces_in', 'nonmanifold_edges_in', 'faces_removed', 'boundary_edges_in'):
            last[k] = first[k]
        last.update(repair=mid, fill=filled, faces_out=filled['faces_out'], boundary_edges_out=filled['boundary_edges_out'])
        return v4, f4, last
    v1, f1, first = manifold(verts, faces, edges='remove', split=False, device=device)
    v2, f2, _, mid = clean.repair(v1, f1, max_hole_edges=int(max_hole_edges), device=device)
    v3, f3, last = manifold(v2, f2, edges='split', device=device)
    for k in ('verts_in', 'faces_in', 'nonmanifold_edges_in', 'faces_removed', 'boundary_edges_in'):
        last[k] = first[k]
    last['repair'] = mid
    return v3, f3, last


def manifold_file(file_in, file_out, edges='split', max_hole_edges=30, device=None, fill='fan'):
    """``file_in`` (any type of mesh_formats) made 2-manifold into the PLY ``file_out``; the report of ``manifold`` (split) or of
    ``remove_fill_split`` (remove, with ``fill``)"""
    _mode(edges, True)
    v, f = _formats.read_mesh(file_in)
    v, f = np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f).astype(np.int32).reshape(-1, 3)
    if edges == 'remove':
        vo, fo, rep = remove_fill_split(v, f, max_hole_edges=max_hole_edges, device=device, fill=fill)
    else:
        vo, fo, rep = manifold(v, f, device=device)
    os.makedirs(os.path.dirname(os.path.abspath(file_out)), exist_ok=True)
    _ply.write_ply(file_out, vo.cpu().numpy(), fo.cpu().numpy())
    return rep


def _row(name, edges, rep):
    row = dict.fromkeys(REPORT_COLUMNS, '')
    row.update({k: rep[k] for k in REPORT_COLUMNS if k in rep})
    if 'repair' in rep:
        row.update({k: rep['repair'][k] for k in ('holes_filled', 'faces_added', 'watertight', 'winding_consistent', 'is_volume')})
    if 'fill' in rep:                                   # fill='area': the holes were closed behind the repair, by holes.fill
        row.update({k: rep['fill'][k] for k in ('holes_filled', 'faces_added')})
    row.update(mesh=name, edges=edges, verdict='closed' if rep['boundary_edges_out'] == 0 else 'open')      # 2-manifold either way
    return row


def manifold_dir(indir, outdir, edges='split', max_hole_edges=30, dataset=None, device=None, fill='fan'):
    """every mesh of ``indir`` as ``outdir/<stem>.ply`` and ``outdir/manifold_report.csv``; a mesh whose output is newer than its
    input keeps its file and its row of the earlier report.  Returns the files written by this run.  ``fill='area'`` with
    ``edges='remove'`` is named 'remove+area' in the report's column 'edges'."""
    _mode(edges, True)
    if edges == 'remove':
        _fill(fill, max_hole_edges)
        if fill == 'area':
            edges = 'remove+area'
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
        if prev.get('verdict') in ('closed', 'open') and prev.get('edges') == edges and not file_utils.call_necessary([f_in], [f_out]):
            print('up to date: %s' % name)
            rows.append(prev)
            continue
        try:
            rows.append(_row(name, edges, manifold_file(f_in, f_out, edges=edges.split('+')[0], max_hole_edges=max_hole_edges, device=device,
                                                        fill=fill)))
            written.append(f_out)
        except Exception as e:                          # named in the report; the run goes on
            if os.path.isfile(f_out):
                os.remove(f_out)                        # a mesh that fails now is not left over from an earlier run
            row = dict.fromkeys(REPORT_COLUMNS, '')
            row.update(mesh=name, edges=edges, verdict='failed: %s' % ' '.join(str(e).split()))
            rows.append(row)
    with open(report_path, 'w', newline='') as fh:
        w = csv.DictWriter(fh, fieldnames=REPORT_COLUMNS)
        w.writeheader()
        w.writerows(rows)
    return written


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m points2surf_amd.manifold',
                                 description='make every mesh of INDIR 2-manifold into OUTDIR: no edge of more than two faces, one fan per vertex')
    ap.add_argument('--indir', required=True)
    ap.add_argument('--outdir', required=True)
    ap.add_argument('--edges', choices=EDGES, default='split',
                    help='split: vertices are split, no face is lost.  remove: the reference script\'s sequence -- faces removed at edges of more '
                         'than two faces, holes filled, vertices split; how many faces it costs on real reconstructions is unmeasured')
    ap.add_argument('--max_hole_edges', type=int, default=30,
                    help='with --edges remove: fill holes of up to this many edges (0 .. 64; with --fill area 0 .. 128)')
    ap.add_argument('--fill', choices=FILLS, default='fan',
                    help='with --edges remove: fan is the fan of clean.repair; area closes the loops behind the split by their minimum-area '
                         'triangulation (points2surf_amd.holes), which adds no edge of more than two faces')
    ap.add_argument('--dataset', default=None, help='a list of shape names: only these meshes')
    ap.add_argument('--gpu_idx', type=int, default=0)
    opt = ap.parse_args(argv)
    most = 128 if opt.edges == 'remove' and opt.fill == 'area' else 64
    if not 0 <= opt.max_hole_edges <= most:
        ap.error('--max_hole_edges must lie in 0 .. %d' % most)
    device = _engine.select_device(opt.gpu_idx)
    for f in manifold_dir(opt.indir, opt.outdir, edges=opt.edges, max_hole_edges=opt.max_hole_edges, dataset=opt.dataset, device=device,
                          fill=opt.fill):
        print(f)
    print(os.path.join(opt.outdir, REPORT_FILE))
    return 0


if __name__ == '__main__':
    sys.exit(main())
