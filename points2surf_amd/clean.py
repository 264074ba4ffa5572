"""Repair and normalisation of raw triangle meshes on the device: the stages ``01_base_meshes_ply``,
``02_meshes_cleaned`` and ``03_meshes`` of the reference's make_dataset.py (convert_meshes :42-68, _clean_mesh :383-413,
_normalize_mesh :71-88), which call trimesh.  The repair (weld, drop collapsed and duplicate faces, orient, fill small
holes, fix inversion, compact) and the normalisation run in libp2s_hip.so (p2s_mesh_repair, p2s_mesh_normalize); their
definitions are in include/p2s_hip.h.  This is the project's own definition of the stage -- UNPINNED: trimesh absent.
The weld joins vertices with EQUAL float32 coordinates (no rounding to a tolerance: trimesh's 1e-8 is below the float32
spacing over most of the unit cube).  Torch tensors are containers only; no CPU fallback.

``python -m points2surf_amd.clean --indir DATASET [--stage convert|clean|normalize|all|check] [--max_faces N]
[--no_enforce_solid] [--max_hole_edges K]``.  ``--stage check`` (not part of ``all``) reads ``03_meshes`` and writes
``DATASET/check_report.csv``: the self-intersections and non-manifold vertices of every mesh (p2s_mesh_check), which
the verdict "a volume" of the repair does not see.
"""
import argparse
import csv
import ctypes
import os

import numpy as np
import torch

from . import _lib
from . import engine as _engine
from . import mesh_formats as _formats
from . import ply as _ply
from .file_utils import call_necessary as _call_necessary

P2S_EFLAT = -7
REPORT_KEYS = ('verts_in', 'faces_in', 'verts_out', 'faces_out', 'verts_welded', 'faces_collapsed', 'faces_duplicate',
               'faces_degenerate', 'faces_flipped', 'components', 'components_unorientable', 'components_inverted',
               'holes_filled', 'faces_added', 'holes_left', 'boundary_edges_left', 'nonmanifold_edges', 'watertight',
               'winding_consistent', 'is_volume')
DIR_BASE, DIR_PLY, DIR_CLEANED, DIR_MESHES = '00_base_meshes', '01_base_meshes_ply', '02_meshes_cleaned', '03_meshes'
REPORT_FILE = 'clean_report.csv'
CHECK_REPORT_FILE = 'check_report.csv'


class FlatMesh(ValueError):
    """the bounding box has a zero extent on an axis: the mesh cannot be normalised (the reference skips it)"""


def report_dict(a):
    """the int64[16] report of p2s_mesh_repair as a dict (REPORT_KEYS)"""
    a = [int(x) for x in a]
    m = (1 << 32) - 1
    return dict(verts_in=a[0] & m, faces_in=a[0] >> 32, verts_out=a[1], faces_out=a[2], verts_welded=a[3],
                faces_collapsed=a[4], faces_duplicate=a[5], faces_degenerate=a[6], faces_flipped=a[7], components=a[8],
                components_unorientable=a[9], components_inverted=a[10], holes_filled=a[11], faces_added=a[12],
                holes_left=a[13], boundary_edges_left=a[14] & m, nonmanifold_edges=a[14] >> 32, watertight=a[15] & 1,
                winding_consistent=(a[15] >> 1) & 1, is_volume=(a[15] >> 2) & 1)


def _device(device):
    if not torch.cuda.is_available():
        raise RuntimeError('points2surf_amd needs a ROCm GPU (gfx950); no CPU fallback exists')
    d = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    return torch.device('cuda', torch.cuda.current_device()) if d.index is None else d


def _verts(verts, dev):
    if isinstance(verts, np.ndarray):
        verts = torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float32))
    v = verts.to(dev, torch.float32).contiguous()
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError('verts must be [V, 3] (got %s)' % (tuple(v.shape),))
    return v


def repair(verts, faces, max_hole_edges=4, device=None, cap_verts=None, cap_faces=None):
    """``verts`` [V, 3] float32, ``faces`` [F, 3] int32 (numpy arrays or tensors) -> (verts, faces, face_src, report):
    device tensors [V', 3] float32, [F', 3] int32, [F'] int32 (the input face id, -1 for an added face) and the report
    dict (REPORT_KEYS).  ``cap_verts`` / ``cap_faces`` size the output buffers (default: V and 4 F, which always
    suffice)."""
    dev = _device(device)
    lib = _lib.load()
    v = _verts(verts, dev)
    if isinstance(faces, np.ndarray):
        faces = torch.from_numpy(np.ascontiguousarray(faces).astype(np.int32))
    f = faces.to(dev, torch.int32).contiguous()
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError('faces must be [F, 3] (got %s)' % (tuple(f.shape),))
    V, F = int(v.shape[0]), int(f.shape[0])
    cv = V if cap_verts is None else int(cap_verts)
    cf = 4 * F if cap_faces is None else int(cap_faces)
    vo = torch.empty((cv, 3), dtype=torch.float32, device=dev)
    fo = torch.empty((cf, 3), dtype=torch.int32, device=dev)
    so = torch.empty((cf,), dtype=torch.int32, device=dev)
    rep = (ctypes.c_int64 * 16)()

    def ptr(t):
        return _engine._ptr(t) if t.numel() else None

    with torch.cuda.device(dev):
        _lib.check(lib.p2s_mesh_repair(ptr(v), V, ptr(f), F, int(max_hole_edges), ptr(vo), cv, ptr(fo), ptr(so), cf, rep,
                                       dev.index, _engine._stream_ptr(dev)))
    r = report_dict(rep)
    return vo[:r['verts_out']], fo[:r['faces_out']], so[:r['faces_out']], r


def normalize(verts, device=None):
    """_normalize_mesh: centre of the bounding box to the origin, largest extent to 1, computed in float64 and rounded
    once to float32.  Raises FlatMesh for a zero extent on an axis."""
    dev = _device(device)
    lib = _lib.load()
    v = _verts(verts, dev)
    out = torch.empty_like(v)
    with torch.cuda.device(dev):
        rc = lib.p2s_mesh_normalize(_engine._ptr(v) if v.numel() else None, int(v.shape[0]), _engine._ptr(out) if v.numel() else None,
                                    None, dev.index, _engine._stream_ptr(dev))
    if rc == P2S_EFLAT:
        raise FlatMesh('the bounding box has a zero extent on an axis')
    _lib.check(rc)
    return out


def clean_mesh_file(file_in, file_out, num_max_faces=None, enforce_solid=True, max_hole_edges=4, device=None):
    """_clean_mesh: repair ``file_in`` and write it to ``file_out`` unless it is rejected -- with ``enforce_solid`` when it
    is not a volume (watertight, consistent winding, positive volume), and when it has ``num_max_faces`` faces or more.
    Returns (report dict, verdict): 'written', or the reason for the rejection."""
    v, f = _formats.read_mesh(file_in)
    vo, fo, _, rep = repair(v, f, max_hole_edges=max_hole_edges, device=device)
    if enforce_solid and not rep['watertight']:
        verdict = 'rejected: not watertight (%d boundary edges, %d edges of more than two faces)' % (
            rep['boundary_edges_left'], rep['nonmanifold_edges'])
    elif enforce_solid and not rep['winding_consistent']:
        verdict = 'rejected: winding not consistent (%d unorientable components)' % rep['components_unorientable']
    elif enforce_solid and not rep['is_volume']:
        verdict = 'rejected: not a volume (the signed volume is not positive)'
    elif num_max_faces is not None and rep['faces_out'] >= num_max_faces:
        verdict = 'rejected: %d faces, the limit is %d' % (rep['faces_out'], num_max_faces)
    elif rep['faces_out'] == 0:
        verdict = 'rejected: no face left'
    else:
        os.makedirs(os.path.dirname(os.path.abspath(file_out)), exist_ok=True)
        _ply.write_ply(file_out, vo.cpu().numpy(), fo.cpu().numpy())
        verdict = 'written'
    return rep, verdict


def _files(directory):
    return [n for n in sorted(os.listdir(directory)) if os.path.isfile(os.path.join(directory, n))] if os.path.isdir(directory) else []


def convert_meshes_dir(indir):
    """convert_meshes: every .off / .ply / .obj / .stl under ``indir/00_base_meshes`` as ``01_base_meshes_ply/<stem>.ply``,
    vertices and faces as the file states them.  Returns the files written."""
    written = []
    out_dir = os.path.join(indir, DIR_PLY)
    os.makedirs(out_dir, exist_ok=True)
    for root, _, names in sorted(os.walk(os.path.join(indir, DIR_BASE))):
        for name in sorted(names):
            if os.path.splitext(name)[1].lower() not in _formats.READERS:
                continue
            f_in, f_out = os.path.join(root, name), os.path.join(out_dir, name[:-4] + '.ply')
            if not _call_necessary([f_in], [f_out]):
                continue
            v, f = _formats.read_mesh(f_in)
            _ply.write_ply(f_out, v, f)
            written.append(f_out)
    return written


def clean_meshes_dir(indir, num_max_faces=None, enforce_solid=True, max_hole_edges=4, device=None):
    """clean_meshes: ``02_meshes_cleaned/<name>`` for every ``01_base_meshes_ply/<name>`` that passes, and
    ``02_meshes_cleaned/clean_report.csv`` with one row per mesh: the report and the verdict.  Returns the files written."""
    in_dir, out_dir = os.path.join(indir, DIR_PLY), os.path.join(indir, DIR_CLEANED)
    os.makedirs(out_dir, exist_ok=True)
    written, rows = [], []
    for name in _files(in_dir):
        f_out = os.path.join(out_dir, name)
        rep, verdict = clean_mesh_file(os.path.join(in_dir, name), f_out, num_max_faces, enforce_solid, max_hole_edges, device)
        rows.append([name] + [rep[k] for k in REPORT_KEYS] + [verdict])
        if verdict == 'written':
            written.append(f_out)
        elif os.path.isfile(f_out):
            os.remove(f_out)                          # a mesh rejected now is not left over from an earlier run
    with open(os.path.join(out_dir, REPORT_FILE), 'w', newline='') as fh:
        w = csv.writer(fh)
        w.writerow(['mesh'] + list(REPORT_KEYS) + ['verdict'])
        w.writerows(rows)
    return written


def normalize_meshes_dir(indir, device=None):
    """normalize_meshes: ``03_meshes/<name>`` for every ``02_meshes_cleaned/<name>``; a mesh with a zero extent is skipped
    as the reference skips it.  Returns the files written."""
    in_dir, out_dir = os.path.join(indir, DIR_CLEANED), os.path.join(indir, DIR_MESHES)
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for name in _files(in_dir):
        if not name.lower().endswith('.ply'):
            continue
        f_in, f_out = os.path.join(in_dir, name), os.path.join(out_dir, name)
        if not _call_necessary([f_in], [f_out]):
            continue
        v, f = _formats.read_mesh(f_in)
        try:
            vn = normalize(v, device=device)
        except FlatMesh:
            print('WARNING: {} has a zero extent and is skipped'.format(f_in))
            continue
        _ply.write_ply(f_out, vn.cpu().numpy(), f)
        written.append(f_out)
    return written


def check_verdict(rep):
    """'self-intersecting' (an intersecting or coplanar pair of faces), else 'non-manifold' (a vertex whose faces are not
    one fan), else 'embedded'; touching pairs are only counted"""
    if rep['intersecting'] + rep['coplanar'] > 0:
        return 'self-intersecting'
    return 'non-manifold' if rep['nonmanifold_vertices'] > 0 else 'embedded'


def check_meshes_dir(indir, device=None):
    """``indir/check_report.csv`` (beside the stage directories, which hold meshes only): one row per ``03_meshes/*.ply`` with the counts of TriMesh.check and the verdict.
    Returns the rows."""
    from . import gt_sdf as _gt
    in_dir = os.path.join(indir, DIR_MESHES)
    rows = []
    for name in _files(in_dir):
        if not name.lower().endswith('.ply'):
            continue
        mesh = _gt.load_mesh(os.path.join(in_dir, name), device=device)
        try:
            rep = mesh.check()
        finally:
            mesh.close()
        rows.append([name] + [rep[k] for k in _gt.CHECK_KEYS] + [check_verdict(rep)])
    with open(os.path.join(indir, CHECK_REPORT_FILE), 'w', newline='') as fh:
        w = csv.writer(fh)
        w.writerow(['mesh'] + list(_gt.CHECK_KEYS) + ['verdict'])
        w.writerows(rows)
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description='write DATASET/01_base_meshes_ply, 02_meshes_cleaned and 03_meshes from 00_base_meshes')
    ap.add_argument('--indir', required=True)
    ap.add_argument('--stage', choices=('convert', 'clean', 'normalize', 'all', 'check'), default='all',
                    help='check (not part of all): DATASET/check_report.csv from 03_meshes, self-intersections and non-manifold vertices')
    ap.add_argument('--max_faces', type=int, default=None, help='reject meshes with this many faces or more')
    ap.add_argument('--no_enforce_solid', action='store_true', help='write meshes that are not a volume too')
    ap.add_argument('--max_hole_edges', type=int, default=4, help='fill holes of at most this many edges (0..64)')
    opt = ap.parse_args(argv)
    files = []
    if opt.stage in ('convert', 'all'):
        files += convert_meshes_dir(opt.indir)
    if opt.stage in ('clean', 'all'):
        files += clean_meshes_dir(opt.indir, opt.max_faces, not opt.no_enforce_solid, opt.max_hole_edges)
    if opt.stage in ('normalize', 'all'):
        files += normalize_meshes_dir(opt.indir)
    if opt.stage == 'check':
        check_meshes_dir(opt.indir)
        files.append(os.path.join(opt.indir, CHECK_REPORT_FILE))
    for f in files:
        print(f)


if __name__ == '__main__':
    main()
