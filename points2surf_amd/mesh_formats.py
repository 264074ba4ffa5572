"""Dependency-free host-side readers for the raw mesh formats the reference converts with trimesh in its
``01_base_meshes_ply`` step (make_dataset.py:42-68: '.off', '.ply', '.obj', '.stl').  File parsing only: every reader
returns (vertices [n, 3] float32, faces [m, 3] int32) exactly as the file states them -- an STL is a triangle soup with
three vertices of its own per face; welding them is the repair's job (points2surf_amd.clean).  Polygons are fanned from
their first vertex.  trimesh is not installed here: UNPINNED.
"""
import os
import struct

import numpy as np

from . import ply as _ply


def _fan(idx, out):
    for j in range(1, len(idx) - 1):
        out.append((idx[0], idx[j], idx[j + 1]))


def _arrays(verts, faces):
    return (np.asarray(verts, dtype=np.float32).reshape(-1, 3), np.asarray(faces, dtype=np.int32).reshape(-1, 3))


def read_off(path):
    """OFF / COFF: header line (the counts may follow on it), '#' comments, one vertex per line (x y z; colours behind
    them are ignored), one face per line ``n i0 .. i(n-1)`` (colours behind them are ignored)"""
    with open(path, 'r') as fh:
        lines = [ln.split('#', 1)[0].split() for ln in fh]
    lines = [ln for ln in lines if ln]
    if not lines or not lines[0][0].upper().endswith('OFF'):
        raise ValueError('%s: not an OFF file' % path)
    counts = lines[0][1:] if len(lines[0]) > 1 else lines[1]
    pos = 1 if len(lines[0]) > 1 else 2
    nv, nf = int(counts[0]), int(counts[1])
    verts = [[float(x) for x in ln[:3]] for ln in lines[pos:pos + nv]]
    faces = []
    for ln in lines[pos + nv:pos + nv + nf]:
        n = int(ln[0])
        _fan([int(t) for t in ln[1:1 + n]], faces)
    if len(verts) != nv or len(lines) < pos + nv + nf:
        raise ValueError('%s: truncated OFF file' % path)
    return _arrays(verts, faces)


def read_obj(path):
    """Wavefront OBJ: ``v x y z`` and ``f`` records only (``i``, ``i/t``, ``i/t/n``, ``i//n``; negative indices count
    from the end); everything else is ignored"""
    verts, faces = [], []
    with open(path, 'r') as fh:
        for line in fh:
            t = line.split()
            if not t:
                continue
            if t[0] == 'v':
                verts.append([float(t[1]), float(t[2]), float(t[3])])
            elif t[0] == 'f':
                idx = []
                for w in t[1:]:
                    i = int(w.split('/', 1)[0])
                    idx.append(i - 1 if i > 0 else len(verts) + i)
                _fan(idx, faces)
    return _arrays(verts, faces)


def read_stl(path):
    """binary (80-byte header, uint32 count, 50 bytes per facet) or ASCII (``vertex x y z``) STL; normals are ignored"""
    with open(path, 'rb') as fh:
        data = fh.read()
    if len(data) >= 84:
        n = struct.unpack_from('<I', data, 80)[0]
        if len(data) == 84 + 50 * n:                  # the size decides: binary files may begin with 'solid' too
            rec = np.frombuffer(data, dtype=np.dtype([('n', '<f4', 3), ('v', '<f4', 9), ('a', '<u2')]), count=n, offset=84)
            return _arrays(rec['v'].reshape(-1, 3), np.arange(3 * n).reshape(n, 3))
    text = data.decode('ascii', 'replace')
    if not text.lstrip().lower().startswith('solid'):
        raise ValueError('%s: neither a binary nor an ASCII STL' % path)
    verts = []
    for line in text.splitlines():
        t = line.split()
        if len(t) == 4 and t[0].lower() == 'vertex':
            verts.append([float(t[1]), float(t[2]), float(t[3])])
    if len(verts) % 3:
        raise ValueError('%s: %d vertex records are no whole number of facets' % (path, len(verts)))
    return _arrays(verts, np.arange(len(verts)).reshape(-1, 3))


READERS = {'.off': read_off, '.obj': read_obj, '.stl': read_stl,
           '.ply': lambda path: _arrays(*_ply.read_ply(path))}


def read_mesh(path):
    ext = os.path.splitext(path)[1].lower()
    if ext not in READERS:
        raise ValueError('%s: unsupported mesh type (one of %s)' % (path, ', '.join(sorted(READERS))))
    return READERS[ext](path)
