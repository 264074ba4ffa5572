"""Ground-truth signed distance to a triangle mesh on the device: what the reference computes with
``trimesh.proximity.signed_distance`` (source/sdf.py:318-348) for the GT file ``05_query_dist/<shape>.npy``
(make_dataset.py:447-474), through libp2s_hip.so (p2s_trimesh_create, p2s_mesh_distance).  Exact point-to-mesh distance
in float64, positive inside like trimesh.  Torch tensors are containers only; no CPU fallback.

``python -m points2surf_amd.gt_sdf --indir DATASET`` writes ``DATASET/05_query_dist`` from ``03_meshes`` and
``05_query_pts``; ``--sign winding`` takes every sign from the generalised winding number (p2s_mesh_winding), which is
defined for open meshes too, where the default ``--sign pseudonormal`` refuses them; ``--sign auto`` checks every mesh for
self-intersections (p2s_mesh_check) and takes the pseudonormal only where it is valid.
"""
import argparse
import ctypes
import os

import numpy as np
import torch

from . import _lib
from . import engine as _engine
from . import ply as _ply
from .file_utils import call_necessary as _call_necessary

METHODS = {'index': 0, 'exhaustive': 1}
WINDING_METHODS = {'tree': 0, 'exhaustive': 1}
SIGNS = ('pseudonormal', 'winding', 'auto')
CHECK_KEYS = ('faces_tested', 'faces_degenerate', 'candidates', 'intersecting', 'coplanar', 'touching', 'duplicate',
              'faces_flagged', 'pairs_inside_component', 'pairs_across_components', 'nonmanifold_vertices', 'pairs_stored')
VOXEL_KEYS = ('inside', 'undecided_columns', 'undecided_voxels', 'fallback', 'tests', 'crossings')
P2S_EINVAL = -1


def winding_rounding(n_faces, terms, n_degenerate=0):
    """the rounding term of the winding bound (include/p2s_hip.h, p2s_mesh_winding): ``terms`` = triangles and dipoles
    added for the query, at most ``n_faces``"""
    return 2.0 ** -53 * n_faces * (terms + n_faces / 256.0 + 32.0) + n_degenerate * 2.0 ** -46 / np.pi


class TriMesh:
    """Device-resident triangle mesh with its distance index (replaces ``trimesh.load`` + the proximity structures of
    ``trimesh.proximity.signed_distance``).  ``verts`` [V, 3], ``faces`` [F, 3]: numpy arrays or tensors."""

    def __init__(self, verts, faces, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError('points2surf_amd needs a ROCm GPU (gfx950); no CPU fallback exists')
        self.lib = _lib.load()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        if isinstance(verts, np.ndarray):
            verts = torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float32))
        if isinstance(faces, np.ndarray):
            faces = torch.from_numpy(np.ascontiguousarray(faces).astype(np.int32))
        v = verts.to(self.device, torch.float32).contiguous()
        f = faces.to(self.device, torch.int32).contiguous()
        if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
            raise ValueError('verts must be [V, 3] and faces [F, 3] (got %s, %s)' % (tuple(v.shape), tuple(f.shape)))
        self.handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.p2s_trimesh_create(_engine._ptr(v), int(v.shape[0]), _engine._ptr(f), int(f.shape[0]),
                                                   self.device.index, _engine._stream_ptr(self.device),
                                                   ctypes.byref(self.handle)))
        self.n_winding = 0
        self.n_verts = int(v.shape[0])

    def info(self):
        """dict: n_faces, closed, inverted, bad_edges (open or non-manifold), grid (cells per axis), tests (point-triangle
        tests of the last indexed distance call), components (of a closed mesh), degenerate (faces under the 2^-90 rule)"""
        a = (ctypes.c_int64 * 8)()
        _lib.check(self.lib.p2s_trimesh_info(self.handle, a))
        return dict(n_faces=int(a[0]), closed=bool(a[1]), inverted=bool(a[2]), bad_edges=int(a[3]), grid=int(a[4]),
                    tests=int(a[5]), components=int(a[6]), degenerate=int(a[7]))

    @property
    def closed(self):
        return self.info()['closed']

    def distance(self, queries, signed=True, method='index', want_face=False, want_closest=False):
        """float64 device tensor [n]: the (signed: positive inside) distance of every query; with ``want_face`` /
        ``want_closest`` also the nearest face [n] int32 / the closest point [n, 3] float64.  ``self.n_winding`` = queries
        of this call whose sign the winding number decided.  ``signed='winding'``: every sign from the generalised
        winding number (inside iff |w| > 0.5), on any mesh, closed or not; ``self.n_winding`` = queries the tree walk left
        undecided, re-decided by the exact sum."""
        q = self._queries(queries)
        n = int(q.shape[0])
        if isinstance(signed, str):
            if signed != 'winding':
                raise ValueError("signed must be True, False or 'winding' (got %r)" % (signed,))
            mode = 2
        else:
            mode = int(bool(signed))
        dist = torch.empty((n,), dtype=torch.float64, device=self.device)
        face = torch.empty((n,), dtype=torch.int32, device=self.device) if want_face else None
        closest = torch.empty((n, 3), dtype=torch.float64, device=self.device) if want_closest else None
        nw = ctypes.c_int64(0)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.p2s_mesh_distance(self.handle, _engine._ptr(q), n, mode, METHODS[method],
                                                  _engine._ptr(dist), _engine._ptr(face), _engine._ptr(closest),
                                                  ctypes.byref(nw), _engine._stream_ptr(self.device)))
        self.n_winding = int(nw.value)
        out = (dist,) + ((face,) if want_face else ()) + ((closest,) if want_closest else ())
        return out[0] if len(out) == 1 else out

    def _queries(self, queries):
        if self.handle is None:
            raise RuntimeError('TriMesh is closed')
        if isinstance(queries, np.ndarray):
            queries = torch.from_numpy(np.ascontiguousarray(queries, dtype=np.float32))
        q = queries.to(self.device, torch.float32).contiguous()
        if q.ndim != 2 or q.shape[1] != 3:
            raise ValueError('queries must be [n, 3] (got %s)' % (tuple(q.shape),))
        return q

    def winding(self, queries, method='tree', tau=2 ** -10, want_bound=False, want_stats=False):
        """float64 device tensor [n]: the generalised winding number of every query (Jacobson et al. 2013; defined for open
        meshes).  ``method='tree'``: far octree nodes as dipoles, their certified error bounds summing to at most ``tau``
        per query; a query with | |w| - 0.5 | within its bound gets the exact sum.  ``'exhaustive'``: the exact sum for
        every query.  ``want_bound``: also the bound [n] (0 where exact); ``want_stats``: also a dict accepted (nodes),
        triangles (evaluated), redecided (queries)."""
        q = self._queries(queries)
        n = int(q.shape[0])
        w = torch.empty((n,), dtype=torch.float64, device=self.device)
        err = torch.empty((n,), dtype=torch.float64, device=self.device) if want_bound else None
        st = (ctypes.c_int64 * 4)()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.p2s_mesh_winding(self.handle, _engine._ptr(q), n, WINDING_METHODS[method], float(tau),
                                                 _engine._ptr(w), _engine._ptr(err), st, _engine._stream_ptr(self.device)))
        out = (w,) + ((err,) if want_bound else ()) + \
            ((dict(accepted=int(st[0]), triangles=int(st[1]), redecided=int(st[2])),) if want_stats else ())
        return out[0] if len(out) == 1 else out

    def check(self, method='index', want_pairs=False, want_flags=False, cap_pairs=None):
        """Self-intersections and non-manifold vertices (p2s_mesh_check): the report as a dict (CHECK_KEYS;
        pairs_inside_component / pairs_across_components are -1 on a mesh that is not closed).  ``want_pairs``: also the
        pairs [n, 2] int32, (f, g) with f < g ascending, and their classes [n] uint8 (1 intersecting, 2 coplanar,
        3 touching); ``want_flags``: also the face flags [F] uint8 (bits 1 / 2 / 4: in an intersecting / coplanar / touching
        pair, 8: degenerate) and the vertex flags [V] uint8 (1: not manifold).  ``cap_pairs`` sizes the pair buffers
        (default: a first call counts); too small a value raises P2SError with the needed count in its message."""
        if self.handle is None:
            raise RuntimeError('TriMesh is closed')
        rep = (ctypes.c_int64 * 16)()
        stream = _engine._stream_ptr(self.device)

        def call(cap, pairs, cls, ff, vf):
            with torch.cuda.device(self.device):
                return self.lib.p2s_mesh_check(self.handle, METHODS[method], int(cap), _engine._ptr(pairs), _engine._ptr(cls),
                                               _engine._ptr(ff), _engine._ptr(vf), rep, stream)
        ff = vf = None
        if want_flags:
            n_faces = self.info()['n_faces']
            ff = torch.empty((n_faces,), dtype=torch.uint8, device=self.device)
            vf = torch.empty((self.n_verts,), dtype=torch.uint8, device=self.device)
        if not want_pairs:
            _lib.check(call(0, None, None, ff, vf))
            out = (dict(zip(CHECK_KEYS, (int(x) for x in rep))),)
        else:
            if cap_pairs is None:
                _lib.check(call(0, None, None, None, None))
                cap_pairs = int(rep[11])
            pairs = torch.empty((max(int(cap_pairs), 1), 2), dtype=torch.int32, device=self.device)
            cls = torch.empty((max(int(cap_pairs), 1),), dtype=torch.uint8, device=self.device)
            _lib.check(call(cap_pairs, pairs, cls, ff, vf))
            n = int(rep[11])
            out = (dict(zip(CHECK_KEYS, (int(x) for x in rep))), pairs[:n], cls[:n])
        out = out + ((ff, vf) if want_flags else ())
        return out[0] if len(out) == 1 else out

    def voxelize(self, res, method='index', max_fallback=None, want_flags=False, want_report=False):
        """Occupancy of this CLOSED mesh on the volume's grid (p2s_mesh_voxelize): ``occ`` [res, res, res] uint8 device
        tensor, x-major with z fastest, 1 where the voxel centre (the float32 nearest to ((i + 0.5) / res) * 2 - 1) lies
        inside (winding number != 0).  Voxels whose column meets an edge, a vertex or an edge-on face within rounding go
        to the exact winding sum, O(faces) each: more than ``max_fallback`` of them (default 4 * res * res) raises P2SError
        with the code P2S_ECAPACITY.  ``want_flags``: also [res, res, res] uint8, 1 for those voxels; ``want_report``:
        also a dict (VOXEL_KEYS).  A mesh that is not closed raises P2SError (P2S_EINVAL)."""
        if self.handle is None:
            raise RuntimeError('TriMesh is closed')
        res = int(res)
        if max_fallback is None:
            max_fallback = 4 * res * res
        shape = (max(res, 0),) * 3
        occ = torch.empty(shape, dtype=torch.uint8, device=self.device)
        flags = torch.empty(shape, dtype=torch.uint8, device=self.device) if want_flags else None
        rep = (ctypes.c_int64 * 8)()
        with torch.cuda.device(self.device):
            rc = self.lib.p2s_mesh_voxelize(self.handle, res, METHODS[method], int(max_fallback), _engine._ptr(occ),
                                            _engine._ptr(flags), rep, _engine._stream_ptr(self.device))
        self.voxel_report = dict(zip(VOXEL_KEYS, (int(x) for x in rep)))
        _lib.check(rc)
        out = (occ,) + ((flags,) if want_flags else ()) + ((self.voxel_report,) if want_report else ())
        return out[0] if len(out) == 1 else out

    def close(self):
        if getattr(self, 'handle', None) is not None and self.handle:
            self.lib.p2s_trimesh_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def auto_sign(mesh):
    """what ``sign='auto'`` uses for ``mesh``: 'pseudonormal' when it is closed and no intersecting or coplanar pair of
    faces lies inside one component (pairs across components are signed component by component anyway, and a mesh of more
    than 16 components by the winding number), else 'winding'.  Returns (sign, the report of mesh.check())."""
    rep = mesh.check()
    return ('pseudonormal' if mesh.closed and rep['pairs_inside_component'] == 0 else 'winding'), rep


def query_dist(mesh, query_pts, sign='pseudonormal'):
    """make_dataset.py:464-474: the signed distances of ``query_pts`` with NaN -> 0, inf -> 1, clamped to [-1, 1], as a
    float32 numpy array (the content of 05_query_dist/<shape>.npy)"""
    if sign not in SIGNS:
        raise ValueError('sign must be one of %s (got %r)' % (SIGNS, sign))
    if sign == 'auto':
        sign = auto_sign(mesh)[0]
    d = mesh.distance(query_pts, signed='winding' if sign == 'winding' else True)
    d = torch.nan_to_num(d, nan=0.0, posinf=1.0, neginf=1.0).clamp_(-1.0, 1.0)
    return d.to(torch.float32).cpu().numpy()


def load_mesh(path, device=None):
    v, f = _ply.read_ply(path)
    return TriMesh(np.asarray(v, dtype=np.float32), np.asarray(f), device=device)


def write_query_dist_dir(mesh_dir, query_pts_dir, out_dir, device=None, sign='pseudonormal'):
    """05_query_dist/<mesh>.npy for every 03_meshes/<mesh> that has 05_query_pts/<mesh>.npy (get_query_pts_dist_ms of
    make_dataset.py:481-530 without the query-point generation); files that are up to date are skipped.  Returns the
    list of files written.  ``sign='pseudonormal'`` refuses a mesh that is not closed; ``'winding'`` signs any mesh;
    ``'auto'`` takes the pseudonormal where auto_sign allows it and prints one line per mesh it switched to the winding
    number."""
    if sign not in SIGNS:
        raise ValueError('sign must be one of %s (got %r)' % (SIGNS, sign))
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for name in sorted(os.listdir(mesh_dir)):
        f_mesh = os.path.join(mesh_dir, name)
        f_pts = os.path.join(query_pts_dir, name + '.npy')
        f_out = os.path.join(out_dir, name + '.npy')
        if not os.path.isfile(f_mesh) or not os.path.isfile(f_pts):
            continue
        if not _call_necessary([f_mesh, f_pts], [f_out]):
            continue
        mesh = load_mesh(f_mesh, device=device)
        try:
            if sign == 'pseudonormal' and not mesh.closed:
                raise ValueError('%s is not closed (%d open or non-manifold edges): no signed distance'
                                 % (f_mesh, mesh.info()['bad_edges']))
            use = sign
            if sign == 'auto':
                use, rep = auto_sign(mesh)
                if use == 'winding':
                    print('%s: signed by the winding number (%s)' % (f_mesh, '%d intersecting and %d coplanar pairs of faces inside '
                          'one component' % (rep['intersecting'], rep['coplanar']) if mesh.closed else 'not closed'))
            np.save(f_out, query_dist(mesh, np.load(f_pts).astype(np.float32), sign=use))
        finally:
            mesh.close()
        written.append(f_out)
    return written


def main(argv=None):
    ap = argparse.ArgumentParser(description='write DATASET/05_query_dist from 03_meshes and 05_query_pts')
    ap.add_argument('--indir', required=True)
    ap.add_argument('--sign', choices=SIGNS, default='pseudonormal',
                    help='pseudonormal: closed meshes only (the default); winding: the generalised winding number, open meshes too; '
                    'auto: the pseudonormal unless the mesh is open or intersects itself inside one component')
    opt = ap.parse_args(argv)
    for f in write_query_dist_dir(os.path.join(opt.indir, '03_meshes'), os.path.join(opt.indir, '05_query_pts'),
                                  os.path.join(opt.indir, '05_query_dist'), sign=opt.sign):
        print(f)


if __name__ == '__main__':
    main()
