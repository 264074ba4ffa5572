"""Screened Poisson baseline on the device: an oriented cloud -> mesh without the network, the stage the
reference runs through MeshLab (eval_dataset.py, poisson.mlx: depth 8, pointWeight 4, scale 1.1), through libp2s_hip.so
(p2s_poisson_reconstruct, p2s_poisson_system).  The definition is the project's own -- regular grids, trilinear elements,
a cascade of levels 3 .. depth, Jacobi-preconditioned CG -- and is not pinned against MeshLab.  Torch tensors are
containers only; no CPU fallback.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from . import engine as _engine

INFO = 48
MIN_DEPTH = 3


class Params(ctypes.Structure):
    """mirror of ``p2s_poisson_params_t``"""
    _fields_ = [('depth', ctypes.c_int32), ('max_iters', ctypes.c_int32), ('point_weight', ctypes.c_double),
                ('scale', ctypes.c_double), ('cg_tol', ctypes.c_double)]


def _inputs(points, normals, device):
    if not torch.cuda.is_available():
        raise RuntimeError('points2surf_amd needs a ROCm GPU (gfx950); no CPU fallback exists')
    out = []
    for a in (points, normals):
        if isinstance(a, np.ndarray):
            a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
        out.append(a)
    dev = torch.device(device) if device is not None else (out[0].device if out[0].is_cuda else torch.device('cuda'))
    if dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    p, nrm = (a.to(dev, torch.float32).contiguous() for a in out)
    if p.ndim != 2 or p.shape[1] != 3 or nrm.shape != p.shape:
        raise ValueError('points and normals must both be [n, 3] (got %s, %s)' % (tuple(p.shape), tuple(nrm.shape)))
    return p, nrm, dev


def _report(info, levels):
    """the dict form of info_host: lo [3], h, iso and per level depth, lambda, n_occ, iterations, residual, ms"""
    return dict(lo=[float(info[0]), float(info[1]), float(info[2])], h=float(info[3]), iso=float(info[4]),
                levels=[dict(depth=d, lam=float(info[8 + 5 * (d - MIN_DEPTH)]), n_occ=int(info[9 + 5 * (d - MIN_DEPTH)]),
                             iterations=int(info[10 + 5 * (d - MIN_DEPTH)]), residual=float(info[11 + 5 * (d - MIN_DEPTH)]),
                             ms=float(info[12 + 5 * (d - MIN_DEPTH)])) for d in levels])


def reconstruct(points, normals, depth=8, point_weight=4.0, scale=1.1, cg_tol=1e-3, want_volume=False, want_report=False,
                max_iters=500, device=None):
    """(verts [V, 3] float32, faces [F, 3] int32) device tensors of the Screened Poisson surface of the cloud ``points``
    with the outward ``normals`` (any length); with ``want_volume`` also the volume [R, R, R] float32, R = 2^depth + 1
    (chi - iso, border nodes <= 0, inside > 0); with ``want_report`` also a dict: lo, h (node (i, j, k) lies at
    lo + h (i, j, k)), iso and per level lambda, n_occ, the CG iterations, the final relative residual and milliseconds.
    A level that reaches ``max_iters`` is reported there, not raised."""
    p, nrm, dev = _inputs(points, normals, device)
    lib = _lib.load()
    prm = Params(int(depth), int(max_iters), float(point_weight), float(scale), float(cg_tol))
    n = int(p.shape[0])
    res = (1 << int(depth)) + 1 if MIN_DEPTH <= int(depth) <= 9 else 1
    vol = torch.empty((res, res, res), dtype=torch.float32, device=dev) if want_volume else None
    info = (ctypes.c_double * INFO)()
    nv, nf = ctypes.c_int64(0), ctypes.c_int64(0)
    # room for a smooth surface (about 3 R^2 vertices at most for a shape that fills the box); the exact counts come back
    # either way, a second call only if that was not enough
    cap_v, cap_f = 8 * res * res, 16 * res * res
    with torch.cuda.device(dev):
        for _ in range(2):
            verts = torch.empty((cap_v, 3), dtype=torch.float32, device=dev)
            faces = torch.empty((cap_f, 3), dtype=torch.int32, device=dev)
            rc = lib.p2s_poisson_reconstruct(_engine._ptr(p), _engine._ptr(nrm), n, ctypes.byref(prm), _engine._ptr(vol),
                                             _engine._ptr(verts), cap_v, _engine._ptr(faces), cap_f, ctypes.byref(nv), ctypes.byref(nf),
                                             info, dev.index, _engine._stream_ptr(dev))
            if rc != _lib.P2S_ECAPACITY:
                break
            cap_v, cap_f = max(int(nv.value), 1), max(int(nf.value), 1)
        _lib.check(rc)
    out = (verts[:nv.value], faces[:nf.value]) + ((vol,) if want_volume else ()) + \
        ((_report(info, range(MIN_DEPTH, int(depth) + 1)),) if want_report else ())
    return out


def system(points, normals, level, x=None, depth=None, point_weight=4.0, scale=1.1, device=None):
    """One level's system as the solver sees it: (b [R, R, R], diag(A) [R, R, R], A x or None, report) with R = 2^level + 1
    and ``x`` a [R, R, R] (or flat) float32 vector.  The yardstick of the solver's kernels (tests/poisson_model.py)."""
    p, nrm, dev = _inputs(points, normals, device)
    lib = _lib.load()
    level = int(level)
    prm = Params(int(depth if depth is not None else level), 1, float(point_weight), float(scale), 1e-3)
    res = (1 << level) + 1 if MIN_DEPTH <= level <= 9 else 1
    b = torch.empty((res, res, res), dtype=torch.float32, device=dev)
    diag = torch.empty_like(b)
    xin = ax = None
    if x is not None:
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        xin = x.to(dev, torch.float32).contiguous()
        if xin.numel() != res ** 3:
            raise ValueError('x must hold %d values (got %d)' % (res ** 3, xin.numel()))
        ax = torch.empty_like(b)
    info = (ctypes.c_double * INFO)()
    with torch.cuda.device(dev):
        _lib.check(lib.p2s_poisson_system(_engine._ptr(p), _engine._ptr(nrm), int(p.shape[0]), ctypes.byref(prm), level,
                                          _engine._ptr(xin), _engine._ptr(b), _engine._ptr(ax), _engine._ptr(diag), info, dev.index,
                                          _engine._stream_ptr(dev)))
    return b, diag, ax, _report(info, [level])
