"""Point normals from the cloud alone: the PCA normal of every point's k nearest neighbours and its
orientation along the minimum spanning forest of the kNN graph (Hoppe's propagation, made unique), through libp2s_hip.so
(p2s_normals_estimate, p2s_normals_orient).  What the Screened Poisson baseline needs where no mesh exists.  Torch tensors
are containers only; no CPU fallback.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from . import engine as _engine

INFO = 8
ORIENT = ('mst', 'none')


def _cloud(points, device):
    """(Cloud, owned): a Cloud is used as it is, anything else becomes one that the caller closes"""
    if isinstance(points, _engine.Cloud):
        return points, False
    if isinstance(points, np.ndarray):
        points = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32))
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError('points must be [n, 3] (got %s)' % (tuple(points.shape),))
    if device is None and points.is_cuda:
        device = points.device
    return _engine.Cloud(points, device=device), True


def _report(info):
    return dict(components=int(info[0]), edges=int(info[1]), rounds=int(info[2]), flipped=int(info[3]))


def _orient(cloud, nrm, k, want_report):
    lib = _lib.load()
    out = torch.empty_like(nrm)
    comp = torch.empty((cloud.n,), dtype=torch.int32, device=cloud.device) if want_report else None
    info = (ctypes.c_int64 * INFO)()
    with torch.cuda.device(cloud.device):
        _lib.check(lib.p2s_normals_orient(cloud.handle, int(k), _engine._ptr(nrm), _engine._ptr(out), _engine._ptr(comp), info,
                                          _engine._stream_ptr(cloud.device)))
    if not want_report:
        return out, None
    rep = _report(info)
    rep['component'] = comp
    return out, rep


def estimate(points, k=16, orient='mst', want_report=False, device=None):
    """(normals [n, 3] float32, variation [n] float32) device tensors of the cloud ``points`` ([n, 3] array or tensor, or an
    engine.Cloud): the unit eigenvector of the smallest eigenvalue of the covariance of every point's ``k`` nearest points
    (the point itself included; a neighbourhood of coincident points gives the zero vector) and
    lambda_0 / (lambda_0 + lambda_1 + lambda_2).  ``orient='mst'`` orients the field as ``orient`` does, ``'none'`` leaves
    the signs as the eigen-solver made them.  With ``want_report`` also a dict: k and, when oriented, components, edges,
    rounds, flipped and component [n] int32 (the smallest point id of every point's component)."""
    if orient not in ORIENT:
        raise ValueError('orient must be one of %s (got %r)' % (ORIENT, orient))
    cloud, owned = _cloud(points, device)
    try:
        lib = _lib.load()
        nrm = torch.empty((cloud.n, 3), dtype=torch.float32, device=cloud.device)
        var = torch.empty((cloud.n,), dtype=torch.float32, device=cloud.device)
        with torch.cuda.device(cloud.device):
            _lib.check(lib.p2s_normals_estimate(cloud.handle, int(k), _engine._ptr(nrm), _engine._ptr(var),
                                                _engine._stream_ptr(cloud.device)))
        rep = None
        if orient == 'mst':
            nrm, rep = _orient(cloud, nrm, k, want_report)
    finally:
        if owned:
            cloud.close()
    if not want_report:
        return nrm, var
    return nrm, var, dict(rep or {}, k=int(k))


def orient(points, normals, k=16, want_report=False, device=None):
    """``normals`` [n, 3] of the cloud ``points`` with consistent signs: only sign bits change.  The graph joins every
    point to its ``k`` nearest; the signs spread along its minimum spanning forest under the order (1 - |a . b|, min id,
    max id), flipping where a . b < 0; every component is then turned so that the normal of its highest point (largest z,
    of equal ones the smallest id) does not point down.  With ``want_report`` also the dict of ``estimate``."""
    cloud, owned = _cloud(points, device)
    try:
        if isinstance(normals, np.ndarray):
            normals = torch.from_numpy(np.ascontiguousarray(normals, dtype=np.float32))
        nrm = normals.to(cloud.device, torch.float32).contiguous()
        if tuple(nrm.shape) != (cloud.n, 3):
            raise ValueError('normals must be [%d, 3] (got %s)' % (cloud.n, tuple(nrm.shape)))
        out, rep = _orient(cloud, nrm, k, want_report)
    finally:
        if owned:
            cloud.close()
    return (out, dict(rep, k=int(k))) if want_report else out
