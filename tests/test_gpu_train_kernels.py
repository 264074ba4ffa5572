"""The training step's generic kernels, one at a time, against float64 numpy (csrc/p2s_train.hip through the test hooks
p2s_debug_train_linear and p2s_debug_train_bn, which run the trainer's own linear_fwd / linear_bwd / colsum / batch-norm
launches on caller-supplied shapes).  tests/test_gpu_train.py checks the same kernels through ~30 stacked layers with a
per-tensor L2 gate; a wrong element at a tile edge, a lost slab or a dropped k pair can pass such a gate, and the network's
layer sizes never reach the N and K guards or the split-slab paths at all.

EXACT CASES.  X, W, b, dY (and the pre-filled dX) are integers from {-2 .. 2} stored as float32.  Every product is at most
4 and every sum at most 4 * 300001 + 2 < 2^24 in magnitude, so every partial sum in any order is an integer that float32
holds exactly: Y, dX, dW and db must equal the float64 result bit for bit, whatever the tiling, the k pairing, the four
accumulators or the slab split.

SENTINELS.  Every output is allocated with TAIL = 4096 floats behind it; the output and the tail are filled with one bit
pattern (a finite -3.3e38 that no case can produce).  After the call no output element may still hold it and every tail
element must.  W / b and dW / db follow the trainer's flat layout (the bias at an offset behind the weight); the tests
leave a TAIL-sized gap between the two, so dW has sentinels behind it as well.

REAL-VALUED GEMM CASES.  |dev - f64| <= (Kred + 8) * 2^-24 * (|A| . |B|) per element: the forward bound of a float32 dot
product of length Kred in any order; 8 covers the combine of the four accumulators and the bias add.  With accum = 1 the
pre-filled dX is one more term of the sum: Kred + 1 terms, and |dX0| joins the magnitude.  db is summed in double and
rounded once: |dev - f64| <= 2^-24 |db| + (M + 4) * 2^-53 * sum|dY|.

BATCH-NORM BOUNDS (u = 2^-24, v = 2^-53, eps = 1e-5; the reference is torch.nn.BatchNorm1d in train mode restated in
float64 with the two-pass variance; S1 = mean|y|, S2 = mean(y^2) per channel).  The kernel sums y and y^2 in double
(y^2 is exact in double) over M terms in a fixed order and forms var = E[y^2] - mean^2:
  dmean = (M + 4) v S1                      sum of M doubles in any order, one division
  em    = u |mean| + dmean                  mean stored as float32
  dvar  = 4 (M + 4) v S2                    (M + 2) v S2 for E[y^2]; 2 |mean| dmean + v mean^2 <= (2 M + 9) v S2 for mean^2
                                            (|mean| <= S1, S1^2 <= S2); v S2 for the subtraction: (3 M + 12) v S2 in all
  invstd in [1 / sqrt(var + eps + dvar), 1 / sqrt(var + eps - dvar)] (dvar < eps is asserted), widened by u + 4 v for the
  float32 store and the double sqrt / division; einv is the larger distance to the float64 value.  A clamp of a negative
  variance to 0 only moves towards the reference, whose variance is >= 0.
  pending variance: (dvar + (u + 4 v) (var + dvar)) M / (M - 1)
  xhat = (y - mean) invstd in float32:      exh = (em inv_hi + |y - mean| einv) (1 + 2 u) + 2 u |xhat|
  z = xhat gamma + beta:                    bz = |gamma| exh + 2 u |xhat gamma| + u |z|;  ReLU does not increase a distance
  d beta  = sum dz in double, stored once:  (M + 4) v sum|dz| + u |d beta|
  d gamma = sum dz xhat (exact products of two float32 in double): sum|dz| exh + (M + 4) v sum|dz xhat| + u |d gamma|
  dL/dy = gamma invstd (dz - m1 - xhat m2), m1 = d beta / M, m2 = d gamma / M, five float32 roundings:
      einner = e(d beta) / M + exh |m2| + (|xhat| + exh) e(d gamma) / M + 3 u (|dz| + |m1| + |xhat m2|)
      edy    = |gamma| (inv_hi einner + einv |inner|) + 3 u |dL/dy|
Every bound is multiplied by 1.001 for the products of two error terms (each at most 2^-20 of a first-order term here).
For the channel with mean 100 and deviation 0.01 at M = 131073: S2 = 1e4, dvar = 5.8e-7 against var + eps = 1.1e-4, so
invstd is known to 0.27 % even in the worst case of the bound: forming E[y^2] - mean^2 in double is safe there, and the
float32 rounding of the stored mean (u * 100 * invstd = 5.7e-4 on xhat) is what dominates that channel's bz.

RELU MASK.  Where the float64 pre-activation lies within bz of zero the two precisions may mask differently; the test sets
dz = 0 at those positions of its INPUT (decided from the float64 forward alone), so either mask gives the same gradient.
The exception is the exact-zero channel: y in {-1, 0, 1} with as many +1 as -1, gamma = 0.75, beta = 0.  Its sum is an
exact 0 in double, the stored mean is 0, and 0 * invstd * gamma + 0 = 0 exactly: z must be an exact zero on the rows with
y = 0, and with dz != 0 there the mask !(z > 0) must remove it (a kernel that masks with z < 0 fails by |gamma invstd dz|).
"""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu

TAIL = 4096
SENT = np.uint32(0xFF7A5A5A)            # finite float32 -3.3e38: not a result of any case
U = 2.0 ** -24
V = 2.0 ** -53
EPS = 1e-5
SLACK = 1.001


@pytest.fixture(scope='module')
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    torch.cuda.set_device(0)
    return torch


# ---------------------------------------------------------------------------------------------------------------------
# buffers with sentinels
# ---------------------------------------------------------------------------------------------------------------------
def _sent_buf(torch, n):
    t = torch.empty(n, dtype=torch.float32, device='cuda')
    t.view(torch.int32).fill_(int(np.array([SENT]).view(np.int32)[0]))
    return t


def _put(t, off, a):
    import torch
    a = np.ascontiguousarray(a, np.float32).ravel()
    t[off:off + a.size] = torch.from_numpy(a).cuda()


def _take(t, off, shape, what, written=True):
    """the output at t[off : off + prod(shape)]: every element overwritten, the TAIL floats behind it untouched"""
    n = int(np.prod(shape))
    h = t[off:off + n + TAIL].cpu().numpy().view(np.uint32)
    assert h.size == n + TAIL
    assert (h[n:] == SENT).all(), '%s: %d sentinel floats behind the output were overwritten' % (what, int((h[n:] != SENT).sum()))
    if written:
        assert (h[:n] != SENT).all(), '%s: %d of %d output elements were never written' % (what, int((h[:n] == SENT).sum()), n)
    return h[:n].view(np.float32).reshape(shape).copy()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def run_linear(torch, X, W, b, dY, accum=0, dX0=None):
    """p2s_debug_train_linear -> dict(Y, dX, dW, db), sentinels checked"""
    from points2surf_amd import _lib
    lib = _lib.load()
    M, K = X.shape
    N = W.shape[0]
    assert W.shape == (N, K) and b.shape == (N,) and dY.shape == (M, N)
    boff = N * K + TAIL
    params = _sent_buf(torch, boff + N)
    _put(params, 0, W)
    _put(params, boff, b)
    grads = _sent_buf(torch, boff + N + TAIL)
    x = torch.from_numpy(np.ascontiguousarray(X, np.float32)).cuda()
    dy = torch.from_numpy(np.ascontiguousarray(dY, np.float32)).cuda()
    y = _sent_buf(torch, M * N + TAIL)
    dx = _sent_buf(torch, M * K + TAIL)
    if accum:
        _put(dx, 0, dX0)
    torch.cuda.synchronize()
    _lib.check(lib.p2s_debug_train_linear(_ptr(x), _ptr(params), boff, _ptr(dy), _ptr(y), _ptr(dx), _ptr(grads), M, N, K,
                                          int(accum), None))
    what = 'M %d N %d K %d accum %d' % (M, N, K, accum)
    return dict(Y=_take(y, 0, (M, N), what + ' Y'), dX=_take(dx, 0, (M, K), what + ' dX', written=not accum),
                dW=_take(grads, 0, (N, K), what + ' dW'), db=_take(grads, boff, (N,), what + ' db'))


def ref_linear(X, W, b, dY, dX0=None):
    X, W, b, dY = (np.asarray(a, np.float64) for a in (X, W, b, dY))
    dX = dY @ W
    if dX0 is not None:
        dX = dX + np.asarray(dX0, np.float64)
    return dict(Y=X @ W.T + b, dX=dX, dW=dY.T @ X, db=dY.sum(axis=0))


def _ints(rng, *shape):
    return rng.integers(-2, 3, shape).astype(np.float32)


def _exact_case(torch, M, N, K, accum, seed=0):
    rng = np.random.default_rng([seed, M, N, K, accum])
    X, W, b, dY = _ints(rng, M, K), _ints(rng, N, K), _ints(rng, N), _ints(rng, M, N)
    dX0 = _ints(rng, M, K) if accum else None
    ref = ref_linear(X, W, b, dY, dX0)
    assert max(np.abs(v).max() for v in ref.values()) < 2 ** 24
    dev = run_linear(torch, X, W, b, dY, accum, dX0)
    for k, v in ref.items():
        want = v.astype(np.float32)
        assert (want.astype(np.float64) == v).all()
        # +0 and -0 are the same sum; nothing else may differ in a single bit
        bad = np.argwhere((dev[k].view(np.uint32) != want.view(np.uint32)) & ~((dev[k] == 0) & (want == 0)))
        first = tuple(bad[0]) if len(bad) else None
        assert first is None, 'M %d N %d K %d accum %d: %s differs at %d elements, first %s: device %r, exact %r' % (
            M, N, K, accum, k, len(bad), first, dev[k][first], want[first])


# ---------------------------------------------------------------------------------------------------------------------
# the GEMM, the K = 3 path, the bias sums: tile edges
# ---------------------------------------------------------------------------------------------------------------------
EDGE_M = [1, 31, 32, 33, 63, 64, 65, 129]
EDGE_N = [1, 2, 31, 33, 64, 65]
EDGE_K = [1, 2, 3, 5, 31, 32, 33, 63, 65]
FULL_CROSS_M = (1, 33, 65)


def _edge_nk(M):
    if M in FULL_CROSS_M:
        return [(N, K) for N in EDGE_N for K in EDGE_K]
    s = EDGE_M.index(M)                 # a diagonal through N x K, shifted per M: every K, every N
    return [(EDGE_N[(i + s) % len(EDGE_N)], K) for i, K in enumerate(EDGE_K)]


def test_the_edge_shapes_cover_every_value():
    for M in EDGE_M:
        nk = _edge_nk(M)
        assert {k for _, k in nk} == set(EDGE_K) and ({n for n, _ in nk} == set(EDGE_N))
    assert 100 <= 2 * sum(len(_edge_nk(M)) for M in EDGE_M) <= 500


@pytest.mark.parametrize('accum', [0, 1])
@pytest.mark.parametrize('M', EDGE_M)
def test_linear_tile_edges_exact(M, accum, torch_cuda):
    for N, K in _edge_nk(M):
        _exact_case(torch_cuda, M, N, K, accum)


# ---------------------------------------------------------------------------------------------------------------------
# dW row slabs (2048 rows each, at most 128), db / CS_LIN3 column-sum slabs (256 rows each, at most 512)
# ---------------------------------------------------------------------------------------------------------------------
SLAB_M = [2047, 2048, 2049, 4097, 262144, 262145, 300001]


@pytest.mark.parametrize('K', [8, 3])
@pytest.mark.parametrize('M', SLAB_M + [131073])
def test_weight_gradient_slab_edges_exact(M, K, torch_cuda):
    _exact_case(torch_cuda, M, 8, K, 0)


@pytest.mark.parametrize('M,N,K', [(2049, 65, 33), (4097, 33, 65)])
def test_weight_gradient_slabs_with_partial_tiles_exact(M, N, K, torch_cuda):
    """the slab stride in the partials is N * K: no multiple of a tile here"""
    _exact_case(torch_cuda, M, N, K, 1)


# ---------------------------------------------------------------------------------------------------------------------
# real-valued GEMM
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('accum', [0, 1])
@pytest.mark.parametrize('M,N,K', [(65, 33, 127), (129, 64, 128), (70, 1024, 128), (5, 512, 1024)])
def test_linear_real_valued_within_the_dot_product_bound(M, N, K, accum, torch_cuda):
    rng = np.random.default_rng([7, M, N, K, accum])
    X, W, b, dY = (rng.standard_normal(s).astype(np.float32) for s in ((M, K), (N, K), (N,), (M, N)))
    dX0 = rng.standard_normal((M, K)).astype(np.float32) if accum else None
    ref = ref_linear(X, W, b, dY, dX0)
    dev = run_linear(torch_cuda, X, W, b, dY, accum, dX0)
    aX, aW, aY = (np.abs(a).astype(np.float64) for a in (X, W, dY))
    bounds = dict(Y=(K + 8) * U * (aX @ aW.T), dW=(M + 8) * U * (aY.T @ aX),
                  dX=(N + 8) * U * (aY @ aW) if not accum else (N + 1 + 8) * U * (aY @ aW + np.abs(dX0).astype(np.float64)),
                  db=U * np.abs(ref['db']) + (M + 4) * V * aY.sum(axis=0))
    for k, bound in bounds.items():
        err = np.abs(dev[k].astype(np.float64) - ref[k])
        print('M %d N %d K %d accum %d: %s worst error / bound %.3g' % (M, N, K, accum, k, float((err / np.maximum(bound, 1e-300)).max())))
        assert (err <= bound).all(), (k, int((err > bound).sum()), float((err / np.maximum(bound, 1e-300)).max()))


# ---------------------------------------------------------------------------------------------------------------------
# column sums and batch-norm
# ---------------------------------------------------------------------------------------------------------------------
def run_bn(torch, y, gamma, beta, dz, relu):
    """p2s_debug_train_bn -> dict(z, mean, invstd, pmean, pvar, dbeta, dgamma, dy), sentinels checked"""
    from points2surf_amd import _lib
    lib = _lib.load()
    M, C = y.shape
    off = C + TAIL
    params = _sent_buf(torch, off + C)
    _put(params, 0, gamma)
    _put(params, off, beta)
    grads = _sent_buf(torch, off + C + TAIL)
    pend = _sent_buf(torch, off + C + TAIL)
    yd = torch.from_numpy(np.ascontiguousarray(y, np.float32)).cuda()
    z = _sent_buf(torch, M * C + TAIL)
    d = _sent_buf(torch, M * C + TAIL)
    _put(d, 0, dz)
    mean, invstd = _sent_buf(torch, C + TAIL), _sent_buf(torch, C + TAIL)
    torch.cuda.synchronize()
    _lib.check(lib.p2s_debug_train_bn(_ptr(yd), _ptr(params), off, _ptr(z), _ptr(mean), _ptr(invstd), _ptr(pend), _ptr(d),
                                      _ptr(grads), M, C, int(relu), None))
    what = 'M %d C %d relu %d ' % (M, C, relu)
    return dict(z=_take(z, 0, (M, C), what + 'z'), mean=_take(mean, 0, (C,), what + 'mean'),
                invstd=_take(invstd, 0, (C,), what + 'invstd'), pmean=_take(pend, 0, (C,), what + 'pending mean'),
                pvar=_take(pend, off, (C,), what + 'pending variance'), dgamma=_take(grads, 0, (C,), what + 'd gamma'),
                dbeta=_take(grads, off, (C,), what + 'd beta'), dy=_take(d, 0, (M, C), what + 'dL/dy', written=False))


BN_C = [1, 63, 64, 65, 130]
BN_M = [2, 3, 5, 255, 256, 257, 1025]
BN_SHAPES = [(M, C) for M in BN_M for C in BN_C] + [(131072, 5), (131073, 5), (131073, 1)]


@pytest.mark.parametrize('M,C', BN_SHAPES)
def test_column_sums_exact_on_integers(M, C, torch_cuda):
    """y and dz integers: d beta bit for bit, the mean exactly float32(sum / M); no ReLU, so the sums are plain"""
    rng = np.random.default_rng([3, M, C])
    y, dz = _ints(rng, M, C), _ints(rng, M, C)
    gamma, beta = rng.standard_normal(C).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    dev = run_bn(torch_cuda, y, gamma, beta, dz, 0)
    dbeta = dz.astype(np.float64).sum(axis=0)
    mean = (y.astype(np.float64).sum(axis=0) / np.float64(M)).astype(np.float32)
    assert (dev['dbeta'].astype(np.float64) == dbeta).all(), (dev['dbeta'], dbeta)
    assert (dev['mean'] == mean).all() and (dev['pmean'] == mean).all(), (dev['mean'], mean)


def _bn_data(M, C, relu):
    rng = np.random.default_rng([5, M, C, relu])
    y = (rng.standard_normal((M, C)) * rng.uniform(0.5, 2.0, C) + rng.uniform(-1.0, 1.0, C)).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C)
    beta = rng.uniform(-0.5, 0.5, C)
    y[:, 0] = (100.0 + 0.01 * rng.standard_normal(M)).astype(np.float32)       # E[y^2] - mean^2 cancels 8 digits
    exact = None
    if C > 1:
        y[:, 1] = 3.5                                                            # variance 0
    if C > 2:
        exact = 2
        col = np.zeros(M, np.float32)
        col[:M // 3] = 1.0
        col[M // 3:2 * (M // 3)] = -1.0
        y[:, 2] = rng.permutation(col)
        gamma[2], beta[2] = 0.75, 0.0
    dz = rng.standard_normal((M, C)).astype(np.float32)
    return y, gamma.astype(np.float32), beta.astype(np.float32), dz, exact


def _bn_reference(y, gamma, beta, relu):
    """float64 forward and its bounds (module docstring)"""
    M = y.shape[0]
    y, g, be = y.astype(np.float64), gamma.astype(np.float64), beta.astype(np.float64)
    r = dict(M=M, y=y, g=g)
    mean = y.sum(axis=0) / M
    var = ((y - mean) ** 2).sum(axis=0) / M
    S1, S2 = np.abs(y).mean(axis=0), (y * y).mean(axis=0)
    dmean = (M + 4) * V * S1
    dvar = 4 * (M + 4) * V * S2
    assert (dvar < EPS).all()
    inv = 1.0 / np.sqrt(var + EPS)
    inv_hi = (1.0 / np.sqrt(var + EPS - dvar)) * (1 + U + 4 * V)
    inv_lo = (1.0 / np.sqrt(var + EPS + dvar)) * (1 - U - 4 * V)
    r.update(mean=mean, var=var, inv=inv, inv_hi=inv_hi, em=U * np.abs(mean) + dmean, einv=np.maximum(inv_hi - inv, inv - inv_lo),
             pvar=var * M / (M - 1.0), epvar=(dvar + (U + 4 * V) * (var + dvar)) * M / (M - 1.0))
    r['xhat'] = (y - mean) * inv
    r['exh'] = (r['em'] * inv_hi + np.abs(y - mean) * r['einv']) * (1 + 2 * U) + 2 * U * np.abs(r['xhat'])
    r['zpre'] = r['xhat'] * g + be
    r['bz'] = np.abs(g) * r['exh'] + 2 * U * np.abs(r['xhat'] * g) + U * np.abs(r['zpre'])
    r['z'] = np.maximum(r['zpre'], 0.0) if relu else r['zpre']
    return r


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('M,C', BN_SHAPES)
def test_batch_norm_forward_and_backward_within_derived_bounds(M, C, relu, torch_cuda):
    y, gamma, beta, dz, exact = _bn_data(M, C, relu)
    r = _bn_reference(y, gamma, beta, relu)
    zero_rows = None
    if relu:
        ambiguous = np.abs(r['zpre']) <= 2 * SLACK * r['bz']
        if exact is not None:
            ambiguous[:, exact] = False
            zero_rows = y[:, exact] == 0
            assert M < 3 or zero_rows.any()
            assert (r['zpre'][zero_rows, exact] == 0).all() and (np.abs(dz[zero_rows, exact]) > 0).all()
        dz = dz.copy()
        dz[ambiguous] = 0.0
    dev = run_bn(torch_cuda, y, gamma, beta, dz, relu)
    g, inv, inv_hi, einv, xhat, exh = r['g'], r['inv'], r['inv_hi'], r['einv'], r['xhat'], r['exh']
    dzm = dz.astype(np.float64) * ((r['zpre'] > 0) if relu else 1.0)
    dbeta, dgamma = dzm.sum(axis=0), (dzm * xhat).sum(axis=0)
    edb = (M + 4) * V * np.abs(dzm).sum(axis=0) + U * np.abs(dbeta)
    edg = (np.abs(dzm) * exh).sum(axis=0) + (M + 4) * V * np.abs(dzm * xhat).sum(axis=0) + U * np.abs(dgamma)
    m1, m2 = dbeta / M, dgamma / M
    inner = dzm - m1 - xhat * m2
    dy = g * inv * inner
    einner = edb / M + exh * np.abs(m2) + (np.abs(xhat) + exh) * edg / M + 3 * U * (np.abs(dzm) + np.abs(m1) + np.abs(xhat * m2))
    edy = np.abs(g) * (inv_hi * einner + einv * np.abs(inner)) + 3 * U * np.abs(dy)
    checks = [('mean', r['mean'], r['em']), ('pmean', r['mean'], r['em']), ('invstd', inv, einv), ('pvar', r['pvar'], r['epvar']),
              ('z', r['z'], r['bz']), ('dbeta', dbeta, edb), ('dgamma', dgamma, edg), ('dy', dy, edy)]
    for k, ref, bound in checks:
        err = np.abs(dev[k].astype(np.float64) - ref)
        ratio = float((err / np.maximum(SLACK * bound, 1e-300)).max())
        print('M %d C %d relu %d: %s worst error / bound %.3g' % (M, C, relu, k, ratio))
        assert (err <= SLACK * bound).all(), (k, int((err > SLACK * bound).sum()), ratio)
    if zero_rows is not None:
        assert (dev['z'][zero_rows, exact] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# refusals: a message, never a fault
# ---------------------------------------------------------------------------------------------------------------------
def test_hooks_refuse_bad_sizes_and_host_pointers(torch_cuda):
    from points2surf_amd import _lib
    lib = _lib.load()
    t = _sent_buf(torch_cuda, 4 * TAIL)
    p = _ptr(t)
    for M, N, K in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4)):
        assert lib.p2s_debug_train_linear(p, p, 16, p, p, p, p, M, N, K, 0, None) == -1
        assert b'p2s_debug_train_linear' in lib.p2s_last_error()
    assert lib.p2s_debug_train_linear(p, p, 15, p, p, p, p, 4, 4, 4, 0, None) == -1         # the bias inside the weight
    assert lib.p2s_debug_train_linear(p, p, 16, p, p, p, p, 4, 4, 4, 2, None) == -1
    host = np.zeros(64, np.float32)
    assert lib.p2s_debug_train_linear(host.ctypes.data_as(ctypes.c_void_p), p, 16, p, p, p, p, 4, 4, 4, 0, None) == -1
    assert b'device memory' in lib.p2s_last_error()
    for M, C in ((1, 4), (0, 4), (4, 0)):
        assert lib.p2s_debug_train_bn(p, p, 4, p, p, p, p, p, p, M, C, 0, None) == -1
        assert b'p2s_debug_train_bn' in lib.p2s_last_error()
    assert lib.p2s_debug_train_bn(p, p, 3, p, p, p, p, p, p, 4, 4, 0, None) == -1
    assert (t.cpu().numpy().view(np.uint32) == SENT).all()
