"""Seeded synthetic stand-ins for what cannot be downloaded offline.

* ``make_weights``: random-init weights of the reference architecture (pretrained
  ``p2s_*_model_*.pth`` files need the network, reference models/download_models_*.py).
  Variance-preserving uniform init + randomised BatchNorm running statistics (so BN
  folding is exercised) + near-identity feature transforms; logits come out O(1) with
  mixed signs, which makes sign/SDF parity meaningful.
* ``make_cloud``: a noisy scan-like point cloud of an analytic solid inside the unit
  cube (the reference normalises clouds to [-0.5,0.5]^3, make_pc_dataset.py:20-36).

Both are numpy-only and bit-reproducible from the seed on any box with this image.
"""
import numpy as np

from .model_spec import state_shapes, NAMED_MODELS


_FC4_BIAS_SHIFT = {'p2s_max': (6.289174, 2.416443), 'p2s_vanilla': (2.6854432, 4.523528),
                   'p2s_uniform': (4.6575, 2.458), 'p2s_no_qstn': (2.3863, 1.8502), 'p2s_small_kNN': (4.2235, 2.2435),
                   'p2s_large_kNN': (4.9557, 2.6857), 'p2s_regression': (3.7676,), 'p2s_shared_encoder': (-0.2, -3.9804),
                   'p2s_small_radius': (2.6671, 1.4694), 'p2s_medium_radius': (3.4947, 2.3483),
                   'p2s_large_radius': (3.9348, 2.7203), 'p2s_max_no_feat_stn': (0.1092, 2.8237),
                   'p2s_max_sum': (3.3387, 1.0881), 'p2s_shared_encoder_sum': (0.5145, 0.1371)}


# Second synthetic weight set of p2s_vanilla: the same weights with the bias of the SIGN logit moved by the median of
# that logit over the 128^3 query grid of the abc_minimal test shape (-1.30, measured with oracle/torch_port.py on 500
# random queries of the grid; the default set is positive for 0.9 % of those queries), so that the decision
# ``sign logit >= 0`` (reference source/sdf_nn.py:16-21) is close for many queries and a sign-flip count has power.
_SIGN_BIAS_EXTRA = {'p2s_vanilla_mixed': ('p2s_vanilla', 1.30)}


# Adversarial derived sets (parity tests of the regimes the default sets never reach): the weights of the base set with
#  * every BatchNorm: gamma of both signs (40 % negative), 5 % of the channels with |gamma| in [1e-6, 1e-3], two channels
#    with gamma exactly 0; running_var log-uniform in [1e-6, 10] and |gamma| = g * sqrt(var + eps), g in U(0.5, 1.5), for
#    the others, so that the folded scale gamma / sqrt(var + eps) stays O(1) and activations do not grow layer by layer;
#  * the STN / QSTN fc3 redrawn without the near-identity scaling (||trans2 - I|| of order 10, quaternions far from
#    [1,0,0,0]); the QSTN fc3 bias moved by ``qstn_shift`` so that some queries of the test shape have sum(q^2) in
#    [0.05, 0.3] (the normalisation s = 2 / sum(q^2) of batch_quat_to_rotmat, reference source/base/utils.py:13-46);
#  * two all-zero rows in every per-point conv of the encoders;
#  * fc4 scaled by ``fc4_scale`` and its bias moved by ``fc4_shift`` (measured on the abc_minimal test shape with
#    oracle/p2s_oracle.py) so that both logits take both signs and tanh^2 is not saturated for most queries.
# name -> (base set, seed of the perturbation, qstn_shift, fc4_scale, fc4_shift); statistics: tests/golden/meta_stress.json
_STRESS = {'p2s_max_stress': ('p2s_max', 9001, None, 0.1, (-6.151, -6.783)),
           'p2s_vanilla_stress': ('p2s_vanilla', 9002, (-1.3, 0.35, -1.14, 1.42), 0.1, (-1.045, -1.576))}
STRESS_MODELS = tuple(sorted(_STRESS))


def _stress(w, seed, qstn_shift, fc4_scale, fc4_shift):
    rng = np.random.default_rng(seed)
    w = {k: v.copy() for k, v in w.items()}
    eps = 1e-5
    for name in sorted(w):
        pre, leaf = name.rsplit('.', 1)
        if not (pre.rsplit('.', 1)[-1].startswith('bn') and leaf == 'weight'):
            continue
        c = w[name].shape[0]
        var = 10.0 ** rng.uniform(-6.0, 1.0, c)
        g = rng.uniform(0.5, 1.5, c) * np.sqrt(var + eps)
        tiny = rng.random(c) < 0.05
        g[tiny] = 10.0 ** rng.uniform(-6.0, -3.0, int(tiny.sum()))
        g *= np.where(rng.random(c) < 0.4, -1.0, 1.0)
        g[rng.choice(c, 2, replace=False)] = 0.0
        w[name] = g.astype(np.float32)
        w[pre + '.running_var'] = var.astype(np.float32)
    for name in sorted(w):
        pre, leaf = name.rsplit('.', 1)
        layer = pre.rsplit('.', 1)[-1]
        if pre.endswith('stn2.fc3') or pre.endswith('stn1.fc3') or pre.startswith('point_stn.fc3'):
            a = np.sqrt(6.0 / w[pre + '.weight'].shape[1])
            w[name] = rng.uniform(-a if leaf == 'weight' else -0.1, a if leaf == 'weight' else 0.1,
                                  w[name].shape).astype(np.float32)
        elif leaf == 'weight' and layer in ('conv1', 'conv2', 'conv3') and '.stn' not in pre and pre.startswith('feat_'):
            W = w[name].copy()
            W[rng.choice(W.shape[0], 2, replace=False)] = 0.0
            w[name] = W
    if qstn_shift is not None:
        for name in sorted(w):
            if name.endswith('stn1.fc3.bias') or name == 'point_stn.fc3.bias':
                w[name] = (w[name] + np.asarray(qstn_shift, dtype=np.float32)).astype(np.float32)
    w['fc4.weight'] = (w['fc4.weight'] * np.float32(fc4_scale)).astype(np.float32)
    w['fc4.bias'] = (w['fc4.bias'] + np.asarray(fc4_shift, dtype=np.float32)).astype(np.float32)
    return w


def make_weights(model='p2s_max', seed=1234, net_size_max=1024, output_dim=None):
    """Returns ({name: float32 ndarray} without ``module.`` prefix, cfg dict)."""
    if isinstance(model, str) and model in _STRESS:
        base, sseed, qshift, fscale, fshift = _STRESS[model]
        w, cfg_out = make_weights(base, seed=seed, net_size_max=net_size_max, output_dim=output_dim)
        return _stress(w, sseed, qshift, fscale, fshift), cfg_out
    if isinstance(model, str) and model in _SIGN_BIAS_EXTRA:
        base, extra = _SIGN_BIAS_EXTRA[model]
        w, cfg_out = make_weights(base, seed=seed, net_size_max=net_size_max, output_dim=output_dim)
        b = w['fc4.bias'].copy()
        b[1] = np.float32(b[1] + np.float32(extra))
        w['fc4.bias'] = b
        return w, cfg_out
    cfg = dict(NAMED_MODELS[model]) if isinstance(model, str) else dict(model)
    if output_dim is None:
        output_dim = int(cfg.get('output_dim', 2))
    single = bool(cfg.get('single_transformer', False))
    shapes = state_shapes(net_size_max=net_size_max, output_dim=output_dim,
                          use_point_stn=cfg.get('use_point_stn', False),
                          shared_transformation=cfg.get('shared_transformation', False),
                          use_feat_stn=cfg.get('use_feat_stn', True), single_transformer=single)
    rng = np.random.default_rng(seed)
    w = {}
    for name, shape in shapes.items():
        leaf = name.rsplit('.', 1)[1]
        layer = name.rsplit('.', 1)[0].rsplit('.', 1)[-1]
        is_bn = layer.startswith('bn')
        if leaf == 'num_batches_tracked':
            w[name] = np.array(1000, dtype=np.int64)
        elif is_bn and leaf == 'weight':
            w[name] = rng.uniform(0.5, 1.5, shape).astype(np.float32)
        elif is_bn and leaf == 'bias':
            w[name] = (0.1 * rng.standard_normal(shape)).astype(np.float32)
        elif leaf == 'running_mean':
            w[name] = (0.1 * rng.standard_normal(shape)).astype(np.float32)
        elif leaf == 'running_var':
            w[name] = rng.uniform(0.5, 1.5, shape).astype(np.float32)
        elif leaf == 'weight':
            fan_in = shape[1]
            a = np.sqrt(6.0 / fan_in)
            w[name] = rng.uniform(-a, a, shape).astype(np.float32)
        elif leaf == 'bias':
            w[name] = rng.uniform(-0.1, 0.1, shape).astype(np.float32)
        else:
            raise AssertionError(name)
    # transforms close to identity (as trained spatial transformers are)
    for name in list(w):
        if name.endswith('stn2.fc3.weight') or name.endswith('stn2.fc3.bias'):
            w[name] = (w[name] * np.float32(0.05)).astype(np.float32)
        if name.endswith('stn1.fc3.weight') or name.endswith('stn1.fc3.bias') \
                or name.startswith('point_stn.fc3.'):
            w[name] = (w[name] * np.float32(0.2)).astype(np.float32)
    # sym_op='sum': the pooled feature is a sum over 300 / 1000 points -- scale the affine in front of the pool so that
    # the features (and with them the logits) stay O(1) like those of the max models
    if cfg.get('sym_op', 'max') == 'sum':
        for pre, npts in (('feat_local', 300.0), ('feat_global', 1000.0), ('feat_local_global', 1300.0)):
            for leaf in ('weight', 'bias'):
                if pre + '.bn3.' + leaf in w:
                    w[pre + '.bn3.' + leaf] = (w[pre + '.bn3.' + leaf] / np.float32(npts)).astype(np.float32)
    # centre the two output logits (the random decoder has a data-dependent offset much larger than
    # its spread; measured once on the abc_minimal fixture) so that tanh is not saturated and the
    # sign logit changes sign across queries
    shift = _FC4_BIAS_SHIFT.get(model if isinstance(model, str) else None)
    if shift is not None and seed == 1234 and output_dim == len(shift) and net_size_max == 1024:
        w['fc4.bias'] = (w['fc4.bias'] + np.asarray(shift, dtype=np.float32)).astype(np.float32)
    cfg_out = dict(
        use_point_stn=bool(cfg.get('use_point_stn', False)),
        shared_transformer=bool(cfg.get('shared_transformation', False)),
        use_feat_stn=bool(cfg.get('use_feat_stn', True)), single_transformer=single,
        uniform_subsample=bool(cfg.get('uniform_subsample', False)), fixed_subsample=False,
        net_size=net_size_max, points_per_patch=int(cfg.get('points_per_patch', 300)), sub_sample_size=1000,
        output_dim=output_dim, patch_radius=float(cfg.get('patch_radius', 0.0)), sym_op=cfg.get('sym_op', 'max'))
    return w, cfg_out


def to_torch_state_dict(w, module_prefix=True):
    import torch
    pre = 'module.' if module_prefix else ''
    return {pre + k: torch.from_numpy(np.array(v)) for k, v in w.items()}


def make_cloud(n_points=50000, seed=0, noise=0.004, kind='blob'):
    """Noisy surface samples of an analytic solid, float32 [N,3], inside [-0.5,0.5]^3."""
    rng = np.random.default_rng(seed)
    if kind == 'sphere':
        d = rng.standard_normal((n_points, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        p = 0.4 * d
    else:
        # star-shaped "blob": radius modulated by low-order harmonics (seeded), scan-like density
        d = rng.standard_normal((n_points, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        ph = rng.uniform(0, 2 * np.pi, 6)
        rad = 0.33 + 0.05 * np.sin(3 * np.arctan2(d[:, 1], d[:, 0]) + ph[0]) \
            + 0.04 * np.cos(4 * np.arccos(np.clip(d[:, 2], -1, 1)) + ph[1]) \
            + 0.03 * np.sin(5 * d[:, 0] + ph[2]) * np.cos(3 * d[:, 1] + ph[3])
        p = d * rad[:, None]
        p[:, 0] *= 1.15
        p[:, 2] *= 0.85
    p = p + noise * rng.standard_normal(p.shape)
    # unit-cube normalisation like make_pc_dataset._to_unit_cube (bbox centre, max extent -> 1)
    lo, hi = p.min(0), p.max(0)
    p = (p - (lo + hi) / 2) / (hi - lo).max()
    return np.ascontiguousarray(p.astype(np.float32))


def standin_cloud(base, seed):
    """One cloud of the stand-in data sets of SURVEY 8d configs 3-5 (the Famous / ABC / Thingi10k test sets cannot be
    downloaded offline): a base cloud under a seeded random rotation, re-normalised to the unit cube the way
    make_pc_dataset._to_unit_cube does (reference make_pc_dataset.py:20-36: translate the bounding-box centre to the
    origin, scale the largest extent to 1).  float64 arithmetic, one rounding to float32; numpy only."""
    rs = np.random.RandomState(int(seed))
    a = rs.standard_normal((3, 3))
    q, r = np.linalg.qr(a)
    q = q * np.sign(np.diag(r))                      # a proper distribution over O(3) ...
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]                           # ... restricted to rotations
    p = np.asarray(base, dtype=np.float64)[:, :3] @ q.T
    lo, hi = p.min(axis=0), p.max(axis=0)
    ext = (hi - lo).max()
    if ext == 0.0:
        return np.ascontiguousarray(p.astype(np.float32))
    return np.ascontiguousarray(((p - (lo + hi) * 0.5) / ext).astype(np.float32))


def make_standin_dataset(root, base_clouds, n_shapes, list_name='testset.txt'):
    """write ``n_shapes`` stand-in clouds (base cloud i mod len(base), rotation seed i) as <root>/04_pts/*.xyz.npy plus the
    shape list; returns the shape names"""
    import os
    os.makedirs(os.path.join(root, '04_pts'), exist_ok=True)
    names = []
    for i in range(int(n_shapes)):
        name = 'standin_%03d' % i
        np.save(os.path.join(root, '04_pts', name + '.xyz.npy'), standin_cloud(base_clouds[i % len(base_clouds)], i))
        names.append(name)
    with open(os.path.join(root, list_name), 'w') as f:
        f.write('\n'.join(names) + '\n')
    return names


def write_model_files(modeldir, model, seed=1234, encoder_cfg=None):
    """<modeldir>/<model>_model.pth (DataParallel-prefixed state_dict) + <model>_params.pth (the pickled train
    Namespace), the two files ``points_to_surf_eval`` loads (reference source/points_to_surf_eval.py:167-170,316) -- for
    the seeded synthetic weights (no pretrained weights exist offline).  Returns (weights, cfg)."""
    import argparse
    import os
    import torch
    w, cfg = make_weights(model, seed=seed)
    os.makedirs(modeldir, exist_ok=True)
    torch.save(to_torch_state_dict(w), os.path.join(modeldir, model + '_model.pth'))
    outputs = ['imp_surf', 'patch_pts_ids', 'p_index'] if int(cfg.get('output_dim', 2)) == 1 else \
        ['imp_surf_magnitude', 'imp_surf_sign', 'patch_pts_ids', 'p_index']
    ns = argparse.Namespace(
        outputs=outputs, points_per_patch=int(cfg.get('points_per_patch', 300)), patch_center='mean',
        sub_sample_size=int(cfg.get('sub_sample_size', 1000)), patch_radius=float(cfg.get('patch_radius', 0.0)),
        uniform_subsample=int(cfg['uniform_subsample']), fixed_subsample=int(cfg.get('fixed_subsample', 0)), net_size=1024,
        use_point_stn=int(cfg['use_point_stn']), use_feat_stn=int(cfg.get('use_feat_stn', True)), sym_op=cfg.get('sym_op', 'max'),
        single_transformer=int(cfg.get('single_transformer', False)), shared_transformer=int(cfg['shared_transformer']),
        batchSize=501)
    torch.save(ns, os.path.join(modeldir, model + '_params.pth'))
    return w, cfg
