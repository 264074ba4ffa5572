"""Training of ``p2s_max`` / ``p2s_max_no_feat_stn`` on the device (include/p2s_hip.h, the p2s_trainer_* entry points;
points2surf_amd/csrc/p2s_train.hip): train-mode forward, the reference's two losses, backward and torch's SGD update,
all fp32.  Tensors are containers; nothing here computes on the CPU or in torch, and nothing falls back.

``python -m points2surf_amd.train --indir DATASET --name NAME --outdir DIR`` replaces the loop of the reference's
source/points_to_surf_train.py for the hyper-parameters listed in ``parse_arguments``: it writes NAME_model.pth and
NAME_params.pth, the two files the evaluation loads.  The ORDER of shapes and patches is this project's own seeded
definition (``epoch_order``), not the reference's DataLoader worker streams.  ``--loader set`` assembles every batch
over all its clouds in one call each (engine.CloudSet; the same bytes as the default per-shape loop, far fewer launches);
``--testset FILE`` adds a validation pass per epoch (``validate``).
"""
import argparse
import ctypes
import math
import os
from collections import OrderedDict

import numpy as np
import torch

from . import _lib, model_spec
from .engine import _f32c, _ptr, _stream_ptr
from .weights import ModelCfg

POOLS = ('feat_local.stn2', 'feat_local', 'feat_global.stn2', 'feat_global')


def _is_buffer(name):
    return name.endswith(('.running_mean', '.running_var'))


def unsupported_reason(cfg):
    """why the device trainer refuses ``cfg`` (None: it trains it)"""
    if cfg.get('use_point_stn'):
        return 'a QSTN (use_point_stn) is not trained on the device'
    if cfg.get('single_transformer'):
        return 'the shared encoder (single_transformer) is not trained on the device'
    if cfg.get('shared_transformer') or cfg.get('shared_transformation'):
        return 'a shared transformer is not trained on the device'
    if cfg.get('sym_op', 'max') != 'max':
        return "sum pooling (sym_op='sum') is not trained on the device"
    if int(cfg.get('output_dim', 2)) != 2:
        return 'regression (output_dim 1) is not trained on the device'
    if float(cfg.get('patch_radius', 0.0) or 0.0) != 0.0:
        return 'a fixed patch radius is not trained on the device'
    if int(cfg.get('net_size', 1024)) != 1024:
        return 'only net size 1024 is trained on the device'
    return None


def init_state(cfg, seed=0):
    """the initial state dict torch's own layer constructors give (Conv1d / Linear: kaiming_uniform(a = sqrt 5) weights,
    U(+-1/sqrt(fan_in)) biases; BatchNorm1d: weight 1, bias 0, mean 0, variance 1, 0 batches), from one seeded generator in
    state_shapes order -- host-side setup, no reference stream is reproduced"""
    gen = torch.Generator().manual_seed(int(seed))
    shapes = model_spec.state_shapes(net_size_max=1024, output_dim=2, use_feat_stn=bool(cfg.get('use_feat_stn', True)))
    out = OrderedDict()
    for name, shape in shapes.items():
        layer, leaf = name.split('.')[-2], name.split('.')[-1]
        if leaf == 'num_batches_tracked':
            out[name] = np.array(0, dtype=np.int64)
        elif layer.startswith('bn'):
            out[name] = np.full(shape, 1.0 if leaf in ('weight', 'running_var') else 0.0, dtype=np.float32)
        elif leaf == 'weight':
            t = torch.empty(shape, dtype=torch.float32)
            torch.nn.init.kaiming_uniform_(t, a=math.sqrt(5), generator=gen)
            out[name] = t.numpy()
        else:
            bound = 1.0 / math.sqrt(shapes[name[:-4] + 'weight'][1])
            t = torch.empty(shape, dtype=torch.float32)
            torch.nn.init.uniform_(t, -bound, bound, generator=gen)
            out[name] = t.numpy()
    return out


class Trainer:
    """One model in training on one device.  ``cfg`` as synth.make_weights returns it (points_per_patch and
    sub_sample_size fix the two point counts); ``state_dict`` None: torch's initialisers from ``seed``."""

    def __init__(self, cfg, state_dict=None, seed=0, device=None):
        why = unsupported_reason(cfg)
        if why:
            raise ValueError('Trainer: %s (p2s_max and p2s_max_no_feat_stn only)' % why)
        self.cfg = dict(cfg)
        self.use_feat_stn = bool(cfg.get('use_feat_stn', True))
        self.P, self.S = int(cfg.get('points_per_patch', 300)), int(cfg.get('sub_sample_size', 1000))
        self.shapes = model_spec.state_shapes(net_size_max=1024, output_dim=2, use_feat_stn=self.use_feat_stn)
        sd = init_state(cfg, seed) if state_dict is None else model_spec.strip_module_prefix(state_dict)
        sd = {k: (v.detach().cpu().numpy() if hasattr(v, 'detach') else np.asarray(v)) for k, v in sd.items()}
        missing = [k for k in self.shapes if k not in sd]
        if missing:
            raise ValueError('Trainer: state dict lacks %s' % missing[:4])
        self.param_names = [k for k in self.shapes if not _is_buffer(k) and not k.endswith('num_batches_tracked')]
        self.buffer_names = [k for k in self.shapes if _is_buffer(k)]
        for k in self.param_names + self.buffer_names:
            if tuple(sd[k].shape) != tuple(self.shapes[k]):
                raise ValueError('Trainer: %s has shape %s, expected %s' % (k, tuple(sd[k].shape), tuple(self.shapes[k])))
        params = np.ascontiguousarray(np.concatenate([sd[k].astype(np.float32).ravel() for k in self.param_names]))
        bufs = np.ascontiguousarray(np.concatenate([sd[k].astype(np.float32).ravel() for k in self.buffer_names]))
        nbt = {int(sd[k]) for k in self.shapes if k.endswith('num_batches_tracked')}
        if len(nbt) != 1:
            raise ValueError('Trainer: the batch-norms disagree on num_batches_tracked: %s' % sorted(nbt))
        self.n_params, self.n_buffers = int(params.size), int(bufs.size)
        if not torch.cuda.is_available():
            raise RuntimeError('points2surf_amd needs a ROCm GPU (gfx950); no CPU fallback exists')
        self.lib = _lib.load()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        mc = ModelCfg(net_size=1024, points_per_patch=self.P, sub_sample_size=self.S, output_dim=2)
        self.handle = ctypes.c_void_p()
        _lib.check(self.lib.p2s_trainer_create(
            ctypes.byref(mc), int(self.use_feat_stn), params.ctypes.data_as(ctypes.c_void_p), params.size,
            bufs.ctypes.data_as(ctypes.c_void_p), bufs.size, nbt.pop(), self.device.index, ctypes.byref(self.handle)))
        self.batch = 0

    def close(self):
        if getattr(self, 'handle', None):
            self.lib.p2s_trainer_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def forward_backward(self, patch_pts_ps, pts_sub_sample_ms, query_ms, dist_abs, sign01, radius):
        """one train-mode forward + backward on a batch -> (magnitude loss, sign loss); inputs are not modified.
        Raises on B < 2 and on a non-finite loss or gradient (nothing is updated then)."""
        dev = self.device
        patch, sub, q = _f32c(patch_pts_ps, dev), _f32c(pts_sub_sample_ms, dev), _f32c(query_ms, dev)
        B = int(patch.shape[0])
        if patch.shape != (B, self.P, 3) or sub.shape != (B, self.S, 3) or q.shape != (B, 3):
            raise ValueError('bad input shapes %s %s %s' % (tuple(patch.shape), tuple(sub.shape), tuple(q.shape)))
        per_item = [_f32c(t.reshape(-1), dev) for t in (dist_abs, sign01, radius)]
        if any(t.shape != (B,) for t in per_item):
            raise ValueError('dist_abs, sign01 and radius must hold one value per item')
        losses = (ctypes.c_double * 2)()
        with torch.cuda.device(dev):
            _lib.check(self.lib.p2s_trainer_forward_backward(self.handle, _ptr(patch), _ptr(sub), _ptr(q), _ptr(per_item[0]),
                                                             _ptr(per_item[1]), _ptr(per_item[2]), B, losses, _stream_ptr(dev)))
        self.batch = B
        return float(losses[0]), float(losses[1])

    def step(self, lr, momentum):
        with torch.cuda.device(self.device):
            _lib.check(self.lib.p2s_trainer_sgd_step(self.handle, float(lr), float(momentum), _stream_ptr(self.device)))

    def _copy_out(self, what, n):
        out = np.empty(n, dtype=np.float32)
        nbt = ctypes.c_int64(0)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.p2s_trainer_copy_out(self.handle, what, out.ctypes.data_as(ctypes.c_void_p), n, ctypes.byref(nbt)))
        return out, int(nbt.value)

    def _split(self, flat, names):
        out, o = OrderedDict(), 0
        for k in names:
            n = int(np.prod(self.shapes[k], dtype=np.int64))
            out[k] = flat[o:o + n].reshape(self.shapes[k]).copy()
            o += n
        return out

    def grads(self):
        """{parameter name: gradient of the last forward_backward} (numpy, state_shapes order)"""
        return self._split(self._copy_out(2, self.n_params)[0], self.param_names)

    def pool_indices(self):
        """{pool name: [B, 1024] int32}: the point every max-pool of the last step picked (lowest index on ties)"""
        names = [p for p in POOLS if self.use_feat_stn or not p.endswith('stn2')]
        out = np.empty((len(names), self.batch, 1024), dtype=np.int32)
        _lib.check(self.lib.p2s_trainer_pool_indices(self.handle, out.ctypes.data_as(ctypes.c_void_p), out.size))
        return OrderedDict((p, out[i]) for i, p in enumerate(names))

    def profile(self, enabled):
        """-> the milliseconds per kernel family of the last profiled step; switches profiling for the next ones"""
        ms = (ctypes.c_double * 8)()
        _lib.check(self.lib.p2s_trainer_profile(self.handle, int(bool(enabled)), ms))
        return dict(zip(('gemm', 'colsum', 'batchnorm', 'pool', 'small'), [float(v) for v in ms[:5]]))

    def resident_bytes(self):
        n = ctypes.c_int64(0)
        _lib.check(self.lib.p2s_trainer_sizes(self.handle, None, None, None, ctypes.byref(n)))
        return int(n.value)

    def state_dict(self, module_prefix=True):
        """the reference's checkpoint: its key names and dtypes (num_batches_tracked int64), ``module.`` in front as
        saving the DataParallel wrapper does"""
        params, nbt = self._copy_out(0, self.n_params)
        vals = self._split(params, self.param_names)
        vals.update(self._split(self._copy_out(1, self.n_buffers)[0], self.buffer_names))
        pre = 'module.' if module_prefix else ''
        out = OrderedDict()
        for k in self.shapes:
            out[pre + k] = torch.tensor(nbt, dtype=torch.int64) if k.endswith('num_batches_tracked') else torch.from_numpy(vals[k])
        return out


# -- command line ------------------------------------------------------------------------------------------------------
def parse_arguments(args=None):
    p = argparse.ArgumentParser(description='train p2s_max on the device')
    p.add_argument('--indir', required=True, help='data set: 04_pts, 05_query_pts, 05_query_dist and the shape list')
    p.add_argument('--name', required=True, help='model name: <outdir>/<name>_model.pth, <name>_params.pth')
    p.add_argument('--outdir', required=True)
    p.add_argument('--trainset', default='trainset.txt', help='shape list inside --indir')
    p.add_argument('--nepoch', type=int, default=150)
    p.add_argument('--lr', type=float, default=0.01)
    p.add_argument('--momentum', type=float, default=0.9)
    p.add_argument('--scheduler_steps', type=int, nargs='*', default=[75, 125], help='epochs at which lr is multiplied by 0.1')
    p.add_argument('--batchSize', type=int, default=501)
    p.add_argument('--points_per_patch', type=int, default=300)
    p.add_argument('--sub_sample_size', type=int, default=1000)
    p.add_argument('--patches_per_shape', type=int, default=1000)
    p.add_argument('--use_feat_stn', type=int, default=1)
    p.add_argument('--seed', type=int, default=3627473)
    p.add_argument('--save_interval', type=int, default=10, help='write the checkpoint every this many epochs (and at the end)')
    p.add_argument('--gpu_idx', type=int, default=0)
    p.add_argument('--loader', choices=('per_shape', 'set'), default='per_shape',
                   help="how a batch is assembled: 'per_shape' one upload, kNN and sub-sample call per shape of the batch; 'set' one "
                        "of each per batch over all clouds (the same bytes, far fewer launches: use it)")
    p.add_argument('--testset', default='', help="shape list inside --indir to validate on after every epoch ('' = no validation)")
    return p.parse_args(args=args)


def epoch_order(n_queries_per_shape, patches_per_shape, seed, epoch):
    """this project's definition of an epoch: from RandomState(seed + epoch), per shape ``patches_per_shape`` distinct query
    indices (all of them, if the shape has fewer), then one permutation of all (shape, query) pairs -> int64 [n, 2]"""
    rs = np.random.RandomState((int(seed) + int(epoch)) & 0x7fffffff)
    pairs = []
    for s, nq in enumerate(n_queries_per_shape):
        ids = rs.permutation(int(nq))[:int(patches_per_shape)]
        pairs.append(np.stack([np.full(ids.shape, s, dtype=np.int64), ids.astype(np.int64)], axis=1))
    pairs = np.concatenate(pairs, axis=0)
    return pairs[rs.permutation(pairs.shape[0])]


def learning_rate(lr, scheduler_steps, epoch):
    """torch MultiStepLR(gamma = 0.1)"""
    return float(lr) * 0.1 ** sum(1 for s in scheduler_steps if epoch >= s)


def params_namespace(opt):
    """the pickled Namespace the evaluation reads (reference source/points_to_surf_eval.py:316)"""
    return argparse.Namespace(
        outputs=['imp_surf_magnitude', 'imp_surf_sign', 'patch_pts_ids', 'p_index'], points_per_patch=int(opt.points_per_patch),
        patch_center='mean', sub_sample_size=int(opt.sub_sample_size), patch_radius=0.0, uniform_subsample=1, fixed_subsample=0,
        net_size=1024, use_point_stn=0, use_feat_stn=int(bool(opt.use_feat_stn)), sym_op='max', single_transformer=0,
        shared_transformer=0, batchSize=int(opt.batchSize), nepoch=int(opt.nepoch), lr=float(opt.lr), momentum=float(opt.momentum),
        scheduler_steps=list(opt.scheduler_steps), patches_per_shape=int(opt.patches_per_shape), seed=int(opt.seed),
        name=opt.name, indir=opt.indir, trainset=opt.trainset, testset=getattr(opt, 'testset', ''),
        loader=getattr(opt, 'loader', 'per_shape'))


class TrainData:
    """One data set on the device: the shape names, their clouds, the set over them (made on first use), and all query
    points and distances concatenated, shape s at rows ``offsets[s] .. offsets[s + 1]``.  ``points_per_patch`` and
    ``sub_sample_size`` are the two point counts of every batch it assembles."""

    def __init__(self, names, clouds, queries, dists, points_per_patch, sub_sample_size):
        self.names, self.clouds = list(names), list(clouds)
        self.P, self.S = int(points_per_patch), int(sub_sample_size)
        for n, q, d in zip(self.names, queries, dists):
            if q.shape[0] != d.shape[0]:
                raise ValueError('%s: %d query points, %d distances' % (n, q.shape[0], d.shape[0]))
        self.n_queries = [int(q.shape[0]) for q in queries]
        self.offsets = np.concatenate([[0], np.cumsum(self.n_queries)]).astype(np.int64)
        self.queries = np.ascontiguousarray(np.concatenate(queries, axis=0), dtype=np.float32).reshape(-1, 3)
        self.dists = np.ascontiguousarray(np.concatenate(dists, axis=0), dtype=np.float32).reshape(-1)
        self.device = self.clouds[0].device
        self._set = None

    @classmethod
    def load(cls, indir, list_file, points_per_patch, sub_sample_size, dev):
        """04_pts, 05_query_pts and 05_query_dist of the shapes ``list_file`` (inside ``indir``) names"""
        from . import engine
        with open(os.path.join(indir, list_file)) as f:
            names = [l.strip() for l in f if l.strip()]
        clouds, queries, dists = [], [], []
        for n in names:
            pts = np.load(os.path.join(indir, '04_pts', n + '.xyz.npy'))
            clouds.append(engine.Cloud(np.ascontiguousarray(pts[:, :3], dtype=np.float32), dev))
            queries.append(np.ascontiguousarray(np.load(os.path.join(indir, '05_query_pts', n + '.ply.npy')), dtype=np.float32))
            dists.append(np.ascontiguousarray(np.load(os.path.join(indir, '05_query_dist', n + '.ply.npy')), dtype=np.float32).reshape(-1))
        return cls(names, clouds, queries, dists, points_per_patch, sub_sample_size)

    def cloudset(self):
        """the set over the clouds; a cloud with fewer points than the patch or the sub-sample is named and refused (the
        shuffle-and-pad branch of such clouds exists per cloud only: loader 'per_shape')"""
        if self._set is None:
            from . import engine
            for n, c in zip(self.names, self.clouds):
                if c.n < max(self.P, self.S):
                    raise ValueError("loader 'set': shape %s has %d points, fewer than points_per_patch %d or sub_sample_size %d"
                                     % (n, c.n, self.P, self.S))
            self._set = engine.CloudSet(self.clouds)
        return self._set

    def close(self):
        if self._set is not None:
            self._set.close()
            self._set = None

    def assemble(self, items, loader, rng):
        """the batch of ``items`` (int64 [n, 2]: shape, query index) -> the six tensors of ``Trainer.forward_backward``.  The
        items are sorted by shape (stably) first; ``rng`` draws the sub-samples in that order.  Both loaders give the same
        bytes and leave ``rng`` in the same state: 'per_shape' makes one upload, one kNN call and one sub-sample call per
        shape of the batch, 'set' one of each per batch (engine.CloudSet)."""
        from . import engine
        dev = self.device
        items = np.asarray(items, dtype=np.int64).reshape(-1, 2)
        items = items[np.argsort(items[:, 0], kind='stable')]
        if loader == 'set':
            cs = self.cloudset()
            rows = self.offsets[items[:, 0]] + items[:, 1]
            q_all, d = self.queries[rows], self.dists[rows]
            q_dev = engine.upload(q_all, dev)
            _, patch, rad = cs.knn_patch(items[:, 0], q_dev, self.P, want_ids=False)
            sub = cs.subsample_uniform(rng, items[:, 0], self.S)[1]
            return (patch, sub, q_dev, engine.upload(np.abs(d), dev), engine.upload((d >= 0).astype(np.float32), dev), rad)
        if loader != 'per_shape':
            raise ValueError("loader must be 'per_shape' or 'set' (got %r)" % (loader,))
        queries = [self.queries[self.offsets[s]:self.offsets[s + 1]] for s in range(len(self.clouds))]
        dists = [self.dists[self.offsets[s]:self.offsets[s + 1]] for s in range(len(self.clouds))]
        clouds = self.clouds
        patch, sub, rad = [], [], []
        for s in np.unique(items[:, 0]):
            q = engine.upload(queries[s][items[items[:, 0] == s, 1]], dev)
            _, p, r = clouds[s].knn_patch(q, self.P, want_ids=False)
            patch.append(p)
            rad.append(r)
            sub.append(rng.subsample_uniform(clouds[s], q.shape[0], self.S)[1])
        d = np.concatenate([dists[s][items[items[:, 0] == s, 1]] for s in np.unique(items[:, 0])])
        q_all = np.concatenate([queries[s][items[items[:, 0] == s, 1]] for s in np.unique(items[:, 0])])
        return (torch.cat(patch), torch.cat(sub), engine.upload(q_all, dev), engine.upload(np.abs(d), dev),
                engine.upload((d >= 0).astype(np.float32), dev), torch.cat(rad))


def losses(pred, dist_abs, sign01, radius):
    """(magnitude loss, sign loss) of given predictions [B, 2] on the device (p2s_train_losses): the training step's loss
    kernel without gradients"""
    dev = pred.device
    pred = _f32c(pred, dev)
    B = int(pred.shape[0])
    if pred.shape != (B, 2):
        raise ValueError('predictions must be [B, 2] (got %s)' % (tuple(pred.shape),))
    per_item = [_f32c(t.reshape(-1), dev) for t in (dist_abs, sign01, radius)]
    if any(t.shape != (B,) for t in per_item):
        raise ValueError('dist_abs, sign01 and radius must hold one value per item')
    out = (ctypes.c_double * 2)()
    with torch.cuda.device(dev):
        _lib.check(_lib.load().p2s_train_losses(_ptr(pred), _ptr(per_item[0]), _ptr(per_item[1]), _ptr(per_item[2]), B, out,
                                                _stream_ptr(dev)))
    return float(out[0]), float(out[1])


def validate(state_dict, opt, data, dev):
    """One validation pass over ``data`` -> (magnitude loss, sign loss), each the mean over the batches.  This project's
    own definition: the order is ``epoch_order(..., epoch=-1)`` and the sub-samples come from a fresh ``Rng(seed + 1)``,
    so every pass sees identical batches of ``--batchSize`` items (the last may be short) and the training stream is not
    touched.  The forward is the inference path (engine.Model, running statistics, fp32) with the configuration the
    evaluation derives from the saved parameters."""
    from . import engine
    from .dropin.source import points_to_surf_eval as ev
    train_opt = params_namespace(opt)
    cfg = dict(ev._engine_cfg(train_opt, ev.get_output_dimensions(train_opt)), encoder_bf16=0)
    sd = model_spec.strip_module_prefix(state_dict)
    model = engine.Model({k: (v.detach().cpu().numpy() if hasattr(v, 'detach') else np.asarray(v)) for k, v in sd.items()}, cfg, dev)
    rng = engine.Rng(int(opt.seed) + 1, dev)
    order = epoch_order(data.n_queries, opt.patches_per_shape, opt.seed, -1)
    total, batches = np.zeros(2), 0
    try:
        for b0 in range(0, order.shape[0], opt.batchSize):
            patch, sub, q, dist_abs, sign01, rad = data.assemble(order[b0:b0 + opt.batchSize], opt.loader, rng)
            logits, _ = model.forward(patch, sub, q)
            total += losses(logits, dist_abs, sign01, rad)
            batches += 1
    finally:
        rng.close()
        model.close()
    return total[0] / max(batches, 1), total[1] / max(batches, 1)


def train(opt):
    from . import engine
    dev = engine.select_device(opt.gpu_idx)
    data = TrainData.load(opt.indir, opt.trainset, opt.points_per_patch, opt.sub_sample_size, dev)
    test = TrainData.load(opt.indir, opt.testset, opt.points_per_patch, opt.sub_sample_size, dev) if opt.testset else None
    if opt.loader == 'set':
        for d in (data, test):
            if d is not None:
                d.cloudset()                                     # a cloud too small for the set fails here, by name
    cfg = dict(use_feat_stn=bool(opt.use_feat_stn), points_per_patch=opt.points_per_patch, sub_sample_size=opt.sub_sample_size,
               net_size=1024, output_dim=2)
    trainer = Trainer(cfg, seed=opt.seed, device=dev)
    rng = engine.Rng(opt.seed, dev)
    os.makedirs(opt.outdir, exist_ok=True)
    model_file = os.path.join(opt.outdir, opt.name + '_model.pth')
    torch.save(params_namespace(opt), os.path.join(opt.outdir, opt.name + '_params.pth'))
    for epoch in range(opt.nepoch):
        lr = learning_rate(opt.lr, opt.scheduler_steps, epoch)
        order = epoch_order(data.n_queries, opt.patches_per_shape, opt.seed, epoch)
        total, batches = np.zeros(2), 0
        for b0 in range(0, order.shape[0], opt.batchSize):
            items = order[b0:b0 + opt.batchSize]
            if items.shape[0] < 2:
                continue                                     # batch-norm needs a batch
            loss = trainer.forward_backward(*data.assemble(items, opt.loader, rng))
            trainer.step(lr, opt.momentum)
            total += loss
            batches += 1
        line = 'epoch %d: lr %g, %d batches, magnitude loss %.6f, sign loss %.6f' % (
            epoch, lr, batches, total[0] / max(batches, 1), total[1] / max(batches, 1))
        if test is not None:
            line += '; validation: magnitude loss %.6f, sign loss %.6f' % validate(trainer.state_dict(), opt, test, dev)
        print(line, flush=True)
        if (epoch + 1) % max(opt.save_interval, 1) == 0 or epoch == opt.nepoch - 1:
            torch.save(trainer.state_dict(), model_file)
    for d in (data, test):
        if d is not None:
            d.close()
    return model_file


if __name__ == '__main__':
    train(parse_arguments())
