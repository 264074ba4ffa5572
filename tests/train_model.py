"""TEST INFRASTRUCTURE ONLY -- the project's restatement of the TRAIN-mode forward of ``p2s_max`` /
``p2s_max_no_feat_stn``, the two losses and the SGD update, with torch functional ops over a state dict.

Follows reference source/points_to_surf_model.py:41-69 (STN), :177-234 (PointNetfeat), :296-352 (PointsToSurfModel),
source/points_to_surf_train.py:537-563 (compute_loss) and source/sdf_nn.py:30-40.  Gradients come from autograd, the
update from ``torch.optim.SGD``.  Any dtype (float64 is the yardstick of the device tests, float32 measures what single
precision alone costs).  A max-pool can be FORCED to given indices -- a gather in place of the max -- so that two
precisions (or the device and the CPU) differentiate the same piecewise-linear function where near-ties resolve differently.
A ReLU can be forced in the same way to given masks (``forced_relu``): a pre-activation within rounding of zero is let
through by one precision and not by the other, which is the same kind of tie.
"""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

POOLS_FEAT_STN = ('feat_local.stn2', 'feat_local', 'feat_global.stn2', 'feat_global')
POOLS_PLAIN = ('feat_local', 'feat_global')


def pool_names(cfg):
    return POOLS_FEAT_STN if cfg.get('use_feat_stn', True) else POOLS_PLAIN


def is_buffer(name):
    return name.endswith(('running_mean', 'running_var', 'num_batches_tracked'))


def zero_grad_bias(name):
    """a conv / fc bias in front of a batch-norm: the batch mean removes it, its gradient is zero in exact arithmetic"""
    if not name.endswith('.bias') or name.split('.')[-2].startswith('bn'):
        return False
    return not (name == 'fc4.bias' or name.endswith('stn2.fc3.bias'))


def zero_grad_names(grads64):
    """the biases whose FLOAT64 gradient is rounding noise (below 1e-9 of their layer's weight gradient): every bias of
    ``zero_grad_bias``, and two kinds of batch-norm bias in front of a max-pool that feeds fc + batch-norm -- bn3.bias of
    PointNetfeat (a per-channel constant through the pool) and stn2.bn3.bias while every pooled maximum is positive (the
    pooled gradient sums to zero over the batch).  A relative error against such a reference is meaningless; they are
    compared against the weight gradient of their layer instead"""
    out = set()
    for k, v in grads64.items():
        if k.endswith('.bias') and np.linalg.norm(v) <= 1e-9 * np.linalg.norm(grads64[k[:-4] + 'weight']):
            out.add(k)
    missing = [k for k in grads64 if zero_grad_bias(k) and k not in out]
    assert not missing, missing
    return out


class TrainModel:
    def __init__(self, weights, cfg, dtype=torch.float64, device='cpu', record=True):
        """``device`` / ``record=False``: the same step on a GPU through torch, without the host copies of the pool
        indices (tools/train_bench.py times it)"""
        self.cfg = dict(cfg)
        self.dtype = dtype
        self.device, self.record = torch.device(device), record
        self.w = OrderedDict()
        for k, v in weights.items():
            v = np.asarray(v)
            if k.endswith('num_batches_tracked'):
                self.w[k] = torch.tensor(int(v), dtype=torch.int64, device=self.device)
            elif is_buffer(k):
                self.w[k] = torch.from_numpy(v.astype(np.float64)).to(self.device, dtype).clone()
            else:
                self.w[k] = torch.from_numpy(v.astype(np.float64)).to(self.device, dtype).clone().requires_grad_(True)
        self.opt = None
        self.pools = {}

    def params(self):
        return OrderedDict((k, v) for k, v in self.w.items() if not is_buffer(k))

    # -- layers --------------------------------------------------------------------------------------------------
    def _bn(self, x, bn):
        w = self.w
        w[bn + '.num_batches_tracked'] += 1
        return F.batch_norm(x, w[bn + '.running_mean'], w[bn + '.running_var'], w[bn + '.weight'], w[bn + '.bias'],
                            True, 0.1, 1e-5)

    def _conv_bn(self, x, conv, bn, relu=True):
        x = self._bn(F.conv1d(x, self.w[conv + '.weight'], self.w[conv + '.bias']), bn)
        return self._relu(x) if relu else x

    def _fc_bn(self, x, fc, bn):
        return self._relu(self._bn(F.linear(x, self.w[fc + '.weight'], self.w[fc + '.bias']), bn))

    def _relu(self, x):
        """forced: the mask of this call (in the order of the forward) replaces x > 0.  Where the two differ, |x| over the
        largest |x| of its channel in this layer is kept in ``self.relu_ties``, and ``self.relu_units`` counts all units"""
        j = len(self.relu_ties)
        if self.forced_relu is None:
            self.relu_ties.append(np.zeros(0))
            return F.relu(x)
        mask = torch.as_tensor(np.asarray(self.forced_relu[j])).to(self.device) != 0
        assert mask.shape == x.shape, (j, mask.shape, x.shape)
        xd = x.detach()
        dims = (0, 2) if xd.dim() == 3 else (0,)
        ratio = xd.abs() / xd.abs().amax(dim=dims, keepdim=True).clamp_min(1e-300)
        self.relu_ties.append(ratio[mask != (xd > 0)].cpu().numpy().astype(np.float64))
        self.relu_units += xd.numel()
        return x * mask.to(x.dtype)

    def _pool(self, x, name, forced):
        if forced is not None:
            idx = torch.as_tensor(np.asarray(forced[name]), dtype=torch.int64).to(self.device)
            self.pools[name] = idx.cpu().numpy().astype(np.int32)
            return x.gather(2, idx.unsqueeze(2)).squeeze(2)
        v, idx = F.max_pool1d(x, x.shape[2], return_indices=True)
        if not self.record:
            return v.squeeze(2)
        self.pools[name] = idx.squeeze(2).cpu().numpy().astype(np.int32)
        self.pool_inputs[name] = x.detach()
        return v.squeeze(2)

    def _trunk(self, x, pre, forced):
        x = self._conv_bn(x, pre + '.conv1', pre + '.bn1')
        x = self._conv_bn(x, pre + '.conv2', pre + '.bn2')
        x = self._conv_bn(x, pre + '.conv3', pre + '.bn3')
        x = self._pool(x, pre, forced)
        x = self._fc_bn(x, pre + '.fc1', pre + '.bn4')
        x = self._fc_bn(x, pre + '.fc2', pre + '.bn5')
        return F.linear(x, self.w[pre + '.fc3.weight'], self.w[pre + '.fc3.bias'])

    def _feat(self, x, pre, forced):
        x = self._conv_bn(x, pre + '.conv0a', pre + '.bn0a')
        x = self._conv_bn(x, pre + '.conv0b', pre + '.bn0b')
        if self.cfg.get('use_feat_stn', True):
            t = self._trunk(x, pre + '.stn2', forced)
            t = (t + torch.eye(64, dtype=x.dtype, device=x.device).view(1, 4096)).view(-1, 64, 64)
            x = torch.bmm(t, x)
        x = self._conv_bn(x, pre + '.conv1', pre + '.bn1')
        x = self._conv_bn(x, pre + '.conv2', pre + '.bn2')
        x = self._conv_bn(x, pre + '.conv3', pre + '.bn3', relu=False)
        return self._pool(x, pre, forced)

    def forward(self, patch_ps, sub_ms, query, forced=None, forced_relu=None):
        """-> pred [B, 2]; the batch-norms run on batch statistics and update their running buffers.  The pooled indices of
        this call are left in ``self.pools`` (and the pooled tensors in ``self.pool_inputs`` when nothing is forced).
        ``forced_relu``: one 0 / 1 array per ReLU in the order of this forward, shaped like its input"""
        self.pools, self.pool_inputs = {}, {}
        self.forced_relu, self.relu_ties, self.relu_units = forced_relu, [], 0
        dt, dev = self.dtype, self.device
        as_t = lambda a: (a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))).to(dev, dt)
        patch = as_t(patch_ps).transpose(1, 2)
        shape = (as_t(sub_ms) - as_t(query).unsqueeze(1)).transpose(1, 2)
        g = self._fc_bn(self._feat(shape.contiguous(), 'feat_global', forced), 'fc1_global', 'bn1_global')
        l = self._fc_bn(self._feat(patch.contiguous(), 'feat_local', forced), 'fc1_local', 'bn1_local')
        f = torch.cat((l, g), dim=1)
        f = self._fc_bn(f, 'fc2', 'bn2')
        f = self._fc_bn(f, 'fc3', 'bn3')
        return F.linear(f, self.w['fc4.weight'], self.w['fc4.bias'])

    def losses(self, pred, dist_abs, sign01, radius):
        dt, dev = self.dtype, self.device
        as_t = lambda a: (a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))).to(dev, dt)
        target = as_t(dist_abs) / as_t(radius)
        mag = F.mse_loss(torch.tanh(torch.abs(pred[:, 0])), torch.tanh(torch.abs(target)))
        sgn = F.binary_cross_entropy_with_logits(pred[:, 1], as_t(sign01), reduction='none').mean()
        return mag, sgn

    def forward_backward(self, patch_ps, sub_ms, query, dist_abs, sign01, radius, forced=None, forced_relu=None):
        """-> (magnitude loss, sign loss) as floats; gradients are left in the parameters' ``.grad``"""
        for p in self.params().values():
            p.grad = None
        pred = self.forward(patch_ps, sub_ms, query, forced, forced_relu)
        self.pred = pred.detach().cpu().numpy().astype(np.float64) if self.record else None
        mag, sgn = self.losses(pred, dist_abs, sign01, radius)
        (mag + sgn).backward()
        return float(mag.detach()), float(sgn.detach())

    def grads(self):
        return OrderedDict((k, v.grad.detach().cpu().numpy().copy()) for k, v in self.params().items())

    def step(self, lr, momentum):
        if self.opt is None:
            self.opt = torch.optim.SGD(list(self.params().values()), lr=lr, momentum=momentum)
        for g in self.opt.param_groups:
            g['lr'] = lr
            g['momentum'] = momentum
        self.opt.step()

    def state(self):
        return OrderedDict((k, v.detach().cpu().numpy().copy()) for k, v in self.w.items())


def make_batch(B, P, S, seed, pad_duplicates=False):
    """a seeded synthetic batch with the value ranges of the data path: patch in patch space (unit ball), sub-sample and
    query in model space (unit cube), |d| below the patch radius.  ``pad_duplicates``: the second half of item 0's patch
    and sub-sample repeats its first point, as a padded patch does -- exact ties in every max-pool"""
    rng = np.random.default_rng(seed)
    patch = rng.standard_normal((B, P, 3))
    patch = (patch / np.linalg.norm(patch, axis=2, keepdims=True) * rng.uniform(0, 1, (B, P, 1)) ** (1 / 3)).astype(np.float32)
    sub = rng.uniform(-0.5, 0.5, (B, S, 3)).astype(np.float32)
    query = rng.uniform(-0.4, 0.4, (B, 3)).astype(np.float32)
    radius = rng.uniform(0.05, 0.2, (B,)).astype(np.float32)
    dist_abs = (radius * rng.uniform(0, 1.5, (B,))).astype(np.float32)
    sign01 = (rng.uniform(0, 1, (B,)) < 0.5).astype(np.float32)
    if pad_duplicates:
        patch[0, P // 2:] = patch[0, 0]
        sub[0, S // 2:] = sub[0, 0]
    return dict(patch=patch, sub=sub, query=query, dist_abs=dist_abs, sign01=sign01, radius=radius)


def rel_err(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    n = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / n) if n > 0 else float(np.linalg.norm(a))


GOLDEN_FULL_BELOW = 4096
GOLDEN_SAMPLES = 1024


def golden_view(a):
    """what the train goldens keep of one tensor: all of it below 4,096 elements, else 1,024 positions seeded by its size"""
    a = np.asarray(a).ravel()
    if a.size < GOLDEN_FULL_BELOW:
        return a
    return a[np.sort(np.random.default_rng(a.size).choice(a.size, GOLDEN_SAMPLES, replace=False))]


def loss_gates(pred32, pred64, losses64, factor=4.0):
    """absolute gates for (magnitude loss, sign loss) of an fp32 implementation that sums in another order: both losses are
    means over the items of functions of one logit with |d/dp (tanh|p| - t)^2| <= 2 and |d/dp BCE| <= 1, so a loss moves by at
    most that constant times the largest logit error.  The logit error of single precision on THESE inputs is measured
    (float32 against float64 restatement, same forced pool indices); ``factor`` covers the other summation order.  The
    difference of the two precisions' LOSSES would underestimate it: the items' errors cancel in the mean.  Floor: the
    rounding of the loss itself"""
    d = np.abs(np.asarray(pred32, np.float64) - np.asarray(pred64, np.float64)).max(axis=0)
    return [factor * lip * float(dj) + 4 * 2.0 ** -24 * abs(l) for lip, dj, l in zip((2.0, 1.0), d, losses64)]
