"""fp32 confirm chains per pooled channel of the screened conv3 on the first N queries of the 256^3 grid of each abc_minimal
cloud (development aid; the device counters of one pipeline call).  usage: python tools/screen_candidates.py [N, default 8192]"""
import glob
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from points2surf_amd import engine, synth  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
w, cfg = synth.make_weights('p2s_max')
model = engine.Model(w, cfg)
out = {}
for path in sorted(glob.glob(os.path.join(ROOT, 'tests', 'golden', 'abc_minimal', '04_pts', '*.xyz.npy'))):
    cloud = engine.Cloud(np.load(path))
    engine.infer_shape(model, cloud, engine.Rng(40938661), 256, 3, q_begin=0, q_end=n, want_queries=False)
    torch.cuda.synchronize()
    c = model.counters()
    items, dense = int(c['conv3_items']), int(c['conv3_items_dense'])
    out[os.path.basename(path)[:8]] = {'queries': n, 'conv3_items': items, 'conv3_items_dense': dense, 'conv3_confirmed': int(c['conv3_confirmed']),
                                       'confirmed_per_channel': c['conv3_confirmed'] / (1024.0 * max(1, items - dense))}
print(json.dumps(out))
