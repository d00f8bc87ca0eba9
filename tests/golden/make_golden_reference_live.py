"""Generate tests/golden/reference_live_golden.npz: the numbers tests/test_oracle_golden.py's live checks read from the REAL reference
(its pointnet2.py, imported read-only with empty cv2/torchvision stubs), recorded so that the same checks run without the reference
checkout.  Needs that checkout:  python tests/golden/make_golden_reference_live.py <reference checkout>

  live_<kind>_y / _tf        eval-mode outputs of PointNetCls(6, 10) / PointNetSeg(6, 300) (seg: [:, ::3, ::4]), seed-31 weights
  live_<kind>_keys / _shapes the reference modules' state_dict names and shapes
  train_<kind>_y / _tf       train-mode forward of PointNetCls(6, 10) / PointNetSeg(6, 30), seed-3 weights, torch seed 0
  train_<kind>_grad_<i>      the gradient of the i-th named parameter after y.square().sum().backward(), <= 128 evenly strided elements
  train_<kind>_state_<i>     the i-th state_dict entry after that step (BatchNorm running statistics), the same sample"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
for m in ('cv2', 'torchvision'):
    sys.modules.setdefault(m, types.ModuleType(m))
sys.path.insert(0, os.path.abspath(sys.argv[1]))
import pointnet2 as ref  # noqa: E402  (the reference implementation itself)

from catgrasp_amd import synth  # noqa: E402

out = {}


def sample(t):
    """<= 128 evenly strided elements of a tensor (tests/test_oracle_golden.py takes the same sample)."""
    return t.detach().flatten()[::max(1, -(-t.numel() // 128))].numpy().copy()


x = torch.from_numpy(np.random.default_rng(5).normal(0, 0.5, (2, 200, 6)).astype(np.float32))
for kind, n_out, cls in (('cls', 10, ref.PointNetCls), ('seg', 300, ref.PointNetSeg)):
    sd = synth.make_state_dict(kind, 6, n_out, seed=31)
    m = cls(6, n_out); m.load_state_dict(sd); m.eval()
    with torch.no_grad():
        y, tf = m(x)
    out[f'live_{kind}_y'] = y.numpy() if kind == 'cls' else y.numpy()[:, ::3, ::4].copy()       # strided sample of (B,N,300)
    out[f'live_{kind}_tf'] = tf.numpy()
    out[f'live_{kind}_keys'] = np.array(list(m.state_dict().keys()))
    out[f'live_{kind}_shapes'] = np.array([','.join(map(str, v.shape)) for v in m.state_dict().values()])

x = torch.from_numpy(np.random.default_rng(8).normal(0, 0.5, (4, 120, 6)).astype(np.float32))
for kind, n_out, name in (('cls', 10, 'PointNetCls'), ('seg', 30, 'PointNetSeg')):
    b = getattr(ref, name)(6, n_out)
    b.load_state_dict(synth.make_state_dict(kind, 6, n_out, seed=3))
    b.train()
    torch.manual_seed(0); y, tf = b(x.clone())
    out[f'train_{kind}_y'], out[f'train_{kind}_tf'] = y.detach().numpy(), tf.detach().numpy()
    y.square().sum().backward()
    for i, (_, p) in enumerate(b.named_parameters()):
        out[f'train_{kind}_grad_{i}'] = sample(p.grad)
    for i, v in enumerate(b.state_dict().values()):
        out[f'train_{kind}_state_{i}'] = sample(v)
path = os.path.join(ROOT, 'tests', 'golden', 'reference_live_golden.npz')
np.savez_compressed(path, **out)
print('wrote', path, os.path.getsize(path), 'bytes')
