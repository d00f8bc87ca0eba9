"""Generate tests/golden/nocs_loss_golden.npz by running the REAL `loss.NocsMinSymmetryCELoss` (loss.py:16-45) on the CPU, forward and
autograd's backward, for nut and screw at B = 2, N = 64, bins = 100, float32.  Build container only.  Uninstallable imports are inert
stubs and `Tensor.cuda()` is the identity, as in make_golden_predicter.py; `transformations` is a stub there, so the reference's
`get_symmetry_tfs` (Utils.py:79-94) cannot run and the transforms come from catgrasp_amd.transforms.get_symmetry_tfs (tested against
the reference's formula in test_transforms_cpu.py).  The inputs come from tests/nocs_loss_ref.make_inputs (targets kept 1e-3 away from
every bin boundary) and are rebuilt from their seeds by the test, so the file holds only a digest of them next to the outputs: the
loss, the gradient's most negative bin per (sample, point, axis) -- the winning symmetry's one-hot position -- and every GRAD_STEP-th
point's gradient."""
import importlib.abc
import importlib.machinery
import os
import sys
import types
from unittest import mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


class StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    roots = ('cv2', 'torchvision', 'open3d', 'trimesh', 'autolab_core', 'pybullet', 'pybullet_data', 'mayavi', 'pybullet_tools', 'pyrender',
             'imgaug', 'skimage', 'ikfast_pybind', 'my_cpp', 'data_reader', 'renderer', 'PointGroup', 'spconv', 'torchprof')

    def find_spec(self, name, path, target=None):
        if name.split('.')[0] in self.roots:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
        return None

    def create_module(self, spec):
        m = mock.MagicMock(name=spec.name)
        m.__name__ = spec.name; m.__path__ = []; m.__spec__ = spec; m.__all__ = []
        return m

    def exec_module(self, module):
        pass


tf_mod = types.ModuleType('transformations'); tf_mod.__all__ = []
sys.modules['transformations'] = tf_mod
sys.meta_path.insert(0, StubFinder())
sys.path.insert(0, '/root/reference')
import loss as ref_loss  # noqa: E402

import nocs_loss_ref as nref  # noqa: E402
from catgrasp_amd.transforms import get_symmetry_tfs  # noqa: E402

torch.Tensor.cuda = lambda self, *a, **k: self          # run the reference's .cuda() path on the CPU
ref_loss.get_symmetry_tfs = get_symmetry_tfs
torch.set_num_threads(1)

B, N, BINS, GRAD_STEP = 2, 64, 100, 32
out = {}
for seed, name in ((5, 'nut'), (6, 'screw')):
    crit = ref_loss.NocsMinSymmetryCELoss({'nocs_class_name': name, 'ce_loss_bins': BINS})
    tfs = crit.symmetry_tfs.numpy()
    pred, target, _ = nref.make_inputs(seed, B, N, BINS, tfs)
    x = torch.from_numpy(pred.reshape(B, N, 3 * BINS)).requires_grad_(True)
    loss = crit(x, torch.from_numpy(target))
    loss.backward()
    grad = x.grad.numpy().reshape(B, N, 3, BINS)
    out.update({f'{name}_seed': np.int64(seed), f'{name}_digest': np.array([pred.astype(np.float64).sum(), target.astype(np.float64).sum()]),
                f'{name}_loss': loss.detach().numpy(), f'{name}_onehot': grad.argmin(-1).astype(np.int16), f'{name}_grad': grad[:, ::GRAD_STEP]})
    print(name, float(loss.detach()), tfs.shape)
out['shape'] = np.array([B, N, BINS, GRAD_STEP])
np.savez_compressed(os.path.join(HERE, 'nocs_loss_golden.npz'), **out)
