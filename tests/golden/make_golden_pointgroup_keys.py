"""state_dict key names and shapes of the reference's PointGroup network at its shipped configuration.  Build container only
(/root/reference).  The REAL PointGroup/model/pointgroup/pointgroup.py is imported and constructed; the packages it imports that
cannot be installed here are stubbed: `spconv` (containers and layers that only register parameters in spconv 1.x's layout, weight
(k0, k1, k2, Cin, Cout) and bias (Cout)), `lib.pointgroup_ops.functions`, `util` and `Utils` (unused by the constructor).  No weight
values are written: names, order and shapes only.

    python tests/golden/make_golden_pointgroup_keys.py      ->  tests/golden/pointgroup_state_keys.json
"""
import argparse
import json
import os
import sys
import types
from collections import OrderedDict

import torch
import yaml
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get('CATGRASP_REFERENCE', '/root/reference')


class SparseModule(nn.Module):
    pass


class SparseSequential(SparseModule):
    def __init__(self, *args, **kwargs):
        super().__init__()
        if len(args) == 1 and isinstance(args[0], OrderedDict):
            for key, module in args[0].items():
                self.add_module(key, module)
        else:
            for idx, module in enumerate(args):
                self.add_module(str(idx), module)
        for name, module in kwargs.items():
            self.add_module(name, module)


class _Conv(SparseModule):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True, indice_key=None):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(kernel_size, kernel_size, kernel_size, in_channels, out_channels))
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_channels))


def main():
    spconv = types.ModuleType('spconv')
    spconv.SparseSequential, spconv.SubMConv3d, spconv.SparseConv3d, spconv.SparseInverseConv3d = SparseSequential, _Conv, _Conv, _Conv
    spconv.modules = types.ModuleType('spconv.modules')
    spconv.modules.SparseModule = SparseModule
    stubs = {'spconv': spconv, 'spconv.modules': spconv.modules}
    for name in ('lib', 'lib.pointgroup_ops', 'lib.pointgroup_ops.functions', 'util', 'Utils'):
        stubs[name] = types.ModuleType(name)
    stubs['lib.pointgroup_ops.functions'].pointgroup_ops = None
    stubs['util'].utils = None
    stubs['Utils'].__all__ = []
    sys.modules.update(stubs)
    sys.path.insert(0, os.path.join(REFERENCE, 'PointGroup', 'model', 'pointgroup'))
    import pointgroup as ref_pointgroup

    with open(os.path.join(REFERENCE, 'PointGroup', 'config', 'config_pointgroup.yaml')) as f:
        config = yaml.safe_load(f)
    cfg = argparse.Namespace()
    for section in config.values():
        if isinstance(section, dict):
            for k, v in section.items():
                setattr(cfg, k, v)
    model = ref_pointgroup.PointGroup(cfg)
    entries = [[k, list(v.shape), str(v.dtype).replace('torch.', '')] for k, v in model.state_dict().items()]
    with open(os.path.join(HERE, 'pointgroup_state_keys.json'), 'w') as f:
        f.write('[\n' + ',\n'.join(json.dumps(e) for e in entries) + '\n]\n')      # one entry per line
    print(len(entries), 'entries')


if __name__ == '__main__':
    main()
