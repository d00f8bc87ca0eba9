"""Launch trace of the PointNet++ set-abstraction stack's HIP dispatch (catgrasp_amd/pointnet2.py), on the CPU.

farthest_point_sample, query_ball_point, group_mlp_max, group_all_mlp_max and _raise_if are replaced by recorders under both the
`primitives` and the `pointnet2` names, and pointnet2._use_hip by "the module is in eval mode", so CPU tensors pass the gate (an
eval-mode call that would check its input for NaN / Inf is recorded as 'check_finite').  The recorders return zero tensors of the
right shape, or the `out` they were given.  Only public entry points are driven: a module's forward with (xyz, points, start) or
(x, start).  What is compared is what would reach the kernels, not how pointnet2.py spells the call:
  * the function and its scalars;
  * every tensor as [ordinal of its storage by first appearance in the case, shape, strides, storage offset];
  * the weights as [level, scale index, kind, cin, cout];
  * out=None as the fresh contiguous (B, S, C) tensor the callee would allocate, err=None as the fresh flag it would allocate;
  * every read-back of an index-error flag as (flag, label), the one group_mlp_max(check_indices=True) performs itself included.
The expected traces (tests/golden/pointnet2_dispatch_trace.json) were recorded with this module's own recorder,
`python tests/test_pointnet2_dispatch_cpu.py --record`, on the commit BEFORE the two set-abstraction classes were given one level
body; regenerate them only from a tree whose launches are known good, never to make a failing case pass."""
import inspect
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from catgrasp_amd import pointnet2 as p2  # noqa: E402
from catgrasp_amd import primitives as prim  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pointnet2_dispatch_trace.json')
RECORDED = ('farthest_point_sample', 'query_ball_point', 'group_mlp_max', 'group_all_mlp_max', '_raise_if')
_SIG = {name: inspect.signature(getattr(prim, name)) for name in RECORDED}     # the real signatures, taken before any patching
GROUP_MLP_MAX_LABEL = 'group_mlp_max (a query ball was empty or an index is out of range)'     # primitives.group_mlp_max's own read-back

SSG_SMALL = dict(npoints=(48, 12), radii=(0.3, 0.6), nsamples=(8, 16), mlps=((32, 32, 64), (64, 64, 128), (128, 256)))
# level 1 mixes the kernel families: (32, 32) is a 'reg' shape, a width of 96 goes to 'tile'
MSG_SMALL = dict(msg=True, npoints=(32, 8), radii=((0.2, 0.4), (0.4, 0.8)), nsamples=((4, 8), (8, 16)),
                 mlps=(((32, 32), (32, 96)), ((64, 64), (64, 96)), (128, 256)))


class Recorder:
    def __init__(self, monkeypatch, levels):
        """levels: {module: its name in the trace}"""
        self.events, self.levels = [], levels
        self._storages, self._weights, self._alive = {}, {}, []
        for name in RECORDED:
            monkeypatch.setattr(prim, name, getattr(self, name))
            monkeypatch.setattr(p2, name, getattr(self, name), raising=False)
        monkeypatch.setattr(p2, '_use_hip', self._use_hip)
        self._cached_weights = p2._cached_weights
        monkeypatch.setattr(p2, '_cached_weights', self._register_weights)

    def _use_hip(self, module, x, validated=False):
        if module.training:
            return False
        if p2.VALIDATE_INPUTS and not validated:
            self.events.append({'fn': 'check_finite', 'x': self._tensor(x)})
        return True

    def _register_weights(self, module, device, prepare):
        Ws = self._cached_weights(module, device, prepare)
        for i, W in enumerate(Ws if isinstance(Ws, (list, tuple)) else [Ws]):
            self._weights[id(W)] = [self.levels[module], i, W.kind, list(W.cin), list(W.cout)]
        return Ws

    def _tensor(self, t):
        if t is None:
            return None
        self._alive.append(t)           # a freed storage's address could come back as another tensor's
        ordinal = self._storages.setdefault(t.untyped_storage().data_ptr(), len(self._storages))
        return [ordinal, list(t.shape), list(t.stride()), t.storage_offset()]

    def _bind(self, fn, args, kwargs):
        a = _SIG[fn].bind(*args, **kwargs)
        a.apply_defaults()
        return dict(a.arguments)

    def _emit(self, fn, a):
        c = {'fn': fn}
        for k, v in a.items():
            if isinstance(v, torch.Tensor):
                c[k] = self._tensor(v)
            elif isinstance(v, prim.SetAbstractionWeights):
                c[k] = self._weights[id(v)]
            elif isinstance(v, bool):
                c[k] = int(v)
            else:
                c[k] = v
        self.events.append(c)

    def farthest_point_sample(self, *args, **kwargs):
        a = self._bind('farthest_point_sample', args, kwargs)
        self._emit('farthest_point_sample', a)
        B = a['xyz'].shape[0]
        idx = torch.zeros((B, a['npoint']), dtype=torch.int64)
        return (idx, torch.zeros((B, a['npoint'], 3))) if a['return_xyz'] else idx

    def query_ball_point(self, *args, **kwargs):
        a = self._bind('query_ball_point', args, kwargs)
        self._emit('query_ball_point', a)
        B, N, _ = a['xyz'].shape
        return torch.zeros((B, a['new_xyz'].shape[1], min(int(a['nsample']), N)), dtype=torch.int64)

    def group_mlp_max(self, *args, **kwargs):
        a = self._bind('group_mlp_max', args, kwargs)
        check = a.pop('check_indices')
        B, S, C = a['xyz'].shape[0], a['idx'].shape[1], a['W'].cout[-1]
        if a['out'] is None:
            a['out'] = torch.zeros((B, S, C) if a['channels_last'] else (B, C, S))
        if a['err'] is None:
            a['err'] = torch.zeros((1,), dtype=torch.int32)
        self._emit('group_mlp_max', a)
        if not check:
            return a['out'], a['err']
        self._raise_if(a['err'], GROUP_MLP_MAX_LABEL)
        return a['out']

    def group_all_mlp_max(self, *args, **kwargs):
        a = self._bind('group_all_mlp_max', args, kwargs)
        self._emit('group_all_mlp_max', a)
        return torch.zeros((a['xyz'].shape[0], a['W'].cout[-1]))

    def _raise_if(self, err, what):
        self.events.append({'fn': 'read_back', 'err': self._tensor(err), 'what': what})


def _encoder(train=(), B=2, **cfg):
    assert B < p2.SIDE_STREAM_MIN_CLOUDS            # the side-stream branch needs real streams: covered on the GPU

    def make():
        enc = p2.PointNet2Encoder(**cfg).eval()
        for name in train:
            getattr(enc, name).train()
        N = 600
        x = torch.zeros(B, N, enc.channel)
        start = (torch.arange(B) % N, torch.arange(B) % enc.sa1.npoint)
        return {enc.sa1: 'sa1', enc.sa2: 'sa2', enc.sa3: 'sa3'}, lambda: enc(x, start=start)
    return make


def _layer(cls, *args, D=3, points=True, **kwargs):
    def make():
        sa = cls(*args, **kwargs).eval()
        B, N = 2, 200
        xyz = torch.zeros(B, N, 3)
        pts = torch.zeros(B, N, D) if points else None
        return {sa: 'sa'}, lambda: sa(xyz, pts, start=torch.tensor([0, 7]))
    return make


CASES = {
    'enc_ssg_small': _encoder(channel=6, **SSG_SMALL),
    'enc_ssg_default': _encoder(channel=6),
    'enc_msg_small': _encoder(channel=6, **MSG_SMALL),
    'enc_msg_default': _encoder(channel=6, msg=True, B=1),
    'enc_ssg_small_channel3': _encoder(channel=3, **SSG_SMALL),
    'enc_msg_small_channel3': _encoder(channel=3, **MSG_SMALL),
    'enc_ssg_small_sa2_in_train_mode': _encoder(channel=6, train=('sa2',), **SSG_SMALL),
    'sa_with_points': _layer(p2.PointNetSetAbstraction, 32, 0.2, 8, 3 + 3, [32, 64]),
    'sa_without_points': _layer(p2.PointNetSetAbstraction, 32, 0.2, 8, 3, [32, 64], points=False),
    'sa_tile_kind': _layer(p2.PointNetSetAbstraction, 32, 0.2, 8, 3 + 3, [64, 128, 256]),
    'sa_group_all': _layer(p2.PointNetSetAbstraction, None, None, None, 3 + 5, [64, 128], group_all=True, D=5),
    'msg_layer': _layer(p2.PointNetSetAbstractionMsg, 32, [0.1, 0.2], [8, 16], 3, [[32, 32], [32, 96]]),
}


def _trace(monkeypatch, case):
    torch.manual_seed(0)
    levels, run = CASES[case]()
    rec = Recorder(monkeypatch, levels)
    with torch.no_grad():
        run()
    return json.loads(json.dumps(rec.events))      # tuples -> lists, as the fixture holds them


@pytest.fixture(scope='module')
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize('case', list(CASES))
def test_launch_trace(monkeypatch, golden, case):
    got, want = _trace(monkeypatch, case), golden[case]
    assert [c['fn'] for c in got] == [c['fn'] for c in want], case
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (case, i)


def test_every_golden_case_is_exercised(golden):
    assert sorted(golden) == sorted(CASES)
    assert all(golden[c] for c in CASES)


def test_traces_hold_what_the_cases_are_there_for(golden):
    """The fixture itself: a mixed-kind multi-scale level, a train-mode level that launches nothing, one read-back per stack."""
    fns = lambda case, fn: [c for c in golden[case] if c['fn'] == fn]
    assert [c['W'][2] for c in fns('enc_msg_small', 'group_mlp_max')] == ['reg', 'tile', 'tile', 'tile']
    assert [c['append_xyz'] for c in fns('enc_msg_small', 'group_mlp_max')] == [0, 0, 0, 168 - 160]     # rows of roundup8(64 + 96 + 3)
    assert fns('sa_tile_kind', 'group_mlp_max')[0]['W'][2] == 'tile' and fns('sa_with_points', 'group_mlp_max')[0]['W'][2] == 'reg'
    for case in CASES:
        if case.startswith('enc_') and 'train' not in case:
            assert [c['what'].split(' ')[0] for c in fns(case, 'read_back')] == ['PointNet2Encoder'], case
            assert len(fns(case, 'check_finite')) == 1, case
    mixed = golden['enc_ssg_small_sa2_in_train_mode']
    assert {c['W'][0] for c in mixed if 'W' in c} == {'sa1', 'sa3'}
    assert [c['what'] for c in mixed if c['fn'] == 'read_back'] == [GROUP_MLP_MAX_LABEL]
    assert [c['what'].split(' ')[0] for c in fns('msg_layer', 'read_back')] == ['PointNetSetAbstractionMsg']


def _record():
    traces = {}
    for case in CASES:
        mp = pytest.MonkeyPatch()
        try:
            traces[case] = _trace(mp, case)
        finally:
            mp.undo()
    with open(FIXTURE, 'w') as f:
        json.dump(traces, f, separators=(',', ':'), sort_keys=True)
        f.write('\n')
    print(f'{FIXTURE}: {len(traces)} cases, {sum(len(t) for t in traces.values())} events, {os.path.getsize(FIXTURE)} bytes')


if __name__ == '__main__':
    if sys.argv[1:] != ['--record']:
        sys.exit('usage: python tests/test_pointnet2_dispatch_cpu.py --record     (on a tree whose launches are known good)')
    _record()
