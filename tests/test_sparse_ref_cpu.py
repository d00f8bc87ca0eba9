"""Pins the yardstick tests/sparse_ref.py: its rule-book restatement of the three sparse convolution layers equals dense float64
torch convolutions to 1e-12 on the scenes that tests/test_sparse_conv_gpu.py uses, with and without the BatchNorm/ReLU prologue
(applied to the sparse rows, then densified) and the residual.  No GPU, no kernel of catgrasp_amd.

Its bitwise model conv_exact (float32, the kernel's own chain) is proved three ways: it lies within gamma(K*cin + 2) * (sum |products|
+ |bias| + |residual|) of the float64 restatement per element, both as that restatement stands and, rigorously, when the restatement
is fed the float32 prologue values the chain reads; it is sensitive to each way a kernel could keep the value and lose the bits (channel order, a
contracted prologue, the epilogue's association, the order of the offsets); and it does not depend on whether an absent row is
skipped or gathered as zeros.  The edge scenes of tests/test_sparse_rules_edges_gpu.py hold what they claim."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sparse_ref as ref
from dense_ref import gamma

SCENES = [dict(n=299), dict(n=1, special=False), dict(n=33, special=False), dict(n=301, seed=5), dict(n=120, special=False, only_item=1)]
IDS = ['full299', 'n1', 'n33', 'n301', 'empty_item0']
CIN, COUT = 6, 5


def _setup(kw, k):
    idx = ref.scene(**kw)
    x = ref.features(len(idx), CIN).astype(np.float64)
    w, b = ref.weights(k, CIN, COUT)
    return idx, x, w.astype(np.float64), b.astype(np.float64)


def _variants(n_out):
    scale, shift = ref.bn_params(CIN)
    res = np.random.default_rng(9).uniform(-1, 1, (n_out, COUT))
    return [(None, None, None), (scale, shift, None), (None, None, res), (scale, shift, res)]


def _pro(x, scale, shift):
    return x if scale is None else np.maximum(x * scale.astype(np.float64) + shift.astype(np.float64), 0.0)


def _at(dense_out, idx):
    return dense_out[idx[:, 0], :, idx[:, 1], idx[:, 2], idx[:, 3]]


def test_the_full_scene_holds_every_trap():
    idx = ref.scene()
    sites = {tuple(r) for r in idx.tolist()}
    assert len(idx) == 299 and len(sites) == 299 and idx.dtype == np.int32
    assert {(0, 0, 0, 0), (1, 8, 11, 16), (0, 3, 4, 16), (0, 3, 5, 0), (0, 5, 6, 7), (1, 5, 6, 7)} <= sites
    nbr = ref.subm_rules(idx, ref.SHAPE)
    row = {tuple(r): i for i, r in enumerate(idx.tolist())}
    assert (nbr[row[(1, 2, 9, 3)]] >= 0).sum() == 1                              # isolated: only itself
    assert (nbr[row[(0, 2, 2, 11)]] >= 0).all()                                  # centre of the full block
    assert row[(0, 3, 5, 0)] not in nbr[row[(0, 3, 4, 16)]] and row[(1, 5, 6, 7)] not in nbr[row[(0, 5, 6, 7)]]
    assert (nbr[:, 13] == np.arange(299)).all()
    _, _, out_shape, dropped = ref.down_rules(idx, ref.SHAPE)
    assert out_shape == (4, 6, 8) and 6 <= dropped.sum() < 150
    assert sorted(set(idx[:, 0].tolist())) == [0, 1]
    assert not np.array_equal(idx, idx[np.argsort(ref.linear_key(idx, ref.SHAPE))])          # the rows are not in key order


@pytest.mark.parametrize('kw', SCENES, ids=IDS)
def test_subm_equals_dense_conv3d(kw):
    idx, x, w, b = _setup(kw, 3)
    nbr = ref.subm_rules(idx, ref.SHAPE)
    wt = torch.from_numpy(w).permute(4, 3, 0, 1, 2).contiguous()
    for scale, shift, res in _variants(len(idx)):
        got = ref.conv(x, nbr, w, b, scale, shift, res)
        want = _at(F.conv3d(torch.from_numpy(ref.dense(idx, _pro(x, scale, shift), ref.BATCH, ref.SHAPE)), wt, torch.from_numpy(b), padding=1).numpy(), idx)
        want = want + (0 if res is None else res)
        assert np.abs(got - want).max() <= 1e-12


def test_subm_k1_is_a_matrix_product():
    idx, x, w, b = _setup(dict(n=299), 1)
    got = ref.conv(x, np.arange(len(idx), dtype=np.int32)[:, None], w, b)
    assert np.abs(got - (x @ w.reshape(CIN, COUT) + b)).max() <= 1e-12


@pytest.mark.parametrize('kw', SCENES, ids=IDS)
def test_down_equals_dense_strided_conv3d(kw):
    idx, x, w, b = _setup(kw, 2)
    out_idx, nbr, out_shape, dropped = ref.down_rules(idx, ref.SHAPE)
    assert out_shape == (4, 6, 8)
    keys = ref.linear_key(out_idx, out_shape)
    assert (np.diff(keys) > 0).all()
    used = np.zeros(len(idx), bool); used[nbr[nbr >= 0]] = True
    assert np.array_equal(used, ~dropped) and (nbr >= 0).sum() == (~dropped).sum()
    wt = torch.from_numpy(w).permute(4, 3, 0, 1, 2).contiguous()
    for scale, shift, res in _variants(len(out_idx)):
        got = ref.conv(x, nbr, w, b, scale, shift, res)
        full = F.conv3d(torch.from_numpy(ref.dense(idx, _pro(x, scale, shift), ref.BATCH, ref.SHAPE)), wt, None, stride=2).numpy()
        assert full.shape[2:] == out_shape
        if len(out_idx):
            want = _at(full, out_idx) + b + (0 if res is None else res)
            assert np.abs(got - want).max() <= 1e-12
        active = np.zeros((ref.BATCH,) + out_shape, bool)
        active[out_idx[:, 0], out_idx[:, 1], out_idx[:, 2], out_idx[:, 3]] = True
        assert np.abs(np.moveaxis(full, 1, -1)[~active]).max(initial=0.0) == 0.0          # no output site is missing


@pytest.mark.parametrize('kw', SCENES, ids=IDS)
def test_inverse_equals_dense_conv_transpose3d(kw):
    idx, _, w, b = _setup(kw, 2)
    w = np.ascontiguousarray(np.swapaxes(w, 3, 4))          # this layer's own Cin -> Cout: COUT channels in, CIN out
    b = ref.weights(2, COUT, CIN, seed=4)[1].astype(np.float64)
    out_idx, _, out_shape, dropped = ref.down_rules(idx, ref.SHAPE)
    nbr = ref.inverse_rules(idx, out_idx, ref.SHAPE)
    assert np.array_equal((nbr >= 0).sum(1), (~dropped).astype(int))
    y = np.random.default_rng(8).uniform(-1, 1, (len(out_idx), COUT))
    wt = torch.from_numpy(w).permute(3, 4, 0, 1, 2).contiguous()
    scale, shift = ref.bn_params(COUT)
    res = np.random.default_rng(9).uniform(-1, 1, (len(idx), CIN))
    for sc, sh, r in [(None, None, None), (scale, shift, None), (None, None, res), (scale, shift, res)]:
        got = ref.conv(y, nbr, w, b, sc, sh, r)
        up = F.conv_transpose3d(torch.from_numpy(ref.dense(out_idx, _pro(y, sc, sh), ref.BATCH, out_shape)), wt, None, stride=2).numpy()
        full = np.zeros((ref.BATCH, CIN) + ref.SHAPE)
        full[:, :, :up.shape[2], :up.shape[3], :up.shape[4]] = up          # zero-padded up to the fine shape
        want = _at(full, idx) + b + (0 if r is None else r)
        assert np.abs(got - want).max() <= 1e-12
        if r is None and dropped.any():
            assert np.array_equal(got[dropped], np.broadcast_to(b, (dropped.sum(), CIN)))          # a dropped site gets the bias only


# ------------------------------------------------------------------------------------------------------- conv_exact
def _tables96():
    idx = ref.scene(n=96)
    out_idx, down, _, _ = ref.down_rules(idx, ref.SHAPE)
    n, m = len(idx), len(out_idx)
    return {'subm': (ref.subm_rules(idx, ref.SHAPE), n, n), 'down': (down, n, m), 'inverse': (ref.inverse_rules(idx, out_idx, ref.SHAPE), m, n),
            'k1': (np.arange(n, dtype=np.int32).reshape(n, 1), n, n)}


def _case(nbr, n_in, n_out, cin, cout, full):
    """Inputs of one launch; full: with prologue, bias and residual."""
    K = nbr.shape[1]
    x = ref.features(n_in, cin)
    rng = np.random.default_rng(9)
    w = rng.uniform(-1, 1, (K, cin, cout)).astype(np.float32) * np.float32(np.sqrt(3.0 / cin))
    if not full:
        return dict(x=x, nbr=nbr, w=w)
    scale, shift = ref.bn_params(cin)
    return dict(x=x, nbr=nbr, w=w, bias=rng.uniform(-1, 1, cout).astype(np.float32), scale=scale, shift=shift,
                residual=rng.uniform(-1, 1, (n_out, cout)).astype(np.float32))


def _on_prologue_values(kw):
    """The launch with the float32 prologue applied beforehand: what the chain reads, and no scale or shift."""
    kw = dict(kw)
    scale, shift = kw.pop('scale', None), kw.pop('shift', None)
    if scale is not None:
        kw['x'] = ref.prologue_f32(kw['x'], scale, shift)
    return kw


def _bound(x, nbr, w, bias=None, scale=None, shift=None, residual=None):
    """Per element gamma(K*cin + 2) * (sum |products| + |bias| + |residual|): K*cin fmaf roundings and two adds.  The products are
    those of the float32 prologue values the chain reads."""
    K, cin, cout = w.shape
    p = np.abs((x if scale is None else ref.prologue_f32(x, scale, shift)).astype(np.float64))
    aw = np.abs(w.astype(np.float64))
    mag = np.zeros((nbr.shape[0], cout))
    for k in range(K):
        rows = np.nonzero(nbr[:, k] >= 0)[0]
        mag[rows] += p[nbr[rows, k]] @ aw[k]
    mag += 0 if bias is None else np.abs(bias.astype(np.float64))
    mag += 0 if residual is None else np.abs(residual.astype(np.float64))
    return gamma(K * cin + 2) * mag


def _check_bound(kw, what=None):
    """conv_exact against the float64 conv within _bound, twice: against conv as it stands (its prologue in float64), and against
    conv on the float32 prologue values, for which the bound is rigorous (every rounding it leaves out happens before the chain).
    -> conv_exact's output"""
    got, bound = ref.conv_exact(**kw), _bound(**kw)
    assert got.dtype == np.float32
    for name, want in (('float64 conv', ref.conv(**kw)), ('float64 conv on the float32 prologue values', ref.conv(**_on_prologue_values(kw)))):
        assert got.shape == want.shape
        err = np.abs(got.astype(np.float64) - want)
        if what:
            print(f'{what} against {name}: max err / bound = {(err / np.maximum(bound, 1e-300)).max():.3g}, max err {err.max():.3g}')
        assert (err <= bound).all(), (what, name)
    return got


@pytest.mark.parametrize('cin,cout', [(6, 3), (32, 48), (224, 112)])
def test_conv_exact_is_within_the_rounding_bound_of_the_float64_restatement(cin, cout):
    for kind, (nbr, n_in, n_out) in _tables96().items():
        for full in (False, True):
            kw = _case(nbr, n_in, n_out, cin, cout, full)
            got = _check_bound(kw, f'{kind} {cin}->{cout} full {full}')
            assert got.shape == (n_out, cout)
            assert np.abs(got.astype(np.float64) - ref.conv(**kw)).max() > 0 or cin * nbr.shape[1] <= 6          # float32 rounding is there to be seen


def test_conv_exact_on_the_edge_scenes_is_within_the_bound():
    for name in ('large', 'dense', 'two'):
        idx, shape, _ = ref.edge_scene(name)
        out_idx, down, _, _ = ref.down_rules(idx, shape)
        for nbr, n_in, n_out in ((ref.subm_rules(idx, shape), len(idx), len(idx)), (down, len(idx), len(out_idx)),
                                 (ref.inverse_rules(idx, out_idx, shape), len(out_idx), len(idx))):
            kw = _case(nbr, n_in, n_out, 16, 16, True)
            _check_bound(kw)


def _share(a, b):
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape
    return float((a.view(np.uint32) != b.view(np.uint32)).mean())


@pytest.mark.parametrize('cin,cout', [(6, 3), (32, 48), (192, 112)])
def test_conv_exact_sees_each_planted_variant(cin, cout):
    """Each variant computes the same value to rounding and must still change bits: what the 1e-4 tests cannot see."""
    nbr, n_in, n_out = _tables96()['subm']
    kw = _case(nbr, n_in, n_out, cin, cout, True)
    args = [kw[k] for k in ('x', 'nbr', 'w', 'bias', 'scale', 'shift', 'residual')]
    exact = ref.conv_exact(**kw)
    want, bound = ref.conv(**kw), _bound(**kw)
    for what, plant in (('ascending channel order', dict(channels='ascending')), ('contracted prologue', dict(contract=True)),
                        ('acc + (bias + residual)', dict(right_epilogue=True)), ('k descending', dict(k_descending=True))):
        planted = ref._chain(*args, **plant)
        share = _share(exact, planted)
        print(f'{cin}->{cout} {what}: {100 * share:.1f} % of {exact.size} elements change bits')
        assert share > 0, what
        assert (np.abs(planted.astype(np.float64) - want) <= bound).all(), what              # and yet the same value: not a planted blunder
    assert _share(exact, ref._chain(*args)) == 0


def test_skipped_rows_and_rows_gathered_as_zeros_have_the_same_bits():
    """The kernel gathers an absent neighbour as a zero row whenever another row of its tile has one; the model skips it.  Here the
    model gathers too: every absent entry points at an added all-zero row (after the prologue: the kernel zeroes the row, not the
    input).  cin = 6 also runs with its channels padded to 8 by zeros against a finite weight."""
    nbr, n_in, n_out = _tables96()['subm']
    for cin, cout in ((6, 3), (32, 48)):
        kw = _case(nbr, n_in, n_out, cin, cout, False)
        kw['bias'] = ref.weights(1, cin, cout)[1]
        exact = ref.conv_exact(**kw)
        x0 = np.concatenate([kw['x'], np.zeros((1, cin), np.float32)])
        gathered = ref.conv_exact(x0, np.where(nbr >= 0, nbr, n_in).astype(np.int32), kw['w'], kw['bias'])
        assert _share(exact, gathered) == 0
        if cin == 6:
            x8 = np.concatenate([kw['x'], np.zeros((n_in, 2), np.float32)], 1)
            w8 = np.concatenate([kw['w'], np.repeat(kw['w'][:, 5:6], 2, 1)], 1)          # the clamped weight row cin - 1
            padded = ref._chain(x8, nbr, w8, kw['bias'], None, None, None)
            assert _share(exact, padded) == 0


def test_conv_exact_prologue_returns_zero_for_nan_and_nan_stays_in_its_rows():
    nbr, n_in, n_out = _tables96()['subm']
    kw = _case(nbr, n_in, n_out, 32, 48, True)
    clean = ref.conv_exact(**kw)
    kw['x'] = kw['x'].copy()
    pos = kw['scale'] > 0
    c = int(np.nonzero(pos)[0][0])
    kw['x'][5, c] = np.nan
    with_nan = ref.conv_exact(**kw)
    assert not np.isnan(with_nan).any()
    kw['x'][5, c] = -np.float32(1e6)                       # a value the ReLU cuts
    assert _share(with_nan, ref.conv_exact(**kw)) == 0 and _share(with_nan, clean) > 0
    kw['x'][5, c] = np.nan
    plain = ref.conv_exact(kw['x'], nbr, kw['w'], kw['bias'])
    reads = (nbr == 5).any(1)
    assert 0 < reads.sum() < n_out and np.isnan(plain[reads]).all() and not np.isnan(plain[~reads]).any()


# ------------------------------------------------------------------------------------------------------ edge scenes
def test_the_large_scene_straddles_the_key_boundaries():
    idx, shape, batch = ref.edge_scene('large')
    assert idx.dtype == np.int32 and 200 <= len(idx) <= 500 and len({tuple(r) for r in idx.tolist()}) == len(idx)
    assert shape == (1201, 1301, 1401) and batch == 9 and sorted(set(idx[:, 0].tolist())) == [0, 1, 8]
    assert (idx[:, 1:] >= 0).all() and (idx[:, 1:] < np.array(shape)).all()
    keys = ref.linear_key(idx, shape)
    nbr = ref.subm_rules(idx, shape)
    row = {tuple(r): i for i, r in enumerate(idx.tolist())}
    for bound, item in ((2 ** 31, 0), (2 ** 32, 1)):
        below, above = np.nonzero(keys == bound - 1)[0], np.nonzero(keys == bound)[0]
        assert len(below) == 1 and len(above) == 1                                  # sites on both sides of the boundary
        i, j = int(below[0]), int(above[0])
        assert idx[i, 0] == idx[j, 0] == item and (idx[i, 1:3] == idx[j, 1:3]).all() and idx[j, 3] == idx[i, 3] + 1
        assert nbr[i, 14] == j and nbr[j, 12] == i                                   # neighbours along d2, across the boundary
        assert (nbr[i] >= 0).all()                                                   # the centre of a full block
        assert (keys[idx[:, 0] == item] < bound).sum() > 27 and (keys[idx[:, 0] == item] >= bound).sum() > 9
    assert ref.site_of_key(2 ** 31 - 1, shape) == idx[keys == 2 ** 31 - 1][0].tolist()
    corner, origin = row[(8, 1200, 1300, 1400)], row[(0, 0, 0, 0)]
    assert (nbr[corner] >= 0).sum() == 8 and (nbr[origin] >= 0).sum() == 8           # blocks clipped to 2x2x2 by the grid
    assert keys.max() == 9 * 1201 * 1301 * 1401 - 1 and keys.min() == 0
    out_idx, down, out_shape, dropped = ref.down_rules(idx, shape)
    assert out_shape == (600, 650, 700) and dropped[corner] and 0 < dropped.sum() < len(idx) // 4
    okeys = ref.linear_key(out_idx, out_shape)
    assert (np.diff(okeys) > 0).all() and okeys.max() == 9 * 600 * 650 * 700 - 1    # the parent of the far block: the last coarse cell
    assert (okeys[out_idx[:, 0] == 8] > 2 ** 31).all() and (out_idx[:, 0] == 8).sum() > 20 and (okeys < 2 ** 31).sum() > 20
    inv = ref.inverse_rules(idx, out_idx, shape)
    assert np.array_equal((inv >= 0).sum(1), (~dropped).astype(int))
    assert not np.array_equal(idx, idx[np.argsort(keys)])


def test_the_small_edge_scenes_hold_what_they_claim():
    idx, shape, batch = ref.edge_scene('unit')
    assert shape == (1, 1, 1) and idx.tolist() != sorted(idx.tolist()) and sorted(idx.tolist()) == [[b, 0, 0, 0] for b in range(3)]
    nbr = ref.subm_rules(idx, shape)
    assert np.array_equal(nbr[:, 13], np.arange(3)) and (nbr >= 0).sum() == 3       # items never touch
    idx, shape, batch = ref.edge_scene('two')
    out_idx, down, out_shape, dropped = ref.down_rules(idx, shape)
    assert len(idx) == 16 and out_shape == (1, 1, 1) and out_idx.tolist() == [[0, 0, 0, 0], [1, 0, 0, 0]] and (down >= 0).all() and not dropped.any()
    assert ((ref.subm_rules(idx, shape) >= 0).sum(1) == 8).all()
    idx, shape, batch = ref.edge_scene('three_two_five')
    out_idx, down, out_shape, dropped = ref.down_rules(idx, shape)
    assert out_shape == (1, 1, 2) and (idx[:, 0] == 0).sum() == 30 and 5 <= (idx[:, 0] == 1).sum() <= 25
    assert np.array_equal(dropped, (idx[:, 1] == 2) | (idx[:, 3] == 4)) and 0 < dropped.sum() < len(idx) and (down < 0).any()
    assert len(out_idx) == 4
    idx, shape, batch = ref.edge_scene('dense')
    assert len(idx) == 240 and shape == (4, 5, 6) and batch == 2
    full = (ref.subm_rules(idx, shape) >= 0).all(1)
    interior = ((idx[:, 1:] >= 1) & (idx[:, 1:] <= np.array(shape) - 2)).all(1)
    assert full.sum() == 2 * (2 * 3 * 4) and np.array_equal(full, interior)          # 27 of 27 neighbours at the interior sites only
    idx, shape, batch = ref.edge_scene('all_dropped')
    out_idx, down, out_shape, dropped = ref.down_rules(idx, shape)
    assert len(idx) == 2 * 19 and dropped.all() and out_idx.shape == (0, 4) and down.shape == (0, 8) and out_shape == (1, 1, 1)
    assert (ref.inverse_rules(idx, out_idx, shape) == -1).all()
    for name, batch, least in (('mostly_dropped', 1, 8), ('mostly_dropped_x20', 20, 256)):
        idx, shape, b = ref.edge_scene(name)
        out_idx, down, out_shape, dropped = ref.down_rules(idx, shape)
        assert b == batch and len(idx) == 27 * batch and len(out_idx) == batch and len(out_idx) * 8 < len(idx) and dropped.sum() == 19 * batch
        assert -(-len(out_idx) * 8 // 256) < -(-len(idx) // 256) or batch == 1      # x20: the sites need more workgroups than the table
        dup, pos = ref.with_dropped_duplicate(name)
        keys = np.sort(ref.linear_key(dup, shape))
        assert pos >= least and pos >= len(out_idx) * 8 and keys[pos] == keys[pos + 1] and (np.diff(keys) == 0).sum() == 1
        twice = dup[ref.linear_key(dup, shape) == keys[pos]]
        assert len(twice) == 2 and (twice[:, 1:] == 2).any(1).all()                 # both rows of the pair are dropped sites
        assert len(ref.down_rules(idx, shape)[0]) == len({tuple(r) for r in (dup[:, :1].tolist())})          # the outputs stay: one per item
