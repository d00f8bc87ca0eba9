"""CPU tests (no GPU) of the yardstick of the NUNOCS loss, tests/nocs_loss_ref.py: its float64 restatement equals a direct torch
composition of the formula (expand, cross_entropy, sum, mean, argmin, gather) for the loss and for autograd's gradient, and equals what
the reference's own module returned (tests/golden/nocs_loss_golden.npz, made by tests/golden/make_golden_nocs_loss.py); its float32
restatement of the header's chains is exact where exactness can be checked on the CPU; its input builder keeps every bin away from a
boundary and reaches both clamps."""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nocs_loss_ref as nref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'nocs_loss_golden.npz')


def torch_composition(pred, target, tfs, bins):
    """The formula as the reference executes it, in the dtype of `pred` (B, N, 3*bins): -> (loss, L (B, S), ids)."""
    B, N = target.shape[:2]
    S = len(tfs)
    homo = torch.cat([target - 0.5, torch.ones_like(target[..., :1])], -1)                       # (B, N, 4)
    moved = torch.matmul(tfs[None].expand(B, S, 4, 4), homo.permute(0, 2, 1)[:, None].expand(B, S, 4, N))
    moved = moved.permute(0, 1, 3, 2)[..., :3] + 0.5                                            # (B, S, N, 3)
    cls = torch.clamp(moved * bins, 0, bins - 1).long()
    x = pred.reshape(B, N, 3, bins)[..., None].expand(-1, -1, -1, -1, S)                        # (B, N, 3, bins, S)
    per_axis = [F.cross_entropy(x[:, :, a].permute(0, 2, 3, 1), cls[..., a], reduction='none') for a in range(3)]   # (B, S, N) each
    L = torch.stack(per_axis, -1).sum(-1).mean(-1)                                              # (B, S)
    ids = L.argmin(1)
    return torch.gather(L, 1, ids[:, None]).mean(), L, ids


@pytest.mark.parametrize('name,B,N,bins', [('identity', 1, 5, 4), ('hnm', 2, 9, 7), ('nut', 3, 17, 10), ('screw', 2, 33, 100)])
def test_float64_restatement_equals_the_torch_composition(name, B, N, bins):
    tfs = nref.symmetry_tfs(name)
    pred, target, _ = nref.make_inputs(11, B, N, bins, tfs)
    loss, L, ids = nref.loss_f64(pred, target, tfs, bins)
    x = torch.from_numpy(pred.reshape(B, N, 3 * bins)).double().requires_grad_(True)
    tl, tL, tids = torch_composition(x, torch.from_numpy(target).double(), torch.from_numpy(tfs).double(), bins)
    (2.5 * tl).backward()
    assert np.array_equal(ids, tids.numpy())
    np.testing.assert_allclose(L, tL.detach().numpy(), rtol=1e-13, atol=0)
    np.testing.assert_allclose(loss, float(tl.detach()), rtol=1e-13, atol=0)
    g = nref.grad_f64(pred, target, tfs, bins, ids, g=2.5)
    np.testing.assert_allclose(g, x.grad.numpy().reshape(g.shape), rtol=1e-11, atol=1e-17)
    assert g.shape == (B, N, 3, bins) and abs(g.sum()) < 1e-12            # softmax minus one-hot sums to zero on every row


@pytest.mark.parametrize('name', ['nut', 'screw'])
def test_float64_restatement_equals_the_reference_module(name):
    z = np.load(GOLDEN)
    B, N, bins, step = (int(v) for v in z['shape'])
    tfs = nref.symmetry_tfs(name)
    pred, target, _ = nref.make_inputs(int(z[f'{name}_seed']), B, N, bins, tfs)
    np.testing.assert_allclose([pred.astype(np.float64).sum(), target.astype(np.float64).sum()], z[f'{name}_digest'], rtol=1e-12)
    loss, L, ids = nref.loss_f64(pred, target, tfs, bins)
    # the module ran in float32 on the CPU: the project's bar
    assert abs(float(z[f'{name}_loss']) - loss) <= 1e-4 * max(1.0, abs(loss))
    # the gap between the best and the second symmetry is far above float32's error, so the module took the same one ...
    srt = np.sort(L, 1)
    assert ((srt[:, 1] - srt[:, 0]) > 1e-3).all()
    k, _ = nref.bins_f64(target, tfs, bins)
    assert np.array_equal(z[f'{name}_onehot'], k[np.arange(B), :, ids])      # ... and put the one-hot where the restatement's bins are
    g = nref.grad_f64(pred, target, tfs, bins, ids)
    np.testing.assert_allclose(z[f'{name}_grad'], g[:, ::step], rtol=1e-4, atol=1e-8)


def test_fmaf32_rounds_once():
    rng = np.random.default_rng(0)
    a, b = (rng.standard_normal(4000).astype(np.float32) for _ in range(2))
    c = (-(a.astype(np.float64) * b) * (1 + rng.standard_normal(4000) * 1e-7)).astype(np.float32)     # heavy cancellation
    a, b, c = (np.concatenate([v, w]) for v, w in zip((a, b, c), (rng.standard_normal((3, 4000)).astype(np.float32))))
    # a double rounding: (1 + 2^-12) * (1 - 2^-12 + 2^-24) 2^-24 + 1 = 1 + 2^-24 + 2^-60 lies above the tie and rounds up to 1 + 2^-23;
    # float64 drops the 2^-60 first, and the tie it leaves would go down to 1
    a = np.concatenate([a, np.float32([1 + 2.0 ** -12])]); b = np.concatenate([b, np.float32([(1 - 2.0 ** -12 + 2.0 ** -24) * 2.0 ** -24])])
    c = np.concatenate([c, np.float32([1.0])])
    got = nref.fmaf32(a, b, c)

    def exact(x, y, z):
        v = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo = np.float32(float(v))                                    # rounded twice: the answer is this or a neighbour
        cands = sorted({lo, np.nextafter(lo, np.float32(-np.inf)), np.nextafter(lo, np.float32(np.inf))}, key=float)
        best = min(cands, key=lambda f: (abs(Fraction(float(f)) - v), int(np.float32(f).view(np.uint32)) & 1))
        return np.float32(best)
    want = np.array([exact(*t) for t in zip(a, b, c)], np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got[-1] == np.nextafter(np.float32(1.0), np.float32(2.0))
    assert (a[-1].astype(np.float64) * b[-1] + 1.0).astype(np.float32) == np.float32(1.0)      # what float64 alone makes of it
    tie = nref.fmaf32(np.float32([2.0 ** -12]), np.float32([2.0 ** -12]), np.float32([1.0]))
    assert tie[0] == np.float32(1.0)                                 # an exact tie goes to even


@pytest.mark.parametrize('name,N,bins', [('screw', 130, 100), ('nut', 63, 128), ('hnm', 65, 4)])
def test_builder_keeps_bins_off_the_boundaries_and_reaches_both_clamps(name, N, bins):
    tfs = nref.symmetry_tfs(name)
    pred, target, redraws = nref.make_inputs(3, 3, N, bins, tfs)
    k64, q = nref.bins_f64(target, tfs, bins)
    assert (np.abs(q - np.rint(q)) >= 1e-3).all() and redraws < 100
    assert np.array_equal(nref.bins_f32(target, tfs, bins), k64)
    assert k64.min() == 0 and k64.max() == bins - 1
    if name != 'hnm':                                                # rotations about z by other than 180 degrees leave the unit cube
        assert (q < 0).any() and (q > bins).any()
    assert target.dtype == np.float32 and pred.dtype == np.float32 and target.min() >= 0 and target.max() <= 1


def test_float32_tree_is_the_header_tree_and_close_to_float64():
    tfs = nref.symmetry_tfs('nut')
    B, N, bins = 2, 2 * nref.SEG + 2, 10
    pred, target, _ = nref.make_inputs(9, B, N, bins, tfs)
    k = nref.bins_f32(target, tfs, bins)
    lse = nref.lse_f64(pred).astype(np.float32)
    loss, L, ids = nref.tree_f32(pred, lse, k)
    loss64, L64, ids64 = nref.loss_f64(pred, target, tfs, bins)
    assert L.dtype == np.float32 and np.array_equal(ids, ids64)
    np.testing.assert_allclose(L, L64, rtol=1e-5)
    np.testing.assert_allclose(loss, loss64, rtol=1e-5)
    # by hand, for one (sample, symmetry): three chains of 64, 64 and 2 points, then the segments in ascending order
    x = pred[1]
    d = lse[1][:, None, :] - np.take_along_axis(x[:, None], k[1][..., None].astype(np.int64), -1)[..., 0]
    v = ((d[..., 0] + d[..., 1]) + d[..., 2])[:, 5]
    parts = []
    for s0 in range(0, N, nref.SEG):
        p = np.float32(0)
        for t in v[s0:s0 + nref.SEG]:
            p = np.float32(p + t)
        parts.append(p)
    want = np.float32(np.float32(np.float32(parts[0] + parts[1]) + parts[2]) / np.float32(N))
    assert L[1, 5].view(np.uint32) == want.view(np.uint32)
    assert nref.SEG == 64


def test_stored_gives_both_storages_of_the_same_logits():
    pred = np.arange(2 * 5 * 3 * 4, dtype=np.float32).reshape(2, 5, 3, 4)
    pm, cm = nref.stored(pred, False), nref.stored(pred, True)
    assert pm.shape == cm.shape == (2, 5, 12) and np.array_equal(pm, cm)
    assert pm.strides == (240, 48, 4) and cm.strides == (240, 4, 20)
