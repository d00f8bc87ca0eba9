"""GPU tests of the NUNOCS symmetry-min cross-entropy loss (catgrasp_amd/loss.py, csrc/nocs_loss.hip) against tests/nocs_loss_ref.py.

Per element, L, loss, lse and the gradient are within 1e-4 * max(1, |ref|) of float64 (the project's bar); the gradient is compared
with the float64 gradient at the kernel's ids.  ids, the bins (through the gradient's one-hot positions, which are its negative
entries) and L equal the float32 restatement of the header's chains bit for bit; the restatement takes the kernel's lse, because expf
and logf are the device library's.

The shapes are the smallest at which the decomposition can go wrong: N in {1, SEG - 1, SEG, SEG + 1, 2 SEG + 2} (one point, a short
segment, a full one, a second segment of one point, three segments), B in {1, 3}, bins in {4, 100, 128} (fewer bins than waves, the
configuration's, the cap with a second bin per lane), S in {1, 2, 12, 72} (identity, hnm, nut, screw; screw needs a second symmetry per
lane), both storages, the full product.  With one point the two storages are the same bytes; the channel-major id then names the
storage in the call, so that the channel-major kernels run with one live lane too.  Every case must take the strict arg-min branch in
at least one row, except screw at bins = 4, N = 1: there the 72 rotations move the one point through at most 16 bin pairs, the
float64 columns of L tie by construction (0 of 20 seeds at B = 1 give a strict row), and only the non-strict rule is asserted."""
import functools

import numpy as np
import pytest
import torch

import nocs_loss_ref as nref
from catgrasp_amd import _lib, loss as nl
from catgrasp_amd import pointnet2 as p2

pytestmark = pytest.mark.gpu

BAR = 1e-4
SEG = nref.SEG
NS = (1, SEG - 1, SEG, SEG + 1, 2 * SEG + 2)
CASES = [(name, B, N, bins) for N in NS for B in (1, 3) for bins in (4, 100, 128) for name in ('identity', 'hnm', 'nut', 'screw')]


def strict_rows_needed(name, N, bins):
    return 0 if (name, N, bins) == ('screw', 1, 4) else 1


def storage(channel_major):
    return nl.CHANNEL_MAJOR if channel_major else nl.POINT_MAJOR


def within_bar(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return bool((np.abs(got - ref) <= BAR * np.maximum(1.0, np.abs(ref))).all())


@functools.lru_cache(maxsize=None)
def case(name, B, N, bins):
    """Inputs and float64 results of one case, computed once and shared by both storages; never modified."""
    tfs = nref.symmetry_tfs(name)
    for attempt in range(20):
        # The arg-min rule needs a row whose float64 gap between the best and the second symmetry exceeds its slack.  That is a property
        # of the inputs in float64 alone, so the seed is advanced until it holds (a few cases with B = 1 need a second or third seed).
        pred, target, _ = nref.make_inputs(1000 * N + 10 * bins + B + 100000 * attempt, B, N, bins, tfs)
        loss64, L64, ids64 = nref.loss_f64(pred, target, tfs, bins)
        srt = np.sort(L64, 1)
        if len(tfs) == 1 or ((srt[:, 1] - srt[:, 0]) > 2 * BAR * np.maximum(1.0, np.abs(srt[:, 0]))).any():
            break
    out = dict(tfs=tfs, pred=pred, target=target, loss64=loss64, L64=L64, ids64=ids64, lse64=nref.lse_f64(pred), k32=nref.bins_f32(target, tfs, bins))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def on_device(pred, channel_major, dev, requires_grad=False):
    """Logical float32 logits (B, N, 3, bins) -> the (B, N, 3*bins) device tensor in one of the two storages."""
    B, N = pred.shape[:2]
    flat = torch.from_numpy(np.array(pred.reshape(B, N, -1))).to(dev)
    x = flat.permute(0, 2, 1).contiguous().permute(0, 2, 1) if channel_major else flat
    # with one point the two storages are the same bytes and the strides fit both: point-major unless the call names the other
    assert nl.layout_of(x) == (nl.CHANNEL_MAJOR if channel_major and N > 1 else nl.POINT_MAJOR)
    assert nl.layout_of(x, storage(channel_major)) == storage(channel_major)
    return x.requires_grad_(requires_grad)


def dev_of(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)                          # a copy: the shared arrays are read-only


def logical(t, bins):
    B, N = t.shape[:2]
    return t.detach().cpu().numpy().reshape(B, N, 3, bins)


def check_argmin(ids, L64):
    """The arg-min rule: the chosen symmetry's float64 loss is within 2 bars of the smallest, and where the runner-up is further away than
    that, the choice is float64's.  -> the number of rows that took this strict branch."""
    strict = 0
    for b, row in enumerate(L64):
        lo = row.min()
        slack = 2 * BAR * max(1.0, abs(lo))
        assert row[ids[b]] <= lo + slack, (b, ids[b], row[ids[b]], lo)
        gap = np.partition(row, 1)[1] - lo if len(row) > 1 else np.inf
        if gap > slack:
            assert ids[b] == row.argmin(), (b, ids[b], row.argmin(), gap)
            strict += 1
    return strict


@pytest.mark.parametrize('channel_major', [True, False], ids=['channel_major', 'point_major'])
@pytest.mark.parametrize('name,B,N,bins', CASES)
def test_loss_table_ids_and_gradient(cuda_device, name, B, N, bins, channel_major):
    c = case(name, B, N, bins)
    tfs, target = dev_of(c['tfs'], cuda_device), dev_of(c['target'], cuda_device)
    x = on_device(c['pred'], channel_major, cuda_device, requires_grad=True)
    loss, ids_t, L_t = nl.nocs_symce_all(x, target, tfs, bins, layout=storage(channel_major) if N == 1 else None)
    assert nl.last_layout == storage(channel_major)
    loss.backward()
    assert loss.dim() == 0 and loss.requires_grad and ids_t.dtype == torch.int32 and tuple(L_t.shape) == (B, len(c['tfs']))
    assert nl.last_pred_ptr == x.data_ptr() and x.grad.stride() == x.stride()          # used where it lies; the gradient in its storage
    # the same call through the plain wrapper, which also hands out lse
    loss_b, ids_b, L_b, lse_t = nl._forward(x.detach(), target, tfs, bins, True, storage(channel_major))
    assert torch.equal(loss_b.reshape(()), loss.detach()) and torch.equal(ids_b, ids_t) and torch.equal(L_b, L_t)
    ids, L, lse, got_loss = ids_t.cpu().numpy(), L_t.cpu().numpy(), lse_t.cpu().numpy(), float(loss.detach())
    grad = logical(x.grad, bins)
    print(f'{name} B={B} N={N} bins={bins} cm={channel_major}: |L-L64| {np.abs(L - c["L64"]).max():.2e}  |loss-loss64| {abs(got_loss - c["loss64"]):.2e}  '
          f'|lse-lse64| {np.abs(lse - c["lse64"]).max():.2e}')
    # float64, per element
    assert within_bar(lse, c['lse64']) and within_bar(L, c['L64']) and within_bar(got_loss, c['loss64'])
    assert check_argmin(ids, c['L64']) >= strict_rows_needed(name, N, bins)
    g64 = nref.grad_f64(c['pred'], c['target'], c['tfs'], bins, ids)
    assert within_bar(grad, g64), np.abs(grad - g64).max()
    # bits: the float32 restatement of the bin chain and of the tree, from the kernel's lse
    loss32, L32, ids32 = nref.tree_f32(c['pred'], lse, c['k32'])
    assert np.array_equal(ids, ids32)
    assert np.array_equal(L.view(np.uint32), L32.view(np.uint32))
    assert np.float32(got_loss).view(np.uint32) == loss32.view(np.uint32)
    onehot = np.arange(bins)[None, None, None, :] == c['k32'][np.arange(B), :, ids][..., None]
    assert np.array_equal(grad < 0, onehot)


@pytest.mark.parametrize('channel_major', [True, False], ids=['channel_major', 'point_major'])
@pytest.mark.parametrize('name,bins', [('screw', 100), ('nut', 128), ('hnm', 4)])
def test_bins_on_and_next_to_the_boundaries_equal_the_float32_chain(cuda_device, name, bins, channel_major):
    """Targets ON bin boundaries, a few ulps and up to 1e-3 / bins off them, and on 0, 0.5 and 1 exactly: float64 is not consulted, the
    kernel must take the bins of the float32 chain.  A wrong bin moves the one-hot and changes L."""
    rng = np.random.default_rng(bins)
    tfs = nref.symmetry_tfs(name)
    grid = rng.integers(0, bins + 1, (2, 40, 3)).astype(np.float32) / np.float32(bins)
    off = rng.choice(np.float32([0, 0, 1e-7, -1e-7, 3e-6, -3e-6, 9e-6, -9e-6]), (2, 40, 3))
    corners = np.stack(np.meshgrid(*[np.float32([0, 0.5, 1])] * 3, indexing='ij'), -1).reshape(1, 27, 3).repeat(2, 0)
    target = np.concatenate([np.clip(grid + off, 0, 1).astype(np.float32), corners], 1)                      # (2, 67, 3): two segments
    B, N = target.shape[:2]
    pred = (rng.standard_normal((B, N, 3, bins)) * 3).astype(np.float32)
    k64, q = nref.bins_f64(target, tfs, bins)
    assert (np.abs(q - np.rint(q)) < 1e-3).mean() > 0.3                   # most of these are inside the band the other tests stay out of
    k32 = nref.bins_f32(target, tfs, bins)
    x = on_device(pred, channel_major, cuda_device, requires_grad=True)
    t, T = torch.from_numpy(target).to(cuda_device), torch.from_numpy(tfs).to(cuda_device)
    loss, ids, L = nl.nocs_symce_all(x, t, T, bins)
    loss.backward()
    lse = nl._forward(x.detach(), t, T, bins, True)[3].cpu().numpy()
    loss32, L32, ids32 = nref.tree_f32(pred, lse, k32)
    ids = ids.cpu().numpy()
    assert np.array_equal(ids, ids32) and np.array_equal(L.cpu().numpy().view(np.uint32), L32.view(np.uint32))
    assert np.float32(float(loss.detach())).view(np.uint32) == loss32.view(np.uint32)
    onehot = np.arange(bins)[None, None, None, :] == k32[np.arange(B), :, ids][..., None]
    assert np.array_equal(logical(x.grad, bins) < 0, onehot)
    # every symmetry's bins, one symmetry at a time: with S = 1 the one-hot shows the bins of that symmetry
    for s in range(0, len(tfs), max(1, len(tfs) // 6)):
        xs = on_device(pred, channel_major, cuda_device, requires_grad=True)
        nl.nocs_symce(xs, t, T[s:s + 1], bins).backward()
        assert np.array_equal(logical(xs.grad, bins) < 0, np.arange(bins)[None, None, None, :] == k32[:, :, s][..., None]), s


@pytest.mark.parametrize('channel_major', [True, False], ids=['channel_major', 'point_major'])
def test_tie_goes_to_the_smaller_index(cuda_device, channel_major):
    c = case('identity', 3, SEG + 1, 100)
    tfs = torch.from_numpy(nref.symmetry_tfs('identity2')).to(cuda_device)
    x = on_device(c['pred'], channel_major, cuda_device)
    loss, ids, L = nl.nocs_symce_all(x, dev_of(c['target'], cuda_device), tfs, 100)
    assert torch.equal(L[:, 0], L[:, 1]) and ids.tolist() == [0, 0, 0]
    assert within_bar(L[:, 0].cpu().numpy(), c['L64'][:, 0]) and within_bar(float(loss.detach()), c['loss64'])
    # and among three: the nut's transforms with the winning one repeated at the end
    n = case('nut', 3, SEG + 1, 100)
    tfs3 = np.concatenate([n['tfs'], n['tfs'][n['ids64'][0]][None]])
    xn = on_device(n['pred'], channel_major, cuda_device)
    _, ids3, L3 = nl.nocs_symce_all(xn, dev_of(n['target'], cuda_device), torch.from_numpy(tfs3).to(cuda_device), 100)
    assert int(ids3[0]) == n['ids64'][0] and torch.equal(L3[0, -1], L3[0, n['ids64'][0]])


@pytest.mark.parametrize('channel_major', [True, False], ids=['channel_major', 'point_major'])
def test_saturated_logits_stay_finite(cuda_device, channel_major):
    """Logits of -80 with one +80 per row: exp(160) overflows float32, so only a max-shifted log-sum-exp survives."""
    B, N, bins = 2, SEG + 3, 100
    tfs = nref.symmetry_tfs('nut')
    _, target, _ = nref.make_inputs(4, B, N, bins, tfs)
    rng = np.random.default_rng(4)
    pred = np.full((B, N, 3, bins), -80, np.float32)
    hot = rng.integers(0, bins, (B, N, 3))
    k, _ = nref.bins_f64(target, tfs, bins)
    hot[:, ::2] = k[:, ::2, 3]                                            # half of the rows: right, under symmetry 3
    np.put_along_axis(pred, hot[..., None], 80, -1)
    loss64, L64, ids64 = nref.loss_f64(pred, target, tfs, bins)
    x = on_device(pred, channel_major, cuda_device, requires_grad=True)
    loss, ids, L = nl.nocs_symce_all(x, torch.from_numpy(target).to(cuda_device), torch.from_numpy(tfs).to(cuda_device), bins)
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(L).all() and torch.isfinite(x.grad).all()
    assert within_bar(float(loss.detach()), loss64) and within_bar(L.cpu().numpy(), L64) and check_argmin(ids.cpu().numpy(), L64) >= 1
    assert within_bar(logical(x.grad, bins), nref.grad_f64(pred, target, tfs, bins, ids.cpu().numpy()))


@pytest.mark.parametrize('channel_major', [True, False], ids=['channel_major', 'point_major'])
def test_upstream_gradient_no_grad_path_module_and_streams(cuda_device, channel_major):
    c = case('screw', 3, 2 * SEG + 2, 100)
    bins = 100
    target, tfs = dev_of(c['target'], cuda_device), dev_of(c['tfs'], cuda_device)
    x = on_device(c['pred'], channel_major, cuda_device, requires_grad=True)
    loss = nl.nocs_symce(x, target, tfs, bins)
    loss.backward()
    g1 = x.grad.clone()
    # upstream gradient: read from the device, not assumed to be 1
    x.grad = None
    (3 * nl.nocs_symce(x, target, tfs, bins)).backward()
    assert torch.allclose(x.grad, 3 * g1, rtol=1e-6, atol=0)
    x.grad = None
    (0.5 * nl.nocs_symce(x, target, tfs, bins)).backward()
    assert torch.equal(x.grad, 0.5 * g1)                                  # a power of two scales every element exactly
    # no_grad, and a pred that asks for no gradient: forward only, nothing kept for a backward
    for ctx, inp in ((torch.no_grad(), x), (torch.enable_grad(), x.detach())):
        with ctx:
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            out = nl.nocs_symce(inp, target, tfs, bins)
            kept = torch.cuda.memory_allocated() - before
        assert not out.requires_grad and out.grad_fn is None and torch.equal(out, loss.detach())
        assert kept < c['lse64'].size * 4                                 # lse (B, N, 3) was not allocated, let alone kept
    # module against function
    crit = nl.NocsMinSymmetryCELoss({'nocs_class_name': 'screw', 'ce_loss_bins': bins})
    x.grad = None
    ml = crit(x, target)
    ml.backward()
    assert torch.equal(ml.detach(), loss.detach()) and torch.equal(x.grad, g1) and ml.dim() == 0
    _, ids, L = nl.nocs_symce_all(x.detach(), target, tfs, bins)
    assert torch.equal(crit.last_ids, ids) and torch.equal(crit.last_per_symmetry, L) and tuple(crit.last_ids.shape) == (3,)
    assert tuple(crit.last_per_symmetry.shape) == (3, 72)
    # two streams, same bits
    outs = []
    for _ in range(2):
        s = torch.cuda.Stream(device=cuda_device)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            xs = on_device(c['pred'], channel_major, cuda_device, requires_grad=True)
            ls, ids_s, L_s = nl.nocs_symce_all(xs, target, tfs, bins)
            ls.backward()
        s.synchronize()
        outs.append((ls.detach(), ids_s, L_s, xs.grad))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    assert torch.equal(outs[0][0], loss.detach()) and torch.equal(outs[0][3], g1)


def test_training_step_of_the_nunocs_network_moves_the_last_layer(cuda_device):
    """PointNetSeg in training mode -> channel-major logits, used in place -> loss -> backward -> Adam."""
    torch.manual_seed(0)
    B, N, bins = 2, 128, 100
    net = p2.PointNetSeg(6, 3 * bins).to(cuda_device).train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    crit = nl.NocsMinSymmetryCELoss({'nocs_class_name': 'nut', 'ce_loss_bins': bins})
    x = torch.rand(B, N, 6, device=cuda_device)
    target = torch.rand(B, N, 3, device=cuda_device)
    pred, _ = net(x)
    assert nl.layout_of(pred) == nl.CHANNEL_MAJOR and pred.requires_grad
    loss = crit(pred, target)
    assert nl.last_pred_ptr == pred.data_ptr() and nl.last_layout == nl.CHANNEL_MAJOR            # the kernel read conv4's output itself
    ref64, _, ids64 = nref.loss_f64(pred.detach().cpu().numpy().reshape(B, N, 3, bins), target.cpu().numpy(), nref.symmetry_tfs('nut'), bins)
    assert within_bar(float(loss.detach()), ref64)
    before = net.conv4.weight.detach().clone()
    opt.zero_grad()
    loss.backward()
    assert net.conv4.weight.grad is not None and torch.isfinite(net.conv4.weight.grad).all() and net.conv4.weight.grad.abs().max() > 0
    assert net.feat.conv1.weight.grad.abs().max() > 0                     # the gradient reaches the first layer
    opt.step()
    assert not torch.equal(net.conv4.weight.detach(), before)
    with torch.no_grad():
        after = crit(net(x)[0], target)
    assert torch.isfinite(after) and not after.requires_grad


def test_limits_raise(cuda_device):
    B, N = 2, 5
    target = torch.rand(B, N, 3, device=cuda_device)
    eye = torch.eye(4, device=cuda_device)[None]
    with pytest.raises(_lib.CatgraspAmdError, match='status -2'):
        nl.nocs_symce(torch.zeros(B, N, 3 * 129, device=cuda_device), target, eye, 129)
    with pytest.raises(_lib.CatgraspAmdError, match='status -2'):
        nl.nocs_symce(torch.zeros(B, N, 12, device=cuda_device), target, eye.repeat(129, 1, 1), 4)
    assert torch.isfinite(nl.nocs_symce(torch.zeros(B, N, 3 * 128, device=cuda_device), target, eye.repeat(128, 1, 1), 128))   # the caps themselves
    with pytest.raises(ValueError, match='neither'):
        nl.nocs_symce(torch.zeros(N, B, 12, device=cuda_device).permute(1, 0, 2), target, eye, 4)       # neither storage: would need a copy
    with pytest.raises(ValueError, match='neither'):
        nl.nocs_symce(torch.zeros(12, N, B, device=cuda_device).permute(2, 1, 0), target, eye, 4)
    with pytest.raises(ValueError):
        nl.nocs_symce(torch.zeros(B, N, 12, device=cuda_device), target, eye, 5)                        # 3 * bins is not the width
    with pytest.raises(_lib.CatgraspAmdError):
        nl.nocs_symce(torch.zeros(B, N, 12, device=cuda_device).double(), target, eye, 4)


@pytest.mark.parametrize('channel_major', [True, False], ids=['channel_major', 'point_major'])
def test_offsets_past_two_to_the_31(cuda_device, channel_major):
    """B N 3 bins = 2 * 2,800,000 * 384 is just past 2^31 elements: sample 1 straddles that offset.  Its row of L, its id and its
    gradient must be the bits of a call on that sample alone (a view, no copy): the trees are per sample, and 0.5 / N is 1 / (2 N)
    exactly.  Both storages, because each has kernels and index expressions of its own."""
    B, N, bins = 2, 2800000, 128
    assert B * N * 3 * bins > 2 ** 31 and N * 3 * bins < 2 ** 31
    g = torch.Generator(device=cuda_device).manual_seed(1)
    store = torch.randn((B, 3 * bins, N) if channel_major else (B, N, 3 * bins), device=cuda_device, generator=g)
    x = (store.permute(0, 2, 1) if channel_major else store).requires_grad_(True)
    target = torch.rand(B, N, 3, device=cuda_device, generator=g)
    tfs = torch.from_numpy(nref.symmetry_tfs('hnm')).to(cuda_device)
    loss, ids, L = nl.nocs_symce_all(x, target, tfs, bins)
    loss.backward()
    x1 = x.detach()[1:2].requires_grad_(True)
    assert x1.data_ptr() == x.data_ptr() + 4 * N * 3 * bins
    loss1, ids1, L1 = nl.nocs_symce_all(x1, target[1:2], tfs, bins)
    (0.5 * loss1).backward()
    assert torch.equal(L[1:2], L1) and torch.equal(ids[1:2], ids1) and torch.isfinite(loss)
    assert torch.equal(x.grad[1:2], x1.grad)
    assert float(x.grad[0].abs().max()) > 0 and float(L.min()) > 0


@pytest.mark.parametrize('channel_major', [True, False], ids=['channel_major', 'point_major'])
@pytest.mark.parametrize('bins', [7, 10])
def test_widths_that_are_no_multiple_of_four(cuda_device, bins, channel_major):
    """3 * bins = 21 and 30: the point-major backward cannot sweep its rows as float4 and takes one float per lane.  Same checks as
    the main test, at B = 2 and a second segment of one point."""
    c = case('nut', 2, SEG + 1, bins)
    tfs, target = dev_of(c['tfs'], cuda_device), dev_of(c['target'], cuda_device)
    x = on_device(c['pred'], channel_major, cuda_device, requires_grad=True)
    loss, ids_t, L_t = nl.nocs_symce_all(x, target, tfs, bins)
    loss.backward()
    lse = nl._forward(x.detach(), target, tfs, bins, True)[3].cpu().numpy()
    ids, L, grad = ids_t.cpu().numpy(), L_t.cpu().numpy(), logical(x.grad, bins)
    assert within_bar(lse, c['lse64']) and within_bar(L, c['L64']) and within_bar(float(loss.detach()), c['loss64'])
    assert check_argmin(ids, c['L64']) >= 1
    assert within_bar(grad, nref.grad_f64(c['pred'], c['target'], c['tfs'], bins, ids))
    loss32, L32, ids32 = nref.tree_f32(c['pred'], lse, c['k32'])
    assert np.array_equal(ids, ids32) and np.array_equal(L.view(np.uint32), L32.view(np.uint32))
    assert np.array_equal(grad < 0, np.arange(bins)[None, None, None, :] == c['k32'][np.arange(2), :, ids][..., None])
