"""Every instantiation of the fused set-abstraction kernels (csrc/setabstraction.hip: sa_reg_kernel, sa_group_mlp_max_kernel;
csrc/sa_tile.hip: sa_tile_kernel) against the plain float64 reference of tests/sa_ref.py, through
primitives.SetAbstractionWeights and primitives.group_mlp_max / group_all_mlp_max.

Exact cases (sa_ref.exact_scene: dyadic inputs, every partial sum a float32 number -- tests/test_sa_ref_cpu.py proves
exactness_margin < 1 for each case of EXACT_CASES) are held to value equality, torch.equal(got, ref.float()): any misrouted row,
channel, bias, centre or tile is a plain mismatch, whatever the summation order.  General-value cases are held to the per-element
bound of sa_ref.sa_bound.

Which case reaches which code:
  reg-sig-*     all 39 width signatures x the three packings (K = 5, 16, 33) of sa_reg_kernel
  reg-k-*       K = 1 .. 65 with beacon lists: every row of a pack slot / row tile carries the result alone once
  reg-d-*       D = 0 .. 13: the `8 ks + j >= c0` skip of sa_last0 / sa_hidden0 and the clamp on the feature index
  reg-out-*     a channels_last slice of a wider, sentinel-filled tensor
  reg-loop-*    the persistent loop: three rounds and a tail, one neighbourhood (idle waves stage weights), one past the CUs
  strip-*       sa_group_mlp_max_kernel: sa_layer<1..8>, weights left in L2, four layers, D = 0 / 5 / 13, beacon lists at K = 65
  tile-k-*      every packing and row-tile count of sa_tile_kernel with beacon lists
  tile-wave-*   every wave share of st_hidden / st_last (32 .. 512 hidden, 32 .. 1024 last; narrow and WIDE instance)
  tile-d-*      the gather: every (3 + D) % 8, D % 4 != 0, the GU = 8 loop at and just past 2048 pieces, a misaligned `points`
  tile-128-*    the 128-row instance and the 64-row one just below its threshold
  tile-slot-*   the XCD-ordered and the plain slot walk around every multiple of the CU count
  tile-all-*    the index-free (group-all) mode
A case whose size depends on the CU count is built for the device it runs on (and for 256 CUs by the CPU module)."""
import zlib
from itertools import product

import numpy as np
import pytest
import torch

import dense_ref as dr
import sa_ref as R

pytestmark = pytest.mark.gpu

N_CU_NOMINAL = 256          # the CPU module builds the CU-count dependent cases for this many


def _case(name, kind, widths, K, D=6, B=2, N=64, S=7, lists='random', G=None, **opt):
    """G: callable n_cu -> number of neighbourhoods (then B = 1, S = G)."""
    return dict(id=name, kind=kind, widths=list(widths), K=K, D=D, B=B, N=N, S=S, lists=lists, G=G, seed=zlib.crc32(name.encode()) & 0xffff,
                **opt)


def _s_for(K):              # B = 2: G = 2 S >= K, so that every row position is the beacon's once
    return max(7, (K + 1) // 2)


def _w(widths):
    return 'x'.join(str(c) for c in widths)


REG_SIGNATURES = [list(s) for n in (1, 2, 3) for s in product((32, 64, 128), repeat=n)]
assert len(REG_SIGNATURES) == 39

REG_SIG = [_case(f'reg-sig-{_w(s)}-K{K}', 'reg', s, K) for s in REG_SIGNATURES for K in (5, 16, 33)]
REG_K = [_case(f'reg-k-{_w(s)}-K{K}', 'reg', s, K, S=_s_for(K), lists='beacon')
         for s in ([32], [64, 128], [128, 128, 128]) for K in (1, 8, 9, 17, 32, 64, 65)]
REG_D = [_case(f'reg-d-{_w(s)}-D{D}', 'reg', s, 5, D=D) for s in ([32], [64, 64, 128]) for D in range(14)]
REG_OUT = [_case(f'reg-out-K{K}', 'reg', [32, 64], K) for K in (5, 16, 33)]
# [32]: 16 waves per workgroup (sa_reg_threads).  K = 2 packs four neighbourhoods per slot; K = 9 and K = 17 give the same loop to
# the two- and one-neighbourhood packings
_ROUNDS = lambda n_cu: 3 * 16 * n_cu + 5
REG_LOOP = ([_case(f'reg-loop-K2-G{p}x', 'reg', [32], 2, N=16, G=(lambda n, p=p: p * _ROUNDS(n))) for p in (1, 2, 4)]
            + [_case('reg-loop-K9-G2x', 'reg', [32], 9, N=16, G=lambda n: 2 * _ROUNDS(n)),
               _case('reg-loop-K17-G1x', 'reg', [32], 17, N=16, G=lambda n: _ROUNDS(n)),
               _case('reg-loop-one', 'reg', [32], 2, N=16, G=lambda n: 1),
               _case('reg-loop-cu+1', 'reg', [32], 2, N=16, G=lambda n: n + 1)])

STRIP_WIDTHS = ([96], [32, 32, 64, 64], [160, 192], [224, 256], [256, 256], [64, 96, 128])
STRIP = ([_case(f'strip-{_w(s)}-K{K}', 'reg', s, K) for s in STRIP_WIDTHS for K in (5, 16, 33)]
         + [_case(f'strip-beacon-{_w(s)}-K65', 'reg', s, 65, S=_s_for(65), lists='beacon') for s in ([96], [224, 256])]
         + [_case(f'strip-d-D{D}', 'reg', [32, 32, 64, 64], 16, D=D) for D in (0, 5, 13)])

TILE_K = [_case(f'tile-k-K{K}', 'tile', [64, 32], K, D=4, S=_s_for(K), lists='beacon') for K in (5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129)]
# hidden widths 32 (an idle wave pair), 64, 96 (half-row shares), 128, 160 (2 + 1 blocks), 288 (3 + 2), 512 (4); each once
TILE_WAVE = [_case(f'tile-wave-{_w(s)}', 'tile', s, 8, D=29) for s in ([32, 64, 96, 32], [128, 160, 160], [288, 288], [512, 1024])]
TILE_D = ([_case(f'tile-d-D{D}', 'tile', [64, 32], 5, D=D) for D in range(14)]
          + [_case(f'tile-d-D{D}', 'tile', [64, 32], 16, D=D) for D in (128, 132, 588)]
          + [_case('tile-d-D128-misaligned', 'tile', [64, 32], 16, D=128, misalign=True)])
# 128-row tiles are taken when ceil(G / 16) >= 2 n_cu (K = 8) or G * 2 row tiles >= 2 n_cu (K = 129)
TILE_128 = [_case(f'tile-128-{_w(s)}-K{K}-{tag}', 'tile', s, K, D=4, G=g)
            for s in ([32], [64, 32])
            for K, tag, g in ((8, 'at', lambda n: 16 * 2 * n + 3), (8, 'below', lambda n: 16 * (2 * n - 1)),
                              (129, 'at', lambda n: 2 * n + 1), (129, 'below', lambda n: n - 1))]
TILE_SLOT = ([_case(f'tile-slot-{ns}', 'tile', [32], 8, D=0, G=(lambda n, ns=ns: 8 * ns)) for ns in (8, 16)]
             + [_case(f'tile-slot-{m}cu{d:+d}', 'tile', [32], 8, D=0, G=(lambda n, m=m, d=d: 8 * (m * n + d)))
                for m in (1, 2, 3, 6) for d in (-1, 0, 1, 7, 8, 9)])
TILE_APPEND = [_case('tile-append', 'tile', [64, 160], 16, D=20, S=37)]
TILE_ALL = [_case(f'tile-all-N{N}', 'tile', [64, 32], N, D=4, N=N, group_all=True) for N in (1, 63, 64, 65, 130)]
# first-level shapes every family accepts: kind 'reg' takes the register kernel for the first, the strip kernel for the others
CROSS = [_case(f'cross-{_w(s)}-K{K}', 'reg', s, K, D=D) for D, K, s in ((6, 32, [64, 64, 128]), (3, 16, [32, 32, 64, 64]),
                                                                         (13, 64, [128, 128, 256]), (6, 8, [96]))]

EXACT_CASES = REG_SIG + REG_K + REG_D + REG_OUT + REG_LOOP + STRIP + TILE_K + TILE_WAVE + TILE_D + TILE_128 + TILE_SLOT + TILE_APPEND + TILE_ALL + CROSS
assert len({c['id'] for c in EXACT_CASES}) == len(EXACT_CASES)

# general values: (name, kind, widths, K, D, B, N, S)
GENERAL_CASES = [('sa1-9-64-64-128', 'reg', [64, 64, 128], 32, 6, 2, 256, 32), ('sa2-131-128-128-256', 'tile', [128, 128, 256], 64, 128, 2, 128, 16),
                 ('strip-64-96-128', 'reg', [64, 96, 128], 16, 6, 2, 128, 24), ('wide-512-256', 'tile', [512, 256], 8, 29, 2, 64, 28),
                 ('tile-K129', 'tile', [64, 32], 129, 4, 2, 200, 8), ('reg-pack4-32-64', 'reg', [32, 64], 8, 0, 3, 100, 21)]


def scene_of(case, n_cu=N_CU_NOMINAL):
    B, S = (1, int(case['G'](n_cu))) if case['G'] else (case['B'], case['S'])
    return R.exact_scene(B, case['N'], S, case['K'], case['D'], case['widths'], case['lists'], case['seed'],
                         group_all=case.get('group_all', False))


def _geometry(kind, K):
    """(neighbourhoods per tile, rows per tile) as the kernels of `kind` lay a launch out (tile: its 64-row instance)."""
    if kind == 'reg':
        return (4 if K <= 8 else 2 if K <= 16 else 1), 32
    kp = 8 if K <= 8 else 16 if K <= 16 else 32 if K <= 32 else 64
    return 64 // kp, 64


def _dev(a, dev, dtype=np.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def _weights(sc, case, dev, kind=None):
    from catgrasp_amd import primitives as prim
    return prim.SetAbstractionWeights(sc['raw'], 3 + case['D'], dev, kind=kind or case['kind'])


def _launch(sc, case, dev, kind=None, **kw):
    from catgrasp_amd import primitives as prim
    W = _weights(sc, case, dev, kind)
    pts = _dev(sc['points'], dev)
    if case.get('misalign'):
        buf = torch.zeros(pts.numel() + 8, device=dev)
        off = 1 + (-(buf.data_ptr() // 4) % 4)              # one float past a 16-byte boundary
        view = buf[off:off + pts.numel()].view(pts.shape)
        view.copy_(pts)
        pts = view
        assert pts.data_ptr() % 16 != 0 and pts.is_contiguous()
    return prim.group_mlp_max(_dev(sc['xyz'], dev), pts, _dev(sc['new_xyz'], dev), _dev(sc['idx'], dev, np.int64), W, channels_last=True, **kw)


def assert_exact(got, ref, case, sc, what=''):
    """torch.equal(got, ref.float()) -- value equality, bit for bit up to the sign of zero; a failure names the first offending
    (b, s, c), its pack slot and the row tile that carries the reference's maximum."""
    want = torch.from_numpy(ref).float()
    got = got.detach().cpu()
    assert got.shape == want.shape, (case['id'], tuple(got.shape), tuple(want.shape))
    if torch.equal(got, want):
        return
    bad = (got != want) | torch.isnan(got)
    b, s, c = [int(v) for v in bad.nonzero()[0]]
    K = case['K']
    pack, rows = _geometry(case['kind'] if not what else what, K)
    g = b * want.shape[1] + s
    k = int(R.sa_ref_rows(sc['xyz'][b:b + 1], None if sc['points'] is None else sc['points'][b:b + 1],
                          None if sc['new_xyz'] is None else sc['new_xyz'][b:b + 1, s:s + 1],
                          None if sc['idx'] is None else sc['idx'][b:b + 1, s:s + 1], sc['layers'])[0, 0, :, c].argmax())
    raise AssertionError(f"{case['id']} {what}: {int(bad.sum())} of {bad.numel()} outputs differ; first at (b, s, c) = ({b}, {s}, {c}): got "
                         f'{got[b, s, c].item()!r}, reference {want[b, s, c].item()!r}; neighbourhood {g} = slot {g // pack}, position '
                         f'{g % pack} of its pack of {pack}; the reference maximum sits in row {k} = row tile {k // rows} ({rows}-row tiles)')


def _n_cu(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _run_exact(case, dev, **kw):
    sc = scene_of(case, _n_cu(dev))
    got = _launch(sc, case, dev, **kw)
    assert_exact(got, R.sa_ref(sc['xyz'], sc['points'], sc['new_xyz'], sc['idx'], sc['layers']), case, sc)
    return sc, got


def _ids(cases):
    return [c['id'] for c in cases]


# ------------------------------------------------------------------------------------------------------- register kernel
@pytest.mark.parametrize('case', REG_SIG, ids=_ids(REG_SIG))
def test_register_kernel_every_signature_and_packing(cuda_device, case):
    _run_exact(case, cuda_device)


@pytest.mark.parametrize('case', REG_K, ids=_ids(REG_K))
def test_register_kernel_every_row_carries_the_maximum_once(cuda_device, case):
    _run_exact(case, cuda_device)


@pytest.mark.parametrize('case', REG_D, ids=_ids(REG_D))
def test_register_kernel_every_input_width(cuda_device, case):
    _run_exact(case, cuda_device)


@pytest.mark.parametrize('case', REG_OUT, ids=_ids(REG_OUT))
def test_register_kernel_writes_a_slice_and_nothing_else(cuda_device, case):
    sc = scene_of(case)
    ref = R.sa_ref(sc['xyz'], sc['points'], sc['new_xyz'], sc['idx'], sc['layers'])
    B, S, C = ref.shape
    wide = torch.full((B, S, C + 11), -77.0, device=cuda_device)
    got = _launch(sc, case, cuda_device, out=wide[:, :, 5:5 + C])
    assert got.data_ptr() == wide[:, :, 5:].data_ptr()
    assert_exact(wide[:, :, 5:5 + C], ref, case, sc)
    assert bool((wide[:, :, :5] == -77.0).all()) and bool((wide[:, :, 5 + C:] == -77.0).all())
    # the (B, C, S) layout of torch.max(new_points, 2)[0], as a slice along the channels too
    from catgrasp_amd import primitives as prim
    wide = torch.full((B, C + 3, S), -77.0, device=cuda_device)
    prim.group_mlp_max(_dev(sc['xyz'], cuda_device), _dev(sc['points'], cuda_device), _dev(sc['new_xyz'], cuda_device),
                       _dev(sc['idx'], cuda_device, np.int64), _weights(sc, case, cuda_device), out=wide[:, 2:2 + C])
    assert_exact(wide[:, 2:2 + C].permute(0, 2, 1), ref, case, sc)
    assert bool((wide[:, :2] == -77.0).all()) and bool((wide[:, 2 + C:] == -77.0).all())


@pytest.mark.parametrize('case', REG_LOOP, ids=_ids(REG_LOOP))
def test_register_kernel_persistent_loop(cuda_device, case):
    _run_exact(case, cuda_device)


# ---------------------------------------------------------------------------------------------------------- strip kernel
@pytest.mark.parametrize('case', STRIP, ids=_ids(STRIP))
def test_strip_kernel(cuda_device, case):
    _run_exact(case, cuda_device)


# ----------------------------------------------------------------------------------------------------------- tile kernel
@pytest.mark.parametrize('case', TILE_K, ids=_ids(TILE_K))
def test_tile_kernel_every_packing_and_row_tile(cuda_device, case):
    _run_exact(case, cuda_device)


@pytest.mark.parametrize('case', TILE_WAVE, ids=_ids(TILE_WAVE))
def test_tile_kernel_every_wave_share(cuda_device, case):
    _run_exact(case, cuda_device)


def _leave_infinities_in_the_strips(dev):
    """The zero pad of the first layer's input meets zero weight columns, so a missing zero fill shows only where the stale strip
    holds a non-finite value (0 * inf = NaN) -- and the stale values of a finite launch are finite.  LDS is not cleared between
    launches: one launch over every resident workgroup of the chip whose 64-wide hidden layer overflows (features 3e38, weights 1)
    leaves +inf in columns 0 .. 63 of every strip of the [64, 32] networks below (same row stride).  Its output is discarded.
    Where a device did clear LDS, the cases after it would only lose this extra sensitivity."""
    from catgrasp_amd import primitives as prim
    n = 3 * 8 * _n_cu(dev)
    W = prim.SetAbstractionWeights([(np.ones((64, 7)), np.zeros(64), None), (np.zeros((32, 64)), np.zeros(32), None)], 7, dev, kind='tile')
    prim.group_mlp_max(torch.zeros(1, 8, 3, device=dev), torch.full((1, 8, 4), 3e38, device=dev), torch.zeros(1, n, 3, device=dev),
                       torch.zeros(1, n, 8, dtype=torch.int64, device=dev), W, channels_last=True, check_indices=False)


@pytest.mark.parametrize('case', TILE_D, ids=_ids(TILE_D))
def test_tile_kernel_gather(cuda_device, case):
    if case['D'] <= 13:
        _leave_infinities_in_the_strips(cuda_device)
    _run_exact(case, cuda_device)


@pytest.mark.parametrize('case', TILE_128, ids=_ids(TILE_128))
def test_tile_kernel_128_row_tiles_and_just_below(cuda_device, case):
    _run_exact(case, cuda_device)


@pytest.mark.parametrize('case', TILE_SLOT, ids=_ids(TILE_SLOT))
def test_tile_kernel_slot_order(cuda_device, case):
    _run_exact(case, cuda_device)


def test_tile_kernel_appends_the_next_level_rows(cuda_device):
    """append_xyz: channels [C, C + n) of every output row = new_xyz ++ zeros, the rows cg_sa_concat_input builds."""
    import ctypes
    from catgrasp_amd import _lib as L
    case = TILE_APPEND[0]
    sc = scene_of(case)
    ref = R.sa_ref(sc['xyz'], sc['points'], sc['new_xyz'], sc['idx'], sc['layers'])
    B, S, C = ref.shape
    ld = (C + 3 + 7) & ~7
    rows = torch.full((B, S, ld), 9.0, device=cuda_device)
    got = _launch(sc, case, cuda_device, out=rows[:, :, :C], append_xyz=ld - C)
    assert_exact(got, ref, case, sc)
    want = torch.empty((B * S, ld), device=cuda_device)
    centres, feats = _dev(sc['new_xyz'], cuda_device), got.contiguous()          # named: both outlive the launch that reads them
    L.check(L.lib().cg_sa_concat_input(L._p(centres), L._p(feats), ctypes.c_long(B * S), ctypes.c_int(C), ctypes.c_int(ld), L._p(want),
                                       L._stream()), 'cg_sa_concat_input')
    assert torch.equal(rows[:, :, C:C + 3].cpu(), torch.from_numpy(sc['new_xyz']).float()) and bool((rows[:, :, C + 3:] == 0).all())
    diff = (rows.view(B * S, ld) != want).nonzero().cpu().tolist()
    assert torch.equal(rows.view(B * S, ld), want), f'{len(diff)} entries differ from cg_sa_concat_input, first (row, column): {diff[:8]}'


@pytest.mark.parametrize('case', TILE_ALL, ids=_ids(TILE_ALL))
def test_tile_kernel_group_all_mode(cuda_device, case):
    from catgrasp_amd import primitives as prim
    sc = scene_of(case)
    got = prim.group_all_mlp_max(_dev(sc['xyz'], cuda_device), _dev(sc['points'], cuda_device), _weights(sc, case, cuda_device), fused=True)
    ref = R.sa_ref(sc['xyz'], sc['points'], None, None, sc['layers'])
    assert_exact(got[:, None, :], ref, case, sc)


@pytest.mark.parametrize('kind', ['reg', 'tile'])
def test_an_out_of_range_index_sets_the_error_flag(cuda_device, kind):
    case = _case('flag', kind, [64, 32], 16, D=4)
    sc = scene_of(case)
    _, err = _launch(sc, case, cuda_device, check_indices=False)
    assert int(err.item()) == 0
    for bad in (case['N'], -1):
        sc['idx'][1, 3, 7] = bad
        _, err = _launch(sc, case, cuda_device, check_indices=False)
        assert int(err.item()) == 1, bad
        with pytest.raises(IndexError):
            _launch(sc, case, cuda_device)


@pytest.mark.parametrize('case', CROSS, ids=_ids(CROSS))
def test_kernel_families_agree(cuda_device, case):
    sc = scene_of(case)
    ref = R.sa_ref(sc['xyz'], sc['points'], sc['new_xyz'], sc['idx'], sc['layers'])
    reg = _launch(sc, case, cuda_device, kind='reg')
    tile = _launch(sc, case, cuda_device, kind='tile')
    assert_exact(reg, ref, case, sc, 'reg')
    assert_exact(tile, ref, case, sc, 'tile')
    assert torch.equal(reg, tile)


# -------------------------------------------------------------------------------------------------------- general values
@pytest.mark.parametrize('name,kind,widths,K,D,B,N,S', GENERAL_CASES, ids=[c[0] for c in GENERAL_CASES])
def test_general_values_within_the_per_element_bound(cuda_device, name, kind, widths, K, D, B, N, S):
    from catgrasp_amd import primitives as prim
    assert B * S <= 64
    sc = R.general_scene(B, N, S, K, D, widths, seed=zlib.crc32(name.encode()) & 0xffff)
    W = prim.SetAbstractionWeights(sc['raw'], 3 + D, cuda_device, kind=kind)
    got = prim.group_mlp_max(_dev(sc['xyz'], cuda_device), _dev(sc['points'], cuda_device), _dev(sc['new_xyz'], cuda_device),
                             _dev(sc['idx'], cuda_device, np.int64), W, channels_last=True)
    ref, bound = R.sa_bound(sc['xyz'], sc['points'], sc['new_xyz'], sc['idx'], sc['layers'])
    worst = dr.check_bound(got.cpu().numpy(), ref, bound, name)
    print(f'{name}: worst error / bound = {worst:.3f}')
