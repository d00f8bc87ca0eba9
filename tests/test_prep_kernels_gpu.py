"""Per-element tests of the kernels that build the networks' inputs and of the small ones around them, against the host chains of
tests/prep_ref.py (proved on the CPU by tests/test_prep_ref_cpu.py):

  * cg_build_grasp_input: bit for bit the float32 chain of grasp_point, and within the derived bound of the float64
    transforms_ref.grasp_transform, on every path of both kernels;
  * cg_build_nunocs_input: bit for bit the float32 chain, and within the derived bound of the float64 normalize_cloud;
  * cg_softmax_pg: labels, confidences and p_G against float64, probabilities within a measured bound (below);
  * cg_sdf_points_inside_batch: the exact byte per candidate of the float32 chain (xf is given in float32, so nothing is undecided).

Case ids name the kernel and the branch a case is meant to reach; tests/test_prep_ref_cpu.py asserts from a host restatement of the
slice logic that the seeded inputs do reach it, and the tests here assert the launcher's routing from the pointers they pass.
Branch -> cases:
  misc.hip  build_grasp_input_staged_kernel
              slice reused across candidates, G % 8 != 0                 test_build_grasp_input[S1-staged-slice-reused]
              re-stage at an object boundary inside a workgroup,
              granule lo & ~3 with lo % 4 != 0, copy tail i + 4 > nfl    test_build_grasp_input[S2-staged-restage-granule-copytail]
              fall-back to global gathers (range > BGI_CAP, and the
              range of exactly BGI_CAP / BGI_CAP + 1 points), the old
              slice used again after it                                  test_build_grasp_input[S3-staged-global-staged]
              strips: wave 0 only / two waves / a second round,
              mean == NULL                                               test_build_grasp_input[S4-staged-n{64,128,1088}-{mean,nomean}]
            build_grasp_input_kernel (n_pts % 64 != 0, or a pointer off 16 bytes)
              pair path, mean == NULL                                    test_build_grasp_input[P1-plain-pairs-n100-{mean,nomean}]
              odd n_pts: scalar tail, a pair across two candidates       test_build_grasp_input[P2-plain-odd-n33]
              G n_pts odd: the last thread holds one point               test_build_grasp_input[P3-plain-odd-total]
              ids off 8 bytes / out off 16 bytes: scalar path, guards    test_build_grasp_input_unaligned[P4-*]
              pair path on an aligned call (cloud off 16 bytes)          test_build_grasp_input_unaligned[P4-cloud-off4]
            both families, same inputs, same bytes                       test_build_grasp_input_families_agree[X-*]
            build_nunocs_input_kernel: threads / waves without a point,
              a multiple of the workgroup, + 1, the config's 8192;
              mean == NULL; the largest extent on each axis; extent 0    test_build_nunocs_input[*], test_build_nunocs_input_degenerate
            softmax_pg_kernel: last workgroup partly filled / full /
              one thread; C = 1; large logits, ties, last class          test_softmax_pg[*]
  sdf.hip   sdf_points_inside_batch_kernel
              last workgroup partly filled, the grid cap of 4096
              workgroups (E = 16384), one candidate past it, > 2 strides test_sdf_points_inside_batch[E*]
              P = 0, one lane, a partial / full / full + 1 round         test_sdf_points_inside_batch[P*]
              only the last point inside, .5 coordinates, -0, a point
              that rounds to nx, points beyond every face                test_sdf_points_inside_batch_planted

Probability bound of cg_softmax_pg.  The device expf is not correctly rounded and its error is not stated in this project, so the
bound is measured: the worst |probs - float64| over all the cases below was 7.62 u (u = 2^-24; B 5000, C 33) on an MI355X.  Four
times that figure, 30.5 u = 1.8e-6, lies above the cap of 1e-6 absolute (16.8 u), so the cap is what the tests assert."""
import ctypes

import numpy as np
import pytest
import torch

import dense_ref as R
import prep_ref as Q
from catgrasp_amd import _lib as L
from catgrasp_amd import ops
from catgrasp_amd._lib import _p, _stream

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))

_ci = ctypes.c_int
SOFTMAX_MEASURED_U = 7.62            # measured, see the module docstring
PROB_BOUND = min(4 * SOFTMAX_MEASURED_U * Q.U32, 1e-6)


def _dev(a, device):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _aligned16(*tensors):
    return all(t.data_ptr() % 16 == 0 for t in tensors)


# ------------------------------------------------------------------------------------------------------ build_grasp_input
GRASP = {'S1-staged-slice-reused': 'S1', 'S2-staged-restage-granule-copytail': 'S2', 'S3-staged-global-staged': 'S3',
         'S4-staged-n64-mean': 'S4-64', 'S4-staged-n64-nomean': 'S4-64-nomean', 'S4-staged-n128-mean': 'S4-128',
         'S4-staged-n128-nomean': 'S4-128-nomean', 'S4-staged-n1088-mean': 'S4-1088', 'S4-staged-n1088-nomean': 'S4-1088-nomean',
         'P1-plain-pairs-n100-mean': 'P1', 'P1-plain-pairs-n100-nomean': 'P1-nomean', 'P2-plain-odd-n33': 'P2', 'P3-plain-odd-total': 'P3'}


@pytest.mark.parametrize('cid', list(GRASP))
def test_build_grasp_input(cuda_device, cid):
    case = Q.grasp_case(GRASP[cid])
    xyz, nrm, ids, T = (_dev(case[k], cuda_device) for k in ('xyz32', 'nrm32', 'ids', 'T12'))
    out = torch.empty(ids.shape + (6,), dtype=torch.float32, device=cuda_device)
    # the launcher's routing: the staged kernel iff n_pts % 64 == 0 and ids, out and both clouds are 16-byte aligned
    assert _aligned16(xyz, nrm, ids, out)
    assert (ids.shape[1] % 64 == 0) == ('staged' in cid)
    ops.build_grasp_input(xyz, nrm, ids, T, _dev(case['mean32'], cuda_device), _dev(case['inv_std32'], cuda_device), out=out)
    ratio = Q.check_grasp(case, out.cpu().numpy(), cid)
    print(f'{cid}: worst error / bound vs float64 {ratio:.3f}')


def _bgi_raw(case, device, ids_off=0, out_off=0, cloud_off=0):
    """cg_build_grasp_input through the C ABI on views offset by *_off ELEMENTS from aligned allocations.
    -> (out, guards unchanged)."""
    G, n_pts = case['ids'].shape
    N = G * n_pts

    def shifted(a, off, pad=0.0):
        flat = torch.from_numpy(np.ascontiguousarray(a).reshape(-1))
        buf = torch.full((4 + off + flat.numel() + 8,), pad, dtype=flat.dtype).to(device)
        assert buf.data_ptr() % 16 == 0
        buf[4 + off:4 + off + flat.numel()] = flat.to(device)
        return buf, buf[4 + off:4 + off + flat.numel()]
    _, xyz = shifted(case['xyz32'], cloud_off)
    _, nrm = shifted(case['nrm32'], cloud_off)
    _, ids = shifted(case['ids'], ids_off, 0)
    obuf, out = shifted(np.zeros(N * 6, np.float32), out_off, -777.0)
    out.fill_(-555.0)
    assert ids.data_ptr() % 8 == (4 * ids_off) % 8 and out.data_ptr() % 16 == (4 * out_off) % 16 and xyz.data_ptr() % 16 == (4 * cloud_off) % 16
    T, mean, inv_std = (_dev(case[k], device) for k in ('T12', 'mean32', 'inv_std32'))
    L.check(L.lib().cg_build_grasp_input(_p(xyz), _p(nrm), _ci(len(case['xyz32'])), _p(ids), _p(T), _p(mean), _p(inv_std), _ci(G), _ci(n_pts),
                                         _p(out), _stream()), 'cg_build_grasp_input')
    torch.cuda.synchronize()
    host = obuf.cpu().numpy()
    lead = 4 + out_off
    guards_ok = bool((host[:lead] == -777.0).all() and (host[lead + N * 6:] == -777.0).all())
    return host[lead:lead + N * 6].reshape(G, n_pts, 6).copy(), guards_ok


UNALIGNED = {'P4-ids-off4': dict(ids_off=1), 'P4-out-off4': dict(out_off=1), 'P4-out-off8': dict(out_off=2),
             'P4-ids-off4-out-off4': dict(ids_off=1, out_off=1), 'P4-ids-off4-out-off12': dict(ids_off=1, out_off=3),
             'P4-cloud-off4': dict(cloud_off=1)}


@pytest.mark.parametrize('cid', list(UNALIGNED))
def test_build_grasp_input_unaligned(cuda_device, cid):
    """The plain kernel takes its 8-byte id load and 16-byte stores only when ids / out are aligned for them: views offset from an
    aligned allocation give the same bytes as the chain, and the elements before and after out stay as they were."""
    case = Q.grasp_case('P4')
    out, guards_ok = _bgi_raw(case, cuda_device, **UNALIGNED[cid])
    assert guards_ok, f'{cid}: the kernel wrote outside out'
    ratio = Q.check_grasp(case, out, cid)
    print(f'{cid}: worst error / bound vs float64 {ratio:.3f}')


@pytest.mark.parametrize('cid', ['X-staged-vs-plain-scalar', 'X-staged-vs-plain-pairs'])
def test_build_grasp_input_families_agree(cuda_device, cid):
    case = Q.grasp_case('X')
    assert case['ids'].shape[1] == 128
    staged, ok0 = _bgi_raw(case, cuda_device)                                            # aligned, n_pts % 64 == 0: the staged kernel
    plain, ok1 = _bgi_raw(case, cuda_device, **(dict(ids_off=1, out_off=1) if 'scalar' in cid else dict(cloud_off=1)))
    assert ok0 and ok1
    R.check_bitwise(plain, staged, cid)
    Q.check_grasp(case, staged, cid)


# ----------------------------------------------------------------------------------------------------- build_nunocs_input
def _run_nunocs(case, device):
    return ops.build_nunocs_input(_dev(case['xyz32'], device), _dev(case['nrm32'], device), _dev(case['ids'], device),
                                  _dev(case['mean32'], device), _dev(case['inv_std32'], device)).cpu().numpy()


@pytest.mark.parametrize('with_mean', [False, True], ids=['nomean', 'mean'])
@pytest.mark.parametrize('n_pts', [1, 63, 1024, 1025, 8192])
@pytest.mark.parametrize('B', [1, 5])
def test_build_nunocs_input(cuda_device, B, n_pts, with_mean):
    case = Q.nunocs_case(B, n_pts, with_mean)
    ratio = Q.check_nunocs(case, _run_nunocs(case, cuda_device), f'nunocs B {B} n_pts {n_pts}')
    print(f'nunocs B {B} n_pts {n_pts} mean {with_mean}: worst error / bound vs float64 {ratio:.3f}')


@pytest.mark.parametrize('with_mean', [False, True], ids=['nomean', 'mean'])
def test_build_nunocs_input_degenerate(cuda_device, with_mean):
    """A cloud of one repeated point: extent 0, divisor 1e-15f; the bytes are whatever the float32 chain gives."""
    case = Q.nunocs_case(5, 1024, with_mean, degenerate=True)
    Q.check_nunocs(case, _run_nunocs(case, cuda_device), 'nunocs degenerate')


# ------------------------------------------------------------------------------------------------------------- softmax_pg
@pytest.mark.parametrize('C', [1, 2, 10, 33])
@pytest.mark.parametrize('B', [1, 255, 256, 257, 5000])
def test_softmax_pg(cuda_device, B, C):
    x, planted = Q.softmax_case(B, C)
    probs, label, conf, pg = (t.cpu().numpy() for t in ops.softmax_pg(_dev(x, cuda_device)))
    worst = float(np.abs(probs.astype(np.float64) - Q.tref.softmax(x.astype(np.float64), axis=1)).max() / Q.U32)
    print(f'softmax B {B} C {C}: worst |probs - float64| {worst:.2f} u')
    Q.check_softmax(x, planted, probs, label, conf, pg, PROB_BOUND, f'softmax B {B} C {C}')


# ------------------------------------------------------------------------------------------------- sdf_points_inside_batch
def _sdf_batch(grid, xf, pts, device):
    g, x, p = _dev(grid, device), _dev(xf, device), _dev(pts, device)
    out = torch.full((len(xf) + 64,), 7, dtype=torch.uint8, device=device)             # 64 guard bytes behind the E results
    nx, ny, nz = grid.shape
    L.check(L.lib().cg_sdf_points_inside_batch(_p(g), _ci(nx), _ci(ny), _ci(nz), _p(x), ctypes.c_long(len(xf)), _p(p),
                                               _ci(len(pts)), _p(out), _stream()), 'cg_sdf_points_inside_batch')
    host = out.cpu().numpy()
    assert (host[len(xf):] == 7).all(), 'the kernel wrote behind out[E]'
    return host[:len(xf)]


SDF_SHAPES = {'E1': (1, 64), 'E3': (3, 64), 'E4': (4, 64), 'E5': (5, 64), 'E64': (64, 64), 'E16384-grid-cap': (16384, 65),
              'E16385-one-past-the-cap': (16385, 64), 'E40000-three-strides': (40000, 33),
              'P0': (37, 0), 'P1': (37, 1), 'P63': (37, 63), 'P64': (37, 64), 'P65': (37, 65), 'P3000': (37, 3000)}


@pytest.mark.parametrize('cid', list(SDF_SHAPES))
def test_sdf_points_inside_batch(cuda_device, cid):
    E, P = SDF_SHAPES[cid]
    grid, xf, pts = Q.sdf_random_case(E, P)
    exp = Q.sdf_inside_chain(grid, xf, pts)
    if E >= 37 and P >= 33:
        assert 0.05 < exp.mean() < 0.95                     # both verdicts are well represented
    got = _sdf_batch(grid, xf, pts, cuda_device)
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, f'{cid}: {len(bad)} of {E} candidates differ from the float32 chain, first {bad[:8].tolist()}'


def test_sdf_points_inside_batch_planted(cuda_device):
    grid, xf, pts, exp, names = Q.sdf_planted_case()
    got = _sdf_batch(grid, xf, pts, cuda_device)
    assert np.array_equal(got, exp), [n for n, a, b in zip(names, got, exp) if a != b]
