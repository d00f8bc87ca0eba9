"""Per-element tests of the dense kernels against float64 / emulated references (tests/dense_ref.py):

  * cg_gemm_bias_act / cg_gemm_bias_relu_groupmax (exact f32): bitwise the k-ordered fmaf chain, on both the wavefront-per-tile and
    the workgroup-tile kernel, incl. ldx > K, ldy > N, row_bias with ld_rb > N, eye_k, bias = null;
  * cg_gemm_bias_act_{f16x3,bf16x3}: within gamma_K of the exact piece products, and within the propagated bound of the float64
    product, incl. the K tail (K % 64 != 0) and the range-guard status bits;
  * cg_pointmlp_max* in all four modes: the 128 -> 1024 stream on inputs whose front layers are exact (small integers), and the
    whole chain on general values within the propagated bound, over the launcher's branches (tail balancing, channel split CS,
    uneven slicing, the negative branch of the atomic max) and the range-guard status bits.

Case ids name the launcher branch a case is meant to reach; the test asserts it, from the launcher's own formulas and this device's
CU count.  Branch -> cases:
  gemm.hip  wavefront-per-tile kernel (<= SMALL_TILES tiles)   test_gemm_f32_bitwise[small-*] (incl. 2047 / 2048 tiles), groupmax[small-*]
            workgroup-tile kernel (> SMALL_TILES tiles)      test_gemm_f32_bitwise[tile-*] (incl. 2049 tiles), strides[tile-*], groupmax[tile-*]
            K tail of the LDS chunk (K % 64 != 0)            K in {8, 16, 72, 80}; ldx > K / ldy > N / row_bias / eye_k / null bias: strides
            group max in registers / per element             groupmax rpg 32, 64 / rpg 7, 40 (groups across 32-row tiles)
  gemm_split.hip  K tail (K % 64 == 16)                      test_gemm_split_pieces_and_bound[*-ktail]; status word: test_gemm_f16x3_status_bits
  pointmlp.hip  CS = 8 / 4 / 2 / 1 (asm stream)              test_pointmlp_f32_bitwise[*-few] / cs_levels[cs4, cs2] / [*-many]
                tail balancing (B >= 2 #CU, B % 2 #CU != 0)  test_pointmlp_f32_cs_levels_and_tail[tail-cs1]
                nsplit > 1, uneven slices, nsplit > ntiles   test_pointmlp_f32_bitwise[N*-ns{2,3,7,64}-*]
                negative branch of atomic_max_f32           test_pointmlp_negative_max_channels[f32]
  pointmlp_split.hip  one tile / several, mid 0 / 1 / 2      test_pointmlp_split_l3_vs_pieces[*], test_pointmlp_general_values_bound[*]
                      tail (B >= #CU, B % #CU != 0, N > 256) test_pointmlp_split_tail[*]
                      nsplit > 1 + negative atomic max       test_pointmlp_negative_max_channels[bf16x3, f16x3, f16fp8x2]
                      status word                            test_pointmlp_status_bits[f16x3, f16fp8x2]"""
import ctypes

import numpy as np
import pytest
import torch

import dense_ref as R
from catgrasp_amd import _lib as L
from catgrasp_amd import folding, ops
from catgrasp_amd._lib import _p, _stream

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))

_ci = ctypes.c_int
SMALL_TILES = 2048                  # gemm.hip: 32 x 32 output tiles up to which the wavefront-per-tile kernel runs
SPLIT = {'f32': False, 'bf16x3': 'bf16', 'f16x3': 'f16', 'f16fp8x2': 'f16fp8'}
RATIOS = {}                         # worst observed error / bound per mode (printed with -s)


def _ratio(mode, r):
    RATIOS[mode] = max(RATIOS.get(mode, 0.0), r)


def _cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to('cuda:0') if dtype is None else t.to(dtype).to('cuda:0')


# ------------------------------------------------------------------------------------------------------------ GEMM helpers
def _gemm(mode, x, K, wp, N, bias=None, row_bias=None, rpg=1, relu=False, eye_k=0, ldy=None, status=None):
    """C ABI call; x: (M, ldx) device tensor (columns >= K are not the matrix), y: (M, ldy) pre-filled with a sentinel."""
    M, ldx = x.shape
    ldy = N if ldy is None else ldy
    y = torch.full((M, ldy), 1234.5, dtype=torch.float32, device=x.device)
    ld_rb = row_bias.shape[1] if row_bias is not None else 0
    name = {'f32': 'cg_gemm_bias_act', 'f16x3': 'cg_gemm_bias_act_f16x3', 'bf16x3': 'cg_gemm_bias_act_bf16x3'}[mode]
    args = (_p(x), _ci(M), _ci(K), _ci(ldx), _p(wp), _ci(N), _p(bias), _p(row_bias), _ci(rpg), _ci(ld_rb), _ci(int(relu)), _ci(eye_k),
            _p(y), _ci(ldy))
    fn = getattr(L.lib(), name)
    st = fn(*args, _p(status), _stream()) if mode == 'f16x3' else fn(*args, _stream())
    assert st == 0, (name, st)
    torch.cuda.synchronize()
    y = y.cpu().numpy()
    assert (y[:, N:] == np.float32(1234.5)).all(), f'{name} wrote columns >= N (ldy = {ldy})'
    return y[:, :N]


def _pack(w, mode):
    if mode == 'f32':
        return _dev(folding.pack_b(w))
    return _dev(folding.pack_b_split(w, R.ELEM[mode]).view(np.int16))


def _x_padded(x, ldx):
    """(M, K) -> (M, ldx) device tensor with NaN in the columns >= K: a kernel that reads them poisons its result."""
    M, K = x.shape
    xp = np.full((M, ldx), np.nan, np.float32)
    xp[:, :K] = x
    return _dev(xp)


def _rows_checked(M):
    """every 32- and 64-row tile boundary (the last row before and the first row of every tile) plus the last row"""
    r = set([0, M - 1])
    for t in range(32, M, 32):
        r.update((t - 1, t))
    return np.array(sorted(r))


def _cols_checked(N, rng):
    c = set([0, N - 1])
    for t in range(32, N, 32):
        c.update((t - 1, t))
    c = sorted(c)
    if len(c) > 48:
        c = sorted(set(c[:16] + c[-16:] + list(rng.choice(c, 16, replace=False))))
    return np.array(c)


def _branch(M, N):
    return 'small' if ((M + 31) // 32) * ((N + 31) // 32) <= SMALL_TILES else 'tile'


# (M, N, K, branch): M / N / K edges on the wavefront-per-tile kernel, the same M edges on the workgroup-tile kernel (N wide enough to
# pass SMALL_TILES), and the small / tile switch at SMALL_TILES - 1, SMALL_TILES, SMALL_TILES + 1 tiles
GEMM_CASES = ([(m, 33, 72, 'small') for m in (1, 31, 32, 33, 127, 128, 129)]
              + [(33, n, 80, 'small') for n in (1, 9, 10, 100, 4096)]
              + [(129, 100, k, 'small') for k in (8, 16, 72, 1088)]
              + [(m, 32 * (SMALL_TILES // ((m + 31) // 32) + 1) - 7, 16, 'tile') for m in (1, 31, 32, 33, 127, 128, 129)]
              + [(32 * (SMALL_TILES - 1), 10, 8, 'small'), (32 * SMALL_TILES, 10, 8, 'small'), (32 * SMALL_TILES + 1, 10, 8, 'tile')])


@pytest.mark.parametrize('M,N,K,branch', GEMM_CASES, ids=[f'{b}-M{m}-N{n}-K{k}' for m, n, k, b in GEMM_CASES])
def test_gemm_f32_bitwise(M, N, K, branch):
    assert _branch(M, N) == branch
    rng = np.random.default_rng(M * 7919 + N * 31 + K)
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    y = _gemm('f32', _x_padded(x, K), K, _pack(w, 'f32'), N, bias=_dev(bias), relu=True)
    rows = _rows_checked(M) if M <= 4096 else np.concatenate([_rows_checked(4096), np.arange(M - 70, M)])
    cols = _cols_checked(N, rng)
    emu = R.gemm_f32_epilogue(R.fma_chain(x[rows], w[cols]), cols, rows, bias=bias, relu=True)
    R.check_bitwise(y[np.ix_(rows, cols)], emu, f'cg_gemm_bias_act {branch} M={M} N={N} K={K}')
    # the whole tensor: the f32 chain bound
    ref, bnd = R.dense_bound(x.astype(np.float64), np.zeros((M, K)), w, bias, 'f32', K + 1)
    _ratio('f32', R.check_bound(y, np.maximum(ref, 0), bnd, 'cg_gemm_bias_act vs float64'))


# ldx > K (NaN-poisoned padding), ldy > N (sentinel columns), row_bias with rows_per_group 1 / 7 / 1000 and ld_rb > N, eye_k, bias = null
LD_CASES = [(M, N, K, rpg, eye, nob) for (M, N, K) in ((100, 40, 72), (33000, 40, 72)) for rpg, eye, nob in ((1, 0, False), (7, 3, False),
                                                                                                       (1000, 64, True))]


@pytest.mark.parametrize('M,N,K,rpg,eye_k,no_bias', LD_CASES,
                         ids=[f'{_branch(m, n)}-M{m}-rpg{r}-eye{e}' + ('-nobias' if nb else '') for m, n, k, r, e, nb in LD_CASES])
def test_gemm_f32_strides_row_bias(M, N, K, rpg, eye_k, no_bias):
    rng = np.random.default_rng(rpg + eye_k)
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = None if no_bias else rng.standard_normal(N).astype(np.float32)
    G = (M + rpg - 1) // rpg
    rb = rng.standard_normal((G, N + 5)).astype(np.float32)
    y = _gemm('f32', _x_padded(x, K + 12), K, _pack(w, 'f32'), N, bias=None if no_bias else _dev(bias), row_bias=_dev(rb), rpg=rpg,
              eye_k=eye_k, ldy=N + 3)
    rows = _rows_checked(min(M, 1100))
    cols = np.arange(N)
    emu = R.gemm_f32_epilogue(R.fma_chain(x[rows], w), cols, rows, bias=bias, eye_k=eye_k, row_bias=rb, rows_per_group=rpg)
    R.check_bitwise(y[rows], emu, f'cg_gemm_bias_act {_branch(M, N)} rpg={rpg} eye_k={eye_k}')


GMAX_CASES = [(98, 64, 32, 7), (448, 100, 64, 32), (65560, 40, 16, 40), (65536, 40, 16, 64), (70 * 40, 60, 8, 40)]


@pytest.mark.parametrize('M,N,K,rpg', GMAX_CASES, ids=[f'{_branch(m, n)}-M{m}-N{n}-rpg{r}' for m, n, k, r in GMAX_CASES])
def test_gemm_groupmax_f32_bitwise(M, N, K, rpg):
    rng = np.random.default_rng(M + rpg)
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    G = M // rpg
    out = torch.empty((G, N), dtype=torch.float32, device='cuda:0')
    xd, wp, bd = _dev(x), _pack(w, 'f32'), _dev(bias)          # held for the kernel's lifetime
    st = L.lib().cg_gemm_bias_relu_groupmax(_p(xd), _ci(M), _ci(K), _ci(K), _p(wp), _ci(N), _p(bd), _ci(rpg), _p(out), _stream())
    assert st == 0
    out = out.cpu().numpy()
    gs = sorted(set([0, G - 1] + list(np.random.default_rng(1).choice(G, min(G, 12), replace=False))))
    rows = np.concatenate([np.arange(g * rpg, (g + 1) * rpg) for g in gs])
    cols = np.arange(N)
    emu = R.gemm_f32_epilogue(R.fma_chain(x[rows], w), cols, rows, bias=bias, relu=True).reshape(len(gs), rpg, N).max(axis=1)
    R.check_bitwise(out[gs], emu, f'cg_gemm_bias_relu_groupmax {_branch(M, N)}')


# ------------------------------------------------------------------------------------------------------------- split GEMMs
SPLIT_GEMM_CASES = ([(m, 33, 80) for m in (1, 31, 32, 33, 127, 128, 129)] + [(129, n, 16) for n in (1, 9, 10, 100, 4096)]
                    + [(257, 100, k) for k in (16, 80, 1088)])


@pytest.mark.parametrize('mode', ['f16x3', 'bf16x3'])
@pytest.mark.parametrize('M,N,K', SPLIT_GEMM_CASES, ids=[f'M{m}-N{n}-K{k}' + ('-ktail' if k % 64 else '') for m, n, k in SPLIT_GEMM_CASES])
def test_gemm_split_pieces_and_bound(mode, M, N, K):
    rng = np.random.default_rng(M * 13 + N + K)
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    st = torch.zeros(1, dtype=torch.int32, device='cuda:0')
    y = _gemm(mode, _x_padded(x, K + 4), K, _pack(w, mode), N, bias=_dev(bias), ldy=N + 1, status=st)
    if mode == 'f16x3':
        assert int(st.item()) == 0
    # (a) the exact piece products: pins the kernel's piece rounding to folding's statement of it
    S, A = R.piece_sum(x, w, mode)
    ref = S + bias.astype(np.float64)
    bnd = R.gamma(K + 1) * (A + np.abs(bias))
    _ratio(mode + ' pieces', R.check_bound(y, ref, bnd, f'{mode} GEMM vs its exact piece products'))
    # (b) the float64 product, with the propagated bound (split term included)
    ref, bnd = R.dense_bound(x.astype(np.float64), np.zeros((M, K)), w, bias, mode, K + 1)
    _ratio(mode, R.check_bound(y, ref, bnd, f'{mode} GEMM vs float64'))


@pytest.mark.parametrize('mode', ['f16x3', 'bf16x3'])
def test_gemm_split_strides_row_bias(mode):
    rng = np.random.default_rng(5)
    M, N, K = 300, 70, 96
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    for rpg, eye_k in ((1, 3), (7, 64), (1000, 0)):
        rb = rng.standard_normal(((M + rpg - 1) // rpg, N + 9)).astype(np.float32)
        y = _gemm(mode, _x_padded(x, K + 8), K, _pack(w, mode), N, row_bias=_dev(rb), rpg=rpg, eye_k=eye_k, relu=True, ldy=N + 6)
        S, A = R.piece_sum(x, w, mode)
        add = rb[np.arange(M) // rpg, :N].astype(np.float64) + np.where(np.arange(N) % (eye_k + 1) == 0, 1.0, 0.0)[None, :] * (eye_k > 0)
        ref = np.maximum(S + add, 0)
        bnd = R.gamma(K + 2) * (A + np.abs(add) + 1)
        _ratio(mode + ' pieces', R.check_bound(y, ref, bnd, f'{mode} GEMM rpg={rpg} eye_k={eye_k}'))


# ----------------------------------------------------------------------------------------------------------- range guard
def test_gemm_f16x3_status_bits():
    rng = np.random.default_rng(9)
    M, N, K = 384, 64, 128                      # three 128-row tiles, two 64-column K chunks
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    wp = _pack(w, 'f16x3')

    def status(x, pre=0):
        st = torch.full((1,), pre, dtype=torch.int32, device='cuda:0')
        _gemm('f16x3', _dev(x), K, wp, N, status=st)
        return int(st.item())
    healthy = rng.standard_normal((M, K)).astype(np.float32)
    assert status(healthy) == 0
    # one wave's share of the staged 128-row tile all zero (rows r with r % 16 in [4w, 4w+4), the dead post-ReLU case): not flagged
    x = healthy.copy()
    r = np.arange(M)
    x[(r % 16 >= 4) & (r % 16 < 8)] = 0
    assert status(x) == 0
    # the whole middle tile below 2^-6 over the whole K: UNDERFLOW; one entry at 2^-6 in its second K chunk: not
    x = healthy.copy()
    x[128:256] *= np.float32(2.0 ** -6 / 8)
    x[128:256] = np.clip(x[128:256], -2.0 ** -6 * 0.99, 2.0 ** -6 * 0.99)
    assert status(x) == 2
    x[200, 100] = 2.0 ** -6
    assert status(x) == 0
    # a single element >= 65504: OVERFLOW
    x = healthy.copy()
    x[300, 5] = 65504.0
    assert status(x) == 1
    x[300, 5] = 65503.0                         # below HALF_MAX: clean (its hi piece rounds to 65504, still finite)
    assert status(x) == 0
    # bits already set by the caller survive
    assert status(healthy, pre=4) == 4
    x = healthy.copy()
    x[0, 0] = 1e6
    assert status(x, pre=2) == 3


# --------------------------------------------------------------------------------------------------------------- PointMLP
def _int_params(rng, B, N, mid, with_t3):
    """Small-integer front layers: every value up to the 128 -> 1024 layer's input is an integer below 2^15 (some above 2048, so the
    f16 lo pieces of the activations are non-zero), computed exactly in every mode; w3 / b3 are full-precision floats."""
    f = lambda a: np.asarray(a, np.float32)
    P = {'x': f(rng.integers(-3, 4, (B, N, 6))),
         't3': f(rng.integers(-2, 3, (B, 9))) if with_t3 else None,
         'w1': f(rng.integers(-9, 10, (64, 6))), 'b1': f(rng.integers(-8, 9, 64)),
         'wm': f(rng.choice([-1, 0, 0, 1], (64, 64))), 'bm': f(rng.integers(-8, 9, 64)),
         't64': f(rng.choice([-1, 0, 0, 1], (B, 64, 64))),
         'w2': f(rng.choice([-3, -2, -1, 0, 0, 0, 1, 2, 3], (128, 64))), 'b2': f(rng.integers(-64, 65, 128)),
         'w3': f(rng.standard_normal((1024, 128)) / np.sqrt(128)), 'b3': f(rng.standard_normal(1024))}
    return P


def _h2_exact(P, mid, b):
    """the 128 -> 1024 layer's input of sample b, (N, 128), exact (int64 arithmetic)"""
    x = P['x'][b].astype(np.int64)
    q = x.copy()
    if P['t3'] is not None:
        q[:, :3] = x[:, :3] @ P['t3'][b].astype(np.int64).reshape(3, 3)
    h = np.maximum(q @ P['w1'].astype(np.int64).T + P['b1'].astype(np.int64), 0)
    if mid == 1:
        h = np.maximum(h @ P['wm'].astype(np.int64).T + P['bm'].astype(np.int64), 0)
    elif mid == 2:
        h = h @ P['t64'][b].astype(np.int64).T
    h2 = np.maximum(h @ P['w2'].astype(np.int64).T + P['b2'].astype(np.int64), 0)
    assert np.abs(h2).max() < 2 ** 15
    return h2.astype(np.float32), h


def _run_pointmlp(P, mode, mid, relu3, nsplit=1, pointfeat=False, status=None, B=None):
    B = P['x'].shape[0] if B is None else B
    dev = 'cuda:0'
    if mode == 'f32':
        pk = lambda w: _dev(folding.pack_b(w))
    else:
        pk = lambda w: _dev(folding.pack_b_split(w, R.ELEM[mode]).view(np.int16))
    w3 = _dev(folding.pack_b_f16fp8x2(P['w3'])) if mode == 'f16fp8x2' else pk(P['w3'])
    kw = dict(t3=_dev(P['t3'][:B]) if P['t3'] is not None else None, mid_mode=mid, nsplit=nsplit, pointfeat=pointfeat)
    if mid == 1:
        kw.update(wm=pk(P['wm']), bm=_dev(P['bm']))
    if mid == 2:
        kw.update(t64=_dev(P['t64'][:B]))
    if mode != 'f32':
        kw.update(split=SPLIT[mode])
        if mode != 'bf16x3':
            kw.update(status=status)
    r = ops.pointmlp_max(_dev(P['x'][:B]), _dev(P['w1']), _dev(P['b1']), pk(P['w2']), _dev(P['b2']), w3, _dev(P['b3']), relu3, **kw)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in r) if pointfeat else r.cpu().numpy()


def _f32_branch(B, N, nsplit):
    """cg_pointmlp_max's launcher: (nsplit in force, tail balancing?, CS)"""
    ntiles = (N + 63) // 64
    ns = min(max(nsplit, 1), ntiles)
    slots = 2 * _cu()
    tail = ns == 1 and ntiles >= 8 and B >= slots and B % slots != 0
    n_main = B - B % slots if tail else B
    wgs = n_main * ns + (B - n_main) * 8
    cs = 1 if tail else 8 if wgs <= 64 else 4 if wgs <= 128 else 2 if wgs <= 256 else 1
    return ns, tail, cs


_REF_CACHE = {}
_CH = np.array(sorted(set(range(0, 1024, 32)) | set(range(31, 1024, 32)) | {100, 333, 517, 700, 901}))   # channels emulated bitwise


def _f32_emulated(P, key, mid, b, relu3):
    """bitwise emulation of sample b's (1024,) output of cg_pointmlp_max on the exact-front inputs"""
    k = (key, mid, b, relu3)
    if k not in _REF_CACHE:
        h2, _ = _h2_exact(P, mid, b)
        acc = R.fma_chain(h2, P['w3'][_CH])             # (N, channels): the L3 stream, k-step order from a zero accumulator
        v = (acc.max(axis=0) + P['b3'][_CH]).astype(np.float32)
        _REF_CACHE[k] = np.maximum(v, np.float32(0)) if relu3 else v
    return _REF_CACHE[k]


_F32_P = {}


def _f32_params(N, mid, with_t3=True):
    if (N, mid) not in _F32_P:
        _F32_P[(N, mid)] = _int_params(np.random.default_rng(N * 3 + mid), 520, N, mid, with_t3)
    return _F32_P[(N, mid)]


F32_MATRIX = [(N, ns, lvl) for N in (1, 63, 64, 65, 511, 512, 2049) for ns in (1, 2, 3, 7, 64) for lvl in ('few', 'many')]


@pytest.mark.parametrize('N,nsplit,level', F32_MATRIX, ids=[f'N{n}-ns{s}-{l}' for n, s, l in F32_MATRIX])
def test_pointmlp_f32_bitwise(N, nsplit, level):
    """few: B = 1 (CS = 8, the channel-split C++ path); many: B * nsplit > 256 workgroups (CS = 1, the hand-scheduled asm stream)"""
    ntiles = (N + 63) // 64
    ns_eff = min(nsplit, ntiles)
    B = 1 if level == 'few' else 257 // ns_eff + 1
    mid = N % 3
    ns, tail, cs = _f32_branch(B, N, nsplit)
    assert not tail and cs == (8 if level == 'few' else 1), (ns, tail, cs)
    P = _f32_params(N, mid)
    out = _run_pointmlp(P, 'f32', mid, True, nsplit=nsplit, B=B)
    for b in sorted(set([0, B - 1])):
        R.check_bitwise(out[b, _CH], _f32_emulated(P, N, mid, b, True), f'cg_pointmlp_max N={N} nsplit={nsplit} (in force {ns}, CS {cs}, '
                                                                     f'uneven {ntiles % ns != 0}) sample {b}')


@pytest.mark.parametrize('B_', ['40', '100', '200', '2cu+5'], ids=['cs8', 'cs4', 'cs2', 'tail-cs1'])
def test_pointmlp_f32_cs_levels_and_tail(B_):
    N = 512
    B = 2 * _cu() + 5 if B_ == '2cu+5' else int(B_)
    ns, tail, cs = _f32_branch(B, N, 1)
    assert cs == {'40': 8, '100': 4, '200': 2, '2cu+5': 1}[B_] and tail == (B_ == '2cu+5')
    P = _f32_params(N, 1)
    out = _run_pointmlp(P, 'f32', 1, True, B=B)
    check = list(range(B - 5, B)) + [0, B // 3] if tail else [0, B // 2, B - 1]
    for b in check:
        R.check_bitwise(out[b, _CH], _f32_emulated(P, N, 1, b, True), f'cg_pointmlp_max B={B} (tail {tail}, CS {cs}) sample {b}')


@pytest.mark.parametrize('mode', ['f32', 'bf16x3', 'f16x3', 'f16fp8x2'])
def test_pointmlp_negative_max_channels(mode):
    """relu3 off, b3 pushed negative and some w3 rows all negative (every point's value of those channels < 0), nsplit > 1: the
    -inf pre-fill and the negative branch of atomic_max_f32 decide the result"""
    rng = np.random.default_rng(77)
    N = 700
    P = _int_params(rng, 3, N, 0, False)
    P['w3'][::7] = -np.abs(P['w3'][::7])
    P['b3'] = (P['b3'] - 50).astype(np.float32)
    out = _run_pointmlp(P, mode, 0, False, nsplit=3)
    for b in range(3):
        h2, _ = _h2_exact(P, 0, b)
        if mode == 'f32':
            acc = R.fma_chain(h2, P['w3'][::7])
            R.check_bitwise(out[b, ::7], (acc.max(axis=0) + P['b3'][::7]).astype(np.float32), 'negative channels, f32')
            assert (out[b, ::7] < 0).all()
        S, A = R.piece_sum(h2, P['w3'], mode) if mode != 'f32' else (h2.astype(np.float64) @ P['w3'].T.astype(np.float64),
                                                                    np.abs(h2.astype(np.float64)) @ np.abs(P['w3'].T.astype(np.float64)))
        ref, bnd = _l3_bound(S, A, P['b3'])
        _ratio(mode + ' pieces', R.check_bound(out[b], ref, bnd, f'{mode} negative channels sample {b}'))


SPLIT_MATRIX = [(mode, N) for mode in ('bf16x3', 'f16x3', 'f16fp8x2') for N in (1, 255, 256, 257, 1000)]


@pytest.mark.parametrize('mode,N', SPLIT_MATRIX, ids=[f'{m}-N{n}' for m, n in SPLIT_MATRIX])
def test_pointmlp_split_l3_vs_pieces(mode, N):
    """front layers exact -> the 128 -> 1024 stream in isolation: within gamma_128 of the exact piece products (max over points)"""
    _split_l3_case(mode, N, 3, 1)


@pytest.mark.parametrize('mode', ['bf16x3', 'f16x3', 'f16fp8x2'])
def test_pointmlp_split_tail(mode):
    B = _cu() + 3
    _split_l3_case(mode, 600, B, 1, tail=True)


def _l3_bound(S, A, b3):
    """the 128 -> 1024 layer on an exact input: per-point sums S (N, 1024) within gamma_128 A; max over points; + b3 (one rounding)"""
    m, e = S.max(axis=0), R.gamma(128) * A.max(axis=0)
    b3 = b3.astype(np.float64)
    return m + b3, e + R.gamma(1) * (np.abs(m) + e + np.abs(b3))


def _split_l3_case(mode, N, B, nsplit, tail=False):
    ntiles = (N + 255) // 256
    is_tail = nsplit == 1 and ntiles > 1 and B >= _cu() and B % _cu() != 0
    assert is_tail == tail
    mid = N % 3
    P = _int_params(np.random.default_rng(N + 11), B, N, mid, True)
    st = torch.zeros(1, dtype=torch.int32, device='cuda:0')
    r = _run_pointmlp(P, mode, mid, True, nsplit=nsplit, status=st, pointfeat=(mid == 2))
    out = r[0] if mid == 2 else r
    if mode != 'bf16x3':
        assert int(st.item()) == 0, 'healthy integer data flagged by the range guard'
    check = list(range(B - 3, B)) + [0] if tail else range(B)
    big = 0
    for b in check:
        h2, hmid = _h2_exact(P, mid, b)
        big = max(big, int(h2.max()))
        if mid == 2:                            # the feature-transformed activation is exact in every mode
            R.check_bitwise(r[1][b], hmid.astype(np.float32), f'{mode} pointfeat sample {b}')
        ref, e = _l3_bound(*R.piece_sum(h2, P['w3'], mode), P['b3'])
        _ratio(mode + ' pieces', R.check_bound(out[b], np.maximum(ref, 0), e, f'{mode} N={N} sample {b} vs exact piece products'))
    assert big > 2048 or N < 64, 'the integer front should reach activations above 2048 (non-zero f16 lo pieces)'


GEN_MATRIX = [(mode, mid, relu3, t3) for mode in ('f32', 'bf16x3', 'f16x3', 'f16fp8x2') for mid in (0, 1, 2)
              for relu3, t3 in ((True, True), (False, False))]


@pytest.mark.parametrize('mode,mid,relu3,with_t3', GEN_MATRIX, ids=[f'{m}-mid{d}-relu{int(r)}-t3{int(t)}' for m, d, r, t in GEN_MATRIX])
def test_pointmlp_general_values_bound(mode, mid, relu3, with_t3):
    rng = np.random.default_rng(mid * 4 + relu3 * 2 + with_t3)
    B, N = 3, 300
    f = lambda a: np.asarray(a, np.float32)
    P = {'x': f(rng.standard_normal((B, N, 6))), 't3': f(np.eye(3).reshape(1, 9) + 0.3 * rng.standard_normal((B, 9))) if with_t3 else None,
         'w1': f(rng.standard_normal((64, 6)) / 2), 'b1': f(rng.standard_normal(64) * 0.5),
         'wm': f(rng.standard_normal((64, 64)) / 8), 'bm': f(rng.standard_normal(64) * 0.5),
         't64': f(np.eye(64)[None] + rng.standard_normal((B, 64, 64)) / 8),
         'w2': f(rng.standard_normal((128, 64)) / 8), 'b2': f(rng.standard_normal(128) * 0.5),
         'w3': f(rng.standard_normal((1024, 128)) / 11), 'b3': f(rng.standard_normal(1024) * 0.5)}
    st = torch.zeros(1, dtype=torch.int32, device='cuda:0')
    r = _run_pointmlp(P, mode, mid, relu3, nsplit=2, status=st, pointfeat=(mid == 2))
    out = r[0] if mid == 2 else r
    if mode in ('f16x3', 'f16fp8x2'):
        assert int(st.item()) == 0
    for b in range(B):
        ref = R.pointmlp_ref(P['x'][b], P, mode, mid, relu3, b)
        _ratio(mode, R.check_bound(out[b], ref['out'], ref['out_e'], f'{mode} mid {mid} sample {b}'))
        if mid == 2:
            _ratio(mode, R.check_bound(r[1][b], ref['pf'], ref['pf_e'], f'{mode} pointfeat sample {b}'))


@pytest.mark.parametrize('mode', ['f16x3', 'f16fp8x2'])
def test_pointmlp_status_bits(mode):
    rng = np.random.default_rng(3)
    N = 512                                     # two 256-point tiles; wave w of a tile carries points [32w, 32w+32)
    f = lambda a: np.asarray(a, np.float32)
    P = {'x': f(rng.standard_normal((2, N, 6))), 't3': None, 'w1': f(rng.standard_normal((64, 6)) / 2), 'b1': f(np.full(64, 0.5)),
         'w2': f(rng.standard_normal((128, 64)) / 8), 'b2': f(rng.standard_normal(128) * 0.5),
         'w3': f(rng.standard_normal((1024, 128)) / 11), 'b3': f(rng.standard_normal(1024))}

    def status(P, pre=0):
        st = torch.full((1,), pre, dtype=torch.int32, device='cuda:0')
        _run_pointmlp(P, mode, 0, True, status=st)
        return int(st.item())
    assert status(P) == 0
    # the first layer's output of ONE wave's 32 points below 2^-6 (inputs 0, b1 small): UNDERFLOW
    Q = dict(P, x=P['x'].copy(), b1=f(np.full(64, 2.0 ** -8)))
    Q['x'][1, 256 + 64:256 + 96] = 0
    Q['x'][1, :256 + 64] = 100.0                 # every other wave's points: outputs well above 2^-6
    Q['x'][1, 256 + 96:] = 100.0
    Q['x'][0] = 100.0
    assert status(Q) == 2
    Q['x'][1, 256 + 95] = 100.0                  # 31 of the 32: not flagged
    assert status(Q) == 0
    # a single input element >= 65504: OVERFLOW; caller's bits survive
    Q = dict(P, x=P['x'].copy())
    Q['x'][0, 17, 3] = 70000.0
    assert status(Q) & 1
    assert status(P, pre=8) == 8
    assert status(Q, pre=8) & 9 == 9


def test_report_ratios():
    """worst observed error / bound per mode over the module (run last; printed with -s)"""
    print('\nobserved error / bound:', {k: f'{v:.3g}' for k, v in sorted(RATIOS.items())})
