"""Host references of the dense kernels (cg_gemm_bias_act*, cg_pointmlp_max*) in float64, with rigorous error bounds.

Used by tests/test_dense_kernels_gpu.py and proved on the CPU by tests/test_dense_ref_cpu.py.

Three kinds of reference:
  * exact-f32 kernels: a bitwise emulation of the k-ordered fmaf chain that v_mfma_f32_32x32x2_f32 evaluates
    (D = fma(a_k1, b_k1, fma(a_k0, b_k0, C)), one rounding per product), in the k order the packing fixes;
  * split kernels on inputs known exactly: the float64 sum of the exact piece products, within gamma_K * sum |piece products|;
  * any kernel on general values: the float64 evaluation of the layer chain, with a bound propagated layer by layer.

Rounding model of the bounds (u = 2^-24, float32's unit roundoff; gamma_n = n u / (1 - n u)):
  * an accumulation of n terms into a float32 accumulator errs by at most gamma_n * sum |terms| (any order, any tree).  The
    16-bit MFMAs sum 16 exact products per instruction, 3 instructions per 16-deep block; n = K (+ the bias) covers up to
    K / (3K/16) > 5 roundings per instruction, and the f32 MFMA chain does exactly K;
  * a float32 add / the t3 product's three terms: gamma of the number of roundings, on the magnitudes;
  * ReLU and max are 1-Lipschitz: they pass an absolute bound through unchanged.
"""
import numpy as np
import torch

from catgrasp_amd import folding

U32 = 2.0 ** -24


def gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U32 / (1.0 - n * U32)


# ----------------------------------------------------------------------------------------------------------------- fmaf
def fmaf(a, b, c):
    """Correctly rounded float32 fma(a, b, c), elementwise with broadcasting (Python has no math.fma before 3.13).

    a*b is exact in float64 (24 + 24 bits).  s = fl64(a*b + c) carries a TwoSum error err.  Rounding s to float32 equals rounding
    the exact sum s + err except when s lands exactly on a float32 midpoint (every float32 midpoint is a double, so the exact sum
    cannot cross one without landing on it); then the exact sum lies on the side of err, and that neighbour is taken."""
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    b = np.asarray(b, dtype=np.float32).astype(np.float64)
    c = np.asarray(c, dtype=np.float32).astype(np.float64)
    with np.errstate(all='ignore'):
        p = a * b
        s = p + c
        bv = s - p
        err = (p - (s - bv)) + (c - bv)
        r = s.astype(np.float32)
        rd = r.astype(np.float64)
        r2 = np.nextafter(r, np.where(s > rd, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
        mid = (rd != s) & ((rd + r2.astype(np.float64)) * 0.5 == s) & (err != 0) & np.isfinite(s)
        if not mid.any():
            return r
        fix = np.where(err > 0, np.maximum(r, r2), np.minimum(r, r2))
        return np.where(mid, fix, r).astype(np.float32)


def chain_order(K):
    """k order of one output element of the exact-f32 MFMA kernels: B fragment Wp[nb][ks][lane][j] = W[..][8 ks + 4 (lane>>5) + j]
    (folding.pack_b), and MFMA j of k-step ks takes k0 = 8 ks + j (lanes 0..31) then k1 = 8 ks + 4 + j (lanes 32..63)."""
    assert K % 8 == 0, K
    return [8 * s + 4 * h + j for s in range(K // 8) for j in range(4) for h in range(2)]


def fma_chain(x, w, order=None):
    """x (M, K), w (N, K) float32 -> (M, N) float32: acc = 0; for k in order: acc = fmaf(x[:, k], w[:, k], acc)."""
    x = np.asarray(x, dtype=np.float32)
    w = np.asarray(w, dtype=np.float32)
    acc = np.zeros((x.shape[0], w.shape[0]), dtype=np.float32)
    for k in (chain_order(x.shape[1]) if order is None else order):
        acc = fmaf(x[:, k, None], w[None, :, k], acc)
    return acc


def gemm_f32_epilogue(acc, cols, rows, bias=None, eye_k=0, row_bias=None, rows_per_group=1, relu=False):
    """gemm.hip's epilogue in float32 on the accumulators acc (len(rows), len(cols)): (+1 folded into the bias of the eye columns
    first) + bias, + row_bias[row // rows_per_group], ReLU."""
    cols = np.asarray(cols)
    rows = np.asarray(rows)
    b = np.zeros(len(cols), np.float32) if bias is None else np.asarray(bias, np.float32)[cols].copy()
    if eye_k > 0:
        b = np.where(cols % (eye_k + 1) == 0, b + np.float32(1), b).astype(np.float32)
    v = (acc + b[None, :]).astype(np.float32)
    if row_bias is not None:
        v = (v + np.asarray(row_bias, np.float32)[(rows // rows_per_group)[:, None], cols[None, :]]).astype(np.float32)
    if relu:
        v = np.maximum(v, np.float32(0))
    return v


# --------------------------------------------------------------------------------------------------------- split pieces
ELEM = {'bf16x3': 'bf16', 'f16x3': 'f16', 'f16fp8x2': 'f16'}
PIECE_U = {'bf16': 2.0 ** -8, 'f16': 2.0 ** -11}          # unit roundoff of one 16-bit piece
PIECE_FLOOR = {'bf16': 2.0 ** -134, 'f16': 2.0 ** -25}    # half the smallest subnormal: the absolute error floor of a piece


def split16(v, elem):
    """float32 array -> (hi, lo) float64 values of its 16-bit pieces, by the host statement of the kernels' rule
    (folding.bf16_split / folding.f16_split: hi = rne(v), lo = rne(v - hi))."""
    v = np.asarray(v, dtype=np.float32)
    if elem == 'bf16':
        h, l = folding.bf16_split(v)
        f = lambda t: (t.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
        return f(h), f(l)
    with np.errstate(over='ignore'):
        h, l = folding.f16_split(v)
    return h.view(np.float16).astype(np.float64), l.view(np.float16).astype(np.float64)


def e4m3(v):
    """float64 / float32 array -> float64 values of its OCP e4m3 image, round to nearest even (torch's float8_e4m3fn cast)."""
    return torch.from_numpy(np.asarray(v, dtype=np.float32)).to(torch.float8_e4m3fn).to(torch.float64).numpy()


def mx_pieces(v, deq_shift=(0, 0)):
    """v (..., K) float32, K % 32 == 0 -> (half(v), hi8, lo8) float64: the f16fp8x2 pieces of folding.pack_b_f16fp8x2 (weights) and
    pointmlp_split.hip (activations), one MX unit = 32 consecutive k: e = frexp exponent of the unit's largest |v| (clamped to
    [-100, 100]); hi8 = e4m3(v / 2^(e-8)) 2^(e-8), lo8 = e4m3((v - half(v)) / 2^(e-19)) 2^(e-19).
    deq_shift: exponents added to the two scales at dequantisation only (a planted wrong scale byte, for the CPU proof)."""
    v = np.asarray(v, dtype=np.float32)
    shp = v.shape
    blk = v.reshape(*shp[:-1], shp[-1] // 32, 32)
    e = np.clip(np.frexp(np.abs(blk).max(axis=-1, keepdims=True))[1], -100, 100).astype(np.float64)
    with np.errstate(over='ignore'):
        h = blk.astype(np.float16).astype(np.float32)
    s_hi, s_lo = np.exp2(e - 8), np.exp2(e - 19)
    hi8 = e4m3(blk / s_hi) * s_hi * 2.0 ** deq_shift[0]
    lo8 = e4m3((blk - h) / s_lo) * s_lo * 2.0 ** deq_shift[1]
    return h.astype(np.float64).reshape(shp), hi8.reshape(shp), lo8.reshape(shp)


def pieces(x, w, mode):
    """The piece products of x (M, K) . w (N, K)^T the kernel of `mode` forms, each exact in float64:
    bf16x3 / f16x3: x_lo w_hi + x_hi w_lo + x_hi w_hi;  f16fp8x2: half(x) half(w) + x_hi8 w_lo8 + x_lo8 w_hi8.
    -> list of (x piece, w piece) pairs."""
    if mode == 'f16fp8x2':
        xh, xh8, xl8 = mx_pieces(x)
        wh, wh8, wl8 = mx_pieces(w)
        return [(xh, wh), (xh8, wl8), (xl8, wh8)]
    xh, xl = split16(x, ELEM[mode])
    wh, wl = split16(w, ELEM[mode])
    return [(xl, wh), (xh, wl), (xh, wh)]


def piece_sum(x, w, mode, drop=None):
    """-> (S, A): float64 sum of the exact piece products and sum of their magnitudes, (M, N).
    drop: optional (pair index, k slice) removed from S (a planted defect for the CPU proof)."""
    S = 0.0
    A = 0.0
    for i, (a, b) in enumerate(pieces(x, w, mode)):
        if drop is not None and drop[0] == i:
            keep = np.ones(a.shape[1], bool)
            keep[drop[1]] = False
            S = S + (a * keep) @ b.T
        else:
            S = S + a @ b.T
        A = A + np.abs(a) @ np.abs(b).T
    return S, A


# --------------------------------------------------------------------------------------------------- propagated bounds
def _piece_err(xmag, wmag, elem):
    """(|x - hi|, |x - hi - lo|) bounds of a value of magnitude <= xmag split into 16-bit pieces: |x - hi| <= u|x| + F (F: the
    subnormal floor), and lo = rne(x - hi) errs by <= u |x - hi| + F."""
    u, F = PIECE_U[elem], PIECE_FLOOR[elem]
    r = u * xmag + F
    return r + (u * r + F), u * r + F          # |x_lo| <= |x - hi| + |delta|, |delta|


def split_term(xmag, w, mode, xblock=None):
    """Bound, (M, N), on |x.w - sum of the kernel's piece products| for inputs of magnitude <= xmag (M, K) and weights w (N, K).

    bf16x3 / f16x3, with x = x_hi + x_lo + dx, w = w_hi + w_lo + dw (dx, dw: the rounding error of the lo pieces):
        x w - (x_lo w_hi + x_hi w_lo + x_hi w_hi) = x_lo w_lo + dw (x - dx) + dx w
    f16fp8x2 (the 128 -> 1024 layer), with r = v - half(v) and e8(.) the e4m3 rounding errors of the hi8 / lo8 images:
        x w - pieces = -r_x r_w - x e8(r_w) - e8(x) w_lo8 - r_x e8(w) - e8(r_x) w_hi8
    where |e8(t)| <= 2^-4 |t| + 2^-10 s (s the unit's scale 2^(e-8) / 2^(e-19), e the frexp exponent of the unit's largest
    magnitude, so s_hi <= 2^-7 m and s_lo <= 2^-18 m for a unit maximum m; xblock: bound on x's unit maxima, (M, K))."""
    w = np.asarray(w, dtype=np.float32)
    if mode == 'f32':
        return 0.0
    if mode == 'f16fp8x2':
        wh, wh8, wl8 = mx_pieces(w)
        w64 = w.astype(np.float64)
        rw = np.abs(w64 - wh)
        mw = np.repeat(np.abs(w64).reshape(w.shape[0], -1, 32).max(axis=-1), 32, axis=-1)
        e8w = 2.0 ** -4 * np.abs(w64) + 2.0 ** -10 * 2.0 ** -7 * mw
        e8rw = 2.0 ** -4 * rw + 2.0 ** -10 * 2.0 ** -18 * mw
        mx = xmag if xblock is None else xblock
        rx = 2.0 ** -11 * xmag + 2.0 ** -25
        e8x = 2.0 ** -4 * xmag + 2.0 ** -10 * 2.0 ** -7 * mx
        e8rx = 2.0 ** -4 * rx + 2.0 ** -10 * 2.0 ** -18 * mx
        return (rx @ rw.T + xmag @ e8rw.T + e8x @ np.abs(wl8).T + rx @ e8w.T + e8rx @ np.abs(wh8).T)
    elem = ELEM[mode]
    wh, wl = split16(w, elem)
    dw = np.abs(w.astype(np.float64) - wh - wl)
    xlo, dx = _piece_err(xmag, None, elem)
    return xlo @ np.abs(wl).T + (xmag + dx) @ dw.T + dx @ np.abs(w.astype(np.float64)).T


def dense_bound(y_in, e_in, w, bias, mode, n_acc, bias_split=False, xblock=None):
    """One dense layer y = W h + b on the reference input y_in (M, K) float64 whose kernel value errs by <= e_in (M, K):
        |y^ - y| <= |W| e_in + gamma_n (|W| |h^| + |b|) + split_term(mode) [+ the bias's own split error]
    with |h^| <= |y_in| + e_in.  n_acc: roundings of the accumulation (K for the chains, + 1 for a bias added after it).
    The bias enters the accumulation (as its initial value, or one float32 add after it: counted in n_acc); bias_split: it is split
    into pieces first (the split kernels' first layer, where b1 rides as the k = 6 column against a constant-1 input).
    -> (y (M, N), bound (M, N)) in float64."""
    w64 = np.asarray(w, dtype=np.float32).astype(np.float64)
    aw = np.abs(w64)
    y = y_in @ w64.T
    hmag = np.abs(y_in) + e_in
    e = e_in @ aw.T + split_term(hmag, w, mode, xblock)
    mag = hmag @ aw.T
    if bias is not None:
        b = np.asarray(bias, dtype=np.float32).astype(np.float64)
        y = y + b[None, :]
        mag = mag + np.abs(b)[None, :]
        if bias_split and mode != 'f32':
            bh, bl = split16(np.asarray(bias, np.float32), ELEM[mode])
            e = e + np.abs(b - bh - bl)[None, :]
    return y, e + gamma(n_acc) * mag


def relu(y, e):
    return np.maximum(y, 0.0), e


def unit_max(v):
    """(M, K) -> (M, K): every entry replaced by the maximum of its 32-wide unit (the MX scale's argument)."""
    M, K = v.shape
    return np.repeat(v.reshape(M, K // 32, 32).max(axis=-1), 32, axis=-1)


# ------------------------------------------------------------------------------------------------------ PointMLP chains
def pointmlp_ref(x, P, mode, mid, relu3, b):
    """Sample b of cg_pointmlp_max* on general values: float64 reference and propagated bound of every stage.
    x (N, 6); P: float32 parameters w1 (64,6) b1 wm (64,64) bm t64 (B,64,64) [weight layout: t64[b][n][k] = T[k][n]] w2 (128,64)
    b2 w3 (1024,128) b3 t3 (B,9) or None.  -> dict: 'out' / 'out_e' (1024,), 'pf' / 'pf_e' (N, 64) for mid 2."""
    x = np.asarray(x, np.float32).astype(np.float64)
    N = x.shape[0]
    q = x.copy()
    eq = np.zeros_like(q)
    if P.get('t3') is not None:
        T = np.asarray(P['t3'][b], np.float32).astype(np.float64).reshape(3, 3)         # q_j = sum_i p_i T[i][j]
        q[:, :3] = x[:, :3] @ T
        eq[:, :3] = gamma(3) * (np.abs(x[:, :3]) @ np.abs(T))
    # L0 6 -> 64: f32: fmaf chain from b1 (6 roundings); split: one 16-deep block with b1 as the k = 6 column (its pieces' error)
    front = 'f16x3' if mode == 'f16fp8x2' else mode          # f16fp8x2 runs the front layers as f16x3
    h, e = dense_bound(q, eq, P['w1'], P['b1'], front, 6 if mode == 'f32' else 16, bias_split=True)
    h, e = relu(h, e)
    r = {}
    if mid == 1:
        h, e = relu(*dense_bound(h, e, P['wm'], P['bm'], front, 65))
    elif mid == 2:
        h, e = dense_bound(h, e, P['t64'][b], None, front, 64)
        r['pf'], r['pf_e'] = h, e
    h, e = relu(*dense_bound(h, e, P['w2'], P['b2'], front, 65))
    xblock = unit_max(np.abs(h) + e) if mode == 'f16fp8x2' else None
    y, ey = dense_bound(h, e, P['w3'], None, mode, 128, xblock=xblock)
    m, em = y.max(axis=0), ey.max(axis=0)
    b3 = np.asarray(P['b3'], np.float32).astype(np.float64)
    out = m + b3
    e_out = em + gamma(1) * (np.abs(m) + em + np.abs(b3))
    if relu3:
        out, e_out = relu(out, e_out)
    r['out'], r['out_e'] = out, e_out
    return r


def check_bound(got, ref, bound, what):
    """|got - ref| <= bound elementwise; -> worst observed / bound ratio (a failure names the worst element)."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref)
    bad = ~(err <= bound)
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, err / np.maximum(bound, 1e-300), -1)), err.shape)
        raise AssertionError(f'{what}: {int(bad.sum())} of {err.size} elements outside the bound; worst at {i}: got {got[i]!r}, '
                             f'ref {ref[i]!r}, err {err[i]:.3e} > bound {bound[i]:.3e}')
    return float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0


def check_bitwise(got, ref, what):
    got = np.asarray(got, np.float32)
    ref = np.asarray(ref, np.float32)
    same = got.view(np.uint32) == ref.view(np.uint32)
    if not same.all():
        i = np.unravel_index(np.argmin(same), same.shape)
        raise AssertionError(f'{what}: {int((~same).sum())} of {same.size} elements differ in their bits; first at {i}: '
                             f'got {got[i]!r}, emulated {ref[i]!r}')
