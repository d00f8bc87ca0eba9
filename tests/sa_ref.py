"""Host reference of the fused set-abstraction kernels (csrc/setabstraction.hip, csrc/sa_tile.hip) in plain numpy float64, and
the scenes tests/test_sa_kernels_gpu.py runs them on.  Proved on the CPU by tests/test_sa_ref_cpu.py.

The reference is the operation itself: gather rows by index, subtract the centre, concatenate [xyz | features], relu(x W^T + b)
per layer, max over the K rows.  It does not pack, pad or reorder: the [features | xyz | pad] column order of the tile kernel and
the pad to 16 of the register kernel are properties of the code under test.

Two kinds of scene:
  * exact scenes: coordinates k/8 on an 8^3 lattice, integer features, integer weights and biases, no BatchNorm.  Every product
    and every partial sum is a multiple of g = 2^-3; while sum |w x| + |b| stays below 2^24 g (exactness_margin < 1) every partial
    sum is a float32 number, so the float32 result is the same in every summation order, with or without FMA, with the bias first
    or last -- and equals the float64 evaluation.  The kernels are held to equality on them;
  * general scenes: random normal values with BatchNorm folded, held to the per-element bound of dense_ref.dense_bound composed
    layer by layer (sa_bound).

Neighbour lists are explicit index arrays: `random` (uniform) or `beacon` (every row of neighbourhood g is one base point, except
row g mod K: the base point's twin, whose raised beacon feature makes every output channel strictly larger -- over G >= K
neighbourhoods every row position carries the result alone once)."""
import numpy as np

import dense_ref as dr
from catgrasp_amd import folding

GRAN = 2.0 ** -3            # common granularity of the exact scenes' inputs


# ------------------------------------------------------------------------------------------------------------ reference
def grouped(xyz, points, new_xyz, idx):
    """-> (B, S, K, 3 + D) float64: [xyz[idx] - centre | points[idx]]; idx None: the group-all layer, one group of all N points,
    coordinates not centred."""
    xyz = np.asarray(xyz, np.float64)
    B = xyz.shape[0]
    if idx is None:
        g = xyz[:, None, :, :]
        f = None if points is None else np.asarray(points, np.float64)[:, None, :, :]
    else:
        idx = np.asarray(idx)
        bi = np.arange(B)[:, None, None]
        g = xyz[bi, idx] - np.asarray(new_xyz, np.float64)[:, :, None, :]
        f = None if points is None else np.asarray(points, np.float64)[bi, idx]
    return g if f is None else np.concatenate([g, f], axis=-1)


def sa_ref_rows(xyz, points, new_xyz, idx, layers):
    """-> (B, S, K, C) float64: the last layer's ReLU'd rows, before the max."""
    x = grouped(xyz, points, new_xyz, idx)
    for w, b in layers:
        x = np.maximum(x @ np.asarray(w, np.float64).T + np.asarray(b, np.float64), 0.0)
    return x


def sa_ref(xyz, points, new_xyz, idx, layers):
    """-> (B, S, C) float64.  layers: [(W (Cout, Cin), b (Cout)), ...], Cin of the first = 3 + D in the order [xyz | features]."""
    return sa_ref_rows(xyz, points, new_xyz, idx, layers).max(axis=2)


def exactness_margin(xyz, points, new_xyz, idx, layers, g=GRAN):
    """Largest (sum_k |w_k x_k| + |b|) / (2^24 g) over all layers, rows and outputs.  Below 1: every partial sum, in any order, is a
    multiple of g below 2^24 g, i.e. exact in float32 (and so is the centring subtraction).  Raises if an input is off the grid."""
    for t in (xyz, points, new_xyz) + tuple(a for l in layers for a in l):
        if t is not None:
            q = np.asarray(t, np.float64) / g
            assert np.array_equal(q, np.round(q)), 'input is not a multiple of the granularity'
    x = grouped(xyz, points, new_xyz, idx)
    m = float(np.abs(x).max()) if x.size else 0.0
    for w, b in layers:
        w = np.asarray(w, np.float64); b = np.asarray(b, np.float64)
        m = max(m, float((np.abs(x) @ np.abs(w).T + np.abs(b)).max()))
        x = np.maximum(x @ w.T + b, 0.0)
    return m / (2.0 ** 24 * g)


def sa_bound(xyz, points, new_xyz, idx, layers):
    """General values: (ref, bound), (B, S, C) float64, of a float32 kernel that accumulates each layer in float32 (any order) on
    float32 inputs and float32 folded weights: dense_ref.dense_bound per layer (mode f32, n_acc = cin + 1: the chain and the
    bias), input error = one rounding of the centred coordinate; ReLU and the max pass an absolute bound through."""
    x = grouped(np.asarray(xyz, np.float32), None if points is None else np.asarray(points, np.float32),
                None if new_xyz is None else np.asarray(new_xyz, np.float32), idx)
    B, S, K, _ = x.shape
    e = np.zeros_like(x)
    if idx is not None:
        e[..., :3] = dr.U32 * np.abs(x[..., :3])
    y, e = x.reshape(B * S * K, -1), e.reshape(B * S * K, -1)
    for w, b in layers:
        y, e = dr.relu(*dr.dense_bound(y, e, w, b, 'f32', w.shape[1] + 1))
    C = y.shape[1]
    return y.reshape(B, S, K, C).max(axis=2), e.reshape(B, S, K, C).max(axis=2)


# --------------------------------------------------------------------------------------------------------------- scenes
def beacon_value(D):
    """The beacon feature's raise: a power of two >= 4 D + 12, so that every first-layer unit of the twin is >= 2 D + 7 > 2 whatever
    the base point's sum (|.| <= 3 + 2 D + 2) and survives the next layer's bias."""
    return 1 << int(np.ceil(np.log2(4 * D + 12)))


def exact_scene(B, N, S, K, D, widths, lists='random', seed=0, density=1.0, group_all=False):
    """-> dict(xyz (B,N,3), points (B,N,D) | None, new_xyz (B,S,3), idx (B,S,K) int64, layers [(W, b)], raw [(W, b, None)]).
    Coordinates k/8, k in [0, 8); centres taken from the points; features in [-2, 2]; weights in {-1, 0, 1}, dense in layer 0 and
    kept with probability `density` in the deeper layers; biases in [-2, 2].  lists 'random': the last layer's bias is raised by
    the smallest integer that leaves >= 97 % of the outputs positive (ReLU hides little).  lists 'beacon' (D > 0, N even): points
    N/2.. are twins of points 0..N/2-1 with feature seed % D raised by beacon_value(D); layer 0's column of that feature is +1
    and the deeper layers' weights are in {0, 1} with at least one 1 per row, so the twin's outputs are strictly larger.
    group_all: S = 1, idx None (K = N)."""
    rng = np.random.default_rng(seed)
    xyz = rng.integers(0, 8, (B, N, 3)) / 8.0
    points = rng.integers(-2, 3, (B, N, D)).astype(np.float64) if D else None
    beacon = lists == 'beacon'
    if beacon:
        assert D > 0 and N % 2 == 0 and not group_all
        fb, h = seed % D, N // 2
        xyz[:, h:] = xyz[:, :h]
        points[:, h:] = points[:, :h]
        points[:, h:, fb] += beacon_value(D)
    if group_all:
        S, K, idx, new_xyz = 1, N, None, None
    else:
        cidx = rng.integers(0, N, (B, S))
        new_xyz = xyz[np.arange(B)[:, None], cidx]
        if beacon:
            base = rng.integers(0, N // 2, (B, S))
            idx = np.repeat(base[:, :, None], K, axis=2)
            g = np.arange(B * S).reshape(B, S)
            idx[np.arange(B)[:, None], np.arange(S)[None, :], g % K] += N // 2
        else:
            idx = rng.integers(0, N, (B, S, K))
        idx = idx.astype(np.int64)
    layers, cin = [], 3 + D
    for li, co in enumerate(widths):
        w = rng.integers(-1, 2, (co, cin)).astype(np.float64)
        if li > 0:
            if beacon:
                w = (rng.random((co, cin)) < 0.25).astype(np.float64)
                w[np.arange(co), np.arange(co) % cin] = 1.0
            elif density < 1.0:
                w *= rng.random((co, cin)) < density
        elif beacon:
            w[:, 3 + fb] = 1.0
        layers.append((w, rng.integers(-2, 3, co).astype(np.float64)))
        cin = co
    if not beacon:
        x = grouped(xyz, points, new_xyz, idx)
        for w, b in layers[:-1]:
            x = np.maximum(x @ w.T + b, 0.0)
        w, b = layers[-1]
        pre = (x @ w.T + b).max(axis=2).ravel()
        low = np.partition(pre, int(0.03 * pre.size))[int(0.03 * pre.size)]
        if low <= 0:
            layers[-1] = (w, b + (np.floor(-low) + 1.0))
    return dict(xyz=xyz, points=points, new_xyz=new_xyz, idx=idx, layers=layers, raw=[(w, b, None) for w, b in layers])


def general_scene(B, N, S, K, D, widths, seed=0, group_all=False):
    """Random normal features and weights with BatchNorm: -> dict like exact_scene's, arrays float32; `raw` holds (w, b, bn) for
    SetAbstractionWeights, `layers` the folded weights rounded to float32 (what the kernels multiply by), `folded64` the folded
    weights before that rounding."""
    rng = np.random.default_rng(seed)
    xyz = (rng.random((B, N, 3)) * 0.4).astype(np.float32)
    points = (rng.normal(size=(B, N, D)) * 0.5).astype(np.float32) if D else None
    if group_all:
        idx, new_xyz = None, None
    else:
        new_xyz = xyz[np.arange(B)[:, None], rng.integers(0, N, (B, S))]
        idx = rng.integers(0, N, (B, S, K)).astype(np.int64)
    raw, layers, folded64, cin = [], [], [], 3 + D
    for co in widths:
        w = rng.normal(0, 1.0 / np.sqrt(cin), (co, cin)); b = rng.normal(0, 0.1, co)
        bn = (rng.uniform(0.5, 1.5, co), rng.normal(0, 0.1, co), rng.normal(0, 0.1, co), rng.uniform(0.5, 1.5, co))
        wf, bf = folding.fold_bn(w, b, bn)
        raw.append((w, b, bn)); folded64.append((wf, bf)); layers.append((wf.astype(np.float32), bf.astype(np.float32)))
        cin = co
    return dict(xyz=xyz, points=points, new_xyz=new_xyz, idx=idx, layers=layers, raw=raw, folded64=folded64)
