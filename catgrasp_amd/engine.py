"""Device forward passes of PointNetCls / PointNetSeg assembled from the HIP kernels.

Call graph per PointNetCls.forward (pointnet2.py:289-299), B samples of N points:
  pass A  cg_pointmlp_max(mid 0)          STN3d conv1..3 + max                 (B,1024)
          3x cg_gemm_bias_act             STN3d fc1,fc2,fc3 + I3               (B,9)
  pass B  cg_pointmlp_max(mid 1, t3)      enc.conv1 -> STNkd conv1..3 + max    (B,1024)
          3x cg_gemm_bias_act             STNkd fc1,fc2,fc3 + I64              (B,4096)
  pass C  cg_pointmlp_max(mid 2, t3,t64)  enc.conv1, .T64, conv2, conv3, max   (B,1024)
          3x cg_gemm_bias_act             fc1,fc2,fc3                          (B,n_out)
The sequence is written once (encoder_forward) for every arithmetic mode; what a mode changes about a launch -- kernel, weight
images, tile geometry, range status -- is decided in _point_pass for the fused passes and in _dense for the GEMMs.
"""
import os
import threading

from . import ops

# Arithmetic of the wide dense layers (inputs, outputs, accumulators and everything outside them are float32 in every mode):
# 'f32'   : exact-f32 MFMA kernels (bitwise an fmaf chain per dot product) -- the reference's arithmetic and the DEFAULT.  On an
#           MI355X it scores 82k candidates/s end to end (0.93 of the f32 matrix peak), above the 50k target of BASELINE.json.
# 'f16x3' : opt-in fast mode.  Split-half MFMA kernels (x = hi + lo IEEE-half pieces, 3 f16 MFMAs per product block, f32 accumulate)
#           for every wide layer: logits within ~2e-6 of the float64 evaluation -- float32's own distance -- at 3.2x the f32 rate.  Half
#           has a narrow exponent range: the kernels report range excursions per call and the engine re-runs such batches with bf16
#           pieces (run_guarded), so a valid checkpoint never fails.
# 'f16fp8x2': opt-in, the fastest mode: 'f16x3' everywhere except the 128 -> 1024 per-point layers (91 % of the matrix work), whose two
#           correction terms run on the block-scaled e4m3 matrix instruction (x_hi8.w_lo8 + x_lo8.w_hi8, one power-of-two scale per 32
#           channels) -- 2 instead of 3 units of matrix time per product block.  Logits within ~5e-5 of the float64 evaluation (the bar is
#           1e-4); same range guard and bf16x3 re-run as 'f16x3'.
# 'bf16x3': the same with bf16 pieces (8 + 8 bits; ~2e-5): float32's exponent range, per-point layers + segmentation head only.
# For scale: the reference's own GPU path runs its Conv1d layers through cuDNN, where TF32 (10-bit mantissa) is PyTorch's default
# on Ampere and later.
MODES = ('f32', 'bf16x3', 'f16x3', 'f16fp8x2')
_default = os.environ.get('CATGRASP_AMD_PRECISION', 'f32')      # process-wide default (set_precision)
if _default not in MODES:
    raise ValueError(f'CATGRASP_AMD_PRECISION={_default!r}: expected one of {MODES}')
_tls = threading.local()                                        # per-thread override stack of the `precision` context manager
TILE_POINTS = 256   # bf16x3 kernel geometry: points per workgroup tile (8 waves, one workgroup per CU)


def current_precision():
    """The arithmetic in force on THIS thread: the innermost `with precision(...)` of the thread, else the process default.  The
    override is thread-local, so two predicters used from two threads (or the range guard's bf16x3 re-run on one of them) cannot
    switch each other's arithmetic; `engine.PRECISION` reads the same value."""
    stack = getattr(_tls, 'stack', None)
    return stack[-1] if stack else _default


def __getattr__(name):          # engine.PRECISION stays readable as an attribute (bench.py, tests)
    if name == 'PRECISION':
        return current_precision()
    raise AttributeError(name)


def set_precision(p):
    """Set the process-wide default arithmetic (threads inside a `with precision(...)` block keep their override)."""
    global _default
    assert p in MODES, p
    _default = p


HALF_OVERFLOW, HALF_UNDERFLOW = 1, 2        # CG_STATUS_HALF_* bits of include/catgrasp_amd.h
HALF_MODES = ('f16x3', 'f16fp8x2')         # modes built on IEEE-half pieces: range-guarded, re-run under bf16x3 when the guard trips
_warned = set()


def new_status(device, n=1):
    """Caller-owned status words for the f16x3 kernels (zeroed int32 device tensor, one word per guarded batch)."""
    import torch
    return torch.zeros((n,), dtype=torch.int32, device=device)


def _warn_once(key, msg):
    if key not in _warned:
        _warned.add(key)
        import warnings
        warnings.warn(msg, RuntimeWarning, stacklevel=3)


def warn_range(bits):
    _warn_once(('range', bits), f'catgrasp_amd: f16x3 range guard tripped (bits={bits}: 1 = a value >= 65504, 2 = a layer output '
                                'below 2^-6); re-evaluating the affected batches with bf16x3 pieces')


class precision:
    """Context manager: run a block of THIS thread under another arithmetic (thread-local; see current_precision)."""

    def __init__(self, p):
        assert p in MODES, p
        self.p = p

    def __enter__(self):
        if not hasattr(_tls, 'stack'):
            _tls.stack = []
        _tls.stack.append(self.p)

    def __exit__(self, *exc):
        _tls.stack.pop()


def run_guarded(forward, W, x):
    """forward(W, x, status) under the active arithmetic.  Under 'f16x3' the half kernels report values that left the half range
    (or layer outputs that sank into the half subnormals) in a per-call status word; such a batch is evaluated again with bf16
    pieces -- float32's exponent range, ~2e-5 instead of ~2e-6 logits error, still inside the 1e-4 bar -- so a valid checkpoint
    never raises and never returns range-damaged numbers.  Costs one 4-byte read-back per call."""
    if current_precision() not in HALF_MODES:
        return forward(W, x, None)
    st = new_status(x.device)
    out = forward(W, x, st)
    bits = int(st.item())
    if bits:
        warn_range(bits)
        with precision('bf16x3'):
            out = forward(W, x, None)
    return out


def run_guarded_features(forward, W, x):
    """run_guarded for the standalone building blocks (STN3d, PointNetEncoder), whose OUTPUT is the raw 1024-wide feature / the
    transform itself rather than logits behind FC layers and a softmax.  The 2-unit mode's e4m3 correction terms reach ~1e-4 of the
    feature scale there (measured 1.1e-4 on tests/test_predicter_gpu.py's encoder case) -- the mode is specified on the nets' logits --
    so under 'f16fp8x2' these blocks run 'f16x3'."""
    if current_precision() == 'f16fp8x2':
        with precision('f16x3'):
            return run_guarded(forward, W, x)
    return run_guarded(forward, W, x)


def _nsplit(B, N, tp=64):
    """Workgroups per sample: keep >= ~1024 workgroups in flight for small batches."""
    ntiles = (N + tp - 1) // tp
    if B >= 1024:
        return 1
    return max(1, min(ntiles, (1024 + B - 1) // B))


def _dense(W, name, x, n_out, bias, status=None, **kw):
    """One folded Linear/Conv1d(k=1) layer on the GEMM kernel of the active arithmetic.  'f16x3': every wide layer has a half
    image (FC tails and segmentation head; the 9- and 10-wide output layers stay exact f32).  'bf16x3': only the per-point
    segmentation head -- measured, splitting the per-candidate FC tails with bf16 pieces buys 3 % of the step and raises the
    logits error from ~2e-5 to ~6e-5 of the 1e-4 bar."""
    if current_precision() in HALF_MODES and W.half_ok.get(name + '.h', False):       # a layer whose weights do not fit the half pieces stays f32
        return ops.gemm_bias_act(x, W[name + '.h'], n_out, bias, split='f16', status=status, **kw)
    if current_precision() == 'bf16x3' and (name + '.s') in W:
        return ops.gemm_bias_act(x, W[name + '.s'], n_out, bias, split='bf16', **kw)
    return ops.gemm_bias_act(x, W[name], n_out, bias, **kw)


def pad_points(x, cin):
    """x (B,N,cin), cin = 3..6 -> (B,N,6): the fused passes read 6 floats per point; missing feature channels are zeros that meet
    zero weight columns (folding._pad_first_layer), i.e. they add exactly +0."""
    import torch
    if x.shape[2] != cin:
        raise ValueError(f'the model takes {cin} input channels, the tensor has {x.shape[2]}')
    if cin == 6:
        return x
    return torch.cat([x, x.new_zeros((x.shape[0], x.shape[1], 6 - cin))], dim=2).contiguous()


def _identity_t64(B, device):
    """The feature transform of an encoder built WITHOUT one (pointnet2.py:229,254-259: feature_transform=False, the reference
    default): pass <2> multiplies by the identity -- exact in f32 (x*1 + 0 + ...), to split precision in the split modes."""
    import torch
    return torch.eye(64, dtype=torch.float32, device=device).reshape(1, 4096).repeat(B, 1).contiguous()


def _point_pass(W, x, w1, tag, relu3, status, mid=None, **kw):
    """One fused per-point pass (first layer `w1`, the 64 -> 128 -> 1024 layers of `tag`, optionally the 64 -> 64 layer `mid` in
    between, max over the points) on the kernel of the active arithmetic -- the ONE place that turns the mode into weight images,
    kernel, tile geometry and range-status forwarding.  'f32': the packed f32 images on 64-point tiles.  Split modes: 256-point
    tiles and the bf16 ('.s') images, or -- under the half-based modes, when EVERY image of the pass fits the half pieces
    (folding.put_half) -- the IEEE-half ('.h') ones, which report range excursions in `status`; under 'f16fp8x2' the 128 -> 1024
    layer of such a pass takes its e4m3 ('.q') image."""
    B, N, _ = x.shape
    mode = current_precision()
    names = [tag + '.w2', tag + '.w3'] + ([mid] if mid else [])
    if mode == 'f32':
        sfx = q = ''
        kw.update(nsplit=_nsplit(B, N))
    else:
        half = mode in HALF_MODES and all(W.half_ok.get(n + '.h', False) for n in names)
        sfx = '.h' if half else '.s'
        q = '.q' if half and mode == 'f16fp8x2' else sfx
        kw.update(nsplit=_nsplit(B, N, TILE_POINTS), tile_points=TILE_POINTS, split={'.s': 'bf16', '.h': 'f16', '.q': 'f16fp8'}[q],
                  status=status if half else None)
    if mid:
        kw.update(wm=W[mid + sfx], bm=W[mid[:-3] + '.bm'])
    return ops.pointmlp_max(x, W[w1 + '.w1'], W[w1 + '.b1'], W[tag + '.w2' + sfx], W[tag + '.b2'], W[tag + '.w3' + q], W[tag + '.b3'], relu3, **kw)


def _tnet_tail(W, tag, g, k, status):
    """The FC tail of an STN3d (k = 3) / STNkd (k = 64) on the pooled feature g (B,1024) -> (B,k*k) transform + I_k."""
    h = _dense(W, tag + '.fc1', g, 512, W[tag + '.fc1b'], relu=True, status=status)
    h = _dense(W, tag + '.fc2', h, 256, W[tag + '.fc2b'], relu=True, status=status)
    return _dense(W, tag + '.fc3', h, k * k, W[tag + '.fc3b'], eye_k=k, status=status)


def encoder_forward(W, x, want_pointfeat=False, status=None):
    """x:(B,N,6) cuda f32 -> global feature (B,1024), trans (B,9), trans_feat TRANSPOSED (B,4096) [, pointfeat].
    For an encoder without a feature transform (W.has_fstn False) trans_feat is None and pass B is skipped."""
    t3 = stn3d_forward(W, x, status)
    t64 = None
    if getattr(W, 'has_fstn', True):
        g = _point_pass(W, x, 'enc', 'fstn', True, status, mid='fstn.wm', t3=t3, mid_mode=1)
        t64 = _tnet_tail(W, 'fstn', g, 64, status)
    r = _point_pass(W, x, 'enc', 'enc', False, status, t3=t3, mid_mode=2, t64=t64 if t64 is not None else _identity_t64(x.shape[0], x.device),
                    pointfeat=want_pointfeat)
    return (r[0], t3, t64, r[1]) if want_pointfeat else (r, t3, t64)


def stn3d_forward(W, x, status=None):
    """A standalone STN3d (pointnet2.py:170-185), and pass A of the encoder.  x:(B,N,6) -> (B,9) row-major 3x3."""
    return _tnet_tail(W, 'stn', _point_pass(W, x, 'stn', 'stn', True, status), 3, status)


def stnkd_forward(W, x):
    """A free-standing STNkd(k) (pointnet2.py:189-223) on x (B,N,k): conv1..3 as row-batched GEMMs over the B*N points (exact f32 in
    every mode: this module is not on the scoring path), max over each cloud's points (cg_group_max), the FC tail + I_k.  The
    (B*N,1024) activation is materialised -- cloud batches are processed in slices of <= 2^18 points to bound it at 1 GB.
    -> (B, k*k) row-major."""
    import torch
    B, N, k = x.shape
    if k != W.k:
        raise ValueError(f'STNkd({W.k}) got a {k}-channel tensor')
    if W.k_pad != k:
        x = torch.cat([x, x.new_zeros((B, N, W.k_pad - k))], dim=2)
    x = x.contiguous()
    step = max(1, (1 << 18) // max(N, 1))
    g = torch.empty((B, 1024), dtype=torch.float32, device=x.device)
    for s in range(0, B, step):
        e = min(B, s + step)
        h = ops.gemm_bias_act(x[s:e].reshape(-1, W.k_pad), W['c1'], 64, W['c1b'], relu=True)
        h = ops.gemm_bias_act(h, W['c2'], 128, W['c2b'], relu=True)
        h = ops.gemm_bias_act(h, W['c3'], 1024, W['c3b'], relu=True)
        g[s:e] = ops.group_max(h, e - s)
    h = ops.gemm_bias_act(g, W['fc1'], 512, W['fc1b'], relu=True)
    h = ops.gemm_bias_act(h, W['fc2'], 256, W['fc2b'], relu=True)
    return ops.gemm_bias_act(h, W['fc3'], k * k, W['fc3b'], eye_k=k)


def encoder_module_forward(W, x, global_feat, status=None):
    """A standalone PointNetEncoder(feature_transform=True).forward (pointnet2.py:240-271) with the module's return layout.
    x:(B,N,6) -> (global (B,1024) | cat([global repeated, pointfeat]) (B,1088,N), trans (B,3,3), trans_feat (B,64,64))."""
    import torch
    B, N, _ = x.shape
    r = encoder_forward(W, x, want_pointfeat=not global_feat, status=status)
    g, t3, t64 = r[0], r[1], r[2]
    trans, trans_feat = t3.view(B, 3, 3), (t64.view(B, 64, 64).transpose(1, 2) if t64 is not None else None)
    if global_feat:
        return g, trans, trans_feat
    return torch.cat([g.view(B, 1024, 1).expand(-1, -1, N), r[3].transpose(1, 2)], 1), trans, trans_feat


FUSED_LAUNCH_MAX_B = 1024      # batches up to this size issue the exact-f32 PointNetCls forward as ONE C call (cg_pointnet_cls_forward)


import ctypes as _ctypes


class _ClsWeightsC(_ctypes.Structure):
    """cg_cls_weights (include/catgrasp_amd.h): device pointers to the folded, packed f32 weights, field order as declared there."""
    _NAMES = ('stn.w1', 'stn.b1', 'stn.w2', 'stn.b2', 'stn.w3', 'stn.b3', 'stn.fc1', 'stn.fc1b', 'stn.fc2', 'stn.fc2b', 'stn.fc3', 'stn.fc3b',
              'enc.w1', 'enc.b1', 'fstn.wm', 'fstn.bm', 'fstn.w2', 'fstn.b2', 'fstn.w3', 'fstn.b3',
              'fstn.fc1', 'fstn.fc1b', 'fstn.fc2', 'fstn.fc2b', 'fstn.fc3', 'fstn.fc3b', 'enc.w2', 'enc.b2', 'enc.w3', 'enc.b3',
              'head.fc1', 'head.fc1b', 'head.fc2', 'head.fc2b', 'head.fc3', 'head.fc3b')
    _fields_ = [(n.replace('.', '_'), _ctypes.c_void_p) for n in _NAMES] + [('n_out', _ctypes.c_int)]


def _cls_forward_one_call(W, x):
    """cls_forward for a small batch: the twelve launches issued from C in one call (csrc/forward.hip) -- what the python chain below
    issues one ctypes call at a time; bit-identical results, ~0.1 ms less interpreter per forward."""
    import ctypes
    import torch
    from . import _lib as L
    ops.require_cuda(x); ops.f32c(x)
    B, N, D = x.shape
    assert D == 6
    ptrs = tuple(W[n].data_ptr() for n in _ClsWeightsC._NAMES)
    cached = getattr(W, '_cls_c', None)
    if cached is None or cached[0] != ptrs:       # keyed on the tensors' addresses: a re-folded / reloaded weight is picked up
        cw = _ClsWeightsC()
        for n, ptr in zip(_ClsWeightsC._NAMES, ptrs):
            t = W[n]
            assert t.dtype == torch.float32 and t.is_cuda, n
            setattr(cw, n.replace('.', '_'), ptr)
        cw.n_out = int(W.n_out)
        W._cls_c = cached = (ptrs, cw)
    cw = cached[1]
    lib = L.lib()
    ws = torch.empty((lib.cg_pointnet_cls_workspace_floats(B),), dtype=torch.float32, device=x.device)
    logits = torch.empty((B, W.n_out), dtype=torch.float32, device=x.device)
    tf = ctypes.c_void_p(0)
    L.check(lib.cg_pointnet_cls_forward(L._p(x), B, N, ctypes.byref(cw), _nsplit(B, N), L._p(ws), L._p(logits),
                                        ctypes.byref(tf), L._stream()), 'cg_pointnet_cls_forward')
    off = (tf.value - ws.data_ptr()) // 4
    t64 = ws[off:off + B * 4096]
    return logits, t64.view(B, 64, 64).transpose(1, 2)      # the FC kernel emits the transform transposed


def cls_forward(W, x, status=None):
    """PointNetCls.forward in eval mode.  x:(B,N,6) -> logits (B,n_out), trans_feat (B,64,64).
    status: optional device int32 word collecting the f16x3 range bits of this batch (see run_guarded)."""
    B = x.shape[0]
    if 0 < B <= FUSED_LAUNCH_MAX_B and current_precision() == 'f32' and getattr(W, 'has_fstn', True) and ops.KERNEL_TIMER is None:
        return _cls_forward_one_call(W, x)
    g, t3, t64 = encoder_forward(W, x, status=status)
    h = _dense(W, 'head.fc1', g, 512, W['head.fc1b'], relu=True, status=status)
    h = _dense(W, 'head.fc2', h, 256, W['head.fc2b'], relu=True, status=status)
    logits = _dense(W, 'head.fc3', h, W.n_out, W['head.fc3b'], status=status)
    return logits, t64.view(B, 64, 64).transpose(1, 2)      # the FC kernel emits the transform transposed


def seg_forward(W, x, status=None):
    """PointNetSeg.forward in eval mode.  x:(B,N,6) -> (B,N,n_out), trans_feat (B,64,64)."""
    B, N, _ = x.shape
    g, t3, t64, pf = encoder_forward(W, x, want_pointfeat=True, status=status)
    # conv1 over cat([global(1024) repeated, pointfeat(64)]) = Wg.g (per cloud) + Wp.pointfeat (per point)
    gb = _dense(W, 'seg.c1g', g, 512, W['seg.c1b'], status=status)
    h = _dense(W, 'seg.c1p', pf.view(B * N, 64), 512, None, relu=True, row_bias=gb, rows_per_group=N, status=status)
    h = _dense(W, 'seg.c2', h, 256, W['seg.c2b'], relu=True, status=status)
    h = _dense(W, 'seg.c3', h, 128, W['seg.c3b'], relu=True, status=status)
    y = _dense(W, 'seg.c4', h, W.n_out, W['seg.c4b'], status=status)
    return y.view(B, N, W.n_out), t64.view(B, 64, 64).transpose(1, 2)


class _EngineModule(type(os)):
    """`engine.PRECISION = ...` used to be how older scripts switched arithmetic; it would now create a real attribute that shadows the
    module __getattr__ above while the kernels keep dispatching on current_precision().  Refuse it instead of ignoring it."""

    def __setattr__(self, name, value):
        if name == 'PRECISION':
            raise AttributeError("engine.PRECISION is read-only: use engine.set_precision(mode) or `with engine.precision(mode):`")
        super().__setattr__(name, value)


import sys as _sys          # noqa: E402
_sys.modules[__name__].__class__ = _EngineModule
