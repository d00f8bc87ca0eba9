"""ctypes binding of libcatgrasp_amd.so (the C ABI declared in include/catgrasp_amd.h).

The HIP library is the product: there is no CPU fallback.  `lib()` raises if the shared object
is missing or does not export every declared symbol; every wrapper raises on a non-zero status.

The header is the one statement of every prototype: `lib()` sets `argtypes` and `restype` of every entry point from it, so
call sites pass plain Python numbers and ctypes converts -- and refuses -- them per parameter: a missing argument is a
TypeError; a float for an integer, a list for a pointer or a ctypes scalar of another type than declared is a
ctypes.ArgumentError; a count >= 2**31 for a `long` arrives intact.  Every pointer parameter is a c_void_p: it takes `_p(tensor)`,
None, an address, `byref(struct)` and ctypes arrays.  Two things ctypes does NOT catch: extra trailing arguments are passed
through, and a `str` is accepted for a pointer.

The clustering entry points have a header of their own, include/catgrasp_amd_cluster.h (same library): `signatures()` and
`declared_symbols()` describe the main header, `cluster_signatures()` the other.  The sparse convolution layers have a third,
include/catgrasp_amd_sparse.h, described by `sparse_signatures()`, and the assembled PointGroup network a fourth,
include/catgrasp_amd_pointgroup.h, described by `pointgroup_signatures()`, and the scene front end (depth image -> point normals) a
fifth, include/catgrasp_amd_scene.h, described by `scene_signatures()`, and the grid index (neighbour queries and normals of any cloud)
a sixth, include/catgrasp_amd_neighbors.h, described by `neighbors_signatures()`, and the k-d tree searches on that index (unbounded
nearest neighbour, ball lists) a seventh, include/catgrasp_amd_kdtree.h, described by `kdtree_signatures()`, and the gradients of the
sparse convolution layers an eighth, include/catgrasp_amd_sparse_grad.h, described by `sparse_grad_signatures()`, and BatchNorm in
batch-statistics mode with ReLU (forward and backward) a ninth, include/catgrasp_amd_bn.h, described by `bn_signatures()`, and the
screened form of the fused per-point pass a tenth, include/catgrasp_amd_screen.h, described by `screen_signatures()`, and the NUNOCS
training loss (forward and backward) an eleventh, include/catgrasp_amd_loss.h, described by `loss_signatures()`.  The gradients of the
dense per-row layers (weight, bias, input, per-group column sums) and BatchNorm + ReLU at the widths of PointNetSeg's head have a
twelfth, which lives inside the package, catgrasp_amd/include/catgrasp_amd_dense.h, described by `dense_signatures()`, and the closed-form
training of PointNet's conv + BatchNorm + max-pool layer a thirteenth, next to it, catgrasp_amd/include/catgrasp_amd_pool.h, described by
`pool_signatures()`.  `lib()` binds and requires all thirteen.
"""
import ctypes
import os
import re

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('CATGRASP_AMD_LIB', os.path.join(_PKG, 'libcatgrasp_amd.so'))   # override: dev ablation builds only
HEADER_PATH = os.path.join(_PKG, '..', 'include', 'catgrasp_amd.h')
CLUSTER_HEADER_PATH = os.path.join(_PKG, '..', 'include', 'catgrasp_amd_cluster.h')   # the clustering entry points: their own header
SPARSE_HEADER_PATH = os.path.join(_PKG, '..', 'include', 'catgrasp_amd_sparse.h')     # the sparse convolution layers: likewise
POINTGROUP_HEADER_PATH = os.path.join(_PKG, '..', 'include', 'catgrasp_amd_pointgroup.h')   # the assembled PointGroup network: likewise
SCENE_HEADER_PATH = os.path.join(_PKG, '..', 'include', 'catgrasp_amd_scene.h')     # the scene front end: likewise
NEIGHBORS_HEADER_PATH = os.path.join(_PKG, '..', 'include', 'catgrasp_amd_neighbors.h')   # the grid index: likewise
KDTREE_HEADER_PATH = os.path.join(_PKG, '..', 'include', 'catgrasp_amd_kdtree.h')   # the k-d tree searches on the grid index: likewise
SPARSE_GRAD_HEADER_PATH = os.path.join(_PKG, '..', 'include', 'catgrasp_amd_sparse_grad.h')   # the sparse layers' gradients: likewise
BN_HEADER_PATH = os.path.join(_PKG, '..', 'include', 'catgrasp_amd_bn.h')   # batch-statistics BatchNorm + ReLU: likewise
SCREEN_HEADER_PATH = os.path.join(_PKG, '..', 'include', 'catgrasp_amd_screen.h')   # the screened per-point pass: likewise
LOSS_HEADER_PATH = os.path.join(_PKG, '..', 'include', 'catgrasp_amd_loss.h')   # the NUNOCS training loss: likewise
DENSE_HEADER_PATH = os.path.join(_PKG, 'include', 'catgrasp_amd_dense.h')   # the dense layers' gradients: likewise, inside the package
POOL_HEADER_PATH = os.path.join(_PKG, 'include', 'catgrasp_amd_pool.h')   # the pooled layer's closed-form training: likewise
_lib = None

_SCALARS = {'int': ctypes.c_int, 'long': ctypes.c_long, 'float': ctypes.c_float, 'double': ctypes.c_double,
            'unsigned long long': ctypes.c_ulonglong, 'size_t': ctypes.c_size_t}
_PROTOTYPE = re.compile(r'([\w\s*]+?)\b(cg_[a-z0-9_]+)\s*\(([^()]*)\)\s*;')


class CatgraspAmdError(RuntimeError):
    pass


def _ctype(decl, what, ret=False):
    t = ' '.join(decl.replace('*', ' * ').split())
    c = ctypes.c_char_p if ret and t == 'const char *' else ctypes.c_void_p if '*' in t else _SCALARS.get(t)
    if c is None:
        raise CatgraspAmdError(f'include/catgrasp_amd.h: {what} has type {t!r}, which the binding does not map')
    return c


def signatures(src=None):
    """{name: (restype, argtypes)} of every function declared in include/catgrasp_amd.h (or in the header text `src`).  A parser for
    THIS header, not for C: comments, preprocessor lines and `typedef struct {...}` blocks are dropped, the rest must be prototypes
    of scalars and pointers inside the `extern "C"` braces; anything else raises."""
    if src is None:
        with open(HEADER_PATH) as f:
            src = f.read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    src = re.sub(r'^\s*#.*$', '', src, flags=re.M)
    src = re.sub(r'\btypedef\s+struct\b[^{}]*\{[^{}]*\}[^;]*;', '', src)
    sigs = {}
    for ret, name, params in _PROTOTYPE.findall(src):
        params = [] if params.strip() == 'void' else [p.strip() for p in params.split(',')]
        sigs[name] = (_ctype(ret, f'the return value of {name}', ret=True),
                      tuple(_ctype(re.sub(r'\w+$', '', p), f'parameter {p!r} of {name}') for p in params))
    rest = _PROTOTYPE.sub('', src).replace('extern "C" {', '', 1).replace('}', '', 1).strip()
    if rest:
        raise CatgraspAmdError(f'include/catgrasp_amd.h: the binding cannot parse {rest[:200]!r}')
    return sigs


def declared_symbols():
    """Names of every function declared in include/catgrasp_amd.h."""
    return sorted(signatures())


def cluster_signatures():
    """signatures() of include/catgrasp_amd_cluster.h: same parser, same type mapping."""
    with open(CLUSTER_HEADER_PATH) as f:
        return signatures(f.read())


def sparse_signatures():
    """signatures() of include/catgrasp_amd_sparse.h: same parser, same type mapping."""
    with open(SPARSE_HEADER_PATH) as f:
        return signatures(f.read())


def pointgroup_signatures():
    """signatures() of include/catgrasp_amd_pointgroup.h: same parser, same type mapping."""
    with open(POINTGROUP_HEADER_PATH) as f:
        return signatures(f.read())


def scene_signatures():
    """signatures() of include/catgrasp_amd_scene.h: same parser, same type mapping."""
    with open(SCENE_HEADER_PATH) as f:
        return signatures(f.read())


def neighbors_signatures():
    """signatures() of include/catgrasp_amd_neighbors.h: same parser, same type mapping."""
    with open(NEIGHBORS_HEADER_PATH) as f:
        return signatures(f.read())


def kdtree_signatures():
    """signatures() of include/catgrasp_amd_kdtree.h: same parser, same type mapping."""
    with open(KDTREE_HEADER_PATH) as f:
        return signatures(f.read())


def sparse_grad_signatures():
    """signatures() of include/catgrasp_amd_sparse_grad.h: same parser, same type mapping."""
    with open(SPARSE_GRAD_HEADER_PATH) as f:
        return signatures(f.read())


def bn_signatures():
    """signatures() of include/catgrasp_amd_bn.h: same parser, same type mapping."""
    with open(BN_HEADER_PATH) as f:
        return signatures(f.read())


def screen_signatures():
    """signatures() of include/catgrasp_amd_screen.h: same parser, same type mapping."""
    with open(SCREEN_HEADER_PATH) as f:
        return signatures(f.read())


def loss_signatures():
    """signatures() of include/catgrasp_amd_loss.h: same parser, same type mapping."""
    with open(LOSS_HEADER_PATH) as f:
        return signatures(f.read())


def dense_signatures():
    """signatures() of catgrasp_amd/include/catgrasp_amd_dense.h: same parser, same type mapping."""
    with open(DENSE_HEADER_PATH) as f:
        return signatures(f.read())


def pool_signatures():
    """signatures() of catgrasp_amd/include/catgrasp_amd_pool.h: same parser, same type mapping."""
    with open(POOL_HEADER_PATH) as f:
        return signatures(f.read())


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CatgraspAmdError(
                f'{LIB_PATH} not found: build it with `python -m catgrasp_amd.build` '
                '(hipcc --offload-arch=gfx950).  There is no CPU fallback.')
        l = ctypes.CDLL(LIB_PATH)
        sigs = {**signatures(), **cluster_signatures(), **sparse_signatures(), **pointgroup_signatures(), **scene_signatures(),
                **neighbors_signatures(), **kdtree_signatures(), **sparse_grad_signatures(), **bn_signatures(), **screen_signatures(),
                **loss_signatures(), **dense_signatures(), **pool_signatures()}
        missing = [s for s in sorted(sigs) if not hasattr(l, s)]
        if missing:
            raise CatgraspAmdError(f'libcatgrasp_amd.so lacks symbols {missing}; rebuild it')
        for name, (restype, argtypes) in sigs.items():
            fn = getattr(l, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = l
    return _lib


def _p(t):
    """Device pointer of a tensor (None -> NULL)."""
    if t is None:
        return ctypes.c_void_p(0)
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    """hipStream_t of torch's current stream on the current device.  torch.cuda.current_stream() builds a Stream object through four
    layers of python (8 us under a profiler, per launch -- a tenth of a 16-candidate predict_batch call); the raw handle is what
    torch's own compiled backends fetch."""
    try:
        return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()))
    except AttributeError:          # a torch build without the private accessor: the public (slower) route
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def check(status, what):
    if status != 0:
        raise CatgraspAmdError(f'{what} failed with status {status}')


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise CatgraspAmdError('catgrasp_amd kernels need CUDA/HIP device tensors (no CPU fallback)')


def f32c(t):
    assert t.dtype == torch.float32 and t.is_contiguous(), (t.dtype, t.is_contiguous())
    return t


def i32c(t):
    assert t.dtype == torch.int32 and t.is_contiguous()
    return t
