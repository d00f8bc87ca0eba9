"""The part of `spconv` that the reference's PointGroup network uses (PointGroup/model/pointgroup/pointgroup.py), on HIP:
SparseConvTensor, SparseModule, SparseSequential, SubMConv3d, SparseConv3d (kernel 2, stride 2) and SparseInverseConv3d.

    import catgrasp_amd.spconv as spconv

Inference only, float32, device tensors only: there is no CPU implementation and no autograd.  Every layer is one launch of the fused
gather-GEMM kernel (csrc/sparse_conv.hip) over an output-stationary rule book `nbr (n_out, K) int32` (csrc/sparse_rules.hip):

  SubMConv3d            k = 3, padding 1: K = 27, outputs = the input sites in the input's row order.  k = 1: a plain matrix product
                        (K = 1, every row reads itself).
  SparseConv3d          kernel 2, stride 2, padding 0: K = 8.  out_shape = (s - 2)//2 + 1 per axis; an input site with a coordinate
                        >= 2*out_shape (the last one of an odd axis) feeds no output; the output sites are the distinct [batch, d//2]
                        of the others, in ascending order of their linear key.
  SparseInverseConv3d   kernel 2, the `indice_key` of its SparseConv3d: K = 8, outputs = that layer's input sites in their order;
                        site x reads its parent x//2 through weight[x % 2]; a site the strided layer dropped gets the bias only.

Weights keep spconv's layout (k0, k1, k2, Cin, Cout) and state_dict keys `weight`, `bias`.  The operation is correlation: the output
at o reads, through kernel offset kk, the input at o*stride - padding + kk; absent neighbours contribute nothing.

Layers that share an `indice_key` share one rule book (stored in the tensor's `indice_dict`).  A SparseSequential in eval mode runs
`BatchNorm1d, ReLU, conv` as the conv's prologue max(x*scale + shift, 0) on the gathered rows; the conv layers also take an
optional `residual` that is added to the output rows in the same launch.

The prologue's max is C's fmaxf, which returns 0 for a NaN: a NaN feature (or a NaN in scale or shift) enters a folded
`BatchNorm1d, ReLU, conv` as 0, where torch.relu in the unfolded sequence would hand it on.  Without a prologue a NaN feature makes
every column of the rows that read its site NaN, and no other row.
"""
import math
from collections import OrderedDict, namedtuple

import torch
from torch import nn

from . import _lib as L
from ._lib import _p, _stream, check

MAX_CIN, MAX_COUT = 224, 112
_NO_KEY = 2 ** 63 - 1
_ERR_RANGE, _ERR_DUPLICATE = 1, 2

# One rule book.  `nbr` serves the layer that built it; a strided layer's book also serves its inverse layer, whose own table
# `inverse_nbr` is built from `out_keys` on first use.
RuleBook = namedtuple('RuleBook', 'out_indices in_indices nbr in_spatial_shape out_spatial_shape kind extra')


class SparseConvTensor(object):
    """features (N, C) float32, indices (N, 4) int32 rows [batch, d0, d1, d2], spatial_shape (three ints), batch_size."""

    def __init__(self, features, indices, spatial_shape, batch_size, grid=None):
        if features.dim() != 2 or indices.dim() != 2 or indices.shape[1] != 4:
            raise ValueError(f'features {tuple(features.shape)} must be (N, C) and indices {tuple(indices.shape)} (N, 4)')
        if features.shape[0] != indices.shape[0]:
            raise ValueError(f'features has {features.shape[0]} rows, indices {indices.shape[0]}')
        spatial_shape = [int(s) for s in spatial_shape]
        if len(spatial_shape) != 3 or min(spatial_shape) < 1 or int(batch_size) < 1:
            raise ValueError(f'spatial_shape {spatial_shape} must be three positive ints and batch_size {batch_size} positive')
        self.features = features
        self.indices = indices if indices.dtype == torch.int32 else indices.int()
        self.spatial_shape = spatial_shape
        self.batch_size = int(batch_size)
        self.indice_dict = {}
        self.grid = grid

    @property
    def spatial_size(self):
        return math.prod(self.spatial_shape)

    @property
    def sparity(self):
        return self.indices.shape[0] / self.spatial_size / self.batch_size

    def find_indice_pair(self, key):
        return None if key is None else self.indice_dict.get(key)

    def replace_feature(self, features, indices=None, spatial_shape=None):
        """This tensor's bookkeeping with other features: the result shares `indice_dict` (so the rule books below are found, not
        rebuilt) and `grid`.  Same sites unless `indices` and `spatial_shape` are given (a layer whose output sites differ)."""
        res = SparseConvTensor(features, self.indices if indices is None else indices,
                               self.spatial_shape if spatial_shape is None else spatial_shape, self.batch_size, self.grid)
        res.indice_dict = self.indice_dict
        return res

    def dense(self, channels_first=True):
        """(batch, C, s0, s1, s2), zeros at inactive sites ((batch, s0, s1, s2, C) if not channels_first)."""
        out = torch.zeros([self.batch_size] + self.spatial_shape + [self.features.shape[1]], dtype=self.features.dtype,
                          device=self.features.device)
        b, d0, d1, d2 = self.indices.long().unbind(1)
        out[b, d0, d1, d2] = self.features
        return out.permute(0, 4, 1, 2, 3).contiguous() if channels_first else out


class SparseModule(nn.Module):
    """Marks modules that take a SparseConvTensor inside a SparseSequential; any other module is applied to `.features`."""
    pass


def _device_features(x, *params):
    if not isinstance(x, SparseConvTensor):
        raise TypeError(f'expected a SparseConvTensor, got {type(x).__name__}')
    if not torch.cuda.is_available() or not x.features.is_cuda or not x.indices.is_cuda:
        raise L.CatgraspAmdError('catgrasp_amd.spconv needs HIP device tensors (there is no CPU fallback)')
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x.features,) + params):
        raise NotImplementedError('catgrasp_amd.spconv is inference only: call it under torch.no_grad()')
    if x.features.dtype != torch.float32:
        raise NotImplementedError(f'catgrasp_amd.spconv is float32 only, got {x.features.dtype}')
    if x.features.shape[0] != x.indices.shape[0]:
        raise ValueError(f'features has {x.features.shape[0]} rows, indices {x.indices.shape[0]}')
    return x.features.detach().contiguous()


def _raise_flag(err, what):
    flag = int(err.item())
    if flag & _ERR_RANGE:
        raise ValueError(f'{what}: a coordinate outside [0, spatial_shape) or a batch index outside [0, batch_size)')
    if flag & _ERR_DUPLICATE:
        raise ValueError(f'{what}: a site is listed twice')


def _sorted_keys(indices, spatial_shape, batch_size, err):
    """Ascending linear keys of the rows and the row of each (the range check reads the flag, so it is known before the lookups)."""
    n = indices.shape[0]
    keys = torch.empty((n,), dtype=torch.int64, device=indices.device)
    check(L.lib().cg_sparse_keys(_p(indices), n, batch_size, *spatial_shape, 0, _p(keys), _p(err), _stream()), 'cg_sparse_keys')
    _raise_flag(err, 'sparse tensor')
    return torch.sort(keys, stable=True)


def identity_rules(n, device):
    """Rule book of a K = 1 layer (SubMConv3d(k=1), nn.Linear as a layer): nbr (n, 1), every row reads itself."""
    return torch.arange(n, dtype=torch.int32, device=device).view(n, 1)


def subm_rules(indices, spatial_shape, batch_size):
    """Rule book of SubMConv3d(k=3, padding=1): nbr (N, 27)."""
    indices = indices.contiguous()
    n, dev = indices.shape[0], indices.device
    err = torch.zeros((1,), dtype=torch.int32, device=dev)
    sk, perm = _sorted_keys(indices, spatial_shape, batch_size, err)
    nbr = torch.empty((n, 27), dtype=torch.int32, device=dev)
    check(L.lib().cg_sparse_rules_subm(_p(indices), _p(sk), _p(perm), n, *spatial_shape, _p(nbr), _p(err), _stream()), 'cg_sparse_rules_subm')
    _raise_flag(err, 'sparse tensor')
    return RuleBook(indices, indices, nbr, list(spatial_shape), list(spatial_shape), 'subm', {})


def down_rules(indices, spatial_shape, batch_size):
    """Rule book of SparseConv3d(kernel 2, stride 2): out_indices (M, 4) in key order, nbr (M, 8); extra['out_keys'] for the inverse."""
    if min(spatial_shape) < 2:
        raise ValueError(f'spatial_shape {spatial_shape} is smaller than the kernel')
    indices = indices.contiguous()
    n, dev = indices.shape[0], indices.device
    out_shape = [(s - 2) // 2 + 1 for s in spatial_shape]
    err = torch.zeros((1,), dtype=torch.int32, device=dev)
    sk, perm = _sorted_keys(indices, spatial_shape, batch_size, err)
    parent = torch.empty((n,), dtype=torch.int64, device=dev)
    check(L.lib().cg_sparse_keys(_p(indices), n, batch_size, *spatial_shape, 1, _p(parent), _p(err), _stream()), 'cg_sparse_keys')
    out_keys = torch.unique(parent)                      # ascending
    if out_keys.numel() and int(out_keys[-1].item()) == _NO_KEY:
        out_keys = out_keys[:-1]
    out_keys = out_keys.contiguous()
    m = out_keys.shape[0]
    out_indices = torch.empty((m, 4), dtype=torch.int32, device=dev)
    nbr = torch.empty((m, 8), dtype=torch.int32, device=dev)
    check(L.lib().cg_sparse_rules_down(_p(out_keys), m, _p(sk), _p(perm), n, *spatial_shape, _p(out_indices), _p(nbr), _p(err), _stream()),
          'cg_sparse_rules_down')
    _raise_flag(err, 'sparse tensor')
    return RuleBook(out_indices, indices, nbr, list(spatial_shape), out_shape, 'down', {'out_keys': out_keys})


def inverse_rules(book):
    """nbr (N_in, 8) of the inverse of the strided layer that built `book`; built once and kept in the book."""
    if book.kind != 'down':
        raise ValueError('the indice_key of a SparseInverseConv3d must belong to a SparseConv3d')
    if 'inverse_nbr' not in book.extra:
        n, out_keys = book.in_indices.shape[0], book.extra['out_keys']
        nbr = torch.empty((n, 8), dtype=torch.int32, device=book.in_indices.device)
        check(L.lib().cg_sparse_rules_inverse(_p(book.in_indices), n, _p(out_keys), out_keys.shape[0], *book.in_spatial_shape, _p(nbr),
                                              _stream()), 'cg_sparse_rules_inverse')
        book.extra['inverse_nbr'] = nbr
    return book.extra['inverse_nbr']


def sparse_conv(features, nbr, weight, bias=None, scale=None, shift=None, residual=None, features_b=None):
    """out[i] = bias + residual[i] + sum_k pro(features[nbr[i, k]]) @ weight[k], one launch.  weight (K, Cin, Cout).
    features_b: a second matrix with the same rows; the layer then reads the concatenation [features | features_b] (Cin = the sum of
    their widths) without forming it (cg_sparse_conv_cat), with the bits of the launch on torch.cat((features, features_b), 1)."""
    K, cin, cout = weight.shape
    n_out = nbr.shape[0]
    cin_b = 0 if features_b is None else features_b.shape[1]
    if features.shape[1] + cin_b != cin:
        raise ValueError(f'features have {features.shape[1] + cin_b} channels, the layer takes {cin}')
    if features_b is not None and features_b.shape[0] != features.shape[0]:
        raise ValueError(f'features has {features.shape[0]} rows, features_b {features_b.shape[0]}')
    if nbr.shape[1] != K:
        raise ValueError(f'the rule book has {nbr.shape[1]} offsets, the weight {K}')
    if (scale is None) != (shift is None):
        raise ValueError('the prologue needs both scale and shift')
    for name, t, shape in (('bias', bias, (cout,)), ('scale', scale, (cin,)), ('shift', shift, (cin,)), ('residual', residual, (n_out, cout)),
                           ('features_b', features_b, (features.shape[0], cin_b))):
        if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_cuda or t.device != features.device):
            raise ValueError(f'{name} must be a float32 tensor of shape {shape} on the device of features')
    out = torch.empty((n_out, cout), dtype=torch.float32, device=features.device)
    cont = lambda t: None if t is None else t.detach().contiguous()
    features_b = cont(features_b)
    tail = (_p(L.f32c(cont(weight))), _p(cont(bias)), _p(cont(scale)), _p(cont(shift)), _p(cont(residual)))
    if features_b is None:
        check(L.lib().cg_sparse_conv(_p(L.f32c(features)), features.shape[0], _p(L.i32c(nbr)), n_out, K, *tail, cin, cout, _p(out), _stream()),
              'cg_sparse_conv')
    else:
        check(L.lib().cg_sparse_conv_cat(_p(L.f32c(features)), features.shape[1], _p(L.f32c(features_b)), cin_b, features.shape[0], _p(L.i32c(nbr)),
                                         n_out, K, *tail, cout, _p(out), _stream()), 'cg_sparse_conv_cat')
    return out


def _triple(v, what):
    v = list(v) if isinstance(v, (list, tuple)) else [v] * 3
    if len(v) != 3:
        raise ValueError(f'{what} must be an int or three ints, got {v}')
    return [int(x) for x in v]


class SparseConvolution(SparseModule):
    """Base of the three layers; the constructor arguments are the reference's (spconv/conv.py)."""

    def __init__(self, ndim, in_channels, out_channels, kernel_size=3, stride=1, padding=0, dilation=1, groups=1, bias=True, subm=False,
                 output_padding=0, transposed=False, inverse=False, indice_key=None):
        super().__init__()
        if ndim != 3 or groups != 1 or transposed or _triple(dilation, 'dilation') != [1, 1, 1] or _triple(output_padding, 'output_padding') != [0, 0, 0]:
            raise NotImplementedError('only 3-D, groups = 1, dilation = 1, non-transposed sparse convolutions are built')
        kernel_size, stride, padding = _triple(kernel_size, 'kernel_size'), _triple(stride, 'stride'), _triple(padding, 'padding')
        if subm:
            # a submanifold layer keeps its sites: stride is moot (the reference ignores it too); k = 3 is centred, so padding must be k // 2
            if kernel_size not in ([1, 1, 1], [3, 3, 3]):
                raise NotImplementedError(f'SubMConv3d is built for kernel sizes 1 and 3, not {kernel_size}')
            if kernel_size == [3, 3, 3] and padding != [1, 1, 1]:
                raise NotImplementedError(f'SubMConv3d(kernel_size=3) needs padding=1, got {padding}')
        elif inverse:
            if kernel_size != [2, 2, 2]:
                raise NotImplementedError(f'SparseInverseConv3d is built for kernel size 2, not {kernel_size}')
            if indice_key is None:
                raise ValueError('SparseInverseConv3d needs the indice_key of its SparseConv3d')
        elif (kernel_size, stride, padding) != ([2, 2, 2], [2, 2, 2], [0, 0, 0]):
            raise NotImplementedError(f'SparseConv3d is built for kernel 2, stride 2, padding 0, not {kernel_size}, {stride}, {padding}')
        if not (in_channels == 6 or (in_channels > 0 and in_channels % 16 == 0 and in_channels <= MAX_CIN)):
            raise ValueError(f'in_channels must be 6 or a multiple of 16 up to {MAX_CIN}, got {in_channels}')
        if not (out_channels == 3 or (out_channels > 0 and out_channels % 16 == 0 and out_channels <= MAX_COUT)):
            raise ValueError(f'out_channels must be 3 or a multiple of 16 up to {MAX_COUT}, got {out_channels}')
        self.ndim, self.in_channels, self.out_channels = ndim, in_channels, out_channels
        self.kernel_size, self.stride, self.padding = kernel_size, stride, padding
        self.dilation, self.output_padding, self.groups = [1, 1, 1], [0, 0, 0], 1
        self.conv1x1 = kernel_size == [1, 1, 1]
        self.transposed, self.inverse, self.subm, self.indice_key = False, inverse, subm, indice_key
        self.weight = nn.Parameter(torch.empty(*kernel_size, in_channels, out_channels))
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        """The reference's initialisation: torch's kaiming-uniform with a = sqrt(5) called on the weight as it is laid out (torch then
        reads the fan from dimension 1 and everything after it), and a bias uniform within 1/sqrt(Cin * kernel volume)."""
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            bound = 1 / math.sqrt(self.in_channels * math.prod(self.kernel_size))
            nn.init.uniform_(self.bias, -bound, bound)

    def _rule_book(self, input):
        """-> (nbr, output indices, output spatial shape)"""
        if self.conv1x1:
            return identity_rules(input.indices.shape[0], input.indices.device), input.indices, input.spatial_shape
        book = input.find_indice_pair(self.indice_key)
        if self.inverse:
            if book is None:
                raise ValueError(f'SparseInverseConv3d: no SparseConv3d with indice_key {self.indice_key!r} has run on this tensor')
            if input.indices.shape[0] != book.out_indices.shape[0]:
                raise ValueError(f'SparseInverseConv3d: the tensor has {input.indices.shape[0]} sites, the SparseConv3d with indice_key '
                                 f'{self.indice_key!r} made {book.out_indices.shape[0]}')
            return inverse_rules(book), book.in_indices, book.in_spatial_shape
        if book is None:
            book = (subm_rules if self.subm else down_rules)(input.indices, input.spatial_shape, input.batch_size)
            if self.indice_key is not None:
                input.indice_dict[self.indice_key] = book
        elif book.kind != ('subm' if self.subm else 'down') or book.in_indices.shape[0] != input.indices.shape[0]:
            raise ValueError(f'indice_key {self.indice_key!r} belongs to another kind of layer or another set of sites')
        return book.nbr, book.out_indices, book.out_spatial_shape

    def forward(self, input, prologue=None, residual=None, features_b=None):
        """prologue: (scale, shift) per input channel, applied as max(x*scale + shift, 0) to the rows the layer reads.
        residual: (n_out, Cout), added to the output rows.
        features_b: (N, C_b) float32 device rows of the same sites; the layer reads [input.features | features_b] (sparse_conv)."""
        feats = _device_features(input, self.weight, self.bias)
        scale, shift = prologue if prologue is not None else (None, None)
        nbr, out_indices, out_shape = self._rule_book(input)
        K = nbr.shape[1]
        out = sparse_conv(feats, nbr, self.weight.detach().reshape(K, self.in_channels, self.out_channels), self.bias, scale, shift, residual,
                          None if features_b is None else features_b.detach().contiguous())
        return input.replace_feature(out, out_indices, out_shape)


class SubMConv3d(SparseConvolution):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True, indice_key=None):
        super().__init__(3, in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, True, indice_key=indice_key)


class SparseConv3d(SparseConvolution):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True, indice_key=None):
        super().__init__(3, in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, indice_key=indice_key)


class SparseInverseConv3d(SparseConvolution):
    def __init__(self, in_channels, out_channels, kernel_size, indice_key, bias=True):
        super().__init__(3, in_channels, out_channels, kernel_size, bias=bias, inverse=True, indice_key=indice_key)


def bn_relu_prologue(bn):
    """(scale, shift) of an eval-mode BatchNorm1d: y = x*scale + shift with scale = gamma / sqrt(var + eps), shift = beta - mean*scale."""
    scale = torch.rsqrt(bn.running_var.detach().float() + bn.eps)
    if bn.weight is not None:
        scale = scale * bn.weight.detach().float()
    shift = -bn.running_mean.detach().float() * scale
    if bn.bias is not None:
        shift = shift + bn.bias.detach().float()
    return scale.contiguous(), shift.contiguous()


class SparseSequential(SparseModule):
    """Sequential container: SparseModules take the SparseConvTensor, any other module is applied to its `.features`.  Constructed
    from positional modules, one OrderedDict, or named modules, like the reference's.  In eval mode a run of
    `BatchNorm1d, ReLU, <sparse convolution>` becomes the convolution's prologue (one launch instead of three; the input tensor's
    features are then left as they were)."""

    def __init__(self, *args, **kwargs):
        super().__init__()
        if len(args) == 1 and isinstance(args[0], OrderedDict):
            for key, module in args[0].items():
                self.add_module(key, module)
        else:
            for idx, module in enumerate(args):
                self.add_module(str(idx), module)
        for name, module in kwargs.items():
            if name in self._modules:
                raise ValueError(f'module name {name!r} is used twice')
            self.add_module(name, module)

    def __len__(self):
        return len(self._modules)

    def __getitem__(self, idx):
        if not -len(self) <= idx < len(self):
            raise IndexError(f'index {idx} is out of range')
        return list(self._modules.values())[idx]

    def add(self, module, name=None):
        name = str(len(self._modules)) if name is None else name
        if name in self._modules:
            raise KeyError(f'module name {name!r} is used twice')
        self.add_module(name, module)

    def _folds(self, mods, i, input):
        return (not self.training and i + 2 < len(mods) and isinstance(input, SparseConvTensor)
                and isinstance(mods[i], nn.BatchNorm1d) and not mods[i].training and mods[i].running_mean is not None
                and isinstance(mods[i + 1], nn.ReLU) and isinstance(mods[i + 2], SparseConvolution))

    def forward(self, input):
        mods = list(self._modules.values())
        i = 0
        while i < len(mods):
            module = mods[i]
            if self._folds(mods, i, input):
                input = mods[i + 2](input, prologue=bn_relu_prologue(module))
                i += 3
                continue
            if isinstance(module, SparseModule):
                if not isinstance(input, SparseConvTensor):
                    raise TypeError(f'{type(module).__name__} needs a SparseConvTensor')
                input = module(input)
            elif isinstance(input, SparseConvTensor):
                if input.indices.shape[0] != 0:
                    input.features = module(input.features)
            else:
                input = module(input)
            i += 1
        return input
