"""The 16-bit data path on the tape (BASELINE.json configs[1] "bf16", configs[4] "fp16"; the reference is fp32-only).

Activations, their gradients and a shadow of every layer's weights are bf16 / fp16 tensors in the BLOCKED layout of
``csrc/blocked16.h`` -- ``[N][C / 8][H][W][8]``: the 8 channels of a group at a pixel are one 16-byte MFMA operand slot --
while the master weights, the weight / bias gradients (accumulated straight into the fp32 arena), Adam and the losses stay
fp32.  A ``Var`` of this kind carries ``meta`` (a ``Blocked``); ``pack`` / ``unpack`` are the only crossings.

Fused activations and the "pre-masked gradient" convention.  A layer is ``y = act(conv(x) + b)`` in ONE kernel (the
reference's ``conv -> ReLU`` / ``leaky_relu(conv)`` pairs, age/vgg.py:78-82, age/models.py:48-50,70-73) and only ``y`` is
stored.  Its ``meta.mask_ref`` is ``y`` itself: the activation's derivative is 1 where ``y > 0`` and ``slope`` elsewhere.
The gradient handed to the producer of a tensor with a ``mask_ref`` is ALREADY multiplied by that derivative: every
operation that consumes such a tensor applies the mask in the epilogue of the kernel that produces its input gradient (the
data-gradient convolution, the pool backward, the fp32 -> 16-bit conversion), so the un-masked gradient never exists in HBM
and nothing like ``unary_kernel`` / ``binary_kernel`` runs on this path.  Sums of gradients commute with the mask, so
several consumers simply add up.

Second order (the gradient penalty, reference srgan.py:360-375).  With relu / leaky_relu and max-pool the networks are
piecewise linear, so every backward operation is again "a linear map, then a mask": ``conv(s, W^T) * mask(ref)``.  Its own
backward is the same kind of call with the roles swapped (the LINEARISED forward: ``conv(s, W) * mask(ref')``) plus a
weight gradient from (tangent, first-backward gradient), so the recorded backward and its double backward reuse the
forward kernels; masks and arg-max positions are constants."""
import collections
import ctypes
import os

import torch

from . import _lib
from . import functional as F
from .tape import Var, accumulates_into

TORCH_DTYPE = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
CODES = {'f32': 0, 'bf16': 1, 'f16': 2, 'fp16': 2}
# code 0: fp32 in the same blocked layout with FOUR channels per 16-byte slot -- the exact form of the 4x4 / stride 2 family
# (v_mfma_f32_32x32x2_f32; the fp32 gradient-penalty chain of the fp16 configuration, the crowd generator).  Conversions, sums
# and that family take it; the 3x3 / pooling / linear kernels are 16-bit only.


def group_size(code):
    return 4 if code == 0 else 8


def active_code():
    """The blocked dtype code the active ``F.storage_dtype`` asks for (None: plain fp32 tensors)."""
    if not F.STORAGE_DTYPE:
        return None
    return 0 if F.STORAGE_DTYPE == F.STORAGE_BLOCKED_F32 else F.STORAGE_DTYPE


class Blocked:
    """Logical shape and conventions of a 16-bit blocked tensor: ``c`` channels (``(c + 7) // 8`` groups) on an h x w plane;
    ``plane`` > 1 marks a FLATTENED tensor (h = w = 1) whose ``c`` entries are the slots of a [c0 / 8][plane][8] tensor."""
    __slots__ = ('n', 'c', 'h', 'w', 'code', 'mask_ref', 'slope', 'plane', 'real')

    def __init__(self, n, c, h, w, code, mask_ref=None, slope=0.0, plane=1, real=None):
        self.n, self.c, self.h, self.w, self.code = n, c, h, w, code
        self.mask_ref, self.slope, self.plane = mask_ref, slope, plane
        self.real = c if real is None else real          # features that exist (flattened tensors: channels x plane)

    @property
    def group(self):
        return group_size(self.code)

    @property
    def groups(self):
        return (self.c + self.group - 1) // self.group

    def like(self, **changes):
        values = {name: getattr(self, name) for name in self.__slots__}
        values.update(changes)
        return Blocked(**values)


def _call(name, *args):
    _lib.check(getattr(_lib.library(), name)(*args), name)


def _new(n, c, h, w, code, device):
    group = group_size(code)
    shape = (n, (c + group - 1) // group, h, w, group)
    if F.POISON:
        return torch.full(shape, float('nan'), dtype=TORCH_DTYPE[code], device=device)
    return torch.empty(shape, dtype=TORCH_DTYPE[code], device=device)


def _ptr(tensor):
    return None if tensor is None else tensor.data_ptr()


# ------------------------------------------------------------------------------------------------ conversions
def pack(x, code, mask_ref=None, slope=0.0):
    """fp32 [N, C, H, W] (or [N, F]) -> blocked 16-bit; with ``mask_ref`` the values are multiplied by the derivative of the
    activation that produced ``mask_ref`` (this is then the PRE-masked gradient of that activated tensor)."""
    shape = x.shape
    n, c = shape[0], shape[1]
    h, w = (shape[2], shape[3]) if len(shape) == 4 else (1, 1)
    if len(shape) not in (2, 4):
        raise ValueError(f'blocked16.pack takes [N, C, H, W] or [N, F], not {shape}')
    F._check_device(x.data)
    data = _new(n, c, h, w, code, x.data.device)
    _call('srgan_h_pack', x.data.data_ptr(), data.data_ptr(), _ptr(mask_ref), float(slope), n, c, h * w, code, F._stream())
    out = F._out(data, (x,), lambda s, needs: (unpack(s, shape),), 'h_pack')
    out.meta = Blocked(n, c, h, w, code, mask_ref, slope)
    return out


def unpack(x, shape=None):
    """blocked 16-bit -> fp32 [N, C, H, W] ([N, C] for 1 x 1 planes unless ``shape`` says otherwise)."""
    meta = x.meta
    if meta.plane != 1:
        raise ValueError('a flattened blocked tensor has no NCHW form: unpack before flatten')
    if shape is None:
        shape = (meta.n, meta.c) if meta.h == meta.w == 1 else (meta.n, meta.c, meta.h, meta.w)
    data = F._empty(shape, x.data)
    _call('srgan_h_unpack', x.data.data_ptr(), data.data_ptr(), meta.n, meta.c, meta.h * meta.w, meta.code, F._stream())
    return F._out(data, (x,), lambda g, needs: (pack(g, meta.code, meta.mask_ref, meta.slope),), 'h_unpack')


def flatten(x):
    """[N, C, H, W] -> [N, C/8 * H * W * 8] as a VIEW (the blocked order: a linear layer behind it permutes its weight
    shadow's columns instead, ``Shadow``)."""
    meta = x.meta
    if meta.h == meta.w == 1:
        return x
    if meta.code == 0:
        raise NotImplementedError('blocked16.flatten: the linear layers behind it are 16-bit only')
    plane, length = meta.h * meta.w, meta.groups * 8 * meta.h * meta.w

    def flat(tensor):
        return None if tensor is None else tensor.view(meta.n, length // 8, 1, 1, 8)
    flat_meta = Blocked(meta.n, length, 1, 1, meta.code, flat(meta.mask_ref), meta.slope, plane, meta.c * plane)

    def backward(s, needs):
        data = s.data.view(meta.n, meta.groups, meta.h, meta.w, 8)
        back = F._out(data, (s,), lambda t, n2: (_reflatten(t, flat_meta),), 'h_unflatten')
        back.meta = meta
        return (back,)
    out = F._out(flat(x.data), (x,), backward, 'h_flatten')
    out.meta = flat_meta
    return out


def _reflatten(t, flat_meta):
    out = F._out(t.data.view(flat_meta.n, flat_meta.c // 8, 1, 1, 8), (t,), None, 'h_flatten')
    out.meta = flat_meta
    if out.node is not None:
        raise NotImplementedError('third-order use of blocked16.flatten')
    return out


def add(a, b):
    if a.meta is None or b.meta is None or a.data.shape != b.data.shape or a.meta.code != b.meta.code:
        raise ValueError('blocked16.add: both operands must be 16-bit blocked tensors of one shape')
    data = torch.empty_like(a.data)
    _call('srgan_h_add', a.data.data_ptr(), b.data.data_ptr(), data.data_ptr(), data.numel() // a.meta.group, a.meta.code, F._stream())
    out = F._out(data, (a, b), lambda g, needs: (g, g), 'h_add')
    out.meta = a.meta
    return out


# ------------------------------------------------------------------------------------------------ pooling
def max_pool2(x):
    """max_pool2d(x, 2, 2) (reference age/vgg.py:76).  Backward: the pooled gradient placed at the arg-max and multiplied
    by the derivative of the activation that produced ``x`` in one pass; the arg-max is recomputed (first maximum)."""
    meta = x.meta
    if meta.h % 2 or meta.w % 2:
        raise ValueError('blocked16.max_pool2 needs even planes')
    if meta.mask_ref is not None and meta.mask_ref.data_ptr() != x.data.data_ptr():
        raise ValueError('blocked16.max_pool2 pools activated tensors (mask = the tensor itself) or plain ones')
    data = _new(meta.n, meta.c, meta.h // 2, meta.w // 2, meta.code, x.data.device)
    _call('srgan_h_maxpool2', x.data.data_ptr(), None, data.data_ptr(), meta.n * meta.groups, meta.h, meta.w, 0, meta.code,
          F._stream())
    out = F._out(data, (x,), lambda g, needs: (_pool_backward(x.data, meta, g),), 'h_max_pool2')
    out.meta = Blocked(meta.n, meta.c, meta.h // 2, meta.w // 2, meta.code)
    return out


def _pool_backward(x_data, meta, g):
    data = torch.empty_like(x_data)
    _call('srgan_h_maxpool2_bwd', x_data.data_ptr(), g.data.data_ptr(), data.data_ptr(), meta.n * meta.groups, meta.h, meta.w,
          1 if meta.mask_ref is not None else 0, float(meta.slope), meta.code, F._stream())
    out = F._out(data, (g,), lambda s, needs: (_pool_gather(x_data, meta, s),), 'h_max_pool2_backward')
    out.meta = meta
    return out


def _pool_gather(x_data, meta, s):
    """``s`` (shape of x, pre-masked) at the arg-max of x: the pool's action on a tangent."""
    data = _new(meta.n, meta.c, meta.h // 2, meta.w // 2, meta.code, x_data.device)
    _call('srgan_h_maxpool2', x_data.data_ptr(), s.data.data_ptr(), data.data_ptr(), meta.n * meta.groups, meta.h, meta.w, 2,
          meta.code, F._stream())
    out = F._out(data, (s,), lambda t, needs: (_pool_backward(x_data, meta, t),), 'h_max_pool2_gather')
    out.meta = Blocked(meta.n, meta.c, meta.h // 2, meta.w // 2, meta.code)
    return out


# ------------------------------------------------------------------------------------------------ weight shadows
def _capturing():
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def _refuse_under_capture(what):
    """A HIP-graph capture records launches only: an allocation would come from the graph's pool and a host-to-device copy is
    illegal, so whatever needs one must exist before the capture (``prepare``)."""
    if _capturing():
        raise RuntimeError(f'blocked16: {what} during a HIP graph capture; call blocked16.prepare(arena) for every network '
                           'of the step (and run the step once eagerly) before capturing it')


def _contract(name, a, b, bias, ref, slope, epi, out_meta, *extents):
    """One launch of a contraction entry point -- they all take (two operands, bias, mask reference, slope, epilogue, output,
    extents ..., code, stream) -- into a fresh tensor of ``out_meta``'s shape: returns (that tensor, ``out_meta``)."""
    data = _new(out_meta.n, out_meta.c, out_meta.h, out_meta.w, out_meta.code, a.device)
    _call(name, a.data_ptr(), b.data_ptr(), bias, _ptr(ref), float(slope), epi, data.data_ptr(), *extents, out_meta.code, F._stream())
    return data, out_meta


class Form(collections.namedtuple('Form', 'name slots source packer tail dtype', defaults=(torch.int32,))):
    """One operand form of a shadow: the buffer ``name`` of ``slots`` 16-byte slots (``dtype`` elements), written from the fp32
    ``source`` by ``srgan_h_pack_<packer>(source, buffer, *tail, stream)``, or in the batched refresh by the job that
    ``srgan_h_pack_job_<packer>(job, first_block, source, buffer, *tail)`` fills in."""
    __slots__ = ()


class Shadow:
    """The 16-bit operand forms of one layer's fp32 master weights: ``forward`` (rows = outputs) and ``transposed`` (the
    data gradient's operand), re-rounded whenever the masters changed -- by ``refresh(arena)`` right behind the optimizer
    update (same stream as the update), or lazily when the version key below moved (checkpoint load, tests).  Every buffer
    (the ``linear_t`` bias rows included) is allocated once and then written in place, so a refresh can be captured.

    A kind of layer is a subclass (``SHADOW_KINDS``): it measures the layer once (``_measure``), enumerates its operand
    forms (``forms``: read by ``repack`` and by the batched refresh only, never on the layer path), and knows the layer's
    contraction launch and weight gradient."""
    kind = None

    def __init__(self, module, code, in_blocked=0, plane=1):
        _refuse_under_capture(f'a new {self.kind} weight shadow')
        self.module, self.code, self.in_blocked, self.plane = module, code, in_blocked, plane
        self.forward = self.transposed = self.down = self.up = self.bias_rows = None
        self.key = None
        self._measure()
        arena = getattr(module.weight, '_srgan_arena', None)
        if arena is not None:
            arena.shadows.append(self)

    def fresh(self):
        if self.key != self._version():
            # the lazy path (first use, checkpoint load, a test that edited the weights): other streams may launch readers of
            # this shadow right away -- they are only ordered behind whatever wrote the masters, not behind this repack
            _refuse_under_capture(f'a {self.kind} weight shadow behind its masters')
            self.repack()
            torch.cuda.current_stream().synchronize()
        return self

    def repack(self):
        """Every form by its single-layer packer, one launch per operand."""
        stream = F._stream()
        for form in self.forms():
            self._pack(form, self._buffer(form.name, form.slots, form.dtype), stream)
        self.key = self._version()

    def _pack(self, form, target, stream):
        _call('srgan_h_pack_' + form.packer, form.source.data_ptr(), target, *form.tail, stream)

    def _fill(self, job, first_block, form, target):
        """``form`` as job(s) of the batched refresh, written to host memory at ``job``: (jobs written, workgroups taken)."""
        name = 'srgan_h_pack_job_' + form.packer
        taken = getattr(_lib.library(), name)(job, first_block, form.source.data_ptr(), target, *form.tail)
        _lib.check(min(taken, 0), name)
        return 1, taken

    def _buffer(self, name, slots, dtype=torch.int32):
        """The device buffer of one operand form (``slots`` 16-byte slots), allocated on first use and then kept."""
        if getattr(self, name, None) is None:
            _refuse_under_capture(f'the first {name} buffer of a {self.kind} weight shadow')
            setattr(self, name, torch.empty(slots * 4, dtype=dtype, device=self.module.weight.device))
        return getattr(self, name).data_ptr()

    def _version(self):
        weight = self.module.weight
        arena = getattr(weight, '_srgan_arena', None)
        bias = getattr(self.module, 'bias', None)
        return (weight.data_ptr(), weight._version, None if bias is None else bias._version,
                None if arena is None else (arena.version, arena.data._version))


class Conv3x3Shadow(Shadow):
    """A 3x3 / stride 1 / padding 1 ``nn.Conv2d``, weights [K][C][3][3]."""
    kind = 'conv3x3'

    def _measure(self):
        self.k, self.c, self.r, self.s = self.module.weight.shape

    def forms(self):
        k, c, r, s = self.k, self.c, self.r, self.s
        slots = _lib.library().srgan_h_conv_weight_slots
        for name, transposed, rows, reduced in (('forward', 0, k, c), ('transposed', 1, c, k)):
            yield Form(name, slots(rows, reduced, r, s), self.module.weight, 'conv_weights', (k, c, r, s, transposed, self.code))

    def launch(self, x, transposed, epi, slope, ref, bias):
        meta = x.meta
        c_in, c_out = (self.k, self.c) if transposed else (self.c, self.k)
        if meta.c != c_in:
            raise ValueError(f'blocked16 conv: input has {meta.c} channels, the layer expects {c_in}')
        operand = self.transposed if transposed else self.forward
        return _contract('srgan_h_conv3x3', x.data, operand, F._ptr(bias), ref, slope, epi,
                         Blocked(meta.n, c_out, meta.h, meta.w, meta.code), meta.n, c_in, c_out, c_out, meta.h, meta.w)

    def weight_gradient(self, x_side, y_side, into):
        xm = x_side.meta
        _call('srgan_h_conv3x3_wgrad', x_side.data.data_ptr(), y_side.data.data_ptr(), into.data_ptr(), xm.n, xm.c, y_side.meta.c,
              xm.h, xm.w, xm.code, F._stream())


class Conv3x3ImageShadow(Shadow):
    """A 3x3 / stride 1 / padding 1 ``nn.Conv2d`` of the fp32 NCHW family (the dense layers' ``conv2``), weights [K][C][3][3]: the
    fp32 WEIGHT IMAGES ``srgan_conv2d_*_bnrelu_image`` stage from (include/srgan_hip.h; ``code`` is 0) -- ``forward`` for the
    convolution, ``transposed`` for its data gradient.  No rounding: the images hold the masters' own bits in the kernel's
    staging order, so the calls that read them are bit-identical to the ones that gather from the masters.  The layer's launches
    live in ``fused.dense_block``; the weight gradient does not read the weights."""
    kind = 'conv3x3_image'

    def _measure(self):
        self.k, self.c, r, s = self.module.weight.shape
        if (r, s) != (3, 3):
            raise ValueError('blocked16: a weight image is the operand of a 3x3 convolution')

    def forms(self):
        floats = _lib.library().srgan_conv3x3_image_floats
        for name, transposed, rows, reduced in (('forward', 0, self.k, self.c), ('transposed', 1, self.c, self.k)):
            yield Form(name, floats(reduced, rows) // 4, self.module.weight, 'conv3x3_image', (self.k, self.c, transposed), torch.float32)


class K4s2Shadow(Shadow):
    """The 4x4 / stride 2 / padding 1 family, weights [A][B][4][4] with A = the channels on the small plane: conv2d weights
    [K][C], conv_transpose2d weights [Cin][Cout].  ``down`` is the operand big -> small plane, ``up`` small -> big."""
    kind = 'k4s2'

    def _measure(self):
        self.a, self.b = self.module.weight.shape[:2]
        self.transpose = isinstance(self.module, torch.nn.ConvTranspose2d)

    def forms(self):
        slots = _lib.library().srgan_h_k4s2_weight_slots
        for name, direction in (('down', 0), ('up', 1)):
            yield Form(name, slots(self.a, self.b, direction, self.code), self.module.weight, 'k4s2_weights',
                       (self.a, self.b, direction, self.code))

    def _fill(self, job, first_block, form, target):
        written = ctypes.c_int32()              # a form of this kind may take several jobs: the filler says how many
        _, taken = super()._fill(job, first_block, form._replace(tail=form.tail + (ctypes.byref(written),)), target)
        return written.value, taken

    def launch(self, x, transposed, epi, slope, ref, bias):
        meta, a, b = x.meta, self.a, self.b
        if self.transpose != transposed:                       # small -> big plane
            if meta.c != a:
                raise ValueError(f'blocked16 transposed 4x4 / s2: input has {meta.c} channels, expected {a}')
            return _contract('srgan_h_conv_transpose4x4s2', x.data, self.up, F._ptr(bias), ref, slope, epi,
                             Blocked(meta.n, b, 2 * meta.h, 2 * meta.w, meta.code), meta.n, a, b, meta.h, meta.w)
        if meta.c != b or meta.h % 2 or meta.w % 2:
            raise ValueError(f'blocked16 4x4 / s2: input [{meta.c}, {meta.h}, {meta.w}], expected {b} channels on an even plane')
        return _contract('srgan_h_conv4x4s2', x.data, self.down, F._ptr(bias), ref, slope, epi,
                         Blocked(meta.n, a, meta.h // 2, meta.w // 2, meta.code), meta.n, b, a, meta.h, meta.w)

    def weight_gradient(self, x_side, y_side, into):
        # conv2d: input side = the big plane; conv_transpose2d: input side = the small plane
        big, small = (y_side, x_side) if self.transpose else (x_side, y_side)
        _call('srgan_h_k4s2_wgrad', big.data.data_ptr(), small.data.data_ptr(), into.data_ptr(), big.meta.n, big.meta.c, small.meta.c,
              big.meta.h, big.meta.w, 1, x_side.meta.code, F._stream())


class LinearShadow(Shadow):
    """An ``nn.Linear`` on a [N, F] blocked matrix of ``in_blocked`` columns (0: the inputs padded to whole groups), which may
    be the flattened view of a [N, C, H, W] tensor (``plane`` = H * W): the shadow's columns follow the blocked order."""
    kind = 'linear'

    def _measure(self):
        weight = self.module.weight
        self.outputs, self.inputs = weight.shape[0], weight.numel() // weight.shape[0]
        self.blocked = self.in_blocked or (self.inputs + 7) // 8 * 8
        self.outputs_padded = (self.outputs + 7) // 8 * 8

    def forms(self):
        """The (rows, cols, rows_real, cols_real, row_stride, col_stride, row_plane, col_plane) of ``srgan_h_pack_matrix``:
        forward operand A[o][f'] = W[o][map(f')]; transposed operand A[f'][o] = W[o][map(f')]."""
        outputs, inputs, blocked, padded = self.outputs, self.inputs, self.blocked, self.outputs_padded
        weight, plane, code = self.module.weight, self.plane, self.code
        yield Form('forward', outputs * blocked // 8, weight, 'matrix', (outputs, blocked, outputs, inputs, inputs, 1, 1, plane, code))
        yield Form('transposed', blocked * padded // 8, weight, 'matrix', (blocked, padded, inputs, outputs, 1, inputs, plane, 1, code))

    def launch(self, x, transposed, epi, slope, ref, bias):
        meta, outputs, blocked = x.meta, self.outputs, self.blocked
        if transposed:
            if meta.c != outputs:
                raise ValueError(f'blocked16 linear (data gradient): input has {meta.c} features, expected {outputs}')
            return _contract('srgan_h_gemm', self.transposed, x.data, None, ref, slope, epi,
                             Blocked(meta.n, blocked, 1, 1, meta.code, plane=self.plane, real=self.inputs),
                             blocked, meta.n, outputs, blocked, 0)
        if meta.c != blocked:
            raise ValueError(f'blocked16 linear: input has {meta.c} (blocked) features, the shadow was built for {blocked}')
        return _contract('srgan_h_gemm', self.forward, x.data, F._ptr(bias), ref, slope, epi, Blocked(meta.n, outputs, 1, 1, meta.code),
                         outputs, meta.n, blocked, outputs, outputs)

    def weight_gradient(self, x_side, y_side, into):
        xm = x_side.meta
        _call('srgan_h_linear_wgrad', y_side.data.data_ptr(), x_side.data.data_ptr(), into.data_ptr(), xm.n, self.outputs, xm.c,
              self.outputs, self.inputs, self.inputs, 1, 1, self.plane, xm.code, F._stream())


class SeedShadow(Shadow):
    """``nn.ConvTranspose2d`` weights [Cin][Cout][R][S] applied to a 1 x 1 input: a linear map Cin -> (Cout, R x S), its
    outputs in the blocked order of a [Cout, R, S] tensor (``plane`` = R * S, ``blocked`` rows).  With a bias, ``bias_rows``
    holds bias[co] of every output row (co, pixel) in that order, as fp32."""
    kind = 'linear_t'

    def _measure(self):
        self.c_in, self.c_out, self.r, self.s = self.module.weight.shape
        self.plane = self.r * self.s
        self.features = self.c_out * self.plane
        self.blocked = (self.c_out + 7) // 8 * 8 * self.plane
        self.c_in_padded = (self.c_in + 7) // 8 * 8

    def forms(self):
        c_in, features, blocked, padded, plane = self.c_in, self.features, self.blocked, self.c_in_padded, self.plane
        weight, code = self.module.weight, self.code
        yield Form('forward', blocked * padded // 8, weight, 'matrix', (blocked, padded, features, c_in, 1, features, plane, 1, code))
        yield Form('transposed', c_in * blocked // 8, weight, 'matrix', (c_in, blocked, c_in, features, features, 1, 1, plane, code))
        if self.module.bias is not None:              # ``blocked`` floats, four to a slot
            yield Form('bias_rows', blocked // 4, self.module.bias, 'bias_rows', (self.c_out, plane), torch.float32)

    def _pack(self, form, target, stream):
        if form.name != 'bias_rows':
            return super()._pack(form, target, stream)
        # the bias rows have no single-layer entry point (a copy, no arithmetic: written in place, the buffer keeps its address)
        channels, plane = form.tail
        full = channels // 8
        rows, bias = self.bias_rows.view(-1, plane, 8), form.source.data
        if full:
            rows[:full].copy_(bias[:full * 8].view(full, 1, 8).expand(full, plane, 8))
        if channels % 8:
            rows[full].zero_()
            rows[full, :, :channels % 8].copy_(bias[full * 8:].view(1, -1).expand(plane, channels % 8))

    def launch(self, x, transposed, epi, slope, ref, bias):
        meta, c_in, c_out, blocked = x.meta, self.c_in, self.c_out, self.blocked
        if transposed:                                         # [N, Cout, R, S] -> [N, Cin]
            if (meta.c, meta.h, meta.w) != (c_out, self.r, self.s):
                raise ValueError('blocked16 seed transposed convolution (data gradient): unexpected input shape')
            return _contract('srgan_h_gemm', self.transposed, x.data, None, ref, slope, epi, Blocked(meta.n, c_in, 1, 1, meta.code),
                             c_in, meta.n, blocked, c_in, 0)
        if meta.c != c_in:
            raise ValueError(f'blocked16 seed transposed convolution: input has {meta.c} features, expected {c_in}')
        rows = None if bias is None else _ptr(self.bias_rows)
        return _contract('srgan_h_gemm', self.forward, x.data, rows, ref, slope, epi, Blocked(meta.n, c_out, self.r, self.s, meta.code),
                         blocked, meta.n, self.c_in_padded, blocked, blocked)

    def weight_gradient(self, x_side, y_side, into):
        xm = x_side.meta
        _call('srgan_h_linear_wgrad', y_side.data.data_ptr(), x_side.data.data_ptr(), into.data_ptr(), xm.n, self.blocked, xm.c,
              self.features, self.c_in, 1, self.features, self.plane, 1, xm.code, F._stream())


SHADOW_KINDS = {cls.kind: cls for cls in (Conv3x3Shadow, Conv3x3ImageShadow, K4s2Shadow, LinearShadow, SeedShadow)}
# the shadow kinds of the batched refresh: all of them (the matrix shadows and the seed layer's bias rows since ABI 1.1's
# SRGAN_FEATURE_BATCHED_SHADOWS)
BATCHED_KINDS = tuple(SHADOW_KINDS)


def shadow_of(module, kind, code, in_blocked=0, plane=1):
    table = module.__dict__.setdefault('_srgan_shadows', {})
    key = (kind, code, in_blocked, plane)
    found = table.get(key)
    if found is None:
        found = table[key] = SHADOW_KINDS[kind](module, code, in_blocked, plane)
    return found.fresh()


class _PackPlan:
    """Every shadow of one arena as ONE launch (``srgan_h_pack_batched``): a device array of jobs, built once from the
    arguments the single-layer packers would get -- the masters live at fixed arena addresses and a shadow keeps its
    buffers, so the table stays valid until the set of shadows changes (and a replayed refresh writes the same addresses)."""

    def __init__(self, shadows):
        _refuse_under_capture('building the batched shadow refresh')
        size = _lib.library().srgan_h_pack_job_bytes()
        self.shadows = list(shadows)
        self.signature = _signature(self.shadows)
        host = ctypes.create_string_buffer(size * 5 * max(1, len(self.shadows)))
        count = blocks = 0
        device = None
        for shadow in self.shadows:
            device = shadow.module.weight.device
            for form in shadow.forms():
                target = shadow._buffer(form.name, form.slots, form.dtype)
                written, taken = shadow._fill(ctypes.byref(host, count * size), blocks, form, target)
                count, blocks = count + written, blocks + taken
        self.count, self.blocks = count, blocks
        self.table = None
        if count:
            self.table = torch.frombuffer(bytearray(host.raw[:count * size]), dtype=torch.uint8).to(device)

    def run(self):
        if self.table is not None:
            _call('srgan_h_pack_batched', self.table.data_ptr(), self.count, self.blocks, F._stream())
        for shadow in self.shadows:
            shadow.key = shadow._version()


def _signature(shadows):
    return tuple((id(s), s.module.weight.data_ptr(), None if s.module.bias is None else s.module.bias.data_ptr()) for s in shadows)


def _plan(arena):
    """The arena's batched refresh, (re)built when its set of shadows changed."""
    plan = getattr(arena, '_pack_plan', None)
    if plan is None or plan.signature != _signature(arena.shadows):
        plan = arena._pack_plan = _PackPlan(arena.shadows)
    return plan


def refresh(arena):
    """Re-round every shadow of the networks' weights in ``arena`` (called right behind the optimizer update, on its stream:
    whatever orders a later reader behind the update orders it behind the shadows too) as ONE batched launch that writes only
    fixed addresses (``SRGAN_H_NO_BATCHED_PACK=1``: the single-layer packers, one launch per operand)."""
    shadows = getattr(arena, 'shadows', ())
    if not shadows:
        return
    if os.environ.get('SRGAN_H_NO_BATCHED_PACK') == '1':
        for shadow in shadows:
            shadow.repack()
        return
    _plan(arena).run()


def stale(arena):
    """True when a master of ``arena`` was written behind its shadows' back (a version key moved: checkpoint load, a copy
    into ``arena.data``, a test editing the weights).  Host-side only: no launch, no synchronisation."""
    return any(shadow.key != shadow._version() for shadow in getattr(arena, 'shadows', ()))


def refresh_if_stale(arena):
    """``refresh(arena)`` on the current stream when ``stale(arena)``; returns whether it re-rounded."""
    if not stale(arena):
        return False
    refresh(arena)
    return True


def prepare(arena):
    """Make the shadows of ``arena`` capture-ready: every buffer (bias rows included) and the batched refresh's device job
    table exist, and the shadows are current.  Call it for every network of a step before capturing the step: inside the
    capture nothing may allocate or copy from the host, and the Adam -> refresh pair it records then only rewrites fixed
    addresses.  (A shadow that the step would create for the first time still raises there: run the step eagerly first.)"""
    _refuse_under_capture('blocked16.prepare')
    if not getattr(arena, 'shadows', ()):
        return
    if os.environ.get('SRGAN_H_NO_BATCHED_PACK') == '1':
        refresh(arena)                                  # the single-layer packers allocate what is missing
        return
    plan = _plan(arena)
    if stale(arena):
        plan.run()


# ------------------------------------------------------------------------------------------------ fused layers
def _parameter(p):
    from .nn import parameter_var
    return None if p is None else parameter_var(p)


def conv3x3(x, module, slope=None):
    """``act(conv2d(x, w, b, stride 1, padding 1))`` for a 3x3 ``nn.Conv2d``: slope None = no activation, 0.0 = ReLU (reference
    age/vgg.py:78-82), other = leaky_relu."""
    if tuple(module.kernel_size) != (3, 3) or tuple(module.stride) != (1, 1) or tuple(module.padding) != (1, 1):
        raise ValueError('blocked16.conv3x3: 3x3 / stride 1 / padding 1 convolutions')
    return _activated_layer(x, module, shadow_of(module, 'conv3x3', x.meta.code), slope)


def linear(x, module, slope=None):
    """``act(linear(x, w, b))`` on a [N, F] blocked matrix (reference age/vgg.py:33-41,48-53); ``x`` may be the flattened view
    of a [N, C, H, W] tensor: the shadow's columns follow the blocked order."""
    meta = x.meta
    if meta.h != 1 or meta.w != 1:
        raise ValueError('blocked16.linear takes [N, F] (flatten first)')
    return _activated_layer(x, module, shadow_of(module, 'linear', meta.code, in_blocked=meta.groups * 8, plane=meta.plane), slope)


def conv4x4s2(x, module, slope=None):
    """``act(conv2d(x, w, b, stride 2, padding 1))`` for a 4x4 ``nn.Conv2d`` (the DCGAN discriminator's stages, reference
    age/models.py:61-73: ``leaky_relu(layer(x), 0.05)``)."""
    if tuple(module.kernel_size) != (4, 4) or tuple(module.stride) != (2, 2) or tuple(module.padding) != (1, 1):
        raise ValueError('blocked16.conv4x4s2: 4x4 / stride 2 / padding 1 convolutions')
    return _activated_layer(x, module, shadow_of(module, 'k4s2', x.meta.code), slope)


def conv_transpose4x4s2(x, module, slope=None):
    """``act(conv_transpose2d(x, w, b, stride 2, padding 1))`` for a 4x4 ``nn.ConvTranspose2d`` (the DCGAN generator's stages,
    reference age/models.py:37-51)."""
    if tuple(module.kernel_size) != (4, 4) or tuple(module.stride) != (2, 2) or tuple(module.padding) != (1, 1) or \
            tuple(module.output_padding) != (0, 0):
        raise ValueError('blocked16.conv_transpose4x4s2: 4x4 / stride 2 / padding 1 transposed convolutions')
    return _activated_layer(x, module, shadow_of(module, 'k4s2', x.meta.code), slope)


def seed_conv_transpose(x, module, slope=None):
    """``conv_transpose2d`` of a [N, Cin] code (a 1 x 1 plane) with a full-plane kernel, stride 1, no padding (the generator's
    ``fc``, reference age/models.py:37,47): a linear map onto a [N, Cout, R, S] tensor."""
    if tuple(module.stride) != (1, 1) or tuple(module.padding) != (0, 0) or x.meta.h != 1 or x.meta.w != 1 or x.meta.plane != 1:
        raise ValueError('blocked16.seed_conv_transpose: a stride-1 unpadded transposed convolution of a 1 x 1 plane')
    return _activated_layer(x, module, shadow_of(module, 'linear_t', x.meta.code), slope)


def _activated_layer(x, module, shadow, slope):
    """The tail of the public layer functions: bias and leaky(slope) in the layer's kernel (slope None: no activation)."""
    return _layer(x, module, shadow, False, 1, 1.0 if slope is None else float(slope), None, True)


def _into_arena(parameter, what, where=' (straight into the fp32 gradient arena)'):
    """Parameter gradients of this path exist only as sums into the fp32 arena, which a plain backward sweep offers."""
    if not accumulates_into(parameter):
        raise NotImplementedError(f'the 16-bit path computes {what} gradients in plain backward sweeps only{where}')


def _layer(x, module, shadow, transposed, epi, slope, ref, use_bias):
    """One contraction ``epi(op(x, W) [+ b])`` recorded on the tape.  transposed: the data-gradient direction (x has the
    layer's OUTPUT features).  epi 1: bias + leaky(slope); epi 2: times mask(ref, slope); epi 0: plain."""
    meta = x.meta
    weight = _parameter(module.weight)
    bias = _parameter(module.bias) if (use_bias and module.bias is not None) else None
    data, out_meta = shadow.launch(x, transposed, epi, slope, ref, bias)
    if epi == 1 and slope != 1.0:
        out_meta.mask_ref, out_meta.slope = data, slope            # an activated tensor is its own mask
    elif epi == 2:
        out_meta.mask_ref, out_meta.slope = ref, slope              # a pre-masked gradient: cotangents arrive masked alike

    def backward(s, needs):
        gx = None
        if needs[0]:
            if meta.mask_ref is not None:
                gx = _layer(s, module, shadow, not transposed, 2, meta.slope, meta.mask_ref, False)
            else:
                gx = _layer(s, module, shadow, not transposed, 0, 1.0, None, False)
        if needs[1]:
            _into_arena(weight, 'weight')
            x_side, y_side = (s, x) if transposed else (x, s)
            shadow.weight_gradient(x_side, y_side, weight.grad_buffer)
        if needs[2]:
            _into_arena(bias, 'bias', '')
            sm = s.meta
            _call('srgan_h_channel_sums', s.data.data_ptr(), bias.grad_buffer.data_ptr(), sm.n, sm.c, sm.h * sm.w, sm.code,
                  F._stream())
        return gx, None, None
    out = F._out(data, (x, weight, bias), backward, 'h_' + shadow.kind + ('_t' if transposed else ''))
    out.meta = out_meta
    return out


def _weight_gradient(shadow, module, x_side, y_side, into):
    """into (fp32, the arena's gradient view of the layer's weight) += d loss / d W from the tensor at the layer's input side
    and the (pre-masked) gradient at its output side."""
    shadow.weight_gradient(x_side, y_side, into)


# ------------------------------------------------------------------------------------------------ batch statistics
def _norm_tensors(x, gamma, beta):
    meta = x.meta
    if meta is None or meta.plane != 1:
        raise ValueError('blocked16 batch norm takes a blocked [N, C, H, W] tensor')
    if gamma.data.numel() != meta.c or beta.data.numel() != meta.c:
        raise ValueError(f'blocked16 batch norm: input has {meta.c} channels, the layer has {gamma.data.numel()}')
    return meta


def _activated(meta, data, slope):
    """The ``Blocked`` of ``leaky(..., slope)`` written into ``data``: an activated tensor is its own mask."""
    out_meta = Blocked(meta.n, meta.c, meta.h, meta.w, meta.code)
    if slope != 1.0:
        out_meta.mask_ref, out_meta.slope = data, slope
    return out_meta


def batch_norm_train(x, gamma, beta, running_mean, running_var, momentum, eps, slope=1.0, num_batches_tracked=None):
    """``F.batch_norm_train`` on a blocked tensor of any code (csrc/blocked16_batch_norm.hip): y = leaky((x - mean_B) *
    rsqrt(var_B + eps) * gamma + beta, slope) with the statistics of THIS batch, the running buffers updated on the device;
    two launches forward, two backward, nothing kept but x, the batch mean and inv_std.  The output is its own mask
    (``slope`` != 1), so the gradient arrives pre-masked and the backward applies only the mask of ``x`` itself.  gamma / beta
    gradients go straight into the fp32 arena.  FIRST ORDER ONLY, as the NCHW op."""
    meta = _norm_tensors(x, gamma, beta)
    n, c, hw, code = meta.n, meta.c, meta.h * meta.w, meta.code
    if n * hw < 2:
        raise ValueError(f'Expected more than 1 value per channel when training, got input size {[n, c, meta.h, meta.w]}')
    if momentum is None:
        raise NotImplementedError('batch_norm_train: momentum=None (cumulative moving average) is not implemented')
    stats = F._empty((2, c), x.data)               # batch mean, inv_std
    data = _new(n, c, meta.h, meta.w, code, x.data.device)
    slope = float(slope)
    _call('srgan_h_batch_norm_stats', x.data.data_ptr(), stats[0].data_ptr(), stats[1].data_ptr(), _ptr(running_mean),
          _ptr(running_var), _ptr(num_batches_tracked), float(momentum), float(eps), n, c, hw, code, F._stream())
    _call('srgan_h_batch_norm_fwd', x.data.data_ptr(), stats[0].data_ptr(), stats[1].data_ptr(), gamma.data.data_ptr(),
          beta.data.data_ptr(), slope, data.data_ptr(), n, c, hw, code, F._stream())
    out = F._out(data, (x, gamma, beta), None, 'h_batch_norm_train')
    out.meta = _activated(meta, data, slope)
    if out.node is None:
        return out                                 # (no_grad: the statistics are dropped with this frame)

    def backward(s, needs):
        if F.grad_enabled():
            raise NotImplementedError('batch_norm_train has a first-order backward only: differentiating a gradient through '
                                      'batch statistics (create_graph=True) is not implemented')
        for need, parameter in ((needs[1], gamma), (needs[2], beta)):
            if need:
                _into_arena(parameter, 'batch-norm parameter')
        sums = F._empty((2, c), x.data)            # sum s (= g_beta), sum s * xhat (= g_gamma)
        _call('srgan_h_batch_norm_bwd_reduce', s.data.data_ptr(), x.data.data_ptr(), stats[0].data_ptr(), stats[1].data_ptr(),
              sums.data_ptr(), gamma.grad_buffer.data_ptr() if needs[1] else None, beta.grad_buffer.data_ptr() if needs[2] else None,
              n, c, hw, code, F._stream())
        gx = None
        if needs[0]:
            gx = Var(_new(n, c, meta.h, meta.w, code, x.data.device))
            _call('srgan_h_batch_norm_bwd_apply', s.data.data_ptr(), x.data.data_ptr(), stats[0].data_ptr(), stats[1].data_ptr(),
                  gamma.data.data_ptr(), sums.data_ptr(), _ptr(meta.mask_ref), float(meta.slope), gx.data.data_ptr(), n, c, hw, code,
                  F._stream())
            gx.meta = meta                          # a pre-masked gradient of x
        return gx, None, None
    out.node.backward = backward
    return out


def batch_norm_eval(x, mean, inv_std, gamma, beta, slope=1.0):
    """The forward kernel with given statistics (``nn.BatchStatNorm2d`` in eval mode on a blocked tensor): forward only."""
    meta = _norm_tensors(x, gamma, beta)
    data = _new(meta.n, meta.c, meta.h, meta.w, meta.code, x.data.device)
    slope = float(slope)
    _call('srgan_h_batch_norm_fwd', x.data.data_ptr(), mean.data.data_ptr(), inv_std.data.data_ptr(), gamma.data.data_ptr(),
          beta.data.data_ptr(), slope, data.data_ptr(), meta.n, meta.c, meta.h * meta.w, meta.code, F._stream())

    def backward(s, needs):
        raise NotImplementedError('blocked16.batch_norm_eval is forward only: a BatchStatNorm2d on blocked tensors is '
                                  'differentiated in training mode')
    out = F._out(data, (x, gamma, beta), backward, 'h_batch_norm_eval')
    out.meta = _activated(meta, data, slope)
    return out


def _frozen_backward(s, x_data, mean, inv_std, gamma, ref, slope, want_gx, gamma_grad, beta_grad):
    """One ``srgan_h_frozen_norm_bwd`` launch on the (pre-masked) blocked ``s``: returns the raw gx = s * gamma * inv_std *
    mask(ref, slope) (None unless ``want_gx``); ``gamma_grad`` += inv_std * sum s (x - mean) and ``beta_grad`` += sum s where
    those fp32 buffers are given."""
    meta = s.meta
    data = _new(meta.n, meta.c, meta.h, meta.w, meta.code, s.data.device) if want_gx else None
    _call('srgan_h_frozen_norm_bwd', s.data.data_ptr(), _ptr(x_data), _ptr(mean), inv_std.data_ptr(), gamma.data.data_ptr(), _ptr(ref),
          float(slope), _ptr(data), _ptr(gamma_grad), _ptr(beta_grad), meta.n, meta.c, meta.h * meta.w, meta.code, F._stream())
    return data


def _frozen_scale(s, gamma, inv_std, ref, slope):
    """``s * gamma * inv_std * mask(ref, slope)`` per channel, recorded: the backward of ``batch_norm_frozen`` inside a recorded
    sweep (the gradient penalty).  Like epi 2 of ``_layer`` the result carries (ref, slope) as its mask: cotangents arrive
    masked alike, so its own backward never applies that mask again (slope ** 2 != slope) -- the gradient for ``s`` is the
    linearised forward, this scale with the mask ``s`` itself carries, and the gradient for gamma is inv_std * sum(u * s),
    straight into the arena; both from one launch.  Differentiating that once more (third order) is refused."""
    data = _frozen_backward(s, None, None, inv_std, gamma, ref, slope, True, None, None)
    s_meta = s.meta

    def backward(u, needs):
        if F.grad_enabled():
            raise NotImplementedError('blocked16.batch_norm_frozen is differentiable twice: a third-order use (a recorded sweep '
                                      'through the backward of its recorded backward) is not implemented')
        if needs[1]:
            _into_arena(gamma, 'batch-norm parameter')
        if not (needs[0] or needs[1]):
            return None, None
        back = _frozen_backward(u, s.data if needs[1] else None, None, inv_std, gamma, s_meta.mask_ref, s_meta.slope, needs[0],
                                gamma.grad_buffer if needs[1] else None, None)
        gs = None
        if needs[0]:
            gs = Var(back)
            gs.meta = s_meta
        return gs, None
    out = F._out(data, (s, gamma), backward, 'h_frozen_norm_scale')
    out.meta = s_meta.like(mask_ref=ref, slope=slope)
    return out


def batch_norm_frozen(x, mean, inv_std, gamma, beta, slope=1.0):
    """The norm with GIVEN statistics (``nn.BatchNorm2d``, which the reference freezes at every step: the norm layers of D /
    DNN) on a blocked tensor of any code: y = leaky((x - mean) * inv_std * gamma + beta, slope) -- the forward kernel of
    ``batch_norm_eval`` -- DIFFERENTIABLE TWICE.  A frozen norm is a per-channel affine map, so every derivative is "scale per
    channel, then mask" (``srgan_h_frozen_norm_bwd``): a plain sweep is ONE launch (gx and the gamma / beta gradients, the
    latter straight into the fp32 arena), a recorded sweep (the gradient penalty) records ``_frozen_scale``, whose own backward
    is again one launch; a third-order use raises.  The output is its own mask (``slope`` != 1), so the gradient arrives
    pre-masked.  The forward entry point refuses fewer than two values per channel: N * H * W == 1 raises ``ValueError``."""
    meta = _norm_tensors(x, gamma, beta)
    if meta.n * meta.h * meta.w < 2:
        raise ValueError(f'blocked16.batch_norm_frozen needs more than 1 value per channel (the forward entry point refuses '
                         f'M < 2), got input size {[meta.n, meta.c, meta.h, meta.w]}')
    data = _new(meta.n, meta.c, meta.h, meta.w, meta.code, x.data.device)
    slope = float(slope)
    _call('srgan_h_batch_norm_fwd', x.data.data_ptr(), mean.data.data_ptr(), inv_std.data.data_ptr(), gamma.data.data_ptr(),
          beta.data.data_ptr(), slope, data.data_ptr(), meta.n, meta.c, meta.h * meta.w, meta.code, F._stream())

    def backward(s, needs):
        if F.grad_enabled():                       # a recorded sweep: the gradient of x only, as a differentiable operation
            if needs[1] or needs[2]:
                _into_arena(None, 'batch-norm parameter')        # (a recorded sweep accumulates into nothing)
            return (_frozen_scale(s, gamma, inv_std.data, meta.mask_ref, meta.slope) if needs[0] else None), None, None
        for need, parameter in ((needs[1], gamma), (needs[2], beta)):
            if need:
                _into_arena(parameter, 'batch-norm parameter')
        if not any(needs):
            return None, None, None
        back = _frozen_backward(s, x.data if needs[1] else None, mean.data, inv_std.data, gamma, meta.mask_ref, meta.slope, needs[0],
                                gamma.grad_buffer if needs[1] else None, beta.grad_buffer if needs[2] else None)
        gx = None
        if needs[0]:
            gx = Var(back)
            gx.meta = meta                          # a pre-masked gradient of x
        return gx, None, None
    out = F._out(data, (x, gamma, beta), backward, 'h_batch_norm_frozen')
    out.meta = _activated(meta, data, slope)
    return out
