"""Layer containers.  They subclass the torch.nn modules the reference uses, so construction order,
default initialisation (same random stream) and ``state_dict`` keys are the reference's; only ``forward``
is replaced: it takes and returns tape ``Var``s and launches HIP kernels.  torch.nn here is a parameter
container / checkpoint format, not a compute path.
"""
import contextlib

import numpy as np
import torch
from torch import nn

from . import functional as F
from .tape import Var
from .utility import current_device


def parameter_var(parameter):
    """The persistent graph leaf of a parameter (rebuilt if the parameter's storage moved)."""
    var = getattr(parameter, '_srgan_var', None)
    if var is None or var.data.data_ptr() != parameter.data.data_ptr():
        var = F.leaf(parameter.data, requires_grad=parameter.requires_grad)
        if var.data.data_ptr() != parameter.data.data_ptr():
            raise RuntimeError('parameters must be contiguous fp32 device tensors (call flatten_parameters first)')
        parameter._srgan_var = var
    var.grad_buffer = parameter.grad
    return var


P = parameter_var


class Conv2d(nn.Conv2d):
    def forward(self, x):
        return F.conv2d(x, P(self.weight), P(self.bias) if self.bias is not None else None, self.stride, self.padding)


class ConvTranspose2d(nn.ConvTranspose2d):
    def forward(self, x):
        return F.conv_transpose2d(x, P(self.weight), P(self.bias) if self.bias is not None else None, self.stride,
                                  self.padding)


class Linear(nn.Linear):
    def forward(self, x):
        return F.linear(x, P(self.weight), P(self.bias) if self.bias is not None else None)


class BatchNorm2d(nn.BatchNorm2d):
    """Always evaluated with the running statistics: the reference freezes every batch-norm layer at each
    step (srgan.py:261,276,538-542), so training mode never updates or uses batch statistics.  gamma / beta
    are still trained.  One fused kernel: y = (x - mean) * rsqrt(var + eps) * gamma + beta.  A tensor in the blocked layout
    (``blocked16``, any code) takes ``_forward_blocked``: differentiable twice, ``slope`` fuses a following leaky-ReLU."""

    def _inverse_std(self):
        key = (id(self.running_var), self.running_var._version, id(self.running_mean), self.running_mean._version)
        cached = getattr(self, '_inv_std_cache', None)
        if cached is None or cached[0] != key:
            variance = self.running_var.detach().contiguous()
            if cached is not None and cached[1].data.shape == variance.shape and cached[1].data.device == variance.device:
                # New statistics (load_state_dict, load_models): refreshed IN PLACE.  The grouped launch tables of
                # fused.py and a captured HIP graph hold the raw device pointers of these two tensors.
                inv, mean = cached[1], cached[2]
                F._unary_raw(F.U_RSQRT, F._unary_raw(F.U_AFFINE, variance, 1.0, self.eps, out=inv.data), out=inv.data)
                mean.data.copy_(self.running_mean.detach())
            else:
                inv = Var(F._unary_raw(F.U_RSQRT, F._unary_raw(F.U_AFFINE, variance, 1.0, self.eps)))
                mean = Var(self.running_mean.detach().clone().contiguous())      # a copy we own: its address never moves
            cached = (key, inv, mean)
            self._inv_std_cache = cached
        return cached[1], cached[2]

    def forward(self, x, relu=False, slope=1.0):
        if x.meta is not None:
            return self._forward_blocked(x, 0.0 if relu else slope)
        inv_std, mean = self._inverse_std()
        out = F.batch_norm_eval(x, mean, inv_std, P(self.weight), P(self.bias), relu=relu)
        return out if relu or slope == 1.0 else F.leaky_relu(out, slope)

    def _forward_blocked(self, x, slope):
        """The frozen layer on a tensor in the blocked layout: the running statistics whatever the mode, the buffers untouched;
        the cached tensors of ``_inverse_std`` keep their addresses when the statistics are reloaded (a captured graph stays
        valid)."""
        from . import blocked16 as B
        inv_std, mean = self._inverse_std()
        return B.batch_norm_frozen(x, mean, inv_std, P(self.weight), P(self.bias), slope=slope)


class BatchStatNorm2d(BatchNorm2d):
    """Batch-norm that is NOT frozen: in training mode it normalises with the statistics of the batch and updates the
    running statistics, as ``torch.nn.BatchNorm2d`` does -- the norm layers of the DCGAN generators, which the reference
    leaves in training mode (srgan.py:171; only D and DNN are frozen, :261,276).  Same parameters, buffers and
    ``state_dict`` keys as ``BatchNorm2d``; in eval mode it IS ``BatchNorm2d``.  ``slope`` fuses the leaky-ReLU that
    follows the layer into the pass (1: none)."""

    def _statistics_changed(self):
        """The running buffers are written by a kernel through raw pointers, which torch's version counters do not see:
        bump them, so that ``_inverse_std`` refreshes its cached tensors (in place) at the next eval-mode forward."""
        for buffer in (self.running_mean, self.running_var, self.num_batches_tracked):
            if buffer is not None:
                torch.autograd.graph.increment_version(buffer)

    def train(self, mode=True):
        if self.training and not mode:      # (a replayed HIP graph trains without passing through ``forward``)
            self._statistics_changed()
        return super().train(mode)

    def forward(self, x, relu=False, slope=1.0):
        if x.meta is not None:
            return self._forward_blocked(x, 0.0 if relu else slope)
        if not self.training:
            out = super().forward(x, relu=relu)
            return out if relu or slope == 1.0 else F.leaky_relu(out, slope)
        if relu:
            slope = 0.0
        if not self.track_running_stats or self.running_mean is None:
            raise NotImplementedError('BatchStatNorm2d needs track_running_stats=True')
        out = F.batch_norm_train(x, P(self.weight), P(self.bias), self.running_mean, self.running_var, self.momentum, self.eps,
                                 slope=slope, num_batches_tracked=self.num_batches_tracked)
        self._statistics_changed()
        return out

    def _forward_blocked(self, x, slope):
        """The same layer on a tensor in the blocked layout (``blocked16``, any code): training mode differentiable to first
        order, eval mode -- the forward kernel with the cached tensors of ``_inverse_std`` -- forward only."""
        from . import blocked16 as B
        if not self.training:
            inv_std, mean = self._inverse_std()
            return B.batch_norm_eval(x, mean, inv_std, P(self.weight), P(self.bias), slope=slope)
        if not self.track_running_stats or self.running_mean is None:
            raise NotImplementedError('BatchStatNorm2d needs track_running_stats=True')
        out = B.batch_norm_train(x, P(self.weight), P(self.bias), self.running_mean, self.running_var, self.momentum, self.eps,
                                 slope=slope, num_batches_tracked=self.num_batches_tracked)
        self._statistics_changed()
        return out


class ReLU(nn.Module):
    def __init__(self, inplace=False):
        super().__init__()

    def forward(self, x):
        return F.relu(x)


class MaxPool2d(nn.Module):
    def __init__(self, kernel_size, stride=None, padding=0):
        super().__init__()
        self.kernel_size, self.stride, self.padding = kernel_size, stride or kernel_size, padding

    def forward(self, x):
        return F.max_pool2d(x, self.kernel_size, self.stride, self.padding)


class AvgPool2d(nn.Module):
    def __init__(self, kernel_size, stride=None):
        super().__init__()
        self.kernel_size, self.stride = kernel_size, stride or kernel_size

    def forward(self, x):
        return F.avg_pool2d(x, self.kernel_size, self.stride)


def draw_state(seed, iteration):
    """The state of ``srgan_random_fill`` on the device: int32 x 4 holding the words {seed_lo, seed_hi, iteration, 0} of a
    64-bit seed and a 32-bit iteration count (both taken modulo their width)."""
    seed = int(seed) & (2 ** 64 - 1)
    words = np.array([seed & 0xffffffff, seed >> 32, int(iteration) & 0xffffffff, 0], dtype=np.uint32)
    return torch.from_numpy(words.view(np.int32)).to(current_device())


class DropoutStream:
    """Which mask a dropout call of one network gets.  Two parts: a device state ``uint32[4] = {seed_lo, seed_hi,
    iteration, 0}`` (the state of ``srgan_random_fill``, created at first use) and a host-side call counter.  A
    training-mode forward of a dropout layer takes ``draw = base + counter++``; the owner resets the counter when the
    network's step of an iteration begins (``begin_step``) and advances the state once per iteration (``advance``), on the
    stream the step runs on, behind the last launch that reads it.  Program order then fixes the draw ids: a captured HIP
    graph bakes in the ids of the eager iterations and replays as the next iteration each time.

    A pass whose place in the host's program order depends on a side-stream setting (the penalty chain's forward, the
    generator step's D(unlabeled)) numbers its calls in a ``section`` of its own -- a quarter of the range each, section 0 is
    the rest of the step -- so that a run draws the same masks with the side streams on and off."""

    SECTIONS = 4

    def __init__(self, base, seed=0, iteration=0, draws=0x10000):
        self.base, self.draws = int(base), int(draws)
        self.seed, self.iteration = int(seed) & (2 ** 64 - 1), int(iteration) & 0xffffffff
        self.counter = 0                  # the next id of the section in progress, relative to base
        self.limit = self.draws // self.SECTIONS
        self._resume = {}                 # section -> where its numbering goes on when it is entered again in this step
        self._state = None

    def state(self):
        if self._state is None:
            self._state = draw_state(self.seed, self.iteration)
        return self._state

    def begin_step(self):
        self.counter, self.limit = 0, self.draws // self.SECTIONS
        self._resume = {}

    @contextlib.contextmanager
    def section(self, index):
        if not 0 < index < self.SECTIONS:
            raise ValueError(f'dropout section {index} outside 1 .. {self.SECTIONS - 1}')
        size = self.draws // self.SECTIONS
        outer = self.counter, self.limit
        self.counter, self.limit = self._resume.get(index, index * size), (index + 1) * size
        try:
            yield self
        finally:
            self._resume[index] = self.counter
            self.counter, self.limit = outer

    def next_draw(self):
        if self.counter >= self.limit:
            raise RuntimeError(f'more than {self.draws // self.SECTIONS} dropout calls in one section of a step: the network\'s '
                               'range of draw ids is used up')
        draw = self.base + self.counter
        self.counter += 1
        return self.state(), draw

    def advance(self):
        F.random_advance(self.state())


class Dropout(nn.Module):
    """Inverted dropout with a mask regenerated on the device (``F.dropout``): nothing is stored, the backward and the
    gradient penalty's double backward draw the same mask again.  In eval mode, or with ``p == 0``, the input itself is
    returned and nothing is launched.  In training mode the layer asks its network's ``DropoutStream`` (``dropout_stream``,
    set by ``attach_dropout_stream``) for the state and the draw id of this call."""

    def __init__(self, p=0.5):
        super().__init__()
        if not 0.0 <= p <= 1.0:
            raise ValueError(f'dropout probability has to be between 0 and 1, but got {p}')
        self.p = float(p)
        self.dropout_stream = None

    def extra_repr(self):
        return f'p={self.p}'

    def forward(self, x):
        if not self.training or self.p == 0.0:
            return x
        if x.meta is not None:
            raise NotImplementedError('nn.Dropout on a blocked (16-bit / blocked-fp32) tensor is not implemented')
        if self.dropout_stream is None:
            raise RuntimeError('nn.Dropout in training mode needs its network\'s dropout stream (nn.attach_dropout_stream)')
        state, draw = self.dropout_stream.next_draw()
        return F.dropout(x, self.p, draw, state)


def active_dropout_layers(module):
    """The dropout layers of ``module`` that do something in training mode (``p > 0``)."""
    return [layer for layer in module.modules() if isinstance(layer, Dropout) and layer.p > 0.0] if module is not None else []


def attach_dropout_stream(module, stream):
    """Hands ``stream`` to every active dropout layer of ``module``; returns how many there are."""
    layers = active_dropout_layers(module)
    for layer in layers:
        layer.dropout_stream = stream
    return len(layers)


Sequential = nn.Sequential
Module = nn.Module
ModuleList = nn.ModuleList


class ParameterArena:
    """All parameters of one network in ONE contiguous device buffer, with a parallel gradient buffer.

    MI355X-first layout: Adam is a single streaming kernel over the arena, ``zero_grad`` one memset, and the
    data-parallel gradient exchange a handful of large RCCL all-reduces instead of one per tensor.  The
    module's Parameters become views into the arena (``state_dict`` is unaffected)."""

    def __init__(self, module, device):
        parameters = [p for p in module.parameters()]
        self.sizes = [p.numel() for p in parameters]
        # keep every tensor 16-byte aligned inside the arena (float4 kernels)
        self.offsets, total = [], 0
        for size in self.sizes:
            self.offsets.append(total)
            total += (size + 3) // 4 * 4
        self.numel = total
        self.data = torch.zeros(total, dtype=torch.float32, device=device)
        self.grad = torch.zeros(total, dtype=torch.float32, device=device)
        self.parameters = parameters
        self.version = 0          # bumped by every optimizer update (raw-pointer writes torch's version counters do not see)
        self.shadows = []         # blocked16.Shadow objects: 16-bit operand forms of these weights, refreshed behind an update
        with torch.no_grad():
            for p, offset, size in zip(parameters, self.offsets, self.sizes):
                view = self.data[offset:offset + size].view(p.shape)
                view.copy_(p.data)
                p.data = view
                p.grad = self.grad[offset:offset + size].view(p.shape)
                p._srgan_var = None
                p._srgan_arena = self
        for buffer_owner in module.modules():      # move buffers (batch-norm statistics) as well
            for name, buffer in list(buffer_owner._buffers.items()):
                if buffer is not None:
                    buffer_owner._buffers[name] = buffer.to(device)

    def zero_grad(self):
        F.fill_(self.grad, 0.0)

    def gradients_into_alternate(self):
        """Context manager: while it is active, every gradient of this network accumulates into a SECOND buffer of the
        arena's size (returned; allocated on first use, zeroed by the caller) instead of ``self.grad`` -- for a backward
        chain that runs on another stream concurrently with one that accumulates into ``self.grad`` (the accumulations are
        read-modify-write kernels, not atomics).  The caller adds the buffer to ``self.grad`` after joining the streams."""
        import contextlib
        if getattr(self, '_alternate', None) is None:
            self._alternate = torch.empty_like(self.grad)
            self._alternate_views = [self._alternate[offset:offset + size].view(p.shape)
                                     for p, offset, size in zip(self.parameters, self.offsets, self.sizes)]
            self._main_views = [self.grad[offset:offset + size].view(p.shape)
                                for p, offset, size in zip(self.parameters, self.offsets, self.sizes)]

        def point_at(views):
            for p, view in zip(self.parameters, views):
                p.grad = view
                var = getattr(p, '_srgan_var', None)
                if var is not None:
                    var.grad_buffer = view

        @contextlib.contextmanager
        def redirected():
            point_at(self._alternate_views)
            try:
                yield self._alternate
            finally:
                point_at(self._main_views)
        return redirected()

    def rebind(self):
        """Re-point ``p.grad`` at the arena (torch utilities such as zero_grad(set_to_none) may drop it)."""
        for p, offset, size in zip(self.parameters, self.offsets, self.sizes):
            p.grad = self.grad[offset:offset + size].view(p.shape)


def flatten_parameters(module, device):
    arena = ParameterArena(module, device)
    module._srgan_arena = arena
    return arena


class frozen_parameters:
    """Context manager: the module's parameters do not receive gradients (used for the discriminator during
    the generator update -- the reference computes and then discards those gradients, srgan.py:304,278)."""

    def __init__(self, module):
        self.vars = [parameter_var(p) for p in module.parameters()]

    def __enter__(self):
        self.previous = [v.requires_grad for v in self.vars]
        for v in self.vars:
            v.requires_grad = False

    def __exit__(self, *exc):
        for v, flag in zip(self.vars, self.previous):
            v.requires_grad = flag
