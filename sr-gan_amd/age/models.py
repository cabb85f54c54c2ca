"""DCGAN generator / discriminator on HIP kernels (surface of reference age/models.py:32-80, identical to
driving/models.py and, for the generator, crowd/models.py:127-147): same module names, construction order (hence the same
initial weights from ``seed_all(0)``) and ``state_dict`` keys.  ``image_size`` may be an (H, W) pair for the rectangular
driving frames; a square int is the reference graph."""
from .. import functional as F
from .. import nn
from ..utility import seed_all

# The reference's module-level switch (age/models.py:13).  Read when a stage is BUILT (``bn=None``), so setting it takes
# effect; ``Generator(batch_norm=...)`` / ``Discriminator(batch_norm=...)`` override it per instance
# (``settings.generator_batch_norm`` / ``settings.discriminator_batch_norm``).
batch_norm = False
LEAK = 0.05


def _blocked_stack_ok(network):
    """The blocked path has the reference configuration -- no batch-norm inside the stages (age/models.py:13) -- or, for a
    network built with ``blocked_batch_norm`` (the generator), stages ``[ConvTranspose2d, BatchStatNorm2d]`` (the norm with
    batch statistics on blocked tensors, ``blocked16.batch_norm_train``), or, for one built with ``blocked_frozen_norm`` (the
    discriminator), stages ``[Conv2d, BatchNorm2d]`` with exactly the frozen class (``blocked16.batch_norm_frozen``)."""
    norms = getattr(network, 'blocked_batch_norm', False)
    frozen = getattr(network, 'blocked_frozen_norm', False)
    return all(len(stage) == 1 or
               (norms and len(stage) == 2 and isinstance(stage[0], nn.ConvTranspose2d) and isinstance(stage[1], nn.BatchStatNorm2d)) or
               (frozen and len(stage) == 2 and isinstance(stage[0], nn.Conv2d) and type(stage[1]) is nn.BatchNorm2d)
               for name, stage in network.named_children())


def _pair(value):
    return (value, value) if isinstance(value, int) else tuple(value)


def _stage(layer_class, norm_class, c_in, c_out, k_size, stride, pad, bn):
    """``Sequential(layer[, norm])`` -- the reference wraps every layer like this, so keys read ``layerN.0.weight``."""
    if bn is None:
        bn = batch_norm
    return nn.Sequential(*([layer_class(c_in, c_out, k_size, stride, pad)] + ([norm_class(c_out)] if bn else [])))


def transpose_convolution(c_in, c_out, k_size, stride=2, pad=1, bn=None):
    """The generator's stage: its norm uses batch statistics in training mode (the reference never freezes G, srgan.py:171)."""
    return _stage(nn.ConvTranspose2d, nn.BatchStatNorm2d, c_in, c_out, k_size, stride, pad, bn)


def convolution(c_in, c_out, k_size, stride=2, pad=1, bn=None):
    """The discriminator's stage: its norm is frozen (the reference freezes D and DNN at every step, srgan.py:261,276)."""
    return _stage(nn.Conv2d, nn.BatchNorm2d, c_in, c_out, k_size, stride, pad, bn)


def _seed_kernel(image_size):
    height, width = _pair(image_size)
    return int(height / 16), int(width / 16)      # four stride-2 stages between the 1x1 code and the image


class Generator(nn.Module):
    """z -> ``fc``: convT(k = S/16) -> ``layer1..3``: convT k4 s2 p1 + leaky 0.05 -> ``layer4``: convT k4 s2 p1 -> tanh."""

    def __init__(self, z_dim=256, image_size=128, conv_dim=64, batch_norm=None, blocked_batch_norm=False):
        seed_all(0)
        super().__init__()
        # with norm layers, stay on the blocked data path under F.storage_dtype (settings.blocked_batch_norm; off: the fp32 graph)
        self.blocked_batch_norm = bool(blocked_batch_norm)
        widths = (conv_dim * 8, conv_dim * 4, conv_dim * 2, conv_dim, 3)
        self.fc = transpose_convolution(z_dim, widths[0], _seed_kernel(image_size), 1, 0, bn=False)
        for index in range(1, 5):
            setattr(self, f'layer{index}', transpose_convolution(widths[index - 1], widths[index], 4,
                                                                 bn=False if index == 4 else batch_norm))
        self.input_size = z_dim

    def forward(self, z):
        if F.STORAGE_DTYPE and z.meta is None and _blocked_stack_ok(self):
            from ..blocked16 import active_code
            return self._forward_blocked(z, active_code())
        out = self.fc(F.view(z, (z.shape[0], z.shape[1], 1, 1)))
        for stage in (self.layer1, self.layer2, self.layer3):
            if len(stage) == 2:       # convT -> norm with the leaky-ReLU fused into the norm's pass
                out = stage[1](stage[0](out), slope=LEAK)
            else:
                out = F.leaky_relu(stage(out), LEAK)
        return F.tanh(self.layer4(out))

    def _forward_blocked(self, z, code):
        """The same graph on the 16-bit data path (``blocked16``): the code and every feature map bf16 / fp16 in the blocked
        layout, ``leaky_relu(convT(x))`` one kernel per stage, fp32 again for the images (tanh on the 3-channel result)."""
        from .. import blocked16 as B
        if code == 0:       # fp32 blocked: the seed layer on the fp32 kernels (one GEMM over its 26-137 M weights), then the stages
            h = B.pack(self.fc(F.view(z, (z.shape[0], z.shape[1], 1, 1))), 0)
        else:
            h = B.seed_conv_transpose(B.pack(F.view(z, (z.shape[0], z.shape[1])), code), self.fc[0])
        for stage in (self.layer1, self.layer2, self.layer3):
            if len(stage) == 2:       # convT -> norm with the leaky-ReLU fused into the norm's pass, all on blocked tensors
                h = stage[1](B.conv_transpose4x4s2(h, stage[0]), slope=LEAK)
            else:
                h = B.conv_transpose4x4s2(h, stage[0], slope=LEAK)
        return F.tanh(B.unpack(B.conv_transpose4x4s2(h, self.layer4[0])))


class Discriminator(nn.Module):
    """``layer1..4``: conv k4 s2 p1 + leaky 0.05; ``features`` = the flattened result; ``layer5``: conv k = S/16 -> outputs."""

    def __init__(self, image_size=128, conv_dim=64, number_of_outputs=1, batch_norm=None, blocked_frozen_norm=False):
        seed_all(0)
        super().__init__()
        # with (frozen) norm layers, stay on the blocked data path under F.storage_dtype (settings.blocked_frozen_norm; off: the
        # fp32 graph)
        self.blocked_frozen_norm = bool(blocked_frozen_norm)
        self.number_of_outputs = number_of_outputs
        widths = (3, conv_dim, conv_dim * 2, conv_dim * 4, conv_dim * 8)
        for index in range(1, 5):
            setattr(self, f'layer{index}', convolution(widths[index - 1], widths[index], 4,
                                                       bn=False if index == 1 else batch_norm))
        self.layer5 = convolution(widths[4], number_of_outputs, _seed_kernel(image_size), 1, 0, False)
        self.features = None

    def forward(self, x):
        if F.STORAGE_DTYPE and x.meta is None and _blocked_stack_ok(self):
            from ..blocked16 import active_code
            return self._forward_blocked(x, active_code())
        out = x
        for stage in (self.layer1, self.layer2, self.layer3, self.layer4):
            out = F.leaky_relu(stage(out), LEAK)
        self.features = F.flatten2d(out)
        scores = self.layer5(out)
        return F.view(scores, (-1,) if self.number_of_outputs == 1 else (-1, self.number_of_outputs))

    def _forward_blocked(self, x, code):
        """The same graph on the 16-bit data path (``blocked16``): every ``leaky_relu(conv(x))`` stage one kernel on bf16 / fp16
        tensors in the blocked layout -- with a frozen norm the convolution, then the norm's pass with the leaky-ReLU fused into
        it; ``features`` (reference order: the NCHW flattening) and the scores leave as fp32."""
        from .. import blocked16 as B
        h = B.pack(x, code)
        for stage in (self.layer1, self.layer2, self.layer3, self.layer4):
            if len(stage) == 2:       # (called as a module, so that forward hooks see the blocked tensors)
                h = stage[1](B.conv4x4s2(h, stage[0]), slope=LEAK)
            else:
                h = B.conv4x4s2(h, stage[0], slope=LEAK)
        trunk = B.unpack(h)
        self.features = F.flatten2d(trunk)
        # the full-plane convolution = a linear map over the flattened trunk: 16-bit through the blocked order's shadow, fp32
        # blocked through the fp32 kernels on the unpacked trunk
        scores = self.layer5(trunk) if code == 0 else B.unpack(B.linear(B.flatten(h), self.layer5[0]))
        return F.view(scores, (-1,) if self.number_of_outputs == 1 else (-1, self.number_of_outputs))
