"""Generate tests/golden/g16_tiny_dcgan_batch_norm*.npz by running the UNMODIFIED upstream reference on CPU with its
``batch_norm`` switch on.

Test infrastructure only, like make_goldens.py (whose helpers and reference stubs it uses; nothing here travels to the GPU
box).  The reference binds the switch as a default argument when ``age/models.py`` is imported (:13,16,24), so setting the
module attribute does nothing; the only way to turn it on without editing the reference is to replace the defaults of its
two stage builders before the networks are constructed.  Usage::

    python tests/golden/make_batch_norm_goldens.py

The fixture is the g5 configuration (conv_dim 8, 32x32, B = 4, the g5 multipliers and the x3 discriminator scale, so the
gradient penalty is active), two steps: initial and final ``state_dict``s of G, D and DNN INCLUDING the batch-norm buffers
(``running_mean``, ``running_var``, ``num_batches_tracked``), the batches, the three random draws, every logged loss, and
the Adam moments of G; G's batch-norm buffers are also kept after EACH step (``s<step>/G_buffers/...``), so that the
first step's can be recomputed from the initial weights alone.  The arrays add up to 2.5 MB, so they are written as three
files that each stay under the limit for a committed file: ``g16_tiny_dcgan_batch_norm.npz`` (configuration, initial
states, batches, draws, losses), ``..._final.npz`` (the final states) and ``..._adam.npz`` (G's Adam moments).
G stays in training mode (reference srgan.py:171) -- batch statistics, running statistics updated twice per step
(srgan.py:290,302) -- while D and DNN are frozen at every step (srgan.py:261,276).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as M  # noqa: E402  (installs the stubs, imports the reference)

import torch  # noqa: E402


def g16_tiny_dcgan_batch_norm():
    import age.models as models
    saved = models.transpose_convolution.__defaults__, models.convolution.__defaults__
    models.transpose_convolution.__defaults__ = (2, 1, True)      # (stride, pad, bn)
    models.convolution.__defaults__ = (2, 1, True)
    try:
        def builders():
            return (models.Generator(image_size=32, conv_dim=8), models.Discriminator(image_size=32, conv_dim=8),
                    models.Discriminator(image_size=32, conv_dim=8))

        experiment = M._image_experiment(builders, batch_size=4, multipliers={
            'matching_loss_multiplier': 1e2, 'contrasting_loss_multiplier': 1e1, 'gradient_penalty_multiplier': 1e2})
    finally:
        models.transpose_convolution.__defaults__, models.convolution.__defaults__ = saved
    norms = [m for m in experiment.G.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert len(norms) == 3 and sum(isinstance(m, torch.nn.BatchNorm2d) for m in experiment.D.modules()) == 3
    with torch.no_grad():
        for p in experiment.D.parameters():
            p.mul_(3.0)
    out = {'batch_size': np.array(4), 'image_size': np.array(32), 'conv_dim': np.array(8), 'd_scale': np.array(3.0)}
    for name in ('D', 'DNN', 'G'):
        out.update(M.state_arrays(f'init/{name}', getattr(experiment, name)))
    generator = torch.Generator().manual_seed(5)
    batches = []
    for step in range(2):
        x, u = M._uniform_images(generator, 4, 32), M._uniform_images(generator, 4, 32)
        y = torch.rand(4, generator=generator) * 85 + 10
        batches.append((x, y, u))
        out[f's{step}/x'], out[f's{step}/y'], out[f's{step}/u'] = M.np32(x), M.np32(y), M.np32(u)
    for step, (x, y, u) in enumerate(batches):          # (run_recorded_steps, plus G's buffers after every step)
        experiment.dnn_training_step(x, y, step)
        out[f's{step}/dnn_loss'] = np.array(M.last_scalars(experiment.dnn_summary_writer)['Discriminator/Labeled Loss'])
        recorder = M.Recorder(experiment)
        with recorder.recording():
            experiment.gan_training_step(x, y, u, step)
        scalars = M.last_scalars(experiment.gan_summary_writer)
        for tag, key in M.GAN_TAGS.items():
            out[f's{step}/{key}'] = np.array(scalars[tag])
        out[f's{step}/z_d'], out[f's{step}/z_g'], out[f's{step}/alpha'] = recorder.z_d, recorder.z_g, recorder.alpha
        out[f's{step}/gradient_norm'] = M.np32(experiment.gradient_norm)
        out.update({f's{step}/G_buffers/{k}': v.detach().cpu().numpy().copy() for k, v in experiment.G.named_buffers()})
    assert all(m.training for m in norms), 'the reference never freezes G'
    assert float(out['s0/gradient_penalty']) > 1.0 and float(out['s1/gradient_penalty']) > 1.0, 'penalty inactive'
    final = {}
    for name in ('D', 'DNN', 'G'):
        final.update(M.state_arrays(f'final/{name}', getattr(experiment, name)))
    assert int(final['final/G/layer1.1.num_batches_tracked']) == 4 and int(final['final/D/layer2.1.num_batches_tracked']) == 0
    M.save('g16_tiny_dcgan_batch_norm', **out)
    M.save('g16_tiny_dcgan_batch_norm_final', **final)
    M.save('g16_tiny_dcgan_batch_norm_adam', **M.adam_arrays('final_adam/G', experiment.G, experiment.g_optimizer))


if __name__ == '__main__':
    g16_tiny_dcgan_batch_norm()
