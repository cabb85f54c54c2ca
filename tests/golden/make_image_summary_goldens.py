"""Generate tests/golden/g17_image_summaries.npz by running the UNMODIFIED upstream reference on CPU.

Test infrastructure only, like make_goldens.py: it needs the reference checkout and matplotlib and never travels to the GPU box;
the emitted fixture holds data only.  Recorded: the reference's own ``CrowdExperiment.convert_density_maps_to_heatmaps``
(crowd/srgan.py:193-217) on three pairs of 16 x 16 maps with ``image_patch_size = 16`` -- the stand-in for the removed
``scipy.misc.imresize`` is the identity at equal sizes, the only case recorded -- and matplotlib's 256 x 3 inferno table.
torchvision is not installed, so ``make_grid`` is not recorded (tests/image_summaries_reference.py restates it and
test_image_summaries_cpu.py pins the restatement by hand-written answers).  Usage::

    python tests/golden/make_image_summary_goldens.py
"""
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _refstubs  # noqa: E402

_refstubs.install()

import matplotlib  # noqa: E402
import scipy.misc  # noqa: E402
import torch  # noqa: E402

import image_summaries_reference as R  # noqa: E402

SIZE = 16


def imresize_identity(array, size, mode=None):
    assert tuple(array.shape) == tuple(size) and mode == 'F'
    return np.asarray(array, dtype=np.float32)


def pairs():
    generator = np.random.RandomState(17)
    random_label = generator.uniform(0.05, 3.0, size=(SIZE, SIZE)).astype(np.float32)
    random_predicted = generator.uniform(0.01, 4.0, size=(SIZE, SIZE)).astype(np.float32)
    constant = np.full((SIZE, SIZE), 0.75, dtype=np.float32)
    heads = np.zeros((SIZE, SIZE), dtype=np.float32)
    heads[3, 5] = heads[11, 12] = 1.0
    heads_predicted = generator.uniform(-0.2, 0.6, size=(SIZE, SIZE)).astype(np.float32)
    return {'random': (random_label, random_predicted), 'constant': (constant, constant.copy()),
            'heads': (heads, heads_predicted)}


def main():
    scipy.misc.imresize = imresize_identity
    from crowd.srgan import CrowdExperiment
    experiment = SimpleNamespace(settings=SimpleNamespace(image_patch_size=SIZE))
    table = np.asarray(matplotlib.colormaps['inferno'].colors, dtype=np.float32)
    assert table.shape == (256, 3) and len({tuple(row) for row in table.tolist()}) == 256
    out = {'inferno': table, 'size': np.array(SIZE)}
    for name, (label, predicted) in pairs().items():
        label_heatmap, predicted_heatmap = CrowdExperiment.convert_density_maps_to_heatmaps(
            experiment, torch.from_numpy(label), torch.from_numpy(predicted))
        heatmaps = np.stack([label_heatmap.numpy(), predicted_heatmap.numpy()])
        assert heatmaps.shape == (2, 3, SIZE, SIZE) and heatmaps.dtype == np.float32
        out[f'{name}/label'], out[f'{name}/predicted'], out[f'{name}/heatmaps'] = label, predicted, heatmaps
        # the restatement against the reference, under the rule of the tests; and the rule's cap holds for the reference alone
        _, _, entries, scaled = R.density_heatmaps(label[None], predicted[None, None], SIZE, table)
        recorded = R.entries_from_colours(heatmaps, table)
        R.check_entries(entries[0], recorded, scaled[0], name)
        near = R.near_an_integer(scaled[0]).reshape(2, -1).mean(axis=1)
        print(f'{name}: {int((entries[0] != recorded).sum())} entries differ from the restatement; '
              f'{near.max():.4f} of a tile within 1e-3 of an integer')
        if name == 'random':
            assert near.max() <= 0.01
    np.savez_compressed(os.path.join(HERE, 'g17_image_summaries.npz'), **out)
    print('wrote g17_image_summaries.npz')


if __name__ == '__main__':
    main()
