"""The steering-angle database in the layout the reference's preprocessor writes (driving/data.py:113-126):
``<directory>/meta.pkl`` -- a pickled pandas frame, column 0 the ``.jpg`` names, column 1 the angles -- and one
``<name>.npy`` per frame, float64 ``[3, S, S]`` in the 0..255 range.  ``driving_datasets`` returns the reference's three
splits (driving/data.py:22-51, driving/srgan.py:17-40) as datasets resident on the device.  The download and the
preprocessing itself stay out of scope."""
import os

import numpy as np

from ..data import ResidentImageDataset, repeat_to_batch, split_slices


def driving_datasets(directory, settings, device=None):
    """``(train, unlabeled, validation)``: the database shuffled by ``sklearn.utils.shuffle(meta, random_state=
    settings.labeled_dataset_seed)`` -- the same seed for all three, as upstream -- and sliced ``[0 : labeled]``,
    ``[labeled + validation : labeled + validation + unlabeled]`` (``unlabeled_dataset_size`` None: up to the validation
    tail) and ``[-validation :]``; a slice shorter than the batch is repeated element by element."""
    import pandas
    import sklearn.utils
    meta = pandas.read_pickle(os.path.join(directory, 'meta.pkl'))
    meta = sklearn.utils.shuffle(meta, random_state=settings.labeled_dataset_seed)
    names, angles = meta.iloc[:, 0].values, meta.iloc[:, 1].values
    frames = {}

    def dataset(part):
        part_names, part_angles = repeat_to_batch(np.array(names[part]), np.array(angles[part], dtype=np.float32),
                                                  settings.batch_size)
        for name in part_names:
            if name not in frames:
                frames[name] = np.load(os.path.join(directory, name.replace('.jpg', '.npy')))
        return ResidentImageDataset([frames[name] for name in part_names], part_angles, device=device, names=part_names)

    return tuple(dataset(part) for part in split_slices(
        settings.labeled_dataset_size, settings.validation_dataset_size, settings.unlabeled_dataset_size, True))
