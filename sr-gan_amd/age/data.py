"""The age database in the layout the reference's preprocessors write (age/data.py:118-162,211-244):
``<directory>/meta.json`` -- a list of ``[image_name, age, gender]`` triples or of dicts with ``image_name`` and
``age`` -- and one RGB image of S x S pixels per name (an image file, or a ``.npy`` of uint8 ``[S, S, 3]``).
``age_datasets`` returns the reference's three splits (age/data.py:22-60, age/srgan.py:19-41) as datasets resident on the
device.  The downloads, the face cropping and the preprocessing itself stay out of scope."""
import json
import os

import numpy as np

from ..data import ResidentImageDataset, repeat_to_batch, split_slices


def read_image(path):
    """uint8 ``[3, S, S]`` of one stored image (the reference reads it with imageio and transposes, age/data.py:54-55)."""
    if path.endswith('.npy'):
        image = np.load(path)
    else:
        from PIL import Image
        with Image.open(path) as handle:
            image = np.asarray(handle.convert('RGB'))
    return np.ascontiguousarray(image.transpose((2, 0, 1)), dtype=np.uint8)


def age_datasets(directory, settings, device=None):
    """``(train, unlabeled, validation)``: the database shuffled by the permutation ``np.random.seed(seed);
    np.random.permutation(n)`` draws upstream (seed: ``settings.labeled_dataset_seed`` for all three; a private
    ``RandomState`` gives the same stream and leaves the process-wide one alone) and sliced ``[0 : labeled]``,
    ``[labeled : labeled + unlabeled]`` and ``[-validation :]``; a slice shorter than the batch is repeated element by
    element.  ``unlabeled_dataset_size`` None, for which upstream's age code has no value, ends the unlabeled slice at
    the validation tail as the driving application does."""
    with open(os.path.join(directory, 'meta.json')) as json_file:
        entries = json.load(json_file)
    names = np.array([entry['image_name'] if isinstance(entry, dict) else entry[0] for entry in entries])
    ages = np.array([entry['age'] if isinstance(entry, dict) else entry[1] for entry in entries])
    permutation = np.random.RandomState(settings.labeled_dataset_seed).permutation(len(names))
    names, ages = names[permutation], ages[permutation]
    frames = {}

    def dataset(part):
        part_names, part_ages = repeat_to_batch(np.array(names[part]), np.array(ages[part], dtype=np.float32),
                                                settings.batch_size)
        for name in part_names:
            if name not in frames:
                frames[name] = read_image(os.path.join(directory, name))
        return ResidentImageDataset([frames[name] for name in part_names], part_ages, device=device, names=part_names)

    return tuple(dataset(part) for part in split_slices(
        settings.labeled_dataset_size, settings.validation_dataset_size, settings.unlabeled_dataset_size, False))
