"""The two tiny databases of tests/golden/g15_image_databases.npz written back to disk in the reference's layouts
(shared by the CPU and the GPU tests of the resident image datasets)."""
import os
from types import SimpleNamespace

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g15_image_databases.npz')
PARTS = ('train', 'unlabeled', 'validation')


def golden():
    return np.load(GOLDEN)


def settings_for(fixture, tag):
    labeled, validation, unlabeled, batch, seed = (int(v) for v in fixture['settings/' + tag])
    return SimpleNamespace(labeled_dataset_size=labeled, validation_dataset_size=validation,
                           unlabeled_dataset_size=None if unlabeled < 0 else unlabeled, batch_size=batch,
                           labeled_dataset_seed=seed)


def write_driving_database(fixture, directory):
    """meta.pkl (through the installed pandas) and one float64 .npy per frame."""
    import pandas
    os.makedirs(directory, exist_ok=True)
    names = fixture['driving/names']
    pandas.DataFrame({0: names, 1: fixture['driving/angles']}).to_pickle(os.path.join(directory, 'meta.pkl'))
    for name, frame in zip(names, fixture['driving/frames']):
        np.save(os.path.join(directory, str(name).replace('.jpg', '.npy')), frame)
    return str(directory)


def write_age_database(fixture, directory):
    """meta.json as recorded and one PNG per image."""
    from PIL import Image
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, 'meta.json'), 'w') as json_file:
        json_file.write(str(fixture['age/meta_json']))
    for name, image in zip(fixture['age/names'], fixture['age/images']):
        Image.fromarray(image).save(os.path.join(directory, str(name)))
    return str(directory)
