"""Generate tests/golden/g15_image_databases.npz by running the UNMODIFIED upstream reference on CPU.

Test infrastructure only, like make_goldens.py: it needs the reference checkout and never travels to the GPU box; the
emitted fixture holds data only.  Two tiny databases in the reference's on-disk layouts are built in a temporary
directory -- a steering-angle database (meta.pkl + float64 .npy frames) and an age database (meta.json + PNG images) --
and the reference's ``SteeringAngleDataset`` / ``AgeDataset`` are run over them for the three splits of
driving/srgan.py:17-40 and age/srgan.py:19-41 under two settings.  Recorded: the databases themselves and, per split,
the dataset's ``image_names``, labels and every item.  Usage::

    python tests/golden/make_image_database_goldens.py

The archive is written with fixed member times, so the same inputs give the same bytes.
"""
import io
import json
import os
import sys
import tempfile
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refstubs  # noqa: E402

_refstubs.install()


def _imread(path, **_):
    from PIL import Image
    with Image.open(path) as handle:
        return np.asarray(handle)


sys.modules['imageio'].imread = _imread           # (_refstubs registers an empty imageio; the reference reads PNGs with it)
for missing in ('requests', 'patoolib'):
    try:
        __import__(missing)
    except ImportError:
        sys.modules[missing] = types.ModuleType(missing)

import torch  # noqa: E402
import age.data as ref_age_data  # noqa: E402
import driving.data as ref_driving_data  # noqa: E402

# name: (labeled_dataset_size, validation_dataset_size, unlabeled_dataset_size, batch_size, labeled_dataset_seed)
SETTINGS = {'A': (5, 4, 6, 4, 3),
            'B': (5, 4, None, 8, 3)}           # the labeled slice is shorter than the batch: the repeat branch
DRIVING_FRAMES, AGE_IMAGES, SIZE = 23, 19, 8


def build_driving_database(directory):
    """23 float64 frames [3, 8, 8] with non-integer values in 0..255 (eighths: exact in fp32, what
    skimage.transform.resize(preserve_range=True) leaves is just as little an integer) and a two-column meta.pkl."""
    import pandas
    generator = np.random.RandomState(15)
    frames = generator.randint(0, 255 * 8 + 1, size=(DRIVING_FRAMES, 3, SIZE, SIZE)).astype(np.float64) / 8
    names = np.array(['{}.jpg'.format(100 + index) for index in range(DRIVING_FRAMES)])
    angles = np.round(generator.uniform(-90, 90, DRIVING_FRAMES), 2)
    pandas.DataFrame({0: names, 1: angles}).to_pickle(os.path.join(directory, 'meta.pkl'))
    for name, frame in zip(names, frames):
        np.save(os.path.join(directory, name.replace('.jpg', '.npy')), frame)
    return {'driving/frames': frames, 'driving/names': names, 'driving/angles': angles}


def build_age_database(directory):
    """19 uint8 RGB PNGs of 8 x 8 and a meta.json of [name, age, gender] triples with two dict entries among them."""
    from PIL import Image
    generator = np.random.RandomState(16)
    images = generator.randint(0, 256, size=(AGE_IMAGES, SIZE, SIZE, 3)).astype(np.uint8)
    names = ['face_{:02d}.png'.format(index) for index in range(AGE_IMAGES)]
    ages = [float(age) for age in generator.randint(10, 96, AGE_IMAGES)]
    entries = [[name, age, 'female' if index % 2 else 'male'] for index, (name, age) in enumerate(zip(names, ages))]
    for index in (4, 11):
        entries[index] = {'image_name': names[index], 'age': ages[index], 'age_standard_deviation': 1.5}
    meta_json = json.dumps(entries)
    with open(os.path.join(directory, 'meta.json'), 'w') as json_file:
        json_file.write(meta_json)
    for name, image in zip(names, images):
        Image.fromarray(image).save(os.path.join(directory, name))
    return {'age/images': images, 'age/names': np.array(names), 'age/ages': np.array(ages), 'age/meta_json': np.array(meta_json)}


def record(prefix, dataset, labels):
    items = [dataset[index] for index in range(len(dataset))]
    return {prefix + '/names': np.array(dataset.image_names).astype(str), prefix + '/labels': np.array(labels, dtype=np.float32),
            prefix + '/items': np.stack([image.numpy() for image, _ in items]).astype(np.float32),
            prefix + '/item_labels': np.array([float(label) for _, label in items], dtype=np.float32)}


def driving_splits(tag, labeled, validation, unlabeled, batch, seed):
    """The three constructor calls of driving/srgan.py:21-37."""
    make = lambda start, end: ref_driving_data.SteeringAngleDataset(start=start, end=end, seed=seed, batch_size=batch)
    unlabeled_start = labeled + validation
    unlabeled_end = unlabeled_start + unlabeled if unlabeled is not None else -validation
    out = {}
    for part, dataset in (('train', make(0, labeled)), ('validation', make(-validation, None)),
                          ('unlabeled', make(unlabeled_start, unlabeled_end))):
        out.update(record('driving/{}/{}'.format(tag, part), dataset, dataset.angles))
    return out


def age_splits(directory, tag, labeled, validation, unlabeled, batch, seed):
    """The three constructor calls of age/srgan.py:27-40.  (Upstream adds ``unlabeled_dataset_size`` to the start without
    looking at it; for None this generator ends the slice at the validation tail, the driving application's rule.)"""
    make = lambda start, end: ref_age_data.AgeDataset(directory, start=start, end=end, seed=seed, batch_size=batch)
    unlabeled_end = labeled + unlabeled if unlabeled is not None else -validation
    out = {}
    for part, dataset in (('train', make(0, labeled)), ('unlabeled', make(labeled, unlabeled_end)),
                          ('validation', make(-validation, None))):
        out.update(record('age/{}/{}'.format(tag, part), dataset, dataset.ages))
    return out


def save(path, arrays):
    """An .npz with sorted members and fixed member times: byte-identical from run to run."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as archive:
        for name in sorted(arrays):
            buffer = io.BytesIO()
            np.lib.format.write_array(buffer, np.asanyarray(arrays[name]), allow_pickle=False)
            member = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            member.compress_type = zipfile.ZIP_DEFLATED
            member.external_attr = 0o644 << 16
            archive.writestr(member, buffer.getvalue(), compresslevel=9)
    print('wrote {}  ({:.1f} KiB, {} arrays)'.format(path, os.path.getsize(path) / 1024, len(arrays)))


def main():
    arrays = {'torch_version': np.array(torch.__version__)}
    with tempfile.TemporaryDirectory() as root:
        driving_directory, age_directory = os.path.join(root, 'driving'), os.path.join(root, 'age')
        os.makedirs(driving_directory)
        os.makedirs(age_directory)
        arrays.update(build_driving_database(driving_directory))
        arrays.update(build_age_database(age_directory))
        ref_driving_data.database_directory = driving_directory        # the reference's module-level path
        for tag, (labeled, validation, unlabeled, batch, seed) in SETTINGS.items():
            arrays['settings/' + tag] = np.array([labeled, validation, -1 if unlabeled is None else unlabeled, batch, seed])
            arrays.update(driving_splits(tag, labeled, validation, unlabeled, batch, seed))
            arrays.update(age_splits(age_directory, tag, labeled, validation, unlabeled, batch, seed))
    save(os.path.join(HERE, 'g15_image_databases.npz'), arrays)


if __name__ == '__main__':
    main()
