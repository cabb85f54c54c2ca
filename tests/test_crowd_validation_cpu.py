"""Crowd validation from the resident database, the parts that need no GPU: the NumPy restatement of
``srgan_crowd_evaluation_sums`` against hand-written answers, the entry point's plumbing and argument checks (made before
any device work), ``evaluation_batch_count``, the UCF-QNRF file order and slices, the fixed draw list of
``ResidentCrowdEvaluationSet`` (scenes held on the CPU device) and the setting's ``ValueError`` without a database."""
import os
import random
import re

import numpy as np
import pytest
import torch

from crowd_validation_reference import contraction_cases, evaluation_scalars, evaluation_sums, order_bounds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 16        # a non-NULL, 16-byte aligned "pointer" for calls that must fail before touching memory
CPU = torch.device('cpu')


# ---- the restatement ------------------------------------------------------------------------------------------------------
def test_the_restatement_on_a_hand_written_case():
    """B = 2 examples of a 2 x 2 plane, M = 2 predicted maps."""
    counts = np.array([3.0, 1.0], dtype=np.float32)
    labels = np.array([[[1, 0], [0.5, 0.5]], [[0, 1], [1, 1]]], dtype=np.float32).reshape(2, 4)        # sums 2 and 3
    maps = np.array([[0, 1, 2, 3], [1, 1, 1, 1]], dtype=np.float32)
    predicted = np.array([[[0, 1, 2, 3], [1, 1, 1, 1]],                  # example 0: e = 0 0 0 0 | 1 0 -1 -2
                          [[1, 1, 1, 2], [0.5, 1, 1, -1]]], dtype=np.float32)      # example 1: e = 0 0 0 1 | -.5 0 0 -2
    sums = evaluation_sums(counts, labels, predicted, maps)
    # d = (1, -2)
    assert sums.tolist() == [-1.0, 3.0, 5.0, 2.0, 1 + 1 + 2 + 1 + 0.5 + 2, 1 + 1 + 4 + 1 + 0.25 + 4, 16.0, 0.0]
    again = evaluation_sums(counts, labels, sums=sums)                     # a second batch without maps, added on top
    assert again.tolist() == [-2.0, 6.0, 10.0, 4.0, 7.5, 11.25, 16.0, 0.0]
    assert evaluation_sums(counts, labels, sums=[0, 0, 0, 0, 0, 0, 0, 9.5])[7] == 9.5
    scalars = evaluation_scalars(again, comparison_value=3.0)
    assert [tag for tag, _ in scalars] == ['ME', 'MAE', 'kNN MAE', 'MSE', 'kNN MSE', 'Ratio MAE GAN DNN']
    assert [value for _, value in scalars] == [-0.5, 1.5, 7.5 / 16, 2.5, 11.25 / 16, 0.5]
    assert len(evaluation_scalars(again)) == 5
    with pytest.raises(ValueError):
        evaluation_sums(counts, labels, predicted, None)
    assert evaluation_sums(counts[:0], labels[:0], sums=again).tolist() == again.tolist()              # B == 0: untouched
    bounds = order_bounds(counts, labels, predicted, maps)
    assert bounds[3] == bounds[6] == bounds[7] == 0 and all(0 < bounds[k] < 1e-12 for k in (0, 1, 2, 4, 5))


def test_the_contraction_cases_tell_a_fused_square_from_a_rounded_one():
    """The cases the GPU test feeds the kernel: the restatement gives the rounded-product value, which is not the fused one."""
    for plane in (1, 4):
        cases = contraction_cases(4, plane)
        assert len(cases) == 4
        for inputs, unfused, fused in cases:
            assert unfused != fused and abs(unfused - fused) <= 2.0 ** -51                  # one unit in the last place apart
            sums = evaluation_sums(*inputs)
            assert sums[2] == unfused and sums[5] == unfused
            assert sums[3] == 17 and sums[6] == 17 * 2 * plane
            e1, e2 = 1.0 - float(inputs[3][0, 0]), 1.5 - float(inputs[3][0, 0])
            assert sums[0] == e1 + e2 == sums[1] == sums[4]


# ---- the entry point ------------------------------------------------------------------------------------------------------
def test_the_library_advertises_and_binds_the_entry_points():
    from srgan_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'srgan_hip.h')).read()
    assert re.search(r'#define\s+SRGAN_FEATURE_CROWD_EVALUATION\s+0x10000u', header)
    assert _lib.capabilities().features & 0x10000
    assert _lib.library().srgan_version() == 110
    assert {'srgan_crowd_evaluation_sums', 'srgan_crowd_evaluation_scratch_bytes'} <= set(_lib.SIGNATURES)
    assert 'srgan_crowd_evaluation_sums' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def evaluation_call(lib, **changes):
    a = dict(dict(counts=PTR, labels=PTR, predicted=PTR, maps=PTR, B=2, M=3, HW=25, sums=PTR, scratch=PTR), **changes)
    return lib.library().srgan_crowd_evaluation_sums(a['counts'], a['labels'], a['predicted'], a['maps'], a['B'], a['M'],
                                                     a['HW'], a['sums'], a['scratch'], None)


def test_argument_errors_are_reported_before_any_device_work():
    from srgan_amd import _lib
    for name in ('counts', 'labels', 'sums', 'scratch'):
        assert evaluation_call(_lib, **{name: None}) == _lib.EINVAL, name
        assert _lib.library().srgan_last_error()
    assert evaluation_call(_lib, predicted=None) == _lib.EINVAL and evaluation_call(_lib, maps=None) == _lib.EINVAL
    assert evaluation_call(_lib, B=-1) == _lib.EINVAL and evaluation_call(_lib, HW=-1) == _lib.EINVAL
    assert evaluation_call(_lib, M=0) == _lib.EINVAL and evaluation_call(_lib, M=-2) == _lib.EINVAL
    assert evaluation_call(_lib, sums=PTR + 4) == _lib.EINVAL and evaluation_call(_lib, scratch=PTR + 4) == _lib.EINVAL
    limit = _lib.capabilities().max_tensor_elements
    assert evaluation_call(_lib, B=1, M=1, HW=limit + 1) == _lib.ERANGE
    assert b'max_tensor_elements' in _lib.library().srgan_last_error()
    assert evaluation_call(_lib, B=2 ** 10, M=2 ** 10, HW=2 ** 11) == _lib.ERANGE                        # 2^31 elements
    assert evaluation_call(_lib, B=2 ** 31 - 1, M=2 ** 31 - 1, HW=2 ** 62) == _lib.ERANGE                # no 64-bit overflow
    assert evaluation_call(_lib, B=2 ** 16, M=0, HW=2 ** 15, predicted=None, maps=None) == _lib.ERANGE   # B * HW without maps
    # zero work: a successful no-op (nothing is launched, the fake pointers are never used)
    assert evaluation_call(_lib, B=0) == 0 and evaluation_call(_lib, HW=0) == 0
    assert evaluation_call(_lib, B=0, M=0, predicted=None, maps=None) == 0
    query = _lib.library().srgan_crowd_evaluation_scratch_bytes
    assert query(-1, 1, 4) == _lib.EINVAL and query(1, -1, 4) == _lib.EINVAL and query(1, 1, -4) == _lib.EINVAL
    assert query(2 ** 10, 2 ** 10, 2 ** 11) == _lib.ERANGE
    # more workgroups (B * ceil(HW / 2048)) than one launch holds: 2^24 - 1 is the last count taken
    assert query(2 ** 24 - 1, 1, 1) == (2 ** 24 - 1) * 24 and query(2 ** 24, 1, 1) == _lib.ERANGE
    assert query(2 ** 23, 1, 100) > 0 and query(2 ** 24, 1, 100) == _lib.ERANGE              # (1.7e9 elements: within 2^31 - 1)
    assert evaluation_call(_lib, B=2 ** 24, M=1, HW=1) == _lib.ERANGE
    assert b'workgroups' in _lib.library().srgan_last_error()
    assert evaluation_call(_lib, B=2 ** 24, M=0, HW=3, predicted=None, maps=None) == _lib.ERANGE
    assert query(0, 3, 0) > 0 and query(2, 3, 25) >= 2 * 3 * 8 and query(2, 0, 25) == query(2, 3, 25)
    assert query(16, 3, 512 * 512) < 1 << 20                  # (an epoch's scratch is a few kilobytes)


# ---- the evaluation sets --------------------------------------------------------------------------------------------------
def test_evaluation_batch_count():
    from srgan_amd.crowd.data import evaluation_batch_count
    assert [evaluation_batch_count(b) for b in (1, 15, 16, 50, 100, 101)] == [101, 8, 8, 3, 2, 2]
    for batch_size in range(1, 130):                          # the reference's loop: break behind batch index * b >= 100
        walked = next(index + 1 for index in range(1000) if index * batch_size >= 100)
        assert evaluation_batch_count(batch_size) == walked, batch_size


def write_ucf_qnrf(directory, split, names, shape=(70, 90), maps='i1nn_maps', seed=0):
    generator = np.random.RandomState(seed)
    for name in names:
        arrays = {'images': generator.randint(0, 256, size=shape + (3,)).astype(np.uint8),
                  'labels': (generator.rand(*shape) < 0.004).astype(np.float32),
                  maps: generator.rand(*shape).astype(np.float32)}
        for kind, array in arrays.items():
            os.makedirs(os.path.join(directory, split, kind), exist_ok=True)
            np.save(os.path.join(directory, split, kind, name + '.npy'), array)


def test_ucf_qnrf_dataset_order_and_slices(tmp_path):
    from srgan_amd.crowd.data import CrowdDataset, UcfQnrfCrowdDataset
    assert [member.value for member in CrowdDataset] == ['UCF QNRF', 'ShanghaiTech', 'World Expo']
    assert CrowdDataset('UCF QNRF') is CrowdDataset.ucf_qnrf
    names = ['img_%04d' % index for index in (7, 1, 12, 3, 9, 4, 10)]
    write_ucf_qnrf(str(tmp_path), 'Train', names)
    write_ucf_qnrf(str(tmp_path), 'Test', ['img_0100', 'img_0101'])
    for stray in ('notes.txt', 'img_0001.npy.bak', 'img_9999.png'):
        open(tmp_path / 'Train' / 'labels' / stray, 'w').close()
    for seed in (0, 3, 101):
        expected = sorted(name + '.npy' for name in names)
        random.seed(seed)
        random.shuffle(expected)
        dataset = UcfQnrfCrowdDataset(str(tmp_path), 'train', seed=seed, map_directory_name='i1nn_maps')
        assert dataset.file_names == expected and len(dataset) == 7
        pick = lambda **k: UcfQnrfCrowdDataset(str(tmp_path), 'train', seed=seed, map_directory_name='i1nn_maps', **k).file_names
        assert pick(number_of_examples=3) == expected[:3]
        assert pick(examples_start=2) == expected[2:]
        assert pick(examples_start=2, number_of_examples=3) == expected[2:5]
        assert pick(examples_start=5, number_of_examples=10) == expected[5:]
        assert pick(examples_start=None, number_of_examples=None) == expected
        labeled, unlabeled = pick(number_of_examples=3), pick(examples_start=3, number_of_examples=None)
        assert not set(labeled) & set(unlabeled) and sorted(labeled + unlabeled) == sorted(expected)
    assert UcfQnrfCrowdDataset(str(tmp_path), 'train', seed=1).file_names != \
        UcfQnrfCrowdDataset(str(tmp_path), 'train', seed=2).file_names
    test = UcfQnrfCrowdDataset(str(tmp_path), 'test', seed=101, map_directory_name='i1nn_maps')
    assert sorted(test.file_names) == ['img_0100.npy', 'img_0101.npy']
    image, label, map_ = test[0]
    assert image.dtype == np.uint8 and image.shape == (70, 90, 3) and label.shape == map_.shape == (70, 90)
    stored = np.load(tmp_path / 'Test' / 'i1nn_maps' / test.file_names[0])
    assert np.array_equal(map_, stored)
    examples = test.examples()
    assert len(examples) == 2 and np.array_equal(examples[0].map, stored) and examples[1].image.shape == (70, 90, 3)


SHAPES = [(80, 100), (88, 100), (96, 128)]


def scenes():
    from srgan_amd.crowd.data import CrowdExample
    return [CrowdExample(image=np.zeros(shape + (3,), dtype=np.uint8), label=np.zeros(shape, dtype=np.float32),
                         map_=np.zeros(shape, dtype=np.float32)) for shape in SHAPES]


def test_the_loaders_own_draws_are_unchanged():
    """``draw_positions`` of a fresh loader, recorded before the per-example rule moved into ``draw_example``."""
    from srgan_amd.crowd.data import DeviceCrowdPatchLoader
    loader = DeviceCrowdPatchLoader(scenes(), 6, 64, seed=3, device=CPU)
    assert loader.draw_positions() == [(2, 37, 51, 0), (2, 59, 44, 1), (2, 54, 48, 0), (2, 43, 67, 1), (2, 55, 52, 1),
                                       (2, 34, 86, 1)]
    assert loader.draw_positions() == [(2, 55, 48, 1), (2, 53, 78, 1), (2, 61, 87, 0), (2, 34, 32, 0), (2, 48, 91, 1),
                                       (2, 45, 79, 0)]
    unflipped = DeviceCrowdPatchLoader(scenes(), 4, 64, seed=7, device=CPU, flip=False)
    assert unflipped.draw_positions() == [(0, 36, 59, 0), (1, 47, 68, 0), (0, 46, 51, 0), (2, 47, 53, 0)]


def test_the_evaluation_sets_draw_list():
    from srgan_amd.crowd.data import DeviceCrowdPatchLoader, ResidentCrowdEvaluationSet, evaluation_batch_count
    loader = DeviceCrowdPatchLoader(scenes(), 50, 64, seed=3, device=CPU)
    fresh = ResidentCrowdEvaluationSet(loader, 50, 64, seed=3, flip=True)
    assert len(fresh) == len(fresh.draws) == evaluation_batch_count(50) * 50 == 150
    assert fresh.scenes is loader                                         # the train set shares the resident scenes
    # the list is the loader's rule on a private generator: the first batch of a fresh loader with the same seed
    assert fresh.draws[:50] == DeviceCrowdPatchLoader(scenes(), 50, 64, seed=3, device=CPU).draw_positions()
    state = loader.generator.get_state()[1].copy()
    for _ in range(5):
        loader.draw_positions()                                           # training moves on ...
    later = ResidentCrowdEvaluationSet(loader, 50, 64, seed=3, flip=True)
    assert later.draws == fresh.draws                                     # ... the list does not depend on it
    moved = loader.generator.get_state()[1].copy()
    ResidentCrowdEvaluationSet(loader, 50, 64, seed=3, flip=True)
    assert np.array_equal(loader.generator.get_state()[1], moved) and not np.array_equal(moved, state)   # nor moves it
    assert ResidentCrowdEvaluationSet(loader, 50, 64, seed=4, flip=True).draws != fresh.draws
    own = ResidentCrowdEvaluationSet(scenes(), 50, 64, seed=101, flip=False, device=CPU)     # uploads its own scenes
    assert own.scenes is not loader and len(own.scenes.images) == 3
    assert own.draws == ResidentCrowdEvaluationSet(scenes(), 50, 64, seed=101, flip=False, device=CPU).draws
    assert all(flip == 0 for *_, flip in own.draws) and any(flip for *_, flip in fresh.draws)
    half = 32
    for scene, y, x, _ in fresh.draws + own.draws:                        # every patch lies inside its scene
        height, width = SHAPES[scene]
        assert half <= y <= height - half and half <= x <= width - half
    with pytest.raises(ValueError):
        ResidentCrowdEvaluationSet(loader, 50, 32, seed=3)                # another patch size than the shared loader's
    with pytest.raises(IndexError):
        fresh.draws[150]


def test_crowd_validation_needs_a_database(monkeypatch):
    from srgan_amd.settings import Settings
    from srgan_amd.crowd.srgan import CrowdExperiment
    from srgan_amd.crowd.dnn import CrowdDnnExperiment
    monkeypatch.delenv('SRGAN_CROWD_DATABASE', raising=False)
    for experiment_class in (CrowdExperiment, CrowdDnnExperiment):
        settings = Settings()
        settings.batch_size, settings.image_patch_size = 2, 64
        settings.crowd_validation = 'device'
        with pytest.raises(ValueError, match='SRGAN_CROWD_DATABASE'):
            experiment_class(settings).dataset_setup()
    settings.crowd_validation = 'host'
    with pytest.raises(ValueError, match='crowd_validation'):
        CrowdExperiment(settings).dataset_setup()
    assert not hasattr(Settings(), 'crowd_validation')                    # opt-in: not among the defaults
