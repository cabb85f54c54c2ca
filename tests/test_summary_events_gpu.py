"""Histograms on the MI355X (csrc/summary_histogram.hip: ``srgan_tensor_histogram``) against the NumPy form of the same contract
(``summary_events.histogram_of_array``, pinned on the CPU against np.histogram), and the event files that whole experiments
leave behind: scalars, pictures and histograms read back from ``logs/<trial>/DNN`` and ``GAN``.

``out`` is a window between NaN-bit guard bands of a larger buffer, pre-filled with the same bits: the call writes every one of
its ``5 + (bins + 1) + bins`` doubles and nothing else.  The launcher gives a workgroup spans of 4096 floats (1024 16-byte
loads) and at most 2048 workgroups; the sizes below sit around those."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from test_image_summaries_gpu import age_experiment, summary_step
from test_summary_events_cpu import decode_png

pytestmark = pytest.mark.gpu
GUARD = 7
SPAN, MAX_WORKGROUPS = 4096, 2048
SMALL_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, SPAN - 1, SPAN, SPAN + 1, SPAN + 4, 3 * SPAN + 1037]
GRID_STRIDE_SIZE = MAX_WORKGROUPS * SPAN + 5 * SPAN + 123          # more spans than workgroups, ragged


@pytest.fixture(scope='module')
def lib():
    import srgan_amd  # noqa: F401
    from srgan_amd import _lib
    _lib.library()
    return _lib


@pytest.fixture(scope='module')
def events():
    from srgan_amd import summary_events
    return summary_events


@pytest.fixture(autouse=True)
def native_writer(monkeypatch):
    monkeypatch.setitem(sys.modules, 'tensorboardX', None)


def bits(array):
    return np.ascontiguousarray(array, dtype=np.float64).view(np.int64)


def call(lib, values, bins, offset=0, expect=0):
    """``out`` of srgan_tensor_histogram over the host array ``values``, uploaded ``offset`` floats past a 16-byte boundary;
    checks the guard bands.  With ``expect`` != 0: asserts that status and that ``out`` kept its NaN bits."""
    values = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
    holder = torch.empty(values.size + offset + 4, dtype=torch.float32, device='cuda')
    assert holder.data_ptr() % 16 == 0
    x = holder[offset:offset + values.size]
    x.copy_(torch.from_numpy(values))
    length = 6 + 2 * max(1, min(int(bins), 1024))
    buffer = torch.full((length + 2 * GUARD,), float('nan'), dtype=torch.float64, device='cuda')
    before = buffer.cpu().numpy().view(np.int64).copy()
    status = lib.library().srgan_tensor_histogram(x.data_ptr() if values.size else None, values.size, bins,
                                                  buffer.data_ptr() + 8 * GUARD, lib.stream_handle())
    torch.cuda.synchronize()
    after = buffer.cpu().numpy()
    assert np.array_equal(after.view(np.int64)[:GUARD], before[:GUARD]) and np.array_equal(after.view(np.int64)[-GUARD:], before[-GUARD:])
    assert status == expect, (status, lib.library().srgan_last_error())
    if expect:
        assert np.array_equal(after.view(np.int64), before)
    return after[GUARD:GUARD + length]


def flat(record):
    return np.concatenate([[record[key] for key in ('min', 'max', 'sum', 'sum_squares', 'finite_count')], record['edges'],
                           record['counts']])


def dyadic(size, seed):
    """Multiples of 1 / 8 in [-64, 64] with both ends present (from two elements on): every sum is exact in fp64."""
    values = np.random.RandomState(seed).randint(-512, 513, size=size).astype(np.float32) / np.float32(8)
    if size >= 2:
        values[size // 3], values[-1] = -64.0, 64.0
    return values


def assert_bitwise(got, want, what):
    different = np.nonzero(bits(got) != bits(want))[0]
    assert different.size == 0, (what, different[:5], np.asarray(got)[different[:5]], np.asarray(want)[different[:5]])


@pytest.mark.parametrize('bins', [1, 2, 30, 1024])
def test_dyadic_data_bit_for_bit(lib, events, bins):
    for size in SMALL_SIZES:
        for offset in ((0, 1) if size in (0, 1, 65, 257, SPAN + 1, 3 * SPAN + 1037) else (0,)):
            values = dyadic(size, size + bins)
            assert_bitwise(call(lib, values, bins, offset), flat(events.histogram_of_array(values, bins)), (size, bins, offset))


def test_more_spans_than_workgroups_and_every_misalignment(lib, events):
    values = dyadic(GRID_STRIDE_SIZE, 3)
    want = flat(events.histogram_of_array(values, 30))
    assert_bitwise(call(lib, values, 30, 3), want, 'grid stride')
    small = dyadic(2 * SPAN + 77, 4)
    want = flat(events.histogram_of_array(small, 7))
    for offset in (0, 1, 2, 3):
        assert_bitwise(call(lib, small, 7, offset), want, offset)


def test_a_count_above_two_to_the_24_is_exact(lib, events):
    """One hot bin: 2^24 + 4096 elements are 1.0, between one 0.0 and two 2.0 -- a float counter would stop at 2^24."""
    size = 2 ** 24 + SPAN + 3
    values = np.ones(size, dtype=np.float32)
    values[[0, 5, size - 1]] = 0.0, 2.0, 2.0
    want = flat(events.histogram_of_array(np.array([0.0, 1.0, 2.0, 2.0], dtype=np.float32), 30))      # the same edges
    counts = want[6 + 30:]
    hot = int(np.nonzero(counts[1:] == 1)[0][0]) + 1
    assert counts[0] == 1 and counts[29] == 2 and hot in (14, 15)
    counts[hot] = size - 3
    want[2:5] = size - 3 + 4, size - 3 + 8, size
    out = call(lib, values, 30, 1)
    assert_bitwise(out, want, 'hot bin')
    assert out[6 + 30 + hot] > 2 ** 24 and out[6 + 30:].sum() == size


@pytest.mark.parametrize('bins', [1, 2, 30, 1024])
def test_random_data(lib, events, bins):
    """Counts and edges bit for bit, min and max exact; the sums within n * 2^-53 * sum |term| of math.fsum: the bound of any
    order of n fp64 additions of exactly representable terms (each addition is off by at most 2^-53 of a partial sum, and no
    partial sum exceeds sum |term| by more than that factor again)."""
    for size in (257, SPAN + 1, 3 * SPAN + 1037, 64 * SPAN + 5):
        values = np.random.RandomState(size + bins).standard_normal(size).astype(np.float32) * np.float32(3) + np.float32(0.5)
        out = call(lib, values, bins, size % 4)
        want = flat(events.histogram_of_array(values, bins))
        assert_bitwise(out[5:], want[5:], (size, bins))
        assert_bitwise(out[[0, 1, 4]], want[[0, 1, 4]], (size, bins))
        wide = values.astype(np.float64)
        assert abs(out[2] - math.fsum(wide)) <= size * 2.0 ** -53 * math.fsum(np.abs(wide))
        assert abs(out[3] - math.fsum(wide * wide)) <= size * 2.0 ** -53 * math.fsum(wide * wide)


def test_special_values(lib, events):
    specials = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-42, -1e-42, 1.401298464324817e-45, -np.nan], dtype=np.float32)
    values = dyadic(2 * SPAN + 9, 11)
    values[::17] = np.resize(specials, values[::17].size)
    for bins in (1, 30, 1024):
        out = call(lib, values, bins, 1)
        assert_bitwise(out, flat(events.histogram_of_array(values, bins)), bins)
        assert out[4] == np.isfinite(values).sum() < values.size
    # only zeros of both signs and subnormals: min == max is not the case, the range is 2e-42 wide
    tiny = np.resize(np.array([-0.0, 0.0, 1e-42, -1e-42], dtype=np.float32), 1000)
    assert_bitwise(call(lib, tiny, 30), flat(events.histogram_of_array(tiny, 30)), 'tiny')
    zeros = call(lib, np.full(300, -0.0, dtype=np.float32), 2)
    assert_bitwise(zeros, np.array([0.0, 0.0, 0.0, 0.0, 300.0, -0.5, 0.0, 0.5, 0.0, 300.0]), 'negative zeros')
    for size in (1, 300, SPAN + 5):                                # all equal: NumPy's +- 0.5 rule
        equal = np.full(size, 2.5, dtype=np.float32)
        out = call(lib, equal, 30)
        assert_bitwise(out, flat(events.histogram_of_array(equal, 30)), size)
        assert (out[5], out[35], out[36 + 15]) == (2.0, 3.0, size)
    for size in (1, 300, 2 * SPAN + 5):                            # nothing finite: all of out is +0.0
        nothing = np.resize(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), size)
        assert_bitwise(call(lib, nothing, 30, 1), np.zeros(66), size)
    huge = np.array([3.4028234663852886e38, -3.4028234663852886e38, 1.0], dtype=np.float32)      # hi - lo needs fp64
    out, want = call(lib, huge, 4), flat(events.histogram_of_array(huge, 4))
    keep = np.arange(out.size) != 2                                 # the sum of these three depends on the order: 1.0 or 0.0
    assert_bitwise(out[keep], want[keep], 'huge')
    assert abs(out[2] - 1.0) <= 3 * 2.0 ** -53 * (2 * 3.4028234663852886e38 + 1)


def test_two_calls_agree_bit_for_bit(lib):
    values = np.random.RandomState(8).standard_normal(300 * SPAN + 11).astype(np.float32)
    first, second = call(lib, values, 30, 2), call(lib, values, 30, 2)
    assert_bitwise(first, second, 'two calls')
    assert first[4] == values.size


def test_argument_errors_leave_out_untouched(lib):
    values = np.arange(16, dtype=np.float32)
    for bins in (0, -1, 1025):
        call(lib, values, bins, expect=lib.EINVAL)
    library, stream = lib.library(), lib.stream_handle()
    x = torch.arange(16, dtype=torch.float32, device='cuda')
    out = torch.full((66,), float('nan'), dtype=torch.float64, device='cuda')
    limit = lib.capabilities().max_tensor_elements
    for arguments, status in (((None, 16, 30, out.data_ptr()), lib.EINVAL), ((x.data_ptr(), 16, 30, None), lib.EINVAL),
                              ((x.data_ptr(), -1, 30, out.data_ptr()), lib.EINVAL),
                              ((x.data_ptr() + 2, 8, 30, out.data_ptr()), lib.EINVAL),
                              ((x.data_ptr(), 16, 30, out.data_ptr() + 4), lib.EINVAL),
                              ((x.data_ptr(), limit + 1, 30, out.data_ptr()), lib.ERANGE)):
        assert library.srgan_tensor_histogram(*arguments, stream) == status, arguments
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    assert library.srgan_tensor_histogram(None, 0, 30, out.data_ptr(), stream) == 0          # n == 0 needs no x
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any()
    assert lib.capabilities().features & 0x20000


def test_add_histogram_of_a_device_tensor_equals_that_of_its_host_copy(lib, events, tmp_path):
    from srgan_amd import functional as F
    from srgan_amd.utility import SummaryWriter
    device_writer, host_writer = SummaryWriter(str(tmp_path / 'device')), SummaryWriter(str(tmp_path / 'host'))
    exact = torch.from_numpy(dyadic(5 * SPAN + 3, 21)).cuda()
    for writer, tensor in ((device_writer, exact), (host_writer, exact.cpu())):
        writer.add_histogram('Exact', tensor, 3, bins='auto')
        writer.add_histogram('Var', F.constant(exact) if tensor.is_cuda else tensor.numpy(), 4, bins=1024)
        writer.add_histogram('Strided', tensor.reshape(-1, 7)[:, ::2] if tensor.numel() % 7 == 0 else tensor[::2], 5, bins=8)
        writer.add_histogram('Half', tensor.half(), 6)
        writer.close()
    assert sorted(device_writer.histograms) == ['Exact', 'Half', 'Strided', 'Var']
    for tag, (step, record) in device_writer.histograms.items():
        host_step, host_record = host_writer.histograms[tag]
        assert step == host_step
        assert_bitwise(flat(record), flat(host_record), tag)
    assert len(device_writer.histograms['Exact'][1]['counts']) == 30
    device_file, = events.event_files(str(tmp_path / 'device'))
    host_file, = events.event_files(str(tmp_path / 'host'))
    for ours, theirs in zip(list(events.read_events(device_file))[1:], list(events.read_events(host_file))[1:]):
        assert ours['step'] == theirs['step'] and ours['values'][0]['tag'] == theirs['values'][0]['tag']
        for key, value in ours['values'][0]['histo'].items():
            assert_bitwise(np.atleast_1d(value), np.atleast_1d(theirs['values'][0]['histo'][key]), key)
    with pytest.raises(ValueError, match='bins'):
        device_writer.add_histogram('Wrong', exact, bins=2000)


def test_arena_histogram_summaries(lib, events):
    experiment = age_experiment(4)
    experiment.gan_summary_writer.step = experiment.dnn_summary_writer.step = 5
    experiment.arena_histogram_summaries()
    gan, dnn = experiment.gan_summary_writer.histograms, experiment.dnn_summary_writer.histograms
    assert sorted(gan) == ['Gradients/D', 'Gradients/G', 'Parameters/D', 'Parameters/G']
    assert sorted(dnn) == ['Gradients/DNN', 'Parameters/DNN']
    for name, records in (('D', gan), ('G', gan), ('DNN', dnn)):
        arena = getattr(experiment, name)._srgan_arena
        for tag, tensor in ((f'Parameters/{name}', arena.data), (f'Gradients/{name}', arena.grad)):
            step, record = records[tag]
            assert step == 5 and record['finite_count'] == tensor.numel() == record['counts'].sum() and len(record['counts']) == 30
            want = events.histogram_of_array(tensor.cpu().numpy(), 30)
            assert_bitwise(flat(record)[[0, 1, 4]], flat(want)[[0, 1, 4]], tag)
            assert_bitwise(flat(record)[5:], flat(want)[5:], tag)
    assert gan['Parameters/D'][1]['max'] > gan['Parameters/D'][1]['min']


# ---- whole experiments ------------------------------------------------------------------------------------------------------
def coefficient_settings(directory, steps):
    from srgan_amd.settings import Settings
    s = Settings()
    s.trial_name, s.logs_directory = 'events', directory
    s.steps_to_run, s.summary_step_period = steps, 2
    s.batch_size, s.labeled_dataset_size, s.unlabeled_dataset_size, s.validation_dataset_size = 16, 32, 64, 16
    s.skip_completed_experiment = False
    return s


def as_float32(scalars):
    return {tag: [(step, np.float32(value)) for step, value in points] for tag, points in scalars.items()}


@pytest.fixture(scope='module')
def coefficient_runs(tmp_path_factory):
    """One coefficient experiment through train() (6 steps), a snapshot of what it left, then the same trial continued to step 8."""
    import srgan_amd  # noqa: F401
    from srgan_amd import summary_events
    from srgan_amd.coefficient.srgan import CoefficientExperiment
    directory = str(tmp_path_factory.mktemp('logs'))
    with pytest.MonkeyPatch.context() as patch:
        patch.setitem(sys.modules, 'tensorboardX', None)
        first = CoefficientExperiment(coefficient_settings(directory, 6))
        first.train()
        after_first = {name: (summary_events.event_files(os.path.join(first.trial_directory, name)),
                              summary_events.scalars(os.path.join(first.trial_directory, name))) for name in ('DNN', 'GAN')}
        resumed = coefficient_settings(directory, 8)
        resumed.trial_name = os.path.basename(first.trial_directory)
        resumed.continue_existing_experiments = True
        second = CoefficientExperiment(resumed)
        second.train()
    return first, after_first, second


def test_train_leaves_complete_event_files(coefficient_runs, events):
    first, after_first, _ = coefficient_runs
    for name, writer in (('DNN', first.dnn_summary_writer), ('GAN', first.gan_summary_writer)):
        files, scalars = after_first[name]
        assert len(files) == 1 and os.path.dirname(files[0]) == os.path.join(first.trial_directory, name)
        assert writer.scalars and sorted(scalars) == sorted(writer.scalars)
        assert as_float32(scalars) == as_float32(writer.scalars), name
        records = list(events.read_events(files[0]))                 # complete: nothing cut off, every checksum right
        assert records[0]['file_version'] == 'brain.Event:2'
        logged = sum('simple_value' in value for record in records for value in record.get('values', ()))
        assert logged == sum(len(points) for points in writer.scalars.values())
        with pytest.raises(ValueError, match='closed'):
            writer._events.add_scalar('late', 0.0, 0)                 # Experiment.close() closed it
    steps = [step for step, _ in first.gan_summary_writer.scalars['1 Validation Error/MAE']]
    assert steps == [0, 2, 4, 5]
    assert 'Discriminator/Gradient Penalty' in after_first['GAN'][1]


def test_a_continued_run_adds_a_second_file(coefficient_runs, events):
    first, after_first, second = coefficient_runs
    assert second.trial_directory == first.trial_directory and second.starting_step == 7
    for name, before, after in (('DNN', first.dnn_summary_writer, second.dnn_summary_writer),
                                ('GAN', first.gan_summary_writer, second.gan_summary_writer)):
        directory = os.path.join(first.trial_directory, name)
        files = events.event_files(directory)
        assert len(files) == 2 and files[0] == after_first[name][0][0]
        merged = {tag: list(points) for tag, points in before.scalars.items()}
        for tag, points in after.scalars.items():
            merged.setdefault(tag, []).extend(points)
        assert as_float32(events.scalars(directory)) == as_float32(merged), name
    assert [step for step, _ in events.scalars(os.path.join(first.trial_directory, 'GAN'))['1 Validation Error/MAE']] == [0, 2, 4, 5, 7]


def test_age_pictures_in_the_file_follow_the_byte_rule(lib, events, tmp_path):
    from srgan_amd.utility import SummaryWriter
    experiment = age_experiment(4, image_summaries=True)
    experiment.dnn_summary_writer, experiment.gan_summary_writer = SummaryWriter(str(tmp_path / 'DNN')), SummaryWriter(str(tmp_path / 'GAN'))
    summary_step(experiment, 3)                                      # end_of_step flushes: no flush() here
    path, = events.event_files(str(tmp_path / 'GAN'))
    pictures = {value['tag']: (record['step'], value['image']) for record in events.read_events(path)
                for value in record.get('values', ()) if 'image' in value}
    memory = experiment.gan_summary_writer.images
    assert sorted(pictures) == sorted(memory) == ['Fake/Offset', 'Fake/Standard', 'Real']
    for tag, (step, (height, width, channels, png)) in pictures.items():
        kept_step, kept = memory[tag]
        assert step == kept_step == 3 and (channels, height, width) == kept.shape
        assert np.array_equal(decode_png(png), events.image_bytes(kept)), tag
    real = events.image_bytes(memory['Real'][1])
    assert real.min() == 0 and real.max() > 128                     # a picture, not a blank
    experiment.close()
    assert list(events.read_events(path))                            # still complete after close()
