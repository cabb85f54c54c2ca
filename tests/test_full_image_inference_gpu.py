"""Full-image crowd inference on the device: the three kernels against their host definitions (window extraction and
overlap average bit for bit, the resize against torch's CPU bilinear) and ``predict_full_example_device`` / ``inference``
/ ``evaluate`` / ``test_summaries`` against the host path and the reference's recorded results (goldens g9, g11)."""
import numpy as np
import pytest
import torch

from helpers import load_golden, assert_close, assert_close_norm
from test_steps_gpu import make_experiment, finish_setup, RTOL
from test_full_image_inference_cpu import host_blend, sliding_windows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    import srgan_amd  # noqa: F401
    from srgan_amd import _lib
    assert torch.cuda.is_available()
    return _lib


def dev(array):
    return torch.from_numpy(np.ascontiguousarray(array)).cuda()


def bits(array):
    return np.ascontiguousarray(array, dtype=np.float32).view(np.uint32)


def host_patch(image, y, x, patch_size):
    from srgan_amd.crowd.data import extract_padded_patch, negative_one_to_one
    return np.ascontiguousarray(negative_one_to_one(extract_padded_patch(image, y, x, patch_size)).transpose(2, 0, 1))


def extract_windows(lib, image, ys, xs, patch_size, first=0, count=None):
    count = len(ys) * len(xs) - first if count is None else count
    scene, device_ys, device_xs = dev(image), dev(np.asarray(ys, np.int32)), dev(np.asarray(xs, np.int32))
    out = torch.full((count, 3, patch_size, patch_size), float('nan'), device='cuda')
    lib.check(lib.library().srgan_crowd_extract_windows(
        scene.data_ptr(), image.shape[0], image.shape[1], device_ys.data_ptr(), len(ys), device_xs.data_ptr(), len(xs),
        first, count, patch_size, out.data_ptr(), lib.stream_handle()), 'srgan_crowd_extract_windows')
    return out.cpu().numpy()


def test_extracted_windows_equal_the_host_dataset_bit_for_bit(lib):
    g = load_golden('g9_crowd_sliding_window')
    size, step = int(g['image_size']), int(g['window_step'])
    from srgan_amd.crowd.data import CrowdExample, DeviceSlidingWindows, ImageSlidingWindowDataset
    for index in range(3):                    # 100 x 150, 64 x 64 and the padded 40 x 90 (clipped above and below)
        image = g[f'e{index}/image']
        example = CrowdExample(image=image, label=np.zeros(image.shape[:2], dtype=np.float32))
        dataset = ImageSlidingWindowDataset(example, size, step)
        windows = DeviceSlidingWindows(example, int(g['batch_size']), size, step)
        seen = 0
        for first, images in windows:
            images = images.cpu().numpy()
            for offset in range(images.shape[0]):
                patch, x, y = dataset[first + offset]
                assert windows.centre(first + offset) == (y, x)
                np.testing.assert_array_equal(bits(images[offset]), bits(patch.numpy()), err_msg=f'e{index} window {first + offset}')
                seen += 1
        assert seen == len(dataset)
    # windows clipped on each of the four sides (and in the corners), a range that starts inside the table
    image = g['e0/image']
    ys, xs = [5, 50, 95], [3, 75, 147]
    got = extract_windows(lib, image, ys, xs, size)
    for window in range(9):
        y, x = ys[window // 3], xs[window % 3]
        np.testing.assert_array_equal(bits(got[window]), bits(host_patch(image, y, x, size)), err_msg=f'centre {(y, x)}')
    assert (got[0][:, :size // 2 - 5, :] == -1).all() and (got[8][:, :, size // 2 + 3:] == -1).all()
    part = extract_windows(lib, image, ys, xs, size, first=4, count=3)
    np.testing.assert_array_equal(bits(part), bits(got[4:7]))
    # a patch size that is even but no multiple of four: the scalar-store form of the kernel
    small = extract_windows(lib, g['e2/image'], [1, 20, 38], [2, 45, 88], 6)
    for window in range(9):
        y, x = [1, 20, 38][window // 3], [2, 45, 88][window % 3]
        np.testing.assert_array_equal(bits(small[window]), bits(host_patch(g['e2/image'], y, x, 6)))


def blend(lib, densities, counts, ys, xs, height, width, patch_size, out=None):
    """(density[H, W], count) of one srgan_crowd_blend_windows call; ``out``: a device buffer of H * W + 1 floats."""
    device_counts, device_ys, device_xs = dev(counts), dev(ys), dev(xs)
    device_densities = None if densities is None else dev(densities)
    if out is None:
        out = torch.full((height * width + 1,), float('nan'), device='cuda')
    lib.check(lib.library().srgan_crowd_blend_windows(
        0 if densities is None else device_densities.data_ptr(), device_counts.data_ptr(), device_ys.data_ptr(), len(ys),
        device_xs.data_ptr(), len(xs), height, width, patch_size, out.data_ptr(), out.data_ptr() + 4 * height * width,
        lib.stream_handle()), 'srgan_crowd_blend_windows')
    result = out.cpu().numpy()
    return result[:-1].reshape(height, width).copy(), result[-1].copy()


def count_chain_length(pixels):
    """L: the longest chain of dependent fp32 additions between a per-pixel term and the scalar count, as the kernel is
    built.  A thread adds its 4 pixels (4), the workgroup's 256 sums meet in block_sum_256: 6 butterfly levels inside a
    wave + 3 additions over the 4 waves (9); one workgroup covers 1024 pixels.  With several workgroups the last one adds
    ceil(workgroups / 256) partial sums per thread and runs the same tree again (9)."""
    workgroups = -(-pixels // 1024)
    return 4 + 9 if workgroups == 1 else 4 + 9 + -(-workgroups // 256) + 9


# (H, W, P, step, the largest and the smallest number of windows covering one pixel; 0: a step wider than the patch)
BLEND_CASES = [(128, 192, 64, 64, 1, 1), (128, 192, 64, 32, 4, 1), (100, 150, 64, 16, 20, 1), (40, 90, 64, 24, 3, 1),
               (200, 200, 64, 100, 4, 0), (448, 672, 224, 224, 1, 1), (448, 672, 224, 112, 4, 1),
               (448, 560, 224, 64, 20, 1), (768, 1024, 224, 128, 9, 1)]


@pytest.mark.parametrize('height,width,patch_size,step,most,least', BLEND_CASES)
def test_blend_windows_equals_the_host_loop(lib, height, width, patch_size, step, most, least):
    windows, _ = sliding_windows(height, width, patch_size, step)
    generator = np.random.RandomState(7 * height + width + step)
    densities = (generator.rand(len(windows), patch_size, patch_size).astype(np.float32) - 0.3) * 3
    counts = (generator.rand(len(windows)).astype(np.float32) - 0.2) * 50
    centres = [windows.centre(index) for index in range(len(windows))]
    expected, terms = host_blend(densities, counts, centres, height, width, patch_size)
    covering = np.zeros((height, width), dtype=np.int32)
    half = patch_size // 2
    for y, x in centres:
        covering[max(y - half, 0):y + half, max(x - half, 0):x + half] += 1
    assert (covering.max(), covering.min()) == (most, least)

    density, count = blend(lib, densities, counts, windows.ys, windows.xs, height, width, patch_size)
    np.testing.assert_array_equal(bits(density), bits(expected))
    exact = terms.astype(np.float64).sum()
    bound = count_chain_length(height * width) * 2.0 ** -24 * np.abs(terms.astype(np.float64)).sum()
    print(f'count {count!r} float64 sum of the terms {exact!r} |difference| {abs(float(count) - exact):.3e} bound {bound:.3e} '
          f'(L = {count_chain_length(height * width)})')
    assert abs(float(count) - exact) <= bound
    # the same call again into a poisoned output: the same bits, density and count
    out = torch.full((height * width + 1,), float('nan'), device='cuda')
    again_density, again_count = blend(lib, densities, counts, windows.ys, windows.xs, height, width, patch_size, out=out)
    out.fill_(-12345.0)
    third_density, third_count = blend(lib, densities, counts, windows.ys, windows.xs, height, width, patch_size, out=out)
    for other_density, other_count in ((again_density, again_count), (third_density, third_count)):
        np.testing.assert_array_equal(bits(other_density), bits(density))
        assert bits(other_count) == bits(count)
    # no densities (a network with a placeholder density): an all-zero map, the same count
    zero_density, zero_count = blend(lib, None, counts, windows.ys, windows.xs, height, width, patch_size)
    assert (bits(zero_density) == 0).all() and bits(zero_count) == bits(count)


@pytest.mark.parametrize('shape,size', [((3, 16, 16), 64), ((2, 56, 56), 224), ((3, 16, 16), 40), ((2, 12, 20), 40),
                                        ((2, 64, 64), 64), ((1, 5, 7), 30)])
def test_resize_bilinear_equals_torch_cpu(lib, shape, size):
    generator = np.random.RandomState(size + shape[1])
    source = ((generator.rand(*shape).astype(np.float32) - 0.4) * 10)
    out = torch.full((shape[0], size, size), float('nan'), device='cuda')
    device_source = dev(source)
    lib.check(lib.library().srgan_crowd_resize_bilinear(device_source.data_ptr(), shape[0], shape[1], shape[2], size,
                                                        out.data_ptr(), lib.stream_handle()), 'srgan_crowd_resize_bilinear')
    got = out.cpu().numpy()
    expected = torch.nn.functional.interpolate(torch.from_numpy(source)[:, None], size=(size, size), mode='bilinear',
                                               align_corners=False)[:, 0].numpy()
    ulp = float(np.spacing(np.abs(source).max()))             # one ulp of the largest input magnitude
    error = float(np.abs(got - expected).max())
    print(f'{shape} -> {size}: max |difference| {error:.3e} = {error / ulp:.2f} ulp of the largest input; '
          f'{(got == expected).mean():.3f} of the outputs exact')
    assert error <= 4 * ulp
    if shape[1:] == (size, size):
        np.testing.assert_array_equal(bits(got), bits(source))           # the identity
    try:
        from PIL import Image
    except ImportError:
        print('PIL is not importable: the comparison with Image.resize(..., BILINEAR) in mode F is skipped')
        return
    for index in range(shape[0]):
        resized = np.asarray(Image.fromarray(source[index]).resize((size, size), Image.BILINEAR))      # float32: mode 'F'
        assert_close_norm(got[index], resized, rtol=1e-3, what=f'PIL {index}')


def test_resize_refuses_downscaling(lib):
    source, out = torch.zeros((1, 32, 32), device='cuda'), torch.zeros((1, 16, 16), device='cuda')
    status = lib.library().srgan_crowd_resize_bilinear(source.data_ptr(), 1, 32, 32, 16, out.data_ptr(), lib.stream_handle())
    assert status == lib.EUNSUPPORTED


def crowd_experiment(golden, networks=None, **overrides):
    from srgan_amd.crowd.models import DCGenerator, KnnDenseNetCat
    size = int(golden['image_size'])
    networks = networks or (lambda: (DCGenerator(image_size=size), KnnDenseNetCat(image_size=size),
                                     KnnDenseNetCat(image_size=size)))
    settings = dict(batch_size=int(golden['batch_size']), image_patch_size=size,
                    test_sliding_window_size=int(golden['window_step']))
    settings.update(overrides)
    experiment = make_experiment(networks, settings, crowd=True)
    finish_setup(experiment)
    experiment.eval_mode()
    return experiment


def test_predict_full_example_device_on_the_reference_examples(lib):
    """Golden g9 (the reference's own predict_full_example on the same weights): the device path against the recorded
    counts and density sums, and against the host method of this build."""
    from srgan_amd.crowd.data import CrowdExample
    g = load_golden('g9_crowd_sliding_window')
    experiment = crowd_experiment(g)
    for index in range(3):
        image = g[f'e{index}/image']
        example = CrowdExample(image=image, label=np.zeros(image.shape[:2], dtype=np.float32))
        count, density = experiment.predict_full_example_device(example, experiment.D)
        host_count, host_density = experiment.predict_full_example(example, experiment.D)
        assert density.shape == image.shape[:2] and density.dtype == np.float32
        print(f'example {index}: device {float(count)!r} host {float(host_count)!r} reference {float(g[f"e{index}/count"])!r}')
        assert_close(count, float(g[f'e{index}/count']), rtol=RTOL, what=f'example {index} count against the reference')
        assert_close(count, float(host_count), rtol=RTOL, what=f'example {index} count against the host path')
        assert_close(float(np.abs(density).sum()), float(g[f'e{index}/label_abs_sum']), rtol=RTOL, atol=1e-6,
                     what=f'example {index} density')
        np.testing.assert_array_equal(density, host_density)          # (both all zero: the placeholder density)


def test_a_quarter_resolution_density_goes_through_the_resize(lib):
    """``JointDCDiscriminator`` predicts its density at a quarter of the patch size: the host method refuses it, the
    device path resizes every window's density and blends -- restated here with torch's CPU bilinear and the host loop."""
    from srgan_amd.crowd.data import CrowdExample, ImageSlidingWindowDataset
    from srgan_amd.crowd.models import DCGenerator, JointDCDiscriminator
    from srgan_amd.srgan import as_var
    from srgan_amd.tape import no_grad
    g = load_golden('g9_crowd_sliding_window')
    size, step, batch_size = int(g['image_size']), int(g['window_step']), int(g['batch_size'])
    experiment = crowd_experiment(g, lambda: (DCGenerator(image_size=size), JointDCDiscriminator(image_size=size),
                                              JointDCDiscriminator(image_size=size)))
    for index in range(3):
        image = g[f'e{index}/image']
        example = CrowdExample(image=image, label=np.zeros(image.shape[:2], dtype=np.float32))
        with pytest.raises((NotImplementedError, ValueError)):       # (the host loop unpacks three outputs: it stops there)
            experiment.predict_full_example(example, experiment.D)
        count, density = experiment.predict_full_example_device(example, experiment.D)
        dataset = ImageSlidingWindowDataset(example, size, step)
        densities, counts, centres = [], [], []
        for start in range(0, len(dataset), batch_size):
            items = [dataset[i] for i in range(start, min(start + batch_size, len(dataset)))]
            with no_grad():
                quarter, batch_counts = experiment.D(as_var(torch.stack([item[0] for item in items])))
            assert tuple(quarter.shape[1:]) == (size // 4, size // 4)
            densities.append(torch.nn.functional.interpolate(quarter.cpu()[:, None], size=(size, size), mode='bilinear',
                                                             align_corners=False)[:, 0].numpy())
            counts.append(batch_counts.cpu().numpy().reshape(-1))
            centres += [(y, x) for _, x, y in items]
        expected_density, terms = host_blend(np.concatenate(densities), np.concatenate(counts), centres, image.shape[0],
                                             image.shape[1], size)
        assert density.shape == image.shape[:2] and float(np.abs(expected_density).max()) > 0
        assert_close(density, expected_density, rtol=RTOL, atol=1e-6, what=f'example {index} density')
        assert_close(float(count), float(np.sum(terms)), rtol=RTOL, atol=1e-6, what=f'example {index} count')


def g11_experiment(**overrides):
    g = load_golden('g11_crowd_evaluation')
    experiment = crowd_experiment(g, test_summary_size=None, map_directory_name='unused', **overrides)
    scenes = [(g[f'scene{i}/image'], g[f'scene{i}/label'], None) for i in range(3)]

    class TestDataset:
        length = len(scenes)

        def __init__(self, dataset, map_directory_name):
            assert dataset == 'test'

        def __getitem__(self, index):
            return scenes[index]
    experiment.dataset_class = TestDataset
    return experiment, g, scenes


def logged(writer):
    return {tag: float(values[-1][1]) for tag, values in writer.scalars.items()}


def test_inference_and_evaluate(lib):
    from srgan_amd.crowd.data import CrowdExample
    from srgan_amd.srgan import Experiment
    experiment, g, scenes = g11_experiment()
    image = scenes[0][0]
    count, density = experiment.inference(image)
    example = CrowdExample(image=image, label=np.zeros(image.shape[:2], dtype=np.float32))
    expected_count, expected_density = experiment.predict_full_example_device(example, experiment.inference_network)
    assert bits(count) == bits(expected_count) and density.shape == image.shape[:2]
    np.testing.assert_array_equal(bits(density), bits(expected_density))
    with pytest.raises(NotImplementedError):
        Experiment.inference(experiment, image)
    # evaluate(): the totals of reference crowd/srgan.py:302-330; its MAE / MSE are test_summaries' MAE / RMSE ** 2
    experiment.test_summaries()
    results = experiment.evaluate(during_training=True)
    assert sorted(results) == ['DNN', 'GAN']
    for name, writer in (('DNN', experiment.dnn_summary_writer), ('GAN', experiment.gan_summary_writer)):
        scalars, totals = logged(writer), results[name]
        assert_close(totals['MAE count'], scalars['0 Test Error/MAE count'], rtol=1e-6, what=f'{name} MAE count')
        assert_close(totals['MSE count'] ** 0.5, scalars['0 Test Error/RMSE count'], rtol=1e-6, what=f'{name} RMSE count')
        assert_close(totals['MAE density'], scalars['0 Test Error/MAE density'], rtol=1e-6, atol=1e-12, what=f'{name} MAE density')
        assert_close(totals['MSE density'] ** 0.5, scalars['0 Test Error/RMSE density'], rtol=1e-6, atol=1e-12,
                     what=f'{name} RMSE density')
        assert_close(totals['Count'], float(sum(scene[1].sum() for scene in scenes)), rtol=1e-6, what=f'{name} Count')
        assert_close(totals['Count error'], totals['MAE count'] * 3, rtol=1e-6, what=f'{name} Count error')
    assert len(experiment.evaluate(during_training=True, number_of_examples=1)) == 2


def test_test_summaries_on_the_device_path(lib):
    """``settings.full_image_inference = 'device'``: the same scalars as the host path (and as the reference, g11)."""
    host, g, _ = g11_experiment()
    assert getattr(host.settings, 'full_image_inference', 'host') == 'host'
    host.test_summaries()
    device, _, _ = g11_experiment(full_image_inference='device')
    device.test_summaries()
    compared = 0
    for host_writer, device_writer, prefix in ((host.dnn_summary_writer, device.dnn_summary_writer, 'dnn'),
                                               (host.gan_summary_writer, device.gan_summary_writer, 'gan')):
        host_scalars, device_scalars = logged(host_writer), logged(device_writer)
        assert sorted(host_scalars) == sorted(device_scalars)
        for tag, value in host_scalars.items():
            print(f'{prefix} {tag}: host {value!r} device {device_scalars[tag]!r}')
            assert_close(device_scalars[tag], value, rtol=RTOL, atol=1e-6, what=f'{prefix} {tag}')
            assert_close(device_scalars[tag], float(g[f'{prefix}/{tag}']), rtol=RTOL, atol=1e-6, what=f'{prefix} {tag} (g11)')
            compared += 1
    assert compared == 12
