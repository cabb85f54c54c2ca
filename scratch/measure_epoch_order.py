"""Measurements behind profiles/epoch_order.md (one MI355X; no rocprofv3 needed).

    python scratch/measure_epoch_order.py kernel                      # the rebuild kernel at n = 5 000, 50 000, 2^20
    python scratch/measure_epoch_order.py batch [--parent data.py]    # host time to enqueue one batch, modes alternated
    python scratch/measure_epoch_order.py run [--steps K]             # driving-fp16-shaped replayed run, capture_loaders off / on

``kernel``: device events around back-to-back ``srgan_epoch_order`` launches (unconditional) after a warm-up launch; the
median of the rounds.  ``batch``: a host clock around the calls that enqueue one batch, the device idle before and
synchronised after each window; ``--parent`` loads another revision's ``sr-gan_amd/data.py`` (``git show <rev>:...`` into a
file) as a third arm in the same process.  ``run``: bench.py's ``driving-fp16`` settings (64 x 192, batch 128, fp16 storage,
loss scale 256) over an in-memory database of 2 048 labeled and 2 048 unlabeled frames with device draws, step graph on; two
experiments in one process, timed windows alternated; ``host_ms_per_step`` is the host clock over a window's enqueues,
images/s the window's wall time after the synchronise."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import srgan_amd  # noqa: E402,F401
from srgan_amd import _lib  # noqa: E402
from srgan_amd.data import ResidentImageDataset, ResidentImageLoader, database_loaders  # noqa: E402
from srgan_amd.nn import draw_state  # noqa: E402


def measure_kernel(rounds):
    library, stream = _lib.library(), _lib.stream_handle()
    results = {}
    for n, launches in ((5000, 200), (50000, 20), (2 ** 20, 1)):
        state = draw_state(2 ** 40 + 17, 0)
        order = torch.empty(n, dtype=torch.int32, device='cuda')

        def launch():
            _lib.check(library.srgan_epoch_order(n, max(n // 128, 1), 0, 0x30002, state.data_ptr(), order.data_ptr(), stream),
                       'srgan_epoch_order')
        launch()
        torch.cuda.synchronize()
        times = []
        for _ in range(rounds if n < 2 ** 20 else max(rounds // 3, 2)):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(launches):
                launch()
            end.record()
            torch.cuda.synchronize()
            times.append(start.elapsed_time(end) / launches)
        assert sorted(order.cpu().tolist()) == list(range(n))
        results[n] = dict(median_ms=statistics.median(times), min_ms=min(times), max_ms=max(times), launches_per_round=launches,
                          rounds=len(times))
        print(f'srgan_epoch_order n = {n}: median {results[n]["median_ms"]:.4f} ms, min {results[n]["min_ms"]:.4f}, '
              f'max {results[n]["max_ms"]:.4f} ({len(times)} rounds of {launches})', flush=True)
    return results


def frames(count, shape, seed):
    generator = np.random.RandomState(seed)
    return ResidentImageDataset(generator.randint(0, 256, size=(count,) + shape).astype(np.uint8),
                                generator.uniform(-1, 1, size=count).astype(np.float32))


def measure_batch(parent, rounds, batches):
    """Host microseconds per batch: 64 x 192 frames, batch 128, 2 048 frames (16 batches per epoch)."""
    dataset = frames(2048, (3, 64, 192), 1).upload()
    arms = {'host': lambda: ResidentImageLoader(dataset, 128, seed=0),
            'device': lambda: ResidentImageLoader(dataset, 128, seed=0, draws='device')}
    if parent:
        spec = importlib.util.spec_from_file_location('srgan_amd.parent_data', parent)
        module = importlib.util.module_from_spec(spec)
        module.__package__ = 'srgan_amd'
        spec.loader.exec_module(module)
        arms['parent'] = lambda: module.ResidentImageLoader(dataset, 128, seed=0)
    iterators = {name: srgan_experiment_iter(make()) for name, make in arms.items()}
    samples = {name: [] for name in arms}
    for name, iterator in iterators.items():                     # warm-up: one epoch each
        for _ in range(16):
            next(iterator)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, iterator in iterators.items():
            torch.cuda.synchronize()
            begin = time.perf_counter()
            for _ in range(batches):
                batch = next(iterator)
            elapsed = time.perf_counter() - begin
            torch.cuda.synchronize()
            del batch
            samples[name].append(1e6 * elapsed / batches)
    results = {}
    for name, values in samples.items():
        results[name] = dict(median_us=statistics.median(values), min_us=min(values), max_us=max(values), rounds=rounds,
                             batches_per_round=batches)
        print(f'{name}: median {results[name]["median_us"]:.1f} us per batch, min {results[name]["min_us"]:.1f}, '
              f'max {results[name]["max_us"]:.1f} ({rounds} rounds of {batches} batches, epochs of 16)', flush=True)
    return results


def srgan_experiment_iter(loader):
    while True:
        for batch in loader:
            yield batch


def driving_experiment(capture_loaders):
    from srgan_amd.driving.srgan import DrivingExperiment
    from srgan_amd.settings import Settings
    from srgan_amd.utility import SummaryWriter, seed_all

    class InMemory(DrivingExperiment):
        image_batch_draws = 'device'

        def dataset_setup(self):
            database_loaders(self, (frames(2048, (3, 64, 192), 1), frames(2048, (3, 64, 192), 2), frames(128, (3, 64, 192), 3)),
                             self.image_size)

    settings = Settings()
    values = dict(batch_size=128, compute_dtype='f16', gradient_penalty_dtype='f32', storage_dtype='f16', loss_scale=256.0,
                  matching_loss_multiplier=1e2, contrasting_loss_multiplier=1e1, gradient_penalty_multiplier=1e2,
                  learning_rate=1e-4, blocked_fp32=True, step_graph=True, step_graph_warmup=2, device_random_draws=True,
                  overlap_dnn_step=True, overlap_generator_forwards=True, overlap_gradient_penalty=True, steps_to_run=10 ** 9)
    for key, value in values.items():
        setattr(settings, key, value)
    experiment = InMemory(settings)
    experiment.capture_loaders = capture_loaders
    experiment.image_size = (64, 192)
    seed_all(0)
    experiment.dataset_setup()
    experiment.model_setup()
    with torch.no_grad():
        for module in experiment.D.modules():
            if isinstance(module, (torch.nn.Conv2d, torch.nn.ConvTranspose2d, torch.nn.Linear)):
                module.weight.mul_(3.0)                          # bench.py's gp_scale of this workload
    experiment.gpu_mode()
    experiment.prepare_optimizers()
    experiment.train_mode()
    experiment.dnn_summary_writer = SummaryWriter(summary_period=10 ** 9)
    experiment.gan_summary_writer = SummaryWriter(summary_period=10 ** 9)
    experiment.start_loaders_at(1)
    experiment.next_step = 1
    experiment.batches = (experiment.infinite_iter(experiment.train_dataset_loader),
                          experiment.infinite_iter(experiment.unlabeled_dataset_loader))
    experiment.loaders = experiment.captured_loaders()
    assert (experiment.loaders is not None) == capture_loaders
    return experiment


def iterate(experiment, steps):
    from srgan_amd.srgan import as_var
    for _ in range(steps):
        step = experiment.next_step
        if experiment.loaders is not None:
            experiment.captured_iteration().run(None, None, None, step, loaders=experiment.loaders)
        else:
            examples, labels = experiment.unpack_labeled(next(experiment.batches[0]))
            experiment.training_iteration(examples, labels, as_var(next(experiment.batches[1])[0]), step)
        experiment.next_step += 1


def measure_run(steps, rounds):
    arms = {'copied inputs': driving_experiment(False), 'captured loaders': driving_experiment(True)}
    for experiment in arms.values():
        iterate(experiment, 6)                                   # two eager iterations, the capture, three replays
        torch.cuda.synchronize()
    samples = {name: [] for name in arms}
    for _ in range(rounds):
        for name, experiment in arms.items():
            torch.cuda.synchronize()
            begin = time.perf_counter()
            iterate(experiment, steps)
            host = time.perf_counter() - begin
            torch.cuda.synchronize()
            wall = time.perf_counter() - begin
            samples[name].append((1e3 * host / steps, 128 * steps / wall))
    results = {}
    for name, values in samples.items():
        captured = arms[name]._captured_iteration
        host, rate = [v[0] for v in values], [v[1] for v in values]
        results[name] = dict(host_ms_per_step_median=statistics.median(host), host_ms_per_step_min=min(host),
                             images_per_second_median=statistics.median(rate), images_per_second_min=min(rate),
                             images_per_second_max=max(rate), replays=captured.replays, input_copies=captured.input_copies,
                             eager_iterations=captured.eager_iterations, rounds=rounds, steps_per_round=steps)
        print(f'{name}: host {results[name]["host_ms_per_step_median"]:.3f} ms per step (min {min(host):.3f}), '
              f'{results[name]["images_per_second_median"]:.0f} images/s (min {min(rate):.0f}, max {max(rate):.0f}); '
              f'{captured.replays} replays, {captured.input_copies} input copies', flush=True)
    return results


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('what', choices=['kernel', 'batch', 'run'])
    parser.add_argument('--parent', default=None, help="another revision's sr-gan_amd/data.py, as a third arm of `batch`")
    parser.add_argument('--rounds', type=int, default=7)
    parser.add_argument('--batches', type=int, default=64)
    parser.add_argument('--steps', type=int, default=40)
    parser.add_argument('--out', default=None, help='write the results as JSON')
    args = parser.parse_args()
    assert torch.cuda.is_available(), 'these are measurements on the GPU'
    if args.what == 'kernel':
        results = measure_kernel(args.rounds)
    elif args.what == 'batch':
        results = measure_batch(args.parent, args.rounds, args.batches)
    else:
        results = measure_run(args.steps, args.rounds)
    if args.out:
        with open(args.out, 'w') as handle:
            json.dump({args.what: results}, handle, indent=1, default=str)


if __name__ == '__main__':
    main()
