"""Timing of one crowd validation_summaries call (the four evaluation epochs; the full-image walk is left out by clearing
dataset_class) from a synthetic resident database: the device path against the host path fed the same patches.

  python scratch/measure_crowd_validation.py time                 five alternating calls per path and size, one JSON line each
  python scratch/measure_crowd_validation.py profile SIZE BATCH   one device-path call: run it under
                                                                  rocprofv3 --kernel-trace --stats --output-format csv -d DIR
  python scratch/measure_crowd_validation.py summarise DIR        the crowd_evaluation dispatches of the kernel trace in DIR

profiles/crowd_validation.md holds the numbers."""
import csv
import glob
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_database(directory, seed=4):
    import numpy as np
    generator = np.random.RandomState(seed)
    for split, count in (('train', 4), ('test', 2)):
        for index in range(count):
            shape = (640 + 16 * index, 768)
            arrays = {'images': generator.randint(0, 256, size=shape + (3,)).astype(np.uint8),
                      'labels': (generator.rand(*shape) < 0.0004).astype(np.float32),
                      'i1nn_maps': generator.rand(*shape).astype(np.float32)}
            for kind, array in arrays.items():
                os.makedirs(os.path.join(directory, 'part_A', split + '_data', kind), exist_ok=True)
                np.save(os.path.join(directory, 'part_A', split + '_data', kind, 'IMG_%d.npy' % index), array)


def make_experiment(directory, size, batch):
    import srgan_amd  # noqa: F401
    from srgan_amd.settings import Settings
    from srgan_amd.crowd.srgan import CrowdExperiment
    from srgan_amd.utility import seed_all
    os.environ['SRGAN_CROWD_DATABASE'] = directory
    os.environ['SRGAN_CROWD_DATABASE_PART'] = 'part_A'
    settings = Settings()
    for key, value in dict(batch_size=batch, image_patch_size=size, labeled_dataset_size=4, unlabeled_dataset_size=4,
                           test_summary_size=None, crowd_validation='device').items():
        setattr(settings, key, value)
    experiment = CrowdExperiment(settings)
    experiment.dataset_setup()
    seed_all(0)
    experiment.model_setup()
    experiment.gpu_mode()
    experiment.prepare_optimizers()
    experiment.eval_mode()
    experiment.dataset_class = None          # the full-image test walk is the same code on both paths: left out
    return experiment


def one_call(experiment, sets):
    import torch
    from srgan_amd.utility import SummaryWriter
    experiment.train_dataset, experiment.validation_dataset = sets
    experiment.dnn_summary_writer, experiment.gan_summary_writer = SummaryWriter(), SummaryWriter()
    torch.cuda.synchronize()
    start = time.perf_counter()
    experiment.validation_summaries(0)
    torch.cuda.synchronize()
    elapsed = (time.perf_counter() - start) * 1e3
    scalars = {}
    for prefix, writer in (('dnn', experiment.dnn_summary_writer), ('gan', experiment.gan_summary_writer)):
        scalars.update({prefix + ' ' + tag: values[-1][1] for tag, values in writer.scalars.items()})
    return elapsed, scalars


def main_time():
    with tempfile.TemporaryDirectory() as directory:
        write_database(directory)
        for size, batch in ((224, 15), (512, 16)):
            experiment = make_experiment(directory, size, batch)
            device_sets = (experiment.train_dataset, experiment.validation_dataset)
            host_sets = tuple([tuple(part.cpu() for part in dataset[index]) for index in range(len(dataset))]
                              for dataset in device_sets)
            one_call(experiment, device_sets)            # warm-up of every shape on both paths
            one_call(experiment, host_sets)
            device, host = [], []
            for _ in range(5):                           # alternating
                elapsed, device_scalars = one_call(experiment, device_sets)
                device.append(elapsed)
                elapsed, host_scalars = one_call(experiment, host_sets)
                host.append(elapsed)
            worst = max(abs(device_scalars[tag] - host_scalars[tag]) / max(abs(host_scalars[tag]), 1e-300)
                        for tag in host_scalars)
            print(json.dumps(dict(
                configuration='%dx%d batch %d' % (size, size, batch), patches_per_set=len(device_sets[0]), device_ms=device,
                host_ms=host, device_median=statistics.median(device), host_median=statistics.median(host),
                worst_relative_scalar_difference=worst, scalars=len(host_scalars))), flush=True)
            del experiment, device_sets, host_sets


def main_profile(size, batch):
    with tempfile.TemporaryDirectory() as directory:
        write_database(directory)
        experiment = make_experiment(directory, size, batch)
        print('profiled call: %.1f ms' % one_call(experiment, (experiment.train_dataset, experiment.validation_dataset))[0])


def main_summarise(directory):
    for path in glob.glob(os.path.join(directory, '**', '*kernel_trace.csv'), recursive=True):
        rows = [row for row in csv.DictReader(open(path)) if 'crowd_evaluation' in row['Kernel_Name']]
        for row in rows:
            name = 'finish' if 'finish' in row['Kernel_Name'] else 'partials'
            print(path, name, 'grid', row.get('Grid_Size_X', row.get('Grid_Size')), 'ns',
                  int(row['End_Timestamp']) - int(row['Start_Timestamp']))


if __name__ == '__main__':
    if sys.argv[1] == 'time':
        main_time()
    elif sys.argv[1] == 'profile':
        main_profile(int(sys.argv[2]), int(sys.argv[3]))
    else:
        main_summarise(sys.argv[2])
