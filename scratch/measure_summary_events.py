"""The records behind profiles/summary_events.md.

  python scratch/measure_summary_events.py device     srgan_tensor_histogram on the crowd discriminator's parameter arena at the
                                                      benchmark size (512 x 512) and on larger flat tensors, beside the download
                                                      of the same tensor: one JSON line per tensor
  python scratch/measure_summary_events.py host       the host time of encoding one crowd summary step's records (no GPU)
"""
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_RATE = 6.3e12          # B/s of a float4 copy, DESIGN.md section 3


def device():
    import torch
    import srgan_amd  # noqa: F401
    from srgan_amd import _lib, nn
    from srgan_amd.crowd.models import KnnDenseNetCat
    from srgan_amd.utility import seed_all
    seed_all(0)
    network = KnnDenseNetCat(image_size=512)
    nn.flatten_parameters(network, torch.device('cuda'))
    tensors = [('crowd D parameter arena, 512 x 512', network._srgan_arena.data)]
    for millions in (20, 137):
        tensors.append((f'{millions} M normal floats', torch.randn(millions * 10 ** 6, device='cuda')))
    tensors.append(('137 M equal floats (one hot bin)', torch.full((137 * 10 ** 6,), 0.25, device='cuda')))
    library, stream = _lib.library(), _lib.stream_handle()
    for name, tensor in tensors:
        out = torch.empty(66, dtype=torch.float64, device='cuda')
        for _ in range(3):
            _lib.check(library.srgan_tensor_histogram(tensor.data_ptr(), tensor.numel(), 30, out.data_ptr(), stream), 'histogram')
        torch.cuda.synchronize()
        times = []
        for _ in range(10):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            _lib.check(library.srgan_tensor_histogram(tensor.data_ptr(), tensor.numel(), 30, out.data_ptr(), stream), 'histogram')
            end.record()
            end.synchronize()
            times.append(start.elapsed_time(end) * 1e3)
        downloads = []
        for _ in range(3):
            torch.cuda.synchronize()
            begin = time.perf_counter()
            tensor.cpu()
            downloads.append((time.perf_counter() - begin) * 1e6)
        n = tensor.numel()
        print(json.dumps({'tensor': name, 'n': n, 'bins': 30, 'histogram_us_median': round(statistics.median(times), 1),
                          'histogram_us_min': round(min(times), 1), 'one_read_at_copy_rate_us': round(4 * n / COPY_RATE * 1e6, 1),
                          'two_reads_at_copy_rate_us': round(8 * n / COPY_RATE * 1e6, 1),
                          'download_us_median': round(statistics.median(downloads), 1), 'finite_count': float(out[4].item())}))


def host():
    """A crowd summary step with the pictures on writes, per writer, about twenty scalars and one map comparison picture
    [3, 680, 1132] (profiles/image_summaries.md); arena histograms would add three records of 30 bins per arena pair."""
    import numpy as np
    import srgan_amd  # noqa: F401
    from srgan_amd import summary_events
    generator = np.random.RandomState(0)
    ramp = np.linspace(0, 1, 1132, dtype=np.float32)[None, None, :] * np.ones((3, 680, 1), dtype=np.float32)
    picture = np.clip(ramp + generator.normal(0, 0.05, size=ramp.shape).astype(np.float32), 0, 1)
    record = summary_events.histogram_of_array(generator.standard_normal(10 ** 6).astype(np.float32), 30)
    with tempfile.TemporaryDirectory() as directory:
        for repeat in range(3):
            writer = summary_events.EventFileWriter(os.path.join(directory, str(repeat)))
            parts = {}
            begin = time.perf_counter()
            for index in range(40):
                writer.add_scalar('1 Validation Error/Scalar %d' % index, 0.5 * index, repeat)
            parts['40 scalars'] = time.perf_counter() - begin
            begin = time.perf_counter()
            for tag in ('Comparison/GAN', 'Comparison/DNN'):
                writer.add_image(tag, picture, repeat)
            parts['2 pictures [3, 680, 1132]'] = time.perf_counter() - begin
            begin = time.perf_counter()
            for index in range(6):
                writer.add_histogram('Parameters/%d' % index, record, repeat)
            parts['6 histograms of 30 bins'] = time.perf_counter() - begin
            writer.close()
            size = os.path.getsize(writer.path)
            begin = time.perf_counter()
            summary_events.crc32c(bytes(1 << 20))
            parts['crc32c of 1 MiB'] = time.perf_counter() - begin
            print(json.dumps({'repeat': repeat, 'file_bytes': size, 'encode_seconds': round(writer.encode_seconds, 4),
                              **{key: round(value, 4) for key, value in parts.items()}}))


if __name__ == '__main__':
    {'device': device, 'host': host}[sys.argv[1]]()
