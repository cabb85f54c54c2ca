"""Time the fused correlation feature loss (F.feature_corrcoef_l1, csrc/feature_losses.hip) and, at shapes where it fits, the
same loss composed from the materialised ``feature_corrcoef`` (F.mm + elementwise tape operations): forward + backward to both
inputs, device events around ``--repeats`` calls after ``--warmup`` calls, torch's peak allocated memory of one call.  Prints one
JSON line per shape.  ``--fused-only`` is the form to run under ``rocprofv3 --kernel-trace --stats`` (a run of its own).

    python scratch/bench_feature_losses.py --shapes 600x4096 600x32768 5000x10 --composed 600x4096 5000x10
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import srgan_amd  # noqa: E402,F401
from srgan_amd import functional as F, srgan  # noqa: E402
from srgan_amd.tape import backward  # noqa: E402

PEAK_FP32_MFMA = 157.3e12


def composed_loss(base, other):
    return F.sum_all(F.abs_(F.sub(srgan.feature_corrcoef(base), srgan.feature_corrcoef(other))))


def one_call(function, x, y):
    base, other = F.leaf(x, requires_grad=True), F.leaf(y, requires_grad=True)
    loss = function(base, other)
    grads = backward(loss, inputs=[base, other])
    return loss, grads


def measure(function, x, y, warmup, repeats):
    for _ in range(warmup):
        one_call(function, x, y)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    one_call(function, x, y)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        one_call(function, x, y)
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    times.sort()
    return {'median_ms': times[len(times) // 2], 'min_ms': times[0], 'max_ms': times[-1], 'peak_bytes_of_a_call': int(peak)}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--shapes', nargs='+', default=['600x4096'])
    parser.add_argument('--composed', nargs='*', default=[])
    parser.add_argument('--fused-only', action='store_true')
    parser.add_argument('--warmup', type=int, default=2)
    parser.add_argument('--repeats', type=int, default=5)
    arguments = parser.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the MI355X'
    for shape in arguments.shapes:
        batch, features = (int(v) for v in shape.split('x'))
        generator = torch.Generator().manual_seed(batch + features)
        x = torch.randn(batch, features, generator=generator).cuda()
        y = (1.5 * torch.randn(batch, features, generator=generator) + 0.3).cuda()
        result = {'shape': [batch, features], 'fused': measure(srgan.feature_covariance_loss, x, y, arguments.warmup, arguments.repeats)}
        # executed flops: 2 F^2 B per Gram matrix formed (padding not counted): the forward forms 2; the backward, per side, forms
        # 2 once per 128 examples and multiplies G into Z once (2 F^2 B)
        gram = 2.0 * features * features * batch
        chunks = -(-batch // 128)
        result['fused']['flops'] = gram * (2 + 2 * (2 * chunks + 1))
        result['fused']['share_of_fp32_mfma_peak_end_to_end'] = result['fused']['flops'] / (result['fused']['median_ms'] * 1e-3) / PEAK_FP32_MFMA
        if shape in arguments.composed and not arguments.fused_only:
            result['composed'] = measure(composed_loss, x, y, arguments.warmup, arguments.repeats)
            fused_loss = float(srgan.feature_covariance_loss(F.constant(x), F.constant(y)).data.cpu()[0])
            composed = float(composed_loss(F.constant(x), F.constant(y)).data.cpu()[0])
            result['loss'] = {'fused': fused_loss, 'composed': composed}
        print(json.dumps(result), flush=True)


if __name__ == '__main__':
    main()
