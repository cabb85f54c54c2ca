"""settings.step_graph on the 16-bit data path (settings.storage_dtype; srgan_amd/graph.py, blocked16.py): a replayed iteration
of the age-vgg-bf16 and driving-fp16 configurations leaves the same losses, weights and Adam state as the eager tape, bit for
bit; the weight shadows stay current across replays, master writes between replays and record eviction; a capture that would
create a shadow is refused; the batched refresh that now covers every shadow kind equals the single-layer packers."""
import gc

import numpy as np
import pytest
import torch

from test_timed_schedule_gpu import bench_arguments

pytestmark = pytest.mark.gpu
LOSSES = ('dnn_loss', 'labeled_loss', 'unlabeled_loss', 'fake_loss', 'gradient_penalty', 'generator_loss')
FORMS = ('forward', 'transposed', 'down', 'up', 'bias_rows')


def _build(monkeypatch, workload, size, batch, step_graph, period=1):
    """The bench's experiment for ``workload`` (its settings: storage / compute / penalty dtypes, loss scale, GP scale) at a
    small size and batch, on ONE stream, with one eager warm-up iteration in front of the captures."""
    import bench
    monkeypatch.setitem(bench.WORKLOADS, workload, dict(bench.WORKLOADS[workload], batch_per_gpu=batch, image_size=size))
    args = bench_arguments(size, batch, workload=workload, step_graph=step_graph, single_stream=True)
    experiment = bench.build_experiment(args, None)
    experiment.settings.step_graph_warmup = 1
    experiment.settings.generator_training_step_period = period
    for optimizer in _optimizers(experiment):
        optimizer.count_on_device()        # both runs through the device-counted Adam entry point (a captured update needs it)
    return experiment


def _optimizers(experiment):
    return experiment.d_optimizer, experiment.g_optimizer, experiment.dnn_optimizer


def _run(monkeypatch, workload, size, batch, step_graph, iterations, period=1, between=None):
    import bench
    experiment = _build(monkeypatch, workload, size, batch, step_graph, period)
    labeled = experiment.infinite_iter(experiment.train_dataset_loader)
    unlabeled = experiment.infinite_iter(experiment.unlabeled_dataset_loader)
    losses = []
    for step in range(iterations):
        if between is not None:
            between(experiment, step)
        bench.one_step(experiment, labeled, unlabeled, step)
        losses.append({name: float(value.data.item()) for name, value in experiment.last_losses.items()
                       if value is not None and name in LOSSES})
    torch.cuda.synchronize()
    return experiment, losses


def _compare(eager, eager_losses, replayed, replayed_losses):
    for step, (a, b) in enumerate(zip(eager_losses, replayed_losses)):
        assert a == b, f'iteration {step}: {a} vs {b}'               # every loss of every iteration, bit for bit
    assert all(np.isfinite(v) for v in eager_losses[-1].values())
    assert eager_losses[-1]['gradient_penalty'] > 0.0                  # the penalty is active
    for name in ('D', 'DNN', 'G'):
        a, b = getattr(eager, name)._srgan_arena.data, getattr(replayed, name)._srgan_arena.data
        assert torch.equal(a, b), (name, float((a - b).abs().max()))
    for a, b in zip(_optimizers(eager), _optimizers(replayed)):
        assert a.step_count == b.step_count and int(b.device_state[0]) == b.step_count
        assert torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)


def _shadows(experiment):
    return [shadow for name in ('D', 'DNN', 'G') for shadow in getattr(experiment, name)._srgan_arena.shadows]


def _check_shadows_current(experiment, monkeypatch):
    """Every shadow buffer equals a fresh single-layer pack of the current masters, bit for bit (the bias rows included)."""
    torch.cuda.synchronize()
    shadows = _shadows(experiment)
    held = [[(name, getattr(s, name).clone()) for name in FORMS if getattr(s, name) is not None] for s in shadows]
    monkeypatch.setenv('SRGAN_H_NO_BATCHED_PACK', '1')
    for s in shadows:
        s.repack()
    monkeypatch.delenv('SRGAN_H_NO_BATCHED_PACK')
    torch.cuda.synchronize()
    rows = 0
    for s, forms in zip(shadows, held):
        for name, before in forms:
            assert torch.equal(before, getattr(s, name)), (s.kind, s.code, name)
            rows += name == 'bias_rows'
    return rows


def test_age_vgg_bf16_replay_matches_the_eager_tape(monkeypatch):
    """configs[1] (bf16 storage, compute and penalty) at 64 x 64, batch 8: six iterations, five of them replayed."""
    eager, eager_losses = _run(monkeypatch, 'age-vgg-bf16', 64, 8, False, 6)
    replayed, replayed_losses = _run(monkeypatch, 'age-vgg-bf16', 64, 8, True, 6)
    captured = replayed._captured_iteration
    assert captured.replays == 5 and captured.eager_iterations == 1 and len(captured.records) == 1
    assert getattr(eager, '_captured_iteration', None) is None
    _compare(eager, eager_losses, replayed, replayed_losses)
    assert eager_losses[-1] != eager_losses[-2]                       # the replays consumed new batches and draws


def test_driving_fp16_replay_with_two_records_matches_the_eager_tape(monkeypatch):
    """configs[4] (fp16 storage, static loss scale 256, fp32 penalty chain) at 64 x 192, batch 4; the generator trains every
    second iteration: two captured graphs in one pool."""
    eager, eager_losses = _run(monkeypatch, 'driving-fp16', (64, 192), 4, False, 6, period=2)
    replayed, replayed_losses = _run(monkeypatch, 'driving-fp16', (64, 192), 4, True, 6, period=2)
    captured = replayed._captured_iteration
    assert captured.replays == 5 and len(captured.records) == 2
    assert replayed.settings.loss_scale == 256.0
    assert replayed.g_optimizer.step_count == 3
    _compare(eager, eager_losses, replayed, replayed_losses)


def test_shadows_stay_current_across_replays_and_master_writes(monkeypatch):
    """After replays every shadow (G's seed-layer bias rows included) is the pack of the current masters; masters written
    between two replays (D and G scaled in place) reach the next replay's forwards exactly as they reach the eager tape's."""
    def write(experiment, step):
        if step == 4:
            with torch.no_grad():
                experiment.D._srgan_arena.data.mul_(0.995)
                experiment.G._srgan_arena.data.mul_(1.01)

    eager, eager_losses = _run(monkeypatch, 'age-vgg-bf16', 64, 8, False, 7, between=write)
    replayed, replayed_losses = _run(monkeypatch, 'age-vgg-bf16', 64, 8, True, 4)
    assert _check_shadows_current(replayed, monkeypatch) >= 1           # after three replays
    replayed, replayed_losses = _run(monkeypatch, 'age-vgg-bf16', 64, 8, True, 7, between=write)
    assert replayed._captured_iteration.replays == 6
    _compare(eager, eager_losses, replayed, replayed_losses)
    assert _check_shadows_current(replayed, monkeypatch) >= 1


def test_record_eviction_keeps_the_results_of_the_eager_tape(monkeypatch):
    """Six learning rates in turn: more keys than graph.MAX_RECORDS, so records are evicted and captured again."""
    from srgan_amd import graph

    def learning_rate(experiment, step):
        for optimizer in _optimizers(experiment):
            optimizer.param_groups[0]['lr'] = 1e-4 * (1.0 + 0.1 * (step % 6))

    iterations = 9
    eager, eager_losses = _run(monkeypatch, 'driving-fp16', (64, 192), 4, False, iterations, between=learning_rate)
    replayed, replayed_losses = _run(monkeypatch, 'driving-fp16', (64, 192), 4, True, iterations, between=learning_rate)
    captured = replayed._captured_iteration
    assert captured.replays == iterations - 1 and len(captured.records) == graph.MAX_RECORDS
    _compare(eager, eager_losses, replayed, replayed_losses)


def test_a_capture_that_would_create_a_shadow_is_refused():
    """A layer never run before, run inside a capture, would allocate its shadow from the graph's pool and copy from the host:
    the RuntimeError comes before any launch is recorded."""
    import srgan_amd  # noqa: F401
    from srgan_amd import blocked16 as B
    from srgan_amd import functional as F
    module = torch.nn.Conv2d(16, 16, 3, padding=1).cuda()
    x = B.pack(F.leaf(torch.rand(2, 16, 8, 8).cuda()), 1)
    torch.cuda.synchronize()
    gc.collect()              # the graphs of earlier tests' experiments are destroyed here, not inside the capture below
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match='during a HIP graph capture'):
        with torch.cuda.graph(graph):
            B.conv3x3(x, module, 0.0)
    assert not getattr(module, '_srgan_shadows', None)
    torch.cuda.synchronize()
    y = B.conv3x3(x, module, 0.0)                                       # the same layer eagerly, afterwards
    torch.cuda.synchronize()
    assert bool(torch.isfinite(B.unpack(y).data).all())


@pytest.mark.parametrize('workload, size', [('age-vgg-bf16', 64), ('driving-fp16', (64, 192))])
def test_batched_refresh_of_every_shadow_kind_equals_the_single_layer_packers(monkeypatch, workload, size):
    """``refresh(arena)`` re-rounds the convolution, matrix and seed-layer shadows and the bias rows of a network in ONE
    srgan_h_pack_batched launch, bit-identical to the single-layer packers (bf16 and fp16)."""
    import bench
    from srgan_amd import blocked16 as B
    experiment = _build(monkeypatch, workload, size, 4, False)
    labeled = experiment.infinite_iter(experiment.train_dataset_loader)
    unlabeled = experiment.infinite_iter(experiment.unlabeled_dataset_loader)
    bench.one_step(experiment, labeled, unlabeled, 0)                   # every shadow of the step exists
    torch.cuda.synchronize()
    kinds = {s.kind for s in _shadows(experiment)}
    assert {'linear_t', 'k4s2'} <= kinds and ('conv3x3' in kinds) == (workload == 'age-vgg-bf16')
    assert any(s.bias_rows is not None for s in _shadows(experiment))
    checked = 0
    for name in ('D', 'DNN', 'G'):
        arena = getattr(experiment, name)._srgan_arena
        with torch.no_grad():
            arena.data.mul_(1.37).add_(0.01)
        monkeypatch.setenv('SRGAN_H_NO_BATCHED_PACK', '1')
        B.refresh(arena)
        monkeypatch.delenv('SRGAN_H_NO_BATCHED_PACK')
        single = [[(form, getattr(s, form).clone()) for form in FORMS if getattr(s, form) is not None] for s in arena.shadows]
        for s in arena.shadows:
            for form in FORMS:
                if getattr(s, form) is not None:
                    getattr(s, form).fill_(-1)
        calls = []
        real_call = B._call
        monkeypatch.setattr(B, '_call', lambda entry, *args: (calls.append(entry), real_call(entry, *args)))
        B.refresh(arena)
        monkeypatch.setattr(B, '_call', real_call)
        assert calls == ['srgan_h_pack_batched'], calls
        assert not B.stale(arena)
        torch.cuda.synchronize()
        for s, forms in zip(arena.shadows, single):
            for form, want in forms:
                assert torch.equal(getattr(s, form), want), (name, s.kind, s.code, form)
                checked += 1
    assert checked >= 10
