"""One training iteration captured ONCE as a HIP graph and replayed (``settings.step_graph = True``).

An iteration of reference srgan.py:104-118 is ~5000 kernel launches whose arguments do not depend on the step: the
shapes are fixed, the parameters / gradient arenas / Adam moments live at fixed addresses, and the tape makes the same
decisions every time.  At 512x512 the GPU is the bottleneck and the Python tape hides behind it; at the reference's own
224x224 the host needs ~94 ms to enqueue ~75 ms of GPU work.  Capturing the iteration on a HIP stream
(``hipStreamBeginCapture`` through ``torch.cuda.graph``: every launch of libsrgan_hip.so goes to torch's current stream,
which is the capturing one) and replaying the instantiated graph removes the host from the loop.

What changes between iterations enters through fixed device buffers that are refreshed before each replay:
* the labeled / unlabeled batches (device-to-device copies into the captured input tensors);
* the three random draws, made on the HOST from the same streams and in the same order as the eager step (z for the
  discriminator step, alpha, z for the generator step), so a replayed run consumes the generators exactly as an eager one
  (with ``settings.device_random_draws`` they are filled on the device by launches captured with the step, from a device
  state the step advances: nothing is drawn on the host or copied, and only an injected draw enters through a buffer);
* Adam's update count, kept on the device (``Adam.count_on_device`` / ``srgan_adam_step_counted``).
With ``experiment.capture_loaders`` (both training loaders in device mode: their batches are launches whose arguments do not
depend on the step, ``device_batch()``) the iteration is handed the LOADERS instead of batches: the capture records their
launches in front of the step, a replay copies no input, and the image loaders' conditional rebuild of the epoch order is part
of the graph.  The loaders' states and orders are persistent buffers made before the capture (``prepare_capture``).

The side streams of the eager schedule (``settings.overlap_dnn_step`` / ``overlap_gradient_penalty`` /
``overlap_generator_forwards``) are captured too: a ``wait_stream`` on the capturing stream forks a chain into the capture,
the joins at the end of the step close it, and the instantiated graph holds the four chains as parallel branches -- they start
together on replay instead of in the order Python reaches them.

The 16-bit data path (``settings.storage_dtype``, round 7) replays too, on a single device.  Its weight shadows (blocked16.py)
are written in place by ONE batched launch per network behind each update, so the captured Adam -> refresh pairs keep them
current from replay to replay; ``blocked16.prepare`` makes every shadow buffer and job table exist before a capture (inside it
nothing may allocate or copy from the host), and masters written between two replays are caught by the shadows' host-side
version keys and re-rounded in front of the next replay.

Iterations whose host-side behaviour differs run eagerly: summary steps (they read losses back), and a graph is keyed
by everything the captured launches baked in (input shapes, whether the generator trains this step, learning rates, the
storage type and the loss scale).
Data-parallel runs (round 5): the exchanges are captured too when they are launches on streams this process owns -- the C
ABI's RCCL entry points on the communicator's stream (``parallel.AbiCommunicator``; forked into the capture by the event
wait in front of a collective, joined by the ``wait()`` of its work object) -- so that eight Python ranks on a 16-CPU
quota replay instead of enqueueing ~4000 launches each; every captured iteration ends with ALL pending optimizer updates
applied (the generator's exchange, which the eager loop hides under the next iteration's DNN step, completes inside the
graph).  Over gloo (host collectives) a data-parallel run stays eager.
"""
import gc

import torch

from . import functional as F
from .settings import option
from .tape import Var

# attributes a training step leaves on the experiment for summaries / tests; after a replay they must again refer to
# the captured tensors (an eager summary step in between rebinds them)
MAX_RECORDS = 4          # captured graphs kept per experiment (they share one memory pool)
STEP_OUTPUTS = ('last_losses', 'gradient_norm', 'labeled_features', 'unlabeled_features', 'fake_features',
                'interpolates_features')


def _copied_out(value):
    if isinstance(value, dict):
        return {key: _copied_out(item) for key, item in value.items()}
    if isinstance(value, Var):
        return Var(F._unary_raw(F.U_COPY, value.data))
    return value


def _flatten(value, out):
    if isinstance(value, (tuple, list)):
        for item in value:
            _flatten(item, out)
    elif value is not None:
        out.append(value)
    return out


def _rebuild(value, replacements):
    if isinstance(value, (tuple, list)):
        return tuple(_rebuild(item, replacements) for item in value)
    return None if value is None else next(replacements)


class CapturedIteration:
    def __init__(self, experiment):
        self.experiment = experiment
        self.records = {}
        self.eager_iterations = 0
        self.replays = 0
        self.input_copies = 0            # batch tensors copied into static buffers in front of replays (loaders captured: none)

    # -------------------------------------------------------------------------------------------------------------
    def optimizers(self):
        e = self.experiment
        return e.dnn_optimizer, e.d_optimizer, e.g_optimizer

    def order_side_streams(self):
        """Replays run on the current stream, eager iterations in between put the DNN step on its side stream without
        joining it (resident batches): at every switch between the two the streams wait for each other, so that an eager
        DNN step never runs next to a replay's and the other way round."""
        side = self.experiment._dnn_stream
        if side is not None:
            main = torch.cuda.current_stream()
            main.wait_stream(side)
            side.wait_stream(main)

    def eager(self, labeled_examples, labels, unlabeled_examples, step):
        e = self.experiment
        self.order_side_streams()
        e.dnn_training_step(labeled_examples, labels, step)
        e.gan_training_step(labeled_examples, labels, unlabeled_examples, step)
        self.eager_iterations += 1

    def loader_batches(self, loaders):
        """``(labeled examples, labels, unlabeled examples)`` of one ``device_batch()`` of each of the two loaders."""
        from .srgan import as_var
        labeled_loader, unlabeled_loader = loaders
        labeled_examples, labels = self.experiment.unpack_labeled(labeled_loader.device_batch())
        return labeled_examples, labels, as_var(unlabeled_loader.device_batch()[0])

    def run(self, labeled_examples, labels, unlabeled_examples, step, loaders=None):
        """One iteration on the given batches, or -- ``loaders``: the ``(train, unlabeled)`` loaders in device mode,
        ``experiment.captured_loaders()`` -- on batches the iteration cuts itself, inside the graph when it is replayed."""
        from .srgan import as_var
        e = self.experiment
        settings = e.settings
        inputs = None if loaders is not None else as_var((labeled_examples, labels, unlabeled_examples))
        for writer in (e.dnn_summary_writer, e.gan_summary_writer):
            writer.step = step
        summary = e.dnn_summary_writer.is_summary_step() or e.gan_summary_writer.is_summary_step()
        if summary or self.eager_iterations < int(option(settings, 'step_graph_warmup')) or \
                option(settings, 'reference_schedule'):
            return self.eager(*(inputs if loaders is None else self.loader_batches(loaders)), step)
        if loaders is None:
            flat = _flatten(inputs, [])
            shapes = tuple(tuple(v.shape) for v in flat)
        else:                          # no batch exists yet: the shapes the loaders will deliver, in the same order
            flat = []
            shapes = tuple(tuple(shape) for shape in loaders[0].batch_shapes()) + (tuple(loaders[1].batch_shapes()[0]),)
        generator_phase = step % settings.generator_training_step_period == 0
        # (the 16-bit path bakes its storage type into every launch and the static loss scale into the scaled backward)
        batch = shapes[-1][0]
        # host draws of THIS iteration, in the order the eager step makes them (srgan.py:286, :364, :301)
        # (a draw injected by a test is used once, exactly as the eager step would use it)
        # settings.device_random_draws: no host draw is made and none is copied -- the fills and the advance of the draws'
        # iteration count are launches captured with the step, and a replay consumes the next iteration of the device state
        # (eager iterations in between advance the same state); only an injected draw still enters through a buffer
        device_draws = e.device_random_draws()
        def drawn(name, draw):
            injected = e._take_draw(name)
            if injected is None:
                return None if device_draws else draw()
            return injected
        host = {'z_d': drawn('z_d', lambda: e.draw_discriminator_noise(batch)),
                'alpha': drawn('alpha', lambda: e.draw_interpolation_alpha(settings.batch_size))}
        if generator_phase:
            host['z_g'] = drawn('z_g', lambda: e.draw_generator_noise(batch))
        host = {name: value.reshape(-1) if name == 'alpha' else value for name, value in host.items() if value is not None}
        # (which draws enter through a buffer is baked in too: with device draws, only the injected ones)
        key = (shapes, generator_phase, F.COMPUTE_DTYPE,
               tuple(o.param_groups[0]['lr'] for o in self.optimizers()), option(settings, 'storage_dtype'),
               float(option(settings, 'loss_scale')), tuple(sorted(host)), loaders is not None)
        record = self.records.get(key)
        if record is not None and record['shadows'] != self.shadow_counts():
            # a weight shadow appeared since this capture (an eager summary step, a new phase): the captured refreshes do not
            # cover it, so the graph is captured again
            del self.records[key]
            record = None
        if record is None:
            record = self.records[key] = self.capture(inputs, flat, host, step, loaders)
        for target, source in zip(record['inputs'], flat):
            F._unary_raw(F.U_COPY, source.data, out=target.data)
            self.input_copies += 1
        for name, value in host.items():
            record['draws'][name].copy_(value, non_blocking=True)
        self.order_side_streams()
        # Masters written since the last step (a checkpoint load, a copy into an arena, a test editing the weights): their
        # 16-bit shadows are re-rounded here, on the replay's stream -- inside the graph they only follow the captured updates.
        self.refresh_stale_shadows()
        # An eager iteration in between (a summary step, a warm-up) may have left an optimizer update waiting for its
        # gradient exchange (``_pending_updates``); the captured ``finish_update`` was a no-op when it was recorded, so it is
        # settled here, before the replay overwrites those gradients.
        e.finish_update()
        record['graph'].replay()
        for optimizer, advanced in zip(self.optimizers(), record['advanced']):
            optimizer.step_count += advanced
        for loader in loaders or ():     # the recorded batches moved the loaders' device states on
            if hasattr(loader, 'replayed'):
                loader.replayed()
        # The step outputs (losses, features, gradient norms: a few hundred floats) are COPIED out of the graphs' shared
        # memory pool: a later replay -- of this graph or of another one that reuses the pool as scratch -- may overwrite
        # the static tensors, and a caller may keep an iteration's losses beyond the next one.
        for name, value in record['outputs'].items():
            setattr(e, name, _copied_out(value))
        self.replays += 1

    def arenas(self):
        e = self.experiment
        return [network._srgan_arena for network in (e.DNN, e.D, e.G) if getattr(network, '_srgan_arena', None) is not None]

    def shadow_counts(self):
        return tuple(len(getattr(arena, 'shadows', ())) for arena in self.arenas())

    def refresh_stale_shadows(self):
        from . import blocked16
        for arena in self.arenas():
            blocked16.refresh_if_stale(arena)

    def capture(self, inputs, flat, host, step, loaders=None):
        e = self.experiment
        device = flat[0].data.device if flat else torch.device('cuda', torch.cuda.current_device())
        static = [Var(torch.empty_like(v.data)) for v in flat]
        draws = {name: torch.empty(value.shape, dtype=torch.float32, device=device) for name, value in host.items()}
        optimizers = self.optimizers()
        for optimizer in optimizers:
            optimizer.count_on_device()
        before = [optimizer.step_count for optimizer in optimizers]
        if e.device_random_draws():
            e.device_draw_state()                             # exists before the capture: made inside it, it would be a host copy
        e.prepare_dropout_streams()                           # (the same for the networks' dropout states, settings.drop_rate)
        for loader in loaders or ():                          # (and for the loaders' states and epoch orders)
            loader.prepare_capture()
        static_inputs = _rebuild(inputs, iter(static)) if loaders is None else None
        injected, e.injected_draws = e.injected_draws, dict(draws)
        graph = torch.cuda.CUDAGraph()
        # ONE memory pool for every captured graph of this experiment: replays are strictly sequential and the step outputs
        # are read before the next replay, so the graphs (generator / no-generator phase, other learning rates, a ragged last
        # batch) can share their activation memory instead of holding a private copy each.
        pool = next(iter(self.records.values()))['graph'].pool() if self.records else None
        if len(self.records) >= MAX_RECORDS:                  # bounded: the oldest capture (and its tensors) goes
            self.records.pop(next(iter(self.records)))
        advanced = None
        e.join_dnn_stream()                                   # nothing eager in flight on a side stream the capture forks
        from . import blocked16
        for arena in self.arenas():                           # shadow buffers, bias rows and pack plans exist and are current:
            blocked16.prepare(arena)                          # the captured refreshes rewrite them in place
        # Cyclic garbage that holds a captured graph or its pool memory (the record evicted above, an experiment dropped by its
        # owner) must not be destroyed while a capture is under way: a graph's destructor calls the runtime, which aborts the
        # process inside a capture.  torch.cuda.graph no longer collects before capturing (torch.compiler.config.
        # force_cudagraph_gc), so it is done here, and the automatic collector stays off until the capture has ended.
        gc.collect()
        collecting = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(graph, pool=pool):
                if loaders is not None:                       # the batches are cut by launches recorded with the step
                    static_inputs = self.loader_batches(loaders)
                e.dnn_training_step(static_inputs[0], static_inputs[1], step)
                e.gan_training_step(static_inputs[0], static_inputs[1], static_inputs[2], step)
                # data parallel: a replay is a closed unit -- the generator's gradient exchange and update, which the
                # eager loop finishes when G is next used (under the next iteration's DNN step), end inside the graph
                e.finish_update()
            advanced = [optimizer.step_count - count for optimizer, count in zip(optimizers, before)]
        finally:
            if collecting:
                gc.enable()
            e.injected_draws = injected
            for optimizer, count in zip(optimizers, before):   # capturing recorded the launches, it did not run them
                optimizer.step_count = count                   # (also when the capture raised)
        outputs = {}
        for name in STEP_OUTPUTS:
            value = getattr(e, name, None)
            outputs[name] = dict(value) if isinstance(value, dict) else value
        # (the pack plans' device job tables are read by the captured refreshes: the record keeps them alive)
        plans = [getattr(arena, '_pack_plan', None) for arena in self.arenas()]
        # (batches: what the recorded loaders fill on every replay, kept so that nothing else in the pool takes their place)
        return dict(graph=graph, inputs=static, draws=draws, advanced=advanced, outputs=outputs, shadows=self.shadow_counts(),
                    plans=plans, batches=static_inputs if loaders is not None else None)
