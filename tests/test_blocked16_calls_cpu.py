"""The host side of the blocked 16-bit path (``blocked16.py``) pinned call by call, on the CPU: which buffers a weight shadow
of every kind allocates, what its single-layer packers and its jobs of the batched refresh are handed, and the argument lists
of the contraction launch (both directions, every epilogue) and of the weight gradient.  ``B._call`` is replaced by a recorder
and ``F._stream`` by a stub, so no kernel runs: modules and tensors live on the CPU and the job fillers never dereference
their pointers.

The transcript is compared with ``golden/blocked16_calls.json``, recorded by this file (``python
tests/test_blocked16_calls_cpu.py > tests/golden/blocked16_calls.json``) at the commit BEFORE the shadow kinds became classes,
where the first two adapters below read ``B.Shadow(module, kind, code, in_blocked, plane)`` and ``B._launch(x, shadow.module,
shadow, transposed, epi, slope, ref, bias)``; nothing in it comes from the code under test.

An entry is the entry point's name and its arguments; a pointer is replaced by what it points at -- [shadow index (jobs
only), the tensor's role, byte offset] -- and the stream by 'stream'.  The cases are the smallest at which each piece of
geometry can go wrong: channel tails below a group, groups of 4 in code 0, a non-square seed kernel, a flattened input with
a padded channel count, both module classes of the 4x4 / stride 2 family."""
import json
import os
import struct

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'blocked16_calls.json')
STREAM = 0x5712EA00
BUFFERS = ('forward', 'transposed', 'down', 'up', 'bias_rows')

# name, the layer, shadow kind, code, (in_blocked, plane), forward input (c, h, w[, plane, real]), output-side tensor (c, h, w)
CASES = [
    ('conv3x3_bf16', lambda: torch.nn.Conv2d(20, 24, 3, padding=1), 'conv3x3', 1, (0, 1), (20, 6, 10), (24, 6, 10)),
    ('conv4x4s2_fp16', lambda: torch.nn.Conv2d(3, 16, 4, 2, 1), 'k4s2', 2, (0, 1), (3, 8, 12), (16, 4, 6)),
    ('conv4x4s2_f32', lambda: torch.nn.Conv2d(3, 16, 4, 2, 1), 'k4s2', 0, (0, 1), (3, 8, 12), (16, 4, 6)),
    ('conv_transpose4x4s2_bf16', lambda: torch.nn.ConvTranspose2d(24, 12, 4, 2, 1), 'k4s2', 1, (0, 1), (24, 3, 5), (12, 6, 10)),
    ('linear_flattened_bf16', lambda: torch.nn.Linear(40, 10), 'linear', 1, (64, 4), (64, 1, 1, 4, 40), (10, 1, 1)),
    ('linear_fp16', lambda: torch.nn.Linear(20, 3), 'linear', 2, (24, 1), (24, 1, 1), (3, 1, 1)),
    ('seed_bf16', lambda: torch.nn.ConvTranspose2d(20, 12, (2, 3), 1, 0), 'linear_t', 1, (0, 1), (20, 1, 1), (12, 2, 3)),
]
BATCH = 2


# ------------------------------------------------------------------------------------------------ the adapters
def make_shadow(B, module, kind, code, in_blocked, plane):
    return B.SHADOW_KINDS[kind](module, code, in_blocked, plane)


def launch(B, shadow, x, transposed, epi, slope, ref, bias):
    return shadow.launch(x, transposed, epi, slope, ref, bias)


def weight_gradient(B, shadow, x_side, y_side, into):
    return B._weight_gradient(shadow, shadow.module, x_side, y_side, into)


# ------------------------------------------------------------------------------------------------ recording
def _blocked(B, code, c, h, w, plane=1, real=None):
    from srgan_amd.tape import Var
    group = B.group_size(code)
    x = Var(torch.zeros(BATCH, (c + group - 1) // group, h, w, group, dtype=B.TORCH_DTYPE[code]))
    x.meta = B.Blocked(BATCH, c, h, w, code, plane=plane, real=real)
    return x


def _roles(shadow, **tensors):
    roles = [('weight', shadow.module.weight), ('bias', shadow.module.bias)]
    roles += [(name, getattr(shadow, name, None)) for name in BUFFERS] + list(tensors.items())
    return [(role, tensor) for role, tensor in roles if tensor is not None]


def _resolve(pointer, roles, index=None):
    """What ``pointer`` points at: [role, byte offset] of the live tensor that holds it ([shadow index, role, offset] for a
    job of the plan)."""
    for role, tensor in roles:
        offset = pointer - tensor.data_ptr()
        if 0 <= offset < max(1, tensor.numel() * tensor.element_size()):
            return [role, offset] if index is None else [index, role, offset]
    raise AssertionError(f'a pointer to no tensor of the case: {pointer:#x}')


def _entries(raw, roles):
    import ctypes
    from srgan_amd import _lib
    entries = []
    for name, args in raw:
        kinds = _lib.SIGNATURES[name][0]
        assert len(kinds) == len(args), name
        entry = [name]
        for kind, value in zip(kinds, args):
            if kind is ctypes.c_void_p and value is not None:
                value = 'stream' if value == STREAM else _resolve(value, roles)
            entry.append(value)
        entries.append(entry)
    del raw[:]
    return entries


def _buffers(shadow):
    return {name: [str(getattr(shadow, name).dtype), getattr(shadow, name).numel()]
            for name in BUFFERS if getattr(shadow, name, None) is not None}


def _meta(meta):
    return [meta.n, meta.c, meta.h, meta.w, meta.code, meta.plane, meta.real]


def _error(call):
    with pytest.raises(ValueError) as caught:
        call()
    return str(caught.value)


def _case(B, raw, shadow, code, x_shape, y_shape):
    """(a), (c) - (f) of one case: everything but its jobs in the plan."""
    from srgan_amd.tape import Var
    module = shadow.module
    out = {}
    shadow.repack()
    out['repack'] = _entries(raw, _roles(shadow))
    out['buffers'] = _buffers(shadow)
    x, y, ref = _blocked(B, code, *x_shape), _blocked(B, code, *y_shape), _blocked(B, code, *x_shape).data
    bias = None if module.bias is None else Var(module.bias.data)

    def run(key, source, transposed, epi, slope, reference, b):
        data, meta = launch(B, shadow, source, transposed, epi, slope, reference, b)
        out[key] = {'calls': _entries(raw, _roles(shadow, input=source.data, output=data, reference=reference)),
                    'output': [str(data.dtype), list(data.shape)], 'meta': _meta(meta)}
    run('forward_epi1', x, False, 1, 0.05, None, bias)
    run('data_gradient_epi2', y, True, 2, 0.5, ref, None)
    run('data_gradient_epi0', y, True, 0, 1.0, None, None)
    into = torch.zeros_like(module.weight.data)
    weight_gradient(B, shadow, x, y, into)
    out['weight_gradient'] = _entries(raw, _roles(shadow, x_side=x.data, y_side=y.data, into=into))
    wrong_x = _blocked(B, code, x_shape[0] + 8, *x_shape[1:])
    wrong_y = _blocked(B, code, y_shape[0] + 8, *y_shape[1:])
    out['wrong_channels'] = [_error(lambda: launch(B, shadow, wrong_x, False, 1, 0.05, None, bias)),
                             _error(lambda: launch(B, shadow, wrong_y, True, 0, 1.0, None, None))]
    assert not raw
    return out


def _plan(B, shadows):
    """(b): the jobs of a plan over ``shadows`` (fresh ones: the plan allocates their buffers), per shadow in table order."""
    plan = B._PackPlan(shadows)
    roles = [(index, _roles(shadow)) for index, shadow in enumerate(shadows)]
    table = plan.table.numpy().tobytes()
    assert len(table) == 80 * plan.count
    jobs = [[] for _ in shadows]
    for at in range(plan.count):
        w, packed, slots, first_block, kind, prec, *p = struct.unpack_from('<QQqqii10i', table, 80 * at)
        owner = next(index for index, own in roles if any(t.data_ptr() <= packed < t.data_ptr() + t.numel() * t.element_size()
                                                          for role, t in own if role in BUFFERS))
        own = roles[owner][1]
        jobs[owner].append({'at': at, 'slots': slots, 'first_block': first_block, 'kind': kind, 'prec': prec, 'p': p,
                            'w': _resolve(w, own, owner), 'packed': _resolve(packed, own, owner)})
    return {'count': plan.count, 'blocks': plan.blocks, 'jobs': jobs, 'buffers': [_buffers(shadow) for shadow in shadows]}


def transcript(monkeypatch=None):
    import srgan_amd  # noqa: F401
    from srgan_amd import blocked16 as B, functional as F
    raw = []
    record, stream = (lambda name, *args: raw.append((name, args))), (lambda: STREAM)
    if monkeypatch is None:
        B._call, F._stream = record, stream
    else:
        monkeypatch.setattr(B, '_call', record)
        monkeypatch.setattr(F, '_stream', stream)
    torch.manual_seed(0)
    modules = [case[1]() for case in CASES]
    out = {'cases': {}}
    for module, (name, _, kind, code, form, x_shape, y_shape) in zip(modules, CASES):
        shadow = make_shadow(B, module, kind, code, *form)
        assert (shadow.kind, shadow.code) == (kind, code)
        out['cases'][name] = _case(B, raw, shadow, code, x_shape, y_shape)
        if name == 'seed_bf16':
            out['seed'] = (shadow.bias_rows.clone(), module.bias.data.clone())
    out['plan'] = _plan(B, [make_shadow(B, module, case[2], case[3], *case[4]) for module, case in zip(modules, CASES)])
    assert not raw
    return out


# ------------------------------------------------------------------------------------------------ the tests
@pytest.fixture(scope='module')
def recorded():
    patch = pytest.MonkeyPatch()
    try:
        return transcript(patch)
    finally:
        patch.undo()


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as handle:
        return json.load(handle)


@pytest.mark.parametrize('name', [case[0] for case in CASES])
@pytest.mark.parametrize('part', ['repack', 'buffers', 'forward_epi1', 'data_gradient_epi2', 'data_gradient_epi0',
                                  'weight_gradient', 'wrong_channels'])
def test_calls_of_a_shadow_kind(recorded, golden, name, part):
    got = json.loads(json.dumps(recorded['cases'][name][part]))
    assert got == golden['cases'][name][part]


def test_jobs_of_the_batched_refresh(recorded, golden):
    got = json.loads(json.dumps(recorded['plan']))
    assert (got['count'], got['blocks']) == (golden['plan']['count'], golden['plan']['blocks'])
    assert got['buffers'] == golden['plan']['buffers']
    for index, case in enumerate(CASES):
        assert got['jobs'][index] == golden['plan']['jobs'][index], case[0]


def test_bias_rows_of_the_seed_layer(recorded):
    """rows[g, p, j] == bias[8 g + j], zero behind the last channel: the single-layer form is a torch copy."""
    rows, bias = recorded['seed']
    channels, plane = 12, 6
    assert rows.dtype == torch.float32 and rows.numel() == (channels + 7) // 8 * plane * 8
    want = torch.zeros((channels + 7) // 8 * 8)
    want[:channels] = bias
    assert torch.equal(rows.view(-1, plane, 8), want.view(-1, 1, 8).expand(-1, plane, 8))


if __name__ == '__main__':
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    result = transcript()
    del result['seed']
    json.dump(result, sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write('\n')
