"""The tables and references of the streaming-kernel tests (streaming_cases.py) on the CPU, no library needed: every float64
reference agrees with torch's own fp32 op to fp32 rounding, the exact-operand cases meet their precondition, and every table
entry reaches the branch it is named for -- re-derived from the hosts' constants, so that a changed constant (or an edited
table) fails here instead of quietly un-covering a kernel.  That holds for all of pool.hip too: the fused norm -> relu -> pool
references against torch's autograd in float64, the workgroups per plane and the ordered / atomic choice of every fused case,
and the kernel srgan_maxpool2d_bwd takes at every window alignment."""
import math

import pytest
import torch
import torch.nn.functional as TF

import streaming_cases as S


def close32(reference64, torch32, what, ulps=2.0):
    error = S.ulp_error(torch32, reference64)
    assert float(error.max()) <= ulps, f'{what}: torch fp32 is {float(error.max()):.2f} ulp from the float64 reference'


# ------------------------------------------------------------------------------------------------- references vs torch
@pytest.mark.parametrize('name', S.UNARY)
def test_unary_references_agree_with_torch(name):
    gen = S.generator('cpu-unary', name)
    x = torch.cat([S.ints((257,), S.X, gen), S.full_mantissa(257, gen)])
    if name in ('sqrt', 'log', 'log1p', 'pow', 'rsqrt', 'reciprocal'):
        x = (x.abs() + 0.25).float().double()
    p0, p1 = {'affine': S.AFFINE_P, 'pow': (1.5, 0.0), 'leaky': (S.LEAKY_SLOPE, 0.0)}.get(name, (0.0, 0.0))
    if name in S.UNARY_FMA:                                 # two roundings in torch: exactly the unfused form
        assert torch.equal(S.two_roundings(name, x, None, p0, p1), S.torch_unary(name, x, p0, p1).double())
        return
    close32(S.unary_ref(name, x, p0, p1), S.torch_unary(name, x, p0, p1), name,
            ulps=4.0 if name in S.TRANSCENDENTAL else 2.0 if name in ('rsqrt', 'reciprocal') else 1.0 if name == 'sqrt' else 0.5)


@pytest.mark.parametrize('name', S.BINARY)
def test_binary_references_agree_with_torch(name):
    gen = S.generator('cpu-binary', name)
    a = torch.cat([S.ints((257,), S.X, gen), S.full_mantissa(257, gen)])
    b = torch.cat([S.ints((257,), S.X, gen), S.full_mantissa(257, gen)])
    p0 = {'leaky_mask_mul': S.LEAKY_SLOPE, 'axpy': S.AXPY_P}.get(name, 0.0)
    if name == 'axpy':
        assert torch.equal(S.two_roundings(name, a, b, p0), S.torch_binary(name, a, b, p0).double())
        return
    close32(S.binary_ref(name, a, b, p0), S.torch_binary(name, a, b, p0), name, ulps=0.5)


def test_special_values_follow_torch_except_under_the_nan_rule():
    x = torch.tensor(S.SPECIALS, dtype=torch.float64)
    for name in S.UNARY:
        p0 = {'affine': S.AFFINE_P[0], 'pow': 1.5, 'leaky': S.LEAKY_SLOPE}.get(name, 0.0)
        p1 = S.AFFINE_P[1] if name == 'affine' else 0.0
        ours, theirs = S.unary_ref(name, x, p0, p1), S.torch_unary(name, x, p0, p1).double()
        differs = [S.SPECIALS[i] for i in (S.ulp_error(theirs, ours) > 4).nonzero().flatten().tolist()]
        if name in S.NAN_RULE_UNARY and name != 'leaky':
            assert float(ours[4]) == 0.0                                              # the NaN becomes 0
        if name == 'relu':                        # (torch.sign and a comparison turn a NaN into 0 as well; leaky gives p0 * NaN)
            assert len(differs) == 1 and math.isnan(differs[0]), (name, differs)
        else:
            assert not differs, (name, differs, ours, theirs)
    a, b = x.repeat_interleave(len(S.SPECIALS)), x.repeat(len(S.SPECIALS))
    for name in S.BINARY:
        p0 = {'leaky_mask_mul': S.LEAKY_SLOPE, 'axpy': S.AXPY_P}.get(name, 0.0)
        ours, theirs = S.binary_ref(name, a, b, p0), S.torch_binary(name, a, b, p0).double()
        differs = S.ulp_error(theirs, ours) > 0.5
        if name == 'max':
            assert not bool((differs & ~(torch.isnan(a) ^ torch.isnan(b))).any())        # only where exactly one operand is a NaN
            theirs = torch.maximum(a.float(), b.float()).double()                         # (torch.fmax above drops it too)
            assert bool(torch.isnan(theirs[torch.isnan(a) ^ torch.isnan(b)]).all())
        else:
            assert not bool(differs.any()), (name, a[differs], b[differs])
    # where torch itself PROPAGATES the NaN that fmaxf drops and `b > 0` refuses:
    nan, one = torch.tensor([math.nan]), torch.tensor([1.0])
    assert math.isnan(float(torch.maximum(nan, one))) and float(S.binary_ref('max', nan, one)) == 1.0
    assert math.isnan(float(torch.relu(nan))) and float(S.unary_ref('relu', nan)) == 0.0
    assert float(S.row_max_ref(torch.tensor([[math.nan, 2.0, 1.0]]))) == 2.0


def test_frozen_norm_references_agree_with_batch_norm_and_autograd():
    for relu in (0, 1):
        for (n, c, hw) in S.BN_BWD:
            gen = S.generator('cpu-bn', n, c, hw)
            v = S.channel_vectors(c, gen)
            x = S.ints((n, c, hw), S.X, gen)
            g = S.ints((n, c, hw), S.X, gen)
            variance = 1.0 / v['inv_std'] ** 2                         # eps below half an ulp of it: inv_std IS 1 / sqrt(var)
            leaf = x.float().requires_grad_(True)
            gamma, beta = v['gamma'].float().requires_grad_(True), v['beta'].float().requires_grad_(True)
            y = TF.batch_norm(leaf, v['mean'].float(), variance.float(), gamma, beta, training=False, eps=1e-30)
            forward = S.chan_affine_ref(x, dict(mean=v['mean'], scale_a=v['inv_std'], scale_b=v['gamma'], shift=v['beta']), None,
                                        relu, (n, c, hw))
            close32(forward, (y.relu() if relu else y).detach(), f'forward {n, c, hw}', ulps=0.0)
            (y.relu() if relu else y).backward(g.float())
            gx, g_gamma, g_beta = S.bn_act_bwd_ref(g, x, v, relu, 0)
            close32(gx, leaf.grad, f'gx {n, c, hw}', ulps=0.0)
            close32(g_gamma, gamma.grad, f'g_gamma {n, c, hw}', ulps=0.0)       # exact operands: torch's fp32 sums are exact too
            close32(g_beta, beta.grad, f'g_beta {n, c, hw}', ulps=0.0)
            a = g * (x - v['mean'].view(1, c, 1))
            assert torch.equal(S.chan_reduce_ref(g, x, v['mean'], v['inv_std']), v['inv_std'] * a.sum(dim=(0, 2)))
            if not relu:
                assert torch.equal(g_gamma, S.chan_reduce_ref(g, x, v['mean'], v['inv_std']))


def test_tangent_reference_agrees_with_autograd():
    """d/d(w, gamma) of sum(q * (w * inv_std * gamma)) is (q * a, inv_std * sum w q)."""
    for (co, ci, taps) in S.TANGENT:
        gen = S.generator('cpu-tangent', co, ci, taps)
        w, q = S.ints((co, ci, taps), S.X, gen), S.ints((co, ci, taps), S.X, gen)
        inv_std, gamma = S.pick(S.SCALES, (ci,), gen), S.pick(S.SCALES, (ci,), gen)
        w_leaf, gamma_leaf = w.clone().requires_grad_(True), gamma.clone().requires_grad_(True)
        scaled = w_leaf * (inv_std * gamma_leaf).view(1, -1, 1)
        (scaled * q).sum().backward()
        w_scaled, w_grad, gamma_grad = S.tangent_ref(w, q, inv_std, gamma)
        assert torch.equal(w_scaled, scaled.detach()) and torch.equal(w_grad, w_leaf.grad) and torch.equal(gamma_grad, gamma_leaf.grad)


def test_loss_references_agree_with_the_reference_expressions():
    gen = S.generator('cpu-loss')
    u, fake, alpha = S.ints((3, 17), S.X, gen), S.ints((3, 17), S.X, gen), S.pick(S.ALPHAS, (3,), gen)
    assert torch.equal(S.gp_interpolate_ref(u, fake, alpha), alpha.view(-1, 1) * u + (1 - alpha.view(-1, 1)) * fake)
    for cm in S.L1_CM + [3]:
        maps = S.ints((3, cm, 50), S.X, gen).requires_grad_(True)
        target = S.ints((3, 50), S.X, gen)
        rows = (maps - target.unsqueeze(1)).abs().mean(dim=1).sum(dim=1)           # reference crowd/srgan.py's map term per example
        assert torch.allclose(S.crowd_l1_ref(maps.detach(), target), rows.detach(), rtol=1e-15)
        g = S.ints((3,), S.X, gen)
        rows.backward(g)
        assert bool((S.crowd_l1_bwd_ref(maps.detach(), target, g) == maps.grad).all())      # sign(0) = 0 in both
        assert bool(((maps.detach() - target.unsqueeze(1)) == 0).any())
    y, bins = torch.tensor([0.5, 1.5, -7.0, 99.0, 2.0]), torch.tensor([0.0, 1.0, 2.0, 3.0])
    index = (y.view(-1, 1) - bins.view(1, -1)).abs().numpy().argmin(axis=1)          # reference utility.py: argmin, the first minimum
    assert S.nearest_bin_ref(y, bins).argmax(dim=1).tolist() == index.tolist() == [0, 1, 0, 3, 2]
    x = torch.tensor([[1.0, 3.0, 3.0], [-math.inf, -math.inf, -math.inf], [0.0, math.inf, 1.0]])
    assert torch.equal(S.row_max_ref(x), x.double().max(dim=1).values)


def test_pooling_references_agree_with_torch():
    for (planes, h, w, k, s, p) in S.MAXPOOL:
        gen = S.generator('pool', planes, h, w, k, s, p)
        x = S.pooling_inputs(planes, h, w, gen)
        values, index = TF.max_pool2d(x.float().unsqueeze(0), k, s, p, return_indices=True)
        oh, ow = values.shape[-2:]
        ours, ours_index = S.maxpool_ref(x, k, s, p, oh, ow)
        assert torch.equal(ours_index, index[0]), (planes, h, w, k, s, p)
        assert bool(((ours == values[0].double()) | (torch.isnan(ours) & torch.isnan(values[0]))).all())
        assert bool(torch.isinf(ours).any()) and bool(torch.isnan(ours).any())
        src = S.ints((planes, h, w), S.X, gen)
        assert torch.equal(S.pool_gather_ref(src, index[0]).reshape(planes, oh, ow), src.reshape(planes, -1).gather(1, index[0].reshape(planes, -1)).reshape(planes, oh, ow))
        g = S.ints((planes, oh, ow), S.X, gen)
        unpooled = TF.max_unpool2d(torch.ones(1, planes, oh, ow, dtype=torch.float64), index, k, s, p, output_size=(h, w))
        scattered = S.pool_scatter_ref(g, index[0], h * w)
        assert float(scattered.sum()) == float(g.sum()) and bool((scattered[unpooled[0].reshape(planes, -1) == 0] == 0).all())
    for (planes, h, w, k) in S.AVGPOOL:
        gen = S.generator('avg', planes, h, w, k)
        x = S.ints((planes, h, w), S.X, gen).requires_grad_(True)
        y = TF.avg_pool2d(x.unsqueeze(0), k, k)[0]
        assert torch.allclose(S.avgpool_ref(x.detach(), k), y.detach(), rtol=1e-15, atol=0)
        g = S.ints(y.shape, S.X, gen)
        y.backward(g)
        assert torch.allclose(S.avgpool_bwd_ref(g, k, h, w), x.grad, rtol=1e-15, atol=0)
        assert torch.equal(S.avgpool_ref(x.detach(), k), S.avgpool_ref(x.detach(), k, k))            # the stride argument: s = k as before
        assert torch.equal(S.avgpool_bwd_ref(g, k, h, w), S.avgpool_bwd_ref(g, k, h, w, k))
        assert torch.equal(S.avgpool_ref(x.detach(), k), x.detach().unfold(1, k, k).unfold(2, k, k).sum(dim=(3, 4)) / (k * k))
    for (planes, h, w, k, s) in S.AVGPOOL_STRIDED:
        gen = S.generator('avg', planes, h, w, k, s)
        x = S.ints((planes, h, w), S.X, gen).requires_grad_(True)
        y = TF.avg_pool2d(x.unsqueeze(0), k, s)[0]
        assert y.shape[1:] == (S.pool_out(h, k, s), S.pool_out(w, k, s))
        assert torch.allclose(S.avgpool_ref(x.detach(), k, s), y.detach(), rtol=1e-15, atol=0)
        g = S.ints(y.shape, S.X, gen)
        y.backward(g)
        # (k = 3: torch adds the ninths, the reference divides the sum: float64 roundings of a sum that may cancel)
        assert torch.allclose(S.avgpool_bwd_ref(g, k, h, w, s), x.grad, rtol=1e-15, atol=0 if k == 2 else 1e-15)


def fused_cases():
    return [('max', case) for case in S.FUSED_MAX_FWD + S.FUSED_MAX_BWD + S.FUSED_MAX_SEQUENCE] + \
        [('avg', case) for case in S.FUSED_AVG + S.FUSED_AVG_SEQUENCE]


def test_fused_pool_references_agree_with_torch_autograd():
    """max_pool2d(relu(batch_norm(x))) and avg_pool2d(relu(batch_norm(x)), 2, 2) in float64 on the CPU, with the gradients to x,
    gamma and beta: on the dyadic operands every float64 operation is exact, so the references EQUAL torch's."""
    for form, case in fused_cases():
        problem = S.fused_pool_problem(form, case)
        v, (k, s, p) = problem['v'], problem['geometry']
        x = problem['x'].clone().requires_grad_(True)
        gamma, beta = v['gamma'].clone().requires_grad_(True), v['beta'].clone().requires_grad_(True)
        variance = 1.0 / v['inv_std'] ** 2                             # eps below half an ulp of it: inv_std IS 1 / sqrt(var)
        activated = TF.batch_norm(x, v['mean'], variance, gamma, beta, training=False, eps=1e-30).relu()
        if form == 'max':
            y, index = TF.max_pool2d(activated, k, s, p, return_indices=True)
            assert torch.equal(problem['index'], index), (form, case)
        else:
            y = TF.avg_pool2d(activated, 2, 2)
        assert torch.equal(problem['y'], y.detach()), (form, case)
        y.backward(problem['g'])
        assert torch.equal(problem['gx'], x.grad), (form, case)
        assert torch.equal(problem['g_gamma'] - problem['old_gamma'], gamma.grad), (form, case)
        assert torch.equal(problem['g_beta'] - problem['old_beta'], beta.grad), (form, case)
        if form == 'max' and (k, s, p) == (3, 2, 1):                     # maxpool_bwd_ref IS the scatter, per plane
            n, c, h, w = case[:4]
            unmasked = S.maxpool_bwd_ref(problem['g'].reshape(n * c, *y.shape[2:]), problem['index'].reshape(n * c, *y.shape[2:]), h, w)
            leaf = activated.detach().clone().requires_grad_(True)
            TF.max_pool2d(leaf, k, s, p).backward(problem['g'])
            assert torch.equal(unmasked.reshape(n, c, h, w), leaf.grad), (form, case)


def test_adam_reference_agrees_with_torch_adam():
    for n in S.ADAM_N:
        for decay in S.ADAM_DECAY:
            for index, step in enumerate(S.adam_expected(n, decay)):
                for theirs, want, scale, measured, bound, name in zip(step['torch'], step['want'], step['scale'], step['measured'],
                                                                      step['bound'], 'pmv'):
                    assert float(S.ulp_error(theirs, want, scale).max()) <= measured, (n, decay, index, name)
                    # with the error measured at the operands' magnitude, the update costs a few roundings (more where a cancelled
                    # m reaches p through m / denom), never the thousands of ulps of a cancelled result
                    assert 2.0 <= bound <= 64.0, (n, decay, index, name, measured)
                print(f'adam n={n} decay={decay} step {index + 1}: fp32 orders vs float64 (p, m, v) '
                      f'{[round(value, 2) for value in step["measured"]]} ulp -> bounds {[round(value, 2) for value in step["bound"]]}')


# ------------------------------------------------------------------------------------------------- preconditions
def test_exact_cases_meet_their_precondition():
    for (n, c, hw) in S.REDUCE_BLOCK + S.REDUCE_ROWS + [(n, c, 1) for n, c in S.REDUCE_COLS] + S.REDUCE_UNALIGNED:
        gen = S.generator('reduce', n, c, hw)
        a, b = S.ints((n, c, hw), S.X, gen), S.ints((n, c, hw), S.X, gen)
        mean, scale = S.pick(S.QUARTERS, (c,), gen), S.pick(S.SCALES, (c,), gen)
        S.assert_exact_limit(S.chan_reduce_magnitude(a, b, mean, scale) + c + S.PREFILL, 3, f'reduce {n, c, hw}')
        # the bound that holds whatever the draw: |a| <= 3, |b - mean| <= 5, scale <= 2
        S.assert_exact_limit(3 * 5 * 2 * n * hw + c + S.PREFILL, 3, f'reduce {n, c, hw} (worst case)')
    for (n, c, hw) in S.BN_BWD:
        S.assert_exact_limit(3 * 5 * 2 * n * hw + c, 3, f'bn_act_bwd {n, c, hw}')           # g_gamma: inv_std * sum g (x - mean)
        S.assert_exact_limit(3 * 4 + n * c * hw, 2, f'bn_act_bwd gx {n, c, hw}')            # gx = g * a onto distinct integers
    for hw in S.AFFINE_HW:
        S.assert_exact_limit(3 * 4 + 2 + 2 * 4 + S.AFFINE_N * S.AFFINE_C * 2 * hw, 4, f'chan_affine {hw}')   # fma(x, a, b) onto distinct integers
    for (co, ci, taps) in S.TANGENT:
        S.assert_exact_limit(2 * 9 * co * taps + ci, 1, f'tangent {co, ci, taps}')           # inv_std * sum w q onto distinct integers
        S.assert_exact_limit(3 * 4 + co * ci * taps, 2, f'tangent w_grad {co, ci, taps}')
    for hw in S.L1_HW:
        S.assert_exact_limit(6 * hw, 2, f'crowd_map_l1 {hw}')                               # sum of |m - t| / Cm, Cm <= 4
    for f in S.GP_F:
        S.assert_exact_limit(3, 2, f'gp_interpolate {f}')
    for (planes, h, w, k) in S.AVGPOOL:
        if k != 3:
            S.assert_exact_limit(3 * k * k, int(math.log2(k * k)), f'avgpool {k}')
    for (planes, h, w, k, s) in S.AVGPOOL_STRIDED:
        if k != 3:                     # forward: k^2 integers; backward: at most ceil(k / s)^2 cotangents per pixel; both times 1 / k^2
            S.assert_exact_limit(3 * k * k, int(math.log2(k * k)), f'avgpool {k} / {s}')
            S.assert_exact_limit(3 * (-(-k // s)) ** 2, int(math.log2(k * k)), f'avgpool {k} / {s} backward')


def test_fused_pool_cases_meet_their_precondition():
    """Per output the sum of absolute values (old contents included) below 2^(24 - f), f = the output's fractional bits: a
    multiple of 1/4, b and fma(x, a, b) of 1/16; S an integer (max form) or a multiple of 1/4 (average form: the 0.25 adds two
    bits everywhere); gx = S * a two more, g_gamma = inv_std * sum S * (x - mean) three more.  Every case has a channel with
    negative gamma, and the tables reach the mask's borderline bn(x) == 0 under a non-zero pooled gradient."""
    borderline = {'max': 0, 'avg': 0}
    for form, case in fused_cases():
        problem = S.fused_pool_problem(form, case)
        v, x = problem['v'], problem['x']
        assert bool((v['gamma'] < 0).any()), (form, case)
        assert bool((v['gamma'] != 0).all()) and bool((v['inv_std'] > 0).all())
        for name, bits in S.FUSED_POOL_FRACTION_BITS[form].items():
            S.assert_exact_limit(problem['magnitudes'][name], bits, f'fused {form} pool {case} {name}')
            unit = 2.0 ** -bits
            assert torch.equal(problem[name] / unit, (problem[name] / unit).round()), (form, case, name)     # the bits are enough
        assert torch.equal(S.batch_norm_eval_ref(x, v) * 16, (S.batch_norm_eval_ref(x, v) * 16).round())
        # the worst case whatever the draw: |x| <= 3, |a| <= 4, |b| <= 2 + 2 * 4, |S| <= 4 * 3 (max: four windows) or 3 / 4
        n, c, h, w = case[:4]
        per_pixel = 12 if form == 'max' else 0.75
        S.assert_exact_limit(per_pixel * 5 * 2 * n * h * w + c, S.FUSED_POOL_FRACTION_BITS[form]['g_gamma'], f'fused {form} pool {case} (worst case)')
        if form == 'avg' or problem['geometry'] == (3, 2, 1):
            pooled = problem['gx'] / (v['inv_std'] * v['gamma']).view(1, -1, 1, 1)
            zero_norm = S.batch_norm_eval_ref(x, v) == 0
            assert bool((pooled[zero_norm] == 0).all())                              # masked: `> 0`
            raw = (S.maxpool_bwd_ref(problem['g'].reshape(n * c, *problem['g'].shape[2:]), problem['index'].reshape(n * c, *problem['g'].shape[2:]), h, w)
                   .reshape(n, c, h, w) if form == 'max' else problem['g'].repeat_interleave(2, dim=2).repeat_interleave(2, dim=3))
            hits = int((zero_norm & (raw != 0)).sum())
            borderline[form] += hits
            if form == 'avg' and n * h * w >= 64:
                assert hits > 0, (form, case)
    assert borderline['max'] > 0 and borderline['avg'] > 0, borderline


# ------------------------------------------------------------------------------------------------- branches
def test_elementwise_lengths_reach_the_tail_and_a_second_grid_stride_trip():
    shapes = {n: S.ew_trips(n) for n in S.EW_LENGTHS}
    assert {tail for _, tail in shapes.values()} == {0, 1, 2, 3}
    assert shapes[3] == (0, 3) and shapes[4] == (1, 0) and shapes[1025] == (1, 1)
    assert max(trips for trips, _ in shapes.values()) == 2 and shapes[S.EW_LENGTHS[-1]] == (2, 1)
    assert S.EW_LENGTHS[-1] // 4 > S.STREAM_BLOCKS * S.THREADS                   # the capped grid cannot cover it in one trip
    assert S.stream_trips(S.ADAM_N[-1]) == 2 and S.stream_trips(S.ADAM_N[-2]) == 1
    assert set(S.OFFSETS) == {0, 1, 2, 3}


def test_affine_planes_straddle_the_flat_rows_switch_and_the_segment_edge():
    paths = {hw: S.affine_path(hw) for hw in S.AFFINE_HW}
    assert paths[255] == ('flat', 1) and paths[256] == ('rows', 1) and paths[1] == ('flat', 1)
    assert paths[4095] == ('rows', 1) and paths[4096] == ('rows', 1) and paths[4097] == ('rows', 2)
    assert [-(-f // S.AFF_SEG) for f in S.GP_F] == [1, 1, 1, 2, 3]
    assert [-(-hw // S.RED_SEG) for hw in S.L1_HW] == [1, 1, 1, 2, 3]


def test_reduce_shapes_reach_their_kernels():
    assert all(S.reduce_path(n, c, 1)[0] == 'cols' for n, c in S.REDUCE_COLS)
    assert {(-(-c // 32), c % 32 == 0, n > 8, n % 8 == 0) for n, c in S.REDUCE_COLS} == \
        {(1, False, False, False), (2, False, True, False), (1, True, False, True), (3, False, True, False)}
    assert all(S.reduce_path(*shape)[0] == 'block' for shape in S.REDUCE_BLOCK)
    assert any(hw > S.THREADS for _, _, hw in S.REDUCE_BLOCK) and any(hw < S.THREADS for _, _, hw in S.REDUCE_BLOCK)
    seen = set()
    for (n, c, hw) in S.REDUCE_ROWS + S.REDUCE_UNALIGNED:
        path, seg, segs = S.reduce_path(n, c, hw)
        if hw == 1:
            assert path == 'cols'             # (a row of one element IS the columns kernel; kept for the window offsets)
            continue
        assert path == 'rows' and seg == S.RED_SEG, (n, c, hw)
        for row in range(n * c):
            for part in range(segs):
                aligned, four, quads, tail = S.rows_run_shape(hw, seg, part, row * hw)
                seen.add((aligned, four > 0, segs > 1, tail > 0))
    # aligned and odd row starts, one and several runs per row, the four-in-flight loop entered and not, with and without a tail
    assert {(True, True, False, False), (True, False, True, True), (False, False, True, True), (True, False, False, False),
            (False, False, False, True)} <= seen, sorted(seen)
    assert any(aligned and four and several for aligned, four, several, _ in seen)


def test_frozen_norm_backward_shapes_reach_the_image_groups_and_both_paths():
    per = {shape: S.bn_bwd_images_per_block(*shape) for shape in S.BN_BWD}
    assert per[(5, 512, 4)] == 4 and per[(5, 512, 9)] == 4                     # groups of 4 images: {0..3}, {4} -- a short last group
    assert 5 % 4 != 0
    assert 4 % 4 == 0 and 9 % 4 != 0                                           # once on the float4 path, once on the scalar one
    assert per[(3, 5, 42)] == per[(2, 4, 1600)] == per[(1, 7, 1)] == 1
    assert 1600 % 4 == 0 and 1600 // 4 > S.THREADS and 42 % 4 != 0


def test_tangent_shapes_reach_both_spans_and_partial_workgroups():
    spans = {S.tangent_span(taps) for _, _, taps in S.TANGENT}
    assert spans == {63, 64}
    assert any((ci * taps) % S.tangent_span(taps) != 0 and ci * taps > S.tangent_span(taps) for _, ci, taps in S.TANGENT)
    assert any(co % S.TANGENT_ROWS != 0 and co > S.TANGENT_ROWS for co, _, _ in S.TANGENT)
    assert any(co % S.TANGENT_ROWS == 0 for co, _, _ in S.TANGENT) and any(co < 4 for co, _, _ in S.TANGENT)


def test_small_kernels_tables():
    assert {(-(-b // S.THREADS)) for b, _ in S.ROW_MAX} == {1, 2} and {f for _, f in S.ROW_MAX} == {1, 2, 10}
    assert any(w % 4 == 0 for _, _, w, _ in S.AVGPOOL) and any(w % 4 != 0 for _, _, w, _ in S.AVGPOOL)
    for k in (2, 3, 4):
        assert {w % 4 == 0 for _, _, w, kk in S.AVGPOOL if kk == k} == {True, False}
    assert all(case['src'][1] > 0 and case['dst'][1] > 0 and case['src'][0] != case['dst'][0] for case in S.COPY_CHANNELS)
    assert {case['accumulate'] for case in S.COPY_CHANNELS} == {0, 1}


def test_fused_pool_shapes_reach_every_workgroup_count_and_both_finishes():
    """(workgroups per plane, thread items in the last, ordered | atomic in the default mode) of every fused case."""
    grid = {case: S.fused_pool_grid('max', *case) for case in S.FUSED_MAX_BWD}
    assert grid[(1, 1, 1, 4)] == (1, 1, 'ordered')                                  # the smallest plane: one float4
    assert grid[(2, 3, 8, 4)] == (1, 8, 'ordered') and grid[(3, 5, 15, 20)] == (1, 75, 'ordered') and 15 % 2 == 1
    assert grid[(2, 3, 32, 128)] == (1, S.POOL_BWD_QUADS, 'ordered')                # exactly one full workgroup
    assert grid[(2, 3, 41, 100)] == (2, 1, 'ordered')                               # the second holds one quad
    assert grid[(3, 2, 80, 64)] == (2, 256, 'ordered')
    assert grid[(1, 4096, 2, 4)] == (1, 2, 'ordered') and grid[(1, 4097, 2, 4)] == (1, 2, 'atomic')
    assert grid[(1, 65535, 1, 4)] == (1, 1, 'atomic')
    assert S.ROW_FINISH_ROWS == 4096 and S.POOL_MAX_PLANES == 65535
    grid = {case: S.fused_pool_grid('avg', *case) for case in S.FUSED_AVG}
    assert grid[(1, 1, 2, 4)] == (1, 1, 'ordered') and grid[(2, 3, 6, 8)] == (1, 6, 'ordered') and grid[(3, 5, 10, 12)] == (1, 15, 'ordered')
    assert grid[(2, 3, 64, 128)] == (1, S.POOL_BWD_QUADS, 'ordered') and grid[(2, 3, 50, 164)] == (2, 1, 'ordered')
    assert grid[(3, 2, 80, 128)] == (2, 256, 'ordered')
    assert grid[(1, 4096, 2, 4)] == (1, 1, 'ordered') and grid[(1, 4097, 2, 4)] == (1, 1, 'atomic')
    for case in S.FUSED_MAX_BWD + S.FUSED_MAX_SEQUENCE:
        assert S.fused_max_bwd_supported(*case, 3, 2, 1), case
    for case in S.FUSED_AVG + S.FUSED_AVG_SEQUENCE:
        assert S.fused_avg_supported(*case), case
    # several parts per channel (images x workgroups per plane) is what ordered_row_finish needs to do anything at all
    assert max(S.fused_pool_parts('max', *case) for case in S.FUSED_MAX_BWD) == 6
    assert max(S.fused_pool_parts('avg', *case) for case in S.FUSED_AVG) == 6
    # back to back: the parts per channel go 2, 6, 1, 2 with another C, N and plane every time
    for form, sequence in (('max', S.FUSED_MAX_SEQUENCE), ('avg', S.FUSED_AVG_SEQUENCE)):
        assert [S.fused_pool_parts(form, *case) for case in sequence] == [2, 6, 1, 2]
        assert all(a[1] != b[1] and a[2:] != b[2:] for a, b in zip(sequence, sequence[1:]))
        assert len({case[0] for case in sequence}) > 1
        assert all(S.fused_pool_grid(form, *case)[2] == 'ordered' for case in sequence)
    for form, cases in S.FUSED_REPEAT.items():
        assert all(S.fused_pool_grid(form, *case)[0] > 1 and S.fused_pool_grid(form, *case)[2] == 'ordered' for case in cases)
    # the fused forward: every geometry of the plain max pool, C coprime to N and to the plane
    assert {case[4:] for case in S.FUSED_MAX_FWD} == {(3, 2, 1), (2, 2, 0), (3, 1, 1), (3, 3, 0)}
    assert all(c > 1 and c % 2 == 1 for _, c, *_ in S.FUSED_MAX_FWD)


def test_maxpool_backward_cases_reach_the_three_kernels():
    """srgan_maxpool2d_bwd: the two four-pixels-per-thread kernels, the scalar gather kernel, and the scalar kernel again
    wherever a W % 4 == 0 case has its gx 1, 2 or 3 floats off a 16-byte boundary."""
    labels = {case: S.maxpool_bwd_path(case[2], *case[3:]) for case in S.MAXPOOL}
    assert set(labels.values()) == {'quad321', 'quad220', 'scalar'}
    assert labels[(12, 16, 16, 3, 2, 1)] == labels[(12, 15, 20, 3, 2, 1)] == labels[(12, 8, 4, 3, 2, 1)] == 'quad321'
    assert labels[(12, 12, 8, 2, 2, 0)] == 'quad220'
    assert labels[(10, 13, 11, 3, 2, 1)] == labels[(10, 13, 11, 2, 2, 0)] == labels[(12, 12, 10, 2, 2, 0)] == 'scalar'       # W % 4 != 0
    assert labels[(12, 9, 7, 3, 1, 1)] == labels[(12, 10, 11, 3, 3, 0)] == labels[(12, 5, 6, 2, 1, 0)] == 'scalar'
    for case, label in labels.items():
        if case[2] % 4 == 0:
            assert label != 'scalar' and all(S.maxpool_bwd_path(case[2], *case[3:], offset) == 'scalar' for offset in (1, 2, 3))
    assert any(planes * h * (w // 4) > S.THREADS for planes, h, w, k, s, p in S.MAXPOOL if w % 4 == 0)      # more than one workgroup
    # the windows of a row that one float4 (w0 % 4 == 0) can meet: 3 (3 / 2 / 1) and 2 (2 / 2 / 0).  The kernels' SPAN -- 4 and 3 -- is
    # an upper bound with one to spare: a loop of SPAN - 1 computes the same values, one of SPAN - 2 loses a window (and fails the cases)
    for (k, s, p), span in (((3, 2, 1), 4), ((2, 2, 0), 3)):
        assert (3 + p) // s - ((p - k + 1 + s - 1) // s if p - k + 1 > 0 else 0) + 2 == span
        met = {sum(any(ow * s - p <= w < ow * s - p + k for w in range(w0, w0 + 4)) for ow in range(64)) for w0 in range(0, 64, 4)}
        assert max(met) == span - 1, (k, s, p, met)
    assert {(w % 4 == 0, k, s) for _, _, w, k, s in S.AVGPOOL_STRIDED} == {(True, 3, 1), (False, 3, 2), (False, 2, 1), (True, 3, 2)}
    assert all(s < k for _, _, _, k, s in S.AVGPOOL_STRIDED)                                               # overlapping windows


def test_transcendental_bounds_are_the_documented_ones():
    """max(2, 4 x torch's CPU fp32 error against float64 on the same inputs) + the formula's further roundings."""
    for name in S.TRANSCENDENTAL:
        for p0 in (S.POW_EXPONENTS if name == 'pow' else [0.0]):
            measured, bound = S.transcendental_bound(name, p0)
            print(f'{name} p0={p0}: torch CPU fp32 {measured:.3f} ulp -> bound {bound:.3f} ulp')
            assert math.isfinite(measured) and 2.0 <= bound <= 16.0, (name, p0, measured, bound)
    x = S.transcendental_inputs('exp')
    assert float(S.unary_ref('exp', x).float()[x == 89.0]) == math.inf


def test_constants_mirror_the_kernel_sources():
    """The constants streaming_cases.py re-derives the branches from, read back from the sources: a change there fails here
    (and then, with the mirror updated, in the branch tests above) instead of silently un-covering a path."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'sr-gan_amd', 'csrc')
    text = {name: open(os.path.join(csrc, name)).read() for name in ('elementwise.hip', 'reduce.hip', 'common.h', 'pool.hip', 'split_finish.h')}
    assert f'constexpr int POOL_BWD_QUADS = {S.POOL_BWD_QUADS};' in text['pool.hip']
    assert f'constexpr int ROW_FINISH_ROWS = {S.ROW_FINISH_ROWS};' in text['split_finish.h']
    assert 'if (split_atomics_forced() || rows > ROW_FINISH_ROWS || parts < 1) return nullptr;' in text['split_finish.h']
    assert text['pool.hip'].count(f'(int64_t)N * C <= {S.POOL_MAX_PLANES}') == 2            # both `_supported` predicates
    assert text['pool.hip'].count('(plane_quads + POOL_BWD_QUADS - 1) / POOL_BWD_QUADS') == 1
    assert text['pool.hip'].count('(items + POOL_BWD_QUADS - 1) / POOL_BWD_QUADS') == 2
    assert 'if (W % 4 == 0 && ((uintptr_t)gx & 15) == 0 && n < ((int64_t)1 << 31)) {\n    const uint32_t quads' in text['pool.hip']

    def product(expression):
        value = 1
        for factor in expression.split('*'):
            value *= int(factor)
        return value
    assert product(re.search(r'constexpr int AFF_SEG = ([0-9 *]+);', text['elementwise.hip']).group(1)) == S.AFF_SEG
    assert product(re.search(r'constexpr int RED_SEG = ([0-9 *]+);', text['reduce.hip']).group(1)) == S.RED_SEG
    assert f'if (HW >= {S.ROWS_MIN_HW}) {{' in text['elementwise.hip']
    assert f'if (C >= {S.BLOCK_MIN_C} && (int64_t)N * HW <= {S.BLOCK_MAX_NHW})' in text['reduce.hip']
    assert f'constexpr int min_wgs = {S.REDUCE_MIN_WGS};' in text['reduce.hip'] and f'seg_cap = {S.REDUCE_SEG_CAP};' in text['reduce.hip']
    assert f'if (blocks > {S.STREAM_BLOCKS}) blocks = {S.STREAM_BLOCKS};' in text['common.h']
    assert f'constexpr int TW_ROWS = {S.TANGENT_ROWS};' in text['reduce.hip'] and 'const int span = 64 - 64 % taps;' in text['reduce.hip']
    assert ('while (per < N && ((int64_t)C * ((N + per - 1) / per) > 2048 || (int64_t)per * HW < 4096) &&' in text['reduce.hip']
            and '(int64_t)C * ((N + 2 * per - 1) / (2 * per)) >= 1024)' in text['reduce.hip'])
    assert 'for (; i + 768 < n4; i += 1024)' in text['reduce.hip']
    assert 'fabsf(x) >= 9.f ? copysignf(1.f, x) : tanhf(x)' in text['elementwise.hip']


def test_a_tanh_saturated_from_nine_is_within_an_ulp():
    """+-1 from |x| = 9 on costs at most 0.51 ulp (at 9 itself; from 9.011 on 1.0 is the nearest fp32 value anyway)."""
    x = torch.linspace(9.0, 9.02, 2001, dtype=torch.float64).float().double()
    error = S.ulp_error(torch.ones_like(x), S.unary_ref('tanh', x))
    assert 0.50 < float(error[0]) == float(error.max()) < 0.52
    assert float(error[x >= 9.011].max()) <= 0.5
