"""The case table of the exact contraction tests (contraction_cases.py) on the CPU, no library needed: the declared kinds cover
every fp32 kernel, every case keeps its partial sums exact in fp32, and the 16-bit table names every 16-bit kernel."""
import contraction_cases as T


def test_declared_kinds_cover_every_fp32_kernel():
    declared = set()
    for entry in T.CONV_CASES + T.GEMM_CASES:
        declared |= entry.reach
        assert entry.reach <= T.FP32_KINDS, entry
        assert not entry.split or entry.reach, f'{entry.shape}: a split case must name the kernel whose split it is there for'
    for reach in list(T.FUSED_WGRAD_REACH.values()) + [T.GROUPED_WGRAD_REACH]:
        declared |= reach
    assert declared | set(T.UNREACHABLE) == set(T.FP32_KINDS), sorted(set(T.FP32_KINDS) - declared - set(T.UNREACHABLE))
    assert set(T.FP32_KINDS) == set(range(0, 7)) | set(range(8, 14))


def test_every_case_keeps_its_partial_sums_exact():
    for entry in T.CONV_CASES:
        assert T.worst_partial_sums(entry.shape) < T.EXACT_LIMIT, entry.shape
    for entry in T.GEMM_CASES:
        batch, fin, fout = entry.shape
        assert T.X * T.W * max(batch, fin, fout) + T.B + T.PREFILL < T.EXACT_LIMIT, entry.shape
    for (cin, cout, k, s, p, hin, batch) in T.CONVT_CASES:
        assert T.X * T.W * cin * k * k + T.B + T.PREFILL < T.EXACT_LIMIT


def test_the_16_bit_table_declares_every_16_bit_kernel():
    assert set(T.REACH16) == set(T.KINDS16) == set(range(14, 20))
    assert not set(T.KINDS16) & set(T.FP32_KINDS)


def test_cases_are_unique():
    shapes = [entry.shape for entry in T.CONV_CASES]
    assert len(shapes) == len(set(shapes))
