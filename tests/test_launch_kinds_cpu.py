"""The launch kinds of the live profile are named once, in csrc/launchers.h's ``enum LaunchKind``; the tables that print them by
number (contraction_cases.KINDS / KINDS16, and through them helpers.profiled and the exact tests) must agree with it."""
import os
import re

from contraction_cases import KINDS, KINDS16

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'sr-gan_amd', 'csrc')
# The kinds no contraction table lists: the batch-norm kernels (0 FLOP; bench.py's workloads never launch them).
BATCH_NORM_KINDS = {20: 'bn_stats', 21: 'bn_fwd', 22: 'bn_bwd_reduce', 23: 'bn_bwd_apply', 24: 'h_frozen_norm_bwd'}


def launch_kinds():
    """{number: name} parsed from the enum: ``KIND_GG_MFMA = 1`` -> ``{1: 'gg_mfma'}``."""
    text = open(os.path.join(CSRC, 'launchers.h')).read()
    body = re.search(r'enum LaunchKind \{(.*?)\n\};', text, flags=re.DOTALL).group(1)
    body = re.sub(r'//[^\n]*', '', body)
    entries = re.findall(r'\bKIND_(\w+)\s*=\s*(\d+)\s*,', body)
    assert len(entries) == len(re.findall(r'\bKIND_\w+', body)), 'an entry without an explicit number'
    kinds = {int(number): name.lower() for name, number in entries}
    assert len(kinds) == len(entries), 'a number is used twice'
    return kinds


def test_the_enum_names_every_kind_of_the_tables_and_only_the_batch_norm_kinds_besides():
    kinds = launch_kinds()
    tables = {**KINDS, **KINDS16}
    assert {number: kinds.get(number) for number in tables} == tables
    assert {number: name for number, name in kinds.items() if number not in tables} == BATCH_NORM_KINDS
    assert 7 not in kinds                                   # unused, and the enum says so
    assert re.search(r'//\s*7 is unused', open(os.path.join(CSRC, 'launchers.h')).read())


def test_no_bracket_call_passes_a_number_as_its_kind():
    """Every profile_bracket_end / _end_bytes call names its kind (argument 6): a KIND_* entry or a LaunchKind variable."""
    calls = 0
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith('.hip'):
            continue
        text = open(os.path.join(CSRC, name)).read()
        for match in re.finditer(r'\bprofile_bracket_end(?:_bytes)?\(', text):
            if text[text.rfind('\n', 0, match.start()) + 1:match.start()] == 'int ':       # the definitions in profile.hip
                continue
            depth, start, arguments = 1, match.end(), []
            at = start
            while depth:
                char = text[at]
                depth += char in '([{'
                depth -= char in ')]}'
                if (char == ',' and depth == 1) or depth == 0:
                    arguments.append(text[start:at].strip())
                    start = at + 1
                at += 1
            calls += 1
            assert re.fullmatch(r'KIND_\w+|kind|c\.kind', arguments[5]), f'{name}: kind argument {arguments[5]!r}'
    assert calls >= 20                                      # (22 call sites in twelve translation units when this was written)
