"""The host-side precision dispatch of the blocked kernels (sr-gan_amd/csrc/precision_dispatch.h), compiled alone with g++
(the header needs no HIP) into a stand-alone program, tests/csrc/precision_dispatch.cpp, that prints what the header did."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LISTS = {'0,1,2': (0, 1, 2), '1,2': (1, 2), 'none': ()}
EINVAL = -1      # SRGAN_EINVAL (sr-gan_amd/csrc/common.h)


@pytest.fixture(scope='module')
def records(tmp_path_factory):
    binary = str(tmp_path_factory.mktemp('precision_dispatch') / 'precision_dispatch')
    subprocess.check_call(['g++', '-O1', '-std=c++17', '-Wall', '-Werror', '-I' + os.path.join(ROOT, 'sr-gan_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'csrc', 'precision_dispatch.cpp'), '-o', binary])
    done = subprocess.run([binary], capture_output=True, text=True, timeout=60)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    return [line.split(' ', 4) for line in done.stdout.splitlines()]


@pytest.mark.parametrize('name', ['0,1,2', '1,2'])
def test_a_listed_code_calls_the_functor_once_with_that_constant(records, name):
    rows = {int(r[2]): r for r in records if r[0] == 'dispatch' and r[1] == name}
    assert sorted(rows) == [-1, 0, 1, 2, 3]
    for dtype in LISTS[name]:
        returned, calls, constant = (int(v) for v in rows[dtype][3].split() + rows[dtype][4].split())
        assert (returned, calls, constant) == (1, 1, dtype), rows[dtype]


@pytest.mark.parametrize('name', ['0,1,2', '1,2', 'none'])
def test_an_unlisted_code_calls_nothing_and_returns_false(records, name):
    rows = {int(r[2]): r for r in records if r[0] == 'dispatch' and r[1] == name}
    unlisted = [dtype for dtype in (-1, 0, 1, 2, 3) if dtype not in LISTS[name]]
    assert {-1, 3} <= set(unlisted) and (name == '0,1,2' or 0 in unlisted)
    for dtype in unlisted:
        returned, calls, constant = (int(v) for v in rows[dtype][3].split() + rows[dtype][4].split())
        assert (returned, calls, constant) == (0, 0, -99), rows[dtype]


@pytest.mark.parametrize('name', ['0,1,2', '1,2', 'none'])
def test_the_check_reports_invalid_argument_with_the_callers_message(records, name):
    rows = {int(r[2]): r for r in records if r[0] == 'check' and r[1] == name}
    for dtype in (-1, 0, 1, 2, 3):
        status, message = int(rows[dtype][3]), rows[dtype][4]
        if dtype in LISTS[name]:
            assert (status, message) == (0, '-'), rows[dtype]
        else:
            assert status == EINVAL and message.startswith("the caller's message: requirement ("), rows[dtype]


def test_slot_channels_and_channel_groups(records):
    assert {int(r[1]): int(r[2]) for r in records if r[0] == 'slot_channels'} == {0: 4, 1: 8, 2: 8}
    groups = {(int(r[1]), int(r[2])): int(r[3]) for r in records if r[0] == 'channel_groups'}
    assert groups == {(C, dtype): -(-C // (4 if dtype == 0 else 8)) for C in (1, 4, 5, 8, 9) for dtype in (0, 1, 2)}
    assert [groups[(C, 0)] for C in (1, 4, 5, 8, 9)] == [1, 1, 2, 2, 3]
    assert [groups[(C, 1)] for C in (1, 4, 5, 8, 9)] == [1, 1, 1, 1, 2]
