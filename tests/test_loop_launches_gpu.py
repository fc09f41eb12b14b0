"""GPU: the launch sequence of every loop form is the committed one (tests/golden/loop_launch_sequences.json, written
by tools/record_loop_launches.py BEFORE the loops' host code was reorganised around ``pipeline._choose_form``): the same
entry points of the C ABI in the same order with the same small arguments, for the priming and two eager iterations of
each case of tests/loop_launches.py -- every form of FusedRenderAndCompare with and without shape optimisation, a point
constraint and the inlier bookkeeping, and MultiObjectRenderAndCompare with one and two views."""
import pytest

import loop_launches as LL

pytestmark = pytest.mark.gpu

CASES = LL.cases()
_decoders = {}


def test_the_fixture_holds_exactly_the_cases_of_the_list():
    assert sorted(LL.load_fixture()) == sorted(CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_launch_sequence_is_the_recorded_one(case):
    want = LL.load_fixture()[case]
    got = LL.record_case(*CASES[case], _decoders)
    assert len(want) > 0
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"{case}: call {k} is {a}, recorded {b}"
    assert [c[0] for c in got] == [c[0] for c in want]
