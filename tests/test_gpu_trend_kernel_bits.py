"""The bits of the trend Gibbs kernels, pinned: every non-instrumented build of gibbs_kernel (stock
and ragged, all regression modes) and gibbs_kernel8 (design in LDS and from L2) runs a short fit,
and the SHA-256 of every array it returns must be the one recorded in
tests/golden/trend_kernel_bits/trend_kernel_bits.json.  The other tests compare the kernels with each other
(bit-identical) and with the float64 oracle (5e-3); neither notices both kernels moving together by
an ulp.  This one does: a change that is meant to keep the arithmetic -- moving a step into a
shared function, reordering a schedule -- passes it unchanged; a change of arithmetic, or of the
toolchain, regenerates the fixture (tests/golden/trend_kernel_bits/make_trend_kernel_bits.py) and says so.

The cases and their shapes: tests/trend_bits_cases.py.  The fixture has a directory of its own
because tests/test_summary_text.py reads every *.json directly under tests/golden as one of its
own cases."""
import json
import os

import pytest

import trend_bits_cases as tc

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trend_kernel_bits", "trend_kernel_bits.json")) as _f:
  _GOLDEN = json.load(_f)["cases"]


@pytest.mark.parametrize("kind,D,T", tc.groups(), ids=lambda v: str(v))
def test_every_build_returns_the_recorded_bits(kind, D, T):
  for P in tc.columns(kind, D, T):
    cid = tc.case_id(kind, D, T, P)
    want = _GOLDEN[cid]
    name, digests = tc.run_case(kind, D, T, P)
    assert name == want["kernel"], cid          # the case still reaches the build it was recorded on
    assert sorted(digests) == sorted(want["sha256"]), cid
    for k, d in digests.items():
      assert d == want["sha256"][k], f"{cid} ({name}): {k}"


def test_the_cases_reach_every_build():
  """The fixture lists exactly the cases of tests/trend_bits_cases.py, and the builds recorded for
  them -- each asserted from kernel_name() by its case above -- are the builds the library holds."""
  assert set(_GOLDEN) == {tc.case_id(k, D, T, P) for k, D, T in tc.groups() for P in tc.columns(k, D, T)}
  assert {c["kernel"] for c in _GOLDEN.values()} == tc.expected_names()


@pytest.mark.parametrize("kind,D,L,first", [(k, D, L, P) for k, v in sorted(tc.STREAMED_FROM.items())
                                            for (D, L), P in sorted(v.items())])
def test_streamed_builds_start_at_the_recorded_columns(kind, D, L, first):
  """The streamed cases sit AT the LDS budget's boundary: one column fewer keeps the design in LDS."""
  T = {8: 1300, 16: 4096}[L]
  assert tc.is_streamed(tc.route_name(kind, D, T, first))
  if first > 1:
    assert not tc.is_streamed(tc.route_name(kind, D, T, first - 1))
