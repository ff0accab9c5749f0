"""The pooled placebo forecasts of the block models without a device: the declaration of
ci_session_pool_placebo_blocks and its test twin, what the binding lists, and the choice
`batch.placebo_pool_route` makes between the one-lane entry, the block-model entry and numpy."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from causalimpact import _native
from causalimpact import batch
from causalimpact import causalimpact_lib as lib

POOL_PARAMS = ["ci_session* session", "const double* scale", "const double* shift", "int32_t num_groups",
               "const int32_t* offsets", "const int32_t* members", "const double* weights", "int32_t max_origins",
               "const int32_t* origins", "const int32_t* horizon", "const double* init", "double* out",
               "const double* seen", "double* predicted_mean", "double* spread_mean", "double* pit_mean"]


def test_the_header_declares_both_entries_and_the_binding_lists_them():
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "causalimpact_amd.h")).read(), flags=re.S)
  declared = {}
  for name in ("ci_session_pool_placebo", "ci_session_pool_placebo_blocks", "ci_test_session_pool_placebo_blocks"):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, name
    declared[name] = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert name in _native.exported_symbols()
    assert list(getattr(_native.load(), name).argtypes) == [C.c_void_p if "*" in p else C.c_int32 for p in declared[name]]
  # the arguments of the one-lane entry, word for word; the test twin takes chunk_entries behind them
  assert declared["ci_session_pool_placebo"] == POOL_PARAMS
  assert declared["ci_session_pool_placebo_blocks"] == POOL_PARAMS
  assert declared["ci_test_session_pool_placebo_blocks"] == POOL_PARAMS + ["int32_t chunk_entries"]
  assert re.search(r"#define\s+CI_ABI_VERSION\s+5\b", text) and _native.ABI_VERSION == 5
  assert callable(_native.Session.pool_placebo) and callable(_native.Session.pool_placebo_blocks)


class _Stub:
  """A session as `placebo_pool_route` sees it: its summaries and the entries it has."""

  def __init__(self, summaries, entries):
    self.summaries = summaries
    for name in entries:
      setattr(self, name, lambda *a, **k: None)


GIBBS = _native.Session.summaries
BOTH = ("pool_placebo", "pool_placebo_blocks")


@pytest.mark.parametrize("what,sess,has_slope,num_seasons,want", [
    ("no block", _Stub(GIBBS, BOTH), True, (), "one_lane"),
    ("one block of 7", _Stub(GIBBS, BOTH), False, (7,), "one_lane"),
    ("one block of 7, a library without the block entry", _Stub(GIBBS, BOTH[:1]), False, (7,), "one_lane"),
    ("two blocks", _Stub(GIBBS, BOTH), False, (4, 3), "blocks"),
    ("one block of 12", _Stub(GIBBS, BOTH), False, (12,), "blocks"),
    ("52 seasons and a slope: d = 53", _Stub(GIBBS, BOTH), True, (52,), "blocks"),
    ("63 seasons and a slope: d = 64", _Stub(GIBBS, BOTH), True, (63,), "blocks"),
    ("two blocks, a library without the block entry", _Stub(GIBBS, BOTH[:1]), False, (4, 3), "host"),
    ("64 seasons and a slope: d = 65", _Stub(GIBBS, BOTH), True, (64,), "host"),
    ("two blocks, no placebo among the summaries", _Stub(("effect", "windows", "paths"), BOTH), False, (4, 3), "host"),
    ("no block, no placebo among the summaries", _Stub(("effect", "windows", "paths"), BOTH), False, (), "host"),
    ("a session without summaries", object(), False, (4, 3), "host"),
], ids=lambda v: v if isinstance(v, str) and " " in v else None)
def test_the_router_chooses_the_entry_by_session_and_model(what, sess, has_slope, num_seasons, want):
  assert batch.placebo_pool_route(sess, has_slope, num_seasons) == want, what


def test_the_route_reaches_the_entry_it_names():
  """`session_pool` pools and finishes through the entry of the route, and through neither on the host."""
  calls = []

  class Sess(_Stub):
    class pb:                                         # pylint: disable=invalid-name
      T, num_series = 9, 2

    def fetch(self, names):
      calls.append(("fetch", tuple(names)))
      return {}

  def entry(name):
    def call(scale, shift, groups, origins, horizon, init=None, seen=None):
      calls.append((name, len(groups), None if seen is None else seen.shape))
      G, O = len(groups), np.asarray(origins).shape[1] if isinstance(origins, np.ndarray) else 3
      out = {"acc": np.zeros((G, O, 2, 4))}
      if seen is not None:
        out.update({k: np.zeros(seen.shape) for k in _native.PLACEBO_OUTPUTS})
      return out
    return call

  one = lib.SeriesInputs(np.zeros(9), np.zeros(9, bool), None, np.zeros((2, 9), np.uint8), (4, 3), False, {})
  chain = batch._PlaceboChain.__new__(batch._PlaceboChain)                     # pylint: disable=protected-access
  for has, want in ((BOTH, "pool_placebo_blocks"), (BOTH[:1], None)):
    del calls[:]
    sess = Sess(GIBBS, ())
    for name in has:
      setattr(sess, name, entry(name))
    pool, finish = chain.session_pool(sess, np.ones(2), np.zeros(2), [one, one], [np.zeros(9)] * 2)
    if want is None:
      assert calls == [("fetch", tuple(lib._PARAMETER_DRAWS))] and finish is _native.finish_placebo_host   # pylint: disable=protected-access
      continue
    assert pool([{0: 1.0}], [{0: [1, 2, 3]}], [2], None).shape == (1, 3, 2, 4)
    means = finish(np.zeros((3, 2, 2, 4)), np.zeros((3, 2)))
    assert sorted(means) == sorted(_native.PLACEBO_OUTPUTS) and means["pit_mean"].shape == (3, 2)
    # the finishing call: no entry, every group empty, the accumulators handed in with `seen`
    assert calls == [(want, 1, None), (want, 3, (3, 2))]
