"""Panels of weekly-seasonal series on the host: the "ragged_seasonal" route of `panel_route`, its
steps class, its launches, and the argument checks of `ci_session_create_ragged_seasonal`, which
run before any device call (no GPU)."""
import ctypes as C

import numpy as np
import pytest

from causalimpact import _native
from causalimpact import batch

_ROUTE = dict(float64=False, standardize_data=True, sampler="gibbs", num_seasonal_blocks=1, P=6)
_LENGTHS = [300, 2048, 2049, 40]


def test_weekly_panel_takes_the_ragged_seasonal_route():
  r = batch.panel_route(**_ROUTE, num_seasons=[7], lengths=_LENGTHS)
  assert r == dict(route="ragged_seasonal", groups=[(4, [0, 1, 3]), (8, [2])])
  # every block of 2..7 seasons, up to the longest series the kernel takes
  for ns in (2, 7):
    r = batch.panel_route(**_ROUTE, num_seasons=[ns], lengths=[65536, 12])
    assert r == dict(route="ragged_seasonal", groups=[(4, [1]), (128, [0])])


def test_route_fall_backs():
  by_length = dict(route="equal_length", groups=[(40, [3]), (300, [0]), (2048, [1]), (2049, [2])])
  # without the seasons: what the route was before
  assert batch.panel_route(**_ROUTE, lengths=_LENGTHS) == by_length
  assert batch.panel_route(**_ROUTE, lengths=_LENGTHS, num_seasons=None) == by_length
  kw = dict(_ROUTE)
  kw["num_seasonal_blocks"] = 2
  assert batch.panel_route(**kw, num_seasons=[4, 7], lengths=_LENGTHS) == by_length
  assert batch.panel_route(**_ROUTE, num_seasons=[12], lengths=_LENGTHS) == by_length
  kw = dict(_ROUTE)
  kw["P"] = 53
  assert batch.panel_route(**kw, num_seasons=[7], lengths=_LENGTHS) == by_length
  assert batch.panel_route(**_ROUTE, num_seasons=[7], lengths=[300, 65537])["route"] == "equal_length"
  per_series = dict(route="per_series", groups=[(b, [b]) for b in range(4)])
  for change in (dict(float64=True), dict(sampler="hmc"), dict(standardize_data=False)):
    kw = dict(_ROUTE)
    kw.update(change)
    assert batch.panel_route(**kw, num_seasons=[7], lengths=_LENGTHS) == per_series
  # a trend panel keeps its route whatever `num_seasons` says
  kw = dict(_ROUTE)
  kw["num_seasonal_blocks"] = 0
  assert batch.panel_route(**kw, num_seasons=[], lengths=[300, 40]) == \
      dict(route="ragged", groups=[(1, [1]), (2, [0])])


def test_seasonal_steps_class_mirrors_the_kernels_grid():
  assert [batch.seasonal_steps_class(t) for t in (3, 2048, 2049, 4096, 4097, 65536)] == \
      [4, 4, 8, 8, 12, 128]
  # ceil(T / 512) rounded up to a multiple of 4, never below 4; a stride rounded up to a multiple of
  # 4 stays in the class of its longest series
  for t in range(3, 9000):
    want = max(4, (-(-t // 512) + 3) // 4 * 4)
    assert batch.seasonal_steps_class(t) == want
    assert batch.seasonal_steps_class((t + 3) & ~3) == want


def test_launches_of_the_seasonal_route_carry_scattered_positions():
  lengths = [500, 40, 3000, 257, 2048, 3, 2049, 41, 4096, 5000]
  r = batch.panel_route(**_ROUTE, num_seasons=[7], lengths=lengths)
  assert r["route"] == "ragged_seasonal"
  assert r["groups"] == [(4, [0, 1, 3, 4, 5, 7]), (8, [2, 6, 8]), (12, [9])]
  for devices in ([0], [0, 1], [0, 1, 2]):
    for shared in (False, True):
      launches = batch.panel_launches(r, devices, shared)
      ids = sorted(b for _, _, part in launches for b in part)
      assert ids == list(range(len(lengths)))                    # every series once, by position
      assert len({(dev, key) for dev, key, _ in launches}) == len(launches)   # one per (class, device)
      for dev, key, part in launches:
        assert dev in devices
        assert {batch.seasonal_steps_class(lengths[b]) for b in part} == {key}
  # one launch holds ids that are no neighbours in the panel
  assert [p for _, _, p in batch.panel_launches(r, [0], False)] == [[0, 1, 3, 4, 5, 7], [2, 6, 8], [9]]


def _creator(entry):
  L = _native.load()
  spec = dict.fromkeys(_native._PARAM_FIELDS, 1.0)   # pylint: disable=protected-access
  B = 3
  prm = _native.make_params([spec] * B)

  def create(lengths, ids=None, change=True, **kw):
    base = dict(T=300, P=0, has_slope=0, num_warmup=1, num_results=2, num_series=B, num_seasons=(7,))
    base.update(kw)
    pb = _native.make_problem(**base)
    Tn, Pn = base["T"], base["P"]
    X = np.zeros((B, Tn, Pn), np.float32) if Pn else None
    ln = None if lengths is None else np.asarray(lengths, np.int32)
    idv = None if ids is None else np.asarray(ids, np.int32)
    sc = np.zeros((max(1, len(base["num_seasons"])), Tn), np.uint8)
    h = C.c_void_p()
    args = [C.byref(pb), None if ln is None else ln.ctypes.data, None if idv is None else idv.ctypes.data,
            np.zeros((B, Tn), np.float32).ctypes.data, np.zeros((B, Tn), np.uint8).ctypes.data,
            None if X is None else X.ctypes.data]
    if entry == "seasonal":
      rc = L.ci_session_create_ragged_seasonal(*args, sc.ctypes.data if change else None, prm, C.byref(h))
    else:
      rc = L.ci_session_create_ragged(*args, prm, C.byref(h))
    assert rc != 0 and not h.value
    return L.ci_last_error().decode()

  return create, prm


# (lengths, keywords of the problem / the call) -> what the message must say
_REFUSALS = [
    (None, {}, ["series_lengths is NULL"]),
    ([300, 280, 270], dict(num_seasons=(4, 7)), ["num_blocks must be 1, got 2"]),
    ([300, 280, 270], dict(num_seasons=()), ["num_blocks must be 1, got 0"]),
    ([300, 280, 270], dict(num_seasons=(12,)), ["2 to 7 seasons, got num_seasons[0]=12"]),
    ([300, 280, 270], dict(P=53), ["at most 52 design columns, got P=53"]),
    ([301, 280, 270], dict(T=301), ["must be a multiple of 4, got T=301"]),
    # (a problem of one block of 2..7 seasons beyond 65536 steps is already refused by the checks
    #  of every session, which come first)
    ([65540, 65000, 64000], dict(T=65540), ["T=65540 exceeds", "65536"]),
    ([300, 2, 280], {}, ["series_lengths[1] must be >= 3, got 2"]),
    ([300, 280, 301], {}, ["series_lengths[2] = 301 exceeds the stride T=300"]),
    ([296, 280, 270], {}, ["max(series_lengths) = 296, T = 300"]),
    ([2052, 2048, 2050], dict(T=2052), ["series_lengths[1] = 2048 runs chunks of 4 steps",
                                        "the longest series (2052) chunks of 8"]),
    ([300, 280, 270], dict(ids=[0, 7, -4]), ["series_ids[2] must be >= 0, got -4"]),
    ([300, 280, 270], dict(flags=_native.FLAG_SEQUENTIAL_SEASONAL), ["do not take CI_FLAG_SEQUENTIAL_SEASONAL"]),
    ([300, 280, 270], dict(flags=_native.FLAG_CLUSTER_SEASONAL), ["do not take CI_FLAG_CLUSTER_SEASONAL"]),
    ([300, 280, 270], dict(flags=_native.FLAG_MULTIWAVE_SEASONAL), ["do not take CI_FLAG_MULTIWAVE_SEASONAL"]),
    ([300, 280, 270], dict(flags=_native.FLAG_SEASONAL_WORKSPACE), ["do not take CI_FLAG_SEASONAL_WORKSPACE"]),
    # the checks of every session come first
    ([300, 280, 270], dict(num_results=0), ["num_results >= 1"]),
]


def test_ragged_seasonal_entry_point_validates_before_any_device_call():
  create, _ = _creator("seasonal")
  assert "season_change is NULL" in create([300, 280, 270], change=False)
  for lengths, kw, parts in _REFUSALS:
    msg = create(lengths, **kw)
    for part in parts:
      assert part in msg, (part, msg)
  # 297..300 steps all fit a stride of 300
  assert "max(series_lengths)" not in create([297, 2, 280])


def test_session_ragged_reports_the_same_refusals():
  """Through the binding: `season_change=` selects the new entry point, its messages come back as a
  NativeError.  (A NULL `season_change` cannot be passed this way: without the keyword the binding
  calls `ci_session_create_ragged`.)"""
  _, prm = _creator("seasonal")
  B = 3
  for lengths, kw, parts in _REFUSALS:
    if lengths is None:
      continue
    kw = dict(kw)
    ids = kw.pop("ids", None)
    base = dict(T=300, P=0, has_slope=0, num_warmup=1, num_results=2, num_series=B, num_seasons=(7,))
    base.update(kw)
    pb = _native.make_problem(**base)
    Tn, Pn = base["T"], base["P"]
    y, m = np.zeros((B, Tn), np.float32), np.zeros((B, Tn), np.uint8)
    X = np.zeros((B, Tn, Pn), np.float32) if Pn else None
    with pytest.raises(_native.NativeError) as err:
      _native.Session.ragged(pb, lengths, y, m, X, prm, series_ids=ids,
                             season_change=np.zeros((1, Tn), np.uint8))
    for part in parts:
      assert part in str(err.value), (part, str(err.value))
  pb = _native.make_problem(T=300, P=0, has_slope=0, num_warmup=1, num_results=2, num_series=B,
                            num_seasons=(7,))
  with pytest.raises(ValueError, match="one entry per series"):
    _native.Session.ragged(pb, [300, 280], np.zeros((B, 300)), np.zeros((B, 300)), None, prm,
                           season_change=np.zeros((1, 300), np.uint8))


def test_the_trend_entry_point_still_refuses_seasonal_problems():
  create, prm = _creator("trend")
  assert "num_blocks must be 0, got 1" in create([300, 280, 270])
  assert "series_lengths is NULL" in create(None, num_seasons=())
  pb = _native.make_problem(T=300, P=0, has_slope=0, num_warmup=1, num_results=2, num_series=3,
                            num_seasons=(7,))
  with pytest.raises(_native.NativeError, match="num_blocks must be 0, got 1"):
    _native.Session.ragged(pb, [300, 280, 270], np.zeros((3, 300)), np.zeros((3, 300)), None, prm)


def test_abi_is_5_and_exports_the_new_entry_point():
  assert _native.ABI_VERSION == 5 and _native.load().ci_abi_version() == 5
  assert "ci_session_create_ragged_seasonal" in _native.exported_symbols()
  assert "ci_session_create_ragged" in _native.exported_symbols()
