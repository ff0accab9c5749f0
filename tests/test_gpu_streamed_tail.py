"""The tail of a streamed fit (ci_session_run_streamed): the last chunk's rows and the arrays without
a time axis are queued while the sampler still runs -- through one gather kernel behind it for the
destinations the device can write (pinned memory), through copies behind a wait on the kernel's end
for the others.  Whatever the chunking, the kind of destination and the route, every byte equals what
run() + fetch() return and no byte of the caller's buffers is left unwritten: the buffers are filled
with NaN before each of two calls into the same `into=` pair.

T = 257 is odd, so the rows of the last chunk start at every alignment modulo 16 bytes (the
kernel's scalar head and tail and its 16-byte body all carry data); T = 300 keeps them aligned.
"""
import numpy as np
import pytest

from causalimpact import _native
from causalimpact import _synthetic as syn
from oracle import ci_oracle as orc

pytestmark = pytest.mark.gpu

W = 5
_CACHE = {}


def _session(T, p, has_slope, B, C, S, seed=(2, 9), seasons=None, data_seed=40):
  """A session and what run() + fetch() give for it (computed once, shared, read-only)."""
  key = (T, p, has_slope, B, C, S, seed, seasons, data_seed)
  if key not in _CACHE:
    ys, masks, Xs, specs = [], [], [], []
    for b in range(B):
      y, mask, X, _ = syn.make_sampler_inputs(T, p, data_seed + b)
      ys.append(y); masks.append(mask); Xs.append(X)
      specs.append(orc.default_spec(y, mask, X, seasons=seasons) if seasons
                   else orc.default_spec(y, mask, X, has_slope=bool(has_slope)))
    kw = dict(num_seasons=tuple(n for n, _ in seasons)) if seasons else {}
    pb = _native.make_problem(T=T, P=p + 1, has_slope=has_slope, num_warmup=W, num_results=S,
                              num_chains=C, num_series=B, seed=seed, **kw)
    sc = np.stack(specs[0]["season_change"]) if seasons else None
    sess = _native.Session(pb, np.stack(ys), np.stack(masks), np.stack(Xs), sc,
                           _native.make_params(specs))
    sess.run()
    want = sess.fetch()
    for v in want.values():
      v.flags.writeable = False
    _CACHE[key] = (sess, want)
  return _CACHE[key]


def _into(pb, want, kind):
  """An (Outputs, arrays) pair for run_streamed(into=...): every array pinned (ci_host_alloc),
  every array pageable (plain numpy), or alternating ("mixed": level and the trajectories pageable,
  slope and the weights pinned, the scalars some of each)."""
  out, arrs = _native.Outputs(), {}
  for i, (name, shp) in enumerate(_native.output_shapes(pb).items()):
    if want is not None and name not in want:
      continue
    pinned = kind == "pinned" or (kind == "mixed" and i % 2 == 0)
    a = _native.pinned_empty(shp) if (pinned and int(np.prod(shp)) > 0) else np.empty(shp, np.float32)
    arrs[name] = a
    setattr(out, name, a.ctypes.data if a.size else None)
  return out, arrs


def _check_streamed(sess, want, chunk, kind, keys=None):
  into = _into(sess.pb, keys, kind)
  for _ in range(2):
    for a in into[1].values():
      a.fill(np.nan)
    ms, got = sess.run_streamed(chunk_draws=chunk, into=into)
    assert ms > 0
    assert set(got) == set(want if keys is None else keys)
    for k in got:
      np.testing.assert_array_equal(got[k], want[k], err_msg=k)


# B = 3 series x C = 5 chains on the eight-wave kernel (P = 6), S = 61 draws
MAIN = dict(T=257, p=5, has_slope=1, B=3, C=5, S=61)


@pytest.mark.parametrize("chunk,kind", [
    (1, "pinned"),       # 61 chunks, the last like every other
    (12, "pinned"),      # 5 x 12 + a one-draw last chunk
    (60, "pinned"),      # S - 1: two chunks, the last one draw
    (61, "pinned"),      # S: the whole result is the last chunk
    (64, "pinned"),      # S + 3
    (12, "pageable"), (61, "pageable"), (1, "pageable"),
    (12, "mixed"), (60, "mixed"), (64, "mixed")])
def test_streamed_tail_equals_run_then_fetch(chunk, kind):
  sess, want = _session(**MAIN)
  assert "gibbs_kernel8" in sess.kernel_name()
  _check_streamed(sess, want, chunk, kind)


@pytest.mark.parametrize("kind", ["pinned", "pageable", "mixed"])
def test_streamed_tail_of_the_product_path_subset(kind):
  """fit_causalimpact asks for everything but the trajectories and the slope."""
  sess, want = _session(**MAIN)
  keys = tuple(k for k in want if k not in ("posterior_trajectories", "slope"))
  _check_streamed(sess, want, 32, kind, keys=keys)


@pytest.mark.parametrize("kind", ["pinned", "pageable"])
def test_streamed_tail_slope_of_a_model_without_one_reads_zero(kind):
  sess, want = _session(T=257, p=5, has_slope=0, B=1, C=3, S=30)
  assert not want["slope"].any()
  _check_streamed(sess, want, 8, kind)       # 8, 8, 8, 6


@pytest.mark.parametrize("chunk,kind", [(7, "pinned"), (23, "mixed"), (24, "pinned")])
def test_streamed_tail_on_the_four_wave_kernel(chunk, kind):
  """P = 20 columns: the LDS regression block of the four-wave kernel; T = 300 keeps every row
  16-byte aligned."""
  sess, want = _session(T=300, p=19, has_slope=1, B=1, C=2, S=24)
  assert "gibbs_kernel<" in sess.kernel_name()
  _check_streamed(sess, want, chunk, kind)


@pytest.mark.parametrize("chunk,kind", [(16, "pinned"), (13, "mixed"), (40, "pageable")])
def test_streamed_tail_of_a_weekly_seasonal_model(chunk, kind):
  """The seasonal kernels publish no progress: chunked copies after the kernel has ended, the
  same tail, the same bytes (seasonal_levels and seasonal_drift_scales included)."""
  sess, want = _session(T=203, p=3, has_slope=0, B=1, C=2, S=40, seasons=((7, 1),))
  assert want["seasonal_levels"].size and want["seasonal_drift_scales"].size
  _check_streamed(sess, want, chunk, kind)


def test_streamed_tail_over_recycled_streams():
  """Two sessions created, streamed and closed back to back on one device, then a third: each takes
  the streams and events the one before parked, which must carry nothing over -- no wait on an
  event of a closed session, no copy still in flight."""
  for seed in ((3, 1), (3, 2), (3, 3)):
    sess, want = _session(T=131, p=5, has_slope=1, B=1, C=4, S=33, seed=seed)
    del _CACHE[(131, 5, 1, 1, 4, 33, seed, None, 40)]
    _check_streamed(sess, want, 10, "pinned")      # 10, 10, 10, 3
    sess.close()
