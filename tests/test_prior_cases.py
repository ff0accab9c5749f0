"""The case table of tests/prior_cases.py, checked on the float64 oracle alone (no GPU): the record keeps
confusable fields apart, every bound clips some draws and spares others, and reading any field for its
sibling moves an output the GPU test compares by at least three of that output's tolerances -- the
condition under which tests/test_gpu_prior_record.py must fail on a kernel that reads the wrong field."""
import numpy as np
import pytest

from causalimpact import _native
from oracle import ci_oracle as orc

import prior_cases as pc

NAMES = [c.name for c in pc.CASES]


def test_the_default_record_is_the_one_that_cannot_tell_fields_apart():
  """What this table exists for: in `default_spec` the siblings coincide."""
  y, mask, X, spec = pc.make_series(120, 4, 1, pc.WEEK)
  assert len({spec[k] for k in ("level_ub", "slope_ub", "drift_ub", "init_level_scale", "init_slope_scale",
                                "init_seasonal_scale")}) == 1
  assert spec["level_conc"] == spec["slope_conc"] and spec["level_scale"] == spec["slope_scale"]
  assert len(pc.separation_failures(spec)) > 0


# every case on its own, and every other record and length that a one-launch batch runs
MEMBERS = [(name, 0, None) for name in NAMES] + [
    m for m in pc.batch_members() if m[1] > 0 or m[2] != pc.CASE_BY_NAME[m[0]].T]


@pytest.mark.parametrize("name,variant,T", MEMBERS)
def test_confusable_fields_are_a_quarter_apart(name, variant, T):
  y, mask, X, spec = pc.case_inputs(name, variant, T)
  assert pc.separation_failures(spec) == [], (name, variant)
  assert spec["weights_prior_scale"] != 1.0
  assert abs(spec["init_level_loc"] - y[~mask][0]) >= spec["outcome_sd"]
  if spec["P"] > 1:
    assert spec["nonzero_prob"] < 1.0 and spec["nonzero_prob"] != min(1.0, 3.0 / spec["P"])


def test_series_of_one_launch_have_three_different_records():
  for bc in pc.BATCH_CASES:
    name = bc.case
    specs = [pc.case_inputs(name, b, T)[3] for b, T in enumerate(bc.lengths)]
    for f in ("level_ub", "obs_ub", "level_conc", "obs_scale", "init_level_scale",
              "obs_scale0", "level_scale0", "weights_prior_scale"):
      vals = [s[f] for s in specs]
      assert all(pc.apart(vals[i], vals[j]) or f.endswith("_ub") and vals[i] != vals[j]
                 for i in range(3) for j in range(i)), (name, f, vals)


@pytest.mark.parametrize("name", NAMES)
def test_bounds_are_the_medians_of_the_unbounded_oracle(name):
  c = pc.CASE_BY_NAME[name]
  y, mask, X, spec = pc.case_inputs(name)
  free = dict(spec, level_ub=pc.NO_BOUND, slope_ub=pc.NO_BOUND, obs_ub=pc.NO_BOUND, drift_ub=pc.NO_BOUND)
  w = orc.fit_gibbs(y, mask, X, free, num_results=c.S, num_warmup=0, seed=pc.SEED)
  assert spec["level_ub"] == np.median(w["level_scale"])
  assert spec["obs_ub"] == np.median(w["obs_scale"] if spec["P"] == 0 else w["obs_scale"] ** 2)
  if c.has_slope:
    assert spec["slope_ub"] == np.median(w["slope_scale"])
  if c.seasons:
    assert spec["drift_ub"] == np.median(w["drift_scales"])
  assert c.T <= 5000 and c.S <= 12 and (c.S == 6) == (c.T >= 4096)


@pytest.mark.parametrize("name,variant,T", MEMBERS)
def test_every_bound_clips_two_draws_and_spares_two(name, variant, T):
  counts = pc.clip_counts(name, variant, T)
  c = pc.CASE_BY_NAME[name]
  assert set(counts) >= {"obs", "level"} | ({"slope"} if c.has_slope else set()) | ({"drift"} if c.seasons else set())
  for scale, (clipped, free) in counts.items():
    if scale.startswith("drift["):
      assert clipped >= 1, (name, scale, clipped, free)        # per block; pooled: 2 and 2 like the others
    else:
      assert clipped >= 2 and free >= 2, (name, scale, clipped, free)


def test_every_field_is_carried_by_a_case_of_every_family_that_reads_it():
  best = pc.carriers()
  families = {c.family for c in pc.CASES}
  assert families == set(pc.FAMILIES)
  always = {"level_conc", "level_scale", "level_ub", "obs_conc", "obs_scale", "obs_ub", "init_level_loc",
            "init_level_scale", "obs_scale0", "level_scale0", "nonzero_prob", "weights_prior_scale"}
  slope = {"slope_conc", "slope_scale", "slope_ub", "init_slope_scale", "slope_scale0"}
  seasonal = {"drift_conc", "drift_scale", "drift_ub", "init_seasonal_scale", "drift_scale0"}
  for family in families:
    cases = [c for c in pc.CASES if c.family == family]
    fields = set(always)
    if any(c.has_slope for c in cases):
      fields |= slope
    if any(c.seasons for c in cases):
      fields |= seasonal
    # every family's kernels hold a slope and -- from family 2 on -- a seasonal block
    assert fields >= always | (seasonal if family >= 2 else set()) | (slope if family != 6 else set()), family
    for f in sorted(fields):
      ratio, name, output = best[(family, f)]
      assert ratio >= pc.MARGIN, (family, f, ratio, name, output)


def test_each_entry_of_drift_scale0_is_carried_by_a_case_with_several_blocks():
  for name in ("seq-workspace", "tp-ref", "tp-d10"):
    s = pc.sensitivity(name)
    for k in range(len(pc.CASE_BY_NAME[name].seasons)):
      assert s[f"drift_scale0[{k}]"][0] >= pc.MARGIN, (name, k, s[f"drift_scale0[{k}]"])


def test_the_inert_block_of_a_long_trend_series_reads_nothing_of_the_seasonal_record():
  """(5000, 3, 0) runs on ci_wide.h with an inert block; its record's drift_* and init_seasonal_scale
  differ from everything else, and the reference it is compared with does not depend on them."""
  spec = pc.case_inputs("wide-long")[3]
  assert pc.inert_fields_change_nothing("wide-long")
  assert spec["drift_conc"] != 1.0 and spec["drift_scale"] != 1.0 and spec["init_seasonal_scale"] > 0.0
  assert pc.apart(spec["drift_ub"], spec["level_ub"]) and pc.apart(spec["drift_conc"], spec["level_conc"])


def test_deviations_are_zero_on_the_reference_itself_and_flag_an_inclusion_flip():
  w = pc.oracle_reference("trend-8w")
  dev = pc.case_deviations("trend-8w", w)
  assert max(dev.values()) == 0.0
  flipped = dict(w, weights=np.where(np.arange(w["weights"].shape[1]) == 0, 0.0, w["weights"]))
  assert pc.case_deviations("trend-8w", flipped)["inclusion"] == np.inf
  off = dict(w, level_scale=w["level_scale"] * (1 + 1e-2))       # 1 %: two tolerances early, half of one late
  assert pc.case_deviations("trend-8w", off)["level_scale"] == pytest.approx(2.0)


def test_series_zero_of_a_batch_draws_from_the_plain_seed():
  assert tuple(_native.series_stream_key(pc.SEED, 0)) == pc.SEED
  assert len({pc.stream(None, b) for b in range(3)}) == 3
