"""Generates tests/golden/trend_kernel_bits/trend_kernel_bits.json, the fixture of tests/test_gpu_trend_kernel_bits.py.

Run on an MI355X with the library built (python __graft_entry__.py), from the repository root:
    python tests/golden/trend_kernel_bits/make_trend_kernel_bits.py [output.json]
Only names and digests are written.  The digests are those of the code the compiler named in the
header made from the sources of the commit it ran at: a toolchain change, or a deliberate change of
the kernels' arithmetic, regenerates the file; a refactor must not.
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
for p in (ROOT, os.path.join(ROOT, "tfp-causalimpact_amd"), os.path.join(ROOT, "tests")):
  if p not in sys.path:
    sys.path.insert(0, p)

import trend_bits_cases as tc  # noqa: E402  pylint: disable=wrong-import-position


def _compiler():
  out = subprocess.run(["hipcc", "--version"], capture_output=True, text=True, check=True).stdout
  return [ln.strip() for ln in out.splitlines() if "version" in ln.lower()]


def _first_streamed(kind, D, T):
  """Smallest P <= 16 whose session reports the streamed build (None: none does)."""
  for P in range(1, 17):
    if tc.is_streamed(tc.route_name(kind, D, T, P)):
      return P
  return None


def main():
  out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "trend_kernel_bits.json")
  for kind in ("four", "eight"):
    for D in (1, 2):
      for T in (100, 300, 1000, 1300, 4096):
        got = _first_streamed(kind, D, T)
        want = tc.STREAMED_FROM[kind].get((D, tc.steps_per_thread(T)))
        assert got == want, (kind, D, T, got, want)
  cases = {}
  for kind, D, T in tc.groups():
    for P in tc.columns(kind, D, T):
      name, digests = tc.run_case(kind, D, T, P)
      cases[tc.case_id(kind, D, T, P)] = {"kernel": name, "sha256": digests}
      print(tc.case_id(kind, D, T, P), name, flush=True)
  seen = {c["kernel"] for c in cases.values()}
  assert seen == tc.expected_names(), (sorted(seen - tc.expected_names()), sorted(tc.expected_names() - seen))
  doc = {
      "header": {
          "what": "SHA-256 of every non-empty array Session.fetch() returns, per case of tests/trend_bits_cases.py",
          "compiler": _compiler(),
          "note": "made by tests/golden/trend_kernel_bits/make_trend_kernel_bits.py on an MI355X; a toolchain change "
                  "(or a deliberate change of the kernels' arithmetic) regenerates this file",
          "fit": {"num_warmup": tc.WARMUP, "num_results": tc.RESULTS, "num_chains": tc.CHAINS,
                  "seed": list(tc.SEED)},
      },
      "cases": cases,
  }
  with open(out_path, "w") as f:
    json.dump(doc, f, indent=1, sort_keys=True)
    f.write("\n")
  print("wrote", out_path, len(cases), "cases,", len(seen), "builds")


if __name__ == "__main__":
  main()
