"""The tail of a streamed fit, from a rocprofv3 trace: what the GPU executes after the sampler ends.

  rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d DIR -- \
      python bench.py --steps 3 --warmup 1
  python tools/streamed_tail_timeline.py DIR [N]       (N: the last N fits only, the timed steps)

One table per fit: every copy and every other kernel that ends after the Gibbs kernel of that fit
and starts before the next fit's, with start and end relative to the Gibbs kernel's end (us).
"""
import csv
import glob
import os
import sys


def rows(root, suffix):
  out = []
  for f in sorted(glob.glob(os.path.join(root, "**", "*" + suffix), recursive=True)):
    with open(f, newline="") as fh:
      out.extend(csv.DictReader(fh))
  return out


def main(root, last=1 << 30):
  kernels = rows(root, "kernel_trace.csv")
  copies = rows(root, "memory_copy_trace.csv")
  ev = []
  for r in kernels:
    ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "kernel", r["Kernel_Name"].split("(")[0]))
  for r in copies:
    what = r.get("Direction") or r.get("Kind") or "copy"
    ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "copy", what))
  ev.sort()
  fits = [e for e in ev if e[2] == "kernel" and "gibbs_kernel" in e[3]]
  if not fits:
    raise SystemExit("no Gibbs kernel in the trace under " + root)
  print(f"{len(kernels)} kernel records, {len(copies)} copy records, {len(fits)} fits")
  for i, (k0, k1, _, name) in enumerate(fits):
    if i < len(fits) - last:
      continue
    nxt = fits[i + 1][0] if i + 1 < len(fits) else 1 << 62
    # (the next fit's set-up kernel belongs to the next fit)
    tail = [e for e in ev if e[1] > k1 and e[0] < nxt and e[0] > k0 and "setup_regression" not in e[3]]
    during = [e for e in ev if e[2] == "copy" and k0 <= e[0] and e[1] <= k1]
    print(f"\nfit {i}: {name}  {(k1 - k0) / 1e3:.1f} us; {len(during)} copies ended inside it"
          + (f", the last {(k1 - max(e[1] for e in during)) / 1e3:.1f} us before its end" if during else ""))
    print(f"  {'what':44s} {'start':>9s} {'end':>9s} {'took':>8s}   (us after the kernel's end)")
    for a, b, kind, what in tail:
      print(f"  {(kind + ' ' + what)[:44]:44s} {(a - k1) / 1e3:9.1f} {(b - k1) / 1e3:9.1f} {(b - a) / 1e3:8.1f}")
    if tail:
      print(f"  {'end of the last one':44s} {'':9s} {(max(e[1] for e in tail) - k1) / 1e3:9.1f}")


if __name__ == "__main__":
  main(sys.argv[1] if len(sys.argv) > 1 else ".", int(sys.argv[2]) if len(sys.argv) > 2 else 1 << 30)
