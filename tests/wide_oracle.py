"""The float64 oracle widened to states of up to 256 components, for checking the multi-wavefront
seasonal kernel (csrc/ci_seasonal_mw.h) beyond the 64 components oracle/ci_oracle.h fixes.

oracle/ stays as it is: its sources are copied into a temporary directory, the one
`#define CI_MAX_D 64` becomes 256, and the copy is compiled with the Makefile's checker flags.  It is
then driven through oracle/ci_oracle.py's own structures (`_make_problem`) by standing in for
`ci_oracle.lib()` while `ci_oracle.fit_gibbs` runs."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile
from unittest import mock

from oracle import ci_oracle as orc

WIDE_MAX_D = 256
# oracle/Makefile's CFLAGS (the checker build: no -march, no contraction)
CHECKER_FLAGS = ["-O2", "-fPIC", "-std=c11", "-Wall", "-Wextra", "-fno-fast-math"]

_ORACLE_DIR = os.path.dirname(os.path.abspath(orc.__file__))
_lib = None
_tmp = None


def build_wide(max_d: int = WIDE_MAX_D) -> str:
  """Compiles the widened copy into a fresh temporary directory; returns the library's path."""
  global _tmp
  _tmp = tempfile.mkdtemp(prefix="ci_wide_oracle_")
  for name in ("ci_oracle.c", "ci_oracle.h"):
    shutil.copy(os.path.join(_ORACLE_DIR, name), os.path.join(_tmp, name))
  hdr = os.path.join(_tmp, "ci_oracle.h")
  with open(hdr) as f:
    text = f.read()
  text, n = re.subn(r"^#define CI_MAX_D 64\b", f"#define CI_MAX_D {int(max_d)}", text, flags=re.M)
  assert n == 1, f"expected exactly one '#define CI_MAX_D 64' in ci_oracle.h, found {n}"
  with open(hdr, "w") as f:
    f.write(text)
  out = os.path.join(_tmp, "libci_oracle_wide.so")
  cc = os.environ.get("CC", "gcc")
  subprocess.check_call([cc] + CHECKER_FLAGS + ["-shared", "-o", out, os.path.join(_tmp, "ci_oracle.c"), "-lm"])
  return out


def wide_lib() -> C.CDLL:
  """The widened oracle (built once per process), with the prototypes ci_oracle.lib() sets."""
  global _lib
  if _lib is None:
    L = C.CDLL(build_wide())
    L.ci_oracle_fit_gibbs.restype = C.c_int
    L.ci_oracle_fit_gibbs.argtypes = [C.POINTER(orc._Problem), C.POINTER(orc._Outputs)]  # pylint: disable=protected-access
    _lib = L
  return _lib


def fit_gibbs(y, mask, X, spec, **kw):
  """ci_oracle.fit_gibbs on the widened build: same arguments, same result dict."""
  L = wide_lib()
  with mock.patch.object(orc, "lib", lambda: L):
    return orc.fit_gibbs(y, mask, X, spec, **kw)
