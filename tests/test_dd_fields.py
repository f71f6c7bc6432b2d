"""The double-double derivative fields (csrc/fields_dd.h, csrc/dd_dev.h) against a 50-digit
mpmath restatement of the same formulas (tests/mp_fields.py: fp64 constants, the phase as the exact
product (om + oml) d), one field at a time:

  * on the DEVICE, through the diagnostic entry point gpk_fields_dd -- the call pgrad_kernel's
    double-double loop makes, one thread per distance.  This is where HIP's default
    -ffp-contract=fast once broke the error-free transforms to 1e-10 while the host stayed exact;
  * on the HOST, by a small program (tests/fields_dd_host.hip) built with hipcc, so that the
    reference and the bar are checked without a GPU.

Four kinds, deriv 1 and 2, 256 distances over the ranges the double-double exp / sincos were
validated on (radial argument <= 60, phase <= 1200 rad) plus d = 0.  Bar: 1e-26 x the field's
absolute-monomial scale -- 100 x the documented 1e-28 of exp and sincos, for the ten or so
double-double operations composed into a field; ten orders of magnitude below both fp64 and the
recorded fp-contract failure.  A field that is identically zero (no cosine: f_f, d_f; an odd
derivative at d = 0) must be exactly 0.

Observed maxima / scale: 2.3e-28 .. 2.5e-28 per kind, the same on the MI355X and on the host (the
device's are recorded in the parity log, tests/helpers.record_parity)."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import field_ulp_inputs as FI
from tests.conftest import ROOT
from tests.helpers import record_parity

CASES = [(k, dv) for k in FI.KINDS for dv in (1, 2)]
NAMES = ("f_w", "f_l", "f_f", "d_w", "d_l", "d_f")


@functools.lru_cache(maxsize=None)
def reference(kind, deriv):
    """(values, scales) [257][6] of mpf, computed once per case and shared by both tests."""
    from tests import mp_fields as MP
    d, a, freq = FI.dd_inputs(kind)
    rows = [MP.component(kind, deriv, x, a, freq) for x in d]
    return [r[0] for r in rows], [r[1] for r in rows]


def worst_errors(kind, deriv, hi, lo):
    """max |hi + lo - exact| / scale per field; exact zeros checked on the way."""
    from tests import mp_fields as MP
    vals, scales = reference(kind, deriv)
    worst = dict.fromkeys(NAMES, 0.0)
    for e in range(len(vals)):
        for x, name in enumerate(NAMES):
            got = MP.mp_of(hi[e, x]) + MP.mp_of(lo[e, x])
            if scales[e][x] == 0:
                assert got == 0, (name, e, hi[e, x], lo[e, x])
                continue
            worst[name] = max(worst[name], float(abs(got - vals[e][x]) / scales[e][x]))
    return worst


def _hipcc():
    cand = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return cand if shutil.which(cand) else None


@functools.lru_cache(maxsize=None)
def _host_program(tmp):
    exe = os.path.join(tmp, "fields_dd_host")
    subprocess.run([_hipcc(), "-O2", "-std=c++17", "--offload-arch=gfx950", "-x", "hip",
                    os.path.join(ROOT, "tests", "fields_dd_host.hip"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    pytest.importorskip("mpmath")
    if _hipcc() is None:
        pytest.skip("hipcc not found")
    return _host_program(str(tmp_path_factory.mktemp("dd")))


@pytest.mark.parametrize("kind,deriv", CASES)
def test_fields_dd_host(host_program, kind, deriv):
    from oracle.gp_oracle import KIND_IDS
    d, a, freq = FI.dd_inputs(kind)
    text = " ".join([str(KIND_IDS[kind]), str(deriv), float(a).hex(), float(freq).hex(), str(len(d))]
                    + [float(x).hex() for x in d])
    out = subprocess.run([host_program], input=text, capture_output=True, text=True, check=True).stdout
    v = np.array([[float.fromhex(t) for t in line.split()] for line in out.splitlines()])
    assert v.shape == (len(d), 12)
    worst = worst_errors(kind, deriv, v[:, :6], v[:, 6:])
    print(kind, deriv, worst)
    assert max(worst.values()) <= FI.DD_BAR, worst


@pytest.mark.gpu
@pytest.mark.parametrize("kind,deriv", CASES)
def test_fields_dd_device(kind, deriv):
    pytest.importorskip("mpmath")
    from gpk.core import fields_dd
    d, a, freq = FI.dd_inputs(kind)
    hi, lo = fields_dd(kind, deriv, d, a, freq)
    assert np.isfinite(hi).all() and np.isfinite(lo).all()
    worst = worst_errors(kind, deriv, hi, lo)
    print(kind, deriv, worst)
    record_parity("test_fields_dd_device", f"{kind}/deriv{deriv}", worst, FI.DD_BAR)
    assert max(worst.values()) <= FI.DD_BAR, worst
