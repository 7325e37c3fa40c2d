"""CPU tests (-m "not gpu") of the long-window contract: even window lengths above 65536, up to 2^22, are accepted by
rc_engine_create; odd lengths and lengths above 2^22 stay RC_EUNSUPPORTED; the host-side parameter
helpers agree with the oracle at the new lengths; the new kernels are hashed into the `spectrum` kernel id."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle import cbind as oc

rocoder_amd = pytest.importorskip("rocoder_amd")
from rocoder_amd import _lib  # noqa: E402
from rocoder_amd.stretcher import derive_params, make_config, offline_output_len  # noqa: E402

LONG_OK = [131072, 1 << 22, 65538, 100000, 4194302]
LONG_BAD = [(1 << 22) + 2, 1 << 23, 131071]


def _create(window_len):
    cfg, _k = make_config(window_len=window_len, factor=4.0, channels=2)
    h = C.c_void_p()
    rc = _lib.lib().rc_engine_create(C.byref(cfg), C.byref(h))
    return rc, h


@pytest.mark.parametrize("N", LONG_OK)
def test_long_windows_are_accepted(N):
    rc, h = _create(N)
    if rc == _lib.RC_OK:  # (a machine with a GPU)
        assert h.value
        _lib.lib().rc_engine_destroy(h)
    else:
        assert rc == _lib.RC_ENODEVICE, rc
        assert not h.value


@pytest.mark.parametrize("N", LONG_BAD)
def test_odd_and_too_long_windows_stay_unsupported(N):
    rc, h = _create(N)
    assert rc == _lib.RC_EUNSUPPORTED and not h.value
    msg = _lib.lib().rc_last_error().decode()
    assert "4194304" in msg and "odd" in msg, msg


@pytest.mark.parametrize("N", [131072, 262144, 1 << 20, 1 << 22, 65538, 100000, 4194302])
@pytest.mark.parametrize("f,p", [(1.5, 1), (8.0, 1), (4.0, 2), (8.0, 3), (2.0, -2), (8.0, -3), (0.4, 1)])
def test_derive_and_output_len_match_oracle_at_long_windows(N, f, p):  # src/stretcher.rs:40-56
    got = derive_params(window_len=N, factor=f, pitch_multiple=p, amplitude=1.0)
    s = oc.Stretcher(factor=f, amplitude=1.0, pitch_multiple=p, window=np.ones(N, np.float32))
    assert got.sample_step_len == s.step
    assert got.samples_needed_per_window == s.samples_needed_per_window
    assert got.corrected_amp_factor == np.float32(s.amp)
    assert got.half_window_len == N // 2
    assert got.hops_per_window == (2 * p if p > 0 else -(-s.samples_needed_per_window // (N - N // 2)))
    for L in (N // 3, N, N + 12345, 3 * N + 7):
        assert offline_output_len(L, window_len=N, factor=f, pitch_multiple=p) == oc.offline_output_len(L, N, f, p)


def test_long_window_kernels_are_hashed_into_the_spectrum_family():
    csrc = os.path.join(ROOT, "rocoder_amd", "csrc")
    ids = json.loads(subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_id.py"), "--json", csrc],
                                    check=True, capture_output=True, text=True).stdout)
    assert sorted(ids) == ["big4", "generic", "hop4", "hopw", "spectrum"]
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_id
    finally:
        sys.path.pop(0)
    assert "rc_long.hip" in kernel_id.FAMILIES["spectrum"] and "rc_long.h" in kernel_id.FAMILIES["spectrum"]
    for fam, files in kernel_id.FAMILIES.items():
        if fam != "spectrum":
            assert not any(f.startswith("rc_long") for f in files), fam
