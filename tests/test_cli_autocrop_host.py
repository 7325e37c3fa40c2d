"""CPU tests (-m "not gpu") of the CLI's --autocrop argument checks: each is refused before the input is opened."""
import os
import subprocess

import pytest

from conftest import ROOT

CLI = os.environ.get("ROCODER_CLI") or os.path.join(ROOT, "rocoder_amd", "bin", "rocoder")


def run(tmp_path, *args):
    out = str(tmp_path / "o.wav")
    r = subprocess.run([CLI, "-i", str(tmp_path / "missing.wav"), "-o", out, *args], capture_output=True, text=True, timeout=60)
    assert not os.path.exists(out)
    return r


def test_autocrop_needs_frames_on_gpu(tmp_path):
    r = run(tmp_path, "--autocrop")
    assert r.returncode != 0 and "--autocrop needs --frames-on-gpu" in r.stderr


@pytest.mark.parametrize("p", ["100", "101", "-1", "30.5", "x", ""])
def test_autocrop_percentile_is_0_to_99(tmp_path, p):
    r = run(tmp_path, "--frames-on-gpu", "--autocrop", "--autocrop-percentile", p)
    assert r.returncode != 0 and "--autocrop-percentile takes an integer of 0 ... 99" in r.stderr


@pytest.mark.parametrize("w", ["0", "0.0", "00:00:00"])
def test_autocrop_window_of_zero(tmp_path, w):
    r = run(tmp_path, "--frames-on-gpu", "--autocrop", "--autocrop-window", w)
    assert r.returncode != 0 and "--autocrop-window takes a duration above 0" in r.stderr


def test_valid_autocrop_arguments_reach_the_input(tmp_path):
    r = run(tmp_path, "--frames-on-gpu", "--autocrop", "--autocrop-window", "0.05", "--autocrop-percentile", "99")
    assert r.returncode != 0 and "cannot open" in r.stderr


def test_usage_names_the_flags():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert "--autocrop-window" in r.stdout + r.stderr and "--autocrop-percentile" in r.stdout + r.stderr
