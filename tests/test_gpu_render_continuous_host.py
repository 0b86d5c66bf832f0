"""The phase-continuous rendering through the host layer: sots_match with "renderMode" in type.HIP.  The WAV it writes must
be the NumPy model's rendering (tests/_render_continuous_model.py) of the parameter track it writes, after the writer's own
24-bit quantisation; without the key the file is the overlap-add one, byte for byte."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _render_continuous_model as CM  # noqa: E402
import _render_model as M  # noqa: E402
from test_gpu_render_host import CHUNKS, HOP, N, PMAX, read_wav24, run_match, stable  # noqa: E402

pytestmark = pytest.mark.gpu


def track_of(csv):
    cells = [l.split(",") for l in csv.read_text().splitlines()[1:]]
    return np.array([[float(x) for x in c[4:8]] for c in cells]).astype(np.float32)


@pytest.mark.parametrize("mode,glide", [("continuous", False), ("continuousGlide", True)])
def test_render_mode_writes_the_models_rendering_of_the_track(tmp_path, O, mode, glide):
    csv = tmp_path / "track.csv"
    out, wav = run_match(tmp_path, mode, {"chunksInFlight": 4, "hopSize": HOP, "renderMatch": True, "renderMode": mode, "matchPath": str(csv)})
    assert out.returncode == 0, out.stderr
    u = track_of(csv)
    assert len(u) == CHUNKS
    got = read_wav24(wav)
    assert len(got) == (CHUNKS - 1) * HOP + N
    want = M.quantise_24bit(CM.render(0, u, [0.0] * 4, PMAX, O.wavetable(), N, HOP, glide))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%d samples differ" % np.count_nonzero(got != want)


def test_without_the_key_the_file_is_the_overlap_add_one(tmp_path):
    keys = {"chunksInFlight": 4, "hopSize": HOP, "renderMatch": True}
    plain, wav_plain = run_match(tmp_path, "plain", keys)
    named, wav_named = run_match(tmp_path, "named", dict(keys, renderMode="overlapAdd"))
    cont, wav_cont = run_match(tmp_path, "cont", dict(keys, renderMode="continuous"))
    assert plain.returncode == 0 and named.returncode == 0 and cont.returncode == 0, plain.stderr + named.stderr + cont.stderr
    assert wav_plain.read_bytes() == wav_named.read_bytes()
    assert stable(plain.stdout) == stable(named.stdout) == stable(cont.stdout)
    assert wav_plain.read_bytes() != wav_cont.read_bytes() and len(wav_plain.read_bytes()) == len(wav_cont.read_bytes())


def test_the_key_takes_effect_only_with_render_match(tmp_path):
    # 2^14 samples of the last chunk's match, as ever
    off, wav_off = run_match(tmp_path, "off", {"chunksInFlight": 4, "hopSize": HOP, "renderMode": "continuous"})
    ref, wav_ref = run_match(tmp_path, "ref", {"chunksInFlight": 4, "hopSize": HOP})
    assert off.returncode == 0 and ref.returncode == 0
    assert wav_off.read_bytes() == wav_ref.read_bytes() and len(wav_off.read_bytes()) == 44 + 3 * (1 << 14)


@pytest.mark.parametrize("bad", ["glide", "Continuous", 1, True])
def test_bad_render_mode_is_refused_before_any_device_work(tmp_path, bad):
    # no device is visible to this run: anything that reached the device first would fail with ITS text
    out, wav = run_match(tmp_path, "bad", {"renderMatch": True, "renderMode": bad}, env={"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"})
    assert out.returncode != 0
    assert "type.HIP.renderMode" in out.stderr and "device" not in out.stderr.lower(), out.stderr
    assert not wav.exists()


def test_render_mode_with_device_kernel_arithmetic_is_refused_before_any_device_work(tmp_path):
    out, wav = run_match(tmp_path, "dk", {"renderMatch": True, "renderMode": "continuous", "deviceKernelArithmetic": True},
                         env={"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"})
    assert out.returncode != 0
    assert "type.HIP.renderMode" in out.stderr and "deviceKernelArithmetic" in out.stderr, out.stderr
    assert not wav.exists()
