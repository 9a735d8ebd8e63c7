"""`hmp3amd -batch` on file images with the tag frames built on the GPU and the finished files fetched together
(hx_multi_file_tags, hx_multi_file_fetch_many): every output is byte for byte the single-file run's, whose tag frame the
host's Tagger builds."""
import os
import subprocess
import sys

import pytest

from hmp3_amd import synth

pytestmark = [pytest.mark.gpu, pytest.mark.one_k6_build]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cli_two_slots_six_short_files_ending_in_pairs(tmp_path):
    """six short files through two slots, tagged (-X2: counts, TOC, LAME fields and both CRCs): the two files a call holds
    are both shorter than a call, so both end in it and come down as one image of two segments; 44.1 kHz, 48 kHz and 32 kHz
    float sources"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_cli as M
    exe = os.path.join(ROOT, "hmp3_amd", "hmp3amd")
    assert os.path.exists(exe), "hmp3_amd/build.sh builds the CLI"
    flags = ["-X2"]
    files, args = [], []
    for i, (sr, fmt, frames) in enumerate([(44100, False, 30), (44100, False, 30), (48000, False, 12), (48000, False, 12), (32000, True, 50), (44100, False, 7)]):
        nsamp = frames * 1152 - 211 * i - 7
        pcm = synth.stream_pcm(9800 + i, frames, sr=sr, rho=0.5, bursts=True)[:nsamp]
        wav = str(tmp_path / ("in%d.wav" % i))
        M.write_wav(wav, pcm, sr, fmt)
        files.append(wav)
        args += [wav, str(tmp_path / ("slots%d.mp3" % i))]
    r = subprocess.run([exe, "-batch", "-slots2"] + args + flags, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-400:]
    assert "6 files through 2 slots" in r.stderr.decode() and "no file images" not in r.stderr.decode()
    for i, wav in enumerate(files):
        got = open(str(tmp_path / ("slots%d.mp3" % i)), "rb").read()
        one = str(tmp_path / ("single%d.mp3" % i))
        r = subprocess.run([exe, wav, one] + flags, capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr.decode()[-400:]
        want = open(one, "rb").read()
        assert len(got) > 1000 and b"Xing" in got[:64] and b"LAME" in got[:256]
        assert got == want, "file %d differs from its single-file run (first at byte %d)" % (i, next((k for k in range(min(len(got), len(want))) if got[k] != want[k]), -1))
