"""`hmp3amd -batch` on file images with the tag frames built on the GPU and the finished files fetched together
(hx_multi_file_tags, hx_multi_file_fetch_many): every output is byte for byte the single-file run's, whose tag frame the
host's Tagger builds."""
import pytest

from gpu_support import batch_vs_single_vs_reference, write_wav
from hmp3_amd import synth

pytestmark = [pytest.mark.gpu, pytest.mark.one_k6_build]


def test_cli_two_slots_six_short_files_ending_in_pairs(tmp_path):
    """six short files through two slots, tagged (-X2: counts, TOC, LAME fields and both CRCs): the two files a call holds
    are both shorter than a call, so both end in it and come down as one image of two segments; 44.1 kHz, 48 kHz and 32 kHz
    float sources"""
    files = []
    for i, (sr, fmt, frames) in enumerate([(44100, False, 30), (44100, False, 30), (48000, False, 12), (48000, False, 12), (32000, True, 50), (44100, False, 7)]):
        nsamp = frames * 1152 - 211 * i - 7
        pcm = synth.stream_pcm(9800 + i, frames, sr=sr, rho=0.5, bursts=True)[:nsamp]
        wav = str(tmp_path / ("in%d.wav" % i))
        write_wav(wav, pcm, sr, fmt)
        files.append(("file %d" % i, wav, str(tmp_path / ("slots%d.mp3" % i))))
    stderr, outputs = batch_vs_single_vs_reference(files, ["-X2"], ["-slots2"], floor=1000, reference=False)
    assert "6 files through 2 slots" in stderr and "no file images" not in stderr
    for got in outputs:
        assert b"Xing" in got[:64] and b"LAME" in got[:256]
