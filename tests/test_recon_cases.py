"""The decoder of tests/mp3_decode.py pinned on the CPU, before anything on the GPU relies on it (no GPU here).

Front half, exact: for every signal frame of every case of tests/recon_cases.py the decoded lines, signs and
side-information fields equal the oracle's own taps of the call that coded the frame, by ==, and every granule's Huffman
decode ends exactly on part2_3_length.  That frame c of the bytes carries the taps of call c is what "call c codes frame
c" means; the oracle's frame count trails the calls (the reservoir holds bytes back, also behind zero blocks) and never
passes them.
Back half: the synthesis window is held to the filter bank's own property, the decoder's output on the oracle's bytes to
the input it was coded from - the lag of the correlation peak is hx_recon_delay()'s documented 2209, and the SNR against
the input has a floor.
Coverage: what the cases reach is asserted from the parsed side information."""
import numpy as np
import pytest

import mp3_decode as M
import recon_cases as R
from oracle import oracle as O

DELAY = 2209            # include/hmp3_amd.h, hx_recon_delay (tests/test_recon_abi.py holds the export to it)
# The decoder's output against the input delayed by DELAY, case cbr128_tones (44.1 kHz CBR 128 joint stereo, 12 tones and
# noise), over the signal's frames: measured here on the oracle's bytes 29.57 dB (left) and 28.92 dB (right).  The floor is
# 6 dB below the lower one: a wrong window, sign or order lands near 0 dB (the first attempt at the synthesis window, with
# the side lobes' signs wrong, gave 6.7 dB on the bank alone and -0.1 dB here).
SNR_MEASURED = (29.57, 28.92)
SNR_FLOOR = min(SNR_MEASURED) - 6.0
GR = {n: i for i, n in enumerate(O.GR_FIELDS)}


@pytest.fixture(scope="module")
def huff():
    return O.huff_tables()


@pytest.fixture(scope="module")
def decoded(huff):
    cache = {}

    def get(name):
        if name not in cache:
            run = R.oracle_run(name)
            cache[name] = run + M.decode(run[2], huff)
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(R.CPU_CASES))
def test_front_half_equals_the_oracles_taps(name, decoded):
    kw, pcm, data, taps, calls, frames_out, y, frames = decoded(name)
    F = len(pcm) // 1152
    assert F <= frames_out <= calls and len(frames) == frames_out and y.shape[0] == 1152 * frames_out
    nch = 1 if kw.get("mode") == 3 else 2
    for f in range(F):
        info = frames[f]
        ix, sg, gr, ms, scfsi = taps[f]
        assert info["decodable"] and info["nch"] == nch
        for g in range(2):
            for ch in range(nch):
                q, where = info["gr"][g][ch], (name, f, g, ch)
                assert q["huff_end"] == q["part2_3_length"], where
                assert np.array_equal(q["ix"], ix[g, ch]), where
                assert np.array_equal(q["sign"][q["ix"] > 0], (sg[g, ch] != 0)[q["ix"] > 0]), where
                if nch == 1:        # (the oracle taps the frame record on the stereo path only: tests/stage_taps.py)
                    continue
                o = gr[g, ch]
                for key in ("part2_3_length", "big_values", "global_gain", "scalefac_compress", "window_switching_flag", "block_type",
                            "mixed_block_flag", "preflag", "scalefac_scale", "count1table_select"):
                    assert q[key] == o[GR[key]], where + (key, q[key], int(o[GR[key]]))
                assert q["nquads"] == max(int(o[GR["aux_nquads"]]), 0), where
                nt = 2 if q["window_switching_flag"] else 3
                assert q["table_select"][:nt] == [int(o[GR["table_select%d" % k]]) for k in range(nt)], where
                if q["window_switching_flag"]:      # (not transmitted otherwise: the oracle's record keeps an earlier granule's)
                    assert q["subblock_gain"] == [int(o[GR["subblock_gain%d" % k]]) for k in range(3)], where
                else:
                    assert (q["region0_count"], q["region1_count"]) == (int(o[GR["region0_count"]]), int(o[GR["region1_count"]])), where
        if nch == 2:
            assert info["ms"] == ms, (name, f)
            assert [sum(b << (3 - k) for k, b in enumerate(c)) for c in info["scfsi"]] == scfsi, (name, f)


@pytest.mark.parametrize("name", list(R.CPU_CASES))
def test_each_case_reaches_what_it_is_there_for(name, decoded):
    kw, pcm, data, taps, calls, frames_out, y, frames = decoded(name)
    got = R.features(frames[:len(pcm) // 1152])
    assert R.REACHES[name] <= got, sorted(R.REACHES[name] - got)


def test_the_cases_together_reach_every_path_of_the_decoder():
    assert set().union(*R.REACHES.values()) == R.EVERYTHING


def test_synthesis_window_reconstructs_through_the_standards_analysis_bank(huff):
    """Analysis by the standard's flow chart with C = D / 32 (shift 32 samples in, window, fold to 64, matrix with
    cos((2 k + 1)(i - 16) pi / 64)), then the decoder's synthesis: the input comes back 481 samples late.  The bank is a
    near-perfect-reconstruction one: its own error is below -90 dB, and the table, put back together from float32
    constants, measured 84.6 dB here; the bound asks for 80.  A wrong sign on one side lobe gives less than 10 dB."""
    dec = M.Decoder(huff)
    c = dec.D / 32.0
    x = np.random.default_rng(1).standard_normal(32 * 18 * 6)
    k, i = np.arange(32)[:, None], np.arange(64)[None, :]
    a = np.cos((2 * k + 1) * (i - 16) * np.pi / 64.0)
    fifo, sub = np.zeros(512), []
    for t in range(len(x) // 32):
        fifo[32:] = fifo[:-32].copy()
        fifo[:32] = x[32 * t:32 * t + 32][::-1]
        sub.append(a @ (c * fifo).reshape(8, 64).sum(0))
    sub = np.array(sub)
    y = np.concatenate([dec._synth(sub[18 * g:18 * g + 18], 0) for g in range(len(sub) // 18)])
    got, want = y[481:], x[:len(x) - 481]
    snr = 10.0 * np.log10((want * want).sum() / ((got - want) ** 2).sum())
    print("filter bank reconstruction: %.2f dB" % snr)
    assert snr > 80.0


def test_delay_and_snr_against_the_input(decoded):
    kw, pcm, data, taps, calls, frames_out, y, frames = decoded(R.SNR_CASE)
    n = len(pcm)
    x = pcm.astype(np.float64)
    for ch in range(2):
        full = np.zeros(len(y))
        full[:n] = x[:, ch]
        c = np.correlate(y[:, ch], full, "full")
        lag = int(np.argmax(np.abs(c))) - (len(y) - 1)
        assert lag == DELAY, (ch, lag)
        got, want = y[DELAY:n, ch], x[:n - DELAY, ch]
        snr = 10.0 * np.log10((want * want).sum() / ((got - want) ** 2).sum())
        print("channel %d: lag %d, SNR %.2f dB (measured %.2f, floor %.2f)" % (ch, lag, snr, SNR_MEASURED[ch], SNR_FLOOR))
        assert snr >= SNR_FLOOR, (ch, snr)


# Per granule of case vbr50_switching_ms, by block type, the best SNR of the decoder's output against the input delayed by
# DELAY (granules whose input is below 100 rms are left out): measured here on the oracle's bytes - start 21.9 dB (one
# granule), short 20.0 dB (one), stop 25.1 dB (two), long 25.1 dB (forty; the worst granules, around the bursts, are at
# 7 - 9 dB: the codec's noise at VBR 50, not the decoder's).  The floor is 6 dB below each: a wrong window or placement of
# the short transforms lands near 0 dB.
GRANULE_SNR_MEASURED = {0: 25.1, 1: 21.9, 2: 20.0, 3: 25.1}


def test_every_block_type_is_held_to_the_input_on_a_switching_case(decoded):
    kw, pcm, data, taps, calls, frames_out, y, frames = decoded("vbr50_switching_ms")
    x, n, best = pcm.astype(np.float64), len(pcm), {}
    for g in range(n // 576):
        a, b = 576 * g, 576 * g + 576
        if a < DELAY:
            continue
        want, got = x[a - DELAY:b - DELAY], y[a:b]
        if (want * want).mean() < 100.0 ** 2:
            continue
        snr = 10.0 * np.log10((want * want).sum() / ((got - want) ** 2).sum())
        bt = frames[g // 2]["gr"][g % 2][0]["block_type"]
        best[bt] = max(best.get(bt, -99.0), snr)
    print("best granule SNR by block type:", {k: round(v, 2) for k, v in sorted(best.items())})
    for bt, measured in GRANULE_SNR_MEASURED.items():
        assert best[bt] >= measured - 6.0, (bt, best[bt])


def test_silence_decodes_to_silence(decoded):
    kw, pcm, data, taps, calls, frames_out, y, frames = decoded("silence")
    assert not y.any()
