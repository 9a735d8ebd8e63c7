"""Random encoder controls, drawn the same way for the GPU parity test (tests/test_gpu_parity.py: kernels against the oracle)
and the CPU one (tests/test_oracle_vs_ref.py: the oracle against the reference)."""


def random_control(rng):
    """a random but accepted E_CONTROL: rate, mode, CBR/VBR, -HF, DC filter, short-block threshold, tuning knobs"""
    sr = int(rng.choice([44100, 48000, 32000, 22050, 24000, 16000]))
    lsf = sr < 32000
    kw = dict(samprate=sr, mode=int(rng.choice([0, 1, 1, 3])))
    if rng.random() < 0.5:
        kw["bitrate"] = int(rng.choice([24, 32, 40, 48, 56, 64, 80] if lsf else [48, 56, 64, 80, 96, 112, 128, 160]))
    else:
        kw["vbr_mnr"] = int(rng.integers(0, 151))
        if rng.random() < 0.3:
            kw["vbr_br_limit"] = int(rng.choice([40, 64, 96, 160]))
        if rng.random() < 0.3:
            kw["vbr_delta_mnr"] = int(rng.integers(-40, 51))
    if not lsf and rng.random() < 0.3:
        kw["hf_flag"] = int(rng.choice([1, 3]))
        kw["freq_limit"] = int(rng.choice([17000, 19000, 22000, 24000]))
    if rng.random() < 0.2:
        kw["filter_select"] = 1
    if rng.random() < 0.3:
        kw["short_block_threshold"] = int(rng.choice([0, 100, 400, 99999]))
    if rng.random() < 0.2:
        kw["freq_limit"] = int(rng.choice([6000, 9000, 14000]))
    if rng.random() < 0.2:
        kw["test1"] = int(rng.integers(0, 12))
    if rng.random() < 0.15:
        kw["quick"] = 1
    if rng.random() < 0.2:
        kw["nsb_limit"] = int(rng.choice([2, 4, 6, 10, 14, 18, 22, 26, 30]))      # subband limit set by the caller
    return kw
