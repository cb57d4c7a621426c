"""The opt-in bf16 codec precision (qwen_tts_set_codec_precision: the vocoder's
convs on k_convh) on the tiny golden model.  The stream comparisons use the
exact-mode stream tests' own bound (test_gpu_codec_mstream.py: 1e-5 max-abs
against the stateless decode of the same codes); the kernel-level bound is
test_gpu_convh.py's.
"""
import numpy as np
import pytest

import qtts
from conftest import golden

pytestmark = pytest.mark.gpu

CODES = np.random.default_rng(2611).integers(0, 2048, size=(3, 24, 16)).astype(np.int32)


@pytest.fixture
def m(tts_tiny):
    """the shared model, handed back in exact mode"""
    try:
        yield tts_tiny
    finally:
        tts_tiny.set_codec_precision("exact")


def test_precision_round_trips_and_rejects_a_bad_value(m):
    assert m.codec_precision() == qtts.CODEC_EXACT
    for v in ("bf16", "exact", qtts.CODEC_BF16, qtts.CODEC_EXACT):
        m.set_codec_precision(v)
        assert m.codec_precision() == {"bf16": 1, "exact": 0}.get(v, v)
    for bad in (2, -1, "fp16"):
        with pytest.raises(ValueError):
            m.set_codec_precision(bad)
    assert m.codec_precision() == qtts.CODEC_EXACT
    assert qtts.lib().qtts_dev_set_codec_precision(m.c.hip, 7) == -1


def test_exact_after_a_bf16_call_is_bit_exact(m):
    before = m.codec_decode(CODES[0])
    m.set_codec_precision("bf16")
    rounded = m.codec_decode(CODES[0])
    m.set_codec_precision("exact")
    np.testing.assert_array_equal(m.codec_decode(CODES[0]), before)
    assert np.all(np.isfinite(rounded)) and not np.array_equal(rounded, before)


def test_bf16_streams_equal_the_stateless_bf16_decode(m):
    """the single stream and a 3-stream ragged multi-stream push; a mode set
    after begin waits for the next begin (the stream latched bf16).  Which
    convs round their operands does not depend on the columns of a call
    (conv_ok with prec set), so a 1-frame push and the 24-frame decode agree;
    measured on an MI355X: 0.0 for all four."""
    m.set_codec_precision("bf16")
    full = [m.codec_decode(CODES[s]) for s in range(3)]
    single = np.concatenate(m.codec_stream([CODES[0, :1], CODES[0, 1:8], CODES[0, 8:]]))
    assert m.codec_mstream_begin(3, 64) == 0
    m.set_codec_precision("exact")                 # latched at begin: these pushes stay bf16
    cuts = [(0, 5, 11, 24), (0, 2, 17, 24), (0, 7, 8, 24)]
    out = [[], [], []]
    for k in range(3):
        o = m.codec_mstream_push_ragged([0, 1, 2], [CODES[s, cuts[s][k]:cuts[s][k + 1]] for s in range(3)])
        assert o is not None
        for s in range(3):
            out[s].append(o[s])
    d = [float(np.abs(single - full[0]).max())]
    d += [float(np.abs(np.concatenate(out[s]) - full[s]).max()) for s in range(3)]
    print("measured  bf16 largest |stream - stateless|: single %.3e, ragged streams %.3e %.3e %.3e" % tuple(d))
    assert max(d) < 1e-5, d


def test_bf16_waveform_against_the_oracle(m):
    """measured on an MI355X: mse 2.974e-05 against the oracle's golden
    waveform.  That is under the project's 1e-4 bar but not 4x
    under it, so the bar is not asserted here: the figure is recorded
    (profiles/codec_bf16_bench.txt) and the correctness bar of the mode is the
    kernel-level bound of test_gpu_convh.py."""
    g = golden("e2e_tiny.npz")
    m.set_codec_precision("bf16")
    a = m.codec_decode(np.ascontiguousarray(g["greedy_codes"]))
    mse = float(np.mean((a.astype(np.float64) - g["greedy_audio"]) ** 2))
    print(f"measured  bf16 codec vs the oracle's golden waveform: mse {mse:.3e}")
    assert a.shape == g["greedy_audio"].shape and np.all(np.isfinite(a))
