"""qwen_tts_generate_batch_stream: generate_batch's codes, bit for bit, with
every utterance's audio delivered in chunks by the multi-stream exact codec.

Bounds are the project's: 1e-5 max-abs between a streamed and a full decode of
the same codes (test_gpu_model.py::test_codec_stream_equals_full_decode).
"""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import manifest, model_dir
from oracle_py import DEFAULT
from synth_model import prompt_ids

import qtts

pytestmark = pytest.mark.gpu

SPK, LANG = "aiden", "english"
THREE = [prompt_ids("short"), prompt_ids("p128", 1300), prompt_ids("p128", 1301)]


class Chunks:
    """collects on_chunk(i, pcm): per utterance the chunk arrays, and the global order of arrival"""

    def __init__(self, nb):
        self.per = [[] for _ in range(nb)]
        self.order = []

    def __call__(self, i, pcm):
        self.per[i].append(pcm)
        self.order.append(i)

    def sizes(self, i):
        return [len(c) for c in self.per[i]]


# ---------------------------------------------------------------- 7. fixed length
def test_fixed_length_three_utterances(tts_tiny):
    m = tts_tiny
    m.set_params(max_tokens=4096, fixed=16, seed=42, **DEFAULT)
    rc, ref = m.generate_batch(THREE, [SPK] * 3, [LANG] * 3)
    assert rc == 0
    ref_codes = m.last_codes_batch(3, 16)
    got = Chunks(3)
    rc, audio = m.generate_batch_stream(THREE, [SPK] * 3, [LANG] * 3, chunk_frames=4, on_chunk=got)
    assert rc == 0
    for b in range(3):
        assert got.sizes(b) == [1920, 4 * 1920, 4 * 1920, 4 * 1920, 3 * 1920], (b, got.sizes(b))
        np.testing.assert_array_equal(np.concatenate(got.per[b]), audio[b])
        np.testing.assert_array_equal(m.last_codes_slot(b, 16), ref_codes[b])
        assert audio[b].shape == ref[b].shape
        d = float(np.abs(audio[b] - ref[b]).max())
        print(f"measured  slot {b}: largest |streamed - generate_batch| {d:.3e}")
        assert d < 1e-5, (b, d)
    assert 0 < m.c.perf_first_packet_ms < m.c.perf_total_ms
    assert m.c.perf_codec_ms > 0


def test_one_utterance_equals_generate_stream(tts_tiny):
    m = tts_tiny
    m.set_params(max_tokens=4096, fixed=16, seed=42, **DEFAULT)
    one = Chunks(1)
    single = m.generate_stream(THREE[0], SPK, LANG, chunk_frames=4, on_chunk=lambda a: one(0, a))
    c1 = m.last_codes()
    got = Chunks(1)
    rc, audio = m.generate_batch_stream([THREE[0]], [SPK], [LANG], chunk_frames=4, on_chunk=got)
    assert rc == 0
    np.testing.assert_array_equal(m.last_codes_slot(0, 16), c1)
    assert got.sizes(0) == one.sizes(0)
    assert audio[0].shape == single.shape
    assert np.abs(audio[0] - single).max() < 1e-5, np.abs(audio[0] - single).max()


# ---------------------------------------------------------------- 8. EOS mode
# default sampling of the tiny EOS model on the "short" prompt, by the CPU oracle
# (frames, stop): seed 2 -> 19 eos, 9 -> 23 eos, 7 -> 16 eos, 1 -> 32 max_tokens
EOS_SEEDS = [2, 9, 7, 1]
CHUNK = 4


def test_eos_mode_ragged_stops():
    md = model_dir("tiny", eos_gain=manifest()["eos_gain"])
    m = qtts.QwenTTS(md)
    try:
        ids = [prompt_ids("short")] * 4
        m.set_params(max_tokens=32, fixed=0, seed=42, **DEFAULT)
        m.set_utterance_sampling([dict(seed=s) for s in EOS_SEEDS])
        rc, ref = m.generate_batch(ids, [SPK] * 4, [LANG] * 4)
        assert rc == 0
        ref_codes = m.last_codes_batch(4, 32)
        frames = [len(c) for c in ref_codes]
        # the precondition, from generate_batch's own result: two different stop
        # frames, a stop that leaves a short tail after the first frame, a run to max_tokens
        assert len({f for f in frames if f < 32}) >= 2, frames
        assert any(f < 32 and (f - 1) % CHUNK != 0 for f in frames), frames
        assert 32 in frames, frames
        got = Chunks(4)
        m.set_utterance_sampling([dict(seed=s) for s in EOS_SEEDS])
        rc, audio = m.generate_batch_stream(ids, [SPK] * 4, [LANG] * 4, chunk_frames=CHUNK, on_chunk=got)
        assert rc == 0
        last_seen = {b: max(i for i, x in enumerate(got.order) if x == b) for b in range(4)}
        for b in range(4):
            np.testing.assert_array_equal(m.last_codes_slot(b, 32), ref_codes[b])
            assert sum(got.sizes(b)) == frames[b] * 1920, (b, got.sizes(b), frames[b])
            assert all(s > 0 and s % 1920 == 0 for s in got.sizes(b))
            np.testing.assert_array_equal(np.concatenate(got.per[b]), audio[b])
            assert audio[b].shape == ref[b].shape
            d = float(np.abs(audio[b] - ref[b]).max())
            assert d < 1e-5, (b, d)
        # no callback for an utterance after its last frame: once its samples
        # are complete it is never called again, and a shorter utterance's last
        # chunk does not come after a longer one's
        for b in range(4):
            done_at = np.cumsum(got.sizes(b)).tolist().index(frames[b] * 1920)
            assert done_at == len(got.per[b]) - 1
        by_len = sorted(range(4), key=lambda b: frames[b])
        for a, b in zip(by_len, by_len[1:]):
            if frames[a] < frames[b]:
                assert last_seen[a] < last_seen[b], (frames, got.order)
        # a short tail was pushed on its own: some stopped utterance ends on a
        # chunk shorter than the one the running utterances got at that poll
        assert any(got.sizes(b)[-1] // 1920 < CHUNK for b in range(4) if frames[b] < 32), \
            [got.sizes(b) for b in range(4)]
    finally:
        m.close()


# ---------------------------------------------------------------- 9. sequence on one fresh context
def test_single_stream_before_and_after_a_batch_stream(tiny_dir):
    m = qtts.QwenTTS(tiny_dir)
    try:
        m.set_params(max_tokens=4096, fixed=12, seed=42, **DEFAULT)
        a = m.generate_stream(THREE[0], SPK, LANG, chunk_frames=4)
        five = [THREE[b % 3] for b in range(5)]
        rc, audio = m.generate_batch_stream(five, [SPK] * 5, [LANG] * 5, chunk_frames=4)
        assert rc == 0 and all(len(x) == 12 * 1920 for x in audio)
        b = m.generate_stream(THREE[0], SPK, LANG, chunk_frames=4)
        np.testing.assert_array_equal(a, b)
        assert np.abs(audio[0] - a).max() < 1e-5
    finally:
        m.close()


# ---------------------------------------------------------------- 10. one-shot arming
def test_forced_codes_are_honoured_and_consumed(tts_tiny):
    m = tts_tiny
    m.set_params(max_tokens=4096, fixed=16, seed=42, **DEFAULT)
    rc, _ = m.generate_batch_stream(THREE, [SPK] * 3, [LANG] * 3, chunk_frames=4)
    assert rc == 0
    c0 = m.last_codes_batch(3, 16)
    assert m.last_drawn(1) is None                  # an unarmed call keeps no record
    f = c0[1].copy()
    f[4, 15] = (f[4, 15] + 1) % 2048
    m.force_codes(f, slot=1)
    rc, a1 = m.generate_batch_stream(THREE, [SPK] * 3, [LANG] * 3, chunk_frames=4)
    assert rc == 0
    c1 = m.last_codes_batch(3, 16)
    np.testing.assert_array_equal(c1[1], f)
    for b in (0, 2):
        np.testing.assert_array_equal(c1[b], c0[b])
    d = m.last_drawn(1)
    assert d is not None
    np.testing.assert_array_equal(d[:5], c0[1][:5])
    # consumed: the next call is free again
    rc, _ = m.generate_batch_stream(THREE, [SPK] * 3, [LANG] * 3, chunk_frames=4)
    assert rc == 0
    for b in range(3):
        np.testing.assert_array_equal(m.last_codes_slot(b, 16), c0[b])
    assert m.last_drawn(1) is None


# ---------------------------------------------------------------- 11. the CLI
def test_cli_batch_stream(tiny_dir):
    ids = ",".join(str(i) for i in prompt_ids("short"))
    base = [qtts.CLI_PATH, "-d", tiny_dir, "-t", ids, "-s", SPK, "-l", LANG, "--fixed-codec-tokens", "8"]
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(base + ["-o", os.path.join(d, "s.wav"), "--batch", "3", "--stream", "2", "--seed-step", "1",
                                   "-v"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert re.search(r"First packet: [0-9.]+ ms", r.stderr), r.stderr
        assert sorted(os.listdir(d)) == ["s.wav", "s_1.wav", "s_2.wav"]
        r = subprocess.run(base + ["-o", os.path.join(d, "b.wav"), "--batch", "3"], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr
        assert "First packet" not in r.stderr
        assert os.path.exists(os.path.join(d, "b.wav"))
