"""qwen_tts_generate_voice_clone_batch_stream: generate_voice_clone_batch's
codes, bit for bit, with every slot's audio delivered in chunks by the
multi-stream exact codec.  The reference frames of all ICL slots are primed in
one ragged push (63, 7 and 17 frames here: 63 takes four passes of 16 while
the others drop out; the x-vector-only slot has none and stays at position
0), so each stream carries the state of decoding reference ++ generated.

Bounds are the project's: codes bit-exact, audio_close (1e-4) against the
oracle, 1e-5 max-abs between two device decodes of the same codes
(test_gpu_codec_mstream_pos.py, test_voice_clone.py::test_voice_clone_stream).
"""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import golden, manifest, model_dir
from oracle_py import DEFAULT, GREEDY
from qtts_io import lookup_ids
from synth_model import prompt_ids
from test_gpu_batch_stream import Chunks, THREE
from test_voice_clone import REF_IDS, _inputs

import qtts

pytestmark = pytest.mark.gpu

LANG = "english"
NREF = [63, 7, 0, 17]            # reference frames per slot (0: x-vector only)
FIXED, CHUNK = 6, 2
PARAMS = {"greedy": GREEDY, "default": DEFAULT}


def audio_close(a, ref):
    assert a is not None and a.shape == ref.shape, (None if a is None else a.shape, ref.shape)
    mse = float(np.mean((a.astype(np.float64) - ref) ** 2)) if len(ref) else 0.0
    assert mse < 1e-4, mse
    if len(ref):
        assert np.abs(a - ref).max() < 1e-4, np.abs(a - ref).max()


def _slots(o):
    """(prompts, ref ids, ref codes, x-vectors) of the four slots"""
    prompts = [prompt_ids("short"), prompt_ids("p128", 1240), prompt_ids("p128", 1241), prompt_ids("p128", 1242)]
    refs = [_inputs(o, max(t, 1), seed=40 + b, spk=True) for b, t in enumerate(NREF)]
    codes = [r[0] if t else None for r, t in zip(refs, NREF)]
    spk = [refs[0][1], None, refs[2][1], refs[3][1]]
    rids = [REF_IDS, REF_IDS[:3] + [4000, 4001] + REF_IDS[-2:], None, REF_IDS]
    return prompts, rids, codes, spk


@pytest.fixture(scope="module", params=sorted(PARAMS))
def run(request, tts_tiny, oracle):
    """one streamed four-slot call, the non-streamed call on the same inputs, the oracle's codes"""
    m, pp = tts_tiny, PARAMS[request.param]
    prompts, rids, codes, spk = _slots(oracle)
    m.set_params(max_tokens=4096, fixed=FIXED, seed=42, **pp)
    got = Chunks(4)
    rc, audio = m.generate_voice_clone_batch_stream(prompts, rids, codes, spk, [LANG] * 4, chunk_frames=CHUNK,
                                                    on_chunk=got)
    scodes = [m.last_codes_slot(b, FIXED) for b in range(4)]
    perf = (m.c.perf_first_packet_ms, m.c.perf_total_ms, m.c.perf_codec_ms)
    rc2, ref = m.generate_voice_clone_batch(prompts, rids, codes, spk, [LANG] * 4)
    rcodes = [m.last_codes_slot(b, FIXED) for b in range(4)]
    _, lang = lookup_ids(oracle.cfg, "aiden", LANG)
    want = []
    for b in range(4):
        pre, tr = oracle.build_icl_prompt(prompts[b], rids[b], codes[b], spk[b], lang, 0)
        want.append(oracle.generate_from_prompt(pre, tr, max_tokens=4096, fixed=FIXED, seed=42, **pp)[0])
    return dict(pp=pp, rc=rc, audio=audio, got=got, scodes=scodes, perf=perf, rc2=rc2, ref=ref, rcodes=rcodes,
                want=want, inputs=(prompts, rids, codes, spk))


# ---------------------------------------------------------------- 2. the four-slot run
def test_codes_are_the_batch_calls_and_the_oracles(run):
    assert run["rc"] == 0 and run["rc2"] == 0
    for b in range(4):
        np.testing.assert_array_equal(run["scodes"][b], run["want"][b])
        np.testing.assert_array_equal(run["scodes"][b], run["rcodes"][b])


def test_chunks_and_audio(run, oracle):
    got, audio = run["got"], run["audio"]
    codes = run["inputs"][2]
    for b in range(4):
        assert got.sizes(b) == [1920, 2 * 1920, 2 * 1920, 1920], (b, got.sizes(b))
        np.testing.assert_array_equal(np.concatenate(got.per[b]), audio[b])
        T, want = NREF[b], run["want"][b]
        full = oracle.codec_decode(np.concatenate([codes[b], want]) if T else want)
        audio_close(audio[b], full[T * 1920:])
        # the non-streamed batch cuts at int(T / tot * samples), at most one
        # sample before the frame boundary (test_voice_clone.py::test_voice_clone_stream)
        a, r = audio[b], run["ref"][b]
        tot = T + len(want)
        off = T * 1920 - int(T / tot * (tot * 1920))
        assert off in (0, 1) and len(r) == len(a) + off, (b, off, len(r), len(a))
        audio_close(r[off:], a)
    first, total, codec = run["perf"]
    assert 0 < first < total and codec > 0


def test_icl_slots_equal_the_single_streamed_call(run, tts_tiny):
    m = tts_tiny
    prompts, rids, codes, spk = run["inputs"]
    m.set_params(max_tokens=4096, fixed=FIXED, seed=42, **run["pp"])
    worst = 0.0
    for b in range(4):
        if not NREF[b]:
            continue
        a = m.generate_voice_clone_stream(prompts[b], rids[b], codes[b], spk[b], LANG, 0, chunk_frames=CHUNK)
        np.testing.assert_array_equal(m.last_codes(), run["scodes"][b])
        assert a.shape == run["audio"][b].shape
        worst = max(worst, float(np.abs(a - run["audio"][b]).max()))
    print(f"measured  largest |batch-streamed slot - generate_voice_clone_stream alone| {worst:.3e}")
    assert worst < 1e-5, worst


# ---------------------------------------------------------------- 3. EOS mode
# default sampling of the tiny EOS model by the CPU oracle, max_tokens 24 (frames, stop):
#   17 reference frames (seed 31): seed 2 -> 18 eos, seed 5 -> 13 eos
#   x-vector only (seed 33):       seed 2 -> 24 max_tokens, seed 7 -> 10 eos
EOS_SEEDS = [2, 5, 2, 7]
EOS_CHUNK = 4


def test_eos_mode_no_callback_after_the_last_frame(oracle):
    m = qtts.QwenTTS(model_dir("tiny", eos_gain=manifest()["eos_gain"]))
    try:
        ids = [prompt_ids("short")] * 4
        icl, xv = _inputs(oracle, 17, seed=31, spk=True), _inputs(oracle, 1, seed=33, spk=True)
        rids = [REF_IDS, REF_IDS, None, None]
        codes = [icl[0], icl[0], None, None]
        spk = [icl[1], icl[1], xv[1], xv[1]]
        m.set_params(max_tokens=24, fixed=0, seed=42, **DEFAULT)
        m.set_utterance_sampling([dict(seed=s) for s in EOS_SEEDS])
        rc, ref = m.generate_voice_clone_batch(ids, rids, codes, spk, [LANG] * 4)
        assert rc == 0
        ref_codes = [m.last_codes_slot(b, 24) for b in range(4)]
        frames = [len(c) for c in ref_codes]
        # the precondition, from the non-streamed call's own result: different stop
        # frames, a stop that leaves a short tail beside a full chunk, a run to max_tokens
        assert len({f for f in frames if f < 24}) >= 2, frames
        assert any(f < 24 and (f - 1) % EOS_CHUNK != 0 for f in frames), frames
        assert 24 in frames, frames
        got = Chunks(4)
        m.set_utterance_sampling([dict(seed=s) for s in EOS_SEEDS])
        rc, audio = m.generate_voice_clone_batch_stream(ids, rids, codes, spk, [LANG] * 4, chunk_frames=EOS_CHUNK,
                                                        on_chunk=got)
        assert rc == 0
        last_seen = {b: max(i for i, x in enumerate(got.order) if x == b) for b in range(4)}
        for b in range(4):
            np.testing.assert_array_equal(m.last_codes_slot(b, 24), ref_codes[b])
            assert sum(got.sizes(b)) == frames[b] * 1920, (b, got.sizes(b), frames[b])
            assert all(s > 0 and s % 1920 == 0 for s in got.sizes(b))
            np.testing.assert_array_equal(np.concatenate(got.per[b]), audio[b])
            T = 0 if codes[b] is None else len(codes[b])
            tot = T + frames[b]
            off = T * 1920 - int(T / tot * (tot * 1920))
            assert off in (0, 1) and len(ref[b]) == len(audio[b]) + off
            audio_close(ref[b][off:], audio[b])
            # once its samples are complete an utterance is never called again
            done_at = np.cumsum(got.sizes(b)).tolist().index(frames[b] * 1920)
            assert done_at == len(got.per[b]) - 1
        by_len = sorted(range(4), key=lambda b: frames[b])
        for a, b in zip(by_len, by_len[1:]):
            if frames[a] < frames[b]:
                assert last_seen[a] < last_seen[b], (frames, got.order)
        # a short tail went out beside the running slots' full chunk
        assert any(got.sizes(b)[-1] // 1920 < EOS_CHUNK for b in range(4) if frames[b] < 24), \
            [got.sizes(b) for b in range(4)]
    finally:
        m.close()


# ---------------------------------------------------------------- 4. the same context before and after
def test_batch_stream_before_and_after_on_one_context(tts_tiny, oracle):
    m = tts_tiny
    prompts, rids, codes, spk = _slots(oracle)

    def plain():
        m.set_params(max_tokens=4096, fixed=8, seed=42, **DEFAULT)
        rc, audio = m.generate_batch_stream(THREE, ["aiden"] * 3, [LANG] * 3, chunk_frames=4)
        assert rc == 0
        return audio

    before = plain()
    m.set_params(max_tokens=4096, fixed=FIXED, seed=42, **DEFAULT)
    rc, a1 = m.generate_voice_clone_batch_stream(prompts, rids, codes, spk, [LANG] * 4, chunk_frames=CHUNK)
    assert rc == 0
    after = plain()
    for x, y in zip(before, after):
        np.testing.assert_array_equal(x, y)
    # and the voice-clone stream itself again, on the state the plain batch stream left
    m.set_params(max_tokens=4096, fixed=FIXED, seed=42, **DEFAULT)
    rc, a2 = m.generate_voice_clone_batch_stream(prompts, rids, codes, spk, [LANG] * 4, chunk_frames=CHUNK)
    assert rc == 0
    for x, y in zip(a1, a2):
        np.testing.assert_array_equal(x, y)


# ---------------------------------------------------------------- 5. from reference audio
def test_audio_batch_stream_equals_encode_plus_codes_call(gpu):
    G = golden("enc_tiny.npz")
    m = qtts.QwenTTS(model_dir("tiny_vc"))
    try:
        assert m.encoders_available() == 3
        m.set_params(max_tokens=4096, fixed=5, seed=42, **GREEDY)
        ids = [prompt_ids("short"), prompt_ids("p128", seed=1235), prompt_ids("short")]
        ref_ids = [[151644, 77091, 198, 2354, 151645, 198], [151644, 77091, 198, 4041, 2244, 151645, 198], None]
        wavs = [G["wav0"], G["wav1"], G["wav0"]]
        xo = [False, False, True]
        got = Chunks(3)
        rc, outs = m.generate_voice_clone_audio_batch_stream(ids, wavs, ref_id_lists=ref_ids, languages=[LANG] * 3,
                                                             x_vector_only=xo, chunk_frames=CHUNK, on_chunk=got)
        assert rc == 0
        assert 0 < m.c.perf_first_packet_ms < m.c.perf_total_ms
        codes = m.encode_audio(wavs)          # the same padded batch encode
        xv = m.speaker_embed(wavs)
        rc2, ref = m.generate_voice_clone_batch_stream(ids, ref_ids, [codes[0], codes[1], None], list(xv),
                                                       [LANG] * 3, chunk_frames=CHUNK)
        assert rc2 == 0
        for b in range(3):
            np.testing.assert_array_equal(outs[b], ref[b])
            np.testing.assert_array_equal(np.concatenate(got.per[b]), outs[b])
    finally:
        m.close()


# ---------------------------------------------------------------- 6. CLI
def test_cli_voice_clone_batch_stream(tiny_dir, tts_tiny, oracle):
    """qwen-tts --ref-codes ... --batch 2 --stream 2 writes the API's slot 0; --batch 2 alone stays refused"""
    codes, sv = _inputs(oracle, 10, seed=5, spk=True)
    ids = prompt_ids("short")
    with tempfile.TemporaryDirectory() as d:
        cf, xf = os.path.join(d, "ref_codes.txt"), os.path.join(d, "xvec.txt")
        np.savetxt(cf, codes, fmt="%d")
        np.savetxt(xf, sv[None], fmt="%.9g")
        cmd = [qtts.CLI_PATH, "-d", tiny_dir, "-t", ",".join(map(str, ids)), "-l", LANG, "-o",
               os.path.join(d, "cli.wav"), "--fixed-codec-tokens", "5", "--seed", "42", "--ref-codes", cf,
               "--ref-text", ",".join(map(str, REF_IDS)), "--xvector", xf, "--batch", "2"]
        r = subprocess.run(cmd + ["--stream", "2"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        tts_tiny.set_params(max_tokens=4096, fixed=5, seed=42)
        rc, a = tts_tiny.generate_voice_clone_batch_stream([ids] * 2, [REF_IDS] * 2, [codes] * 2, [sv] * 2, [LANG] * 2,
                                                           chunk_frames=2)
        assert rc == 0
        api = os.path.join(d, "api.wav")
        assert qtts.lib().qwen_tts_write_wav(api.encode(), a[0].ctypes.data_as(qtts._fp), len(a[0]), 24000) == 0
        assert open(os.path.join(d, "cli.wav"), "rb").read() == open(api, "rb").read()
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "voice clone runs at --batch 1 without --stream" in r.stderr
