"""Voice handles and the voice-clone work queue, plain and streamed
(qwen_tts_voice_*, qwen_tts_generate_voice_queue[_stream]): the queue's decode
with every utterance spoken in a cloned voice through the ICL prompt.  A handle
primes the codec with its reference frames once; every admission of the
streamed form, initial or refill, restores that snapshot into the slot's
stream instead of pushing the reference frames again.

Bounds are the project's: codes bit-exact, 1e-5 max-abs between two device
decodes of the same codes, audio_close (1e-4) against the oracle.
"""
import numpy as np
import pytest

from conftest import golden, manifest, model_dir
from oracle_py import DEFAULT, GREEDY, Oracle
from qtts_io import lookup_ids
from synth_model import prompt_ids
from test_gpu_queue_stream import _discipline, _tiny_prompts
from test_voice_clone import REF_IDS, _inputs

import qtts

pytestmark = pytest.mark.gpu

SPF = 1920
LANG = "english"
MAX_TOKENS, SLOTS, CHUNK = 24, 3, 4
# three voices: ICL with 17 reference frames, ICL with 63, x-vector only
NREF = [17, 63, 0]
VOICE = [0, 1, 2, 1, 0, 2, 1]            # the voice of each of the 7 utterances
# default sampling of the tiny EOS model by the CPU oracle, max_tokens 24
# (utterance: seed -> frames, stop):
#   0 (17 frames): 6 -> 14 eos      1 (63 frames): 3 -> 9 eos      2 (x-vector): 2 -> 24 max_tokens
#   3 (63 frames): 1 -> 11 eos      4 (17 frames): 8 -> 7 eos      5 (x-vector): 2 -> 7 eos
#   6 (63 frames): 3 -> 11 eos
# so utterance 1 stops first and its slot is refilled with utterance 3, an ICL voice
SEEDS = [6, 3, 2, 1, 8, 2, 3]


def audio_close(a, ref, what=""):
    assert a is not None and a.shape == ref.shape, (what, None if a is None else a.shape, ref.shape)
    mse = float(np.mean((a.astype(np.float64) - ref) ** 2)) if len(ref) else 0.0
    assert mse < 1e-4, (what, mse)
    if len(ref):
        assert np.abs(a - ref).max() < 1e-4, (what, np.abs(a - ref).max())


def _voice_inputs(o):
    """(ref ids, ref codes, x-vector) of the three voices"""
    a, b, c = _inputs(o, 17, seed=31, spk=True), _inputs(o, 63, seed=32, spk=True), _inputs(o, 1, seed=33, spk=True)
    return [(REF_IDS, a[0], a[1]), (REF_IDS[:3] + [4000, 4001] + REF_IDS[-2:], b[0], b[1]), (None, None, c[1])]


def _streamed(m, prompts, voices, slots=SLOTS, chunk=CHUNK):
    """generate_voice_queue_stream with the admissions and the chunks logged in arrival order"""
    events = []
    seq = iter(range(len(prompts)))

    def next_fn():
        u = next(seq, -1)
        events.append(("admit", u, 0))
        return u

    rc, audio = m.generate_voice_queue_stream(prompts, voices, [LANG] * len(prompts), slots=slots, next_fn=next_fn,
                                              chunk_frames=chunk, on_chunk=lambda u, a: events.append(("chunk", u, a)))
    return rc, audio, events


@pytest.fixture(scope="module")
def run(gpu):
    """the 7-utterance run in both forms, a second streamed call on the primed
    handles, the single calls and the oracle's results"""
    md = model_dir("tiny", eos_gain=manifest()["eos_gain"])
    m, o = qtts.QwenTTS(md), Oracle(md)
    try:
        prompts = _tiny_prompts()[:7]
        vin = _voice_inputs(o)
        _, lang = lookup_ids(o.cfg, "aiden", LANG)
        want = []
        for u in range(7):
            rid, rc_, sv = vin[VOICE[u]]
            pre, tr = o.build_icl_prompt(prompts[u], rid, rc_, sv, lang, 0)
            want.append(o.generate_from_prompt(pre, tr, max_tokens=MAX_TOKENS, fixed=0, seed=SEEDS[u], **DEFAULT))
        hs = [m.voice_create(*v) for v in vin]
        assert all(hs)
        info0 = [m.voice_info(h) for h in hs]
        voices = [hs[v] for v in VOICE]
        per = [dict(seed=s) for s in SEEDS]
        r = dict(prompts=prompts, vin=vin, want=want, info0=info0)

        # the other streaming calls on this context, before any voice call
        def others():
            m.set_params(max_tokens=4096, fixed=8, seed=42, **DEFAULT)
            rc1, a1 = m.generate_queue_stream(prompts[:5], ["aiden"] * 5, [LANG] * 5, slots=2, chunk_frames=4)
            ids = [prompts[0]] * 2
            rc2, a2 = m.generate_voice_clone_batch_stream(ids, [vin[0][0], None], [vin[0][1], None],
                                                          [vin[0][2], vin[2][2]], [LANG] * 2, chunk_frames=2)
            assert rc1 == 0 and rc2 == 0
            return a1 + a2
        r["before"] = others()

        m.set_params(max_tokens=MAX_TOKENS, fixed=0, seed=42, **DEFAULT)
        m.set_utterance_sampling(per)
        r["prc"], r["paudio"] = m.generate_voice_queue(prompts, voices, [LANG] * 7, slots=SLOTS)
        r["pcodes"] = [m.queue_codes(i) for i in range(7)]
        r["pstats"] = m.queue_stats()
        r["info1"] = [m.voice_info(h) for h in hs]      # the plain form primes nothing

        m.set_utterance_sampling(per)
        r["src"], r["saudio"], r["events"] = _streamed(m, prompts, voices)
        r["scodes"] = [m.queue_codes(i) for i in range(7)]
        r["sstats"] = m.queue_stats()
        r["perf"] = (m.c.perf_first_packet_ms, m.c.perf_total_ms, m.c.perf_codec_ms)
        r["info2"] = [m.voice_info(h) for h in hs]

        m.set_utterance_sampling(per)
        r["src2"], r["saudio2"], _ = _streamed(m, prompts, voices)
        r["scodes2"] = [m.queue_codes(i) for i in range(7)]
        r["info3"] = [m.voice_info(h) for h in hs]

        r["after"] = others()

        # every utterance alone, plain and streamed
        r["alone_codes"], r["alone_stream"] = [], []
        for u in range(7):
            rid, rc_, sv = vin[VOICE[u]]
            m.set_params(max_tokens=MAX_TOKENS, fixed=0, seed=SEEDS[u], **DEFAULT)
            assert m.generate_voice_clone(prompts[u], rid, rc_, sv, LANG) is not None
            r["alone_codes"].append(m.last_codes())
            a = m.generate_voice_clone_stream(prompts[u], rid, rc_, sv, LANG, 0, chunk_frames=CHUNK)
            np.testing.assert_array_equal(m.last_codes(), r["alone_codes"][u])
            r["alone_stream"].append(a)
        r["decode"] = [o.codec_decode(np.concatenate([vin[VOICE[u]][1], want[u][0]]) if NREF[VOICE[u]]
                                      else want[u][0]) for u in range(7)]
        for h in hs:
            m.voice_free(h)
        return r
    finally:
        m.close()
        o.close()


def test_the_oracles_results_make_the_run_meaningful(run):
    """from the oracle alone: different lengths, an EOS stop before max_tokens,
    and a refill that admits an ICL voice"""
    frames = [len(c) for c, _ in run["want"]]
    stops = [s for _, s in run["want"]]
    assert len(set(frames)) >= 2, frames
    assert any(s == 1 and f < MAX_TOKENS for f, s in zip(frames, stops)), (frames, stops)
    assert all(f > 0 for f in frames), frames
    # in-order admission on 3 slots: the first slot to free takes utterance 3, and so on
    busy = [(frames[b], b) for b in range(SLOTS)]
    refills = []
    for u in range(SLOTS, 7):
        t, b = min(busy)
        busy.remove((t, b))
        refills.append(u)
        busy.append((t + frames[u], b))
    assert any(NREF[VOICE[u]] > 0 for u in refills), refills


def test_codes_are_the_oracles_and_the_single_calls(run):
    assert run["prc"] == 0 and run["src"] == 0
    for u in range(7):
        want, stop = run["want"][u]
        np.testing.assert_array_equal(run["pcodes"][u], want)
        np.testing.assert_array_equal(run["scodes"][u], want)
        np.testing.assert_array_equal(run["pcodes"][u], run["alone_codes"][u])
        np.testing.assert_array_equal(run["scodes"][u], run["alone_codes"][u])
        assert run["pstats"]["stop_reason"][u] == stop and run["sstats"]["stop_reason"][u] == stop, u


def test_plain_audio(run):
    for u in range(7):
        T, full = NREF[VOICE[u]], run["decode"][u]
        tot = T + len(run["want"][u][0])
        cut = int(T / tot * len(full))          # the non-streamed batch's float cut
        audio_close(run["paudio"][u], full[cut:], f"utterance {u}")


def test_streamed_audio(run):
    class Stats:       # (_discipline reads the frames per utterance from queue_stats)
        def queue_stats(self):
            return run["sstats"]
    _discipline(Stats(), run["saudio"], run["events"], list(range(7)), chunk=CHUNK)
    worst = 0.0
    for u in range(7):
        a, T = run["saudio"][u], NREF[VOICE[u]]
        assert len(a) == len(run["want"][u][0]) * SPF, u
        audio_close(a, run["decode"][u][T * SPF:], f"utterance {u}")
        alone = run["alone_stream"][u]
        assert alone.shape == a.shape, u
        worst = max(worst, float(np.abs(a - alone).max()))
    print(f"measured  largest |queue-streamed utterance - generate_voice_clone_stream alone| {worst:.3e}")
    assert worst < 1e-5, worst
    first, total, codec = run["perf"]
    assert 0 < first < total and codec > 0


def test_queue_stats_show_refills(run):
    for st in (run["pstats"], run["sstats"]):
        assert st["slots"] == SLOTS and st["refills"] == 4, st
        assert st["frames_per_utt"] == [len(c) for c, _ in run["want"]], st


def test_handles_are_primed_once_and_reused(run):
    assert [i["n_ref_frames"] for i in run["info0"]] == NREF
    assert [i["primed"] for i in run["info0"]] == [0, 0, 0]
    assert [i["primed"] for i in run["info1"]] == [0, 0, 0]
    assert [i["primed"] for i in run["info2"]] == [1, 1, 0]      # an x-vector-only voice never has a snapshot
    assert [i["primed"] for i in run["info3"]] == [1, 1, 0]
    # the second call, on the primed handles, only restores: bit for bit the first call's result
    assert run["src2"] == 0
    for u in range(7):
        np.testing.assert_array_equal(run["scodes2"][u], run["scodes"][u])
        np.testing.assert_array_equal(run["saudio2"][u], run["saudio"][u])


def test_other_streaming_calls_unchanged_on_the_same_context(run):
    assert len(run["before"]) == len(run["after"]) == 7
    for x, y in zip(run["before"], run["after"]):
        np.testing.assert_array_equal(x, y)


def test_refused_before_the_device_is_touched(tts_tiny, oracle, capfd):
    md = model_dir("tiny", eos_gain=manifest()["eos_gain"])
    m = qtts.QwenTTS(md)
    try:
        vin = _voice_inputs(oracle)
        prompts = _tiny_prompts()[:2]
        mine, other = m.voice_create(*vin[0]), tts_tiny.voice_create(*vin[0])
        assert mine and other
        m.set_params(max_tokens=8, fixed=0, seed=42, **DEFAULT)
        m.set_utterance_sampling([dict(seed=1), dict(seed=2)])      # consumed by the refused call
        bytes0 = m.state_bytes()
        got = []
        capfd.readouterr()
        for voices, msg in (([mine, other], "utterance 1: the voice handle belongs to another context"),
                            ([None, mine], "utterance 0: no voice handle (NULL)")):
            for stream in (False, True):
                if stream:
                    rc, audio = m.generate_voice_queue_stream(prompts, voices, [LANG] * 2, slots=2,
                                                              on_chunk=lambda u, a: got.append(u))
                else:
                    rc, audio = m.generate_voice_queue(prompts, voices, [LANG] * 2, slots=2)
                assert rc == -1 and all(a is None for a in audio) and not got
                assert msg in capfd.readouterr().err
        assert not m.c.sampling
        # armed forcing: refused and disarmed, as the queue does
        m.force_codes(np.zeros((1, 16), np.int32), slot=0)
        rc, audio = m.generate_voice_queue_stream(prompts, [mine, mine], [LANG] * 2, slots=2,
                                                  on_chunk=lambda u, a: got.append(u))
        assert rc == -1 and all(a is None for a in audio) and not got and not m.c.force
        assert "forced codes / taps are armed" in capfd.readouterr().err
        assert m.state_bytes() == bytes0                       # no generation state was allocated
        assert m.voice_info(mine)["primed"] == 0
        # the handle still works where it belongs
        rc, audio = m.generate_voice_queue_stream(prompts, [mine, mine], [LANG] * 2, slots=2)
        assert rc == 0 and all(a is not None for a in audio) and m.voice_info(mine)["primed"] == 1
        m.voice_free(mine)
        tts_tiny.voice_free(other)
    finally:
        m.close()


def test_voice_create_refusals(tts_tiny, oracle, capfd):
    m = tts_tiny
    codes, sv = _inputs(oracle, 5, seed=3, spk=True)
    capfd.readouterr()
    assert m.voice_create(None, None, None) is None
    assert "voice clone needs reference codes or a speaker embedding" in capfd.readouterr().err
    assert m.voice_create([1, 2, 3], codes, sv) is None
    assert "ICL voice clone needs the reference text ids" in capfd.readouterr().err
    assert m.voice_create(REF_IDS[:-1] + [10 ** 8], codes, sv) is None
    assert "out of range" in capfd.readouterr().err
    assert m.voice_info(None) is None


def test_voice_create_audio_equals_the_encoders(gpu):
    G = golden("enc_tiny.npz")
    m = qtts.QwenTTS(model_dir("tiny_vc"))
    try:
        assert m.encoders_available() == 3
        ref_ids = [151644, 77091, 198, 2354, 151645, 198]
        ids = [prompt_ids("short"), prompt_ids("p128", seed=1235)]
        wav = G["wav0"]
        codes, xv = m.encode_audio_api(wav), m.speaker_embedding_api(wav)
        v_audio, v_codes = m.voice_create_audio(wav, ref_ids), m.voice_create(ref_ids, codes, xv)
        x_audio, x_codes = m.voice_create_audio(wav, None, x_vector_only=True), m.voice_create(None, None, xv)
        assert v_audio and v_codes and x_audio and x_codes
        assert m.voice_info(v_audio)["n_ref_frames"] == len(codes) and m.voice_info(x_audio)["n_ref_frames"] == 0
        m.set_params(max_tokens=4096, fixed=5, seed=42, **GREEDY)
        # the handle made from audio holds the encoders' codes and x-vector: the same utterances, bit for bit
        rc1, a1 = m.generate_voice_queue_stream(ids, [v_audio, x_audio], [LANG] * 2, slots=2, chunk_frames=2)
        c1 = [m.queue_codes(i) for i in range(2)]
        rc2, a2 = m.generate_voice_queue_stream(ids, [v_codes, x_codes], [LANG] * 2, slots=2, chunk_frames=2)
        c2 = [m.queue_codes(i) for i in range(2)]
        assert rc1 == 0 and rc2 == 0
        a = m.generate_voice_clone(ids[0], ref_ids, codes, xv, LANG)
        assert a is not None
        np.testing.assert_array_equal(c1[0], m.last_codes())
        for i in range(2):
            np.testing.assert_array_equal(c1[i], c2[i])
            np.testing.assert_array_equal(a1[i], a2[i])
        for v in (v_audio, v_codes, x_audio, x_codes):
            m.voice_free(v)
    finally:
        m.close()
