"""Instruct and voice design on the GPU (qwen_tts_set_utterance_instruct): the
instruct's projected ids stand in front of the prompt rows and nothing else
changes.

The expected codes come from the unchanged oracle port: the oracle's own
prompt with Oracle.embed_text of every instruct id concatenated in front, run
through Oracle.generate_from_prompt.  Bars: codes bit-exact (parity.codes_equal),
audio audio_close (1e-4) to the oracle's codec decode of those codes.

Instruct lengths: 1, the two that make the prompt 16 and 17 rows (the <= 16-row
prefill kernel's limit, computed from the unarmed p_len), and 40.
"""
import numpy as np
import pytest

from conftest import manifest, model_dir
from oracle_py import DEFAULT, Oracle
from parity import codes_equal
from qtts_io import lookup_ids
from synth_model import prompt_ids

import qtts

pytestmark = pytest.mark.gpu

SPF = 1920
RNG = np.random.Generator(np.random.PCG64(20240))
POOL = RNG.integers(1000, 100000, size=64).tolist()   # instruct ids are drawn from here: ins(n) = POOL[:n]


def ins(n, off=0):
    return POOL[off:off + n]


def audio_close(a, ref, what):
    assert a is not None and a.shape == ref.shape, (what, None if a is None else a.shape, ref.shape)
    mse = float(np.mean((a.astype(np.float64) - ref) ** 2)) if len(ref) else 0.0
    assert mse < 1e-4, (what, mse)
    if len(ref):
        assert np.abs(a - ref).max() < 1e-4, (what, np.abs(a - ref).max())


@pytest.fixture(scope="module")
def tiny(gpu, tiny_dir):
    m = qtts.QwenTTS(tiny_dir)
    o = Oracle(tiny_dir)
    yield m, o
    m.close()
    o.close()


@pytest.fixture(scope="module")
def tiny_eos(gpu):
    md = model_dir("tiny", eos_gain=manifest()["eos_gain"])
    m = qtts.QwenTTS(md)
    o = Oracle(md)
    yield m, o
    m.close()
    o.close()


_ORC = {}


def want(o, ids, speaker, language, instruct, max_tokens, fixed, seed):
    """the oracle's run of one utterance with its instruct (codes, stop reason, waveform), cached per oracle"""
    key = (id(o), tuple(ids), speaker, language, tuple(instruct), max_tokens, fixed, seed)
    if key not in _ORC:
        s, l = lookup_ids(o.cfg, speaker, language)
        pre, tr = o.build_prompt(ids, s, l)
        if len(instruct):
            pre = np.concatenate([np.stack([o.embed_text(i) for i in instruct]), pre])
        codes, stop = o.generate_from_prompt(pre, tr, max_tokens=max_tokens, fixed=fixed, seed=seed, **DEFAULT)
        _ORC[key] = (codes, stop, o.codec_decode(codes))
    return _ORC[key]


def p_len_of(o, speaker="aiden", language="english"):
    s, l = lookup_ids(o.cfg, speaker, language)
    return o.build_prompt(prompt_ids("short"), s, l)[0].shape[0]


def lengths(o):
    p = p_len_of(o)
    return [1, 16 - p, 17 - p, 40]


# ---------------------------------------------------------------- 1. single runs
def test_lengths_hit_the_16_row_boundary(tiny):
    _, o = tiny
    assert lengths(o) == [1, 6, 7, 40]   # (aiden / english on the short prompt: p_len 10)


@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("mode", ["fixed", "eos"])
def test_single(tiny, tiny_eos, mode, k):
    m, o = tiny if mode == "fixed" else tiny_eos
    n = lengths(o)[k]
    ids = prompt_ids("short")
    max_tokens, fixed = (4096, 6) if mode == "fixed" else (32, 0)
    m.set_params(max_tokens=max_tokens, fixed=fixed, seed=11, **DEFAULT)
    m.set_utterance_instruct([ins(n)])
    audio = m.generate(ids, "aiden", "english")
    assert not m.c.instruct
    codes, stop, wav = want(o, ids, "aiden", "english", ins(n), max_tokens, fixed, 11)
    codes_equal(m.last_codes(), codes, f"instruct of {n} ids, {mode}")
    audio_close(audio, wav, f"instruct of {n} ids, {mode}")
    plain, _, _ = want(o, ids, "aiden", "english", [], max_tokens, fixed, 11)
    assert codes.shape != plain.shape or not np.array_equal(codes, plain)   # (the instruct changes the utterance)


@pytest.mark.parametrize("language", ["english", "auto"])
def test_voice_design_no_speaker(tiny, language):
    m, o = tiny
    ids = prompt_ids("short")
    m.set_params(max_tokens=4096, fixed=6, seed=3, **DEFAULT)
    for speaker in (None, ""):
        m.set_utterance_instruct([ins(7)])
        audio = m.generate(ids, speaker, language)
        codes, _, wav = want(o, ids, None, language, ins(7), 4096, 6, 3)
        codes_equal(m.last_codes(), codes, f"voice design, {language}")
        audio_close(audio, wav, f"voice design, {language}")


# ---------------------------------------------------------------- 2. batch
def test_batch_of_four_mixed_instructs(tiny):
    m, o = tiny
    prompts = [prompt_ids("short"), prompt_ids("p128", 1300), prompt_ids("short"), prompt_ids("p128", 1301)]
    per = [None, ins(1), ins(7), ins(40)]
    m.set_params(max_tokens=4096, fixed=6, seed=5, **DEFAULT)
    m.generate(prompts[0], "aiden", "english")
    unarmed = m.last_codes()
    m.set_utterance_instruct(per)
    rc, audio = m.generate_batch(prompts, ["aiden"] * 4, ["english"] * 4)
    assert rc == 0 and not m.c.instruct
    got = m.last_codes_batch(4)
    for b in range(4):
        codes, _, wav = want(o, prompts[b], "aiden", "english", per[b] or [], 4096, 6, 5)
        codes_equal(got[b][:6], codes, f"slot {b}")
        audio_close(audio[b], wav, f"slot {b}")
    np.testing.assert_array_equal(got[0][:6], unarmed)   # the none-slot equals the unarmed call


# ---------------------------------------------------------------- 3. streaming
def test_streams_give_the_non_streamed_codes(tiny):
    m, o = tiny
    ids = prompt_ids("short")
    m.set_params(max_tokens=4096, fixed=9, seed=8, **DEFAULT)
    m.set_utterance_instruct([ins(7)])
    m.generate(ids, "aiden", "english")
    base = m.last_codes()
    chunks = []
    m.set_utterance_instruct([ins(7)])
    audio = m.generate_stream(ids, "aiden", "english", chunk_frames=4, on_chunk=chunks.append)
    np.testing.assert_array_equal(m.last_codes(), base)
    np.testing.assert_array_equal(np.concatenate(chunks), audio)
    assert len(chunks[0]) == SPF
    codes, _, wav = want(o, ids, "aiden", "english", ins(7), 4096, 9, 8)
    codes_equal(base, codes, "streamed single")
    audio_close(audio, wav, "streamed single")
    # the batch form
    per = [ins(40), None, ins(1)]
    prompts = [ids, prompt_ids("p128", 1300), ids]
    m.set_utterance_instruct(per)
    rc, plain_audio = m.generate_batch(prompts, ["aiden"] * 3, ["english"] * 3)
    assert rc == 0
    base = m.last_codes_batch(3)
    got = {b: [] for b in range(3)}
    m.set_utterance_instruct(per)
    rc, audio = m.generate_batch_stream(prompts, ["aiden"] * 3, ["english"] * 3, chunk_frames=4,
                                        on_chunk=lambda b, a: got[b].append(a))
    assert rc == 0 and not m.c.instruct
    now = m.last_codes_batch(3)
    for b in range(3):
        np.testing.assert_array_equal(now[b], base[b])
        np.testing.assert_array_equal(np.concatenate(got[b]), audio[b])
        codes, _, wav = want(o, prompts[b], "aiden", "english", per[b] or [], 4096, 9, 8)
        codes_equal(now[b][:9], codes, f"streamed slot {b}")
        audio_close(audio[b], wav, f"streamed slot {b}")


# ---------------------------------------------------------------- 4. queue
@pytest.mark.parametrize("cache", [16, 0], ids=["cache", "one-pass"])
@pytest.mark.parametrize("streamed", [False, True], ids=["plain", "stream"])
def test_queue_seven_on_three(tiny_eos, cache, streamed):
    """mixed instructs (none, repeats) and per-utterance seeds; with the cache
    off the refills' p_len - 1 rows are 16 and 17 (utterances 3 and 4)"""
    m, o = tiny_eos
    p = p_len_of(o)
    a, b = ins(17 - p), ins(18 - p, 20)
    per = [ins(40), None, ins(1), a, b, a, None]
    prompts = [prompt_ids("short"), prompt_ids("p128", 1300), prompt_ids("p128", 1301), prompt_ids("short"),
               prompt_ids("p128", 1310), prompt_ids("p128", 1311), prompt_ids("short")]
    assert [p + len(x or []) - 1 for x in per[3:5]] == [16, 17]
    m.prefix_cache(cache)
    try:
        m.set_params(max_tokens=32, fixed=0, seed=7, **DEFAULT)
        m.set_utterance_instruct(per)
        m.set_utterance_sampling([{"seed": 100 + u} for u in range(7)])
        chunks = {u: [] for u in range(7)}
        if streamed:
            rc, audio = m.generate_queue_stream(prompts, ["aiden"] * 7, ["english"] * 7, slots=3, chunk_frames=4,
                                                on_chunk=lambda u, x: chunks[u].append(x))
        else:
            rc, audio = m.generate_queue(prompts, ["aiden"] * 7, ["english"] * 7, slots=3)
        assert rc == 0 and not m.c.instruct and not m.c.sampling
        st = m.queue_stats()
        assert st["slots"] == 3 and st["refills"] == 4, st
        for u in range(7):
            codes, stop, wav = want(o, prompts[u], "aiden", "english", per[u] or [], 32, 0, 100 + u)
            codes_equal(m.queue_codes(u), codes, f"utterance {u} (slot {st['slot'][u]})")
            assert st["stop_reason"][u] == stop, u
            audio_close(audio[u], wav, f"utterance {u}")
            if streamed:
                np.testing.assert_array_equal(np.concatenate(chunks[u]), audio[u])
    finally:
        m.prefix_cache(16)


# ---------------------------------------------------------------- 5. one-shot
def test_one_shot_and_refusals(tiny):
    m, o = tiny
    ids = prompt_ids("short")
    m.set_params(max_tokens=4096, fixed=4, seed=2, **DEFAULT)
    plain, _, _ = want(o, ids, "aiden", "english", [], 4096, 4, 2)

    def plain_ok():
        assert m.generate(ids, "aiden", "english") is not None
        codes_equal(m.last_codes(), plain, "a plain call")

    m.set_utterance_instruct([ins(7)])
    assert m.generate(ids, "aiden", "english") is not None and not m.c.instruct
    assert not np.array_equal(m.last_codes(), plain)
    plain_ok()                                               # the call after an armed call is plain
    m.set_utterance_instruct([ins(7), ins(1)])               # 2 instructs for 3 utterances
    rc, audio = m.generate_batch([ids] * 3, ["aiden"] * 3, ["english"] * 3)
    assert rc == -1 and audio == [None] * 3 and not m.c.instruct
    plain_ok()
    m.set_utterance_instruct([ins(7)] * 2)                   # 2 instructs for a queue of 3
    rc, audio = m.generate_queue([ids] * 3, ["aiden"] * 3, ["english"] * 3, slots=2)
    assert rc == -1 and not m.c.instruct
    plain_ok()
    m.set_utterance_instruct([ins(7)])                       # voice clone takes no instruct
    vec = np.zeros(m.cfg.talker_hidden, np.float32)
    assert m.generate_voice_clone(ids, spk_embed=vec, language="english") is None and not m.c.instruct
    plain_ok()
    with pytest.raises(ValueError):
        m.set_utterance_instruct([[m.cfg.talker_text_vocab]])   # an id out of range
    assert not m.c.instruct
    plain_ok()
