"""The streaming work queue (qwen_tts_generate_queue_stream): the queue's
decode -- admission, refill, retire, tail compaction, codes bit for bit -- with
every utterance's audio delivered as it is decoded, through multi-stream
codec streams at independent positions (a refilled slot's stream restarts at 0
beside its neighbours).

Bars: codes equal to qwen_tts_generate_queue's and to the oracle's single runs
(the reference's at full size); audio within 1e-5 of the device's full codec
decode of the same codes and audio_close (1e-4) to the oracle's; at full size
the bar test_gpu_queue.py applies to the same fixture.
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, manifest, model_dir
from oracle_py import DEFAULT, Oracle
from parity import codes_equal
from qtts_io import lookup_ids
from synth_model import prompt_ids

import qtts

pytestmark = pytest.mark.gpu

SPF = 1920
# The part of queue_stats that the inputs decide.  In EOS mode the rest
# (frames, rows_launched, the occupancies and, after the tail compaction, the
# slot an utterance finished on) also depends on WHEN the host reads the stop
# mirror: the sampler of frame `step`, already running, writes a slot's EOS
# into it early in the frame, so a read that comes late enough sees that stop
# one iteration sooner and refills one frame sooner.  That is so for the plain
# queue as well (its tests pin none of these), and the pushes change the
# host's timing: on the tiny model, 10 prompts on 3 slots launched 70 frames
# plain and 68 / 68 / 69 streamed with chunk 4 / 1 / 1000, each repeatably.
# In fixed-length mode no stop is read from the mirror and the whole of
# queue_stats is compared (test_fixed_length_refills_on_the_same_frame).
STATS_OF_THE_INPUTS = ("slots", "refills", "used", "stop_reason", "frames_per_utt")


def audio_close(a, ref, what):
    assert a is not None and a.shape == ref.shape, (what, None if a is None else a.shape, ref.shape)
    mse = float(np.mean((a.astype(np.float64) - ref) ** 2)) if len(ref) else 0.0
    assert mse < 1e-4, (what, mse)
    if len(ref):
        assert np.abs(a - ref).max() < 1e-4, (what, np.abs(a - ref).max())


def _tiny_prompts():
    return [prompt_ids("short"), prompt_ids("p128", 1300), prompt_ids("p128", 1301), prompt_ids("short")] + \
        [prompt_ids("p128", 1310 + i) for i in range(6)]


@pytest.fixture(scope="module")
def tiny_eos():
    md = model_dir("tiny", eos_gain=manifest()["eos_gain"])
    m = qtts.QwenTTS(md)
    o = Oracle(md)
    yield m, o
    m.close()
    o.close()


_ORC, _QUEUE = {}, {}


def _single(o, ids, max_tokens, fixed, seed):
    """the oracle's single run of one utterance (codes, stop reason, waveform), cached"""
    key = (tuple(int(i) for i in ids), max_tokens, fixed, seed)
    if key not in _ORC:
        s, l = lookup_ids(o.cfg, "aiden", "english")
        want, stop = o.generate_codes(ids, s, l, max_tokens=max_tokens, fixed=fixed, seed=seed, **DEFAULT)
        _ORC[key] = (want, stop, o.codec_decode(want))
    return _ORC[key]


def _plain_queue(m, key, prompts, slots, max_tokens, fixed, seed):
    """qwen_tts_generate_queue on the same inputs (codes, stats), once per case"""
    if key not in _QUEUE:
        n = len(prompts)
        m.set_params(max_tokens=max_tokens, fixed=fixed, seed=seed, **DEFAULT)
        rc, _ = m.generate_queue(prompts, ["aiden"] * n, ["english"] * n, slots=slots)
        assert rc == 0
        _QUEUE[key] = ([m.queue_codes(i) for i in range(n)], m.queue_stats())
    return _QUEUE[key]


def _streamed(m, prompts, slots, chunk=4, order=None):
    """generate_queue_stream with the admissions and the chunks logged in arrival order"""
    n = len(prompts)
    events = []
    seq = iter(order if order is not None else range(n))

    def next_fn():
        u = next(seq, -1)
        events.append(("admit", u, 0))
        return u

    rc, audio = m.generate_queue_stream(prompts, ["aiden"] * n, ["english"] * n, slots=slots, next_fn=next_fn,
                                        chunk_frames=chunk, on_chunk=lambda u, a: events.append(("chunk", u, a)))
    return rc, audio, events


def _discipline(m, audio, events, taken, chunk=4):
    """the callbacks of a run: per taken utterance 1 frame first, whole frames,
    the chunks are its audio bit for bit, none before its admission, none for
    the others"""
    frames = m.queue_stats()["frames_per_utt"]
    admitted, chunks = set(), {}
    for kind, u, a in events:
        if kind == "admit":
            admitted.add(u)
            continue
        assert u in admitted, f"utterance {u}: a chunk before its admission"
        chunks.setdefault(u, []).append(a)
    assert set(chunks) == set(taken), (sorted(chunks), taken)
    for u in taken:
        sizes = [len(a) for a in chunks[u]]
        assert sizes[0] == SPF and all(k > 0 and k % SPF == 0 for k in sizes), (u, sizes)
        assert sum(sizes) == frames[u] * SPF, (u, sizes, frames[u])
        # after the first packet and one aligning chunk, whole cadence chunks until the tail
        assert all(k == chunk * SPF for k in sizes[2:-1]), (u, sizes)
        np.testing.assert_array_equal(np.concatenate(chunks[u]), audio[u])


def _tiny_check(m, o, prompts, audio, taken, max_tokens, fixed, seed):
    st = m.queue_stats()
    for i in taken:
        want, stop, wav = _single(o, prompts[i], max_tokens, fixed, seed)
        codes_equal(m.queue_codes(i), want, f"utterance {i} (slot {st['slot'][i]})")
        assert st["stop_reason"][i] == stop, (i, st["stop_reason"][i], stop)
        full = m.codec_decode(np.ascontiguousarray(m.queue_codes(i)))
        assert audio[i].shape == full.shape, i
        d = float(np.abs(audio[i] - full).max())
        assert d < 1e-5, (i, d)
        audio_close(audio[i], wav, f"utterance {i} audio")


# ---------------------------------------------------------------- 1. EOS lengths, 10 on 3
@pytest.mark.parametrize("compact", [None, "0"], ids=["compact", "nocompact"])
def test_ten_eos_utterances_on_three_slots(tiny_eos, monkeypatch, compact):
    m, o = tiny_eos
    prompts = _tiny_prompts()
    monkeypatch.delenv("QTTS_QUEUE_COMPACT", raising=False)
    if compact is not None:
        monkeypatch.setenv("QTTS_QUEUE_COMPACT", compact)
    qcodes, qst = _plain_queue(m, ("eos", compact), prompts, 3, 32, 0, 7)
    m.set_params(max_tokens=32, fixed=0, seed=7, **DEFAULT)
    rc, audio, events = _streamed(m, prompts, 3)
    assert rc == 0
    st = m.queue_stats()
    assert st["slots"] == 3 and st["refills"] == 7, st
    for k in STATS_OF_THE_INPUTS:
        assert st[k] == qst[k], (k, st, qst)
    print(f"measured  frames launched: streamed {st['frames']} (rows {st['rows_launched']}), "
          f"plain {qst['frames']} (rows {qst['rows_launched']})")
    assert set(st["stop_reason"]) == {1, 2}, st
    assert (st["rows_launched"] < 3 * st["frames"]) == (compact is None), st
    for i in range(10):
        np.testing.assert_array_equal(m.queue_codes(i), qcodes[i])
    _tiny_check(m, o, prompts, audio, range(10), 32, 0, 7)
    _discipline(m, audio, events, list(range(10)))
    assert m.c.perf_first_packet_ms > 0 and m.c.perf_codec_ms > 0


# ---------------------------------------------------------------- 2. fixed length: every slot refilled on the same frame
def test_fixed_length_refills_on_the_same_frame(tiny_eos):
    m, o = tiny_eos
    prompts = _tiny_prompts()[:7]
    qcodes, qst = _plain_queue(m, ("fixed",), prompts, 3, 4096, 8, 42)
    m.set_params(max_tokens=4096, fixed=8, seed=42, **DEFAULT)
    rc, audio, events = _streamed(m, prompts, 3)
    assert rc == 0
    st = m.queue_stats()
    assert st["frames_per_utt"] == [8] * 7 and st["refills"] == 4, st
    assert st == qst, (st, qst)
    for i in range(7):
        np.testing.assert_array_equal(m.queue_codes(i), qcodes[i])
    _tiny_check(m, o, prompts, audio, range(7), 4096, 8, 42)
    _discipline(m, audio, events, list(range(7)))


# ---------------------------------------------------------------- 3. partial take
def test_partial_take(tiny_eos):
    m, o = tiny_eos
    prompts = _tiny_prompts()[:6]
    m.set_params(max_tokens=32, fixed=0, seed=7, **DEFAULT)
    rc, audio, events = _streamed(m, prompts, 2, order=[1, 3, 5])
    assert rc == 0
    for i in (0, 2, 4):
        assert audio[i] is None and m.queue_codes(i) is None
    _tiny_check(m, o, prompts, audio, [1, 3, 5], 32, 0, 7)
    _discipline(m, audio, events, [1, 3, 5])


# ---------------------------------------------------------------- 4. arming
def test_per_utterance_sampling_and_forcing(tiny_eos):
    m, o = tiny_eos
    prompts = _tiny_prompts()[:6]
    per = [dict(seed=100 + i, temperature=0.8 + 0.03 * i, top_k=40 + i) for i in range(6)]
    m.set_params(max_tokens=24, fixed=0, seed=7, **DEFAULT)
    m.set_utterance_sampling(per)
    rc, _ = m.generate_queue(prompts, ["aiden"] * 6, ["english"] * 6, slots=2)
    assert rc == 0
    want = [m.queue_codes(i) for i in range(6)]
    m.set_utterance_sampling(per)
    rc, audio, events = _streamed(m, prompts, 2)
    assert rc == 0 and not m.c.sampling
    for i in range(6):
        np.testing.assert_array_equal(m.queue_codes(i), want[i])
    _discipline(m, audio, events, list(range(6)))
    # the armed run differs from the plain one somewhere (the arming was used)
    plain, _ = _plain_queue(m, ("plain6",), prompts, 2, 24, 0, 7)
    assert any(not np.array_equal(a, b) for a, b in zip(plain, want))
    # forcing is not defined for the queue: refused and disarmed
    m.set_params(max_tokens=24, fixed=0, seed=7, **DEFAULT)
    m.force_codes(np.zeros((1, 16), np.int32), slot=0)
    got = []
    rc, audio = m.generate_queue_stream(prompts[:2], ["aiden"] * 2, ["english"] * 2, slots=2,
                                        on_chunk=lambda u, a: got.append(u))
    assert rc == -1 and all(a is None for a in audio) and not got and not m.c.force
    rc, audio, events = _streamed(m, prompts, 2)
    assert rc == 0
    for i in range(6):
        np.testing.assert_array_equal(m.queue_codes(i), plain[i])


# ---------------------------------------------------------------- 5. the other streaming calls on the same ctx
def test_same_ctx_streams_afterwards(tiny_eos):
    m, o = tiny_eos
    prompts = _tiny_prompts()[:5]
    m.set_params(max_tokens=32, fixed=0, seed=7, **DEFAULT)
    rc, _, _ = _streamed(m, prompts, 2)
    assert rc == 0
    m.set_params(max_tokens=4096, fixed=8, seed=42, **DEFAULT)
    chunks = []
    a = m.generate_stream(prompts[0], "aiden", "english", chunk_frames=4, on_chunk=chunks.append)
    assert a is not None and len(chunks) >= 2
    np.testing.assert_array_equal(np.concatenate(chunks), a)
    full = m.codec_decode(np.ascontiguousarray(m.last_codes()))
    assert a.shape == full.shape and np.abs(a - full).max() < 1e-5
    per = {}
    rc, audio = m.generate_batch_stream(prompts[:3], ["aiden"] * 3, ["english"] * 3, chunk_frames=4,
                                        on_chunk=lambda i, x: per.setdefault(i, []).append(x))
    assert rc == 0
    codes = m.last_codes_batch(3, 8)
    for b in range(3):
        np.testing.assert_array_equal(np.concatenate(per[b]), audio[b])
        full = m.codec_decode(np.ascontiguousarray(codes[b]))
        assert audio[b].shape == full.shape and np.abs(audio[b] - full).max() < 1e-5, b
    # and the queue streams again after them
    m.set_params(max_tokens=32, fixed=0, seed=7, **DEFAULT)
    rc, audio, events = _streamed(m, prompts, 2)
    assert rc == 0
    _discipline(m, audio, events, list(range(5)))


# ---------------------------------------------------------------- 6. full size: positions far past the window
def test_eos17_two_slots_streamed_vs_reference(gpu):
    """The reference's three full-size EOS utterances (stops 157 / 395 / 218)
    on 2 slots, streamed: the third starts at position 0 in the slot the first
    frees while the second is at position 157 and continues to 395."""
    g = np.load(os.path.join(GOLDEN, "long_eos17.npz"))
    man = json.load(open(os.path.join(GOLDEN, "long_manifest.json")))["eos17"]
    m = qtts.QwenTTS(model_dir("1.7b", eos_gain=man["eos_gain"]))
    try:
        m.set_params(max_tokens=4096, fixed=0, seed=man["seed"], **DEFAULT)
        prompts = [g["prompt_ids"][b, :int(g["prompt_len"][b])] for b in range(3)]
        sizes = {}
        rc, audio = m.generate_queue_stream(prompts, man["speakers"], [man["language"]] * 3, slots=2, chunk_frames=4,
                                            on_chunk=lambda u, a: sizes.setdefault(u, []).append(len(a)))
        assert rc == 0
        st = m.queue_stats()
        assert st["refills"] == 1 and st["slot"][2] == 0, st
        for i in range(3):
            n = int(g["stop_step"][i])
            assert st["stop_reason"][i] == 1 and st["frames_per_utt"][i] == n, (i, st)
            codes_equal(m.queue_codes(i), g["codes"][i, :n], f"eos17 streamed: utterance {i}")
            a = audio[i]
            assert a is not None and len(a) == n * SPF, i
            assert sizes[i][0] == SPF and sum(sizes[i]) == n * SPF, (i, sizes[i][:4])
            sub = a[::man["audio_stride"]]
            d = sub.astype(np.float64) - g["audio_sub"][i, :len(sub)]
            mse, mx = float(np.mean(d * d)), float(np.abs(d).max())
            assert mse < 1e-4 and mx < 1e-3, (i, mse, mx)      # test_gpu_queue.py's bar for this fixture
    finally:
        m.close()
