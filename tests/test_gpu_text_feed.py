"""Incremental text input (qwen_tts_generate_fed_stream / _fed_batch_stream,
qtts_dev_text_append): for the same content ids every feed schedule gives the
same codes bit for bit, in any slot, whatever the other slots are fed.

The row rule (DESIGN.md "Incremental text input"): with content ids c[0..m)
trailing row r is proj(c[r + 1]) for r < m - 1 and row m - 1 is tts_eos; the
frame that draws frame r adds row r to the talker input of frame r + 1, so
frame f needs row f published (or the text closed) and row r first reaches the
codes of frame r + 1.

Bounds are the project's: 1e-5 max-abs between two chunkings of the same codes
(test_gpu_batch_stream.py); the GEMV float64 bar of test_gpu_kernels.py
(gemv_bound: 2e-6 * sum|a x| + 1e-6 per contraction) for the appended rows.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import manifest, model_dir
from oracle_py import DEFAULT
from qtts_io import read_model_tensors
from synth_model import prompt_ids
from test_gpu_kernels import bf16_f64, gemv_bound

import qtts

pytestmark = pytest.mark.gpu

SPK, LANG = "aiden", "english"
SHORT, P128, P128B = prompt_ids("short"), prompt_ids("p128", 1300), prompt_ids("p128", 1301)


def content(ids):
    """the content ids of a chat-template prompt: between the 3 role ids and the 5 closing ids"""
    return list(ids[3:-5])


class Log:
    """audio chunks per utterance and the order of chunks and wait = 1 calls"""

    def __init__(self, nb=1):
        self.per = [[] for _ in range(nb)]
        self.events = []      # ("chunk", i, samples) | ("wait", [frames_done per utterance])

    def chunk(self, i, pcm):
        self.per[i].append(pcm)
        self.events.append(("chunk", i, len(pcm)))


def feed_all(ids_per):
    """schedule A: everything and the close at the first callback"""
    sent = [False] * len(ids_per)

    def feed(h, wait):
        for u, ids in enumerate(ids_per):
            if not sent[u]:
                assert h.push(u, ids) == 0 and h.close(u) == 0
                sent[u] = True
    return feed


def run_one(m, feed, log=None, chunk=4, frames=16):
    log = log or Log()
    audio = m.generate_fed_stream(feed, SPK, LANG, chunk_frames=chunk, on_chunk=lambda a: log.chunk(0, a))
    assert audio is not None
    return m.last_codes_slot(0, frames), audio, log


def check_audio(audio, log, i, ref=None):
    assert all(len(c) > 0 and len(c) % 1920 == 0 for c in log.per[i])
    np.testing.assert_array_equal(np.concatenate(log.per[i]), audio)
    if ref is not None:
        assert audio.shape == ref.shape
        d = float(np.abs(audio - ref).max())
        print(f"measured  largest |audio - schedule A's| {d:.3e}")
        assert d < 1e-5, d


# ---------------------------------------------------------------- 1. schedules, one utterance
def test_schedules_one_utterance(tts_tiny):
    m = tts_tiny
    ids = content(P128)
    assert len(ids) == 30
    m.set_params(max_tokens=4096, fixed=16, seed=42, **DEFAULT)
    codes_a, audio_a, log_a = run_one(m, feed_all([ids]))
    assert codes_a.shape[0] == 16
    check_audio(audio_a, log_a, 0)

    pos = [0]

    def feed_b(h, wait):   # one id per callback
        if pos[0] < len(ids):
            assert h.push(0, ids[pos[0]:pos[0] + 1]) == 0
            pos[0] += 1
            if pos[0] == len(ids):
                assert h.close(0) == 0
    codes_b, audio_b, log_b = run_one(m, feed_b)
    np.testing.assert_array_equal(codes_b, codes_a)
    check_audio(audio_b, log_b, 0, audio_a)

    # C: two ids, nothing on wait = 0, three more at every wait = 1
    log_c = Log()
    st = dict(pos=0, waits=0)

    def feed_c(h, wait):
        if not wait:
            return
        if st["pos"]:
            st["waits"] += 1
            log_c.events.append(("wait", [h.state(0)[1]]))
            assert h.state(0)[2], "wait = 1 with an utterance that is not starved"
        n = 2 if st["pos"] == 0 else 3
        assert h.push(0, ids[st["pos"]:st["pos"] + n]) == 0
        st["pos"] = min(st["pos"] + n, len(ids))
        if st["pos"] == len(ids):
            assert h.close(0) == 0
    codes_c, audio_c, _ = run_one(m, feed_c, log_c)
    assert st["waits"] >= 2, st          # (precondition: the run did starve)
    np.testing.assert_array_equal(codes_c, codes_a)
    check_audio(audio_c, log_c, 0, audio_a)
    # every frame decoded before a wait = 1 call was delivered before that call
    seen = 0
    for ev in log_c.events:
        if ev[0] == "chunk":
            seen += ev[2]
        else:
            assert seen == ev[1][0] * 1920, (seen, ev)


# ---------------------------------------------------------------- 2. late close
def test_late_close_starves_at_the_eos_row(tts_tiny):
    m = tts_tiny
    ids = content(SHORT)
    assert len(ids) == 7
    m.set_params(max_tokens=4096, fixed=16, seed=42, **DEFAULT)
    codes_a, audio_a, _ = run_one(m, feed_all([ids]))
    seen = []
    st = dict(pushed=False)

    def feed(h, wait):
        if not st["pushed"]:
            assert h.push(0, ids) == 0
            st["pushed"] = True
        elif wait:
            seen.append(h.state(0))
            assert h.close(0) == 0
    codes, audio, log = run_one(m, feed)
    # 7 ids are 6 rows: frames 0..5 run, frame 6 needs the eos row
    assert seen == [(7, 6, True)], seen
    np.testing.assert_array_equal(codes, codes_a)
    check_audio(audio, log, 0, audio_a)


# ---------------------------------------------------------------- 3. the layout
@pytest.mark.parametrize("name", ["short", "p128"])
def test_layout_equals_the_unfed_call(tts_tiny, name):
    """Fed and unfed runs share the layout, not the arithmetic: the unfed text
    rows go through rows_proj (k_gemv / k_gemvb / k_mgemm by row count, 7 + n
    rows at once), the fed ones through k_tf_proj, and the fed prefill projects
    7 rows where the unfed one projects all.  Equal codes are a property of
    these inputs at seed 42 (no near-tie met; none had to be replaced)."""
    m = tts_tiny
    tpl = SHORT if name == "short" else P128
    m.set_params(max_tokens=4096, fixed=16, seed=42, **DEFAULT)
    rc, _ = m.generate_batch_stream([tpl], [SPK], [LANG], chunk_frames=4)
    assert rc == 0
    want = m.last_codes_slot(0, 16)
    codes, _, _ = run_one(m, feed_all([content(tpl)]))
    np.testing.assert_array_equal(codes, want)


def test_layout_negative_control(tts_tiny):
    """content id j is trailing row j - 1, added by the frame that draws frame
    j - 1 to the talker input of frame j: frames [0, j) cannot see it, frame j
    is the first that can."""
    m = tts_tiny
    ids = content(P128)
    j = 5
    m.set_params(max_tokens=4096, fixed=16, seed=42, **DEFAULT)
    codes_a, _, _ = run_one(m, feed_all([ids]))
    other = list(ids)
    other[j] = ids[j] + 1 if ids[j] + 1 != ids[j - 1] else ids[j] + 2
    codes_x, _, _ = run_one(m, feed_all([other]))
    np.testing.assert_array_equal(codes_x[:j], codes_a[:j])
    assert not np.array_equal(codes_x[j:], codes_a[j:])


# ---------------------------------------------------------------- 4. batch of 3
def single_runs(m, contents, frames, samplings=None):
    out = []
    for u, ids in enumerate(contents):
        if samplings:
            m.set_utterance_sampling([samplings[u]])
        out.append(run_one(m, feed_all([ids]), frames=frames)[:2])
    return out


def test_batch_of_three_own_schedules(tts_tiny):
    m = tts_tiny
    contents = [content(SHORT), content(P128), content(P128B)]
    m.set_params(max_tokens=4096, fixed=12, seed=42, **DEFAULT)
    alone = single_runs(m, contents, 12)
    log = Log(3)
    st = dict(p2=0, s0=False, s1=0, starved_seen=[])

    def feed(h, wait):
        if not st["s0"]:                      # slot 0: everything at once
            assert h.push(0, contents[0]) == 0 and h.close(0) == 0
            st["s0"] = True
        if st["p2"] < len(contents[2]):       # slot 2: one id per callback
            assert h.push(2, contents[2][st["p2"]:st["p2"] + 1]) == 0
            st["p2"] += 1
            if st["p2"] == len(contents[2]):
                assert h.close(2) == 0
        f0 = h.state(0)[1]
        if st["s1"] == 0:                     # slot 1: two ids, the rest once slot 0 has 6 frames
            assert h.push(1, contents[1][:2]) == 0
            st["s1"] = 1
        elif st["s1"] == 1 and f0 >= 6:
            assert h.push(1, contents[1][2:]) == 0 and h.close(1) == 0
            st["s1"] = 2
        elif st["s1"] == 1:
            st["starved_seen"].append((f0, h.state(1)))
    held0 = m.text_held_frames()
    rc, audio = m.generate_fed_batch_stream(3, feed, [SPK] * 3, [LANG] * 3, chunk_frames=4, on_chunk=log.chunk)
    assert rc == 0
    # precondition: slot 1 sat starved at one frame while slot 0 advanced over >= 3 launches
    held = m.text_held_frames() - held0
    print(f"measured  held frames {held}")
    assert held >= 3, held
    stuck = [(f0, s) for f0, s in st["starved_seen"] if s[2]]
    assert len({f0 for f0, _ in stuck}) >= 3 and len({s[1] for _, s in stuck}) == 1, st["starved_seen"]
    for b in range(3):
        np.testing.assert_array_equal(m.last_codes_slot(b, 12), alone[b][0])
        check_audio(audio[b], log, b, alone[b][1])


# ---------------------------------------------------------------- 5. EOS mode
# default sampling of the tiny EOS model on the "short" prompt, by the CPU oracle
# (test_gpu_batch_stream.py): seed 2 -> 19 eos, 9 -> 23 eos, 7 -> 16 eos, 1 -> 32 max_tokens
EOS_SEEDS = [2, 9, 7, 1]


def test_eos_mode_starved_across_a_stop():
    md = model_dir("tiny", eos_gain=manifest()["eos_gain"])
    m = qtts.QwenTTS(md)
    try:
        ids = content(SHORT)
        m.set_params(max_tokens=32, fixed=0, seed=42, **DEFAULT)
        alone = single_runs(m, [ids] * 4, 32, [dict(seed=s) for s in EOS_SEEDS])
        frames = [len(c) for c, _ in alone]
        assert frames[2] < frames[0] < 32 and frames[3] == 32, frames   # (the oracle's stops)
        log = Log(4)
        st = dict(start=False, released=False, late=[], stuck=[])

        def feed(h, wait):
            if not st["start"]:
                for u in range(3):
                    assert h.push(u, ids) == 0 and h.close(u) == 0
                assert h.push(3, ids) == 0          # slot 3: the close withheld -> starved at the eos row
                st["start"] = True
                return
            f0 = h.state(0)[1]
            if not st["released"]:
                st["stuck"].append((f0, h.state(3)))
                if f0 >= frames[2] + 2 or wait:     # slot 2's EOS is behind us
                    assert h.close(3) == 0
                    st["released"] = True
            elif h.state(3)[1] >= 30 and not st["late"]:
                # slots 0..2 stopped long ago (polled since): pushes and closes do nothing
                st["late"] = [h.push(2, ids[:1]), h.close(2), h.push(0, ids[:2])]
        m.set_utterance_sampling([dict(seed=s) for s in EOS_SEEDS])
        rc, audio = m.generate_fed_batch_stream(4, feed, [SPK] * 4, [LANG] * 4, chunk_frames=4, on_chunk=log.chunk)
        assert rc == 0
        assert st["late"] == [0, 0, 0], st["late"]
        # slot 3 sat at frame 6 (7 ids: 6 rows) while slot 0 passed slot 2's stop
        assert any(s == (7, 6, True) and f0 > frames[2] for f0, s in st["stuck"]), st["stuck"]
        for b in range(4):
            np.testing.assert_array_equal(m.last_codes_slot(b, 32), alone[b][0])
            check_audio(audio[b], log, b, alone[b][1])
            sizes = [len(c) for c in log.per[b]]
            assert np.cumsum(sizes).tolist().index(frames[b] * 1920) == len(sizes) - 1   # no callback after its last frame
    finally:
        m.close()


# ---------------------------------------------------------------- 6. 17 slots: the wide kernel
def test_seventeen_slots_hold(tts_tiny):
    m = tts_tiny
    short, long_ = content(SHORT), content(P128)
    m.set_params(max_tokens=4096, fixed=6, seed=42, **DEFAULT)
    alone = single_runs(m, [short, long_], 6)
    st = dict(start=False, rest=False)

    def feed(h, wait):
        if not st["start"]:
            for u in range(16):
                assert h.push(u, short) == 0 and h.close(u) == 0
            assert h.push(16, long_[:2]) == 0
            st["start"] = True
        elif not st["rest"] and (h.state(0)[1] >= 3 or wait):
            assert h.push(16, long_[2:]) == 0 and h.close(16) == 0
            st["rest"] = True
    wide0, held0 = qtts.lib().qtts_hip_gemv_wide_launches(), m.text_held_frames()
    rc, audio = m.generate_fed_batch_stream(17, feed, [SPK] * 17, [LANG] * 17, chunk_frames=4)
    assert rc == 0
    assert qtts.lib().qtts_hip_gemv_wide_launches() > wide0
    assert m.text_held_frames() - held0 == 2      # slot 16 ran frame 0, then waited for frames 1 and 2 of slot 0
    np.testing.assert_array_equal(m.last_codes_slot(0, 6), alone[0][0])
    np.testing.assert_array_equal(m.last_codes_slot(16, 6), alone[1][0])
    assert np.abs(audio[16] - alone[1][1]).max() < 1e-5


# ---------------------------------------------------------------- 7. armings
def test_armings(tts_tiny):
    m = tts_tiny
    contents = [content(SHORT), content(P128)]
    per = [dict(seed=7, temperature=0.7, top_k=20), dict(seed=11, top_p=0.8)]
    m.set_params(max_tokens=4096, fixed=10, seed=42, **DEFAULT)
    alone = single_runs(m, contents, 10, per)
    m.set_utterance_sampling(per)
    rc, _ = m.generate_fed_batch_stream(2, feed_all(contents), [SPK] * 2, [LANG] * 2, chunk_frames=4)
    assert rc == 0
    for b in range(2):
        np.testing.assert_array_equal(m.last_codes_slot(b, 10), alone[b][0])
    assert not np.array_equal(alone[0][0], run_one(m, feed_all([contents[0]]), frames=10)[0])   # (the rows were used)
    # one instruct: the fed run equals the unfed armed call
    ins = [151644, 872, 198, 501, 502, 503, 151645, 198]
    m.set_utterance_instruct([ins])
    rc, _ = m.generate_batch_stream([SHORT], [SPK], [LANG], chunk_frames=4)
    assert rc == 0
    want = m.last_codes_slot(0, 10)
    m.set_utterance_instruct([ins])
    got = run_one(m, feed_all([contents[0]]), frames=10)[0]
    np.testing.assert_array_equal(got, want)
    assert not np.array_equal(got, run_one(m, feed_all([contents[0]]), frames=10)[0])
    # forcing is refused and disarmed: the next call runs free
    plain = run_one(m, feed_all([contents[0]]), frames=10)[0]
    m.force_codes(np.zeros((2, 16), np.int32))
    called = []
    assert m.generate_fed_stream(lambda h, w: called.append(w)) is None
    assert not called
    np.testing.assert_array_equal(run_one(m, feed_all([contents[0]]), frames=10)[0], plain)


# ---------------------------------------------------------------- 8. abort
def test_abort_leaves_the_context_clean(tts_tiny):
    m = tts_tiny
    m.set_params(max_tokens=4096, fixed=16, seed=42, **DEFAULT)
    before = m.generate(SHORT, SPK, LANG)
    codes_before = m.last_codes()
    ids = content(P128)
    aborted = []

    def aborting():
        st = dict(sent=False)

        def feed(h, wait):
            if not st["sent"]:
                assert h.push(0, ids) == 0 and h.close(0) == 0
                st["sent"] = True
            if h.state(0)[1] >= 5:
                aborted.append(h.state(0)[1])
                return -1
        return feed
    assert m.generate_fed_stream(aborting(), SPK, LANG, chunk_frames=4) is None
    rc, audio = m.generate_fed_batch_stream(1, aborting(), [SPK], [LANG])
    assert rc == -1 and audio == [None]
    assert aborted == [5, 5], aborted
    after = m.generate(SHORT, SPK, LANG)
    np.testing.assert_array_equal(m.last_codes(), codes_before)
    np.testing.assert_array_equal(after, before)


# ---------------------------------------------------------------- 9. the append, kernel level
class GenParams(C.Structure):   # qtts_gen_params_t
    _fields_ = [("temperature", C.c_float), ("top_p", C.c_float), ("repetition_penalty", C.c_float),
                ("top_k", C.c_int), ("st_temperature", C.c_float), ("st_top_p", C.c_float), ("st_top_k", C.c_int),
                ("fixed_codec_tokens", C.c_int), ("seed", C.c_int)]


PAD, EOS_T = 151671, 151673   # tts_pad / tts_eos text ids (include/qwen_tts.h)


def test_append_kernel_level(tts_tiny, tiny_dir):
    m = tts_tiny
    lib, dev = qtts.lib(), C.c_void_p(m.c.hip)
    ids = content(P128)
    H = m.cfg.talker_hidden
    ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
    gp = GenParams(0.9, 1.0, 1.05, 50, 0.9, 1.0, 50, 4, 42)
    assert lib.qtts_dev_begin(dev, 3, 4, 16, C.byref(gp)) == 0
    # a one-row prompt per slot: prefill row 0 = proj(first id), the tts_eos row alone behind it
    text = [PAD, EOS_T, ids[0]]
    for b in range(3):
        plan = [2, -1, 0, b, 0, 1, -1, 1, b, 0]
        assert lib.qtts_dev_prompt(dev, b, (C.c_int * 3)(*text), 3, (C.c_int * 10)(*plan), 2, 1, 1, 0) == 0
        assert lib.qtts_dev_text_open(dev, b) == 0
    eos_row = np.zeros(H, np.float32)

    def append(b, chunk, close=0):
        a = np.ascontiguousarray(chunk, np.int32)
        return lib.qtts_dev_text_append(dev, b, a.ctypes.data_as(ip), len(chunk), close)

    def state(b):
        r, o, h = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        assert lib.qtts_dev_text_state(dev, b, C.byref(r), C.byref(o), C.byref(h)) == 0
        return r.value, o.value

    def rows(b, n):
        out = np.zeros((n, H), np.float32)
        assert lib.qtts_dev_get_trailing(dev, b, 0, n, out.ctypes.data_as(fp)) == 0
        return out
    # the row after the last is marked first, so "untouched" can be seen (row 31 of slot 0: past 30 ids + eos)
    n = len(ids)
    before = rows(0, n + 2)
    assert state(0) == (0, 1)
    at = 0
    for g in (1, 2, 5, 16, 6):
        assert append(0, ids[at:at + g]) == 0
        at += g
        assert state(0) == (at, 1)             # the count is published, the text still open
    assert at == n
    for i in range(n):
        assert append(1, ids[i:i + 1]) == 0
    assert append(2, ids[:16]) == 0 and append(2, ids[16:], close=1) == 0
    assert state(1) == (n, 1) and state(2) == (n + 1, 0)
    got = rows(0, n + 2)
    np.testing.assert_array_equal(got[:n], rows(1, n))
    np.testing.assert_array_equal(got[:n], rows(2, n))
    np.testing.assert_array_equal(got[n:], before[n:])     # rows n and n + 1 of slot 0: untouched
    # the refusals
    assert append(2, ids[:1]) == -1                          # closed
    assert append(0, [1 << 30]) == -1                        # past any text vocabulary
    assert append(0, [-1]) == -1
    assert state(0) == (n, 1)
    # float64 reference from the model's tensors, stage by stage under the GEMV bar
    t = read_model_tensors(tiny_dir)
    emb = t["talker.model.text_embedding.weight"][1]
    w1, b1 = t["talker.text_projection.linear_fc1.weight"][1], t["talker.text_projection.linear_fc1.bias"][1]
    w2, b2 = t["talker.text_projection.linear_fc2.weight"][1], t["talker.text_projection.linear_fc2.bias"][1]

    def f64(x):
        return bf16_f64(np.asarray(x)) if np.asarray(x).dtype == np.uint16 else np.asarray(x, np.float64)
    e = f64(emb[np.asarray(ids)])
    z = e @ f64(w1).T + f64(b1)
    h1 = z / (1.0 + np.exp(-z))
    ref = h1 @ f64(w2).T + f64(b2)
    W1 = np.asarray(w1) if np.asarray(w1).dtype == np.uint16 else None
    W2 = np.asarray(w2) if np.asarray(w2).dtype == np.uint16 else None
    assert W1 is not None and W2 is not None, "the synthetic model stores the projection in bf16"
    # stage 1 within gemv_bound (+ 2e-7 relative for bias / SiLU, xgemm_ref's epilogue figure; |SiLU'| <= 1.1),
    # carried through |W2|, plus stage 2's own bound
    b_1 = 1.1 * (gemv_bound(W1, e.astype(np.float32)) + 2e-7 * np.abs(z)) + 2e-7 * np.abs(h1)
    bound = gemv_bound(W2, h1.astype(np.float32)) + b_1 @ np.abs(f64(w2)).T + 2e-7 * np.abs(ref)
    err = np.abs(got[:n].astype(np.float64) - ref)
    print(f"measured  largest err / bound {float((err / bound).max()):.3f}")
    assert np.all(err <= bound), float((err / bound).max())
    # the eos row of a close is the prompt's own tts_eos row
    np.testing.assert_array_equal(rows(2, n + 1)[n], before[0])
    # growth past the 64 allocated rows (the one append that waits): what was there is kept, what
    # follows lands behind it -- a row depends on its id alone
    assert append(1, ids + ids[:10]) == 0 and state(1) == (2 * n + 10, 1)
    grown = rows(1, 2 * n + 10)
    np.testing.assert_array_equal(grown[:n], got[:n])
    np.testing.assert_array_equal(grown[n:2 * n], got[:n])
    np.testing.assert_array_equal(grown[2 * n:], got[:10])
    np.testing.assert_array_equal(rows(0, n), got[:n])       # (and the other slots moved with the block)


# ---------------------------------------------------------------- the CLI
def test_cli_stdin_ids(tts_tiny, tiny_dir):
    """qwen-tts --stdin-ids: content ids from stdin (commas, blanks and newlines), EOF closes;
    the wav is the API's for the same ids"""
    ids = content(SHORT)
    text = f"{ids[0]},{ids[1]} {ids[2]}\n" + ", ".join(map(str, ids[3:]))    # (no newline at the end: EOF ends the number)
    with tempfile.TemporaryDirectory() as d:
        cmd = [qtts.CLI_PATH, "-d", tiny_dir, "--stdin-ids", "-s", SPK, "-l", LANG, "-o", os.path.join(d, "cli.wav"),
               "--fixed-codec-tokens", "8", "--seed", "42", "--stream", "4"]
        r = subprocess.run(cmd, input=text, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        tts_tiny.set_params(max_tokens=4096, fixed=8, seed=42)
        a = run_one(tts_tiny, feed_all([ids]), frames=8)[1]
        api = os.path.join(d, "api.wav")
        assert qtts.lib().qwen_tts_write_wav(api.encode(), a.ctypes.data_as(qtts._fp), len(a), 24000) == 0
        assert open(os.path.join(d, "cli.wav"), "rb").read() == open(api, "rb").read()
        r = subprocess.run(cmd + ["-t", "1,2,3"], input=text, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--stdin-ids takes the content ids from stdin" in r.stderr
