"""Teacher-forced decode on the GPU: forced codes, the free-draw record and
logit taps (include/qwen_tts.h qwen_tts_force_codes / _tap_draw / _last_drawn
/ _tap_result), against the model's own free runs and against the reference's
recorded runs (tests/golden/e2e_tiny.npz, long_hd128*.npz) and the oracle's
sampler trace (Oracle.trace_draw).

Unless noted: the `tiny` model, 16 fixed frames, the prompt of e2e_tiny.npz.
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden, model_dir
from oracle_py import DEFAULT, GREEDY, Oracle
from qtts_io import lookup_ids
from synth_model import prompt_ids

import qtts

pytestmark = pytest.mark.gpu
E = golden("e2e_tiny.npz")
IDS = prompt_ids("short")
SPK, LANG = "aiden", "english"
G = 16
FULL = dict(DEFAULT, top_p=0.9, st_top_p=0.9)   # top_p < 1: the sampler's full (softmax + nucleus) path


def _audio_close(a, ref, what, mse_bar=1e-4, max_bar=1e-3):
    """the waveform bar of tests/test_gpu_long.py"""
    assert a is not None and a.shape == ref.shape, (what, None if a is None else a.shape, ref.shape)
    d = a.astype(np.float64) - ref
    mse, mx = float(np.mean(d * d)), float(np.abs(d).max())
    assert mse < mse_bar and mx < max_bar, (what, mse, mx)


def _run(m, pp=DEFAULT, seed=42, fixed=16, max_tokens=4096, forced=None, taps=(), slot=0):
    m.set_params(max_tokens=max_tokens, fixed=fixed, seed=seed, **pp)
    if forced is not None:
        m.force_codes(forced, slot)
    for f, g in taps:
        m.tap_draw(f, g, slot)
    a = m.generate(IDS, SPK, LANG)
    return a, (m.last_codes() if a is not None else None)


@pytest.fixture(scope="module")
def tiny(gpu, tiny_dir):
    m = qtts.QwenTTS(tiny_dir)
    yield m
    m.close()


@pytest.fixture(scope="module")
def free_default(tiny):
    """the free run every test compares with (== the reference's seed-42 run), computed once"""
    a, c = _run(tiny)
    np.testing.assert_array_equal(c, E["sampled_codes"])
    a.setflags(write=False)
    c.setflags(write=False)
    return a, c


@pytest.fixture(scope="module")
def traces(oracle):
    """Oracle.trace_draw of the reference's seed-42 utterance at the tapped draws"""
    s, l = lookup_ids(oracle.cfg, SPK, LANG)
    par = dict(max_tokens=4096, fixed=16, seed=42, **DEFAULT)
    return {fg: oracle.trace_draw(IDS, s, l, fg[0], fg[1], **par) for fg in TAPS}


TAPS = [(15, 0), (9, 1), (12, 7)]


# 1. identity ---------------------------------------------------------------
@pytest.mark.parametrize("pp,env", [(DEFAULT, {}), (DEFAULT, {"QTTS_HIP_SAMPLE_W": "0"}), (GREEDY, {}), (FULL, {})],
                         ids=["default", "sample_w0", "greedy", "top_p0.9"])
def test_forcing_own_codes_is_identity(tiny, monkeypatch, pp, env):
    """Forcing the model's own free-run codes changes nothing: codes, audio
    and the free continuation (frames 8-15 after forcing 0-7, which needs every
    RNG advance of the forced frames) are bit-identical to the free run, and
    the free-draw record equals the codes.  The four settings launch the forced
    form of every sampler family: 1024-thread fast path (default, greedy), the
    256-thread fast path (QTTS_HIP_SAMPLE_W=0) and the full path (top_p 0.9)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    a0, c0 = _run(tiny, pp)
    assert tiny.last_drawn() is None   # (an unarmed run keeps no record)
    a1, c1 = _run(tiny, pp, forced=c0)
    np.testing.assert_array_equal(c1, c0)
    np.testing.assert_array_equal(a1, a0)
    np.testing.assert_array_equal(tiny.last_drawn(), c0)
    a2, c2 = _run(tiny, pp, forced=c0[:8])
    np.testing.assert_array_equal(c2, c0)
    np.testing.assert_array_equal(a2, a0)
    np.testing.assert_array_equal(tiny.last_drawn(), c0)


# 2. steering against the reference ----------------------------------------
def _tap_checks(m, traces):
    """per tap: do its values meet the stage bar allclose(1e-4, 1e-4) against the oracle's trace"""
    out = []
    for i, fg in enumerate(TAPS):
        lg, bits, drawn = m.tap_result(i)
        tr = traces[fg]
        assert lg.shape == tr["logits"].shape, (fg, lg.shape)
        out.append(bool(np.allclose(lg, tr["logits"], rtol=1e-4, atol=1e-4)))
        print(f"tap {fg}: max |gpu - oracle| {np.abs(lg - tr['logits']).max():.3g}, drawn {drawn}, "
              f"oracle {tr['result']}")
    return out


def test_steering_on_reference_codes(tiny, free_default, traces, oracle):
    """Seed 43 forced onto the reference's seed-42 codes: the stored codes are
    the forced ones, the audio is the reference's, and the sampler's inputs at
    three draws are the oracle's for the seed-42 utterance at the stage bar --
    the history is the reference's although no draw of this run chose it."""
    ref = E["sampled_codes"]
    a, c = _run(tiny, seed=43, forced=ref, taps=TAPS)
    np.testing.assert_array_equal(c, ref)
    _audio_close(a, E["sampled_audio"], "steered audio vs the reference's")
    assert not np.array_equal(tiny.last_drawn(), ref)   # (seed 43 draws its own ids)
    assert _tap_checks(tiny, traces) == [True, True, True]
    V, eos = tiny.cfg.talker_vocab_size, tiny.cfg.codec_eos_id
    lg0, bits0, _ = tiny.tap_result(0)
    sup = np.array([i for i in range(V - 1024, V) if i != eos])
    assert lg0.shape == (V,) and np.all(lg0[sup] == np.float32(-1e9))
    assert np.isfinite(lg0).all() and lg0[eos] != np.float32(-1e9)
    for i, fg in enumerate(TAPS):
        assert tiny.tap_result(i)[1] != traces[fg]["rng_bits"], fg   # another seed, another RNG state
    # control: the same comparison fails once the history differs from the
    # reference's -- one forced code changed in the frame before the (15, 0)
    # draw and one in the group before the (9, 1) draw
    bad = ref.copy()
    bad[14, 15] = (bad[14, 15] + 1) % 2048
    bad[9, 0] = (bad[9, 0] + 1) % 2048
    _, cb = _run(tiny, seed=43, forced=bad, taps=TAPS)
    np.testing.assert_array_equal(cb, bad)
    ok = _tap_checks(tiny, traces)
    assert ok[0] is False and ok[1] is False, ok


# 3. RNG contract -----------------------------------------------------------
def test_rng_contract_under_forcing(tiny, free_default, traces):
    """Seed 42 with the reference's codes forced: every draw is the
    reference's (the free-draw record equals its codes at all 256 draws) and
    the RNG state before each tapped draw is the oracle's, bit for bit."""
    ref = E["sampled_codes"]
    a, c = _run(tiny, seed=42, forced=ref, taps=TAPS)
    np.testing.assert_array_equal(c, ref)
    d = tiny.last_drawn()
    assert d.shape == (16, G)
    np.testing.assert_array_equal(d, ref)
    for i, fg in enumerate(TAPS):
        lg, bits, drawn = tiny.tap_result(i)
        assert bits == traces[fg]["rng_bits"], (fg, hex(bits), hex(traces[fg]["rng_bits"]))
        assert drawn == traces[fg]["result"] == ref[fg]


# 4. partial masks ----------------------------------------------------------
def test_partial_masks(tiny, free_default):
    _, free = free_default
    ref = E["sampled_codes"]
    # group 0 of every frame from the reference's run, under another seed
    mask = np.full((16, G), -1, np.int32)
    mask[:, 0] = ref[:, 0]
    _, c = _run(tiny, seed=43, forced=mask)
    d = tiny.last_drawn()
    np.testing.assert_array_equal(c[:, 0], ref[:, 0])
    np.testing.assert_array_equal(d[:, 1:], c[:, 1:])     # free groups: drawn == stored
    assert not np.array_equal(d[:, 0], c[:, 0])
    # one entry: frame 5, group 3
    mask = np.full((6, G), -1, np.int32)
    mask[5, 3] = (free[5, 3] + 7) % 2048
    _, c = _run(tiny, seed=42, forced=mask)
    d = tiny.last_drawn()
    np.testing.assert_array_equal(c[:5], free[:5])
    np.testing.assert_array_equal(c[5, :3], free[5, :3])
    assert c[5, 3] == mask[5, 3] and d[5, 3] == free[5, 3]
    keep = np.ones((16, G), bool)
    keep[5, 3] = False
    np.testing.assert_array_equal(d[keep], c[keep])
    assert not np.array_equal(c[5:], free[5:])            # (the rest of the run follows the replaced id)


# 5. EOS mode ---------------------------------------------------------------
def test_eos_follows_the_forced_id(gpu, tiny_eos_dir):
    """EOS-stop mode on the eos_gain model, the reference's EOS fixtures of
    that model (e2e_tiny.npz eoss_codes: default sampling, seed 7, stops by
    itself): forcing the reference's codes stops where it stopped; a forced EOS
    stops the slot there and leaves the rest of that frame undrawn; a forced
    non-EOS continues where the free draw was EOS."""
    ref = E["eoss_codes"]
    m = qtts.QwenTTS(tiny_eos_dir)
    try:
        eos = m.cfg.codec_eos_id
        kw = dict(pp=DEFAULT, seed=7, fixed=0, max_tokens=32)
        _, c0 = _run(m, **kw)
        np.testing.assert_array_equal(c0, ref)
        stop0 = (m.c.last_stop_reason, m.c.last_stop_step)
        assert stop0[0] == 1 and len(ref) < 32
        # the reference's codes forced: the same stop
        _, c = _run(m, forced=ref, **kw)
        np.testing.assert_array_equal(c, ref)
        assert (m.c.last_stop_reason, m.c.last_stop_step) == stop0
        d = m.last_drawn()
        S = len(ref)                      # the stop frame: its group-0 draw is EOS, nothing else is drawn
        assert d.shape == (S + 1, G) and d[S, 0] == eos and np.all(d[S, 1:] == -1)
        np.testing.assert_array_equal(d[:S], ref)
        # a forced EOS at frame 3
        f = np.full((4, G), -1, np.int32)
        f[3, 0] = eos
        a, c = _run(m, forced=f, **kw)
        assert c.shape == (3, G) and a.shape == (3 * 1920,)
        np.testing.assert_array_equal(c, ref[:3])
        assert (m.c.last_stop_reason, m.c.last_stop_step) == (1, 3)
        d = m.last_drawn()
        assert d.shape == (4, G) and d[3, 0] == ref[3, 0] and np.all(d[3, 1:] == -1)
        # the free draw at frame S is EOS; a forced non-EOS id continues there
        f = np.full((S + 1, G), -1, np.int32)
        f[S, 0] = 5
        _, c = _run(m, forced=f, **kw)
        d = m.last_drawn()
        assert len(c) > S and c[S, 0] == 5 and d[S, 0] == eos
        np.testing.assert_array_equal(c[:S], ref)
        assert np.all(d[S, 1:] >= 0)      # the frame's other groups were drawn
    finally:
        m.close()


# 6. batch ------------------------------------------------------------------
def test_batch_only_the_forced_slot_changes(tiny):
    idl = [IDS, prompt_ids("p128", seed=5), prompt_ids("p128", seed=6)]
    tiny.set_params(max_tokens=4096, fixed=16, seed=42, **DEFAULT)
    rc, a0 = tiny.generate_batch(idl, [SPK] * 3, [LANG] * 3)
    assert rc == 0
    c0 = tiny.last_codes_batch(3, 16)
    # slot 1 forced onto its own codes, altered at the last group of frame 4
    # (every draw of frame 4 still sees the unaltered history)
    f = c0[1].copy()
    f[4, 15] = (f[4, 15] + 1) % 2048
    tiny.force_codes(f, slot=1)
    rc, a1 = tiny.generate_batch(idl, [SPK] * 3, [LANG] * 3)
    assert rc == 0
    c1 = tiny.last_codes_batch(3, 16)
    for b in (0, 2):
        np.testing.assert_array_equal(c1[b], c0[b])
        np.testing.assert_array_equal(a1[b], a0[b])
        np.testing.assert_array_equal(tiny.last_drawn(b), c0[b])   # unforced slots: drawn == stored
    np.testing.assert_array_equal(c1[1], f)
    d = tiny.last_drawn(1)
    np.testing.assert_array_equal(d[:5], c0[1][:5])
    assert not np.array_equal(d[5:], c0[1][5:])
    assert not np.array_equal(a1[1], a0[1])


# 7. one-shot, graphs -------------------------------------------------------
def test_one_shot_and_plain_graphs_return(gpu, tiny_dir, free_default):
    a_free, c_free = free_default
    m = qtts.QwenTTS(tiny_dir)
    try:
        a, c = _run(m)
        np.testing.assert_array_equal(c, c_free)
        bytes0 = m.state_bytes()
        f = c_free.copy()
        f[2, 0] = (f[2, 0] + 1) % 2048
        _, ca = _run(m, forced=f, taps=[(3, 0)])
        np.testing.assert_array_equal(ca, f)
        assert m.state_bytes() > bytes0                 # (the tables exist while armed)
        # nothing armed now: the plain graphs, a plain run
        a, c = _run(m)
        np.testing.assert_array_equal(c, c_free)
        np.testing.assert_array_equal(a, a_free)
        assert m.state_bytes() == bytes0
        assert m.last_drawn() is None and m.tap_result(0) is None
        _, cb = _run(m, forced=f, taps=[(3, 0)])
        np.testing.assert_array_equal(cb, f)
        assert m.tap_result(0) is not None
    finally:
        m.close()


# 8. refusals ---------------------------------------------------------------
def test_refusals_leave_the_context_usable(tiny, free_default):
    a_free, c_free = free_default
    V, Vs, eos = tiny.cfg.talker_vocab_size, tiny.cfg.subtalker_vocab_size, tiny.cfg.codec_eos_id

    def plain_ok():
        a, c = _run(tiny)
        np.testing.assert_array_equal(c, c_free)
        np.testing.assert_array_equal(a, a_free)
        assert tiny.last_drawn() is None

    for f, g, bad in ((1, 0, V - 1024 if eos != V - 1024 else V - 1023), (1, 0, V), (2, 3, Vs)):
        x = c_free.copy()
        x[f, g] = bad
        with pytest.raises(ValueError):
            tiny.force_codes(x)
    plain_ok()                                          # (a refused arming armed nothing)
    for i in range(qtts.MAX_TAPS):
        assert tiny.tap_draw(i, i) == i
    with pytest.raises(ValueError):
        tiny.tap_draw(9, 9)
    a, c = _run(tiny)                                   # consumes the 8 taps
    np.testing.assert_array_equal(c, c_free)
    assert all(tiny.tap_result(i) is not None for i in range(qtts.MAX_TAPS))
    plain_ok()
    tiny.force_codes(c_free, slot=1)                    # slot >= the batch of the call that consumes it
    assert _run(tiny)[0] is None
    plain_ok()
    assert _run(tiny, forced=np.zeros((17, G), np.int32))[0] is None   # more frames than the run generates
    plain_ok()
    assert _run(tiny, taps=[(16, 0)])[0] is None        # a tap past them
    plain_ok()
    tiny.set_params(max_tokens=16, fixed=0, seed=42, **DEFAULT)
    tiny.force_codes(c_free)
    rc, audio = tiny.generate_queue([IDS, IDS], [SPK] * 2, [LANG] * 2, slots=2)
    assert rc == -1 and all(x is None for x in audio)
    plain_ok()                                          # (the refused queue call disarmed)


# 9. hd128, 640 frames ------------------------------------------------------
@pytest.fixture(scope="module")
def hd128(gpu):
    m = qtts.QwenTTS(model_dir("hd128"))
    yield m
    m.close()


def _long_man():
    return json.load(open(os.path.join(GOLDEN, "long_manifest.json")))


def test_hd128_640_frames_every_draw_vs_reference(hd128):
    """All 10,240 draws of the 640-frame reference run, each under the
    reference's own history."""
    g, man = np.load(os.path.join(GOLDEN, "long_hd128.npz")), _long_man()["hd128"]
    ref = g["decode_codes"]
    assert ref.shape == (man["frames"], G)
    hd128.set_params(max_tokens=4096, fixed=man["frames"], seed=man["seed"], **DEFAULT)
    hd128.force_codes(ref)
    a = hd128.generate(g["prompt_ids"], SPK, LANG)
    assert a is not None
    np.testing.assert_array_equal(hd128.last_codes(), ref)
    d = hd128.last_drawn()
    bad = np.argwhere(d != ref)
    assert len(bad) == 0, (len(bad), bad[:8].tolist())


# 10. hd128, 4096 frames ----------------------------------------------------
MAX_EXCUSED = 8   # of 65,536 draws: one known flip in 27,756 puts the expectation near 2-3


@pytest.mark.slow
def test_hd128_4096_frames_every_draw_vs_reference(hd128):
    """The reference's whole 4096-frame run forced: all 65,536 draws compared,
    frames 1735-4095 included (test_hd128_max_capacity_vs_reference stops at
    the first flip).  Every mismatch must be recorded in
    forced_near_ties.json (tools/classify_forced.py) with a two-sided near-tie
    verdict, at most MAX_EXCUSED of them; the known one, (1734, 12) drawn
    1927, is among them."""
    g, man = np.load(os.path.join(GOLDEN, "long_hd128_max.npz")), _long_man()["hd128max"]
    ref = g["codes"]
    assert ref.shape == (4096, G)
    known = [k for k in json.load(open(os.path.join(GOLDEN, "forced_near_ties.json")))["draws"]
             if k["fixture"] == "long_hd128_max"]
    hd128.set_params(max_tokens=man["frames"], fixed=man["frames"], seed=man["seed"], **DEFAULT)
    hd128.force_codes(ref)
    a = hd128.generate(g["prompt_ids"], man["speaker"], man["language"])
    assert a is not None
    np.testing.assert_array_equal(hd128.last_codes(), ref)
    d = hd128.last_drawn()
    assert d.shape == ref.shape
    bad = [(int(f), int(q), int(d[f, q])) for f, q in np.argwhere(d != ref)]
    print("mismatching draws:", bad)
    excused = {(k["frame"], k["group"], k["drawn"]) for k in known
               if k["verdict"] == "fp near-tie" and k["ratio_gpu"] <= 1.0 and k["reference"] == ref[k["frame"], k["group"]]}
    assert (1734, 12, 1927) in bad
    assert all(b in excused for b in bad), [b for b in bad if b not in excused]
    assert len(bad) <= MAX_EXCUSED, len(bad)
    assert a.shape[0] == int(g["audio_len"])
    st = man["audio_stride"]
    _audio_close(a[::st], g["audio_sub"], "every 256th sample, the whole run")
    _audio_close(a[:1920], g["audio_first"], "first frame")
    _audio_close(a[-1920:], g["audio_last"], "last frame")
