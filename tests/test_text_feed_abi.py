"""Incremental text input at the drop-in boundary, on a CPU box: the library
exports the entries, both headers and the binding declare them, the context
layout did not move, and the fed calls refuse what they must before they touch
a device (a ctx without a device model: anything that went further would not
return these messages)."""
import ctypes as C
import os

import qtts
from conftest import ROOT
from test_abi import header_symbols

PUBLIC = ["qwen_tts_feed_ids", "qwen_tts_feed_close", "qwen_tts_feed_state", "qwen_tts_generate_fed_stream",
          "qwen_tts_generate_fed_batch_stream"]
DEVICE = ["qtts_dev_text_open", "qtts_dev_text_append", "qtts_dev_get_trailing", "qtts_dev_text_state",
          "qtts_hip_text_held_frames", "qtts_dev_text_append_ms"]
_ip = C.POINTER(C.c_int)


def test_library_exports_and_headers_and_binding_declare_the_symbols():
    lib = qtts.lib()
    missing = [s for s in PUBLIC + DEVICE if not hasattr(lib, s)]
    assert not missing, missing
    assert set(PUBLIC) <= set(header_symbols(os.path.join(ROOT, "include", "qwen_tts.h")))
    assert set(DEVICE) <= set(header_symbols(os.path.join(ROOT, "include", "qtts_hip.h")))
    assert set(PUBLIC + DEVICE) <= set(qtts.EXPORTS)
    for name in ("generate_fed_stream", "generate_fed_batch_stream", "text_held_frames"):
        assert callable(getattr(qtts.QwenTTS, name)), name
    for name in ("push", "close", "state"):
        assert callable(getattr(qtts.FeedHandle, name)), name


def test_ctypes_signatures():
    lib = qtts.lib()
    f = lib.qwen_tts_generate_fed_batch_stream
    assert f.restype is C.c_int
    assert f.argtypes == [C.POINTER(qtts.Ctx), C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_int,
                          qtts.TEXT_FEED_CB, C.c_void_p, qtts.BATCH_AUDIO_CB, C.c_void_p, C.POINTER(C.c_void_p), _ip]
    g = lib.qwen_tts_generate_fed_stream
    assert g.restype is C.c_void_p
    assert g.argtypes == [C.POINTER(qtts.Ctx), C.c_char_p, C.c_char_p, C.c_int, qtts.TEXT_FEED_CB, C.c_void_p,
                          qtts.AUDIO_CB, C.c_void_p, _ip]
    assert lib.qwen_tts_feed_ids.argtypes == [C.c_void_p, C.c_int, _ip, C.c_int]
    assert lib.qwen_tts_feed_close.argtypes == [C.c_void_p, C.c_int]
    assert lib.qwen_tts_feed_state.argtypes == [C.c_void_p, C.c_int, _ip, _ip, _ip]
    assert lib.qtts_dev_text_append.argtypes == [C.c_void_p, C.c_int, _ip, C.c_int, C.c_int]
    assert lib.qtts_hip_text_held_frames.restype is C.c_longlong
    # qwen_tts_text_feed_cb: int (feed, wait, userdata)
    assert qtts.TEXT_FEED_CB._restype_ is C.c_int
    assert qtts.TEXT_FEED_CB._argtypes_ == (C.c_void_p, C.c_int, C.c_void_p)


def test_ctx_layout_did_not_move():
    assert qtts.lib().qwen_tts_abi_sizeof_ctx() == C.sizeof(qtts.Ctx)


def _ctx():
    ctx = qtts.Ctx()
    ctx.max_new_tokens = 16
    ctx.config.talker_text_vocab = 151936
    return ctx


def _call(ctx, nb, feed):
    k = max(nb, 1)
    out, ns = (C.c_void_p * k)(), (C.c_int * k)()
    for i in range(k):
        out[i] = 0xdead0   # (the call clears what it does not fill)
    rc = qtts.lib().qwen_tts_generate_fed_batch_stream(C.byref(ctx), nb, None, None, 4, feed, None,
                                                       qtts.BATCH_AUDIO_CB(), None, out, ns)
    return rc, out


def _never(calls):
    def cb(f, wait, u):
        calls.append(wait)
        return 0
    return qtts.TEXT_FEED_CB(cb)


def test_null_feed_callback_refused(capfd):
    rc, out = _call(_ctx(), 1, C.cast(None, qtts.TEXT_FEED_CB))
    assert rc == -1 and not out[0]
    assert "no feed callback" in capfd.readouterr().err


def test_slot_count_refused_before_the_device(capfd):
    calls = []
    rc, _ = _call(_ctx(), 0, _never(calls))
    assert rc == -1
    rc, out = _call(_ctx(), 65, _never(calls))
    assert rc == -1 and not calls
    assert "65 slots, at most 64" in capfd.readouterr().err
    assert all(not o for o in out)


def test_armed_forcing_refused_and_disarmed(capfd):
    ctx = _ctx()
    libc = C.CDLL(None)
    libc.calloc.restype = C.c_void_p
    libc.calloc.argtypes = [C.c_size_t, C.c_size_t]
    ctx.force = libc.calloc(1, 256)   # an empty force_arm_t: what qwen_tts_tap_draw / _force_codes leave armed
    calls = []
    rc, out = _call(ctx, 1, _never(calls))
    assert rc == -1 and not calls and not out[0]
    assert not ctx.force
    assert "forced codes / taps are armed" in capfd.readouterr().err


def test_utterance_closed_empty_fails_before_the_device(capfd):
    lib = qtts.lib()
    seen = []

    def cb(f, wait, u):
        seen.append(wait)
        ids = (C.c_int * 2)(2354, 2244)
        assert lib.qwen_tts_feed_ids(f, 2, ids, 2) == -1      # a bad utterance index
        assert lib.qwen_tts_feed_ids(f, 0, ids, 2) == 0
        assert lib.qwen_tts_feed_close(f, 1) == 0              # utterance 1: closed with nothing
        assert lib.qwen_tts_feed_ids(f, 1, ids, 1) == -1       # and a push after the close
        return 0
    rc, out = _call(_ctx(), 2, qtts.TEXT_FEED_CB(cb))
    assert rc == -1 and seen == [1]
    assert all(not o for o in out)
    err = capfd.readouterr().err
    assert "utterance 1 was closed without an id" in err
    assert "utterance 2 of 2" in err and "utterance 1 is closed" in err


def test_feed_entries_outside_a_callback():
    lib = qtts.lib()
    ids = (C.c_int * 1)(5)
    assert lib.qwen_tts_feed_ids(None, 0, ids, 1) == -1
    assert lib.qwen_tts_feed_close(None, 0) == -1
    assert lib.qwen_tts_feed_state(None, 0, None, None, None) == -1


def test_no_progress_and_abort_before_the_device(capfd):
    rc, _ = _call(_ctx(), 1, _never([]))
    assert rc == -1
    assert "feed made no progress" in capfd.readouterr().err
    rc, _ = _call(_ctx(), 1, qtts.TEXT_FEED_CB(lambda f, w, u: -3))
    assert rc == -1
    assert "aborted" in capfd.readouterr().err
