"""The streamed voice-clone batch and the ragged multi-stream push at the
drop-in boundary, on a CPU box: the library exports them, both headers and the
binding declare them, the context layout did not move, and the calls refuse a
bad slot count or a context without a device before they touch one."""
import ctypes as C
import os

import qtts
from conftest import ROOT
from test_abi import header_symbols

PUBLIC = ["qwen_tts_generate_voice_clone_batch_stream", "qwen_tts_generate_voice_clone_audio_batch_stream",
          "qwen_tts_codec_mstream_push_ragged"]
DEVICE = ["qtts_dev_codec_mstream_push_host_ragged", "qtts_dev_codec_mstream_push_slots_ragged",
          "qtts_dev_codec_mstream_prime"]


def test_library_exports_and_headers_and_binding_declare_the_symbols():
    lib = qtts.lib()
    missing = [s for s in PUBLIC + DEVICE if not hasattr(lib, s)]
    assert not missing, missing
    assert set(PUBLIC) <= set(header_symbols(os.path.join(ROOT, "include", "qwen_tts.h")))
    assert set(DEVICE) <= set(header_symbols(os.path.join(ROOT, "include", "qtts_hip.h")))
    assert set(PUBLIC + DEVICE) <= set(qtts.EXPORTS)
    assert lib.qwen_tts_generate_voice_clone_batch_stream.argtypes[10] is qtts.BATCH_AUDIO_CB
    assert lib.qwen_tts_generate_voice_clone_audio_batch_stream.argtypes[10] is qtts.BATCH_AUDIO_CB
    for name in ("generate_voice_clone_batch_stream", "generate_voice_clone_audio_batch_stream",
                 "codec_mstream_push_ragged"):
        assert callable(getattr(qtts.QwenTTS, name)), name


def test_header_no_longer_says_the_voice_clone_batch_does_not_stream():
    with open(os.path.join(ROOT, "include", "qwen_tts.h")) as f:
        text = " ".join(f.read().split())
    assert "voice-clone batch calls do not stream" not in text


def test_ctx_layout_did_not_move():
    assert qtts.lib().qwen_tts_abi_sizeof_ctx() == C.sizeof(qtts.Ctx)
    assert qtts.Ctx._fields_[-1][0] == "force"


def _call(n, ctx):
    lib = qtts.lib()
    k = max(n, 1)
    tx = (C.c_char_p * k)(*[b"1,2,3"] * k)
    out, ns = (C.c_void_p * k)(), (C.c_int * k)()
    rc = lib.qwen_tts_generate_voice_clone_batch_stream(C.byref(ctx), n, tx, None, None, None, None, None, 0, 4,
                                                        qtts.BATCH_AUDIO_CB(), None, out, ns)
    return rc, out


def test_slot_count_refused_before_the_device(capfd):
    """nb = 0 and nb = 65: -1 from a ctx that has no device model at all, the limit named"""
    ctx = qtts.Ctx()
    rc, out = _call(0, ctx)
    assert rc == -1
    capfd.readouterr()
    rc, out = _call(65, ctx)
    assert rc == -1
    err = capfd.readouterr().err
    assert "qwen_tts_generate_voice_clone_batch_stream: 65 slots, at most 64" in err
    assert all(not o for o in out)


def test_audio_form_keeps_the_encoders_limit(capfd):
    """the reference-audio form: 1..16 utterances, refused from a ctx without a device"""
    lib = qtts.lib()
    ctx = qtts.Ctx()
    for n in (0, 17):
        k = max(n, 1)
        tx = (C.c_char_p * k)(*[b"1,2,3"] * k)
        w = (C.c_float * 1920)()
        wp = (C.POINTER(C.c_float) * k)(*[C.cast(w, C.POINTER(C.c_float))] * k)
        nw = (C.c_int * k)(*[1920] * k)
        out, ns = (C.c_void_p * k)(), (C.c_int * k)()
        capfd.readouterr()
        assert lib.qwen_tts_generate_voice_clone_audio_batch_stream(C.byref(ctx), n, tx, None, wp, nw, None, None, 0, 4,
                                                                    qtts.BATCH_AUDIO_CB(), None, out, ns) == -1
        assert "1..16 utterances" in capfd.readouterr().err
        assert all(not o for o in out)


def test_ragged_push_refuses_a_ctx_without_a_device():
    lib = qtts.lib()
    ctx = qtts.Ctx()
    st, codes, cnt = (C.c_int * 1)(0), (C.c_int * 16)(), (C.c_int * 1)(1)
    o = (C.c_float * 1920)()
    po = (C.POINTER(C.c_float) * 1)(C.cast(o, C.POINTER(C.c_float)))
    assert lib.qwen_tts_codec_mstream_push_ragged(C.byref(ctx), 1, st, codes, cnt, 1, po) == -1
    assert lib.qtts_dev_codec_mstream_push_host_ragged(None, 1, st, codes, cnt, 1, po) == -1
    assert lib.qtts_dev_codec_mstream_push_slots_ragged(None, 1, st, st, st, cnt, po) == -1
    assert lib.qtts_dev_codec_mstream_prime(None, 1, st, codes, cnt, 1) == -1
