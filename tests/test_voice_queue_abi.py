"""Codec snapshots, voice handles and the voice-clone work queue at the drop-in
boundary, on a CPU box: the library exports them, both headers and the binding
declare them with the signatures the headers state, the context layout did not
move, and every entry answers NULL / -1 to NULL arguments or a context without
a device before it touches one."""
import ctypes as C
import os
import re

import qtts
from conftest import ROOT
from test_abi import header_symbols

PUBLIC = ["qwen_tts_codec_mstream_save", "qwen_tts_codec_mstream_restore", "qwen_tts_codec_snapshot_free",
          "qwen_tts_codec_snapshot_pos", "qwen_tts_voice_create", "qwen_tts_voice_create_audio",
          "qwen_tts_voice_info", "qwen_tts_voice_free", "qwen_tts_generate_voice_queue",
          "qwen_tts_generate_voice_queue_stream"]
DEVICE = ["qtts_dev_codec_mstream_save", "qtts_dev_codec_mstream_restore", "qtts_dev_codec_snapshot_free",
          "qtts_dev_codec_snapshot_pos", "qtts_dev_codec_snapshot_bytes"]


def _params(header, name):
    """number of parameters of `name` as the header declares it"""
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, src)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"])


def test_library_exports_and_headers_and_binding_declare_the_symbols():
    lib = qtts.lib()
    missing = [s for s in PUBLIC + DEVICE if not hasattr(lib, s)]
    assert not missing, missing
    assert set(PUBLIC) <= set(header_symbols(os.path.join(ROOT, "include", "qwen_tts.h")))
    assert set(DEVICE) <= set(header_symbols(os.path.join(ROOT, "include", "qtts_hip.h")))
    assert set(PUBLIC + DEVICE) <= set(qtts.EXPORTS)
    for name in ("voice_create", "voice_create_audio", "voice_info", "voice_free", "generate_voice_queue",
                 "generate_voice_queue_stream", "codec_mstream_save", "codec_mstream_restore",
                 "codec_snapshot_free"):
        assert callable(getattr(qtts.QwenTTS, name)), name


def test_binding_signatures_are_the_headers():
    lib = qtts.lib()
    for name in PUBLIC:
        assert len(getattr(lib, name).argtypes) == _params("qwen_tts.h", name), name
    for name in DEVICE:
        assert len(getattr(lib, name).argtypes) == _params("qtts_hip.h", name), name
    vq, vqs = lib.qwen_tts_generate_voice_queue, lib.qwen_tts_generate_voice_queue_stream
    assert vq.argtypes[7] is qtts.QUEUE_NEXT_CB and vqs.argtypes[7] is qtts.QUEUE_NEXT_CB
    assert vqs.argtypes[10] is qtts.BATCH_AUDIO_CB
    # the queue's argument list with `speakers` replaced by `voices` and `non_streaming` added
    assert len(vq.argtypes) == len(lib.qwen_tts_generate_queue.argtypes) + 1
    assert len(vqs.argtypes) == len(lib.qwen_tts_generate_queue_stream.argtypes) + 1
    assert lib.qwen_tts_voice_create.restype is C.c_void_p and lib.qwen_tts_codec_mstream_save.restype is C.c_void_p


def test_ctx_layout_did_not_move():
    """the library that has the voice handles still has the context layout of the ctypes mirror:
    nothing was added to qwen_tts_ctx_t for them"""
    assert hasattr(qtts.lib(), "qwen_tts_voice_create")
    assert qtts.lib().qwen_tts_abi_sizeof_ctx() == C.sizeof(qtts.Ctx)
    assert qtts.Ctx._fields_[-1][0] == "force"


def test_null_arguments_give_null_or_minus_one_without_a_device():
    lib = qtts.lib()
    ctx = qtts.Ctx()   # no device model behind it
    codes, xv = (C.c_int * 16)(), (C.c_float * 8)()
    wav = (C.c_float * 1920)()
    fp = C.cast(wav, C.POINTER(C.c_float))
    assert not lib.qwen_tts_voice_create(None, b"1,2,3,4,5", codes, 1, xv)
    assert not lib.qwen_tts_voice_create(C.byref(ctx), b"1,2,3,4,5", codes, 1, xv)
    assert not lib.qwen_tts_voice_create_audio(None, b"1,2,3,4,5", fp, 1920, 0)
    assert not lib.qwen_tts_voice_create_audio(C.byref(ctx), b"1,2,3,4,5", fp, 1920, 0)
    assert not lib.qwen_tts_voice_create_audio(C.byref(ctx), b"1,2,3,4,5", None, 1920, 0)
    n, p = C.c_int(7), C.c_int(7)
    assert lib.qwen_tts_voice_info(None, C.byref(n), C.byref(p)) == -1 and (n.value, p.value) == (7, 7)
    lib.qwen_tts_voice_free(None)
    assert not lib.qwen_tts_codec_mstream_save(None, 0)
    assert not lib.qwen_tts_codec_mstream_save(C.byref(ctx), 0)
    assert lib.qwen_tts_codec_mstream_restore(None, 0, None) == -1
    assert lib.qwen_tts_codec_mstream_restore(C.byref(ctx), 0, None) == -1
    lib.qwen_tts_codec_snapshot_free(None)
    assert lib.qwen_tts_codec_snapshot_pos(None) == -1
    assert not lib.qtts_dev_codec_mstream_save(None, 0)
    assert lib.qtts_dev_codec_mstream_restore(None, 0, None) == -1
    lib.qtts_dev_codec_snapshot_free(None)
    assert lib.qtts_dev_codec_snapshot_pos(None) == -1 and lib.qtts_dev_codec_snapshot_bytes(None) == -1


def test_voice_queue_refuses_before_the_device(capfd):
    lib = qtts.lib()
    ctx = qtts.Ctx()
    tx = (C.c_char_p * 2)(b"1,2,3", b"1,2,3")
    vs = (C.c_void_p * 2)()
    out, ns = (C.c_void_p * 2)(), (C.c_int * 2)()
    nocb = qtts.QUEUE_NEXT_CB()
    for c in (None, C.byref(ctx)):
        assert lib.qwen_tts_generate_voice_queue(c, 2, tx, vs, None, 0, 2, nocb, None, out, ns) == -1
        assert lib.qwen_tts_generate_voice_queue(c, 2, tx, None, None, 0, 2, nocb, None, out, ns) == -1
        assert lib.qwen_tts_generate_voice_queue_stream(c, 2, tx, vs, None, 0, 2, nocb, None, 4,
                                                        qtts.BATCH_AUDIO_CB(), None, out, ns) == -1
        assert lib.qwen_tts_generate_voice_queue_stream(c, 2, tx, None, None, 0, 2, nocb, None, 4,
                                                        qtts.BATCH_AUDIO_CB(), None, out, ns) == -1
    capfd.readouterr()
    assert lib.qwen_tts_generate_voice_queue_stream(C.byref(ctx), 2, tx, vs, None, 0, 65, nocb, None, 4,
                                                    qtts.BATCH_AUDIO_CB(), None, out, ns) == -1
    assert "qwen_tts_generate_voice_queue_stream: 65 slots, at most 64" in capfd.readouterr().err
    assert all(not o for o in out)
