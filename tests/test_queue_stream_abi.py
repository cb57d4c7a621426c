"""The streaming work queue and the any-position multi-stream codec entries at
the drop-in boundary, on a CPU box: the library exports them, both headers and
the binding declare them, the context layout did not move, and the calls
refuse a bad slot count or a ctx without a device before they touch one."""
import ctypes as C
import os

import qtts
from conftest import ROOT
from test_abi import header_symbols

PUBLIC = ["qwen_tts_generate_queue_stream", "qwen_tts_codec_mstream_push_any", "qwen_tts_codec_mstream_reset"]
DEVICE = ["qtts_dev_codec_mstream_push_host_any", "qtts_dev_codec_mstream_push_slots_at",
          "qtts_dev_codec_mstream_reset"]


def test_library_exports_and_headers_and_binding_declare_the_symbols():
    lib = qtts.lib()
    missing = [s for s in PUBLIC + DEVICE if not hasattr(lib, s)]
    assert not missing, missing
    assert set(PUBLIC) <= set(header_symbols(os.path.join(ROOT, "include", "qwen_tts.h")))
    assert set(DEVICE) <= set(header_symbols(os.path.join(ROOT, "include", "qtts_hip.h")))
    assert set(PUBLIC + DEVICE) <= set(qtts.EXPORTS)
    assert lib.qwen_tts_generate_queue_stream.argtypes[6] is qtts.QUEUE_NEXT_CB
    assert lib.qwen_tts_generate_queue_stream.argtypes[9] is qtts.BATCH_AUDIO_CB
    for name in ("generate_queue_stream", "codec_mstream_push_any", "codec_mstream_reset"):
        assert callable(getattr(qtts.QwenTTS, name)), name


def test_ctx_layout_did_not_move():
    assert qtts.lib().qwen_tts_abi_sizeof_ctx() == C.sizeof(qtts.Ctx)
    assert qtts.Ctx._fields_[-1][0] == "force"


def _call(nb, ctx, nq=3):
    lib = qtts.lib()
    tx = (C.c_char_p * nq)(*[b"1,2,3"] * nq)
    out, ns = (C.c_void_p * nq)(), (C.c_int * nq)()
    rc = lib.qwen_tts_generate_queue_stream(C.byref(ctx), nq, tx, None, None, nb, qtts.QUEUE_NEXT_CB(), None, 4,
                                            qtts.BATCH_AUDIO_CB(), None, out, ns)
    return rc, out


def test_slot_count_refused_before_the_device(capfd):
    """0 and 65 slots: -1 from a ctx that has no device model at all, the limit named"""
    ctx = qtts.Ctx()
    rc, out = _call(0, ctx)
    assert rc == -1
    rc, out = _call(65, ctx)
    assert rc == -1
    err = capfd.readouterr().err
    assert "qwen_tts_generate_queue_stream: 65 slots, at most 64" in err, err
    assert all(not o for o in out)


def test_codec_entries_refuse_a_ctx_without_a_device():
    lib = qtts.lib()
    ctx = qtts.Ctx()
    st, codes = (C.c_int * 1)(0), (C.c_int * 16)()
    o = (C.c_float * 1920)()
    po = (C.POINTER(C.c_float) * 1)(C.cast(o, C.POINTER(C.c_float)))
    assert lib.qwen_tts_codec_mstream_push_any(C.byref(ctx), 1, st, codes, 1, po) == -1
    assert lib.qwen_tts_codec_mstream_reset(C.byref(ctx), 0) == -1
    assert lib.qtts_dev_codec_mstream_reset(None, 0) == -1
    assert lib.qtts_dev_codec_mstream_push_host_any(None, 1, st, codes, 1, po) == -1
    f0 = (C.c_int * 1)(0)
    assert lib.qtts_dev_codec_mstream_push_slots_at(None, 1, st, st, f0, 1, po) == -1
    assert all(v == 0.0 for v in o)
