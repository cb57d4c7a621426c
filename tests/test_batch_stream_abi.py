"""The batch-streaming entry points at the drop-in boundary, on a CPU box: the
library exports them, both headers and the binding declare them, the context
layout did not move, and qwen_tts_generate_batch_stream refuses a bad slot
count before it touches a device."""
import ctypes as C
import os

import qtts
from conftest import ROOT
from test_abi import header_symbols

PUBLIC = ["qwen_tts_generate_batch_stream", "qwen_tts_codec_mstream_begin", "qwen_tts_codec_mstream_push"]
DEVICE = ["qtts_dev_codec_mstream_begin", "qtts_dev_codec_mstream_push_slots", "qtts_dev_codec_mstream_push_host",
          "qtts_dev_codec_mstream_pos", "qtts_hip_xgemm_seg_case"]


def test_library_exports_and_headers_and_binding_declare_the_symbols():
    lib = qtts.lib()
    missing = [s for s in PUBLIC + DEVICE if not hasattr(lib, s)]
    assert not missing, missing
    assert set(PUBLIC) <= set(header_symbols(os.path.join(ROOT, "include", "qwen_tts.h")))
    assert set(DEVICE) <= set(header_symbols(os.path.join(ROOT, "include", "qtts_hip.h")))
    assert set(PUBLIC + DEVICE) <= set(qtts.EXPORTS)
    assert lib.qwen_tts_generate_batch_stream.argtypes[6] is qtts.BATCH_AUDIO_CB
    assert lib.qtts_hip_xgemm_seg_case.argtypes[0] is C.POINTER(qtts.XGemmDesc)
    for name in ("generate_batch_stream", "codec_mstream", "codec_mstream_begin", "codec_mstream_push",
                 "codec_mstream_pos"):
        assert callable(getattr(qtts.QwenTTS, name)), name
    assert callable(qtts.Kernels.xgemm_seg_case)


def test_ctx_layout_did_not_move():
    assert qtts.lib().qwen_tts_abi_sizeof_ctx() == C.sizeof(qtts.Ctx)
    assert qtts.Ctx._fields_[-1][0] == "force"


def _call(n, ctx):
    lib = qtts.lib()
    k = max(n, 1)
    tx = (C.c_char_p * k)(*[b"1,2,3"] * k)
    out, ns = (C.c_void_p * k)(), (C.c_int * k)()
    rc = lib.qwen_tts_generate_batch_stream(C.byref(ctx), n, tx, None, None, 4, qtts.BATCH_AUDIO_CB(), None, out, ns)
    return rc, out


def test_slot_count_refused_before_the_device(capfd):
    """nb = 0 and nb = 65: -1 from a ctx that has no device model at all, the limit named"""
    ctx = qtts.Ctx()
    rc, out = _call(0, ctx)
    assert rc == -1
    rc, out = _call(65, ctx)
    assert rc == -1
    assert "65 slots, at most 64" in capfd.readouterr().err
    assert all(not o for o in out)


def test_codec_mstream_entries_refuse_a_ctx_without_a_device():
    lib = qtts.lib()
    ctx = qtts.Ctx()
    assert lib.qwen_tts_codec_mstream_begin(C.byref(ctx), 3, 64) == -1
    st, codes = (C.c_int * 1)(0), (C.c_int * 16)()
    o = (C.c_float * 1920)()
    po = (C.POINTER(C.c_float) * 1)(C.cast(o, C.POINTER(C.c_float)))
    assert lib.qwen_tts_codec_mstream_push(C.byref(ctx), 1, st, codes, 1, po) == -1
    assert lib.qtts_dev_codec_mstream_pos(None, 0) == -1
