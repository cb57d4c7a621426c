"""Per-utterance sampling parameters and seeds at the drop-in boundary, on a
CPU box: the library exports and the headers declare the new entry points, the
ctypes signatures load, the ctx mirror has the library's size, every entry
refuses a missing handle and a ctx without a device model, the arming refuses
bad values, and the CLI lists --seed-step."""
import ctypes as C
import math
import os
import re
import subprocess

import qtts

HOST = ["qwen_tts_sampling_defaults", "qwen_tts_set_utterance_sampling"]
DEV = ["qtts_dev_slot_params", "qtts_hip_sample_slot_launches", "qtts_hip_sample_top_k_rows"]
INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


def _default():
    return qtts.Sampling(0.9, 1.0, 1.05, 50, 0.9, 1.0, 50, 42)


def test_library_exports_and_headers_declare_the_symbols():
    lib = qtts.lib()
    missing = [s for s in HOST + DEV if not hasattr(lib, s)]
    assert not missing, missing
    assert set(HOST + DEV) <= set(qtts.EXPORTS)
    for header, names in (("qwen_tts.h", HOST), ("qtts_hip.h", DEV)):
        txt = open(os.path.join(INCLUDE, header)).read()
        for s in names:
            assert re.search(r"^(int|long long) %s\(" % s, txt, re.M), (header, s)
    assert "qwen_tts_sampling_t" in open(os.path.join(INCLUDE, "qwen_tts.h")).read()
    assert "qtts_slot_params_t" in open(os.path.join(INCLUDE, "qtts_hip.h")).read()


def test_ctypes_signatures_load_and_ctx_mirror_matches():
    lib = qtts.lib()
    ip, fp, vp = C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_void_p
    ctx = C.POINTER(qtts.Ctx)
    want = {"qwen_tts_sampling_defaults": (C.c_int, [ctx, C.POINTER(qtts.Sampling)]),
            "qwen_tts_set_utterance_sampling": (C.c_int, [ctx, C.c_int, C.POINTER(qtts.Sampling)]),
            "qtts_dev_slot_params": (C.c_int, [vp, C.c_int, C.POINTER(qtts.SlotParams)]),
            "qtts_hip_sample_slot_launches": (C.c_longlong, []),
            "qtts_hip_sample_top_k_rows": (C.c_int, [vp, vp, C.c_int, ip, fp, fp, vp, C.c_int, vp])}
    for name, (res, args) in want.items():
        f = getattr(lib, name)
        assert f.restype is res and list(f.argtypes or []) == args, name
    # the arming lives behind one pointer of its own in the ctx
    assert "sampling" in [n for n, _ in qtts.Ctx._fields_]
    assert lib.qwen_tts_abi_sizeof_ctx() == C.sizeof(qtts.Ctx)
    # seven values and a seed, 32 bytes: the device table's row
    assert C.sizeof(qtts.Sampling) == 32 and C.sizeof(qtts.SlotParams) == 32
    assert callable(qtts.QwenTTS.set_utterance_sampling) and callable(qtts.Kernels.sample_top_k_rows)
    assert lib.qtts_hip_sample_slot_launches() >= 0   # (callable without a device)


def test_entries_refuse_a_missing_handle():
    lib = qtts.lib()
    s = _default()
    assert lib.qwen_tts_sampling_defaults(None, C.byref(s)) == -1
    assert lib.qwen_tts_set_utterance_sampling(None, 1, C.byref(s)) == -1
    ctx = qtts.Ctx()   # a ctx without a device model
    assert lib.qwen_tts_sampling_defaults(C.byref(ctx), C.byref(s)) == -1
    assert lib.qwen_tts_set_utterance_sampling(C.byref(ctx), 1, C.byref(s)) == -1
    assert not ctx.sampling and not ctx.force
    p = qtts.SlotParams(0.9, 1.0, 1.05, 50, 0.9, 1.0, 50, 42)
    assert lib.qtts_dev_slot_params(None, 0, C.byref(p)) == -1
    k, f = (C.c_int * 1)(50), (C.c_float * 1)(1.0)
    assert lib.qtts_hip_sample_top_k_rows(None, None, 64, k, f, f, None, 1, None) == -1


def test_arming_refuses_bad_values():
    """validated at arming time, before any device is needed: a ctx whose
    device handle is a dummy is never dereferenced by the arming entries"""
    lib = qtts.lib()
    ctx = qtts.Ctx()
    ctx.hip = 1   # (only tested for NULL here; no generation call follows)
    ok = _default()
    bad = []
    for field in ("temperature", "top_p", "repetition_penalty", "subtalker_temperature", "subtalker_top_p"):
        for v in (math.nan, math.inf, -math.inf):
            s = _default()
            setattr(s, field, v)
            bad.append(s)
    for field, v in (("top_p", 0.0), ("top_p", -0.5), ("subtalker_top_p", 0.0), ("repetition_penalty", 0.0),
                     ("repetition_penalty", -1.0)):
        s = _default()
        setattr(s, field, v)
        bad.append(s)
    for s in bad:
        assert lib.qwen_tts_set_utterance_sampling(C.byref(ctx), 1, C.byref(s)) == -1
        assert not ctx.sampling
        # a bad set anywhere in the list refuses the whole arming
        two = (qtts.Sampling * 2)(ok, s)
        assert lib.qwen_tts_set_utterance_sampling(C.byref(ctx), 2, two) == -1
        assert not ctx.sampling
    for n in (0, -1):
        assert lib.qwen_tts_set_utterance_sampling(C.byref(ctx), n, C.byref(ok)) == -1
    assert lib.qwen_tts_set_utterance_sampling(C.byref(ctx), 1, None) == -1
    assert not ctx.sampling
    # a good one arms (temperature <= 0 and top_k <= 0 are the reference's own cases), a later one replaces it
    s = _default()
    s.temperature, s.top_k = 0.0, 0
    assert lib.qwen_tts_set_utterance_sampling(C.byref(ctx), 1, C.byref(s)) == 0 and ctx.sampling
    three = (qtts.Sampling * 3)(ok, ok, ok)
    assert lib.qwen_tts_set_utterance_sampling(C.byref(ctx), 3, three) == 0 and ctx.sampling
    # a refused arming leaves the earlier one in place
    assert lib.qwen_tts_set_utterance_sampling(C.byref(ctx), 1, C.byref(bad[0])) == -1 and ctx.sampling
    d = qtts.Sampling()
    ctx.temperature, ctx.top_k, ctx.sample_seed = 0.7, 33, 9
    assert lib.qwen_tts_sampling_defaults(C.byref(ctx), C.byref(d)) == 0
    assert (round(d.temperature, 6), d.top_k, d.sample_seed) == (0.7, 33, 9)
    # (the dummy ctx is Python's, never qwen_tts_free'd: its last arming, a few dozen bytes, stays allocated)


def test_cli_help_lists_seed_step():
    r = subprocess.run([qtts.CLI_PATH, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    assert "--seed-step" in r.stdout + r.stderr
