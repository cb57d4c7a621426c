"""Teacher-forced decode at the drop-in boundary, on a CPU box: the library
exports and the headers declare the new entry points, the ctypes signatures
load, the CLI lists its two flags and refuses a malformed --force-codes file
before it loads a model, and the entries refuse a missing handle without
touching a device."""
import ctypes as C
import os
import re
import subprocess

import qtts

HOST = ["qwen_tts_force_codes", "qwen_tts_tap_draw", "qwen_tts_last_drawn", "qwen_tts_tap_result"]
DEV = ["qtts_dev_force", "qtts_dev_tap", "qtts_dev_get_drawn", "qtts_dev_get_tap"]
INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


def test_library_exports_and_headers_declare_the_symbols():
    lib = qtts.lib()
    missing = [s for s in HOST + DEV if not hasattr(lib, s)]
    assert not missing, missing
    assert set(HOST + DEV) <= set(qtts.EXPORTS)
    for header, names in (("qwen_tts.h", HOST), ("qtts_hip.h", DEV)):
        txt = open(os.path.join(INCLUDE, header)).read()
        for s in names:
            assert re.search(r"^int %s\(" % s, txt, re.M), (header, s)


def test_ctypes_signatures_load_and_ctx_mirror_matches():
    lib = qtts.lib()
    ip, fp, up = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_uint)
    ctx = C.POINTER(qtts.Ctx)
    want = {"qwen_tts_force_codes": [ctx, C.c_int, ip, C.c_int], "qwen_tts_tap_draw": [ctx, C.c_int, C.c_int, C.c_int],
            "qwen_tts_last_drawn": [ctx, C.c_int, ip, C.c_int],
            "qwen_tts_tap_result": [ctx, C.c_int, fp, C.c_int, up, ip],
            "qtts_dev_force": [C.c_void_p, C.c_int, ip, C.c_int], "qtts_dev_tap": [C.c_void_p, C.c_int, C.c_int, C.c_int],
            "qtts_dev_get_drawn": [C.c_void_p, C.c_int, ip, C.c_int],
            "qtts_dev_get_tap": [C.c_void_p, C.c_int, fp, C.c_int, up, ip]}
    for name, args in want.items():
        f = getattr(lib, name)
        assert f.restype is C.c_int and list(f.argtypes) == args, name
    # the arming lives behind one pointer at the end of the ctx
    assert qtts.Ctx._fields_[-1][0] == "force"
    assert lib.qwen_tts_abi_sizeof_ctx() == C.sizeof(qtts.Ctx)
    for m in ("force_codes", "tap_draw", "last_drawn", "tap_result"):
        assert callable(getattr(qtts.QwenTTS, m))
    assert qtts.MAX_TAPS == 8


def test_entries_refuse_a_missing_handle():
    lib = qtts.lib()
    codes = (C.c_int * 16)(*range(16))
    assert lib.qwen_tts_force_codes(None, 0, codes, 1) == -1
    assert lib.qwen_tts_tap_draw(None, 0, 0, 0) == -1
    assert lib.qwen_tts_last_drawn(None, 0, codes, 1) == -1
    assert lib.qwen_tts_tap_result(None, 0, None, 0, None, None) == -1
    ctx = qtts.Ctx()   # a ctx without a device model
    assert lib.qwen_tts_force_codes(C.byref(ctx), 0, codes, 1) == -1
    assert lib.qwen_tts_tap_draw(C.byref(ctx), 0, 0, 0) == -1
    assert lib.qwen_tts_last_drawn(C.byref(ctx), 0, codes, 1) == -1
    assert lib.qwen_tts_tap_result(C.byref(ctx), 0, None, 0, None, None) == -1
    assert not ctx.force
    assert lib.qtts_dev_force(None, 0, codes, 1) == -1
    assert lib.qtts_dev_tap(None, 0, 0, 0) == -1
    assert lib.qtts_dev_get_drawn(None, 0, codes, 1) == -1
    assert lib.qtts_dev_get_tap(None, 0, None, 0, None, None) == -1


def test_cli_help_lists_both_flags():
    r = subprocess.run([qtts.CLI_PATH, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    txt = r.stdout + r.stderr
    assert "--force-codes" in txt and "--dump-drawn" in txt


def test_cli_refuses_a_malformed_force_file_before_loading_a_model(tmp_path):
    for name, body in (("short.txt", "1 2 3\n"), ("word.txt", " ".join(["7"] * 15) + " x\n"), ("empty.txt", "")):
        p = tmp_path / name
        p.write_text(body)
        r = subprocess.run([qtts.CLI_PATH, "-d", "/nonexistent", "-t", "1,2,3", "--force-codes", str(p)],
                           capture_output=True, text=True)
        assert r.returncode != 0, name
        assert "--force-codes needs 16 ints per frame" in r.stderr or "bad number" in r.stderr, (name, r.stderr)
        assert "Loading model" not in r.stderr and "failed to load model" not in r.stderr, (name, r.stderr)
    r = subprocess.run([qtts.CLI_PATH, "-d", "/nonexistent", "-t", "1,2,3", "--force-codes", str(tmp_path / "absent")],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "failed to load model" not in r.stderr
