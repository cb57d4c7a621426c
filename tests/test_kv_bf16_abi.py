"""The bf16 talker KV cache switch at the drop-in boundary, on a CPU box: the
library exports the new entry points, the CLI lists its flag, and the setters
refuse a missing handle or an unknown element type without touching a device."""
import ctypes as C
import subprocess

import qtts

NEW_SYMBOLS = ["qwen_tts_set_kv_cache_dtype", "qwen_tts_kv_cache_dtype", "qtts_dev_set_kv_dtype", "qtts_dev_kv_dtype",
               "qtts_dev_get_kv", "qtts_dev_get_attn", "qtts_hip_attn_decode"]


def test_library_exports_kv_cache_symbols():
    lib = qtts.lib()
    missing = [s for s in NEW_SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing
    assert set(NEW_SYMBOLS) <= set(qtts.EXPORTS)
    assert (qtts.KV_F32, qtts.KV_BF16) == (0, 1)


def test_cli_usage_lists_kv_cache_flag():
    r = subprocess.run([qtts.CLI_PATH], capture_output=True, text=True)
    assert r.returncode != 0
    txt = r.stdout + r.stderr
    assert "--kv-cache" in txt and "bf16" in txt and "fp32" in txt


def test_cli_rejects_unknown_kv_cache_value():
    r = subprocess.run([qtts.CLI_PATH, "-d", "/nonexistent", "-t", "1,2,3", "--kv-cache", "fp8"],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "--kv-cache takes fp32 or bf16" in r.stderr


def test_setters_refuse_null_handle_and_bad_dtype():
    lib = qtts.lib()
    for dtype in (0, 1, 2, -1):
        assert lib.qtts_dev_set_kv_dtype(None, dtype) == -1
        assert lib.qwen_tts_set_kv_cache_dtype(None, dtype) == -1
    assert lib.qtts_dev_kv_dtype(None) == -1
    assert lib.qwen_tts_kv_cache_dtype(None) == -1
    # a ctx without a device model (what qwen_tts_load leaves when it fails half way)
    ctx = qtts.Ctx()
    assert lib.qwen_tts_set_kv_cache_dtype(C.byref(ctx), 1) == -1
    assert lib.qwen_tts_kv_cache_dtype(C.byref(ctx)) == -1
    assert lib.qtts_dev_get_kv(None, 0, 0, 0, 1, None, None) == -1
    assert lib.qtts_dev_get_attn(None, None, None) == -1


def test_attn_decode_refuses_bad_arguments_before_any_device_work():
    lib = qtts.lib()
    one = C.c_void_p(16)   # never dereferenced: the argument checks come first
    ok = [one] * 9
    assert lib.qtts_hip_attn_decode(*([None] + ok[1:]), 4, 2, 32, 64, 1, 1e-6, 0, None) == -1
    assert lib.qtts_hip_attn_decode(*ok, 4, 2, 32, 64, 1, 1e-6, 2, None) == -1    # element type
    assert lib.qtts_hip_attn_decode(*ok, 4, 2, 32, 0, 1, 1e-6, 1, None) == -1     # capacity
    assert lib.qtts_hip_attn_decode(*ok, 4, 2, 32, 64, 0, 1e-6, 1, None) == -1    # rows
