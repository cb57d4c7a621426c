"""The bf16 talker KV cache switch at the drop-in boundary, on a CPU box: the
library exports the new entry points, the CLI lists its flag, and the setters
refuse a missing handle or an unknown element type without touching a device."""
import ctypes as C
import subprocess

import qtts

NEW_SYMBOLS = ["qwen_tts_set_kv_cache_dtype", "qwen_tts_kv_cache_dtype", "qtts_dev_set_kv_dtype", "qtts_dev_kv_dtype",
               "qtts_dev_get_kv", "qtts_dev_get_attn", "qtts_hip_attn_decode",
               "qtts_hip_attn_decode_ex", "qtts_hip_attn_cached", "qtts_hip_attn_o"]


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


def test_attn_decode_ex_refuses_bad_arguments_before_any_device_work():
    """the arguments of qtts_hip_attn_decode plus the skip flags (which may be NULL)"""
    lib = qtts.lib()
    one = C.c_void_p(16)
    ok = [one] * 9
    for skip in (None, one):
        for i in range(9):   # every pointer
            ptrs = ok[:i] + [None] + ok[i + 1:]
            assert lib.qtts_hip_attn_decode_ex(*ptrs, 4, 2, 32, 64, 1, 1e-6, 0, skip, None) == -1, i
        assert lib.qtts_hip_attn_decode_ex(*ok, 4, 2, 32, 64, 1, 1e-6, 2, skip, None) == -1    # element type
        assert lib.qtts_hip_attn_decode_ex(*ok, 0, 2, 32, 64, 1, 1e-6, 0, skip, None) == -1    # heads
        assert lib.qtts_hip_attn_decode_ex(*ok, 4, 0, 32, 64, 1, 1e-6, 0, skip, None) == -1    # kv heads
        assert lib.qtts_hip_attn_decode_ex(*ok, 4, 2, 0, 64, 1, 1e-6, 0, skip, None) == -1     # head size
        assert lib.qtts_hip_attn_decode_ex(*ok, 4, 2, 32, 0, 1, 1e-6, 1, skip, None) == -1     # capacity
        assert lib.qtts_hip_attn_decode_ex(*ok, 4, 2, 32, 64, 0, 1e-6, 1, skip, None) == -1    # rows
        assert lib.qtts_hip_attn_decode_ex(*ok, 4, 2, 32, 64, 65536, 1e-6, 1, skip, None) == -1


def _cached(lib, out=16, q=16, ld_q=256, kc=16, vc=16, qn=16, kn=16, cos=16, sin=16, row_b=16, pos=16, NH=4, KV=2,
            HD=32, S=64, slots=2, rows=3, win=0, kv_dtype=0, prep=1):
    p = lambda v: C.c_void_p(v) if v else None
    return lib.qtts_hip_attn_cached(p(out), p(q), ld_q, p(kc), p(vc), p(qn), p(kn), p(cos), p(sin), p(row_b), p(pos),
                                    NH, KV, HD, S, slots, rows, 1e-6, win, kv_dtype, prep, None)


def test_attn_cached_refuses_bad_arguments_before_any_device_work():
    lib = qtts.lib()
    for name in ("out", "q", "kc", "vc", "row_b", "pos"):
        for prep in (0, 1):
            assert _cached(lib, prep=prep, **{name: 0}) == -1, name
    for name in ("qn", "kn", "cos", "sin"):   # read by the prep kernel only
        assert _cached(lib, prep=1, **{name: 0}) == -1, name
    for bad in (dict(NH=0), dict(KV=0), dict(HD=0), dict(S=0), dict(slots=0), dict(rows=0), dict(rows=65536),
                dict(win=-1), dict(kv_dtype=2), dict(kv_dtype=-1), dict(prep=2), dict(prep=-1),
                dict(NH=3),                      # NH % KV
                dict(HD=4, ld_q=2048), dict(HD=136, ld_q=2048), dict(HD=12, ld_q=2048),
                dict(HD=24, ld_q=2048), dict(HD=40, ld_q=2048), dict(HD=96, ld_q=2048),   # no power of two: k_attn's lane groups
                dict(ld_q=255),                  # a fused row is (NH + 2 KV) HD wide
                dict(prep=0, ld_q=127),          # a q row NH HD
                dict(kv_dtype=1, win=16, prep=0)):   # no bf16 window path
        assert _cached(lib, **bad) == -1, bad


def _attn_o(lib, ptrs=None, R=64, NH=4, KV=2, HD=16, S=16, rows=2):
    ptrs = [C.c_void_p(16)] * 10 if ptrs is None else ptrs
    return lib.qtts_hip_attn_o(*ptrs, R, NH, KV, HD, S, rows, 1e-6, None)


def test_attn_o_refuses_bad_arguments_and_reports_uncovered_shapes_before_any_device_work():
    lib = qtts.lib()
    one = C.c_void_p(16)
    for i in range(10):
        assert _attn_o(lib, [one] * i + [None] + [one] * (9 - i)) == -1, i
    for bad in (dict(R=0), dict(NH=0), dict(KV=0), dict(HD=0), dict(S=0), dict(rows=0), dict(rows=65536)):
        assert _attn_o(lib, **bad) == -1, bad
    # 1: not a shape k_attn_o covers (qtts_attn_o_covers) -- the caller takes the two-kernel path
    for other in (dict(NH=4, KV=4), dict(NH=8, KV=2), dict(S=17), dict(HD=8), dict(HD=24), dict(HD=256)):
        assert _attn_o(lib, **other) == 1, other
    assert _attn_o(lib, [one] * 9 + [C.c_void_p(8)]) == 1   # W_o rows are read as 16-byte loads
