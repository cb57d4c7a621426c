"""The prefill attention precision switch without a device: the setter and
getter refuse what they must, the launch counter answers, the CLI parses
--prefill-attn.  (QTTS_HIP_PREFILL_ATTN is read when a device model is created,
which needs a device: test_gpu_attn_tileh.py holds that one.)"""
import ctypes as C
import subprocess

import qtts


def test_setter_and_getter_refuse_without_a_device_model():
    L, ctx, null = qtts.lib(), qtts.Ctx(), C.POINTER(qtts.Ctx)()   # (a zeroed ctx: no device model behind it)
    for v in (qtts.PREFILL_ATTN_EXACT, qtts.PREFILL_ATTN_BF16, 2):
        assert L.qwen_tts_set_prefill_attention_precision(null, v) == -1
        assert L.qwen_tts_set_prefill_attention_precision(C.byref(ctx), v) == -1
        assert L.qtts_dev_set_prefill_attention_precision(None, v) == -1
    assert L.qwen_tts_prefill_attention_precision(null) == -1
    assert L.qwen_tts_prefill_attention_precision(C.byref(ctx)) == -1
    assert L.qtts_dev_prefill_attention_precision(None) == -1 and qtts.Kernels.attn_tileh_launches() >= 0


def test_cli_parses_the_flag():
    r = subprocess.run([qtts.CLI_PATH, "--prefill-attn", "fp16"], capture_output=True, text=True)
    assert r.returncode == 1 and "--prefill-attn takes exact or bf16" in r.stderr
    r = subprocess.run([qtts.CLI_PATH, "--prefill-attn", "bf16"], capture_output=True, text=True)   # no model: usage
    assert r.returncode != 0 and "--prefill-attn takes" not in r.stderr
    assert "--prefill-attn exact|bf16" in r.stderr + r.stdout
