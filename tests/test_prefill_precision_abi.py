"""The prefill precision switch without a device: the setter and getter refuse
what they must, the planner knows force 3 / 4 and the new plan ids, the CLI
parses --prefill.  (QTTS_HIP_PREFILL is read when a device model is created,
which needs a device: test_gpu_prefill_bf16.py holds that one.)"""
import ctypes as C
import subprocess

import pytest

import qtts
import rows_gemm_ref as G
from rows_gemm_cases import describe, fake_ptrs


def test_setter_and_getter_refuse_without_a_device_model():
    L, ctx, null = qtts.lib(), qtts.Ctx(), C.POINTER(qtts.Ctx)()   # (a zeroed ctx: no device model behind it)
    for v in (qtts.PREFILL_EXACT, qtts.PREFILL_BF16, 2):
        assert L.qwen_tts_set_prefill_precision(null, v) == -1
        assert L.qwen_tts_set_prefill_precision(C.byref(ctx), v) == -1
        assert L.qtts_dev_set_prefill_precision(None, v) == -1
    assert L.qwen_tts_prefill_precision(null) == -1 and L.qwen_tts_prefill_precision(C.byref(ctx)) == -1
    assert L.qtts_dev_prefill_precision(None) == -1 and qtts.Kernels.pgemmh_launches() >= 0
    assert len(qtts.RG_NAMES) == 7 and qtts.RG_NAMES_BF16 == ["k_pgemmh<2>", "k_pgemmh<4>"]


@pytest.mark.parametrize("M,R,C_,force,want", [
    (17, 32, 256, 3, ("k_pgemmh<2>", 1, [1, 1, 1], 256)),
    (257, 288, 512, 4, ("k_pgemmh<4>", 2, [2, 3, 2], 512)),
    (257, 96, 2048, 3, ("k_pgemmh<2>", 8, [1, 3, 8], 256)),
    (300, 6144, 2048, 4, ("k_pgemmh<4>", 4, [24, 3, 4], 512)),   # split only while tiles x kz < 256
    (129, 96, 1280, 3, ("k_pgemmh<2>", 2, [1, 2, 2], 256)),      # 20 stages: columns of 10, not of 5
    (129, 96, 128, 3, None), (129, 48, 256, 4, None), (16, 96, 256, 3, None),
])
def test_planner(M, R, C_, force, want):
    cs, Mp = G.Case(M, R, C_, force=force), (M + 127) // 128 * 128
    d = describe(cs, fake_ptrs(cs))
    p = qtts.Kernels.rows_gemm_plan(d, 8 * M * R, Mp * C_, force)
    assert (p and (p["kernel"], p["kz"], p["grid"], p["block"])) == want
    assert qtts.Kernels.rows_gemm_plan(d, 8 * M * R, Mp * C_ - 1, force) is None   # one element short of the plane


def test_cli_parses_the_flag():
    r = subprocess.run([qtts.CLI_PATH, "--prefill", "fp16"], capture_output=True, text=True)
    assert r.returncode == 1 and "--prefill takes exact or bf16" in r.stderr
    r = subprocess.run([qtts.CLI_PATH, "--prefill", "bf16"], capture_output=True, text=True)   # accepted; no model: usage
    assert r.returncode != 0 and "--prefill takes" not in r.stderr and "--prefill exact|bf16" in r.stderr + r.stdout
