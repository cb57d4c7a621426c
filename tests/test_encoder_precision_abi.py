"""The encoder precision switch without a device: setters, getters, the launch
counter, the CLI's --encoder, and qtts_hip_econvh_case's refusals before any
device call.  (QTTS_HIP_ENC needs a device model: test_gpu_econvh.py.)"""
import ctypes as C
import subprocess

import enc_kernel_cases as CS
import qtts


def test_setter_and_getter_refuse_without_a_device_model():
    L, ctx, null = qtts.lib(), qtts.Ctx(), C.POINTER(qtts.Ctx)()   # (a zeroed ctx: no device model behind it)
    for v in (qtts.ENC_EXACT, qtts.ENC_BF16, 2):
        assert L.qwen_tts_set_encoder_precision(null, v) == -1
        assert L.qwen_tts_set_encoder_precision(C.byref(ctx), v) == -1
        assert L.qtts_dev_set_encoder_precision(None, v) == -1
    assert L.qwen_tts_encoder_precision(null) == -1
    assert L.qwen_tts_encoder_precision(C.byref(ctx)) == -1
    assert L.qtts_dev_encoder_precision(None) == -1 and qtts.Kernels.econvh_launches() >= 0


def test_cli_parses_the_flag():
    r = subprocess.run([qtts.CLI_PATH, "--encoder", "fp16"], capture_output=True, text=True)
    assert r.returncode == 1 and "--encoder takes exact or bf16" in r.stderr
    r = subprocess.run([qtts.CLI_PATH, "--encoder", "bf16"], capture_output=True, text=True)   # no model: usage
    assert r.returncode != 0 and "--encoder takes" not in r.stderr
    assert "--encoder exact|bf16" in r.stderr + r.stdout


def _set(**kw):
    return lambda d: [setattr(d, k, v) for k, v in kw.items()]


def _item(name, i, v):
    return lambda d: getattr(d, name).__setitem__(i, v)


# what qtts_hip_econv_case refuses on the TDNN case (test_enc_kernel_abi.py): the plan's refusals, then its own
REFUSED = [_set(nb=0), _set(nb=17), _set(M=0), _set(ci=0), _set(kw=0), _set(nmax=0),
           _item("lout", 1, CS.TDNN.nmax + 1), _item("lout", 0, -1), _item("lin", 2, 2), _item("lin", 2, 1),
           _set(w=None), _set(x=None), _set(y=None), _set(stride=0), _set(dil=0), _set(padl=-1), _set(pmode=3),
           _set(part=1 << 20, part_elems=10)]


def test_econvh_case_refuses_what_econv_case_refuses(capfd):
    L = qtts.lib()
    for i, mutate in enumerate(REFUSED):
        cv = CS.STFT if i == len(REFUSED) - 1 else CS.TDNN  # (the workspace case needs a split: kz 8)
        for fn in (L.qtts_hip_econv_case, L.qtts_hip_econvh_case):
            desc, _ = CS.host_desc(cv)                       # dummy addresses: a call that went on would fault
            mutate(desc)
            assert fn(C.byref(desc), C.byref(qtts.EConvPlan()), None) == -1, (i, fn.__name__)
    assert L.qtts_hip_econvh_case(None, None, None) == -1
    capfd.readouterr()
