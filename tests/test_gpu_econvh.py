"""k_econvh (the bf16 encoder precision's contraction) through
qtts_hip_econvh_case, on the descriptors, buffers (NaN margins, sentinels) and
float64 helpers of enc_kernel_cases.py / enc_kernel_ref.py.

Plane 0 of k_ewsplit is the weight rounded to bf16 nearest even and the kernel
rounds x' the same way: at most U = 2^-9 relative error each.  Bars, with b_acc
= C_DOT sum|w||x'| + C_ABS + sum|w| d_in (enc_kernel_ref.py's bound for
k_econv), taken through the epilogue as there:
  rounded    against float64 on the rounded operands: their b_acc, with
             sum|w_r| flip for the d_in term.  A prologue leaves the kernel's
             fp32 x' up to d = d_in + 2^-24 |x'| from the float64 one; across a
             rounding boundary the two round apart by flip = max |rne(x' +- d)
             - rne(x')| (zero without a prologue).
  unrounded  against plain float64: 2 U sum|w||x'| + b_acc ((1 + u)^2 - 1 <
             2 U for u = U / (1 + U), nearest even's worst case).
"""
import os
import subprocess
import sys
from dataclasses import replace

import numpy as np
import pytest

import enc_kernel_cases as CS
import enc_kernel_ref as E
import qtts
from conftest import golden, model_dir
from xgemm_ref import C_ABS, C_DOT, EPS_OP, planes

pytestmark = pytest.mark.gpu
U = 2.0 ** -9

CASES = {
    "a-one-tile": E.Conv("a", 64, 64, 1, lin=(64,), lout=(64,)),
    "b-tails": E.Conv("b", 65, 64, 1, lin=(65,), lout=(65,)),
    "c-k40": E.Conv("c", 48, 8, 5, padl=4, lin=(70,), lout=(70,)),
    "d-seanet": E.Conv("d", 32, 16, 8, stride=4, padl=4, lin=(203,), lout=(51,), act_in=1, bias=True),
    "e-tdnn": E.Conv("e", 33, 24, 3, dil=2, padl=2, pmode=E.PAD_REFLECT, lin=(130, 64), lout=(130, 64), bias=True,
                     act_out=E.ACT_RELU),                    # K 72, Kp 96: a 64-k stage and a 32-k one
    "f-downsample": CS.DOWNSAMPLE,
    "g-rows": CS.rows_case(288, 130, 65, "none"),            # kz 2 over nk 9: stages of 64 + 64 and 64 + 64 + 32
    "h-deep": E.Conv("h", 64, 2048, 1, lin=(64,), lout=(64,), kz=16),
    "i-ragged": E.Conv("i", 40, 24, 3, padl=2, lin=(70, 33), lout=(70, 33)),
    "j-epilogue": CS.rows_case(64, 48, 65, "gelu", bias=True, bias2=True, vec=True, res=True),
}


def _rne(v):
    return planes(np.asarray(v, np.float32))[0]


def _reference(cv, d, rounded):
    """(outs, bounds) as E.conv_reference gives them, for the bar `rounded` or not"""
    w = d["w"].astype(np.float64)
    wr = _rne(w) if rounded else w
    outs, bounds = [], []
    for b in range(cv.nb):
        L, lo = cv.lin[b], cv.lout[b]
        s = d["x"][b].astype(np.float64)
        d_in = np.zeros_like(s)
        if cv.act_in:                                        # (no case here has the Res2Net sum)
            d_in = d_in + np.where(s < 0, E.FUNC_ERR_MAX, 0.0)
            s = E.elu64(s)
        cols = E.windows(cv, s, L, lo)
        if rounded:
            dd = np.where(d_in > 0, d_in + E.F32_EPS * np.abs(s), 0.0)
            flip = np.maximum(np.abs(_rne(s + dd) - _rne(s)), np.abs(_rne(s - dd) - _rne(s)))
            cols = E.windows(cv, _rne(s), L, lo)
            b_acc = C_DOT * (np.abs(wr) @ np.abs(cols)) + C_ABS + np.abs(wr) @ E.windows(cv, flip, L, lo)
        else:
            b_acc = (C_DOT + 2 * U) * (np.abs(w) @ np.abs(cols)) + C_ABS + np.abs(w) @ E.windows(cv, d_in, L, lo)
        u = wr @ cols
        if cv.bias:
            u = u + d["bias"].astype(np.float64)[:, None]
        if cv.bias2:
            u = u + d["bias2"][b].astype(np.float64)[:, None]
        v = E.act64(cv.act_out, u)
        lip = E.LIP[cv.act_out] * np.ones((cv.M, 1))
        if cv.vec:
            v = v * d["vec"].astype(np.float64)[:, None]
            lip = lip * np.abs(d["vec"].astype(np.float64))[:, None]
        if cv.res:
            v = v + d["res"][b, :, :lo].astype(np.float64)
        outs.append(v)
        bounds.append(lip * b_acc + EPS_OP * np.abs(v))
    return outs, bounds


def _run(gpu, cv, d, entry=None):
    """(plan, y buffer after the launch, layout) of one qtts_hip_econvh_case launch"""
    import torch
    lo = E.layout(cv, d)
    dev = {k: torch.from_numpy(np.ascontiguousarray(lo[k])).to(gpu)
           for k in ("w", "x", "x2", "y", "bias", "bias2", "vec") if k in lo}
    ran = (entry or qtts.Kernels.econvh_case)(CS.describe(cv, lo, {k: t.data_ptr() for k, t in dev.items()}))
    torch.cuda.synchronize()
    assert ran is not None, cv.id()
    return ran, dev["y"].cpu().numpy(), lo


@pytest.mark.parametrize("name", CASES)
def test_econvh(gpu, name):
    cv = CASES[name]
    d = E.make_inputs(cv)
    ran, y, lo = _run(gpu, cv, d)
    assert ran["rows"] == cv.rows and ran == qtts.Kernels.econv_plan(CS.host_desc(cv)[0])
    assert ran["kz"] > 1 or name not in ("g-rows", "h-deep")
    for rounded in (True, False):
        ratio = E.check(cv, lo, y, (d,) + _reference(cv, d, rounded))   # (and nothing else written)
        print(f"err / bound  {name:14s} {'rounded' if rounded else 'unrounded':9s} {ratio:.4f}")


def test_exact_grid(gpu):
    """bf16-representable integers, sums below 2^24: equal to float64 and to k_econv, bit for bit"""
    cv = E.Conv("grid", 65, 24, 3, padl=2, lin=(70,), lout=(70,))
    rng = np.random.default_rng(5)
    d = {"w": rng.integers(-4, 5, (cv.M, cv.K)).astype(np.float32),
         "x": rng.integers(-8, 9, (1, cv.ci, 70)).astype(np.float32)}
    ref = d["w"].astype(np.float64) @ E.windows(cv, d["x"][0].astype(np.float64), 70, 70)
    assert np.abs(ref).max() < 2 ** 24 and np.array_equal(_rne(d["w"]), d["w"]) and np.array_equal(_rne(d["x"]), d["x"])
    _, y, lo = _run(gpu, cv, d)
    assert np.array_equal(y[lo["yidx"][0]].astype(np.float64), ref)
    _, y3, _ = _run(gpu, cv, d, qtts.Kernels.econv_case)
    assert y.tobytes() == y3.tobytes()


def test_a_row_equals_the_utterance_alone(gpu):
    cv = CASES["i-ragged"]
    d = E.make_inputs(cv)
    _, y, lo = _run(gpu, cv, d)
    _, y1, lo1 = _run(gpu, replace(cv, lin=cv.lin[1:], lout=cv.lout[1:]), {"w": d["w"], "x": d["x"][1:]})
    assert y[lo["yidx"][1]].tobytes() == y1[lo1["yidx"][0]].tobytes()


def test_model_switch(gpu, monkeypatch):
    monkeypatch.delenv("QTTS_HIP_ENC", raising=False)
    G = golden("enc_tiny.npz")
    wavs = [G["wav0"], G["wav1"]]
    m = qtts.QwenTTS(model_dir("tiny_vc"))

    def encode():
        c0 = qtts.Kernels.econvh_launches()
        xv = m.speaker_embed(wavs)
        codes, lats = m.encode_audio(wavs, latent=True)
        return qtts.Kernels.econvh_launches() - c0, [xv] + codes + lats

    try:
        n0, before = encode()
        assert n0 == 0 and m.encoder_precision() == qtts.ENC_EXACT
        m.set_encoder_precision("bf16")
        n1, half = encode()
        assert n1 > 0 and m.encoder_precision() == qtts.ENC_BF16 and all(np.isfinite(a).all() for a in half)
        m.set_encoder_precision("exact")
        n2, after = encode()
        assert n2 == 0 and [a.tobytes() for a in after] == [a.tobytes() for a in before]
    finally:
        m.close()
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import qtts; m = qtts.QwenTTS(sys.argv[2]); "
            "print('precision', m.encoder_precision()); m.close()")
    r = subprocess.run([sys.executable, "-c", code, os.path.dirname(qtts.__file__), model_dir("tiny_vc")],
                       env=dict(os.environ, QTTS_HIP_ENC="bf16"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "precision 1" in r.stdout, r.stderr[-2000:]
