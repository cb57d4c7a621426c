"""k_xlinh (k_xlinh.hip: the codec linears on one bf16 plane per operand)
through qtts_hip_xgemm_case with force_path 8, against the float64 reference of
xgemm_ref.py computed from the fp32 inputs, and the codec linear precision
switch (qwen_tts_set_codec_linear_precision) on the tiny golden model.

Bound per output element: b_acc + b_round, pushed through the epilogue as
xgemm_ref.epilogue does.  b_acc is test_gpu_xgemm.py's (2e-6 sum |a||w| + 1e-6).
b_round = (2^-8 + 2^-18) sum |a||w|: each operand rounded to the nearest bf16
carries a relative error <= 2^-9, so a product <= 2 * 2^-9 + 2^-18
(test_gpu_convh.py's bound without the SnakeBeta term).  Derived, not tuned.

Every case runs a second time with A and W on the bf16 grid: nothing is rounded
then and b_acc alone must hold -- the run a dropped K step, a wrong tail or a
wrong swizzle cannot pass.
"""
from dataclasses import replace

import numpy as np
import pytest

import qtts
import xgemm_ref as X
from attn_ref import rne_bf16, widen
from conftest import golden
from test_gpu_xgemm import run_case
from xgemm_cases import describe, fake_ptrs, lin, shipped

XH = 8                            # QTTS_XP_XLINH
C_ROUND = 2.0 ** -8 + 2.0 ** -18
TR = X.XA_TRANS

# M 1 / 4 / 5 / 33 / 130: partial and multiple row tiles, both sides of k_xgemv's 4 rows.  N 80: a half
# column tile.  K 96: a 32-deep last stage; K 1024: two stages per phase.  With a workspace of 8 M N floats
# the phase kernel and k_xg_reduce run; without one (and on the last two, which fill >= 256 tiles) the tile kernel.
def _p(M, N):
    return 8 * M * N


XLINH = [
    lin(XH, 1, 64, 64, part=_p(1, 64)),
    lin(XH, 1, 80, 1024, e=X.XE_BIAS_T, a=TR, part=_p(1, 80)),
    lin(XH, 4, 80, 96, e=X.XE_BIAS_N, part=_p(4, 80)),
    lin(XH, 4, 64, 1024, e=X.XE_SILU_MUL, a=TR),
    lin(XH, 5, 64, 96, e=X.XE_BIAS_N_GELU, a=TR, part=_p(5, 64)),
    lin(XH, 5, 80, 1024, e=X.XE_SCALE_RESID_N),
    lin(XH, 33, 80, 64, e=X.XE_BIAS_GAMMA_RES_T, part=_p(33, 80)),
    lin(XH, 33, 64, 96, a=TR, part=_p(33, 64) - 1),                   # one float short: the tile kernel
    lin(XH, 130, 80, 96, e=X.XE_BIAS_T, part=_p(130, 80)),
    lin(XH, 130, 64, 1024, e=X.XE_BIAS_GAMMA_RES_T, a=TR, part=_p(130, 64)),
    lin(XH, 130, 80, 64, e=X.XE_SCALE_RESID_N, a=TR),
    lin(XH, 130, 80, 1024, e=X.XE_SILU_MUL, part=_p(130, 80)),
    lin(XH, 130, 5520, 96, e=X.XE_SILU_MUL, part=_p(130, 5520)),
    lin(XH, 1030, 1040, 64, e=X.XE_BIAS_N, a=TR),
]
REFUSED = [lin(XH, 64, 72, 64), lin(XH, 64, 64, 80), lin(XH, 64, 64, 64, lda=70)]


def _on_grid(a):
    return widen(rne_bf16(np.asarray(a, np.float32))).reshape(a.shape).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [False, True], ids=["rounded", "grid-exact"])
@pytest.mark.parametrize("sp", XLINH, ids=[sp.id() for sp in XLINH])
def test_xlinh(gpu, sp, grid):
    d = X.make_inputs(sp)
    if grid:
        d["A"], d["W"] = _on_grid(d["A"]), _on_grid(d["W"])
    acc, b_acc = X.accumulate(sp, d)
    if not grid:
        b_acc = b_acc + C_ROUND * (np.abs(d["A"].astype(np.float64)) @ np.abs(d["W"].astype(np.float64)).T)
    ref, bound = X.epilogue(sp, d, acc, b_acc)
    if sp.emode in X.T_MODES:
        ref, bound = ref.T, bound.T
    ran, C, C0 = run_case(gpu, sp, d)
    assert ran == (XH, 1), (ran, sp.id())
    R, Cn = ref.shape
    got = C[:R, :Cn].astype(np.float64)
    assert np.all(np.isfinite(got)), sp.id()
    err = np.abs(got - ref)
    print(f"err / bound  k_xlinh {'grid-exact' if grid else 'rounded':10s} {float(np.max(err / bound)):.4f}  {sp.id()}")
    assert np.all(err <= bound), (sp.id(), float(np.max(err / bound)), np.argwhere(~(err <= bound))[:4])
    mask = np.ones(C.shape, bool)
    mask[:R, :Cn] = False                          # beside the output: untouched, bit for bit
    assert np.array_equal(C.view(np.uint32)[mask], C0.view(np.uint32)[mask]), sp.id()


@pytest.mark.gpu
@pytest.mark.parametrize("sp", REFUSED, ids=[sp.id() for sp in REFUSED])
def test_xlinh_refuses_what_it_does_not_cover(gpu, sp):
    ran, C, C0 = run_case(gpu, sp)
    assert ran is None and np.array_equal(C.view(np.uint32), C0.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("amode", [X.XA_ROWS, TR], ids=["rows", "trans"])
@pytest.mark.parametrize("N,K", [(64, 1024), (5520, 96)], ids=["N64-K1024", "N5520-K96"])
def test_a_row_does_not_depend_on_the_rows_beside_it(gpu, N, K, amode):
    """one input row inside calls of 1, 4, 33 and 130 rows, at row 0, at the
    call's last row (a partial tile's last row; row 1 of the second row-wave of
    the third tile at 130) and in the second row-wave (row 32 + 5), with and
    without the workspace (phase kernel / tile kernel; at N 5520 the 130-row
    call is the tile kernel either way): byte-equal outputs"""
    rng = np.random.default_rng(N + K)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    row = rng.standard_normal(K).astype(np.float32)
    outs = []
    for M, at in ((1, 0), (4, 3), (33, 32), (130, 129), (130, 37), (4, 0)):
        for part in (8 * M * N, 0):
            A = rng.standard_normal((M, K)).astype(np.float32)
            A[at] = row
            ran, C, _ = run_case(gpu, lin(XH, M, N, K, a=amode, part=part), {"A": A, "W": W})
            assert ran == (XH, 1)
            outs.append(C[at, :N].copy())
    assert np.all(np.isfinite(outs[0])) and np.any(outs[0] != 0)
    for o in outs[1:]:
        assert np.array_equal(o.view(np.uint32), outs[0].view(np.uint32))


def test_planner_answers_xlinh_only_when_asked_and_whatever_m():
    """host only: no default descriptor of a 1.7B decode plans path 8; forced,
    the answer is (8, 1) at every row count"""
    for T in (1, 16, 128):
        for name, sp in shipped(T):
            plan = qtts.Kernels.xgemm_plan(describe(sp, fake_ptrs(sp)), sp.part, -1)
            assert plan is not None and plan[0] != XH, (name, plan)
            if sp.kind == "lin":
                for M in (1, 4, 5, 33, 130, 8192):
                    q = replace(sp, M=M)
                    assert qtts.Kernels.xgemm_plan(describe(q, fake_ptrs(q)), q.part, XH) == (XH, 1), (name, M)


# ---------------------------------------------------------------- the switch on the tiny golden model
CODES = np.random.default_rng(2612).integers(0, 2048, size=(3, 24, 16)).astype(np.int32)


@pytest.fixture(params=[False, True], ids=["linears", "linears+convs"])
def m(tts_tiny, request):
    """the shared model with the conv switch as the case says, handed back exact"""
    try:
        tts_tiny.set_codec_precision("bf16" if request.param else "exact")
        yield tts_tiny
    finally:
        tts_tiny.set_codec_precision("exact")
        tts_tiny.set_codec_linear_precision("exact")


@pytest.mark.gpu
def test_switch_round_trips_rejects_a_bad_value_and_leaves_exact_alone(m):
    conv = m.codec_precision()
    m.set_codec_precision("exact")
    before = m.codec_decode(CODES[0])
    m.set_codec_precision(conv)
    for v in ("bf16", "exact", qtts.CODEC_BF16):
        m.set_codec_linear_precision(v)
        assert m.codec_linear_precision() == {"bf16": 1, "exact": 0}.get(v, v) and m.codec_precision() == conv
    for bad in (2, -1, "fp16"):
        with pytest.raises(ValueError):
            m.set_codec_linear_precision(bad)
    assert qtts.lib().qtts_dev_set_codec_linear_precision(m.c.hip, 7) == -1
    assert m.codec_linear_precision() == qtts.CODEC_BF16
    rounded = m.codec_decode(CODES[0])
    assert np.all(np.isfinite(rounded)) and not np.array_equal(rounded, before)
    m.set_codec_linear_precision("exact")
    m.set_codec_precision("exact")
    np.testing.assert_array_equal(m.codec_decode(CODES[0]), before)


@pytest.mark.gpu
def test_streams_equal_the_stateless_decode(m):
    """the single stream pushed as 1 + 7 + 16 frames and a 3-stream ragged
    multi-stream against the stateless decode of the same 24 frames, and a mode
    set after begin waits for the next begin.  A row of k_xlinh does not depend
    on the rows beside it, so the expectation is 0.0; the bar is the exact-mode
    stream tests' 1e-5."""
    m.set_codec_linear_precision("bf16")
    full = [m.codec_decode(CODES[s]) for s in range(3)]
    single = np.concatenate(m.codec_stream([CODES[0, :1], CODES[0, 1:8], CODES[0, 8:]]))
    assert m.codec_mstream_begin(3, 64) == 0
    m.set_codec_linear_precision("exact")          # latched at begin: these pushes stay bf16
    cuts = [(0, 5, 11, 24), (0, 2, 17, 24), (0, 7, 8, 24)]
    out = [[], [], []]
    for k in range(3):
        o = m.codec_mstream_push_ragged([0, 1, 2], [CODES[s, cuts[s][k]:cuts[s][k + 1]] for s in range(3)])
        assert o is not None
        for s in range(3):
            out[s].append(o[s])
    d = [float(np.abs(single - full[0]).max())]
    d += [float(np.abs(np.concatenate(out[s]) - full[s]).max()) for s in range(3)]
    print("measured  bf16 linears, largest |stream - stateless|: single %.3e, ragged streams %.3e %.3e %.3e" % tuple(d))
    assert max(d) < 1e-5, d


@pytest.mark.gpu
def test_waveform_against_the_oracle(m):
    """recorded, not asserted, for the reason test_bf16_waveform_against_the_oracle
    gives (profiles/codec_lin_bf16_bench.txt holds the figures)"""
    g = golden("e2e_tiny.npz")
    m.set_codec_linear_precision("bf16")
    a = m.codec_decode(np.ascontiguousarray(g["greedy_codes"]))
    mse = float(np.mean((a.astype(np.float64) - g["greedy_audio"]) ** 2))
    print(f"measured  bf16 linears (convs {m.codec_precision()}) vs the oracle's golden waveform: mse {mse:.3e}")
    assert a.shape == g["greedy_audio"].shape and np.all(np.isfinite(a))
